"""Content soak of the DEFAULT Farneback mode (fast level kernels + exact re-run of the pairs they flag) against the oracle
(reference site: cv2.calcOpticalFlowFarneback + np.mean / np.var of |flow|, app/analyzers/video.py:45-48, and ai_susp,
video.py:54-56).

Seeded pairs of 320 x 320 frames from every content family of tests/content_families.py (28 families x 12 pairs by default):
natural-looking (smooth / 1/f fields with translation, zoom, rotation, fades, scene cuts, letter- and pillar-boxing,
saturation, blocks, text), static scenes (fresh noise per frame; bit-identical frames but for a small patch), degenerate (flat,
constant, steps, gradients) and adversarial (ramps, stripes, checkerboards of any cell size, with and without overlays).
Asserted for EVERY pair, no family excepted: flow_mean / flow_var within rel 1e-6 (abs 1e-7) of the oracle and |delta ai_susp| <= 1e-6
for the texture value that makes ai_susp most sensitive to the flow (tex -> infinity: ai_susp = 1 - (1 + mot), so |delta ai_susp| =
|delta flow_mean|); fb_mode = exact bit-identical.  The CPU experiment behind the two flag criteria
(tools/experiments/fb_illposed_run.py, 3 120 pairs) is the same generator, so this soak is in-sample; its out-of-sample counterpart is
tests/test_gpu_holdout.py (sixteen hold-out families of tests/holdout_families.py, 1 023 pairs each, refereed by fb_mode = exact on the GPU).

Round 4 kept a carve-out here for exactly periodic checkerboards, keyed on the family's name.  Round 5 found the mechanism (cv2's
warp takes "inside" or "outside" at the top / left border by the SIGN of a flow component that is pure rounding residue of its
running sums) and the level kernels flag it (avd_fbfast.hip, role_ne): the carve-out is gone.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.content_families import families  # noqa: E402

PER_FAMILY = int(os.environ.get("AVD_SOAK_PER_FAMILY", "12"))   # larger one-off runs: profiles/r05_soak_*.txt
SEED0 = int(os.environ.get("AVD_SOAK_SEED0", "9000"))


def test_default_mode_on_every_content_family(oracle):
    import avd_hip
    fam = families()
    jobs = [(name, SEED0 + 7919 * i + 17 * j) for j, name in enumerate(fam) for i in range(PER_FAMILY)]
    frames = np.empty((2 * len(jobs), 320, 320), np.uint8)
    for k, (name, seed) in enumerate(jobs):
        frames[2 * k], frames[2 * k + 1] = fam[name](np.random.default_rng(seed))
    with avd_hip.Context(0) as c, avd_hip.Context(0) as cx:
        assert c.get_option("fb_mode") == 1 and c.get_option("fb_rerun") == 1        # the library default
        cx.set_option("fb_mode", 0)
        fm, fv = c.farneback_pairs(frames)                     # pairs (2k, 2k + 1) are the soak; the ones in between are ignored
        rerun_total = c.get_option("rerun_pairs")
        rec = c.analyze_frames(np.repeat(frames[..., None], 3, axis=3))   # the same pairs through the records: which were re-run, and why
        xm, xv = cx.farneback_pairs(frames)
    worst, reruns = 0.0, {}
    for k, (name, seed) in enumerate(jobs):
        if k % 100 == 99:
            print(f"[soak] {k + 1} of {len(jobs)} pairs checked against the oracle", flush=True)
        a, b = frames[2 * k], frames[2 * k + 1]
        m, v = oracle.flow_stats(oracle.farneback(a, b))
        assert xm[2 * k] == m and xv[2 * k] == v, ("exact", name, seed)           # exact mode: bit-identical on every family
        dm = abs(float(fm[2 * k]) - float(m))
        worst = max(worst, dm)
        assert fm[2 * k] == pytest.approx(m, rel=1e-6, abs=1e-7), (name, seed, float(fm[2 * k]), float(m))
        assert fv[2 * k] == pytest.approx(v, rel=1e-6, abs=1e-7), (name, seed, float(fv[2 * k]), float(v))
        assert dm <= 1e-6 * max(1.0, abs(m)), (name, seed, dm)               # |delta ai_susp| bound at tex -> infinity
        assert rec["flow_mean"][2 * k + 1] == fm[2 * k] and rec["flow_var"][2 * k + 1] == fv[2 * k], (name, seed)   # both entry points agree
        if rec["reserved"][2 * k + 1]:
            r = reruns.setdefault(name, [0, 0, 0])
            r[0] += 1
            r[1] += bool(rec["reserved"][2 * k + 1] & 0x0F)      # the solver's criterion (singular equations / runaway flow)
            r[2] += bool(rec["reserved"][2 * k + 1] & 0xF0)      # the border-sign criterion
    print(f"[soak] {len(jobs)} pairs, {len(fam)} families: max |delta flow_mean| = {worst:.3g}; pairs re-run in the call (incl. the in-between "
          f"pairs): {rerun_total}; re-run soak pairs per family [total, solver criterion, border-sign criterion] of {PER_FAMILY}: {reruns}")
