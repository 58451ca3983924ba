"""Hold-out soak of the DEFAULT Farneback mode (fast level kernels + exact re-run of the pairs they flag; reference site:
cv2.calcOpticalFlowFarneback + np.mean / np.var of |flow|, app/analyzers/video.py:45-48, and ai_susp, video.py:54-56): the out-of-sample
counterpart of tests/test_gpu_soak.py, on the sixteen families of tests/holdout_families.py -- content that did not exist when the thresholds of the
two flag criteria were derived, part of it aimed at the right / bottom edge of cv2's inside / outside test, which the fast kernels do not guard.

The referee is fb_mode = exact ON THE GPU (bit-identical to the oracle on every pair ever tested, and confirmed against the CPU oracle here on the two
pinned pairs of each family), so each test checks 1 023 pairs, not a dozen: 512 pairs of the family, composed on the device, and the 511 pairs in between
(scene cuts between unrelated content, reported as `cut_between`).  Asserted on every one of them, with the project's stated tolerances
(tests/test_gpu_soak.py) and no name excepted:
  a flagged pair equals exact mode bit for bit; an unflagged pair is within rel 1e-6 / abs 1e-7 on flow_mean and flow_var and |delta flow_mean| <=
  1e-6 * max(1, |m|); the records of avd_analyze_frames carry the same statistics; the flag words count up to rerun_pairs; everything is finite;
  the dense flow of the first 16 pairs (and the 15 between them) is bit-identical where flagged and within 1e-5 px elsewhere.
So that the fast kernels are what is tested: at least three quarters of the pairs stay unflagged in the families of holdout_families.MOSTLY_UNFLAGGED,
and no family but near_duplicate holds a bit-identical pair.  On one MI355X a family's test takes 0.15 - 0.75 s, the file 6 s.

The one-off run of the same check over 2 013 264 pairs (tools/fuzz_fast_vs_exact.py, profiles/holdout_fuzz.txt) found two violators; their frames are fixtures
(tests/golden/holdout_fuzz_*.npz) and the last two tests here: the first is closed (kTinyFlow), the second is open and stated as a strict expected failure.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import holdout_families as H  # noqa: E402

PAIRS = 512
DENSE_PAIRS = 16
NAMES = tuple(H.PINNED_SHA256)


@pytest.fixture(scope="module")
def exact():
    import avd_hip
    c = avd_hip.Context(0)
    c.set_option("fb_mode", 0)
    yield c
    c.close()


def _line(tag, s):
    return (f"[holdout] {tag}: {s['pairs']} pairs; flagged {s['flagged']} (solver criterion {s['solver']}, border-sign criterion {s['border']}); "
            f"{s['differ']} differ bitwise from exact; max |delta flow_mean| = {s['max_dmean']:.3g}")


@pytest.mark.parametrize("name", NAMES)
def test_default_mode_on_holdout_family(ctx, exact, oracle, tmp_path, name):
    j = NAMES.index(name)
    seeds = H.seeds_for_tests(j, PAIRS)
    make = H.holdout_families()[name]
    dev = torch.device("cuda", 0)
    pairs = make(H.bank(), seeds, dev)
    assert pairs.shape == (PAIRS, 2, 320, 320) and pairs.dtype == torch.uint8 and pairs.is_cuda
    G = pairs.reshape(2 * PAIRS, 320, 320)

    def who(p):                                   # pair p of the 1 023 -> family, seed(s), index
        return (name, seeds[p // 2], p) if p % 2 == 0 else (H.CUT_BETWEEN, name, seeds[p // 2], seeds[p // 2 + 1], p)

    def dump(p):
        path = tmp_path / f"{name}_pair{p}.npz"
        np.savez_compressed(path, prev=G[p].cpu().numpy(), next=G[p + 1].cpu().numpy())
        return str(path)

    # the device composed the bytes the CPU does: the two pinned pairs, and a CPU rebuild of them
    assert (H.pair_sha256(pairs[0]), H.pair_sha256(pairs[1])) == H.PINNED_SHA256[name]
    host = make(H.bank(), seeds[:2], "cpu")
    assert (H.pair_sha256(host[0]), H.pair_sha256(host[1])) == H.PINNED_SHA256[name]
    identical = (pairs[:, 0] == pairs[:, 1]).flatten(1).all(1)
    assert not bool(identical.any()), (name, [seeds[int(k)] for k in identical.nonzero()[:, 0]])      # near_duplicate: one pixel differs
    if name == "near_duplicate":
        assert bool(((pairs[:, 0] != pairs[:, 1]).flatten(1).sum(1) == 1).all())

    r = H.run_default_and_exact(ctx, exact, G)
    flagged = r["reserved"] != 0
    fam_sel, cut_sel = slice(0, None, 2), slice(1, None, 2)
    print()
    print(_line(name, H.summarise(r, fam_sel)))
    print(_line(f"{H.CUT_BETWEEN} ({name})", H.summarise(r, cut_sel)))

    for k in ("fm", "fv", "xm", "xv", "rec_mean", "rec_var"):
        assert r[k].shape == (2 * PAIRS - 1,) and np.isfinite(r[k]).all(), (name, k)
    bad = H.check(r["fm"], r["fv"], r["xm"], r["xv"], flagged)
    assert not bad, [(who(b[0]), b[1:], dump(b[0])) for b in bad[:4]]
    differ = np.nonzero((r["rec_mean"] != r["fm"]) | (r["rec_var"] != r["fv"]))[0]                    # both entry points agree
    assert differ.size == 0, [who(int(p)) for p in differ[:4]]
    assert int(flagged.sum()) == r["rerun_records_call"] == r["rerun_pairs_call"], name
    if name in H.MOSTLY_UNFLAGGED:
        assert int(flagged[fam_sel].sum()) * 4 <= PAIRS, (name, int(flagged[fam_sel].sum()))

    # dense flow: the first 16 pairs of the family and the 15 between them, in a call of their own (with its own flag words)
    D = G[:2 * DENSE_PAIRS]
    _, _, flow = ctx.farneback_pairs(D, want_flow=True)
    rec = ctx.analyze_frames(D[..., None].expand(-1, -1, -1, 3).contiguous())
    _, _, xflow = exact.farneback_pairs(D, want_flow=True)
    assert np.isfinite(flow).all() and np.isfinite(xflow).all()
    for p in range(2 * DENSE_PAIRS - 1):
        assert bool(rec["reserved"][p + 1]) == bool(flagged[p]), who(p)                              # a pair's flag does not depend on the call
        if flagged[p]:
            assert np.array_equal(flow[p].view(np.uint32), xflow[p].view(np.uint32)), (who(p), dump(p))
        else:
            d = float(np.abs(flow[p] - xflow[p]).max())
            assert d <= H.FLOW_TOL, (who(p), d, dump(p))

    # the referee itself: exact mode equals the CPU oracle, bit for bit, on the two pinned pairs rebuilt on the CPU
    for k in range(2):
        a, b = host[k].numpy()
        m, v = oracle.flow_stats(oracle.farneback(a, b))
        assert r["xm"][2 * k] == m and r["xv"][2 * k] == v, ("exact mode against the oracle", name, seeds[k])
        assert np.array_equal(xflow[2 * k], oracle.farneback(a, b)), ("exact mode's dense flow against the oracle", name, seeds[k])


# ---- what the one-off fuzz found (tools/fuzz_fast_vs_exact.py, profiles/holdout_fuzz.txt): 2 violators in 2 013 264 pairs, both unflagged, exact mode equal to the oracle --------
_BANDING = ("the solver criterion does not see this pair (determinant cancellation 940 at 40 px, kCondMax 2000; well-posed in-sample content reaches 975, so the threshold "
            "cannot simply move): no branch of cv2's warp flips, a 1.9e-9 px difference of the 40-px level's second iteration doubles through the next ten to 1.1e-4 px of dense "
            "flow; the oracle itself moves 3.0e-4 px under +-1 ulp on its pyramid.  Observed on the MI355X: flow_mean 0.563321054 against 0.563321590 (rel 9.5e-7, inside), "
            "flow_var 0.817975163 against 0.817975998 (rel 1.02e-6, OUTSIDE rel 1e-6).  The kernels are left as they are for this one")
FINDINGS = (
    # border-sign criterion: a residue-sized dy of +1.3e-12 .. +5.5e-12 px (cv2) / -1.8e-12 .. -3.1e-12 px (fast) at row 0 next to a 160-grey-level edge, above the old kTinyFlow
    # of 1e-12: unflagged, flow_var off by rel 5.8e-6.  kTinyFlow is 1e-10 since: the pair is flagged and bit-identical
    pytest.param("rot_checker", 2200023830, 0xF0, id="rot_checker-2200023830"),
    pytest.param("banding", 1700059141, None, id="banding-1700059141", marks=pytest.mark.xfail(strict=True, reason=_BANDING)),
)


def _finding(name, seed):
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"holdout_fuzz_{name}_{seed}.npz"))
    return np.stack([z["prev"], z["next"]])


@pytest.mark.parametrize("name,seed", [p.values[:2] for p in FINDINGS])
def test_fuzz_finding_is_reproducible_and_the_referee_right(exact, oracle, name, seed):
    """the committed frames ARE (family, seed), composed on the device; exact mode equals the CPU oracle on them, statistics and dense flow"""
    pair = _finding(name, seed)
    rebuilt = H.holdout_families()[name](H.bank(), [seed], torch.device("cuda", 0))[0]
    assert np.array_equal(rebuilt.cpu().numpy(), pair)
    xm, xv, xflow = exact.farneback_pairs(pair, want_flow=True)
    want = oracle.farneback(pair[0], pair[1])
    assert np.array_equal(xflow[0], want) and (xm[0], xv[0]) == oracle.flow_stats(want)


@pytest.mark.parametrize("name,seed,flag_bits", FINDINGS)
def test_fuzz_finding_is_inside_the_guarantee(ctx, exact, name, seed, flag_bits):
    pair = _finding(name, seed)
    r = H.run_default_and_exact(ctx, exact, pair)
    print(f"\n[holdout] finding {name} {seed}: flag word {int(r['reserved'][0]):#x}; default ({r['fm'][0]:.9g}, {r['fv'][0]:.9g}), exact ({r['xm'][0]:.9g}, {r['xv'][0]:.9g})")
    if flag_bits is not None:
        assert r["reserved"][0] & flag_bits, hex(int(r["reserved"][0]))
    bad = H.check(r["fm"], r["fv"], r["xm"], r["xv"], r["reserved"] != 0)
    assert not bad, bad
    _, _, flow = ctx.farneback_pairs(pair, want_flow=True)
    _, _, xflow = exact.farneback_pairs(pair, want_flow=True)
    if r["reserved"][0]:
        assert np.array_equal(flow.view(np.uint32), xflow.view(np.uint32))
    else:
        assert float(np.abs(flow - xflow).max()) <= H.FLOW_TOL
