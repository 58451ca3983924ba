"""The throughput shape of the fast Farneback level kernel (csrc/avd_fbfast.hip: 320 px, and 160 px as one strip per pair) at small pair
counts, and the 320-px level's last launch, which stores the flow itself only for a call that hands it to its caller (everything else
reads |flow|; avd_debug_fetch "flow0" has the launch repeated with the stores).

The level sizes are fixed by the library; the small dimension is the pair count.  1 pair is the smallest case, 9 pairs the first count at
which a launch has more than one pair per XCD group (ppx = (npairs + 7) >> 3 = 2) and workgroups with p >= npairs that leave at once.

Reference: fb_mode = 0 (the exact kernels, bit-identical to the oracle: tests/test_gpu_fbfast.py), computed once per module.  On well-posed
content the fast kernels' flow equals it bit for bit at every level (the horizontal window sums differ by double ulps that the float cast of
the flow swallows), so the comparisons are array_equal.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from avd_hip import synth  # noqa: E402
from tests.content_families import families as _families  # noqa: E402

PAIRS = (1, 2, 3, 9)             # clips of 2, 3, 4 and 10 frames


def _levels(c, n):
    return [c.debug_fetch(f"flow{k}", (n - 1, 2, 320 >> k, 320 >> k), np.float32) for k in range(4)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _gray(oracle, clip):
    return np.stack([oracle.resize_linear(oracle.bgr2gray(f), 320, 320) for f in clip])


@pytest.fixture(scope="module")
def smooth(oracle):
    """ten frames of a smooth translating field, no duplicate, no scene cut: well-posed pairs"""
    return _gray(oracle, synth.make_clip(10, 320, 320, seed=41, dup_every=0, scene_cut=False))


@pytest.fixture(scope="module")
def exact_ctx():
    import avd_hip
    c = avd_hip.Context(0)
    c.set_option("fb_mode", 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def exact_smooth(exact_ctx, smooth):
    """exact mode on the ten frames, once: (flow_mean, flow_var, dense flow, the four level flows).  Pairs are independent of each other,
    so the first n - 1 entries are the reference of the clip's first n frames."""
    fm, fv, flow = exact_ctx.farneback_pairs(smooth, want_flow=True)
    return fm, fv, flow, _levels(exact_ctx, len(smooth))


@pytest.mark.parametrize("npairs", PAIRS)
def test_level_flows_equal_exact_mode(smooth, exact_smooth, npairs):
    """Every level's flow of the default mode against exact mode, with both 160-px shapes (fb_wide160 0 / 1) and with the first launch's
    resize folded in or not (fb_fold_up / fb_fold_up160: the UP and the plain form of both instantiations)."""
    import avd_hip
    n = npairs + 1
    xm, xv, xflow, xlv = exact_smooth
    with avd_hip.Context(0) as c:
        c.set_option("fb_mode", 1)
        for wide in (0, 1):
            for fold, fold160 in ((5, 1), (0, 0)):
                c.set_option("fb_wide160", wide)
                c.set_option("fb_fold_up", fold)
                c.set_option("fb_fold_up160", fold160)
                tag = (npairs, wide, fold, fold160)
                fm, fv, flow = c.farneback_pairs(smooth[:n], want_flow=True)
                assert c.get_option("rerun_pairs") == 0, tag
                assert c.get_option("fb_wide160_used") == wide, tag
                lv = _levels(c, n)
                for k in range(4):
                    nd = int(np.count_nonzero(_bits(lv[k]) != _bits(xlv[k][:npairs])))
                    print(f"[fbfast balance] pairs {npairs} wide160 {wide} fold {fold}/{fold160} level {k}: {nd} of {lv[k].size} values differ")
                    assert np.array_equal(lv[k], xlv[k][:npairs]), (tag, k, nd)
                assert np.array_equal(flow, xflow[:npairs]), tag
                assert np.array_equal(fm, xm[:npairs]) and np.array_equal(fv, xv[:npairs]), tag


def test_identical_frames_and_a_flagged_pair(oracle, exact_ctx, smooth):
    """A run of identical frames (those pairs are exempt from the border-sign criterion: their zero flow is structural) next to a pair the
    kernels flag (a ramp against itself rolled: its workgroups leave at the flag word from the level that raised it on), in both 160-px
    shapes.  Records equal exact mode's: the flagged pair IS the exact kernels' result, the rest is well-posed (an identical pair's flow is
    zero except along the last row and column, where cv2's warp counts as outside)."""
    import avd_hip
    ramp, rolled = _families()["ramp_roll"](np.random.default_rng(3))
    frames = np.stack([smooth[0], smooth[1], smooth[1], smooth[1], smooth[1], smooth[2], ramp, rolled, smooth[4], smooth[5]])
    same, hard = (1, 2, 3), 6
    clip = np.repeat(frames[..., None], 3, axis=3)
    want = exact_ctx.analyze_frames(clip).copy()
    exact_ctx.farneback_pairs(frames)
    xlv = _levels(exact_ctx, len(frames))
    with avd_hip.Context(0) as c:
        for wide in (0, 1):
            c.set_option("fb_wide160", wide)
            rec = c.analyze_frames(clip)
            assert rec["reserved"][hard + 1] != 0 and not any(rec["reserved"][p + 1] for p in same), (wide, rec["reserved"].tolist())
            unflagged = [p for p in range(len(frames) - 1) if not rec["reserved"][p + 1]]
            for key in ("flow_mean", "flow_var"):
                assert np.array_equal(rec[key][1:][unflagged], want[key][1:][unflagged]), (wide, key)
                assert rec[key][hard + 1] == want[key][hard + 1], (wide, key)
            lv = _levels(c, len(frames))
            for k in range(4):
                for p in same:
                    # a flow of the size of the sums' rounding residue (1e-10 px here): its bits follow the summation order, which the two modes
                    # do not share -- the default mode's stated tolerance (tests/test_gpu_fbfast.py, FLOW_TOL), not bit-identity
                    assert np.abs(lv[k][p] - xlv[k][p]).max() <= 1e-5, (wide, k, p)
            assert np.array_equal(lv[0][hard], xlv[0][hard]), wide           # the re-run wrote the exact flow where the caller reads it


@pytest.mark.parametrize("npairs", PAIRS)
def test_flow_nobody_reads(smooth, exact_smooth, npairs):
    """The same clip with the dense flow requested and without: the statistics are equal, the dense flow is exact mode's, and after the
    call without it the next calls of the context give what a fresh context gives (nothing later depends on a buffer that call left
    unwritten)."""
    import avd_hip
    n = npairs + 1
    xm, xv, xflow, (xlv0, *_) = exact_smooth
    clip = np.repeat(smooth[:n][..., None], 3, axis=3)
    with avd_hip.Context(0) as fresh:
        want_rec = fresh.analyze_frames(clip).copy()
    with avd_hip.Context(0) as c:
        fm0, fv0 = c.farneback_pairs(smooth[:n])                              # first, so that no earlier call has left this flow in the buffer
        late = _levels(c, n)[0]                                               # the debug reader, after a call that stored no flow
        assert np.array_equal(late, xlv0[:npairs]) and np.array_equal(_levels(c, n)[0], late)
        fm1, fv1, flow = c.farneback_pairs(smooth[:n], want_flow=True)
        assert np.array_equal(fm0, fm1) and np.array_equal(fv0, fv1)
        assert np.array_equal(flow, xflow[:npairs])
        rec = c.analyze_frames(clip)                                          # records path: no dense flow either
        assert rec.tobytes() == want_rec.tobytes()
        assert np.array_equal(rec["flow_mean"][1:], fm0) and np.array_equal(rec["flow_var"][1:], fv0)
        fm2, fv2, flow2 = c.farneback_pairs(smooth[:n], want_flow=True)       # and the flow again, after two calls that did not want it
        assert np.array_equal(flow2, flow) and np.array_equal(fm2, fm0) and np.array_equal(fv2, fv0)
        assert c.analyze_frames(clip).tobytes() == want_rec.tobytes()


def test_one_flagged_pair_is_rerun(exact_ctx, smooth):
    """One pair of the hard set (tests/test_gpu_fbfast.py: a ramp against itself rolled by 25 px) alone and among well-posed pairs: flagged,
    re-run, and the records are exact mode's."""
    import avd_hip
    ramp = (np.add.outer(np.arange(320), np.arange(320)) % 256).astype(np.uint8)
    rolled = np.roll(ramp, 25, axis=1)
    alone = np.stack([ramp, rolled])
    among = np.stack([smooth[0], smooth[1], smooth[2], ramp, rolled])
    with avd_hip.Context(0) as c:
        for frames, hard in ((alone, 0), (among, 3)):
            clip = np.repeat(frames[..., None], 3, axis=3)
            want = exact_ctx.analyze_frames(clip).copy()
            rec = c.analyze_frames(clip)
            assert rec["reserved"][hard + 1] != 0 and c.get_option("rerun_pairs") >= 1, rec["reserved"].tolist()
            keep = [i for i in range(len(frames)) if i == hard + 1 or not rec["reserved"][i]]
            # the flagged pair and the well-posed ones (frames 0 .. 2); the pair that ends one scene and begins the other is arbitrary
            # content, compared where it was flagged or not at all
            keep = [i for i in keep if i != hard or hard == 0]
            for key in ("lap_sum", "lap_sumsq", "ham", "flow_mean", "flow_var"):
                assert np.array_equal(rec[key][keep], want[key][keep]), (hard, key, rec[key].tolist(), want[key].tolist())
