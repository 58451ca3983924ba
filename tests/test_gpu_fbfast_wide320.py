"""The second shape of the 320-px level of the fast Farneback kernel (csrc/avd_fbfast.hip, option "fb_wide320"): the launches that read a
320-px flow run a pair as ONE workgroup of five 64-column blocks (15 waves, lane column = image column, the replicated border columns only
in the vsum ring) instead of two strips of three blocks.  Every column is computed by the same instructions on the same operands in both
shapes, so everything the level leaves -- its flow, |flow| and with it flow_mean / flow_var, the flag words -- is compared with
array_equal, on ill-posed content too.

The level size is fixed by the library; the small dimension is the pair count.  1 pair is the smallest case, 9 pairs the first count at
which a launch has more than one pair per XCD group (ppx = (npairs + 7) >> 3 = 2) and workgroups with p >= npairs that leave at once.

Which launches take the new shape (debug buffer "fb_wide320_launches", per call): those whose input flow is a 320-px buffer.  With the
first launch's resize folded in (fb_fold_up bit 1, the default) that is the second and the third: 2 per chunk; with fb_fold_up = 0 the
first launch reads what k_flow_up wrote and takes the new shape too: 3 per chunk.

Reference of the well-posed clip: fb_mode = 0 (the exact kernels), computed once per module, as tests/test_gpu_fbfast_balance.py does.
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


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _launches(c):
    return int(c.debug_fetch("fb_wide320_launches", (1,), np.int32)[0])


def _bgr(frames):
    return np.repeat(frames[..., None], 3, axis=3)


@pytest.fixture(scope="module")
def smooth(oracle):
    """ten frames of a smooth translating field, no duplicate, no scene cut: well-posed pairs"""
    clip = synth.make_clip(10, 320, 320, seed=41, dup_every=0, scene_cut=False)
    return np.stack([oracle.resize_linear(oracle.bgr2gray(f), 320, 320) for f in clip])


@pytest.fixture(scope="module")
def exact_smooth(smooth):
    """exact mode on the ten frames, once: (flow_mean, flow_var, dense flow, the four level flows); pairs are independent of each other"""
    import avd_hip
    with avd_hip.Context(0) as c:
        c.set_option("fb_mode", 0)
        fm, fv, flow = c.farneback_pairs(smooth, want_flow=True)
        return fm, fv, flow, _levels(c, len(smooth))


def _border_bands():
    """a flat field whose only texture lies in columns 0-14 and 305-319: noise bands, moved down by one pixel between the frames"""
    rng = np.random.default_rng(17)
    a = np.full((320, 320), 128, np.uint8)
    a[:, :15] = rng.integers(0, 256, (320, 15), dtype=np.uint8)
    a[:, 305:] = rng.integers(0, 256, (320, 15), dtype=np.uint8)
    return np.stack([a, np.roll(a, 1, axis=0), np.roll(a, 2, axis=0)])


def _noise_pan(step):
    """white noise panned horizontally by `step` px per frame (a window of a wider field: new columns enter at the border)"""
    field = np.random.default_rng(23).integers(0, 256, (320, 320 + 16), dtype=np.uint8)
    x0 = 8
    return np.stack([field[:, x0 - step * i: x0 - step * i + 320] for i in range(3)])


@pytest.mark.parametrize("npairs", PAIRS)
def test_both_shapes_equal_and_equal_exact_mode(smooth, exact_smooth, npairs):
    """fb_wide320 1 against 0 on the smooth clip: all four level flows, the dense flow, flow_mean and flow_var, bit for bit, and equal to
    exact mode; no pair re-run; the shape the call took and how many launches ran in it."""
    import avd_hip
    n = npairs + 1
    xm, xv, xflow, xlv = exact_smooth
    with avd_hip.Context(0) as c:
        c.set_option("fb_mode", 1)
        for fold, want_launches in ((5, 2), (0, 3)):
            c.set_option("fb_fold_up", fold)
            got = {}
            for wide in (0, 1):
                c.set_option("fb_wide320", wide)
                tag = (npairs, fold, wide)
                fm, fv, flow = c.farneback_pairs(smooth[:n], want_flow=True)
                assert c.get_option("rerun_pairs") == 0, tag
                assert c.get_option("fb_wide320_used") == wide, tag
                assert _launches(c) == (want_launches if wide else 0), tag
                got[wide] = (fm, fv, flow, _levels(c, n))
            (fm0, fv0, flow0, lv0), (fm1, fv1, flow1, lv1) = got[0], got[1]
            for k in range(4):
                nd = int(np.count_nonzero(_bits(lv1[k]) != _bits(lv0[k])))
                print(f"[fbfast wide320] pairs {npairs} fold {fold} level {k}: {nd} of {lv1[k].size} values differ between the shapes")
                assert _same_bits(lv1[k], lv0[k]), (npairs, fold, k, nd)
                assert np.array_equal(lv1[k], xlv[k][:npairs]), (npairs, fold, k)
            assert _same_bits(flow1, flow0) and _same_bits(fm1, fm0) and _same_bits(fv1, fv0), (npairs, fold)
            assert np.array_equal(flow1, xflow[:npairs]), (npairs, fold)
            assert np.array_equal(fm1, xm[:npairs]) and np.array_equal(fv1, xv[:npairs]), (npairs, fold)


@pytest.mark.parametrize("name,frames", [("bands", _border_bands()), ("pan+3", _noise_pan(3)), ("pan-3", _noise_pan(-3))])
def test_border_columns(name, frames):
    """Texture only in the outermost fifteen columns, and noise panned by +-3 px: what reaches the replica slots of the vsum ring, lanes 0 and
    319 and the solver's first and last chunk.  The shapes agree bit for bit on the flag words and on the flow, whatever the flags are: with
    the exact re-run on (what a caller gets) and off (what the kernels themselves left, every level)."""
    import avd_hip
    n = len(frames)
    with avd_hip.Context(0) as c:
        c.set_option("fb_mode", 1)
        got = {}
        for wide in (0, 1):
            c.set_option("fb_wide320", wide)
            c.set_option("fb_rerun", 1)
            rec = c.analyze_frames(_bgr(frames)).copy()
            fm, fv, flow = c.farneback_pairs(frames, want_flow=True)
            assert c.get_option("fb_wide320_used") == wide and _launches(c) == 2 * wide
            c.set_option("fb_rerun", 0)
            rm, rv, raw = c.farneback_pairs(frames, want_flow=True)
            got[wide] = (rec, fm, fv, flow, rm, rv, raw, _levels(c, n))
        a, b = got[0], got[1]
        print(f"[fbfast wide320] {name}: flags {a[0]['reserved'].tolist()} / {b[0]['reserved'].tolist()}")
        assert np.array_equal(a[0]["reserved"], b[0]["reserved"]), name
        assert a[0].tobytes() == b[0].tobytes(), name
        for i in range(1, 7):
            assert _same_bits(a[i], b[i]), (name, i)
        for k in range(4):
            assert _same_bits(a[7][k], b[7][k]), (name, k)


def test_identical_frames_and_a_flagged_pair(smooth):
    """The clip of tests/test_gpu_fbfast_balance.py: a run of identical frames (exempt from the border-sign criterion) next to a pair the
    kernels flag (its workgroups leave at the flag word).  Flag words, statistics and level flows are the same bits in both shapes, the
    flagged pair included."""
    import avd_hip
    ramp, rolled = _families()["ramp_roll"](np.random.default_rng(3))
    frames = np.stack([smooth[0], smooth[1], smooth[1], smooth[1], smooth[1], smooth[2], ramp, rolled, smooth[4], smooth[5]])
    same, hard = (1, 2, 3), 6
    with avd_hip.Context(0) as c:
        got = {}
        for wide in (0, 1):
            c.set_option("fb_wide320", wide)
            rec = c.analyze_frames(_bgr(frames)).copy()
            assert rec["reserved"][hard + 1] != 0 and not any(rec["reserved"][p + 1] for p in same), (wide, rec["reserved"].tolist())
            assert c.get_option("fb_wide320_used") == wide and _launches(c) == 2 * wide
            got[wide] = (rec, _levels(c, len(frames)))
        (rec0, lv0), (rec1, lv1) = got[0], got[1]
        for key in ("reserved", "flow_mean", "flow_var"):
            assert _same_bits(rec1[key], rec0[key]), key
        assert rec1.tobytes() == rec0.tobytes()
        for k in range(4):
            assert _same_bits(lv1[k], lv0[k]), k


def test_both_store_forms(smooth):
    """The level's last launch in the new shape without the flow stores (analyze_frames: |flow| only; "flow0" is then fetched through the
    repeated launch) and with them (farneback_pairs(want_flow=True)): the same bits, and the two-strip shape's."""
    import avd_hip
    n = 4
    with avd_hip.Context(0) as c:
        got = {}
        for wide in (0, 1):
            c.set_option("fb_wide320", wide)
            rec = c.analyze_frames(_bgr(smooth[:n])).copy()
            assert c.get_option("fb_wide320_used") == wide and _launches(c) == 2 * wide
            late = _levels(c, n)[0]
            fm, fv, flow = c.farneback_pairs(smooth[:n], want_flow=True)
            stored = _levels(c, n)[0]
            assert _same_bits(late, stored), wide
            assert _same_bits(rec["flow_mean"][1:], fm) and _same_bits(rec["flow_var"][1:], fv), wide
            assert _same_bits(np.moveaxis(stored, 1, -1), flow), wide          # the dense flow is the level's flow, interleaved
            got[wide] = (rec, stored, flow)
        assert got[0][0].tobytes() == got[1][0].tobytes()
        assert _same_bits(got[0][1], got[1][1]) and _same_bits(got[0][2], got[1][2])


def test_the_320_px_shape_follows_what_is_in_flight():
    """fb_wide320 = 2: a call enqueued while another context of the process holds an undrained call runs a pair as one workgroup, a call that
    has the chip to itself as two strips; the records are the same either way."""
    import avd_hip
    clip = synth.make_clip(6, 360, 640, seed=31, dup_every=0)
    with avd_hip.Context(0) as a, avd_hip.Context(0) as b:
        b.set_option("fb_wide320", 2)
        alone = b.analyze_frames(clip).copy()
        assert b.get_option("fb_wide320_used") == 0 and _launches(b) == 0
        rec = np.zeros(len(clip), avd_hip.RECORD_DTYPE)
        keep = a.analyze_frames_async(clip, rec)               # enqueued, not drained
        shared = b.analyze_frames(clip).copy()
        assert b.get_option("fb_wide320_used") == 1 and _launches(b) == 2
        a.synchronize()
        del keep
        assert np.array_equal(alone, shared) and np.array_equal(rec, alone)
        again = b.analyze_frames(clip)
        assert b.get_option("fb_wide320_used") == 0 and np.array_equal(again, alone)
