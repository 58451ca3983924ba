"""The resizing first launch of the 320-px level of the fast Farneback kernel in the five-block shape (csrc/avd_fbfast.hip, UpN; option
"fb_wide320_up"): a pair is ONE workgroup of five 64-column blocks as in the level's other two launches (tests/test_gpu_fbfast_wide320.py),
and each normal-equation wave forms the launch's input flow -- cv2's resize(160-px flow, INTER_LINEAR) * 2 -- for its own columns in
registers, where the two-strip launch has its chain wave hand it over through an LDS ring.  The operations and their operands are the same
per column in both forms (one device function for the horizontal blend, one for the vertical), so everything is compared bit for bit:
option 1 against 0, on well-posed and on ill-posed content.

The level size is fixed by the library; the small dimension is the pair count.  1 pair is the smallest case, 9 pairs the first count with
two pairs per XCD group and workgroups that leave at once.

Which launches take the shape (debug buffers, per call): "fb_wide320_up_launches" counts the resizing launch (1 per chunk with the option
on, the fold on and the call in the five-block shape, else 0), "fb_wide320_launches" the launches that read a 320-px flow as before (2,
and 3 with fb_fold_up = 0, where k_flow_up resizes and the first launch is a plain one).

What the content reaches: lane column 0 (weights (1, 0)), column 319 (the copied value), coarse rows clipped at 0 and 159, the look-ahead
past the last image row -- the border bands, the noise pans and the sheared clip have a 160-px flow that changes from row to row and from
column to column, so a wrong coarse row, column or weight shows as different bits.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from avd_hip import synth  # noqa: E402
from tests.content_families import families as _families  # noqa: E402

PAIRS = (1, 2, 9)


def _levels(c, n):
    return [c.debug_fetch(f"flow{k}", (n - 1, 2, 320 >> k, 320 >> k), np.float32) for k in range(4)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _launches(c):
    """(launches that read a 320-px flow, resizing launches) of the last call in the five-block shape"""
    return (int(c.debug_fetch("fb_wide320_launches", (1,), np.int32)[0]), int(c.debug_fetch("fb_wide320_up_launches", (1,), np.int32)[0]))


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


def _noise_pan_vertical(step):
    """the same, panned vertically: new rows enter at the top or the bottom border"""
    field = np.random.default_rng(29).integers(0, 256, (320 + 16, 320), dtype=np.uint8)
    y0 = 8
    return np.stack([field[y0 - step * i: y0 - step * i + 320] for i in range(3)])


def _shear():
    """white noise whose upper half pans left and whose lower half pans right, 2 px per frame: the flow changes sign across row 160"""
    field = np.random.default_rng(31).integers(0, 256, (320, 320 + 16), dtype=np.uint8)
    x0 = 8
    frames = []
    for i in range(3):
        f = np.empty((320, 320), np.uint8)
        f[:160] = field[:160, x0 + 2 * i: x0 + 2 * i + 320]
        f[160:] = field[160:, x0 - 2 * i: x0 - 2 * i + 320]
        frames.append(f)
    return np.stack(frames)


@pytest.mark.parametrize("npairs", PAIRS)
def test_three_forms_agree(smooth, exact_smooth, npairs):
    """Under fb_wide320 = 1 on the smooth clip: fb_wide320_up 1 against 0, both against fb_fold_up = 0 (k_flow_up, then three plain five-block
    launches) and against exact mode: all four level flows, the dense flow, flow_mean and flow_var, bit for bit; no pair re-run; the launch
    counts."""
    import avd_hip
    n = npairs + 1
    xm, xv, xflow, xlv = exact_smooth
    with avd_hip.Context(0) as c:
        c.set_option("fb_mode", 1)
        c.set_option("fb_wide320", 1)
        got = {}
        for fold, up, want in ((5, 1, (2, 1)), (5, 0, (2, 0)), (0, 1, (3, 0)), (0, 0, (3, 0))):
            c.set_option("fb_fold_up", fold)
            c.set_option("fb_wide320_up", up)
            fm, fv, flow = c.farneback_pairs(smooth[:n], want_flow=True)
            assert c.get_option("rerun_pairs") == 0, (npairs, fold, up)
            assert c.get_option("fb_wide320_used") == 1 and _launches(c) == want, (npairs, fold, up, _launches(c))
            got[fold, up] = (fm, fv, flow, _levels(c, n))
        fm1, fv1, flow1, lv1 = got[5, 1]
        for key in ((5, 0), (0, 1), (0, 0)):
            fm0, fv0, flow0, lv0 = got[key]
            for k in range(4):
                nd = int(np.count_nonzero(_bits(lv1[k]) != _bits(lv0[k])))
                print(f"[fbfast wide320 up] pairs {npairs} against fold, up = {key} level {k}: {nd} of {lv1[k].size} values differ")
                assert _same_bits(lv1[k], lv0[k]), (npairs, key, k, nd)
            assert _same_bits(flow1, flow0) and _same_bits(fm1, fm0) and _same_bits(fv1, fv0), (npairs, key)
        for k in range(4):
            assert np.array_equal(lv1[k], xlv[k][:npairs]), (npairs, k)
        assert np.array_equal(flow1, xflow[:npairs]), npairs
        assert np.array_equal(fm1, xm[:npairs]) and np.array_equal(fv1, xv[:npairs]), npairs


@pytest.mark.parametrize("name,frames", [("bands", _border_bands()), ("pan+3", _noise_pan(3)), ("pan-3", _noise_pan(-3)), ("shear", _shear()),
                                         ("vpan+3", _noise_pan_vertical(3)), ("vpan-3", _noise_pan_vertical(-3))])
def test_flow_that_changes_per_row_and_column(name, frames):
    """Content whose 160-px flow varies from row to row and column to column, up to the borders.  Option 1 against 0, with the exact re-run
    on (what a caller gets) and off (what the kernels themselves left, every level): flag words, records and flows are the same bits."""
    import avd_hip
    n = len(frames)
    with avd_hip.Context(0) as c:
        c.set_option("fb_mode", 1)
        c.set_option("fb_wide320", 1)
        got = {}
        for up in (0, 1):
            c.set_option("fb_wide320_up", up)
            c.set_option("fb_rerun", 1)
            rec = c.analyze_frames(_bgr(frames)).copy()
            fm, fv, flow = c.farneback_pairs(frames, want_flow=True)
            assert _launches(c) == (2, up), (name, up, _launches(c))
            c.set_option("fb_rerun", 0)
            rm, rv, raw = c.farneback_pairs(frames, want_flow=True)
            got[up] = (rec, fm, fv, flow, rm, rv, raw, _levels(c, n))
        a, b = got[0], got[1]
        print(f"[fbfast wide320 up] {name}: flags {a[0]['reserved'].tolist()} / {b[0]['reserved'].tolist()}")
        assert np.array_equal(a[0]["reserved"], b[0]["reserved"]), name
        assert a[0].tobytes() == b[0].tobytes(), name
        for i in range(1, 7):
            assert _same_bits(a[i], b[i]), (name, i)
        for k in range(4):
            assert _same_bits(a[7][k], b[7][k]), (name, k)


def test_both_store_forms(smooth):
    """analyze_frames (the level's last launch keeps |flow| only; "flow0" is then fetched through the repeated launch) and
    farneback_pairs(want_flow=True), with the resizing launch in the five-block shape: the same bits, and those of the option off."""
    import avd_hip
    n = 4
    with avd_hip.Context(0) as c:
        c.set_option("fb_wide320", 1)
        got = {}
        for up in (0, 1):
            c.set_option("fb_wide320_up", up)
            rec = c.analyze_frames(_bgr(smooth[:n])).copy()
            assert _launches(c) == (2, up), (up, _launches(c))
            late = _levels(c, n)[0]
            fm, fv, flow = c.farneback_pairs(smooth[:n], want_flow=True)
            stored = _levels(c, n)[0]
            assert _same_bits(late, stored), up
            assert _same_bits(rec["flow_mean"][1:], fm) and _same_bits(rec["flow_var"][1:], fv), up
            assert _same_bits(np.moveaxis(stored, 1, -1), flow), up              # the dense flow is the level's flow, interleaved
            got[up] = (rec, stored, flow)
        assert got[0][0].tobytes() == got[1][0].tobytes()
        assert _same_bits(got[0][1], got[1][1]) and _same_bits(got[0][2], got[1][2])


def test_the_shape_follows_what_is_in_flight():
    """fb_wide320 = 2, fb_wide320_up = 1: a call enqueued while another context of the process holds an undrained call runs the resizing
    launch as one workgroup per pair, the same call alone as two strips; the records are the same either way."""
    import avd_hip
    clip = synth.make_clip(6, 360, 640, seed=31, dup_every=0)
    with avd_hip.Context(0) as a, avd_hip.Context(0) as b:
        b.set_option("fb_wide320", 2)
        b.set_option("fb_wide320_up", 1)
        alone = b.analyze_frames(clip).copy()
        assert b.get_option("fb_wide320_used") == 0 and _launches(b) == (0, 0)
        rec = np.zeros(len(clip), avd_hip.RECORD_DTYPE)
        keep = a.analyze_frames_async(clip, rec)               # enqueued, not drained
        shared = b.analyze_frames(clip).copy()
        assert b.get_option("fb_wide320_used") == 1 and _launches(b) == (2, 1)
        a.synchronize()
        del keep
        assert np.array_equal(alone, shared) and np.array_equal(rec, alone)
        again = b.analyze_frames(clip)
        assert _launches(b) == (0, 0) and np.array_equal(again, alone)


def test_identical_frames_and_a_flagged_pair(smooth):
    """(Last in the file.)  The clip of tests/test_gpu_fbfast_balance.py: a run of identical frames next to a pair the kernels flag.  A pair
    that a coarser level has flagged makes its workgroup leave at the first barrier in the resizing five-block launch too; records and level
    flows equal those of the option off, the flagged pair included."""
    import avd_hip
    ramp, rolled = _families()["ramp_roll"](np.random.default_rng(3))
    frames = np.stack([smooth[0], smooth[1], smooth[1], smooth[1], smooth[1], smooth[2], ramp, rolled, smooth[4], smooth[5]])
    same, hard = (1, 2, 3), 6
    with avd_hip.Context(0) as c:
        c.set_option("fb_wide320", 1)
        got = {}
        for up in (0, 1):
            c.set_option("fb_wide320_up", up)
            rec = c.analyze_frames(_bgr(frames)).copy()
            assert rec["reserved"][hard + 1] != 0 and not any(rec["reserved"][p + 1] for p in same), (up, rec["reserved"].tolist())
            assert _launches(c) == (2, up), (up, _launches(c))
            got[up] = (rec, _levels(c, len(frames)))
        (rec0, lv0), (rec1, lv1) = got[0], got[1]
        for key in ("reserved", "flow_mean", "flow_var"):
            assert _same_bits(rec1[key], rec0[key]), key
        assert rec1.tobytes() == rec0.tobytes()
        for k in range(4):
            assert _same_bits(lv1[k], lv0[k]), k
