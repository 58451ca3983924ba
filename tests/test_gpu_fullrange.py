"""Full-range 4:2:0 pictures (AVD_FMT_FULL_RANGE: ffmpeg's yuvj420p and its semi-planar form) in the fused ingest.

Definition under test: a picture with the flag gives, BIT FOR BIT, what the BGR entry points give on the BGR frame libswscale's table
converter makes of it with full-range tables (tests/yuv_tables_reference.py: the literal tables, tied to the pinned limited-range converter by
tests/test_fullrange_host.py) -- and what the CPU oracle's preprocess gives on that frame.  There is no tolerance in this file.

Every plane set holds the enumeration of (Y, U, V) over {0, 1, 15, 16, 17, 127, 128, 129, 234, 235, 240, 254, 255}^3, one 2 x 2 cell
each, beside seeded random bytes (yuv_tables_reference.enum_planes): the enumeration reaches both ends of the full-range index window of
the gray tables, Y + offset = -226 at (Y, U) = (0, 0) and 480 at (255, 255), five entries outside the window the tables had before.
Every kernel case asserts the kernel that ran from "ingest_plan", "ingest_rotate" and "ingest_range"."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import avd_hip  # noqa: E402
from avd_hip import AvdError, _lib, synth  # noqa: E402
from tests import yuv_tables_reference as ref  # noqa: E402
from tests.ingest_gpu_kit import P_LDS, P_PITCH, check_plan  # noqa: E402
from tests.test_gpu_i420 import _device_view  # noqa: E402

KERNEL_NAMES = ("bgr_scalar", "bgr_vec16", "bgr_staged", "nv12_scalar", "nv12_tables", "i420_scalar", "i420_tables", "nv12_strip", "i420_strip")
SCALAR, TABLES, STRIP = {"nv12": 3, "i420": 5}, {"nv12": 4, "i420": 6}, {"nv12": 7, "i420": 8}


def _check_plan(ctx, h, w, kernel, rows, rotate, full):
    """h, w: the DISPLAYED picture"""
    p = check_plan(ctx, h, w, kernel, rows, rotate=rotate, full_range=full)
    tag = (h, w, rotate, full, p)
    if kernel not in SCALAR.values():
        # the three gray tables behind the tile: 704 entries each hold the limited window [-221, 475], the full one [-226, 480] needs 707 at least
        assert p[P_LDS] >= (rows + 2) * p[P_PITCH] + 3 * 4 * (707 if full else 704), tag
        if not full:
            assert p[P_LDS] == ((rows + 2) * p[P_PITCH] + 15) // 16 * 16 + 3 * 4 * 704, tag      # as it was before there was a range
        assert p[P_LDS] <= 64 * 1024, tag


# ---- the displayed pictures and what is expected of them, formed once and left unchanged ---------------------------------------------------
_cases = {}


def _displayed(ctx, oracle, h, w):
    """-> (NV12 planes of the displayed picture, {full: (small320, hash1024, lap_sum, lap_sumsq) of avd_preprocess_bgr on the restatement's BGR
    frames}); the CPU oracle's preprocess of those frames is compared here, once"""
    key = (h, w)
    if key not in _cases:
        n = ref.enum_frames(h, w) + 1
        y, uv = ref.enum_planes(n, h, w, seed=h + w)
        want = {}
        for full in (False, True):
            bgr = ref.nv12_to_bgr(y, uv, full)
            want[full] = ctx.preprocess_bgr(bgr)
            for name, a, b in zip(("small320", "hash1024", "lap_sum", "lap_sumsq"), want[full], oracle.preprocess_bgr(bgr)):
                assert np.array_equal(a, b), (key, full, name)
        _cases[key] = ((y, uv), want)
    return _cases[key]


def _stored(displayed, k, kind):
    """the stored planes whose picture, turned k quarter turns clockwise, is `displayed` (an NV12 pair)"""
    s = synth.rotate_planes(displayed, (4 - k) % 4)
    return synth.nv12_to_i420(*s) if kind == "i420" else s


def _equal(got, want, tag):
    for name, a, b in zip(("small320", "hash1024", "lap_sum", "lap_sumsq"), got, want):
        assert np.array_equal(a, b), (tag, name, int(np.count_nonzero(np.asarray(a) != np.asarray(b))))


# ---- 1: every fill, both surface kinds, host and device input ----------------------------------------------------------------------------------
# (name, displayed h, w, rotate, fill, rows per band, view).  view "plus1": device planes whose Y plane starts one byte off a 16-byte
# boundary, which takes the tables away from a width that would have them.  36 x 2064: bands of 7 rows, the last one a single row (the
# tables sit lower in LDS than the launcher reserved for; class (2064, 7) of tests/test_gpu_ingest_plan.py).
FILLS = [
    ("tables", 64, 96, 0, TABLES, 14, "host"), ("tables", 64, 96, 0, TABLES, 14, "device"),
    ("scalar", 38, 50, 0, SCALAR, 14, "host"), ("scalar", 38, 50, 0, SCALAR, 14, "device"),
    ("scalar-offset", 64, 96, 0, SCALAR, 14, "plus1"),
    ("flipped-tables", 64, 96, 2, TABLES, 14, "host"), ("flipped-tables", 64, 96, 2, TABLES, 14, "device"),
    ("flipped-scalar", 38, 50, 2, SCALAR, 14, "host"), ("flipped-scalar", 38, 50, 2, SCALAR, 14, "device"),
    ("strip", 64, 96, 1, STRIP, 14, "host"), ("strip", 64, 96, 1, STRIP, 14, "device"),
    ("strip", 64, 96, 3, STRIP, 14, "host"), ("strip", 64, 96, 3, STRIP, 14, "device"),
    ("short-last-band", 36, 2064, 0, TABLES, 7, "host"), ("short-last-band", 36, 2064, 0, TABLES, 7, "device"),
    ("short-last-band-strip", 36, 2064, 1, STRIP, 7, "device"),
]


def _input(stored, view):
    if view == "host":
        return stored
    torch = pytest.importorskip("torch")
    if view == "device":
        return tuple(torch.from_numpy(p).to("cuda:0") for p in stored)
    return tuple(_device_view(torch, p, (1 if i == 0 else 0, 0, False)) for i, p in enumerate(stored))


@pytest.mark.parametrize("kind", ["nv12", "i420"])
@pytest.mark.parametrize("name,h,w,k,fill,rows,view", FILLS, ids=[f"{c[0]}-k{c[3]}-{c[6]}" for c in FILLS])
def test_every_fill_with_full_range_constants(ctx, oracle, kind, name, h, w, k, fill, rows, view):
    displayed, want = _displayed(ctx, oracle, h, w)
    stored = _stored(displayed, k, kind)
    assert stored[0].shape[1:] == ((w, h) if k & 1 else (h, w))               # quarter turns: stored 96 high, 64 wide
    planes = _input(stored, view)
    got = ctx.preprocess_picture(planes, k, full_range=True)
    _check_plan(ctx, h, w, fill[kind], rows, k, True)
    _equal(got, want[True], (kind, name, k, view, "full"))
    assert ctx.stage_bytes() == (sum(p.nbytes for p in stored) if view == "host" else 0)
    # 2: the same planes without the flag are the limited-range pictures they always were, through the same kernel
    got = ctx.preprocess_picture(planes, k)
    _check_plan(ctx, h, w, fill[kind], rows, k, False)
    _equal(got, want[False], (kind, name, k, view, "limited"))


# ---- 2: the flag is not ignored, and its absence changes nothing -------------------------------------------------------------------------------
def test_without_the_flag_nothing_changed(ctx, oracle):
    displayed, want = _displayed(ctx, oracle, 64, 96)
    y, uv = displayed
    planar = synth.nv12_to_i420(y, uv)
    limited = ctx.preprocess_nv12(y, uv)                                       # the format's own entry point: limited range
    assert ctx.ingest_range() == 0
    _equal(limited, want[False], "avd_preprocess_nv12")
    _equal(ctx.preprocess_picture((y, uv)), limited, "descriptor, no flag")
    _equal(ctx.preprocess_i420(*planar), limited, "avd_preprocess_i420")
    _equal(ctx.preprocess_nv12(y, uv, full_range=False), limited, "keyword False")
    full = ctx.preprocess_nv12(y, uv, full_range=True)
    assert ctx.ingest_range() == 1
    _equal(full, want[True], "keyword True")
    _equal(ctx.preprocess_i420(*planar, full_range=True), full, "i420 keyword True")
    assert not np.array_equal(full[3], limited[3]) and not np.array_equal(full[0], limited[0])
    # limited-range tables stretch the luma by 255 / 219: on random bytes most of that is clipped away again, but the second moment of
    # the Laplacian still differs in every frame
    assert (full[3] != limited[3]).all()
    bgr = ref.nv12_to_bgr(y, uv, True)
    ctx.preprocess_bgr(bgr)
    assert ctx.ingest_range() == 0                                             # a BGR launch has no range
    with avd_hip.Context(0) as fresh:
        with pytest.raises(AvdError, match="ingest_range"):
            fresh.ingest_range()                                               # no ingest launch yet


# ---- 3: a batch that mixes ranges ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch():
    """four 6-frame clips: NV12 limited 64 x 96, NV12 full 48 x 112, I420 full stored 96 x 64 and turned once, BGR 64 x 80; the 4:2:0 ones
    with the enumeration in their first frames"""
    a = ref.enum_planes(6, 64, 96, seed=41)
    b = ref.enum_planes(6, 48, 112, seed=42)
    c = synth.nv12_to_i420(*ref.enum_planes(6, 96, 64, seed=43))
    d = synth.make_clip(6, 64, 80, seed=44, dup_every=3)
    clips, turns, ranges = [a, b, c, d], [0, 0, 1, 0], [False, True, True, False]
    c_nv12 = ref.enum_planes(6, 96, 64, seed=43)
    bgr = [ref.nv12_to_bgr(*a, False), ref.nv12_to_bgr(*b, True), np.ascontiguousarray(np.rot90(ref.nv12_to_bgr(*c_nv12, True), -1, axes=(1, 2))), d]
    return clips, turns, ranges, bgr


@pytest.mark.parametrize("mode", [1, 0], ids=["fast", "exact"])
def test_a_batch_of_both_ranges(ctx, batch, mode):
    clips, turns, ranges, bgr = batch
    try:
        ctx.set_option("fb_mode", mode)
        single = [ctx.analyze_pictures([c], [k], [r])[0] for c, k, r in zip(clips, turns, ranges)]
        for i in range(4):
            assert single[i].tobytes() == ctx.analyze_frames(bgr[i]).tobytes(), (mode, i)       # the same context, the BGR frames of the clip
        assert single[0].tobytes() == ctx.analyze_frames_nv12(*clips[0]).tobytes()
        assert single[1].tobytes() == ctx.analyze_frames_nv12(*clips[1], full_range=True).tobytes()
        assert single[1].tobytes() != ctx.analyze_frames_nv12(*clips[1]).tobytes()
        assert single[2].tobytes() == ctx.analyze_frames_i420(*clips[2], rotate=1, full_range=True).tobytes()
        got = ctx.analyze_pictures(clips, turns, ranges)
        assert [len(r) for r in got] == [6, 6, 6, 6]
        assert np.concatenate(got).tobytes() == np.concatenate(single).tobytes()
        assert ctx.ingest_range() == 0                                         # the last clip's launch: BGR
        got = ctx.analyze_pictures(clips[:3], turns[:3], ranges[:3])
        assert np.concatenate(got).tobytes() == np.concatenate(single[:3]).tobytes()
        assert ctx.ingest_range() == 1 and ctx.ingest_rotate() == 1
        if mode == 1:
            rec = np.zeros(24, avd_hip.RECORD_DTYPE)
            keep, counts = ctx.analyze_pictures_async(clips, rec, turns, ranges)
            ctx.synchronize()
            del keep
            assert counts == [6, 6, 6, 6] and rec.tobytes() == np.concatenate(single).tobytes()
            rec = np.zeros(6, avd_hip.RECORD_DTYPE)
            keep = ctx.analyze_frames_i420_async(*clips[2], rec, rotate=1, full_range=True)
            ctx.synchronize()
            del keep
            assert rec.tobytes() == single[2].tobytes()
    finally:
        ctx.set_option("fb_mode", 1)
    with pytest.raises(ValueError, match="one range per clip"):
        ctx.analyze_pictures(clips, turns, ranges[:3])


# ---- 4: refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    y, uv = ref.enum_planes(3, 64, 96, seed=5)
    _, u, v = synth.nv12_to_i420(y, uv)
    bgr = synth.random_frames(3, 64, 96, seed=6)
    ctx.preprocess_picture((y, uv), 2, full_range=True)                        # the call before
    before = ctx.debug_fetch("ingest_plan", (8,), np.int32)
    assert (ctx.ingest_rotate(), ctx.ingest_range()) == (2, 1)
    L, H = ctx._L, ctx._h
    FULL = _lib.AVD_FMT_FULL_RANGE

    def call(clip, fmt, edit=None):
        p, n, keep = ctx._picture(clip, 0)
        p.format = fmt
        if edit:
            edit(p)
        rec = np.zeros(3, avd_hip.RECORD_DTYPE)
        small = np.empty((3, 320, 320), np.uint8)
        rcs = (L.avd_analyze_pictures(H, ctypes.byref(p), 1, rec.ctypes.data), L.avd_analyze_pictures_async(H, ctypes.byref(p), 1, rec.ctypes.data),
               L.avd_preprocess_picture(H, ctypes.byref(p), small.ctypes.data, None, None, None))
        assert rcs[0] == rcs[1] == rcs[2], rcs
        return rcs[0], L.avd_last_error(H).decode()

    ARG = -1
    assert call(bgr, _lib.AVD_FMT_BGR24 | FULL) == (ARG, "AVD_FMT_FULL_RANGE describes 4:2:0 samples: a BGR picture has no range")
    assert call(bgr, _lib.AVD_FMT_BGR24 | FULL, lambda p: setattr(p, "rotate", 1))[1].startswith("AVD_FMT_FULL_RANGE")   # before the BGR turn
    for clip, fmt in (((y, uv), _lib.AVD_FMT_NV12), ((y, u, v), _lib.AVD_FMT_I420)):
        assert call(clip, 3 | FULL) == (ARG, "bad avd_picture.format")
        assert call(clip, fmt | 0x200) == (ARG, "bad avd_picture.format")
        assert call(clip, fmt | FULL | 0x200) == (ARG, "bad avd_picture.format")
        assert call(clip, fmt | FULL | 0x10000) == (ARG, "bad avd_picture.format")
        assert call(clip, fmt | 0x200, lambda p: setattr(p, "rotate", 4)) == (ARG, "bad avd_picture.format")        # format before rotate
        assert call(clip, fmt | FULL, lambda p: setattr(p, "rotate", 4)) == (ARG, "avd_picture.rotate must be 0 .. 3 quarter turns")
        assert call(clip, fmt | FULL, lambda p: setattr(p, "reserved", 1)) == (ARG, "avd_picture.reserved must be 0")
        assert call(clip, fmt | FULL, lambda p: setattr(p, "mem", 2)) == (ARG, "mem must be AVD_MEM_HOST or AVD_MEM_DEVICE")
        rc, msg = call(clip, fmt | FULL, lambda p: setattr(p, "w", 95))
        assert rc == -4 and "even width and height" in msg, (rc, msg)
    with pytest.raises(AvdError, match="a BGR picture has no range"):
        ctx.preprocess_picture(bgr, 0, full_range=True)
    with pytest.raises(AvdError, match="a BGR picture has no range"):
        ctx.analyze_pictures([(y, uv), bgr], None, [True, True])               # the second clip of a batch
    # nothing was launched by any of them
    assert np.array_equal(ctx.debug_fetch("ingest_plan", (8,), np.int32), before)
    assert (ctx.ingest_rotate(), ctx.ingest_range()) == (2, 1)
    assert call((y, uv), _lib.AVD_FMT_NV12 | FULL)[0] == 0 and (ctx.ingest_rotate(), ctx.ingest_range()) == (0, 1)   # the descriptor itself is fine


# ---- 5: end to end -------------------------------------------------------------------------------------------------------------------------------
def test_a_full_range_y4m_end_to_end(tmp_path, monkeypatch):
    """A .y4m with XCOLORRANGE=FULL: the drop-in analyzer, the streaming FrameAnalyzer and the per-file pipeline give what they give on the
    BGR frames libswscale makes of yuvj420p, across streaming chunk boundaries, for both surfaces a .y4m can yield; without the token the
    same file is a limited-range clip with another result."""
    from app.analyzers import video
    from avd_hip import pipeline, sources
    n, h, w = 10, 64, 96
    y, uv = ref.enum_planes(n, h, w, seed=25)
    path, plain = str(tmp_path / "mjpeg.y4m"), str(tmp_path / "plain.y4m")
    sources.write_y4m(path, y, uv, fps=(4, 1), full_range=True)                # 4 fps: step 2 -> 5 sampled frames
    sources.write_y4m(plain, y, uv, fps=(4, 1))
    monkeypatch.setenv("AVD_CHUNK_FRAMES", "2")                                # chunks of 2 + carry: 2, 2, 1
    monkeypatch.delenv("AVD_Y4M_SURFACE", raising=False)
    bgr = ref.nv12_to_bgr(y, uv, True)
    npy = str(tmp_path / "mjpeg.npy")
    np.save(npy, bgr)
    meta = {"fps": 4.0, "duration": n / 4.0}                                   # what the .y4m header says; size from the frames
    want = video.analyze(npy, dict(meta))
    got = video.analyze(path, {})
    assert got == want and len(got["timeline"]) == 2
    assert video.analyze(plain, {}) != want
    monkeypatch.setenv("AVD_Y4M_SURFACE", "i420")
    assert video.analyze(path, {}) == want
    monkeypatch.delenv("AVD_Y4M_SURFACE")
    full_meta = {"width": w, "height": h, "fps": 4.0, "duration": n / 4.0, "bit_rate": 2_000_000}
    body, body_bgr = pipeline.analyze_path(path, dict(full_meta)), pipeline.analyze_path(npy, dict(full_meta))
    assert body["video"] == body_bgr["video"] == want
    with avd_hip.Context(0) as c:
        fa = avd_hip.FrameAnalyzer(chunk=3, ctx=c)
        rec = fa.records_stream(iter(bgr))
        src = sources.open_source(path)
        assert src.full_range and src.surface == "nv12"
        assert fa.records_stream_nv12(src.sampled(1), full_range=src.full_range).tobytes() == rec.tobytes()
        src.close()
        planar = sources.open_source(path, planar=True)
        assert fa.records_stream_i420(planar.sampled(1), full_range=planar.full_range).tobytes() == rec.tobytes()
        assert fa.records_stream_i420(planar.sampled(1)).tobytes() != rec.tobytes()
        planar.close()
