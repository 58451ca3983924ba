"""Rotated decoder pictures in the fused 4:2:0 ingest: avd_picture with rotate = 1, 2, 3 (include/avd.h).

Definition under test: the displayed picture is D = np.rot90(S, -rotate) of every stored plane, and every output of a call with rotate = k
equals, BIT FOR BIT, the output of the format's own entry point on D's planes.  So every case builds the DISPLAYED planes first, takes the
CPU oracle's results on them (tests.test_gpu_i420._reference: NV12 -> BGR, then the BGR oracle) once per geometry, and hands the library
the planes turned back (synth.rotate_planes(D, 4 - k)) with rotate = k.  There is no tolerance in this file.

The kernels: a half turn runs flipped instantiations of the four 4:2:0 fills (same kernel ids, same tables / scalar dispatch); a quarter
turn runs the strip fill (kernel ids 7 nv12_strip, 8 i420_strip) for every geometry and alignment.  Every case reads "ingest_plan" and
"ingest_rotate", so a case that silently took another fill fails."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import avd_hip  # noqa: E402
from avd_hip import AvdError, _lib, synth  # noqa: E402
from tests.test_gpu_i420 import VIEWS, _check_outputs, _device_view, _heights, _reference  # noqa: E402
from tests.ingest_gpu_kit import GRAY_TABLES, check_plan  # noqa: E402
from tests.test_nv12 import _planes  # noqa: E402

KERNEL_NAMES = ("bgr_scalar", "bgr_vec16", "bgr_staged", "nv12_scalar", "nv12_tables", "i420_scalar", "i420_tables", "nv12_strip", "i420_strip")
NV12_SCALAR, NV12_TABLES, I420_SCALAR, I420_TABLES, NV12_STRIP, I420_STRIP = 3, 4, 5, 6, 7, 8


def _check_plan(ctx, h, w, kernel, rows, rotate, lds=None):
    """h, w: the DISPLAYED picture"""
    check_plan(ctx, h, w, kernel, rows, 0, lds, lds_behind_tile=0 if kernel in (NV12_SCALAR, I420_SCALAR) else GRAY_TABLES, rotate=rotate)


_displayed = {}


def _displayed_case(oracle, h, w, n=2):
    """The displayed planes of a geometry (NV12 form, independent random bytes) and the oracle's results on them: formed once, shared by
    every rotation and surface kind, left unchanged."""
    key = (n, h, w)
    if key not in _displayed:
        y, uv = _planes(n, h, w, seed=h + w)
        _displayed[key] = ((y, uv), _reference(oracle, y, uv))
    return _displayed[key]


def _stored(displayed, k, kind):
    """the stored planes whose picture, turned k quarter turns clockwise, is `displayed` (an NV12 pair)"""
    s = synth.rotate_planes(displayed, (4 - k) % 4)
    return synth.nv12_to_i420(*s) if kind == "i420" else s


def _cases(widths_rows, ks, name):
    return [pytest.param(kind, k, w, r, h, id=f"{kind}-{name}-k{k}-w{w}-r{r}-h{h}")
            for kind in ("nv12", "i420") for k in ks for w, r in widths_rows for h in _heights(r)]


# ---- 1: the strip fills over the plan classes -------------------------------------------------------------------------------------------
# (displayed width, rows per band).  The stored picture is w rows of h columns.  Odd row counts make bands start on an odd stored column,
# so one chroma sample is split between two workgroups; 34 is no multiple of 16 (the reflected halo rows are copied in 16-byte words that
# end in the tile row's padding); 2064, 4112 and 12272 take several passes of the workgroup over the displayed columns.
STRIP_PLANS = [(34, 14), (48, 14), (2064, 7), (4112, 9), (12272, 1)]


@pytest.mark.parametrize("kind,k,w,rows,h", _cases(STRIP_PLANS, (1, 3), "strip"))
def test_strip_fill_plan_classes(ctx, oracle, kind, k, w, rows, h):
    displayed, want = _displayed_case(oracle, h, w)
    stored = _stored(displayed, k, kind)
    assert stored[0].shape == (2, w, h)
    got = ctx.preprocess_picture(stored, k)
    _check_plan(ctx, h, w, I420_STRIP if kind == "i420" else NV12_STRIP, rows, k)
    _check_outputs(ctx, got, want, (kind, k, h, w))
    assert ctx.stage_bytes() == sum(p.nbytes for p in stored)             # the stored planes, separately allocated


# ---- 2: the half turn: the same two fills per surface kind --------------------------------------------------------------------------------
HALF_TABLE_PLANS = [(48, 14), (2064, 7), (16384, 1)]
HALF_SCALAR_PLANS = [(34, 14), (1922, 14)]


@pytest.mark.parametrize("kind,k,w,rows,h", _cases(HALF_TABLE_PLANS, (2,), "tables") + _cases(HALF_SCALAR_PLANS, (2,), "scalar"))
def test_half_turn_plan_classes(ctx, oracle, kind, k, w, rows, h):
    displayed, want = _displayed_case(oracle, h, w)
    stored = _stored(displayed, 2, kind)
    assert stored[0].shape == (2, h, w)
    got = ctx.preprocess_picture(stored, 2)
    tables = w % 16 == 0
    kernel = {("nv12", True): NV12_TABLES, ("nv12", False): NV12_SCALAR, ("i420", True): I420_TABLES, ("i420", False): I420_SCALAR}[kind, tables]
    _check_plan(ctx, h, w, kernel, rows, 2, 57696 if w == 16384 else None)     # 3 * 16416 + 3 * 4 * 704, as unrotated
    _check_outputs(ctx, got, want, (kind, 2, h, w))
    assert ctx.stage_bytes() == sum(p.nbytes for p in stored)


def test_rotate_0_through_the_descriptor_is_todays_call(ctx, oracle):
    displayed, want = _displayed_case(oracle, 44, 48)
    got = ctx.preprocess_picture(synth.nv12_to_i420(*displayed), 0)
    _check_plan(ctx, 44, 48, I420_TABLES, 14, 0)
    _check_outputs(ctx, got, want, "i420 k0")
    got = ctx.preprocess_picture(displayed, 0)
    _check_plan(ctx, 44, 48, NV12_TABLES, 14, 0)
    _check_outputs(ctx, got, want, "nv12 k0")
    bgr = oracle.nv12_to_bgr(*displayed)
    got = ctx.preprocess_picture(bgr)
    assert ctx.ingest_rotate() == 0
    _check_outputs(ctx, got, want, "bgr")
    with avd_hip.Context(0) as fresh:
        with pytest.raises(AvdError, match="ingest_rotate"):
            fresh.ingest_rotate()                                             # no ingest launch yet


# ---- 3: alignment and strides on device views -----------------------------------------------------------------------------------------------
# displayed 46 x 2064 (7 rows per band) throughout.  view -> (base offset, row padding, odd frame stride) per plane, as VIEWS of
# tests/test_gpu_i420.py.  The strip fill's spans are unaligned by nature: every view runs the one fill and gives the oracle's results.
A_H, A_W, A_ROWS = 46, 2064, 7
STRIP_VIEWS_I420 = {
    "y_base+1": ((1, 0, False), (0, 0, False), (0, 0, False)),
    "padded_row_stride": ((0, 13, False), (0, 7, False), (0, 7, False)),
    "odd_frame_stride": ((0, 0, True), (0, 0, True), (0, 0, True)),
    "chroma_8mod16": ((0, 0, False), (8, 0, False), (24, 0, False)),
    "everything_odd": ((3, 5, True), (1, 3, True), (7, 3, True)),
}
STRIP_VIEWS_NV12 = {
    "y_base+1": ((1, 0, False), (0, 0, False)),
    "padded_row_stride": ((0, 13, False), (0, 6, False)),
    "odd_frame_stride": ((0, 0, True), (0, 0, True)),
    "uv_base+1": ((0, 0, False), (1, 0, False)),
}


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("kind,view", [("i420", v) for v in STRIP_VIEWS_I420] + [("nv12", v) for v in STRIP_VIEWS_NV12])
def test_strip_fill_on_every_alignment(ctx, oracle, kind, view, k):
    torch = pytest.importorskip("torch")
    displayed, want = _displayed_case(oracle, A_H, A_W)
    stored = _stored(displayed, k, kind)
    specs = (STRIP_VIEWS_I420 if kind == "i420" else STRIP_VIEWS_NV12)[view]
    views = [_device_view(torch, p, spec) for p, spec in zip(stored, specs)]
    if view == "chroma_8mod16":
        assert views[1].data_ptr() % 16 == 8 and views[2].data_ptr() % 16 == 8
    got = ctx.preprocess_picture(tuple(views), k)
    _check_plan(ctx, A_H, A_W, I420_STRIP if kind == "i420" else NV12_STRIP, A_ROWS, k)
    _check_outputs(ctx, got, want, (kind, view, k))
    assert ctx.stage_bytes() == 0


@pytest.mark.parametrize("view", list(VIEWS))
def test_half_turn_dispatches_as_the_unrotated_i420_kernels(ctx, oracle, view):
    torch = pytest.importorskip("torch")
    displayed, want = _displayed_case(oracle, A_H, A_W)
    kernel, *specs = VIEWS[view]                                               # the kernel the UNROTATED call runs on this view
    views = [_device_view(torch, p, spec) for p, spec in zip(_stored(displayed, 2, "i420"), specs)]
    got = ctx.preprocess_picture(tuple(views), 2)
    _check_plan(ctx, A_H, A_W, kernel, A_ROWS, 2)
    _check_outputs(ctx, got, want, view)
    ctx.preprocess_i420(*views)                                                # and it does: same view, same kernel
    _check_plan(ctx, A_H, A_W, kernel, A_ROWS, 0)


@pytest.mark.parametrize("view,kernel,specs", [("aligned16_padded", NV12_TABLES, ((32, 16, False), (16, 16, False))),
                                               ("y_base+1", NV12_SCALAR, ((1, 16, False), (0, 16, False))),
                                               ("uv_row_stride%16=8", NV12_SCALAR, ((0, 16, False), (0, 8, False))),
                                               ("y_frame_stride_odd", NV12_SCALAR, ((0, 16, True), (0, 16, False)))])
def test_half_turn_dispatches_as_the_unrotated_nv12_kernels(ctx, oracle, view, kernel, specs):
    torch = pytest.importorskip("torch")
    displayed, want = _displayed_case(oracle, A_H, A_W)
    views = [_device_view(torch, p, spec) for p, spec in zip(_stored(displayed, 2, "nv12"), specs)]
    got = ctx.preprocess_picture(tuple(views), 2)
    _check_plan(ctx, A_H, A_W, kernel, A_ROWS, 2)
    _check_outputs(ctx, got, want, view)
    ctx.preprocess_nv12(*views)
    _check_plan(ctx, A_H, A_W, kernel, A_ROWS, 0)


# ---- 4: the whole clip ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole_clip():
    """stored 96 x 160, 5 frames, NV12"""
    return synth.bgr_to_nv12(synth.make_clip(5, 96, 160, seed=83, dup_every=3))


@pytest.mark.parametrize("k", [1, 2, 3])
def test_analyze_pictures_equals_the_call_on_the_turned_planes(ctx, whole_clip, k):
    torch = pytest.importorskip("torch")
    y, uv = whole_clip
    turned = synth.rotate_planes((y, uv), k)
    planar = synth.nv12_to_i420(y, uv)
    try:
        for mode in (1, 0):                                                    # the default (fast) mode, then the exact kernels
            ctx.set_option("fb_mode", mode)
            want = ctx.analyze_frames_nv12(*turned).tobytes()
            assert ctx.analyze_pictures([(y, uv)], [k])[0].tobytes() == want, (k, mode, "host nv12")
            assert ctx.analyze_frames_nv12(y, uv, rotate=k).tobytes() == want
            assert ctx.analyze_frames_i420(*planar, rotate=k).tobytes() == want, (k, mode, "host i420")
            dev = tuple(torch.from_numpy(p).to("cuda:0") for p in (y, uv))
            assert ctx.analyze_pictures([dev], [k])[0].tobytes() == want, (k, mode, "device nv12")
            assert ctx.ingest_rotate() == k
            dev3 = tuple(torch.from_numpy(p).to("cuda:0") for p in planar)
            assert ctx.analyze_pictures([dev3], [k])[0].tobytes() == want, (k, mode, "device i420")
            # the async twin
            rec = np.zeros(5, avd_hip.RECORD_DTYPE)
            keep = ctx.analyze_pictures_async([dev], rec, [k])
            ctx.synchronize()
            del keep
            assert rec.tobytes() == want, (k, mode, "async")
            rec = np.zeros(5, avd_hip.RECORD_DTYPE)
            keep = ctx.analyze_frames_i420_async(*planar, rec, rotate=k)
            ctx.synchronize()
            del keep
            assert rec.tobytes() == want, (k, mode, "async i420")
    finally:
        ctx.set_option("fb_mode", 1)


def test_exact_mode_equals_the_oracle_on_the_turned_bgr_frames(ctx, oracle, whole_clip):
    """The anchor outside the library: the records of the turned BGR frames (what cv2 hands the reference), exact mode, bit for bit."""
    from tests.test_host_and_abi import _records_from_oracle
    y, uv = whole_clip
    bgr = np.ascontiguousarray(np.rot90(oracle.nv12_to_bgr(y, uv), -1, axes=(1, 2)))
    try:
        ctx.set_option("fb_mode", 0)
        rec = ctx.analyze_pictures([(y, uv)], [1])[0]
    finally:
        ctx.set_option("fb_mode", 1)
    assert np.array_equal(rec, _records_from_oracle(oracle, bgr))


def test_a_call_made_while_a_picture_analysis_is_pending():
    """avd_analyze_pictures_async obeys the rule of the other entries (tests/test_gpu_pending_call.py): any other call on the context first
    completes it.  The pending clip has flagged pairs in its last Farneback chunk, so the exact re-run is pending when the other call
    arrives; its records equal the same input analysed alone by a blocking call on a fresh context."""
    from tests.content_families import flagged_mix
    gray = flagged_mix(23, 3)                                              # 24 frames, 320 x 320
    stored = synth.rotate_planes(synth.bgr_to_nv12(np.ascontiguousarray(np.repeat(gray[..., None], 3, axis=3))), 3)   # displayed after k = 1
    other = synth.nv12_to_i420(*synth.bgr_to_nv12(synth.make_clip(24, 240, 320, seed=13, dup_every=0)))
    with avd_hip.Context(0) as c:
        want = c.analyze_pictures([stored], [1])[0].copy()
        want_rerun = c.get_option("rerun_pairs")
    with avd_hip.Context(0) as c:
        want_other = c.preprocess_picture(other, 3)
    assert int(np.count_nonzero(want["reserved"][1:])) >= 3
    with avd_hip.Context(0) as c:
        rec = np.zeros(24, avd_hip.RECORD_DTYPE)
        keep = c.analyze_pictures_async([stored], rec, [1])
        got_other = c.preprocess_picture(other, 3)                         # drains the pending call first: its records are there already
        assert rec.tobytes() == want.tobytes()
        c.synchronize()
        del keep
        assert c.get_option("rerun_pairs") == want_rerun
        # and the other way round: a picture call drains a pending NV12 one
        y0, uv0 = synth.rotate_planes(stored, 1)
        rec_nv = np.zeros(24, avd_hip.RECORD_DTYPE)
        keep = c.analyze_frames_nv12_async(y0, uv0, rec_nv)
        again = c.analyze_pictures([stored], [1])[0]
        assert rec_nv.tobytes() == want.tobytes()
        c.synchronize()
        del keep
    assert again.tobytes() == want.tobytes()
    for a, b in zip(got_other, want_other):
        assert np.array_equal(a, b)


# ---- 5: a batch ---------------------------------------------------------------------------------------------------------------------------------
def test_a_batch_of_every_format_and_rotation(ctx):
    """One call: a BGR clip, an NV12 clip turned once, an I420 clip as stored (the case avd_clip cannot express) and an I420 clip turned
    three times -- displayed geometries 64 x 96, 112 x 80, 48 x 64 and 72 x 40 -- equals the per-clip calls, byte for byte."""
    bgr = synth.make_clip(3, 64, 96, seed=31, dup_every=2)
    nv = synth.bgr_to_nv12(synth.make_clip(4, 80, 112, seed=32, dup_every=0))             # displayed 112 x 80
    p0 = synth.nv12_to_i420(*synth.bgr_to_nv12(synth.make_clip(2, 48, 64, seed=33)))
    p3 = synth.nv12_to_i420(*synth.bgr_to_nv12(synth.make_clip(5, 40, 72, seed=34, dup_every=3)))   # displayed 72 x 40
    clips, turns = [bgr, nv, p0, p3], [0, 1, 0, 3]
    single = [ctx.analyze_pictures([c], [k])[0] for c, k in zip(clips, turns)]
    assert single[1].tobytes() == ctx.analyze_frames_nv12(*synth.rotate_planes(nv, 1)).tobytes()
    assert single[2].tobytes() == ctx.analyze_frames_i420(*p0).tobytes()
    assert single[3].tobytes() == ctx.analyze_frames_i420(*synth.rotate_planes(p3, 3)).tobytes()
    assert single[0].tobytes() == ctx.analyze_frames(bgr).tobytes()
    got = ctx.analyze_pictures(clips, turns)
    assert [len(r) for r in got] == [3, 4, 2, 5]
    assert np.concatenate(got).tobytes() == np.concatenate(single).tobytes()
    assert ctx.stage_bytes() == bgr.nbytes + sum(p.nbytes for p in nv + p0 + p3)          # the STORED planes
    _check_plan(ctx, 72, 40, I420_STRIP, 14, 3)                                           # the last clip's launch
    rec = np.zeros(14, avd_hip.RECORD_DTYPE)
    keep, counts = ctx.analyze_pictures_async(clips, rec, turns)
    ctx.synchronize()
    del keep
    assert counts == [3, 4, 2, 5] and rec.tobytes() == np.concatenate(single).tobytes()


# ---- 6: refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    y, uv = _planes(2, 64, 64, seed=5)
    _, u, v = synth.nv12_to_i420(y, uv)
    bgr = synth.random_frames(2, 64, 64, seed=6)
    ctx.preprocess_picture((y, uv), 2)                                      # the call before
    before = ctx.debug_fetch("ingest_plan", (8,), np.int32)
    assert ctx.ingest_rotate() == 2
    L, H = ctx._L, ctx._h

    def call(clip, rotate=0, edit=None):
        p, n, keep = ctx._picture(clip, 0)
        p.rotate = rotate
        if edit:
            edit(p)
        rec = np.zeros(2, avd_hip.RECORD_DTYPE)
        small = np.empty((2, 320, 320), np.uint8)
        rcs = (L.avd_analyze_pictures(H, ctypes.byref(p), 1, rec.ctypes.data), L.avd_analyze_pictures_async(H, ctypes.byref(p), 1, rec.ctypes.data),
               L.avd_preprocess_picture(H, ctypes.byref(p), small.ctypes.data, None, None, None))
        assert rcs[0] == rcs[1] == rcs[2], rcs
        return rcs[0], L.avd_last_error(H).decode()

    def stored_size(h, w):
        def edit(p):
            p.h, p.w = h, w
        return edit

    assert call((y, u, v), 1)[0] == 0 and ctx.ingest_rotate() == 1          # the descriptor itself is fine
    ctx.preprocess_picture((y, uv), 2)
    rc, msg = call(bgr, 1)
    assert rc == -4 and "BGR" in msg, (rc, msg)                             # AVD_ERR_UNSUPPORTED
    for clip in ((y, uv), (y, u, v)):
        rc, msg = call(clip, 4)
        assert rc == -1 and "rotate" in msg, (rc, msg)                      # AVD_ERR_ARG
        rc, msg = call(clip, -1)
        assert rc == -1 and "rotate" in msg, (rc, msg)
        rc, msg = call(clip, 1, stored_size(64, 63))                        # an odd stored width
        assert rc == -4 and "even width and height" in msg, (rc, msg)
        rc, msg = call(clip, 1, stored_size(64, 30))                        # displayed 30 x 64: a displayed side below 32
        assert rc == -4 and "smaller than 32x32" in msg, (rc, msg)
        rc, msg = call(clip, 3, stored_size(30, 64))
        assert rc == -4 and "smaller than 32x32" in msg, (rc, msg)
        rc, msg = call(clip, 1, lambda p: setattr(p, "struct_size", p.struct_size - 8))
        assert rc == -1 and "struct_size" in msg, (rc, msg)
        rc, msg = call(clip, 1, lambda p: setattr(p, "struct_size", p.struct_size + 8))
        assert rc == -1 and "struct_size" in msg, (rc, msg)
        rc, msg = call(clip, 1, lambda p: setattr(p, "reserved", 1))
        assert rc == -1 and "reserved" in msg, (rc, msg)
        rc, msg = call(clip, 1, lambda p: setattr(p, "format", 3))
        assert rc == -1 and "format" in msg, (rc, msg)

    def unequal(p):
        p.row_stride[2] = p.row_stride[1] + 8
    rc, msg = call((y, u, v), 1, unequal)
    assert rc == -1 and "share their strides" in msg, (rc, msg)
    # nothing was launched by any of them
    assert np.array_equal(ctx.debug_fetch("ingest_plan", (8,), np.int32), before) and ctx.ingest_rotate() == 2


# ---- 7: the drop-in -----------------------------------------------------------------------------------------------------------------------------
def test_a_turned_y4m_through_the_drop_in(oracle, tmp_path, monkeypatch):
    """A .y4m with XAVD_ROTATE=90 and empty meta: the summary carries the displayed size, and the whole result equals analyze() on a .npy of
    the turned BGR frames (what cv2.VideoCapture hands the reference), across streaming chunk boundaries."""
    from app.analyzers import video
    from avd_hip import sources
    n, h, w = 10, 96, 128
    y, uv = synth.bgr_to_nv12(synth.make_clip(n, h, w, seed=25, dup_every=4))
    path = str(tmp_path / "portrait.y4m")
    sources.write_y4m(path, y, uv, fps=(4, 1), rotate=90)                  # 4 fps: step 2 -> 5 sampled frames
    monkeypatch.setenv("AVD_CHUNK_FRAMES", "2")                            # chunks of 2 + carry: 2, 2, 1
    monkeypatch.delenv("AVD_Y4M_SURFACE", raising=False)
    got = video.analyze(path, {})
    assert (got["summary"]["w"], got["summary"]["h"]) == (h, w) == (96, 128)       # displayed: 96 wide, 128 high
    assert len(got["timeline"]) == 2 and got["timeline"] is got["timeline_ai"]
    npy = str(tmp_path / "portrait.npy")
    np.save(npy, np.ascontiguousarray(np.rot90(oracle.nv12_to_bgr(y, uv), -1, axes=(1, 2))))
    want = video.analyze(npy, {"fps": 4.0, "duration": n / 4.0})           # what the .y4m header says; size from the frames
    assert got == want
    monkeypatch.setenv("AVD_Y4M_SURFACE", "i420")
    assert video.analyze(path, {}) == want
