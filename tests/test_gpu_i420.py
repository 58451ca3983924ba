"""Planar 4:2:0 (I420) ingest: k_preprocess with the I420 fill policy and the avd_*_i420 entry points (include/avd.h).

The arithmetic is the NV12 kernels' -- swscale's tables, nearest chroma, cv2's gray -- so every result is compared BIT FOR BIT: with the
CPU oracle (NV12 -> BGR, then the BGR oracle) on the interleaved form of the same planes, and with the NV12 entry points.  There is no
tolerance in this file.  U and V are independent random bytes (tests.test_nv12._planes de-interleaved), so a swapped or shared chroma
plane cannot pass.

Every kernel case reads the "ingest_plan" debug buffer and asserts the kernel and the rows per band it was written for (literals taken
from the band plan as avd_preprocess.hip documents it, and from the NV12 sweep of tests/test_gpu_ingest_plan.py), so a case that
silently took the other fill fails.  What is new against NV12: two 8-byte chroma loads per 16-pixel chunk (planes aligned to 8, not 16),
a third plane pointer, and host staging that copies overlapping plane spans once ("stage_bytes")."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import avd_hip  # noqa: E402
from avd_hip import AvdError, synth  # noqa: E402
from tests.ingest_gpu_kit import check_outputs as _check_outputs  # noqa: E402
from tests.ingest_gpu_kit import check_plan as _check_plan  # noqa: E402
from tests.ingest_gpu_kit import heights_even as _heights  # noqa: E402
from tests.ingest_gpu_kit import reference  # noqa: E402
from tests.test_nv12 import _planes  # noqa: E402

KERNEL_NAMES = ("bgr_scalar", "bgr_vec16", "bgr_staged", "nv12_scalar", "nv12_tables", "i420_scalar", "i420_tables")
I420_SCALAR, I420_TABLES = 5, 6


def _reference(oracle, y, uv):
    """the oracle on swscale's BGR of the NV12 form"""
    return reference(oracle, oracle.nv12_to_bgr(y, uv))


def _cases(kernel, widths_rows):
    return [pytest.param(kernel, w, r, h, id=f"{KERNEL_NAMES[kernel]}-w{w}-r{r}-h{h}") for w, r in widths_rows for h in _heights(r)]


# ---- 1, 2: the two fills over the plan classes, contiguous host planes --------------------------------------------------------------
# Table fill: odd row counts make a band start on an odd row, so the chroma row it shares with the row above is split across two
# workgroups; 16384 asks for more than 48 KiB of dynamic LDS.  Scalar fill: widths that are not a multiple of 16.
TABLE_PLANS = [(48, 14), (2064, 7), (4112, 9), (6128, 5), (12272, 1), (16384, 1)]
SCALAR_PLANS = [(34, 14), (1922, 14), (8190, 3), (12274, 1)]


@pytest.mark.parametrize("kernel,w,rows,h", _cases(I420_TABLES, TABLE_PLANS) + _cases(I420_SCALAR, SCALAR_PLANS))
def test_i420_plan_classes(ctx, oracle, kernel, w, rows, h):
    y, uv = _planes(2, h, w, seed=h + w)
    got = ctx.preprocess_i420(*synth.nv12_to_i420(y, uv))
    lds = 57696 if (kernel, w) == (I420_TABLES, 16384) else None          # 3 * 16416 + 3 * 4 * 704, as NV12
    _check_plan(ctx, h, w, kernel, rows, lds=lds)
    _check_outputs(ctx, got, _reference(oracle, y, uv), (h, w))
    assert ctx.stage_bytes() == y.nbytes + uv.nbytes                      # three separately allocated planes: three spans


# ---- 3: alignment dispatch on device views ------------------------------------------------------------------------------------------
# The table fill needs w % 16 == 0, the Y plane (base, row stride, frame stride) on multiples of 16 and the U and V planes on multiples
# of 8 -- not 16: a contiguous frame has its V plane at 5wh/4.  view -> (base offset, row padding, odd frame stride) of Y, U, V; a chroma
# row of the image is 1032 bytes (8 mod 16).
A_N, A_H, A_W, A_ROWS = 2, 46, 2064, 7
VIEWS = {
    "aligned16_padded": (I420_TABLES, (32, 16, False), (48, 8, False), (16, 8, False)),       # chroma row stride 1040
    "chroma_8mod16": (I420_TABLES, (0, 16, False), (8, 16, False), (24, 16, False)),         # U, V bases at 8 mod 16, row stride 1048
    "u_base+4": (I420_SCALAR, (0, 16, False), (4, 8, False), (0, 8, False)),
    "v_base+4": (I420_SCALAR, (0, 16, False), (0, 8, False), (4, 8, False)),
    "chroma_row_stride%8=4": (I420_SCALAR, (0, 16, False), (0, 4, False), (0, 4, False)),   # 1036
    "y_base+3": (I420_SCALAR, (3, 16, False), (0, 8, False), (0, 8, False)),
    "y_row_stride%16=8": (I420_SCALAR, (0, 8, False), (0, 8, False), (0, 8, False)),
    "y_frame_stride_odd": (I420_SCALAR, (0, 16, True), (0, 8, False), (0, 8, False)),
}


def _device_view(torch, host, plane_spec):
    """host uint8[n, rows, row_bytes] -> a device view with the same values: base pointer = a 16-byte boundary + offset, row stride = row
    bytes + pad, frame stride = the next multiple of 16 that holds the rows (+ 1 if odd is asked for)."""
    offset, pad, odd = plane_spec
    n, rows, row_bytes = host.shape
    rs = row_bytes + pad
    fs = (rs * rows + 15) // 16 * 16 + (1 if odd else 0)
    flat = torch.empty(16 + offset + n * fs + 16, dtype=torch.uint8, device="cuda:0")
    offset += -flat.data_ptr() % 16
    # laid out on the host and uploaded as one flat copy: no strided copy kernel of torch's is needed
    staged = np.zeros(flat.numel(), np.uint8)
    np.lib.stride_tricks.as_strided(staged[offset:], host.shape, (fs, rs, 1))[...] = host
    flat.copy_(torch.from_numpy(staged))
    view = flat.as_strided(tuple(host.shape), (fs, rs, 1), offset)
    assert (view.data_ptr() - plane_spec[0]) % 16 == 0 and view.stride(1) == rs and view.stride(0) % 16 == (1 if odd else 0)
    return view


@pytest.fixture(scope="module")
def align_input(oracle):
    """The image and its oracle results, formed once and left unchanged."""
    y, uv = _planes(A_N, A_H, A_W, seed=A_H + A_W)
    return synth.nv12_to_i420(y, uv), _reference(oracle, y, uv)


@pytest.mark.parametrize("view", list(VIEWS))
def test_alignment_dispatch(ctx, align_input, view):
    """Every view equals the oracle (so they equal each other); 8-byte aligned chroma planes still run the table fill."""
    torch = pytest.importorskip("torch")
    planes, want = align_input
    kernel, *specs = VIEWS[view]
    views = [_device_view(torch, p, spec) for p, spec in zip(planes, specs)]
    if view == "chroma_8mod16":
        assert views[1].data_ptr() % 16 == 8 and views[2].data_ptr() % 16 == 8 and views[1].stride(1) % 16 == 8
    got = ctx.preprocess_i420(*views)
    _check_plan(ctx, A_H, A_W, kernel, A_ROWS)
    _check_outputs(ctx, got, want, view)
    assert ctx.stage_bytes() == 0


# ---- 4: one contiguous buffer per clip (a y4m map, a rawvideo pipe) ------------------------------------------------------------------
C_N, C_H, C_W = 3, 34, 48
C_Y, C_C = C_H * C_W, (C_H // 2) * (C_W // 2)                              # 1632, 408: a frame is Y | U | V = 2448 bytes


def _one_buffer(planes, gap):
    """-> (flat uint8 buffer, offset of frame 0, frame stride): every frame Y | U | V behind a `gap`-byte marker"""
    y, u, v = planes
    fs = gap + C_Y + 2 * C_C
    flat = np.zeros(C_N * fs, np.uint8)
    for f in range(C_N):
        o = f * fs + gap
        flat[o:o + C_Y] = y[f].ravel()
        flat[o + C_Y:o + C_Y + C_C] = u[f].ravel()
        flat[o + C_Y + C_C:o + fs - gap] = v[f].ravel()
    return flat, gap, fs


def _views_of(flat, off, fs, strided):
    """the three planes as strided views of one flat buffer (numpy array or torch tensor)"""
    return (strided(flat, (C_N, C_H, C_W), (fs, C_W, 1), off), strided(flat, (C_N, C_H // 2, C_W // 2), (fs, C_W // 2, 1), off + C_Y),
            strided(flat, (C_N, C_H // 2, C_W // 2), (fs, C_W // 2, 1), off + C_Y + C_C))


@pytest.fixture(scope="module")
def clip_input(oracle):
    y, uv = _planes(C_N, C_H, C_W, seed=C_H + C_W + 1)
    return synth.nv12_to_i420(y, uv), _reference(oracle, y, uv)


@pytest.mark.parametrize("gap,kernel", [(6, I420_SCALAR), (0, I420_TABLES)], ids=["frame_marker_gap", "no_gap"])
def test_one_contiguous_buffer_per_clip(ctx, clip_input, gap, kernel):
    """With the 6-byte marker the frame stride is 2454, no multiple of 8: scalar.  Without it 2448: tables, the V plane at offset 2040 (8 mod
    16).  On the host the three plane spans overlap almost entirely and are staged as ONE span, from y to the end of the last V plane."""
    torch = pytest.importorskip("torch")
    planes, want = clip_input
    flat, off, fs = _one_buffer(planes, gap)
    assert fs == (2454 if gap else 2448) and (off + C_Y + C_C - gap) == 2040
    np_strided = lambda a, shape, strides, o: np.lib.stride_tricks.as_strided(a[o:], shape, strides)
    host = _views_of(flat, off, fs, np_strided)
    assert all(np.array_equal(a, b) for a, b in zip(host, planes))
    got = ctx.preprocess_i420(*host)
    _check_plan(ctx, C_H, C_W, kernel, 14)
    _check_outputs(ctx, got, want, ("host", gap))
    one_span = (C_N - 1) * fs + C_Y + 2 * C_C                             # y of frame 0 .. end of V of the last frame
    assert ctx.stage_bytes() == one_span == flat.size - gap
    # the same buffer resident on the device: used in place, nothing is staged
    dflat = torch.from_numpy(flat).to("cuda:0")
    assert dflat.data_ptr() % 16 == 0
    dev = _views_of(dflat, off, fs, lambda t, shape, strides, o: t.as_strided(shape, strides, o))
    got = ctx.preprocess_i420(*dev)
    _check_plan(ctx, C_H, C_W, kernel, 14)
    _check_outputs(ctx, got, want, ("device", gap))
    assert ctx.stage_bytes() == 0


def test_stage_bytes_of_separate_planes_and_of_the_other_surfaces(ctx, clip_input):
    planes, want = clip_input
    with avd_hip.Context(0) as fresh:
        with pytest.raises(AvdError, match="stage_bytes"):
            fresh.stage_bytes()                                           # no ingest call yet
        got = fresh.preprocess_i420(*planes)                              # three separately allocated planes: three spans
        assert fresh.stage_bytes() == sum(p.nbytes for p in planes) == C_N * (C_Y + 2 * C_C)
        _check_plan(fresh, C_H, C_W, I420_TABLES, 14)                     # each span starts on a 256-byte boundary of the staging buffer
        _check_outputs(fresh, got, want, "separate")
        # YV12 order in one buffer (V before U): still one span
        y, u, v = planes
        flat = np.concatenate([y.ravel(), v.ravel(), u.ravel()])
        yy = flat[:y.size].reshape(y.shape)
        vv = flat[y.size:y.size + v.size].reshape(v.shape)
        uu = flat[y.size + v.size:].reshape(u.shape)
        got = fresh.preprocess_i420(yy, uu, vv)
        assert fresh.stage_bytes() == flat.size
        _check_outputs(fresh, got, want, "yv12 order")
    y, uv = synth.i420_to_nv12(*planes)
    ctx.preprocess_nv12(y, uv)
    assert ctx.stage_bytes() == y.nbytes + uv.nbytes
    bgr = synth.random_frames(2, 40, 48, seed=3)
    ctx.analyze_frames(bgr)
    assert ctx.stage_bytes() == bgr.nbytes


# ---- 5: the whole path -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole_clip():
    clip = synth.make_clip(6, 360, 640, seed=71, dup_every=3)
    y, uv = synth.bgr_to_nv12(clip)
    return (y, uv), synth.nv12_to_i420(y, uv)


def test_analyze_i420_equals_nv12_and_the_oracle(ctx, oracle, whole_clip):
    from tests.test_host_and_abi import _records_from_oracle
    (y, uv), (_, u, v) = whole_clip
    rec = ctx.analyze_frames_i420(y, u, v)
    assert rec.tobytes() == ctx.analyze_frames_nv12(y, uv).tobytes()
    assert np.array_equal(rec, _records_from_oracle(oracle, oracle.nv12_to_bgr(y, uv)))
    # strided planes: a decoder's pitch larger than the width, and a frame gap
    yp, up, vp = np.zeros((6, 368, 704), np.uint8), np.zeros((6, 190, 352), np.uint8), np.zeros((6, 190, 352), np.uint8)
    yp[:, :360, :640], up[:, :180, :320], vp[:, :180, :320] = y, u, v
    assert np.array_equal(ctx.analyze_frames_i420(yp[:, :360, :640], up[:, :180, :320], vp[:, :180, :320]), rec)
    # YV12 is the same call with the chroma pointers exchanged: it equals NV12 with the chroma bytes exchanged
    _, vu = synth.i420_to_nv12(y, v, u)
    assert not np.array_equal(u, v)
    assert ctx.analyze_frames_i420(y, v, u).tobytes() == ctx.analyze_frames_nv12(y, vu).tobytes()


def test_i420_device_planes_and_async(ctx, whole_clip):
    torch = pytest.importorskip("torch")
    (y, uv), planes = whole_clip
    want = ctx.analyze_frames_nv12(y, uv)
    dev = [torch.from_numpy(p).to("cuda:0") for p in planes]
    assert np.array_equal(ctx.analyze_frames_i420(*dev), want)
    rec = np.zeros(len(y), want.dtype)
    keep = ctx.analyze_frames_i420_async(*dev, rec)
    ctx.synchronize()
    del keep
    assert rec.tobytes() == want.tobytes()


def test_a_call_made_while_an_i420_analysis_is_pending():
    """The async form obeys the rule of the other entries: any other call on the context first completes it.  As in
    tests/test_gpu_pending_call.py the pending clip has flagged pairs in its last Farneback chunk, so the exact re-run is pending when the
    other call arrives; its records equal the same input analysed alone by a blocking call on a fresh context."""
    from tests.content_families import flagged_mix
    gray = flagged_mix(23, 3)                                              # 24 frames, 320 x 320
    planes = synth.nv12_to_i420(*synth.bgr_to_nv12(np.ascontiguousarray(np.repeat(gray[..., None], 3, axis=3))))
    other = synth.nv12_to_i420(*synth.bgr_to_nv12(synth.make_clip(24, 240, 320, seed=13, dup_every=0)))
    with avd_hip.Context(0) as c:
        want = c.analyze_frames_i420(*planes).copy()
        want_rerun = c.get_option("rerun_pairs")
    with avd_hip.Context(0) as c:
        want_other = c.preprocess_i420(*other)
    assert int(np.count_nonzero(want["reserved"][1:])) >= 3
    with avd_hip.Context(0) as c:
        rec = np.zeros(24, avd_hip.RECORD_DTYPE)
        keep = c.analyze_frames_i420_async(*planes, rec)
        got_other = c.preprocess_i420(*other)                              # drains the pending call first: its records are there already
        assert rec.tobytes() == want.tobytes()
        c.synchronize()
        del keep
        assert c.get_option("rerun_pairs") == want_rerun
        # and the other way round: an I420 call drains a pending BGR one
        bgr = np.ascontiguousarray(np.repeat(gray[..., None], 3, axis=3))
        rec_bgr = np.zeros(24, avd_hip.RECORD_DTYPE)
        keep = c.analyze_frames_async(bgr, rec_bgr)
        again = c.analyze_frames_i420(*planes)
        assert rec_bgr["ham"][0] == -1 and int(np.count_nonzero(rec_bgr["reserved"][1:])) >= 3
        c.synchronize()
        del keep
    assert rec.tobytes() == want.tobytes() and again.tobytes() == want.tobytes()
    for a, b in zip(got_other, want_other):
        assert np.array_equal(a, b)


def test_i420_argument_checks(ctx):
    z = lambda *shape: np.zeros(shape, np.uint8)
    for h, w in ((66, 64), (64, 66)):                                      # sizes the binding accepts ...
        ctx.preprocess_i420(z(1, h, w), z(1, h // 2, w // 2), z(1, h // 2, w // 2))
    L, H = ctx._L, ctx._h
    y, c = z(2, 65, 66), z(2, 33, 33)

    def call(h, w, yp=y.ctypes.data, up=c.ctypes.data, vp=c.ctypes.data, c_row=None):
        rec = np.zeros(2, avd_hip.RECORD_DTYPE)
        cr = w // 2 if c_row is None else c_row
        rc = L.avd_analyze_frames_i420(H, yp, up, vp, 0, 2, h, w, w, cr, h * w, (h // 2) * cr, rec.ctypes.data)
        return rc, L.avd_last_error(H).decode()
    assert call(64, 64)[0] == 0
    for h, w in ((65, 64), (64, 65)):                                      # odd height, odd width
        rc, msg = call(h, w)
        assert rc == -4 and "I420 needs even width and height" in msg, (h, w, rc, msg)
    rc, msg = call(30, 48)
    assert rc == -4 and "smaller than 32x32" in msg, (rc, msg)
    rc, msg = call(64, 64, vp=None)
    assert rc == -1 and "null I420 plane" in msg, (rc, msg)
    rc, msg = call(64, 64, c_row=31)                                       # chroma rows shorter than w / 2
    assert rc == -1 and "I420 planes" in msg, (rc, msg)
    rc, msg = call(64, 16386)
    assert rc == -1, (rc, msg)
    small = np.empty((2, 320, 320), np.uint8)
    rc = L.avd_preprocess_i420(H, y.ctypes.data, None, c.ctypes.data, 0, 2, 64, 64, 64, 32, 64 * 64, 32 * 32, small.ctypes.data, None, None, None)
    assert rc == -1 and "null I420 plane" in L.avd_last_error(H).decode()


# ---- 6: the drop-in ------------------------------------------------------------------------------------------------------------------------
def test_y4m_through_the_drop_in_both_ways(ctx, oracle, tmp_path, monkeypatch):
    """video.analyze on a .y4m with AVD_Y4M_SURFACE=i420 (the file's planes, views of the map) and without (the host interleave, NV12):
    equal result dicts, equal to the oracle's, across streaming chunk boundaries with their one-frame carry."""
    from app.analyzers import video
    from avd_hip import analyzer, sources
    n, h, w = 40, 96, 128
    y, uv = synth.bgr_to_nv12(synth.make_clip(n, h, w, seed=21, dup_every=4))
    path = str(tmp_path / "clip.y4m")
    sources.write_y4m(path, y, uv, fps=(8, 1))                             # 8 fps: step 4 -> 10 sampled frames
    monkeypatch.setenv("AVD_CHUNK_FRAMES", "4")                            # chunks of 4 + carry: 4, 4, 2
    meta = {"width": 0, "height": 0, "fps": 0.0, "duration": 0.0}
    monkeypatch.delenv("AVD_Y4M_SURFACE", raising=False)
    as_nv12 = video.analyze(path, meta)
    monkeypatch.setenv("AVD_Y4M_SURFACE", "i420")
    taken = []
    real = analyzer.FrameAnalyzer.records_stream_i420
    monkeypatch.setattr(analyzer.FrameAnalyzer, "records_stream_i420", lambda self, s: taken.append(1) or real(self, s))
    as_i420 = video.analyze(path, meta)
    assert taken == [1]                                                    # the planar route was the one that ran
    assert as_i420 == as_nv12 and as_i420["timeline"] is as_i420["timeline_ai"]
    want = oracle.analyze_sampled_frames(oracle.nv12_to_bgr(y[::4], uv[::4]), {"fps": 8.0, "width": w, "height": h, "duration": n / 8.0})
    assert as_i420["timeline"] == want["timeline"] and as_i420["summary"] == want["summary"]
    # FrameAnalyzer directly: 10 frames in chunks of 4 equal one call, and the NV12 streamer
    fa = analyzer.FrameAnalyzer(chunk=4, ctx=ctx)
    src = sources.Y4mSource(path, planar=True)
    rec = fa.records_stream_i420(src.sampled(4))
    src.close()
    assert len(rec) == 10
    assert rec.tobytes() == ctx.analyze_frames_i420(*synth.nv12_to_i420(y[::4], uv[::4])).tobytes()
    assert rec.tobytes() == fa.records_stream_nv12(zip(y[::4], uv[::4])).tobytes()
    assert fa.records_stream_i420(iter(())).size == 0
