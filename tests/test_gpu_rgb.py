"""RGB producers' layouts in the fused ingest: AVD_FMT_RGB24, AVD_FMT_BGRA32, AVD_FMT_RGBA32 and AVD_FMT_RGBP (include/avd.h).

Definition under test: if B is the BGR24 arrangement of the same pixels (alpha dropped), every output equals the BGR entry point's on B --
which is the oracle's preprocess_bgr(B).  Everything is compared BIT FOR BIT; there is no tolerance in this file.

Every case names the kernel and the rows per band it was written for and reads both back from the "ingest_plan" debug buffer, and the layout
from "ingest_format", so a case that silently took another fill fails instead of passing.  The expected kernels and row counts are literals:
AVD_FMT_RGB24 runs BGR's plan under BGR's ids (the staged kernel with NI = 3 / 4 / 6 / 8 / 9 row chunks per lane for w <= 672 / 1024 / 1360 /
2048 / 4096, 7-row bands above 2048, the 16-byte fill above 4096, the scalar fill otherwise); the 32-bit layouts and AVD_FMT_RGBP run the
generic kernel with a 16-byte fill (ids 10 and 12) or a scalar fill (9 and 11) on the band plan of the width: 14 rows up to 2048 px, 7 rows
up to 4096, then 9 at 4112; 13 rows at 3041.  AVD_FMT_RGBP also has a staged kernel (id 13) with BGR's NI classes up to NI = 8, that is up to
2048 px; from 2064 px on it runs its 16-byte fill."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import avd_hip  # noqa: E402
from avd_hip import _lib, synth  # noqa: E402
from avd_hip import Pixels  # noqa: E402
from tests.ingest_gpu_kit import P_KERNEL, check_outputs, check_plan, reference  # noqa: E402
from tests.ingest_gpu_kit import heights as _heights  # noqa: E402
from tests.ingest_gpu_kit import raw_picture_at as _raw_picture  # noqa: E402
from tests.ingest_gpu_kit import same_records as _same_records  # noqa: E402

BGR, NV12, I420, RGB24, BGRA32, RGBA32, RGBP, FULL = 0, 1, 2, 0x10, 0x11, 0x12, 0x13, 0x100
NEW = (RGB24, BGRA32, RGBA32, RGBP)
NAMES = {BGR: "bgr24", RGB24: "rgb24", BGRA32: "bgra32", RGBA32: "rgba32", RGBP: "rgbp"}
# enum IngestKernel (avd_internal.h) and the layout of "ingest_plan" (include/avd.h)
BGR_SCALAR, BGR_VEC16, BGR_STAGED = 0, 1, 2
PX32_SCALAR, PX32_VEC16, RGBP_SCALAR, RGBP_VEC16, RGBP_STAGED = 9, 10, 11, 12, 13
SCALAR = {RGB24: BGR_SCALAR, BGRA32: PX32_SCALAR, RGBA32: PX32_SCALAR, RGBP: RGBP_SCALAR}
VEC16 = {RGB24: BGR_VEC16, BGRA32: PX32_VEC16, RGBA32: PX32_VEC16, RGBP: RGBP_VEC16}
# (kernel, NI) of an aligned clip up to 672 px wide
ALIGNED = {RGB24: (BGR_STAGED, 3), BGRA32: (PX32_VEC16, 0), RGBA32: (PX32_VEC16, 0), RGBP: (RGBP_STAGED, 3)}


def _check_plan(ctx, fmt, h, w, kernel, rows, ni=0):
    check_plan(ctx, h, w, kernel, rows, ni, fmt=fmt, rotate=0, full_range=False)


def _check_outputs(ctx, oracle, got, ref_bgr, tag):
    """got = (small320, hash, lap_sum, lap_sumsq) of the call that just ran on ctx; ref_bgr = B, the frames the oracle sees."""
    check_outputs(ctx, got, reference(oracle, ref_bgr), tag)


def arrange(bgr, fmt, alpha=None):
    """BGR frames uint8[N,H,W,3] -> the same pixels in layout fmt.  alpha: None = random bytes, or the value of every fourth byte."""
    if fmt == BGR:
        return bgr
    if fmt == RGB24:
        return np.ascontiguousarray(bgr[..., ::-1])
    if fmt == RGBP:
        return np.ascontiguousarray(bgr[..., ::-1].transpose(0, 3, 1, 2))
    a = (np.random.default_rng(bgr.shape[1] * 31 + bgr.shape[2]).integers(0, 256, bgr.shape[:3] + (1,), dtype=np.uint8) if alpha is None
         else np.full(bgr.shape[:3] + (1,), alpha, np.uint8))
    return np.concatenate([bgr if fmt == BGRA32 else bgr[..., ::-1], a], axis=-1)


# ---- RGB24: BGR's plan, BGR's kernels, the other coefficient constants ---------------------------------------------------------------------
# kernel, NI, widths, rows per band: both sides of every NI boundary
RGB24_PLANS = [
    (BGR_STAGED, 3, (32, 48, 256, 272, 672), 14),
    (BGR_STAGED, 4, (688, 1024), 14),
    (BGR_STAGED, 6, (1040, 1360), 14),
    (BGR_STAGED, 8, (1376, 2048), 14),
    (BGR_STAGED, 9, (2064, 4096), 7),
    (BGR_VEC16, 0, (4112,), 9),
    (BGR_SCALAR, 0, (33,), 14),
    (BGR_SCALAR, 0, (3041,), 13),
]
# RGBP: BGR's staged classes up to NI = 8, then its own 16-byte fill on the generic plan
RGBP_PLANS = [
    (RGBP_STAGED, 3, (32, 48, 256, 272, 672), 14),
    (RGBP_STAGED, 4, (688, 1024), 14),
    (RGBP_STAGED, 6, (1040, 1360), 14),
    (RGBP_STAGED, 8, (1376, 2048), 14),
    (RGBP_VEC16, 0, (2064, 4096), 7),
    (RGBP_VEC16, 0, (4112,), 9),
    (RGBP_SCALAR, 0, (35,), 14),
    (RGBP_SCALAR, 0, (3041,), 13),
]
# the generic kernel's plan (the 32-bit layouts): kind, widths, rows per band -- every class of the plan at its boundaries
GENERIC_PLANS = [
    ("vec16", (32, 48, 2048), 14),
    ("vec16", (2064, 4096), 7),
    ("vec16", (4112,), 9),
    ("scalar", (35,), 14),
    ("scalar", (3041,), 13),
]


def _expand_staged(plans):
    return [pytest.param(k, ni, w, rows, h, id=f"k{k}-ni{ni}-w{w}-r{rows}-h{h}") for k, ni, widths, rows in plans for w in widths
            for h in _heights(rows)]


def _expand_generic():
    return [pytest.param(kind, w, rows, h, id=f"{kind}-w{w}-r{rows}-h{h}") for kind, widths, rows in GENERIC_PLANS for w in widths
            for h in _heights(rows)]


@pytest.mark.parametrize("kernel,ni,w,rows,h", _expand_staged(RGB24_PLANS))
def test_rgb24_plan_classes(ctx, oracle, kernel, ni, w, rows, h):
    B = synth.random_frames(2, h, w, seed=h * 7 + w)
    got = ctx.preprocess_picture(Pixels(arrange(B, RGB24), RGB24))
    _check_plan(ctx, RGB24, h, w, kernel, rows, ni)
    _check_outputs(ctx, oracle, got, B, ("rgb24", h, w))


@pytest.mark.parametrize("fmt", (BGRA32, RGBA32), ids=lambda f: NAMES[f])
@pytest.mark.parametrize("kind,w,rows,h", _expand_generic())
def test_px32_plan_classes(ctx, oracle, fmt, kind, w, rows, h):
    B = synth.random_frames(2, h, w, seed=h * 7 + w + 1)
    got = ctx.preprocess_picture(Pixels(arrange(B, fmt), fmt))
    _check_plan(ctx, fmt, h, w, VEC16[fmt] if kind == "vec16" else SCALAR[fmt], rows)
    _check_outputs(ctx, oracle, got, B, (NAMES[fmt], h, w))
    assert ctx.stage_copies() == 1 and ctx.stage_bytes() == 2 * h * w * 4


@pytest.mark.parametrize("kernel,ni,w,rows,h", _expand_staged(RGBP_PLANS))
def test_rgbp_plan_classes(ctx, oracle, kernel, ni, w, rows, h):
    """planes from one [N,3,H,W] host stack: ONE staging copy"""
    B = synth.random_frames(2, h, w, seed=h * 7 + w + 2)
    got = ctx.preprocess_picture(Pixels(arrange(B, RGBP), RGBP))
    _check_plan(ctx, RGBP, h, w, kernel, rows, ni)
    _check_outputs(ctx, oracle, got, B, ("rgbp", h, w))
    assert ctx.stage_copies() == 1 and ctx.stage_bytes() == 2 * 3 * h * w


# ---- the fourth byte -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", (BGRA32, RGBA32), ids=lambda f: NAMES[f])
@pytest.mark.parametrize("w,kind", [(48, "vec16"), (35, "scalar")])
def test_alpha_is_ignored(ctx, oracle, fmt, w, kind):
    h = 44
    B = synth.random_frames(2, h, w, seed=w)
    outs = []
    for alpha in (None, 0, 255):
        got = ctx.preprocess_picture(Pixels(arrange(B, fmt, alpha), fmt))
        _check_plan(ctx, fmt, h, w, VEC16[fmt] if kind == "vec16" else SCALAR[fmt], 14)
        _check_outputs(ctx, oracle, got, B, (NAMES[fmt], w, alpha))
        outs.append(got + (ctx.debug_fetch("area", (2, 32, 32), np.uint8),))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a, b)


# ---- strides and alignment, device input -----------------------------------------------------------------------------------------------------
def _device_flat(torch, nbytes):
    flat = torch.empty(nbytes + 32, dtype=torch.uint8, device="cuda:0")
    return flat, -flat.data_ptr() % 16                       # the buffer and the offset of its first 16-byte boundary


def _place(torch, flat, host_flat):
    flat.copy_(torch.from_numpy(host_flat))
    torch.cuda.synchronize()


@pytest.mark.parametrize("fmt", (RGB24, BGRA32, RGBA32), ids=lambda f: NAMES[f])
@pytest.mark.parametrize("view,kind", [("row_padding", "vec16"), ("base+4", "scalar"), ("row_stride%16=8", "scalar")])
def test_packed_views_on_the_device(ctx, oracle, fmt, view, kind):
    """a row stride with padding runs the 16-byte fill (the staged one for RGB24); a base off by 4 bytes or a row stride that is no multiple
    of 16 runs the scalar fill -- with identical results"""
    torch = pytest.importorskip("torch")
    n, h, w, px = 2, 43, 64, (3 if fmt == RGB24 else 4)
    B = synth.random_frames(n, h, w, seed=fmt)
    host = arrange(B, fmt)
    off, rs = {"row_padding": (0, w * px + 32), "base+4": (4, w * px + 32), "row_stride%16=8": (0, w * px + 8)}[view]
    fs = (rs * h + 15) // 16 * 16
    flat, a16 = _device_flat(torch, off + n * fs)
    staged = np.zeros(flat.numel(), np.uint8)
    np.lib.stride_tricks.as_strided(staged[a16 + off:], host.shape, (fs, rs, px, 1))[...] = host
    _place(torch, flat, staged)
    t = flat.as_strided(host.shape, (fs, rs, px, 1), a16 + off)
    got = ctx.preprocess_picture(Pixels(t, fmt))
    if kind == "scalar":
        _check_plan(ctx, fmt, h, w, SCALAR[fmt], 14)
    else:
        _check_plan(ctx, fmt, h, w, ALIGNED[fmt][0], 14, ALIGNED[fmt][1])
    _check_outputs(ctx, oracle, got, B, (NAMES[fmt], view))
    assert ctx.stage_copies() == 0 and ctx.stage_bytes() == 0


# where the R, G and B planes of a clip lie in one device buffer, in units of one plane's span S (+ bytes): name -> ((r, g, b), kind)
RGBP_PLACEMENTS = {
    "separate_b_g_r_order": (((2, 512), (1, 256), (0, 0)), "aligned"),      # allocated apart, B lowest: gaps between the spans
    "gbrp_permuted_pointers": (((2, 0), (0, 0), (1, 0)), "aligned"),        # ffmpeg's gbrp: G, B, R stored adjacent, handed over as R, G, B
    "g_plane_off_by_8": (((0, 0), (1, 264), (2, 512)), "scalar"),
    "b_plane_off_by_8": (((0, 0), (1, 256), (2, 520)), "scalar"),
}


@pytest.mark.parametrize("place", list(RGBP_PLACEMENTS))
def test_rgbp_plane_placements_on_the_device(ctx, oracle, place):
    torch = pytest.importorskip("torch")
    n, h, w = 2, 43, 64
    B = synth.random_frames(n, h, w, seed=len(place))
    planes = arrange(B, RGBP)                                  # [n, 3, h, w]
    S = n * h * w
    where, kind = RGBP_PLACEMENTS[place]
    flat, a16 = _device_flat(torch, 3 * S + 1024)
    staged = np.zeros(flat.numel(), np.uint8)
    offs = [a16 + units * S + extra for units, extra in where]
    for c, o in enumerate(offs):
        staged[o:o + S] = planes[:, c].reshape(-1)
    _place(torch, flat, staged)
    got = _raw_picture(ctx, RGBP, [flat.data_ptr() + o for o in offs], 1, n, h, w, [w] * 3, [h * w] * 3)
    if kind == "aligned":
        _check_plan(ctx, RGBP, h, w, RGBP_STAGED, 14, 3)
    else:
        _check_plan(ctx, RGBP, h, w, RGBP_SCALAR, 14)
    _check_outputs(ctx, oracle, got, B, ("rgbp", place))


def test_rgbp_separate_host_planes_are_three_copies(ctx, oracle):
    """host planes allocated apart, in B,G,R address order (a channels-first view with a negative channel stride over a buffer with gaps)"""
    n, h, w = 2, 43, 64
    B = synth.random_frames(n, h, w, seed=99)
    planes = arrange(B, RGBP)
    S, gap = n * h * w, 300
    buf = np.zeros(3 * S + 2 * gap, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[2 * (S + gap):], (n, 3, h, w), (h * w, -(S + gap), w, 1))
    view[...] = planes
    assert view[:, 2].ctypes.data < view[:, 1].ctypes.data < view[:, 0].ctypes.data
    got = ctx.preprocess_picture(Pixels(view, RGBP))
    # every span is staged on a 256-byte boundary: the aligned kernel
    _check_plan(ctx, RGBP, h, w, RGBP_STAGED, 14, 3)
    _check_outputs(ctx, oracle, got, B, "separate host planes")
    assert ctx.stage_copies() == 3 and ctx.stage_bytes() == 3 * S


# ---- channel order ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", NEW, ids=lambda f: NAMES[f])
@pytest.mark.parametrize("w", (48, 35))
def test_single_channel_frames(ctx, oracle, fmt, w):
    """R = 255 -> gray 76, G = 255 -> 150, B = 255 -> 29: a swapped or shifted coefficient cannot pass (both fills of every layout)"""
    h = 44
    B = np.zeros((3, h, w, 3), np.uint8)
    B[0, ..., 2] = 255
    B[1, ..., 1] = 255
    B[2, ..., 0] = 255
    got = ctx.preprocess_picture(Pixels(arrange(B, fmt, 255), fmt))
    assert ctx.ingest_format() == fmt
    kernel = SCALAR[fmt] if w == 35 else ALIGNED[fmt][0]
    assert ctx.debug_fetch("ingest_plan", (8,), np.int32)[P_KERNEL] == kernel
    _check_outputs(ctx, oracle, got, B, (NAMES[fmt], w))
    area = ctx.debug_fetch("area", (3, 32, 32), np.uint8)
    for f, gray in enumerate((76, 150, 29)):
        assert (got[0][f] == gray).all() and (area[f] == gray).all(), (NAMES[fmt], f)
    assert not got[2].any() and not got[3].any()               # constant frames: the Laplacian vanishes


# ---- lists -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", NEW, ids=lambda f: NAMES[f])
def test_host_lists_equal_the_strided_call(ctx, oracle, fmt):
    h, w = 43, 64
    B = synth.random_frames(3, h, w, seed=fmt + 7)
    order = [0, 2, 1, 0]                                       # shuffled, with a repeated frame
    frames = [np.ascontiguousarray(f) for f in arrange(B, fmt)]
    got = ctx.preprocess_frame_list([frames[i] for i in order], fmt)
    assert ctx.ingest_list() == (1, 4)
    _check_plan(ctx, fmt, h, w, ALIGNED[fmt][0], 14, ALIGNED[fmt][1])
    _check_outputs(ctx, oracle, got, B[order], (NAMES[fmt], "host list"))
    px = {RGB24: 3, BGRA32: 4, RGBA32: 4, RGBP: 3}[fmt]
    assert ctx.stage_bytes() == 3 * h * w * px                 # the repeated frame crosses the link once
    strided = ctx.preprocess_picture(Pixels(np.ascontiguousarray(arrange(B, fmt)[order]), fmt))
    assert ctx.ingest_list() == (0, 0)
    for a, b in zip(got, strided):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("fmt", NEW, ids=lambda f: NAMES[f])
@pytest.mark.parametrize("misalign", (False, True), ids=("aligned", "one_frame_off"))
def test_device_lists(ctx, oracle, fmt, misalign):
    """torch device frames, each its own tensor ([3,H,W] for RGBP); one frame that is not 16-byte aligned sends the list through the scalar fill"""
    torch = pytest.importorskip("torch")
    h, w = 43, 64
    B = synth.random_frames(3, h, w, seed=fmt + 11)
    host = arrange(B, fmt)
    frames = [torch.from_numpy(np.ascontiguousarray(f)).to("cuda:0") for f in host]
    if misalign:
        flat = torch.zeros(host[1].size + 64, dtype=torch.uint8, device="cuda:0")
        off = -flat.data_ptr() % 16 + 8
        frames[1] = flat[off:off + host[1].size].view(host[1].shape)
        frames[1].copy_(torch.from_numpy(np.ascontiguousarray(host[1])))
        assert frames[1].data_ptr() % 16 == 8
    order = [2, 0, 1, 2]
    got = ctx.preprocess_frame_list([frames[i] for i in order], fmt)
    assert ctx.ingest_list() == (1, 4)
    if misalign:
        _check_plan(ctx, fmt, h, w, SCALAR[fmt], 14)
    else:
        _check_plan(ctx, fmt, h, w, ALIGNED[fmt][0], 14, ALIGNED[fmt][1])
    _check_outputs(ctx, oracle, got, B[order], (NAMES[fmt], "device list", misalign))
    assert ctx.stage_bytes() == 0 and ctx.stage_copies() == 0


# The listed instantiations of the plan classes that no other case of the suite launches (the lists above and those of
# tests/test_gpu_framelist.py are 64 px wide or BGR's first width per fill): layout, kernel, NI, width, rows per band.  Two frames of the
# smallest height above the minimum, the first width of the class (RGB24_PLANS / RGBP_PLANS).
LISTED_PLANS = [
    (BGR, BGR_STAGED, 4, 688, 14), (BGR, BGR_STAGED, 8, 1376, 14),
    (RGB24, BGR_STAGED, 4, 688, 14), (RGB24, BGR_STAGED, 6, 1040, 14), (RGB24, BGR_STAGED, 8, 1376, 14), (RGB24, BGR_STAGED, 9, 2064, 7),
    (RGB24, BGR_VEC16, 0, 4112, 9),
    (RGBP, RGBP_STAGED, 4, 688, 14), (RGBP, RGBP_STAGED, 6, 1040, 14), (RGBP, RGBP_STAGED, 8, 1376, 14), (RGBP, RGBP_VEC16, 0, 4112, 9),
]


@pytest.mark.parametrize("fmt,kernel,ni,w,rows", LISTED_PLANS, ids=[f"{NAMES[c[0]]}-k{c[1]}-ni{c[2]}-w{c[3]}" for c in LISTED_PLANS])
def test_host_lists_plan_classes(ctx, oracle, fmt, kernel, ni, w, rows):
    h = 33
    B = synth.random_frames(2, h, w, seed=h * 7 + w + fmt)
    frames = [np.ascontiguousarray(f) for f in arrange(B, fmt)]
    got = ctx.preprocess_frame_list(frames, fmt)
    assert ctx.ingest_list() == (1, 2)
    _check_plan(ctx, fmt, h, w, kernel, rows, ni)
    _check_outputs(ctx, oracle, got, B, (NAMES[fmt], "host list", w))


# ---- batches ---------------------------------------------------------------------------------------------------------------------------------
def _mixed_clips():
    """BGR, NV12, I420 and the four new layouts at two geometries, with B of each RGB-family clip"""
    rng = np.random.default_rng(5)
    clips, twins = [], []
    for i, fmt in enumerate((BGR, RGB24, BGRA32, RGBA32, RGBP)):
        h, w = ((43, 64), (36, 80))[i & 1]
        B = synth.random_frames(2 + (i & 1), h, w, seed=100 + i)
        clips.append(B if fmt == BGR else Pixels(arrange(B, fmt), fmt))
        twins.append(B)
    for planar in (False, True):
        h, w = (44, 64) if planar else (36, 80)
        y = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
        if planar:
            c = (y, rng.integers(0, 256, (2, h // 2, w // 2), dtype=np.uint8), rng.integers(0, 256, (2, h // 2, w // 2), dtype=np.uint8))
        else:
            c = (y, rng.integers(0, 256, (2, h // 2, w), dtype=np.uint8))
        clips.append(c)
        twins.append(c)
    return clips, twins


def test_mixed_batches(ctx):
    clips, twins = _mixed_clips()
    try:
        for mode in (1, 0):
            ctx.set_option("fb_mode", mode)
            alone = [ctx.analyze_pictures([c])[0] for c in clips]
            # an RGB-family clip alone equals the BGR entry point on B
            for c, t, a in zip(clips, twins, alone):
                if isinstance(c, Pixels):
                    _same_records(a, ctx.analyze_frames(t), (mode, NAMES[c.fmt], "BGR twin"))
            got = ctx.analyze_pictures(clips)
            assert len(got) == len(clips)
            for i, (g, a) in enumerate(zip(got, alone)):
                _same_records(g, a, (mode, i))
        # the async form, drained by another call
        ctx.set_option("fb_mode", 1)
        alone = [ctx.analyze_pictures([c])[0] for c in clips]
        rec = np.zeros(sum(len(a) for a in alone), _lib.RECORD_DTYPE)
        keep, counts = ctx.analyze_pictures_async(clips, rec)
        assert counts == [len(a) for a in alone]
        ctx.preprocess_bgr(twins[0])                           # any other call drains the pending one
        for i, (g, a) in enumerate(zip(np.split(rec, np.cumsum(counts)[:-1]), alone)):
            _same_records(g, a, ("async", i))
        del keep
    finally:
        ctx.set_option("fb_mode", 1)


def test_mixed_frame_list_batch(ctx):
    """avd_analyze_frame_lists over every new layout equals one list per call"""
    lists = []
    for i, fmt in enumerate(NEW):
        h, w = ((43, 64), (36, 80))[i & 1]
        B = synth.random_frames(3, h, w, seed=200 + i)
        lists.append(([np.ascontiguousarray(f) for f in arrange(B, fmt)], fmt))
    alone = [ctx.analyze_frame_lists([l])[0] for l in lists]
    for g, a in zip(ctx.analyze_frame_lists(lists), alone):
        _same_records(g, a, "lists")


# ---- streaming and the drop-in -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", NEW, ids=lambda f: NAMES[f])
def test_records_stream(ctx, fmt):
    B = synth.random_frames(7, 43, 64, seed=fmt + 300)
    fa = avd_hip.FrameAnalyzer(ctx=ctx, chunk=3)               # chunks of 3 + the carry frame: 3, 3, 1
    want = fa.records_stream(iter(B))
    got = fa.records_stream(iter(arrange(B, fmt)), fmt)
    assert ctx.ingest_format() == fmt and ctx.ingest_list()[0] == 1
    _same_records(got, want, NAMES[fmt])
    _same_records(got, ctx.analyze_frames(B), (NAMES[fmt], "whole clip"))


def test_drop_in_analyze_on_an_rgbp_source(monkeypatch):
    from app.analyzers import video
    from avd_hip import sources
    B = synth.random_frames(5, 44, 64, seed=17)

    class Fake(sources.FrameSource):
        fps, width, height, frame_count = 4.0, 64, 44, 5

        def __init__(self, surface, frames):
            self.surface, self._frames = surface, frames

        def sampled(self, step):
            return iter(self._frames[::step])

    monkeypatch.setenv("AVD_CHUNK_FRAMES", "2")
    results = {}
    for surface, frames in (("bgr", B), ("rgbp", arrange(B, RGBP)), ("rgba32", arrange(B, RGBA32))):
        monkeypatch.setattr(sources, "open_source", lambda path, s=surface, f=frames: Fake(s, f))
        results[surface] = video.analyze("clip.fake", {})
    assert results["bgr"]["timeline"] and len(results["bgr"]["timeline"]) == len(results["rgbp"]["timeline"])
    assert results["rgbp"] == results["bgr"] and results["rgba32"] == results["bgr"]


# ---- refusals on the device path -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", NEW, ids=lambda f: NAMES[f])
def test_refusals_launch_nothing(ctx, fmt):
    B = synth.random_frames(2, 43, 64, seed=3)
    ctx.preprocess_bgr(B)
    assert ctx.ingest_format() == BGR
    clip = Pixels(arrange(B, fmt), fmt)
    with pytest.raises(avd_hip.AvdError, match=r"avd status -1: AVD_FMT_FULL_RANGE describes 4:2:0 samples: an RGB picture has no range"):
        ctx.preprocess_picture(clip, 0, True)
    for rotate in (1, 2, 3):
        with pytest.raises(avd_hip.AvdError, match=r"avd status -4: a turned RGB picture is not on the path"):
            ctx.preprocess_picture(clip, rotate)
    with pytest.raises(avd_hip.AvdError, match=r"avd status -4: a turned RGB picture"):
        ctx.analyze_pictures([B, clip], [0, 1])
    with pytest.raises(avd_hip.AvdError, match=r"avd status -1: AVD_FMT_FULL_RANGE"):
        ctx.preprocess_frame_list([np.ascontiguousarray(f) for f in clip.data], fmt, 0, True)
    with pytest.raises(avd_hip.AvdError, match=r"avd status -4: a turned RGB picture"):
        ctx.preprocess_frame_list([np.ascontiguousarray(f) for f in clip.data], fmt, 3)
    assert ctx.ingest_format() == BGR                          # still the launch before the refusals
    ctx.preprocess_picture(clip)
    assert ctx.ingest_format() == fmt


def test_ingest_format_needs_a_launch():
    with avd_hip.Context(0) as c:
        with pytest.raises(avd_hip.AvdError, match="ingest_format not recorded yet"):
            c.ingest_format()
