"""4:2:2 pictures in the fused ingest: AVD_FMT_YUYV422, AVD_FMT_UYVY422, AVD_FMT_I422 and AVD_FMT_NV16 (include/avd.h).

Definition under test (tests/yuv422_reference.py, tied to the pinned 4:2:0 converters by tests/test_yuv422_host.py): pixel (y, x) takes the
chroma sample (y, x >> 1) of its own row through libswscale's tables; every output equals the BGR entry point's on those BGR frames, which is
the oracle's preprocess_bgr.  Everything is compared BIT FOR BIT; there is no tolerance in this file but in the end-to-end comparison with
the oracle's float chain, which has the tolerance of the build's smoke run.

Every case reads the kernel and the rows per band it was written for back from "ingest_plan" and the layout from "ingest_format", so a case
that silently took the other fill fails.  Kernel ids: 14 yuyv_scalar, 15 yuyv_tables (both packed layouts), 16 i422_scalar, 17 i422_tables,
18 nv16_scalar, 19 nv16_tables.  The band plan is the generic kernel's, keyed by the width as for 4:2:0; the heights may be odd here, and a
band begins on any row.  One case runs the four layouts on the same samples, so the reference is formed once per geometry."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import avd_hip  # noqa: E402
from avd_hip import Pixels, _lib, synth  # noqa: E402
from tests import yuv422_reference as ref  # noqa: E402
from tests.ingest_gpu_kit import check_plan  # noqa: E402
from tests.ingest_gpu_kit import check_outputs as _check_outputs  # noqa: E402
from tests.ingest_gpu_kit import raw_picture as _raw_picture  # noqa: E402
from tests.ingest_gpu_kit import reference as _reference  # noqa: E402
from tests.ingest_gpu_kit import same_records as _same_records  # noqa: E402
from tests.test_gpu_i420 import _device_view  # noqa: E402

BGR, NV12, I420, RGBP, FULL = 0, 1, 2, 0x13, 0x100
YUYV, UYVY, I422, NV16 = ref.LAYOUTS
NEW = ref.LAYOUTS
NAMES = ref.NAMES
SCALAR = {YUYV: 14, UYVY: 14, I422: 16, NV16: 18}
TABLES = {YUYV: 15, UYVY: 15, I422: 17, NV16: 19}
PLANES = {YUYV: 1, UYVY: 1, I422: 3, NV16: 2}


def _check_plan(ctx, fmt, h, w, kernel, rows, full_range=False, lds=None):
    check_plan(ctx, h, w, kernel, rows, 0, lds, fmt=fmt, rotate=0, full_range=full_range)


def _clip(fmt, y, u, v):
    return Pixels(ref.pack(fmt, y, u, v), fmt)


# ---- the two fills over the plan classes, host input ---------------------------------------------------------------------------------------
# (w, rows per band) -> heights: the I420 sweep's (even plans a two-row and a full last band, odd plans a one-row and a full one) plus ODD
# heights -- 33, the smallest, and 43 = 3 * 14 + 1, whose last band is a single row of a 14-row plan; 37 = 4 * 9 + 1 likewise at 9 rows.
TABLE_PLANS = {(48, 14): (44, 42, 33, 43), (2064, 7): (36, 42, 37), (4112, 9): (46, 36, 37), (6128, 5): (36, 40, 33), (12272, 1): (34, 33),
               (16384, 1): (34, 33)}
SCALAR_PLANS = {(34, 14): (44, 42, 33, 43), (1922, 14): (44, 33), (8190, 3): (34, 36, 35), (12274, 1): (34, 33)}


def _cases(plans, kind):
    return [pytest.param(kind, w, r, h, id=f"{kind}-w{w}-r{r}-h{h}") for (w, r), hs in plans.items() for h in hs]


@pytest.mark.parametrize("kind,w,rows,h", _cases(TABLE_PLANS, "tables") + _cases(SCALAR_PLANS, "scalar"))
def test_plan_classes(ctx, oracle, kind, w, rows, h):
    n = 2
    y, u, v = ref.random_planes(n, h, w, seed=h * 7 + w)
    want = _reference(oracle, ref.to_bgr(y, u, v, False))
    for fmt in NEW:
        got = ctx.preprocess_picture(_clip(fmt, y, u, v))
        lds = 57696 if (kind, w) == ("tables", 16384) else None              # 3 * 16416 + 3 * 4 * 704, as NV12
        _check_plan(ctx, fmt, h, w, (TABLES if kind == "tables" else SCALAR)[fmt], rows, lds=lds)
        _check_outputs(ctx, got, want, (NAMES[fmt], h, w))
        # packed: one span of 2w-byte rows; separately allocated planes: one copy each; two bytes per pixel either way
        assert ctx.stage_copies() == PLANES[fmt] and ctx.stage_bytes() == 2 * n * h * w, NAMES[fmt]


# ---- both ranges on content that reaches both ends of the table window ------------------------------------------------------------------------
@pytest.mark.parametrize("full_range", (False, True), ids=("limited", "full"))
@pytest.mark.parametrize("w,kind", [(48, "tables"), (34, "scalar")])
def test_both_ranges_on_enumerated_content(ctx, oracle, w, kind, full_range):
    n, h = 4, 33
    y, u, v = ref.enum_planes(n, h, w, seed=w + full_range)
    want = _reference(oracle, ref.to_bgr(y, u, v, full_range))
    other = _reference(oracle, ref.to_bgr(y, u, v, not full_range))
    assert not np.array_equal(want[0], other[0])
    for fmt in NEW:
        got = ctx.preprocess_picture(_clip(fmt, y, u, v), 0, full_range)
        _check_plan(ctx, fmt, h, w, (TABLES if kind == "tables" else SCALAR)[fmt], 14, full_range)
        _check_outputs(ctx, got, want, (NAMES[fmt], w, full_range))


def test_yv16_is_i422_with_the_chroma_pointers_exchanged(ctx, oracle):
    y, u, v = ref.random_planes(2, 33, 48, seed=16)
    got = ctx.preprocess_picture(Pixels((y, v, u), I422))
    _check_plan(ctx, I422, 33, 48, TABLES[I422], 14)
    _check_outputs(ctx, got, _reference(oracle, ref.to_bgr(y, v, u, False)), "yv16")
    assert not np.array_equal(got[0], ctx.preprocess_picture(Pixels((y, u, v), I422))[0])


# ---- alignment dispatch on device views ---------------------------------------------------------------------------------------------------
A_N, A_H, A_W = 2, 33, 48
# view -> (tables?, per plane (base offset from a 16-byte boundary, row padding, odd frame stride)); planes a layout lacks are not used.
# Every misalignment the launcher tells apart, on plane 0 (all layouts) and on the chroma planes (NV16: 16 bytes; I422: 8).
VIEWS = {
    "aligned_padded": (True, (32, 16, False), (48, 16, False), (16, 16, False)),
    "base+1": (False, (1, 16, False), (0, 16, False), (0, 16, False)),
    "pitch_8mod16": (False, (0, 8, False), (0, 16, False), (0, 16, False)),
    "frame_stride_odd": (False, (0, 16, True), (0, 16, False), (0, 16, False)),
    "chroma_8mod16": ({I422: True, NV16: False}, (0, 16, False), (8, 8, False), (24, 8, False)),        # I422: still the table fill
    "chroma_4mod8": ({I422: False, NV16: False}, (0, 16, False), (4, 16, False), (12, 16, False)),
    "chroma_pitch_4mod8": ({I422: False, NV16: False}, (0, 16, False), (0, 4, False), (0, 4, False)),
}


@pytest.fixture(scope="module")
def align_input(oracle):
    """The samples and their oracle results, formed once and left unchanged."""
    y, u, v = ref.random_planes(A_N, A_H, A_W, seed=A_H + A_W)
    return (y, u, v), _reference(oracle, ref.to_bgr(y, u, v, False))


# a packed layout has no chroma plane: the chroma views are cases of I422 and NV16 only
ALIGN_CASES = [pytest.param(view, fmt, id=f"{view}-{NAMES[fmt]}") for view, spec in VIEWS.items() for fmt in NEW
               if not isinstance(spec[0], dict) or fmt in spec[0]]


@pytest.mark.parametrize("view,fmt", ALIGN_CASES)
def test_alignment_dispatch(ctx, align_input, view, fmt):
    torch = pytest.importorskip("torch")
    tables, *specs = VIEWS[view]
    if isinstance(tables, dict):
        tables = tables[fmt]
    (y, u, v), want = align_input
    clip = ref.pack(fmt, y, u, v)
    host = [clip.reshape(A_N, A_H, 2 * A_W)] if PLANES[fmt] == 1 else list(clip)
    views = [_device_view(torch, np.ascontiguousarray(p), spec) for p, spec in zip(host, specs)]
    if (view, fmt) == ("chroma_8mod16", I422):
        assert views[1].data_ptr() % 16 == 8 and views[2].data_ptr() % 16 == 8
    got = _raw_picture(ctx, fmt, views, A_N, A_H, A_W)
    _check_plan(ctx, fmt, A_H, A_W, (TABLES if tables else SCALAR)[fmt], 14)
    _check_outputs(ctx, got, want, (view, NAMES[fmt]))
    assert ctx.stage_bytes() == 0 and ctx.stage_copies() == 0


# ---- host staging -------------------------------------------------------------------------------------------------------------------------
def test_a_dense_i422_frame_stack_is_one_copy(ctx, oracle):
    """what a C422 .y4m map is: Y | U | V of a frame adjacent, frame after frame; an odd height puts V on 8 mod 16 -- still the table fill"""
    n, h, w = 3, 33, 48
    y, u, v = ref.random_planes(n, h, w, seed=77)
    want = _reference(oracle, ref.to_bgr(y, u, v, False))
    for gap, kernel in ((0, TABLES[I422]), (6, SCALAR[I422])):                  # a FRAME marker makes the frame stride 6 mod 8: scalar
        fs = gap + 2 * h * w
        flat = np.zeros(n * fs, np.uint8)
        strided = lambda o, shape: np.lib.stride_tricks.as_strided(flat[gap + o:], (n,) + shape, (fs, shape[1], 1))
        planes = (strided(0, (h, w)), strided(h * w, (h, w // 2)), strided(h * w + h * (w // 2), (h, w // 2)))
        for dst, src in zip(planes, (y, u, v)):
            dst[...] = src
        got = ctx.preprocess_picture(Pixels(planes, I422))
        _check_plan(ctx, I422, h, w, kernel, 14)
        _check_outputs(ctx, got, want, ("one buffer", gap))
        assert ctx.stage_copies() == 1 and ctx.stage_bytes() == (n - 1) * fs + 2 * h * w


def test_row_padded_packed_host_clip(ctx, oracle):
    n, h, w = 2, 35, 48
    y, u, v = ref.random_planes(n, h, w, seed=78)
    want = _reference(oracle, ref.to_bgr(y, u, v, False))
    for fmt in (YUYV, UYVY):
        buf = np.zeros((n, h, w + 8, 2), np.uint8)
        buf[:, :, :w] = ref.pack(fmt, y, u, v)
        got = ctx.preprocess_picture(Pixels(buf[:, :, :w], fmt))
        _check_plan(ctx, fmt, h, w, TABLES[fmt], 14)
        _check_outputs(ctx, got, want, NAMES[fmt])
        rs = 2 * (w + 8)
        assert ctx.stage_copies() == 1 and ctx.stage_bytes() == rs * h * (n - 1) + rs * (h - 1) + 2 * w


# ---- frame lists ----------------------------------------------------------------------------------------------------------------------------
def _frames_of(fmt, clip, to=lambda a: np.array(a)):
    """the clip as per-frame arrays, every plane of every frame an allocation of its own"""
    if PLANES[fmt] == 1:
        return [to(f) for f in clip]
    return [tuple(to(pl[f]) for pl in clip) for f in range(len(clip[0]))]


@pytest.mark.parametrize("fmt", NEW, ids=lambda f: NAMES[f])
def test_host_lists_equal_the_strided_call(ctx, oracle, fmt):
    h, w = 33, 48
    y, u, v = ref.random_planes(3, h, w, seed=fmt + 7)
    order = [0, 2, 1, 0]                                       # shuffled, with a repeated frame
    frames = _frames_of(fmt, ref.pack(fmt, y, u, v))
    got = ctx.preprocess_frame_list([frames[i] for i in order], fmt, 0, True)
    assert ctx.ingest_list() == (1, 4)
    _check_plan(ctx, fmt, h, w, TABLES[fmt], 14, True)
    _check_outputs(ctx, got, _reference(oracle, ref.to_bgr(y[order], u[order], v[order], True)), (NAMES[fmt], "host list"))
    assert ctx.stage_bytes() == 3 * 2 * h * w and ctx.stage_copies() == 3 * PLANES[fmt]      # the repeated frame crosses the link once
    strided = ctx.preprocess_picture(_clip(fmt, y[order], u[order], v[order]), 0, True)
    assert ctx.ingest_list() == (0, 0)
    for a, b in zip(got, strided):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("fmt", NEW, ids=lambda f: NAMES[f])
@pytest.mark.parametrize("misalign", (False, True), ids=("aligned", "one_frame_off"))
def test_device_lists(ctx, oracle, fmt, misalign):
    """torch device frames, each plane its own tensor, listed in another order than they were allocated in; one plane of one frame that is
    not aligned sends the whole list through the scalar fill"""
    torch = pytest.importorskip("torch")
    h, w = 33, 48
    y, u, v = ref.random_planes(3, h, w, seed=fmt + 11)
    frames = _frames_of(fmt, ref.pack(fmt, y, u, v), lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0"))
    if misalign:
        last = frames[1] if PLANES[fmt] == 1 else frames[1][-1]
        flat = torch.zeros(last.numel() + 64, dtype=torch.uint8, device="cuda:0")
        off = -flat.data_ptr() % 16 + 4                        # 4 mod 16: misaligned for the 8-byte chroma loads of I422 too
        moved = flat[off:off + last.numel()].view(last.shape)
        moved.copy_(last)
        assert moved.data_ptr() % 8 == 4
        frames[1] = moved if PLANES[fmt] == 1 else frames[1][:-1] + (moved,)
    torch.cuda.synchronize()
    order = [2, 0, 1, 2]
    got = ctx.preprocess_frame_list([frames[i] for i in order], fmt)
    assert ctx.ingest_list() == (1, 4)
    _check_plan(ctx, fmt, h, w, (SCALAR if misalign else TABLES)[fmt], 14)
    _check_outputs(ctx, got, _reference(oracle, ref.to_bgr(y[order], u[order], v[order], False)), (NAMES[fmt], "device list", misalign))
    assert ctx.stage_bytes() == 0 and ctx.stage_copies() == 0


# ---- batches, the asynchronous form -----------------------------------------------------------------------------------------------------------
def _mixed_clips():
    """the four layouts with NV12, I420, BGR and RGBP clips, two geometries (one of odd height), mixed ranges
    -> (clips, ranges, the BGR twin of every 4:2:2 clip or None)"""
    rng = np.random.default_rng(5)
    clips, ranges, twins = [], [], []
    for i, fmt in enumerate(NEW):
        h, w = ((33, 48), (36, 80))[i & 1]
        full = bool(i & 2) != bool(i & 1)
        y, u, v = ref.random_planes(2 + (i & 1), h, w, seed=100 + i)
        clips.append(_clip(fmt, y, u, v))
        ranges.append(full)
        twins.append(ref.to_bgr(y, u, v, full))
    y = rng.integers(0, 256, (2, 36, 80), dtype=np.uint8)
    clips += [(y, rng.integers(0, 256, (2, 18, 80), dtype=np.uint8)),
              (y, rng.integers(0, 256, (2, 18, 40), dtype=np.uint8), rng.integers(0, 256, (2, 18, 40), dtype=np.uint8)),
              synth.random_frames(3, 33, 48, seed=104), Pixels(np.ascontiguousarray(synth.random_frames(2, 36, 80, seed=105).transpose(0, 3, 1, 2)), RGBP)]
    ranges += [True, False, False, False]
    twins += [None] * 4
    return clips, ranges, twins


def test_mixed_batches(ctx):
    clips, ranges, twins = _mixed_clips()
    try:
        for mode in (1, 0):
            ctx.set_option("fb_mode", mode)
            alone = [ctx.analyze_pictures([c], None, [r])[0] for c, r in zip(clips, ranges)]
            for c, t, a in zip(clips, twins, alone):
                if t is not None:                              # a 4:2:2 clip alone equals the BGR entry point on the definition's frames
                    _same_records(a, ctx.analyze_frames(t), (mode, NAMES[c.fmt], "BGR twin"))
            got = ctx.analyze_pictures(clips, None, ranges)
            assert len(got) == len(clips)
            for i, (g, a) in enumerate(zip(got, alone)):
                _same_records(g, a, (mode, i))
    finally:
        ctx.set_option("fb_mode", 1)


def test_async_and_a_call_made_while_one_is_pending(ctx, oracle):
    clips, ranges, twins = _mixed_clips()
    clips, ranges = clips[:4], ranges[:4]
    alone = [ctx.analyze_pictures([c], None, [r])[0] for c, r in zip(clips, ranges)]
    rec = np.zeros(sum(len(a) for a in alone), _lib.RECORD_DTYPE)
    keep, counts = ctx.analyze_pictures_async(clips, rec, None, ranges)
    assert counts == [len(a) for a in alone]
    # a 4:2:2 call made while that one is pending: it drains the pending call first, and is itself right
    y, u, v = ref.random_planes(2, 33, 48, seed=9)
    got = ctx.preprocess_picture(_clip(UYVY, y, u, v))
    for i, (g, a) in enumerate(zip(np.split(rec, np.cumsum(counts)[:-1]), alone)):
        _same_records(g, a, ("async", i))
    _check_plan(ctx, UYVY, 33, 48, TABLES[UYVY], 14)
    _check_outputs(ctx, got, _reference(oracle, ref.to_bgr(y, u, v, False)), "while pending")
    del keep
    # the list form, drained by synchronize()
    lists = [(_frames_of(c.fmt, c.data), c.fmt) for c in clips]
    rec2 = np.zeros_like(rec)
    keep, counts2 = ctx.analyze_frame_lists_async(lists, rec2, None, ranges)
    ctx.synchronize()
    assert counts2 == counts and rec2.tobytes() == rec.tobytes()
    del keep


# ---- refusals through the real entry points ---------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    torch = pytest.importorskip("torch")
    B = synth.random_frames(2, 33, 48, seed=3)
    ctx.preprocess_bgr(B)
    assert ctx.ingest_format() == BGR
    y, u, v = ref.random_planes(2, 33, 48, seed=4)
    for fmt in NEW:
        clip = _clip(fmt, y, u, v)
        for rotate in (1, 2, 3):
            with pytest.raises(avd_hip.AvdError, match=r"avd status -4: a turned 4:2:2 picture is not on the path"):
                ctx.preprocess_picture(clip, rotate)
        with pytest.raises(avd_hip.AvdError, match=r"avd status -4: a turned 4:2:2 picture"):
            ctx.analyze_pictures([B, clip], [0, 1])
        with pytest.raises(avd_hip.AvdError, match=r"avd status -4: a turned 4:2:2 picture"):
            ctx.preprocess_frame_list(_frames_of(fmt, clip.data), fmt, 3)
    # an odd width
    with pytest.raises(avd_hip.AvdError, match=r"avd status -4: YUYV422 needs even width"):
        ctx.preprocess_picture(Pixels(np.zeros((2, 33, 35, 2), np.uint8), YUYV))
    with pytest.raises(avd_hip.AvdError, match=r"avd status -4: UYVY422 needs even width"):
        ctx.preprocess_frame_list([np.zeros((33, 35, 2), np.uint8)], UYVY)
    # I422 chroma planes at different strides: the binding refuses them itself, so the descriptor is written out by hand
    views = [torch.zeros(s, dtype=torch.uint8, device="cuda:0") for s in ((2, 33, 48), (2, 33, 24), (2, 33, 32))]
    with pytest.raises(avd_hip.AvdError, match=r"avd status -1: the U and V planes of an I422 picture share their strides"):
        _raw_picture(ctx, I422, views, 2, 33, 48)
    with pytest.raises(avd_hip.AvdError, match=r"avd status -4: I422 needs even width"):
        _raw_picture(ctx, I422, views[:2] + views[1:2], 2, 33, 47)
    assert ctx.ingest_format() == BGR                          # still the launch before the refusals
    ctx.preprocess_picture(_clip(NV16, y, u, v))
    assert ctx.ingest_format() == NV16


# ---- FFmpeg up to 7.0: planar 4:2:2 through the 4:2:0 special converter -----------------------------------------------------------------------
def test_i420_call_with_a_doubled_chroma_stride_uses_the_even_chroma_rows(ctx, oracle):
    """Documentation (this case passes without the 4:2:2 layouts): the existing I420 call on a 4:2:2 buffer with the chroma row stride
    doubled converts with chroma rows 0, 2, 4 ... only -- what FFmpeg's unscaled yuv422p converter did up to 7.0."""
    h, w = 36, 48
    y, u, v = ref.random_planes(2, h, w, seed=70)
    got = ctx.preprocess_i420(y, u[:, 0::2], v[:, 0::2])
    assert ctx.ingest_format() == I420
    even = lambda c: np.repeat(c[:, 0::2], 2, axis=1)
    _check_outputs(ctx, got, _reference(oracle, ref.to_bgr(y, even(u), even(v), False)), "even chroma rows")
    assert not np.array_equal(got[0], oracle.preprocess_bgr(ref.to_bgr(y, u, v, False))[0])


# ---- streaming and the drop-in ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full_range", (False, True), ids=("limited", "full"))
def test_a_c422_y4m_end_to_end(tmp_path, monkeypatch, oracle, full_range):
    """A C422 .y4m of odd height through the drop-in analyzer, across streaming chunk boundaries: what the BGR frames of the definition give,
    and what the oracle chain makes of them (the tolerance of the build's smoke run: the default Farneback mode)."""
    from app.analyzers import video
    from avd_hip import sources
    n, h, w = 10, 65, 96
    y, u, v = ref.enum_planes(n, h, w, seed=25)
    path = str(tmp_path / "mjpeg.y4m")
    sources.write_y4m(path, y, ref.pack(NV16, y, u, v)[1], fps=(4, 1), full_range=full_range)      # 4 fps: step 2 -> 5 sampled frames
    monkeypatch.setenv("AVD_CHUNK_FRAMES", "2")                                                     # chunks of 2 + carry: 2, 2, 1
    bgr = ref.to_bgr(y, u, v, full_range)
    npy = str(tmp_path / "mjpeg.npy")
    np.save(npy, bgr)
    meta = {"fps": 4.0, "duration": n / 4.0}
    want = video.analyze(npy, dict(meta))
    got = video.analyze(path, {})
    assert got == want and len(got["timeline"]) == 2
    o = oracle.analyze_sampled_frames(bgr[::2], {"width": w, "height": h, "fps": 4.0, "duration": n / 4.0})
    assert np.allclose(got["timeline"], o["timeline"], rtol=0, atol=1e-6), (got["timeline"], o["timeline"])
    for k, val in o["summary"].items():
        assert abs(got["summary"][k] - val) <= 1e-6 * max(1.0, abs(val)), k
    with avd_hip.Context(0) as c:
        fa = avd_hip.FrameAnalyzer(chunk=3, ctx=c)
        rec = fa.records_stream(iter(bgr))
        src = sources.open_source(path)
        assert src.surface == "i422" and src.full_range == full_range
        assert fa.records_stream_i422(src.sampled(1), full_range=src.full_range).tobytes() == rec.tobytes()
        # the last chunk: the carry frame and one more, each Y | U | V of the map merged into ONE copy (a FRAME marker lies between them)
        assert (c.ingest_format(), c.ingest_list(), c.stage_copies(), c.stage_bytes()) == (I422, (1, 2), 2, 2 * 2 * h * w)
        assert fa.records_stream_i422(src.sampled(1), full_range=not full_range).tobytes() != rec.tobytes()
        src.close()
        if not full_range:                                     # records_stream takes the packed layouts, limited range
            for fmt in (YUYV, UYVY):
                assert fa.records_stream(iter(ref.pack(fmt, y, u, v)), fmt).tobytes() == rec.tobytes()
