"""10-bit 4:2:0 pictures in 16-bit words in the fused ingest: AVD_FMT_P010 and AVD_FMT_I010 (include/avd.h).

Definition under test (tests/yuv10_reference.py, tied to the pinned 8-bit converter by tests/test_yuv10_host.py): every word is narrowed to
8 bits -- P010 min(255, (s + 128) >> 8), I010 min(255, (s + 2) >> 2) -- and the NV12 / I420 picture of those samples gives every output.
Everything is compared BIT FOR BIT, with no tolerance anywhere: against the oracle on the definition's BGR frames, against the BGR entry point
on those frames, and against the NV12 / I420 call on the narrowed planes.

Every case reads "ingest_plan" (kernel id, rows per band, and the dynamic LDS bytes, which must be NV12's at that displayed geometry),
"ingest_format", "ingest_range" and "ingest_rotate" back, so a case that silently took another fill fails.  Kernel ids: 20 p010_scalar,
21 p010_tables, 22 i010_scalar, 23 i010_tables, 24 p010_strip, 25 i010_strip; a half turn runs under 20 .. 23."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import avd_hip  # noqa: E402
from avd_hip import Pixels, _lib, synth  # noqa: E402
from tests import yuv10_reference as ref  # noqa: E402
from tests import yuv_tables_reference as ytr  # noqa: E402
from tests.ingest_gpu_kit import P_KERNEL, P_LDS, check_plan  # noqa: E402
from tests.ingest_gpu_kit import check_outputs as _check_outputs  # noqa: E402
from tests.ingest_gpu_kit import plan as _plan  # noqa: E402
from tests.ingest_gpu_kit import raw_picture as _raw_picture  # noqa: E402
from tests.ingest_gpu_kit import reference as _reference  # noqa: E402
from tests.ingest_gpu_kit import same_records as _same_records  # noqa: E402
from tests.test_gpu_i420 import _device_view, _heights  # noqa: E402

BGR, NV12, I420, FULL = 0, 1, 2, 0x100
P010, I010 = ref.LAYOUTS
NEW = ref.LAYOUTS
NAMES = ref.NAMES
SCALAR = {P010: 20, I010: 22}
TABLES = {P010: 21, I010: 23}
STRIP = {P010: 24, I010: 25}
PLANES = {P010: 2, I010: 3}
NV12_SCALAR, NV12_TABLES, NV12_STRIP = 3, 4, 7


def _check_plan(ctx, fmt, h, w, kernel, rows, nv12_lds, rotate=0, full_range=False):
    """h, w: the DISPLAYED picture; nv12_lds: the LDS bytes the NV12 launch of the same displayed geometry and fill shape asked for"""
    check_plan(ctx, h, w, kernel, rows, 0, nv12_lds, fmt=fmt, rotate=rotate, full_range=full_range)


def _same(got, other, tag):
    for name, a, b in zip(("small320", "hash", "lap_sum", "lap_sumsq"), got, other):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (tag, name)


def _turn(planes, k):
    """the stored planes whose picture, turned k quarter turns clockwise, is `planes` (include/avd.h: D = np.rot90(S, -k))"""
    return tuple(np.ascontiguousarray(np.rot90(p, k, axes=(-2, -1))) for p in planes)


def _nv12_run(ctx, clip8, rotate, full_range, kernel):
    """the 8-bit call on the narrowed planes -> (its outputs, the LDS bytes of its launch)"""
    out = ctx.preprocess_picture(clip8, rotate, full_range)
    p = _plan(ctx)
    assert p[P_KERNEL] == kernel, (p, kernel)
    return out, p[P_LDS]


def _sweep(ctx, oracle, h, w, rows, rotate, kind, seed):
    """one displayed geometry, both layouts: against the oracle on the definition's frames and against the NV12 and I420 calls on the narrowed
    planes; kind: which fill shape must have run"""
    n = 2
    disp = ref.random_planes10(n, h, w, seed)
    stored = _turn(disp, rotate)
    nv_kernel = {"tables": NV12_TABLES, "scalar": NV12_SCALAR, "strip": NV12_STRIP}[kind]
    ids = {"tables": TABLES, "scalar": SCALAR, "strip": STRIP}[kind]
    want = None
    for fmt in NEW:
        clip = ref.pack(fmt, *stored)
        if want is None:                                       # the same samples in both layouts: one reference, one pair of 8-bit calls
            want = _reference(oracle, ref.to_bgr(fmt, ref.pack(fmt, *disp), False))
            nv, lds = _nv12_run(ctx, ref.narrowed_nv12(fmt, clip), rotate, False, nv_kernel)
            _check_outputs(ctx, nv, want, ("nv12 on the narrowed planes", h, w, rotate))
            i420 = ctx.preprocess_picture(ref.narrowed_i420(fmt, clip), rotate)
        else:
            assert np.array_equal(ref.narrowed_nv12(fmt, clip)[0], ref.narrowed_nv12(NEW[0], ref.pack(NEW[0], *stored))[0])
        got = ctx.preprocess_picture(Pixels(clip, fmt), rotate)
        _check_plan(ctx, fmt, h, w, ids[fmt], rows, lds, rotate)
        _check_outputs(ctx, got, want, (NAMES[fmt], h, w, rotate))
        _same(got, nv, (NAMES[fmt], "nv12"))
        _same(got, i420, (NAMES[fmt], "i420"))
        # separately allocated planes of the STORED picture: one copy each, three bytes per pixel
        assert ctx.stage_copies() == PLANES[fmt] and ctx.stage_bytes() == 3 * n * h * w, NAMES[fmt]


# ---- 1: the table and scalar fills over the plan classes of tests/test_gpu_i420.py ------------------------------------------------------------
TABLE_PLANS = [(48, 14), (2064, 7), (4112, 9), (6128, 5), (12272, 1), (16384, 1)]
SCALAR_PLANS = [(34, 14), (1922, 14), (8190, 3), (12274, 1)]


def _cases(plans, kind, ks=(0,)):
    return [pytest.param(kind, k, w, r, h, id=f"{kind}-k{k}-w{w}-r{r}-h{h}") for k in ks for w, r in plans for h in _heights(r)]


@pytest.mark.parametrize("kind,k,w,rows,h", _cases(TABLE_PLANS, "tables") + _cases(SCALAR_PLANS, "scalar"))
def test_plan_classes(ctx, oracle, kind, k, w, rows, h):
    _sweep(ctx, oracle, h, w, rows, 0, kind, seed=h * 7 + w)
    if w == 16384:
        assert _plan(ctx)[P_LDS] == 57696                      # 3 * 16416 + 3 * 4 * 704: more than 48 KiB of dynamic LDS, as NV12


# ---- 2: the strip fills over the classes of tests/test_gpu_rotate.py, half turns on tables and scalar -----------------------------------------
STRIP_PLANS = [(34, 14), (48, 14), (2064, 7), (4112, 9), (12272, 1)]
HALF_TABLE_PLANS = [(48, 14), (2064, 7), (16384, 1)]
HALF_SCALAR_PLANS = [(34, 14), (1922, 14)]


@pytest.mark.parametrize("kind,k,w,rows,h", _cases(STRIP_PLANS, "strip", (1, 3)))
def test_strip_fill_plan_classes(ctx, oracle, kind, k, w, rows, h):
    _sweep(ctx, oracle, h, w, rows, k, "strip", seed=h * 5 + w + k)


@pytest.mark.parametrize("kind,k,w,rows,h", _cases(HALF_TABLE_PLANS, "tables", (2,)) + _cases(HALF_SCALAR_PLANS, "scalar", (2,)))
def test_half_turn_plan_classes(ctx, oracle, kind, k, w, rows, h):
    _sweep(ctx, oracle, h, w, rows, 2, kind, seed=h * 3 + w)


# ---- 3: both ranges on enumerated content; words outside the 10-bit samples -------------------------------------------------------------------
@pytest.mark.parametrize("full_range", (False, True), ids=("limited", "full"))
@pytest.mark.parametrize("w,kind,rotate", [(48, "tables", 0), (34, "scalar", 0), (48, "strip", 1)])
def test_both_ranges_on_enumerated_content(ctx, oracle, w, kind, rotate, full_range):
    h = 36
    n = ytr.enum_frames(h, w) + 1
    disp = ref.enum_planes10(n, h, w, seed=w + full_range)
    stored = _turn(disp, rotate)
    rng = np.random.default_rng(w)
    ids = {"tables": TABLES, "scalar": SCALAR, "strip": STRIP}[kind]
    nv_kernel = {"tables": NV12_TABLES, "scalar": NV12_SCALAR, "strip": NV12_STRIP}[kind]
    bgr = ref.to_bgr(I010, ref.pack(I010, *disp), full_range)
    want = _reference(oracle, bgr)
    assert not np.array_equal(want[0], _reference(oracle, ref.to_bgr(I010, ref.pack(I010, *disp), not full_range))[0])
    from_bgr = ctx.preprocess_bgr(bgr)                          # the BGR entry point on the definition's frames
    nv, lds = _nv12_run(ctx, ref.narrowed_nv12(I010, ref.pack(I010, *stored)), rotate, full_range, nv_kernel)
    for fmt in NEW:
        clip = ref.pack(fmt, *stored)
        if fmt == P010:                                        # random non-zero low six bits never change a P010 sample
            clip = tuple(p | rng.integers(0, 64, p.shape, dtype=np.uint16) for p in clip)
            assert any((p & 63).any() for p in clip)
        got = ctx.preprocess_picture(Pixels(clip, fmt), rotate, full_range)
        _check_plan(ctx, fmt, h, w, ids[fmt], 14, lds, rotate, full_range)
        _check_outputs(ctx, got, want, (NAMES[fmt], w, full_range))
        _same(got, from_bgr, (NAMES[fmt], "bgr entry point"))
        _same(got, nv, (NAMES[fmt], "nv12"))


@pytest.mark.parametrize("w,kind,rotate", [(48, "tables", 0), (34, "scalar", 2), (48, "strip", 3)])
def test_words_above_the_samples_are_defined(ctx, oracle, w, kind, rotate):
    """I010 words above 1023 (0xFFFF among them) and every P010 word: the definition is total, super-white clips to 255 before the tables"""
    n, h = 2, 36
    rng = np.random.default_rng(w + rotate)
    ids = {"tables": TABLES, "scalar": SCALAR, "strip": STRIP}[kind]
    nv_kernel = {"tables": NV12_TABLES, "scalar": NV12_SCALAR, "strip": NV12_STRIP}[kind]
    disp = tuple(rng.integers(0, 65536, s, dtype=np.uint16) for s in ((n, h, w), (n, h // 2, w // 2), (n, h // 2, w // 2)))
    for p in disp:
        p.reshape(-1)[:8] = (0xFFFF, 0xFFFE, 0xFFFD, 1024, 1023, 1021, 0xFF80, 0xFF7F)
    stored = _turn(disp, rotate)
    for fmt in NEW:
        y, u, v = stored
        clip = (y, u, v) if fmt == I010 else (y, np.ascontiguousarray(np.stack([u, v], -1).reshape(u.shape[:-1] + (-1,))))     # the words as they are
        dclip = disp if fmt == I010 else (disp[0], np.ascontiguousarray(np.stack(disp[1:], -1).reshape(disp[1].shape[:-1] + (-1,))))
        want = _reference(oracle, ref.to_bgr(fmt, dclip, False))
        nv, lds = _nv12_run(ctx, ref.narrowed_nv12(fmt, clip), rotate, False, nv_kernel)
        got = ctx.preprocess_picture(Pixels(clip, fmt), rotate)
        _check_plan(ctx, fmt, h, w, ids[fmt], 14, lds, rotate)
        _check_outputs(ctx, got, want, (NAMES[fmt], kind))
        _same(got, nv, (NAMES[fmt], "nv12"))
    assert (ref.narrowed_i420(I010, disp)[0] == 255).mean() > 0.9          # nearly every random word is super-white as I010


# ---- 4: alignment dispatch on device views and row-padded host clips -----------------------------------------------------------------------------
A_N, A_H, A_W = 2, 34, 48


@pytest.fixture(scope="module")
def align_input(oracle):
    """The samples, their oracle results and the LDS bytes of NV12's two fills at this geometry; formed once and left unchanged."""
    planes = ref.random_planes10(A_N, A_H, A_W, seed=A_H + A_W)
    want = _reference(oracle, ref.to_bgr(I010, planes, False))
    with avd_hip.Context(0) as c:
        y8, uv8 = ref.narrowed_nv12(I010, planes)
        _, lds_t = _nv12_run(c, (y8, uv8), 0, False, NV12_TABLES)
        _, lds_s = _nv12_run(c, (np.zeros((A_N, A_H, A_W + 8), np.uint8)[:, :, 1:A_W + 1], uv8), 0, False, NV12_SCALAR)
    return planes, want, {True: lds_t, False: lds_s}


def _align_cases():
    out = []
    for fmt in NEW:
        for plane in range(PLANES[fmt]):
            for off in (2, 4, 8, 16):                          # 2-byte aligned as it must be; only 16 keeps the 16-byte loads
                specs = [(off if p == plane else 0, 16, False) for p in range(PLANES[fmt])]
                out.append(pytest.param(fmt, specs, off == 16, id=f"{NAMES[fmt]}-plane{plane}+{off}"))
        for pad in (2, 16):
            out.append(pytest.param(fmt, [(0, pad, False)] + [(0, 16, False)] * (PLANES[fmt] - 1), pad == 16, id=f"{NAMES[fmt]}-y_row+{pad}"))
            out.append(pytest.param(fmt, [(0, 16, False)] + [(0, pad, False)] * (PLANES[fmt] - 1), pad == 16, id=f"{NAMES[fmt]}-c_row+{pad}"))
    return out


@pytest.mark.parametrize("fmt,specs,tables", _align_cases())
def test_alignment_dispatch(ctx, align_input, fmt, specs, tables):
    torch = pytest.importorskip("torch")
    planes, want, lds = align_input
    host = [np.ascontiguousarray(p).view(np.uint8) for p in ref.pack(fmt, *planes)]          # [n, rows, row bytes]
    views = [_device_view(torch, p, spec) for p, spec in zip(host, specs)]
    assert all(v.data_ptr() % 2 == 0 and v.stride(1) % 2 == 0 for v in views)
    got = _raw_picture(ctx, fmt, views, A_N, A_H, A_W)
    _check_plan(ctx, fmt, A_H, A_W, (TABLES if tables else SCALAR)[fmt], 14, lds[tables])
    _check_outputs(ctx, got, want, (NAMES[fmt], specs))
    assert ctx.stage_bytes() == 0 and ctx.stage_copies() == 0
    # a quarter turn has one fill whatever the alignment: the same views as the stored planes of a turned picture run the strip fill
    _raw_picture(ctx, fmt, views, A_N, A_H, A_W, 1)
    assert _plan(ctx)[P_KERNEL] == STRIP[fmt] and ctx.ingest_rotate() == 1


@pytest.mark.parametrize("pad,tables", [(8, True), (1, False)], ids=("rows+16B", "rows+2B"))
def test_row_padded_host_clips(ctx, align_input, pad, tables):
    planes, want, lds = align_input
    for fmt in NEW:
        clip = []
        for p in ref.pack(fmt, *planes):
            buf = np.zeros(p.shape[:2] + (p.shape[2] + pad,), np.uint16)
            buf[:, :, :p.shape[2]] = p
            clip.append(buf[:, :, :p.shape[2]])
        got = ctx.preprocess_picture(Pixels(tuple(clip), fmt))
        _check_plan(ctx, fmt, A_H, A_W, (TABLES if tables else SCALAR)[fmt], 14, lds[tables])
        _check_outputs(ctx, got, want, (NAMES[fmt], pad))
        assert ctx.stage_copies() == PLANES[fmt]
        spans = [p.strides[0] * (A_N - 1) + p.strides[1] * (p.shape[1] - 1) + 2 * p.shape[2] for p in clip]
        assert ctx.stage_bytes() == sum(spans)


# ---- 5: V first ---------------------------------------------------------------------------------------------------------------------------------
def test_v_first_i010_is_i010_with_the_chroma_pointers_exchanged(ctx, oracle, align_input):
    (y, u, v), want, lds = align_input
    got = ctx.preprocess_picture(Pixels((y, v, u), I010))
    _check_plan(ctx, I010, A_H, A_W, TABLES[I010], 14, lds[True])
    _check_outputs(ctx, got, _reference(oracle, ref.to_bgr(I010, (y, v, u), False)), "v first")
    assert not np.array_equal(got[0], want[0])


# ---- 6: frame lists -----------------------------------------------------------------------------------------------------------------------------
def _frames_of(clip, to=lambda a: np.array(a)):
    """the clip as per-frame tuples, every plane of every frame an allocation of its own"""
    return [tuple(to(pl[f]) for pl in clip) for f in range(len(clip[0]))]


@pytest.mark.parametrize("fmt", NEW, ids=lambda f: NAMES[f])
def test_host_lists_equal_the_strided_call(ctx, oracle, fmt):
    h, w = 34, 48
    planes = ref.random_planes10(3, h, w, seed=fmt + 7)
    order = [0, 2, 1, 0]                                       # shuffled, with a repeated frame
    clip = ref.pack(fmt, *planes)
    frames = _frames_of(clip)
    got = ctx.preprocess_frame_list([frames[i] for i in order], fmt, 0, True)
    assert ctx.ingest_list() == (1, 4)
    p = _plan(ctx)
    assert (p[P_KERNEL], ctx.ingest_format(), ctx.ingest_range(), ctx.ingest_rotate()) == (TABLES[fmt], fmt, 1, 0)
    ordered = tuple(pl[order] for pl in clip)
    _check_outputs(ctx, got, _reference(oracle, ref.to_bgr(fmt, ordered, True)), (NAMES[fmt], "host list"))
    assert ctx.stage_bytes() == 3 * 3 * h * w and ctx.stage_copies() == 3 * PLANES[fmt]      # the repeated frame crosses the link once
    strided = ctx.preprocess_picture(Pixels(ordered, fmt), 0, True)
    assert ctx.ingest_list() == (0, 0) and _plan(ctx)[P_LDS] == p[P_LDS]
    _same(got, strided, NAMES[fmt])
    # turned: the strip fill from a table of plane pointers
    got = ctx.preprocess_frame_list([frames[i] for i in order], fmt, 3)
    assert (_plan(ctx)[P_KERNEL], ctx.ingest_rotate(), ctx.ingest_list()) == (STRIP[fmt], 3, (1, 4))
    _same(got, ctx.preprocess_picture(ref.narrowed_nv12(fmt, ordered), 3), (NAMES[fmt], "turned list"))


@pytest.mark.parametrize("fmt", NEW, ids=lambda f: NAMES[f])
@pytest.mark.parametrize("misalign", (False, True), ids=("aligned", "one_frame_off"))
def test_device_lists(ctx, oracle, fmt, misalign):
    """torch device frames (int16: the same bits), each plane its own tensor, listed in another order than they were allocated in; one plane
    of one frame that is only 8-byte aligned sends the whole list through the scalar fill"""
    torch = pytest.importorskip("torch")
    h, w = 34, 48
    planes = ref.random_planes10(3, h, w, seed=fmt + 11)
    clip = ref.pack(fmt, *planes)
    frames = _frames_of(clip, lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to("cuda:0"))
    if misalign:
        last = frames[1][-1]
        flat = torch.zeros(last.numel() + 32, dtype=torch.int16, device="cuda:0")
        off = (-flat.data_ptr() % 16) // 2 + 4                 # 8 mod 16: enough for I420's chroma loads, not for I010's
        moved = flat[off:off + last.numel()].view(last.shape)
        moved.copy_(last)
        assert moved.data_ptr() % 16 == 8
        frames[1] = frames[1][:-1] + (moved,)
    torch.cuda.synchronize()
    order = [2, 0, 1, 2]
    got = ctx.preprocess_frame_list([frames[i] for i in order], fmt)
    assert ctx.ingest_list() == (1, 4)
    assert (_plan(ctx)[P_KERNEL], ctx.ingest_format(), ctx.ingest_range(), ctx.ingest_rotate()) == ((SCALAR if misalign else TABLES)[fmt], fmt, 0, 0)
    _check_outputs(ctx, got, _reference(oracle, ref.to_bgr(fmt, tuple(pl[order] for pl in clip), False)), (NAMES[fmt], "device list", misalign))
    assert ctx.stage_bytes() == 0 and ctx.stage_copies() == 0


# ---- 7, 8: batches, the asynchronous form -------------------------------------------------------------------------------------------------------
def _mixed_clips():
    """P010 and I010 clips with NV12 and BGR clips and a rotated, full-range one; two geometries
    -> (clips, rotations, ranges, the BGR twin of every 10-bit clip or None)"""
    rng = np.random.default_rng(5)
    clips, rotates, ranges, twins = [], [], [], []
    for i, (fmt, rot, full) in enumerate(((P010, 0, False), (I010, 0, True), (P010, 1, True), (I010, 3, False), (I010, 2, False))):
        h, w = ((34, 48), (36, 80))[i & 1]
        disp = ref.random_planes10(2 + (i & 1), h, w, seed=100 + i)
        clips.append(Pixels(ref.pack(fmt, *_turn(disp, rot)), fmt))
        rotates.append(rot)
        ranges.append(full)
        twins.append(ref.to_bgr(fmt, ref.pack(fmt, *disp), full))
    y = rng.integers(0, 256, (2, 36, 80), dtype=np.uint8)
    clips += [(y, rng.integers(0, 256, (2, 18, 80), dtype=np.uint8)), synth.random_frames(3, 34, 48, seed=104)]
    rotates += [0, 0]
    ranges += [True, False]
    twins += [None, None]
    return clips, rotates, ranges, twins


def test_mixed_batches(ctx):
    clips, rotates, ranges, twins = _mixed_clips()
    try:
        for mode in (1, 0):
            ctx.set_option("fb_mode", mode)
            alone = [ctx.analyze_pictures([c], [k], [r])[0] for c, k, r in zip(clips, rotates, ranges)]
            for c, t, a in zip(clips, twins, alone):
                if t is not None:                              # a 10-bit clip alone equals the BGR entry point on the definition's frames
                    _same_records(a, ctx.analyze_frames(t), (mode, NAMES[c.fmt], "BGR twin"))
            got = ctx.analyze_pictures(clips, rotates, ranges)
            assert len(got) == len(clips)
            for i, (g, a) in enumerate(zip(got, alone)):
                _same_records(g, a, (mode, i))
    finally:
        ctx.set_option("fb_mode", 1)


def test_async_and_a_call_made_while_one_is_pending(ctx, oracle, align_input):
    clips, rotates, ranges, _ = _mixed_clips()
    clips, rotates, ranges = clips[:4], rotates[:4], ranges[:4]
    alone = [ctx.analyze_pictures([c], [k], [r])[0] for c, k, r in zip(clips, rotates, ranges)]
    rec = np.zeros(sum(len(a) for a in alone), _lib.RECORD_DTYPE)
    keep, counts = ctx.analyze_pictures_async(clips, rec, rotates, ranges)
    assert counts == [len(a) for a in alone]
    # a 10-bit call made while that one is pending: it drains the pending call first, and is itself right
    planes, want, lds = align_input
    got = ctx.preprocess_picture(Pixels(ref.pack(P010, *planes), P010))
    for i, (g, a) in enumerate(zip(np.split(rec, np.cumsum(counts)[:-1]), alone)):
        _same_records(g, a, ("async", i))
    _check_plan(ctx, P010, A_H, A_W, TABLES[P010], 14, lds[True])
    _check_outputs(ctx, got, want, "while pending")
    del keep
    # the list form, drained by synchronize()
    lists = [(_frames_of(c.data), c.fmt) for c in clips]
    rec2 = np.zeros_like(rec)
    keep, counts2 = ctx.analyze_frame_lists_async(lists, rec2, rotates, ranges)
    ctx.synchronize()
    assert counts2 == counts and rec2.tobytes() == rec.tobytes()
    del keep


# ---- 9: streaming -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,rotate,full_range", [(P010, 1, False), (I010, 0, True)], ids=("p010-turned", "i010-full"))
def test_records_stream_across_a_chunk_boundary(fmt, rotate, full_range):
    n, h, w = 5, 34, 48
    disp = ref.random_planes10(n, h, w, seed=fmt)
    clip = ref.pack(fmt, *_turn(disp, rotate))
    with avd_hip.Context(0) as c:
        want = c.analyze_pictures([Pixels(clip, fmt)], [rotate], [full_range])[0]
        fa = avd_hip.FrameAnalyzer(chunk=2, ctx=c)             # chunks of 2 + carry: 2, 2, 1
        stream = fa.records_stream_p010 if fmt == P010 else fa.records_stream_i010
        got = stream(iter(_frames_of(clip, lambda a: a)), rotate, full_range)        # views of the stack: nothing is copied, nothing narrowed
        assert got.tobytes() == want.tobytes()
        # the last chunk: the carry frame and one more
        assert (c.ingest_format(), c.ingest_list(), c.ingest_rotate(), c.ingest_range()) == (fmt, (1, 2), rotate, int(full_range))
        assert c.stage_bytes() == 2 * 3 * h * w
        assert got.tobytes() == c.analyze_frames(ref.to_bgr(fmt, ref.pack(fmt, *disp), full_range)).tobytes()


# ---- 10: host staging ---------------------------------------------------------------------------------------------------------------------------
def test_stage_bytes_and_copies(ctx, oracle):
    n, h, w = 3, 34, 48
    planes = ref.random_planes10(n, h, w, seed=77)
    want = _reference(oracle, ref.to_bgr(I010, planes, False))
    got = ctx.preprocess_picture(Pixels(ref.pack(P010, *planes), P010))
    assert (ctx.stage_copies(), ctx.stage_bytes()) == (2, 3 * n * h * w)
    _check_outputs(ctx, got, want, "p010")
    got = ctx.preprocess_picture(Pixels(planes, I010))          # separately allocated planes
    assert (ctx.stage_copies(), ctx.stage_bytes()) == (3, 3 * n * h * w)
    # a dense yuv420p10le frame stack: Y | U | V of a frame adjacent, frame after frame -- ONE copy, and still the table fill
    fs = 3 * h * w // 2                                        # words per frame
    flat = np.zeros(n * fs, np.uint16)
    strided = lambda o, shape: np.lib.stride_tricks.as_strided(flat[o:], (n,) + shape, (2 * fs, 2 * shape[1], 2))
    dense = (strided(0, (h, w)), strided(h * w, (h // 2, w // 2)), strided(h * w + h * w // 4, (h // 2, w // 2)))
    for dst, src in zip(dense, planes):
        dst[...] = src
    got = ctx.preprocess_picture(Pixels(dense, I010))
    assert (ctx.stage_copies(), ctx.stage_bytes()) == (1, 3 * n * h * w)
    assert (_plan(ctx)[P_KERNEL], ctx.ingest_format()) == (TABLES[I010], I010)
    _check_outputs(ctx, got, want, "dense stack")


# ---- 11: refusals through the real entry points -------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    torch = pytest.importorskip("torch")
    B = synth.random_frames(2, 34, 48, seed=3)
    ctx.preprocess_bgr(B)
    assert ctx.ingest_format() == BGR
    zeros = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(avd_hip.AvdError, match=r"avd status -4: P010 needs even width and height"):
        ctx.preprocess_picture(Pixels((np.zeros((2, 34, 35), np.uint16), np.zeros((2, 17, 35), np.uint16)), P010))
    with pytest.raises(avd_hip.AvdError, match=r"avd status -4: I010 needs even width and height"):
        ctx.preprocess_frame_list([(np.zeros((35, 48), np.uint16), np.zeros((17, 24), np.uint16), np.zeros((17, 24), np.uint16))], I010)
    with pytest.raises(avd_hip.AvdError, match=r"avd status -4: frame smaller than 32x32"):
        ctx.analyze_pictures([B, Pixels((np.zeros((2, 30, 48), np.uint16), np.zeros((2, 15, 48), np.uint16)), P010)])
    # what the binding cannot produce: the descriptor written out by hand
    views = [zeros(2, 34, 96), zeros(2, 17, 48), zeros(2, 17, 64)]
    with pytest.raises(avd_hip.AvdError, match=r"avd status -1: the U and V planes of an I010 picture share their strides"):
        _raw_picture(ctx, I010, views, 2, 34, 48)
    with pytest.raises(avd_hip.AvdError, match=r"avd status -1: strides smaller than the P010 planes"):
        _raw_picture(ctx, P010, [zeros(2, 34, 48), zeros(2, 17, 96)], 2, 34, 48)         # rows of w bytes: an 8-bit plane
    with pytest.raises(avd_hip.AvdError, match=r"avd status -1: strides smaller than the I010 planes"):
        _raw_picture(ctx, I010, [zeros(2, 34, 96), zeros(2, 17, 24), zeros(2, 17, 24)], 2, 34, 48)
    flat = zeros(2 * 34 * 96 + 16)
    odd = flat[1:1 + 2 * 34 * 96].view(2, 34, 96)
    assert odd.data_ptr() % 2 == 1
    for fmt, rest in ((P010, [zeros(2, 17, 96)]), (I010, [zeros(2, 17, 48), zeros(2, 17, 48)])):
        with pytest.raises(avd_hip.AvdError, match=r"avd status -1: 16-bit samples need 2-byte aligned planes and strides"):
            _raw_picture(ctx, fmt, [odd] + rest, 2, 34, 48)
        with pytest.raises(avd_hip.AvdError, match=r"avd status -1: 16-bit samples need 2-byte aligned planes and strides"):
            _raw_picture(ctx, fmt, [zeros(2, 34, 97)[:, :, :96]] + rest, 2, 34, 48)
    for layout in (0x24, 0x2F, 0x32, 0x3F):
        with pytest.raises(avd_hip.AvdError, match=r"avd status -1: bad avd_picture.format"):
            _raw_picture(ctx, layout, views[:1] + views[1:2] * 2, 2, 34, 48)
    assert ctx.ingest_format() == BGR                          # still the launch before the refusals
    planes = ref.random_planes10(2, 34, 48, seed=4)
    ctx.preprocess_picture(Pixels(planes, I010))
    assert ctx.ingest_format() == I010
