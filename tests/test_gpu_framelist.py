"""Clips as lists of separately allocated frames (include/avd_frame_list.h) on the GPU.

Definition under test: every output of a list equals, BIT FOR BIT and in both fb_modes, the output of the format's own strided entry point
(avd_picture) on the same frames stacked in list order -- for every fill, rotation and range, for host and device frames, for frames in any
address order and frames that repeat.  There is no tolerance in this file.  The strided results are formed once per case from the stacked
frames and shared by the host and the device form; one case per format is compared with the CPU oracle directly.

n = 4 frames of seeded noise.  The geometries are the smallest that reach each kernel once: 4:2:0 stored 48 x 64 (the table fills) and 50 x 70
(even, w % 16 != 0: the scalar fills), both with rotate 1, 2, 3 (strip and flipped fills); BGR 67 x 101 (scalar) and the first bgr_vec16 and
bgr_staged width of tests/test_gpu_ingest_plan.py's BGR_PLANS at its smallest height.  Every case asserts the kernel that ran from
"ingest_plan" and "ingest_list" == (1, n).

Host frames are cut out of one pool buffer at shuffled, gapped places (a decoder's frame pool): address order, alignment and the number of
staging copies are then the test's and not the allocator's.  Device frames are separate torch tensors allocated in another order than the
list's."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import avd_hip  # noqa: E402
from avd_hip import AvdError, _lib, analyzer, synth  # noqa: E402
from tests import test_framelist_host as host_rows  # noqa: E402
from tests import yuv_tables_reference as ref  # noqa: E402
from tests.test_gpu_ingest_plan import BGR_PLANS, BGR_STAGED, BGR_VEC16, _heights  # noqa: E402

BGR, NV12, I420 = _lib.AVD_FMT_BGR24, _lib.AVD_FMT_NV12, _lib.AVD_FMT_I420
NAMES = {BGR: "bgr", NV12: "nv12", I420: "i420"}
PLANES = {BGR: 1, NV12: 2, I420: 3}
KERNEL_NAMES = ("bgr_scalar", "bgr_vec16", "bgr_staged", "nv12_scalar", "nv12_tables", "i420_scalar", "i420_tables", "nv12_strip", "i420_strip")
SCALAR, TABLES, STRIP = {NV12: 3, I420: 5}, {NV12: 4, I420: 6}, {NV12: 7, I420: 8}
N = 4
ORDER = [2, 0, 3, 1]                                     # list position -> place in the pool / allocation rank
OUT = ("small320", "hash1024", "lap_sum", "lap_sumsq")


def _kernel(ctx):
    return KERNEL_NAMES[ctx.debug_fetch("ingest_plan", (8,), np.int32)[7]]


def _stack(fmt, n, h, w, seed):
    """the stacked planes of n frames of noise: (bgr,), (y, uv) or (y, u, v)"""
    rng = np.random.default_rng(seed)
    shapes = {BGR: [(n, h, w, 3)], NV12: [(n, h, w), (n, h // 2, w)], I420: [(n, h, w), (n, h // 2, w // 2), (n, h // 2, w // 2)]}[fmt]
    return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in shapes)


def _clip(fmt, stack):
    """what the strided entry points take"""
    return stack[0] if fmt == BGR else tuple(stack)


def _item(fmt, planes):
    return planes[0] if fmt == BGR else tuple(planes)


def _pool_frames(fmt, stack, order=ORDER, gap=4096, lead=0):
    """-> (per-frame planes cut out of ONE host buffer: plane p of frame f at slot order[f] of plane p's region, `gap` bytes between slots,
    every slot on a 64-byte boundary + lead; the buffer)"""
    n = stack[0].shape[0]
    sizes = [int(np.prod(p.shape[1:])) for p in stack]
    slot = [(s + gap + 63) // 64 * 64 for s in sizes]
    pool = np.zeros(sum(sl * n for sl in slot) + 128, np.uint8)
    base = -pool.ctypes.data % 64 + lead
    frames = []
    for f in range(n):
        planes = []
        for p, plane in enumerate(stack):
            o = base + sum(slot[:p]) * n + slot[p] * order[f]
            view = pool[o:o + sizes[p]].reshape(plane.shape[1:])
            view[...] = plane[f]
            planes.append(view)
        frames.append(_item(fmt, planes))
    return frames, pool


def _device_frames(torch, fmt, stack, order=ORDER):
    """separate device tensors, allocated in `order` and not in list order"""
    n = stack[0].shape[0]
    frames = [None] * n
    for f in sorted(range(n), key=lambda i: order[i]):
        frames[f] = _item(fmt, [torch.from_numpy(np.ascontiguousarray(p[f])).to("cuda:0") for p in stack])
    return frames


def _equal(got, want, tag):
    for name, a, b in zip(OUT, got, want):
        assert np.array_equal(a, b), (tag, name, int(np.count_nonzero(np.asarray(a) != np.asarray(b))))


def _plane_bytes(stack):
    return sum(int(np.prod(p.shape[1:])) for p in stack)


# ---- the cases: (format, stored h, w, rotate, kernel) ------------------------------------------------------------------------------------------
def _smallest(kernel):
    _, _, widths, rows = next(p for p in BGR_PLANS if p[0] == kernel)
    rows = rows[0] if isinstance(rows, tuple) else rows
    return min(_heights(rows)), widths[0]


CASES = [(BGR, 67, 101, 0, "bgr_scalar"), (BGR, *_smallest(BGR_VEC16), 0, "bgr_vec16"), (BGR, *_smallest(BGR_STAGED), 0, "bgr_staged")]
for _fmt in (NV12, I420):
    for _k in range(4):
        CASES.append((_fmt, 48, 64, _k, KERNEL_NAMES[(STRIP if _k & 1 else TABLES)[_fmt]]))
        CASES.append((_fmt, 50, 70, _k, KERNEL_NAMES[(STRIP if _k & 1 else SCALAR)[_fmt]]))
CASE_IDS = [f"{NAMES[c[0]]}-{c[1]}x{c[2]}-k{c[3]}-{c[4]}" for c in CASES]

_refs = {}


def _reference(ctx, fmt, h, w, k, full=False, stack=None, key=None):
    """-> (the stacked planes, the STRIDED entry points' preprocess outputs and records on them); formed once per case and left unchanged"""
    key = key or (fmt, h, w, k, full)
    if key not in _refs:
        stack = stack if stack is not None else _stack(fmt, N, h, w, seed=1000 * fmt + 10 * h + w + k)
        pre = ctx.preprocess_picture(_clip(fmt, stack), k, full)
        rec = ctx.analyze_pictures([_clip(fmt, stack)], [k], [full])[0]
        assert ctx.ingest_list() == (0, 0)                                       # a strided clip takes no table
        _refs[key] = (stack, pre, rec)
    return _refs[key]


def _run_list(ctx, fmt, frames, k, full, want, kernel, n, tag):
    pre, rec = want
    got = ctx.preprocess_frame_list(frames, fmt, k, full)
    assert (_kernel(ctx), ctx.ingest_list(), ctx.ingest_rotate()) == (kernel, (1, n), k), tag
    _equal(got, pre, tag)
    got = ctx.analyze_frame_lists([(frames, fmt)], [k], [full])[0]
    assert (_kernel(ctx), ctx.ingest_list()) == (kernel, (1, n)), tag
    assert got.tobytes() == rec.tobytes(), (tag, got, rec)


# ---- 1: separately allocated frames, list order != allocation order -----------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("fmt,h,w,k,kernel", CASES, ids=CASE_IDS)
def test_separately_allocated_frames(ctx, fmt, h, w, k, kernel, mem):
    stack, pre, rec = _reference(ctx, fmt, h, w, k)
    if mem == "host":
        frames, pool = _pool_frames(fmt, stack)
        first = [(f if fmt == BGR else f[0]).ctypes.data for f in frames]
        assert first != sorted(first) and first != sorted(first, reverse=True)   # neither ascending nor descending
    else:
        torch = pytest.importorskip("torch")
        frames = _device_frames(torch, fmt, stack)
    _run_list(ctx, fmt, frames, k, False, (pre, rec), kernel, N, (NAMES[fmt], h, w, k, mem))
    if mem == "host":
        assert (ctx.stage_bytes(), ctx.stage_copies()) == (N * _plane_bytes(stack), N * PLANES[fmt])
    else:
        assert (ctx.stage_bytes(), ctx.stage_copies()) == (0, 0)


@pytest.mark.parametrize("fmt,h,w", [(BGR, 67, 101), (NV12, 48, 64), (I420, 48, 64)], ids=["bgr", "nv12", "i420"])
def test_a_list_against_the_oracle(ctx, oracle, fmt, h, w):
    stack = _reference(ctx, fmt, h, w, 0)[0]
    if fmt == BGR:
        bgr = stack[0]
    else:
        y, uv = stack if fmt == NV12 else synth.i420_to_nv12(*stack)
        bgr = oracle.nv12_to_bgr(y, uv)
    frames, pool = _pool_frames(fmt, stack)
    got = ctx.preprocess_frame_list(frames, fmt)
    assert ctx.ingest_list() == (1, N)
    _equal(got, oracle.preprocess_bgr(bgr), (NAMES[fmt], "oracle"))
    try:
        ctx.set_option("fb_mode", 0)                                             # the exact kernels: bit-identical to the oracle everywhere
        rec = ctx.analyze_frame_lists([(frames, fmt)])[0]
    finally:
        ctx.set_option("fb_mode", 1)
    small, hsh, s, q = oracle.preprocess_bgr(bgr)
    fm, fv = oracle.farneback_pairs(small)
    assert rec["lap_sum"].tolist() == s.tolist() and rec["lap_sumsq"].tolist() == q.tolist()
    assert rec["ham"].tolist() == [-1] + [int(np.sum(hsh[i] ^ hsh[i - 1])) for i in range(1, N)]
    assert rec["flow_mean"][1:].tobytes() == fm.tobytes() and rec["flow_var"][1:].tobytes() == fv.tobytes()


# ---- 2: views of one stacked array ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("fmt,h,w,k,kernel", [c for c in CASES if c[3] in (0, 1)], ids=[i for c, i in zip(CASES, CASE_IDS) if c[3] in (0, 1)])
def test_views_of_one_stack(ctx, fmt, h, w, k, kernel, mem):
    stack, pre, rec = _reference(ctx, fmt, h, w, k)
    if fmt == I420:                                                             # one buffer per clip: Y, U, V of a frame adjacent
        y, u, v = stack
        flat = np.concatenate([y.reshape(N, -1), u.reshape(N, -1), v.reshape(N, -1)], axis=1).copy()
        a, b = y[0].size, y[0].size + u[0].size
        planes = (flat[:, :a].reshape(y.shape), flat[:, a:b].reshape(u.shape), flat[:, b:].reshape(v.shape))
    else:
        planes = tuple(p.copy() for p in stack)
    if mem == "device":
        torch = pytest.importorskip("torch")
        if fmt == I420:
            dflat = torch.from_numpy(flat).to("cuda:0")
            planes = (dflat[:, :a].unflatten(1, y.shape[1:]), dflat[:, a:b].unflatten(1, u.shape[1:]), dflat[:, b:].unflatten(1, v.shape[1:]))
        else:
            planes = tuple(torch.from_numpy(p).to("cuda:0") for p in planes)
    else:
        ctx.preprocess_picture(_clip(fmt, planes), k)
        strided_bytes = ctx.stage_bytes()
        assert strided_bytes == N * _plane_bytes(stack)
    frames = [_item(fmt, [p[f] for p in planes]) for f in range(N)]
    _run_list(ctx, fmt, frames, k, False, (pre, rec), kernel, N, (NAMES[fmt], h, w, k, mem, "views"))
    if mem == "host":
        assert ctx.stage_bytes() == strided_bytes
        assert ctx.stage_copies() == (2 if fmt == NV12 else 1)                   # NV12: a Y stack and a chroma stack, as the strided clip
    else:
        assert (ctx.stage_bytes(), ctx.stage_copies()) == (0, 0)


# ---- 3: a frame that appears twice ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("fmt,h,w,kernel", [(BGR, 67, 101, "bgr_scalar"), (NV12, 48, 64, "nv12_tables"), (I420, 48, 64, "i420_tables")],
                         ids=["bgr", "nv12", "i420"])
def test_a_repeated_frame(ctx, fmt, h, w, kernel, mem):
    base = _reference(ctx, fmt, h, w, 0)[0]
    dup = tuple(p[[0, 1, 1, 3]] for p in base)                                   # the stacked clip with frame 1 duplicated
    stack, pre, rec = _reference(ctx, fmt, h, w, 0, stack=dup, key=(fmt, h, w, "dup"))
    if mem == "host":
        frames, pool = _pool_frames(fmt, base)
    else:
        torch = pytest.importorskip("torch")
        frames = _device_frames(torch, fmt, base)
    frames = [frames[0], frames[1], frames[1], frames[3]]
    _run_list(ctx, fmt, frames, 0, False, (pre, rec), kernel, N, (NAMES[fmt], mem, "repeat"))
    assert rec["ham"][2] == 0
    if mem == "host":
        assert (ctx.stage_bytes(), ctx.stage_copies()) == (3 * _plane_bytes(base), 3 * PLANES[fmt])


# ---- 4: one frame off by one byte in an otherwise aligned list ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("fmt", [BGR, NV12, I420], ids=["bgr", "nv12", "i420"])
def test_one_frame_off_by_one_byte(ctx, fmt, mem):
    """Frame 2's first plane is the view at offset 1 of a larger buffer.  Device: that frame alone takes the 16-byte fills from the whole list.
    Host: a frame is judged where it is STAGED, and a span of its own lands on a 256-byte boundary -- the view at offset 1 runs the vector
    fill; the misalignment survives staging where frame 1 is the view at offset 0 of the same buffer (overlapping windows: one merged span,
    frame 2 one byte into it), which is the host list of this case."""
    h, w = 48, 64
    aligned, scalar = {BGR: ("bgr_staged", "bgr_scalar"), NV12: ("nv12_tables", "nv12_scalar"), I420: ("i420_tables", "i420_scalar")}[fmt]
    base = _stack(fmt, N, h, w, seed=77 + fmt)
    size = base[0][0].size
    rng = np.random.default_rng(5)
    big = rng.integers(0, 256, size + 16, dtype=np.uint8)
    shape = base[0].shape[1:]
    first = base[0].copy()
    first[1], first[2] = big[:size].reshape(shape), big[1:size + 1].reshape(shape)
    stack = (first,) + tuple(base[1:])
    pre = ctx.preprocess_picture(_clip(fmt, stack), 0)
    rec = ctx.analyze_pictures([_clip(fmt, stack)])[0]
    assert _kernel(ctx) == aligned
    if mem == "host":
        frames, pool = _pool_frames(fmt, stack)
        hold = np.zeros(size + 16 + 64, np.uint8)
        o = -hold.ctypes.data % 64
        hold[o:o + size + 16] = big
        rest = lambda f: () if fmt == BGR else tuple(frames[f][1:])
        lone = list(frames)
        lone[2] = _item(fmt, (hold[o + 1:o + 1 + size].reshape(shape),) + rest(2))
        assert (lone[2] if fmt == BGR else lone[2][0]).ctypes.data % 16 == 1
        _run_list(ctx, fmt, lone, 0, False, (pre, rec), aligned, N, (NAMES[fmt], "host", "lone frame: re-aligned by its staging copy"))
        frames[1] = _item(fmt, (hold[o:o + size].reshape(shape),) + rest(1))
        frames[2] = lone[2]
    else:
        torch = pytest.importorskip("torch")
        frames = _device_frames(torch, fmt, stack)
        dbig = torch.from_numpy(big).to("cuda:0")
        assert dbig.data_ptr() % 16 == 0
        view = dbig[1:size + 1].unflatten(0, shape)
        frames[2] = view if fmt == BGR else (view,) + tuple(frames[2][1:])
    _run_list(ctx, fmt, frames, 0, False, (pre, rec), scalar, N, (NAMES[fmt], mem, "off by one"))


# ---- 5: row-padded frames, full range ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("fmt", [NV12, I420], ids=["nv12", "i420"])
@pytest.mark.parametrize("k", [0, 1])
def test_row_padded_full_range_frames(ctx, oracle, fmt, k, mem):
    h, w, pad = 48, 64, 16
    n = ref.enum_frames(h, w) + 1                                               # the enumeration reaches both ends of the full-range table window
    assert n == N
    y, uv = ref.enum_planes(n, h, w, seed=h + w)
    stack = (y, uv) if fmt == NV12 else synth.nv12_to_i420(y, uv)
    stack, pre, rec = _reference(ctx, fmt, h, w, k, True, stack=stack, key=(fmt, "enum", k))
    assert ctx.ingest_range() == 1
    if k == 0:
        _equal(pre, oracle.preprocess_bgr(ref.nv12_to_bgr(y, uv, True)), "the full-range restatement")
        assert not np.array_equal(pre[0], ctx.preprocess_picture(_clip(fmt, stack), 0, False)[0])      # the flag is not ignored
    padded = []
    for f in range(n):
        planes = []
        for p in stack:
            wide = np.zeros((p.shape[1], p.shape[2] + pad), np.uint8)
            wide[:, :p.shape[2]] = p[f]
            planes.append(wide)
        padded.append(planes)
    if mem == "host":
        frames = [tuple(p[:, :p.shape[1] - pad] for p in planes) for planes in padded]
    else:
        torch = pytest.importorskip("torch")
        frames = [tuple(torch.from_numpy(p).to("cuda:0")[:, :p.shape[1] - pad] for p in planes) for planes in padded]
    kernel = KERNEL_NAMES[(STRIP if k else TABLES)[fmt]]
    _run_list(ctx, fmt, frames, k, True, (pre, rec), kernel, n, (NAMES[fmt], k, mem, "padded"))
    assert ctx.ingest_range() == 1
    if mem == "host":
        spans = sum((p.shape[2] + pad) * (p.shape[1] - 1) + p.shape[2] for p in stack)
        assert (ctx.stage_bytes(), ctx.stage_copies()) == (n * spans, n * PLANES[fmt])
    with pytest.raises(ValueError, match="share their row strides"):
        ctx.preprocess_frame_list(frames[:1] + [tuple(np.ascontiguousarray(p[1]) for p in stack)] if mem == "host" else
                                  frames[:1] + [tuple(p.contiguous() for p in frames[1])], fmt, k, True)


# ---- 6: a batch of lists ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 0], ids=["fast", "exact"])
def test_a_batch_of_lists(ctx, mode):
    specs = [(NV12, 64, 48, 1, True, 4), (I420, 48, 64, 0, False, 0), (BGR, 67, 101, 0, False, 1), (I420, 50, 70, 2, False, 4), (NV12, 48, 64, 0, False, 3)]
    stacks = [_stack(f, n, h, w, seed=300 + i) for i, (f, h, w, k, fr, n) in enumerate(specs)]
    hold = [_pool_frames(f, s, order=list(range(n))[::-1]) for (f, h, w, k, fr, n), s in zip(specs, stacks)]
    lists = [(frames, f) for (frames, _), (f, *_) in zip(hold, specs)]
    try:
        import torch
        lists[4] = (_device_frames(torch, NV12, stacks[4], order=[1, 2, 0]), NV12)      # host and device lists in one call
    except ImportError:
        pass
    turns, ranges = [s[3] for s in specs], [s[4] for s in specs]
    try:
        ctx.set_option("fb_mode", mode)
        single = [ctx.analyze_frame_lists([l], [k], [fr])[0] for l, k, fr in zip(lists, turns, ranges)]
        assert [len(r) for r in single] == [4, 0, 1, 4, 3]
        for i, (f, h, w, k, fr, n) in enumerate(specs):
            if n:
                assert single[i].tobytes() == ctx.analyze_pictures([_clip(f, stacks[i])], [k], [fr])[0].tobytes(), (mode, i)
        assert single[2]["ham"].tolist() == [-1] and single[2]["flow_mean"].tolist() == [0.0]
        got = ctx.analyze_frame_lists(lists, turns, ranges)
        assert [len(r) for r in got] == [4, 0, 1, 4, 3]
        assert np.concatenate(got).tobytes() == np.concatenate(single).tobytes()
        assert ctx.ingest_list() == (1, 3) and _kernel(ctx) == "nv12_tables"      # the last list's launch
        assert all(r["ham"][0] == -1 for r in got if len(r))
        assert ctx.analyze_frame_lists([lists[1]], [0], [False])[0].size == 0 and ctx.analyze_frame_lists([]) == []
    finally:
        ctx.set_option("fb_mode", 1)


# ---- 7: asynchronous ----------------------------------------------------------------------------------------------------------------------------
def test_async_owns_its_pointer_arrays_and_is_drained_by_another_call(ctx):
    specs = [(NV12, 48, 64, 3), (BGR, 67, 101, 0), (I420, 48, 64, 2)]
    stacks = [_stack(f, N, h, w, seed=500 + i) for i, (f, h, w, k) in enumerate(specs)]
    hold = [_pool_frames(f, s) for (f, *_), s in zip(specs, stacks)]
    lists = [(frames, f) for (frames, _), (f, *_) in zip(hold, specs)]
    turns = [s[3] for s in specs]
    want = np.concatenate(ctx.analyze_frame_lists(lists, turns))
    # the pointer arrays are overwritten as soon as the call has returned
    rec = np.zeros(3 * N, avd_hip.RECORD_DTYPE)
    keep, counts = ctx.analyze_frame_lists_async(lists, rec, turns)
    assert counts == [N] * 3
    for arrays, _ in keep:
        for a in arrays:
            ctypes.memset(a, 0xEE, ctypes.sizeof(a))
    ctx.synchronize()
    assert rec.tobytes() == want.tobytes()
    # a call of another kind drains the pending one: its records are there before synchronize()
    other = _stack(BGR, 2, 40, 48, seed=9)[0]
    rec = np.zeros(3 * N, avd_hip.RECORD_DTYPE)
    keep, counts = ctx.analyze_frame_lists_async(lists, rec, turns)
    assert not rec["lap_sumsq"].any()
    pre = ctx.preprocess_bgr(other)
    assert rec.tobytes() == want.tobytes()
    assert ctx.ingest_list() == (0, 0) and len(pre[2]) == 2
    ctx.synchronize()
    # and a list call drains a pending strided one
    rec2 = np.zeros(2, avd_hip.RECORD_DTYPE)
    keep2 = ctx.analyze_frames_async(other, rec2)
    got = np.concatenate(ctx.analyze_frame_lists(lists, turns))
    assert rec2.tobytes() == ctx.analyze_frames(other).tobytes() and got.tobytes() == want.tobytes()
    del keep, keep2


# ---- 8: the streaming analyzer stacks nothing -----------------------------------------------------------------------------------------------------
def test_streaming_takes_frames_where_they_lie(ctx, monkeypatch):
    n, h, w = 8, 48, 64
    fa = analyzer.FrameAnalyzer(ctx=ctx, chunk=3)
    bgr = _stack(BGR, n, 67, 101, seed=61)[0]
    y, uv = _stack(NV12, n, h, w, seed=62)
    _, u, v = synth.nv12_to_i420(y, uv)
    want = [ctx.analyze_frames(bgr), ctx.analyze_frames_nv12(y, uv), ctx.analyze_frames_i420(y, u, v), ctx.analyze_frames_i420(y, u, v, rotate=1, full_range=True)]
    calls = []
    real = np.stack
    monkeypatch.setattr(np, "stack", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    own = lambda a: np.array(a, copy=True)                                       # every frame an allocation of its own
    got = [fa.records_stream(own(bgr[i]) for i in range(n)),
           fa.records_stream_nv12((own(y[i]), own(uv[i])) for i in range(n)),
           fa.records_stream_i420((own(y[i]), own(u[i]), own(v[i])) for i in range(n)),
           fa.records_stream_i420(((own(y[i]), own(u[i]), own(v[i])) for i in range(n)), rotate=1, full_range=True)]
    assert ctx.ingest_list() == (1, 3)                                           # the last chunk: the carry frame and two new ones
    # row-padded frames of one pitch go through as they lie: no dense copy is made of them either
    copies = []
    real_dense = np.ascontiguousarray
    monkeypatch.setattr(np, "ascontiguousarray", lambda *a, **kw: copies.append(1) or real_dense(*a, **kw))

    def padded(p):
        wide = np.zeros((p.shape[0], p.shape[1] + 16), np.uint8)
        wide[:, :p.shape[1]] = p
        return wide[:, :p.shape[1]]
    got.append(fa.records_stream_nv12((padded(y[i]), padded(uv[i])) for i in range(n)))
    want.append(want[1])
    assert ctx.stage_bytes() == 3 * ((w + 16) * (h - 1) + w + (w + 16) * (h // 2 - 1) + w)
    monkeypatch.undo()
    assert not calls and not copies
    for g, wnt in zip(got, want):
        assert g.tobytes() == wnt.tobytes()
    assert fa.records_stream(iter(())).size == 0


# ---- 9: every refusal row through the C-ABI -------------------------------------------------------------------------------------------------------
def _descriptor(c, keep):
    L = _lib.AvdFrameList()
    L.struct_size, L.format, L.mem, L.n, L.h, L.w = ctypes.sizeof(L) + c["size_delta"], c["fmt"], c["mem"], c["n"], c["h"], c["w"]
    L.rotate, L.reserved = c["rotate"], c["reserved"]
    for p in range(3):
        L.row_stride[p] = c["rows"][p]
        m = max(c["n"], 0)
        arr = (ctypes.c_void_p * max(m, 1))(*(c["addrs"][p] + [0] * m)[:m])
        keep.append(arr)
        L.plane[p] = None if (c["null_arrays"] >> p) & 1 else ctypes.cast(arr, ctypes.c_void_p)
    return L


def test_every_refusal_row_through_the_c_abi(ctx):
    stack = _stack(NV12, N, 48, 64, seed=3)
    frames, pool = _pool_frames(NV12, stack)
    ctx.preprocess_frame_list(frames, NV12, 2, True)                             # the call before
    state = lambda: (ctx.debug_fetch("ingest_plan", (8,), np.int32).tolist(), ctx.ingest_list(), ctx.ingest_rotate(), ctx.ingest_range(),
                     ctx.stage_bytes(), ctx.stage_copies())
    before = state()
    assert before[1:] == ((1, N), 2, 1, N * _plane_bytes(stack), 2 * N)
    L, H = ctx._L, ctx._h
    rec = np.zeros(16, avd_hip.RECORD_DTYPE)
    small = np.empty((4, 320, 320), np.uint8)
    good, n, keep_good = ctx._frame_list(frames, NV12)
    for name, c, (status, text) in host_rows.REFUSALS:
        keep = []
        d = _descriptor(c, keep)
        pair = (_lib.AvdFrameList * 2)(good, d)                                  # the second list of a batch, behind a valid one
        for rc in (L.avd_analyze_frame_lists(H, ctypes.byref(d), 1, rec.ctypes.data), L.avd_analyze_frame_lists_async(H, ctypes.byref(d), 1, rec.ctypes.data),
                   L.avd_preprocess_frame_list(H, ctypes.byref(d), small.ctypes.data, None, None, None),
                   L.avd_analyze_frame_lists(H, pair, 2, rec.ctypes.data),
                   L.avd_analyze_frame_lists(H, ctypes.byref(d), 1, None)):      # a null records pointer is refused LAST
            assert (rc, L.avd_last_error(H).decode()) == (status, text), name
        assert state() == before, name
    assert not rec["lap_sumsq"].any()
    # null records, nothing else wrong
    assert L.avd_analyze_frame_lists(H, ctypes.byref(good), 1, None) == -1 and L.avd_last_error(H).decode() == "null pointer"
    assert L.avd_analyze_frame_lists(H, None, 1, rec.ctypes.data) == -1 and L.avd_last_error(H).decode() == "bad clip list"
    assert L.avd_preprocess_frame_list(H, None, small.ctypes.data, None, None, None) == -1 and L.avd_last_error(H).decode() == "null frame list"
    assert state() == before
    empty = _lib.AvdFrameList * 1
    e, _, _ = ctx._frame_list([], I420)
    assert L.avd_analyze_frame_lists(H, empty(e), 1, None) == 0                  # no frames: no records to write
    assert state() == before
    assert L.avd_analyze_frame_lists(H, ctypes.byref(good), 1, rec.ctypes.data) == 0 and ctx.ingest_list() == (1, N)      # the descriptor itself is fine
    with avd_hip.Context(0) as fresh:
        for name in ("ingest_list", "stage_copies"):
            with pytest.raises(AvdError, match=name):
                fresh.debug_fetch(name, (2,), np.int32)
    del keep_good
