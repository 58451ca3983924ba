"""Option "ingest_group" on the device (include/avd.h): the clips of one avd_analyze_* call that share a group key are ingested by ONE ingest
launch and ONE k_hash launch per group.

Contract: the option has no effect on results.  Every test runs the same input on a context with "ingest_group" = 1 and on one with 0 and
compares the records (np.array_equal and equal bytes) and the debug buffers "small" and "area" with np.array_equal; what the call launched is
read from "ingest_call" / "ingest_groups".  At least one case per test is also held against the CPU oracle, bit for bit, in exact mode.

One call goes through ONE entry point, so a call holds strided clips (avd_analyze_pictures / _batch) or frame lists (avd_analyze_frame_lists),
not both: the interleaved-keys call is made through each, host and device members side by side in both.

Frames are 96 x 64 (16-byte fills) and 100 x 66 (scalar fills) unless a test says otherwise; clip lengths come from {1, 2, 3, 5}, so that
frames x bands is no multiple of 8 and the idle tail blocks of the ingest grid occur.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import avd_hip  # noqa: E402
from avd_hip import AvdError, Pixels, _lib, synth  # noqa: E402
from tests.content_families import pink, u8  # noqa: E402
from tests.ingest_gpu_kit import P_KERNEL, P_NI, plan  # noqa: E402
from tests.test_host_and_abi import _records_from_oracle  # noqa: E402

FAST, EXACT = 1, 0
MODES = pytest.mark.parametrize("mode", [FAST, EXACT], ids=["fast", "exact"])
REC = avd_hip.RECORD_DTYPE
BGR, NV12, I420 = _lib.AVD_FMT_BGR24, _lib.AVD_FMT_NV12, _lib.AVD_FMT_I420
WIDE, TALL = (64, 96), (66, 100)                    # (h, w): 16-byte fills, scalar fills
BGR_SCALAR, BGR_STAGED, NV12_TABLES = 0, 2, 4       # kernel ids (include/avd.h, "ingest_plan")


def torch():
    import torch as t
    return t


def dev(a):
    """a numpy array (uint16 as the same bits in int16) -> a device tensor of its own"""
    a = np.ascontiguousarray(a)
    return torch().from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def bgr(n, geom, seed):
    return synth.make_clip(n, geom[0], geom[1], seed=seed, dup_every=0, scene_cut=False)


def layout_clip(l, frames, device=False):
    """BGR frames uint8[N,H,W,3] -> the clip in layout row l (avd_hip._lib.LAYOUTS) as analyze_pictures takes it.  The chroma of the 4:2:2
    layouts repeats the 4:2:0 rows and the 16-bit layouts shift the 8-bit samples: generated content, compared between two runs of the library."""
    y, uv = synth.bgr_to_nv12(frames)
    uv422 = np.repeat(uv, 2, axis=1)
    put = dev if device else np.ascontiguousarray
    v = l.value
    if v == BGR:
        return put(frames)
    if v == NV12:
        return (put(y), put(uv))
    if v == I420:
        return tuple(put(p) for p in synth.nv12_to_i420(y, uv))
    if v == _lib.AVD_FMT_RGB24:
        return Pixels(put(frames[..., ::-1]), v)
    if v in (_lib.AVD_FMT_BGRA32, _lib.AVD_FMT_RGBA32):
        px = frames if v == _lib.AVD_FMT_BGRA32 else frames[..., ::-1]
        return Pixels(put(np.concatenate([px, np.full(px.shape[:3] + (1,), 200, np.uint8)], axis=-1)), v)
    if v == _lib.AVD_FMT_RGBP:
        return Pixels(put(frames[..., ::-1].transpose(0, 3, 1, 2)), v)
    if v in (_lib.AVD_FMT_YUYV422, _lib.AVD_FMT_UYVY422):
        pair = (y, uv422) if v == _lib.AVD_FMT_YUYV422 else (uv422, y)
        return Pixels(put(np.stack(pair, axis=-1)), v)
    if v == _lib.AVD_FMT_I422:
        return Pixels((put(y), put(uv422[..., 0::2]), put(uv422[..., 1::2])), v)
    if v == _lib.AVD_FMT_NV16:
        return Pixels((put(y), put(uv422)), v)
    if v == _lib.AVD_FMT_P010:
        return Pixels((put(y.astype(np.uint16) << 8), put(uv.astype(np.uint16) << 8)), v)
    if v == _lib.AVD_FMT_I010:
        return Pixels(tuple(put(p.astype(np.uint16) << 2) for p in synth.nv12_to_i420(y, uv)), v)
    raise AssertionError(l)


# ---- the two contexts ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def new_pair():
    """make(mode) -> (a context with the option on, one with it off), both in that Farneback mode; closed behind the test"""
    made = []

    def make(mode=FAST):
        pair = []
        for group in (1, 0):
            c = avd_hip.Context(0)
            c.set_option("fb_mode", mode)
            c.set_option("ingest_group", group)
            assert c.get_option("ingest_group") == group
            pair.append(c)
        made.extend(pair)
        return tuple(pair)
    yield make
    for c in made:
        c.close()


def same(got, want):
    return got.dtype == REC and np.array_equal(got, want) and got.tobytes() == want.tobytes()


def buffers(c, frames=None):
    """("small", "area") of the call that just ran on c; frames: the buffers' frames whose cells the call wrote (all of them unless it restored slots)"""
    n = int(c.stream_call()[3])
    small = c.debug_fetch("small", (n, 320, 320), np.uint8)
    area = c.debug_fetch("area", (n, 1024), np.uint8)
    return small, (area if frames is None else area[frames])


def run_both(pair, call, frames=None, tag=None):
    """the same call on both contexts -> the grouped one's records (a list, one array per clip); records and buffers compared"""
    g, u = pair
    got, want = call(g), call(u)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert same(a, b), (tag, i, a, b)
    for name, a, b in zip(("small", "area"), buffers(g, frames), buffers(u, frames)):
        assert np.array_equal(a, b), (tag, name, int(np.count_nonzero(a != b)))
    live = sum(len(a) > 0 for a in want)
    assert u.ingest_call().tolist() == [live, live, 0, 0], tag
    assert u.ingest_groups()[:, 1].tolist() == [1] * live, tag
    return got


def alone_kernel(c, call_one):
    """the kernel id a clip runs alone (on the context with the option off)"""
    call_one(c)
    return plan(c)[P_KERNEL]


# ---- 1. the StreamMux shape: eight one-frame NV12 device frame lists of one geometry ---------------------------------------------------
def test_eight_one_frame_device_lists(new_pair, oracle):
    g, u = pair = new_pair(EXACT)
    y, uv = synth.bgr_to_nv12(bgr(8, WIDE, 11))
    lists = [([(dev(y[i]), dev(uv[i]))], NV12) for i in range(8)]          # sixteen allocations
    got = run_both(pair, lambda c: c.analyze_frame_lists(lists), tag="eight lists")
    assert g.ingest_call().tolist() == [1, 1, 1, 8]
    assert g.ingest_list() == (2, 8)                                        # a grouped launch, its frames
    alone = alone_kernel(u, lambda c: c.analyze_frame_lists(lists[:1]))
    assert alone == NV12_TABLES and u.ingest_list() == (1, 1)
    assert g.ingest_groups().tolist() == [[0, 8, 8, alone]]
    for i in range(8):                                                      # one frame a clip: the moments, ham -1, no flow
        assert same(got[i], _records_from_oracle(oracle, oracle.nv12_to_bgr(y[i:i + 1], uv[i:i + 1]))), i


# ---- 2. seven clips with interleaved keys -----------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("entry", ["pictures", "lists"])
def test_seven_clips_with_interleaved_keys(new_pair, oracle, entry, mode):
    g, u = pair = new_pair(mode)
    a, b, c6 = bgr(2, WIDE, 21), bgr(3, WIDE, 22), bgr(1, WIDE, 23)
    wide_rows = np.zeros((1, 64, 112, 3), np.uint8)                         # the same BGR geometry in rows of 336 bytes
    wide_rows[:, :, :96] = bgr(1, WIDE, 24)
    padded = wide_rows[:, :, :96]
    nv = synth.bgr_to_nv12(bgr(2, WIDE, 25))
    nvj = synth.bgr_to_nv12(bgr(1, WIDE, 26))
    turned = synth.nv12_to_i420(*synth.bgr_to_nv12(bgr(5, (96, 64), 27)))   # stored 64 wide, 96 high: displayed 96 x 64 after a quarter turn
    rotates, ranges = [0, 0, 0, 0, 0, 1, 0], [False, False, False, False, True, False, False]
    if entry == "pictures":         # strided clips: host, device, host with padded rows, ..., host
        clips = [a, dev(b), padded, nv, nvj, turned, c6]
        call = lambda c: c.analyze_pictures(clips, rotates, ranges)
    else:                           # frame lists: a host list, a device list of the same strides, a host list with padded rows, ..., a host list
        frames = lambda planes: list(zip(*planes))
        lists = [(list(a), BGR), ([dev(f) for f in b], BGR), (list(padded), BGR), (frames(nv), NV12), (frames(nvj), NV12), (frames(turned), I420), (list(c6), BGR)]
        call = lambda c: c.analyze_frame_lists(lists, rotates, ranges)
    got = run_both(pair, call, tag=entry)
    # what plan_groups says of these keys (tests/test_ingest_group_host.py): the three BGR clips of one stride together -- host and device
    # members in one launch --, the padded one alone, NV12 apart from full-range NV12, the turned I420 clip alone; in the order of first members
    assert g.ingest_call().tolist() == [5, 5, 1, 6]
    rows = g.ingest_groups().tolist()
    assert [r[:3] for r in rows] == [[0, 3, 6], [2, 1, 1], [3, 1, 2], [4, 1, 1], [5, 1, 5]]
    assert rows[0][3] == rows[1][3] == BGR_STAGED and rows[2][3] == rows[3][3] == NV12_TABLES
    assert rows == [[r[0], r[1], r[2], k] for r, k in zip(rows, [w[3] for w in u.ingest_groups().tolist() if w[0] in (0, 2, 3, 4, 5)])]
    if mode == EXACT:
        for i, clip in ((0, a), (1, b), (6, c6), (2, np.ascontiguousarray(padded))):
            assert same(got[i], _records_from_oracle(oracle, clip)), i


# ---- 3. every layout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", _lib.LAYOUTS, ids=[l.name for l in _lib.LAYOUTS])
def test_every_layout_at_both_geometries(new_pair, oracle, layout):
    g, u = pair = new_pair(EXACT)
    is420 = layout.ydiv == 2
    is_yuv = layout.value not in (BGR, _lib.AVD_FMT_RGB24, _lib.AVD_FMT_BGRA32, _lib.AVD_FMT_RGBA32, _lib.AVD_FMT_RGBP)
    cases = [(geom, 0, False) for geom in (WIDE, TALL)]
    if is420:
        cases += [(WIDE, r, False) for r in (1, 2, 3)] + [(TALL, 1, False)]
    if is_yuv:
        cases += [(WIDE, 0, True), (TALL, 0, True)]
    for geom, rot, full in cases:
        tag = (layout.name, geom, rot, full)
        stored = (geom[1], geom[0]) if rot & 1 else geom                    # the displayed picture is geom
        src = [bgr(2, stored, 31), bgr(3, stored, 32)]
        clips = [layout_clip(layout, s) for s in src]
        got = run_both(pair, lambda c: c.analyze_pictures(clips, [rot] * 2, [full] * 2), tag=tag)
        assert g.ingest_call().tolist() == [1, 1, 1, 5], tag
        alone = alone_kernel(u, lambda c: c.analyze_pictures(clips[:1], [rot], [full]))
        assert g.ingest_groups().tolist() == [[0, 2, 5, alone]], tag
        assert plan(g)[:2] == list(geom), tag
        if layout.value == BGR:
            for a, s in zip(got, src):
                assert same(a, _records_from_oracle(oracle, s)), tag


def test_an_aligned_and_a_misaligned_clip_are_two_launches(new_pair, oracle):
    g, u = pair = new_pair(EXACT)
    t = torch()
    src = [bgr(2, WIDE, 41), bgr(3, WIDE, 42), bgr(1, WIDE, 43)]
    flat = t.zeros(src[1].size + 16, dtype=t.uint8, device="cuda")
    odd = flat[1:1 + src[1].size].view(src[1].shape)                        # the same strides at an odd address
    odd.copy_(dev(src[1]))
    assert odd.data_ptr() % 16 == 1
    clips = [dev(src[0]), odd, dev(src[2])]
    got = run_both(pair, lambda c: c.analyze_batch(clips), tag="misaligned")
    assert g.ingest_call().tolist() == [2, 2, 1, 3]
    assert g.ingest_groups().tolist() == [[0, 2, 3, BGR_STAGED], [1, 1, 3, BGR_SCALAR]]
    assert u.ingest_groups().tolist() == [[0, 1, 2, BGR_STAGED], [1, 1, 3, BGR_SCALAR], [2, 1, 1, BGR_STAGED]]
    for a, s in zip(got, src):
        assert same(a, _records_from_oracle(oracle, s))


# ---- 4. every NI class of the band plan -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,ni", [(640, 3), (768, 4), (1024, 4), (1280, 6), (1536, 8), (2048, 8), (4096, 9)])
def test_every_ni_class(new_pair, oracle, w, ni):
    """NI = max(3, ceil((rows per band + 2) / (256 // (w / 16)))) by the band plan's rule: 768, 1024, 1536, 2048 and 4096 give 4, 4, 8, 8, 9;
    640 and 1280 are here for 3 and 6.  Height 34: bands of 14 rows (640 ... 2048) end in a short band of 6, bands of 7 rows (4096) in one of 6."""
    g, u = pair = new_pair(EXACT)
    rgbp = next(l for l in _lib.LAYOUTS if l.value == _lib.AVD_FMT_RGBP)
    src = [bgr(1, (34, w), 51), bgr(2, (34, w), 52)]
    for name, clips in (("bgr", src), ("rgbp", [layout_clip(rgbp, s) for s in src])):
        got = run_both(pair, lambda c: c.analyze_pictures(clips), tag=(name, w))
        assert g.ingest_call().tolist() == [1, 1, 1, 3]
        p = plan(g)
        assert 34 % p[2] != 0, "precondition: the last band is short"
        assert p[P_NI] == (ni if name == "bgr" or ni <= 8 else 0), (name, p)      # planar RGB has no staged kernel of NI 9
        alone = alone_kernel(u, lambda c: c.analyze_pictures(clips[:1]))
        assert g.ingest_groups().tolist() == [[0, 2, 3, alone]] and plan(u)[P_NI] == p[P_NI]
        if name == "bgr" and w in (640, 768):
            for a, s in zip(got, src):
                assert same(a, _records_from_oracle(oracle, s))


# ---- 5. "stream_map" ------------------------------------------------------------------------------------------------------------------------
def patch_clip():
    """a static background with a moving patch, 64 x 96: the fast level kernels flag its pairs (as in tests/test_gpu_stream_map.py)"""
    bg = u8(pink(np.random.default_rng(5), 1.2, size=480)[100:164, 100:196])
    out = []
    for k in range(7):
        f = bg.copy()
        f[10 + 5 * k:16 + 5 * k, 8 + 9 * k:18 + 9 * k] = 255 - f[10 + 5 * k:16 + 5 * k, 8 + 9 * k:18 + 9 * k]
        out.append(f)
    return np.ascontiguousarray(np.repeat(np.stack(out)[..., None], 3, axis=-1))


@MODES
def test_three_mapped_streams_in_rounds(new_pair, oracle, mode):
    g, u = pair = new_pair(mode)
    streams = [bgr(7, WIDE, 61), patch_clip(), bgr(7, WIDE, 63)]
    with avd_hip.Context(0) as ref:                                        # never a slot, never a map, the option off
        ref.set_option("fb_mode", mode)
        whole = [ref.analyze_frames(s) for s in streams]
    if mode == FAST:
        assert whole[1]["reserved"][3:].any(), "precondition: a pair behind the first round is flagged, so the exact re-run reads the grouped small"
    else:
        assert same(whole[0], _records_from_oracle(oracle, streams[0]))
    for c in pair:
        c.stream_map({0: 3, 1: 1, 2: 8})
    got, at = [[], [], []], 0
    for rnd, n in enumerate((3, 1, 3)):
        chunk = [s[at:at + n] for s in streams]
        # from the second round on every clip lies behind its carry frame: the output frames of the group are 1 .. n, n + 2 .. 2n + 1, ...
        own = None if rnd == 0 else np.concatenate([np.arange(n) + i * (n + 1) + 1 for i in range(3)])
        out = run_both(pair, lambda c: c.analyze_batch(chunk), frames=own, tag=("round", rnd))
        assert g.ingest_call().tolist() == [1, 1, 1, 3 * n]
        assert g.stream_call().tolist() == u.stream_call().tolist() == ([0, 0, 1, 9] if rnd == 0 else [3, 1, 1, 3 * n + 3])
        for o, k in zip(out, got):
            k.append(o)
        at += n
    for i in range(3):
        assert same(np.concatenate(got[i]), whole[i]), i
    assert g.stream_state().tolist() == u.stream_state().tolist()


def test_stream_mux_grouped_equals_ungrouped():
    clips = [synth.bgr_to_nv12(bgr(3, WIDE, 70 + i)) for i in range(4)]
    streams = lambda: [(list(zip(y, uv)), NV12) for y, uv in clips]
    with avd_hip.Context(0) as c:
        off = avd_hip.StreamMux(ctx=c, chunk=1, group=False).run(streams())
        assert c.ingest_call().tolist() == [4, 4, 0, 0]
        c.set_option("ingest_group", 0)
        on = avd_hip.StreamMux(ctx=c, chunk=1, group=True).run(streams())
        assert c.ingest_call().tolist() == [1, 1, 1, 4] and c.get_option("ingest_group") == 0      # restored
        whole = [c.analyze_frames_nv12(y, uv) for y, uv in clips]
    for a, b, w in zip(on, off, whole):
        assert same(a, b) and same(a, w)


# ---- 6. more geometries than the cache holds ----------------------------------------------------------------------------------------------
def test_five_geometries_interleaved(new_pair, oracle):
    g, u = pair = new_pair(EXACT)
    geoms = [WIDE, TALL, (48, 64), (56, 80), (40, 72)]
    src = [bgr(1 + (i + r) % 3, geoms[i], 80 + 5 * r + i) for r in range(2) for i in range(5)]      # geometry i at positions i and i + 5
    got = run_both(pair, lambda c: c.analyze_batch(src), tag="five geometries")
    total = sum(len(s) for s in src)
    assert g.ingest_call().tolist() == [5, 5, 5, total]
    assert [r[:3] for r in g.ingest_groups().tolist()] == [[i, 2, len(src[i]) + len(src[i + 5])] for i in range(5)]
    for i in (0, 1, 5, 9):
        assert same(got[i], _records_from_oracle(oracle, src[i])), i


# ---- 7. asynchronous calls, refusals, history ------------------------------------------------------------------------------------------------
def test_async_call_with_another_call_behind_it(new_pair, oracle):
    g, u = pair = new_pair(EXACT)
    clips = [bgr(2, WIDE, 91), bgr(5, WIDE, 92), bgr(3, TALL, 93)]
    other = bgr(2, TALL, 94)
    want = u.analyze_batch(clips)
    rec = np.zeros(10, REC)
    keep = g.analyze_batch_async(clips, rec)
    assert g.ingest_call().tolist() == [2, 2, 1, 7]
    after = g.analyze_frames(other)                                         # issued while the grouped call is pending: that call is drained first
    del keep
    assert same(rec, np.concatenate(want))
    assert same(after, u.analyze_frames(other)) and g.ingest_call().tolist() == [1, 1, 0, 0]
    for a, s in zip(np.split(rec, [2, 7]), clips):
        assert same(a, _records_from_oracle(oracle, s))


def test_refusals_leave_everything_as_it_was(new_pair, oracle):
    g, u = new_pair(EXACT)
    for bad in (2, -1):
        with pytest.raises(AvdError, match="ingest_group:"):
            g.set_option("ingest_group", bad)
        assert g.get_option("ingest_group") == 1
    with pytest.raises(AvdError, match="ingest_group:"):
        u.set_option("ingest_group", 2)
    assert u.get_option("ingest_group") == 0
    clips = [bgr(2, WIDE, 95), bgr(1, WIDE, 96)]
    g.stream_map({0: 1, 1: 2})
    first = g.analyze_batch(clips)
    before = (g.ingest_call().tolist(), g.ingest_groups().tolist(), g.stream_state().tolist(), g.stream_call().tolist())
    assert before[0] == [1, 1, 1, 3]
    with pytest.raises(AvdError, match="32x32"):
        g.analyze_batch(clips + [np.zeros((1, 20, 20, 3), np.uint8)])       # the third clip is refused
    assert (g.ingest_call().tolist(), g.ingest_groups().tolist(), g.stream_state().tolist(), g.stream_call().tolist()) == before
    assert g.get_option("ingest_group") == 1
    for a, s in zip(first, clips):
        assert same(a, _records_from_oracle(oracle, s))


def test_a_grouped_call_does_not_depend_on_the_contexts_history(new_pair, oracle):
    g, u = new_pair(EXACT)
    clips = [bgr(3, WIDE, 97), bgr(2, TALL, 98), bgr(2, WIDE, 99)]
    fresh = g.analyze_batch(clips)
    small = buffers(g)
    # other formats, other groupings, then the memory given back
    u.set_option("ingest_group", 1)
    u.analyze_pictures([synth.bgr_to_nv12(bgr(2, TALL, 100)), synth.bgr_to_nv12(bgr(1, TALL, 101)), bgr(5, (40, 72), 102)])
    u.analyze_frame_lists([(list(bgr(2, WIDE, 103)), BGR), (list(bgr(1, WIDE, 104)), BGR)])
    u.release_workspace()
    later = u.analyze_batch(clips)
    assert u.ingest_call().tolist() == g.ingest_call().tolist() == [2, 2, 1, 5]
    for a, b, s in zip(later, fresh, clips):
        assert same(a, b) and same(a, _records_from_oracle(oracle, s))
    for a, b in zip(buffers(u), small):
        assert np.array_equal(a, b)


# ---- 8. profiling on ----------------------------------------------------------------------------------------------------------------------
def test_regions_follow_the_launches(new_pair, oracle):
    """A call records at most 96 regions.  48 one-frame clips of one geometry are 96 ingest and hash regions with a launch pair per clip -- with the
    Farneback regions behind them avd_kernel_ms refuses the call -- and 2 with one launch pair for all.  The regions tile their stage: the first
    begins where stage 0 begins, the last hash region ends where it ends, so their sum IS the stage, up to the rounding of float32 sums
    (eps = 1e-5 of the stage: tests/test_gpu_profiling.py derives it)."""
    g, u = pair = new_pair(EXACT)
    clips = [bgr(1, WIDE, 110 + i) for i in range(48)]
    plain = run_both(pair, lambda c: c.analyze_batch(clips), tag="unprofiled")
    for c in pair:
        c.set_profiling(True)
    profiled = run_both(pair, lambda c: c.analyze_batch(clips), tag="profiled")
    assert g.ingest_call().tolist() == [1, 1, 1, 48] and u.ingest_call().tolist() == [48, 48, 0, 0]
    with pytest.raises(AvdError, match="more kernel regions than the library records"):
        u.kernel_ms()
    K, S = g.kernel_ms(), g.stage_ms()
    assert K["preprocess"] > 0 and K["hash"] > 0
    assert abs(K["preprocess"] + K["hash"] - S[0]) <= 1e-5 * S[0], (K, S)
    for a, b in zip(profiled, plain):
        assert same(a, b)                                                    # records are unchanged by profiling
    assert same(profiled[0], _records_from_oracle(oracle, clips[0]))
    # three geometries, two clips each: three launch pairs, six regions, still the whole stage
    mixed = [bgr(2, geom, 120 + i) for i, geom in enumerate((WIDE, TALL, (48, 64), WIDE, TALL, (48, 64)))]
    run_both(pair, lambda c: c.analyze_batch(mixed), tag="mixed")
    assert g.ingest_call().tolist() == [3, 3, 3, 12]
    for c in pair:
        K, S = c.kernel_ms(), c.stage_ms()
        assert abs(K["preprocess"] + K["hash"] - S[0]) <= 1e-5 * S[0], (K, S)
