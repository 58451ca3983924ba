"""Option "stream_map" on the device (include/avd.h): several clips of ONE call continue a stream slot each.

Contract: a clip at a mapped position continues its slot exactly as the one-clip call with "stream_slot" does, so a clip sent in chunks through
mapped calls -- beside other streams, in whatever rounds -- gives the records of the clip sent whole.  The referee is that of
tests/test_gpu_stream.py: the same clip in ONE call on a context that has never selected a slot or set a map (``ref``, one per Farneback mode,
created for this module; every whole-clip reference is computed once and shared), and every comparison is np.array_equal plus equal bytes.

Frames are 48 x 64, 56 x 80 and 64 x 96; every streaming context is created by its test.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import avd_hip  # noqa: E402
from avd_hip import AvdError, _lib, synth  # noqa: E402
from tests.content_families import pink, u8  # noqa: E402

FAST, EXACT = 1, 0
MODES = pytest.mark.parametrize("mode", [FAST, EXACT], ids=["fast", "exact"])
REC = avd_hip.RECORD_DTYPE
BGR, NV12, I420 = _lib.AVD_FMT_BGR24, _lib.AVD_FMT_NV12, _lib.AVD_FMT_I420
GEOMS = ((48, 64), (56, 80), (64, 96))


# ---- content (generated once) ---------------------------------------------------------------------------------------------------------
def _bgr(gray):
    return np.ascontiguousarray(np.repeat(np.asarray(gray)[..., None], 3, axis=-1))


def plain(n, geom, seed):
    return synth.make_clip(n, geom[0], geom[1], seed=seed, dup_every=0, scene_cut=False)


class Material:
    def __init__(self):
        a = plain(3, GEOMS[0], 1)
        b = plain(3, GEOMS[0], 2)
        # the 7-frame window-boxed clip of tests/test_gpu_stream.py: frame 3 duplicates frame 2 (ham 0, flow exactly 0), frames 4 .. 6 are another
        # scene -- the duplicate pair and the cut lie across the rounds of (3, 1, 3)
        boxed = np.full((7, 48, 64, 3), 16, np.uint8)
        boxed[:, 8:28, 8:36] = np.stack([a[0], a[1], a[2], a[2], b[0], b[1], b[2]])[:, 8:28, 8:36]
        self.clip7 = boxed
        # a static background with a moving patch, 64 x 96: every pair is flagged by the fast level kernels (as in tests/test_gpu_stream.py)
        bg = u8(pink(np.random.default_rng(5), 1.2, size=480)[100:164, 100:196])
        base = []
        for k in range(8):
            f = bg.copy()
            f[10 + 5 * k:16 + 5 * k, 8 + 9 * k:18 + 9 * k] = 255 - f[10 + 5 * k:16 + 5 * k, 8 + 9 * k:18 + 9 * k]
            base.append(f)
        self.patch = _bgr(np.stack(base))
        self.calm = plain(6, GEOMS[1], 3)                          # no pair flagged (asserted where it matters)
        self.nv12 = synth.bgr_to_nv12(plain(7, GEOMS[1], 31))       # (y, uv) stacks
        self.i420 = synth.nv12_to_i420(*synth.bgr_to_nv12(plain(7, GEOMS[2], 32)))      # (y, u, v) stacks
        self.eight = [plain(5, GEOMS[i % 3], 40 + i) for i in range(8)]
        self.long = plain(8, GEOMS[0], 5)[np.arange(515) % 8]
        self.wav = (np.sin(np.arange(20000) * 0.05) * 0.3).astype(np.float32)
        self.mux = [synth.bgr_to_nv12(plain(n, GEOMS[i % 3], 60 + i)) for i, n in enumerate((7, 5, 3, 6))]


@pytest.fixture(scope="module")
def mat():
    return Material()


@pytest.fixture(scope="module")
def ref():
    """(mode, key, call) -> the whole-clip records, from a context per mode that never selects a slot and never sets a map; computed once per key"""
    ctxs, cache = {}, {}
    for mode in (FAST, EXACT):
        ctxs[mode] = avd_hip.Context(0)
        ctxs[mode].set_option("fb_mode", mode)

    def whole(mode, key, call):
        if (mode, key) not in cache:
            rec = call(ctxs[mode])
            rec.setflags(write=False)
            cache[(mode, key)] = rec
        return cache[(mode, key)]
    yield whole
    for c in ctxs.values():
        c.close()


@pytest.fixture
def new_ctx():
    made = []

    def make(mode):
        c = avd_hip.Context(0)
        c.set_option("fb_mode", mode)
        made.append(c)
        return c
    yield make
    for c in made:
        c.close()


def same(got, want):
    return got.dtype == REC and np.array_equal(got, want) and got.tobytes() == want.tobytes()


def state(c):
    return c.stream_state().tolist()


def want_state(frames_by_slot, position_by_slot):
    return [[frames_by_slot.get(k, 0), position_by_slot.get(k, -1)] for k in range(1, 9)]


# ---- 1. three streams of different layouts and geometries --------------------------------------------------------------------------------
@MODES
def test_three_streams_of_different_layouts(mat, ref, new_ctx, mode):
    y, uv = mat.nv12
    Y, U, V = mat.i420
    w_bgr = ref(mode, "clip7", lambda r: r.analyze_frames(mat.clip7))
    w_nv12 = ref(mode, "nv12", lambda r: r.analyze_frames_nv12(y, uv))
    w_i420 = ref(mode, "i420", lambda r: r.analyze_frames_i420(Y, U, V))
    # what the boxed clip was built for
    assert w_bgr["ham"][0] == -1 and w_bgr["ham"][3] == 0 and w_bgr["flow_mean"][3] == 0.0 and w_bgr["flow_var"][3] == 0.0
    assert w_bgr["ham"][4] > 0 and w_bgr["flow_mean"][4] > 0.0
    c = new_ctx(mode)
    c.stream_map({0: 2, 1: 5, 2: 1})
    assert c.get_option("stream_map") == 3
    got, calls = [[], [], []], []
    at = 0
    for rnd, n in enumerate((3, 1, 3)):
        s = slice(at, at + n)
        if rnd == 1:          # a round through the frame-list entry: a BGR list, an NV12 list, an I420 list
            out = c.analyze_frame_lists([(list(mat.clip7[s]), BGR), (list(zip(y[s], uv[s])), NV12), (list(zip(Y[s], U[s], V[s])), I420)])
        else:                 # the picture entry: a BGR stack, an NV12 pair, an I420 picture
            out = c.analyze_pictures([mat.clip7[s], (y[s], uv[s]), (Y[s], U[s], V[s])])
        for g, o in zip(got, out):
            g.append(o)
        calls.append(c.stream_call().tolist())
        at += n
    for g, w in zip(got, (w_bgr, w_nv12, w_i420)):
        assert same(np.concatenate(g), w), (np.concatenate(g), w)
    # clips that continued a filled slot, restore launches, save launches, frames in the buffers (restored frames included)
    assert calls == [[0, 0, 1, 9], [3, 1, 1, 6], [3, 1, 1, 12]]
    assert state(c) == want_state({2: 7, 5: 7, 1: 7}, {2: 0, 5: 1, 1: 2})


# ---- 2. eight streams of one frame per call ---------------------------------------------------------------------------------------------
@MODES
def test_eight_streams_of_one_frame_per_call(mat, ref, new_ctx, mode):
    c = new_ctx(mode)
    c.stream_map({i: 8 - i for i in range(8)})
    got = [[] for _ in range(8)]
    for k in range(5):
        for g, o in zip(got, c.analyze_batch([clip[k:k + 1] for clip in mat.eight])):
            g.append(o)
        assert c.stream_call().tolist() == ([0, 0, 1, 8] if k == 0 else [8, 1, 1, 16])      # every clip is n = 1 behind a carry
    for i, g in enumerate(got):
        assert same(np.concatenate(g), ref(mode, ("eight", i), lambda r: r.analyze_frames(mat.eight[i]))), i
    assert state(c) == want_state({k: 5 for k in range(1, 9)}, {8 - i: i for i in range(8)})


# ---- 3. ragged rounds ------------------------------------------------------------------------------------------------------------------
@MODES
def test_ragged_rounds(mat, ref, new_ctx, mode):
    A, B, C, D = mat.eight[0][:5], mat.eight[1][:4], mat.eight[2][:3], mat.eight[3][:4]
    E = mat.calm                                                    # position 4 is not mapped: a new clip every call
    e = [E[0:2], E[2:3], E[3:6]]
    rounds = [
        [A[0:2], B[0:2], C[:0], D[0:3], e[0]],                     # C has not joined yet
        [A[2:3], B[:0], C[0:2], D[3:4], e[1]],                     # B is absent, C joins, D gives its last frame
        [A[3:5], B[2:4], C[2:3], D[:0], e[2]],                     # D has ended
    ]
    c = new_ctx(mode)
    c.stream_map({0: 3, 1: 4, 2: 6, 3: 7})
    got = [[] for _ in range(5)]
    for r in rounds:
        for g, o in zip(got, c.analyze_batch(r)):
            g.append(o)
    for i, (name, clip) in enumerate((("A", A), ("B", B), ("C", C), ("D", D))):
        out = np.concatenate(got[i])
        assert same(out, ref(mode, ("ragged", name), lambda r: r.analyze_frames(clip))), name
    assert got[2][0].size == 0 and got[2][1]["ham"][0] == -1       # the late stream starts a clip
    for k, chunk in enumerate(e):
        assert same(got[4][k], ref(mode, ("ragged-E", k), lambda r: r.analyze_frames(chunk))), k      # that chunk analysed alone
        assert got[4][k]["ham"][0] == -1
    assert state(c) == want_state({3: 5, 4: 4, 6: 3, 7: 4}, {3: 0, 4: 1, 6: 2, 7: 3})
    # a mapped position the call does not list leaves its slot alone
    before = state(c)
    c.analyze_batch([A[:0]])
    assert state(c) == before and c.stream_call().tolist() == [0, 0, 0, 0]


# ---- 4. the flagged boundary pair -------------------------------------------------------------------------------------------------------
@MODES
def test_flagged_boundary_pair_beside_an_unflagged_stream(mat, ref, new_ctx, mode):
    clip = mat.patch[:5]
    whole = ref(mode, "patch5", lambda r: r.analyze_frames(clip))
    calm = ref(mode, "calm", lambda r: r.analyze_frames(mat.calm))
    assert not calm["reserved"].any()
    if mode == FAST:
        assert whole["reserved"][2:].all(), "precondition: the fast kernels flag the pair across the calls and those behind it"
    c = new_ctx(mode)
    c.stream_map({0: 1, 1: 2})
    a1, b1 = c.analyze_batch([mat.calm[:4], clip[:2]])
    assert c.get_option("rerun_pairs") == np.count_nonzero(b1["reserved"]) + np.count_nonzero(a1["reserved"])
    a2, b2 = c.analyze_batch([mat.calm[4:], clip[2:]])
    assert same(np.concatenate([b1, b2]), whole)                   # bit-identical, flag words included
    assert same(np.concatenate([a1, a2]), calm)
    handed = np.count_nonzero(a2["reserved"]) + np.count_nonzero(b2["reserved"])
    assert c.get_option("rerun_pairs") == handed
    if mode == FAST:
        assert b2["reserved"][0] != 0 and handed == 3              # the pair across the calls was flagged and re-run exactly
        exact = ref(EXACT, "patch5", lambda r: r.analyze_frames(clip))
        for field in ("flow_mean", "flow_var", "ham", "lap_sum", "lap_sumsq"):
            assert b2[field][0].tobytes() == exact[field][2].tobytes(), field


# ---- 5. the Farneback chunk seam ----------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("na", [511, 510], ids=["carry-at-512", "first-own-frame-at-512"])
def test_second_stream_at_the_chunk_seam(mat, ref, new_ctx, mode, na):
    """the buffers of call 2 are [carry_a][a x na][carry_b][b x 3]: carry_b is frame na + 1, and the 512-pair scratch ends its first chunk
    with frame 512 -- the carry frame itself (na = 511), or the first own frame behind it (na = 510)"""
    A, B = mat.long[:na + 1], mat.eight[5][:4]
    c = new_ctx(mode)
    c.stream_map({0: 1, 1: 2})
    a1, b1 = c.analyze_batch([A[:1], B[:1]])
    a2, b2 = c.analyze_batch([A[1:], B[1:]])
    call = c.stream_call().tolist()
    assert call == [2, 1, 1, na + 5] and call[3] - 1 > 512         # more than 512 pairs: two chunks
    assert same(np.concatenate([a1, a2]), ref(mode, ("long", na), lambda r: r.analyze_frames(A)))
    assert same(np.concatenate([b1, b2]), ref(mode, "seam-B", lambda r: r.analyze_frames(B)))


# ---- 6. the map and "stream_slot" on the same slot -------------------------------------------------------------------------------------
@MODES
def test_map_and_stream_slot_share_the_slots(mat, ref, new_ctx, mode):
    whole = ref(mode, "clip7", lambda r: r.analyze_frames(mat.clip7))
    calm = ref(mode, "calm", lambda r: r.analyze_frames(mat.calm))
    c = new_ctx(mode)
    c.stream_map({0: 4})
    first, other = c.analyze_batch([mat.clip7[:3], mat.calm])      # position 1 is not mapped
    assert same(other, calm)
    c.stream_map(None)
    assert c.get_option("stream_map") == 0
    assert same(c.analyze_frames(mat.calm), calm)                   # other work between the calls: no slot, no map
    small = c.preprocess_bgr(mat.eight[2])[0]
    c.farneback_pairs(small)
    c.release_workspace()
    c.audio_features(mat.wav, 2000)
    c.stream_slot(4)
    assert c.stream_frames() == 3
    second = c.analyze_frames(mat.clip7[3:4])                       # the same slot through "stream_slot"
    c.stream_slot(0)
    c.release_workspace()
    c.stream_map({1: 4})                                            # and through the map again, at another position
    c.preprocess_bgr(mat.calm)                                      # the entry points that ignore the map, with it set
    c.farneback_pairs(small[:3])
    other, third = c.analyze_batch([mat.calm, mat.clip7[4:]])
    assert same(other, calm)
    assert same(np.concatenate([first, second, third]), whole)
    assert state(c) == want_state({4: 7}, {4: 1})


# ---- 7. asynchronous calls back to back --------------------------------------------------------------------------------------------------
@MODES
def test_two_async_calls_without_a_synchronize_between(mat, ref, new_ctx, mode):
    clip = mat.patch[:5]                                            # every pair flagged in fast mode: both calls leave a re-run to the drain
    whole = ref(mode, "patch5", lambda r: r.analyze_frames(clip))
    calm = ref(mode, "calm", lambda r: r.analyze_frames(mat.calm))
    c = new_ctx(mode)
    c.stream_map({0: 1, 1: 2})
    r1, r2 = np.zeros(2 + 3, REC), np.zeros(3 + 3, REC)
    k1 = c.analyze_batch_async([clip[:2], mat.calm[:3]], r1)
    k2 = c.analyze_batch_async([clip[2:], mat.calm[3:]], r2)       # drains the first call (the existing rule), then continues both clips
    c.synchronize()
    del k1, k2
    assert same(np.concatenate([r1[:2], r2[:3]]), whole)
    assert same(np.concatenate([r1[2:], r2[3:]]), calm)
    if mode == FAST:
        assert r2["reserved"][0] != 0 and c.get_option("rerun_pairs") == 3


# ---- 8. refusals and atomicity ---------------------------------------------------------------------------------------------------------------
def test_option_refusals(new_ctx):
    c = new_ctx(FAST)
    for bad in (-2, -100, (64 << 4) | 1, (0 << 4) | 9, (3 << 4) | 15, 1 << 20):
        with pytest.raises(AvdError, match=r"avd status -1: stream_map: .*0 \.\.\. 63.*0 \.\.\. 8"):
            c.set_option("stream_map", bad)
        assert c.get_option("stream_map") == 0
    c.set_option("stream_map", (0 << 4) | 1)
    c.set_option("stream_map", (63 << 4) | 8)
    assert c.get_option("stream_map") == 2
    with pytest.raises(AvdError, match=r"avd status -1: stream_map: .*already mapped at another position"):
        c.set_option("stream_map", (5 << 4) | 1)
    c.set_option("stream_map", (0 << 4) | 1)                        # the same slot at the same position: nothing changes
    assert c.get_option("stream_map") == 2 and state(c) == want_state({}, {1: 0, 8: 63})
    for k in (1, 8):
        with pytest.raises(AvdError, match=r"avd status -1: stream_slot: .*stream_map"):
            c.stream_slot(k)
        assert c.get_option("stream_slot") == 0
    for bad in (9, -1):                                             # the range refusal keeps its message
        with pytest.raises(AvdError, match=r"stream_slot: .*1 \.\.\. 8"):
            c.stream_slot(bad)
    c.stream_slot(0)                                                # slot 0 is what holds anyway
    c.set_option("stream_map", (0 << 4) | 3)                        # a position takes another slot; slot 1 is free again
    c.set_option("stream_map", (7 << 4) | 1)
    assert state(c) == want_state({}, {3: 0, 1: 7, 8: 63})
    c.set_option("stream_map", (63 << 4) | 0)                       # slot 0 unmaps
    assert c.get_option("stream_map") == 2
    c.set_option("stream_map", -1)
    assert c.get_option("stream_map") == 0 and state(c) == want_state({}, {})
    c.stream_slot(2)
    for v in ((0 << 4) | 1, (0 << 4) | 0):
        with pytest.raises(AvdError, match=r"avd status -1: stream_map: .*stream_slot"):
            c.set_option("stream_map", v)
    c.set_option("stream_map", -1)                                  # clearing is always accepted
    assert c.get_option("stream_slot") == 2 and c.get_option("stream_map") == 0
    with pytest.raises(AvdError):
        c.stream_map({0: 1})
    c.stream_slot(0)
    c.stream_map({0: 1})
    assert c.get_option("stream_map") == 1


@MODES
def test_a_refused_call_leaves_every_slot_alone(mat, ref, new_ctx, mode):
    whole = ref(mode, "clip7", lambda r: r.analyze_frames(mat.clip7))
    calm = ref(mode, "calm", lambda r: r.analyze_frames(mat.calm))
    c = new_ctx(mode)
    c.stream_map({0: 1, 1: 2, 2: 3})
    a1, b1, _ = c.analyze_batch([mat.clip7[:3], mat.calm[:2], mat.calm[:0]])
    before = state(c)
    assert before == want_state({1: 3, 2: 2}, {1: 0, 2: 1, 3: 2})
    tiny = np.zeros((2, 16, 16, 3), np.uint8)                       # a clip the library does not take (smaller than 32 x 32)
    for bad in ([mat.clip7[3:], mat.calm[2:], tiny], [tiny, mat.calm[2:], mat.eight[0]]):
        with pytest.raises(AvdError):
            c.analyze_batch(bad)
        assert state(c) == before
        with pytest.raises(AvdError):
            c.analyze_batch_async(bad, np.zeros(sum(len(x) for x in bad), REC))
        assert state(c) == before
    a2, b2, fresh = c.analyze_batch([mat.clip7[3:], mat.calm[2:], mat.eight[0]])
    assert same(np.concatenate([a1, a2]), whole) and same(np.concatenate([b1, b2]), calm)
    assert same(fresh, ref(mode, ("eight", 0), lambda r: r.analyze_frames(mat.eight[0])))       # slot 3 was empty: a new clip
    assert state(c) == want_state({1: 7, 2: 6, 3: 5}, {1: 0, 2: 1, 3: 2})


def test_allgather_last_records_is_refused_after_a_mapped_call(mat, new_ctx):
    c = new_ctx(FAST)
    c.stream_map({0: 1})
    c.analyze_batch([mat.calm[:2]])
    with pytest.raises(AvdError, match=r"avd status -4: .*stream_map"):      # AVD_ERR_UNSUPPORTED, ahead of the communicator check
        c.allgather_last_records(1)
    c.stream_map(None)
    c.analyze_batch([mat.calm[:2]])
    with pytest.raises(AvdError, match=r"avd status -1: avd_comm_init has not been called"):
        c.allgather_last_records(1)


# ---- 9. profiling ------------------------------------------------------------------------------------------------------------------------
def test_regions_of_a_mapped_call_tile_its_stages(new_ctx):
    """The ONE restore launch lies in the first preprocess region and the ONE save launch in the `other` region of stage 3: with K = kernel_ms()
    and S = stage_ms() of a mapped call without a flagged pair, the regions recorded between two stage events sum to that stage (they share
    the events; 1e-5 of the stage covers the float32 rounding of at most 96 terms, as tests/test_gpu_profiling.py derives it), and no id
    appears that a plain call lacks."""
    a, b = plain(6, (96, 128), 1), plain(5, (64, 96), 2)
    c = new_ctx(FAST)
    c.stream_map({0: 1, 1: 2})
    c.analyze_batch([a[:3], b[:2]])
    c.set_profiling(True)
    ra, rb = c.analyze_batch([a[3:], b[2:]])
    K, S = c.kernel_ms(), c.stage_ms()
    c.set_profiling(False)
    print(f"\n[stream_map profiling] K {K}\n                       S {S}")
    assert c.stream_call().tolist() == [2, 1, 1, 8]
    assert not ra["reserved"].any() and not rb["reserved"].any() and c.get_option("rerun_pairs") == 0
    assert set(K) == set(avd_hip.Context.KERNEL_IDS)
    flow = ("pyramid", "polyexp", "level40", "flow_up80", "level80", "flow_up160", "level160", "flow_up320", "level320", "stats", "records")
    for inner, outer in ((K["preprocess"] + K["hash"], S[0]), (sum(K[k] for k in flow), S[2]), (K["other"], S[1] + S[3])):
        assert outer > 0 and abs(inner - outer) <= 1e-5 * outer, (inner, outer, K, S)
    assert K["rerun"] == 0.0


# ---- 10. StreamMux --------------------------------------------------------------------------------------------------------------------------
def test_stream_mux_from_host_planes(mat, ref, new_ctx):
    c = new_ctx(FAST)
    streams = [(iter(list(zip(y, uv))), NV12) for y, uv in mat.mux]                 # 7, 5, 3 and 6 surfaces of three geometries
    got = avd_hip.StreamMux(ctx=c, chunk=2).run(streams)
    for i, (y, uv) in enumerate(mat.mux):
        assert same(got[i], ref(FAST, ("mux", i), lambda r: r.analyze_frames_nv12(y, uv))), i
    assert c.get_option("stream_map") == 0 and c.get_option("stream_slot") == 0
    # the last round (of four) staged its own bytes and nothing else: stream 0's seventh surface, no carry frame
    assert c.stage_bytes() == mat.mux[0][0][6].nbytes + mat.mux[0][1][6].nbytes
    assert c.stream_call().tolist() == [1, 1, 1, 2]
    assert [s[0] for s in state(c)] == [7, 5, 3, 6, 0, 0, 0, 0]
