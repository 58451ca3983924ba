"""Stream slots on the device (include/avd.h, options "stream_slot" / "stream_reset" / "stream_frames"): calls that continue one clip.

Contract: with slot k selected, a call of n frames on a filled slot returns, bit for bit and in both Farneback modes, records [1:] of the same
call made on the slot's frame followed by the n frames; on an empty slot what it returns today.  So a clip sent in chunks through a slot gives
the records of the clip sent whole -- every comparison below is np.array_equal on the records against that whole-clip call made on a context
that never selects a slot (``ref``, one per mode, created for this module).  Where no whole-clip call exists (a stream whose chunks change
layout and geometry) the records are put together from calls without a slot: avd_preprocess_* per chunk (moments, hash bits, 320 x 320
gray) and the whole-clip call on all the gray frames as one 320 x 320 clip (flow statistics and flag words).

Frames are 48 x 64 to 64 x 96; every streaming context is created by its test.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import avd_hip  # noqa: E402
from avd_hip import AvdError, Pixels, _lib, synth  # noqa: E402
from tests.content_families import pink, u8  # noqa: E402

FAST, EXACT = 1, 0
MODES = pytest.mark.parametrize("mode", [FAST, EXACT], ids=["fast", "exact"])
REC = avd_hip.RECORD_DTYPE


# ---- content (generated once) ---------------------------------------------------------------------------------------------------------
def _bgr(gray):
    return np.ascontiguousarray(np.repeat(np.asarray(gray)[..., None], 3, axis=-1))


class Material:
    def __init__(self):
        a = synth.make_clip(3, 48, 64, seed=1, dup_every=0, scene_cut=False)
        b = synth.make_clip(3, 48, 64, seed=2, dup_every=0, scene_cut=False)
        # 7 frames: frame 3 duplicates frame 2 (the pair lies across the boundaries of (3, 1, 3) and 1 x 7), frames 4 .. 6 are another scene.
        # The pictures are window-boxed (rows 8 .. 27, columns 8 .. 35 of 48 x 64 on limited-range black).  That is what makes the flow of the
        # duplicate EXACTLY zero: cv2's FarnebackUpdateMatrices takes r2 = r3 = 0 for the neighbour frame in its last row and column (the
        # bilinear gather would leave the image; oracle/avd_oracle.c, avdo_update_matrices), so there h = b / 2 of the frame itself -- two
        # bit-identical frames with texture at the bottom or right edge have a small non-zero flow in cv2, in the oracle and so in both modes
        # (1e-6 .. 1e-3 px mean on unboxed clips), and only a frame that is flat there at every pyramid level has none.
        boxed = np.full((7, 48, 64, 3), 16, np.uint8)
        boxed[:, 8:28, 8:36] = np.stack([a[0], a[1], a[2], a[2], b[0], b[1], b[2]])[:, 8:28, 8:36]
        self.clip7 = boxed
        # a static background with a moving patch, 64 x 96: every pair is flagged by the fast level kernels (border sign; tests/content_families.py
        # static_local_change, tests/history_calls.py big_clip)
        bg = u8(pink(np.random.default_rng(5), 1.2, size=480)[100:164, 100:196])
        base = []
        for k in range(8):
            f = bg.copy()
            f[10 + 5 * k:16 + 5 * k, 8 + 9 * k:18 + 9 * k] = 255 - f[10 + 5 * k:16 + 5 * k, 8 + 9 * k:18 + 9 * k]
            base.append(f)
        self.patch = _bgr(np.stack(base))
        self.other = synth.make_clip(4, 56, 80, seed=3, dup_every=2)
        self.second = synth.make_clip(6, 64, 96, seed=4, dup_every=0)             # the second stream of the interleaved test: another geometry
        self.long = synth.make_clip(8, 48, 64, seed=5, dup_every=0)[np.arange(515) % 8]
        self.wav = (np.sin(np.arange(20000) * 0.05) * 0.3).astype(np.float32)
        self.surfaces = list(zip(*synth.bgr_to_nv12(synth.make_clip(7, 64, 96, seed=6, dup_every=3))))


@pytest.fixture(scope="module")
def mat():
    return Material()


@pytest.fixture(scope="module")
def ref():
    """mode -> a context that never selects a slot: the whole-clip calls"""
    ctxs = {}
    for mode in (FAST, EXACT):
        ctxs[mode] = avd_hip.Context(0)
        ctxs[mode].set_option("fb_mode", mode)
    yield ctxs
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


def split(clip, sizes):
    assert sum(sizes) == len(clip)
    at = np.cumsum((0,) + tuple(sizes))
    return [clip[a:b] for a, b in zip(at, at[1:])]


def through_slot(c, slot, chunks, call=None):
    """the chunks in turn through an emptied slot -> their records, concatenated"""
    call = call or (lambda c, k, x: c.analyze_frames(x))
    c.stream_reset(slot)
    c.stream_slot(slot)
    out = [call(c, k, x) for k, x in enumerate(chunks)]
    c.stream_slot(0)
    return np.concatenate(out)


def same(got, want):
    return got.dtype == REC and np.array_equal(got, want) and got.tobytes() == want.tobytes()


# ---- splits ---------------------------------------------------------------------------------------------------------------------------
def _by_entry(c, k, x):
    """one chunk through another entry point each: the strided call, a batch of one, a picture, a frame list"""
    return [lambda: c.analyze_frames(x), lambda: c.analyze_batch([x])[0], lambda: c.analyze_pictures([x])[0],
            lambda: c.analyze_frame_lists([(list(x), _lib.AVD_FMT_BGR24)])[0]][k % 4]()


@MODES
@pytest.mark.parametrize("sizes", [(7,), (3, 1, 3), (1,) * 7], ids=["7", "3-1-3", "1x7"])
def test_splits_give_the_whole_clip(mat, ref, new_ctx, mode, sizes):
    whole = ref[mode].analyze_frames(mat.clip7)
    # what the clip was built for: the duplicate (ham 0, flow exactly 0) and the cut lie across the boundaries of (3, 1, 3)
    assert whole["ham"][0] == -1 and whole["ham"][3] == 0 and whole["flow_mean"][3] == 0.0 and whole["flow_var"][3] == 0.0
    assert whole["ham"][4] > 0 and whole["flow_mean"][4] > 0.0
    c = new_ctx(mode)
    got = through_slot(c, 1, split(mat.clip7, sizes), _by_entry)
    assert same(got, whole), (got, whole)
    c.stream_slot(1)
    assert c.stream_frames() == 7


@MODES
def test_empty_slot_is_todays_call_and_frames_are_counted(mat, ref, new_ctx, mode):
    c = new_ctx(mode)
    a, b = mat.clip7[:3], mat.clip7[3:]
    assert c.get_option("stream_slot") == 0 and c.stream_frames() == 0
    c.stream_slot(3)
    assert c.get_option("stream_slot") == 3 and c.stream_frames() == 0
    got = c.analyze_frames(a)
    assert got["ham"][0] == -1 and got["flow_mean"][0] == 0.0 and got["reserved"][0] == 0
    assert same(got, ref[mode].analyze_frames(a))
    assert c.stream_frames() == 3
    assert c.analyze_frames(a[:0]).size == 0 and c.stream_frames() == 3            # a call without frames
    c.analyze_frames(b)
    assert c.stream_frames() == 7
    c.stream_slot(4)
    assert c.stream_frames() == 0                                                  # another slot
    c.stream_slot(0)
    assert c.stream_frames() == 0                                                  # no slot
    c.stream_slot(3)
    assert c.stream_frames() == 7
    assert c.get_option("stream_reset") == 0
    c.stream_reset(4)
    assert c.stream_frames() == 7
    c.stream_reset(3)
    assert c.stream_frames() == 0 and c.get_option("stream_reset") == 0
    assert same(c.analyze_frames(b), ref[mode].analyze_frames(b))                  # emptied: a new clip
    c.stream_slot(5)
    c.analyze_frames(a)
    c.stream_reset(0)                                                              # all slots
    assert c.stream_frames() == 0
    c.stream_slot(3)
    assert c.stream_frames() == 0


# ---- a boundary pair the fast kernels flag ----------------------------------------------------------------------------------------------
def test_flagged_boundary_pair_is_rerun_exactly(mat, ref, new_ctx):
    clip = mat.patch[:4]
    whole, exact = ref[FAST].analyze_frames(clip), ref[EXACT].analyze_frames(clip)
    assert whole["reserved"][2] != 0, "precondition: the fast kernels flag the pair across the boundary"
    c = new_ctx(FAST)
    c.stream_slot(1)
    first = c.analyze_frames(clip[:2])
    got = c.analyze_frames(clip[2:])
    assert got["reserved"][0] != 0
    assert c.get_option("rerun_pairs") == np.count_nonzero(got["reserved"]) >= 1
    assert same(np.concatenate([first, got]), whole)
    for field in ("flow_mean", "flow_var", "ham", "lap_sum", "lap_sumsq"):
        assert got[field][0].tobytes() == exact[field][2].tobytes(), field         # the exact kernels' result, bit for bit
    # and in exact mode, where nothing is flagged, the split is the whole clip too
    e = new_ctx(EXACT)
    assert same(through_slot(e, 1, split(clip, (2, 2))), exact)


# ---- one stream whose chunks change layout and geometry ----------------------------------------------------------------------------------
def _p010(y, uv):
    return Pixels((y.astype(np.uint16) << 8, uv.astype(np.uint16) << 8), _lib.AVD_FMT_P010)


@MODES
def test_chunks_may_change_layout_and_geometry(ref, new_ctx, mode):
    bgr = synth.make_clip(2, 48, 64, seed=11, dup_every=0, scene_cut=False)
    y1, uv1 = synth.bgr_to_nv12(synth.make_clip(3, 64, 96, seed=12, dup_every=0, scene_cut=False))
    i420 = synth.nv12_to_i420(*synth.bgr_to_nv12(synth.make_clip(2, 56, 80, seed=13, dup_every=0, scene_cut=False)))
    frames420 = [tuple(p[i] for p in i420) for i in range(2)]
    wide = _p010(*synth.bgr_to_nv12(synth.make_clip(2, 48, 96, seed=14, dup_every=0, scene_cut=False)))
    c = new_ctx(mode)
    c.stream_slot(2)
    got = np.concatenate([c.analyze_frames(bgr), c.analyze_frames_nv12(y1, uv1),
                          c.analyze_frame_lists([(frames420, _lib.AVD_FMT_I420)])[0], c.analyze_pictures([wide], [1])[0]])
    assert c.stream_frames() == 9
    # the reference, from the calls that know no slot
    r = ref[mode]
    parts = [r.preprocess_bgr(bgr), r.preprocess_nv12(y1, uv1), r.preprocess_frame_list(frames420, _lib.AVD_FMT_I420), r.preprocess_picture(wide, 1)]
    small, bits, s, q = (np.concatenate([p[i] for p in parts]) for i in range(4))
    # the flow statistics and flag words of the nine gray frames: the whole-clip call on them as a 320 x 320 clip with B = G = R, which is its
    # own 320 x 320 gray image (checked), so its pairs are the stream's pairs; its moments and hash bits are those of other pictures
    gray = r.analyze_frames(_bgr(small))
    assert np.array_equal(r.debug_fetch("small", (9, 320, 320), np.uint8), small)
    want = np.zeros(9, REC)
    want["lap_sum"], want["lap_sumsq"] = s, q
    want["ham"][0] = -1
    want["ham"][1:] = (bits[1:] != bits[:-1]).sum(axis=1)
    for field in ("flow_mean", "flow_var", "reserved"):
        want[field] = gray[field]
    assert same(got, want), (got, want)


# ---- a continued call of two Farneback chunks --------------------------------------------------------------------------------------------
@MODES
def test_a_continued_call_of_514_frames(mat, ref, new_ctx, mode):
    whole = ref[mode].analyze_frames(mat.long)                   # 515 frames: 514 pairs, the scratch holds 512
    c = new_ctx(mode)
    got = through_slot(c, 8, split(mat.long, (1, 514)))
    assert same(got, whole)


# ---- other work between two chunks --------------------------------------------------------------------------------------------------------
@MODES
def test_work_between_two_chunks(mat, ref, new_ctx, mode):
    whole = ref[mode].analyze_frames(mat.clip7)
    c = new_ctx(mode)
    c.stream_slot(1)
    first = c.analyze_frames(mat.clip7[:3])
    c.stream_slot(0)
    assert same(c.analyze_frames(mat.other), ref[mode].analyze_frames(mat.other))            # a slot-0 clip of other content, another geometry
    small = c.preprocess_bgr(mat.second)[0]
    c.farneback_pairs(small)
    c.release_workspace()
    c.audio_features(mat.wav, 2000)
    c.stream_slot(1)
    assert c.stream_frames() == 3
    c.preprocess_bgr(mat.other)                                                              # the entry points that ignore the option, with it set
    c.farneback_pairs(small[:3])
    assert c.stream_frames() == 3
    second = c.analyze_frames(mat.clip7[3:])
    assert same(np.concatenate([first, second]), whole)


# ---- two slots interleaved ----------------------------------------------------------------------------------------------------------------
@MODES
def test_two_slots_interleaved(mat, ref, new_ctx, mode):
    a, b = mat.clip7, mat.second
    c = new_ctx(mode)
    out = {1: [], 2: []}
    for slot, chunk in ((1, a[:4]), (2, b[:2]), (1, a[4:]), (2, b[2:])):
        c.stream_slot(slot)
        out[slot].append(c.analyze_frames(chunk))
    assert same(np.concatenate(out[1]), ref[mode].analyze_frames(a))
    assert same(np.concatenate(out[2]), ref[mode].analyze_frames(b))


# ---- asynchronous chunks back to back ------------------------------------------------------------------------------------------------------
@MODES
def test_two_async_chunks_without_a_synchronize_between(mat, ref, new_ctx, mode):
    clip = mat.patch[:5]                                         # every pair flagged in fast mode: both calls leave a re-run to the drain
    whole = ref[mode].analyze_frames(clip)
    c = new_ctx(mode)
    c.stream_slot(1)
    r1, r2 = np.zeros(2, REC), np.zeros(3, REC)
    k1 = c.analyze_frames_async(clip[:2], r1)
    k2 = c.analyze_frames_async(clip[2:], r2)                    # drains the first call (the existing rule), then continues it
    c.synchronize()
    del k1, k2
    assert same(np.concatenate([r1, r2]), whole)
    if mode == FAST:
        assert r2["reserved"][0] != 0 and c.get_option("rerun_pairs") == 3


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
@MODES
def test_refusals_leave_the_slot_alone(mat, ref, new_ctx, mode):
    whole = ref[mode].analyze_frames(mat.clip7)
    c = new_ctx(mode)
    c.stream_slot(2)
    first = c.analyze_frames(mat.clip7[:3])
    for bad in (9, -1):
        with pytest.raises(AvdError, match=r"stream_slot: .*1 \.\.\. 8"):
            c.stream_slot(bad)
        assert c.get_option("stream_slot") == 2 and c.stream_frames() == 3
        with pytest.raises(AvdError, match=r"stream_reset: .*1 \.\.\. 8"):
            c.stream_reset(bad)
        assert c.stream_frames() == 3
    with pytest.raises(AvdError, match="unknown option"):
        c.set_option("stream_frames", 0)                                            # read-only
    with pytest.raises(AvdError, match="stream_slot: one clip per call"):
        c.analyze_batch([mat.clip7[3:5], mat.clip7[5:]])
    assert c.stream_frames() == 3
    with pytest.raises(AvdError, match="stream_slot: one clip per call"):
        c.analyze_batch_async([mat.clip7[3:5], mat.other], np.zeros(6, REC))
    assert c.stream_frames() == 3
    with pytest.raises(AvdError):
        c.analyze_frames(np.zeros((2, 16, 16, 3), np.uint8))                        # a clip the library does not take (smaller than 32 x 32)
    assert c.stream_frames() == 3
    second = c.analyze_batch([mat.clip7[3:], mat.clip7[:0]])[0]                      # one non-empty clip: accepted, whatever empty ones the call lists
    assert c.stream_frames() == 7
    assert same(np.concatenate([first, second]), whole)
    # with no slot selected the same batch is what it always was
    c.stream_slot(0)
    two = c.analyze_batch([mat.clip7[3:5], mat.clip7[5:]])
    assert same(two[0], ref[mode].analyze_frames(mat.clip7[3:5])) and same(two[1], ref[mode].analyze_frames(mat.clip7[5:]))


# ---- the streaming analyzer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 2, 5])
def test_streaming_analyzer_with_resident_carry(mat, ref, new_ctx, chunk):
    want = avd_hip.FrameAnalyzer(ctx=ref[FAST], chunk=chunk).records_stream_nv12(iter(mat.surfaces))
    assert same(want, ref[FAST].analyze_frames_nv12(*(np.stack(p) for p in zip(*mat.surfaces))))
    c = new_ctx(FAST)
    got = avd_hip.FrameAnalyzer(ctx=c, chunk=chunk).records_stream_nv12(iter(mat.surfaces), resident_carry=True)
    assert same(got, want)
    assert c.get_option("stream_slot") == 0
    # the last chunk staged its own frames and nothing else: no carry frame
    last = len(mat.surfaces) % chunk or chunk
    frame_bytes = sum(p.nbytes for p in mat.surfaces[0])
    assert c.stage_bytes() == last * frame_bytes
    c.stream_slot(1)
    assert c.stream_frames() == len(mat.surfaces)


# ---- profiling ------------------------------------------------------------------------------------------------------------------------------
def test_regions_of_a_continued_call_tile_its_stages(mat, new_ctx):
    """The copies that restore and save the slot's frame lie inside existing regions: with K = kernel_ms() and S = stage_ms() of a continued
    call without a flagged pair, the regions recorded between two stage events sum to that stage (they share the events; 1e-5 of the stage
    covers the float32 rounding of at most 96 terms, as tests/test_gpu_profiling.py derives it), and no id appears that a plain call lacks."""
    clip = synth.make_clip(6, 96, 128, seed=1, dup_every=0, scene_cut=False)
    c = new_ctx(FAST)
    c.stream_slot(1)
    c.analyze_frames(clip[:3])
    c.set_profiling(True)
    rec = c.analyze_frames(clip[3:])
    K, S = c.kernel_ms(), c.stage_ms()
    c.set_profiling(False)
    print(f"\n[stream profiling] K {K}\n                   S {S}")
    assert not rec["reserved"].any() and c.get_option("rerun_pairs") == 0
    assert set(K) == set(avd_hip.Context.KERNEL_IDS)
    flow = ("pyramid", "polyexp", "level40", "flow_up80", "level80", "flow_up160", "level160", "flow_up320", "level320", "stats", "records")
    for inner, outer in ((K["preprocess"] + K["hash"], S[0]), (sum(K[k] for k in flow), S[2]), (K["other"], S[1] + S[3])):
        assert outer > 0 and abs(inner - outer) <= 1e-5 * outer, (inner, outer, K, S)
    assert K["rerun"] == 0.0
