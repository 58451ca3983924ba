"""The profiling instruments on the device, held to the text of include/avd.h (avd_set_profiling, avd_stage_ms, enum avd_kernel_id,
avd_kernel_ms, avd_timer_*) and to the ``timing_reps`` hooks of the extensions.  Run with ``-s``: every test prints what it measures.

No assertion here is a speed expectation.  Each is one of three kinds:

  structural   an id is zero or positive, a value is unchanged, an error is raised;
  nesting      events on one in-order stream are ordered, so an inner interval is never longer than the outer one;
  outside      a bound that does not come from the code under test: the host clock around a call that ends in a synchronise, torch's own
               events on torch's stream, the hardware peaks of the MI355X.

eps(x) = 1e-5 * x is DERIVED, not measured: hipEventElapsedTime returns float32; a sum of at most 97 such terms, each rounded by 2^-24, is off
by less than 6e-6 of the outer interval, and timestamps of one clock keep nested intervals nested exactly.

With K = kernel_ms() and S = stage_ms() of one call, the events of a one-clip call lie on the stream in this order (| = one event that both
decompositions use; header: the region that opens a stage "is bounded by the stage's OWN event"):

  wake |s0 = preprocess| [hash] |s1 = other| (table upload) |s2 = pyramid| [polyexp .. stats][records] |s3 = other| (copy-out) |s4 = end|
  and, when the last chunk had flagged pairs, behind s4:  [rerun: exact kernels, records again, copy-out again] end

so K[preprocess] + K[hash] <= S[0], the Farneback / statistics / record ids <= S[2], K[other] <= S[1] + S[3], and the deferred re-run lies
outside every stage."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import avd_hip  # noqa: E402
from avd_hip import synth  # noqa: E402
from tests import history_calls as T  # noqa: E402

IDS = avd_hip.Context.KERNEL_IDS
ALWAYS = {"preprocess", "hash", "records", "other"}                     # every call
FLOW = {"pyramid", "polyexp", "level40", "level80", "level160", "level320", "stats"}     # every call with a pair of frames
FLOW_UP = {"flow_up80", "flow_up160", "flow_up320"}
IN_STAGE2 = sorted((FLOW | FLOW_UP | {"records"}))

HBM_PEAK = 8.0e12        # bytes / s: MI355X_MICROARCH.md, table "At a glance", row "HBM3E peak BW: 8.0 TB/s spec"
BF16_PEAK = 2.5e15       # FLOP / s: the same table, row "Peak BF16/FP16 MFMA: ~2.5 PF dense"


def eps(x):
    return 1e-5 * x


# ---- content ---------------------------------------------------------------------------------------------------------------------------
def plain_clip(seed=1):
    """one smooth translating scene, no cut: no pair is flagged (asserted where it is used)"""
    return synth.make_clip(6, 96, 128, seed=seed, dup_every=0, scene_cut=False)


def flagged_clip():
    """the four 320 x 320 frames of tests/history_calls.py (FB_FLAGGED: pairs 0 and 2 are flagged) as a BGR clip"""
    return T._bgr(T.fb_frames())


def batch_of_three(first):
    """three clips of two geometries, `first` at both ends"""
    assert first.shape[1:3] != (48, 64)
    return [first, synth.make_clip(3, 48, 64, seed=48, dup_every=0, scene_cut=False), first.copy()]


# ---- the expected regions, from the header's description of the options ------------------------------------------------------------------
def expected_regions(opts, pairs=True, flagged=False):
    """ids that must be > 0 for a call under `opts` (include/avd.h, avd_set_option); every other id must be exactly 0.
    fb_mode 0: the exact kernels, a k_flow_up launch in front of the 80-, 160- and 320-px levels, never a re-run.
    fb_mode 1: "fb_fold_up" bit 0 -- the 320-px level resizes the 160-px flow itself (no flow_up320); bit 1 -- the 160- and 80-px levels do so
    in a prologue (no flow_up160, no flow_up80); bit 2 changes the launch count of the 80- and 40-px levels, not the regions.
    "fb_fold_up160" -- the 160-px level resizes itself whenever it runs as ONE strip per pair ("fb_wide160" 1; 2 = by what is in flight: a clip
    alone runs two strips), so no flow_up160 then; with two strips "fb_fold_up" decides.  AVD_K_RERUN: fast mode, "fb_rerun" on, a flagged pair."""
    want = set(ALWAYS)
    if not pairs:
        return want
    want |= FLOW
    if opts.get("fb_mode", 1) == 0:
        return want | FLOW_UP
    fold, fold160, wide = opts.get("fb_fold_up", 5), opts.get("fb_fold_up160", 1), opts.get("fb_wide160", 2)
    one_strip = wide == 1                                  # 2: the test's context is the only one with a call in flight
    if not fold & 1:
        want.add("flow_up320")
    if not fold & 2:
        want.add("flow_up80")
        if not (fold160 and one_strip):
            want.add("flow_up160")
    if flagged and opts.get("fb_rerun", 1):
        want.add("rerun")
    return want


def check_regions(K, want, tag):
    assert set(K) == set(IDS)
    for name in IDS:
        if name in want:
            assert K[name] > 0, (tag, name, K)
        else:
            assert K[name] == 0.0, (tag, name, K)


def check_nesting(K, S, opts, tag, rerun_inline=False):
    """(d) of the module's contract; rerun_inline: a call of several chunks settles all but its last chunk inside stage 2"""
    inner = K["preprocess"] + K["hash"]
    assert inner <= S[0] + eps(S[0]), (tag, "stage 0", inner, S[0])
    inner = sum(K[k] for k in IN_STAGE2) + (K["rerun"] if rerun_inline else 0.0)
    assert inner <= S[2] + eps(S[2]), (tag, "stage 2", inner, S[2])
    assert K["other"] <= S[1] + S[3] + eps(S[1] + S[3]), (tag, "stages 1 + 3", K["other"], S[1], S[3])
    two_kernel = opts.get("fb_mode", 1) == 0 and not opts.get("fb_fused", 0xF) & 1
    if two_kernel:
        assert S[4] > 0 and S[5] > 0, (tag, S)
    else:
        assert S[4] <= K["level320"] + eps(K["level320"]), (tag, "stage 4", S[4], K["level320"])
        assert S[5] == 0.0, (tag, S)


def profiled(ctx, call):
    """-> (what `call` returns, kernel_ms(), stage_ms()) of a call made with profiling on"""
    ctx.set_profiling(True)
    try:
        out = call(ctx)
        return out, ctx.kernel_ms(), ctx.stage_ms()
    finally:
        ctx.set_profiling(False)


def _blocking(clip):
    return lambda c: c.analyze_frames(clip)


def _async(clip):
    def call(c):
        rec = np.zeros(len(clip), avd_hip.RECORD_DTYPE)
        keep = c.analyze_frames_async(clip, rec)
        c.synchronize()
        del keep
        return rec
    return call


def _batch(clips):
    return lambda c: np.concatenate(c.analyze_batch(clips))


def _context(opts):
    c = avd_hip.Context(0)
    for k, v in opts.items():
        c.set_option(k, v)
    return c


# ---- 2 (a) + (d): which regions exist, and how they nest --------------------------------------------------------------------------------
ROWS = [("fast-defaults", {}, "plain", "blocking")]
ROWS += [(f"fast-fold{f}-up160_{u}-wide{w}", {"fb_fold_up": f, "fb_fold_up160": u, "fb_wide160": w}, "plain", "blocking")
         for f in (0, 2, 7) for u in (0, 1) for w in (0, 1)]
ROWS += [("exact-fused-0xF", {"fb_mode": 0, "fb_fused": 0xF}, "plain", "blocking"),
         ("exact-fused-0x0", {"fb_mode": 0, "fb_fused": 0x0}, "plain", "blocking"),
         ("one-frame", {}, "one", "blocking"),
         ("batch-of-three", {}, "batch", "blocking"),
         ("flagged-fast", {}, "flagged", "blocking"),
         ("flagged-fast-no-rerun", {"fb_rerun": 0}, "flagged", "blocking"),
         ("flagged-exact", {"fb_mode": 0}, "flagged", "blocking"),
         ("flagged-fast-async", {}, "flagged", "async")]


@pytest.mark.parametrize("tag,opts,content,how", ROWS, ids=[r[0] for r in ROWS])
def test_regions_and_nesting(tag, opts, content, how):
    clip = {"plain": plain_clip, "one": lambda: plain_clip()[:1], "batch": plain_clip, "flagged": flagged_clip}[content]()
    call = _batch(batch_of_three(clip)) if content == "batch" else (_async(clip) if how == "async" else _blocking(clip))
    with _context(opts) as c:
        rec, K, S = profiled(c, call)
        rerun = c.get_option("rerun_pairs")
    flagged = content == "flagged"
    print(f"\n[profiling] {tag}: rerun_pairs {rerun}  sum K {sum(K.values()):.4f} ms  S {[round(v, 4) for v in S]}\n            K {({k: round(v, 4) for k, v in K.items()})}")
    will_rerun = flagged and opts.get("fb_mode", 1) == 1 and opts.get("fb_rerun", 1) == 1
    if will_rerun:
        assert rerun > 0 and np.count_nonzero(rec["reserved"]) == rerun, tag       # the clip is what the row claims
    else:
        assert rerun == 0 and not rec["reserved"].any(), tag
    check_regions(K, expected_regions(opts, pairs=content != "one", flagged=flagged), tag)
    assert len(S) == 6 and all(v >= 0 for v in S)
    assert S[0] > 0 and S[2] > 0 and S[3] > 0, (tag, S)
    assert (S[1] > 0) if content == "batch" else (S[1] >= 0), (tag, S)             # the clip-start table: calls with several clips
    check_nesting(K, S, opts, tag)
    if will_rerun:
        # the deferred re-run: every stage event was recorded at enqueue, the re-run lies behind them
        total, stages = sum(K.values()), sum(S[:4])
        assert total - stages >= K["rerun"] - eps(total), (tag, total, stages, K["rerun"])


def test_timer_contains_both_decompositions():
    """(d), the timer: with avd_timer_start in front of an asynchronous call and avd_timer_stop behind it, T holds every region and every
    stage, and the host clock around the sequence (avd_timer_stop synchronises) holds T.  (e): the two decompositions differ by nothing but
    gaps between adjacent event packets, whose size is measured independently of the library: torch events back to back on torch's stream."""
    import torch
    clip = plain_clip()
    t0 = time.perf_counter()
    s = torch.cuda.current_stream()
    torch.cuda.synchronize()
    print(f"\n[profiling] torch's stream ready after {time.perf_counter() - t0:.2f} s")
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(101)]
    for e in evs:
        e.record(s)
    s.synchronize()
    gap = float(np.median([evs[i].elapsed_time(evs[i + 1]) for i in range(100)]))
    with avd_hip.Context(0) as c:
        c.analyze_frames(clip)                              # the workspace is reserved: the timed call allocates nothing
        rec = np.zeros(len(clip), avd_hip.RECORD_DTYPE)
        c.set_profiling(True)
        try:
            t0 = time.perf_counter()
            c.timer_start()
            keep = c.analyze_frames_async(clip, rec)
            timer = c.timer_stop()
            wall = (time.perf_counter() - t0) * 1e3
            c.synchronize()
            del keep
            K, S = c.kernel_ms(), c.stage_ms()
        finally:
            c.set_profiling(False)
        assert c.get_option("rerun_pairs") == 0
    total, stages = sum(K.values()), sum(S[:4])
    allow = 6 * 10 * gap
    print(f"\n[profiling] default row: T {timer:.4f} ms  sum K {total:.4f} ms  sum S[0..3] {stages:.4f} ms  wall {wall:.4f} ms\n"
          f"[profiling] event-to-event gap on an idle torch stream: median {gap * 1e3:.2f} us; |sum K - sum S| = {abs(total - stages) * 1e3:.2f} us, "
          f"allowance 6 x 10 x median = {allow * 1e3:.2f} us")
    assert gap > 0
    assert total <= timer + eps(timer), (total, timer)
    assert stages <= timer + eps(timer), (stages, timer)
    assert timer <= wall, (timer, wall)
    assert abs(total - stages) <= allow, (total, stages, gap)


# ---- 2 (b): the last drained call, and nothing else ----------------------------------------------------------------------------------------
def test_values_change_only_when_a_profiled_call_is_drained():
    clip, other = plain_clip(), plain_clip(seed=2)[:4]
    with avd_hip.Context(0) as c:
        _, K0, S0 = profiled(c, _blocking(clip))
        c.set_profiling(True)
        try:
            rec = np.zeros(len(other), avd_hip.RECORD_DTYPE)
            keep = c.analyze_frames_async(other, rec)
            assert c.kernel_ms() == K0 and c.stage_ms() == S0       # floats compared exactly: the same bits until the call is drained
            c.synchronize()
            del keep
            K1, S1 = c.kernel_ms(), c.stage_ms()
            assert K1 != K0 and S1 != S0                            # twenty-one event times of another call
        finally:
            c.set_profiling(False)
        c.analyze_frames(clip)
        assert c.kernel_ms() == K1 and c.stage_ms() == S1           # profiling off: nothing is recorded, nothing replaced
        rec = np.zeros(len(clip), avd_hip.RECORD_DTYPE)
        keep = c.analyze_frames_async(clip, rec)
        c.synchronize()
        del keep
        assert c.kernel_ms() == K1 and c.stage_ms() == S1


def test_other_entry_points_leave_the_analyze_calls_values():
    """header: "the LAST drained avd_analyze_* call".  avd_farneback_pairs runs the launchers that record kernel marks; a bare avd_synchronize
    behind it must not read them as a call's timeline."""
    clip = plain_clip()
    rng = np.random.default_rng(0)
    smalls = np.ascontiguousarray(flagged_clip()[..., 0])
    with avd_hip.Context(0) as c:
        c.vit_set_weights((rng.standard_normal((768, 768)) * 0.02).astype(np.float32), None)
        c.set_profiling(True)
        try:
            c.analyze_frames(clip)
            K0, S0 = c.kernel_ms(), c.stage_ms()
            c.preprocess_bgr(clip)
            assert c.kernel_ms() == K0 and c.stage_ms() == S0
            c.farneback_pairs(smalls)
            assert c.get_option("rerun_pairs") > 0                  # the call ran, its re-run included
            assert c.kernel_ms() == K0 and c.stage_ms() == S0
            c.vit_patch_embed(clip[:2])
            c.audio_features(rng.standard_normal(16000).astype(np.float32), 8000)
            c.synchronize()                                         # nothing is pending
            assert c.kernel_ms() == K0, "a call other than avd_analyze_* replaced the kernel times"
            assert c.stage_ms() == S0
            c.synchronize()
            assert c.kernel_ms() == K0 and c.stage_ms() == S0
        finally:
            c.set_profiling(False)
    check_regions(K0, expected_regions({}), "before the other entry points")


# ---- 2 (c): an overflow is reported, then forgotten ---------------------------------------------------------------------------------------
OVERFLOW_TEXT = "more kernel regions than the library records"       # header (avd_kernel_ms) and the library's message


def test_overflow_is_reported_for_that_call_only():
    clips = [synth.make_clip(2, 32, 32, seed=100 + i, dup_every=0, scene_cut=False) for i in range(48)]     # 2 x 48 ingest regions alone
    with avd_hip.Context(0) as c:
        c.set_profiling(True)
        try:
            recs = c.analyze_batch(clips)
            with pytest.raises(avd_hip.AvdError, match=OVERFLOW_TEXT):
                c.kernel_ms()
            S = c.stage_ms()
            assert S[0] > 0 and S[1] > 0 and S[2] > 0 and S[3] > 0, S        # the five stage events are the call's own
        finally:
            c.set_profiling(False)
        c.set_profiling(False)
        plain = c.analyze_batch(clips)
        assert np.concatenate(recs).tobytes() == np.concatenate(plain).tobytes()
        rec, K, S = profiled(c, _blocking(plain_clip()))
    assert not rec["reserved"].any()
    check_regions(K, expected_regions({}), "after the overflow")
    check_nesting(K, S, {}, "after the overflow")


def test_overflow_of_farneback_pairs_is_not_the_next_calls():
    """avd_farneback_pairs with profiling on records ten marks per chunk in exact mode (pyramid, polyexp, four levels, three resizes,
    statistics): ten chunks of 512 pairs are more than the 96 the library holds.  Nobody drains that overflow as a call's; the next profiled
    avd_analyze_* call must report normally."""
    import torch
    chunks = 10
    base = torch.from_numpy(np.ascontiguousarray(synth.make_clip(8, 320, 320, seed=3, dup_every=0, scene_cut=False)[..., 0])).cuda()
    frames = base[torch.arange(chunks * 512 + 1, device="cuda") % 8]
    with avd_hip.Context(0) as c:
        c.set_option("fb_mode", 0)
        c.set_profiling(True)
        try:
            t0 = time.perf_counter()
            fm, fv = c.farneback_pairs(frames)
            print(f"\n[profiling] avd_farneback_pairs, {chunks * 512} pairs in exact mode: {(time.perf_counter() - t0) * 1e3:.1f} ms wall")
            assert len(fm) == chunks * 512 and np.array_equal(fm[:8], fm[8:16]) and np.array_equal(fv[512:520], fv[:8])
            c.analyze_frames(plain_clip())
            K, S = c.kernel_ms(), c.stage_ms()              # raises on a library that carries the overflow over
        finally:
            c.set_profiling(False)
    check_regions(K, expected_regions({"fb_mode": 0}), "after avd_farneback_pairs")
    check_nesting(K, S, {"fb_mode": 0}, "after avd_farneback_pairs")


# ---- 2 (f): waiting for a producer is not the library's time -------------------------------------------------------------------------------
def test_the_wait_for_a_producer_is_in_the_timer_and_in_no_region():
    import torch
    dev = torch.device("cuda", 0)
    clip = torch.from_numpy(plain_clip()).to(dev)
    a = torch.randn(4096, 4096, device=dev)
    b = torch.randn(4096, 4096, device=dev)
    out = torch.empty_like(a)
    s = torch.cuda.current_stream(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def produce(reps):
        e0.record(s)
        for _ in range(reps):
            torch.mm(a, b, out=out)
        e1.record(s)

    produce(1)                                              # the first matmul loads its kernel: not part of any measurement
    s.synchronize()
    reps = 4
    while True:                                             # the repeat count, found once and untimed
        produce(reps)
        s.synchronize()
        if e0.elapsed_time(e1) >= 30.0:
            break
        reps *= 2
        assert reps <= 4096
    with avd_hip.Context(0) as c:
        c.analyze_frames(clip)                              # workspace reserved
        torch.cuda.synchronize()
        rec = np.zeros(clip.shape[0], avd_hip.RECORD_DTYPE)
        c.set_profiling(True)
        try:
            t0 = time.perf_counter()
            produce(reps)
            enqueue_ms = (time.perf_counter() - t0) * 1e3
            c.timer_start()
            c.wait_stream(s.cuda_stream)
            keep = c.analyze_frames_async(clip, rec)
            timer = c.timer_stop()
            c.synchronize()
            del keep
            K, S = c.kernel_ms(), c.stage_ms()
        finally:
            c.set_profiling(False)
        assert c.get_option("rerun_pairs") == 0
    s.synchronize()
    D = e0.elapsed_time(e1)
    total, stages = sum(K.values()), sum(S[:4])
    print(f"\n[profiling] producer: {reps} matmuls of 4096^3, D = {D:.3f} ms on torch's events, enqueued by the host in {enqueue_ms:.3f} ms\n"
          f"[profiling] T {timer:.4f} ms  sum K {total:.4f} ms  sum S[0..3] {stages:.4f} ms")
    assert D >= 20.0, D
    assert timer >= 0.5 * D, (timer, D)                     # milliseconds, and the wait lies inside the timer
    assert total <= timer - 0.5 * D, (total, timer, D)      # the empty launch in front of the first mark keeps it out of the first region
    assert stages <= timer - 0.5 * D, (stages, timer, D)


# ---- 2 (g): a region cannot beat the hardware ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["bgr", "nv12"])
def test_preprocess_region_against_the_hbm_peak(layout):
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    n, h, w = 8, 1080, 1920
    if layout == "bgr":
        planes = (torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=dev, generator=g),)
        call = lambda c: c.analyze_frames(planes[0])
    else:
        planes = (torch.randint(16, 236, (n, h, w), dtype=torch.uint8, device=dev, generator=g),
                  torch.randint(16, 241, (n, h // 2, w), dtype=torch.uint8, device=dev, generator=g))
        call = lambda c: c.analyze_frames_nv12(*planes)
    nbytes = sum(p.numel() for p in planes)
    assert nbytes == (n * h * w * 3 if layout == "bgr" else n * h * w * 3 // 2)
    torch.cuda.synchronize()
    with avd_hip.Context(0) as c:
        call(c)                                             # tables and workspace
        c.set_profiling(True)
        try:
            t0 = time.perf_counter()
            call(c)
            wall = (time.perf_counter() - t0) * 1e3
            K = c.kernel_ms()
        finally:
            c.set_profiling(False)
    floor = nbytes / HBM_PEAK * 1e3
    print(f"\n[profiling] {layout} 8 x 1080p, {nbytes / 1e6:.1f} MB: K[preprocess] {K['preprocess']:.4f} ms = {nbytes / K['preprocess'] / 1e9:.2f} TB/s; "
          f"floor {floor:.4f} ms, wall {wall:.3f} ms")
    assert K["preprocess"] >= floor, (K["preprocess"], floor)
    assert K["preprocess"] <= wall, (K["preprocess"], wall)


# ---- 2 (h): profiling changes no result -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 0], ids=["fast", "exact"])
@pytest.mark.parametrize("content", ["plain", "flagged"])
def test_profiling_changes_no_record(content, mode):
    clip = plain_clip() if content == "plain" else flagged_clip()
    calls = {"blocking": _blocking(clip), "async": _async(clip), "batch": _batch(batch_of_three(clip))}
    with _context({"fb_mode": mode}) as c:
        for how, call in calls.items():
            want = call(c)
            want_rerun = c.get_option("rerun_pairs")
            got, K, _ = profiled(c, call)
            assert got.tobytes() == want.tobytes(), (content, mode, how)
            assert c.get_option("rerun_pairs") == want_rerun, (content, mode, how)
            assert (want_rerun > 0) == (content == "flagged" and mode == 1), (content, mode, how, want_rerun)
            assert (K["rerun"] > 0) == (want_rerun > 0)


# ---- 2 (i): several chunks --------------------------------------------------------------------------------------------------------------------
def test_a_call_of_two_chunks():
    clip = synth.make_clip(8, 32, 32, seed=5, dup_every=0)[np.arange(515) % 8]          # 514 pairs: chunks of 512 and 2
    with avd_hip.Context(0) as c:
        want = c.analyze_frames(clip)
        rerun = c.get_option("rerun_pairs")
        rec, K, S = profiled(c, _blocking(clip))            # kernel_ms() does not raise: 2 x 9 + 6 regions
        assert c.get_option("rerun_pairs") == rerun
    print(f"\n[profiling] two chunks: rerun_pairs {rerun}  K {({k: round(v, 4) for k, v in K.items()})}  S {[round(v, 4) for v in S]}")
    assert rec.tobytes() == want.tobytes()
    assert not rec["reserved"][513:].any()                  # the last chunk has no flagged pair: every re-run of this call ran inside stage 2
    assert (K["rerun"] > 0) == (rerun > 0)
    inner = K["preprocess"] + K["hash"]
    assert inner <= S[0] + eps(S[0]), (inner, S[0])
    inner = sum(K[k] for k in IN_STAGE2) + K["rerun"]
    assert inner <= S[2] + eps(S[2]), (inner, S[2])


# ---- 3: the timing_reps hooks ---------------------------------------------------------------------------------------------------------------
REPS = (2, 8)


def _check_hook(tag, run, floor_ms):
    """run(R) -> (output array, ms or None).  ms is the MEAN of R launches: R * ms fits into the host's time for the call (a sum, or a division
    by R - 1, would not at R = 2), it is not below the hardware floor, and the output is the untimed call's"""
    want, none = run(0)
    assert none is None
    for R in REPS:
        t0 = time.perf_counter()
        got, ms = run(R)
        wall = (time.perf_counter() - t0) * 1e3
        print(f"\n[profiling] {tag}: timing_reps {R}: {ms * 1e3:.2f} us per launch (floor {floor_ms * 1e3:.2f} us), R x ms {R * ms:.4f} ms, wall {wall:.3f} ms")
        assert ms > 0, (tag, R)
        assert R * ms <= wall, (tag, R, ms, wall)
        assert ms >= floor_ms, (tag, R, ms, floor_ms)
        assert np.asarray(got).tobytes() == np.asarray(want).tobytes(), (tag, R)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_hook_vit_patch_embed(bf16):
    frames = synth.make_clip(7, 96, 128, seed=3, dup_every=0)
    rng = np.random.default_rng(0)
    with avd_hip.Context(0) as c:
        c.vit_set_weights((rng.standard_normal((768, 768)) * 0.02).astype(np.float32), rng.standard_normal(768).astype(np.float32))
        _check_hook(f"vit_patch_embed {'bf16' if bf16 else 'f32'}", lambda R: c.vit_patch_embed(frames, timing_reps=R, bf16=bf16),
                    2.0 * (7 * 196) * 768 * 768 / BF16_PEAK * 1e3)
        tok = np.empty((7, 196, 768), np.float32)
        assert c._L.avd_vit_patch_embed(c._h, frames.ctypes.data, 0, 7, 96, 128, 128 * 3, 96 * 128 * 3, tok.ctypes.data, 0, 0, 2, None) == 0
        assert bf16 or tok.tobytes() == c.vit_patch_embed(frames)[0].tobytes()


def test_hook_cnn_forward():
    from avd_hip import cnn as host_cnn
    frames = synth.make_clip(2, 96, 128, seed=4, dup_every=0)
    w, b = host_cnn.seeded_parameters(0)
    nw, nb = avd_hip.Context.cnn_param_counts()
    with avd_hip.Context(0) as c:
        c.cnn_set_weights(w, b)
        _check_hook("cnn_forward", lambda R: c.cnn_forward(frames, timing_reps=R), (2 * nw + 4 * nb) / HBM_PEAK * 1e3)
        logits = np.empty((2, 1000), np.float32)
        assert c._L.avd_cnn_forward(c._h, frames.ctypes.data, 0, 2, 96, 128, 128 * 3, 96 * 128 * 3, logits.ctypes.data, 2, None) == 0
        assert logits.tobytes() == c.cnn_forward(frames)[0].tobytes()


def test_hook_layernorm_and_softmax():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4096, 768)).astype(np.float32)
    g, b = rng.standard_normal(768).astype(np.float32), rng.standard_normal(768).astype(np.float32)
    z = rng.standard_normal((4096, 1000)).astype(np.float32)
    with avd_hip.Context(0) as c:
        _check_hook("layernorm 4096 x 768 f32", lambda R: c.layernorm(x, g, b, timing_reps=R), 2 * x.nbytes / HBM_PEAK * 1e3)
        _check_hook("softmax 4096 x 1000", lambda R: c.softmax(z, timing_reps=R), 2 * z.nbytes / HBM_PEAK * 1e3)
        y = np.empty_like(x)
        assert c._L.avd_layernorm(c._h, x.ctypes.data, 0, 0, 4096, 768, g.ctypes.data, b.ctypes.data, 1e-5, y.ctypes.data, 2, None) == 0
        assert y.tobytes() == c.layernorm(x, g, b)[0].tobytes()
        p = np.empty_like(z)
        assert c._L.avd_softmax(c._h, z.ctypes.data, 0, 4096, 1000, p.ctypes.data, 2, None) == 0
        assert p.tobytes() == c.softmax(z)[0].tobytes()
