"""Option "cv2_model": the library follows the oracle's model switches (include/avd.h; oracle.model(flags), the same bit values).

Masks tested: 1 (GAUSS_MULADD), 8 (THREE_SCALES), 16 (RESIZE_LERP), 25 (all three), and 0 as the control.  The referee is the CPU oracle under
oracle.model(mask).  Bit 16 leaves flow_mean of the small clips bit-identical, so every comparison is on the DENSE flow, never on the statistics alone.

  * avd_farneback_pairs, fb_mode 0, fused and two-kernel path: dense flow, flow_mean, flow_var np.array_equal to the oracle's, and different from
    the same call under mask 0 (no flag is a no-op on the device);
  * the pyramid alone (pyr1 .. pyr3, pyr0 where the blur is not folded) against the oracle's blur + resize under the mask: bits 1 and 16 without
    the schedule;
  * fb_mode 1 on the small clips, two 270 x 480 clips and two pairs the fast kernels flag (a 2-px checkerboard against its inverse, a saturated
    step edge against a ramp): flagged pairs bit for bit, the others within the header's tolerances (rel 1e-6 on the statistics, 1e-5 px on the
    flow); the two ill-posed pairs flagged under every mask; bits 3 and 7 of `reserved` clear under bit 8;
  * through the records: avd_analyze_frames, a stream slot (2 + 3 frames), a batch of two clips, an asynchronous call whose option is changed
    before it is drained;
  * the option itself, the "fb_model" debug buffer, profiling under bit 8, and independence of what the context ran before.
"""
import numpy as np
import pytest

from avd_hip import synth

pytestmark = pytest.mark.gpu

MASKS = [1, 8, 16, 25]
KS = {0: (3, 0.0), 1: (3, 0.5), 2: (9, 1.5), 3: (19, 3.5)}     # ksize, sigma of the pyramid blur per scale (as tests/test_gpu_pyramid_bands.py)
FLOW_TOL = 1e-5                                                # px, include/avd.h


def _bgr(gray):
    return np.repeat(np.ascontiguousarray(gray)[..., None], 3, axis=3)


@pytest.fixture(scope="module")
def clips(oracle):
    """name -> (BGR clip or None, small uint8[n, 320, 320])"""
    out = {}
    for name, (n, h, w, seed) in {"a": (5, 96, 128, 0), "b": (5, 72, 96, 5), "c": (8, 270, 480, 0), "d": (8, 180, 320, 5)}.items():
        clip = synth.make_clip(n, h, w, seed=seed, dup_every=4)
        out[name] = (clip, oracle.preprocess_bgr(clip)[0])
    # two pairs the fast level kernels flag: a 2-px checkerboard against its inverse; a saturated step edge against an unrelated ramp
    yy, xx = np.mgrid[0:320, 0:320]
    chk = (((yy // 2) + (xx // 2)) % 2 * 200).astype(np.uint8)
    step = np.zeros((320, 320), np.uint8)
    step[:, 190:] = 255
    ramp = (np.add.outer(np.arange(320), np.arange(320)) % 256).astype(np.uint8)
    out["checker"] = (None, np.stack([chk, (200 - chk).astype(np.uint8)]))
    out["step"] = (None, np.stack([step, ramp]))
    for _, s in out.values():
        s.setflags(write=False)
    return out


class _Refs:
    """the oracle under a mask, per clip, computed once: flow [np, 320, 320, 2], flow_mean, flow_var"""

    def __init__(self, oracle, clips):
        self.oracle, self.clips, self.cache = oracle, clips, {}

    def __call__(self, mask, name):
        key = (mask, name)
        if key not in self.cache:
            small = self.clips[name][1]
            with self.oracle.model(mask):
                flow = np.stack([self.oracle.farneback(small[p], small[p + 1]) for p in range(len(small) - 1)])
            st = [self.oracle.flow_stats(f) for f in flow]
            r = (flow, np.array([s[0] for s in st], np.float32), np.array([s[1] for s in st], np.float32))
            for a in r:
                a.setflags(write=False)
            self.cache[key] = r
        return self.cache[key]


@pytest.fixture(scope="module")
def refs(oracle, clips):
    return _Refs(oracle, clips)


def _ctx(mask, mode, **options):
    import avd_hip
    c = avd_hip.Context(0)
    c.set_option("fb_mode", mode)
    for k, v in options.items():
        c.set_option(k, v)
    c.set_option("cv2_model", mask)
    return c


@pytest.fixture(scope="module")
def device_default(clips):
    """fused mask -> clip -> the exact mode's dense flow under mask 0"""
    out = {}
    for fused in (0xF, 0):
        with _ctx(0, 0, fb_fused=fused) as c:
            out[fused] = {name: c.farneback_pairs(clips[name][1], want_flow=True)[2] for name in ("a", "b")}
    return out


@pytest.mark.parametrize("fused", [0xF, 0])
@pytest.mark.parametrize("mask", [0] + MASKS)
def test_pairs_exact_mode_is_the_oracle_under_the_mask(clips, refs, device_default, mask, fused):
    with _ctx(mask, 0, fb_fused=fused) as c:
        for name in ("a", "b"):
            fm, fv, flow = c.farneback_pairs(clips[name][1], want_flow=True)
            want, wm, wv = refs(mask, name)
            for p in range(len(want)):
                ndiff = int(np.count_nonzero(flow[p] != want[p]))
                print(f"[cv2_model] mask {mask} fused {fused:#x} clip {name} pair {p}: {ndiff} flow values differ from the oracle")
                assert np.array_equal(flow[p], want[p]), (mask, fused, name, p, ndiff)
            assert np.array_equal(fm, wm) and np.array_equal(fv, wv), (mask, fused, name)
            if mask:
                for p in range(len(want)):
                    assert not np.array_equal(flow[p], device_default[fused][name][p]), ("the flag is a no-op on the device", mask, fused, name, p)
            st = c.fb_model()
            assert st[0] == mask and st[1] == (3 if mask & 8 else 4) and st[3] == (0 if mask & 1 else 1), st.tolist()


@pytest.mark.parametrize("fold_blur", [1, 0])
@pytest.mark.parametrize("mask", [0] + MASKS)
def test_pyramid_alone(oracle, clips, mask, fold_blur):
    small = np.concatenate([clips["a"][1][:3], clips["d"][1][:2]])
    with _ctx(mask, 0, fb_fold_blur=fold_blur) as c:
        c.farneback_pairs(small)
        folded = int(c.fb_model()[3])
        assert folded == (fold_blur if not mask & 1 else 0)
        assert c.get_option("fb_fold_blur") == fold_blur          # what the caller set
        for k in range(1 if folded else 0, 4):
            wl = 320 >> k
            got = c.debug_fetch(f"pyr{k}", (len(small), wl, wl), np.float32)
            with oracle.model(mask):
                want = np.stack([oracle.resize_linear_f32(oracle.gaussian_blur(f.astype(np.float32), *KS[k]), wl, wl) for f in small])
            ndiff = int(np.count_nonzero(got.view(np.uint32) != want.view(np.uint32)))
            assert ndiff == 0, (mask, fold_blur, k, ndiff)
        if folded:
            with pytest.raises(Exception, match="pyr0"):
                c.debug_fetch("pyr0", (len(small), 320, 320), np.float32)


@pytest.mark.parametrize("mask", [0] + MASKS)
def test_fast_mode_keeps_its_guarantee(clips, refs, mask):
    with _ctx(mask, 1) as c:
        assert c.get_option("fb_rerun") == 1
        for name in ("a", "b", "c", "d", "checker", "step"):
            small = clips[name][1]
            fm, fv, flow = c.farneback_pairs(small, want_flow=True)
            rerun = c.get_option("rerun_pairs")
            rec = c.analyze_frames(_bgr(small))                  # the same pairs through the records: the flag words
            reserved = rec["reserved"][1:]
            assert c.get_option("rerun_pairs") == int(np.count_nonzero(reserved)) == rerun, (mask, name, reserved.tolist(), rerun)
            assert np.array_equal(rec["flow_mean"][1:], fm) and np.array_equal(rec["flow_var"][1:], fv), (mask, name)
            want, wm, wv = refs(mask, name)
            for p in range(len(want)):
                d = float(np.abs(flow[p].astype(np.float64) - want[p].astype(np.float64)).max())
                print(f"[cv2_model] fast, mask {mask} clip {name} pair {p}: flag word {int(reserved[p]):#x}, max |delta flow| {d:.3g} px, "
                      f"flow_mean {float(fm[p])!r} oracle {float(wm[p])!r}")
                if reserved[p]:
                    assert np.array_equal(flow[p], want[p]) and fm[p] == wm[p] and fv[p] == wv[p], (mask, name, p)
                else:
                    assert d <= FLOW_TOL, (mask, name, p, d)
                    assert fm[p] == pytest.approx(wm[p], rel=1e-6, abs=1e-7) and fv[p] == pytest.approx(wv[p], rel=1e-6, abs=1e-7), (mask, name, p)
            if name in ("checker", "step"):
                assert reserved[0] != 0, ("an ill-posed pair was not flagged", mask, name)
            if mask & 8:
                assert not (reserved & 0x88).any(), (mask, name, [hex(int(v)) for v in reserved])
            st = c.fb_model()
            assert st[0] == mask and st[1] == (3 if mask & 8 else 4) and st[2] == (5 & (4 if mask & 16 else 7) & (3 if mask & 8 else 7)), st.tolist()


def _flow_records_match(rec, wm, wv, mode, tag):
    """records [1:] of ONE clip against the oracle's statistics under the mask"""
    assert rec["ham"][0] == -1 and rec["flow_mean"][0] == 0
    for p in range(len(wm)):
        r = rec[p + 1]
        if mode == 0 or r["reserved"]:
            assert r["flow_mean"] == wm[p] and r["flow_var"] == wv[p], (tag, p)
        else:
            assert r["flow_mean"] == pytest.approx(wm[p], rel=1e-6, abs=1e-7) and r["flow_var"] == pytest.approx(wv[p], rel=1e-6, abs=1e-7), (tag, p)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("mask", [0] + MASKS)
def test_through_the_records(oracle, clips, refs, mask, mode):
    import avd_hip
    clip = clips["a"][0]
    meta = {"width": 128, "height": 96, "fps": 30.0, "duration": 5.0}
    _, wm, wv = refs(mask, "a")
    with oracle.model(mask):
        want = oracle.analyze_sampled_frames(clip, meta)
    with _ctx(mask, mode) as c:
        got = avd_hip.FrameAnalyzer(ctx=c).analyze(clip, meta)
        if mode == 0:
            assert got["timeline"] == want["timeline"], (mask, got["timeline"], want["timeline"])
        else:
            assert np.allclose(got["timeline"], want["timeline"], rtol=0, atol=1e-6)
        for k, v in want["summary"].items():
            assert abs(got["summary"][k] - v) <= (1e-9 if mode == 0 else 1e-6) * max(1.0, abs(v)), (mask, mode, k)
        whole = c.analyze_frames(clip)
        _flow_records_match(whole, wm, wv, mode, ("whole", mask, mode))
        # 2 + 3 frames through a stream slot: the records of the whole clip
        c.stream_slot(1)
        parts = np.concatenate([c.analyze_frames(clip[:2]), c.analyze_frames(clip[2:])])
        c.stream_slot(0)
        assert parts.tobytes() == whole.tobytes(), (mask, mode)
        # two clips of a batch
        recs = c.analyze_batch([clip, clips["b"][0]])
        assert recs[0].tobytes() == whole.tobytes()
        _flow_records_match(recs[1], *refs(mask, "b")[1:], mode, ("batch", mask, mode))
        # asynchronous, the option changed before the call is drained: the pending call keeps its model
        rec = np.zeros(len(clip), avd_hip.RECORD_DTYPE)
        c.analyze_frames_async(clip, rec)
        c.set_option("cv2_model", 0)
        c.synchronize()
        assert rec.tobytes() == whole.tobytes(), (mask, mode)
        assert c.get_option("cv2_model") == 0 and c.fb_model()[0] == mask


def test_the_option_itself(clips, monkeypatch):
    import avd_hip
    assert (avd_hip.CV2_GAUSS_MULADD, avd_hip.CV2_THREE_SCALES, avd_hip.CV2_RESIZE_LERP) == (1, 8, 16)
    monkeypatch.delenv("AVD_CV2_MODEL", raising=False)
    with avd_hip.Context(0) as c:
        assert c.get_option("cv2_model") == 0
        with pytest.raises(avd_hip.AvdError, match="fb_model"):
            c.fb_model()                                         # an error before any call that ran the Farneback stage
        for good in (0, 1, 8, 9, 16, 17, 24, 25):
            c.set_option("cv2_model", good)
            assert c.get_option("cv2_model") == good
        c.set_option("cv2_model", 9)
        for bad in (2, 3, 4, 6, 32, 64, -1):
            with pytest.raises(avd_hip.AvdError, match=r"^avd status -1: cv2_model:"):
                c.set_option("cv2_model", bad)
            assert c.get_option("cv2_model") == 9, bad
        c.farneback_pairs(clips["a"][1][:2])
        assert c.fb_model().tolist() == [9, 3, 1, 0]                  # three scales: "fb_fold_up" loses bit 4; mul + add taps: the blur is not folded
        c.release_workspace()
        assert c.get_option("cv2_model") == 9
        c.set_option("fb_fold_up", 7)
        c.set_option("cv2_model", 16)
        c.farneback_pairs(clips["a"][1][:2])
        assert c.fb_model().tolist() == [16, 4, 4, 1] and c.get_option("fb_fold_up") == 7
        c.set_option("cv2_model", 0)
        c.farneback_pairs(clips["a"][1][:2])
        assert c.fb_model().tolist() == [0, 4, 7, 1]
    for text, want in (("8", 8), ("0x19", 25), ("2", 0)):
        monkeypatch.setenv("AVD_CV2_MODEL", text)
        with avd_hip.Context(0) as c:
            assert c.get_option("cv2_model") == want, text


@pytest.mark.parametrize("mode", [0, 1])
def test_profiling_under_three_scales(clips, mode):
    clip = clips["c"][0]
    with _ctx(8, mode) as c:
        c.set_profiling(True)
        c.analyze_frames(clip)
        c.analyze_frames(clip)
        stage, kern = c.stage_ms(), c.kernel_ms()
        assert kern["level40"] == 0.0 and kern["flow_up80"] == 0.0, kern
        assert kern["level80"] > 0 and kern["level160"] > 0 and kern["level320"] > 0, kern
        # stage 2 is the Farneback stage with the statistics and the records; the regions that remain are consecutive intervals between its two events
        inside = ["pyramid", "polyexp", "level80", "flow_up160", "level160", "flow_up320", "level320", "stats", "records"]
        total = sum(kern[k] for k in inside)
        print(f"[cv2_model] profiling under bit 8, fb_mode {mode}: stage 2 = {stage[2]:.5f} ms, its regions sum to {total:.5f} ms; {kern}")
        assert total == pytest.approx(stage[2], rel=1e-4), (stage, kern)          # (float32 event differences, summed)


def test_results_do_not_depend_on_the_model_run_before(clips):
    clip = clips["a"][0]
    with _ctx(0, 1) as fresh:
        want = fresh.analyze_frames(clip)
        want_flow = fresh.debug_fetch("flow0", (len(clip) - 1, 2, 320, 320), np.float32)
    with _ctx(25, 1) as c:
        other = c.analyze_frames(clip)
        assert other.tobytes() != want.tobytes()
        c.set_option("cv2_model", 0)
        got = c.analyze_frames(clip)
        flow = c.debug_fetch("flow0", (len(clip) - 1, 2, 320, 320), np.float32)
    assert got.tobytes() == want.tobytes()
    assert flow.tobytes() == want_flow.tobytes()
