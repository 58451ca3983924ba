"""A call made on a context while an asynchronous analysis is pending on it (avd_analyze_*_async submitted, avd_synchronize not
yet called).  Contract (include/avd.h, avd_analyze_frames_async): any other call on the context first completes the pending one --
its records buffer is filled and the exact re-run of the pairs the fast Farneback level kernels flagged is settled -- so:

  * the pending call's records are byte-equal to the same input analysed alone by a blocking call on a fresh context in the same
    mode, whatever was called in between (calls that reuse the workspace the re-run rebuilds the records from, grow it, drop the
    Farneback scratch, change the options the call was submitted with, fail their argument check, or are the extensions');
  * those reference records are anchored to independent references: lap_sum / lap_sumsq / ham equal the CPU oracle exactly, the
    flow statistics equal an exact-mode context bit for bit on flagged pairs (reserved != 0) and within rel 1e-6 elsewhere, and the
    exact mode's equal the CPU oracle's;
  * the call made in between returns what it returns on a fresh context.

Every fast-mode case asserts, as a precondition, that the pending clip has at least 3 flagged pairs in its last Farneback chunk: a
case cannot pass without the re-run being pending when the other call arrives.
"""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import avd_hip  # noqa: E402
from avd_hip import AvdError, synth  # noqa: E402
from tests.content_families import flagged_mix  # noqa: E402

N = 24                   # frames of every pending call: 23 pairs, one Farneback chunk (the last one)
MIN_FLAGGED = 3
REL, ABS = 1e-6, 1e-7
FAST, EXACT = 1, 0


def _bgr(gray):
    return np.ascontiguousarray(np.repeat(gray[..., None], 3, axis=3))


class Material:
    """inputs of the pending calls and of the calls made in between (generated once per module)"""

    def __init__(self):
        import torch
        self.clip = _bgr(flagged_mix(N - 1, 3))                                   # 320 x 320 BGR, host
        self.clip_dev = torch.from_numpy(self.clip).cuda()
        self.y, self.uv = synth.bgr_to_nv12(self.clip)
        a = _bgr(flagged_mix(13, 22))                                              # 14 frames, 320 x 320
        b = _bgr(flagged_mix(9, 23)).repeat(2, axis=1).repeat(2, axis=2)           # 10 frames, 640 x 640
        self.batch = [a, b]
        assert sum(len(k) for k in self.batch) == N
        rng = np.random.default_rng(7)
        self.pre_same = synth.random_frames(N, 320, 320, seed=11)                  # the pending call's frame count
        self.pre_grow = synth.random_frames(3 * N, 360, 640, seed=12)              # more frames, another geometry: the workspace grows
        self.nv12_y, self.nv12_uv = synth.bgr_to_nv12(synth.make_clip(N, 240, 320, seed=13, dup_every=0))
        self.fb_few = flagged_mix(5, 14)
        self.fb_many = rng.integers(0, 256, (515, 320, 320), dtype=np.uint8)      # 514 pairs > 512: the Farneback scratch grows
        self.other_clip = synth.make_clip(6, 360, 640, seed=15, dup_every=2)
        self.other_batch = [synth.make_clip(5, 180, 320, seed=16), synth.random_frames(4, 96, 128, seed=17)]
        self.bad = np.zeros((2, 16, 16, 3), np.uint8)                              # smaller than 32 x 32: AVD_ERR_UNSUPPORTED
        # extensions
        from tests.test_cnn import seeded_parameters
        self.cnn_w, self.cnn_b = seeded_parameters(0)
        self.cnn_frames = synth.make_clip(2, 180, 320, seed=18)
        self.vit_w = (rng.standard_normal((768, 768)) * 0.02).astype(np.float32)
        self.vit_b = (rng.standard_normal(768) * 0.1).astype(np.float32)
        self.vit_frames = synth.random_frames(2, 224, 224, seed=19)
        self.ln_x = rng.standard_normal((64, 768)).astype(np.float32)
        self.ln_g = rng.standard_normal(768).astype(np.float32)
        self.ln_b = rng.standard_normal(768).astype(np.float32)
        self.sm_x = (rng.standard_normal((64, 1000)) * 4).astype(np.float32)
        self.wav = (np.sin(np.arange(40000) * 0.05) * 0.3 + rng.standard_normal(40000) * 0.05).astype(np.float32)


@pytest.fixture(scope="module")
def mat():
    return Material()


# ---- the pending calls ------------------------------------------------------------------------------------------------------
def _submit(c, mat, kind, rec):
    """enqueue the pending call; -> what must stay alive until it is drained"""
    if kind == "bgr_host":
        return c.analyze_frames_async(mat.clip, rec)
    if kind == "bgr_device":
        return c.analyze_frames_async(mat.clip_dev, rec)
    if kind == "nv12":
        return c.analyze_frames_nv12_async(mat.y, mat.uv, rec)
    if kind == "batch":
        return c.analyze_batch_async(mat.batch, rec)
    raise ValueError(kind)


def _blocking(c, mat, kind):
    if kind == "bgr_host":
        return c.analyze_frames(mat.clip)
    if kind == "bgr_device":
        return c.analyze_frames(mat.clip_dev)
    if kind == "nv12":
        return c.analyze_frames_nv12(mat.y, mat.uv)
    if kind == "batch":
        return np.concatenate(c.analyze_batch(mat.batch))
    raise ValueError(kind)


def _clips_bgr(mat, kind):
    """the pending call's clips as BGR frames, as the oracle sees them"""
    from oracle import oracle as O
    if kind in ("bgr_host", "bgr_device"):
        return [mat.clip]
    if kind == "nv12":
        return [O.nv12_to_bgr(mat.y, mat.uv)]
    return list(mat.batch)


# ---- what the calls made in between return on a fresh context -----------------------------------------------------------------
def _interleave(c, mat, what, mode):
    """-> the call's outputs (a tuple of arrays), and the options to restore after synchronize"""
    if what == "preprocess_same":
        return c.preprocess_bgr(mat.pre_same), {}
    if what == "preprocess_grow":
        return c.preprocess_bgr(mat.pre_grow), {}
    if what == "preprocess_nv12":
        return c.preprocess_nv12(mat.nv12_y, mat.nv12_uv), {}
    if what == "farneback_few":
        return c.farneback_pairs(mat.fb_few), {}
    if what == "farneback_many":
        return c.farneback_pairs(mat.fb_many), {}
    if what == "analyze_frames":
        return (c.analyze_frames(mat.other_clip),), {}
    if what == "analyze_batch_async":
        rec = np.zeros(sum(len(k) for k in mat.other_batch), avd_hip.RECORD_DTYPE)
        keep = c.analyze_batch_async(mat.other_batch, rec)
        c.synchronize()
        del keep
        return (rec,), {}
    if what == "option_fb_rerun":
        c.set_option("fb_rerun", 0)                   # applies to the calls submitted after it
        assert c.get_option("fb_rerun") == 0
        return (), {"fb_rerun": 1}
    if what == "option_fb_mode":
        c.set_option("fb_mode", 1 - mode)
        assert c.get_option("fb_mode") == 1 - mode
        return (), {"fb_mode": mode}
    if what == "bad_arguments":
        with pytest.raises(AvdError, match="status -4"):
            c.preprocess_bgr(mat.bad)
        return (), {}
    if what == "cnn_forward":
        return (c.cnn_forward(mat.cnn_frames)[0],), {}
    if what == "vit_patch_embed":
        return (c.vit_patch_embed(mat.vit_frames)[0],), {}
    if what == "layernorm":
        return (c.layernorm(mat.ln_x, mat.ln_g, mat.ln_b)[0],), {}
    if what == "softmax":
        return (c.softmax(mat.sm_x)[0],), {}
    if what == "audio_features":
        return (c.audio_features(mat.wav, 4096),), {}
    raise ValueError(what)


def _set_weights(c, mat, what):
    """weights are state of the context: uploaded before the pending call is submitted"""
    if what == "cnn_forward":
        c.cnn_set_weights(mat.cnn_w, mat.cnn_b)
    elif what == "vit_patch_embed":
        c.vit_set_weights(mat.vit_w, mat.vit_b)


class Refs:
    """results of blocking calls on fresh contexts, computed once"""

    def __init__(self, mat):
        self.mat, self._pending, self._inter = mat, {}, {}

    def pending(self, kind, mode):
        key = (kind, mode)
        if key not in self._pending:
            with avd_hip.Context(0) as c:
                c.set_option("fb_mode", mode)
                self._pending[key] = (_blocking(c, self.mat, kind).copy(), c.get_option("rerun_pairs"))
        return self._pending[key]

    def interleaved(self, what, mode):
        key = (what, mode)
        if key not in self._inter:
            with avd_hip.Context(0) as c:
                c.set_option("fb_mode", mode)
                _set_weights(c, self.mat, what)
                out, _ = _interleave(c, self.mat, what, mode)
                self._inter[key] = (tuple(np.array(o, copy=True) for o in out), c.get_option("rerun_pairs"))
        return self._inter[key]


@pytest.fixture(scope="module")
def refs(mat):
    return Refs(mat)


def _flagged_in_last_chunk(rec):
    # N - 1 < 128 pairs: the whole call is one Farneback chunk, the last one
    return int(np.count_nonzero(rec["reserved"][1:]))


# ---- the reference records against independent references ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bgr_host", "bgr_device", "nv12", "batch"])
def test_the_references_agree_with_the_oracle_and_the_exact_mode(mat, refs, oracle, kind):
    fast, _ = refs.pending(kind, FAST)
    exact, _ = refs.pending(kind, EXACT)
    assert _flagged_in_last_chunk(fast) >= MIN_FLAGGED, _flagged_in_last_chunk(fast)
    assert not exact["reserved"].any()
    f0 = 0
    for frames in _clips_bgr(mat, kind):
        n = len(frames)
        small, hsh, s, q = oracle.preprocess_bgr(frames)
        ham = np.array([-1] + [int(np.count_nonzero(hsh[f] != hsh[f - 1])) for f in range(1, n)], np.int64)
        for rec in (fast, exact):
            r = rec[f0:f0 + n]
            assert np.array_equal(r["lap_sum"], s) and np.array_equal(r["lap_sumsq"], q), kind
            assert np.array_equal(r["ham"], ham), kind
            assert r["flow_mean"][0] == 0 and r["flow_var"][0] == 0 and r["reserved"][0] == 0, kind
        if kind == "bgr_host":
            # the exact kernels are cv2's Farneback bit for bit (the CPU oracle); the other kinds anchor their fast records to them
            fm, fv = oracle.farneback_pairs(small)
            assert np.array_equal(exact["flow_mean"][1:], fm) and np.array_equal(exact["flow_var"][1:], fv)
        f0 += n
    flagged = fast["reserved"] != 0
    for key in ("flow_mean", "flow_var"):
        assert np.array_equal(fast[key][flagged], exact[key][flagged]), key
        np.testing.assert_allclose(fast[key], exact[key], rtol=REL, atol=ABS, err_msg=key)
    # the blocking references agree with each other where the input is the same
    if kind == "bgr_device":
        assert refs.pending("bgr_host", FAST)[0].tobytes() == fast.tobytes()


# ---- one pending call, one call in between, then avd_synchronize -----------------------------------------------------------------
INTERLEAVED = ["preprocess_same", "preprocess_grow", "preprocess_nv12", "farneback_few", "farneback_many", "analyze_frames",
               "analyze_batch_async", "option_fb_rerun", "option_fb_mode", "bad_arguments"]
EXTENSIONS = ["cnn_forward", "vit_patch_embed", "layernorm", "softmax", "audio_features"]
RUNS_FARNEBACK = {"farneback_few", "farneback_many", "analyze_frames", "analyze_batch_async"}

CASES = ([(k, FAST, w) for k in ("bgr_host", "bgr_device", "nv12", "batch") for w in INTERLEAVED]
         + [("bgr_host", EXACT, w) for w in INTERLEAVED]
         + [("bgr_host", FAST, w) for w in EXTENSIONS])


@pytest.mark.parametrize("kind,mode,what", CASES, ids=[f"{k}-{'fast' if m else 'exact'}-{w}" for k, m, w in CASES])
def test_a_call_made_while_an_analysis_is_pending(mat, refs, kind, mode, what):
    want, want_rerun = refs.pending(kind, mode)
    if mode == FAST:
        assert _flagged_in_last_chunk(want) >= MIN_FLAGGED          # the re-run is pending when the other call arrives
    want_out, want_out_rerun = refs.interleaved(what, mode)
    with avd_hip.Context(0) as c:
        c.set_option("fb_mode", mode)
        _set_weights(c, mat, what)
        rec = np.zeros(N, avd_hip.RECORD_DTYPE)
        keep = _submit(c, mat, kind, rec)
        out, restore = _interleave(c, mat, what, mode)
        c.synchronize()
        del keep
        rerun = c.get_option("rerun_pairs")
        for name, value in restore.items():
            c.set_option(name, value)
            assert c.get_option(name) == value
    assert rec.tobytes() == want.tobytes(), [int(f) for f in np.nonzero(rec != want)[0]]
    assert len(out) == len(want_out)
    for i, (got, exp) in enumerate(zip(out, want_out)):
        assert np.array_equal(got, exp), (what, i)
    # "rerun_pairs" reports the last call that ran the Farneback stage
    assert rerun == (want_out_rerun if what in RUNS_FARNEBACK else want_rerun)


def test_a_waiting_thread_and_a_call_in_between():
    """Context A holds a pending flagged clip; a second thread waits in B.synchronize() with tail_help on, so it may settle A's re-run
    while the main thread calls A.farneback_pairs(); then A.synchronize().  Who settles A's call changes nothing."""
    clip_a = _bgr(flagged_mix(N - 1, 3))
    clip_b = _bgr(flagged_mix(63, 24))
    fb = flagged_mix(5, 14)
    with avd_hip.Context(0) as c:
        want_a = c.analyze_frames(clip_a).copy()
        want_b = c.analyze_frames(clip_b).copy()
    with avd_hip.Context(0) as c:
        want_fm, want_fv = c.farneback_pairs(fb)
    assert _flagged_in_last_chunk(want_a) >= MIN_FLAGGED
    with avd_hip.Context(0) as a, avd_hip.Context(0) as b:
        assert a.get_option("tail_help") == 1 and b.get_option("tail_help") == 1
        for rnd in range(4):
            rec_a = np.zeros(len(clip_a), avd_hip.RECORD_DTYPE)
            rec_b = np.zeros(len(clip_b), avd_hip.RECORD_DTYPE)
            keep_a = a.analyze_frames_async(clip_a, rec_a)
            keep_b = b.analyze_frames_async(clip_b, rec_b)
            errors = []

            def wait_b():
                try:
                    b.synchronize()
                except Exception as e:                      # reported by the main thread
                    errors.append(e)
            th = threading.Thread(target=wait_b)
            th.start()
            fm, fv = a.farneback_pairs(fb)
            a.synchronize()
            th.join()
            del keep_a, keep_b
            assert not errors, errors
            assert rec_a.tobytes() == want_a.tobytes(), rnd
            assert rec_b.tobytes() == want_b.tobytes(), rnd
            assert np.array_equal(fm, want_fm) and np.array_equal(fv, want_fv), rnd
