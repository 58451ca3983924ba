"""Several tracks per avd_audio_features call (option "audio_cut") and 16-bit PCM as decoded (option "audio_format") on the GPU.

The contract (include/avd.h) is equality, so almost every check here is np.array_equal on bytes:

  * the records of track t of a batch, and its rows of debug buffers "audio_xw" / "audio_mag", are those of avd_audio_features on that track's
    samples alone -- at win = 8000 over tracks that cover full windows only, shorter than a window, one sample, a repeated short length and
    short lengths with L % 4 = 0, 1, 2, 3, and at win = 1001 where every window takes the direct sum;
  * int16 samples give what their float32 form (s * 2^-15) gives, alone and in a batch, from host memory and from a device tensor;
  * the cut list is one-shot: the call after a batch, and after a REFUSED batch, is an ordinary single-track call;
  * a batch leaves nothing behind in a context, drains a pending asynchronous analysis first, and survives avd_release_workspace.

Two checks are not equalities: every bin of one batch's "audio_mag" against np.fft.rfft with the bound of tests/test_gpu_audio_spectrum.py
(TOL = 1e-12 * sum|xw|, imported from there, derived in its docstring), and analyze_waves on all cases of tests/golden/audio_golden.json in one
call against the reference's own outputs within the 1e-6 of tests/test_audio.py.
"""
import ctypes
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import avd_hip  # noqa: E402
from avd_hip import AvdError  # noqa: E402
from avd_hip import audio as host_audio  # noqa: E402
from avd_hip._lib import AUDIO_WINDOW_DTYPE, AVD_MEM_DEVICE, AVD_MEM_HOST  # noqa: E402
from tests.test_gpu_audio_spectrum import TOL  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SETS = {8000: (16037, 8000, 5, 1, 12000, 7999, 8001, 12000, 16002),
        1001: (2500, 1001, 3, 2002)}


def _track(n, seed):
    rng = np.random.default_rng([n, seed])
    i = np.arange(n)
    x = 0.3 * np.sin(2 * np.pi * (0.01 + 0.003 * seed) * i + seed) + 0.05 * rng.standard_normal(n)
    w = np.clip(x, -1, 1).astype(np.float32)
    w.setflags(write=False)
    return w


def _tracks(win):
    return [_track(n, k) for k, n in enumerate(SETS[win])]


def _counts(lens, win):
    return [-(-n // win) for n in lens]


class Single:
    """a track analysed alone: its records and its rows of the two scratch buffers"""

    def __init__(self, c, wav, win):
        self.rec = c.audio_features(wav, win).copy()
        self.plan = c.audio_plan()
        self.xw, self.mag = c.audio_xw(), c.audio_mag()


@pytest.fixture(scope="module")
def singles(ctx):
    return {win: [Single(ctx, w, win) for w in _tracks(win)] for win in SETS}


def _rows_equal(got, want, lengths, half):
    """rows of audio_xw (half = False) or audio_mag: the entries the window owns; what lies behind a short window's is nobody's"""
    assert len(got) == len(want) == len(lengths)
    for w, L in enumerate(lengths):
        k = L // 2 + 1 if half else L
        assert np.array_equal(got[w, :k], want[w, :k]), ("mag" if half else "xw", w, L)


# ---- batch == per-track calls -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", sorted(SETS))
def test_a_batch_equals_the_per_track_calls(ctx, singles, win):
    tracks, lens = _tracks(win), SETS[win]
    got = ctx.audio_features_many(tracks, win)
    counts = _counts(lens, win)
    assert [len(g) for g in got] == counts
    firsts = np.concatenate([[0], np.cumsum(counts)])[:-1]
    lasts = [n - (c - 1) * win for n, c in zip(lens, counts)]
    assert ctx.audio_tracks().tolist() == [[int(f), c, l] for f, c, l in zip(firsts, counts, lasts)]
    nfull = sum(n // win for n in lens) if win == 8000 else 0
    assert ctx.audio_plan() == (sum(counts), win, lasts[-1], nfull)
    assert ctx.get_option("audio_cut") == 0                                     # the call took the list
    xw, mag = ctx.audio_xw(), ctx.audio_mag()
    assert xw.shape == (sum(counts), win) and mag.shape == (sum(counts), win // 2 + 1)
    for t, (g, s) in enumerate(zip(got, singles[win])):
        assert np.array_equal(g.view(np.uint8), s.rec.view(np.uint8)), (win, t)
        lengths = s.rec["length"].tolist()
        assert lengths == [win] * (counts[t] - 1) + [lasts[t]]
        _rows_equal(xw[firsts[t]:firsts[t] + counts[t]], s.xw, lengths, False)
        _rows_equal(mag[firsts[t]:firsts[t] + counts[t]], s.mag, lengths, True)
    if win == 8000:
        assert sorted({l % 4 for l in lasts if l != win}) == [0, 1, 2, 3] and lasts.count(4000) == 2
        assert nfull == 8 and [s.plan[3] for s in singles[win]] == [2, 1, 0, 0, 1, 0, 1, 1, 2]
    else:
        assert all(s.plan[3] == 0 for s in singles[win])


def test_every_bin_of_a_batch_against_numpy(ctx):
    tracks = _tracks(8000)
    ctx.audio_features_many(tracks, 8000)
    mag = ctx.audio_mag()
    w = 0
    for t, wav in enumerate(tracks):
        for s in range(0, len(wav), 8000):
            seg = wav[s:s + 8000]
            xw = seg.astype(np.float64) * np.hanning(len(seg))
            ref = np.abs(np.fft.rfft(xw)) + 1e-9
            err = np.abs(mag[w, :len(ref)] - ref)
            k = int(np.argmax(err))
            assert err[k] <= TOL * np.sum(np.abs(xw)), (t, w, len(seg), k, err[k], np.sum(np.abs(xw)))
            w += 1
    assert w == len(mag)


# ---- int16 ------------------------------------------------------------------------------------------------------------------------------------
def _pcm_track(n, seed):
    rng = np.random.default_rng([16, n, seed])
    s = rng.integers(-32768, 32768, n).astype(np.int16)
    if n >= 64:
        s[:2] = (-32768, 32767)
        s[10:14] = (9000, 0, 0, -9000)                       # a run of zeros between opposite signs
        s[20] = 300; s[21:40] = 0; s[40] = -300
        s[50:54] = (-1, 0, 1, 0)
        s[-2:] = (32767, -32768)
    return s


def _as_float(s):
    return s.astype(np.float32) * np.float32(2.0 ** -15)


@pytest.mark.parametrize("where", ["host", "device"])
def test_int16_equals_its_float32_form_alone_and_in_a_batch(ctx, where):
    import torch
    lens = (8037, 8000, 3, 9002)
    pcm = [_pcm_track(n, k) for k, n in enumerate(lens)]
    want = [ctx.audio_features(_as_float(s), 8000).copy() for s in pcm]
    give = (lambda s: torch.from_numpy(s).cuda()) if where == "device" else (lambda s: s)
    for s, w in zip(pcm, want):
        got = ctx.audio_features(give(s), 8000)
        assert np.array_equal(got.view(np.uint8), w.view(np.uint8)), len(s)
    many = ctx.audio_features_many([give(s) for s in pcm], 8000)
    assert ctx.audio_tracks()[:, 1].tolist() == _counts(lens, 8000)
    for g, w in zip(many, want):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
    floats = ctx.audio_features_many([give(_as_float(s)) for s in pcm], 8000)
    for g, w in zip(floats, want):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
    assert ctx.get_option("audio_format") == 0                                  # set for the calls, restored behind them
    with pytest.raises(ValueError, match="all float32 or all int16"):
        ctx.audio_features_many([pcm[0], _as_float(pcm[1])], 8000)


def _raw(c, ptr, mem, n, win, max_windows):
    out = np.zeros(max(max_windows, 1), AUDIO_WINDOW_DTYPE)
    rc = c._L.avd_audio_features(c._h, ctypes.c_void_p(ptr), mem, n, win, ctypes.c_void_p(out.ctypes.data), max_windows)
    return rc, out[:max_windows]


def test_the_format_option_persists_and_the_device_pointer_is_taken_as_it_is(ctx):
    import torch
    s = _pcm_track(8037, 5)
    want = ctx.audio_features(_as_float(s), 8000).copy()
    dev = torch.from_numpy(np.concatenate([np.zeros(3, np.int16), s])).cuda()    # the samples begin 6 bytes into the tensor
    torch.cuda.synchronize()
    ptr = dev.data_ptr() + 6
    try:
        ctx.set_option("audio_format", 1)
        for _ in range(2):                                                      # durable: it holds until it is changed
            assert ctx.get_option("audio_format") == 1
            rc, got = _raw(ctx, ptr, AVD_MEM_DEVICE, len(s), 8000, 2)
            assert rc == 0 and np.array_equal(got.view(np.uint8), want.view(np.uint8))
        rc, got = _raw(ctx, s.ctypes.data, AVD_MEM_HOST, len(s), 8000, 2)
        assert rc == 0 and np.array_equal(got.view(np.uint8), want.view(np.uint8))
        for bad in (2, -1, 16):
            with pytest.raises(AvdError, match="audio_format:"):
                ctx.set_option("audio_format", bad)
            assert ctx.get_option("audio_format") == 1                          # the old value stays
        # an odd address is refused before anything is staged or read: host and device
        raw = np.zeros(2 * len(s) + 2, np.uint8)
        for odd, mem in ((raw.ctypes.data | 1, AVD_MEM_HOST), (ptr + 1, AVD_MEM_DEVICE)):
            rc, got = _raw(ctx, odd, mem, len(s), 8000, 2)
            assert rc != 0 and not got.view(np.uint8).any()
            with pytest.raises(AvdError, match="2-byte aligned"):
                ctx._check(rc)
        rc, got = _raw(ctx, ptr, AVD_MEM_DEVICE, len(s), 8000, 2)                # and the context takes the next call as before
        assert rc == 0 and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    finally:
        ctx.set_option("audio_format", 0)
    assert np.array_equal(ctx.audio_features(_as_float(s), 8000).view(np.uint8), want.view(np.uint8))


# ---- the cut list -------------------------------------------------------------------------------------------------------------------------
def test_the_cut_option_refuses_what_the_header_says(ctx):
    ctx.set_option("audio_cut", -1)
    assert ctx.get_option("audio_cut") == 0
    for bad in (0, -2, -100):
        with pytest.raises(AvdError, match="audio_cut:"):
            ctx.set_option("audio_cut", bad)
    ctx.set_option("audio_cut", 10)
    ctx.set_option("audio_cut", 20)
    for bad in (20, 19, 1):
        with pytest.raises(AvdError, match="audio_cut:.*ascending"):
            ctx.set_option("audio_cut", bad)
        assert ctx.get_option("audio_cut") == 2
    for v in range(21, 21 + 61):
        ctx.set_option("audio_cut", v)
    assert ctx.get_option("audio_cut") == 63
    with pytest.raises(AvdError, match="audio_cut:.*63"):
        ctx.set_option("audio_cut", 1000)
    assert ctx.get_option("audio_cut") == 63
    ctx.set_option("audio_cut", -1)
    assert ctx.get_option("audio_cut") == 0
    # n == 0 with cuts pending: AVD_OK, nothing written, the list cleared
    ctx.set_option("audio_cut", 7)
    assert len(ctx.audio_features(np.zeros(0, np.float32), 1001)) == 0
    assert ctx.get_option("audio_cut") == 0


def test_the_cut_list_is_one_shot_also_when_the_call_is_refused(ctx, singles):
    win = 1001
    wav = _tracks(win)[0]                                                       # 2500 samples: three windows alone
    want = singles[win][0].rec
    n = len(wav)

    def plain_call_equals_the_single_track_result():
        assert ctx.get_option("audio_cut") == 0
        assert np.array_equal(ctx.audio_features(wav, win).view(np.uint8), want.view(np.uint8))
        assert ctx.audio_tracks().tolist() == [[0, 3, 2500 - 2002]]

    # after a batch
    ctx.set_option("audio_cut", 100)
    rc, got = _raw(ctx, wav.ctypes.data, AVD_MEM_HOST, n, win, 4)               # 1 + 3 windows: one more than the samples alone would need
    assert rc == 0 and got["length"].tolist() == [100, 1001, 1001, 398] and ctx.audio_tracks().tolist() == [[0, 1, 100], [1, 3, 398]]
    plain_call_equals_the_single_track_result()
    # a cut at or beyond n
    for cut in (n, n + 5):
        ctx.set_option("audio_cut", 100)
        ctx.set_option("audio_cut", cut)
        with pytest.raises(AvdError, match="audio_cut: beyond the buffer"):
            ctx.audio_features(wav, win)
        plain_call_equals_the_single_track_result()
    # max_windows one below the sum of the tracks' windows (1 + 3) while ceil(n / win) = 3 fits
    ctx.set_option("audio_cut", 100)
    rc, out = _raw(ctx, wav.ctypes.data, AVD_MEM_HOST, n, win, 3)
    assert rc != 0 and not out.view(np.uint8).any()
    with pytest.raises(AvdError, match="windows array too small"):
        ctx._check(rc)
    plain_call_equals_the_single_track_result()
    # a window length of 0
    ctx.set_option("audio_cut", 100)
    with pytest.raises(AvdError, match="1..8192"):
        ctx.audio_features(wav, 0)
    plain_call_equals_the_single_track_result()
    # a refused call is not a call: the debug buffers still describe the last one that ran
    ctx.set_option("audio_cut", n)
    with pytest.raises(AvdError):
        ctx.audio_features(wav, win)
    assert ctx.audio_plan() == (3, win, 498, 0)


# ---- 64 tracks, 65 tracks ---------------------------------------------------------------------------------------------------------------------
def test_sixty_four_tracks_of_one_window_each_and_a_sixty_fifth(ctx, monkeypatch):
    win = 256
    lens = [win - (k % 40) for k in range(65)]                                  # 40 distinct lengths, the full one among them, repeats
    tracks = [_track(n, 100 + k) for k, n in enumerate(lens)]
    want = [ctx.audio_features(w, win).copy() for w in tracks]
    calls = []
    inner = ctx._audio_call
    monkeypatch.setattr(ctx, "_audio_call", lambda *a, **k: (calls.append(len(a[6]) + 1 if len(a) > 6 else len(k.get("cuts", ())) + 1), inner(*a, **k))[1])
    got = ctx.audio_features_many(tracks[:64], win)
    assert calls == [64] and ctx.audio_tracks().tolist() == [[k, 1, lens[k]] for k in range(64)]
    assert ctx.audio_plan() == (64, win, lens[63], 0)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), k
    del calls[:]
    got = ctx.audio_features_many(tracks, win)
    assert calls == [64, 1] and len(got) == 65
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), k
    assert ctx.audio_tracks().tolist() == [[0, 1, lens[64]]]


# ---- history and ordering -----------------------------------------------------------------------------------------------------------------
def test_a_batch_leaves_nothing_behind_and_survives_a_release(singles):
    tracks = _tracks(8000)
    with avd_hip.Context(0) as fresh:
        want = fresh.audio_features(tracks[0], 8000).copy()
        want_mag = fresh.audio_mag()
    assert np.array_equal(want.view(np.uint8), singles[8000][0].rec.view(np.uint8))
    with avd_hip.Context(0) as c:
        c.audio_features_many(_tracks(1001), 1001)
        first = c.audio_features_many(tracks, 8000)
        got = c.audio_features(tracks[0], 8000)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
        assert c.audio_plan() == (3, 8000, 37, 2) and c.audio_tracks().tolist() == [[0, 3, 37]]
        _rows_equal(c.audio_mag(), want_mag, [8000, 8000, 37], True)
        c.release_workspace()
        with pytest.raises(AvdError):
            c.audio_mag()
        again = c.audio_features_many(tracks, 8000)
        for a, b, s in zip(first, again, singles[8000]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)) and np.array_equal(a.view(np.uint8), s.rec.view(np.uint8))


def test_a_batch_drains_a_pending_asynchronous_analysis(singles):
    from avd_hip import synth
    clip = synth.make_clip(8, 180, 320, seed=5, dup_every=3)
    with avd_hip.Context(0) as c:
        want = c.analyze_frames(clip).copy()
    tracks = _tracks(1001)
    with avd_hip.Context(0) as c:
        rec = np.zeros(len(clip), avd_hip.RECORD_DTYPE)
        keep = c.analyze_frames_async(clip, rec)
        got = c.audio_features_many(tracks, 1001)
        assert rec.tobytes() == want.tobytes()                                  # filled by the audio call's drain, ahead of avd_synchronize
        c.synchronize()
        del keep
    assert rec.tobytes() == want.tobytes()
    for g, s in zip(got, singles[1001]):
        assert np.array_equal(g.view(np.uint8), s.rec.view(np.uint8))


# ---- pinned outputs -------------------------------------------------------------------------------------------------------------------------
def test_analyze_waves_against_the_reference_outputs_in_one_call(ctx, monkeypatch):
    from oracle import audio_oracle
    from tests.test_audio import _close, _wave_of
    cases = [c for c in json.load(open(os.path.join(HERE, "golden", "audio_golden.json")))["cases"] if c.get("named") != "extract_fails"]
    assert 1 < len(cases) <= 64
    calls = []
    inner = ctx._audio_call
    monkeypatch.setattr(ctx, "_audio_call", lambda *a, **k: (calls.append(1), inner(*a, **k))[1])
    got = host_audio.analyze_waves([(_wave_of(c), 16000) for c in cases], ctx)
    assert len(calls) == 1 and len(ctx.audio_tracks()) == len(cases)
    for g, c in zip(got, cases):
        assert _close(g, c["out"], 1e-6), (c.get("seed", c.get("named")), g, c["out"])
    del audio_oracle
