"""Tracks at the decoder's rate on the GPU (options "audio_rate" / "audio_channels", include/avd.h): k_audio_resample in front of the analyzer.

The rule is integer arithmetic after its first step, so every check is an equality:

  * debug buffer "audio_pcm" (the converted tracks) against the numpy restatement tests/audio_resample_reference.py with np.array_equal;
  * the records, byte for byte, against avd_audio_features under "audio_format" 1 on the restatement's int16 output.

Shapes: a call reports its tile size in "audio_rs_plan"; the lengths are 1 frame, T/2 - 1 frames, and the frames that give one tile of outputs
less one, exactly one, one more, and three tiles and one (at the upsampling rate 8000 the output count moves in steps of two, so the nearest
count at or above).  One long track (13.5 million frames at 44100) carries m * D past 2^31.
"""
import ctypes
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import avd_hip  # noqa: E402
from avd_hip import AvdError  # noqa: E402
from avd_hip import audio as host_audio  # noqa: E402
from avd_hip._lib import AUDIO_WINDOW_DTYPE, AVD_MEM_DEVICE, AVD_MEM_HOST  # noqa: E402
from tests import audio_resample_reference as ref  # noqa: E402


def _signal(n, channels, dtype, seed):
    """speech-like level with full-scale excursions; float32 tracks carry values beyond +-1 and between the 16-bit steps"""
    rng = np.random.default_rng([n, channels, seed])
    i = np.arange(n)[:, None]
    x = 0.4 * np.sin(2 * np.pi * (0.011 + 0.004 * np.arange(channels)[None, :]) * i + seed) + 0.2 * rng.standard_normal((n, channels))
    x[rng.integers(0, n, max(1, n // 50))] *= 4.0
    if dtype == np.int16:
        return np.clip(np.rint(x * 32768), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)


def _frames_for(outputs, rate):
    """the fewest frames that give at least `outputs` output samples"""
    U, D, _ = ref.ratio(rate)
    return (outputs - 1) * D // U + 1


def _bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _converted(ctx, wav, rate, win):
    """one converted call -> (records, the converted track, "audio_rs_plan")"""
    rec = ctx.audio_features(wav, win, rate=rate).copy()
    return rec, ctx.audio_pcm(), ctx.audio_resample_plan()


def _check_track(ctx, wav, rate, win=8000):
    rec, pcm, plan = _converted(ctx, wav, rate, win)
    want = ref.convert(wav, rate)
    assert plan[0] == rate and plan[1] == (wav.shape[1] if wav.ndim == 2 else 1) and plan[6] == len(wav) and plan[7] == len(want)
    assert pcm.dtype == np.int16 and np.array_equal(pcm, want), (rate, wav.shape, wav.dtype, np.flatnonzero(pcm != want)[:5])
    assert _bytes_equal(rec, ctx.audio_features(want, win)), (rate, wav.shape, wav.dtype, win)
    assert (ctx.get_option("audio_rate"), ctx.get_option("audio_channels"), ctx.get_option("audio_format")) == (0, 1, 0)
    return want


# ---- rates, channel counts, sample types, lengths, windows ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["int16", "float32"])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("rate", [48000, 44100, 24000, 8000, 16000])
def test_every_length_around_the_tile(ctx, rate, channels, dtype):
    U, D, T = ref.ratio(rate)
    _, _, plan = _converted(ctx, _signal(1, channels, dtype, 0), rate, 8000)
    assert plan[2:5] == (U, D, T) and plan[5] in (256, 512, 1024)
    tile = plan[5]
    lengths = [1, max(1, T // 2 - 1)]
    for outputs in (tile - 1, tile, tile + 1, 3 * tile + 1):
        n = _frames_for(outputs, rate)
        assert 0 <= ref.n_out(n, rate) - outputs < max(1, -(-U // D))
        lengths.append(n)
    for k, n in enumerate(lengths):
        _check_track(ctx, _signal(n, channels, dtype, k), rate)
    _check_track(ctx, _signal(lengths[-1], channels, dtype, 9), rate, win=1001)           # a short last window, the direct transform


def test_the_taps_buffer_is_the_restatements_bank(ctx):
    for rate in (48000, 44100, 24000, 8000, 11025, 16000):
        ctx.audio_features(np.zeros(5, np.int16), 8000, rate=rate)
        got = ctx.audio_resample_taps()
        assert got.dtype == np.int32 and np.array_equal(got, ref.bank(rate)[0]), rate


# ---- every row of the bank, read back through the kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [48000, 44100, 24000, 8000])
def test_impulses_at_d_consecutive_frames_read_every_bank_entry(ctx, rate):
    U, D, T = ref.ratio(rate)
    n, p0 = 2 * T + D + 8, T
    tracks = []
    for p in range(p0, p0 + D):
        x = np.zeros(n, np.int16)
        x[p] = 32767
        tracks.append(x)
    seen = np.zeros((U, T), bool)
    for g in range(0, D, 64):
        group = tracks[g:g + 64]
        ctx.audio_features_many(group, 8000, rate=rate)
        pcm, rows, taps = ctx.audio_pcm(), ctx.audio_resample_tracks(), ctx.audio_resample_taps().astype(np.int64)
        assert len(rows) == len(group)
        for j, (first, count) in enumerate(rows.tolist()):
            p = p0 + g + j
            y = pcm[first:first + count]
            assert count == ref.n_out(n, rate) and np.array_equal(y, ref.convert(group[j], rate)), (rate, p)
            m = np.arange(count)
            k = p - (m * D) // U + T // 2 - 1                                         # the tap of output m that meets frame p
            hit = (k >= 0) & (k < T)
            want = np.zeros(count, np.int64)
            want[hit] = np.clip((taps[(m * D % U)[hit], k[hit]] * 32767 + 16384) >> 15, -32768, 32767)
            assert np.array_equal(y, want), (rate, p)
            assert not seen[(m * D % U)[hit], k[hit]].any()
            seen[(m * D % U)[hit], k[hit]] = True
    assert seen.all()                                                                  # every entry exactly once


# ---- edge values --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [48000, 44100, 8000])
def test_a_full_scale_square_clamps_at_both_ends(ctx, rate):
    x = np.where((np.arange(4802) // 7) % 2 == 0, 32767, -32768).astype(np.int16)
    want = _check_track(ctx, x, rate)
    if rate != 8000:
        assert want.max() == 32767 and want.min() == -32768


def test_stereo_sums_that_cancel_and_odd_sums(ctx):
    rng = np.random.default_rng(5)
    left = rng.integers(-32768, 32768, 5000).astype(np.int16)
    anti = np.stack([left, (-left.astype(np.int32)).clip(-32768, 32767).astype(np.int16)], axis=1)
    want = _check_track(ctx, anti, 48000)
    assert np.abs(want).max() <= 1                                                    # floor((L - L + 1) / 2) = 0; L = -32768 meets R = 32767
    odd = np.stack([left, left ^ 1], axis=1)                                          # L + R is odd everywhere, below and above zero
    assert ((odd[:, 0].astype(np.int64) + odd[:, 1]) % 2 == 1).all()
    for rate in (44100, 16000):
        _check_track(ctx, odd, rate)
    extremes = np.array([[32767, 32767], [-32768, -32768], [-32768, 32767], [-1, 0], [0, -1], [-1, -2]] * 40, np.int16)
    assert np.array_equal(_check_track(ctx, extremes, 16000)[:6], [32767, -32768, 0, 0, 0, -1])


def test_float_ties_overrange_nan_and_infinities(ctx):
    special = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 32766.5, 32767.5, -32768.5, 40000.0, -40000.0, 1e30, -1e30], np.float64) / 32768.0
    special = np.concatenate([special, [np.nan, np.inf, -np.inf, 1.0, -1.0, 0.99999, 3.4e38, -3.4e38, 1e-45, -0.0]]).astype(np.float32)
    want = _check_track(ctx, special, 16000)
    assert want[:16].tolist() == [0, 2, 2, 0, -2, -2, 32766, 32767, -32768, 32767, -32768, 32767, -32768, 0, 32767, -32768]
    rng = np.random.default_rng(8)
    x = (rng.integers(-70000, 70000, 6000) / 2.0 / 32768.0).astype(np.float32)         # every second value a tie, a third beyond full scale
    x[rng.integers(0, 6000, 60)] = np.nan
    x[rng.integers(0, 6000, 20)] = np.inf
    x[rng.integers(0, 6000, 20)] = -np.inf
    for rate, channels in ((48000, 1), (44100, 2), (8000, 2)):
        _check_track(ctx, x if channels == 1 else x.reshape(-1, 2), rate)


# ---- alignment ----------------------------------------------------------------------------------------------------------------------------
def _raw(c, ptr, mem, n, win, max_windows, rate, channels, fmt, cuts=()):
    """a call of the C-ABI as a caller of it makes it: the options set, the call, the options back"""
    out = np.zeros(max(max_windows, 1), AUDIO_WINDOW_DTYPE)
    c.set_option("audio_rate", rate)
    c.set_option("audio_channels", channels)
    c.set_option("audio_format", fmt)
    try:
        for cut in cuts:
            c.set_option("audio_cut", cut)
        rc = c._L.avd_audio_features(c._h, ctypes.c_void_p(ptr), mem, n, win, ctypes.c_void_p(out.ctypes.data), max_windows)
    finally:
        c.set_option("audio_rate", 0)
        c.set_option("audio_channels", 1)
        c.set_option("audio_format", 0)
    return rc, out[:max_windows]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("dtype,channels", [(np.int16, 2), (np.float32, 1)], ids=["int16-stereo", "float32-mono"])
def test_every_input_address_mod_16(ctx, where, dtype, channels):
    rate, n = 48000, 3 * 3072 + 50
    wav = _signal(n, channels, dtype, 3)
    want_pcm = ref.convert(wav, rate)
    want = ctx.audio_features(want_pcm, 8000).copy()
    size = np.dtype(dtype).itemsize
    flat = wav.reshape(-1)
    for offset in range(0, 16, size):
        room = np.zeros(flat.nbytes + 64, np.uint8)
        if where == "device":
            import torch
            room[offset:offset + flat.nbytes] = flat.view(np.uint8)
            dev = torch.from_numpy(room).cuda()
            torch.cuda.synchronize()
            assert dev.data_ptr() % 16 == 0
            ptr, mem = dev.data_ptr() + offset, AVD_MEM_DEVICE
        else:
            base = (-room.ctypes.data) % 16 + offset                                    # first byte of the track: address = offset mod 16
            room[base:base + flat.nbytes] = flat.view(np.uint8)
            ptr, mem = room.ctypes.data + base, AVD_MEM_HOST
        assert ptr % 16 == offset
        rc, got = _raw(ctx, ptr, mem, n, 8000, len(want), rate, channels, 1 if dtype == np.int16 else 0)
        assert rc == 0, ctx._L.avd_last_error(ctx._h)
        assert np.array_equal(ctx.audio_pcm(), want_pcm), (where, offset)
        assert _bytes_equal(got, want), (where, offset)


# ---- a long track: m * D passes 2^31 -------------------------------------------------------------------------------------------------------------
def test_a_track_of_thirteen_and_a_half_million_frames(ctx):
    rate, n = 44100, 13_500_000
    U, D, T = ref.ratio(rate)
    rng = np.random.default_rng(44)
    wav = np.zeros(n, np.int16)
    wav[:6000] = rng.integers(-20000, 20000, 6000)
    wav[-6000:] = rng.integers(-20000, 20000, 6000)
    at = ((1 << 31) // D) * D // U                                                      # the frames around which m * D passes 2^31
    wav[at - 3000:at + 3000] = rng.integers(-20000, 20000, 6000)
    total = ref.n_out(n, rate)
    assert (total - 1) * D > 1 << 31
    rec = ctx.audio_features(wav, 8000, rate=rate)
    pcm, plan = ctx.audio_pcm(), ctx.audio_resample_plan()
    assert plan[6:] == (n, total) and len(pcm) == total and len(rec) == -(-total // 8000)
    assert np.array_equal(pcm[:2048], ref.convert(wav, rate, 0, 2048)) and pcm[:2048].any()
    assert np.array_equal(pcm[-2048:], ref.convert(wav, rate, total - 2048, 2048)) and pcm[-2048:].any()
    m = (1 << 31) // D - 1024
    assert np.array_equal(pcm[m:m + 2048], ref.convert(wav, rate, m, 2048)) and pcm[m:m + 2048].any()
    quiet = np.flatnonzero(pcm)
    assert ((quiet < 2300) | (quiet > total - 2300) | (np.abs(quiet - (1 << 31) // D) < 1200)).all()          # nothing lands anywhere else


# ---- batches ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,channels,dtype", [(48000, 2, np.int16), (24000, 1, np.float32), (44100, 2, np.float32)])
def test_five_tracks_cut_at_every_frame_mod_d(ctx, rate, channels, dtype):
    U, D, _ = ref.ratio(rate)
    lens = [3072 + 1, 2 * D + 1, 1, 3 * 3072 + 2, 700]
    starts = np.concatenate([[0], np.cumsum(lens)])
    if D == 3:
        assert sorted({int(s) % D for s in starts[1:-1]}) == [0, 1, 2]
    tracks = [_signal(n, channels, dtype, 20 + k) for k, n in enumerate(lens)]
    alone = []
    for t in tracks:
        rec, pcm, _ = _converted(ctx, t, rate, 1001)
        alone.append((rec, pcm))
        assert np.array_equal(pcm, ref.convert(t, rate))
    got = ctx.audio_features_many(tracks, 1001, rate=rate)
    pcm, rows = ctx.audio_pcm(), ctx.audio_resample_tracks()
    counts = [ref.n_out(n, rate) for n in lens]
    assert rows.tolist() == [[int(f), c] for f, c in zip(np.concatenate([[0], np.cumsum(counts)[:-1]]), counts)]
    assert ctx.audio_tracks()[:, 1].tolist() == [-(-c // 1001) for c in counts] and ctx.get_option("audio_cut") == 0
    for (first, count), g, (rec, single) in zip(rows.tolist(), got, alone):
        assert np.array_equal(pcm[first:first + count], single)
        assert _bytes_equal(g, rec)


def test_sixty_four_tracks(ctx):
    rate = 44100
    lens = [300 + 7 * k for k in range(64)]
    tracks = [_signal(n, 2, np.int16, 100 + k) for k, n in enumerate(lens)]
    got = ctx.audio_features_many(tracks, 8000, rate=rate)
    pcm, rows = ctx.audio_pcm(), ctx.audio_resample_tracks()
    want_pcm, want_rows = ref.convert_many(tracks, rate)
    assert np.array_equal(rows, want_rows) and np.array_equal(pcm, want_pcm)
    assert len({(n * 441) % 160 for n in np.cumsum(lens)}) > 8
    want = ctx.audio_features_many([want_pcm[f:f + c] for f, c in want_rows.tolist()], 8000)
    assert len(got) == 64 and all(_bytes_equal(g, w) for g, w in zip(got, want))
    with pytest.raises(AvdError, match="audio_cut:.*63"):
        for k in range(64):
            ctx.set_option("audio_cut", 10 + k)
    ctx.set_option("audio_cut", -1)


def test_the_cut_list_is_one_shot_after_a_refused_converted_call(ctx):
    rate, wav = 48000, _signal(9000, 2, np.int16, 31)
    want = ctx.audio_features(ref.convert(wav, rate), 1001).copy()                      # 3000 output samples: three windows
    flat = wav.reshape(-1)
    for cuts, max_windows, why in (((100, 9000), 8, "audio_cut: beyond the buffer"), ((100,), 3, "windows array too small")):
        rc, out = _raw(ctx, flat.ctypes.data, AVD_MEM_HOST, 9000, 1001, max_windows, rate, 2, 1, cuts)
        assert rc != 0 and not out.view(np.uint8).any()
        with pytest.raises(AvdError, match=why):
            ctx._check(rc)
        assert ctx.get_option("audio_cut") == 0
        assert _bytes_equal(ctx.audio_features(wav, 1001, rate=rate), want)
        assert ctx.audio_resample_tracks().tolist() == [[0, 3000]]
    # cuts are frames: the cut at frame 100 ends a track of ceil(100 / 3) = 34 output samples
    rc, out = _raw(ctx, flat.ctypes.data, AVD_MEM_HOST, 9000, 1001, 4, rate, 2, 1, (100,))
    assert rc == 0 and ctx.audio_resample_tracks().tolist() == [[0, 34], [34, 2967]] and out["length"].tolist() == [34, 1001, 1001, 965]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_next_call_alone(ctx):
    rate, wav = 44100, _signal(5000, 2, np.int16, 41)
    want_pcm = ref.convert(wav, rate)
    want = ctx.audio_features(want_pcm, 8000).copy()
    nwin = len(want)

    def next_call_is_unaffected():
        assert (ctx.get_option("audio_rate"), ctx.get_option("audio_channels")) == (0, 1)
        assert _bytes_equal(ctx.audio_features(wav, 8000, rate=rate), want) and np.array_equal(ctx.audio_pcm(), want_pcm)

    next_call_is_unaffected()
    for bad in (44000, 1, -48000, 15999, 384000):
        with pytest.raises(AvdError, match=": audio_rate:"):
            ctx.set_option("audio_rate", bad)
        assert ctx.get_option("audio_rate") == 0                                        # the old value stays
        with pytest.raises(AvdError, match="audio_rate:"):
            ctx.audio_features(wav, 8000, rate=bad)
    next_call_is_unaffected()
    for bad in (0, 3, 6, -1):
        with pytest.raises(AvdError, match=": audio_channels:"):
            ctx.set_option("audio_channels", bad)
        assert ctx.get_option("audio_channels") == 1
    with pytest.raises(AvdError, match="audio_channels:"):
        ctx.audio_features(np.zeros((100, 3), np.int16), 8000, rate=rate)
    next_call_is_unaffected()
    # an odd address (int16), an address that is 2 mod 4 (float32): refused before anything is staged or read
    room = np.zeros(4 * wav.size + 32, np.uint8)
    even = room.ctypes.data + (-room.ctypes.data) % 16
    for ptr, fmt, why in ((even + 1, 1, "2-byte aligned"), (even + 2, 0, "audio_rate: float32 samples need a 4-byte aligned wav"), (even + 3, 0, "4-byte aligned")):
        rc, out = _raw(ctx, ptr, AVD_MEM_HOST, 5000, 8000, nwin, rate, 2, fmt)
        assert rc != 0 and not out.view(np.uint8).any()
        with pytest.raises(AvdError, match=why):
            ctx._check(rc)
        next_call_is_unaffected()
    # max_windows one short of the OUTPUT's window count
    assert nwin == 1
    long = _signal(44100, 1, np.int16, 42)                                              # 16000 output samples: two windows
    rc, out = _raw(ctx, long.ctypes.data, AVD_MEM_HOST, 44100, 8000, 1, rate, 1, 1)
    assert rc != 0 and not out.view(np.uint8).any()
    with pytest.raises(AvdError, match="windows array too small"):
        ctx._check(rc)
    rc, out = _raw(ctx, long.ctypes.data, AVD_MEM_HOST, 44100, 8000, 2, rate, 1, 1)
    assert rc == 0 and out["length"].tolist() == [8000, 8000]
    next_call_is_unaffected()
    # the debug buffers describe the last call that ran, and only if it converted
    ctx.audio_features(want_pcm, 8000)
    for name in ("audio_rs_plan", "audio_rs_taps", "audio_rs_tracks", "audio_pcm"):
        with pytest.raises(AvdError, match="did not convert"):
            ctx.debug_fetch(name, (8,), np.int32)


# ---- history ----------------------------------------------------------------------------------------------------------------------------
def test_a_default_call_does_not_depend_on_converted_calls_before_it(ctx):
    plain = np.clip(_signal(20037, 1, np.float32, 50)[:, 0], -1, 1)
    pcm16 = _signal(9000, 1, np.int16, 51)[:, 0].copy()
    with avd_hip.Context(0) as fresh:
        want = fresh.audio_features(plain, 8000).copy(), fresh.audio_features(pcm16, 1001).copy()

    def same():
        assert _bytes_equal(ctx.audio_features(plain, 8000), want[0]) and _bytes_equal(ctx.audio_features(pcm16, 1001), want[1])
        assert (ctx.get_option("audio_rate"), ctx.get_option("audio_channels"), ctx.get_option("audio_format")) == (0, 1, 0)

    ctx.audio_features(_signal(4000, 2, np.float32, 52), 8000, rate=44100)
    same()
    ctx.audio_features(_signal(400000, 2, np.int16, 53), 8000, rate=192000)             # growth of every converter buffer, another bank
    ctx.audio_features(_signal(3000, 1, np.int16, 54), 8000, rate=11025)                # the wide bank
    same()
    ctx.release_workspace()
    same()
    wav = _signal(7000, 2, np.int16, 55)
    rec, pcm, _ = _converted(ctx, wav, 44100, 8000)                                     # the bank is uploaded again after the release
    assert np.array_equal(pcm, ref.convert(wav, 44100))
    ctx.release_workspace()
    with pytest.raises(AvdError, match="not allocated"):
        ctx.audio_pcm()
    same()


# ---- helpers and the drop-in ----------------------------------------------------------------------------------------------------------------
def test_analyze_decoded_equals_analyze_wave_on_the_restatements_output(ctx):
    wav = _signal(48000 * 2 + 77, 2, np.int16, 60)
    want = host_audio.analyze_wave(ref.convert(wav, 48000), 16000, ctx)
    assert host_audio.analyze_decoded(wav, 48000, ctx) == want
    mono = _signal(44100, 1, np.float32, 61)
    many = host_audio.analyze_decoded_many([(wav, 48000), (mono[:, 0], 44100), (wav[:30000], 48000)], ctx)
    assert many[0] == want and many[1] == host_audio.analyze_wave(ref.convert(mono, 44100), 16000, ctx)
    assert many[2] == host_audio.analyze_wave(ref.convert(wav[:30000], 48000), 16000, ctx)


def test_the_drop_in_converts_a_44100_stereo_wav_itself(ctx, tmp_path, monkeypatch):
    from app.analyzers import audio as drop_in
    wav = _signal(44100 * 2 + 5, 2, np.int16, 70)
    p = tmp_path / "decoded.wav"
    with wave.open(str(p), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(44100)
        w.writeframes(wav.astype("<i2").tobytes())
    monkeypatch.setenv("AVD_AUDIO_RESAMPLE", "1")
    got = drop_in.analyze(str(p), {"duration": 2.0})
    assert "error" not in got["flags_audio"], got["flags_audio"]
    assert got == host_audio.analyze_wave(ref.convert(wav, 44100), 16000, ctx)
    monkeypatch.delenv("AVD_AUDIO_RESAMPLE")
    if not __import__("shutil").which("ffmpeg"):
        assert "error" in drop_in.analyze(str(p), {"duration": 2.0})["flags_audio"]      # unset: as before
