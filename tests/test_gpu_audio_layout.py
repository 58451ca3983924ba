"""Planar and 5.1 / 7.1 tracks on the GPU (options "audio_layout" / "audio_plane_stride", include/avd.h): the layout source phase of the converter
(mix_span in k_audio_resample_layout / k_audio_resample_map_layout) and the slots' save (k_audio_slot_save_layout / _map_layout).

The referee is the numpy restatement (tests/audio_layout_reference.py on top of tests/audio_resample_reference.py): debug buffer "audio_pcm" must
equal it with np.array_equal, and the records must be byte for byte those of a plain 16 kHz call on the restatement's int16 output.  The rule is
integer arithmetic after the narrowing, so there is no tolerance anywhere.

Shapes: a tile of the converter is 256 ... 1024 outputs ("audio_rs_plan"[5]), so every case is a few thousand frames; lengths sit around the
tile's edge, around T / 2 and at 1 frame, and an odd n makes consecutive planes differ in alignment."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import avd_hip  # noqa: E402
from avd_hip import AvdError  # noqa: E402
from avd_hip import audio as host_audio  # noqa: E402
from avd_hip._lib import AUDIO_WINDOW_DTYPE, AVD_MEM_HOST  # noqa: E402
from tests import audio_layout_reference as lay  # noqa: E402
from tests import audio_resample_reference as ref  # noqa: E402

WIN = 64
LAYOUTS = (1, 2, 6, 8)
PLANAR = 0x100


@pytest.fixture(autouse=True)
def _clean(ctx):
    """every test begins with empty audio slots, no lists and the audio options at their defaults, whatever an earlier one left behind"""
    def reset():
        ctx.set_option("audio_track_slot", -1)
        ctx.set_option("audio_cut", -1)
        ctx.set_option("audio_slot", 0)
        ctx.set_option("audio_slot_reset", 0)
        for name, v in (("audio_rate", 0), ("audio_channels", 1), ("audio_format", 0), ("audio_layout", 0), ("audio_plane_stride", 0)):
            ctx.set_option(name, v)
    reset()
    yield
    reset()


def _signal(n, channels, dtype, seed):
    """[n, channels]: int16 over the full range, or float32 that leaves [-1, 1) now and then (the narrowing clamps)"""
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.int16:
        return rng.integers(-32768, 32768, (n, channels)).astype(np.int16)
    return (rng.standard_normal((n, channels)) * 0.5).astype(np.float32)


def _as_call(frames, planar):
    return np.ascontiguousarray(frames.T) if planar else frames


def _bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _outputs(rate, n):
    return ref.n_out(n, rate)


def _frames_for(rate, m):
    """the fewest frames that give at least m outputs"""
    U, D, _ = ref.ratio(rate)
    n = max(1, (m - 1) * D // U - 2)
    while _outputs(rate, n) < m:
        n += 1
    return n


def _plain(ctx, pcm, win=WIN):
    """the records of a plain 16 kHz call on int16 samples"""
    return ctx.audio_features(np.ascontiguousarray(pcm), win).copy() if len(pcm) else np.zeros(0, AUDIO_WINDOW_DTYPE)


def _check(ctx, frames, rate, layout, planar, win=WIN):
    want = lay.convert(frames, rate, layout)
    rec = ctx.audio_features(_as_call(frames, planar), win, rate=rate, layout=layout, planar=planar).copy()
    got = ctx.audio_pcm()
    assert np.array_equal(got, want), (rate, layout, planar, len(frames), np.flatnonzero(got != want)[:8])
    assert ctx.audio_resample_plan()[1] == layout
    assert _bytes_equal(rec, _plain(ctx, want, win)), (rate, layout, planar, len(frames))
    return rec, want


def _tile(ctx, rate):
    ctx.audio_features(np.zeros((1, 1), np.int16), WIN, rate=rate, layout=1)
    return ctx.audio_resample_plan()[5]


# ---- every rate, type, layout, form and length ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["int16", "float32"])
@pytest.mark.parametrize("rate", [48000, 44100, 16000, 8000])
def test_every_layout_and_length_equals_the_restatement(ctx, rate, dtype):
    tile = _tile(ctx, rate)
    _, _, T = ref.ratio(rate)
    lengths = {1, max(1, T // 2 - 1), _frames_for(rate, tile - 1), _frames_for(rate, tile), _frames_for(rate, tile + 1), _frames_for(rate, tile + 1) | 1,
               _frames_for(rate, 2 * tile + 37) | 1}
    assert {_outputs(rate, n) for n in lengths} >= {tile, tile + 1} or rate == 8000           # 8000 doubles: odd counts do not exist there
    seed = 0
    for layout in LAYOUTS:
        for planar in (False, True):
            for n in sorted(lengths):
                seed += 1
                _check(ctx, _signal(n, layout, dtype, rate + seed), rate, layout, planar)


# ---- equivalences ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["int16", "float32"])
@pytest.mark.parametrize("rate", [48000, 44100])
def test_planar_and_interleaved_stereo_and_mono_are_audio_channels_2_and_1(ctx, rate, dtype):
    n = _frames_for(rate, 2 * _tile(ctx, rate) + 101) | 1
    for channels in (1, 2):
        frames = _signal(n, channels, dtype, 7 + channels)
        old = ctx.audio_features(frames, WIN, rate=rate).copy()
        old_pcm = ctx.audio_pcm()
        assert np.array_equal(old_pcm, ref.convert(frames, rate))
        for planar in (False, True):
            rec = ctx.audio_features(_as_call(frames, planar), WIN, rate=rate, layout=channels, planar=planar).copy()
            assert np.array_equal(ctx.audio_pcm(), old_pcm) and _bytes_equal(rec, old), (channels, planar)


# ---- alignment and strides -------------------------------------------------------------------------------------------------------------------------
def _strided(flat, off, channels, n, stride, device):
    """[channels, n] over flat[off ...], planes `stride` samples apart, in host or device memory, without a copy"""
    if device:
        import torch
        return torch.as_strided(flat, (channels, n), (stride, 1), off)
    item = flat.dtype.itemsize
    return np.lib.stride_tricks.as_strided(flat[off:], shape=(channels, n), strides=(stride * item, item), writeable=False)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["int16", "float32"])
def test_every_plane_0_address_and_stride(ctx, device, dtype):
    rate, layout = 48000, 6
    item = np.dtype(dtype).itemsize
    n = _frames_for(rate, _tile(ctx, rate) + 77) | 1                                       # odd: consecutive dense planes differ in alignment
    frames = _signal(n, layout, dtype, 21)
    want = lay.convert(frames, rate, layout)
    want_rec = _plain(ctx, want)
    ring = 3 * n + 5
    room = np.zeros(layout * ring + 32, dtype)
    base = ((-room.ctypes.data) % 16) // item
    if device:
        import torch
        dev = torch.zeros(len(room), dtype=torch.int16 if item == 2 else torch.float32, device="cuda")
        base = ((-dev.data_ptr()) % 16) // item
    seen = set()
    for shift in range(16 // item):
        for stride in (n, n + 1, n + 7, ring):
            room[:] = 12345 if item == 2 else np.nan                                           # what lies between the planes must not matter
            off = base + shift
            for c in range(layout):
                room[off + c * stride:off + c * stride + n] = frames[:, c]
            if device:
                dev.copy_(torch.from_numpy(room))
                src = _strided(dev, off, layout, n, stride, True)
                seen.add(src.data_ptr() % 16)
            else:
                src = _strided(room, off, layout, n, stride, False)
                seen.add(src.ctypes.data % 16)
            rec = ctx.audio_features(src, WIN, rate=rate, layout=layout, planar=True).copy()
            assert np.array_equal(ctx.audio_pcm(), want), (shift, stride)
            assert _bytes_equal(rec, want_rec), (shift, stride)
            assert int(ctx.debug_fetch("stage_bytes", (1,), np.int64)[0]) == (0 if device else layout * n * item), (shift, stride)
            got = ctx.audio_layout()
            assert got[:4].tolist() == [layout, 1, layout, stride] and got[4:].tolist() == list(lay.TABLE[layout]) + [0, 0]
    assert seen == set(range(0, 16, item))
    # interleaved 7.1 at every address of its sample type
    frames = _signal(n, 8, dtype, 22)
    want = lay.convert(frames, rate, 8)
    room = np.zeros(8 * n + 32, dtype)
    base = ((-room.ctypes.data) % 16) // item
    for shift in range(16 // item):
        flat = room[base + shift:base + shift + 8 * n]
        flat[:] = frames.reshape(-1)
        if device:
            dev8 = torch.zeros(len(room), dtype=torch.int16 if item == 2 else torch.float32, device="cuda")
            b8 = ((-dev8.data_ptr()) % 16) // item
            src = dev8[b8 + shift:b8 + shift + 8 * n]
            src.copy_(torch.from_numpy(np.ascontiguousarray(flat)))
            assert src.data_ptr() % 16 == shift * item
        else:
            src = flat
            assert src.ctypes.data % 16 == shift * item
        ctx.audio_features(src, WIN, rate=rate, layout=8)
        assert np.array_equal(ctx.audio_pcm(), want), shift
        assert int(ctx.debug_fetch("stage_bytes", (1,), np.int64)[0]) == (0 if device else 8 * n * item)


# ---- content ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
def test_one_hot_channels_recover_the_weights_and_the_extremes_stay_inside_16_bits(ctx, planar):
    n = 777
    for layout in LAYOUTS:
        for c in range(layout):
            for full in (32767, -32768):
                frames = np.zeros((n, layout), np.int16)
                frames[:, c] = full
                _, pcm = _check(ctx, frames, 16000, layout, planar)                         # 16000: no filter, "audio_pcm" is M itself
                assert (pcm == (lay.TABLE[layout][c] * full + 16384) >> 15).all(), (layout, c, full)
        for full in (32767, -32768):
            _, pcm = _check(ctx, np.full((n, layout), full, np.int16), 16000, layout, planar)
            assert (pcm == full).all()
            _check(ctx, np.full((n, layout), full, np.int16), 44100, layout, planar)
            ones = np.full((n, layout), 1.5 if full > 0 else -1.5, np.float32)                # float32 beyond full scale: clamped per sample first
            _, pcm = _check(ctx, ones, 16000, layout, planar)
            assert (pcm == full).all()
    for layout in (6, 8):
        frames = np.zeros((n, layout), np.int16)
        frames[:, 3] = 32767                                                                 # LFE alone: silence
        _, pcm = _check(ctx, frames, 48000, layout, planar)
        assert not pcm.any()


@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
def test_an_lfe_of_nan_and_inf_changes_nothing(ctx, planar):
    for layout in (6, 8):
        for rate in (48000, 16000):
            frames = _signal(2999, layout, np.float32, 31 + layout)
            frames[:, 3] = 0.0
            want = lay.convert(frames, rate, layout)
            for poison in (np.nan, np.inf, -np.inf, 3.0e38):
                bad = frames.copy()
                bad[:, 3] = poison
                bad[::7, 3] = -poison if poison == poison else np.nan
                rec = ctx.audio_features(_as_call(bad, planar), WIN, rate=rate, layout=layout, planar=planar).copy()
                assert np.array_equal(ctx.audio_pcm(), want), (layout, rate, poison)
                assert _bytes_equal(rec, _plain(ctx, want))


# ---- batches ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tracks,rate,layout,planar,dtype", [(5, 44100, 6, True, np.float32), (5, 48000, 8, False, np.int16), (64, 48000, 6, True, np.int16),
                                                             (64, 8000, 2, True, np.float32)], ids=["5-planar-5.1", "5-interleaved-7.1", "64-planar-5.1", "64-planar-stereo"])
def test_a_cut_call_gives_every_track_its_own_bytes(ctx, tracks, rate, layout, planar, dtype):
    tile = _tile(ctx, rate)
    big = _frames_for(rate, tile + 50)
    lens = [(big if t % 16 == 0 else 150 + 31 * t) | 1 for t in range(tracks)]               # odd frames: every later track begins at an odd position
    wavs = [_signal(n, layout, dtype, 50 + t) for t, n in enumerate(lens)]
    wants = [lay.convert(w, rate, layout) for w in wavs]
    recs = ctx.audio_features_many([_as_call(w, planar) for w in wavs], WIN, rate=rate, layout=layout, planar=planar)
    recs = [r.copy() for r in recs]
    assert np.array_equal(ctx.audio_pcm(), np.concatenate(wants))
    assert ctx.audio_layout()[:4].tolist() == [layout, int(planar), layout, sum(lens) if planar else 0]
    for t in range(tracks):
        assert _bytes_equal(recs[t], _plain(ctx, wants[t])), t
    if tracks == 5:                                                                          # the same tracks from device memory
        import torch
        dev = [torch.from_numpy(_as_call(w, planar)).cuda() for w in wavs]
        again = ctx.audio_features_many(dev, WIN, rate=rate, layout=layout, planar=planar)
        assert all(_bytes_equal(a, b) for a, b in zip(again, recs))
        assert int(ctx.debug_fetch("stage_bytes", (1,), np.int64)[0]) == 0


# ---- slots -----------------------------------------------------------------------------------------------------------------------------------------
def _chunk_bounds(rate, tile, total):
    _, D, T = ref.ratio(rate)
    U = ref.ratio(rate)[0]
    span = tile * D // U
    sizes = [max(1, s) for s in (T // 2 - 1, 1, 1, T // 2, T, T + 1, span - 1, 1, span + 1, 3)]
    bounds, at = [0], 0
    for s in sizes:
        if at + s >= total:
            break
        at += s
        bounds.append(at)
    return bounds + [total]


@pytest.mark.parametrize("rate,layout,planar,dtype", [(44100, 6, True, np.float32), (48000, 8, False, np.int16), (48000, 2, True, np.int16), (8000, 6, True, np.int16),
                                                      (16000, 8, True, np.float32)], ids=["44100-planar-5.1-f32", "48000-interleaved-7.1-s16", "48000-planar-stereo-s16",
                                                                                        "8000-planar-5.1-s16", "16000-planar-7.1-f32"])
def test_a_track_through_a_slot_in_chunks_is_the_whole_call(ctx, rate, layout, planar, dtype):
    tile = _tile(ctx, rate)
    total = _frames_for(rate, 2 * tile + 333) | 1
    frames = _signal(total, layout, dtype, 60 + layout)
    whole, want = _check(ctx, frames, rate, layout, planar)
    bounds = _chunk_bounds(rate, tile, total)
    assert len(bounds) > 8
    ring = np.zeros((layout, total + 9), frames.dtype)                                       # planar chunks are column slices of a wider array:
    ring[:, 4:4 + total] = frames.T                                                          # each call has its own plane-0 address, one stride
    recs, pcm = [], []
    for k, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        chunk = ring[:, 4 + a:4 + b] if planar else frames[a:b]
        recs.append(ctx.audio_features(chunk, WIN, rate=rate, slot=3, last=b == total, layout=layout, planar=planar).copy())
        pcm.append(ctx.audio_pcm())
        if planar and layout > 1:
            assert ctx.audio_layout()[3] == total + 9
    assert np.array_equal(np.concatenate(pcm), want)
    assert _bytes_equal(np.concatenate(recs), whole)


def test_history_across_release_workspace_and_a_pending_asynchronous_call(ctx):
    rate, layout = 44100, 6
    total = 9001
    frames = _signal(total, layout, np.float32, 71)
    whole, want = _check(ctx, frames, rate, layout, True)
    planar = _as_call(frames, True)
    video = np.random.default_rng(72).integers(0, 255, (3, 240, 320, 3), dtype=np.uint8)
    recs, pcm = [], []

    def go(a, b):
        recs.append(ctx.audio_features(planar[:, a:b], WIN, rate=rate, slot=2, last=b == total, layout=layout, planar=True).copy())
        pcm.append(ctx.audio_pcm())

    go(0, 2000)
    ctx.release_workspace()                                                                  # the scratch goes, the slot's history stays
    go(2000, 2045)
    ctx.audio_features(_signal(3000, 2, np.int16, 73), WIN, rate=48000)                      # another bank, no layout, slot 0
    go(2045, 5000)
    rec_async = np.zeros(len(video), avd_hip.RECORD_DTYPE)
    keep = ctx.analyze_frames_async(video, rec_async)                                        # a pending asynchronous analysis: drained first
    go(5000, 7000)
    ctx.synchronize()
    del keep
    assert rec_async.view(np.uint8).any()
    go(7000, total)
    assert np.array_equal(np.concatenate(pcm), want) and _bytes_equal(np.concatenate(recs), whole)


def test_a_mapped_round_of_three_planar_streams_with_a_late_joiner_and_an_end(ctx):
    rate, layout = 48000, 6
    tile = _tile(ctx, rate)
    lens = [_frames_for(rate, tile + 400) | 1, 2 * 1501, 1777]
    wavs = [_signal(n, layout, np.int16, 80 + t) for t, n in enumerate(lens)]
    wholes, wants = zip(*[_check(ctx, w, rate, layout, True) for w in wavs])
    P = [_as_call(w, True) for w in wavs]
    recs, pcm = [[] for _ in wavs], [[] for _ in wavs]

    def round_(members):
        """members: [(track, a, b)]; slot = track + 1"""
        got = ctx.audio_features_mapped([P[t][:, a:b] for t, a, b in members], [t + 1 for t, _, _ in members], [b == lens[t] for t, _, b in members], WIN,
                                        rate=rate, layout=layout, planar=True)
        new = ctx.audio_pcm()
        rows = ctx.audio_resample_tracks()
        assert ctx.audio_layout()[:4].tolist() == [layout, 1, layout, sum(b - a for _, a, b in members)]
        at = 0
        for (t, _, _), rec, row in zip(members, got, rows):
            recs[t].append(rec.copy())
            pcm[t].append(new[at:at + row[1]])
            at += row[1]

    round_([(0, 0, 1001), (1, 0, 1501)])
    round_([(1, 1501, 3002), (2, 0, 1000), (0, 1001, 1050)])                                 # track 2 joins; track 1 ends
    round_([(2, 1000, 1777), (0, 1050, lens[0])])                                            # both end
    for t in range(3):
        assert np.array_equal(np.concatenate(pcm[t]), wants[t]), t
        assert _bytes_equal(np.concatenate(recs[t]), wholes[t]), t


def test_a_slot_keeps_its_layout(ctx):
    rate = 48000
    frames = _signal(4001, 6, np.int16, 90)
    whole, want = _check(ctx, frames, rate, 6, True)
    P = _as_call(frames, True)
    first = ctx.audio_features(P[:, :2000], WIN, rate=rate, slot=4, layout=6, planar=True).copy()
    pcm = [ctx.audio_pcm()]
    state = [ctx.get_option("audio_slot_frames")]
    for how in (dict(layout=6, planar=False), dict(layout=8, planar=True), dict()):
        other = np.zeros((100, how.get("layout", 2)), np.int16)
        other = _as_call(other, how.get("planar", False))
        with pytest.raises(AvdError, match="audio_slot: win"):
            ctx.audio_features(other, WIN, rate=rate, slot=4, **how)
        with pytest.raises(AvdError, match="audio_track_slot: win"):
            ctx.audio_features_mapped([other], [4], [False], WIN, rate=rate, **how)
    # the refused calls left the slot as it was: the track goes on to the whole call's bytes, with another stride
    wide = np.zeros((6, 5000), np.int16)
    wide[:, 17:17 + 2001] = P[:, 2000:]
    rest = ctx.audio_features(wide[:, 17:17 + 2001], WIN, rate=rate, slot=4, last=True, layout=6, planar=True).copy()
    pcm.append(ctx.audio_pcm())
    assert np.array_equal(np.concatenate(pcm), want) and _bytes_equal(np.concatenate([first, rest]), whole)
    assert state


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def _raw(c, ptr, n, max_windows, rate, layout, stride, fmt, cuts=(), slot=0, entries=(), mem=AVD_MEM_HOST):
    """a call of the C-ABI as a caller of it makes it: the options set, the call, the options back -> (status, records, the error text)"""
    out = np.zeros(max(max_windows, 1), AUDIO_WINDOW_DTYPE)
    c.set_option("audio_rate", rate)
    c.set_option("audio_layout", layout)
    c.set_option("audio_plane_stride", stride)
    c.set_option("audio_format", fmt)
    try:
        c.set_option("audio_slot", slot)
        for cut in cuts:
            c.set_option("audio_cut", cut)
        for e in entries:
            c.set_option("audio_track_slot", e)
        rc = c._L.avd_audio_features(c._h, ctypes.c_void_p(ptr), mem, n, WIN, ctypes.c_void_p(out.ctypes.data), max_windows)
    finally:
        c.set_option("audio_slot", 0)
        for name, v in (("audio_rate", 0), ("audio_layout", 0), ("audio_plane_stride", 0), ("audio_format", 0)):
            c.set_option(name, v)
    why = ""
    if rc != 0:
        try:
            c._check(rc)
        except AvdError as e:
            why = str(e)
    return rc, out[:max_windows], why


def test_every_new_refusal_in_its_order_and_the_next_call_unaffected(ctx):
    # at the set: the old value stays
    ctx.set_option("audio_layout", 6 | PLANAR)
    for bad in (3, 4, 5, 7, 9, PLANAR, 0x200 | 2, 0x106 | 0x400, -1, -6):
        with pytest.raises(AvdError, match=r"^avd status -?\d+: audio_layout:"):
            ctx.set_option("audio_layout", bad)
        assert ctx.get_option("audio_layout") == 6 | PLANAR
    ctx.set_option("audio_plane_stride", 12)
    with pytest.raises(AvdError, match=r"^avd status -?\d+: audio_plane_stride:"):
        ctx.set_option("audio_plane_stride", -1)
    assert ctx.get_option("audio_plane_stride") == 12
    ctx.set_option("audio_layout", 0)
    ctx.set_option("audio_plane_stride", 0)
    # at the call
    rate, layout, n = 48000, 6, 3001
    frames = _signal(n, layout, np.int16, 95)
    want = lay.convert(frames, rate, layout)
    want_rec = _plain(ctx, want)
    need = len(want_rec)
    P = np.zeros((layout, n + 8), np.int16)
    P[:, :n] = frames.T
    good = dict(ptr=P.ctypes.data, n=n, max_windows=need, rate=rate, layout=layout | PLANAR, stride=n + 8, fmt=1)

    def the_good_call():
        rc, out, text = _raw(ctx, **good)
        assert rc == 0, text
        assert np.array_equal(ctx.audio_pcm(), want) and _bytes_equal(out, want_rec)

    the_good_call()
    f32 = np.zeros(layout * (n + 8) + 4, np.float32)
    for form in (dict(), dict(slot=5), dict(entries=(5,))):
        aligned = "2-byte aligned"
        refusals = [
            # each call has later faults as well, and is refused for the earliest
            (dict(ptr=P.ctypes.data + 1, stride=n - 1, cuts=(n,), max_windows=0), aligned),
            (dict(stride=n - 1, cuts=(n,), max_windows=0), "audio_plane_stride:"),
            (dict(stride=1, max_windows=0), "audio_plane_stride:"),
            (dict(cuts=(n,), max_windows=0), "audio_cut: beyond the buffer" if "slot" not in form else "audio_slot: one track per call"),
            (dict(max_windows=0), "windows array too small"),
        ]
        for how, why in refusals:
            args = {**good, **form, **how}
            rc, out, text = _raw(ctx, **args)
            assert rc != 0 and why in text, (form, how, rc, text)
            assert not out.view(np.uint8).any()
            the_good_call()                                                                   # ... and the next call is what it always was
        rc, out, text = _raw(ctx, **{**good, **form, "ptr": f32.ctypes.data + 2, "fmt": 0, "stride": n - 1})
        assert rc != 0 and "4-byte aligned" in text, (form, text)
        rc, out, text = _raw(ctx, **{**good, **form, "ptr": f32.ctypes.data, "fmt": 0, "stride": n - 1})
        assert rc != 0 and "audio_plane_stride:" in text, (form, text)
    # a stride is not read without the planar flag, and neither option without a rate
    inter = np.ascontiguousarray(frames)
    rc, out, text = _raw(ctx, inter.ctypes.data, n, need, rate, layout, 5, 1)
    assert rc == 0 and np.array_equal(ctx.audio_pcm(), want), text
    mono = np.ascontiguousarray(want)
    rc, out, text = _raw(ctx, mono.ctypes.data, len(mono), need, 0, layout | PLANAR, 5, 1)
    assert rc == 0 and _bytes_equal(out, want_rec), text
    # while "audio_layout" is not 0, "audio_channels" is not read
    ctx.set_option("audio_channels", 2)
    the_good_call()
    ctx.set_option("audio_channels", 1)
    for slot in (5,):
        ctx.set_option("audio_slot", slot)
        assert ctx.get_option("audio_slot_frames") == 0                                       # every refused slot call left its slot empty
        ctx.set_option("audio_slot", 0)


# ---- the debug buffer ------------------------------------------------------------------------------------------------------------------------------
def test_the_audio_layout_debug_buffer(ctx):
    with avd_hip.Context(0) as fresh:
        with pytest.raises(AvdError, match="audio_layout"):
            fresh.audio_layout()
        fresh.audio_features(np.zeros(100, np.float32), WIN)                                  # a call that does not convert records nothing
        with pytest.raises(AvdError, match="audio_layout"):
            fresh.audio_layout()
        fresh.audio_features(np.zeros((100, 2), np.int16), WIN, rate=48000)                   # by "audio_channels": id 0, the stereo weights
        assert fresh.audio_layout().tolist() == [0, 0, 2, 0, 16384, 16384, 0, 0, 0, 0, 0, 0]
        fresh.audio_features(np.zeros(100, np.float32), WIN, rate=16000)
        assert fresh.audio_layout().tolist() == [0, 0, 1, 0, 32768, 0, 0, 0, 0, 0, 0, 0]
    ring = np.zeros((8, 4000), np.float32)
    ctx.audio_features(ring[:, 5:1006], WIN, rate=44100, layout=8, planar=True)
    assert ctx.audio_layout().tolist() == [8, 1, 8, 4000] + list(lay.TABLE[8])
    assert ctx.audio_resample_plan()[:2] == (44100, 8)
    ctx.audio_features(np.zeros((1001, 6), np.int16), WIN, rate=44100, layout=6)
    assert ctx.audio_layout().tolist() == [6, 0, 6, 0] + list(lay.TABLE[6]) + [0, 0]
    ctx.audio_features(np.zeros((2, 1001), np.int16), WIN, rate=8000, layout=2, planar=True)
    assert ctx.audio_layout().tolist() == [2, 1, 2, 1001, 16384, 16384, 0, 0, 0, 0, 0, 0]
    ctx.audio_features(np.zeros(100, np.float32), WIN)                                        # the last call that CONVERTED
    assert ctx.audio_layout()[0] == 2
    assert (ctx.get_option("audio_layout"), ctx.get_option("audio_plane_stride")) == (0, 0)   # the binding put both back


# ---- the helpers and the drop-in -------------------------------------------------------------------------------------------------------------------
def test_the_helpers_and_the_drop_in_on_a_written_6_channel_wav(ctx, tmp_path, monkeypatch):
    import wave
    from app.analyzers import audio as dropin
    rate, n = 48000, 48000 + 4801
    pcm = _signal(n, 6, np.int16, 99)
    pcm[:, 3] = 32767                                                                         # a loud LFE that must not be heard
    path = tmp_path / "surround.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(6); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(pcm.astype("<i2").tobytes())
    mono = lay.convert(pcm, rate, 6)
    want = host_audio.analyze_wave(mono, 16000, ctx)
    assert host_audio.analyze_decoded(pcm, rate, ctx, layout=host_audio.layout_of(6)) == want
    assert host_audio.analyze_decoded(np.ascontiguousarray(pcm.T), rate, ctx, layout=6, planar=True) == want
    packets = [np.ascontiguousarray(pcm.T)[:, a:a + 1024] for a in range(0, n, 1024)]
    assert host_audio.analyze_decoded_chunks(iter(packets), rate, ctx, layout=6, planar=True) == want
    assert host_audio.analyze_decoded_streams([packets, packets[:20]], rate, ctx, layout=6, planar=True)[0] == want
    assert host_audio.analyze_decoded_many([(pcm, rate), (pcm[:5000], rate)], ctx, layout=6)[0] == want
    meta = {"duration": n / rate}
    monkeypatch.setenv("AVD_AUDIO_RESAMPLE", "1")
    monkeypatch.setenv("AVD_AUDIO_LAYOUT", "1")
    monkeypatch.delenv("AVD_AUDIO_CHUNK", raising=False)
    assert dropin.analyze(str(path), meta) == want
    monkeypatch.setenv("AVD_AUDIO_CHUNK", "1000")
    assert dropin.analyze(str(path), meta) == want
    monkeypatch.delenv("AVD_AUDIO_LAYOUT")
    monkeypatch.delenv("AVD_AUDIO_CHUNK")
    assert dropin.analyze(str(path), meta) != want                                            # without the second variable: the usual way, first channel only
