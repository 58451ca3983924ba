"""A track continued across avd_audio_features calls on the GPU (options "audio_slot", "audio_end", "audio_slot_reset", include/avd.h):
k_audio_resample with a two-part source (the slot's history | the call's frames), the analyzer over [held | new], one save launch per call.

The referee is the one-call path (slot 0), which tests/test_gpu_audio_resample.py pins against the numpy restatement: for ANY split of a track
into calls the concatenated records are byte for byte those of one slot-0 call on the joined samples, and the concatenated new outputs (debug
buffer "audio_pcm" after each call) are that call's "audio_pcm".  Everything is integer arithmetic or the same kernels over the same sample
values, so every check is np.array_equal -- no tolerance anywhere.

Shapes.  win 64 and 1001 keep a track to a few thousand outputs (a tile and a bit, so that more than one workgroup runs and a tile boundary falls
inside a call); chunk lengths are 1, T/2 - 1, T/2, T/2 + 1, T - 1, T, one tile's frames -1 / +0 / +1, and lengths that land a boundary on a
window edge and on a 16-byte line; one track (44.1 kHz, 13.5 million frames, win 8000) carries m D past 2^31 and runs the 80 x 100 transform.
After every call the read-only options are held to the rule."""
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


@pytest.fixture(autouse=True)
def _empty_slots(ctx):
    """every test begins with eight empty audio slots, whatever an earlier one left behind"""
    ctx.set_option("audio_slot_reset", 0)
    yield


def _ratio(rate):
    return ref.ratio(rate) if rate else (1, 1, 0)


def _outputs(rate, n, last=False):
    """M of the rule"""
    U, D, T = _ratio(rate)
    return -(-(n if last else max(0, n - T // 2)) * U // D)


def _signal(n, channels, dtype, seed):
    """speech-like level with full-scale excursions; float32 tracks carry values beyond +-1 and between the 16-bit steps"""
    rng = np.random.default_rng([n, channels, seed])
    i = np.arange(n)[:, None]
    x = 0.4 * np.sin(2 * np.pi * (0.011 + 0.004 * np.arange(channels)[None, :]) * i + seed) + 0.2 * rng.standard_normal((n, channels))
    x[rng.integers(0, n, max(1, n // 50))] *= 4.0
    if dtype == np.int16:
        return np.clip(np.rint(x * 32768), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)


def _bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _whole(ctx, wav, win, rate):
    """the referee: one slot-0 call -> (records, its "audio_pcm"; an unconverted track: its own samples)"""
    if rate:
        rec = ctx.audio_features(wav, win, rate=rate).copy()
        return rec, ctx.audio_pcm()
    return ctx.audio_features(wav[:, 0], win).copy(), wav[:, 0]


def _cuts(n, sizes):
    """chunk boundaries 0 = b0 < b1 < ... = n, the lengths taken from `sizes` in turn (cycled; lengths below 1 are skipped)"""
    sizes = [s for s in sizes if s >= 1]
    at, k, out = 0, 0, [0]
    while at < n:
        at = min(n, at + sizes[k % len(sizes)])
        out.append(at)
        k += 1
    return out


def _chunked(ctx, wav, win, rate, bounds, slot=1, flush=False, device=False, state=None):
    """the track in calls wav[b0:b1], wav[b1:b2], ... on `slot` -> (records, new outputs), each concatenated.  The last call is marked as the end
    (flush: an empty marked call follows the last samples instead).  After every call the read-only options are held to the rule.
    state: {"frames": ...} to continue a track begun by an earlier _chunked (then `bounds` goes on from there and the end is not marked)."""
    recs, pcm = [], []
    calls = [(wav[a:b], b == len(wav) and not flush and state is None) for a, b in zip(bounds[:-1], bounds[1:])]
    if flush and state is None:
        calls.append((wav[:0], True))
    frames = state["frames"] if state else 0
    for chunk, last in calls:
        arg = chunk if rate else chunk[:, 0]
        if device:
            import torch
            arg = torch.from_numpy(np.ascontiguousarray(arg)).cuda()
        rec = ctx.audio_features(arg, win, rate=rate or None, slot=slot, last=last)
        m0, m1 = _outputs(rate, frames), _outputs(rate, frames + len(chunk), last)
        assert len(rec) == (-(-m1 // win) if last else m1 // win) - m0 // win
        recs.append(rec.copy())
        if rate:
            new = ctx.audio_pcm()
            assert len(new) == m1 - m0 and ctx.audio_resample_plan()[6:] == (len(chunk), m1 - m0)
            pcm.append(new)
        else:
            pcm.append(chunk[:, 0])
        frames = 0 if last else frames + len(chunk)
        assert ctx.get_option("audio_slot") == 0 and ctx.get_option("audio_end") == 0
        ctx.set_option("audio_slot", slot)
        try:
            got = tuple(ctx.get_option("audio_slot_" + k) for k in ("frames", "held", "windows"))
        finally:
            ctx.set_option("audio_slot", 0)
        assert got == ((frames, m1 % win, len(rec)) if frames else (0, 0, 0)), (got, frames, m1, win)
    if state is not None:
        state["frames"] = frames
    return np.concatenate(recs), np.concatenate(pcm)


def _check_split(ctx, wav, win, rate, sizes, want=None, **how):
    want = want or _whole(ctx, wav, win, rate)
    rec, pcm = _chunked(ctx, wav, win, rate, _cuts(len(wav), sizes), **how)
    assert np.array_equal(pcm, want[1]), (rate, wav.shape, wav.dtype, sizes[:6], np.flatnonzero(pcm != want[1])[:5] if len(pcm) == len(want[1]) else (len(pcm), len(want[1])))
    assert _bytes_equal(rec, want[0]), (rate, wav.shape, wav.dtype, win, sizes[:6])
    return want


def _track_frames(rate, extra_outputs=300):
    """frames that give one tile of outputs and a bit, and three supports: more than one workgroup, a tile boundary inside a call"""
    U, D, T = _ratio(rate)
    tile = 1024 if not rate else min(1024, max(256, 4096 * U // D // 256 * 256))
    return (tile + extra_outputs) * D // U + 3 * T + 7, tile * D // U


# ---- whole == chunks --------------------------------------------------------------------------------------------------------------------------
# an unconverted track ("audio_rate" 0) is mono by definition: there is no stereo call of it
CASES = [(rate, dtype, channels) for rate in (16000, 48000, 44100, 11025, 192000, 0) for dtype in (np.int16, np.float32) for channels in (1, 2) if rate or channels == 1]


@pytest.mark.parametrize("rate,dtype,channels", CASES, ids=["%d-%s-%d" % (r, np.dtype(d).name, c) for r, d, c in CASES])
def test_whole_equals_chunks(ctx, rate, dtype, channels):
    U, D, T = _ratio(rate)
    n, per_tile = _track_frames(rate)
    wav = _signal(n, channels, dtype, rate // 1000)
    want = _whole(ctx, wav, 64, rate)
    assert len(want[0]) == -(-_outputs(rate, n, True) // 64) > 4
    # the supports' edges: T/2 - 1, T/2, T/2 + 1, T - 1, T, and single frames in between
    _check_split(ctx, wav, 64, rate, [T // 2 - 1, 1, T // 2, 1, 1, T // 2 + 1, T - 1, 1, T, 1, 1, 1], want)
    # one tile's frames - 1, + 1, + 0: the first call ends a frame short of the tile, the second a frame beyond the next
    _check_split(ctx, wav, 64, rate, [per_tile - 1, per_tile + 1, per_tile], want)
    # frame by frame through the head of the track (no output at all until T/2 frames are in; the history fills and then shifts), then the rest
    head = 2 * T + 3 * max(1, D // U) + 5
    _check_split(ctx, wav, 64, rate, [1] * head + [n], want)
    # another window length: the short last window takes its own tables, a full one the direct transform
    _check_split(ctx, wav, 1001, rate, [per_tile // 3 + 1, 5, T + 2])


@pytest.mark.parametrize("rate", [48000, 44100, 0])
def test_from_device_memory(ctx, rate):
    U, D, T = _ratio(rate)
    n, per_tile = _track_frames(rate)
    for dtype, channels in ((np.int16, 2 if rate else 1), (np.float32, 1)):
        wav = _signal(n, channels, dtype, 5)
        _check_split(ctx, wav, 64, rate, [T // 2 + 1, per_tile - 1, 1, T - 1, 777], device=True)


@pytest.mark.parametrize("rate", [48000, 44100, 11025, 0])
def test_boundaries_on_a_window_edge_and_on_a_16_byte_line(ctx, rate):
    U, D, T = _ratio(rate)
    win = 64
    n, _ = _track_frames(rate)
    wav = _signal(n, 2 if rate else 1, np.int16, 8)
    # N with M(N) a multiple of win: the call leaves nothing held, the next one begins a window
    edges = []
    N = T // 2 + 1
    while len(edges) < 3 and N < n:
        if _outputs(rate, N) and _outputs(rate, N) % win == 0 and _outputs(rate, N - 1) % win != 0:
            edges.append(N)
            N += 2 * win * D // U
        N += 1
    assert len(edges) == 3
    bounds = [0] + edges + [n]
    rec, pcm = _chunked(ctx, wav, win, rate, bounds)
    want = _whole(ctx, wav, win, rate)
    assert np.array_equal(pcm, want[1]) and _bytes_equal(rec, want[0])
    # chunk lengths that are whole 16-byte lines of the buffer (int16 stereo: 4 frames a line; mono: 8), from an aligned start
    room = np.zeros(wav.size + 8, np.int16)
    base = ((-room.ctypes.data) % 16) // 2
    aligned = room[base:base + wav.size].reshape(wav.shape)
    aligned[:] = wav
    assert aligned.ctypes.data % 16 == 0
    _check_split(ctx, aligned, win, rate, [8 * 13, 8 * 40, 8], want)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("dtype,channels", [(np.int16, 2), (np.float32, 1), (np.int16, 1)], ids=["int16-stereo", "float32-mono", "int16-mono"])
def test_every_input_address_mod_16(ctx, device, dtype, channels):
    rate = 48000
    n, _ = _track_frames(rate)
    wav = _signal(n, channels, dtype, 3)
    want = _whole(ctx, wav, 64, rate)
    size = np.dtype(dtype).itemsize
    room = np.zeros(wav.size + 16, dtype)
    base = ((-room.ctypes.data) % 16) // size
    flat = room[base:base + wav.size]
    flat[:] = wav.reshape(-1)
    # chunk k begins k * size bytes further into its line than chunk k - 1: lengths of lines + one sample (stereo: frames, so two samples)
    step = 16 // size // channels
    sizes = [step * 20 + 1 + (k % 3) * step for k in range(64)]
    bounds = _cuts(n, sizes)
    if device:
        import torch
        dev = torch.from_numpy(flat).cuda()
        torch.cuda.synchronize()
        assert dev.data_ptr() % 16 == 0
        chunks = [dev[a * channels:b * channels] for a, b in zip(bounds[:-1], bounds[1:])]
        residues = {c.data_ptr() % 16 for c in chunks}
    else:
        chunks = [flat[a * channels:b * channels] for a, b in zip(bounds[:-1], bounds[1:])]
        residues = {c.ctypes.data % 16 for c in chunks}
    assert residues == set(range(0, 16, size * channels)), residues                     # every address a frame can begin at
    recs, pcm = [], []
    for k, c in enumerate(chunks):
        recs.append(ctx.audio_features(c, 64, rate=rate, channels=channels, slot=2, last=k == len(chunks) - 1).copy())
        pcm.append(ctx.audio_pcm())
    assert np.array_equal(np.concatenate(pcm), want[1]) and _bytes_equal(np.concatenate(recs), want[0])


# ---- flushing ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [48000, 44100, 16000, 0])
def test_an_empty_flush_call_and_a_one_call_track(ctx, rate):
    U, D, T = _ratio(rate)
    n, per_tile = _track_frames(rate, 100)
    wav = _signal(n, 1, np.float32, 12)
    want = _check_split(ctx, wav, 64, rate, [per_tile + 5, T, 300], flush=True)
    # one call with "audio_end" == slot 0
    rec = ctx.audio_features(wav if rate else wav[:, 0], 64, rate=rate or None, slot=3, last=True)
    assert _bytes_equal(rec, want[0])
    if rate:
        assert np.array_equal(ctx.audio_pcm(), want[1])
    # an empty call without "audio_end": nothing happens, on an empty slot and on a filled one
    for slot_filled in (False, True):
        if slot_filled:
            ctx.audio_features(wav[:500] if rate else wav[:500, 0], 64, rate=rate or None, slot=3)
        assert len(ctx.audio_features(wav[:0] if rate else wav[:0, 0], 64, rate=rate or None, slot=3)) == 0
        ctx.set_option("audio_slot", 3)
        # the empty call wrote no record: "audio_slot_windows" says so, whatever the call before it wrote
        assert (ctx.get_option("audio_slot_frames"), ctx.get_option("audio_slot_windows")) == ((500, 0) if slot_filled else (0, 0))
        assert ctx.get_option("audio_slot_held") == (_outputs(rate, 500) % 64 if slot_filled else 0)
        ctx.set_option("audio_slot", 0)
    ctx.set_option("audio_slot_reset", 3)
    # a flush of an EMPTY slot: an empty track
    assert len(ctx.audio_features(wav[:0] if rate else wav[:0, 0], 64, rate=rate or None, slot=3, last=True)) == 0


# ---- 64-bit positions ---------------------------------------------------------------------------------------------------------------------------
def test_a_track_continued_past_m_d_two_to_the_31(ctx):
    rate, n, win = 44100, 13_500_000, 8000
    U, D, T = ref.ratio(rate)
    rng = np.random.default_rng(44)
    wav = np.zeros((n, 1), np.int16)
    wav[:6000, 0] = rng.integers(-20000, 20000, 6000)
    at = ((1 << 31) // D) * D // U                                                      # the frames around which m * D passes 2^31
    wav[at - 60000:, 0] = rng.integers(-20000, 20000, n - at + 60000)
    bounds = [0, 6_000_000, at - 50_000, at + 20_001, n - 3, n]
    assert bounds == sorted(bounds) and _outputs(rate, bounds[2]) * D < 1 << 31 < _outputs(rate, bounds[3]) * D
    want_rec = ctx.audio_features(wav, win, rate=rate).copy()
    assert ctx.audio_plan()[3] == len(want_rec) - 1 > 600                               # the 80 x 100 transform, and a short last window
    recs, frames = [], 0
    for k, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        last = b == n
        recs.append(ctx.audio_features(wav[a:b], win, rate=rate, slot=8, last=last).copy())
        if k >= 2:                                                                      # the calls that straddle and follow 2^31
            first, count = _outputs(rate, a), _outputs(rate, b, last) - _outputs(rate, a)
            new = ctx.audio_pcm()
            assert len(new) == count and np.array_equal(new, ref.convert(wav, rate, first, count)) and (count < 100 or new.any())
    assert _bytes_equal(np.concatenate(recs), want_rec)


# ---- slots are state ----------------------------------------------------------------------------------------------------------------------------
def test_two_slots_interleaved(ctx):
    a = _signal(9000, 2, np.int16, 20)
    b = _signal(7000, 1, np.float32, 21)
    want_a, want_b = _whole(ctx, a, 64, 48000), _whole(ctx, b, 1001, 44100)
    ba, bb = _cuts(len(a), [1500, 49, 3000]), _cuts(len(b), [45, 2000, 46, 1])
    sa, sb = {"frames": 0}, {"frames": 0}
    ra, rb, pa, pb = [], [], [], []
    for k in range(max(len(ba), len(bb)) - 1):
        # each slot's call k, alternating; the end of either track is an empty marked call below
        if k + 1 < len(ba):
            r, p = _chunked(ctx, a, 64, 48000, ba[k:k + 2], slot=1, state=sa)
            ra.append(r); pa.append(p)
        if k + 1 < len(bb):
            r, p = _chunked(ctx, b, 1001, 44100, bb[k:k + 2], slot=2, state=sb)
            rb.append(r); pb.append(p)
    ra.append(ctx.audio_features(a[:0], 64, rate=48000, slot=1, last=True).copy()); pa.append(ctx.audio_pcm())
    rb.append(ctx.audio_features(b[:0], 1001, rate=44100, slot=2, last=True).copy()); pb.append(ctx.audio_pcm())
    assert _bytes_equal(np.concatenate(ra), want_a[0]) and np.array_equal(np.concatenate(pa), want_a[1])
    assert _bytes_equal(np.concatenate(rb), want_b[0]) and np.array_equal(np.concatenate(pb), want_b[1])


def test_a_slot_survives_everything_else_on_the_context(ctx):
    rate, win = 44100, 64
    wav = _signal(12000, 2, np.int16, 30)
    want = _whole(ctx, wav, win, rate)
    other = _signal(5000, 1, np.float32, 31)
    frames = np.random.default_rng(32).integers(0, 255, (3, 240, 320, 3), dtype=np.uint8)
    bounds = [0, 2000, 2045, 5000, 8000, 11000, 12000]
    state = {"frames": 0}
    recs, pcm = [], []

    def go(k):
        r, p = _chunked(ctx, wav, win, rate, bounds[k:k + 2], slot=4, state=state)
        recs.append(r); pcm.append(p)
    go(0)
    ctx.release_workspace()                                                             # the scratch goes, the slot stays
    go(1)
    ctx.audio_features_many([other[:, 0], other[:3000, 0]], 1001)                       # a slot-0 batch, another window length
    ctx.audio_features(other, 8000, rate=48000)                                         # a slot-0 converted call at another rate: another bank
    go(2)
    ctx.analyze_frames(frames)                                                          # video
    ctx.set_option("stream_reset", 0)                                                   # the video slots' options do not reach the audio slots
    go(3)
    rec_async = np.zeros(len(frames), avd_hip.RECORD_DTYPE)
    keep = ctx.analyze_frames_async(frames, rec_async)                                  # a pending asynchronous analysis: drained first
    go(4)
    ctx.synchronize()
    del keep
    assert rec_async.view(np.uint8).any()
    recs.append(ctx.audio_features(wav[bounds[5]:], win, rate=rate, slot=4, last=True).copy()); pcm.append(ctx.audio_pcm())
    assert np.array_equal(np.concatenate(pcm), want[1]) and _bytes_equal(np.concatenate(recs), want[0])


def test_audio_slot_reset(ctx):
    wav = _signal(6000, 1, np.int16, 40)
    want = _whole(ctx, wav, 64, 48000)
    for k in (1, 2, 3):
        ctx.audio_features(wav[:1000 * k], 64, rate=48000, slot=k)

    def frames_of(k):
        ctx.set_option("audio_slot", k)
        try:
            return ctx.get_option("audio_slot_frames")
        finally:
            ctx.set_option("audio_slot", 0)
    assert [frames_of(k) for k in (1, 2, 3, 4)] == [1000, 2000, 3000, 0]
    ctx.set_option("audio_slot_reset", 2)
    assert ctx.get_option("audio_slot_reset") == 0 and [frames_of(k) for k in (1, 2, 3)] == [1000, 0, 3000]
    # the emptied slot starts a new track -- with other values than its last one, which no longer bind it
    assert _bytes_equal(ctx.audio_features(wav, 64, rate=48000, slot=2, last=True), want[0])
    ctx.audio_features(wav[:10, 0].astype(np.float32), 1001, slot=2)
    ctx.set_option("audio_slot_reset", 0)
    assert [frames_of(k) for k in (1, 2, 3)] == [0, 0, 0]
    with pytest.raises(AvdError, match="audio_slot_reset:"):
        ctx.set_option("audio_slot_reset", 9)
    for bad in (-1, 9):
        with pytest.raises(AvdError, match="audio_slot:"):
            ctx.set_option("audio_slot", bad)
    assert ctx.get_option("audio_slot") == 0
    for bad in (0, 2, -1):
        with pytest.raises(AvdError, match="audio_end:"):
            ctx.set_option("audio_end", bad)
    assert ctx.get_option("audio_end") == 0
    rec = ctx.audio_features(wav, 64, rate=48000)                                       # "audio_end" with slot 0 selected has no effect
    ctx.set_option("audio_end", 1)
    assert ctx.get_option("audio_end") == 1
    assert _bytes_equal(ctx.audio_features(wav, 64, rate=48000), rec) and ctx.get_option("audio_end") == 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def _raw(c, wav, n, win, max_windows, rate, channels, fmt, slot, end=False, cuts=(), ptr=None):
    """a call of the C-ABI as a caller of it makes it: the options set, the call, the options back -> (status, records, the error text)"""
    out = np.zeros(max(max_windows, 1), AUDIO_WINDOW_DTYPE)
    c.set_option("audio_rate", rate)
    c.set_option("audio_channels", channels)
    c.set_option("audio_format", fmt)
    c.set_option("audio_slot", slot)
    try:
        for cut in cuts:
            c.set_option("audio_cut", cut)
        if end:
            c.set_option("audio_end", 1)
        rc = c._L.avd_audio_features(c._h, ctypes.c_void_p(wav.ctypes.data if ptr is None else ptr), AVD_MEM_HOST, n, win, ctypes.c_void_p(out.ctypes.data), max_windows)
        state = tuple(c.get_option("audio_slot_" + k) for k in ("frames", "held", "windows")) + (c.get_option("audio_end"), c.get_option("audio_cut"))
    finally:
        c.set_option("audio_rate", 0)
        c.set_option("audio_channels", 1)
        c.set_option("audio_format", 0)
        c.set_option("audio_slot", 0)
    why = ""
    if rc != 0:
        try:
            c._check(rc)
        except AvdError as e:
            why = str(e)
    return rc, out[:max_windows], why, state


def test_every_refusal_leaves_the_slot_untouched(ctx):
    rate, win = 48000, 64
    wav = _signal(9000, 2, np.int16, 50)
    want = _whole(ctx, wav, win, rate)
    first = ctx.audio_features(wav[:4000], win, rate=rate, slot=5).copy()
    pcm = [ctx.audio_pcm()]
    held = _outputs(rate, 4000) % win
    before = (4000, held, len(first), 0, 0)
    rest, flat = wav[4000:], np.ascontiguousarray(wav[4000:]).reshape(-1)
    need = (held + _outputs(rate, 9000, True) - _outputs(rate, 4000) + win - 1) // win
    refusals = [
        # in the documented order: each call has every LATER fault as well, and is refused for the earliest
        (dict(cuts=(10,), win=win + 1, max_windows=0), "audio_slot: one track per call"),
        (dict(win=win + 1, max_windows=0), "audio_slot: win,"),
        (dict(rate=44100, max_windows=0), "audio_slot: win,"),
        (dict(channels=1, n=2 * len(rest), max_windows=0), "audio_slot: win,"),
        (dict(fmt=0, n=len(rest) // 2, max_windows=0), "audio_slot: win,"),
        (dict(max_windows=need - 1), "audio_slot: windows array too small"),
    ]
    for how, why in refusals:
        args = dict(n=len(rest), win=win, max_windows=need, rate=rate, channels=2, fmt=1, slot=5, end=True)
        args.update(how)
        rc, out, text, state = _raw(ctx, flat, **args)
        assert rc != 0 and why in text, (how, rc, text)
        assert not out.view(np.uint8).any()
        assert state == before, (how, state)                                            # the slot as it was; "audio_end" and the cut list consumed
    # too long a track: 2^31 - 1 outputs passed (nothing is read: the refusal comes before anything is staged)
    rc, out, text, state = _raw(ctx, flat, n=3 * 2 ** 31, win=win, max_windows=2 ** 30, rate=rate, channels=2, fmt=1, slot=5)
    assert rc != 0 and "audio_slot: more than 2^31 - 1 output samples" in text and state == before
    # an odd address and a misaligned float32 come first of all, as for every call
    rc, out, text, state = _raw(ctx, flat, n=10, win=win, max_windows=need, rate=rate, channels=2, fmt=1, slot=5, ptr=flat.ctypes.data + 1, cuts=(3,))
    assert rc != 0 and "2-byte aligned" in text and state == before
    # "audio_end" was consumed by each refused call: the next call is NOT the last ...
    rc, out, text, state = _raw(ctx, flat, n=1000, win=win, max_windows=need, rate=rate, channels=2, fmt=1, slot=5)
    assert rc == 0 and state[0] == 5000 and state[3] == 0
    recs = [first, out[:state[2]].copy()]
    pcm.append(ctx.audio_pcm())
    # ... and the track still gives the whole-track records
    recs.append(ctx.audio_features(wav[5000:], win, rate=rate, slot=5, last=True).copy())
    pcm.append(ctx.audio_pcm())
    assert _bytes_equal(np.concatenate(recs), want[0]) and np.array_equal(np.concatenate(pcm), want[1])


def test_audio_end_is_consumed_by_a_refused_call(ctx):
    wav = _signal(3000, 1, np.int16, 55)
    flat = wav.reshape(-1)
    want = _whole(ctx, wav, 64, 48000)
    # refused for its window length, with "audio_end" set: the flag is gone, the slot is still empty
    rc, out, text, state = _raw(ctx, flat, n=3000, win=9000, max_windows=100, rate=48000, channels=1, fmt=1, slot=6, end=True)
    assert rc != 0 and "audio window" in text and state == (0, 0, 0, 0, 0)
    rc, out, text, state = _raw(ctx, flat, n=1500, win=64, max_windows=100, rate=48000, channels=1, fmt=1, slot=6)
    assert rc == 0 and state[0] == 1500                                                 # not taken as the last call
    a = out[:state[2]].copy()
    b = ctx.audio_features(wav[1500:], 64, rate=48000, slot=6, last=True)
    assert _bytes_equal(np.concatenate([a, b]), want[0])


# ---- the helpers and the drop-in ----------------------------------------------------------------------------------------------------------------
def test_the_chunked_helpers_equal_their_whole_track_forms(ctx):
    wav = _signal(48000 * 2 + 77, 2, np.int16, 60)
    pieces = lambda a, size: (a[i:i + size] for i in range(0, len(a), size))            # noqa: E731
    want = host_audio.analyze_decoded(wav, 48000, ctx)
    assert host_audio.analyze_decoded_chunks(pieces(wav, 4096), 48000, ctx) == want
    assert host_audio.analyze_decoded_chunks(pieces(wav, 1024), 48000, ctx, slot=7) == want
    assert host_audio.analyze_decoded_chunks(iter([wav]), 48000, ctx) == want
    mono = _signal(44100 + 3, 1, np.float32, 61)
    assert host_audio.analyze_decoded_chunks(pieces(mono[:, 0], 4410), 44100, ctx) == host_audio.analyze_decoded(mono, 44100, ctx)
    ready = ref.convert(wav, 48000)
    assert host_audio.analyze_wave_chunks(pieces(ready, 5000), 16000, ctx) == host_audio.analyze_wave(ready, 16000, ctx)
    f32 = (ready.astype(np.float32) / np.float32(32768.0))
    assert host_audio.analyze_wave_chunks(pieces(f32, 8000), 16000, ctx) == host_audio.analyze_wave(f32, 16000, ctx)
    assert ctx.get_option("audio_slot") == 0


def test_the_drop_in_reads_a_wav_in_chunks(ctx, tmp_path, monkeypatch):
    from app.analyzers import audio as drop_in
    wav = _signal(44100 * 2 + 5, 2, np.int16, 70)
    p = tmp_path / "decoded.wav"
    with wave.open(str(p), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(44100)
        w.writeframes(wav.astype("<i2").tobytes())
    monkeypatch.setenv("AVD_AUDIO_RESAMPLE", "1")
    whole = drop_in.analyze(str(p), {"duration": 2.0})
    assert "error" not in whole["flags_audio"], whole["flags_audio"]
    reads = []
    real = host_audio.read_wav_chunks
    monkeypatch.setattr(host_audio, "read_wav_chunks", lambda path, chunk: (reads.append(len(c)) or c for c in real(path, chunk)))
    for chunk in ("4096", "1000"):
        monkeypatch.setenv("AVD_AUDIO_CHUNK", chunk)
        reads.clear()
        assert drop_in.analyze(str(p), {"duration": 2.0}) == whole
        assert reads == [int(chunk)] * (len(wav) // int(chunk)) + [len(wav) % int(chunk)]
    monkeypatch.setenv("AVD_AUDIO_CHUNK", "0")
    reads.clear()
    assert drop_in.analyze(str(p), {"duration": 2.0}) == whole and reads == []


# ---- run-order independence ----------------------------------------------------------------------------------------------------------------------
def test_slot_0_does_not_depend_on_slot_use(ctx):
    wav = _signal(20000, 2, np.int16, 80)
    mono = _signal(9000, 1, np.float32, 81)

    def slot0(c):
        a = c.audio_features(wav, 1001, rate=44100).copy()
        pcm = c.audio_pcm()
        b = c.audio_features(mono[:, 0], 8000).copy()
        many = c.audio_features_many([mono[:4000, 0], mono[4000:, 0]], 64)
        return a, pcm, b, many[0].copy(), many[1].copy()
    with avd_hip.Context(0) as fresh:
        want = slot0(fresh)
    with avd_hip.Context(0) as c:
        before = slot0(c)
        c.audio_features(wav[:7000], 1001, rate=44100, slot=1)
        c.audio_features(mono[:100, 0], 8000, slot=2)
        mid = slot0(c)                                                                  # with two slots filled
        c.audio_features(wav[7000:], 1001, rate=44100, slot=1, last=True)
        c.set_option("audio_slot_reset", 0)
        after = slot0(c)
    for got in (before, mid, after):
        assert all(_bytes_equal(g, w) for g, w in zip(got, want))
