"""Several continued tracks in ONE avd_audio_features call on the GPU (option "audio_track_slot", include/avd.h): one gather launch (k_audio_gather),
one converter launch with a source per track (k_audio_resample_map), the analyzer over a region [held | new] per track, one save launch
(k_audio_slot_save_map) -- however many tracks the call has.

The referee is one slot-0 call per whole track (tests/test_gpu_audio_resample.py pins that path against the numpy restatement), and for the slots'
state the single-slot path (tests/test_gpu_audio_stream.py): for any split of the tracks into chunks, and any assignment of the chunks to calls and
to positions within a call, each track's concatenated records are byte for byte the referee's, and its concatenated new outputs (debug buffer
"audio_pcm", which after a list call holds the tracks' new outputs side by side) are the referee's "audio_pcm".  Integer arithmetic, or the same
kernels over the same sample values: every check is np.array_equal -- no tolerance anywhere.

Shapes are those of tests/test_gpu_audio_stream.py, whose helpers this file uses: win 64 and 1001, tracks of one converter tile plus about 300
outputs plus 3 T frames, so that more than one workgroup runs per track and a tile boundary falls inside a call."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import avd_hip  # noqa: E402
from avd_hip import AvdError  # noqa: E402
from avd_hip import audio as host_audio  # noqa: E402
from avd_hip._lib import AUDIO_WINDOW_DTYPE, AVD_MEM_DEVICE, AVD_MEM_HOST  # noqa: E402
from tests import test_gpu_audio_stream as st  # noqa: E402  (helpers only: _signal, _whole, _outputs, _ratio, _cuts, _track_frames, _bytes_equal)

END = 0x10


@pytest.fixture(autouse=True)
def _empty_slots(ctx):
    """every test begins with eight empty audio slots and no list, whatever an earlier one left behind"""
    ctx.set_option("audio_track_slot", -1)
    ctx.set_option("audio_slot_reset", 0)
    yield
    ctx.set_option("audio_track_slot", -1)


def _slot_state(ctx, slot):
    ctx.set_option("audio_slot", slot)
    try:
        return tuple(ctx.get_option("audio_slot_" + k) for k in ("frames", "held", "windows"))
    finally:
        ctx.set_option("audio_slot", 0)


class Run:
    """Tracks handed over in rounds: one list call per round.  Keeps what each track has given so far, holds every round to the rule -- record
    counts, "audio_map_call", "audio_rs_tracks", "audio_tracks", the read-only slot options -- and compares with the referee at the end."""

    def __init__(self, ctx, wavs, win, rate, device=False):
        self.ctx, self.wavs, self.win, self.rate, self.device = ctx, wavs, win, rate, device
        self.at = [0] * len(wavs)                               # frames of each track handed over
        self.slot_of = [0] * len(wavs)                          # the slot each unfinished track lives in (0: not begun)
        self.recs, self.pcm = [[] for _ in wavs], [[] for _ in wavs]
        self.calls = []                                         # "audio_map_call" of every round

    def round(self, members):
        """members: [(track, frames, slot)] in call order; slot 0 = the whole track in this call.  A track ends when its frames run out."""
        ctx, win, rate = self.ctx, self.win, self.rate
        chunks, slots, lasts, plan = [], [], [], []
        for t, n, slot in members:
            a, b = self.at[t], self.at[t] + n
            assert 0 < n and b <= len(self.wavs[t]) and self.slot_of[t] in (0, slot) and (slot or (a == 0 and b == len(self.wavs[t])))
            chunk = self.wavs[t][a:b] if rate else self.wavs[t][a:b, 0]
            last = b == len(self.wavs[t])
            if self.device:
                import torch
                chunks.append(torch.from_numpy(np.ascontiguousarray(chunk)).cuda())
            else:
                chunks.append(chunk)
            slots.append(slot)
            lasts.append(last)
            m0, m1 = st._outputs(rate, a), st._outputs(rate, b, last)
            plan.append((t, slot, a, b, last, m0, m1, (-(-m1 // win) if last else m1 // win) - m0 // win))
        got = ctx.audio_features_mapped(chunks, slots, lasts, win, rate=rate or None)
        assert ctx.get_option("audio_track_slot") == 0 and ctx.get_option("audio_cut") == 0 and ctx.get_option("audio_slot") == 0
        call = ctx.audio_map_call()
        self.calls.append(call)
        held = [m0 % win for _, _, _, _, _, m0, _, _ in plan]
        fresh = [m1 - m0 for _, _, _, _, _, m0, m1, _ in plan]
        counts = [p[7] for p in plan]
        assert [len(g) for g in got] == counts
        assert call[:2] == (len(members), sum(1 for s in slots if s)) and all(v in (0, 1) for v in call[2:])
        assert call[2] == int(any(held) or not rate)            # a gather only where something is held, or the call's own samples are not converted
        assert call[3] == int(bool(rate) and any(fresh))
        assert call[4] == int(any(counts))                      # no analyzer pass (and no record copy) when no track completes a window
        assert call[5] == int(any(s and not l for s, l in zip(slots, lasts)))
        if call[4]:
            rows = ctx.audio_tracks()
            assert len(rows) == len(members) and [int(r[1]) for r in rows] == counts
            assert [int(r[0]) for r in rows] == [sum(counts[:i]) for i in range(len(counts))]
        if rate:
            rs = ctx.audio_resample_tracks()
            assert [int(r[1]) for r in rs] == fresh and ctx.audio_resample_plan()[6:] == (sum(b - a for _, _, a, b, _, _, _, _ in plan), sum(fresh))
            # regions apart: a track's [held | new] ends before the next one's begins
            for i in range(len(rs) - 1):
                assert int(rs[i][0]) + fresh[i] <= int(rs[i + 1][0]) - held[i + 1]
            assert int(rs[0][0]) == held[0]
            new = ctx.audio_pcm()
            assert len(new) == sum(fresh)
            parts = np.split(new, np.cumsum(fresh)[:-1])
        else:
            parts = [np.asarray(c.cpu()) if self.device else c for c in chunks]
        for (t, slot, a, b, last, m0, m1, count), rec, part in zip(plan, got, parts):
            self.recs[t].append(rec.copy())
            self.pcm[t].append(part)
            self.at[t] = b
            self.slot_of[t] = 0 if last else slot
            if slot:
                assert _slot_state(ctx, slot) == ((0, 0, 0) if last else (b, m1 % win, count)), (slot, a, b)
        return got

    def finish(self, wants):
        for t, want in enumerate(wants):
            assert self.at[t] == len(self.wavs[t])
            pcm, rec = np.concatenate(self.pcm[t]), np.concatenate(self.recs[t])
            assert np.array_equal(pcm, want[1]), (t, self.rate, np.flatnonzero(pcm != want[1])[:5] if len(pcm) == len(want[1]) else (len(pcm), len(want[1])))
            assert st._bytes_equal(rec, want[0]), (t, self.rate, self.win)


def _rounds(run, bounds, order):
    """every track in its own chunks (bounds[t]), a round per chunk index; the position <-> slot assignment is order(round)"""
    k = 0
    while any(k + 1 < len(b) for b in bounds):
        live = [t for t, b in enumerate(bounds) if k + 1 < len(b)]
        run.round([(t, bounds[t][k + 1] - bounds[t][k], t + 1) for t in order(k, live)])
        k += 1


# ---- mixed rounds over every case ------------------------------------------------------------------------------------------------------------------
CASES = [(48000, np.int16, 2), (44100, np.float32, 1), (11025, np.int16, 1), (192000, np.int16, 2), (16000, np.float32, 2), (0, np.float32, 1), (0, np.int16, 1)]


@pytest.mark.parametrize("win", [64, 1001])
@pytest.mark.parametrize("rate,dtype,channels", CASES, ids=["%d-%s-%d" % (r, np.dtype(d).name, c) for r, d, c in CASES])
def test_three_tracks_in_rounds(ctx, rate, dtype, channels, win):
    U, D, T = st._ratio(rate)
    n, per_tile = st._track_frames(rate)
    wavs = [st._signal(n + extra, channels, dtype, seed) for extra, seed in ((0, 1), (-101, 2), (57, 3))]
    wants = [st._whole(ctx, w, win, rate) for w in wavs]
    # a different chunk list per track: the supports' edges; the tile's edges; frame by frame through the head, then uneven pieces
    head = 2 * T + 3 * max(1, D // U) + 5
    lists = ([T // 2 - 1, 1, T // 2, 1, 1, T // 2 + 1, T - 1, 1, T, 1, 1, 1], [per_tile - 1, per_tile + 1, per_tile], [1] * head + [T + 2, per_tile // 3 + 1, 5])
    bounds = [st._cuts(len(w), sizes) for w, sizes in zip(wavs, lists)]
    run = Run(ctx, wavs, win, rate)
    _rounds(run, bounds, lambda k, live: live[::-1] if k % 2 else live)         # the assignment reversed every round
    run.finish(wants)
    assert max(c[0] for c in run.calls) == 3 and min(c[0] for c in run.calls) == 1


# ---- single rounds with mixed outcomes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [48000, 0])
def test_count_0_an_end_among_others_and_a_late_joiner(ctx, rate):
    win = 64
    n, per_tile = st._track_frames(rate)
    wavs = [st._signal(n - 13 * t, 2 if rate else 1, np.int16, 10 + t) for t in range(4)]
    wants = [st._whole(ctx, w, win, rate) for w in wavs]
    run = Run(ctx, wavs, win, rate)
    q = (n - 60) // 5                                                           # a fifth of a track: a few windows at either rate
    run.round([(0, q, 1), (1, q, 2), (2, q, 3)])
    # round 2: the middle track gives one frame and completes no window -- count 0 between tracks that do
    assert st._outputs(rate, q + 1) // win == st._outputs(rate, q) // win
    got = run.round([(0, q, 1), (1, 1, 2), (2, q, 3)])
    assert [len(g) > 0 for g in got] == [True, False, True]
    # round 3: a stream joins (slot 8), and track 0 ENDS here (0x10) while the others go on
    run.round([(3, q + 200, 8), (0, len(wavs[0]) - 2 * q, 1), (1, q - 50, 2), (2, q // 2, 3)])
    assert run.calls[-1][:2] == (4, 4) and run.calls[-1][5] == 1 and _slot_state(ctx, 1) == (0, 0, 0)
    run.round([(1, len(wavs[1]) - run.at[1], 2), (2, len(wavs[2]) - run.at[2], 3), (3, q, 8)])
    run.round([(3, len(wavs[3]) - run.at[3], 8)])
    assert run.calls[-1][5] == 0                                                 # the last track ends: nothing to save
    run.finish(wants)
    assert [_slot_state(ctx, k) for k in (1, 2, 3, 8)] == [(0, 0, 0)] * 4


def test_a_round_in_which_nothing_completes_a_window(ctx):
    rate, win = 48000, 1001
    wavs = [st._signal(9000, 2, np.int16, 20 + t) for t in range(2)]
    wants = [st._whole(ctx, w, win, rate) for w in wavs]
    run = Run(ctx, wavs, win, rate)
    run.round([(0, 40, 1), (1, 49, 2)])                                          # below T/2 frames: no output at all, nothing held, a history
    assert run.calls[-1] == (2, 2, 0, 0, 0, 1)
    run.round([(1, 300, 2), (0, 600, 1)])                                        # outputs, but no window yet
    assert run.calls[-1] == (2, 2, 0, 1, 0, 1)
    run.round([(0, 100, 1), (1, 100, 2)])                                        # held samples now: a gather
    assert run.calls[-1] == (2, 2, 1, 1, 0, 1)
    run.round([(0, 8260, 1), (1, 8551, 2)])                                      # both end: no save
    assert run.calls[-1] == (2, 2, 1, 1, 1, 0)
    run.finish(wants)


# ---- mapped against single-slot ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,dtype", [(44100, np.int16), (0, np.float32)])
def test_the_same_chunks_through_audio_slot(ctx, rate, dtype):
    win = 64
    n, per_tile = st._track_frames(rate)
    wavs = [st._signal(n - 7 * t, 1, dtype, 30 + t) for t in range(3)]
    run = Run(ctx, wavs, win, rate)
    bounds = [st._cuts(len(w), sizes) for w, sizes in zip(wavs, ([700, 45, 1300], [per_tile + 1, 46, 3], [999]))]
    k = 0
    while any(k + 1 < len(b) for b in bounds):
        live = [t for t, b in enumerate(bounds) if k + 1 < len(b)]
        got = run.round([(t, bounds[t][k + 1] - bounds[t][k], t + 1) for t in live])
        for t, rec in zip(live, got):
            a, b = bounds[t][k], bounds[t][k + 1]
            chunk = wavs[t][a:b] if rate else wavs[t][a:b, 0]
            one = ctx.audio_features(chunk, win, rate=rate or None, slot=t + 5, last=b == len(wavs[t]))
            assert st._bytes_equal(one, rec)
            assert _slot_state(ctx, t + 5) == _slot_state(ctx, t + 1)            # the same slot state after every round
        k += 1
    run.finish([st._whole(ctx, w, win, rate) for w in wavs])


def test_list_calls_and_single_slot_calls_alternate_on_one_slot(ctx):
    rate, win = 48000, 64
    wav, other = st._signal(9000, 2, np.int16, 40), st._signal(5000, 2, np.int16, 41)
    want, want_other = st._whole(ctx, wav, win, rate), st._whole(ctx, other, win, rate)
    recs, pcm = [], []
    got = ctx.audio_features_mapped([wav[:2000], other], [4, 0], [False, False], win, rate=rate)      # a list call (with a whole track beside it)
    recs.append(got[0].copy()); pcm.append(ctx.audio_pcm()[:st._outputs(rate, 2000)])
    assert st._bytes_equal(got[1], want_other[0])
    recs.append(ctx.audio_features(wav[2000:5045], win, rate=rate, slot=4).copy()); pcm.append(ctx.audio_pcm())       # a single-slot call
    got = ctx.audio_features_mapped([other[:1], wav[5045:7000]], [0, 4], [False, False], win, rate=rate)             # a list call
    recs.append(got[1].copy()); pcm.append(ctx.audio_pcm()[1:])
    recs.append(ctx.audio_features(wav[7000:], win, rate=rate, slot=4, last=True).copy()); pcm.append(ctx.audio_pcm())
    assert st._bytes_equal(np.concatenate(recs), want[0]) and np.array_equal(np.concatenate(pcm), want[1])


# ---- entry limits ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [48000, 0])
def test_8_continued_and_56_whole_tracks_in_one_call(ctx, rate):
    win = 64
    channels = 2 if rate else 1
    long = [st._signal(2400 + 31 * k, channels, np.int16, 50 + k) for k in range(8)]
    short = [st._signal(150 + 7 * k, channels, np.int16, 70 + k) for k in range(56)]
    arg = (lambda w: w) if rate else (lambda w: w[:, 0])
    want_long = [st._whole(ctx, w, win, rate)[0] for w in long]
    want_short = ctx.audio_features_many([arg(w) for w in short], win, rate=rate or None)
    want_short = [w.copy() for w in want_short]
    first = ctx.audio_features_mapped([arg(w[:1200]) for w in long], list(range(1, 9)), [False] * 8, win, rate=rate or None)
    # the continued tracks among the whole ones, at every eighth position
    chunks, slots, lasts, where = [], [], [], {}
    it = iter(short)
    for pos in range(64):
        if pos % 8 == 5:
            k = pos // 8
            where[pos] = k
            chunks.append(arg(long[k][1200:])); slots.append(k + 1); lasts.append(k % 2 == 0)
        else:
            chunks.append(arg(next(it))); slots.append(0); lasts.append(False)
    got = ctx.audio_features_mapped(chunks, slots, lasts, win, rate=rate or None)
    assert ctx.audio_map_call()[:2] == (64, 8)
    shorts = [g for pos, g in enumerate(got) if pos not in where]
    assert all(st._bytes_equal(g, w) for g, w in zip(shorts, want_short))
    for pos, k in where.items():
        rest = got[pos] if k % 2 == 0 else np.concatenate([got[pos], ctx.audio_features(arg(long[k][:0]), win, rate=rate or None, slot=k + 1, last=True)])
        assert st._bytes_equal(np.concatenate([first[k], rest]), want_long[k]), k


def test_the_option_and_its_limits(ctx):
    assert ctx.get_option("audio_track_slot") == 0
    for k in range(64):
        ctx.set_option("audio_track_slot", k + 1 if k < 8 else 0)
    assert ctx.get_option("audio_track_slot") == 64
    with pytest.raises(AvdError, match=": audio_track_slot: at most 64"):
        ctx.set_option("audio_track_slot", 0)
    assert ctx.get_option("audio_track_slot") == 64
    ctx.set_option("audio_track_slot", -1)
    assert ctx.get_option("audio_track_slot") == 0
    ctx.set_option("audio_track_slot", 3 | END)
    for bad, why in ((END, "0x10"), (3, "already in the list"), (3 | END, "already in the list"), (9, "slot 0 ... 8"), (0x20, "slot 0 ... 8"), (0x103, "slot 0 ... 8"), (-2, "slot 0 ... 8")):
        with pytest.raises(AvdError, match=": audio_track_slot:.*" + why):
            ctx.set_option("audio_track_slot", bad)
        assert ctx.get_option("audio_track_slot") == 1                           # the list as it was
    # the two ways of choosing slots never hold at once
    with pytest.raises(AvdError, match=": audio_slot: refused while"):
        ctx.set_option("audio_slot", 2)
    assert ctx.get_option("audio_slot") == 0
    ctx.set_option("audio_slot", 0)                                              # 0 is no selection: accepted
    ctx.set_option("audio_track_slot", -1)
    ctx.set_option("audio_slot", 2)
    with pytest.raises(AvdError, match=": audio_track_slot: refused while"):
        ctx.set_option("audio_track_slot", 0)
    ctx.set_option("audio_track_slot", -1)                                       # clearing is always accepted
    assert ctx.get_option("audio_track_slot") == 0
    ctx.set_option("audio_slot", 0)


@pytest.mark.parametrize("rate,dtype", [(0, np.float32), (0, np.int16), (44100, np.int16)])
def test_a_list_of_zeros_is_the_plain_cut_call(ctx, rate, dtype):
    win = 1001
    tracks = [st._signal(n, 1, dtype, 80 + n % 7)[:, 0] for n in (3000, 1001, 17, 2002, 1500)]
    want = [w.copy() for w in ctx.audio_features_many(tracks, win, rate=rate or None)]
    plain = (ctx.audio_plan(), ctx.audio_tracks().copy(), ctx.audio_xw().copy(), ctx.audio_mag().copy(), ctx.audio_pcm().copy() if rate else None)
    got = ctx.audio_features_mapped(tracks, [0] * 5, [False] * 5, win, rate=rate or None)
    assert all(st._bytes_equal(g, w) for g, w in zip(got, want))
    assert ctx.audio_plan() == plain[0] and np.array_equal(ctx.audio_tracks(), plain[1])
    # only the windows' own entries are defined: a short last window fills its first `last` entries of a row
    lens = [min(win, m - k * win) for m in (st._outputs(rate, len(t), True) for t in tracks) for k in range(-(-m // win))]
    xw, mag = ctx.audio_xw(), ctx.audio_mag()
    for w, L in enumerate(lens):
        assert np.array_equal(xw[w, :L].view(np.uint64), plain[2][w, :L].view(np.uint64)) and np.array_equal(mag[w, :L // 2 + 1].view(np.uint64), plain[3][w, :L // 2 + 1].view(np.uint64))
    if rate:
        assert np.array_equal(ctx.audio_pcm(), plain[4])
    assert ctx.audio_map_call() == (5, 0, int(not rate), int(bool(rate)), 1, 0)


# ---- alignment ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("rate,dtype,channels", [(48000, np.int16, 2), (48000, np.float32, 1), (0, np.int16, 1), (0, np.float32, 1)],
                         ids=["48000-int16-stereo", "48000-float32-mono", "0-int16", "0-float32"])
def test_track_starts_at_every_offset_mod_16_bytes(ctx, device, rate, dtype, channels):
    win = 64
    size = np.dtype(dtype).itemsize * channels                                   # bytes per frame
    per_line = 16 // size
    # lengths of whole lines + 1 frame: track k of a call begins k frames into its line.  Odd lengths put the cuts at odd positions
    nt = min(per_line + 1, 8)                                                   # (eight slots: int16 mono has its eight residues in eight tracks)
    wavs = [st._signal(1800 + 40 * k, channels, dtype, 90 + k) for k in range(nt)]
    wants = [st._whole(ctx, w, win, rate) for w in wavs]
    run = Run(ctx, wavs, win, rate, device=device)
    firsts = [per_line * (100 + 3 * k) + 1 for k in range(nt)]
    assert {sum(firsts[:k]) * size % 16 for k in range(nt)} == set(range(0, 16, size))
    run.round([(k, firsts[k], k + 1) for k in range(nt)])
    seconds = [per_line * (50 + k) + 3 for k in range(nt)]                       # held samples in front now: other residues on the destination's side
    run.round([(k, seconds[k], k + 1) for k in range(nt)][::-1])
    run.round([(k, len(wavs[k]) - run.at[k], k + 1) for k in range(nt)])
    run.finish(wants)


def test_a_buffer_that_begins_anywhere(ctx):
    """the C-ABI with the call's buffer itself at every 2-byte residue of a 16-byte line (int16 mono, unconverted and converted)"""
    win = 64
    for rate in (0, 48000):
        a, b = st._signal(700, 1, np.int16, 110)[:, 0], st._signal(901, 1, np.int16, 111)[:, 0]
        want = [w.copy() for w in ctx.audio_features_many([a, b], win, rate=rate or None)]
        room = np.zeros(len(a) + len(b) + 16, np.int16)
        base = ((-room.ctypes.data) % 16) // 2
        for shift in range(8):
            flat = room[base + shift:base + shift + len(a) + len(b)]
            flat[:len(a)], flat[len(a):] = a, b
            assert flat.ctypes.data % 16 == 2 * shift
            rc, out, why = _raw(ctx, flat, len(flat), win, 64, rate, 1, 1, entries=(0, 0), cuts=(len(a),))
            assert rc == 0, why
            assert st._bytes_equal(out[:len(want[0]) + len(want[1])], np.concatenate(want))


# ---- win 8000 ----------------------------------------------------------------------------------------------------------------------------------------
def test_three_tracks_take_the_80_by_100_transform(ctx):
    rate, win = 48000, 8000
    wavs = [st._signal(3 * 48000 - 500 * t, 2, np.int16, 120 + t) for t in range(3)]
    wants = [st._whole(ctx, w, win, rate) for w in wavs]
    run = Run(ctx, wavs, win, rate)
    for k in range(3):
        run.round([(t, min(48000, len(wavs[t]) - run.at[t]), t + 1) for t in ((0, 1, 2), (2, 0, 1), (1, 2, 0))[k]])
        assert ctx.audio_plan()[3] >= 3                                          # full windows of every track on the 80 x 100 path
    run.finish(wants)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
def _raw(c, wav, n, win, max_windows, rate, channels, fmt, entries=(), cuts=(), end=False, ptr=None, null_windows=False):
    """a call of the C-ABI as a caller of it makes it: the options set, the call, the options back -> (status, records, the error text)"""
    out = np.zeros(max(max_windows, 1), AUDIO_WINDOW_DTYPE)
    c.set_option("audio_rate", rate)
    c.set_option("audio_channels", channels)
    c.set_option("audio_format", fmt)
    try:
        for cut in cuts:
            c.set_option("audio_cut", cut)
        for e in entries:
            c.set_option("audio_track_slot", e)
        if end:
            c.set_option("audio_end", 1)
        rc = c._L.avd_audio_features(c._h, ctypes.c_void_p(wav.ctypes.data if ptr is None else ptr), AVD_MEM_HOST, n, win,
                                     None if null_windows else ctypes.c_void_p(out.ctypes.data), max_windows)
        assert (c.get_option("audio_track_slot"), c.get_option("audio_cut"), c.get_option("audio_end")) == (0, 0, 0)    # consumed, whatever became of the call
    finally:
        c.set_option("audio_rate", 0)
        c.set_option("audio_channels", 1)
        c.set_option("audio_format", 0)
    why = ""
    if rc != 0:
        try:
            c._check(rc)
        except AvdError as e:
            why = str(e)
    return rc, out[:max_windows], why


def test_every_refusal_in_its_order_leaves_every_slot_untouched(ctx):
    rate, win = 48000, 64
    wavs = [st._signal(9000 - 100 * t, 2, np.int16, 130 + t) for t in range(2)]
    wants = [st._whole(ctx, w, win, rate) for w in wavs]
    run = Run(ctx, wavs, win, rate)
    run.round([(0, 4000, 5), (1, 3000, 6)])
    before = [_slot_state(ctx, k) for k in range(1, 9)]
    rest = [np.ascontiguousarray(wavs[0][4000:6000]), np.ascontiguousarray(wavs[1][3000:6000])]
    flat = np.concatenate([r.reshape(-1) for r in rest])
    n, cut = 5000, 2000
    need = sum((st._outputs(rate, a) % win + st._outputs(rate, b) - st._outputs(rate, a)) // win for a, b in ((4000, 6000), (3000, 6000)))
    # slot 7 is bound to another window length by a call of its own
    ctx.audio_features(wavs[0][:500], 1001, rate=rate, slot=7)
    before[6] = _slot_state(ctx, 7)
    good = dict(n=n, win=win, max_windows=need, rate=rate, channels=2, fmt=1, entries=(5, 6), cuts=(cut,))
    refusals = [
        # in the documented order: each call has later faults as well, and is refused for the earliest
        (dict(win=9000, ptr=flat.ctypes.data + 1, cuts=(n,), end=True, entries=(5, 6, 7), max_windows=0), "audio window"),
        (dict(ptr=flat.ctypes.data + 1, cuts=(n,), end=True, entries=(5, 6, 7), max_windows=0), "2-byte aligned"),
        (dict(cuts=(n,), end=True, entries=(5, 6, 7), max_windows=0), "audio_cut: beyond the buffer"),
        (dict(end=True, entries=(5, 6, 7), max_windows=0), "audio_track_slot: ends are given in the list"),
        (dict(entries=(5, 6, 7), max_windows=0), "audio_track_slot: the list needs one entry per track"),
        (dict(entries=(5, 7), max_windows=0), "audio_track_slot: win,"),
        (dict(n=3 * 2 ** 31, max_windows=0), "audio_track_slot: more than 2^31 - 1 output samples"),
        (dict(max_windows=need - 1), "audio_track_slot: windows array too small"),
        (dict(null_windows=True), "audio_track_slot: windows array too small"),
    ]
    for how, why in refusals:
        args = dict(good)
        args.update(how)
        rc, out, text = _raw(ctx, flat, **args)
        assert rc != 0 and why in text, (how, rc, text)
        assert not out.view(np.uint8).any()
        assert [_slot_state(ctx, k) for k in range(1, 9)] == before, how
    # float32 samples need 4 bytes at every rate
    f32 = np.zeros(64, np.float32)
    rc, out, text = _raw(ctx, f32, 10, win, 4, 0, 1, 0, entries=(1,), ptr=f32.ctypes.data + 2)
    assert rc != 0 and "audio_track_slot: float32 samples need a 4-byte aligned wav" in text
    # the refused calls consumed their lists: this call has none and is a plain whole-track call
    rc, out, text = _raw(ctx, flat, 500, win, 8, rate, 2, 1)
    assert rc == 0 and [_slot_state(ctx, k) for k in range(1, 9)] == before
    # ... and the tracks go on to the referee's bytes, first through the very call that was refused
    rc, out, text = _raw(ctx, flat, **good)
    assert rc == 0, text
    k0 = (st._outputs(rate, 4000) % win + st._outputs(rate, 6000) - st._outputs(rate, 4000)) // win
    run.recs[0].append(out[:k0].copy()); run.recs[1].append(out[k0:need].copy())
    new = ctx.audio_pcm()
    f0 = st._outputs(rate, 6000) - st._outputs(rate, 4000)
    run.pcm[0].append(new[:f0]); run.pcm[1].append(new[f0:])
    run.at = [6000, 6000]
    run.round([(1, len(wavs[1]) - 6000, 6), (0, len(wavs[0]) - 6000, 5)])
    run.finish(wants)


# ---- across other work --------------------------------------------------------------------------------------------------------------------------------
def test_rounds_across_everything_else_on_the_context(ctx):
    rate, win = 44100, 64
    wavs = [st._signal(12000 - 300 * t, 2, np.int16, 140 + t) for t in range(3)]
    wants = [st._whole(ctx, w, win, rate) for w in wavs]
    other = st._signal(5000, 1, np.float32, 145)
    frames = np.random.default_rng(146).integers(0, 255, (3, 240, 320, 3), dtype=np.uint8)
    run = Run(ctx, wavs, win, rate)
    go = lambda n, order=(0, 1, 2): run.round([(t, n + 11 * t, t + 1) for t in order])      # noqa: E731
    go(2000)
    ctx.release_workspace()                                                     # the scratch goes, the slots stay
    go(45, (2, 1, 0))
    slot0 = ctx.audio_features(other, 8000, rate=48000).copy()                   # a slot-0 converted call at another rate: another bank, unaffected by the slots
    many = [m.copy() for m in ctx.audio_features_many([other[:, 0], other[:3000, 0]], 1001)]
    go(3000)
    ctx.analyze_frames(frames)                                                   # video
    ctx.set_option("stream_reset", 0)
    go(2500, (1, 0, 2))
    rec_async = np.zeros(len(frames), avd_hip.RECORD_DTYPE)
    keep = ctx.analyze_frames_async(frames, rec_async)                           # a pending asynchronous analysis: drained first
    go(1000)
    ctx.synchronize()
    del keep
    assert rec_async.view(np.uint8).any()
    run.round([(t, len(wavs[t]) - run.at[t], t + 1) for t in (0, 1, 2)])
    run.finish(wants)
    with avd_hip.Context(0) as fresh:                                            # what a context that never saw a slot gives for the slot-0 calls
        assert st._bytes_equal(fresh.audio_features(other, 8000, rate=48000), slot0)
        assert all(st._bytes_equal(a, b) for a, b in zip(fresh.audio_features_many([other[:, 0], other[:3000, 0]], 1001), many))


# ---- the helpers ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_stream_helpers_equal_their_whole_track_forms(ctx):
    pieces = lambda a, size: (a[i:i + size] for i in range(0, len(a), size))    # noqa: E731
    wavs = [st._signal(n, 2, np.int16, 150 + n % 5) for n in (48000 + 77, 30000, 40001)]
    want = [host_audio.analyze_decoded(w, 48000, ctx) for w in wavs]
    assert host_audio.analyze_decoded_streams([pieces(w, 4096) for w in wavs], 48000, ctx) == want
    assert host_audio.analyze_decoded_streams([pieces(wavs[0], 1024), iter([wavs[1]]), pieces(wavs[2], 9999)], 48000, ctx) == want
    assert [_slot_state(ctx, k) for k in (1, 2, 3)] == [(0, 0, 0)] * 3 and ctx.get_option("audio_slot") == 0
    ready = [st.ref.convert(w, 48000) for w in wavs]
    assert host_audio.analyze_wave_streams([pieces(r, 5000) for r in ready], 16000, ctx) == [host_audio.analyze_wave(r, 16000, ctx) for r in ready]
    f32 = [(r.astype(np.float32) / np.float32(32768.0)) for r in ready[:2]]
    assert host_audio.analyze_wave_streams([pieces(f32[0], 8000), pieces(f32[1], 3001)], 16000, ctx) == [host_audio.analyze_wave(f, 16000, ctx) for f in f32]
    # a stream that gives nothing is the empty track; one that breaks leaves no half track behind
    assert host_audio.analyze_wave_streams([iter([]), pieces(f32[1], 3001)], 16000, ctx)[1] == host_audio.analyze_wave(f32[1], 16000, ctx)

    def broken():
        yield wavs[0][:5000]
        yield wavs[0][5000:9000]
        raise OSError("the decoder gave up")
    with pytest.raises(OSError):
        host_audio.analyze_decoded_streams([pieces(wavs[1], 4096), broken()], 48000, ctx)
    assert [_slot_state(ctx, k) for k in (1, 2)] == [(0, 0, 0)] * 2 and ctx.get_option("audio_track_slot") == 0


def test_device_chunks(ctx):
    rate, win = 48000, 64
    n, _ = st._track_frames(rate)
    for dtype, channels, r in ((np.int16, 2, rate), (np.float32, 1, rate), (np.float32, 1, 0)):
        wavs = [st._signal(n - 9 * t, channels, dtype, 160 + t) for t in range(2)]
        run = Run(ctx, wavs, win, r, device=True)
        run.round([(0, 1111, 2), (1, 1501, 1)])
        run.round([(1, len(wavs[1]) - 1501, 1), (0, len(wavs[0]) - 1111, 2)])
        run.finish([st._whole(ctx, w, win, r) for w in wavs])
    assert AVD_MEM_DEVICE != AVD_MEM_HOST
