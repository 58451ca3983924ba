"""A track continued across avd_audio_features calls (options "audio_slot", "audio_end", "audio_slot_reset" and the read-only three,
include/avd.h), without a GPU.

  * the header's text: the options, the rule, no new export;
  * M(N) and W of the rule, as csrc/avd_audio_stream.h computes them, against a brute-force count of the outputs whose support lies in [0, N),
    taken with tests/audio_resample_reference.py's ratios: every rate, N = 0 ... 3 T and around 2^31 / D;
  * plan_continue through tests/audio_stream_check.cpp, a stand-alone program built with AddressSanitizer and UBSan by tests/audio_stream_kit.py
    and RUN AS A PROGRAM: every rate, chunks of 1, T/2 - 1, T/2, T/2 + 1, T - 1, T and one tile's frames +- 1; its tiles, concatenated, are
    plan_convert's coverage of the whole track (checked there output by output, and here against audio_resample_kit's plan); two mutated
    planners (the T/2 hold-back dropped, the history one frame short) must be rejected by it;
  * Context.audio_features(slot=, last=) and avd_hip.audio.analyze_*_chunks against a context that only records.

Every comparison here is between integers: equality throughout, no tolerance."""
import os
import re

import numpy as np
import pytest

from avd_hip import _lib
from avd_hip import audio as host_audio
from tests import audio_resample_kit as rs_kit
from tests import audio_resample_reference as ref
from tests import audio_stream_kit as kit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS = ('"audio_slot"', '"audio_end"', '"audio_slot_reset"', '"audio_slot_frames"', '"audio_slot_held"', '"audio_slot_windows"')


def ratio(rate):
    return ref.ratio(rate) if rate else (1, 1, 0)


def count_outputs(rate, n):
    """outputs m >= 0 whose last tap floor(m D / U) + T/2 lies at or below frame n - 1, counted one by one"""
    U, D, T = ratio(rate)
    m = 0
    while (m * D) // U + T // 2 <= n - 1:
        m += 1
    return m


def rule_outputs(rate, n, last=False):
    """the rule's closed form (the tests below hold it to the count): what the recording library goes by, at any n"""
    U, D, T = ratio(rate)
    return -(-(n if last else max(0, n - T // 2)) * U // D)


# ---- the header's text ---------------------------------------------------------------------------------------------------------------------
def test_header_documents_the_options_and_the_rule():
    text = open(os.path.join(ROOT, "include", "avd.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for name in OPTIONS:
        assert name in flat, name
    assert "M(N) = ceil(max(0, N - T/2) U / D)" in flat and "W = floor(M / win)" in flat and "min(N, T - 1)" in flat
    assert "byte for byte the records of ONE slot-0 call" in flat
    assert flat.count('begins "audio_slot:"') >= 2 and "survives avd_release_workspace" in flat
    # no function is added
    assert re.search(r"#define\s+AVD_ABI_VERSION\s+3\b", text) and len(_lib.EXPORTS) == 43
    assert "audio_slot" not in " ".join(_lib.EXPORTS)
    capi = open(os.path.join(ROOT, "ai-video-detector_amd", "csrc", "avd_capi.hip")).read()
    for name in OPTIONS:
        assert '{%s,' % name in capi, name
    for doc, what in (("README.md", "audio_slot"), ("DESIGN.md", "7.3"), ("INTEGRATION.md", "analyze_decoded_chunks")):
        assert what in open(os.path.join(ROOT, doc)).read(), doc


def test_the_plan_header_is_plain_host_code():
    text = open(kit.HEADER).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes == ['"avd_audio_resample.h"']


# ---- M(N) and W ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", (0,) + ref.RATES)
def test_outputs_after_equals_the_brute_force_count(rate):
    U, D, T = ratio(rate)
    # every N = 0 ... 3 T (and a little beyond where T = 0) in-process: the closed forms against the count ...
    for n in range(0, 3 * T + 41):
        assert rule_outputs(rate, n) == count_outputs(rate, n) == _lib.Context.audio_outputs_after(n, rate), (rate, n)
        assert _lib.Context.audio_outputs_after(n, rate, True) == rule_outputs(rate, n, True) == (ref.n_out(n, rate) if rate else n), (rate, n)
    # ... and the header, a process per value, at a sample of them with every edge
    for n in list(range(0, 3 * T + 1, max(1, T // 25))) + [T // 2 - 1, T // 2, T // 2 + 1, T - 1, T, 3 * T]:
        if n < 0:
            continue
        want = count_outputs(rate, n)
        assert kit.outputs_after(rate, n) == want == rule_outputs(rate, n) == _lib.Context.audio_outputs_after(n, rate), (rate, n)
        assert kit.outputs_after(rate, n, last=True) == (ref.n_out(n, rate) if rate else n) == _lib.Context.audio_outputs_after(n, rate, True)


@pytest.mark.parametrize("rate", ref.RATES)
def test_outputs_after_around_two_to_the_31_over_d(rate):
    U, D, T = ratio(rate)
    for n in ((2 ** 31) // D - 1, (2 ** 31) // D, (2 ** 31) // D + 1):
        got = kit.outputs_after(rate, n)
        if got > 2 ** 31 - 1:
            continue
        # got is the count: output got - 1 has its support in [0, n), output got does not
        assert got == 0 or ((got - 1) * D) // U + T // 2 <= n - 1
        assert (got * D) // U + T // 2 > n - 1
        assert got == _lib.Context.audio_outputs_after(n, rate)


@pytest.mark.parametrize("rate", (0, 16000, 44100, 192000, 11025))
def test_windows_and_held_follow_the_rule(rate):
    U, D, T = ratio(rate)
    for win in (1, 64, 1001):
        before = 0
        for n, last in ((T // 2, False), (1, False), (700, False), (0, False), (5000, False), (3, True)):
            p = kit.plan(rate, win, before, n, last)
            m0 = count_outputs(rate, before)
            m1 = -(-(before + n) * U // D) if last else count_outputs(rate, before + n)
            assert (p["m_before"], p["m_after"]) == (m0, m1)
            w0, w1 = m0 // win, (-(-m1 // win) if last else m1 // win)
            assert p["windows"] == w1 - w0 and p["held_before"] == m0 - w0 * win
            assert p["held_after"] == (0 if last else m1 - w1 * win) and p["held_after"] < win
            assert p["hist_before"] == min(before, max(T - 1, 0)) and p["hist_after"] == (0 if last else min(before + n, max(T - 1, 0)))
            before += n


# ---- plan_continue, through the sanitized program ----------------------------------------------------------------------------------------------
def test_every_check_of_the_program():
    status, out = kit.run()
    assert status == 0 and re.fullmatch(r"audio stream: \d+ calls checked, 0 failures\n", out), (status, out)
    assert int(out.split()[2]) > 20000


def test_a_dropped_hold_back_is_rejected():
    status, out = kit.run(mutated="no_holdback")
    assert status == 1 and "FAIL" in out and "has not arrived" in out and not re.search(r", 0 failures", out), (status, out)
    # a track that is not filtered has nothing to hold back: the mutation shows only where T > 0
    assert kit.plan(16000, 64, 0, 1000, mutated="no_holdback") == kit.plan(16000, 64, 0, 1000)
    assert kit.plan(48000, 64, 0, 3000, mutated="no_holdback")["m_after"] == 1000 and kit.plan(48000, 64, 0, 3000)["m_after"] == 984


def test_a_history_one_frame_short_is_rejected():
    status, out = kit.run(mutated="short_history")
    assert status == 1 and "FAIL" in out and "the history begins at" in out and not re.search(r", 0 failures", out), (status, out)
    assert kit.plan(48000, 64, 3000, 10, mutated="short_history")["hist_before"] == 98 and kit.plan(48000, 64, 3000, 10)["hist_before"] == 99


@pytest.mark.parametrize("rate", ref.RATES)
def test_the_tiles_of_the_calls_cover_what_plan_convert_covers(rate):
    U, D, T, tile_out, _ = rs_kit.taps(rate)
    per_tile = tile_out * D // U
    total = per_tile + 3 * T + 11                              # two tiles of the whole track; every call below is a process of its own
    whole = rs_kit.plan(rate, total)
    want = [(m, (m * D) // U - (T // 2 - 1 if T else 0), (m * D) % U) for m in range(whole["n_out"])]     # per output: first frame of its support, phase
    assert [(t[1], t[0], t[3]) for t in whole["tiles"]] == [want[m] for m in range(0, whole["n_out"], tile_out)]
    for chunk in ((T // 2 + 1, T, per_tile - 1, per_tile + 1) if T else (37, per_tile - 1, per_tile + 1)):
        got, before = [], 0
        while before < total:
            n = min(chunk, total - before)
            p = kit.plan(rate, 64, before, n, before + n == total)
            assert p["refused"] == 0 and p["ntiles"] == len(p["tiles"])
            at = p["m_before"]
            for in0, out0, count, phase in p["tiles"]:
                assert out0 == p["held_before"] + at - p["m_before"] and 1 <= count <= tile_out
                got += [(at + j, in0 + (phase + j * D) // U, (phase + j * D) % U) for j in range(count)]
                at += count
            assert at == p["m_after"]
            before += n
        assert got == want, (rate, chunk)


# ---- the Python helpers against a recording context ---------------------------------------------------------------------------------------------
class _FakeLibrary:
    def __init__(self, owner):
        self.owner = owner

    def avd_audio_features(self, h, ptr, mem, n, win, out_ptr, nwin):
        o = self.owner
        slot, last = o.options["audio_slot"], bool(o.options["audio_end"])
        o.options["audio_end"] = 0
        o.calls.append({"ptr": ptr, "n": n, "win": win, "nwin": nwin, "slot": slot, "last": last, "rate": o.options["audio_rate"],
                        "channels": o.options["audio_channels"], "format": o.options["audio_format"]})
        if o.fail_call == len(o.calls):
            return -1
        if slot:                                                       # the rule, restated: what the library would do to the slot
            rate = o.options["audio_rate"]
            U, D, T = ratio(rate)
            frames = o.frames.get(slot, 0)
            m0, m1 = rule_outputs(rate, frames), rule_outputs(rate, frames + n, last)
            wrote = (-(-m1 // win) if last else m1 // win) - m0 // win
            assert nwin >= wrote, ("the record array is too small", nwin, wrote)
            o.calls[-1]["wrote"] = wrote
            o.frames[slot] = 0 if last else frames + n
            o.held[slot] = 0 if last else m1 % win
            if wrote:
                rec = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_uint8 * (48 * nwin)).from_address(out_ptr)).view(_lib.AUDIO_WINDOW_DTYPE)
                rec["length"][:wrote] = win
                rec["nbins"][:wrote] = np.arange(m0 // win, m0 // win + wrote)      # the window's number in the track
        return 0


class Recorder(_lib.Context):
    """a Context without a library: what the audio helpers do above the C-ABI, call by call"""

    def __init__(self, fail_call=0, **options):
        self._h = None
        self.device = 0
        self.calls, self.sets, self.frames, self.held = [], [], {}, {}
        self.options = {"audio_format": 0, "audio_rate": 0, "audio_channels": 1, "audio_slot": 0, "audio_end": 0, **options}
        self.fail_call = fail_call
        self._L = _FakeLibrary(self)

    def _check(self, rc):
        if rc != 0:
            raise _lib.AvdError("avd status %d" % rc)

    def set_option(self, name, value):
        self.sets.append((name, value))
        if name == "audio_slot" and not 0 <= value <= 8:
            raise _lib.AvdError("audio_slot: refused")
        if name == "audio_slot_reset":
            for k in range(1, 9):
                if value in (0, k):
                    self.frames[k] = self.held[k] = 0
        else:
            self.options[name] = value

    def get_option(self, name):
        slot = self.options["audio_slot"]
        if name == "audio_slot_frames":
            return min(self.frames.get(slot, 0), 2 ** 31 - 1)
        if name == "audio_slot_held":
            return self.held.get(slot, 0)
        return self.options[name]


def test_features_with_a_slot_sizes_from_the_rule_and_restores():
    r = Recorder(audio_slot=3)
    sizes = []
    for n, last in ((40, False), (1, False), (1000, False), (0, False), (2000, False), (7, True)):
        out = r.audio_features(np.zeros((n, 2), np.int16), 64, rate=48000, slot=5, last=last)
        sizes.append(len(out))
        assert r.calls[-1]["nwin"] == r.calls[-1]["wrote"] == len(out)               # exactly the rule's count, not a bound
        assert (r.calls[-1]["slot"], r.calls[-1]["last"], r.calls[-1]["rate"], r.calls[-1]["channels"], r.calls[-1]["format"]) == (5, last, 48000, 2, 1)
        assert r.options["audio_slot"] == 3 and r.options["audio_end"] == 0 and r.options["audio_rate"] == 0
    assert sum(sizes) == -(-ref.n_out(3048, 48000) // 64) and sizes[0] == sizes[1] == 0
    # an unconverted track, float32
    r = Recorder()
    assert [len(r.audio_features(np.zeros(n, np.float32), 10, slot=1, last=l)) for n, l in ((25, False), (4, False), (1, False), (3, True))] == [2, 0, 1, 1]
    assert [c["rate"] for c in r.calls] == [0] * 4 and r.options["audio_slot"] == 0
    # slot 0: the option is not touched at all
    r = Recorder()
    r.audio_features(np.zeros(9, np.float32), 4)
    assert r.sets == [] and r.calls[0]["nwin"] == 3


def test_a_saturated_slot_is_sized_by_a_bound_and_trimmed():
    r = Recorder()
    r.frames[2] = 2 ** 31 + 5
    out = r.audio_features(np.zeros(6400, np.int16), 64, rate=16000, slot=2)
    assert r.calls[0]["nwin"] > r.calls[0]["wrote"] == len(out) and len(out) in (100, 101)


def test_the_slot_option_comes_back_after_an_exception():
    r = Recorder(fail_call=1, audio_slot=2, audio_rate=44100)
    with pytest.raises(_lib.AvdError):
        r.audio_features(np.zeros(30, np.int16), 4, rate=48000, slot=7, last=True)
    assert r.calls[0]["slot"] == 7 and r.calls[0]["last"]
    assert (r.options["audio_slot"], r.options["audio_rate"], r.options["audio_format"]) == (2, 44100, 0)
    r = Recorder(audio_slot=2)
    with pytest.raises(_lib.AvdError, match="audio_slot"):
        r.audio_features(np.zeros(30, np.int16), 4, slot=9)
    assert r.calls == [] and r.options["audio_slot"] == 2


class ChunkRecorder:
    """what the chunked helpers hand to Context.audio_features, chunk by chunk"""

    def __init__(self, fail_at=0):
        self.calls, self.sets, self.fail_at = [], [], fail_at

    def set_option(self, name, value):
        self.sets.append((name, value))

    def audio_converted_length(self, n, rate):
        return _lib.Context.audio_converted_length(n, rate)

    def audio_features(self, wav, win, rate=None, slot=0, last=False):
        self.calls.append({"id": id(wav), "first": None if not len(wav) else np.asarray(wav).reshape(len(wav), -1)[0, 0], "n": len(wav), "shape": wav.shape,
                           "dtype": wav.dtype, "win": win, "rate": rate, "slot": slot, "last": last})
        if self.fail_at == len(self.calls):
            raise _lib.AvdError("failed")
        rec = np.zeros(1, _lib.AUDIO_WINDOW_DTYPE)
        rec["length"], rec["nbins"], rec["sum_mag"], rec["sumsq"] = win, win // 2 + 1, 1.0, 1.0
        return rec


def _numbered_chunks(sizes, channels, dtype):
    at = 0
    for n in sizes:
        a = np.zeros((n, channels), dtype)
        a[:, 0] = np.arange(at, at + n) % 30000
        at += n
        yield a


def test_the_chunked_helpers_pass_every_chunk_once_and_mark_only_the_last():
    sizes = [4096, 4096, 1, 4096, 100]
    r = ChunkRecorder()
    got = host_audio.analyze_decoded_chunks(_numbered_chunks(sizes, 2, np.int16), 48000, r, slot=4)
    assert [c["n"] for c in r.calls] == sizes and [c["last"] for c in r.calls] == [False] * 4 + [True]
    assert [c["first"] for c in r.calls] == [0, 4096, 8192, 8193, 12289]                  # every chunk once, in order
    assert {(c["slot"], c["rate"], c["win"], c["dtype"], c["shape"][1]) for c in r.calls} == {(4, 48000, 8000, np.dtype(np.int16), 2)}
    assert r.sets == [("audio_slot_reset", 4)]
    assert len(got["timeline"]) == max(1, round(ref.n_out(sum(sizes), 48000) / 16000))
    r = ChunkRecorder()
    host_audio.analyze_wave_chunks(_numbered_chunks(sizes, 2, np.float32), 16000, r)
    assert [c["n"] for c in r.calls] == sizes and [c["last"] for c in r.calls] == [False] * 4 + [True]
    assert {(c["slot"], c["rate"], c["win"], c["dtype"], len(c["shape"])) for c in r.calls} == {(1, None, 8000, np.dtype(np.float32), 1)}       # the first channel
    # one chunk: it is the last
    r = ChunkRecorder()
    host_audio.analyze_decoded_chunks(_numbered_chunks([77], 1, np.int16), 44100, r)
    assert [(c["n"], c["last"]) for c in r.calls] == [(77, True)]


def test_the_chunked_helpers_empty_the_slot_after_an_exception():
    r = ChunkRecorder(fail_at=2)
    with pytest.raises(_lib.AvdError):
        host_audio.analyze_decoded_chunks(_numbered_chunks([10, 10, 10, 10], 1, np.int16), 48000, r, slot=2)
    assert len(r.calls) == 2 and r.sets == [("audio_slot_reset", 2), ("audio_slot_reset", 2)]

    def broken():
        yield np.zeros((5, 1), np.int16)
        raise OSError("the decoder gave up")
    r = ChunkRecorder()
    with pytest.raises(OSError):
        host_audio.analyze_decoded_chunks(broken(), 48000, r, slot=2)
    assert r.calls == [] and r.sets[-1] == ("audio_slot_reset", 2)


def test_read_wav_chunks_reads_the_file_in_pieces(tmp_path):
    import wave
    frames = (np.arange(2 * 1000).reshape(1000, 2) % 2000 - 1000).astype("<i2")
    path = str(tmp_path / "t.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(44100)
        w.writeframes(frames.tobytes())
    pieces = list(host_audio.read_wav_chunks(path, 300))
    assert [len(p) for p in pieces] == [300, 300, 300, 100] and all(p.dtype == np.int16 and p.shape[1] == 2 for p in pieces)
    assert np.array_equal(np.concatenate(pieces), host_audio.read_wav_frames(path)[0])
    assert host_audio.wav_info(path) == (2, 2, 44100, 1000)
