"""Several continued tracks in one avd_audio_features call (option "audio_track_slot", include/avd.h), without a GPU.

  * the header's text: the option, its refusals in their order, the guarantee, the debug buffers; no new export;
  * csrc/avd_audio_map.h through tests/audio_map_check.cpp, a stand-alone program built with AddressSanitizer and UBSan by tests/audio_map_kit.py
    and RUN AS A PROGRAM: calls of 1 ... 4 tracks at every rate, win 64 / 1001 / 8000, slots empty, with a short and a full history, with nothing
    and with win - 1 samples held, chunks of 1, T/2 +- 1, T - 1, T and a tile's frames +- 1, tracks whole, continued and ended -- regions apart and
    [held | new], every window inside the analysed part of one region, every tile with its own track's source row, every track's Continue
    plan_continue's, record counts summing to the plan's total, the refusals in their order; two mutated planners (a track's windows running over
    its held remainder into the next region; a track handed its neighbour's history) must be rejected by it;
  * single plans of the header against the rule restated here;
  * Context.audio_features_mapped and avd_hip.audio.analyze_*_streams against a context that only records.

Every comparison here is between integers: equality throughout, no tolerance."""
import os
import re

import numpy as np
import pytest

from avd_hip import _lib
from avd_hip import audio as host_audio
from tests import audio_map_kit as kit
from tests import audio_resample_reference as ref
from tests.test_audio_stream_host import Recorder, _FakeLibrary, _numbered_chunks, ratio, rule_outputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFUSALS = ('"audio_cut: beyond the buffer"', "ends are given in the list", "other than cuts + 1", "other than at its first call", "2^31 - 1 outputs", "max_windows below the sum")


# ---- the header's text ---------------------------------------------------------------------------------------------------------------------
def test_header_documents_the_option_and_its_refusal_order():
    text = open(os.path.join(ROOT, "include", "avd.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    assert '"audio_track_slot"' in flat and '"audio_map_call"' in flat and 'begins "audio_track_slot:"' in flat
    at = [flat.index(r, flat.index("Refusals of a list call")) for r in REFUSALS]
    assert at == sorted(at), at                                 # the order the checks come in
    assert "one filter bank per call" in flat and "byte for byte those of ONE slot-0 call on its joined samples" in flat
    assert "a list of zeros" in flat and "never hold at once" in flat
    # no function is added
    assert re.search(r"#define\s+AVD_ABI_VERSION\s+3\b", text) and len(_lib.EXPORTS) == 43
    assert "track_slot" not in " ".join(_lib.EXPORTS) and "audio_map" not in " ".join(_lib.EXPORTS)
    capi = open(os.path.join(ROOT, "ai-video-detector_amd", "csrc", "avd_capi.hip")).read()
    assert '{"audio_track_slot",' in capi
    for doc, what in (("README.md", "audio_track_slot"), ("DESIGN.md", "7.4"), ("INTEGRATION.md", "analyze_decoded_streams")):
        assert what in open(os.path.join(ROOT, doc)).read(), doc


def test_the_plan_header_is_plain_host_code():
    text = open(kit.HEADER).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes == ["<algorithm>", "<cstddef>", "<vector>", '"avd_audio_plan.h"', '"avd_audio_resample.h"', '"avd_audio_stream.h"']
    # the three audio headers are as they were: the tile is 40 bytes, and the tables this path adds stand beside it
    resample = open(os.path.join(kit.CSRC, "avd_audio_resample.h")).read()
    assert "sizeof(Tile) == 40" in resample and "tile_track" not in resample
    assert "static_assert(sizeof(Source) == 32" in text


# ---- plan_map, through the sanitized program -----------------------------------------------------------------------------------------------
def test_every_check_of_the_program():
    status, out = kit.run()
    assert status == 0 and re.fullmatch(r"audio map: \d+ calls checked, 0 failures\n", out), (status, out)
    assert int(out.split()[2]) > 9000


def test_windows_that_run_into_the_next_region_are_rejected():
    status, out = kit.run(mutated="windows_overrun")
    assert status == 1 and "FAIL" in out and "runs over the analysed" in out and not re.search(r", 0 failures", out), (status, out)
    # the records no longer sum to what the rule hands out
    good, bad = kit.plan(48000, 64, 3000, [1000], [1, 2], [5000, 777]), kit.plan(48000, 64, 3000, [1000], [1, 2], [5000, 777], mutated="windows_overrun")
    assert good["records"] == bad["records"] and good["tracks"] == bad["tracks"]            # the plan's own counts are the rule's; its window table is not


def test_a_neighbours_history_is_rejected():
    status, out = kit.run(mutated="neighbour_history")
    assert status == 1 and "FAIL" in out and "is handed the history of slot" in out and not re.search(r", 0 failures", out), (status, out)


@pytest.mark.parametrize("rate", (0, 16000, 44100, 48000, 11025, 192000))
def test_single_plans_follow_the_rule(rate):
    U, D, T = ratio(rate)
    win = 64
    frames = [0, 3 * T + 70, T // 2 + 1, 1000, 0, 0, 0, 5]                      # what slots 1 ... 8 have absorbed
    lens = [700, 1, 900, 333, 64]
    entries = [2, 3 | 0x10, 0, 8, 1]                                            # continued, ended, whole, continued, continued on an empty slot
    cuts = list(np.cumsum(lens)[:-1])
    p = kit.plan(rate, win, sum(lens), cuts, entries, frames)
    assert p["refused"] == 0 and p["continued"] == 4 and len(p["tracks"]) == 5
    at, records, end = 0, 0, 0
    for t, n, e in zip(p["tracks"], lens, entries):
        slot, last = e & 15, e == 0 or bool(e & 0x10)
        before = frames[slot - 1] if slot else 0
        m0, m1 = rule_outputs(rate, before), rule_outputs(rate, before + n, last)
        held, have = m0 % win, m0 % win + m1 - m0
        count = -(-have // win) if last else have // win
        assert (t["slot"], t["last"], t["begin"], t["n"], t["held"], t["fresh"], t["first"], t["count"]) == (slot, int(last), at, n, held, m1 - m0, records, count)
        assert t["held_after"] == (0 if last else have - count * win)
        assert t["region"] >= end and t["region"] % 8 == 0
        end = t["region"] + have
        at += n
        records += count
    assert p["records"] == records and p["total"] >= end and p["saves"] == 3
    assert p["gather"] == sum(1 for t in p["tracks"] if t["held"]) + (5 if rate == 0 else 0)
    # the same call with too small a records array, and with a cut at the buffer's end
    assert kit.plan(rate, win, sum(lens), cuts, entries, frames, max_windows=records - 1)["refused"] == 8
    assert kit.plan(rate, win, sum(lens), cuts[:-1] + [sum(lens)], entries, frames)["refused"] == 3
    assert kit.plan(rate, win, sum(lens), cuts, entries[:-1], frames)["refused"] == 5


# ---- the Python helpers against a recording context -----------------------------------------------------------------------------------------
class _MapLibrary(_FakeLibrary):
    """the recording library of tests/test_audio_stream_host.py, which also takes an "audio_track_slot" list: the rule, restated per track"""

    def avd_audio_features(self, h, ptr, mem, n, win, out_ptr, nwin):
        o = self.owner
        entries, cuts = o.lists["audio_track_slot"], o.lists["audio_cut"]
        o.lists = {"audio_track_slot": [], "audio_cut": []}                    # one-shot, whatever becomes of the call
        if not entries:
            return super().avd_audio_features(h, ptr, mem, n, win, out_ptr, nwin)
        assert o.options["audio_slot"] == 0 and o.options["audio_end"] == 0 and len(entries) == len(cuts) + 1
        rate = o.options["audio_rate"]
        bounds = [0] + cuts + [n]
        o.calls.append({"ptr": ptr, "n": n, "win": win, "nwin": nwin, "entries": entries, "cuts": cuts, "rate": rate, "channels": o.options["audio_channels"],
                        "format": o.options["audio_format"], "wrote": []})
        if o.fail_call == len(o.calls):
            return -1
        for e, a, b in zip(entries, bounds[:-1], bounds[1:]):
            slot, last = e & 15, e == 0 or bool(e & 0x10)
            frames = o.frames.get(slot, 0) if slot else 0
            m0, m1 = rule_outputs(rate, frames), rule_outputs(rate, frames + b - a, last)
            o.calls[-1]["wrote"].append((-(-m1 // win) if last else m1 // win) - m0 // win)
            if slot:
                o.frames[slot] = 0 if last else frames + b - a
                o.held[slot] = 0 if last else m1 % win
        assert nwin == sum(o.calls[-1]["wrote"]), ("the record array is the rule's sum", nwin, o.calls[-1]["wrote"])
        return 0


class MapRecorder(Recorder):
    def __init__(self, fail_call=0, fail_entry=None, **options):
        super().__init__(fail_call, **options)
        self.lists = {"audio_track_slot": [], "audio_cut": []}
        self.fail_entry = fail_entry
        self._L = _MapLibrary(self)

    def set_option(self, name, value):
        self.sets.append((name, value))
        if name in self.lists:
            if value == -1:
                self.lists[name] = []
                return
            if name == "audio_track_slot" and (self.options["audio_slot"] != 0 or value == self.fail_entry):
                raise _lib.AvdError("audio_track_slot: refused")
            self.lists[name].append(value)
            return
        if name == "audio_slot" and value != 0 and self.lists["audio_track_slot"]:
            raise _lib.AvdError("audio_slot: refused while a list is held")
        self.sets.pop()
        super().set_option(name, value)

    def get_option(self, name):
        return len(self.lists[name]) if name in self.lists else super().get_option(name)


def test_features_mapped_sets_the_list_in_track_order_and_sizes_from_the_rule():
    r = MapRecorder(audio_slot=3)
    r.frames[5], r.held[5] = 3000, rule_outputs(48000, 3000) % 64
    chunks = [np.zeros((n, 2), np.int16) for n in (700, 40, 2000, 1)]
    got = r.audio_features_mapped(chunks, [5, 2, 0, 7], [False, True, False, True], 64, rate=48000)
    c = r.calls[0]
    assert c["entries"] == [5, 2 | 0x10, 0, 7 | 0x10] and c["cuts"] == [700, 740, 2740] and c["n"] == 2741      # track order; a whole track has no end mark
    assert (c["rate"], c["channels"], c["format"]) == (48000, 2, 1) and [len(g) for g in got] == c["wrote"] and len(r.calls) == 1
    assert c["wrote"] == [(r.held[5] if False else (rule_outputs(48000, 3700) // 64 - rule_outputs(48000, 3000) // 64)), 1, -(-ref.n_out(2000, 48000) // 64), 1]
    # the options as they were; the lists gone
    assert r.options["audio_slot"] == 3 and r.options["audio_rate"] == 0 and r.options["audio_format"] == 0 and r.lists == {"audio_track_slot": [], "audio_cut": []}
    # the list is set after the cuts, entry by entry, and "audio_slot" is 0 while it is held
    names = [n for n, _ in r.sets]
    assert names.index("audio_track_slot") > max(i for i, n in enumerate(names) if n == "audio_cut")
    assert [v for n, v in r.sets if n == "audio_track_slot"] == c["entries"]
    # an unconverted float32 call
    r = MapRecorder()
    got = r.audio_features_mapped([np.zeros(25, np.float32), np.zeros(9, np.float32)], [1, 0], [False, False], 10)
    assert [len(g) for g in got] == [2, 1] and r.calls[0]["rate"] == 0 and r.calls[0]["format"] == 0 and r.frames[1] == 25 and r.held[1] == 5
    assert [len(g) for g in r.audio_features_mapped([np.zeros(6, np.float32)], [1], [True], 10)] == [2]


def test_the_list_is_cleared_after_an_exception():
    # the library refuses the third entry: the entries set so far and the cuts go, the options come back
    r = MapRecorder(fail_entry=4, audio_slot=2, audio_rate=44100)
    with pytest.raises(_lib.AvdError, match="audio_track_slot"):
        r.audio_features_mapped([np.zeros(30, np.int16)] * 3, [1, 3, 4], [False] * 3, 4, rate=48000, channels=1)
    assert r.calls == [] and r.lists == {"audio_track_slot": [], "audio_cut": []}
    assert r.sets[-4:-2] == [("audio_cut", -1), ("audio_track_slot", -1)] or ("audio_track_slot", -1) in r.sets
    assert (r.options["audio_slot"], r.options["audio_rate"], r.options["audio_format"]) == (2, 44100, 0)
    # the call itself fails: it has taken the list
    r = MapRecorder(fail_call=1, audio_slot=2)
    with pytest.raises(_lib.AvdError):
        r.audio_features_mapped([np.zeros(30, np.int16)] * 2, [1, 3], [False, True], 4, rate=48000, channels=1)
    assert len(r.calls) == 1 and r.lists == {"audio_track_slot": [], "audio_cut": []} and r.options["audio_slot"] == 2
    # a slot too far along for the rule's counts: refused by the binding, with the caller's selected slot back
    r = MapRecorder(audio_slot=3)
    r.frames[2] = 2 ** 31 + 5
    with pytest.raises(ValueError, match="2\\^31"):
        r.audio_features_mapped([np.zeros(30, np.int16)] * 2, [1, 2], [False, False], 4)
    assert r.calls == [] and r.options["audio_slot"] == 3 and r.lists == {"audio_track_slot": [], "audio_cut": []}
    # what the binding refuses itself
    r = MapRecorder()
    for bad in (dict(chunks=[], slots=[], lasts=[]), dict(chunks=[np.zeros(3, np.int16)], slots=[1, 2], lasts=[False]),
                dict(chunks=[np.zeros(3, np.int16), np.zeros(3, np.float32)], slots=[1, 2], lasts=[False, False]),
                dict(chunks=[np.zeros(3, np.int16), np.zeros(0, np.int16)], slots=[1, 2], lasts=[False, False])):
        with pytest.raises(ValueError):
            r.audio_features_mapped(bad["chunks"], bad["slots"], bad["lasts"], 4)
    assert r.calls == [] and r.sets == []


class StreamRecorder:
    """what the stream helpers hand to Context.audio_features_mapped, round by round"""

    def __init__(self, fail_at=0):
        self.calls, self.sets, self.fail_at = [], [], fail_at

    def set_option(self, name, value):
        self.sets.append((name, value))

    def audio_converted_length(self, n, rate):
        return _lib.Context.audio_converted_length(n, rate)

    def audio_features(self, wav, win, rate=None, slot=0, last=False):
        self.calls.append({"single": True, "n": len(wav), "slot": slot, "last": last})
        return np.zeros(0, _lib.AUDIO_WINDOW_DTYPE)

    def audio_features_mapped(self, chunks, slots, lasts, win, rate=None, channels=1):
        self.calls.append({"n": [len(c) for c in chunks], "first": [int(np.asarray(c).reshape(len(c), -1)[0, 0]) for c in chunks], "slots": list(slots), "lasts": list(lasts),
                           "win": win, "rate": rate, "shape": {c.shape[1:] for c in chunks}, "dtype": {c.dtype for c in chunks}})
        if self.fail_at == len(self.calls):
            raise _lib.AvdError("failed")
        rec = np.zeros(1, _lib.AUDIO_WINDOW_DTYPE)
        rec["length"], rec["nbins"], rec["sum_mag"], rec["sumsq"] = win, win // 2 + 1, 1.0, 1.0
        return [rec] * len(chunks)


def test_the_stream_helpers_make_one_call_per_round_and_reset_their_slots():
    sizes = ([4096, 4096, 100], [4096], [300, 0, 300, 300, 300, 7])                 # an empty piece is skipped
    r = StreamRecorder()
    got = host_audio.analyze_decoded_streams([_numbered_chunks(s, 2, np.int16) for s in sizes], 48000, r)
    assert [c["slots"] for c in r.calls] == [[1, 2, 3], [1, 3], [1, 3], [3], [3]]   # one call per round, over the streams that gave something
    assert [c["n"] for c in r.calls] == [[4096, 4096, 300], [4096, 300], [100, 300], [300], [7]]
    assert [c["lasts"] for c in r.calls] == [[False, True, False], [False, False], [True, False], [False], [True]]   # each ends in the round of its last piece
    assert [c["first"] for c in r.calls] == [[0, 0, 0], [4096, 300], [8192, 600], [900], [1200]]     # every piece once, in order
    assert all(c["win"] == 8000 and c["rate"] == 48000 and c["shape"] == {(2,)} and c["dtype"] == {np.dtype(np.int16)} for c in r.calls)
    resets = [("audio_slot_reset", k) for k in (1, 2, 3)]
    assert r.sets == resets + resets and len(got) == 3                           # emptied first, reset at the end
    assert [len(g["timeline"]) for g in got] == [max(1, round(ref.n_out(sum(s), 48000) / 16000)) for s in sizes]
    # 16 kHz tracks: the first channel, in their own type; a stream that gives nothing is the empty track
    r = StreamRecorder()
    host_audio.analyze_wave_streams([_numbered_chunks([5000, 20], 2, np.float32), iter([])], 16000, r)
    assert [c.get("slots") for c in r.calls] == [[1], [1], None] and r.calls[0]["rate"] is None and r.calls[0]["shape"] == {()} and r.calls[2] == {"single": True, "n": 0, "slot": 0, "last": False}
    with pytest.raises(ValueError):
        host_audio.analyze_wave_streams([iter([])] * 9, 16000, StreamRecorder())


def test_the_stream_helpers_reset_their_slots_after_an_exception():
    r = StreamRecorder(fail_at=2)
    with pytest.raises(_lib.AvdError):
        host_audio.analyze_decoded_streams([_numbered_chunks([10] * 4, 1, np.int16), _numbered_chunks([10] * 4, 1, np.int16)], 48000, r)
    assert len(r.calls) == 2 and r.sets[-2:] == [("audio_slot_reset", 1), ("audio_slot_reset", 2)] and len(r.sets) == 4

    def broken():
        yield np.zeros((5, 1), np.int16)
        raise OSError("the decoder gave up")
    r = StreamRecorder()
    with pytest.raises(OSError):
        host_audio.analyze_decoded_streams([broken()], 48000, r)
    assert r.calls == [] and r.sets == [("audio_slot_reset", 1)] * 2


def test_the_calls_of_a_run_without_streams_are_unchanged():
    """what audio_features and audio_features_many hand to the library does not know the new option"""
    r = MapRecorder()
    r.audio_features(np.zeros(9, np.float32), 4)
    r.audio_features(np.zeros((40, 2), np.int16), 64, rate=48000, slot=5)
    r.audio_features_many([np.zeros(9, np.float32), np.zeros(5, np.float32)], 4)
    assert "audio_track_slot" not in [n for n, _ in r.sets] and all("entries" not in c for c in r.calls)
    plain = Recorder()
    plain.audio_features(np.zeros(9, np.float32), 4)
    plain.audio_features(np.zeros((40, 2), np.int16), 64, rate=48000, slot=5)
    keys = ("n", "win", "nwin", "slot", "last", "rate", "channels", "format")
    assert [[c[k] for k in keys] for c in r.calls[:2]] == [[c[k] for k in keys] for c in plain.calls]
