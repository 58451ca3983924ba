"""Several tracks per avd_audio_features call and 16-bit PCM as decoded, without a GPU (include/avd.h: options "audio_format" and "audio_cut",
debug buffer "audio_tracks").

  * the header's text and the unchanged export list;
  * the int16 rule over all 65536 values: float32(s) * 2^-15 is s / 32768 rounded to float32 and is what read_wav_pcm returns;
  * csrc/avd_audio_plan.h through tests/audio_plan_check.cpp, a stand-alone program built with AddressSanitizer and UBSan by
    tests/audio_plan_kit.py and RUN AS A PROGRAM; one mutated planner (windows counted from the buffer's start) must be rejected by it;
  * Context.audio_features_many and avd_hip.audio.analyze_waves against a context that only records its calls.
"""
import os
import re
import wave

import numpy as np
import pytest

from avd_hip import _lib
from avd_hip import audio as host_audio
from tests import audio_plan_kit as kit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the header -------------------------------------------------------------------------------------------------------------------------
def _audio_block():
    text = open(os.path.join(ROOT, "include", "avd.h")).read()
    end = text.index("typedef struct avd_audio_window")
    return re.sub(r"\s*\n \*\s*", " ", text[text.rindex("/*", 0, end):end])


def test_header_names_the_options_and_the_debug_buffer():
    flat = _audio_block()
    for name in ('"audio_format"', '"audio_cut"', '"audio_tracks"', '"audio_plan"'):
        assert name in flat, name
    assert "(float)s * 2^-15" in flat and "one-shot" in flat and "byte for byte" in flat
    assert "audio_cut: beyond the buffer" in flat and "at most 63" in flat


def test_nothing_is_exported_for_it():
    text = open(os.path.join(ROOT, "include", "avd.h")).read()
    assert len(_lib.EXPORTS) == 43
    assert re.search(r"#define\s+AVD_ABI_VERSION\s+3\b", text)
    assert not re.search(r"\bavd_audio_(?!features\b|window\b)\w+\s*\(", text)
    for name in ("audio_features_many", "audio_tracks", "audio_features"):
        assert callable(getattr(_lib.Context, name))
    assert callable(host_audio.analyze_waves) and callable(host_audio.read_wav_native)


# ---- the int16 rule ---------------------------------------------------------------------------------------------------------------------
def test_the_int16_rule_over_all_65536_values(tmp_path):
    s = np.arange(-32768, 32768, dtype=np.int32)
    rule = s.astype(np.int16).astype(np.float32) * np.float32(2.0 ** -15)
    assert rule.dtype == np.float32
    assert np.array_equal(rule, (s.astype(np.float64) / 32768.0).astype(np.float32))
    assert np.array_equal(rule.astype(np.float64), s / 32768.0)                        # not merely rounded alike: exact
    p = tmp_path / "all.wav"
    with wave.open(str(p), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(s.astype("<i2").tobytes())
    as_float, sr = host_audio.read_wav_pcm(str(p))
    assert sr == 16000 and as_float.dtype == np.float32 and np.array_equal(as_float, rule)
    native, sr = host_audio.read_wav_native(str(p))
    assert sr == 16000 and native.dtype == np.int16 and np.array_equal(native, s)


def test_the_native_reader_takes_the_first_channel_and_leaves_other_widths_alone(tmp_path):
    pcm = np.arange(-50, 50, dtype="<i2")
    p = tmp_path / "stereo.wav"
    with wave.open(str(p), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(np.stack([pcm, -pcm], axis=1).tobytes())
    got, _ = host_audio.read_wav_native(str(p))
    assert got.dtype == np.int16 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, pcm)
    q = tmp_path / "wide.wav"
    with wave.open(str(q), "wb") as w:
        w.setnchannels(1); w.setsampwidth(4); w.setframerate(16000)
        w.writeframes((pcm.astype("<i4") << 16).tobytes())
    got, _ = host_audio.read_wav_native(str(q))
    want, _ = host_audio.read_wav_pcm(str(q))
    assert got.dtype == np.float32 and np.array_equal(got, want)


# ---- the plan header, through the sanitized program -------------------------------------------------------------------------------------------
def test_the_plan_header_is_plain_host_code():
    text = open(kit.HEADER).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
    assert "std::cos" not in text and "std::sin" not in text        # no table value is formed in it: avd_audio.hip builds them, one function for every length


def test_every_check_of_the_plan_program():
    status, out = kit.run()
    assert status == 0 and re.fullmatch(r"audio plan: \d+ plans checked, 0 failures\n", out), (status, out)
    assert int(out.split()[2]) > 6000


def test_the_mutated_planner_is_rejected():
    """windows counted from the buffer's start instead of the track's start"""
    status, out = kit.run(mutated=True)
    assert status == 1 and "FAIL" in out, (status, out)
    assert not re.search(r", 0 failures", out)
    # the mutation is a change of the rule, not a crash: a single track still plans as before
    assert kit.plan(20, 8, (), mutated=True)["windows"] == [(0, 8, -1), (8, 8, -1), (16, 4, 0)]
    assert kit.plan(20, 8, (4,), mutated=True)["windows"] != kit.plan(20, 8, (4,))["windows"]


def test_a_layout_written_out_by_hand():
    p = kit.plan(20, 4, (5, 9))
    assert p["refused"] == 0 and p["nwin"] == 6 and p["nfull"] == 0
    assert p["tracks"] == [(0, 2, 1), (2, 1, 4), (3, 3, 3)]
    assert p["windows"] == [(0, 4, -1), (4, 1, 0), (5, 4, -1), (9, 4, -1), (13, 4, -1), (17, 3, 3)]
    assert p["lengths"] == [1, 3] and p["arena"] == 12 and p["max_dft_len"] == 4
    assert p["upload_bytes"] == 8 * 12 + 16 * 6 + 4 * 6


def test_shared_sets_and_the_fft_list_at_8000():
    lens = [16037, 8000, 5, 1, 12000, 7999, 8001, 12000, 16002]
    cuts = np.cumsum(lens)[:-1].tolist()
    p = kit.plan(sum(lens), 8000, cuts)
    assert [t[1] for t in p["tracks"]] == [3, 1, 1, 1, 2, 1, 2, 2, 3] and [t[2] for t in p["tracks"]] == [37, 8000, 5, 1, 4000, 7999, 1, 4000, 2]
    assert p["lengths"] == [37, 5, 1, 4000, 7999, 2] and p["nfull"] == 8
    assert {l % 4 for l in p["lengths"]} == {0, 1, 2, 3}


def test_the_refusal_order():
    assert kit.plan(10, 4, (5, 10), 100)["refused"] == 1                 # a cut at n: beyond the buffer
    assert kit.plan(10, 4, (5, 11), 0)["refused"] == 1                   # ... ahead of the windows array
    assert kit.plan(10, 4, (5, 9), 4)["refused"] == 0
    assert kit.plan(10, 4, (5, 9), 3)["refused"] == 2                    # one below the sum, although ceil(10 / 4) = 3 fits


@pytest.mark.parametrize("bad", [("5",), ("0", "4", "9"), ("5", "9000", "9")])
def test_dump_mode_refuses_what_it_cannot_plan(bad):
    status, _ = kit.run(*bad)
    assert status == 2


# ---- audio_features_many / analyze_waves against a recording context ----------------------------------------------------------------------------
class _FakeLibrary:
    def __init__(self, owner):
        self.owner = owner

    def avd_audio_features(self, h, ptr, mem, n, win, out_ptr, nwin):
        o = self.owner
        o.calls.append({"ptr": ptr, "mem": mem, "n": n, "win": win, "nwin": nwin, "cuts": list(o.cuts), "format": o.options["audio_format"]})
        o.cuts = []                                                       # one-shot, as in the library
        if o.fail_call == len(o.calls):
            return -1
        # the record of window w of the call says so: length = the call's number, nbins = w
        rec = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_uint8 * (48 * nwin)).from_address(out_ptr)).view(_lib.AUDIO_WINDOW_DTYPE) if nwin else np.zeros(0, _lib.AUDIO_WINDOW_DTYPE)
        rec["length"] = len(o.calls)
        rec["nbins"] = np.arange(nwin)
        return 0


class Recorder(_lib.Context):
    """a Context without a library: what the audio helpers do above the C-ABI, call by call"""

    def __init__(self, fail_call=0, audio_format=0):
        self._h = None
        self.device = 0
        self.calls, self.cuts, self.sets = [], [], []
        self.options = {"audio_format": audio_format}
        self.fail_call = fail_call
        self._L = _FakeLibrary(self)

    def _check(self, rc):
        if rc != 0:
            raise _lib.AvdError("avd status %d" % rc)

    def set_option(self, name, value):
        self.sets.append((name, value))
        if name == "audio_cut":
            if value == -1:
                self.cuts = []
            else:
                assert value > 0 and (not self.cuts or value > self.cuts[-1]) and len(self.cuts) < 63, (value, self.cuts)
                self.cuts.append(value)
        else:
            self.options[name] = value

    def get_option(self, name):
        return len(self.cuts) if name == "audio_cut" else self.options[name]


def _tracks(lens, dtype=np.float32, seed=0):
    rng = np.random.default_rng(seed)
    return [(rng.integers(-3000, 3000, n).astype(dtype) if dtype == np.int16 else rng.standard_normal(n).astype(dtype)) for n in lens]


def test_many_sets_ascending_cuts_and_splits_the_records():
    lens = [10, 3, 8, 1]
    r = Recorder()
    out = r.audio_features_many(_tracks(lens), 4)
    (call,) = r.calls
    assert call["cuts"] == [10, 13, 21] and call["n"] == 22 and call["win"] == 4 and call["nwin"] == 3 + 1 + 2 + 1
    assert call["format"] == 0 and call["mem"] == _lib.AVD_MEM_HOST
    assert [len(o) for o in out] == [3, 1, 2, 1]
    assert np.concatenate([o["nbins"] for o in out]).tolist() == list(range(7))        # the call's records, track after track
    assert all(name == "audio_cut" for name, _ in r.sets)                              # float32: the format option is not touched


def test_many_makes_one_call_per_64_tracks():
    lens = [5 + (i % 3) for i in range(130)]
    r = Recorder()
    out = r.audio_features_many(_tracks(lens), 4)
    assert [len(c["cuts"]) + 1 for c in r.calls] == [64, 64, 2]
    starts = np.concatenate([[0], np.cumsum(lens)])
    for k, c in enumerate(r.calls):
        first = starts[64 * k]
        assert c["cuts"] == [int(s - first) for s in starts[64 * k + 1:min(64 * k + 64, 130)]]
        assert c["n"] == int(starts[min(64 * k + 64, 130)] - first)
        assert c["ptr"] - r.calls[0]["ptr"] == 4 * first                               # one concatenated buffer, float32
    assert len(out) == 130 and [int(o["length"][0]) for o in out] == [1] * 64 + [2] * 64 + [3] * 2
    assert [len(o) for o in out] == [2] * 130


def test_many_with_int16_sets_and_restores_the_format_also_after_an_exception():
    lens = [6, 6, 6]
    r = Recorder()
    r.audio_features_many(_tracks(lens, np.int16), 4)
    assert r.calls[0]["format"] == 1 and r.options["audio_format"] == 0
    lens = [5] * 70
    r = Recorder(fail_call=2)
    with pytest.raises(_lib.AvdError):
        r.audio_features_many(_tracks(lens, np.int16), 4)
    assert len(r.calls) == 2 and r.options["audio_format"] == 0 and r.cuts == []
    assert r.calls[1]["ptr"] - r.calls[0]["ptr"] == 2 * 64 * 5                         # int16: two bytes a sample
    r = Recorder(fail_call=1, audio_format=1)                                          # a caller who keeps format 1 keeps it
    with pytest.raises(_lib.AvdError):
        r.audio_features(np.zeros(9, np.int16), 4)
    assert r.options["audio_format"] == 1 and r.calls[0]["format"] == 1
    r = Recorder(fail_call=1)
    with pytest.raises(_lib.AvdError):
        r.audio_features(np.zeros(9, np.int16), 4)
    assert r.options["audio_format"] == 0 and r.calls[0]["format"] == 1
    r = Recorder()
    assert len(r.audio_features(np.zeros(9, np.float32), 4)) == 3 and r.calls[0]["format"] == 0 and r.sets == []
    r = Recorder(audio_format=1)                                                       # the samples handed over decide, not what the option was left at
    r.audio_features(np.zeros(9, np.float32), 4)
    assert r.calls[0]["format"] == 0 and r.options["audio_format"] == 1 and r.sets == [("audio_format", 0), ("audio_format", 1)]


def test_many_refuses_mixed_tracks_and_passes_empty_ones_by():
    r = Recorder()
    with pytest.raises(ValueError, match="all float32 or all int16"):
        r.audio_features_many([np.zeros(4, np.float32), np.zeros(4, np.int16)], 4)
    with pytest.raises(ValueError):
        r.audio_features_many([np.zeros((4, 2), np.float32)], 4)
    assert r.calls == [] and r.sets == []
    assert r.audio_features_many([], 4) == []
    out = r.audio_features_many([np.zeros(0, np.float32), np.ones(5, np.float32), np.zeros(0, np.float32), np.ones(4, np.float32)], 4)
    assert [len(o) for o in out] == [0, 2, 0, 1] and r.calls[0]["cuts"] == [5] and r.calls[0]["n"] == 9


def test_analyze_waves_groups_by_window_length_and_keeps_the_input_order(monkeypatch):
    seen = []
    monkeypatch.setattr(host_audio, "features_to_result", lambda values, dur: {"dur": dur, "windows": len(values["rms"])})
    monkeypatch.setattr(host_audio, "window_values", lambda rec: (seen.append(int(rec["length"][0])), {"rms": list(rec["nbins"])})[1])
    waves = [(np.ones(9, np.float32), 8), (np.ones(30, np.float32), 20), (np.ones((5, 2), np.float32), 8), (np.ones(11, np.float32), 20),
             (np.ones(8, np.int16), 8)]
    r = Recorder()
    out = host_audio.analyze_waves(waves, r)
    assert [(c["win"], len(c["cuts"]) + 1, c["format"]) for c in r.calls] == [(4, 2, 0), (10, 2, 0), (4, 1, 1)]      # one call per win and sample type
    assert [o["windows"] for o in out] == [3, 3, 2, 2, 2]
    assert [o["dur"] for o in out] == [9 / 8, 30 / 20, 5 / 8, 11 / 20, 1.0]
    assert seen == [1, 1, 2, 2, 3]                                   # the call each record array came from: group by group, and inside a group in input order
    assert r.options["audio_format"] == 0
