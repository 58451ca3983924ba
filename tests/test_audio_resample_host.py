"""Tracks at the decoder's rate (options "audio_rate" / "audio_channels", include/avd.h), without a GPU.

  * csrc/avd_audio_resample.h through tests/audio_resample_check.cpp, a stand-alone program built with AddressSanitizer and UBSan by
    tests/audio_resample_kit.py and RUN AS A PROGRAM: ratios, filter banks, output ranges, tile table; two mutated planners (a 32-bit tile
    base, a dropped last output) must be rejected by it;
  * the header's filter banks against the numpy restatement (tests/audio_resample_reference.py), entry for entry;
  * the signal quality of the restatement;
  * the header's text; Context.audio_features(_many) with rate and avd_hip.audio.analyze_decoded(_many) against a context that only records.

Bounds.  Banks: exact equality, but for an entry whose unrounded value lies within 1e-9 of a half (libm and numpy may differ in the last bits
of h; 32768 * 1e-15 is far below 1e-9) -- and the restatement has no such entry: its nearest approach to a half is 1.46e-6 (22050).  Signal
quality: 6 LSB for a 1 kHz sine of 20000 peak (5 measured), 4 LSB of residue of a 10 kHz tone at 48 kHz (3 measured), as the rule was stated.
"""
import os
import re

import numpy as np
import pytest

from avd_hip import _lib
from avd_hip import audio as host_audio
from tests import audio_resample_kit as kit
from tests import audio_resample_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- ratios and banks -----------------------------------------------------------------------------------------------------------------------
WANT_RATIOS = {8000: (2, 1, 32), 11025: (640, 441, 32), 12000: (4, 3, 32), 16000: (1, 1, 0), 22050: (320, 441, 46), 24000: (2, 3, 50), 32000: (1, 2, 66),
               44100: (160, 441, 92), 48000: (1, 3, 100), 88200: (80, 441, 182), 96000: (1, 6, 198), 176400: (40, 441, 364), 192000: (1, 12, 396)}


def test_the_thirteen_ratios():
    assert tuple(sorted(WANT_RATIOS)) == ref.RATES == host_audio.RESAMPLE_RATES == _lib.Context.AUDIO_RATES
    for rate, want in WANT_RATIOS.items():
        assert ref.ratio(rate) == want, rate
        assert kit.taps(rate)[:3] == want, rate
        assert max(r * t for r, _, t in [want]) <= 20480


@pytest.mark.parametrize("rate", ref.RATES)
def test_the_bank_equals_the_restatement_entry_for_entry(rate):
    U, D, T, _, got = kit.taps(rate)
    want, unrounded = ref.bank(rate)
    assert got.shape == want.shape == (U, T)
    if T == 0:
        return
    near_half = np.abs(np.abs(unrounded - np.floor(unrounded)) - 0.5) < 1e-9
    print("rate %d: nearest approach of an unrounded entry to a half %.3g" % (rate, np.abs(np.abs(unrounded - np.floor(unrounded)) - 0.5).min()))
    assert not near_half.any()                                   # the exception is empty for the restatement itself ...
    assert np.array_equal(got, want)                             # ... so every entry is equal


@pytest.mark.parametrize("rate", ref.RATES)
def test_bank_properties(rate):
    q, _ = ref.bank(rate)
    got = kit.taps(rate)[4]
    for b in (q, got):
        if b.shape[1] == 0:
            assert rate == 16000
            continue
        assert (b.sum(axis=1) == 32768).all()
        mag = np.abs(b).sum(axis=1).max()
        print("rate %d: sum|q| at most %d, entries %d ... %d" % (rate, mag, b.min(), b.max()))
        if rate >= 16000:
            assert mag <= 65535 and 32768 * int(mag) + 16384 < 2 ** 31 and b.min() >= -32768 and b.max() <= 32767
        else:
            assert mag == 77084 and b.max() == 32768             # what asks for the wide accumulator and 32-bit entries


# ---- the plan header, through the sanitized program ---------------------------------------------------------------------------------------------
def test_the_header_is_plain_host_code():
    text = open(kit.HEADER).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes


def test_every_check_of_the_program():
    status, out = kit.run()
    assert status == 0 and re.fullmatch(r"audio resample: \d+ plans checked, 0 failures\n", out), (status, out)
    assert int(out.split()[2]) > 6000


def test_a_32_bit_tile_base_is_rejected():
    status, out = kit.run(mutated="base32")
    assert status == 1 and "FAIL" in out and not re.search(r", 0 failures", out), (status, out)
    # short tracks plan as before: the mutation shows only where m D leaves 32 bits
    assert kit.plan(44100, 100000, (), mutated="base32") == kit.plan(44100, 100000)
    assert kit.plan(44100, 13500000, (), mutated="base32")["tiles"][-1] != kit.plan(44100, 13500000)["tiles"][-1]


def test_a_dropped_last_output_is_rejected():
    status, out = kit.run(mutated="floor")
    assert status == 1 and "FAIL" in out and not re.search(r", 0 failures", out), (status, out)
    assert kit.plan(48000, 3000, (), mutated="floor") == kit.plan(48000, 3000)              # D divides n: nothing to drop
    assert kit.plan(48000, 3001, (), mutated="floor")["n_out"] == 1000 and kit.plan(48000, 3001)["n_out"] == 1001


@pytest.mark.parametrize("rate,n", [(48000, 10000), (44100, 13500000), (8000, 700), (192000, 50000), (16000, 2500)])
def test_the_tiles_are_those_of_the_restatement(rate, n):
    p = kit.plan(rate, n)
    assert p["refused"] == 0 and p["n_out"] == ref.n_out(n, rate) and p["tracks"] == [(0, ref.n_out(n, rate))]
    want = ref.tiles(n, rate, p["tile_out"])
    assert p["ntiles"] == len(want)
    assert p["tiles"] == (want if len(want) <= 64 else [want[0], want[-1]])


def test_tracks_and_refusals_of_a_batch():
    p = kit.plan(48000, 10, (5, 9))
    assert p["tracks"] == [(0, 2), (2, 2), (4, 1)] and p["n_out"] == 5
    assert [t[:3] for t in p["tiles"]] == [(0 - 49, 0, 2), (5 - 49, 2, 2), (9 - 49, 4, 1)]        # every track from its own start, T/2 - 1 = 49 frames before it
    assert kit.plan(48000, 10, (5, 10))["refused"] == 1
    assert kit.plan(8000, 2 ** 31)["refused"] == 3


# ---- signal quality of the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [48000, 44100])
def test_a_1_khz_sine_comes_back_within_6_lsb(rate):
    s = np.rint(20000 * np.sin(2 * np.pi * 1000 * np.arange(rate) / rate)).astype(np.int16)
    y = ref.convert(s, rate).astype(np.int64)
    assert len(y) == 16000
    ideal = 20000 * np.sin(2 * np.pi * 1000 * np.arange(len(y)) / 16000)
    err = np.abs(y - ideal)[200:-200].max()
    print("rate %d: 1 kHz sine, largest error %.3f LSB" % (rate, err))
    assert err <= 6


def test_a_10_khz_tone_at_48_khz_leaves_at_most_4_lsb():
    s = np.rint(20000 * np.sin(2 * np.pi * 10000 * np.arange(48000) / 48000)).astype(np.int16)
    residue = np.abs(ref.convert(s, 48000).astype(np.int64))[200:-200].max()
    print("10 kHz tone at 48 kHz: residue %d LSB" % residue)
    assert residue <= 4


def test_the_restatement_on_values_written_out_by_hand():
    assert ref.narrow(np.array([0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768, 1.0, 2.0, -1.0, -3.0, np.nan, np.inf, -np.inf], np.float32)).tolist() == \
        [0, 2, 2, 0, -2, 32767, 32767, -32768, -32768, 0, 32767, -32768]
    assert ref.downmix(np.array([[3, 4], [-3, -4], [5, -5], [32767, 32767], [-32768, -32768], [-1, 0]], np.int16)).tolist() == [4, -3, 0, 32767, -32768, 0]
    x = np.array([[100, 300], [-7, 9]], np.int16)
    assert np.array_equal(ref.convert(x, 16000), np.array([200, 1], np.int16))                       # 16000: downmix only
    # a constant comes back as itself away from the ends: every phase sums to 32768
    y = ref.convert(np.full(5000, 12345, np.int16), 44100)
    assert (y[40:-40] == 12345).all() and len(y) == ref.n_out(5000, 44100) == 1815


# ---- the header's text ---------------------------------------------------------------------------------------------------------------------
def test_header_names_the_options_and_the_debug_buffers():
    text = open(os.path.join(ROOT, "include", "avd.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for name in ('"audio_rate"', '"audio_channels"', '"audio_rs_plan"', '"audio_rs_taps"', '"audio_rs_tracks"', '"audio_pcm"'):
        assert name in flat, name
    assert "unpinned" in flat and "floor((L + R + 1) / 2)" in flat and "ties to even" in flat
    for rate in ref.RATES:
        assert str(rate) in flat
    assert re.search(r"#define\s+AVD_ABI_VERSION\s+3\b", text) and len(_lib.EXPORTS) == 43
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        assert "unpinned" in open(os.path.join(ROOT, doc)).read(), doc


# ---- the Python helpers against a recording context ---------------------------------------------------------------------------------------------
class _FakeLibrary:
    def __init__(self, owner):
        self.owner = owner

    def avd_audio_features(self, h, ptr, mem, n, win, out_ptr, nwin):
        o = self.owner
        o.calls.append({"ptr": ptr, "mem": mem, "n": n, "win": win, "nwin": nwin, "cuts": list(o.cuts), **o.options})
        o.cuts = []
        if o.fail_call == len(o.calls):
            return -1
        rec = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_uint8 * (48 * nwin)).from_address(out_ptr)).view(_lib.AUDIO_WINDOW_DTYPE) if nwin else np.zeros(0, _lib.AUDIO_WINDOW_DTYPE)
        rec["length"] = len(o.calls)
        rec["nbins"] = np.arange(nwin)
        return 0


class Recorder(_lib.Context):
    """a Context without a library: what the audio helpers do above the C-ABI, call by call"""

    def __init__(self, fail_call=0, **options):
        self._h = None
        self.device = 0
        self.calls, self.cuts, self.sets = [], [], []
        self.options = {"audio_format": 0, "audio_rate": 0, "audio_channels": 1, **options}
        self.fail_call = fail_call
        self._L = _FakeLibrary(self)

    def _check(self, rc):
        if rc != 0:
            raise _lib.AvdError("avd status %d" % rc)

    def set_option(self, name, value):
        self.sets.append((name, value))
        if name == "audio_cut":
            self.cuts = [] if value == -1 else self.cuts + [value]
        elif name == "audio_rate" and value != 0 and value not in ref.RATES:
            raise _lib.AvdError("audio_rate: refused")
        elif name == "audio_channels" and value not in (1, 2):
            raise _lib.AvdError("audio_channels: refused")
        else:
            self.options[name] = value

    def get_option(self, name):
        return len(self.cuts) if name == "audio_cut" else self.options[name]


def test_features_with_a_rate_sets_the_options_counts_output_windows_and_restores():
    r = Recorder()
    out = r.audio_features(np.zeros((48000 * 2 + 1, 2), np.int16), 8000, rate=48000)
    (call,) = r.calls
    assert (call["n"], call["audio_rate"], call["audio_channels"], call["audio_format"]) == (96001, 48000, 2, 1)
    assert call["nwin"] == len(out) == 5                                                   # 32001 output samples: four windows and a short one
    assert r.options == {"audio_format": 0, "audio_rate": 0, "audio_channels": 1}
    r = Recorder()
    r.audio_features(np.zeros(44100, np.float32), 1001, rate=44100)                        # flat mono float32
    assert (r.calls[0]["n"], r.calls[0]["nwin"], r.calls[0]["audio_channels"], r.calls[0]["audio_format"]) == (44100, 16, 1, 0)
    r = Recorder()
    r.audio_features(np.zeros(10, np.int16), 4, rate=8000, channels=2)                     # flat stereo: five frames, ten output samples
    assert (r.calls[0]["n"], r.calls[0]["nwin"]) == (5, 3)
    with pytest.raises(ValueError):
        r.audio_features(np.zeros(9, np.int16), 4, rate=8000, channels=2)


def test_the_options_come_back_after_an_exception_and_keep_a_callers_values():
    r = Recorder(fail_call=1, audio_rate=44100, audio_channels=2)
    with pytest.raises(_lib.AvdError):
        r.audio_features(np.zeros(30, np.int16), 4, rate=48000)
    assert r.calls[0]["audio_rate"] == 48000 and r.calls[0]["audio_channels"] == 1
    assert r.options == {"audio_format": 0, "audio_rate": 44100, "audio_channels": 2}
    r = Recorder()
    with pytest.raises(_lib.AvdError, match="audio_rate"):
        r.audio_features(np.zeros(30, np.int16), 4, rate=44000)
    assert r.calls == [] and r.options == {"audio_format": 0, "audio_rate": 0, "audio_channels": 1}
    with pytest.raises(_lib.AvdError, match="audio_channels"):
        r.audio_features(np.zeros((10, 3), np.int16), 4, rate=48000)
    assert r.calls == [] and r.options == {"audio_format": 0, "audio_rate": 0, "audio_channels": 1} and r.cuts == []
    # without a rate nothing new is touched
    r = Recorder()
    r.audio_features(np.zeros(9, np.float32), 4)
    assert r.sets == [] and r.calls[0]["nwin"] == 3


def test_many_with_a_rate_cuts_in_frames_and_counts_each_tracks_own_windows():
    lens = [10, 3, 8, 1]                                                                   # frames at 48000: 4, 1, 3, 1 output samples
    r = Recorder()
    out = r.audio_features_many([np.zeros((n, 2), np.int16) for n in lens], 2, rate=48000)
    (call,) = r.calls
    assert call["cuts"] == [10, 13, 21] and call["n"] == 22 and call["audio_channels"] == 2 and call["audio_rate"] == 48000
    assert [len(o) for o in out] == [2, 1, 2, 1] and call["nwin"] == 6
    assert r.options == {"audio_format": 0, "audio_rate": 0, "audio_channels": 1}
    lens = [7] * 70
    r = Recorder(fail_call=2)
    with pytest.raises(_lib.AvdError):
        r.audio_features_many([np.zeros((n, 2), np.float32) for n in lens], 2, rate=8000)
    assert len(r.calls) == 2 and r.calls[1]["ptr"] - r.calls[0]["ptr"] == 64 * 7 * 2 * 4          # frames of two float32 samples
    assert r.calls[0]["nwin"] == 64 * 7 and r.options == {"audio_format": 0, "audio_rate": 0, "audio_channels": 1} and r.cuts == []
    with pytest.raises(ValueError, match="one channel count"):
        Recorder().audio_features_many([np.zeros((4, 2), np.int16), np.zeros(4, np.int16)], 2, rate=8000)


def test_analyze_decoded_many_groups_by_rate_channels_and_type(monkeypatch):
    monkeypatch.setattr(host_audio, "features_to_result", lambda values, dur: {"dur": dur, "windows": len(values["rms"])})
    monkeypatch.setattr(host_audio, "window_values", lambda rec: {"rms": list(rec["nbins"])})
    waves = [(np.zeros((48000, 2), np.int16), 48000), (np.zeros(44100, np.int16), 44100), (np.zeros((24001, 2), np.int16), 48000),
             (np.zeros((48000, 2), np.float32), 48000), (np.zeros((96000, 1), np.int16), 48000)]
    r = Recorder()
    out = host_audio.analyze_decoded_many(waves, r)
    assert [(c["audio_rate"], c["audio_channels"], c["audio_format"], len(c["cuts"]) + 1, c["win"]) for c in r.calls] == \
        [(48000, 2, 1, 2, 8000), (44100, 1, 1, 1, 8000), (48000, 2, 0, 1, 8000), (48000, 1, 1, 1, 8000)]
    assert [o["windows"] for o in out] == [2, 2, 2, 2, 4]
    assert [o["dur"] for o in out] == [1.0, 1.0, 8001 / 16000, 1.0, 2.0]
    one = host_audio.analyze_decoded(np.zeros((44100 * 3, 2), np.float32), 44100, Recorder())
    assert one == {"dur": 3.0, "windows": 6}
    with pytest.raises(ValueError):
        host_audio.analyze_decoded(np.zeros((10, 3), np.int16), 48000, Recorder())


def test_read_wav_frames_returns_every_channel(tmp_path):
    import wave
    pcm = np.arange(-50, 50, dtype="<i2")
    p = tmp_path / "stereo.wav"
    with wave.open(str(p), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(44100)
        w.writeframes(np.stack([pcm, -pcm], axis=1).tobytes())
    got, sr = host_audio.read_wav_frames(str(p))
    assert sr == 44100 and got.dtype == np.int16 and got.shape == (100, 2) and np.array_equal(got[:, 0], pcm) and np.array_equal(got[:, 1], -pcm)
    first, _ = host_audio.read_wav_native(str(p))
    assert np.array_equal(first, pcm)                                                       # the older readers keep their meaning
