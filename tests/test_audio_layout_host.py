"""Planar and 5.1 / 7.1 tracks (options "audio_layout" / "audio_plane_stride", include/avd.h), without a GPU.

  * the two options, the four ids and the planar flag in the header, the library's option table and the binding;
  * the downmix weights: derived from the gains (tests/audio_layout_reference.py), equal to the table the header writes out and to what
    csrc/avd_audio_resample.h derives (through tests/audio_layout_check.cpp, a stand-alone program built with AddressSanitizer and UBSan by
    tests/audio_layout_kit.py and RUN AS A PROGRAM); every row sums to 32768; the accumulator stays inside 32 bits;
  * layouts 1 and 2 against the existing restatement's downmix (tests/audio_resample_reference.py) on every pair of a value set that holds the
    extremes, both signs and +-1 around every rounding boundary of (L + R + 1) >> 1 (the parity of L + R at both ends of the range and at 0);
  * the LDS sizing of a layout launch against the bound lds_bytes(r, 2) + 4 max_span(r) + 16 at all thirteen rates;
  * Context.audio_features(_many, _mapped) and the avd_hip.audio helpers with layout / planar against a context that only records; the drop-in's
    two environment variables.
"""
import os
import re
import wave

import numpy as np
import pytest

from avd_hip import _lib
from avd_hip import audio as host_audio
from tests import audio_layout_kit as kit
from tests import audio_layout_reference as lay
from tests import audio_resample_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ai-video-detector_amd", "csrc")


# ---- names: header, option table, binding ----------------------------------------------------------------------------------------------------
def test_options_ids_and_flag_are_named_in_header_library_and_binding():
    header = open(os.path.join(ROOT, "include", "avd.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    for name, value in (("AVD_AUDIO_LAYOUT_MONO", "1"), ("AVD_AUDIO_LAYOUT_STEREO", "2"), ("AVD_AUDIO_LAYOUT_5POINT1", "6"), ("AVD_AUDIO_LAYOUT_7POINT1", "8"),
                        ("AVD_AUDIO_PLANAR", "0x100")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), header), name
    for text in ('"audio_layout"', '"audio_plane_stride"', "FL FR FC LFE BL BR SL SR", "unpinned", "6786, 6786, 9598, 0, 4799, 4799", "5249, 5249, 7422, 0, 3712, 3712, 3712, 3712",
                 "(sum_c w_c s_c + 16384) >> 15", "int32[12]"):
        assert text in flat, text
    assert "downmixes other layouts first" not in flat and "downmix other layouts first" not in flat
    assert re.search(r"#define\s+AVD_ABI_VERSION\s+3\b", header) and len(_lib.EXPORTS) == 43           # no function is added
    capi = open(os.path.join(CSRC, "avd_capi.hip")).read()
    for option in ("audio_layout", "audio_plane_stride"):
        assert re.search(r'\{"%s", &avd_ctx::%s, true,' % (option, option), capi), option
        assert '"%s: ' % option in capi                                                              # the refusal's message begins with the name
    assert '{"audio_layout", ctx->audio_layout_rec' in capi                                          # the debug buffer
    binding = open(os.path.join(ROOT, "ai-video-detector_amd", "avd_hip", "_lib.py")).read()
    for text in ('"audio_layout"', '"audio_plane_stride"'):
        assert text in binding, text
    assert _lib.Context.AUDIO_LAYOUTS == (1, 2, 6, 8) and _lib.Context.AUDIO_PLANAR == 0x100 == lay.PLANAR


# ---- weights -----------------------------------------------------------------------------------------------------------------------------------
def test_the_weights_come_from_the_gains_and_every_row_sums_to_32768():
    for layout in (1, 2, 6, 8):
        w = lay.derive(layout)
        assert w == lay.TABLE[layout] == host_audio.LAYOUT_WEIGHTS[layout] and sum(w) == 32768 and len(w) == layout
        channels, got = kit.weights(layout)
        assert channels == layout and tuple(got[:layout]) == w and not any(got[layout:])
    assert lay.TABLE[6][3] == 0 and lay.TABLE[8][3] == 0                                             # LFE
    assert kit.weights(3) == (0, [0] * 8)


def test_the_accumulator_stays_inside_32_bits_at_the_extremes():
    for layout in (1, 2, 6, 8):
        w = np.array(lay.TABLE[layout], np.int64)
        for s in (-32768, 32767):
            acc = int((w * s).sum()) + 16384
            assert abs(acc) < 2 ** 31 and abs(int((w * s).sum())) <= 2 ** 30
        assert lay.mix(np.full((1, layout), -32768), layout)[0] == -32768 and lay.mix(np.full((1, layout), 32767), layout)[0] == 32767


def test_layouts_1_and_2_are_the_existing_downmix_on_the_corners():
    edge = [-32768, -32767, -32766, -3, -2, -1, 0, 1, 2, 3, 32765, 32766, 32767]
    rng = np.random.default_rng(5)
    values = np.array(edge + list(rng.integers(-32768, 32768, 243)), np.int16)
    L, R = np.meshgrid(values, values, indexing="ij")
    pairs = np.stack([L.ravel(), R.ravel()], axis=1)                                                # 65536 pairs: every corner, both parities of L + R
    assert np.array_equal(lay.mix(pairs, 2), ref.downmix(pairs).astype(np.int16))
    assert np.array_equal(lay.mix(pairs, 2).astype(np.int64), (pairs[:, 0].astype(np.int64) + pairs[:, 1] + 1) >> 1)
    every = np.arange(-32768, 32768, dtype=np.int16)
    assert np.array_equal(lay.mix(every[:, None], 1), ref.downmix(every[:, None]).astype(np.int16))
    # float32 input: narrowing comes first, per sample
    x = np.array([[0.5, -0.5], [1.5, np.nan], [3.05e-5, 3.05e-5], [-1.0, 1.0], [np.inf, -np.inf]], np.float32)
    assert np.array_equal(lay.convert(x, 16000, 2), ref.convert(x, 16000))
    assert np.array_equal(lay.convert(np.ascontiguousarray(x.T), 16000, 2, planar=True), ref.convert(x, 16000))


# ---- the plan header -----------------------------------------------------------------------------------------------------------------------------
def test_every_check_of_the_program():
    status, out = kit.run()
    assert status == 0 and re.fullmatch(r"audio layout: \d+ checks, 0 failures\n", out), (status, out)
    assert int(out.split()[2]) > 2000


@pytest.mark.parametrize("rate", ref.RATES)
def test_the_lds_of_a_layout_launch_respects_the_bound(rate):
    layout, stereo, span = kit.lds(rate)
    assert layout <= stereo + 4 * span + 16, (rate, layout, stereo, span)
    assert layout <= 160 * 1024


def test_the_kernel_has_its_layout_instantiations_and_no_new_kernel_id():
    hip = open(os.path.join(CSRC, "avd_audio.hip")).read()
    for name in ("k_audio_resample_layout", "k_audio_resample_map_layout", "k_audio_slot_save_layout", "k_audio_slot_save_map_layout", "mix_span"):
        assert name in hip, name
    assert "lds_layout_bytes" in hip and "lds_layout_bytes" in open(kit.HEADER).read()


# ---- the Python helpers against a recording context ---------------------------------------------------------------------------------------------
class _FakeLibrary:
    def __init__(self, owner):
        self.owner = owner

    def avd_audio_features(self, h, ptr, mem, n, win, out_ptr, nwin):
        o = self.owner
        o.calls.append({"ptr": ptr, "mem": mem, "n": n, "win": win, "nwin": nwin, "cuts": list(o.cuts), "entries": list(o.entries), **o.options})
        o.cuts, o.entries = [], []
        if o.fail_call == len(o.calls):
            return -1
        rec = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_uint8 * (48 * nwin)).from_address(out_ptr)).view(_lib.AUDIO_WINDOW_DTYPE) if nwin else np.zeros(0, _lib.AUDIO_WINDOW_DTYPE)
        rec["length"] = len(o.calls)
        rec["nbins"] = np.arange(nwin)
        return 0


DEFAULTS = {"audio_format": 0, "audio_rate": 0, "audio_channels": 1, "audio_layout": 0, "audio_plane_stride": 0, "audio_slot": 0}


class Recorder(_lib.Context):
    """a Context without a library: what the audio helpers do above the C-ABI, call by call"""

    def __init__(self, fail_call=0, **options):
        self._h = None
        self.device = 0
        self.calls, self.cuts, self.entries, self.sets, self.gets = [], [], [], [], []
        self.options = {**DEFAULTS, **options}
        self.fail_call = fail_call
        self._L = _FakeLibrary(self)

    def _check(self, rc):
        if rc != 0:
            raise _lib.AvdError("avd status %d" % rc)

    def set_option(self, name, value):
        self.sets.append((name, value))
        if name == "audio_cut":
            self.cuts = [] if value == -1 else self.cuts + [value]
        elif name == "audio_track_slot":
            self.entries = [] if value == -1 else self.entries + [value]
        elif name in ("audio_end", "audio_slot_reset"):
            pass
        elif name == "audio_rate" and value != 0 and value not in ref.RATES:
            raise _lib.AvdError("audio_rate: refused")
        elif name == "audio_channels" and value not in (1, 2):
            raise _lib.AvdError("audio_channels: refused")
        elif name == "audio_layout" and value != 0 and (value & ~0x100) not in (1, 2, 6, 8):
            raise _lib.AvdError("audio_layout: refused")
        elif name == "audio_plane_stride" and value < 0:
            raise _lib.AvdError("audio_plane_stride: refused")
        else:
            self.options[name] = value

    def get_option(self, name):
        self.gets.append(name)
        if name in ("audio_slot_frames", "audio_slot_held", "audio_slot_windows"):
            return 0
        return len(self.cuts) if name == "audio_cut" else self.options[name]


def test_a_planar_call_sets_both_options_and_restores_them():
    r = Recorder()
    x = np.zeros((6, 96001), np.float32)
    out = r.audio_features(x, 8000, rate=48000, layout=6, planar=True)
    (call,) = r.calls
    assert (call["n"], call["audio_rate"], call["audio_layout"], call["audio_plane_stride"], call["audio_format"]) == (96001, 48000, 6 | 0x100, 96001, 0)
    assert call["ptr"] == x.ctypes.data and call["nwin"] == len(out) == 5
    assert r.options == DEFAULTS and ("audio_channels", 1) not in r.sets and not any(n == "audio_channels" for n, _ in r.sets)
    # interleaved 7.1, int16: frames of eight samples, no stride
    r = Recorder(audio_layout=2, audio_plane_stride=77)
    r.audio_features(np.zeros((30, 8), np.int16), 4, rate=16000, layout=8)
    assert (r.calls[0]["n"], r.calls[0]["audio_layout"], r.calls[0]["audio_plane_stride"], r.calls[0]["audio_format"], r.calls[0]["nwin"]) == (30, 8, 0, 1, 8)
    assert r.options == {**DEFAULTS, "audio_layout": 2, "audio_plane_stride": 77}                    # a caller's own values come back
    # flat interleaved
    r = Recorder()
    r.audio_features(np.zeros(60, np.int16), 4, rate=16000, layout=6)
    assert r.calls[0]["n"] == 10
    with pytest.raises(ValueError):
        r.audio_features(np.zeros(61, np.int16), 4, rate=16000, layout=6)
    with pytest.raises(ValueError):
        r.audio_features(np.zeros((30, 6), np.int16), 4, rate=16000, layout=8)
    with pytest.raises(ValueError):
        r.audio_features(np.zeros((6, 30), np.int16), 4, rate=16000, layout=8, planar=True)
    with pytest.raises(ValueError):
        r.audio_features(np.zeros((30, 5), np.int16), 4, rate=16000, layout=5)
    with pytest.raises(ValueError, match="rate"):
        r.audio_features(np.zeros((30, 6), np.int16), 4, layout=6)


def test_the_options_come_back_after_a_failure():
    r = Recorder(fail_call=1, audio_rate=44100, audio_layout=6, audio_plane_stride=9)
    with pytest.raises(_lib.AvdError):
        r.audio_features(np.zeros((2, 30), np.int16), 4, rate=48000, layout=2, planar=True)
    assert (r.calls[0]["audio_rate"], r.calls[0]["audio_layout"], r.calls[0]["audio_plane_stride"]) == (48000, 2 | 0x100, 30)
    assert r.options == {**DEFAULTS, "audio_rate": 44100, "audio_layout": 6, "audio_plane_stride": 9}
    r = Recorder()
    with pytest.raises(_lib.AvdError, match="audio_rate"):
        r.audio_features(np.zeros((2, 30), np.int16), 4, rate=44000, layout=2, planar=True)
    assert r.calls == [] and r.options == DEFAULTS and r.cuts == []


def test_nothing_new_is_touched_without_a_layout():
    r = Recorder()
    r.audio_features(np.zeros((20, 2), np.int16), 4, rate=48000)
    r.audio_features_many([np.zeros((20, 2), np.int16)] * 2, 4, rate=48000)
    r.audio_features(np.zeros(9, np.float32), 4)
    touched = {n for n, _ in r.sets} | set(r.gets)
    assert "audio_layout" not in touched and "audio_plane_stride" not in touched
    assert all(c["audio_layout"] == 0 and c["audio_plane_stride"] == 0 for c in r.calls)
    with pytest.raises(_lib.AvdError, match="audio_channels"):                                       # three columns without a layout: as ever
        r.audio_features(np.zeros((10, 3), np.int16), 4, rate=48000)
    with pytest.raises(ValueError):
        host_audio.analyze_decoded(np.zeros((10, 3), np.int16), 48000, Recorder())


def test_the_stride_is_taken_from_a_sliced_array():
    ring = np.zeros((6, 1000), np.int16)
    r = Recorder()
    r.audio_features(ring[:, 100:400], 4, rate=16000, layout=6, planar=True)
    (call,) = r.calls
    assert call["ptr"] == ring.ctypes.data + 200 and call["n"] == 300 and call["audio_plane_stride"] == 1000 and call["audio_layout"] == 6 | 0x100
    # rows that are not dense (every second sample), or a transposed view: copied dense, stride n
    r = Recorder()
    r.audio_features(ring[:, ::2], 4, rate=16000, layout=6, planar=True)
    assert r.calls[0]["n"] == 500 and r.calls[0]["audio_plane_stride"] == 500 and r.calls[0]["ptr"] != ring.ctypes.data
    r = Recorder()
    r.audio_features(np.zeros((300, 2), np.float32).T, 4, rate=16000, layout=2, planar=True)
    assert r.calls[0]["n"] == 300 and r.calls[0]["audio_plane_stride"] == 300
    # mono planar: one plane, [n] or [1, n]
    r = Recorder()
    r.audio_features(np.zeros(50, np.int16), 4, rate=16000, layout=1, planar=True)
    assert (r.calls[0]["n"], r.calls[0]["audio_layout"], r.calls[0]["audio_plane_stride"]) == (50, 1 | 0x100, 50)


def test_many_joins_planar_tracks_along_the_frame_axis():
    lens = [10, 3, 8, 1]
    r = Recorder()
    out = r.audio_features_many([np.zeros((6, n), np.int16) for n in lens], 2, rate=48000, layout=6, planar=True)
    (call,) = r.calls
    assert call["cuts"] == [10, 13, 21] and call["n"] == 22 and call["audio_plane_stride"] == 22 and call["audio_layout"] == 6 | 0x100
    assert [len(o) for o in out] == [2, 1, 2, 1] and r.options == DEFAULTS
    # more than 64 tracks: the second call begins 64 tracks further IN EACH PLANE, the stride stays the whole buffer's
    r = Recorder()
    r.audio_features_many([np.zeros((2, 7), np.float32)] * 70, 2, rate=8000, layout=2, planar=True)
    assert len(r.calls) == 2 and r.calls[1]["ptr"] - r.calls[0]["ptr"] == 64 * 7 * 4
    assert [c["audio_plane_stride"] for c in r.calls] == [490, 490] and [c["n"] for c in r.calls] == [448, 42]
    # interleaved 5.1: frames of six
    r = Recorder()
    r.audio_features_many([np.zeros((7, 6), np.float32)] * 70, 2, rate=8000, layout=6)
    assert r.calls[1]["ptr"] - r.calls[0]["ptr"] == 64 * 7 * 6 * 4 and r.calls[0]["audio_plane_stride"] == 0


def test_mapped_and_the_chunk_and_stream_helpers_pass_the_layout(monkeypatch):
    r = Recorder()
    out = r.audio_features_mapped([np.zeros((6, 40), np.int16), np.zeros((6, 24), np.int16)], [1, 0], [False, False], 4, rate=16000, layout=6, planar=True)
    (call,) = r.calls
    assert call["entries"] == [1, 0] and call["cuts"] == [40] and call["n"] == 64 and call["audio_plane_stride"] == 64 and call["audio_layout"] == 6 | 0x100
    assert [len(o) for o in out] == [10, 6] and r.options == DEFAULTS
    monkeypatch.setattr(host_audio, "features_to_result", lambda values, dur: {"dur": dur, "windows": len(values["rms"])})
    monkeypatch.setattr(host_audio, "window_values", lambda rec: {"rms": list(rec["nbins"])})
    r = Recorder()
    got = host_audio.analyze_decoded_chunks([np.zeros((8, 16000), np.float32), np.zeros((8, 8000), np.float32)], 16000, r, layout=8, planar=True)
    assert [c["n"] for c in r.calls] == [16000, 8000] and all(c["audio_layout"] == 8 | 0x100 and c["audio_slot"] == 1 for c in r.calls)
    assert got["dur"] == 1.5
    r = Recorder()
    got = host_audio.analyze_decoded_streams([[np.zeros((2, 16000), np.int16)], [np.zeros((2, 8000), np.int16), np.zeros((2, 0), np.int16)]], 16000, r, layout=2, planar=True)
    assert [c["n"] for c in r.calls] == [24000] and r.calls[0]["audio_layout"] == 2 | 0x100 and [g["dur"] for g in got] == [1.0, 0.5]
    r = Recorder()
    got = host_audio.analyze_decoded_many([(np.zeros((48000, 6), np.int16), 48000), (np.zeros((24000, 6), np.int16), 48000)], r, layout=6)
    assert len(r.calls) == 1 and r.calls[0]["audio_layout"] == 6 and r.calls[0]["cuts"] == [48000] and [g["dur"] for g in got] == [1.0, 0.5]
    one = host_audio.analyze_decoded(np.zeros((6, 44100), np.float32), 44100, Recorder(), layout=6, planar=True)
    assert one == {"dur": 1.0, "windows": 2}


def test_layout_of():
    assert [host_audio.layout_of(c) for c in (1, 2, 6, 8)] == [1, 2, 6, 8]
    for c in (0, 3, 4, 5, 7, 9, 0x102):
        with pytest.raises(ValueError):
            host_audio.layout_of(c)
    with pytest.raises(ValueError):
        host_audio.analyze_decoded(np.zeros((6, 10), np.int16), 48000, Recorder(), planar=True)      # planar needs a layout


# ---- the drop-in ---------------------------------------------------------------------------------------------------------------------------------
def _write_wav(path, channels, frames=4800, rate=48000):
    pcm = (np.arange(frames * channels, dtype=np.int64) * 37 % 2001 - 1000).astype("<i2").reshape(frames, channels)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(pcm.tobytes())
    return pcm


def test_the_drop_in_takes_surround_files_only_with_both_variables(tmp_path, monkeypatch):
    from app.analyzers import audio as dropin
    path = tmp_path / "surround.wav"
    pcm = _write_wav(path, 6)
    monkeypatch.delenv("AVD_AUDIO_LAYOUT", raising=False)
    assert dropin._channel_counts() == (1, 2) and dropin._read_decoded(str(path)) is None and dropin._chunked_rate(str(path)) is None
    monkeypatch.setenv("AVD_AUDIO_LAYOUT", "1")
    frames, sr = dropin._read_decoded(str(path))
    assert sr == 48000 and np.array_equal(frames, pcm) and dropin._chunked_rate(str(path)) == (48000, 6)
    assert dropin._layout_kw(6) == {"layout": 6} and dropin._layout_kw(8) == {"layout": 8} and dropin._layout_kw(2) == {} and dropin._layout_kw(1) == {}
    _write_wav(tmp_path / "five.wav", 5)
    assert dropin._read_decoded(str(tmp_path / "five.wav")) is None                                  # no layout of five channels
    # analyze(): with AVD_AUDIO_RESAMPLE and AVD_AUDIO_LAYOUT the file goes to analyze_decoded with its layout; without the second it does not
    seen = []

    class _Pool:
        def borrow(self, device):
            import contextlib
            return contextlib.nullcontext("ctx")

    monkeypatch.setattr(dropin._analyzer, "default_pool", lambda: _Pool())
    monkeypatch.setattr(dropin._audio, "analyze_decoded", lambda wav, sr, ctx, **kw: seen.append((wav.shape, sr, kw)) or {"ok": 1})
    monkeypatch.setattr(dropin._audio, "extract_wav_16k", lambda path, native=False: (_ for _ in ()).throw(RuntimeError("ffmpeg_convert_failed")))
    monkeypatch.setenv("AVD_AUDIO_RESAMPLE", "1")
    assert dropin.analyze(str(path), {"duration": 0.1}) == {"ok": 1} and seen == [((4800, 6), 48000, {"layout": 6})]
    monkeypatch.delenv("AVD_AUDIO_LAYOUT")
    assert dropin.analyze(str(path), {"duration": 0.1})["flags_audio"] == {"error": "ffmpeg_convert_failed"} and len(seen) == 1
    monkeypatch.setenv("AVD_AUDIO_LAYOUT", "1")
    monkeypatch.delenv("AVD_AUDIO_RESAMPLE")
    assert dropin.analyze(str(path), {"duration": 0.1})["flags_audio"] == {"error": "ffmpeg_convert_failed"} and len(seen) == 1
