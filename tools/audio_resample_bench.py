#!/usr/bin/env python3
"""Tracks at the decoder's rate (options "audio_rate" / "audio_channels"): what the converter in front of the audio analyzer costs, one run on an
MI355X -> profiles/audio_resample.json.

    python tools/audio_resample_bench.py --parent-lib PATH/libavd_hip.so [--rounds 9] [--out profiles/audio_resample.json]

--parent-lib is the library of the PARENT commit, built from a checkout of it (make -C ai-video-detector_amd/csrc): the no-regression
figures compare with the parent's code, never with the code under test.  Without it those columns are left out and the file says so.

Every figure is the median over --rounds rounds, with the smallest and the largest, after two unrecorded rounds; variants that are compared
run in alternation inside a round.  Milliseconds.

  * converted: a 60 s stereo int16 track at 48000 and at 44100, from pageable host memory and from device memory: wall clock of the blocking
    call; and "stream_ms", the context's stream between two events around the call (device input: no staging copy in it).
  * ready_16k: the SAME 60 s as a ready 16 kHz int16 track (the converter's own output) through this build and through the parent's library,
    the same two ways.  converter_stream_ms = converted stream_ms - ready_16k stream_ms of this build, round by round: the converter's launch
    with its tile-table upload, set against the bytes it moves (input read + output written).
  * batch: thirteen 10 s tracks at 44100 in one call (twelve cuts), per track.
  * no_regression: with "audio_rate" 0, one 16 kHz float32 track of 60 s through this build and the parent's, alternating, records compared
    byte for byte.
  * cpu_restatement: tests/audio_resample_reference.py on the same 48000 track, once, as context only.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ai-video-detector_amd"))
sys.path.insert(0, ROOT)

WIN, OUT_RATE, SECONDS = 8000, 16000, 60


class Lib:
    """the entry points the measurement needs, bound from any libavd_hip.so"""

    def __init__(self, path):
        self.L = L = C.CDLL(path)
        vp = C.c_void_p
        L.avd_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.avd_destroy.argtypes = [vp]
        L.avd_last_error.argtypes = [vp]
        L.avd_last_error.restype = C.c_char_p
        L.avd_set_option.argtypes = [vp, C.c_char_p, C.c_int]
        L.avd_audio_features.argtypes = [vp, vp, C.c_int, C.c_int64, C.c_int, vp, C.c_int]
        L.avd_timer_start.argtypes = [vp]
        L.avd_timer_stop.argtypes = [vp, C.POINTER(C.c_float)]
        L.avd_debug_fetch.argtypes = [vp, C.c_char_p, vp, C.c_size_t]
        L.avd_debug_fetch.restype = C.c_int64
        self.h = vp()
        if L.avd_create(0, C.byref(self.h)) != 0:
            raise SystemExit("avd_create failed: no usable HIP device")

    def close(self):
        self.L.avd_destroy(self.h)

    def check(self, rc):
        if rc != 0:
            raise SystemExit("avd status %d: %s" % (rc, (self.L.avd_last_error(self.h) or b"").decode()))

    def option(self, name, value):
        self.check(self.L.avd_set_option(self.h, name.encode(), int(value)))

    def call(self, ptr, mem, n, out, fmt, rate=0, channels=1, cuts=()):
        """-> (wall clock ms, stream ms) of one blocking avd_audio_features call"""
        self.option("audio_format", fmt)
        if rate:
            self.option("audio_rate", rate)
            self.option("audio_channels", channels)
        for c in cuts:
            self.option("audio_cut", c)
        ms = C.c_float()
        self.check(self.L.avd_timer_start(self.h))
        t0 = time.perf_counter()
        rc = self.L.avd_audio_features(self.h, ptr, mem, n, WIN, out.ctypes.data, len(out))
        wall = (time.perf_counter() - t0) * 1e3
        self.check(rc)
        self.check(self.L.avd_timer_stop(self.h, C.byref(ms)))
        if rate:
            self.option("audio_rate", 0)
            self.option("audio_channels", 1)
        self.option("audio_format", 0)
        return wall, float(ms.value)

    def pcm(self, n_out):
        v = np.zeros(n_out, np.int16)
        got = self.L.avd_debug_fetch(self.h, b"audio_pcm", v.ctypes.data, v.nbytes)
        assert got == v.nbytes, got
        return v


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def stereo_track(rate, seconds, rng):
    n = rate * seconds + 37
    t = np.arange(n)[:, None]
    x = 0.3 * np.sin(2 * np.pi * np.array([220.0, 330.0])[None, :] * t / rate) + 0.05 * rng.standard_normal((n, 2))
    return np.clip(np.rint(x * 32768), -32768, 32767).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_resample.json"))
    a = ap.parse_args()
    import torch
    from avd_hip import _lib
    _lib.build()
    new = Lib(_lib.SO_PATH)
    old = Lib(a.parent_lib) if a.parent_lib else None
    rec_dtype = _lib.AUDIO_WINDOW_DTYPE
    rng = np.random.default_rng(0)
    n_out_of = _lib.Context.audio_converted_length
    result = {"device": "MI355X", "win": WIN, "rounds": a.rounds, "unit": "ms; median, min and max over the rounds",
              "baseline": "the parent commit's library" if old else "none: --parent-lib was not given", "converted": [], "ready_16k": []}
    for rate in (48000, 44100):
        wav = stereo_track(rate, SECONDS, rng)
        n, n_out = len(wav), n_out_of(len(wav), rate)
        dev = torch.from_numpy(wav).cuda()
        out = np.zeros(-(-n_out // WIN), rec_dtype)
        new.call(wav.ctypes.data, 0, n, out, 1, rate, 2)
        ready = new.pcm(n_out)                                                   # the same 60 s as a ready 16 kHz track
        want = out.copy()
        ready_dev = torch.from_numpy(ready).cuda()
        torch.cuda.synchronize()
        libs = [("this_build", new)] + ([("parent", old)] if old else [])
        times = {}
        for r in range(a.rounds + 2):
            for where, ptr, rptr, mem in (("host", wav.ctypes.data, ready.ctypes.data, 0), ("device", dev.data_ptr(), ready_dev.data_ptr(), 1)):
                got = {("converted", where): new.call(ptr, mem, n, out, 1, rate, 2)}
                assert out.tobytes() == want.tobytes()
                for name, lib in libs:
                    got[(name, where)] = lib.call(rptr, mem, n_out, out, 1)
                    assert out.tobytes() == want.tobytes(), "the records of the ready track differ from the converted call's"
                got[("converter", where)] = (0.0, got[("converted", where)][1] - got[("this_build", where)][1])
                if r >= 2:
                    for k, v in got.items():
                        times.setdefault(k, ([], []))
                        times[k][0].append(v[0]); times[k][1].append(v[1])
        moved = wav.nbytes + 2 * n_out
        for where in ("host", "device"):
            conv = spread(times[("converter", where)][1])
            row = {"rate": rate, "channels": 2, "type": "int16", "seconds": SECONDS, "memory": where, "input_bytes": int(wav.nbytes), "output_samples": int(n_out),
                   "wall_ms": spread(times[("converted", where)][0]), "stream_ms": spread(times[("converted", where)][1]),
                   "converter_stream_ms": conv, "converter_bytes_moved": int(moved),
                   "converter_GB_per_s_at_median": round(moved / 1e9 / (conv["median"] / 1e3), 1) if conv["median"] > 0 else None}
            result["converted"].append(row)
            print(json.dumps(row), flush=True)
            row = {"rate": OUT_RATE, "from_rate": rate, "memory": where, "samples": int(n_out),
                   **{name: {"wall_ms": spread(times[(name, where)][0]), "stream_ms": spread(times[(name, where)][1])} for name, _ in libs}}
            result["ready_16k"].append(row)
            print(json.dumps(row), flush=True)
        if rate == 48000:
            from tests import audio_resample_reference as ref
            t0 = time.perf_counter()
            cpu = ref.convert(wav, rate)
            result["cpu_restatement_48000_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            assert np.array_equal(cpu, ready), "the converted track differs from the restatement"
    # thirteen 10 s tracks at 44100 in one call
    tracks = [stereo_track(44100, 10, rng)[:441000 + 3 * k] for k in range(13)]
    whole = np.concatenate(tracks)
    cuts = np.cumsum([len(t) for t in tracks])[:-1].tolist()
    out = np.zeros(sum(-(-n_out_of(len(t), 44100) // WIN) for t in tracks), rec_dtype)
    batch = [new.call(whole.ctypes.data, 0, len(whole), out, 1, 44100, 2, cuts)[0] / 13 for _ in range(a.rounds + 2)][2:]
    result["batch_13x10s_44100_host_wall_ms_per_track"] = spread(batch)
    print(json.dumps(result["batch_13x10s_44100_host_wall_ms_per_track"]), flush=True)
    # audio_rate 0: one 16 kHz float32 track, this build against the parent
    flt = (0.3 * rng.standard_normal(SECONDS * OUT_RATE + 37)).astype(np.float32)
    out_new, out_old = (np.zeros(-(-len(flt) // WIN), rec_dtype) for _ in range(2))
    t_new, t_old = [], []
    for r in range(a.rounds + 2):
        w = new.call(flt.ctypes.data, 0, len(flt), out_new, 0)[0]
        if r >= 2:
            t_new.append(w)
        if old:
            w = old.call(flt.ctypes.data, 0, len(flt), out_old, 0)[0]
            assert out_new.tobytes() == out_old.tobytes(), "audio_rate 0: the records differ from the parent's"
            if r >= 2:
                t_old.append(w)
    result["no_regression_16k_float32_60s_host_wall_ms"] = {"this_build": spread(t_new), **({"parent": spread(t_old), "records": "byte-identical"} if old else {})}
    print(json.dumps(result["no_regression_16k_float32_60s_host_wall_ms"]), flush=True)
    new.close()
    if old:
        old.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
