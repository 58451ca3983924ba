#!/usr/bin/env python3
"""Several audio tracks per call against one call per track, 16-bit PCM against float32, and the host's share: one run on an MI355X ->
profiles/audio_batch.json.

    python tools/audio_batch_bench.py --parent-lib PATH/libavd_hip.so [--rounds 9] [--out profiles/audio_batch.json]

--parent-lib is the library of the PARENT commit, built from a checkout of it (make -C ai-video-detector_amd/csrc): the baseline of every
"in turn" figure is the parent's code, never the code under test.  Without it those columns are left out and the file says so.

What is measured, as wall-clock time of the blocking calls from pageable host memory (what a service pays), in milliseconds per track:

  * K = 1, 4, 13, 32 tracks of 10 s and of 60 s at 16 kHz, win = 8000.  Track k is 3 k + 1 samples longer than a whole number of windows, so
    every track ends in a short window of its own length, as files of a service do; and K = 13 once more with tails of 4001 + 3 k samples,
    where the short windows' tables are as large as a service's typically are (half a window);
      batch     one avd_audio_features call with K - 1 cuts           (this tree's library)
      in_turn   K calls, one per track                                (this tree's library)
      parent    K calls, one per track                                (the parent's library)
    The three are run in alternation, round after round, after two unrecorded rounds; the file keeps the median and the spread over rounds.
  * int16 PCM against float32 for one 60 s track, alternating.
  * debug buffer "audio_host": the microseconds the host spent forming the tables of the short lengths in the last call.
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

WIN, RATE = 8000, 16000
KS = (1, 4, 13, 32)
SECONDS = (10, 60)


class Lib:
    """the four entry points the measurement needs, bound from any libavd_hip.so"""

    def __init__(self, path):
        self.L = L = C.CDLL(path)
        vp = C.c_void_p
        L.avd_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.avd_destroy.argtypes = [vp]
        L.avd_last_error.argtypes = [vp]
        L.avd_last_error.restype = C.c_char_p
        L.avd_set_option.argtypes = [vp, C.c_char_p, C.c_int]
        L.avd_audio_features.argtypes = [vp, vp, C.c_int, C.c_int64, C.c_int, vp, C.c_int]
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

    def features(self, wav, out, cuts=()):
        for c in cuts:
            self.option("audio_cut", c)
        self.check(self.L.avd_audio_features(self.h, wav.ctypes.data, 0, wav.size, WIN, out.ctypes.data, len(out)))

    def host_us(self):
        v = np.zeros(2, np.int32)
        got = self.L.avd_debug_fetch(self.h, b"audio_host", v.ctypes.data, v.nbytes)
        return [int(x) for x in v] if got == v.nbytes else None


def make_tracks(k, seconds, tail, rng):
    return [(0.3 * rng.standard_normal(seconds * RATE + tail + 3 * i)).astype(np.float32) for i in range(k)]


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_batch.json"))
    a = ap.parse_args()
    from avd_hip import _lib
    _lib.build()
    new = Lib(_lib.SO_PATH)
    old = Lib(a.parent_lib) if a.parent_lib else None
    rec_dtype = _lib.AUDIO_WINDOW_DTYPE
    rng = np.random.default_rng(0)
    result = {"device": "MI355X", "win": WIN, "rounds": a.rounds, "unit": "ms per track, wall clock of the blocking calls, pageable host memory",
              "baseline": "in_turn on the parent commit's library" if old else "none: --parent-lib was not given", "per_track": []}
    # (seconds, tracks, samples the first track has beyond a whole number of windows)
    cases = [(seconds, k, 1) for seconds in SECONDS for k in KS] + [(seconds, 13, 4001) for seconds in SECONDS]
    for seconds, k, tail in cases:
        tracks = make_tracks(k, seconds, tail, rng)
        whole = np.concatenate(tracks)
        cuts = np.cumsum([len(t) for t in tracks])[:-1].tolist()
        counts = [-(-len(t) // WIN) for t in tracks]
        out_all = np.zeros(sum(counts), rec_dtype)
        outs = [np.zeros(c, rec_dtype) for c in counts]

        def batch():
            new.features(whole, out_all, cuts)

        def in_turn(lib):
            for t, o in zip(tracks, outs):
                lib.features(t, o)

        variants = [("batch", batch), ("in_turn", lambda: in_turn(new))] + ([("parent", lambda: in_turn(old))] if old else [])
        times = {name: [] for name, _ in variants}
        host = []
        for r in range(a.rounds + 2):
            for name, run in variants:
                t0 = time.perf_counter()
                run()
                dt = (time.perf_counter() - t0) * 1e3 / k
                if r >= 2:
                    times[name].append(dt)
                    if name == "batch":
                        host.append(new.host_us()[0] / 1e3 / k)
        # the batch is the same numbers as the calls in turn, and the parent's: checked on the last round's outputs
        want = np.concatenate(outs)
        assert out_all.tobytes() == want.tobytes(), "the batch's records differ from the per-track calls'"
        row = {"seconds": seconds, "tracks": k, "first_tail": tail, **{name: spread(ms) for name, ms in times.items()}, "batch_table_host": spread(host)}
        row["in_turn_over_batch"] = round(row["in_turn"]["median"] / row["batch"]["median"], 3)
        if old:
            row["parent_over_batch"] = round(row["parent"]["median"] / row["batch"]["median"], 3)
            row["parent_over_in_turn"] = round(row["parent"]["median"] / row["in_turn"]["median"], 3)
        result["per_track"].append(row)
        print(json.dumps(row), flush=True)
    # int16 against float32, one 60 s track
    pcm = rng.integers(-20000, 20000, 60 * RATE + 37).astype(np.int16)
    flt = pcm.astype(np.float32) * np.float32(2.0 ** -15)
    out_i, out_f = (np.zeros(-(-len(pcm) // WIN), rec_dtype) for _ in range(2))
    t_i, t_f = [], []
    for r in range(a.rounds + 2):
        new.option("audio_format", 1)
        t0 = time.perf_counter(); new.features(pcm, out_i); dt_i = (time.perf_counter() - t0) * 1e3
        new.option("audio_format", 0)
        t0 = time.perf_counter(); new.features(flt, out_f); dt_f = (time.perf_counter() - t0) * 1e3
        if r >= 2:
            t_i.append(dt_i); t_f.append(dt_f)
    assert out_i.tobytes() == out_f.tobytes(), "int16 records differ from their float32 form's"
    result["pcm16_60s"] = {"int16": spread(t_i), "float32": spread(t_f), "bytes_staged": {"int16": int(pcm.nbytes), "float32": int(flt.nbytes)},
                           "float32_over_int16": round(statistics.median(t_f) / statistics.median(t_i), 3)}
    print(json.dumps(result["pcm16_60s"]), flush=True)
    new.close()
    if old:
        old.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
