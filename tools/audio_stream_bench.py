#!/usr/bin/env python3
"""A track continued across avd_audio_features calls (option "audio_slot"): what the calls cost, one run on an MI355X -> profiles/audio_stream.json.

    python tools/audio_stream_bench.py --parent-lib PATH/libavd_hip.so [--rounds 5] [--out profiles/audio_stream.json]

--parent-lib is the library of the PARENT commit, built from a checkout of it (make -C ai-video-detector_amd/csrc): the no-regression figures
compare with the parent's code, never with the code under test.  Without it those parts are left out and the file says so.

Every figure is the median over --rounds rounds, with the smallest and the largest, after one unrecorded round.  Milliseconds, wall clock of the
blocking calls.  Nothing here is a gate; the per-chunk figure is expected to be launch-bound and is reported as found.

  * stream: a 60 s 48 kHz stereo int16 track whole (slot 0), then through audio slot 1 in chunks of 1 s, 0.5 s and 4096 frames, from pageable
    host memory and from device memory: "per_track_ms" (all calls of the track, the option calls included) and "per_call_ms" (that over the
    number of calls).  The concatenated records of every chunked track are compared with the whole call's, byte for byte.
  * slot_0: the whole call through this build and through the parent's library, alternating, records compared byte for byte; the condition is
    that this build's median lies inside the parent's own spread of the same run.
  * bench: `python bench.py --gpus 1 --steps K --warmup W` under this build and under the parent's library, alternating, each run a process of
    its own.
"""
import argparse
import ctypes as C
import json
import os
import runpy
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ai-video-detector_amd"))
sys.path.insert(0, ROOT)

WIN, RATE, SECONDS = 8000, 48000, 60
CHUNKS = (("1 s", 48000), ("0.5 s", 24000), ("4096 frames", 4096))


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

    def whole(self, ptr, mem, n, out):
        """one slot-0 call -> wall clock ms"""
        t0 = time.perf_counter()
        rc = self.L.avd_audio_features(self.h, ptr, mem, n, WIN, out.ctypes.data, len(out))
        ms = (time.perf_counter() - t0) * 1e3
        self.check(rc)
        return ms

    def chunked(self, ptr, mem, n, frame_bytes, chunk, out):
        """the track through audio slot 1 in calls of `chunk` frames, the last one marked -> (wall clock ms of the track, calls, records written)"""
        at, calls, wrote = 0, 0, 0
        t0 = time.perf_counter()
        self.option("audio_slot", 1)
        while at < n:
            m = min(chunk, n - at)
            if at + m == n:
                self.option("audio_end", 1)
            rc = self.L.avd_audio_features(self.h, ptr + at * frame_bytes, mem, m, WIN, out.ctypes.data + wrote * out.itemsize, len(out) - wrote)
            if rc != 0:
                self.option("audio_slot", 0)
                self.check(rc)
            # a record that was written has length >= 1; the array starts as zeros
            while wrote < len(out) and out["length"][wrote] > 0:
                wrote += 1
            at += m
            calls += 1
        self.option("audio_slot", 0)
        return (time.perf_counter() - t0) * 1e3, calls, wrote


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def stereo_track(rate, seconds, rng):
    n = rate * seconds + 37
    t = np.arange(n)[:, None]
    x = 0.3 * np.sin(2 * np.pi * np.array([220.0, 330.0])[None, :] * t / rate) + 0.05 * rng.standard_normal((n, 2))
    return np.clip(np.rint(x * 32768), -32768, 32767).astype(np.int16)


def child_bench(a):
    """bench.py as it is, under the given library; its one JSON line goes out as it comes"""
    from avd_hip import _lib
    if a.lib:
        _lib.SO_PATH = os.path.abspath(a.lib)              # another build of the library under the same binding
    sys.argv = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup)]
    runpy.run_path(sys.argv[0], run_name="__main__")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_stream.json"))
    ap.add_argument("--child-bench", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_bench:
        return child_bench(a)
    import torch
    from avd_hip import _lib
    _lib.build()
    new = Lib(_lib.SO_PATH)
    old = Lib(a.parent_lib) if a.parent_lib else None
    rec_dtype = _lib.AUDIO_WINDOW_DTYPE
    wav = stereo_track(RATE, SECONDS, np.random.default_rng(0))
    n, n_out = len(wav), _lib.Context.audio_converted_length(len(wav), RATE)
    dev = torch.from_numpy(wav).cuda()
    torch.cuda.synchronize()
    nwin = -(-n_out // WIN)
    result = {"device": "MI355X", "track": "%d s, %d Hz, stereo int16, %d frames" % (SECONDS, RATE, n), "win": WIN, "windows": nwin, "rounds": a.rounds,
              "unit": "ms, wall clock of the blocking calls; median, min and max over the rounds",
              "baseline": "the parent commit's library" if old else "none: --parent-lib was not given", "stream": []}
    for lib in [new] + ([old] if old else []):
        lib.option("audio_format", 1)
        lib.option("audio_rate", RATE)
        lib.option("audio_channels", 2)
    want = np.zeros(nwin, rec_dtype)
    new.whole(wav.ctypes.data, 0, n, want)
    # ---- the track whole and in chunks, through this build ----
    for where, ptr, mem in (("host", wav.ctypes.data, 0), ("device", dev.data_ptr(), 1)):
        rows = {"whole": ([], 1)}
        for r in range(a.rounds + 1):
            out = np.zeros(nwin, rec_dtype)
            ms = new.whole(ptr, mem, n, out)
            assert out.tobytes() == want.tobytes()
            if r >= 1:
                rows["whole"][0].append(ms)
            for name, chunk in CHUNKS:
                out = np.zeros(nwin + 1, rec_dtype)
                ms, calls, wrote = new.chunked(ptr, mem, n, 4, chunk, out)
                assert wrote == nwin and out[:nwin].tobytes() == want.tobytes(), "the chunked track's records differ from the whole call's (%s, %s)" % (name, where)
                rows.setdefault(name, ([], calls))
                if r >= 1:
                    rows[name][0].append(ms)
        for name, (ms, calls) in rows.items():
            row = {"split": name, "memory": where, "calls": calls, "per_track_ms": spread(ms), "per_call_ms": spread([m / calls for m in ms]),
                   "records": "byte-identical to the whole call's"}
            result["stream"].append(row)
            print(json.dumps(row), flush=True)
    # ---- slot 0: this build against the parent, alternating ----
    if old:
        slot0 = {}
        for where, ptr, mem in (("host", wav.ctypes.data, 0), ("device", dev.data_ptr(), 1)):
            t_new, t_old = [], []
            for r in range(a.rounds + 1):
                out_new, out_old = np.zeros(nwin, rec_dtype), np.zeros(nwin, rec_dtype)
                a_ms, b_ms = new.whole(ptr, mem, n, out_new), old.whole(ptr, mem, n, out_old)
                assert out_new.tobytes() == out_old.tobytes() == want.tobytes(), "slot 0: the records differ from the parent's"
                if r >= 1:
                    t_new.append(a_ms); t_old.append(b_ms)
            s_new, s_old = spread(t_new), spread(t_old)
            slot0[where] = {"this_build": s_new, "parent": s_old, "records": "byte-identical",
                            "this_build_median_within_parent_range": bool(s_old["min"] <= s_new["median"] <= s_old["max"])}
        result["slot_0_whole_call_ms"] = slot0
        print(json.dumps(slot0), flush=True)
    new.close()
    if old:
        old.close()
    del dev
    # ---- bench.py, each run a process of its own: nothing more is started on the device after one that fails ----
    if not a.no_bench:
        forms = [("this_build", None)] + ([("parent", a.parent_lib)] if a.parent_lib else [])
        runs = {}
        for r in range(a.rounds):
            for form, lib in forms[r % len(forms):] + forms[:r % len(forms)]:
                cmd = [sys.executable, os.path.abspath(__file__), "--child-bench", "--bench-steps", str(a.bench_steps), "--bench-warmup", str(a.bench_warmup)]
                if lib:
                    cmd += ["--lib", lib]
                got = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=300)
                line = json.loads(got.stdout.decode().strip().splitlines()[-1])
                runs.setdefault(form, []).append(line)
                print("round %d %s bench: %s" % (r, form, json.dumps(line)[:200]), file=sys.stderr, flush=True)
        bench = {form: {"value_median": statistics.median(x["value"] for x in v), "value_rounds": [x["value"] for x in v], "unit": v[0].get("unit")} for form, v in runs.items()}
        if "parent" in bench:
            lo, hi = min(bench["parent"]["value_rounds"]), max(bench["parent"]["value_rounds"])
            bench["this_build_median_within_parent_range"] = bool(lo <= bench["this_build"]["value_median"] <= hi)
        result["bench"] = bench
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
