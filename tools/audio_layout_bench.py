#!/usr/bin/env python3
"""Planar and 5.1 tracks as the decoder hands them over (options "audio_layout" / "audio_plane_stride"): what the layout source phase of the
converter costs, one run on an MI355X -> profiles/audio_layout.json.

    python tools/audio_layout_bench.py --parent-lib PATH/libavd_hip.so [--runs 5] [--out profiles/audio_layout.json]

--parent-lib is the library of the PARENT commit, built from a checkout of it (make -C ai-video-detector_amd/csrc): the comparisons are with the
parent's code, never with the code under test.

Workloads: a 60 s track at 48 kHz, and thirteen 10 s tracks in one call ("audio_cut"), each from device memory and from pageable host memory.
Per workload, after two unrecorded rounds, --runs rounds in which every variant runs once, in alternation.  A figure is the wall clock of the
blocking call in milliseconds (median, min, max), host work of the variant included:

  (a) interleaved stereo, int16 and float32, by "audio_channels" 2: the parent's library and this build.  The records are compared by SHA-256.
  (b) planar stereo on this build ("audio_layout" 2 | 0x100), int16 and float32 -- and what the parent's user must do with the same planar
      buffer: transpose it to interleaved (numpy on the host, torch on the device) and make call (a).
  (c) planar 5.1 float32 on this build ("audio_layout" 6 | 0x100) -- and the parent's way: a float downmix to mono (numpy / torch, the layout's
      gains) and the parent's mono call.  (The parent's result is a float mix narrowed afterwards: close to, not equal to, the stated rule.)

Gates, evaluated here and written into the file:
  * (a) on this build lies inside the parent's own range: its median is at most the parent's maximum; records byte-identical.
  * planar stereo from device memory takes no longer than the parent's interleaved stereo maximum plus the parent's own spread (max - min of
    its runs): it reads the same bytes once.
The 5.1 and transpose comparisons are reported, not gated."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ai-video-detector_amd"))
sys.path.insert(0, ROOT)

WIN, RATE, PLANAR = 8000, 48000, 0x100
GAINS_5POINT1 = np.array([np.sqrt(0.5), np.sqrt(0.5), 1.0, 0.0, 0.5, 0.5])


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

    def call(self, ptr, mem, n, out, fmt, channels=1, layout=0, cuts=()):
        """one blocking avd_audio_features call at RATE; layout 0: by "audio_channels" """
        self.option("audio_format", fmt)
        self.option("audio_rate", RATE)
        if layout:
            self.option("audio_layout", layout)
        else:
            self.option("audio_channels", channels)
        for c in cuts:
            self.option("audio_cut", c)
        self.check(self.L.avd_audio_features(self.h, ptr, mem, n, WIN, out.ctypes.data, len(out)))
        if layout:
            self.option("audio_layout", 0)


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def make_tracks(lens, channels, rng):
    """[sum(lens), channels] int16 and float32: tones plus noise"""
    n = sum(lens)
    t = np.arange(n)[:, None]
    x = 0.25 * np.sin(2 * np.pi * (200.0 + 55.0 * np.arange(channels))[None, :] * t / RATE) + 0.05 * rng.standard_normal((n, channels))
    f = x.astype(np.float32)
    return np.clip(np.rint(x * 32768), -32768, 32767).astype(np.int16), f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_layout.json"))
    a = ap.parse_args()
    import torch
    from avd_hip import _lib
    _lib.build()
    new, old = Lib(_lib.SO_PATH), Lib(a.parent_lib)
    rec_dtype = _lib.AUDIO_WINDOW_DTYPE
    n_out_of = _lib.Context.audio_converted_length
    rng = np.random.default_rng(0)
    result = {"device": "MI355X", "rate": RATE, "win": WIN, "runs": a.runs, "unit": "ms, wall clock of the blocking call with the variant's host work; median, min, max",
              "baseline": "the parent commit's library", "workloads": [], "gates": {}}
    gates_ok = True
    workloads = (("track_60s", [60 * RATE + 37]), ("batch_13x10s", [10 * RATE + 3 * k + 1 for k in range(13)]))
    for name, lens in workloads:
        n = sum(lens)
        cuts = np.cumsum(lens)[:-1].tolist()
        out = np.zeros(sum(-(-n_out_of(m, RATE) // WIN) for m in lens), rec_dtype)
        s16, f32 = make_tracks(lens, 2, rng)
        _, six = make_tracks(lens, 6, rng)
        host = {"i_s16": s16, "i_f32": f32, "p_s16": np.ascontiguousarray(s16.T), "p_f32": np.ascontiguousarray(f32.T), "p6_f32": np.ascontiguousarray(six.T)}
        dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
        gains_host = (GAINS_5POINT1 / GAINS_5POINT1.sum()).astype(np.float32)
        gains_dev = torch.from_numpy(gains_host).cuda()
        torch.cuda.synchronize()
        for where in ("device", "host"):
            mem = 1 if where == "device" else 0
            buf = dev if where == "device" else host
            ptr = (lambda k: buf[k].data_ptr()) if where == "device" else (lambda k: buf[k].ctypes.data)

            def transposed(k):
                if where == "device":
                    t = buf[k].t().contiguous()
                    torch.cuda.synchronize()
                    return t, t.data_ptr()
                t = np.ascontiguousarray(buf[k].T)
                return t, t.ctypes.data

            def downmixed():
                if where == "device":
                    t = (gains_dev[:, None] * buf["p6_f32"]).sum(0).contiguous()
                    torch.cuda.synchronize()
                    return t, t.data_ptr()
                t = np.ascontiguousarray(gains_host @ buf["p6_f32"])
                return t, t.ctypes.data

            def parent_transpose(k, fmt):
                keep, p = transposed(k)
                old.call(p, mem, n, out, fmt, 2, 0, cuts)

            def parent_downmix():
                keep, p = downmixed()
                old.call(p, mem, n, out, 0, 1, 0, cuts)

            variants = [
                ("a_interleaved_s16_parent", lambda: old.call(ptr("i_s16"), mem, n, out, 1, 2, 0, cuts), "s16"),
                ("a_interleaved_s16_this_build", lambda: new.call(ptr("i_s16"), mem, n, out, 1, 2, 0, cuts), "s16"),
                ("a_interleaved_f32_parent", lambda: old.call(ptr("i_f32"), mem, n, out, 0, 2, 0, cuts), "f32"),
                ("a_interleaved_f32_this_build", lambda: new.call(ptr("i_f32"), mem, n, out, 0, 2, 0, cuts), "f32"),
                ("b_planar_s16_this_build", lambda: new.call(ptr("p_s16"), mem, n, out, 1, 2, 2 | PLANAR, cuts), "s16"),
                ("b_planar_f32_this_build", lambda: new.call(ptr("p_f32"), mem, n, out, 0, 2, 2 | PLANAR, cuts), "f32"),
                ("b_planar_s16_parent_transpose_then_a", lambda: parent_transpose("p_s16", 1), "s16"),
                ("b_planar_f32_parent_transpose_then_a", lambda: parent_transpose("p_f32", 0), "f32"),
                ("c_planar_5point1_f32_this_build", lambda: new.call(ptr("p6_f32"), mem, n, out, 0, 6, 6 | PLANAR, cuts), None),
                ("c_planar_5point1_f32_parent_host_downmix_then_mono", parent_downmix, None),
            ]
            times, sha = {v[0]: [] for v in variants}, {}
            for r in range(a.runs + 2):
                for vname, run, same in variants:
                    out[:] = 0
                    t0 = time.perf_counter()
                    run()
                    ms = (time.perf_counter() - t0) * 1e3
                    digest = hashlib.sha256(out.tobytes()).hexdigest()
                    if same:                                         # every stereo variant of one sample type gives the same records
                        assert sha.setdefault(same, digest) == digest, "%s: records differ (SHA-256)" % vname
                    if r >= 2:
                        times[vname].append(ms)
            row = {"workload": name, "memory": where, "frames": int(n), "tracks": len(lens), "records_sha256": sha,
                   **{k: spread(v) for k, v in times.items()}}
            checks = {}
            for t in ("s16", "f32"):
                p, b, pl = row["a_interleaved_%s_parent" % t], row["a_interleaved_%s_this_build" % t], row["b_planar_%s_this_build" % t]
                checks["a_%s_inside_parent_range" % t] = b["median"] <= p["max"]
                if where == "device":
                    checks["planar_%s_within_parent_max_plus_spread" % t] = pl["median"] <= p["max"] + (p["max"] - p["min"])
            row["gates"] = checks
            gates_ok = gates_ok and all(checks.values())
            result["workloads"].append(row)
            print(json.dumps(row), flush=True)
    result["gates"] = {"all": gates_ok, "records": "byte-identical by SHA-256 (asserted per call)"}
    new.close()
    old.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["gates"]))


if __name__ == "__main__":
    main()
