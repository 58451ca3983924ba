#!/usr/bin/env python3
"""Planar I420 ingest against NV12 ingest, same box, same process, alternating (profiles/i420_vs_nv12_ingest.json).

  1. kernel: N x 1080p device-resident surfaces through avd_analyze_frames_nv12 / avd_analyze_frames_i420 with profiling on;
     avd_kernel_ms(AVD_K_PREPROCESS) of each call (device input: the ingest kernel alone, no staging copy).  WARM warm-up calls
     of each kind, then CALLS measured calls of each kind, alternating; median and spread (max - min) per kind.  The yardstick is
     the NV12 kernel, the margin its own spread.
  2. host: one clip in ONE pageable host buffer, Y | U | V per frame (what a .y4m map or a yuv420p rawvideo pipe holds), end to
     end (wall clock around the blocking call): the planes handed to avd_analyze_frames_i420 as views of the buffer, against
     today's route -- Y4mSource's host interleave (two strided stores per frame into a new uv plane) followed by
     avd_analyze_frames_nv12.  The interleave alone is timed too.

usage: i420_ab.py [--frames 120] [--height 1080] [--width 1920] [--warm 3] [--calls 9] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ai-video-detector_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import avd_hip  # noqa: E402
from avd_hip import synth  # noqa: E402


def stats(v):
    v = sorted(float(x) for x in v)
    return {"median": v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]), "min": v[0], "max": v[-1],
            "spread": v[-1] - v[0], "calls": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    n, h, w = a.frames, a.height, a.width
    base = synth.make_clip(8, h, w, seed=1, dup_every=0)
    y8, uv8 = synth.bgr_to_nv12(base)
    idx = np.arange(n) % 8
    y, uv = np.ascontiguousarray(y8[idx]), np.ascontiguousarray(uv8[idx])
    _, u, v = synth.nv12_to_i420(y, uv)
    ctx = avd_hip.Context(0)
    out = {"frames": n, "height": h, "width": w, "warm": a.warm, "calls": a.calls}

    # ---- 1: the ingest kernels on device-resident surfaces ----
    dy, duv, du, dv = (torch.from_numpy(p).to("cuda:0") for p in (y, uv, u, v))
    torch.cuda.synchronize()
    ctx.set_profiling(True)
    runs = {"nv12": lambda: ctx.analyze_frames_nv12(dy, duv), "i420": lambda: ctx.analyze_frames_i420(dy, du, dv)}
    ms = {k: [] for k in runs}
    plan = {}
    ref = None
    for i in range(a.warm + a.calls):
        for kind, run in runs.items():
            rec = run()
            assert ref is None or rec.tobytes() == ref.tobytes(), kind
            ref = rec
            plan[kind] = int(ctx.debug_fetch("ingest_plan", (8,), np.int32)[7])
            if i >= a.warm:
                ms[kind].append(ctx.kernel_ms()["preprocess"])
    ctx.set_profiling(False)
    out["kernel_ms"] = {k: stats(x) for k, x in ms.items()}
    out["kernel_ms"]["ingest_kernel"] = plan
    d = out["kernel_ms"]["i420"]["median"] - out["kernel_ms"]["nv12"]["median"]
    out["kernel_ms"]["i420_minus_nv12"] = d
    out["kernel_ms"]["within_nv12_spread"] = bool(d <= out["kernel_ms"]["nv12"]["spread"])
    del dy, duv, du, dv

    # ---- 2: host-resident input, end to end ----
    luma, chroma = h * w, (h // 2) * (w // 2)
    fs = luma + 2 * chroma
    flat = np.empty(n * fs, np.uint8)
    view = lambda off, rows, cols: np.lib.stride_tricks.as_strided(flat[off:], (n, rows, cols), (fs, cols, 1))
    fy, fu, fv = view(0, h, w), view(luma, h // 2, w // 2), view(luma + chroma, h // 2, w // 2)
    fy[...], fu[...], fv[...] = y, u, v

    def interleave():
        uvs = np.empty((n, h // 2, w), np.uint8)
        for f in range(n):                       # per frame, as Y4mSource.sampled does
            uvs[f][:, 0::2] = fu[f]
            uvs[f][:, 1::2] = fv[f]
        return uvs

    def planar():
        return ctx.analyze_frames_i420(fy, fu, fv)

    def today():
        return ctx.analyze_frames_nv12(fy, interleave())

    wall = {"i420_one_buffer": [], "interleave_then_nv12": [], "interleave_alone": []}
    staged = {}
    for i in range(a.warm + a.calls):
        for kind, run in (("i420_one_buffer", planar), ("interleave_then_nv12", today), ("interleave_alone", interleave)):
            t0 = time.perf_counter()
            r = run()
            dt = (time.perf_counter() - t0) * 1e3
            if kind != "interleave_alone":
                assert r.tobytes() == ref.tobytes(), kind
                staged[kind] = ctx.stage_bytes()
            if i >= a.warm:
                wall[kind].append(dt)
    out["host_ms"] = {k: stats(x) for k, x in wall.items()}
    out["host_ms"]["stage_bytes"] = staged
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
