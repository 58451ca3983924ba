#!/usr/bin/env python3
"""Clips as lists of separately allocated frames against the strided clip, same box, same process, alternating (profiles/framelist_ingest.json).

1  kernel: N x 1080p frames resident in HBM as NV12, I420 and BGR, the same frames given once as ONE strided stack (avd_analyze_pictures) and
   once as a list of N separate device allocations (avd_analyze_frame_lists), profiling on; avd_kernel_ms(AVD_K_PREPROCESS) of each call
   (device input: the ingest kernel alone).  WARM warm-up calls of each form, then CALLS measured calls of each, alternating; median and
   spread (max - min) of each.  The yardstick is the strided kernel of the same run: the list passes if its median lies inside the strided
   form's own spread (min .. max); the ratio of the medians is reported either way.  The records of the two forms must be identical.
   AVD_K_PREPROCESS is the KERNEL alone: the list form's per-call upload of its table of plane pointers (frames x planes x 8 bytes, one
   copy from pinned memory) is enqueued in front of the first mark and is in neither figure -- this is not the whole cost of the list path
   on device input; part 2 times whole calls.
2  host: N separately allocated 1080p NV12 host frames, pageable and pinned; wall time from the list of frames to the records
   (a) np.stack of the frames, then the strided call -- what the streaming analyzer did -- and (b) the list call; alternating, median and
   spread of each, the staging copies of each ("stage_copies") and the ratio b / a.

usage: framelist_ab.py [--frames 120] [--height 1080] [--width 1920] [--warm 3] [--calls 9] [--host-calls 5] [--out FILE]"""
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
from avd_hip import _lib, synth  # noqa: E402


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
    ap.add_argument("--host-calls", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    n, h, w = a.frames, a.height, a.width
    bgr8 = synth.make_clip(8, h, w, seed=1, dup_every=0)
    y8, uv8 = synth.bgr_to_nv12(bgr8)
    idx = np.arange(n) % 8
    host = {"nv12": (_lib.AVD_FMT_NV12, (y8, uv8)), "i420": (_lib.AVD_FMT_I420, synth.nv12_to_i420(y8, uv8)), "bgr": (_lib.AVD_FMT_BGR24, (bgr8,))}
    out = {"frames": n, "height": h, "width": w, "warm": a.warm, "calls": a.calls, "host_calls": a.host_calls}
    ctx = avd_hip.Context(0)

    # ---- 1: the ingest kernel, list against strided ------------------------------------------------------------------------------------------
    ctx.set_profiling(True)
    kernel = {}
    for name, (fmt, planes8) in host.items():
        stack = tuple(torch.from_numpy(np.ascontiguousarray(p[idx])).to("cuda:0") for p in planes8)
        order = np.random.default_rng(7).permutation(n)                 # allocation order != list order
        frames = [None] * n
        for f in order:
            fr = tuple(torch.from_numpy(np.ascontiguousarray(p[idx[f]])).to("cuda:0") for p in planes8)
            frames[f] = fr[0] if name == "bgr" else fr
        torch.cuda.synchronize()
        clip = stack[0] if name == "bgr" else stack
        ms = {"strided": [], "list": []}
        plan, ref = {}, None
        for i in range(a.warm + a.calls):
            for form in ("strided", "list"):
                rec = ctx.analyze_pictures([clip])[0] if form == "strided" else ctx.analyze_frame_lists([(frames, fmt)])[0]
                assert ref is None or rec.tobytes() == ref.tobytes(), (name, form)
                ref = rec
                assert ctx.ingest_list() == ((1, n) if form == "list" else (0, 0))
                plan[form] = int(ctx.debug_fetch("ingest_plan", (8,), np.int32)[7])
                if i >= a.warm:
                    ms[form].append(ctx.kernel_ms()["preprocess"])
        s, l = stats(ms["strided"]), stats(ms["list"])
        kernel[name] = {"strided": s, "list": l, "kernel_id": plan, "ratio_list_to_strided": l["median"] / s["median"],
                        "list_median_within_strided_spread": bool(s["min"] <= l["median"] <= s["max"])}
        del stack, frames, clip
        torch.cuda.empty_cache()
    ctx.set_profiling(False)
    out["kernel_ms"] = kernel

    # ---- 2: host frames, list against stack-then-strided -------------------------------------------------------------------------------------
    hosts = {}
    for kind in ("pageable", "pinned"):
        def alloc(src):
            if kind == "pinned":
                t = torch.empty(src.shape, dtype=torch.uint8).pin_memory()
                buf = t.numpy()
                buf[...] = src
                return buf, t
            return np.array(src, copy=True), None
        frames, keep = [], []
        for f in range(n):
            y, ty = alloc(y8[idx[f]])
            uv, tuv = alloc(uv8[idx[f]])
            frames.append((y, uv))
            keep.append((ty, tuv))
        wall = {"stack_then_strided": [], "list": []}
        copies, ref = {}, None
        for i in range(1 + a.host_calls):
            for form in wall:
                t0 = time.perf_counter()
                if form == "list":
                    rec = ctx.analyze_frame_lists([(frames, _lib.AVD_FMT_NV12)])[0]
                else:
                    rec = ctx.analyze_frames_nv12(np.stack([fr[0] for fr in frames]), np.stack([fr[1] for fr in frames]))
                dt = (time.perf_counter() - t0) * 1e3
                assert ref is None or rec.tobytes() == ref.tobytes(), (kind, form)
                ref = rec
                copies[form] = {"stage_copies": ctx.stage_copies(), "stage_bytes": ctx.stage_bytes()}
                if i >= 1:
                    wall[form].append(dt)
        sa, sb = stats(wall["stack_then_strided"]), stats(wall["list"])
        hosts[kind] = {"stack_then_strided_ms": sa, "list_ms": sb, "staging": copies, "ratio_list_to_stack": sb["median"] / sa["median"],
                       "frames_per_s": {"stack_then_strided": n / sa["median"] * 1e3, "list": n / sb["median"] * 1e3}}
        del frames, keep
    out["host_wall"] = hosts
    ctx.close()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
