#!/usr/bin/env python3
"""The ingest kernel on rotated pictures against the unrotated one, same box, same process, alternating (profiles/rotate_ingest.json).

N x 1080p device-resident NV12 surfaces through avd_analyze_pictures with rotate = 0, 1, 2, 3 and profiling on;
avd_kernel_ms(AVD_K_PREPROCESS) of each call (device input: the ingest kernel alone, no staging copy).  WARM warm-up calls of each
kind, then CALLS measured calls of each kind, alternating; median and spread (max - min) per kind.  The yardstick is the rotate-0
kernel of the same run (the table fill, unchanged by the rotation work):
  * the half turn (the flipped table fill) is reported against it, the margin is rotate 0's own spread;
  * the quarter turns (the strip fill) have one derived bar, 3 x the rotate-0 time: the traffic bound of the alternative, a transpose
    pre-pass (read the picture, write it turned, read it again).
Every kind analyses the SAME stored surfaces (the displayed pictures differ, so the records do; each kind's records must repeat).

usage: rotate_ab.py [--frames 120] [--height 1080] [--width 1920] [--warm 3] [--calls 9] [--out FILE]"""
import argparse
import json
import os
import sys

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
    y8, uv8 = synth.bgr_to_nv12(synth.make_clip(8, h, w, seed=1, dup_every=0))
    idx = np.arange(n) % 8
    dy, duv = (torch.from_numpy(np.ascontiguousarray(p[idx])).to("cuda:0") for p in (y8, uv8))
    torch.cuda.synchronize()
    ctx = avd_hip.Context(0)
    out = {"frames": n, "height": h, "width": w, "warm": a.warm, "calls": a.calls}
    ctx.set_profiling(True)
    kinds = (0, 1, 2, 3)
    ms = {k: [] for k in kinds}
    plan, ref = {}, {}
    for i in range(a.warm + a.calls):
        for k in kinds:
            rec = ctx.analyze_pictures([(dy, duv)], [k])[0]
            assert k not in ref or rec.tobytes() == ref[k].tobytes(), k
            ref[k] = rec
            p = ctx.debug_fetch("ingest_plan", (8,), np.int32)
            assert ctx.ingest_rotate() == k
            plan[k] = {"h": int(p[0]), "w": int(p[1]), "rows_per_band": int(p[2]), "nbands": int(p[3]), "lds_bytes": int(p[6]), "kernel": int(p[7])}
            if i >= a.warm:
                ms[k].append(ctx.kernel_ms()["preprocess"])
    ctx.set_profiling(False)
    ctx.close()
    res = {f"rotate{k}": stats(ms[k]) for k in kinds}
    base = res["rotate0"]["median"]
    res["ingest_plan"] = {f"rotate{k}": plan[k] for k in kinds}
    res["ratio_to_rotate0"] = {f"rotate{k}": res[f"rotate{k}"]["median"] / base for k in (1, 2, 3)}
    d = res["rotate2"]["median"] - base
    res["half_turn_minus_rotate0"] = d
    res["half_turn_within_rotate0_spread"] = bool(d <= res["rotate0"]["spread"])
    res["quarter_turn_bar_ms"] = 3.0 * base
    res["quarter_turns_below_bar"] = bool(max(res["rotate1"]["median"], res["rotate3"]["median"]) < 3.0 * base)
    out["kernel_ms"] = res
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
