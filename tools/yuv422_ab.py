#!/usr/bin/env python3
"""The 4:2:2 layouts of the fused ingest against the NV12 table kernel and the BGR kernel of the same run (profiles/yuv422_ingest.json).

avd_kernel_ms(AVD_K_PREPROCESS) of N x 1080p device-resident frames, profiling on (device input: the ingest kernel alone, no staging copy).
Every series holds the SAME picture: an NV12 clip, the 4:2:2 pictures whose chroma rows 2k and 2k + 1 are both the NV12 picture's chroma row
k (by the chroma-row-pairs identity of include/avd.h they convert to the same BGR frames), in the four layouts, and those BGR frames
(oracle.nv12_to_bgr).  So every series' records must hash alike, which is checked.

    nv12                           the 4:2:0 table kernel: one chroma row serves two luma rows (1.5 bytes per pixel)
    bgr                            the staged BGR kernel (3 bytes per pixel)
    yuyv422, uyvy422, i422, nv16   the new table kernels (2 bytes per pixel: 1.33 x NV12's)

One process; WARM warm-up rounds, then CALLS measured rounds, a round being one call of every series in turn.  Per series the median and the
spread (max - min) of its calls.  The yardsticks are the nv12 and the bgr series of the SAME run.  One derived bar: a 4:2:2 table kernel must
take less than 8/3 of the BGR kernel's time -- the traffic of the only alternative with identical results, a conversion pass that reads 2 and
writes 3 bytes per pixel followed by the 3-byte BGR ingest.

usage: yuv422_ab.py [--frames 120] [--height 1080] [--width 1920] [--warm 3] [--calls 9] [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ai-video-detector_amd")):
    sys.path.insert(0, _p)
LAYOUTS = ("yuyv422", "uyvy422", "i422", "nv16")
KERNELS = {"nv12": 4, "bgr": 2, "yuyv422": 15, "uyvy422": 15, "i422": 17, "nv16": 19}      # "ingest_plan"[7] of an aligned 1080p clip
BAR = 8.0 / 3.0


def stats(v):
    v = sorted(float(x) for x in v)
    return {"median": v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]), "min": v[0], "max": v[-1],
            "spread": v[-1] - v[0], "calls": [round(x, 5) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import avd_hip
    from avd_hip import Pixels, synth
    from oracle import oracle as O
    n, h, w = a.frames, a.height, a.width
    y8, uv8 = synth.bgr_to_nv12(synth.make_clip(8, h, w, seed=1, dup_every=0))
    bgr8 = O.nv12_to_bgr(y8, uv8)
    c8 = np.repeat(uv8, 2, axis=1)                              # chroma rows 2k and 2k + 1 := row k: uint8[8, h, w], U,V interleaved
    yuyv8 = np.stack([y8, c8], -1)                              # Y0 U Y1 V: the luma byte, then the chroma byte of the same column
    pick = torch.arange(n, device="cuda:0") % 8
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")[pick].contiguous()
    y, c = dev(y8), dev(c8)
    clips = {"nv12": (y, dev(uv8)), "bgr": dev(bgr8), "yuyv422": Pixels(dev(yuyv8), avd_hip.AVD_FMT_YUYV422),
             "uyvy422": Pixels(dev(yuyv8[..., ::-1]), avd_hip.AVD_FMT_UYVY422),
             "i422": Pixels((y, dev(c8[..., 0::2]), dev(c8[..., 1::2])), avd_hip.AVD_FMT_I422), "nv16": Pixels((y, c), avd_hip.AVD_FMT_NV16)}
    torch.cuda.synchronize()
    ctx = avd_hip.Context(0)
    ctx.set_profiling(True)
    ms = {k: [] for k in clips}
    sha, kernel = {}, {}
    for i in range(a.warm + a.calls):
        for kind, clip in clips.items():
            rec = ctx.analyze_pictures([clip])[0]
            digest = hashlib.sha256(rec.tobytes()).hexdigest()[:16]
            assert sha.setdefault(kind, digest) == digest, kind
            kernel[kind] = int(ctx.debug_fetch("ingest_plan", (8,), np.int32)[7])
            if i >= a.warm:
                ms[kind].append(ctx.kernel_ms()["preprocess"])
    ctx.set_profiling(False)
    ctx.close()
    assert kernel == KERNELS, kernel
    s = {k: stats(v) for k, v in ms.items()}
    out = {"frames": n, "height": h, "width": w, "warm": a.warm, "calls": a.calls,
           "what": "avd_kernel_ms(AVD_K_PREPROCESS), ms per call of `frames` device-resident frames; one process, series alternating; per series "
                   "the median and spread (max - min) of its calls",
           "series": s, "ingest_kernel": kernel, "records_sha": sha, "every_series_records_equal": len(set(sha.values())) == 1,
           "bar": "a 4:2:2 table kernel takes less than 8/3 of the BGR kernel's time of the same run"}
    for name in LAYOUTS:
        m = s[name]["median"]
        out[name] = {"ratio_to_nv12": m / s["nv12"]["median"], "byte_ratio_to_nv12": 4.0 / 3.0, "ratio_to_bgr": m / s["bgr"]["median"],
                     "bar_ms": BAR * s["bgr"]["median"], "under_the_bar": bool(m < BAR * s["bgr"]["median"]),
                     "worst_call_under_the_bar": bool(s[name]["max"] < BAR * s["bgr"]["min"])}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not out["every_series_records_equal"]:
        sys.exit("the records differ between the series")


if __name__ == "__main__":
    main()
