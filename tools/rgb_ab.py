#!/usr/bin/env python3
"""The RGB layouts of the fused ingest against BGR, against the parent commit, and against what a caller did before (profiles/rgb_ingest.json).

avd_kernel_ms(AVD_K_PREPROCESS) of N x 1080p device-resident frames, profiling on (device input: the ingest kernel alone, no staging copy).
Every series holds the SAME pixels, so every series' records must hash alike:

    bgr on the parent              a checkout of the parent commit with its library built, given with --parent
    bgr on this tree               the templated fills must have left BGR's code alone
    rgb24, bgra32, rgba32, rgbp    AVD_FMT_RGB24 / _BGRA32 / _RGBA32 / _RGBP (avd_hip.Pixels) on this tree
    bgr_on_rgb24_buffer            a control: the BGR fill on the rgb24 series' buffer (other results, not hashed) -- what of rgb24's distance
                                   from bgr is the buffer's place in memory and what the constants
    rearrange_<layout>             what a caller does without them: the torch rearrangement to BGR24 (flip / permute / index off alpha, then
                                   .contiguous()), timed by HIP events on torch's stream; it is followed by the BGR ingest

One RUN is one process (two builds of the library cannot share one): it makes WARM warm-up calls of every series it has, then CALLS measured
calls of each, alternating, and reports each series' median.  The parent's run repeats its one series in place of the four it lacks, so that
both trees make the same sequence of calls (the control included).  The driver starts RUNS runs of each tree, alternating parent, this tree, parent, ... on the same
box, and reports per series the median and the spread (max - min) of the runs' medians.  The yardstick is the parent's own run-to-run spread.

usage: rgb_ab.py --parent DIR [--runs 5] [--frames 120] [--height 1080] [--width 1920] [--warm 2] [--calls 5] [--out FILE]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ("rgb24", "bgra32", "rgba32", "rgbp")
BYTE_RATIO = {"rgb24": 1.0, "bgra32": 4.0 / 3.0, "rgba32": 4.0 / 3.0, "rgbp": 1.0}


def stats(v):
    v = sorted(float(x) for x in v)
    return {"median": v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]), "min": v[0], "max": v[-1],
            "spread": v[-1] - v[0], "runs": len(v)}


def worker(a):
    """one run of one tree: prints one JSON line {"series": {name: {"median": ms, "calls": [...]}}, "sha": {...}, "ingest_kernel": {...}}"""
    for p in (a.root, os.path.join(a.root, "ai-video-detector_amd")):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import avd_hip
    from avd_hip import synth
    n, h, w = a.frames, a.height, a.width
    d8 = torch.from_numpy(synth.make_clip(8, h, w, seed=1, dup_every=0)).to("cuda:0")
    bgr = d8[torch.arange(n, device="cuda:0") % 8].contiguous()
    clips = {"bgr": bgr}
    if a.branch:
        alpha = torch.full((n, h, w, 1), 255, dtype=torch.uint8, device="cuda:0")
        clips["rgb24"] = bgr.flip(-1).contiguous()
        clips["bgra32"] = torch.cat([bgr, alpha], -1).contiguous()
        clips["rgba32"] = torch.cat([bgr.flip(-1), alpha], -1).contiguous()
        clips["rgbp"] = bgr.flip(-1).permute(0, 3, 1, 2).contiguous()
        del alpha
    torch.cuda.synchronize()
    ctx = avd_hip.Context(0)
    ctx.set_profiling(True)
    runs = {"bgr": lambda: ctx.analyze_frames(bgr)}
    if a.branch:
        fmts = {"rgb24": avd_hip.AVD_FMT_RGB24, "bgra32": avd_hip.AVD_FMT_BGRA32, "rgba32": avd_hip.AVD_FMT_RGBA32, "rgbp": avd_hip.AVD_FMT_RGBP}
        for name in LAYOUTS:
            runs[name] = lambda name=name: ctx.analyze_pictures([avd_hip.Pixels(clips[name], fmts[name])])[0]
        runs["bgr_on_rgb24_buffer"] = lambda: ctx.analyze_frames(clips["rgb24"])
    else:
        # a tree without the layouts makes the same sequence of calls: its one series in their place (not reported: what a call is preceded
        # by must not differ between the trees)
        for name in LAYOUTS:
            runs[name + "_repeat"] = runs["bgr"]
        runs["control_repeat"] = runs["bgr"]
    ms = {k: [] for k in runs}
    sha, kernel = {}, {}
    for i in range(a.warm + a.calls):
        for kind, run in runs.items():
            rec = run()
            digest = hashlib.sha256(rec.tobytes()).hexdigest()[:16]
            assert sha.setdefault(kind, digest) == digest, kind
            kernel[kind] = int(ctx.debug_fetch("ingest_plan", (8,), np.int32)[7])
            if i >= a.warm:
                ms[kind].append(ctx.kernel_ms()["preprocess"])
    ctx.set_profiling(False)
    ctx.close()
    out = {k: {"median": stats(x)["median"], "calls": [round(float(t), 5) for t in x]} for k, x in ms.items() if not k.endswith("_repeat")}
    if a.branch:
        # what a caller does today: the rearrangement to BGR24 on torch's stream, HIP events around it
        rearrange = {"rgb24": lambda t: t.flip(-1).contiguous(), "bgra32": lambda t: t[..., :3].contiguous(),
                     "rgba32": lambda t: t[..., :3].flip(-1).contiguous(), "rgbp": lambda t: t.permute(0, 2, 3, 1).flip(-1).contiguous()}
        for name in LAYOUTS:
            t = []
            for i in range(a.warm + a.calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                b = rearrange[name](clips[name])
                e1.record()
                torch.cuda.synchronize()
                if i == 0:
                    assert torch.equal(b, bgr), name
                if i >= a.warm:
                    t.append(e0.elapsed_time(e1))
                del b
            out["rearrange_" + name] = {"median": stats(t)["median"], "calls": [round(float(x), 5) for x in t]}
    keep = lambda d: {k: v for k, v in d.items() if not k.endswith("_repeat")}
    print(json.dumps({"series": out, "sha": keep(sha), "ingest_kernel": keep(kernel)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--branch", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent or not os.path.isdir(os.path.join(a.parent, "ai-video-detector_amd")):
        sys.exit("--parent: a checkout of the parent commit with its library built")
    shape = ["--frames", str(a.frames), "--height", str(a.height), "--width", str(a.width), "--warm", str(a.warm), "--calls", str(a.calls)]
    trees = {"parent": ["--root", os.path.abspath(a.parent)], "branch": ["--root", ROOT, "--branch"]}
    got = {k: [] for k in trees}
    for r in range(a.runs):
        for name, args in trees.items():
            # a fresh child process per run; a run that fails or outlives its limit ends the measurement (nothing more is started on the GPU)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"] + args + shape, capture_output=True, text=True, timeout=a.timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-4000:])
                sys.exit(f"run {r} of {name} ended with status {p.returncode}")
            got[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(f"run {r} {name}: " + ", ".join(f"{k} {v['median']:.4f}" for k, v in got[name][-1]["series"].items()), file=sys.stderr, flush=True)
    out = {"frames": a.frames, "height": a.height, "width": a.width, "warm": a.warm, "calls_per_run": a.calls, "runs": a.runs,
           "what": "avd_kernel_ms(AVD_K_PREPROCESS), ms per call of `frames` device-resident frames (rearrange_*: HIP events on torch's stream around "
                   "the rearrangement to BGR24); per series the median and spread of the runs' medians",
           "series": {}}
    for name, runs in got.items():
        for k in runs[0]["series"]:
            out["series"][f"{k}_{name}"] = dict(stats([r["series"][k]["median"] for r in runs]), run_medians=[round(r["series"][k]["median"], 5) for r in runs])
        shas = {k: sorted({r["sha"][k] for r in runs}) for k in runs[0]["sha"]}
        assert all(len(v) == 1 for v in shas.values()), shas
        out.setdefault("records_sha", {})[name] = {k: v[0] for k, v in shas.items()}
        out.setdefault("ingest_kernel", {})[name] = runs[0]["ingest_kernel"]
    want = out["records_sha"]["parent"]["bgr"]
    same = all(v == want for k, v in out["records_sha"]["branch"].items() if k != "bgr_on_rgb24_buffer")
    out["every_series_records_equal_the_parents_bgr"] = same
    s = out["series"]
    par, bgr = s["bgr_parent"], s["bgr_branch"]
    out["bgr"] = {"branch_minus_parent": bgr["median"] - par["median"], "parent_spread": par["spread"],
                  "within_parent_spread": bool(abs(bgr["median"] - par["median"]) <= par["spread"])}
    ctl = s["bgr_on_rgb24_buffer_branch"]
    out["rgb24_control"] = {"bgr_on_rgb24_buffer_minus_bgr": ctl["median"] - bgr["median"], "rgb24_minus_bgr_on_its_buffer": s["rgb24_branch"]["median"] - ctl["median"],
                            "rgb24_within_parent_spread_of_bgr_on_its_buffer": bool(abs(s["rgb24_branch"]["median"] - ctl["median"]) <= par["spread"])}
    # per run of this tree: the layout's ingest against rearrangement + BGR ingest of the SAME run
    for name in LAYOUTS:
        lay, re = s[f"{name}_branch"], s[f"rearrange_{name}_branch"]
        per_run = [r["series"][name]["median"] < r["series"]["rearrange_" + name]["median"] + r["series"]["bgr"]["median"] for r in got["branch"]]
        out[name] = {"ratio_to_bgr": lay["median"] / bgr["median"], "byte_ratio": BYTE_RATIO[name], "minus_bgr": lay["median"] - bgr["median"],
                     "within_parent_spread_of_bgr": bool(abs(lay["median"] - bgr["median"]) <= par["spread"]),
                     "rearrange_plus_bgr": re["median"] + bgr["median"], "faster_than_rearrange_plus_bgr_in_every_run": bool(all(per_run))}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not same:
        sys.exit("the records differ from the parent's")


if __name__ == "__main__":
    main()
