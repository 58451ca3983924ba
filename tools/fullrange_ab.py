#!/usr/bin/env python3
"""The re-dimensioned 4:2:0 table kernels against the parent commit's, and full range against limited (profiles/fullrange_ingest.json).

The gray tables of the table fills carry their length and index bias with the conversion constants since full range exists
(csrc/avd_preprocess.hip); before, both were literals.  Three series of avd_kernel_ms(AVD_K_PREPROCESS), N x 1080p device-resident
surfaces, NV12 and I420, profiling on (device input: the ingest kernel alone, no staging copy):

    limited on the parent     a checkout of the parent commit with its library built, given with --parent
    limited on this tree
    full on this tree         the same planes with AVD_FMT_FULL_RANGE

One RUN is one process (two builds of the library cannot share one): it uploads the planes, makes WARM warm-up calls of every series it has,
then CALLS measured calls of each, alternating, and reports each series' median.  The parent's run makes its two series twice per round, so
that both trees make the same sequence of calls.  The driver starts RUNS runs of each tree, alternating
parent, this tree, parent, ... on the same box, and reports per series the median and the spread (max - min) of the runs' medians.  The
yardstick is the parent's own run-to-run spread.  The records of the limited series are hashed: this tree must compute what the parent
computes.

usage: fullrange_ab.py --parent DIR [--runs 5] [--frames 120] [--height 1080] [--width 1920] [--warm 2] [--calls 5] [--out FILE]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(v):
    v = sorted(float(x) for x in v)
    return {"median": v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]), "min": v[0], "max": v[-1],
            "spread": v[-1] - v[0], "runs": len(v)}


def worker(a):
    """one run of one tree: prints one JSON line {series: {"median": ms, "calls": [...]}, "sha": {series: ...}}"""
    for p in (a.root, os.path.join(a.root, "ai-video-detector_amd")):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import avd_hip
    from avd_hip import synth
    n, h, w = a.frames, a.height, a.width
    y8, uv8 = synth.bgr_to_nv12(synth.make_clip(8, h, w, seed=1, dup_every=0))
    idx = np.arange(n) % 8
    y, uv = np.ascontiguousarray(y8[idx]), np.ascontiguousarray(uv8[idx])
    _, u, v = synth.nv12_to_i420(y, uv)
    dy, duv, du, dv = (torch.from_numpy(p).to("cuda:0") for p in (y, uv, u, v))
    torch.cuda.synchronize()
    ctx = avd_hip.Context(0)
    ctx.set_profiling(True)
    runs = {"nv12_limited": lambda: ctx.analyze_frames_nv12(dy, duv), "i420_limited": lambda: ctx.analyze_frames_i420(dy, du, dv)}
    if a.full:
        runs["nv12_full"] = lambda: ctx.analyze_frames_nv12(dy, duv, full_range=True)
        runs["i420_full"] = lambda: ctx.analyze_frames_i420(dy, du, dv, full_range=True)
    else:
        # a tree without the flag makes the same sequence of calls: its two limited series once more (not reported: what a call is preceded
        # by must not differ between the trees)
        runs["nv12_repeat"] = runs["nv12_limited"]
        runs["i420_repeat"] = runs["i420_limited"]
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
    ap.add_argument("--full", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent or not os.path.isdir(os.path.join(a.parent, "ai-video-detector_amd")):
        sys.exit("--parent: a checkout of the parent commit with its library built")
    shape = ["--frames", str(a.frames), "--height", str(a.height), "--width", str(a.width), "--warm", str(a.warm), "--calls", str(a.calls)]
    trees = {"parent": ["--root", os.path.abspath(a.parent)], "branch": ["--root", ROOT, "--full"]}
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
           "what": "avd_kernel_ms(AVD_K_PREPROCESS), ms per call of `frames` device-resident frames; per series the median and spread of the runs' medians",
           "series": {}}
    for name, runs in got.items():
        for k in runs[0]["series"]:
            out["series"][f"{k}_{name}"] = dict(stats([r["series"][k]["median"] for r in runs]), run_medians=[round(r["series"][k]["median"], 5) for r in runs])
        shas = {k: sorted({r["sha"][k] for r in runs}) for k in runs[0]["sha"]}
        assert all(len(v) == 1 for v in shas.values()), shas
        out.setdefault("records_sha", {})[name] = {k: v[0] for k, v in shas.items()}
        out.setdefault("ingest_kernel", {})[name] = runs[0]["ingest_kernel"]
    same = all(out["records_sha"]["branch"][k] == v for k, v in out["records_sha"]["parent"].items())
    out["limited_records_equal_the_parents"] = same
    s = out["series"]
    for kind in ("nv12", "i420"):
        par, lim, full = s[f"{kind}_limited_parent"], s[f"{kind}_limited_branch"], s[f"{kind}_full_branch"]
        out[kind] = {"limited_branch_minus_parent": lim["median"] - par["median"], "full_minus_limited": full["median"] - lim["median"],
                     "parent_spread": par["spread"],
                     "limited_within_parent_spread": bool(abs(lim["median"] - par["median"]) <= par["spread"]),
                     "full_within_parent_spread_of_limited": bool(abs(full["median"] - lim["median"]) <= par["spread"])}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not same:
        sys.exit("the limited-range records differ from the parent's")


if __name__ == "__main__":
    main()
