#!/usr/bin/env python3
"""Cost of the per-clip ingest and hash launches of a batch call, and what option "ingest_group" makes of it (profiles/ingest_group.json).

Forms, each in a process of its own:
  parent   ANOTHER build of libavd_hip.so (`--parent-lib`: the commit before the option existed).  The baseline.
  off      this build, "ingest_group" = 0
  on       this build, "ingest_group" = 1
Workloads (all input resident in HBM):
  mapped8 / mapped1   eight streams of N x 1080p NV12 surfaces, separately allocated, through ONE mapped call per round ("stream_map") in
                      chunks of 8 and of 1 frames a stream
  short13             thirteen 20-frame 720p BGR clips per call
  batch32             32 clips of N x 1080p BGR frames in one call (`--batch-clips` fewer if they do not fit)
  bench               `python bench.py --gpus 1 --steps K --warmup W` (forms parent and off only): the headline
A round runs every workload once per form, and the order of the forms rotates from round to round, so that over three rounds no form always
follows the same one.  A process warms up with WARM passes, times PASSES passes with profiling off (host clock from the first call to the last
record: frames/s), then runs one pass with profiling on and sums avd_kernel_ms preprocess + hash over its calls -- the ingest regions per
pass; a call with more regions than the library records (96) has no such figure and is reported as null.  Reported: per workload and form the
median over the rounds and the rounds' own figures (their spread), ONE SHA-256 over the records of all forms, which must agree, and what the
issue asks of the figures: "off" inside the parent's range of rounds, "on" at chunk 1 below it by more than the spread.

usage: ingest_group_cost.py [--rounds 3] [--warm 1] [--passes 3] [--frames 120] [--parent-lib PATH] [--workloads a,b] [--out FILE]
       ingest_group_cost.py --child FORM WORKLOAD ...   (internal)"""
import argparse
import hashlib
import json
import os
import runpy
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ai-video-detector_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

FORMS = ("parent", "off", "on")
WORKLOADS = ("mapped8", "mapped1", "short13", "batch32", "bench")


def median(v):
    v = sorted(float(x) for x in v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def child_bench(a):
    """bench.py as it is, under the library of the form; its one JSON line goes out as it comes"""
    sys.argv = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup)]
    runpy.run_path(sys.argv[0], run_name="__main__")


def child(a):
    from avd_hip import _lib
    if a.lib:
        _lib.SO_PATH = os.path.abspath(a.lib)              # another build of the library under the same binding
    if a.workload == "bench":
        return child_bench(a)
    import avd_hip
    from avd_hip import synth
    import torch
    ctx = avd_hip.Context(0)
    if a.form != "parent":
        ctx.set_option("ingest_group", int(a.form == "on"))
    n = a.frames
    if a.workload.startswith("mapped"):
        chunk, S, fmt = int(a.workload[6:]), 8, _lib.AVD_FMT_NV12
        y8, uv8 = synth.bgr_to_nv12(synth.make_clip(8, 1080, 1920, seed=1, dup_every=3))
        y8, uv8 = torch.from_numpy(y8).to("cuda:0"), torch.from_numpy(uv8).to("cuda:0")
        streams = []
        for s in range(S):                                 # every stream its own content (the clip shifted by 32 s columns), every surface its own allocation
            ys, uvs = torch.roll(y8, 32 * s, dims=2), torch.roll(uv8, 32 * s, dims=2)
            streams.append([(ys[f % 8].clone(), uvs[f % 8].clone()) for f in range(n)])
        calls = [[(st[i:i + chunk], fmt) for st in streams] for i in range(0, n, chunk)]
        frames = S * n
        submit = lambda call, rec: ctx.analyze_frame_lists_async(call, rec)
        count = lambda call: sum(len(c) for c, _ in call)
    else:
        k, m, h, w = (13, 20, 720, 1280) if a.workload == "short13" else (a.batch_clips, n, 1080, 1920)
        base = torch.from_numpy(synth.make_clip(8, h, w, seed=2, dup_every=3)).to("cuda:0")
        idx = torch.arange(m, device="cuda:0") % 8
        calls = [[torch.roll(base, 24 * c, dims=2)[idx].contiguous() for c in range(k)]]      # every clip its own content and memory
        frames = k * m
        submit = lambda call, rec: ctx.analyze_batch_async(call, rec)
        count = lambda call: sum(len(c) for c in call)
    torch.cuda.synchronize()
    mapped = a.workload.startswith("mapped")

    def one_pass(profile):
        out, ingest = [], 0.0
        if mapped:
            ctx.stream_reset(0)
            ctx.stream_map({s: s + 1 for s in range(8)})
        for call in calls:
            rec = np.zeros(count(call), avd_hip.RECORD_DTYPE)
            keep = submit(call, rec)
            ctx.synchronize()
            del keep
            if profile and ingest is not None:
                try:
                    kms = ctx.kernel_ms()
                    ingest += kms["preprocess"] + kms["hash"]
                except avd_hip.AvdError:                  # more regions than the library records: no figure for this workload
                    ingest = None
            out.append(rec)
        if mapped:
            ctx.stream_map(None)
        return np.concatenate(out), ingest

    for _ in range(a.warm):
        one_pass(False)
    fps = []
    for _ in range(a.passes):
        t0 = time.perf_counter()
        rec, _ = one_pass(False)
        fps.append(frames / (time.perf_counter() - t0))
    ctx.set_profiling(True)
    rec2, ingest_ms = one_pass(True)
    ctx.set_profiling(False)
    assert rec.tobytes() == rec2.tobytes()
    launches = [int(v) for v in ctx.ingest_call()] if a.form != "parent" else None      # of the last call of the pass
    ctx.close()
    print(json.dumps({"form": a.form, "workload": a.workload, "frames_per_s": median(fps), "ingest_kernel_ms": ingest_ms, "calls": len(calls),
                      "ingest_call": launches, "records_sha256": hashlib.sha256(rec.tobytes()).hexdigest()}))


def spread(v):
    return max(v) - min(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2, metavar=("FORM", "WORKLOAD"))
    ap.add_argument("--lib", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--batch-clips", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        a.form, a.workload = a.child
        return child(a)
    workloads = [w for w in a.workloads.split(",") if w]
    if any(w not in WORKLOADS for w in workloads):
        ap.error("--workloads: " + ", ".join(WORKLOADS))
    forms = FORMS if a.parent_lib else FORMS[1:]
    runs = {}
    for r in range(a.rounds):
        for wl in workloads:
            mine = [f for f in forms if not (wl == "bench" and f == "on")]
            for form in mine[r % len(mine):] + mine[:r % len(mine)]:      # every form takes every place in the order once per len(forms) rounds
                cmd = [sys.executable, os.path.abspath(__file__), "--child", form, wl, "--frames", str(a.frames), "--batch-clips", str(a.batch_clips),
                       "--warm", str(a.warm), "--passes", str(a.passes), "--bench-steps", str(a.bench_steps), "--bench-warmup", str(a.bench_warmup)]
                if form == "parent":
                    cmd += ["--lib", a.parent_lib]
                # a child that faults, aborts or runs into its time limit ends the whole measurement: nothing more is started on the device
                got = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=300)
                runs.setdefault((form, wl), []).append(json.loads(got.stdout.decode().strip().splitlines()[-1]))
                print(f"round {r} {form} {wl}: {json.dumps(runs[(form, wl)][-1])[:300]}", file=sys.stderr, flush=True)
    out = {"rounds": a.rounds, "warm": a.warm, "passes": a.passes, "frames": a.frames, "batch_clips": a.batch_clips,
           "parent_library": "the parent commit's build" if a.parent_lib else "not measured", "workloads": {}}
    for wl in workloads:
        row = {}
        if wl == "bench":
            for form in (f for f in forms if f != "on"):
                v = [x["value"] for x in runs[(form, wl)]]
                row[form] = {"value_median": median(v), "value_rounds": v, "unit": runs[(form, wl)][0].get("unit")}
            if a.parent_lib:
                row["off_within_parent_range"] = bool(min(row["parent"]["value_rounds"]) <= row["off"]["value_median"] <= max(row["parent"]["value_rounds"]))
            out["workloads"][wl] = row
            continue
        for form in forms:
            v = runs[(form, wl)]
            ing = [x["ingest_kernel_ms"] for x in v]
            row[form] = {"frames_per_s_median": median(x["frames_per_s"] for x in v), "frames_per_s_rounds": [round(x["frames_per_s"], 1) for x in v],
                         "ingest_kernel_ms_median": None if None in ing else median(ing),
                         "ingest_kernel_ms_rounds": [None if x is None else round(x, 4) for x in ing], "calls_per_pass": v[0]["calls"],
                         "ingest_call_of_the_last_call": v[0]["ingest_call"]}
        shas = {x["records_sha256"] for f in forms for x in runs[(f, wl)]}
        row["records_identical"] = len(shas) == 1
        row["records_sha256"] = sorted(shas)
        if a.parent_lib:
            p = row["parent"]
            row["off_fps_within_parent_range"] = bool(min(p["frames_per_s_rounds"]) <= row["off"]["frames_per_s_median"] <= max(p["frames_per_s_rounds"]))
            if p["ingest_kernel_ms_median"] is not None and row["on"]["ingest_kernel_ms_median"] is not None:
                noise = max(spread(p["ingest_kernel_ms_rounds"]), spread(row["on"]["ingest_kernel_ms_rounds"]))
                row["on_ingest_below_parent_range_by_more_than_the_spread"] = bool(
                    max(row["on"]["ingest_kernel_ms_rounds"]) < min(p["ingest_kernel_ms_rounds"]) - noise)
                row["ratio_on_to_parent"] = {k: row["on"][k + "_median"] / p[k + "_median"] for k in ("frames_per_s", "ingest_kernel_ms")}
        out["workloads"][wl] = row
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
