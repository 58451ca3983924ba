#!/usr/bin/env python3
"""What option "cv2_model" costs, and that its default costs nothing (profiles/cv2_model.json).

Forms, each in a process of its own:
  parent   ANOTHER build of libavd_hip.so (`--parent-lib`: the commit before the option existed).  The baseline.
  m0       this build, "cv2_model" = 0
  m1 / m8 / m16 / m25   this build under the mask (mul + add taps / three scales / lerp resize / all three): reported, not gated -- the unfolded
           forms these run cost what they cost
Workloads:
  clip3    one resident 120 x 1080p BGR clip analysed over and over with three clips in flight (avd_hip.ClipsInFlight, depth 3): frames/s by the
           host clock over PASSES passes of CLIPS clips after WARM warm-up passes
  bench    `python bench.py --gpus 1 --steps K --warmup W` (forms parent and m0 only): the headline
A round runs every form once per workload, and the order of the forms rotates from round to round, so that no form always follows the same one
(alternating on one box).  Reported per workload and form: the median over the rounds and the rounds' own figures; for clip3 a SHA-256 over the
records (parent and m0 must agree, every mask must differ from m0) and the "fb_model" debug buffer; and the condition the issue sets: m0 inside
the parent's range of rounds, on both workloads (and, beside it, the one-sided form: not below that range).

usage: cv2_model_cost.py [--rounds 3] [--warm 1] [--passes 3] [--clips 6] [--frames 120] [--parent-lib PATH] [--workloads a,b] [--out FILE]
       cv2_model_cost.py --child FORM WORKLOAD ...   (internal)"""
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

MASKS = (0, 1, 8, 16, 25)
FORMS = ("parent",) + tuple(f"m{m}" for m in MASKS)
WORKLOADS = ("clip3", "bench")


def median(v):
    v = sorted(float(x) for x in v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def child(a):
    from avd_hip import _lib
    if a.lib:
        _lib.SO_PATH = os.path.abspath(a.lib)              # another build of the library under the same binding
    if a.workload == "bench":                              # bench.py as it is, under the library of the form; its one JSON line goes out as it comes
        sys.argv = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup)]
        return runpy.run_path(sys.argv[0], run_name="__main__")
    import avd_hip
    from avd_hip import synth
    import torch
    mask = 0 if a.form == "parent" else int(a.form[1:])
    clip = torch.from_numpy(synth.make_clip(8, 1080, 1920, seed=1, dup_every=3)).to("cuda:0")
    clip = clip[torch.arange(a.frames, device="cuda:0") % 8].contiguous()
    torch.cuda.synchronize()
    runner = avd_hip.ClipsInFlight(device=0, depth=3)
    if a.form != "parent":
        for c in runner.ctxs:
            c.set_option("cv2_model", mask)

    def one_pass():
        return [rec for _, rec in runner.run((i, clip) for i in range(a.clips))]

    for _ in range(a.warm):
        one_pass()
    fps = []
    for _ in range(a.passes):
        t0 = time.perf_counter()
        recs = one_pass()
        fps.append(a.clips * a.frames / (time.perf_counter() - t0))
    assert all(r.tobytes() == recs[0].tobytes() for r in recs)
    state = [int(v) for v in runner.ctxs[0].fb_model()] if a.form != "parent" else None
    rerun = int(np.count_nonzero(recs[0]["reserved"]))
    for c in runner.ctxs:
        c.close()
    print(json.dumps({"form": a.form, "workload": a.workload, "frames_per_s": median(fps), "frames_per_s_passes": [round(x, 1) for x in fps],
                      "fb_model": state, "flagged_pairs_per_clip": rerun, "records_sha256": hashlib.sha256(recs[0].tobytes()).hexdigest()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2, metavar=("FORM", "WORKLOAD"))
    ap.add_argument("--lib", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--clips", type=int, default=6)
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
            mine = [f for f in forms if wl != "bench" or f in ("parent", "m0")]
            for form in mine[r % len(mine):] + mine[:r % len(mine)]:      # every form takes every place in the order once per len(mine) rounds
                cmd = [sys.executable, os.path.abspath(__file__), "--child", form, wl, "--frames", str(a.frames), "--clips", str(a.clips),
                       "--warm", str(a.warm), "--passes", str(a.passes), "--bench-steps", str(a.bench_steps), "--bench-warmup", str(a.bench_warmup)]
                if form == "parent":
                    cmd += ["--lib", a.parent_lib]
                # a child that faults, aborts or runs into its time limit ends the whole measurement: nothing more is started on the device
                got = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=300)
                runs.setdefault((form, wl), []).append(json.loads(got.stdout.decode().strip().splitlines()[-1]))
                print(f"round {r} {form} {wl}: {json.dumps(runs[(form, wl)][-1])[:300]}", file=sys.stderr, flush=True)
    out = {"rounds": a.rounds, "warm": a.warm, "passes": a.passes, "frames": a.frames, "clips_per_pass": a.clips, "clips_in_flight": 3,
           "parent_library": "the parent commit's build" if a.parent_lib else "not measured", "workloads": {}}
    for wl in workloads:
        row = {}
        if wl == "bench":
            for form in (f for f in forms if f in ("parent", "m0")):
                v = [x["value"] for x in runs[(form, wl)]]
                row[form] = {"value_median": median(v), "value_rounds": v, "unit": runs[(form, wl)][0].get("unit")}
            if a.parent_lib:
                row["m0_within_parent_range"] = bool(min(row["parent"]["value_rounds"]) <= row["m0"]["value_median"] <= max(row["parent"]["value_rounds"]))
                row["m0_not_below_parent_range"] = bool(min(row["parent"]["value_rounds"]) <= row["m0"]["value_median"])
            out["workloads"][wl] = row
            continue
        for form in forms:
            v = runs[(form, wl)]
            row[form] = {"frames_per_s_median": median(x["frames_per_s"] for x in v), "frames_per_s_rounds": [round(x["frames_per_s"], 1) for x in v],
                         "fb_model": v[0]["fb_model"], "flagged_pairs_per_clip": v[0]["flagged_pairs_per_clip"],
                         "records_sha256": sorted({x["records_sha256"] for x in v})}
        sha0 = row["m0"]["records_sha256"]
        row["masks_change_the_records"] = all(row[f]["records_sha256"] != sha0 for f in forms if f not in ("parent", "m0"))
        if a.parent_lib:
            p = row["parent"]
            row["m0_records_are_the_parents"] = row["parent"]["records_sha256"] == sha0 and len(sha0) == 1
            row["m0_fps_within_parent_range"] = bool(min(p["frames_per_s_rounds"]) <= row["m0"]["frames_per_s_median"] <= max(p["frames_per_s_rounds"]))
            row["m0_fps_not_below_parent_range"] = bool(min(p["frames_per_s_rounds"]) <= row["m0"]["frames_per_s_median"])
            row["ratio_to_parent"] = {f: row[f]["frames_per_s_median"] / p["frames_per_s_median"] for f in forms if f != "parent"}
        out["workloads"][wl] = row
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
