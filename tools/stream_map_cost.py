#!/usr/bin/env python3
"""Cost of serving several live streams from one context: in turn through eight stream slots (option "stream_slot", one call per stream and
round) against ONE mapped call per round (option "stream_map"), on one box, alternating (profiles/stream_map.json).

Workload: S streams of N x 1080p NV12 surfaces each, separately allocated and resident in HBM (decoder pools), sent as frame lists in chunks
of 8 and of 1.
  turn_parent  every round, stream s selects slot s + 1 and sends its chunk alone -- on ANOTHER build of libavd_hip.so (`--parent-lib`: the
               commit before the map existed).  The baseline.
  turn         the same calls on this build
  mapped       position s mapped to slot s + 1; every round is one analyze_frame_lists_async over all streams
Each (form, chunk) runs in a process of its own and the processes alternate: round r runs the three forms at chunk 8, then at chunk 1, and
the order of the forms rotates from round to round, so that over three rounds no form always follows the same one.
A process warms up with WARM passes over the streams, times PASSES passes with profiling off (host clock from the first call to the last
record: frames/s over all streams), then runs one pass with profiling on and sums avd_kernel_ms preprocess + hash over its calls (the
ingest kernels).  Reported: per form and chunk the median over the rounds of the passes' median frames/s and of the ingest time, the rounds'
own figures (their spread), the calls per pass, and ONE SHA-256 over the records of all forms, which must agree.  No threshold: the figures
are recorded as they come out.

usage: stream_map_cost.py [--streams 8] [--frames 120] [--rounds 3] [--warm 1] [--passes 5] [--parent-lib PATH] [--out FILE]
       stream_map_cost.py --child FORM CHUNK ...   (internal)"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ai-video-detector_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

FORMS = ("turn_parent", "turn", "mapped")


def median(v):
    v = sorted(float(x) for x in v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def child(a):
    from avd_hip import _lib
    if a.lib:
        _lib.SO_PATH = os.path.abspath(a.lib)              # another build of the library under the same binding
    import avd_hip
    from avd_hip import synth
    import torch
    n, chunk, fmt, S = a.frames, a.chunk, _lib.AVD_FMT_NV12, a.streams
    y8, uv8 = synth.bgr_to_nv12(synth.make_clip(8, a.height, a.width, seed=1, dup_every=3))
    y8, uv8 = torch.from_numpy(y8).to("cuda:0"), torch.from_numpy(uv8).to("cuda:0")
    streams = []
    for s in range(S):                                     # every stream its own content (the clip shifted by 32 s columns), every surface its own allocation
        ys, uvs = torch.roll(y8, 32 * s, dims=2), torch.roll(uv8, 32 * s, dims=2)
        streams.append([(ys[f % 8].clone(), uvs[f % 8].clone()) for f in range(n)])
    torch.cuda.synchronize()
    ctx = avd_hip.Context(0)
    rounds = [[st[i:i + chunk] for st in streams] for i in range(0, n, chunk)]
    mapped = a.form == "mapped"

    def one_pass(profile):
        out, ingest, calls = [[] for _ in range(S)], 0.0, 0
        ctx.stream_reset(0)
        if mapped:
            ctx.stream_map({s: s + 1 for s in range(S)})
        for rnd in rounds:
            if mapped:
                rec = np.zeros(sum(len(c) for c in rnd), avd_hip.RECORD_DTYPE)
                keep = ctx.analyze_frame_lists_async([(c, fmt) for c in rnd], rec)
                ctx.synchronize()
                del keep
                calls += 1
                if profile:
                    k = ctx.kernel_ms()
                    ingest += k["preprocess"] + k["hash"]
                at = 0
                for s, c in enumerate(rnd):
                    out[s].append(rec[at:at + len(c)])
                    at += len(c)
            else:
                for s, c in enumerate(rnd):
                    ctx.stream_slot(s + 1)
                    rec = np.zeros(len(c), avd_hip.RECORD_DTYPE)
                    keep = ctx.analyze_frame_lists_async([(c, fmt)], rec)
                    ctx.synchronize()
                    del keep
                    calls += 1
                    if profile:
                        k = ctx.kernel_ms()
                        ingest += k["preprocess"] + k["hash"]
                    out[s].append(rec)
        if mapped:
            ctx.stream_map(None)
        else:
            ctx.stream_slot(0)
        return np.concatenate([np.concatenate(o) for o in out]), ingest, calls

    for _ in range(a.warm):
        one_pass(False)
    fps = []
    for _ in range(a.passes):
        t0 = time.perf_counter()
        rec, _, calls = one_pass(False)
        fps.append(S * n / (time.perf_counter() - t0))
    ctx.set_profiling(True)
    rec2, ingest_ms, _ = one_pass(True)
    ctx.set_profiling(False)
    assert rec.tobytes() == rec2.tobytes()
    ctx.close()
    print(json.dumps({"form": a.form, "chunk": chunk, "frames_per_s": median(fps), "ingest_kernel_ms": ingest_ms, "calls": calls,
                      "records_sha256": hashlib.sha256(rec.tobytes()).hexdigest()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2, metavar=("FORM", "CHUNK"))
    ap.add_argument("--lib", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        a.form, a.chunk = a.child[0], int(a.child[1])
        return child(a)
    if not 1 <= a.streams <= 8:
        ap.error("--streams 1 ... 8: a context has eight stream slots")
    forms = FORMS if a.parent_lib else FORMS[1:]
    runs = {}
    for r in range(a.rounds):
        for chunk in (8, 1):
            for form in forms[r % len(forms):] + forms[:r % len(forms)]:      # every form takes every place in the order once per len(forms) rounds
                cmd = [sys.executable, os.path.abspath(__file__), "--child", form, str(chunk), "--streams", str(a.streams), "--frames", str(a.frames),
                       "--height", str(a.height), "--width", str(a.width), "--warm", str(a.warm), "--passes", str(a.passes)]
                if form == "turn_parent":
                    cmd += ["--lib", a.parent_lib]
                # a child that faults, aborts or runs into its time limit ends the whole measurement: nothing more is started on the device
                got = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=300)
                runs.setdefault((form, chunk), []).append(json.loads(got.stdout.decode().strip().splitlines()[-1]))
                print(f"round {r} {form} chunk {chunk}: {runs[(form, chunk)][-1]}", file=sys.stderr, flush=True)
    out = {"workload": f"{a.streams} streams of {a.frames} x {a.height}p NV12 surfaces, separately allocated in HBM, frame lists", "rounds": a.rounds,
           "warm": a.warm, "passes": a.passes, "turn_parent_library": "the parent commit's build" if a.parent_lib else "not measured", "chunks": {}}
    for chunk in (8, 1):
        row = {}
        for form in forms:
            v = runs[(form, chunk)]
            row[form] = {"frames_per_s_median": median(x["frames_per_s"] for x in v), "frames_per_s_rounds": [round(x["frames_per_s"], 1) for x in v],
                         "ingest_kernel_ms_median": median(x["ingest_kernel_ms"] for x in v),
                         "ingest_kernel_ms_rounds": [round(x["ingest_kernel_ms"], 4) for x in v], "calls_per_pass": v[0]["calls"]}
        shas = {x["records_sha256"] for f in forms for x in runs[(f, chunk)]}
        row["records_identical"] = len(shas) == 1
        row["records_sha256"] = sorted(shas)
        base = "turn_parent" if a.parent_lib else "turn"
        row["ratio_mapped_to_" + base] = {k: row["mapped"][k + "_median"] / row[base][k + "_median"] for k in ("frames_per_s", "ingest_kernel_ms")}
        if a.parent_lib:
            lo, hi = min(row["turn_parent"]["frames_per_s_rounds"]), max(row["turn_parent"]["frames_per_s_rounds"])
            row["turn_within_turn_parent_spread"] = bool(lo <= row["turn"]["frames_per_s_median"] <= hi)
        out["chunks"][str(chunk)] = row
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
