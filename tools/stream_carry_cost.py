#!/usr/bin/env python3
"""Cost of the carry frame between the calls of one stream: prepended to the next call (the default streaming path, any build) against
resident in a stream slot (option "stream_slot"), on one box, alternating (profiles/stream_carry.json).

Workload: N x 1080p NV12 surfaces, separately allocated and resident in HBM (a decoder pool), sent as frame lists in chunks of 8 and of 1.
  prepended   call k carries [last surface of call k - 1] + its chunk and drops record 0: what FrameAnalyzer._stream does
  resident    slot 1 emptied and selected, call k carries its chunk alone (analyze_frame_lists_async + synchronize)
Each (form, chunk) runs in a process of its own -- so that `--parent-lib` can put ANOTHER build of libavd_hip.so under the prepended form
(the commit before the option existed) -- and the processes alternate: round r runs prepended/8, resident/8, prepended/1, resident/1.
A process warms up with WARM passes over the stream, times PASSES passes with profiling off (host clock from the first call to the last
record: frames/s), then runs one pass with profiling on and sums avd_kernel_ms preprocess + hash over its calls (the ingest kernels).
Reported: per form and chunk the median over the rounds of the passes' median frames/s and of the ingest time, the ingested frames per
pass, and that the two forms' records are identical.  No threshold: the figures are recorded as they come out.

usage: stream_carry_cost.py [--frames 120] [--rounds 5] [--warm 2] [--passes 7] [--parent-lib PATH] [--out FILE]
       stream_carry_cost.py --child FORM CHUNK ...   (internal)"""
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
    n, chunk, fmt = a.frames, a.chunk, _lib.AVD_FMT_NV12
    y8, uv8 = synth.bgr_to_nv12(synth.make_clip(8, a.height, a.width, seed=1, dup_every=3))
    surfaces = [(torch.from_numpy(y8[f % 8].copy()).to("cuda:0"), torch.from_numpy(uv8[f % 8].copy()).to("cuda:0")) for f in range(n)]
    torch.cuda.synchronize()
    ctx = avd_hip.Context(0)
    chunks = [surfaces[i:i + chunk] for i in range(0, n, chunk)]

    def one_pass(profile):
        out, ingest, ingested = [], 0.0, 0
        carry = None
        if a.form == "resident":
            ctx.stream_reset(1)
            ctx.stream_slot(1)
        for c in chunks:
            if a.form == "resident":
                rec = np.zeros(len(c), avd_hip.RECORD_DTYPE)
                keep = ctx.analyze_frame_lists_async([(c, fmt)], rec)
                ctx.synchronize()
                del keep
                ingested += len(c)
            else:
                rec = ctx.analyze_frame_lists([(c if carry is None else [carry] + c, fmt)])[0]
                ingested += len(rec)
                rec = rec if carry is None else rec[1:]
                carry = c[-1]
            if profile:
                k = ctx.kernel_ms()
                ingest += k["preprocess"] + k["hash"]
            out.append(rec)
        if a.form == "resident":
            ctx.stream_slot(0)
        return np.concatenate(out), ingest, ingested

    for _ in range(a.warm):
        one_pass(False)
    fps = []
    for _ in range(a.passes):
        t0 = time.perf_counter()
        rec, _, ingested = one_pass(False)
        fps.append(n / (time.perf_counter() - t0))
    ctx.set_profiling(True)
    rec2, ingest_ms, _ = one_pass(True)
    ctx.set_profiling(False)
    assert rec.tobytes() == rec2.tobytes()
    ctx.close()
    print(json.dumps({"form": a.form, "chunk": chunk, "frames_per_s": median(fps), "ingest_kernel_ms": ingest_ms, "ingested_frames": ingested,
                      "calls": len(chunks), "records_sha256": hashlib.sha256(rec.tobytes()).hexdigest()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2, metavar=("FORM", "CHUNK"))
    ap.add_argument("--lib", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        a.form, a.chunk = a.child[0], int(a.child[1])
        return child(a)
    runs = {}
    for r in range(a.rounds):
        for chunk in (8, 1):
            for form in ("prepended", "resident"):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", form, str(chunk), "--frames", str(a.frames), "--height", str(a.height),
                       "--width", str(a.width), "--warm", str(a.warm), "--passes", str(a.passes)]
                if form == "prepended" and a.parent_lib:
                    cmd += ["--lib", a.parent_lib]
                # a child that faults, aborts or runs into its time limit ends the whole measurement: nothing more is started on the device
                got = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=300)
                runs.setdefault((form, chunk), []).append(json.loads(got.stdout.decode().strip().splitlines()[-1]))
                print(f"round {r} {form} chunk {chunk}: {runs[(form, chunk)][-1]}", file=sys.stderr, flush=True)
    out = {"workload": f"{a.frames} x {a.height}p NV12 surfaces, separately allocated in HBM, frame lists", "rounds": a.rounds, "warm": a.warm,
           "passes": a.passes, "prepended_library": "the parent commit's build" if a.parent_lib else "this build", "chunks": {}}
    for chunk in (8, 1):
        row = {}
        for form in ("prepended", "resident"):
            v = runs[(form, chunk)]
            row[form] = {"frames_per_s_median": median(x["frames_per_s"] for x in v), "frames_per_s_rounds": [round(x["frames_per_s"], 1) for x in v],
                         "ingest_kernel_ms_median": median(x["ingest_kernel_ms"] for x in v),
                         "ingest_kernel_ms_rounds": [round(x["ingest_kernel_ms"], 4) for x in v],
                         "ingested_frames_per_pass": v[0]["ingested_frames"], "calls_per_pass": v[0]["calls"]}
        row["records_identical"] = len({x["records_sha256"] for f in ("prepended", "resident") for x in runs[(f, chunk)]}) == 1
        row["ratio_resident_to_prepended"] = {k: row["resident"][k + "_median"] / row["prepended"][k + "_median"] for k in ("frames_per_s", "ingest_kernel_ms")}
        out["chunks"][str(chunk)] = row
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
