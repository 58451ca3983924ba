#!/usr/bin/env python3
"""Several continued tracks per avd_audio_features call (option "audio_track_slot"): what a round of eight live streams costs, one run on an
MI355X -> profiles/audio_slot_map.json.

    python tools/audio_map_bench.py --parent-lib PATH/libavd_hip.so [--rounds 3] [--bench-rounds 5] [--out profiles/audio_slot_map.json]

--parent-lib is the library of the PARENT commit, built from a checkout of it (make -C ai-video-detector_amd/csrc): every condition compares
with the parent's code, never with the code under test.

Workload: eight 60 s 48 kHz stereo int16 tracks, handed over in rounds of one chunk per track -- chunks of 1 s, 0.5 s and 4096 frames, from
pageable host memory and from device memory.  Forms:
  (a) in turn through "audio_slot" on the parent's library: eight calls a round;
  (b) the same on this build;
  (c) ONE call per round with an "audio_track_slot" list, on this build.
Each form runs in a process of its own, --rounds times, the order of the forms rotating from round to round; a process makes one unrecorded pass
and reports the median of three.  Reported: median and range over the rounds, ms per track (all calls of the pass over eight) and ms per round.
One SHA-256 per track over its concatenated records must come out the same from every form, chunk size and memory.
Conditions, all against the parent: (b) inside the parent's range of rounds; the one-track figures of profiles/audio_stream.json (whole, and slot 1
in 1 s chunks) inside the parent's range; bench.py inside the parent's range (--bench-rounds alternating runs each).  No ratio is fixed for (c):
it is reported against (a)."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ai-video-detector_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from audio_stream_bench import CHUNKS, RATE, SECONDS, WIN, Lib, spread, stereo_track  # noqa: E402

TRACKS = 8
END = 0x10


def outputs_after(frames, last):
    """M of the slots' rule at 48 kHz: U 1, D 3, T 100"""
    return -(-(frames if last else max(0, frames - 50)) // 3)


def in_turn(lib, ptrs, mem, n, chunk, outs):
    """round by round, stream k through audio slot k + 1 -> (ms of the pass, rounds)"""
    at, rounds = 0, 0
    wrote = [0] * TRACKS
    t0 = time.perf_counter()
    while at < n:
        m = min(chunk, n - at)
        for k in range(TRACKS):
            lib.option("audio_slot", k + 1)
            if at + m == n:
                lib.option("audio_end", 1)
            out = outs[k]
            lib.check(lib.L.avd_audio_features(lib.h, ptrs[k] + at * 4, mem, m, WIN, out.ctypes.data + wrote[k] * out.itemsize, len(out) - wrote[k]))
            wrote[k] = (-(-outputs_after(at + m, True) // WIN)) if at + m == n else outputs_after(at + m, False) // WIN
        at += m
        rounds += 1
    lib.option("audio_slot", 0)
    return (time.perf_counter() - t0) * 1e3, rounds


def mapped(lib, gather, mem, n, chunk, outs, scratch):
    """round by round, ONE call with a list: the round's chunks side by side in one buffer (a service's decoders write them there) -> (ms, rounds)"""
    at, rounds = 0, 0
    wrote = [0] * TRACKS
    t0 = time.perf_counter()
    while at < n:
        m = min(chunk, n - at)
        last = at + m == n
        ptr = gather(at, m)                                  # the round's buffer: [track 0's chunk | track 1's | ...]
        for k in range(1, TRACKS):
            lib.option("audio_cut", k * m)
        for k in range(TRACKS):
            lib.option("audio_track_slot", (k + 1) | (END if last else 0))
        after = (-(-outputs_after(at + m, True) // WIN)) if last else outputs_after(at + m, False) // WIN
        count = after - wrote[0]
        lib.check(lib.L.avd_audio_features(lib.h, ptr, mem, TRACKS * m, WIN, scratch.ctypes.data, TRACKS * count))
        for k in range(TRACKS):
            outs[k][wrote[k]:after] = scratch[k * count:(k + 1) * count]
            wrote[k] = after
        at += m
        rounds += 1
    return (time.perf_counter() - t0) * 1e3, rounds


def child(a):
    """one form in this process -> one JSON line"""
    import torch
    lib = Lib(os.path.abspath(a.lib))
    rng = np.random.default_rng(0)
    base = stereo_track(RATE, SECONDS, rng)
    wavs = [np.ascontiguousarray(np.roll(base, 977 * k, axis=0) // (1 + k % 3)) for k in range(TRACKS)]      # eight different tracks of one length
    n = len(base)
    nwin = -(-outputs_after(n, True) // WIN)
    from avd_hip import _lib
    rec = _lib.AUDIO_WINDOW_DTYPE
    devs = [torch.from_numpy(w).cuda() for w in wavs]
    # the mapped form's round buffer.  Host: the chunks are copied side by side round by round, INSIDE the measured time (a service whose decoders
    # write into one buffer saves that).  Device: the rounds' buffers are laid out before the pass, OUTSIDE the time -- decoders that decode on the
    # device write there
    host_round = np.zeros((TRACKS * 48000, 2), np.int16)
    torch.cuda.synchronize()
    for name, v in (("audio_format", 1), ("audio_rate", RATE), ("audio_channels", 2)):
        lib.option(name, v)
    result = {"form": a.child, "passes": {}, "sha": None}
    shas = set()

    def host_gather(at, m):
        for k in range(TRACKS):
            host_round[k * m:(k + 1) * m] = wavs[k][at:at + m]
        return host_round.ctypes.data
    keep = {}

    def dev_rounds(chunk):
        """every round's [track 0's chunk | track 1's | ...] one after another: round r begins TRACKS * r * chunk frames in"""
        keep.clear()
        keep["all"] = torch.cat([d[at:at + chunk] for at in range(0, n, chunk) for d in devs])
        torch.cuda.synchronize()

    def dev_gather(at, m):
        return keep["all"].data_ptr() + TRACKS * at * 4
    scratch = np.zeros(TRACKS * 8, rec)
    for where, mem in (("host", 0), ("device", 1)):
        ptrs = [w.ctypes.data for w in wavs] if mem == 0 else [d.data_ptr() for d in devs]
        for name, chunk in CHUNKS:
            ms = []
            if a.child == "c" and mem == 1:
                dev_rounds(chunk)
            for r in range(4):
                outs = [np.zeros(nwin + 1, rec) for _ in range(TRACKS)]
                if a.child == "c":
                    t, rounds = mapped(lib, host_gather if mem == 0 else dev_gather, mem, n, chunk, outs, scratch)
                else:
                    t, rounds = in_turn(lib, ptrs, mem, n, chunk, outs)
                shas.add(tuple(hashlib.sha256(o[:nwin].tobytes()).hexdigest() for o in outs))
                if r:
                    ms.append(t)
            result["passes"]["%s/%s" % (name, where)] = {"ms": statistics.median(ms), "rounds": rounds}
    assert len(shas) == 1, "the records of a track differ between chunk sizes or memories"
    result["sha"] = list(shas.pop())
    # the one-track figures of profiles/audio_stream.json: whole, and slot 1 in 1 s chunks (forms a and b)
    if a.child != "c":
        one = {}
        for where, ptr, mem in (("host", wavs[0].ctypes.data, 0), ("device", devs[0].data_ptr(), 1)):
            whole, slot = [], []
            for r in range(6):
                out = np.zeros(nwin + 1, rec)
                t = lib.whole(ptr, mem, n, out[:nwin])
                assert hashlib.sha256(out[:nwin].tobytes()).hexdigest() == result["sha"][0]
                t2 = lib.chunked(ptr, mem, n, 4, 48000, np.zeros(nwin + 1, rec))[0]
                if r:
                    whole.append(t); slot.append(t2)
            one[where] = {"whole_ms": statistics.median(whole), "slot_1s_ms": statistics.median(slot)}
        result["one_track"] = one
    lib.close()
    print(json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=False)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench-rounds", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_slot_map.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--lib", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_lib:
        raise SystemExit("--parent-lib is needed: every condition compares with the parent commit's library")
    from avd_hip import _lib
    _lib.build()
    libs = {"a": os.path.abspath(a.parent_lib), "b": _lib.SO_PATH, "c": _lib.SO_PATH}
    forms = ["a", "b", "c"]
    runs = {f: [] for f in forms}
    for r in range(max(3, a.rounds)):
        for f in forms[r % 3:] + forms[:r % 3]:
            # a process per form and round; a failure ends the run: nothing more is started on the device after it
            got = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f, "--lib", libs[f]], check=True, stdout=subprocess.PIPE, timeout=400)
            runs[f].append(json.loads(got.stdout.decode().strip().splitlines()[-1]))
            print("round %d form %s done" % (r, f), file=sys.stderr, flush=True)
    shas = {tuple(x["sha"]) for v in runs.values() for x in v}
    assert len(shas) == 1, "the records differ between the forms"
    result = {"device": "MI355X", "workload": "%d tracks of %d s, %d Hz, stereo int16; win %d" % (TRACKS, SECONDS, RATE, WIN), "rounds": max(3, a.rounds),
              "unit": "ms, wall clock of the blocking calls with their option calls; median, min and max over the rounds (a process each, order rotating)",
              "forms": {"a": "in turn through \"audio_slot\", the parent commit's library", "b": "in turn through \"audio_slot\", this build",
                        "c": "one call per round with an \"audio_track_slot\" list, this build (host memory: the round's chunks are copied side by side first, inside the time; device memory: the rounds' buffers are laid out before the pass, outside it)"},
              "records_sha256_per_track": list(shas.pop()), "records": "one SHA-256 per track, the same from every form, chunk size and memory", "passes": []}
    for key in runs["a"][0]["passes"]:
        rounds = runs["a"][0]["passes"][key]["rounds"]
        row = {"chunk/memory": key, "rounds_per_pass": rounds}
        for f in forms:
            ms = [x["passes"][key]["ms"] for x in runs[f]]
            row[f] = {"per_track_ms": spread([m / TRACKS for m in ms]), "per_round_ms": spread([m / rounds for m in ms])}
        lo, hi = row["a"]["per_round_ms"]["min"], row["a"]["per_round_ms"]["max"]
        row["b_median_within_parent_range"] = bool(lo <= row["b"]["per_round_ms"]["median"] <= hi)
        row["c_over_a"] = round(row["c"]["per_round_ms"]["median"] / row["a"]["per_round_ms"]["median"], 3)
        row["c_beats_a_by_more_than_the_spread"] = bool(row["c"]["per_round_ms"]["max"] < lo)
        result["passes"].append(row)
        print(json.dumps(row), flush=True)
    one = {}
    for where in ("host", "device"):
        for what in ("whole_ms", "slot_1s_ms"):
            p, b = [x["one_track"][where][what] for x in runs["a"]], [x["one_track"][where][what] for x in runs["b"]]
            one["%s/%s" % (what, where)] = {"parent": spread(p), "this_build": spread(b), "this_build_median_within_parent_range": bool(min(p) <= statistics.median(b) <= max(p))}
    result["one_track"] = one
    print(json.dumps(one), flush=True)
    if not a.no_bench:
        bench = {"this_build": [], "parent": []}
        order = [("this_build", None), ("parent", libs["a"])]
        for r in range(a.bench_rounds):
            for form, lib in order[r % 2:] + order[:r % 2]:
                cmd = [sys.executable, os.path.join(ROOT, "tools", "audio_stream_bench.py"), "--child-bench", "--bench-steps", str(a.bench_steps), "--bench-warmup", str(a.bench_warmup)]
                if lib:
                    cmd += ["--lib", lib]
                got = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=300)
                bench[form].append(json.loads(got.stdout.decode().strip().splitlines()[-1])["value"])
                print("bench round %d %s: %s" % (r, form, bench[form][-1]), file=sys.stderr, flush=True)
        lo, hi = min(bench["parent"]), max(bench["parent"])
        result["bench"] = {"this_build": {"median": statistics.median(bench["this_build"]), "runs": bench["this_build"]}, "parent": {"median": statistics.median(bench["parent"]), "runs": bench["parent"]},
                           "this_build_median_within_parent_range": bool(lo <= statistics.median(bench["this_build"]) <= hi)}
        print(json.dumps(result["bench"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
