#!/usr/bin/env python3
"""One-off hunt for violators of the default Farneback mode's guarantee, on the GPU: the hold-out families of tests/holdout_families.py, composed
on the device, through the default mode (fast level kernels + exact re-run of flagged pairs) and through fb_mode = exact as the referee, with the
checker of the tests (holdout_families.check): a flagged pair bit-identical, an unflagged one within rel 1e-6 / abs 1e-7 on flow_mean / flow_var
and |delta flow_mean| <= 1e-6 * max(1, |m|).  tests/test_gpu_holdout.py is the fixed-seed slice of this run that stays in the suite.

    python tools/fuzz_fast_vs_exact.py --pairs 1000000 --seed0 1000000000 --out out/fuzz

--pairs   family pairs in all, spread evenly over the sixteen families and rounded up to whole chunks of 512 pairs (1 024 frames); the 511 pairs
          between them (scene cuts between unrelated content) are checked as well and reported as the row cut_between
--seed0   seed of pair i of family j is seed0 + j * 10 ** 8 + i; at least 10 ** 7, the tests' seeds lie below
--out     directory for the table (holdout_fuzz.txt) and every violator's two frames (.npz, with family, seed and the figures)
--cv2-model  option "cv2_model" of BOTH contexts (a mask of 1, 8 and 16; default 0): the referee is fb_mode = exact under the same mask, and
          violators are confirmed against the CPU oracle under oracle.model(mask)

Violators, and only they, are confirmed against the CPU oracle (is the referee right about them?).  Nothing is retried: the first error of the
library or the HIP runtime ends the run with what the table holds so far and a non-zero exit status.
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ai-video-detector_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import avd_hip  # noqa: E402
from tests import holdout_families as H  # noqa: E402

CHUNK = 512                   # pairs per chunk: 1 024 frames
FAMILY_STRIDE = 10 ** 8


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=10_000)
    ap.add_argument("--seed0", type=int, default=1_000_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "fuzz"))
    ap.add_argument("--cv2-model", type=lambda t: int(t, 0), default=0, help="option cv2_model of both contexts (mask of 1, 8, 16)")
    ap.add_argument("--commit", default=None, help="the commit the tree is at, where the run has no git to ask")
    a = ap.parse_args()
    if a.seed0 < H.FUZZ_SEED_MIN:
        ap.error(f"--seed0 must be at least {H.FUZZ_SEED_MIN}: the committed tests use the seeds below")
    os.makedirs(a.out, exist_ok=True)
    fam = H.holdout_families()
    chunks = max(1, -(-a.pairs // (CHUNK * len(fam))))
    if chunks * CHUNK > FAMILY_STRIDE:
        ap.error("--pairs: more than 10 ** 8 pairs per family")
    rows = {name: dict(pairs=0, flagged=0, solver=0, border=0, differ=0, max_dmean=0.0, violators=0) for name in list(fam) + [H.CUT_BETWEEN]}
    violators, error = [], None
    dev = torch.device("cuda", 0)
    t0 = time.time()
    oracle = None
    with avd_hip.Context(0) as default, avd_hip.Context(0) as exact:
        exact.set_option("fb_mode", 0)
        if a.cv2_model:
            default.set_option("cv2_model", a.cv2_model)
            exact.set_option("cv2_model", a.cv2_model)
        try:
            for c in range(chunks):
                for j, (name, make) in enumerate(fam.items()):
                    seeds = [a.seed0 + j * FAMILY_STRIDE + c * CHUNK + i for i in range(CHUNK)]
                    G = make(H.bank(), seeds, dev).reshape(2 * CHUNK, H.S, H.S)
                    r = H.run_default_and_exact(default, exact, G)
                    flagged = r["reserved"] != 0
                    bad = H.check(r["fm"], r["fv"], r["xm"], r["xv"], flagged)
                    if not (np.array_equal(r["rec_mean"], r["fm"]) and np.array_equal(r["rec_var"], r["fv"])):
                        p = int(np.nonzero((r["rec_mean"] != r["fm"]) | (r["rec_var"] != r["fv"]))[0][0])
                        bad.append((p, "records differ from avd_farneback_pairs", float(r["rec_mean"][p]), float(r["fm"][p])))
                    if not int(flagged.sum()) == r["rerun_records_call"] == r["rerun_pairs_call"]:
                        bad.append((0, "flag words and rerun_pairs disagree", int(flagged.sum()), (r["rerun_records_call"], r["rerun_pairs_call"])))
                    for row, sel in ((name, slice(0, None, 2)), (H.CUT_BETWEEN, slice(1, None, 2))):
                        s = H.summarise(r, sel)
                        for k in ("pairs", "flagged", "solver", "border", "differ"):
                            rows[row][k] += s[k]
                        rows[row]["max_dmean"] = max(rows[row]["max_dmean"], s["max_dmean"])
                    for p, kind, got, want in bad:
                        row = name if p % 2 == 0 else H.CUT_BETWEEN
                        rows[row]["violators"] += 1
                        prev, nxt = G[p].cpu().numpy(), G[p + 1].cpu().numpy()
                        if oracle is None:
                            from oracle import oracle as oracle
                            oracle.lib()
                        with oracle.model(a.cv2_model):
                            om, ov = oracle.flow_stats(oracle.farneback(prev, nxt))      # the CPU oracle's word on the violator
                        v = dict(family=name, row=row, seed=seeds[p // 2], seed_next=seeds[(p + 1) // 2], pair_in_chunk=p, kind=kind, got=str(got), want=str(want),
                                 reserved=int(r["reserved"][p]), default=(float(r["fm"][p]), float(r["fv"][p])), exact=(float(r["xm"][p]), float(r["xv"][p])),
                                 oracle=(float(om), float(ov)), exact_is_oracle=bool(r["xm"][p] == om and r["xv"][p] == ov))
                        violators.append(v)
                        np.savez_compressed(os.path.join(a.out, f"violator_{len(violators):04d}_{row}_{seeds[p // 2]}.npz"), prev=prev, next=nxt,
                                            **{k: np.array(str(x)) for k, x in v.items()})
                        print("VIOLATOR", v, flush=True)
                if c % 10 == 9 or c == chunks - 1:
                    done = sum(x["pairs"] for x in rows.values())
                    print(f"[fuzz] chunk {c + 1} of {chunks}: {done} pairs, {len(violators)} violators, {time.time() - t0:.0f} s", flush=True)
        except (avd_hip.AvdError, RuntimeError) as e:          # the library's status or torch's HIP error: stop here, retry nothing
            error = f"{type(e).__name__}: {e}"
            print("ERROR, the run ends here:", error, flush=True)
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
        except OSError:
            commit = "unknown"
    total = {k: (max if k == "max_dmean" else sum)(x[k] for x in rows.values()) for k in next(iter(rows.values()))}
    lines = ["default Farneback mode (fast level kernels + exact re-run of flagged pairs) against fb_mode = exact, hold-out families of tests/holdout_families.py",
             f"tools/fuzz_fast_vs_exact.py --pairs {a.pairs} --seed0 {a.seed0} --cv2-model {a.cv2_model}: {chunks} chunks of {CHUNK} pairs per family; seed of pair i of family j = seed0 + j * 10 ** 8 + i",
             f"commit {commit}; bank {H.BANK_SHA256[:16]}; {time.time() - t0:.0f} s" + (f"; ENDED BY AN ERROR: {error}" if error else ""),
             "flagged = re-run exactly (solver criterion: flag word & 0x0F, border-sign criterion: & 0xF0); differ = flow_mean or flow_var not bit-identical to exact;",
             "violator = outside the guarantee (flagged: bit-identical; unflagged: rel 1e-6 / abs 1e-7 on both statistics, |delta flow_mean| <= 1e-6 * max(1, |m|))",
             "",
             f"{'family':<18}{'pairs':>9}{'flagged':>9}{'solver':>9}{'border':>9}{'differ':>9}{'max |d mean|':>14}{'violators':>11}"]
    for name, x in list(rows.items()) + [("total", total)]:
        lines.append(f"{name:<18}{x['pairs']:>9}{x['flagged']:>9}{x['solver']:>9}{x['border']:>9}{x['differ']:>9}{x['max_dmean']:>14.3g}{x['violators']:>11}")
    for v in violators:
        lines.append("violator: " + repr(v))
    text = "\n".join(lines) + "\n"
    with open(os.path.join(a.out, "holdout_fuzz.txt"), "w") as f:
        f.write(text)
    print(text)
    return 2 if error else (1 if violators else 0)


if __name__ == "__main__":
    sys.exit(main())
