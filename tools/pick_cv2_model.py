#!/usr/bin/env python3
"""Which "cv2_model" does a real OpenCV follow?  Reads the stage-level golden vectors of tests/golden/make_cv2_golden.py and names the mask to
export as AVD_CV2_MODEL (include/avd.h, option "cv2_model").

    python tools/pick_cv2_model.py tests/golden/cv2_stage_golden.npz

For each of the eight masks the library accepts (combinations of 1 GAUSS_MULADD, 8 THREE_SCALES, 16 RESIZE_LERP) the CPU oracle's Farneback runs
on the file's own <clip>/small320 frames under oracle.model(mask), pair by pair, and is compared with what cv2 left there: the dense flow
<clip>/flow[p] where the file holds it, else <clip>/flow_mean[p] and flow_var[p].  Per mask: the pairs that are bit-identical, the largest
difference, and the first pairs that are not.  A mask matches when EVERY pair is bit-identical; the smallest such mask is named
("AVD_CV2_MODEL=<mask>", exit status 0), or the tool says that none matches (exit status 1): then the wheel does something the oracle does not
model, and the row with the most identical pairs says how close the model is.

The tool runs the oracle only (tools may; the product never imports it) and needs no GPU.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ai-video-detector_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402

MASKS = [a | b | c for c in (0, 16) for b in (0, 8) for a in (0, 1)]          # 0, 1, 8, 9, 16, 17, 24, 25
NAMES = {1: "GAUSS_MULADD", 8: "THREE_SCALES", 16: "RESIZE_LERP"}


def mask_name(mask: int) -> str:
    return " | ".join(n for b, n in NAMES.items() if mask & b) or "default model"


def clip_keys(z):
    """the clips of a golden file: every <key> with <key>/small320"""
    return sorted(k[:-len("/small320")] for k in z.files if k.endswith("/small320"))


def evaluate(z, oracle) -> dict:
    """mask -> {"pairs", "identical", "max_diff", "misses": [(clip, pair, what, difference)]}"""
    out = {}
    for mask in MASKS:
        row = dict(pairs=0, identical=0, max_diff=0.0, misses=[])
        with oracle.model(mask):
            for key in clip_keys(z):
                small = np.ascontiguousarray(z[key + "/small320"], dtype=np.uint8)
                dense = z[key + "/flow"] if key + "/flow" in z.files else None
                want_m = z[key + "/flow_mean"] if key + "/flow_mean" in z.files else None
                want_v = z[key + "/flow_var"] if key + "/flow_var" in z.files else None
                for p in range(len(small) - 1):
                    if not ((dense is not None and p < len(dense)) or (want_m is not None and want_v is not None and p < len(want_m))):
                        continue                      # nothing stored for this pair
                    flow = oracle.farneback(small[p], small[p + 1])
                    if dense is not None and p < len(dense):
                        ref = np.asarray(dense[p], np.float32).reshape(flow.shape)
                        same = np.array_equal(flow.view(np.uint32), ref.view(np.uint32))
                        diff, what = float(np.abs(flow.astype(np.float64) - ref.astype(np.float64)).max()), "flow"
                    else:
                        m, v = oracle.flow_stats(flow)
                        rm, rv = np.float32(want_m[p]), np.float32(want_v[p])
                        same = bool(m == rm and v == rv)
                        diff, what = max(abs(float(m) - float(rm)), abs(float(v) - float(rv))), "flow_mean / flow_var"
                    row["pairs"] += 1
                    row["identical"] += bool(same)
                    row["max_diff"] = max(row["max_diff"], diff)
                    if not same:
                        row["misses"].append((key, p, what, diff))
        out[mask] = row
    return out


def pick(rows: dict):
    """the smallest mask under which every pair is bit-identical, or None"""
    for mask in MASKS:
        if rows[mask]["pairs"] > 0 and rows[mask]["identical"] == rows[mask]["pairs"]:
            return mask
    return None


def report(rows: dict) -> str:
    lines = [f"{'mask':>4}  {'model':<44}{'pairs':>6}{'identical':>11}{'max |diff|':>13}  first pairs that differ"]
    for mask in MASKS:
        r = rows[mask]
        miss = ", ".join(f"{k}[{p}] ({what}: {d:.3g})" for k, p, what, d in r["misses"][:3]) + (" ..." if len(r["misses"]) > 3 else "")
        lines.append(f"{mask:>4}  {mask_name(mask):<44}{r['pairs']:>6}{r['identical']:>11}{r['max_diff']:>13.3g}  {miss}")
    best = pick(rows)
    if best is None:
        if not any(r["pairs"] for r in rows.values()):
            lines.append("no mask matches: the file holds no <clip>/small320 with a flow to compare")
        else:
            close = max(MASKS, key=lambda m: (rows[m]["identical"], -rows[m]["max_diff"]))
            lines.append(f"no mask matches: no combination of the modelled choices reproduces every pair (closest: {close}, {mask_name(close)}, "
                         f"{rows[close]['identical']} of {rows[close]['pairs']} pairs)")
    else:
        lines.append(f"AVD_CV2_MODEL={best}   ({mask_name(best)}: every pair bit-identical)")
    return "\n".join(lines)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("golden", help="cv2_stage_golden.npz as tests/golden/make_cv2_golden.py writes it")
    a = ap.parse_args(argv)
    from oracle import oracle
    oracle.lib()
    with np.load(a.golden) as z:
        rows = evaluate(z, oracle)
    print(report(rows))
    return 0 if pick(rows) is not None else 1


if __name__ == "__main__":
    sys.exit(main())
