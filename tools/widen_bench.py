#!/usr/bin/env python3
"""Engine.widen_merge against what it is measured against, in one process and on the same inputs: per shape x K, the device
time of whole calls of `widen` on K finetunes with one shared base that is also the output base, next to
  * Engine.geo_merge in mode model_stock - the nearest existing operator: statistics (an ordered fp64 Gram) plus a combine
    pass, 2K + 3 tensor passes where widen has 3K + 2 and the ranking,
  * Engine.dare_merge (dare_linear) at density 1: the one-pass operator widen reduces to when every weight is alpha, and
  * a clone() of as many bytes as widen's algorithmic traffic, (3K + 2) * element size bytes per element (half read, half
    written): the plain-streaming rate of the box.
Then one profiled call: the time of each kernel by HIP events (profiled launches are serialised, so their sum exceeds the
whole call).
Timing: HIP events around `reps` back-to-back calls after a warm-up, `--rounds` such windows per contender, the
contenders ALTERNATING inside every round; medians, with the max - min spread of the rounds in ms.  No threshold is
asserted: the ratios and the spreads are printed, one JSON line per case; --out appends them to a file.

    python tools/widen_bench.py [--shapes 8192x8192,28672x8192] [--ks 2,3] [--dtype bf16]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from delta_bench_common import ALPHAS as alphas, DT, HBM_PEAK_GBPS, alternate, append_lines, cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192x8192,28672x8192")
    ap.add_argument("--ks", default="2,3")
    ap.add_argument("--ratio", type=float, default=1.0)
    ap.add_argument("--calibration", type=float, default=1.0)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per contender and case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "widen_bench.txt"),
                    help="append the JSON lines to this file ('' for none)")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("widen_bench: medians of at least five alternating rounds")
    if not torch.cuda.is_available():
        sys.exit("widen_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    lines = []
    for rows, cols, k, base, fts, bases in cases(args.shapes, args.ks, DT[args.dtype], dev):
        nbytes = (3 * k + 2) * base.numel() * base.element_size()
        blob = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        widen = lambda: eng.widen_merge(fts, bases, alphas[:k], base, ratio=args.ratio, calibration=args.calibration)
        contenders = {"widen": widen,
                      "model_stock": lambda: eng.geo_merge(fts, bases, alphas[:k], base, mode="model_stock"),
                      "dare_linear": lambda: eng.dare_merge(fts, bases, alphas[:k], base, density=1.0, sign_election=False),
                      "clone": lambda: blob.clone()}
        times = alternate(contenders, args.seconds, args.rounds)
        eng.ctx.profile(True)
        eng.ctx.profile_reset()
        try:
            _, rep = widen()
            table = eng.ctx.profile_table()
        finally:
            eng.ctx.profile(False)
        rec = {"widen_bench": f"{rows}x{cols}", "dtype": args.dtype, "k": k, "ratio": args.ratio, "calibration": args.calibration,
               "calibrated_share": [[round(c / cols, 4) for c in row] for row in rep.calibrated], "bytes": nbytes, "rounds": args.rounds}
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            rec[f"{name}_ms"] = round(med[name], 4)
            rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
            rec[f"{name}_rounds_ms"] = [round(v, 4) for v in t]
        rec["widen_GBps"] = round(nbytes / med["widen"] / 1e6, 1)
        rec["widen_share_of_8TBps"] = round(nbytes / med["widen"] / 1e6 / HBM_PEAK_GBPS, 3)
        for other in ("clone", "model_stock", "dare_linear"):
            rec[f"widen_ratio_to_{other}"] = round(med["widen"] / med[other], 3)
        rec["kernels_ms"] = {name: [int(table[name][0]), round(float(table[name][1]), 4)] for name in table}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del blob
    append_lines(lines, args.out or None)


if __name__ == "__main__":
    main()
