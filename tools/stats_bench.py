#!/usr/bin/env python3
"""Engine.delta_stats against what it is measured against, in one process and on the same inputs: per shape x K, the
device time of whole calls at m = 1 (density 0.2) and at m = 4 (0.05, 0.1, 0.2, 0.5) on K finetunes with one shared
base, next to
  * Engine.ties_merge at density 0.2 - the same three selection levels, 4K + 5 tensor passes against at most 5 (K + 1)
    here, and
  * a clone() of as many bytes as the call's algorithmic traffic, 5 (K + 1) * element size bytes per element read (a
    clone reads half of its bytes and writes the other half): the plain-streaming rate of the box.
What m = 4 costs over m = 1 is printed as a ratio, and - from the per-kernel profile of a few extra calls - split into
the selection (stats_hist + stats_select, which should not grow with m), the fused pass and the Gram.
Timing: HIP events around `reps` back-to-back calls after a warm-up, `--rounds` such windows per contender, the
contenders ALTERNATING inside every round; medians, with the max - min spread of the rounds in ms.  No threshold is
asserted: the ratios and the spreads are printed, one JSON line per case; --out appends them to a file.

    python tools/stats_bench.py [--shapes 8192x8192,28672x8192] [--ks 2,3] [--dtype bf16]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from delta_bench_common import ALPHAS as alphas, DT, alternate, append_lines, cases

M1 = (0.2,)
M4 = (0.05, 0.1, 0.2, 0.5)
GROUPS = {"selection": ("stats_hist", "stats_select"), "pass": ("stats_pass", "stats_fold"), "gram": ("geo_gram", "geo_gram_fold")}


def kernel_ms(eng, fn, calls=5):
    """{group: ms per call} from the library's per-kernel profile"""
    fn()
    eng.ctx.profile(True)
    eng.ctx.profile_reset()
    try:
        for _ in range(calls):
            fn()
        table = eng.ctx.profile_table()
    finally:
        eng.ctx.profile(False)
    return {g: round(sum(table.get(n, (0, 0.0))[1] for n in names) / calls, 4) for g, names in GROUPS.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192x8192,28672x8192")
    ap.add_argument("--ks", default="2,3")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per contender and case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("stats_bench: the comparison wants at least five alternating rounds")
    if not torch.cuda.is_available():
        sys.exit("stats_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    lines = []
    for rows, cols, k, base, fts, bases in cases(args.shapes, args.ks, DT[args.dtype], dev):
        nbytes = 5 * (k + 1) * base.numel() * base.element_size()
        blob = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        stats = lambda dens: (lambda: eng.delta_stats(fts, bases, alphas[:k], dens))
        contenders = {"stats_m1": stats(M1), "stats_m4": stats(M4),
                      "ties": lambda: eng.ties_merge(fts, bases, alphas[:k], base, density=0.2),
                      "clone": lambda: blob.clone()}
        times = alternate(contenders, args.seconds, args.rounds)
        rep = eng.delta_stats(fts, bases, alphas[:k], M4)
        rec = {"stats_bench": f"{rows}x{cols}", "dtype": args.dtype, "k": k, "densities_m1": list(M1), "densities_m4": list(M4),
               "conflict_share_m4": [round(c / rep.n, 6) for c in rep.conflict], "bytes": nbytes, "rounds": args.rounds}
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            rec[f"{name}_ms"] = round(med[name], 4)
            rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
            rec[f"{name}_rounds_ms"] = [round(v, 4) for v in t]
        rec["m4_ratio_to_m1"] = round(med["stats_m4"] / med["stats_m1"], 4)
        rec["stats_m1_ratio_to_ties"] = round(med["stats_m1"] / med["ties"], 4)
        rec["stats_m4_ratio_to_ties"] = round(med["stats_m4"] / med["ties"], 4)
        rec["stats_m1_ratio_to_clone"] = round(med["stats_m1"] / med["clone"], 3)
        rec["stats_m1_GBps"] = round(nbytes / med["stats_m1"] / 1e6, 1)
        rec["kernels_m1_ms"] = kernel_ms(eng, stats(M1))
        rec["kernels_m4_ms"] = kernel_ms(eng, stats(M4))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del blob
    append_lines(lines, args.out)


if __name__ == "__main__":
    main()
