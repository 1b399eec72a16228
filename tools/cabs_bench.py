#!/usr/bin/env python3
"""Engine.cabs_merge against what it is measured against, in one process and on the same inputs: per shape x K, the device
time of whole calls of `cabs` (conflict-aware on and off) on K finetunes with one shared base that is also the output
base, next to
  * Engine.dare_merge (dare_linear) at density 1: the same K + 2 tensor passes in one fused kernel, without a selection -
    the natural yardstick,
  * Engine.ties_merge at density 0.25: a comparable trim by a GLOBAL cut, 4K + 5 tensor passes, and
  * a clone() of as many bytes as cabs's algorithmic traffic, (K + 2) * element size bytes per element (half read, half
    written): the plain-streaming rate of the box.
Then one profiled call of each cabs flavour: the time of each kernel by HIP events.
Timing: HIP events around `reps` back-to-back calls after a warm-up, `--rounds` such windows per contender, the
contenders ALTERNATING inside every round; medians, with the max - min spread of the rounds in ms.  No threshold is
asserted: the ratios and the spreads are printed, one JSON line per case; --out appends them to a file.

    python tools/cabs_bench.py [--shapes 8192x8192,28672x8192] [--ks 2,3] [--dtype bf16] [--n 64] [--m 256]
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
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per contender and case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "cabs_bench.txt"),
                    help="append the JSON lines to this file ('' for none)")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("cabs_bench: medians of at least five alternating rounds")
    if not torch.cuda.is_available():
        sys.exit("cabs_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    lines = []
    for rows, cols, k, base, fts, bases in cases(args.shapes, args.ks, DT[args.dtype], dev):
        nbytes = (k + 2) * base.numel() * base.element_size()
        blob = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        cabs = lambda ca: eng.cabs_merge(fts, bases, alphas[:k], base, n_keep=args.n, group=args.m, conflict_aware=ca)
        contenders = {"cabs": lambda: cabs(True),
                      "cabs_independent": lambda: cabs(False),
                      "dare_linear": lambda: eng.dare_merge(fts, bases, alphas[:k], base, density=1.0, sign_election=False),
                      "ties": lambda: eng.ties_merge(fts, bases, alphas[:k], base, density=0.25),
                      "clone": lambda: blob.clone()}
        times = alternate(contenders, args.seconds, args.rounds)
        rec = {"cabs_bench": f"{rows}x{cols}", "dtype": args.dtype, "k": k, "n_keep": args.n, "group": args.m, "bytes": nbytes,
               "rounds": args.rounds}
        for ca, name in ((True, "cabs"), (False, "cabs_independent")):
            eng.ctx.profile(True)
            eng.ctx.profile_reset()
            try:
                _, rep = cabs(ca)
                table = eng.ctx.profile_table()
            finally:
                eng.ctx.profile(False)
            rec[f"{name}_kept_share"] = [round(c / rep.n, 4) for c in rep.kept]
            rec[f"{name}_surplus"] = rep.surplus
            rec[f"{name}_covered_share"] = round(rep.covered / rep.n, 4)
            rec[f"{name}_overlap_share"] = round(rep.overlap / rep.n, 4)
            rec[f"{name}_kernels_ms"] = {kn: [int(table[kn][0]), round(float(table[kn][1]), 4)] for kn in table}
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            rec[f"{name}_ms"] = round(med[name], 4)
            rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
            rec[f"{name}_rounds_ms"] = [round(v, 4) for v in t]
        rec["cabs_GBps"] = round(nbytes / med["cabs"] / 1e6, 1)
        rec["cabs_share_of_8TBps"] = round(nbytes / med["cabs"] / 1e6 / HBM_PEAK_GBPS, 3)
        for other in ("clone", "dare_linear", "ties", "cabs_independent"):
            rec[f"cabs_ratio_to_{other}"] = round(med["cabs"] / med[other], 3)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del blob
    append_lines(lines, args.out or None)


if __name__ == "__main__":
    main()
