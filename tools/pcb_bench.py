#!/usr/bin/env python3
"""Engine.pcb_merge against what it is measured against, in one process and on the same inputs: per shape x K, the device
time of whole calls of `pcb` on K finetunes with one shared base that is also the output base, next to
  * Engine.ties_merge at density 0.2 - the nearest existing operator: one three-level select (4K + 5 tensor passes) where
    pcb has two and two transcendentals per entry and pass, and
  * a clone() of as many bytes as pcb's algorithmic traffic, (7K + 8) * element size bytes per element (half read, half
    written): the plain-streaming rate of the box.
Then one profiled call: the time of each kernel by HIP events (profiled launches are serialised, so their sum exceeds the
whole call).
Timing: HIP events around `reps` back-to-back calls after a warm-up, `--rounds` such windows per contender, the
contenders ALTERNATING inside every round; medians, with the max - min spread of the rounds in ms.  No threshold is
asserted: the ratios and the spreads are printed, one JSON line per case; --out appends them to a file.

    python tools/pcb_bench.py [--shapes 8192x8192,28672x8192] [--ks 2,3] [--ratio 0.1] [--clip 0.0001] [--dtype bf16]
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
    ap.add_argument("--ratio", type=float, default=0.1)
    ap.add_argument("--clip", type=float, default=0.0001)
    ap.add_argument("--density", type=float, default=0.2, help="of ties")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per contender and case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("pcb_bench: the comparison wants at least five alternating rounds")
    if not torch.cuda.is_available():
        sys.exit("pcb_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    lines = []
    for rows, cols, k, base, fts, bases in cases(args.shapes, args.ks, DT[args.dtype], dev):
        nbytes = (7 * k + 8) * base.numel() * base.element_size()
        blob = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        pcb = lambda: eng.pcb_merge(fts, bases, alphas[:k], base, ratio=args.ratio, clip=args.clip)
        contenders = {"pcb": pcb,
                      "ties": lambda: eng.ties_merge(fts, bases, alphas[:k], base, density=args.density),
                      "clone": lambda: blob.clone()}
        times = alternate(contenders, args.seconds, args.rounds)
        eng.ctx.profile(True)
        eng.ctx.profile_reset()
        try:
            _, rep = pcb()
            table = eng.ctx.profile_table()
        finally:
            eng.ctx.profile(False)
        rec = {"pcb_bench": f"{rows}x{cols}", "dtype": args.dtype, "k": k, "ratio": args.ratio, "clip": args.clip,
               "ties_density": args.density, "covered_share": round(rep.covered / base.numel(), 6),
               "contested_share": round(rep.contested / base.numel(), 6), "bytes": nbytes, "rounds": args.rounds}
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            rec[f"{name}_ms"] = round(med[name], 4)
            rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
            rec[f"{name}_rounds_ms"] = [round(v, 4) for v in t]
        rec["pcb_GBps"] = round(nbytes / med["pcb"] / 1e6, 1)
        rec["pcb_share_of_8TBps"] = round(nbytes / med["pcb"] / 1e6 / HBM_PEAK_GBPS, 3)
        rec["pcb_ratio_to_clone"] = round(med["pcb"] / med["clone"], 3)
        rec["pcb_ratio_to_ties"] = round(med["pcb"] / med["ties"], 3)
        rec["kernels_ms"] = {name: [int(table[name][0]), round(float(table[name][1]), 4)] for name in table}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del blob
    append_lines(lines, args.out)


if __name__ == "__main__":
    main()
