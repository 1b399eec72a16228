#!/usr/bin/env python3
"""Engine.sce_merge next to what it is reported against, in one process and on the same inputs: per shape x K, the device
time of `sce` with selection (`--select-topk`, default 0.1) and without (select_topk 1.0) on K finetunes with one shared
base that is also the output base, next to
  * Engine.ties_merge at `--density` (default 0.2) on the same inputs: 4K + 5 tensor passes against SCE's 5K + 6, and
  * a clone() of as many bytes as each variant's algorithmic traffic, (5K + 6) resp. (2K + 3) * element size bytes per
    element (half read, half written): the plain-streaming rate of the box.
Timing: HIP events around `reps` back-to-back calls after a warm-up, `--rounds` such windows per contender, the
contenders ALTERNATING inside every round; medians, with the max - min spread of the rounds in ms.  Nothing is gated: the
numbers are reported.  One JSON line per case; --out appends them to a file.

    python tools/sce_bench.py [--shapes 8192x8192,28672x8192] [--ks 2,3] [--select-topk 0.1] [--density 0.2] [--dtype bf16]
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
    ap.add_argument("--select-topk", type=float, default=0.1)
    ap.add_argument("--density", type=float, default=0.2, help="of the ties run it is reported against")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per contender and case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sce_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    lines = []
    for rows, cols, k, base, fts, bases in cases(args.shapes, args.ks, DT[args.dtype], dev):
        es = base.numel() * base.element_size()
        nbytes = {"sce": (5 * k + 6) * es, "sce_all": (2 * k + 3) * es}
        blobs = {name: torch.empty(b // 2, dtype=torch.uint8, device=dev) for name, b in nbytes.items()}
        sce = lambda topk: (lambda: eng.sce_merge(fts, bases, alphas[:k], base, select_topk=topk))
        contenders = {"sce": sce(args.select_topk), "sce_all": sce(1.0),
                      "ties": lambda: eng.ties_merge(fts, bases, alphas[:k], base, density=args.density),
                      "clone_sce": lambda: blobs["sce"].clone(), "clone_sce_all": lambda: blobs["sce_all"].clone()}
        times = alternate(contenders, args.seconds, args.rounds)
        eng.ctx.profile(True)
        eng.ctx.profile_reset()
        _, rep = eng.sce_merge(fts, bases, alphas[:k], base, select_topk=args.select_topk)
        table = eng.ctx.profile_table()
        eng.ctx.profile(False)
        rec = {"sce_bench": f"{rows}x{cols}", "dtype": args.dtype, "k": k, "select_topk": args.select_topk, "ties_density": args.density,
               "nz_share": round(rep.nz / base.numel(), 6), "selected_over_asked": round(rep.selected / max(rep.k_keep, 1), 6),
               "weights": [round(w, 6) for w in rep.weights], "rounds": args.rounds,
               "kernel_ms": {n: round(v[1], 4) for n, v in sorted(table.items())}}
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            rec[f"{name}_ms"] = round(med[name], 4)
            rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
        for mode in ("sce", "sce_all"):
            rec[f"{mode}_bytes"] = nbytes[mode]
            rec[f"{mode}_GBps"] = round(nbytes[mode] / med[mode] / 1e6, 1)
            rec[f"{mode}_share_of_8TBps"] = round(nbytes[mode] / med[mode] / 1e6 / HBM_PEAK_GBPS, 3)
            rec[f"{mode}_ratio_to_clone"] = round(med[mode] / med[f"clone_{mode}"], 3)
            rec[f"{mode}_ratio_to_ties"] = round(med[mode] / med["ties"], 4)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del blobs
    append_lines(lines, args.out)


if __name__ == "__main__":
    main()
