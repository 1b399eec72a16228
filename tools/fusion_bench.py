#!/usr/bin/env python3
"""Engine.fusion_merge against what it is measured against, in one process and on the same inputs: per shape, the device
time of whole calls of `arcee_fusion` and `nearswap` on one finetune whose base is also the output base, next to
  * Engine.dare_merge (dare_linear) at density 1 with K = 1 - the yardstick of nearswap: the same tensor passes in one
    fused kernel,
  * Engine.ties_merge at density 0.2 with K = 1 - the yardstick of arcee_fusion's selection: three radix levels, then a
    fused pass, and
  * clone()s of as many bytes as each operator's algorithmic traffic (arcee_fusion: 12 tensor passes, nearswap: 4), half
    read and half written: the plain-streaming rate of the box.
Then the per-kernel profile of one arcee_fusion call (HIP events around every launch): the share of fusion_rowkl - two
software exponentials per element in unfused fp64 - is the number of interest.
Timing: HIP events around `reps` back-to-back calls after a warm-up, `--rounds` such windows per contender, the
contenders ALTERNATING inside every round; medians, with the max - min spread of the rounds in ms.  No threshold is
asserted: the ratios and the spreads are printed, one JSON line per case; --out appends them to a file.

    python tools/fusion_bench.py [--shapes 8192x8192,28672x8192] [--dtype bf16] [--iqr 1.5] [--t 0.003]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from delta_bench_common import DT, HBM_PEAK_GBPS, alternate, append_lines, cases

ARCEE_PASSES, NEARSWAP_PASSES = 12, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192x8192,28672x8192")
    ap.add_argument("--iqr", type=float, default=1.5)
    ap.add_argument("--t", type=float, default=3e-3, help="nearswap's t: one sigma of the deltas of these inputs")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per contender and case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("fusion_bench: the comparison wants at least five alternating rounds")
    if not torch.cuda.is_available():
        sys.exit("fusion_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    lines = []
    for rows, cols, _, base, fts, bases in cases(args.shapes, "1", DT[args.dtype], dev):
        ft = fts[0]
        tensor_bytes = base.numel() * base.element_size()
        blob_a = torch.empty(ARCEE_PASSES * tensor_bytes // 2, dtype=torch.uint8, device=dev)
        blob_n = torch.empty(NEARSWAP_PASSES * tensor_bytes // 2, dtype=torch.uint8, device=dev)
        contenders = {"arcee_fusion": lambda: eng.fusion_merge(ft, base, base, mode="arcee", iqr_mult=args.iqr),
                      "nearswap": lambda: eng.fusion_merge(ft, base, base, mode="nearswap", t=args.t),
                      "dare_linear": lambda: eng.dare_merge(fts, bases, [1.0], base, density=1.0, sign_election=False),
                      "ties": lambda: eng.ties_merge(fts, bases, [1.0], base, density=0.2),
                      "clone_arcee_bytes": lambda: blob_a.clone(),
                      "clone_nearswap_bytes": lambda: blob_n.clone()}
        times = alternate(contenders, args.seconds, args.rounds)
        _, rep = eng.fusion_merge(ft, base, base, mode="arcee", iqr_mult=args.iqr)
        _, nrep = eng.fusion_merge(ft, base, base, mode="nearswap", t=args.t)
        rec = {"fusion_bench": f"{rows}x{cols}", "dtype": args.dtype, "iqr": args.iqr, "t": args.t,
               "selected_share": round(rep.selected / base.numel(), 6), "clipped_share": round(nrep.clipped / base.numel(), 6),
               "arcee_bytes": ARCEE_PASSES * tensor_bytes, "nearswap_bytes": NEARSWAP_PASSES * tensor_bytes, "rounds": args.rounds}
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            rec[f"{name}_ms"] = round(med[name], 4)
            rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
            rec[f"{name}_rounds_ms"] = [round(v, 4) for v in t]
        rec["nearswap_GBps"] = round(NEARSWAP_PASSES * tensor_bytes / med["nearswap"] / 1e6, 1)
        rec["nearswap_share_of_8TBps"] = round(rec["nearswap_GBps"] / HBM_PEAK_GBPS, 3)
        rec["nearswap_ratio_to_clone"] = round(med["nearswap"] / med["clone_nearswap_bytes"], 3)
        rec["nearswap_ratio_to_dare_linear"] = round(med["nearswap"] / med["dare_linear"], 4)
        rec["arcee_GBps"] = round(ARCEE_PASSES * tensor_bytes / med["arcee_fusion"] / 1e6, 1)
        rec["arcee_ratio_to_clone"] = round(med["arcee_fusion"] / med["clone_arcee_bytes"], 3)
        rec["arcee_ratio_to_ties"] = round(med["arcee_fusion"] / med["ties"], 4)
        # the per-kernel profile of arcee_fusion: events around every launch (serialises the call), three calls
        eng.ctx.profile(True)
        eng.ctx.profile_reset()
        for _ in range(3):
            eng.fusion_merge(ft, base, base, mode="arcee", iqr_mult=args.iqr)
        table = eng.ctx.profile_table()
        eng.ctx.profile(False)
        total = sum(ms for _, ms in table.values())
        rec["profile_ms_per_call"] = {name: round(ms / 3, 4) for name, (_, ms) in table.items()}
        rec["profile_share"] = {name: round(ms / total, 4) for name, (_, ms) in table.items()}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del blob_a, blob_n
    append_lines(lines, args.out)


if __name__ == "__main__":
    main()
