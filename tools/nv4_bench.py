#!/usr/bin/env python3
"""Engine.nv4_quant and Engine.nv4_dequant against what they are measured against, in one process and on the same
inputs, per shape in bf16:
  * both next to a clone() of as many bytes as their algorithmic traffic - quant reads the tensor TWICE (the maximum,
    then the codes): 4 + 9 / 16 bytes per element; dequant 2 + 9 / 16;
  * both next to Engine.mx4_quant / Engine.mx4_dequant on the same tensor, the other 4-bit data type.
Every call ends in its one readback (the counters and g / the flag word), which the timings include.
Timing: HIP events around `reps` back-to-back calls after a warm-up, `--rounds` such windows per contender, the
contenders ALTERNATING inside every round; medians, with the max - min spread of the rounds in ms.  No threshold is
asserted: the ratios and the spreads are printed, one JSON line per case; --out appends them to a file.

    python tools/nv4_bench.py [--shapes 8192x8192,28672x8192]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from delta_bench_common import HBM_PEAK_GBPS, alternate, append_lines, cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192x8192,28672x8192")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per contender and case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "nv4_bench.txt"),
                    help="append the JSON lines to this file ('' for none)")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("nv4_bench: medians of at least five alternating rounds")
    if not torch.cuda.is_available():
        sys.exit("nv4_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    lines = []
    for rows, cols, _, base, fts, _ in cases(args.shapes, "1", torch.bfloat16, dev):
        ft, n = fts[0], base.numel()
        codes, sc, g, rep = eng.nv4_quant(ft)
        codes4, sc4, _ = eng.mx4_quant(ft)
        nbytes = {"quant": 4 * n + n // 2 + n // 16, "dequant": 2 * n + n // 2 + n // 16}
        blobs = {k: torch.empty(v // 2, dtype=torch.uint8, device=dev) for k, v in nbytes.items()}
        contenders = {"quant": lambda: eng.nv4_quant(ft),
                      "dequant": lambda: eng.nv4_dequant(codes, sc, g, torch.bfloat16),
                      "quant_clone": lambda: blobs["quant"].clone(),
                      "dequant_clone": lambda: blobs["dequant"].clone(),
                      "mx4_quant": lambda: eng.mx4_quant(ft),
                      "mx4_dequant": lambda: eng.mx4_dequant(codes4, sc4, torch.bfloat16)}
        times = alternate(contenders, args.seconds, args.rounds)
        med = {name: statistics.median(t) for name, t in times.items()}
        rec = {"nv4_bench": f"{rows}x{cols}", "dtype": "bf16", "quant_bytes": nbytes["quant"], "dequant_bytes": nbytes["dequant"],
               "blocks": rep.blocks, "saturated": rep.saturated, "zero_scale_blocks": rep.zero_scale_blocks, "rounds": args.rounds}
        for name, t in times.items():
            rec[f"{name}_ms"] = round(med[name], 4)
            rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
            rec[f"{name}_rounds_ms"] = [round(v, 4) for v in t]
        for name in ("quant", "dequant"):
            rec[f"{name}_GBps"] = round(nbytes[name] / med[name] / 1e6, 1)
            rec[f"{name}_share_of_8TBps"] = round(nbytes[name] / med[name] / 1e6 / HBM_PEAK_GBPS, 3)
            rec[f"{name}_ratio_to_clone"] = round(med[name] / med[f"{name}_clone"], 3)
            rec[f"{name}_ratio_to_mx4_{name}"] = round(med[name] / med[f"mx4_{name}"], 3)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del blobs, codes, sc, codes4, sc4
    append_lines(lines, args.out or None)


if __name__ == "__main__":
    main()
