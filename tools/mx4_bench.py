#!/usr/bin/env python3
"""Engine.mx4_quant and Engine.mx4_dequant against what they are measured against, in one process and on the same
inputs, per shape in bf16:
  * both next to a clone() of as many bytes as their algorithmic traffic, 2 + 17 / 32 bytes per element (2 read and half
    a byte of codes plus 1 / 32 of a scale byte written, or the reverse): the plain-streaming rate of the box;
  * both next to Engine.fp8_quant / Engine.fp8_dequant on the same tensor, the other on-disk data type.
Every call ends in its one readback (the counters / the flag word), which the timings include.
Timing: HIP events around `reps` back-to-back calls after a warm-up, `--rounds` such windows per contender, the
contenders ALTERNATING inside every round; medians, with the max - min spread of the rounds in ms.  No threshold is
asserted: the ratios and the spreads are printed, one JSON line per case; --out appends them to a file.

    python tools/mx4_bench.py [--shapes 8192x8192,28672x8192]
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
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "mx4_bench.txt"),
                    help="append the JSON lines to this file ('' for none)")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("mx4_bench: medians of at least five alternating rounds")
    if not torch.cuda.is_available():
        sys.exit("mx4_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    lines = []
    for rows, cols, _, base, fts, _ in cases(args.shapes, "1", torch.bfloat16, dev):
        ft, n = fts[0], base.numel()
        codes, sc, rep = eng.mx4_quant(ft)
        codes8, sc8, _ = eng.fp8_quant(ft)
        nbytes = 2 * n + n // 2 + n // 32
        blob = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        contenders = {"quant": lambda: eng.mx4_quant(ft),
                      "dequant": lambda: eng.mx4_dequant(codes, sc, torch.bfloat16),
                      "clone": lambda: blob.clone(),
                      "fp8_quant": lambda: eng.fp8_quant(ft),
                      "fp8_dequant": lambda: eng.fp8_dequant(codes8, sc8, torch.bfloat16)}
        times = alternate(contenders, args.seconds, args.rounds)
        med = {name: statistics.median(t) for name, t in times.items()}
        rec = {"mx4_bench": f"{rows}x{cols}", "dtype": "bf16", "bytes": nbytes, "blocks": rep.blocks, "saturated": rep.saturated,
               "rounds": args.rounds}
        for name, t in times.items():
            rec[f"{name}_ms"] = round(med[name], 4)
            rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
            rec[f"{name}_rounds_ms"] = [round(v, 4) for v in t]
        for name in ("quant", "dequant"):
            rec[f"{name}_GBps"] = round(nbytes / med[name] / 1e6, 1)
            rec[f"{name}_share_of_8TBps"] = round(nbytes / med[name] / 1e6 / HBM_PEAK_GBPS, 3)
            rec[f"{name}_ratio_to_clone"] = round(med[name] / med["clone"], 3)
            rec[f"{name}_ratio_to_fp8_{name}"] = round(med[name] / med[f"fp8_{name}"], 3)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del blob, codes, sc, codes8, sc8
    append_lines(lines, args.out or None)


if __name__ == "__main__":
    main()
