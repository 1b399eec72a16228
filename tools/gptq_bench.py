#!/usr/bin/env python3
"""Engine.gptq_quant and Engine.gptq_dequant against what they are measured against, in one process and on the same
inputs, per shape in bf16 at group size 128:
  * both next to a clone() of as many bytes as their algorithmic traffic - quant reads the tensor once and writes the
    four tensors: 2 + 1 / 2 + 2 / g + 1 / (2 g) bytes per element (g_idx aside); dequant the same the other way;
  * both next to Engine.nv4_quant / Engine.nv4_dequant on the same tensor, the other 4-bit data type with real
    divisions.
Every call ends in its one readback (the counters / the flag word), which the timings include.
Timing: HIP events around `reps` back-to-back calls after a warm-up, `--rounds` such windows per contender, the
contenders ALTERNATING inside every round; medians, with the max - min spread of the rounds in ms.  No threshold is
asserted: the ratios and the spreads are printed, one JSON line per case; --out appends them to a file.

    python tools/gptq_bench.py [--shapes 8192x8192,28672x8192]
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
    ap.add_argument("--group-size", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per contender and case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "gptq_bench.txt"),
                    help="append the JSON lines to this file ('' for none)")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("gptq_bench: medians of at least five alternating rounds")
    if not torch.cuda.is_available():
        sys.exit("gptq_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    g = args.group_size
    lines = []
    for rows, cols, _, base, fts, _ in cases(args.shapes, "1", torch.bfloat16, dev):
        ft, n = fts[0], base.numel()
        *four, rep = eng.gptq_quant(ft, g)
        codes, sc, gs, _ = eng.nv4_quant(ft)
        nbytes = 2 * n + n // 2 + 2 * n // g + n // (2 * g)
        blob = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        contenders = {"quant": lambda: eng.gptq_quant(ft, g),
                      "dequant": lambda: eng.gptq_dequant(*four, torch.bfloat16),
                      "clone": lambda: blob.clone(),
                      "nv4_quant": lambda: eng.nv4_quant(ft),
                      "nv4_dequant": lambda: eng.nv4_dequant(codes, sc, gs, torch.bfloat16)}
        times = alternate(contenders, args.seconds, args.rounds)
        med = {name: statistics.median(t) for name, t in times.items()}
        rec = {"gptq_bench": f"{rows}x{cols}", "dtype": "bf16", "group_size": g, "bytes": nbytes, "groups": rep.groups,
               "clipped": rep.clipped, "scale_clamped": rep.scale_clamped, "rounds": args.rounds}
        for name, t in times.items():
            rec[f"{name}_ms"] = round(med[name], 4)
            rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
            rec[f"{name}_rounds_ms"] = [round(v, 4) for v in t]
        for name in ("quant", "dequant"):
            rec[f"{name}_GBps"] = round(nbytes / med[name] / 1e6, 1)
            rec[f"{name}_share_of_8TBps"] = round(nbytes / med[name] / 1e6 / HBM_PEAK_GBPS, 3)
            rec[f"{name}_ratio_to_clone"] = round(med[name] / med["clone"], 3)
            rec[f"{name}_ratio_to_nv4_{name}"] = round(med[name] / med[f"nv4_{name}"], 3)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del blob, four, codes, sc
    append_lines(lines, args.out or None)


if __name__ == "__main__":
    main()
