#!/usr/bin/env python3
"""Engine.delta_apply and Engine.delta_pack against what they are measured against, in one process and on the same
inputs, per shape in bf16:
  * delta_apply (1 and 2 bits, a scale per row) next to a clone() of as many bytes as its algorithmic traffic,
    2 + 2 + bits / 8 bytes per element (the base read, the output written, the planes read): the plain-streaming rate of
    the box;
  * delta_apply next to Engine.lora_apply at r = 64, the other way a compact finetune becomes a tensor;
  * delta_pack at bits = 2 next to Engine.ties_merge at the same density with K = 1: the same three selection levels,
    then one fused pass.
Then one profiled call of each delta_pack flavour: the time of each kernel by HIP events.
Timing: HIP events around `reps` back-to-back calls after a warm-up, `--rounds` such windows per contender, the
contenders ALTERNATING inside every round; medians, with the max - min spread of the rounds in ms.  No threshold is
asserted: the ratios and the spreads are printed, one JSON line per case; --out appends them to a file.

    python tools/dpack_bench.py [--shapes 8192x8192,28672x8192] [--density 0.25] [--rank 64]
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
    ap.add_argument("--density", type=float, default=0.25)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per contender and case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "dpack_bench.txt"),
                    help="append the JSON lines to this file ('' for none)")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("dpack_bench: medians of at least five alternating rounds")
    if not torch.cuda.is_available():
        sys.exit("dpack_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    lines = []
    for rows, cols, _, base, fts, _ in cases(args.shapes, "1", torch.bfloat16, dev):
        ft, n = fts[0], base.numel()
        g = torch.Generator(device=dev).manual_seed(1)
        a = (torch.randn(args.rank, cols, generator=g, device=dev) * 0.02).to(torch.bfloat16)
        b = (torch.randn(rows, args.rank, generator=g, device=dev) * 0.02).to(torch.bfloat16)
        packs = {bits: eng.delta_pack(ft, base, bits=bits, density=args.density if bits == 2 else 1.0) for bits in (1, 2)}
        nbytes = {bits: n * 4 + bits * n // 8 for bits in (1, 2)}
        blobs = {bits: torch.empty(nbytes[bits] // 2, dtype=torch.uint8, device=dev) for bits in (1, 2)}
        contenders = {"apply_1bit": lambda: eng.delta_apply(base, packs[1][0], None, packs[1][2]),
                      "clone_1bit": lambda: blobs[1].clone(),
                      "apply_2bit": lambda: eng.delta_apply(base, packs[2][0], packs[2][1], packs[2][2]),
                      "clone_2bit": lambda: blobs[2].clone(),
                      "lora_apply": lambda: eng.lora_apply(base, a, b, 0.5),
                      "pack_1bit": lambda: eng.delta_pack(ft, base, bits=1),
                      "pack_2bit": lambda: eng.delta_pack(ft, base, bits=2, density=args.density),
                      "ties_k1": lambda: eng.ties_merge([ft], [base], [1.0], base, density=args.density)}
        times = alternate(contenders, args.seconds, args.rounds)
        rec = {"dpack_bench": f"{rows}x{cols}", "dtype": "bf16", "density": args.density, "lora_rank": args.rank,
               "apply_bytes": nbytes, "rounds": args.rounds}
        for bits in (1, 2):
            eng.ctx.profile(True)
            eng.ctx.profile_reset()
            try:
                rep = eng.delta_pack(ft, base, bits=bits, density=args.density if bits == 2 else 1.0)[3]
                table = eng.ctx.profile_table()
            finally:
                eng.ctx.profile(False)
            rec[f"pack_{bits}bit_kept_share"] = round(rep.kept / n, 4)
            rec[f"pack_{bits}bit_relative_residual"] = round(rep.rel_residual, 4)
            rec[f"pack_{bits}bit_kernels_ms"] = {kn: [int(table[kn][0]), round(float(table[kn][1]), 4)] for kn in table}
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            rec[f"{name}_ms"] = round(med[name], 4)
            rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
            rec[f"{name}_rounds_ms"] = [round(v, 4) for v in t]
        for bits in (1, 2):
            rec[f"apply_{bits}bit_GBps"] = round(nbytes[bits] / med[f"apply_{bits}bit"] / 1e6, 1)
            rec[f"apply_{bits}bit_share_of_8TBps"] = round(nbytes[bits] / med[f"apply_{bits}bit"] / 1e6 / HBM_PEAK_GBPS, 3)
            rec[f"apply_{bits}bit_ratio_to_clone"] = round(med[f"apply_{bits}bit"] / med[f"clone_{bits}bit"], 3)
            rec[f"apply_{bits}bit_ratio_to_lora_apply"] = round(med[f"apply_{bits}bit"] / med["lora_apply"], 3)
        rec["pack_2bit_ratio_to_ties_k1"] = round(med["pack_2bit"] / med["ties_k1"], 3)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del blobs, packs
    append_lines(lines, args.out or None)


if __name__ == "__main__":
    main()
