#!/usr/bin/env python3
"""Engine.tsv_merge against what it is measured against, in one process and on the same inputs: per shape x K, the time
of whole calls of `tsv` (rank 64, q = 2) on K finetunes with one shared base that is also the output base, next to
  * Engine.ties_merge at density 0.2 on the same tensors, and
  * a clone() of as many bytes as tsv's algorithmic traffic, (2 K (2 q + 3) + 2) * element size bytes per element (half
    read, half written): the plain-streaming rate of the box.
A tsv call synchronises the stream at every orthonormalisation and runs a Jacobi eigensolver on the host in between, so
its time is wall time between two device synchronisations; ties and clone are timed by HIP events around back-to-back
calls.  `--rounds` windows per contender, the contenders ALTERNATING inside every round; medians, with the max - min
spread of the rounds.  Then one profiled call: the time of each kernel by HIP events (profiled launches are serialised),
the host time inside xl_sym_eig of that call (debug query "eig_host_us") and what remains of its wall time (copies,
synchronisations, the fp64 whitening and core on the host).  For tsv_apply alone the FLOP rate 2 rows cols Rp / time is
set against the 155 TF the fp32 MFMA has measured.  No threshold is asserted: one JSON line per case; --out appends them.

    python tools/tsv_bench.py [--shapes 8192x8192,28672x8192] [--ks 2,3] [--rank 64] [--power-iters 2] [--dtype bf16]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from delta_bench_common import ALPHAS as alphas, DT, append_lines, cases, window

FP32_MFMA_TF = 155.0


def wall_ms(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192x8192,28672x8192")
    ap.add_argument("--ks", default="2,3")
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--power-iters", type=int, default=2)
    ap.add_argument("--density", type=float, default=0.2, help="of ties")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--seconds", type=float, default=1.0, help="timed work per streaming contender and case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("tsv_bench: the comparison wants at least five alternating rounds")
    if not torch.cuda.is_available():
        sys.exit("tsv_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    q = args.power_iters
    lines = []
    for rows, cols, k, base, fts, bases in cases(args.shapes, args.ks, DT[args.dtype], dev):
        nbytes = (2 * k * (2 * q + 3) + 2) * base.numel() * base.element_size()
        blob = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        tsv = lambda: eng.tsv_merge(fts, bases, alphas[:k], base, rank=args.rank, power_iters=q, key=1)
        streaming = {"ties": lambda: eng.ties_merge(fts, bases, alphas[:k], base, density=args.density), "clone": lambda: blob.clone()}
        tsv()                                                       # warm-up: the workspace, the code objects
        reps = {}
        for name, fn in streaming.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            reps[name] = max(5, int(args.seconds * 1e3 / args.rounds / max(window(fn, 3), 1e-3)))
        times = {"tsv": [], "ties": [], "clone": []}
        for _ in range(args.rounds):
            times["tsv"].append(wall_ms(tsv))
            for name, fn in streaming.items():
                times[name].append(window(fn, reps[name]))
        eng.ctx.profile(True)
        eng.ctx.profile_reset()
        try:
            eig0 = eng.ctx.debug_query("eig_host_us")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, rep = tsv()
            torch.cuda.synchronize()
            profiled_ms = (time.perf_counter() - t0) * 1e3
            eig_ms = (eng.ctx.debug_query("eig_host_us") - eig0) / 1e3
            table = eng.ctx.profile_table()
        finally:
            eng.ctx.profile(False)
        kernels = {name: [int(table[name][0]), round(float(table[name][1]), 4)] for name in table}
        kernel_ms = sum(v[1] for v in kernels.values())
        rec = {"tsv_bench": f"{rows}x{cols}", "dtype": args.dtype, "k": k, "rank": args.rank, "power_iters": q, "R": rep.R, "Rp": rep.Rp,
               "L": rep.width, "kept": [rep.kept_U, rep.kept_W], "share": [round(s, 4) for s in rep.share], "ties_density": args.density,
               "bytes": nbytes, "rounds": args.rounds}
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            rec[f"{name}_ms"] = round(med[name], 4)
            rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
            rec[f"{name}_rounds_ms"] = [round(v, 4) for v in t]
        rec["tsv_ratio_to_ties"] = round(med["tsv"] / med["ties"], 2)
        rec["tsv_ratio_to_clone"] = round(med["tsv"] / med["clone"], 2)
        rec["profiled_call_ms"] = round(profiled_ms, 3)
        rec["kernels_ms"] = kernels
        rec["kernels_sum_ms"] = round(kernel_ms, 3)
        rec["host_sym_eig_ms"] = round(eig_ms, 3)
        rec["host_other_ms"] = round(profiled_ms - kernel_ms - eig_ms, 3)
        apply_ms = kernels["tsv_apply"][1]
        rec["tsv_apply_TF"] = round(2.0 * rows * cols * rep.Rp / apply_ms / 1e9, 2)
        rec["tsv_apply_share_of_155TF"] = round(rec["tsv_apply_TF"] / FP32_MFMA_TF, 3)
        mm_flop = 2.0 * rows * cols * rep.width * k * (2 * q + 2)
        rec["xl_delta_mm_TF"] = round(mm_flop / kernels["xl_delta_mm"][1] / 1e9, 2)
        rec["xl_delta_mm_GBps"] = round(2.0 * base.numel() * base.element_size() * k * (2 * q + 2) / kernels["xl_delta_mm"][1] / 1e6, 1)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del blob
    append_lines(lines, args.out)


if __name__ == "__main__":
    main()
