#!/usr/bin/env python3
"""Time Engine.lora_extract at model shapes against two yardsticks measured in the same process:
  - a clone() of (2q + 2) * 2 tensors' bytes: what the delta products must at least read (finetune + base per product);
  - torch.svd_lowrank (the same q) on the materialised fp32 delta.
Also prints the per-kernel profile of one call, which shows how much of the call the host eigensolver and its
synchronisations take (the wall time minus the kernels' time).
usage: python tools/extract_bench.py [--rank 64] [--power-iters 2] [--reps 5] [--shapes 8192x8192,28672x8192]"""
import argparse
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--power-iters", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="8192x8192,28672x8192")
    args = ap.parse_args()
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    q, r = args.power_iters, args.rank
    for shape in args.shapes.split(","):
        rows, cols = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(1)
        base = (0.02 * torch.randn(rows, cols, device="cuda", generator=g)).bfloat16()
        ft = (base.float() + 0.003 * torch.randn(rows, cols, device="cuda", generator=g)).bfloat16()
        t_x = timed(lambda: eng.lora_extract(ft, base, r, power_iters=q, name="bench"), args.reps)
        t_c = timed(lambda: [(ft.clone(), base.clone()) for _ in range(2 * q + 2)], args.reps)
        delta = ft.float() - base.float()
        t_s = timed(lambda: torch.svd_lowrank(delta, q=r + 8, niter=q), max(1, args.reps // 2))
        eng.ctx.profile(True)
        eng.ctx.profile_reset()
        t0 = time.perf_counter()
        eng.lora_extract(ft, base, r, power_iters=q, name="bench")
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        table = eng.ctx.profile_table()
        eng.ctx.profile(False)
        kern = sum(ms for _, ms in table.values())
        print(f"{rows} x {cols} bf16, r = {r}, q = {q}: lora_extract {t_x:.2f} ms; clone of {(2 * q + 2) * 2} tensors {t_c:.2f} ms; "
              f"torch.svd_lowrank on the fp32 delta {t_s:.2f} ms")
        print(f"  profiled call: wall {wall:.2f} ms, kernels {kern:.2f} ms, host (eigensolver, copies, synchronisations) {wall - kern:.2f} ms")
        for name, (n, ms) in sorted(table.items(), key=lambda kv: -kv[1][1]):
            print(f"    {name:14s} {n:3d} launches {ms:9.3f} ms")
        del delta


if __name__ == "__main__":
    main()
