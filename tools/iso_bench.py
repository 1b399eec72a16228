#!/usr/bin/env python3
"""Engine.iso_merge and its GEMM, measured in one process and on the same inputs.

  1. `iso_gemm` alone through the probe, per form - NT (A B^T), NT symmetric (the lower tiles, mirrored) and NN (A B) - at
     --gemm-shapes: the FLOP rate 2 M N K / time (the symmetric mode: of the M (M + 128) / 2 x N outputs it computes)
     against the 155 TF the fp32 MFMA has measured and the 28 to 30 TF of tsv_apply (profiles/tsv_bench.txt).  The
     forms ALTERNATE inside every round; medians of --rounds windows timed by HIP events, with the max - min spread.
  2. Whole calls of `iso_c` per shape x K (K finetunes with one shared base that is also the output base): a call
     synchronises the stream once per iteration, so its time is wall time between two device synchronisations; medians
     of --rounds calls with the spread, the steps, the GEMM count and the last residual.  Then one profiled call: the
     time of each kernel by HIP events (profiled launches are serialised) and what remains of its wall time.
  3. The same function written with torch: `torch.linalg.svd` of the fp32 task sum on the device, mean(S) U V^T, at
     --svd-shape (a shape where it ends within the time a step may take), alternating with iso_merge on the same inputs.
No threshold is asserted: one JSON line per case; --out appends them.  What a run leaves out is listed as not measured.

    python tools/iso_bench.py [--shapes 8192x8192,28672x8192] [--ks 2,3] [--gemm-shapes 4096x4096x4096,...] [--svd-shape 2048x2048]
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
TSV_APPLY_TF = (28.0, 30.0)


def wall_ms(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(rec, name, t):
    rec[f"{name}_ms"] = round(statistics.median(t), 4)
    rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
    rec[f"{name}_rounds_ms"] = [round(v, 4) for v in t]


def gemm_case(eng, M, N, K, rounds):
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g, device=dev)
    bt = torch.randn(N, K, generator=g, device=dev)
    b = torch.randn(K, N, generator=g, device=dev)
    forms = {"nt": lambda: eng.iso_gemm(a, bt, form=0), "nn": lambda: eng.iso_gemm(a, b, form=1)}
    flop = {"nt": 2.0 * M * N * K, "nn": 2.0 * M * N * K}
    if M == N:
        forms["nt_sym"] = lambda: eng.iso_gemm(a, a, form=0, sym=True)
        tiles = (M + 127) // 128
        flop["nt_sym"] = 2.0 * (tiles * (tiles + 1) // 2) * 128 * 128 * K
    reps = {}
    for name, fn in forms.items():
        fn()
        torch.cuda.synchronize()
        reps[name] = max(2, min(50, int(200.0 / max(window(fn, 1), 1e-3))))
    times = {name: [] for name in forms}
    for _ in range(rounds):
        for name, fn in forms.items():
            times[name].append(window(fn, reps[name]))
    rec = {"iso_gemm_bench": f"{M}x{N}x{K}", "rounds": rounds, "ceiling_TF": FP32_MFMA_TF, "tsv_apply_TF": list(TSV_APPLY_TF)}
    for name, t in times.items():
        spread(rec, name, t)
        rec[f"{name}_TF"] = round(flop[name] / statistics.median(t) / 1e9, 2)
        rec[f"{name}_share_of_155TF"] = round(rec[f"{name}_TF"] / FP32_MFMA_TF, 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192x8192,28672x8192")
    ap.add_argument("--ks", default="2,3")
    ap.add_argument("--gemm-shapes", default="4096x4096x4096,8192x8192x8192,1024x8192x1024,8192x28672x8192")
    ap.add_argument("--svd-shape", default="2048x2048")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--max-iter", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("iso_bench: the comparison wants at least five alternating rounds")
    if not torch.cuda.is_available():
        sys.exit("iso_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for shape in [s for s in args.gemm_shapes.split(",") if s]:
        M, N, K = (int(v) for v in shape.split("x"))
        emit(gemm_case(eng, M, N, K, args.rounds))
        torch.cuda.empty_cache()

    for rows, cols, k, base, fts, bases in cases(args.shapes, args.ks, DT[args.dtype], dev) if args.shapes else ():
        iso = lambda: eng.iso_merge(fts, bases, alphas[:k], base, tol=args.tol, max_iter=args.max_iter)
        iso()                                                       # warm-up: the workspace, the code objects
        times = [wall_ms(iso) for _ in range(args.rounds)]
        eng.ctx.profile(True)
        eng.ctx.profile_reset()
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, rep = iso()
            torch.cuda.synchronize()
            profiled_ms = (time.perf_counter() - t0) * 1e3
            table = eng.ctx.profile_table()
        finally:
            eng.ctx.profile(False)
        kernels = {name: [int(table[name][0]), round(float(table[name][1]), 4)] for name in table}
        kernel_ms = sum(v[1] for v in kernels.values())
        q, c = rep.steps.count("q"), rep.steps.count("c")
        s, L = rep.s, rep.L
        tiles = (s + 127) // 128
        sym_flop = 2.0 * (tiles * (tiles + 1) // 2) * 128 * 128
        rec = {"iso_bench": f"{rows}x{cols}", "dtype": args.dtype, "k": k, "tol": args.tol, "max_iter": args.max_iter, "steps": rep.steps,
               "iterations": rep.iterations, "gemms": 3 * q + 2 * c + 1, "converged": rep.converged, "last_e": rep.e[-1],
               "sigma_bar": rep.sigma_bar, "workspace_bytes": int(eng.lib.dll.smhip_iso_workspace(rows, cols)), "rounds": args.rounds}
        spread(rec, "iso", times)
        rec["profiled_call_ms"] = round(profiled_ms, 3)
        rec["kernels_ms"] = kernels
        rec["kernels_sum_ms"] = round(kernel_ms, 3)
        rec["host_other_ms"] = round(profiled_ms - kernel_ms, 3)
        nt_flop = (len(rep.steps) + 1) * sym_flop * L + q * sym_flop * s
        rec["iso_gemm_nt_TF"] = round(nt_flop / kernels["iso_gemm_nt"][1] / 1e9, 2)
        if "iso_gemm_nn" in kernels:
            rec["iso_gemm_nn_TF"] = round((q + c) * 2.0 * s * s * L / kernels["iso_gemm_nn"][1] / 1e9, 2)
        emit(rec)

    if args.svd_shape:
        rows, cols = (int(v) for v in args.svd_shape.split("x"))
        for _, _, k, base, fts, bases in cases(args.svd_shape, args.ks.split(",")[0], DT[args.dtype], dev):
            a32 = [torch.tensor(a, device=dev, dtype=torch.float32) for a in alphas[:k]]

            def by_svd():
                T = torch.zeros(rows, cols, dtype=torch.float32, device=dev)
                for f, b, a in zip(fts, bases, a32):
                    T += (f.float() - b.float()) * a
                U, S, Vh = torch.linalg.svd(T, full_matrices=False)
                return (base.float() + S.mean() * (U @ Vh)).to(base.dtype)

            iso = lambda: eng.iso_merge(fts, bases, alphas[:k], base, tol=args.tol, max_iter=args.max_iter)
            iso(), by_svd()
            times = {"iso": [], "torch_svd": []}
            for _ in range(args.rounds):
                times["iso"].append(wall_ms(iso))
                times["torch_svd"].append(wall_ms(by_svd))
            out, rep, delta = eng.iso_merge(fts, bases, alphas[:k], base, tol=args.tol, max_iter=args.max_iter, want_delta=True)
            ref = by_svd().float() - base.float()
            rec = {"iso_vs_svd": args.svd_shape, "dtype": args.dtype, "k": k, "steps": rep.steps, "rounds": args.rounds,
                   "out_delta_rel_diff": float(torch.linalg.norm((out.float() - base.float()) - ref) / torch.linalg.norm(ref))}
            for name, t in times.items():
                spread(rec, name, t)
            rec["svd_ratio_to_iso"] = round(rec["torch_svd_ms"] / rec["iso_ms"], 2)
            emit(rec)
    append_lines(lines, args.out)


if __name__ == "__main__":
    main()
