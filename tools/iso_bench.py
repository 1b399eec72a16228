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
--gemm bf16x3 adds the split product on the bf16 MFMA (csrc/sm_iso3.hpp) to 1. and 2.: its forms alternate with the fp32
forms inside every round (keys ending in _bf16x3, with their ratio to the fp32 time), and whole calls alternate between
the two modes, a record each.
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


def gemm_case(eng, M, N, K, rounds, modes=("fp32",)):
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g, device=dev)
    bt = torch.randn(N, K, generator=g, device=dev)
    b = torch.randn(K, N, generator=g, device=dev)
    forms, flop = {}, {}
    tiles = (M + 127) // 128
    for mode in modes:
        tag = "" if mode == "fp32" else f"_{mode}"
        forms["nt" + tag] = lambda mode=mode: eng.iso_gemm(a, bt, form=0, gemm=mode)
        forms["nn" + tag] = lambda mode=mode: eng.iso_gemm(a, b, form=1, gemm=mode)
        flop["nt" + tag] = flop["nn" + tag] = 2.0 * M * N * K
        if M == N:
            forms["nt_sym" + tag] = lambda mode=mode: eng.iso_gemm(a, a, form=0, sym=True, gemm=mode)
            flop["nt_sym" + tag] = 2.0 * (tiles * (tiles + 1) // 2) * 128 * 128 * K
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
    for name in [n for n in times if n.endswith("_bf16x3")]:
        rec[f"{name}_time_over_fp32"] = round(rec[f"{name}_ms"] / rec[f"{name[:-7]}_ms"], 3)
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
    ap.add_argument("--gemm", default="fp32", choices=("fp32", "bf16x3"), help="bf16x3: also the split product, alternating with fp32")
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
    modes = ("fp32",) if args.gemm == "fp32" else ("fp32", args.gemm)

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for shape in [s for s in args.gemm_shapes.split(",") if s]:
        M, N, K = (int(v) for v in shape.split("x"))
        emit(gemm_case(eng, M, N, K, args.rounds, modes))
        torch.cuda.empty_cache()

    for rows, cols, k, base, fts, bases in cases(args.shapes, args.ks, DT[args.dtype], dev) if args.shapes else ():
        call = lambda mode: eng.iso_merge(fts, bases, alphas[:k], base, tol=args.tol, max_iter=args.max_iter, gemm=mode)
        for mode in modes:
            call(mode)                                              # warm-up: the workspace, the code objects
        alternating = {mode: [] for mode in modes}
        for _ in range(args.rounds):
            for mode in modes:
                alternating[mode].append(wall_ms(lambda: call(mode)))
        for mode in modes:
            iso, times = (lambda: call(mode)), alternating[mode]
            nt_name, nn_name = ("iso_gemm_nt", "iso_gemm_nn") if mode == "fp32" else ("iso_gemm3_nt", "iso_gemm3_nn")
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
            rec = {"iso_bench": f"{rows}x{cols}", "dtype": args.dtype, "k": k, "gemm": mode, "tol": args.tol, "max_iter": args.max_iter, "steps": rep.steps,
                   "iterations": rep.iterations, "gemms": 3 * q + 2 * c + 1, "converged": rep.converged, "last_e": rep.e[-1],
                   "sigma_bar": rep.sigma_bar, "workspace_bytes": int(eng.lib.dll.smhip_iso_workspace(rows, cols)), "rounds": args.rounds}
            spread(rec, "iso", times)
            rec["profiled_call_ms"] = round(profiled_ms, 3)
            rec["kernels_ms"] = kernels
            rec["kernels_sum_ms"] = round(kernel_ms, 3)
            rec["host_other_ms"] = round(profiled_ms - kernel_ms, 3)
            nt_flop = (len(rep.steps) + 1) * sym_flop * L + q * sym_flop * s
            rec[f"{nt_name}_TF"] = round(nt_flop / kernels[nt_name][1] / 1e9, 2)
            if nn_name in kernels:
                rec[f"{nn_name}_TF"] = round((q + c) * 2.0 * s * s * L / kernels[nn_name][1] / 1e9, 2)
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
