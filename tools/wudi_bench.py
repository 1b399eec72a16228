#!/usr/bin/env python3
"""Engine.wudi_merge and its three GEMM kernels, measured in one process and on the same inputs.

  1. Per shape x K, --rounds alternating rounds of (a) one profiled `wudi` call of --kernel-iters steps and (b) profiled
     `iso_gemm_nt` launches of the same M, N, K on fp32 operands: the symmetric mode at C x C x R (what `wudi_gram` computes)
     and the plain form at R x C x C (`wudi_rhs`, `wudi_step`).  The profile hook puts HIP events around every launch; a
     kernel's time is its total over the call divided by its launches.  FLOP rates against the 155 TF the fp32 MFMA has
     measured, and each kernel's ratio to `iso_gemm_nt` in the same round: what the 16-bit operand staging of
     `wudi_gram` / `wudi_rhs` gains or costs over an fp32 operand, and what the seven-plane epilogue costs `wudi_step`.
     Medians of the rounds with the max - min spread.
  2. Whole calls at --iters (300) steps: wall time between two device synchronisations, alternating with the same
     function written with torch matmuls and `torch.optim.Adam` on the device, at --whole-shapes.
No threshold is asserted: one JSON line per case; --out appends them.  What a run leaves out is listed as not measured.

    python tools/wudi_bench.py [--shapes 8192x8192,8192x28672,28672x8192] [--ks 2,3] [--whole-shapes 8192x8192] [--iters 300]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from delta_bench_common import DT, append_lines, cases

FP32_MFMA_TF = 155.0


def wall_ms(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def profiled(eng, fn):
    """{kernel: ms per launch} of one call"""
    eng.ctx.profile(True)
    eng.ctx.profile_reset()
    try:
        fn()
        torch.cuda.synchronize()
        table = eng.ctx.profile_table()
    finally:
        eng.ctx.profile(False)
    return {name: float(table[name][1]) / int(table[name][0]) for name in table}


def med(rec, name, values, digits=3):
    rec[name] = round(statistics.median(values), digits)
    rec[f"{name}_spread"] = round(max(values) - min(values), digits)


def torch_wudi(fts, bases, alphas, base, iters, lr, lam):
    ds = [f.float() - b.float() for f, b in zip(fts, bases)]
    S = P = None
    for d, a in zip(ds, alphas):
        sh = (d.T @ d) * (a / float((d.double() ** 2).sum()))
        S = sh if S is None else S + sh
        P = d @ sh if P is None else P + d @ sh
    X = torch.nn.Parameter(sum(d * a for d, a in zip(ds, alphas)), requires_grad=False)
    del ds
    opt = torch.optim.Adam([X], lr=lr)
    for _ in range(iters):
        X.grad = 2.0 * (X @ S - P)
        opt.step()
    return (base.float() + lam * X).to(base.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192x8192,8192x28672,28672x8192")
    ap.add_argument("--whole-shapes", default="8192x8192")
    ap.add_argument("--ks", default="2,3")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--kernel-iters", type=int, default=4)
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("wudi_bench: the comparison wants at least five alternating rounds")
    if not torch.cuda.is_available():
        sys.exit("wudi_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for rows, cols, k, base, fts, bases in cases(args.shapes, args.ks, DT[args.dtype], dev) if args.shapes else ():
        alphas = [1.0] * k
        wudi = lambda: eng.wudi_merge(fts, bases, alphas, base, iters=args.kernel_iters, lr=args.lr)
        g = torch.Generator(device=dev).manual_seed(rows + cols)
        x = torch.randn(rows, cols, generator=g, device=dev)
        s = torch.randn(cols, cols, generator=g, device=dev)
        dt = torch.randn(cols, rows, generator=g, device=dev)
        wudi()                                                      # warm-up: the workspace, the code objects
        tiles = (cols + 127) // 128
        flop = {"wudi_gram": 2.0 * (tiles * (tiles + 1) // 2) * 128 * 128 * rows, "wudi_rhs": 2.0 * rows * cols * cols,
                "wudi_step": 2.0 * rows * cols * cols}
        tf = {name: [] for name in list(flop) + ["iso_gemm_nt_sym", "iso_gemm_nt"]}
        for _ in range(args.rounds):
            table = profiled(eng, wudi)
            for name in flop:
                tf[name].append(flop[name] / table[name] / 1e9)
            tf["iso_gemm_nt_sym"].append(flop["wudi_gram"] / profiled(eng, lambda: eng.iso_gemm(dt, dt, form=0, sym=True))["iso_gemm_nt"] / 1e9)
            tf["iso_gemm_nt"].append(flop["wudi_step"] / profiled(eng, lambda: eng.iso_gemm(x, s, form=0))["iso_gemm_nt"] / 1e9)
        rec = {"wudi_kernels": f"{rows}x{cols}", "dtype": args.dtype, "k": k, "rounds": args.rounds, "ceiling_TF": FP32_MFMA_TF,
               "workspace_bytes": int(eng.lib.dll.smhip_wudi_workspace(rows, cols))}
        for name, v in tf.items():
            med(rec, f"{name}_TF", v, 2)
            rec[f"{name}_share_of_155TF"] = round(rec[f"{name}_TF"] / FP32_MFMA_TF, 3)
        for name, ref in (("wudi_gram", "iso_gemm_nt_sym"), ("wudi_rhs", "iso_gemm_nt"), ("wudi_step", "iso_gemm_nt")):
            med(rec, f"{name}_over_{ref}", [a / b for a, b in zip(tf[name], tf[ref])])
        emit(rec)
        del x, s, dt
        if f"{rows}x{cols}" in args.whole_shapes.split(","):
            whole = lambda: eng.wudi_merge(fts, bases, alphas, base, iters=args.iters, lr=args.lr)
            by_torch = lambda: torch_wudi(fts, bases, alphas, base, args.iters, args.lr, 1.0)
            times = {"wudi": [], "torch": []}
            for _ in range(args.rounds):
                times["wudi"].append(wall_ms(whole))
                times["torch"].append(wall_ms(by_torch))
            out, rep, delta = eng.wudi_merge(fts, bases, alphas, base, iters=args.iters, lr=args.lr, want_delta=True)
            ref = by_torch().float() - base.float()
            rec = {"wudi_whole": f"{rows}x{cols}", "dtype": args.dtype, "k": k, "iters": args.iters, "rounds": args.rounds,
                   "grad_sq_first": rep.grad_sq_first, "grad_sq_last": rep.grad_sq_last,
                   "out_delta_rel_diff": float(torch.linalg.norm((out.float() - base.float()) - ref) / torch.linalg.norm(ref))}
            med(rec, "wudi_ms", times["wudi"])
            med(rec, "torch_ms", times["torch"])
            rec["torch_ratio_to_wudi"] = round(rec["torch_ms"] / rec["wudi_ms"], 2)
            emit(rec)
            del ref, out, delta
        else:
            emit({"wudi_whole": f"{rows}x{cols}", "k": k, "not_measured": "not in --whole-shapes"})
    append_lines(lines, args.out)


if __name__ == "__main__":
    main()
