#!/usr/bin/env python3
"""Engine.ties_merge against what it is measured against, in one process: per shape x K, the device time of the TIES
merge of K finetunes on one shared base that is also the output base (HIP events, after warm-up, repeated to fill at
least --seconds), its effective GB/s on the algorithmic byte count - selection reads K + 1 tensors, the merge reads
K + 1 and writes one: (2K + 3) * element size bytes per element - and
  * a clone() of as many bytes (half read, half written): the plain-streaming rate of the box, and
  * a torch restatement of the operator on the device (kthvalue per finetune plus element-wise ops): a TIMING baseline
    only; correctness is tests/ties_oracle.py's on the CPU.  The operator must be faster than it.
One JSON line per case; --out appends them to a file.

    python tools/ties_bench.py [--shapes 8192x8192,28672x8192,8192x28672] [--ks 2,3] [--density 0.2] [--dtype bf16]
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from delta_bench_common import ALPHAS as alphas, DT, HBM_PEAK_GBPS, append_lines, cases


def timed(fn, seconds: float, warmup: int = 5, min_reps: int = 10) -> float:
    """mean ms per call over enough calls to fill `seconds`"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    reps = max(min_reps, int(seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def torch_ties(fts, base, alphas, density, lam, normalize):
    """the operator with torch's own device kernels (the selection sorts); returns (out, how the threshold was found)"""
    n = base.numel()
    k = n if density == 1 else int(density * n)
    b = base.float().view(-1)
    how = "kthvalue"
    tvs = []
    for ft, alpha in zip(fts, alphas):
        d = ft.float().view(-1) - b
        mag = d.abs()
        try:
            tau = torch.kthvalue(mag, n - k + 1).values
        except RuntimeError:
            how = "sort"
            tau = torch.sort(mag, descending=True).values[k - 1]
        tvs.append(torch.where((mag >= tau) & (d != 0), d * alpha, torch.zeros((), device=d.device)))
        del d, mag
    S = torch.zeros_like(b)
    for tv in tvs:
        S = S + tv
    pos = S >= 0
    M, D = torch.zeros_like(b), torch.zeros_like(b)
    for tv, alpha in zip(tvs, alphas):
        m = torch.where(pos, tv > 0, tv < 0)
        M = M + torch.where(m, tv, torch.zeros((), device=b.device))
        D = D + m.float() * alpha
    if normalize:
        M = M / torch.where(D.abs() < 1e-8, torch.ones_like(D), D)
    return (b + lam * M).to(base.dtype).view(base.shape), how


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192x8192,28672x8192,8192x28672")
    ap.add_argument("--ks", default="2,3")
    ap.add_argument("--density", type=float, default=0.2)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    lines = []
    for rows, cols, k, base, fts, bases in cases(args.shapes, args.ks, DT[args.dtype], dev):
        nbytes = (2 * k + 3) * base.numel() * base.element_size()
        ms = timed(lambda: eng.ties_merge(fts, bases, alphas[:k], base, density=args.density), args.seconds)
        eng.ctx.profile(True)
        eng.ctx.profile_reset()
        _, rep = eng.ties_merge(fts, bases, alphas[:k], base, density=args.density)
        table = eng.ctx.profile_table()
        eng.ctx.profile(False)
        blob = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        clone_ms = timed(lambda: blob.clone(), args.seconds)
        del blob
        how = torch_ties(fts, base, alphas[:k], args.density, 1.0, True)[1]
        torch_ms = timed(lambda: torch_ties(fts, base, alphas[:k], args.density, 1.0, True), args.seconds, warmup=1, min_reps=3)
        rec = {"ties_bench": f"{rows}x{cols}", "dtype": args.dtype, "k": k, "density": args.density,
               "ms": round(ms, 4), "GBps": round(nbytes / ms / 1e6, 1), "share_of_8TBps": round(nbytes / ms / 1e6 / HBM_PEAK_GBPS, 3),
               "kernel_ms": {n: round(v[1], 4) for n, v in sorted(table.items())},
               "kept_over_asked": [round(c / max(rep.k_keep, 1), 4) for c in rep.kept],
               "clone_ms": round(clone_ms, 4), "clone_GBps": round(nbytes / clone_ms / 1e6, 1),
               "ratio_to_clone": round(ms / clone_ms, 3),
               "torch_ms": round(torch_ms, 3), "torch_select": how, "speedup_over_torch": round(torch_ms / ms, 2),
               "faster_than_torch": bool(ms < torch_ms)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    append_lines(lines, args.out)
    if not all(rec["faster_than_torch"] for rec in lines):
        sys.exit("ties_merge lost to the torch restatement in at least one case")


if __name__ == "__main__":
    main()
