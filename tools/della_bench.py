#!/usr/bin/env python3
"""Engine.della_merge next to what it is reported against, in one process and on the same inputs: per case (shape : K) the
device time of whole calls of `della` and `della_linear` on K finetunes with one shared base that is also the output
base, next to
  * Engine.dare_merge in both modes at the same density (the same fused pass with ONE threshold and no rank pass),
  * a clone() of as many bytes as DELLA's algorithmic traffic - the rank pass reads K + 1 tensors and writes K 16-bit
    thresholds per element, the merge reads K + 1 tensors and the K thresholds and writes one tensor - half read, half
    written: the plain-streaming rate of the box, and
  * a torch restatement on the device (argsort twice for the ranks, a pre-drawn uniform tensor instead of a generator
    call, masked fp32 operations; its ties are argsort's, so it is a timing contender, not an oracle).
The split of one call between `della_rank` and `della_merge` comes from the profile table.  Timing: HIP events around
`reps` back-to-back calls after a warm-up, `--rounds` such windows per contender, the contenders ALTERNATING inside every
round; medians, with the max - min spread of the rounds in ms.  Nothing is gated: the numbers are reported.  One JSON
line per case; --out appends them to a file.

    python tools/della_bench.py [--cases 8192x8192:2,8192x8192:3,28672x8192:2,8192x28672:2] [--density 0.5] [--epsilon 0.15]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from delta_bench_common import ALPHAS as alphas, DT, HBM_PEAK_GBPS, alternate, append_lines, cases


def torch_della(fts, base, weights, draws, density, epsilon, sign_election):
    """DELLA with torch operators only; draws: one uniform [0, 1) tensor per finetune, made outside the timed region"""
    c = base.shape[-1]
    b = base.float()
    ramp = torch.arange(c, device=base.device).expand(base.shape)
    tvs = []
    for f, a, h in zip(fts, weights, draws):
        d = f.float() - b
        rank = torch.empty_like(ramp).scatter_(-1, d.abs().argsort(dim=-1), ramp)
        p = (density - epsilon) + (2.0 * epsilon / max(c - 1, 1)) * rank.float()
        tvs.append(torch.where((h < p) & (d != 0), d / p * a, 0.0))
    s = sum(tvs)
    if sign_election:
        pos = s >= 0
        agree = [torch.where(pos, tv > 0, tv < 0) for tv in tvs]
        m = sum(torch.where(g, tv, 0.0) for g, tv in zip(agree, tvs))
        den = sum(torch.where(g, a, 0.0) for g, a in zip(agree, weights))
        m = m / torch.where(den.abs() < 1e-8, 1.0, den)
    else:
        m = s / sum(weights)
    return (b + m).to(base.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="8192x8192:2,8192x8192:3,28672x8192:2,8192x28672:2", help="rows x cols : K, comma separated")
    ap.add_argument("--density", type=float, default=0.5)
    ap.add_argument("--epsilon", type=float, default=0.15)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per contender and case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="leave the torch restatement out")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("della_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    key = 0x0123456789ABCDEF
    lines = []
    for case in args.cases.split(","):
        shape, ks = case.split(":")
        for rows, cols, k, base, fts, bases in cases(shape, ks, DT[args.dtype], dev):
            es = base.element_size()
            nbytes = base.numel() * ((k + 1) * es + 2 * k + (k + 1) * es + 2 * k + es)
            blob = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            della = lambda se: (lambda: eng.della_merge(fts, bases, alphas[:k], base, density=args.density, epsilon=args.epsilon,
                                                        sign_election=se, key=key))
            dare = lambda se: (lambda: eng.dare_merge(fts, bases, alphas[:k], base, density=args.density, sign_election=se, key=key))
            contenders = {"della": della(True), "della_linear": della(False), "dare_ties": dare(True), "dare_linear": dare(False),
                          "clone": lambda: blob.clone()}
            if not args.no_torch:
                g = torch.Generator(device=dev).manual_seed(1)
                draws = [torch.rand(base.shape, generator=g, device=dev) for _ in range(k)]
                contenders["torch_della"] = lambda: torch_della(fts, base, alphas[:k], draws, args.density, args.epsilon, True)
            times = alternate(contenders, args.seconds, args.rounds)
            eng.ctx.profile(True)
            eng.ctx.profile_reset()
            _, rep = eng.della_merge(fts, bases, alphas[:k], base, density=args.density, epsilon=args.epsilon, key=key)
            table = eng.ctx.profile_table()
            eng.ctx.profile(False)
            kernel_ms = {n: round(v[1], 4) for n, v in sorted(table.items())}
            rec = {"della_bench": f"{rows}x{cols}", "dtype": args.dtype, "k": k, "density": args.density, "epsilon": args.epsilon,
                   "thresholds": [rep.threshold_lo, rep.threshold_hi], "kept_share": [round(c / base.numel(), 6) for c in rep.kept],
                   "bytes": nbytes, "rounds": args.rounds, "kernel_ms": kernel_ms,
                   "rank_share_of_kernels": round(kernel_ms.get("della_rank", 0.0) / max(sum(kernel_ms.values()), 1e-9), 4)}
            med = {name: statistics.median(t) for name, t in times.items()}
            for name, t in times.items():
                rec[f"{name}_ms"] = round(med[name], 4)
                rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
            for mode, other in (("della", "dare_ties"), ("della_linear", "dare_linear")):
                rec[f"{mode}_GBps"] = round(nbytes / med[mode] / 1e6, 1)
                rec[f"{mode}_share_of_8TBps"] = round(nbytes / med[mode] / 1e6 / HBM_PEAK_GBPS, 3)
                rec[f"{mode}_ratio_to_clone"] = round(med[mode] / med["clone"], 3)
                rec[f"{mode}_ratio_to_{other}"] = round(med[mode] / med[other], 3)
            if "torch_della" in med:
                rec["torch_della_over_della"] = round(med["torch_della"] / med["della"], 2)
                del draws
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del blob
    append_lines(lines, args.out)


if __name__ == "__main__":
    main()
