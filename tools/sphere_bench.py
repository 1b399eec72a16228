#!/usr/bin/env python3
"""Engine.sphere_merge against what it is measured against, in one process and on the same inputs: per shape x K, the
device time of `karcher` and `multislerp`, per tensor and per row, on K finetunes with one shared base that is also the
output base, next to
  * Engine.geo_merge(model_stock), per tensor and per row: the SAME two streaming kernels (geo_gram, geo_combine) with
    another scalar step between them - the expectation is that the whole-tensor times sit within the rounds' spread of it;
  * a clone() of as many bytes as the operator moves - (2K + 3) * element size bytes per element in delta space (the Gram
    pass reads K + 1 tensors, the combine pass reads K + 1 and writes one), (2K + 1) in weight space, which reads no
    base - half read, half written: the plain-streaming rate of the box; and
  * the same mean iterated IN TENSOR SPACE with torch kernels on the same inputs (fp32 vectors; the log map, the step and
    the renormalisation each stream the K tensors), for as many iterations as the engine's whole-tensor call took: what
    the Gram-space iteration saves.
Timing: HIP events around `reps` back-to-back calls after a warm-up, `--rounds` such windows per contender, the
contenders ALTERNATING inside every round; medians, with the max - min spread of the rounds in ms.  One JSON line per
case, appended to --out.

    python tools/sphere_bench.py [--cases 8192x8192:2,8192x8192:3,28672x8192:2,28672x8192:3] [--dtype bf16]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from delta_bench_common import ALPHAS as alphas, DT, HBM_PEAK_GBPS, alternate, append_lines, cases


def tensor_space(xs, weights, iterations, rowwise):
    """the Karcher mean of the fp32 vectors xs on the device, `iterations` log-map steps, no host synchronisation"""
    dims = tuple(range(1, xs[0].ndim)) if rowwise else None
    dot = lambda a, b: (a * b).sum(dim=dims, keepdim=True) if rowwise else (a * b).sum()
    norms = [dot(x, x).sqrt() for x in xs]
    us = [x / n for x, n in zip(xs, norms)]
    m = sum(w * u for w, u in zip(weights, us))
    m = m / dot(m, m).sqrt()
    for _ in range(iterations):
        t = torch.zeros_like(m)
        for w, u in zip(weights, us):
            d = dot(m, u).clamp(-1.0, 1.0)
            theta = torch.acos(d)
            f = torch.where(theta < 1e-8, torch.ones_like(theta), theta / torch.sin(theta))
            t = t + (w * f) * (u - d * m)
        tau = dot(t, t).sqrt().clamp_min(1e-30)
        m = torch.cos(tau) * m + (torch.sin(tau) / tau) * t
        m = m / dot(m, m).sqrt()
    return sum(w * n for w, n in zip(weights, norms)) * m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="8192x8192:2,8192x8192:3,28672x8192:2,28672x8192:3", help="shape:K, comma separated")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per contender and case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "sphere_bench.txt"),
                    help="append the JSON lines to this file ('' for none)")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("sphere_bench: medians of at least five alternating rounds")
    if not torch.cuda.is_available():
        sys.exit("sphere_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    lines = []
    for case in args.cases.split(","):
        shape, ks = case.split(":")
        for rows, cols, k, base, fts, bases in cases(shape, ks, DT[args.dtype], dev):
            per = base.numel() * base.element_size()
            blobs = {name: torch.empty(passes * per // 2, dtype=torch.uint8, device=dev)
                     for name, passes in (("delta", 2 * k + 3), ("weight", 2 * k + 1))}
            sphere = lambda mode, rowwise=False: (lambda: eng.sphere_merge(fts, bases, alphas[:k], base, mode=mode, rowwise=rowwise))
            stock = lambda rowwise=False: (lambda: eng.geo_merge(fts, bases, alphas[:k], base, mode="model_stock", rowwise=rowwise))
            _, rep = eng.sphere_merge(fts, bases, alphas[:k], base, mode="karcher")
            _, rep_rows = eng.sphere_merge(fts, bases, alphas[:k], base, mode="karcher", rowwise=True)
            xs = [f.float() for f in fts]
            weights = [a / sum(alphas[:k]) for a in alphas[:k]]
            contenders = {"karcher": sphere("karcher"), "karcher_rowwise": sphere("karcher", True),
                          "multislerp": sphere("multislerp"), "multislerp_rowwise": sphere("multislerp", True),
                          "model_stock": stock(), "model_stock_rowwise": stock(True),
                          "torch_tensor_space": lambda: tensor_space(xs, weights, rep.iterations, False),
                          "torch_tensor_space_rowwise": lambda: tensor_space(xs, weights, rep_rows.iters_max, True),
                          "clone_delta": lambda: blobs["delta"].clone(), "clone_weight": lambda: blobs["weight"].clone()}
            times = alternate(contenders, args.seconds, args.rounds)
            rec = {"sphere_bench": f"{rows}x{cols}", "dtype": args.dtype, "k": k, "rounds": args.rounds,
                   "iterations": rep.iterations, "converged": rep.converged, "rowwise_iters_max": rep_rows.iters_max,
                   "rowwise_rows_unconverged": rep_rows.rows_unconverged,
                   "bytes": {name: int(b.numel() * 2) for name, b in blobs.items()}}
            med = {name: statistics.median(t) for name, t in times.items()}
            for name, t in times.items():
                rec[f"{name}_ms"] = round(med[name], 4)
                rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
            clone_of = {"karcher": "weight", "karcher_rowwise": "weight", "multislerp": "delta", "multislerp_rowwise": "delta",
                        "model_stock": "delta", "model_stock_rowwise": "delta"}
            for name, which in clone_of.items():
                rec[f"{name}_ratio_to_clone"] = round(med[name] / med[f"clone_{which}"], 3)
                rec[f"{name}_share_of_8TBps"] = round(blobs[which].numel() * 2 / med[name] / 1e6 / HBM_PEAK_GBPS, 3)
            for name, other in (("multislerp", "model_stock"), ("multislerp_rowwise", "model_stock_rowwise")):
                rec[f"{name}_minus_{other}_ms"] = round(med[name] - med[other], 4)
                rec[f"{name}_within_spread_of_{other}"] = bool(abs(med[name] - med[other]) <= max(rec[f"{name}_spread_ms"], rec[f"{other}_spread_ms"]))
            rec["torch_tensor_space_over_karcher"] = round(med["torch_tensor_space"] / med["karcher"], 2)
            rec["torch_tensor_space_rowwise_over_karcher_rowwise"] = round(med["torch_tensor_space_rowwise"] / med["karcher_rowwise"], 2)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del blobs, xs
    append_lines(lines, args.out or None)


if __name__ == "__main__":
    main()
