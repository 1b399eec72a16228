#!/usr/bin/env python3
"""Engine.geo_merge against what it is measured against, in one process and on the same inputs: per shape x K, the device
time of `model_stock` (per tensor and per row), and at K = 2 of `nuslerp` and `slerp`, on K finetunes with one shared base
that is also the output base, next to
  * a clone() of as many bytes as the operator moves - (2K + 3) * element size bytes per element in delta space (the Gram
    pass reads K + 1 tensors, the combine pass reads K + 1 and writes one), (2K + 1) for slerp, which reads no base - half
    read, half written: the plain-streaming rate of the box, and
  * Engine.dare_merge (dare_linear) on the same inputs against a clone() of ITS bytes, (K + 2) per element: the one-pass
    operator of the same family.
The figure of a case is each operator's time over its clone; dare_linear's ratio from the same run is the yardstick (the
geometric kernels carry no generator, so their ratio is expected to be no worse - the record says whether it is).
Timing: HIP events around `reps` back-to-back calls after a warm-up, `--rounds` such windows per contender, the
contenders ALTERNATING inside every round; medians, with the max - min spread of the rounds in ms.  One JSON line per
case, appended to --out.

    python tools/geo_bench.py [--cases 8192x8192:2,8192x8192:3,28672x8192:2,8192x28672:2] [--dtype bf16]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from delta_bench_common import ALPHAS as alphas, DT, HBM_PEAK_GBPS, alternate, append_lines, cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="8192x8192:2,8192x8192:3,28672x8192:2,8192x28672:2", help="shape:K, comma separated")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per contender and case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "geo_bench.txt"),
                    help="append the JSON lines to this file ('' for none)")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("geo_bench: medians of at least five alternating rounds")
    if not torch.cuda.is_available():
        sys.exit("geo_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    lines = []
    for case in args.cases.split(","):
        shape, ks = case.split(":")
        for rows, cols, k, base, fts, bases in cases(shape, ks, DT[args.dtype], dev):
            per = base.numel() * base.element_size()
            blobs = {name: torch.empty(passes * per // 2, dtype=torch.uint8, device=dev)
                     for name, passes in (("delta", 2 * k + 3), ("weight", 2 * k + 1), ("dare", k + 2))}
            geo = lambda mode, rowwise=False: (lambda: eng.geo_merge(fts, bases, alphas[:k], base, mode=mode, rowwise=rowwise))
            contenders = {"model_stock": geo("model_stock"), "model_stock_rowwise": geo("model_stock", True)}
            if k == 2:
                contenders.update({"nuslerp": geo("nuslerp"), "slerp": geo("slerp")})
            contenders.update({"dare_linear": lambda: eng.dare_merge(fts, bases, alphas[:k], base, density=0.5, sign_election=False),
                               "clone_delta": lambda: blobs["delta"].clone(), "clone_dare": lambda: blobs["dare"].clone()})
            if k == 2:
                contenders["clone_weight"] = lambda: blobs["weight"].clone()
            times = alternate(contenders, args.seconds, args.rounds)
            rec = {"geo_bench": f"{rows}x{cols}", "dtype": args.dtype, "k": k, "rounds": args.rounds,
                   "bytes": {name: int(b.numel() * 2) for name, b in blobs.items()}}
            med = {name: statistics.median(t) for name, t in times.items()}
            for name, t in times.items():
                rec[f"{name}_ms"] = round(med[name], 4)
                rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
            clone_of = {"model_stock": "delta", "model_stock_rowwise": "delta", "nuslerp": "delta", "slerp": "weight", "dare_linear": "dare"}
            for name, which in clone_of.items():
                if name in med:
                    rec[f"{name}_ratio_to_clone"] = round(med[name] / med[f"clone_{which}"], 3)
                    rec[f"{name}_GBps"] = round(blobs[which].numel() * 2 / med[name] / 1e6, 1)
                    rec[f"{name}_share_of_8TBps"] = round(blobs[which].numel() * 2 / med[name] / 1e6 / HBM_PEAK_GBPS, 3)
            rec["no_worse_than_dare_linear"] = {name: bool(rec[f"{name}_ratio_to_clone"] <= rec["dare_linear_ratio_to_clone"])
                                                for name in clone_of if name != "dare_linear" and name in med}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del blobs
    append_lines(lines, args.out or None)


if __name__ == "__main__":
    main()
