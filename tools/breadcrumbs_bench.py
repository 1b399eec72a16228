#!/usr/bin/env python3
"""Engine.breadcrumbs_merge against what it is measured against, in one process and on the same inputs: per shape x K,
the device time of `breadcrumbs_ties` and `breadcrumbs` on K finetunes with one shared base that is also the output
base, next to
  * Engine.ties_merge at the same density on the same inputs - THE yardstick: both move 4K + 5 tensor passes, Breadcrumbs
    adds on-chip work only (a second compare per element at levels 2-3, one more compare in the merge pass), and
  * a clone() of as many bytes as the algorithmic traffic, (2K + 3) * element size bytes per element (half read, half
    written): the plain-streaming rate of the box.
Timing: HIP events around `reps` back-to-back calls after a warm-up, `--rounds` such windows per contender, the
contenders ALTERNATING inside every round; medians, with the max - min spread of the rounds in ms.  Acceptance per case:
median(breadcrumbs_ties) <= median(ties) + 2 * (max - min of ties's rounds).  One JSON line per case; --out appends them
to a file; the exit status is non-zero when a case misses the acceptance.

    python tools/breadcrumbs_bench.py [--shapes 8192x8192,28672x8192] [--ks 2,3] [--density 0.9] [--gamma 0.01] [--dtype bf16]
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
    ap.add_argument("--shapes", default="8192x8192,28672x8192")
    ap.add_argument("--ks", default="2,3")
    ap.add_argument("--density", type=float, default=0.9)
    ap.add_argument("--gamma", type=float, default=0.01)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per contender and case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("breadcrumbs_bench: the acceptance wants at least five alternating rounds")
    if not torch.cuda.is_available():
        sys.exit("breadcrumbs_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    lines = []
    for rows, cols, k, base, fts, bases in cases(args.shapes, args.ks, DT[args.dtype], dev):
        nbytes = (2 * k + 3) * base.numel() * base.element_size()
        blob = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        crumbs = lambda se: (lambda: eng.breadcrumbs_merge(fts, bases, alphas[:k], base, density=args.density, gamma=args.gamma,
                                                           sign_election=se))
        contenders = {"breadcrumbs_ties": crumbs(True), "breadcrumbs": crumbs(False),
                      "ties": lambda: eng.ties_merge(fts, bases, alphas[:k], base, density=args.density),
                      "clone": lambda: blob.clone()}
        times = alternate(contenders, args.seconds, args.rounds)
        _, rep = eng.breadcrumbs_merge(fts, bases, alphas[:k], base, density=args.density, gamma=args.gamma, sign_election=True)
        rec = {"breadcrumbs_bench": f"{rows}x{cols}", "dtype": args.dtype, "k": k, "density": args.density, "gamma": args.gamma,
               "kept_share": [round(c / base.numel(), 6) for c in rep.kept],
               "dropped_top_share": [round(c / base.numel(), 6) for c in rep.dropped_top],
               "bytes": nbytes, "rounds": args.rounds}
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            rec[f"{name}_ms"] = round(med[name], 4)
            rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
            rec[f"{name}_rounds_ms"] = [round(v, 4) for v in t]
        for mode in ("breadcrumbs_ties", "breadcrumbs"):
            rec[f"{mode}_GBps"] = round(nbytes / med[mode] / 1e6, 1)
            rec[f"{mode}_share_of_8TBps"] = round(nbytes / med[mode] / 1e6 / HBM_PEAK_GBPS, 3)
            rec[f"{mode}_ratio_to_clone"] = round(med[mode] / med["clone"], 3)
            rec[f"{mode}_ratio_to_ties"] = round(med[mode] / med["ties"], 4)
        bound = med["ties"] + 2.0 * (max(times["ties"]) - min(times["ties"]))
        rec["acceptance_bound_ms"] = round(bound, 4)
        rec["within_ties_noise"] = bool(med["breadcrumbs_ties"] <= bound)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del blob
    append_lines(lines, args.out)
    if not all(rec["within_ties_noise"] for rec in lines):
        sys.exit("breadcrumbs_ties took longer than ties plus twice the spread of ties in at least one case")


if __name__ == "__main__":
    main()
