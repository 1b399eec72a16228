#!/usr/bin/env python3
"""Engine.consensus_merge against what it is measured against, in one process and on the same inputs: per shape x K, the
device time of whole calls of `consensus_ta` and `consensus_ties` on K finetunes with one shared base that is also the
output base, next to
  * Engine.dare_merge (dare_linear) at density 1 - the yardstick of consensus_ta: the same K + 2 tensor passes in one
    fused kernel, a Philox block per octet and finetune where Consensus has its masks,
  * Engine.ties_merge at the same density - the yardstick of consensus_ties: the same three selection levels, 4K + 5 tensor
    passes, and
  * a clone() of as many bytes as consensus_ta's algorithmic traffic, (K + 2) * element size bytes per element (half read,
    half written): the plain-streaming rate of the box.
Timing: HIP events around `reps` back-to-back calls after a warm-up, `--rounds` such windows per contender, the
contenders ALTERNATING inside every round; medians, with the max - min spread of the rounds in ms.  No threshold is
asserted: the ratios and the spreads are printed, one JSON line per case; --out appends them to a file.

    python tools/consensus_bench.py [--shapes 8192x8192,28672x8192] [--ks 2,3] [--density 0.2] [--dtype bf16]
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
    ap.add_argument("--density", type=float, default=0.2, help="of consensus_ties and ties")
    ap.add_argument("--mask-lambda", type=float, default=0.4)
    ap.add_argument("--consensus-k", type=int, default=2)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per contender and case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("consensus_bench: the comparison wants at least five alternating rounds")
    if not torch.cuda.is_available():
        sys.exit("consensus_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    lines = []
    for rows, cols, k, base, fts, bases in cases(args.shapes, args.ks, DT[args.dtype], dev):
        nbytes = (k + 2) * base.numel() * base.element_size()
        blob = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        cons = lambda ties: (lambda: eng.consensus_merge(fts, bases, alphas[:k], base, ties=ties, density=args.density,
                                                         mask_lambda=args.mask_lambda, consensus_k=args.consensus_k))
        contenders = {"consensus_ta": cons(False),
                      "dare_linear": lambda: eng.dare_merge(fts, bases, alphas[:k], base, density=1.0, sign_election=False),
                      "consensus_ties": cons(True),
                      "ties": lambda: eng.ties_merge(fts, bases, alphas[:k], base, density=args.density),
                      "clone": lambda: blob.clone()}
        times = alternate(contenders, args.seconds, args.rounds)
        _, rep = eng.consensus_merge(fts, bases, alphas[:k], base, ties=False, mask_lambda=args.mask_lambda, consensus_k=args.consensus_k)
        rec = {"consensus_bench": f"{rows}x{cols}", "dtype": args.dtype, "k": k, "density": args.density,
               "mask_lambda": args.mask_lambda, "consensus_k": args.consensus_k,
               "selected_share_ta": round(rep.selected / base.numel(), 6), "bytes": nbytes, "rounds": args.rounds}
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            rec[f"{name}_ms"] = round(med[name], 4)
            rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
            rec[f"{name}_rounds_ms"] = [round(v, 4) for v in t]
        rec["consensus_ta_GBps"] = round(nbytes / med["consensus_ta"] / 1e6, 1)
        rec["consensus_ta_share_of_8TBps"] = round(nbytes / med["consensus_ta"] / 1e6 / HBM_PEAK_GBPS, 3)
        rec["consensus_ta_ratio_to_clone"] = round(med["consensus_ta"] / med["clone"], 3)
        rec["consensus_ta_ratio_to_dare_linear"] = round(med["consensus_ta"] / med["dare_linear"], 4)
        rec["consensus_ties_ratio_to_ties"] = round(med["consensus_ties"] / med["ties"], 4)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del blob
    append_lines(lines, args.out)


if __name__ == "__main__":
    main()
