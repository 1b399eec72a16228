#!/usr/bin/env python3
"""The three EMR-Merging calls against what they are measured against, in one process and on the same inputs: per shape x
K, the device time of whole calls on K finetunes with one shared base that is also the output base -
  * Engine.emr_merge next to Engine.dare_merge (dare_linear) at density 1, the same K + 2 tensor passes in one fused
    kernel, and next to a clone() of as many bytes as its algorithmic traffic, (K + 2) * element size bytes per element
    (half read, half written): the plain-streaming rate of the box;
  * Engine.emr_mask (finetune 0 against the unified model) next to Engine.delta_pack at 1 bit with a scale per tensor:
    the same walk over whole rows, one more tensor read; both end in the row fold of geo_gram_fold;
  * Engine.emr_apply next to Engine.delta_apply of that 1-bit pack and next to a clone() of its algorithmic bytes,
    3 * element size + 1 / 8 bytes per element.
Timing: HIP events around `reps` back-to-back calls after a warm-up, `--rounds` such windows per contender, the
contenders ALTERNATING inside every round; medians, with the max - min spread of the rounds in ms.  No threshold is
asserted: the ratios and the spreads are printed, one JSON line per case; --out appends them to a file.

    python tools/emr_bench.py [--shapes 8192x8192,28672x8192] [--ks 2,3] [--dtype bf16]
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
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per contender and case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("emr_bench: the comparison wants at least five alternating rounds")
    if not torch.cuda.is_available():
        sys.exit("emr_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    lines = []
    for rows, cols, k, base, fts, bases in cases(args.shapes, args.ks, DT[args.dtype], dev):
        es, n = base.element_size(), base.numel()
        merge_bytes = (k + 2) * n * es
        apply_bytes = 3 * n * es + n // 8
        blob = torch.empty(merge_bytes // 2, dtype=torch.uint8, device=dev)
        blob_apply = torch.empty(apply_bytes // 2, dtype=torch.uint8, device=dev)
        uni, rep = eng.emr_merge(fts, bases, base)
        mask, scale, mrep = eng.emr_mask(fts[0], base, uni)
        sign, _, dscale, _ = eng.delta_pack(fts[0], base, bits=1, scale="tensor")
        contenders = {"emr": lambda: eng.emr_merge(fts, bases, base),
                      "dare_linear": lambda: eng.dare_merge(fts, bases, alphas[:k], base, density=1.0, sign_election=False),
                      "clone": lambda: blob.clone(),
                      "emr_mask": lambda: eng.emr_mask(fts[0], base, uni),
                      "delta_pack": lambda: eng.delta_pack(fts[0], base, bits=1, scale="tensor"),
                      "emr_apply": lambda: eng.emr_apply(base, uni, mask, scale),
                      "delta_apply": lambda: eng.delta_apply(base, sign, None, dscale),
                      "clone_apply": lambda: blob_apply.clone()}
        times = alternate(contenders, args.seconds, args.rounds)
        rec = {"emr_bench": f"{rows}x{cols}", "dtype": args.dtype, "k": k, "bytes": merge_bytes, "apply_bytes": apply_bytes,
               "contested_share": round(rep.contested / n, 6), "mask_share": round(mrep.c / n, 6), "lambda": mrep.lam,
               "rounds": args.rounds}
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            rec[f"{name}_ms"] = round(med[name], 4)
            rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
            rec[f"{name}_rounds_ms"] = [round(v, 4) for v in t]
        rec["emr_GBps"] = round(merge_bytes / med["emr"] / 1e6, 1)
        rec["emr_share_of_8TBps"] = round(merge_bytes / med["emr"] / 1e6 / HBM_PEAK_GBPS, 3)
        rec["emr_ratio_to_clone"] = round(med["emr"] / med["clone"], 3)
        rec["emr_ratio_to_dare_linear"] = round(med["emr"] / med["dare_linear"], 4)
        rec["emr_mask_ratio_to_delta_pack"] = round(med["emr_mask"] / med["delta_pack"], 4)
        rec["emr_apply_ratio_to_delta_apply"] = round(med["emr_apply"] / med["delta_apply"], 4)
        rec["emr_apply_ratio_to_clone"] = round(med["emr_apply"] / med["clone_apply"], 3)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del blob, blob_apply
    append_lines(lines, args.out)


if __name__ == "__main__":
    main()
