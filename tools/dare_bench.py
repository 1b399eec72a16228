#!/usr/bin/env python3
"""Engine.dare_merge against what it is measured against, in one process and on the same inputs: per shape x K and per
mode (dare_ties, dare_linear), the device time of the DARE merge of K finetunes on one shared base that is also the
output base, next to
  * Engine.ties_merge on the same inputs (4K + 5 tensor passes against DARE's K + 2: DARE must be the faster one), and
  * a clone() of as many bytes as the kernel's algorithmic traffic, (K + 2) * element size bytes per element (half
    read, half written): the plain-streaming rate of the box, and optionally
  * --ab-lib: the same library built with -DSM_DARE_NO_PHILOX (tools/build_variant.sh NAME "-DSM_DARE_NO_PHILOX" side_7),
    whose mask is the constant all-kept: the gap to it is the generator's cost.
Timing: HIP events around `reps` back-to-back calls after a warm-up, `--rounds` such windows per contender, the
contenders ALTERNATING inside every round; the median is reported with the (max - min) / median spread of the rounds.
One JSON line per case; --out appends them to a file.

    python tools/dare_bench.py [--shapes 8192x8192,28672x8192,8192x28672] [--ks 2,3] [--density 0.2] [--dtype bf16]
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
    ap.add_argument("--shapes", default="8192x8192,28672x8192,8192x28672")
    ap.add_argument("--ks", default="2,3")
    ap.add_argument("--density", type=float, default=0.2)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per contender and case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ab-lib", default=None, help="a variant of the library to time next to the in-tree one (all-kept mask)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dare_bench: no GPU - a timing needs the device")
    from shardmerge_amd.engine import Engine, get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    variant = None
    if args.ab_lib:
        from shardmerge_amd._lib import SmhipLibrary
        variant = Engine(lib=SmhipLibrary(Path(args.ab_lib)), device=dev)
    key = 0x0123456789ABCDEF
    lines = []
    for rows, cols, k, base, fts, bases in cases(args.shapes, args.ks, DT[args.dtype], dev):
        nbytes = (k + 2) * base.numel() * base.element_size()
        blob = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dare = lambda e, se: (lambda: e.dare_merge(fts, bases, alphas[:k], base, density=args.density, sign_election=se, key=key))
        contenders = {"dare_ties": dare(eng, True), "dare_linear": dare(eng, False),
                      "ties": lambda: eng.ties_merge(fts, bases, alphas[:k], base, density=args.density),
                      "clone": lambda: blob.clone()}
        if variant is not None:
            contenders["dare_ties_no_philox"] = dare(variant, True)
            contenders["dare_linear_no_philox"] = dare(variant, False)
        res = {name: (statistics.median(t), (max(t) - min(t)) / statistics.median(t))
               for name, t in alternate(contenders, args.seconds, args.rounds).items()}
        _, rep = eng.dare_merge(fts, bases, alphas[:k], base, density=args.density, key=key)
        rec = {"dare_bench": f"{rows}x{cols}", "dtype": args.dtype, "k": k, "density": args.density,
               "effective_density": rep.density, "kept_share": [round(c / base.numel(), 6) for c in rep.kept],
               "bytes": nbytes, "rounds": args.rounds}
        for name, (ms, spread) in res.items():
            rec[f"{name}_ms"] = round(ms, 4)
            rec[f"{name}_spread"] = round(spread, 4)
        for mode in ("dare_ties", "dare_linear"):
            ms = res[mode][0]
            rec[f"{mode}_GBps"] = round(nbytes / ms / 1e6, 1)
            rec[f"{mode}_share_of_8TBps"] = round(nbytes / ms / 1e6 / HBM_PEAK_GBPS, 3)
            rec[f"{mode}_ratio_to_clone"] = round(ms / res["clone"][0], 3)
            rec[f"{mode}_speedup_over_ties"] = round(res["ties"][0] / ms, 2)
            if variant is not None:
                rec[f"{mode}_philox_cost"] = round(ms / res[f"{mode}_no_philox"][0] - 1.0, 4)
        rec["faster_than_ties"] = bool(max(res["dare_ties"][0], res["dare_linear"][0]) < res["ties"][0])
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del blob
    append_lines(lines, args.out)
    if not all(rec["faster_than_ties"] for rec in lines):
        sys.exit("dare_merge was not faster than ties_merge in at least one case")


if __name__ == "__main__":
    main()
