#!/usr/bin/env python3
"""The fused EMR pass against what it replaces, in one process and on the same inputs.

Kernels (default): per shape x K, K bf16 finetunes on one shared base that is also the output base -
  * Engine.emr_merge_masks (one fused pass and one fold) next to Engine.emr_merge followed by K Engine.emr_mask calls,
    the composition it equals bit for bit; both as whole calls (HIP events around `reps` back-to-back calls after a
    warm-up, `--rounds` windows per contender, the contenders ALTERNATING inside every round; medians and the max - min
    spread of the rounds);
  * the same fused call with the debug option "emr_fused_geo_fold" = 1, which folds the same [R][7K] partials with
    geo_gram_fold instead of emr_fold;
  * the per-kernel split of one profiled call of each contender (events around each launch).
--cli: end to end on the synthetic on-disk model of tools/cli_bench.py - wall time and bytes read (iostats) of ONE
`merge --emr-packs` run against the plain merge followed by K `emr-task` runs, and whether the packs are equal.
No threshold is asserted: the ratios and the spreads are printed, one JSON line per case; --out appends them to a file.

    python tools/emr_fused_bench.py [--shapes 8192x8192,28672x8192] [--ks 2,3] [--cli] [--blocks 4] [--k 3]
"""
import argparse
import asyncio
import json
import shutil
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from delta_bench_common import DT, alternate, append_lines, cases


def profiled(eng, call):
    """{kernel: ms} of one call, by events around each launch"""
    eng.ctx.profile(True)
    eng.ctx.profile_reset()
    try:
        call()
        table = eng.ctx.profile_table()
    finally:
        eng.ctx.profile(False)
    return {name: round(table[name][1], 4) for name in table}


def kernels(args, eng):
    dev = eng.device
    lines = []
    for rows, cols, k, base, fts, bases in cases(args.shapes, args.ks, DT[args.dtype], dev):
        es, n = base.element_size(), base.numel()
        uni, _ = eng.emr_merge(fts, bases, base)

        def composed():
            out, _ = eng.emr_merge(fts, bases, base)
            for i in range(k):
                eng.emr_mask(fts[i], base, out)

        def fused_geo():
            eng.ctx.debug_option("emr_fused_geo_fold", 1)
            try:
                eng.emr_merge_masks(fts, bases, base)
            finally:
                eng.ctx.debug_option("emr_fused_geo_fold", 0)

        contenders = {"fused": lambda: eng.emr_merge_masks(fts, bases, base), "merge_then_masks": composed, "fused_geo_fold": fused_geo}
        times = alternate(contenders, args.seconds, args.rounds)
        rec = {"emr_fused_bench": f"{rows}x{cols}", "dtype": args.dtype, "k": k, "rounds": args.rounds,
               "fused_bytes": (k + 2) * n * es + k * n // 8, "composed_bytes": (k + 2) * n * es + k * (3 * n * es + n // 8)}
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            rec[f"{name}_ms"] = round(med[name], 4)
            rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
            rec[f"{name}_rounds_ms"] = [round(v, 4) for v in t]
        rec["fused_ratio_to_merge_then_masks"] = round(med["fused"] / med["merge_then_masks"], 4)
        rec["fused_GBps"] = round(rec["fused_bytes"] / med["fused"] / 1e6, 1)
        # the per-kernel split, and the two folds on the same partials: five profiled calls each, the median
        split = {"fused": [], "fused_geo_fold": [], "merge_then_masks": []}
        for _ in range(args.rounds):
            for name, fn in contenders.items():
                split[name].append(profiled(eng, fn))
        for name, runs in split.items():
            rec[f"{name}_kernels_ms"] = {kn: round(statistics.median(r[kn] for r in runs), 4) for kn in runs[0]}
        folds = {"emr_fold": [r["emr_fold"] for r in split["fused"]], "geo_gram_fold": [r["geo_gram_fold"] for r in split["fused_geo_fold"]]}
        for name, t in folds.items():
            rec[f"{name}_ms"] = round(statistics.median(t), 4)
            rec[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
        rec["emr_fold_ratio_to_geo_gram_fold"] = round(rec["emr_fold_ms"] / rec["geo_gram_fold_ms"], 4)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del uni
    append_lines(lines, args.out)


def cli(args):
    import yaml
    from cli_bench import write_models
    from shardmerge_amd import iostats
    from shardmerge_amd.__main__ import run_merge
    from shardmerge_amd.config import MergeConfig
    from shardmerge_amd.merge.emr_packs import EmrPackOptions
    from shardmerge_amd.merge.emr_task import run_emr_task
    root = Path(args.root)
    if root.exists():
        shutil.rmtree(root)
    root.mkdir(parents=True)
    cfg_path, n_params = write_models(root, args.blocks, args.k, args.device if torch.cuda.is_available() else "cpu", args.model)
    doc = yaml.safe_load(open(cfg_path))
    for i, m in enumerate(doc["finetune_merge"]):
        m.update(alpha=1.0, is_output=i == args.k - 1)
    doc["merge_options"] = {"operator": "emr"}
    storage = root / "storage"

    def timed(label, work):
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        iostats.snapshot(reset=True)
        t0 = time.time()
        work()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        dt = time.time() - t0
        st = iostats.snapshot(reset=True)
        return {"step": label, "seconds": round(dt, 3), "read_GB": st.get("read", {}).get("GB", 0.0), "stages": st}     # (the loader's reads)

    def config(out):
        doc["output_dir"] = str(storage / out)
        path = root / f"{out.replace('/', '_')}.yaml"
        yaml.safe_dump(doc, open(path, "w"))
        return MergeConfig.from_yaml(path)

    steps = []
    fused_cfg = config("org/uni")
    steps.append(timed("merge --emr-packs", lambda: asyncio.run(run_merge(fused_cfg, args.device, clean_cache=False,
                                                                            emr_pack_options=EmrPackOptions(storage, "org/uni")))))
    plain_cfg = config("org/uni_plain")
    steps.append(timed("merge", lambda: asyncio.run(run_merge(plain_cfg, args.device, clean_cache=False))))
    for i in range(1, args.k + 1):
        steps.append(timed(f"emr-task org/ft{i}", lambda i=i: asyncio.run(run_emr_task(f"org/ft{i}", "org/base", "org/uni_plain",
                                                                                       storage / f"org/task{i}", storage, device=args.device))))
    equal = all((storage / f"org/ft{i}-emr" / "emr_model.safetensors").read_bytes() ==
                (storage / f"org/task{i}" / "emr_model.safetensors").read_bytes() for i in range(1, args.k + 1))
    rec = {"emr_fused_cli": "end to end", "model": args.model, "blocks": args.blocks, "k": args.k, "params": n_params, "steps": steps,
           "with_packs_seconds": steps[0]["seconds"], "merge_then_tasks_seconds": round(sum(s["seconds"] for s in steps[1:]), 3),
           "with_packs_read_GB": steps[0]["read_GB"], "merge_then_tasks_read_GB": round(sum(s["read_GB"] for s in steps[1:]), 3),
           "pack_bytes_equal": equal}
    print(json.dumps(rec), flush=True)
    append_lines([rec], args.out)
    if not args.keep:
        shutil.rmtree(root)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192x8192,28672x8192")
    ap.add_argument("--ks", default="2,3")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed work per contender and case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--cli", action="store_true", help="the end-to-end comparison instead of the kernels")
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--model", default="llama3-8b", choices=["llama3-8b", "llama3-70b"])
    ap.add_argument("--root", default="/dev/shm/smemrfused")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--keep", action="store_true")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("emr_fused_bench: the comparison wants at least five alternating rounds")
    if not torch.cuda.is_available():
        sys.exit("emr_fused_bench: no GPU - a timing needs the device")
    from shardmerge_amd.constants import tune_hip_queues
    tune_hip_queues()
    from shardmerge_amd.engine import get_engine
    if args.cli:
        cli(args)
    else:
        kernels(args, get_engine("cuda:0"))


if __name__ == "__main__":
    main()
