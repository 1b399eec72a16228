#!/usr/bin/env python3
"""End-to-end `python -m shard merge` on an on-disk synthetic model:
writes base + K finetunes with Llama-3-8B block shapes under a RAM-backed directory, then
runs the CLI's merge with the prefetching loader on and off and prints one JSON line per run
(wall time includes reading the safetensors shards, H2D, the merge, D2H and writing the output).

    python tools/cli_bench.py [--blocks 4] [--k 2] [--root /dev/shm/smcli] [--device cuda] [--lora-rank R] [--delta-bits B]

--lora-rank R writes every finetune as a LoRA adapter of rank R instead (adapter_config.json +
adapter_model.safetensors, every 2-D block projection targeted); input_GB is then what the run reads.
--delta-bits B (1 or 2; 2 at --delta-density) compresses every full finetune into a delta pack with `compress-delta`'s
driver and runs every merge twice: with the full finetunes, then with the packs in their place ("finetunes": "full" /
"delta"), input_GB being what each run reads.
"""
import argparse
import asyncio
import json
import os
import shutil
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import yaml
from safetensors.torch import save_file

BLOCK = [("self_attn.q_proj.weight", 4096, 4096), ("self_attn.k_proj.weight", 1024, 4096),
         ("self_attn.v_proj.weight", 1024, 4096), ("self_attn.o_proj.weight", 4096, 4096),
         ("mlp.gate_proj.weight", 14336, 4096), ("mlp.up_proj.weight", 14336, 4096),
         ("mlp.down_proj.weight", 4096, 14336), ("input_layernorm.weight", 1, 4096),
         ("post_attention_layernorm.weight", 1, 4096)]
BLOCK_70B = [("self_attn.q_proj.weight", 8192, 8192), ("self_attn.k_proj.weight", 1024, 8192),
             ("self_attn.v_proj.weight", 1024, 8192), ("self_attn.o_proj.weight", 8192, 8192),
             ("mlp.gate_proj.weight", 28672, 8192), ("mlp.up_proj.weight", 28672, 8192),
             ("mlp.down_proj.weight", 8192, 28672), ("input_layernorm.weight", 1, 8192),
             ("post_attention_layernorm.weight", 1, 8192)]
SIGMA = (0.002, 0.003, 0.0025, 0.004)


def write_models(root: Path, blocks: int, k: int, gen_device: str, model: str = "llama3-8b", lora_rank: int = 0):
    storage = root / "storage"
    factors = {i: {} for i in range(1, k + 1)}
    uris = ["org/base"] + [f"org/ft{i}" for i in range(1, k + 1)]
    g = torch.Generator(device=gen_device).manual_seed(1000)
    total = 0
    block = BLOCK_70B if model == "llama3-70b" else BLOCK
    hidden = block[0][2]
    for b in range(-1, blocks + 1):               # -1: embed shard, blocks: norm + lm_head shard
        if b == -1:
            items = [("model.embed_tokens.weight", 2048, hidden)]
            shard = "model-embed.safetensors"
        elif b == blocks:
            items = [("model.norm.weight", 1, hidden), ("lm_head.weight", 2048, hidden)]
            shard = "model-head.safetensors"
        else:
            items = [(f"model.layers.{b}.{n}", r, c) for n, r, c in block]
            shard = f"model-{b:05d}.safetensors"
        base = {}
        for name, r, c in items:
            shape = (c,) if r == 1 else (r, c)
            base[name] = (torch.randn(shape, generator=g, device=gen_device) * 0.02).to(torch.bfloat16)
        for which, uri in enumerate(uris):
            d = storage / uri
            d.mkdir(parents=True, exist_ok=True)
            if which and lora_rank:
                for name, t in base.items():
                    if ".layers." in name and t.ndim == 2:
                        module = "base_model.model." + name[: -len(".weight")]
                        sig = (SIGMA[which - 1] / 0.5 / lora_rank ** 0.5) ** 0.5    # s B A ~ SIGMA at s = 0.5
                        factors[which][f"{module}.lora_A.weight"] = (torch.randn((lora_rank, t.shape[1]), generator=g, device=gen_device) * sig).to(torch.bfloat16).cpu()
                        factors[which][f"{module}.lora_B.weight"] = (torch.randn((t.shape[0], lora_rank), generator=g, device=gen_device) * sig).to(torch.bfloat16).cpu()
                continue
            if which == 0:
                tens = {n: t.cpu() for n, t in base.items()}
            else:
                tens = {n: (t.float() + torch.randn(t.shape, generator=g, device=gen_device) * SIGMA[which - 1]).to(torch.bfloat16).cpu()
                        for n, t in base.items()}
            save_file(tens, str(d / shard), metadata={"format": "pt"})
            idx_path = d / "model.safetensors.index.json"
            doc = json.load(open(idx_path)) if idx_path.exists() else {"metadata": {"total_size": 0}, "weight_map": {}}
            doc["weight_map"].update({n: shard for n in tens})
            json.dump(doc, open(idx_path, "w"))
            if which == 0:
                total += sum(t.numel() for t in tens.values())
    for which in factors if lora_rank else ():
        d = storage / uris[which]
        save_file(factors[which], str(d / "adapter_model.safetensors"), metadata={"format": "pt"})
        json.dump({"peft_type": "LORA", "r": lora_rank, "lora_alpha": lora_rank / 2, "bias": "none",
                   "target_modules": sorted({n.split(".")[-3] for n, _, _ in block if n.endswith("proj.weight")})},
                  open(d / "adapter_config.json", "w"))
    cfg = {"output_base_model": "org/base",
           "finetune_merge": [{"model": f"org/ft{i}", "base": "org/base", "alpha": (0.3, 0.5, 0.2, 0.4)[i - 1], "is_input": i == 1}
                              for i in range(1, k + 1)],
           "output_dir": str(root / "merged"), "output_dtype": "bfloat16", "device": "cuda",
           "cache_dir": str(root / "cache"), "storage_dir": str(storage)}
    p = root / "merge.yaml"
    yaml.safe_dump(cfg, open(p, "w"))
    return p, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--root", default="/dev/shm/smcli")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--keep", action="store_true")
    ap.add_argument("--model", default="llama3-8b", choices=["llama3-8b", "llama3-70b"],
                    help="block shapes; llama3-70b with --k 3 is the metric's configuration (1.7 GB of bf16 per block and model)")
    ap.add_argument("--runs", default="0,1,0,1", help="SHARDMERGE_PREFETCH value of each run")
    ap.add_argument("--lora-rank", type=int, default=0, help="write the finetunes as LoRA adapters of this rank")
    ap.add_argument("--delta-bits", type=int, default=0, choices=[0, 1, 2], help="also run with the finetunes as delta packs of this many bits")
    ap.add_argument("--delta-density", type=float, default=0.25, help="--delta-bits 2: the density of the packs")
    args = ap.parse_args()
    if args.delta_bits and args.lora_rank:
        sys.exit("cli_bench: --delta-bits compresses full finetunes; it does not combine with --lora-rank")
    from shardmerge_amd.constants import tune_hip_queues
    tune_hip_queues()
    root = Path(args.root)
    if root.exists():
        shutil.rmtree(root)
    root.mkdir(parents=True)
    t0 = time.time()
    cfg_path, n_params = write_models(root, args.blocks, args.k, args.device if torch.cuda.is_available() else "cpu", args.model,
                                     args.lora_rank)
    size_of = lambda uri: sum(f.stat().st_size for f in (root / "storage" / uri).rglob("*.safetensors"))
    uris = [f"org/ft{i}" for i in range(1, args.k + 1)]
    configs = [("full", cfg_path, size_of("org/base") + sum(size_of(u) for u in uris))]
    if args.delta_bits:
        from shardmerge_amd.merge.compress import run_compression
        t1 = time.time()
        for u in uris:
            asyncio.run(run_compression(u, "org/base", root / "storage" / (u + "_delta"), root / "storage", args.delta_bits,
                                        args.delta_density if args.delta_bits == 2 else None, device=args.device))
        doc = yaml.safe_load(open(cfg_path))
        for m in doc["finetune_merge"]:
            m["model"] += "_delta"
        delta_cfg = root / "merge_delta.yaml"
        yaml.safe_dump(doc, open(delta_cfg, "w"))
        configs.append(("delta", delta_cfg, size_of("org/base") + sum(size_of(u + "_delta") for u in uris)))
        print(f"# compressed {args.k} finetunes to {args.delta_bits} bit(s) in {time.time() - t1:.1f} s", file=sys.stderr)
    print(f"# wrote {args.k + 1} models, {n_params / 1e6:.0f} M params each, in {time.time() - t0:.1f} s under {root}", file=sys.stderr)

    from shardmerge_amd.__main__ import run_merge
    from shardmerge_amd.config import MergeConfig
    from shardmerge_amd import iostats
    for kind, path, read_bytes in configs:
        for prefetch in args.runs.split(","):
            inplace = prefetch.endswith("i")              # "1i": prefetch on + in-place output shards (SHARDMERGE_INPLACE)
            prefetch = prefetch.rstrip("i")
            os.environ["SHARDMERGE_INPLACE"] = "1" if inplace else "0"
            os.environ["SHARDMERGE_PREFETCH"] = prefetch
            out_dir = root / "merged"
            if out_dir.exists():
                shutil.rmtree(out_dir)
            config = MergeConfig.from_yaml(path)
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            iostats.snapshot(reset=True)
            t0 = time.time()
            asyncio.run(run_merge(config, args.device, clean_cache=False))
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            dt = time.time() - t0
            st = iostats.snapshot(reset=True)
            in_gb, out_gb = read_bytes / 1e9, 2.0 * n_params / 1e9
            rec = {"cli_merge": "end to end", "model": args.model, "lora_rank": args.lora_rank, "finetunes": kind, "delta_bits": args.delta_bits if kind == "delta" else 0, "prefetch": prefetch == "1", "inplace_shards": inplace, "blocks": args.blocks, "k": args.k,
                   "params": n_params, "seconds": round(dt, 3), "merged_GBps": round(out_gb / dt, 3), "input_GB": round(in_gb, 2),
                   "stages": st}
            # what the PCIe link allows: every input byte crosses it once, every output byte once, at the H2D rate
            # measured on the copy stream in this run (the two directions are separate lanes: max, not sum)
            h2d = st.get("h2d", {}).get("GBps")
            if h2d:
                rec["pcie_bound_merged_GBps"] = round(out_gb / (max(in_gb, out_gb) / h2d), 3)
                rec["fraction_of_pcie_bound"] = round(rec["merged_GBps"] / rec["pcie_bound_merged_GBps"], 3)
            print(json.dumps(rec))
    if not args.keep:
        shutil.rmtree(root)


if __name__ == "__main__":
    main()
