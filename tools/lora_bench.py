#!/usr/bin/env python3
"""smhip_lora_apply against the copy rate: per shape x rank x factor dtype, the device time of
Engine.lora_apply (HIP events, after warm-up, repeated to fill at least --seconds) and, in the same process, of a
clone() of the same base tensor (the same bytes moved: one read, one write).  One JSON line per case:
time, effective GB/s (base read + output write) and the ratio to the clone.
--dora also times the DoRA apply (a magnitude vector: norm pass, row factors, apply pass) in the same process; its
bytes are two reads and one write of the base plus the magnitude, and it is reported against lora_apply and the clone.
--embedding times the embedding-LoRA layout on [128256 x 4096] and [128256 x 8192] bases instead of --shapes.

    python tools/lora_bench.py [--shapes 8192x8192,28672x8192,8192x28672] [--ranks 16,64,256] [--factors bf16,f16,f32]
                               [--dora | --embedding]
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def timed(fn, seconds: float, warmup: int = 5) -> float:
    """mean ms per call over enough calls to fill `seconds`"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    reps = max(10, int(seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192x8192,28672x8192,8192x28672")
    ap.add_argument("--ranks", default="16,64,256")
    ap.add_argument("--factors", default="bf16,f16,f32")
    ap.add_argument("--base", default="bf16")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--dora", action="store_true", help="also time the DoRA apply (a magnitude vector)")
    ap.add_argument("--embedding", action="store_true", help="time the embedding layout at [128256 x 4096 | 8192]")
    args = ap.parse_args()
    if args.embedding:
        args.shapes = "128256x4096,128256x8192"
    from shardmerge_amd.engine import get_engine
    eng = get_engine("cuda:0")
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for shape in args.shapes.split(","):
        rows, cols = (int(v) for v in shape.split("x"))
        base = (torch.randn(rows, cols, generator=g, device=dev) * 0.02).to(DT[args.base])
        clone_ms = timed(lambda: base.clone(), args.seconds)
        nbytes = 2 * base.numel() * base.element_size()
        for rank in (int(r) for r in args.ranks.split(",")):
            for fname in args.factors.split(","):
                if args.embedding:        # lora_embedding_A [r, num_embeddings], lora_embedding_B [dim, r]
                    a = (torch.randn(rank, rows, generator=g, device=dev) * 0.05).to(DT[fname])
                    b = (torch.randn(cols, rank, generator=g, device=dev) * 0.05).to(DT[fname])
                else:
                    a = (torch.randn(rank, cols, generator=g, device=dev) * 0.05).to(DT[fname])
                    b = (torch.randn(rows, rank, generator=g, device=dev) * 0.05).to(DT[fname])
                ms = timed(lambda: eng.lora_apply(base, a, b, 2.0, embedding=args.embedding), args.seconds)
                rec = {"lora_bench": f"{rows}x{cols}", "base": args.base, "rank": rank, "factors": fname,
                       "ms": round(ms, 4), "GBps": round(nbytes / ms / 1e6, 1), "clone_ms": round(clone_ms, 4),
                       "clone_GBps": round(nbytes / clone_ms / 1e6, 1), "ratio_to_clone": round(ms / clone_ms, 3)}
                if args.embedding:
                    rec["layout"] = "embedding"
                if args.dora:
                    m = torch.rand(rows, generator=g, device=dev) + 0.5
                    dms = timed(lambda: eng.lora_apply(base, a, b, 2.0, magnitude=m), args.seconds)
                    dbytes = 3 * base.numel() * base.element_size() + m.numel() * m.element_size()
                    rec.update({"dora_ms": round(dms, 4), "dora_GBps": round(dbytes / dms / 1e6, 1),
                                "dora_to_lora": round(dms / ms, 3), "dora_to_clone": round(dms / clone_ms, 3)})
                    del m
                print(json.dumps(rec), flush=True)
                lines.append(rec)
                del a, b
        del base
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
