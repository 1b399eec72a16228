"""What tools/ties_bench.py, dare_bench.py and breadcrumbs_bench.py share: the inputs, the alternating timer and the
JSON-lines output."""
import json
from pathlib import Path

import torch

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
HBM_PEAK_GBPS = 8000.0
ALPHAS = [0.5, 0.3, 0.4, 0.25, 0.6, 0.1, 0.35, 0.45, 0.2, 0.15, 0.55, 0.05, 0.7, 0.3, 0.5, 0.4]


def window(fn, reps: int) -> float:
    """mean ms per call over `reps` back-to-back calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(contenders, seconds: float, rounds: int, warmup: int = 5):
    """{name: [ms per round]}: every round times each contender once, in turn"""
    reps = {}
    for name, fn in contenders.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        reps[name] = max(10, int(seconds * 1e3 / rounds / max(window(fn, 3), 1e-3)))
    times = {name: [] for name in contenders}
    for _ in range(rounds):
        for name, fn in contenders.items():
            times[name].append(window(fn, reps[name]))
    return times


def cases(shapes: str, ks: str, dtype: torch.dtype, dev):
    """(rows, cols, k, base, finetunes, bases) per shape x K: K finetunes on one shared base that is also the output base"""
    g = torch.Generator(device=dev).manual_seed(0)
    for shape in shapes.split(","):
        rows, cols = (int(v) for v in shape.split("x"))
        base = (torch.randn(rows, cols, generator=g, device=dev) * 0.02).to(dtype)
        for k in (int(v) for v in ks.split(",")):
            fts = [(base.float() + torch.randn(rows, cols, generator=g, device=dev) * 3e-3).to(dtype) for _ in range(k)]
            yield rows, cols, k, base, fts, [base] * k
            del fts
            torch.cuda.empty_cache()
        del base
        torch.cuda.empty_cache()


def append_lines(lines, out) -> None:
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        with open(out, "a") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")
