#!/usr/bin/env python3
"""bench.py - merged-weight GB/s of the spectral-merge hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload llama3-70b-slice|llama3-8b|8192sq] [--k K]
                    [--full] [--dump-outputs DIR]

A plain run sets up, warms up, times the --steps steps and prints the headline (value, ms_per_step).
--full adds everything else it measures: the same steps in the other norm mode, the per-kernel
profile with the roofline (and its two rocprofv3 --pmc passes) and the CPU baseline.
--dump-outputs DIR writes what the last timed step computed: every merged tensor as
DIR/merged_<i>.npy (float32; rank 0; a tensor larger than its share of a 48 MB budget is
sampled at fixed, seeded positions), so that two builds can be compared output for output.

Default workload = the configuration BASELINE.json's metric is quoted on: the Llama-3-70B
3-finetune merge, this GPU's 1/8 slice of the block tensors (10 of 80 blocks), K = 3.
`--gpus N` without a torchrun environment starts the N ranks itself (a child
`python -m torch.distributed.run`, spawned before this process touches the GPU).

One "step" = one pass of the hot path (shardmerge_amd Engine.merge_layer through
libshardmerge_hip.so: deltas -> forward 2-D FFT -> order statistics -> SLERP blend
-> inverse FFT -> add-back -> bf16) over every block tensor of the workload, with
all inputs already resident in HBM.  For N > 1 the driver launches one rank per
GPU (torch.distributed.run); every rank merges its own, equally sized tensor list
(weak scaling, no data-path collective); the shared base tensors are staged once
with ONE RCCL broadcast from rank 0 before the timed region (reported as
base_broadcast_ms).  Rank 0 prints one JSON line.

value    = bytes of merged bf16 weights produced by ALL ranks / max-over-ranks time
roofline = the dominant kernel's algorithmic bytes / its measured device time
           (HIP events on the launch stream, taken in a separate profiled pass so
           that the event syncs do not perturb the timed steps) vs 8 TB/s
cpu_baseline = the CPU oracle (a port of the reference's algorithm; the reference
           itself cannot travel to the GPU box) on a bounded sample, rank 0, N=1.
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

HBM_PEAK = 8.0e12
SIGMAS = (0.002, 0.003, 0.0025, 0.004)
ALPHAS = (0.3, 0.5, 0.2, 0.4)

# block tensor shapes (rows, cols); 1-D norms have rows = 1 (SURVEY section 8 header)
LLAMA3_8B_BLOCK = [(4096, 4096), (1024, 4096), (1024, 4096), (4096, 4096),
                   (14336, 4096), (14336, 4096), (4096, 14336), (1, 4096), (1, 4096)]
LLAMA3_70B_BLOCK = [(8192, 8192), (1024, 8192), (1024, 8192), (8192, 8192),
                    (28672, 8192), (28672, 8192), (8192, 28672), (1, 8192), (1, 8192)]


def workload_shapes(name: str, blocks: int):
    if name == "llama3-8b":
        return LLAMA3_8B_BLOCK * (blocks or 32), "Llama-3-8B block tensors (9 per block x %d blocks)" % (blocks or 32)
    if name == "llama3-70b-slice":
        return LLAMA3_70B_BLOCK * (blocks or 10), "Llama-3-70B block tensors, this rank's 1/8 slice (9 per block x %d blocks)" % (blocks or 10)
    if name == "8192sq":
        return [(8192, 8192)] * (blocks or 4), "synthetic [8192x8192] tensors x %d" % (blocks or 4)
    raise SystemExit(f"unknown workload {name}")


def self_launch(n_gpus: int, argv):
    """--gpus N > 1 outside torchrun: start the N ranks as a CHILD process (this process has not
    initialised the GPU yet and never does) and return its exit code."""
    import socket
    import subprocess
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve())] + list(argv)
    return subprocess.call(cmd, env=env)


def alg_bytes_per_elem(k: int) -> int:
    """B_alg = 60n (K=2), 122n (K=3), 182n (K=4)."""
    if k <= 1:
        return 8
    return 60 * (k // 2) + 62 * (k - 1 - k // 2)       # floor(k/2) raw pairs, the other pairs see an fp32 intermediate


# algorithmic HBM bytes per element of ONE launch of each kernel on a RAW pair (both inputs
# bf16 deltas sharing a base) - SURVEY 8(d) phase table: P1 = F1, P2 = F2, P3/P6 = selection,
# P4 = reduce (fused away), P5 = blend, P7 = I1, P8 = I2
KERNEL_ALG_BYTES = {
    "f1_rows_fwd": 14.0,     # read 3 bf16 tensors (6n) + write two half-spectra (8n)
    "f2_cols_fwd": 14.0,     # read 8n + write Re a, Im a, Re b (6n)
    "i1_cols_inv": 8.0,      # read Re R + Im a (4n) + write 4n
    "i2_rows_inv": 8.0,      # read 4n + base 2n + write bf16 2n   (or: read 4n + write fp32 4n)
    "blend": 6.0,
    "slerp_reduce": 4.0,
    "select_lvl2": 4.0,      # the cutoff's level-2 pass over (Re a, Re b)
    "select_lvl2_cull": 0.0, # the cull's level-2 pass over Re R: normally done inside the blend's sweep (speculation on the
                             # threshold's level-1 bin), this launch then returns at once; 2n when it has to run
    "select_hist": 3.0,
    "combine": 6.0,
}
# norm_mode = reference_cpu: the torch.norm emulation's own passes (per delta: read finetune + base once for the
# summaries, 1/16 of them for the estimate; per pair merge: a sample of the two Re planes)
REF_NORM_BYTES_PER_DELTA = 4.0 + 0.25
REF_NORM_BYTES_PER_PAIR = 0.5


def norms_fused_in_row_pass(rows: int, cols: int) -> bool:
    """reference_cpu, round 4: the forward row pass k_f1 summarises its own deltas (no separate pass over finetunes and
    bases) when its row plan can - whole groups of 2048 elements per row, at least two chunks of 65536 - and the shape
    does not take the folded row pass k_f1q (14336 / 16384 / 28672 rows over <= 8192 columns), which keeps the
    separate summary pass (sm_pipeline.hpp: fusable_rows, fold_shape)."""
    folded = rows in (14336, 16384, 28672) and cols <= 8192
    return rows > 1 and cols % 2048 == 0 and rows * cols >= 2 * 65536 and not folded


def moved_bytes_per_elem(k: int, norm_mode: str, shape=None) -> float:
    """HBM bytes per tensor element this implementation moves for one K-way layer: 56n for
    a raw pair (K = 2), 85n at K = 3 (every delta's rows alone, intermediates stay spectral), plus the norm
    emulation's passes in reference_cpu mode (shape: a tensor whose row pass carries the summaries has no such pass)."""
    if k <= 1:
        return 8.0
    if k == 2:
        base = 14 + 14 + 4 + 6 + 2 + 8 + 8
    else:
        pairs = k - 1
        # (row passes: one launch for all K deltas, the K signals of a row block on one XCD - the shared base rows are
        #  read from HBM once: K (2 + 4) + 2 instead of 8 K; PMC: profiles/traffic_latest.json)
        base = (k * 6 + 2) + k * 7 + pairs * (4 + 6 + 2) + (pairs - 1) * 4 + 16
    if norm_mode == "reference_cpu":
        if shape is not None and norms_fused_in_row_pass(*shape):
            base += k * 0.25 + (k - 1) * REF_NORM_BYTES_PER_PAIR          # the sampled prefix estimate only
        else:
            # (the summary pass reads the shared base once per chunk as well: 2 K + 2 instead of 4 K)
            base += (k * (REF_NORM_BYTES_PER_DELTA - 2.0) + 2.0) + (k - 1) * REF_NORM_BYTES_PER_PAIR
    return float(base)


def moved_bytes_of(shapes, k: int, norm_mode: str) -> float:
    """element-weighted mean of moved_bytes_per_elem over a tensor list"""
    tot = sum(r * c for r, c in shapes)
    return sum(moved_bytes_per_elem(k, norm_mode, (r, c)) * r * c for r, c in shapes) / max(tot, 1)


def csrc_stamp() -> str:
    """sha256 over the kernel sources: profiles/traffic_latest.json is only quoted for the code it was measured on"""
    import hashlib
    h = hashlib.sha256()
    for f in sorted((REPO / "shardmerge_amd" / "csrc").glob("*")):
        if f.suffix in (".hpp", ".hip", ".inc") and f.is_file():
            h.update(f.name.encode())
            h.update(f.read_bytes())
    return h.hexdigest()[:16]


def kernel_alg_bytes_per_elem(name: str, k: int) -> float:
    """Algorithmic bytes per tensor element summed over ALL launches of kernel `name` in one
    K-way layer merge as THIS implementation runs it: K-1 pair merges;
    K = 2: one fused two-signal pair.  K >= 3: every delta's rows are transformed alone first (row
    pairs; the norms come with it), column passes per signal once the pairing is known, every
    non-final result stays in the spectral domain (spec_norm + spec_rescale, no transforms)."""
    pairs = max(k - 1, 1)
    per = KERNEL_ALG_BYTES.get(name, 0.0)
    if k >= 3:
        inter = pairs - 1                        # spectral intermediates produced and consumed
        table = {
            "f1_rows_fwd": k * 8.0,                        # every delta alone (row pairs): 4n in + 4n out, norms included
            "f2_cols_fwd": 0.0,                            # (the fused two-signal column pass is K = 2's)
            "f2s_cols_fwd1": k * 7.0,                      # 4n in + Re, Im out (role a) or Re out (role b)
            "i1_cols_inv": 8.0, "i2_rows_inv": 8.0,        # the final inverse only
            "spec_norm": inter * 4.0,                      # Re R + Im a (fallback: normally fused into select_lvl2 / f2s)
            "spec_rescale": inter * 4.0,                   # role b: Re in, Re out (role a: 8n)
            "select_hist": per * 2 * pairs,
        }
    else:
        table = {"select_hist": per * 2 * pairs}
    if k >= 2 and name in table:
        return table[name]
    return per * pairs


def make_inputs(shapes, k, device, seed, shared_base=None):
    """bf16 base + k finetunes per tensor, generated on the GPU."""
    g = torch.Generator(device=device).manual_seed(seed)
    layers = []
    for i, (r, c) in enumerate(shapes):
        shape = (c,) if r == 1 else (r, c)
        if shared_base is not None:
            base = shared_base[i]
        else:
            base = (torch.randn(shape, generator=g, device=device) * 0.02).to(torch.bfloat16)
        fts = [(base.float() + torch.randn(shape, generator=g, device=device) * SIGMAS[j % 4]).to(torch.bfloat16)
               for j in range(k)]
        layers.append((base, fts))
    return layers


def run_step(engines, layers, k, norm_mode="exact", sink=None):
    """One pass over the tensor list.  With more than one engine the tensors are merged
    concurrently, one worker thread + HIP stream + workspace per engine (the C calls release
    the GIL); tensors are independent units, so this is the same job, pipelined.
    sink(i, out), if given, is called with every merged tensor on the stream that produced it."""
    if len(engines) == 1:
        outs = 0
        for i, (base, fts) in enumerate(layers):
            out, rep = engines[0][0].merge_layer(fts, [base] * k, ALPHAS[:k], base, norm_mode=norm_mode)
            outs += out.numel()
            if sink is not None:
                sink(i, out)
        return outs
    import threading
    counts = [0] * len(engines)
    errors = []
    # shared work queue in model order: neighbouring tensors differ in shape, so the streams run
    # different kernels side by side (sorting by size made all of them run the same kernel: slower)
    order = list(range(len(layers)))
    cursor = [0]
    lock = threading.Lock()

    def work(w):
        eng, stream = engines[w]
        try:
            with torch.cuda.stream(stream):
                while True:
                    with lock:
                        if cursor[0] >= len(order):
                            break
                        i = order[cursor[0]]
                        cursor[0] += 1
                    base, fts = layers[i]
                    out, rep = eng.merge_layer(fts, [base] * k, ALPHAS[:k], base, norm_mode=norm_mode)
                    counts[w] += out.numel()
                    if sink is not None:
                        sink(i, out)
            stream.synchronize()
        except Exception as e:            # surface worker failures
            errors.append(e)

    threads = [threading.Thread(target=work, args=(w,)) for w in range(len(engines))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    return sum(counts)


DUMP_BUDGET_BYTES = 48 << 20   # --dump-outputs: float32 bytes written in all
DUMP_SEED = 20251015


class OutputDump:
    """--dump-outputs: a run_step sink that keeps, on the device, every merged tensor of one step as float32 - whole,
    or at fixed positions (a seeded sample drawn once, the same in every run) when it is larger than its equal share
    of DUMP_BUDGET_BYTES - and writes them as DIR/merged_<i>.npy."""

    def __init__(self, shapes, device):
        import numpy as np
        share = DUMP_BUDGET_BYTES // 4 // max(len(shapes), 1)
        self.index = []
        for i, (r, c) in enumerate(shapes):
            n = r * c
            if n <= share:
                self.index.append(None)
            else:
                pos = np.unique(np.random.default_rng([DUMP_SEED, i]).integers(0, n, size=share))
                self.index.append(torch.from_numpy(pos).to(device))
        self.got = {}

    def __call__(self, i, out):
        flat = out.reshape(-1)
        self.got[i] = (flat if self.index[i] is None else flat.index_select(0, self.index[i])).float()

    def write(self, out_dir):
        import numpy as np
        d = Path(out_dir)
        d.mkdir(parents=True, exist_ok=True)
        for i in range(len(self.index)):
            np.save(d / f"merged_{i:03d}.npy", self.got[i].cpu().numpy())


CPU_BASELINE_THREADS = 16      # capped: the sort-bound oracle gets SLOWER with hundreds of threads


def cpu_baseline(k: int):
    """The CPU oracle (the reference's algorithm as it is: full sorts, torch's CPU norms) on a bounded sample of the
    workload: ONE synthetic [8192 x 8192] bf16 layer - SURVEY 8(d)'s micro-benchmark shape - merged K-way with the
    benchmarked K (K - 1 pair merges; K > 3 is timed at K = 3 and scaled), on a stated, capped number of threads."""
    from oracle import spectral_oracle as so
    rows = cols = 8192
    kk = min(max(k, 2), 3)
    base, fts = so.synthetic_layer(rows, cols, kk, seed=1000)
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    threads = max(1, min(CPU_BASELINE_THREADS, avail))
    torch.set_num_threads(threads)
    t0 = time.time()
    so.merge_layer(fts, [base] * kk, so.ALPHAS[:kk], base)
    dt = time.time() - t0
    dt_k = dt * max(k - 1, 1) / (kk - 1)
    v = 2.0 * rows * cols / dt_k / 1e9
    return {"value": v, "unit": "GB/s", "cores": threads, "kind": "port",
            "sample": f"oracle.merge_layer, K={kk} ({kk - 1} SLERP-FFT pair merge(s)) on one synthetic [{rows}x{cols}] bf16 layer, "
                      f"{threads} threads of {avail} available ({dt:.1f} s)" + (f"; scaled to K={k}: {dt_k:.1f} s" if kk != k else "")}


def load_traffic(workload: str, k: int, kernel: str):
    """Per-launch HBM bytes of `kernel` from the committed rocprofv3 --pmc summary
    (profiles/traffic_latest.json, written by tools/traffic_run.sh).  The file is stamped with
    the workload it was measured on; a stamp that does not match this run gives None (traffic
    is per-launch on a shape mix: another workload's number would be wrong, not stale)."""
    tf = REPO / "profiles" / "traffic_latest.json"
    if not tf.exists():
        return None
    try:
        data = json.load(open(tf))
    except Exception:
        return None
    meta = data.get("_meta", {})
    if meta.get("workload") != workload or int(meta.get("k", -1)) != int(k):
        return None
    if meta.get("csrc_sha") != csrc_stamp():          # measured on other kernel sources: not this code's traffic
        return None
    return data.get(kernel, {}).get("hbm_bytes_per_launch")


def live_traffic(workload: str, k: int):
    """HBM traffic per launch of every kernel, measured IN THIS RUN: two `rocprofv3 --pmc` passes (FETCH_SIZE, WRITE_SIZE:
    they do not fit one pass) over one single-stream step of one block of the workload, as child processes (the program
    itself behind `--`, cwd /tmp), corrected as MI355X_MICROARCH.md prescribes (tools/pmc_traffic.py).  Returns
    ({kernel: record}, None) or (None, why not)."""
    import shutil
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None, "rocprofv3 not found"
    if any(k_.startswith(("ROCPROF", "ROCP_")) for k_ in os.environ) or "rocprof" in os.environ.get("LD_PRELOAD", ""):
        return None, "this run is itself under a profiler"
    sys.path.insert(0, str(REPO / "tools"))
    import pmc_traffic
    child = [sys.executable, str(REPO / "bench.py"), "--workload", workload, "--k", str(k), "--blocks", "1", "--steps", "1", "--warmup", "0",
             "--streams", "1", "--no-cpu-baseline", "--no-profile", "--no-alt-mode", "--prewarm-seconds", "0", "--no-live-traffic"]
    got = {}
    try:
        with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
            for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
                d = os.path.join(tmp, ctr)
                r = subprocess.run([prof, "--pmc", ctr, "--output-format", "csv", "-d", d, "--"] + child, cwd="/tmp",
                                   env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, timeout=300)
                if r.returncode != 0:
                    return None, f"rocprofv3 --pmc {ctr} exited {r.returncode}: {r.stderr.decode(errors='replace')[-300:]}"
                got[ctr] = pmc_traffic.load(d, ctr)
        return pmc_traffic.aggregate(got["FETCH_SIZE"], got["WRITE_SIZE"]), None
    except Exception as exc:            # a profiler problem must not cost the bench line
        return None, f"{type(exc).__name__}: {exc}"


def product_path_bench(args, world, rank, device, dist):
    """--product-path: the PRODUCT's multi-GPU loop (distributed.py: plan, base-shard broadcasts a window ahead,
    prefetching loader, in-place output shards), timed end to end on a synthetic on-disk model - what `python -m shard
    merge` does under torchrun.  Strong scaling: ONE model of --blocks Llama-3-70B blocks (default 2 per rank), K
    finetunes, partitioned over the N ranks.  Reports merged GB/s (output bytes / max-over-ranks wall time) and, per
    rank, the share of its loop spent waiting for a base shard's payload."""
    import asyncio
    import shutil
    sys.path.insert(0, str(REPO / "tools"))
    import cli_bench
    from shardmerge_amd import distributed as sd
    from shardmerge_amd.config import MergeConfig
    from shardmerge_amd.index import LocalModelIndex
    k = args.k
    blocks = args.blocks or 2 * world
    root = Path(args.product_root)
    os.environ["LOCAL_RANK"] = str(device.index)        # (a one-GPU rehearsal over gloo puts every rank on the same card)
    model = "llama3-8b" if args.workload == "llama3-8b" else "llama3-70b"
    if rank == 0:
        if root.exists():
            shutil.rmtree(root)
        root.mkdir(parents=True)
        cfg_path, n_params = cli_bench.write_models(root, blocks, k, str(device), model)
    if dist:
        dist.barrier()
    cfg_path = root / "merge.yaml"

    def one_run():
        if rank == 0 and (root / "merged").exists():
            shutil.rmtree(root / "merged")
        torch.cuda.synchronize()
        if dist:
            dist.barrier()
        cfg = MergeConfig.from_yaml(cfg_path)
        t0 = time.time()
        st = asyncio.run(sd.run_partitioned_merge(cfg, LocalModelIndex(cfg.storage_path), str(device)))
        torch.cuda.synchronize()
        if dist:
            dist.barrier()
        return time.time() - t0, st

    for _ in range(max(args.warmup, 1)):
        one_run()
    times, stats = [], None
    for _ in range(args.steps):
        dt, stats = one_run()
        times.append(dt)
    dt = sum(times)
    per_rank = [stats]
    if dist:
        tmax = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
        per_rank = [None] * world
        dist.all_gather_object(per_rank, stats)
    if rank == 0:
        out_bytes = sum(s_["out_bytes"] for s_ in per_rank)
        total_out = 0
        for f in (root / "merged").glob("*.safetensors"):
            total_out += f.stat().st_size
        result = {
            "metric": "merged-weight GB/s per GPU + % HBM roofline, Llama-3-70B 3-way FFT merge",
            "mode": "product_path (distributed.run_partitioned_merge end to end: disk -> H2D -> merge -> D2H -> disk)",
            "value": total_out * args.steps / dt / 1e9, "unit": "GB/s", "n_gpus": world, "steps": args.steps, "warmup": max(args.warmup, 1),
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f32", "data": f"synthetic safetensors under {root}", "norm_mode": "reference_cpu",
            "config": {"workload": f"{model} block tensors x {blocks} blocks (+ embedding, norm, lm_head), K={k}, one model partitioned over {world} rank(s)",
                       "k": k, "parallelism": f"tensor-partition x{world}: one broadcast per base shard, no reduction"},
            "output_GB": round(total_out / 1e9, 3), "input_GB": round(total_out * (k + 1) / 1e9, 3),
            "per_rank": [{"rank": s_["rank"], "tensors": s_["tensors"], "out_GB": round(s_["out_bytes"] / 1e9, 3),
                          "loop_s": round(s_["loop_s"], 3), "wait_base_pct": round(100.0 * s_["wait_base_s"] / max(s_["loop_s"], 1e-9), 1),
                          "merge_pct": round(100.0 * s_["merge_s"] / max(s_["loop_s"], 1e-9), 1)} for s_ in per_rank],
        }
        print(json.dumps(result))
        if not os.environ.get("SHARDMERGE_BENCH_KEEP"):
            shutil.rmtree(root, ignore_errors=True)
    if dist:
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--prewarm-seconds", type=float, default=1.5, help="untimed steps in front of the warmup steps (clock ramp of an idle GPU)")
    ap.add_argument("--workload", default="llama3-70b-slice",
                    help="llama3-70b-slice (default: the metric's configuration) | llama3-8b | 8192sq")
    ap.add_argument("--blocks", type=int, default=0)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--streams", type=int, default=8, help="tensors merged concurrently (one engine/stream/workspace each)")
    ap.add_argument("--norm-mode", default="reference_cpu", choices=["reference_cpu", "exact"],
                    help="reference_cpu (default): every norm as the reference's device=cpu run takes it (torch.norm's CPU kernel, "
                         "emulated exactly) - the mode whose output matches the reference as it is; exact: accurate L2 norms")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-alt-mode", action="store_true", help="skip the extra timed steps in the other norm mode")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="do not run the two rocprofv3 --pmc passes for roofline.traffic (the committed profiles/traffic_latest.json is quoted when its stamp matches)")
    ap.add_argument("--product-path", action="store_true",
                    help="measure shardmerge_amd.distributed.run_partitioned_merge end to end instead of resident tensors: "
                         "synthetic safetensors models under --product-root, N ranks partition ONE model (strong scaling), "
                         "base shards travel by broadcast, every rank writes its results into the output shards")
    ap.add_argument("--product-root", default="/dev/shm/smbench_product")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline does not need: the steps in the other norm mode, the per-kernel profile "
                         "and roofline (with its rocprofv3 --pmc passes) and the CPU baseline (the --no-* options still apply)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/merged_<i>.npy (float32, rank 0; large tensors at "
                         "fixed, seeded positions; at most 48 MB in all)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.product_path:
        ap.error("--dump-outputs measures the resident-tensor path, not --product-path")
    from shardmerge_amd.constants import tune_hip_queues
    tune_hip_queues()                   # 8 engines + their side streams: before the first GPU call (children inherit it)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # not under torchrun: start the ranks as a child before anything here touches the GPU
        raise SystemExit(self_launch(args.gpus, sys.argv[1:]))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # one rank per GPU.  (Rehearsal on a one-GPU box: SHARDMERGE_BENCH_BACKEND=gloo lets several
    # ranks share the card - RCCL itself refuses two ranks on one device.)
    backend = os.environ.get("SHARDMERGE_BENCH_BACKEND", "nccl")
    dev_index = local_rank if backend == "nccl" else local_rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)

    if args.product_path:
        return product_path_bench(args, world, rank, device, dist)

    from shardmerge_amd.engine import Engine, get_engine
    engine = get_engine(device)
    engines = [(engine, torch.cuda.current_stream(device))]
    for _ in range(1, max(1, args.streams)):
        engines.append((Engine(device=device), torch.cuda.Stream(device=device)))

    # tuning experiments only: SMHIP_DEBUG=fold_columns=0,spectral_intermediates=0 (library test hooks)
    for item in filter(None, os.environ.get("SMHIP_DEBUG", "").split(",")):
        key, val = item.split("=")
        for eng, _ in engines:
            eng.ctx.debug_option(key, int(val))

    shapes, desc = workload_shapes(args.workload, args.blocks)
    k = args.k
    # stage inputs: rank 0 owns the shared base; ONE RCCL broadcast distributes it
    bcast_ms = None
    shared = None
    if world > 1:
        g = torch.Generator(device=device).manual_seed(1000)
        total = sum(r * c for r, c in shapes)
        flat = torch.empty(total, dtype=torch.bfloat16, device=device)
        if rank == 0:
            flat.copy_((torch.randn(total, generator=g, device=device) * 0.02).to(torch.bfloat16))
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.time()
        dist.broadcast(flat, src=0)
        torch.cuda.synchronize()
        bcast_ms = (time.time() - t0) * 1e3
        shared, off = [], 0
        for r, c in shapes:
            shared.append(flat[off:off + r * c].view((c,) if r == 1 else (r, c)))
            off += r * c
    layers = make_inputs(shapes, k, device, seed=1000 + 17 * rank, shared_base=shared)
    n_elems = sum(r * c for r, c in shapes)
    dump = OutputDump(shapes, device) if args.dump_outputs and rank == 0 else None

    # the GPU of a fresh box idles at its lowest clocks and the first steps of a process also pay for code-object
    # loading and workspace growth: run untimed steps for --prewarm-seconds before the W warmup steps (one fresh
    # box measured 67 GB/s in this mode next to 95 GB/s for the accurate-norm steps that followed in the same
    # process; every other run 80-83: DESIGN.md section 7)
    t_pre = time.time()
    prewarm_steps = 0
    while args.prewarm_seconds > 0 and (time.time() - t_pre < args.prewarm_seconds or prewarm_steps < 3):     # the first step alone takes ~2 s
        run_step(engines, layers, k, args.norm_mode)
        torch.cuda.synchronize()
        prewarm_steps += 1
    for _ in range(args.warmup):
        run_step(engines, layers, k, args.norm_mode)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    t0 = time.time()
    for step in range(args.steps):
        run_step(engines, layers, k, args.norm_mode, sink=dump if step == args.steps - 1 else None)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    dt = time.time() - t0
    if dist:
        tmax = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    if dump is not None:
        dump.write(args.dump_outputs)

    out_bytes = 2.0 * n_elems * args.steps * world
    value = out_bytes / dt / 1e9
    result = {
        "metric": "merged-weight GB/s per GPU + % HBM roofline, Llama-3-70B 3-way FFT merge",
        "value": value, "unit": "GB/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "prewarm_steps": prewarm_steps,
        "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic", "norm_mode": args.norm_mode,
        "config": {"workload": f"{desc}, K={k} finetunes, bf16 in/out, resident in HBM", "workload_id": args.workload, "tensors_per_step": len(shapes),
                   "params_per_step_per_gpu": n_elems, "k": k, "parallelism": f"tensor-partition x{world} (no data-path collective)", "streams_per_gpu": len(engines)},
        "per_gpu_GBps": value / world,
        # canonical algorithmic bytes (60n / 122n / 182n - what the REFERENCE's data flow needs) per second
        # over the HBM peak: an effective, speedup-style figure ...
        "pipeline_hbm_frac": alg_bytes_per_elem(k) * n_elems * args.steps / dt / HBM_PEAK,
        # ... and the bytes this implementation actually moves (it keeps intermediates spectral, fuses the norms)
        "pipeline_hbm_frac_moved": moved_bytes_of(shapes, k, args.norm_mode) * n_elems * args.steps / dt / HBM_PEAK,
        "pipeline_bytes_per_elem": {"canonical": alg_bytes_per_elem(k), "moved": round(moved_bytes_of(shapes, k, args.norm_mode), 3)},
        "spectral_intermediates": not any(item.startswith("spectral_intermediates=0") for item in os.environ.get("SMHIP_DEBUG", "").split(",")),
        "base_broadcast_ms": bcast_ms,
    }
    # the cull selection's speculation: how often the guessed level-1 bin was right
    checked = sum(eng.ctx.debug_query("spec_checked") for eng, _ in engines)
    hits = sum(eng.ctx.debug_query("spec_hits") for eng, _ in engines)
    result["cull_speculation"] = {"checked": checked, "confirmed": hits, "hit_rate": (hits / checked) if checked else None}

    if args.full and not args.no_alt_mode:
        # the same steps in the other norm mode, for comparison (the headline stays the conforming mode's)
        alt = "exact" if args.norm_mode == "reference_cpu" else "reference_cpu"
        run_step(engines, layers, k, alt)
        torch.cuda.synchronize()
        if dist:
            dist.barrier()
        t0 = time.time()
        for _ in range(args.steps):
            run_step(engines, layers, k, alt)
        torch.cuda.synchronize()
        if dist:
            dist.barrier()
        dta = time.time() - t0
        if dist:
            tmax = torch.tensor([dta], device=device, dtype=torch.float64)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dta = float(tmax.item())
        result["alt_norm_mode"] = {"norm_mode": alt, "value": out_bytes / dta / 1e9, "ms_per_step": dta / args.steps * 1e3,
                                   "pipeline_hbm_frac": alg_bytes_per_elem(k) * n_elems * args.steps / dta / HBM_PEAK}

    if rank == 0 and args.full and not args.no_profile:
        # per-kernel device time: HIP events around every launch on the launch stream
        # (library profiling mode), one extra pass, single stream
        engine.ctx.profile(True)
        engine.ctx.profile_reset()
        run_step(engines[:1], layers, k, args.norm_mode)
        torch.cuda.synchronize()
        table = engine.ctx.profile_table()
        engine.ctx.profile(False)
        tot_ms = sum(ms for _, ms in table.values())
        kern = {name: {"launches": n, "total_ms": round(ms, 3), "share": round(ms / tot_ms, 4) if tot_ms else 0}
                for name, (n, ms) in table.items()}
        dom = max(table.items(), key=lambda kv: kv[1][1])[0]
        # algorithmic bytes of the dominant kernel over the step: per-element bytes of its
        # launches on one tensor (SURVEY 8d / DESIGN.md 5) x elements of every tensor
        n_2d = sum(r * c for r, c in shapes)
        per_elem = kernel_alg_bytes_per_elem(dom, k)
        alg = per_elem * n_2d
        launches, dom_ms = table[dom]
        traffic, traffic_src = None, None
        if world == 1 and not args.no_live_traffic:
            live, why = live_traffic(args.workload, k)
            if live is not None and dom in live:
                traffic, traffic_src = live[dom]["hbm_bytes_per_launch"], "two rocprofv3 --pmc passes (FETCH_SIZE x 2, WRITE_SIZE) in this run, one block, single stream"
                result["traffic_by_kernel"] = {n_: round(v["hbm_bytes_per_launch"]) for n_, v in live.items() if not n_.startswith("_") and v["launches"]}
            else:
                traffic_src = f"live measurement unavailable ({why})"
        if traffic is None:
            traffic = load_traffic(args.workload, k, dom)
            if traffic is not None:
                traffic_src = "profiles/traffic_latest.json (stamped with this tree's kernel sources)"
        result["roofline"] = {"bound": "hbm", "kernel": dom, "achieved": alg / (dom_ms / 1e3) / 1e9, "peak": HBM_PEAK / 1e9,
                              "unit": "GB/s", "frac": alg / (dom_ms / 1e3) / HBM_PEAK, "traffic": traffic, "traffic_source": traffic_src,
                              "alg_bytes_per_launch": alg / launches, "avg_launch_ms": dom_ms / launches,
                              "alg_bytes_per_elem_per_layer": per_elem}
        # every streaming kernel's own fraction of the HBM peak (same measurement)
        result["kernel_hbm_frac"] = {
            name: round(kernel_alg_bytes_per_elem(name, k) * n_2d / (ms / 1e3) / HBM_PEAK, 4)
            for name, (n, ms) in table.items() if kernel_alg_bytes_per_elem(name, k) > 0 and ms > 0}
        result["kernels"] = kern
        result["device_ms_profiled_step"] = round(tot_ms, 3)
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline(k)
    if rank == 0:
        print(json.dumps(result))
    if dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
