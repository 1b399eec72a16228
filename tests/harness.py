"""What the tests of two or more operators share, each thing defined once: the two engine fixtures, the synthetic inputs
and the bit-exact comparisons, the YAML documents and the CLI call, the gloo rank runs, and the per-tensor walk over the
on-disk model of tests/lora_fixtures.py that an operator's expected outputs are built on.

What does NOT belong here: anything that names one operator's options, kernels or oracle.  That stays in the operator's
own tests/X_checks.py, which imports from here."""
import os
import re
import socket
import struct
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import yaml
from click.testing import CliRunner

from tests import lora_fixtures as lf

REPO = Path(__file__).resolve().parents[1]

DTYPES = (torch.bfloat16, torch.float16, torch.float32)
KS = (1, 2, 3, 5, 16)
ALPHAS = (0.5, 0.3, 0.4, 0.25, 0.6, 0.1, 0.35, 0.45, 0.2, 0.15, 0.55, 0.05, 0.7, 0.3, 0.5, 0.4)
SMALL = (97, 131)                                # 12707 elements: not a multiple of 8


# ---- fixtures: a test module imports the one it uses by name, pytest then registers it in that module ------
@pytest.fixture()
def emul(monkeypatch):
    from tests.emul.loader import emul_engine
    from shardmerge_amd import engine as engine_mod
    eng = emul_engine()
    monkeypatch.setattr(engine_mod, "get_engine", lambda device=None: eng)
    return eng


@pytest.fixture(scope="module")
def eng():
    from shardmerge_amd.engine import get_engine
    return get_engine("cuda:0")


# ---- inputs and comparisons ---------------------------------------------------------------------------------
def raw(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def f32_bits(x: float) -> bytes:
    return struct.pack("<f", x)


def f64_bits(x: float) -> bytes:
    return struct.pack("<d", float(x))


def make_inputs(shape, k, in_dtype=torch.bfloat16, bo_dtype=None, seed=0, own_bases=False, sigma=3e-3, device="cpu"):
    """(finetunes, bases, base_out): a base N(0, 0.02^2), finetunes base + N(0, sigma^2), all rounded to their dtype;
    own_bases: every finetune has a base of its own and base_out is yet another tensor"""
    g = torch.Generator(device=device).manual_seed(1000 + seed)
    rn = lambda s: torch.randn(shape, generator=g, device=device, dtype=torch.float32) * s
    bo_dtype = bo_dtype or in_dtype
    shared = rn(0.02)
    bases = [(rn(0.02) if own_bases else shared).to(in_dtype) for _ in range(k)]
    if not own_bases:
        bases = [bases[0]] * k
    fts = [(bases[i].float() + rn(sigma)).to(in_dtype) for i in range(k)]
    base_out = rn(0.02).to(bo_dtype) if own_bases or bo_dtype != in_dtype else bases[0]
    return fts, bases, base_out


def profile_of(engine, call):
    """{kernel name: launches} of one call"""
    engine.ctx.profile(True)
    engine.ctx.profile_reset()
    try:
        call()
        table = engine.ctx.profile_table()
    finally:
        engine.ctx.profile(False)
    return {n: table[n][0] for n in table}


def assert_outputs(out_dir, expected):
    got = lf.read_outputs(out_dir)
    assert sorted(got) == sorted(expected)
    for name in expected:
        assert got[name].dtype == expected[name].dtype and got[name].shape == expected[name].shape, name
        assert torch.equal(raw(got[name]), raw(expected[name])), name


# ---- configs and the CLI --------------------------------------------------------------------------------------
def ties_models(third):
    """layer 0: all three finetunes, layer 1: ft1 and `third`; ft2 is a finetune of ft1 (its own base)"""
    return [{"model": "org/ft1", "base": "org/base", "alpha": 0.5, "is_input": True},
            {"model": "org/ft2", "base": "org/ft1", "alpha": 0.3, "end_layer": 0},
            {"model": third, "base": "org/base", "alpha": 0.4, "is_output": True}]


def yaml_config(tmp_path, options, models=None):
    """the smallest document MergeConfig.from_yaml reads: one org/ft1 entry unless `models` is given"""
    doc = {"output_base_model": "org/base", "finetune_merge": models or [{"model": "org/ft1", "base": "org/base"}],
           "output_dir": str(tmp_path / "merged")}
    if options is not None:
        doc["merge_options"] = options
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(doc))
    return p


def write_config(root, models, out_dir, options, device=None):
    """a run on the on-disk model that lora_fixtures.setup_k3 writes under `root`, the output going to root / out_dir"""
    cfg = {"output_base_model": "org/base", "finetune_merge": models, "output_dir": str(root / out_dir),
           "output_dtype": "bfloat16", "cache_dir": str(root / "cache"), "storage_dir": str(root / "storage")}
    if options is not None:
        cfg["merge_options"] = dict(options)
    if device:
        cfg["device"] = device
    p = root / f"{out_dir}.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return p


def run_cli(cfg_path, command="merge"):
    from shardmerge_amd.__main__ import cli
    return CliRunner().invoke(cli, [command, str(cfg_path)])


# ---- rank runs --------------------------------------------------------------------------------------------------
def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def start_ranks(cfg, world=2, extra_env=None):
    """one tests/dist_worker.py process per gloo rank, started; extra_env overrides, a value of None removes the variable"""
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        env.update(extra_env or {})
        env = {k: v for k, v in env.items() if v is not None}
        procs.append(subprocess.Popen([sys.executable, str(REPO / "tests" / "dist_worker.py"), str(cfg)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    return procs


def run_ranks(cfg, world=2, extra_env=None, timeout=300):
    """the ranks' outputs, after every rank has ended with return code 0; the timeout only caps a hang"""
    procs = start_ranks(cfg, world, extra_env)
    outs = [p.communicate(timeout=timeout)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    return outs


# ---- expected outputs ---------------------------------------------------------------------------------------------
def layer_of(name):
    """the layer of a block tensor, None for a passthrough tensor"""
    m = re.match(r"model\.layers\.(\d+)\.", name)
    return int(m.group(1)) if m else None


def covering(models, layer):
    """[(position in models, entry)] of the entries whose start_layer..end_layer window covers the layer"""
    return [(i, e) for i, e in enumerate(models)
            if e.get("start_layer", 0) <= layer and (e.get("end_layer", -1) == -1 or layer <= e["end_layer"])]


def expected_by_tensor(base, full, models, merge):
    """the expected outputs of a run of `models` (the finetune_merge entries the config was written with) on the on-disk
    model: passthrough tensors from their provider (the embedding from ft1, the rest from `full`, the tensors of the
    entry that is neither org/ft1 nor org/ft2), block tensors from merge(fts, bases, alphas, base_out, name), the
    operator's oracle call, on the entries that cover the tensor's layer"""
    stored = {"org/base": base, "org/ft1": lf.model_tensors(1), "org/ft2": lf.model_tensors(2)}
    out = {}
    for name, _ in lf.TENSORS:
        layer = layer_of(name)
        if layer is None:
            out[name] = stored["org/ft1"][name] if name == "model.embed_tokens.weight" else full[name]
            continue
        entries = [e for _, e in covering(models, layer)]
        out[name] = merge([stored.get(e["model"], full)[name] for e in entries], [stored[e["base"]][name] for e in entries],
                          [e.get("alpha") for e in entries], base[name], name)
    return out
