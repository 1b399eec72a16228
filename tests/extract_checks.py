"""Checks of the low-rank extraction shared by the emulator tier (tests/test_extract_host.py) and the GPU tier
(tests/test_extract_gpu.py): the primitives of csrc/sm_extract.hpp through smhip_xl_probe and Engine.lora_extract against
tests/extract_oracle.py, bit for bit (the tolerance is zero and derived: every value is an fp32 fma chain, an fp64 sum or
a one-rounding fp64 operation in a stated order); a layout check on exact integers and the quality checks, which do not
use the oracle."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from shardmerge_amd import _lib
from shardmerge_amd.merge.dare import tensor_key
from tests import extract_oracle as xo

S = xo.SEG
SHAPES = ((1, 1), (3, 5), (17, 33), (130, 257), (64, S - 1), (64, S), (64, S + 1), (2 * S + 100, 48))
WIDTHS = (16, 32, 80, 272)
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
EXTRACT_SHAPES = ((320, 192), (192, 320))
RANKS = (8, 16, 64)
POWERS = (0, 1, 2)
KEY = 0x0123456789ABCDEF


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host(t):
    return t.detach().cpu()


def pair(rows, cols, dtype, seed, scale=0.02, offset=0):
    """(finetune, base) of `dtype`; offset: views one element into their storage (not 16-byte aligned)"""
    g = torch.Generator().manual_seed(seed)
    n = rows * cols
    base = torch.randn(n + offset, generator=g).to(dtype)
    ft = (base.float() + scale * torch.randn(n + offset, generator=g)).to(dtype)
    return ft[offset:].view(rows, cols), base[offset:].view(rows, cols)


def on(engine, t):
    """the tensor on the engine's device with the same storage offset"""
    if engine.device.type == "cpu":
        return t
    off = t.storage_offset()
    flat = torch.empty(off + t.numel(), dtype=t.dtype, device=engine.device)
    flat[off:] = t.reshape(-1)
    return flat[off:].view(t.shape)


# ---- 1. the primitives -----------------------------------------------------------------------------------------
def check_fill(engine, nrows, L):
    y = engine.xl_probe(_lib.XL_FILL, rows=nrows, L=L, key=KEY)
    ref = xo.fill(nrows, L, KEY)
    assert np.array_equal(bits32(host(y).numpy()), bits32(ref)), (nrows, L)
    assert set(np.unique(ref)) <= {-1.0, 1.0}
    y2 = engine.xl_probe(_lib.XL_FILL, rows=nrows, L=L, key=KEY + 1)
    if nrows * L >= 256:
        assert not torch.equal(host(y), host(y2))                 # the key matters
        assert abs(float(ref.mean())) < 6.0 / np.sqrt(ref.size)   # 6 sigma of a fair coin


def check_delta_mm(engine, rows, cols, L, dtype, offset=0, special=False, seed=0):
    ft, base = pair(rows, cols, dtype, 100 + seed + rows + cols, offset=offset)
    if special:                                                    # zeros and a denormal delta
        ft = ft.clone()
        ft.view(-1)[::3] = base.reshape(-1)[::3]
        if dtype == torch.float32 and ft.numel() > 4:
            ft.view(-1)[4] = base.reshape(-1)[4] + 1e-41
    D = xo.delta(ft, base)
    g = torch.Generator().manual_seed(7 + seed)
    for trans in (0, 1):
        X = torch.randn(rows if trans else cols, L, generator=g)
        args = dict(rows=rows, cols=cols, L=L, trans=trans, finetune=on(engine, ft), base=on(engine, base), x=X)
        y = host(engine.xl_probe(_lib.XL_DELTA_MM, **args)).numpy()
        ref = xo.delta_mm(D, X.numpy(), trans)
        assert np.array_equal(bits32(y), bits32(ref)), (rows, cols, L, str(dtype), trans, offset,
                                                         float(np.abs(y - ref).max()))
        y2 = host(engine.xl_probe(_lib.XL_DELTA_MM, **args)).numpy()
        assert np.array_equal(bits32(y), bits32(y2)), "two calls differ"


def check_delta_mm_nonfinite(engine):
    """NaN and +-Inf in the delta propagate to the panel as the fma chain propagates them"""
    ft, base = pair(17, 33, torch.float32, 5)
    ft = ft.clone()
    ft[2, 3], ft[5, 7], ft[9, 30] = float("nan"), float("inf"), float("-inf")
    D = xo.delta(ft, base)
    g = torch.Generator().manual_seed(3)
    for trans in (0, 1):
        X = torch.randn(17 if trans else 33, 16, generator=g)
        y = host(engine.xl_probe(_lib.XL_DELTA_MM, rows=17, cols=33, L=16, trans=trans, finetune=on(engine, ft), base=on(engine, base), x=X)).numpy()
        ref = xo.delta_mm(D, X.numpy(), trans)
        assert np.array_equal(np.isnan(y), np.isnan(ref)) and np.isnan(ref).any()
        ok = ~np.isnan(ref)
        assert np.array_equal(bits32(y)[ok], bits32(ref)[ok])
    with pytest.raises(ValueError, match="model.layers.0.q_proj.weight"):
        engine.lora_extract(on(engine, ft), on(engine, base), 4, name="model.layers.0.q_proj.weight")


def check_layout_integers(engine, rows, cols, dtype=torch.bfloat16):
    """independent of the oracle: small integers and +-1, every sum exact in any order; D is asymmetric"""
    g = torch.Generator().manual_seed(rows)
    Di = torch.randint(-3, 4, (rows, cols), generator=g)
    base = torch.randint(-4, 5, (rows, cols), generator=g)
    ft = (base + Di).to(dtype)
    base = base.to(dtype)
    for trans in (0, 1):
        K = rows if trans else cols
        Xi = torch.randint(0, 2, (K, 32), generator=g) * 2 - 1
        y = host(engine.xl_probe(_lib.XL_DELTA_MM, rows=rows, cols=cols, L=32, trans=trans, finetune=on(engine, ft), base=on(engine, base), x=Xi.float()))
        ref = (Di.T if trans else Di).to(torch.int64) @ Xi.to(torch.int64)
        assert torch.equal(y.to(torch.int64), ref) and torch.equal(y, ref.float()), (rows, cols, trans)


def check_gram(engine, m, L):
    g = torch.Generator().manual_seed(m + L)
    P = torch.randn(m, L, generator=g)
    G = host(engine.xl_probe(_lib.XL_GRAM, rows=m, L=L, x=P)).numpy()
    ref = xo.gram(P.numpy())
    assert np.array_equal(bits64(G), bits64(ref)), (m, L)
    assert np.array_equal(G, G.T)
    G2 = host(engine.xl_probe(_lib.XL_GRAM, rows=m, L=L, x=P)).numpy()
    assert np.array_equal(bits64(G), bits64(G2))


def check_panel_mm(engine, m, L, L2, out_dtype, trans):
    g = torch.Generator().manual_seed(m + L + L2)
    P, T = torch.randn(m, L, generator=g), torch.randn(L, L2, generator=g)
    y = host(engine.xl_probe(_lib.XL_PANEL_MM, rows=m, L=L, L2=L2, x=P, t=T, trans=trans, out_dtype=out_dtype))
    ref = xo.round_factor(xo.panel_mm(P.numpy(), T.numpy()), out_dtype)
    ref = ref.T.contiguous() if trans else ref
    assert torch.equal(y.view(torch.int16 if out_dtype != torch.float32 else torch.int32),
                       ref.view(torch.int16 if out_dtype != torch.float32 else torch.int32)), (m, L, L2, str(out_dtype), trans)


def gram_matrix(L, rank, seed):
    """a Gram as orth meets it: PSD, of the given rank"""
    g = torch.Generator().manual_seed(seed)
    P = torch.randn(3 * L, rank, generator=g) @ torch.randn(rank, L, generator=g)
    return xo.gram(P.float().numpy())


def check_sym_eig(engine, L, rank):
    G = gram_matrix(L, rank, L + rank)
    e = engine.xl_probe(_lib.XL_SYM_EIG, rows=1, L=L, x=torch.from_numpy(G)).numpy()
    lam, V = xo.sym_eig(G)
    assert np.array_equal(bits64(e[:L]), bits64(lam)) and np.array_equal(bits64(e[L:].reshape(L, L)), bits64(V)), (L, rank)
    # and what it is for, against LAPACK: fp64 accuracy relative to the largest eigenvalue
    ref = np.linalg.eigvalsh(G)[::-1]
    assert np.abs(lam - ref).max() <= 1e-13 * ref[0] * L, (L, rank, np.abs(lam - ref).max() / ref[0])
    assert np.abs(V.T @ V - np.eye(L)).max() < 1e-12 and np.all(np.diff(lam) <= 0)
    assert all(V[np.argmax(np.abs(V[:, i])), i] > 0 for i in range(L))


# ---- 3. the whole extraction -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def extract_case(rows, cols, rank, q, low_rank=0):
    """inputs and the oracle's result, computed once per process; low_rank: the finetune is a merged adapter of that rank"""
    ft, base = pair(rows, cols, torch.bfloat16, 11 * rows + rank)
    if low_rank:
        g = torch.Generator().manual_seed(rows + low_rank)
        # small integers: the delta is EXACTLY of that rank (a bf16 rounding of the sum would fill the spectrum with noise)
        base = torch.randint(-8, 9, (rows, cols), generator=g).bfloat16()
        prod = torch.randint(-1, 2, (rows, low_rank), generator=g) @ torch.randint(-1, 2, (low_rank, cols), generator=g)
        ft = (base.float() + prod.float()).bfloat16()
    name = f"layers.{rows}x{cols}.weight"
    return ft, base, name, xo.extract(ft, base, rank, q, tensor_key(5, name))


def assert_extract_equals(a, b, rep, ref, factor_dtype, label):
    ra, rb = xo.round_factor(ref["a32"], factor_dtype), xo.round_factor(ref["b32"], factor_dtype)
    as_int = torch.int32 if factor_dtype == torch.float32 else torch.int16
    assert torch.equal(host(a).view(as_int), ra.view(as_int)), (label, "A")
    assert torch.equal(host(b).view(as_int), rb.view(as_int)), (label, "B")
    assert rep.width == ref["L"] and rep.effective_rank == ref["rho"] and rep.orth_ranks == ref["orth_ranks"], (label, rep, ref["rho"], ref["orth_ranks"])
    assert np.array_equal(bits64(np.array(rep.sigma)), bits64(ref["sigma"])), (label, "sigma")
    assert bits64(np.array([rep.delta_sq, rep.share])).tolist() == bits64(np.array([ref["delta_sq"], ref["share"]])).tolist(), (label, rep.delta_sq, rep.share, ref["delta_sq"], ref["share"])


def check_extract(engine, rows, cols, rank, q, factor_dtype, low_rank=0):
    ft, base, name, ref = extract_case(rows, cols, rank, q, low_rank)
    a, b, rep = engine.lora_extract(on(engine, ft), on(engine, base), rank, power_iters=q, factor_dtype=factor_dtype, seed=5, name=name)
    label = f"{rows}x{cols} r={rank} q={q} {factor_dtype}"
    print(f"{label}: rho {rep.effective_rank}, orth {rep.orth_ranks}, share {rep.share:.6f}")
    assert tuple(a.shape) == (rank, cols) and tuple(b.shape) == (rows, rank) and a.dtype == b.dtype == factor_dtype
    assert_extract_equals(a, b, rep, ref, factor_dtype, label)
    a2, b2, rep2 = engine.lora_extract(on(engine, ft), on(engine, base), rank, power_iters=q, factor_dtype=factor_dtype, seed=5, name=name)
    assert torch.equal(host(a), host(a2)) and torch.equal(host(b), host(b2)) and rep == rep2, "two calls differ"
    return rep


def check_extract_against(engine, other, rows, cols, rank, q=2, factor_dtype=torch.bfloat16):
    """the device against the emulator library (the shapes whose numpy chain takes more than a few seconds)"""
    ft, base = pair(rows, cols, torch.bfloat16, rows + cols)
    name = "model.layers.3.mlp.down_proj.weight"
    a, b, rep = engine.lora_extract(on(engine, ft), on(engine, base), rank, power_iters=q, factor_dtype=factor_dtype, seed=1, name=name)
    a2, b2, rep2 = other.lora_extract(ft, base, rank, power_iters=q, factor_dtype=factor_dtype, seed=1, name=name)
    print(f"{rows}x{cols} r={rank}: rho {rep.effective_rank}, orth {rep.orth_ranks}, share {rep.share:.6f}")
    assert torch.equal(host(a).view(torch.int16), a2.view(torch.int16)) and torch.equal(host(b).view(torch.int16), b2.view(torch.int16))
    assert rep.orth_ranks == rep2.orth_ranks and rep.effective_rank == rep2.effective_rank
    assert bits64(np.array(rep.sigma + [rep.delta_sq, rep.share])).tolist() == bits64(np.array(rep2.sigma + [rep2.delta_sq, rep2.share])).tolist()


# ---- 4. quality, independent of the oracle -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def quality_inputs():
    """the three 320 x 192 fp32 deltas, the exact-rank one, and their fp64 singular values.  The base is zero: the
    inputs ARE the deltas (over a base of O(1) values the fp32 sum base + d would add rounding noise of 1e-5 of the
    delta to it, and the exact-rank input would not be of exact rank)"""
    g = torch.Generator().manual_seed(2024)
    rows, cols = 320, 192
    U, _ = torch.linalg.qr(torch.randn(rows, cols, generator=g, dtype=torch.float64))
    W, _ = torch.linalg.qr(torch.randn(cols, cols, generator=g, dtype=torch.float64))
    spec = 0.05 / torch.arange(1, cols + 1, dtype=torch.float64)
    d1 = (U * spec) @ W.T
    d2 = 0.003 * torch.randn(rows, cols, generator=g, dtype=torch.float64)
    exact = 1e-3 * torch.randn(rows, 16, generator=g, dtype=torch.float64) @ torch.randn(16, cols, generator=g, dtype=torch.float64)
    d3 = exact + 0.05 * d2
    base = torch.zeros(rows, cols)
    out = {}
    for name, d in (("decay", d1), ("gauss", d2), ("lowrank+noise", d3), ("exact16", exact)):
        ft = base + d.float()
        D = (ft.double() - base.double())                          # the delta the function sees, exactly
        out[name] = (ft, base, D, torch.linalg.svdvals(D))
    return out


def check_quality(engine, which, rank):
    ft, base, D, sv = quality_inputs()[which]
    a, b, rep = engine.lora_extract(on(engine, ft), on(engine, base), rank, power_iters=2, factor_dtype=torch.float32, name=which)
    err = torch.linalg.norm(D - host(b).double() @ host(a).double())
    best = torch.sqrt((sv[rank:] ** 2).sum())
    ratio = float(err / best)
    print(f"quality {which} r={rank}: ||D - BA|| / ||D - D_r|| = {ratio:.5f}, share {rep.share:.6f}")
    assert ratio <= 1.02, (which, rank, ratio)
    assert abs(rep.residual_bound - float(err / torch.linalg.norm(D))) < 1e-4
    return ratio


def check_exact_rank(engine, rank):
    ft, base, D, sv = quality_inputs()["exact16"]
    a, b, rep = engine.lora_extract(on(engine, ft), on(engine, base), rank, power_iters=2, factor_dtype=torch.float32, name="exact16")
    rel = float(torch.linalg.norm(D - host(b).double() @ host(a).double()) / torch.linalg.norm(D))
    print(f"exact rank 16, r={rank}: rho {rep.effective_rank}, ||D - BA|| / ||D|| = {rel:.3e}")
    return rep, host(a), host(b), rel


# ---- 5. the round trip -------------------------------------------------------------------------------------------
def check_round_trip(engine, rank):
    g = torch.Generator().manual_seed(8)
    n = 1024
    base = (0.02 * torch.randn(n, n, generator=g)).bfloat16()
    a0 = (0.02 * torch.randn(8, n, generator=g)).bfloat16()
    b0 = (0.02 * torch.randn(n, 8, generator=g)).bfloat16()
    bd = on(engine, base)
    ft = engine.lora_apply(bd, on(engine, a0), on(engine, b0), 1.0)
    a, b, rep = engine.lora_extract(ft, bd, rank, factor_dtype=torch.bfloat16, name="round.trip")
    back = engine.lora_apply(bd, a, b, 1.0)
    share = float((host(back).view(torch.int16) != host(ft).view(torch.int16)).float().mean())
    # the fp64 optimum, its factors split and rounded the same way, applied by the same lora_apply
    D = host(ft).double() - base.double()
    U, sv, Vh = torch.linalg.svd(D, full_matrices=False)
    s = torch.sqrt(sv[:rank])
    keep = sv[:rank] > 1e-6 * sv[0]
    br = ((U[:, :rank] * s) * keep).float().bfloat16()
    ar = ((Vh[:rank] * s[:, None]) * keep[:, None]).float().bfloat16()
    ref_back = engine.lora_apply(bd, on(engine, ar), on(engine, br), 1.0)
    ref_share = float((host(ref_back).view(torch.int16) != host(ft).view(torch.int16)).float().mean())
    msg = f"round trip r={rank}: differing elements {share:.6f}, fp64 optimum {ref_share:.6f}, rho {rep.effective_rank}"
    print(msg)
    assert share <= ref_share * 1.1 + 1e-4, msg
    return share, ref_share


# ---- 7. the C ABI ------------------------------------------------------------------------------------------------
def check_c_abi(engine):
    ft, base = pair(32, 48, torch.bfloat16, 1)
    ft, base = on(engine, ft), on(engine, base)
    dll, h = engine.lib.dll, engine.ctx.h
    need = int(dll.smhip_lora_extract_workspace(32, 48, 8))
    assert need > 0 and dll.smhip_lora_extract_workspace(32, 48, 0) == 0 and dll.smhip_lora_extract_workspace(32, 48, 257) == 0
    ws = engine._xl_workspace(need)
    a = torch.empty(8, 48, dtype=torch.bfloat16, device=engine.device)
    b = torch.empty(32, 8, dtype=torch.bfloat16, device=engine.device)
    rep = _lib.ExtractReport()

    def call(a_ptr=None, b_ptr=None, rep_ref=None, **over):
        f = dict(finetune=ft.data_ptr(), base=base.data_ptr(), in_dtype=_lib.BF16, rows=32, cols=48, rank=8, power_iters=2, key=1,
                 factor_dtype=_lib.BF16, workspace=ws.data_ptr(), workspace_bytes=need)
        f.update(over)
        d = _lib.ExtractDesc(**f)
        return dll.smhip_lora_extract(h, C.byref(d), a.data_ptr() if a_ptr is None else a_ptr, b.data_ptr() if b_ptr is None else b_ptr,
                                      C.byref(rep) if rep_ref is None else rep_ref, engine._stream())
    assert call() == _lib.OK
    bad = [dict(finetune=None), dict(base=None), dict(rank=0), dict(rank=257), dict(power_iters=5), dict(power_iters=-1),
           dict(in_dtype=3), dict(factor_dtype=-1), dict(rows=0), dict(cols=0), dict(workspace=None),
           dict(workspace_bytes=need - 1), dict(workspace=ws.data_ptr() + 8)]
    for over in bad:
        assert call(**over) == _lib.ERR_ARG, over
        assert b"lora_extract" in dll.smhip_last_error(h)
    assert call(a_ptr=C.c_void_p(None)) == _lib.ERR_ARG and call(b_ptr=C.c_void_p(None)) == _lib.ERR_ARG
    assert call(rep_ref=C.POINTER(_lib.ExtractReport)()) == _lib.ERR_ARG
    assert dll.smhip_lora_extract(h, None, a.data_ptr(), b.data_ptr(), C.byref(rep), engine._stream()) == _lib.ERR_ARG
    for kw in (dict(rank=0), dict(rank=300), dict(rank=True), dict(power_iters=5), dict(factor_dtype=torch.int8)):
        with pytest.raises(ValueError):
            engine.lora_extract(ft, base, **{"rank": 4, **kw})
    with pytest.raises(ValueError):
        engine.lora_extract(ft, base[:, :40], 4)


def check_profile(engine, q, rank=8, shape=(320, 192)):
    """the profile names of the header and their launch counts"""
    ft, base = pair(*shape, torch.bfloat16, 2)
    ft, base = on(engine, ft), on(engine, base)
    engine.ctx.profile(True)
    engine.ctx.profile_reset()
    try:
        engine.lora_extract(ft, base, rank, power_iters=q)
        table = engine.ctx.profile_table()
    finally:
        engine.ctx.profile(False)
    want = {"xl_fill": 1, "xl_delta_mm": 2 * q + 2, "xl_fold": 2 * q + 2, "xl_gram": 2 * q + 2, "xl_gram_fold": 2 * q + 2,
            "xl_panel_mm": 2 * q + 3, "geo_gram": 1, "geo_gram_fold": 1}
    assert {k: v[0] for k, v in table.items()} == want, table


# ---- 6. the command ----------------------------------------------------------------------------------------------
def run_cli(args):
    from click.testing import CliRunner
    from shardmerge_amd.__main__ import cli
    return CliRunner().invoke(cli, [str(a) for a in args])


def extract_args(root, model, out, device, rank=8, more=()):
    return ["extract-lora", model, "--base", "org/base", "--rank", rank, "--out", root / "storage" / out,
            "--storage-dir", root / "storage", "--device", device, *more]


def check_command(tmp_path, engine, device):
    """extract-lora of a materialised rank-8 adapter: the three files, the reader accepts them, `merge` takes DIR as an
    entry, two runs give the same bytes"""
    import asyncio
    import json
    from shardmerge_amd.adapter import LoraAdapter, base_tensor_meta
    from shardmerge_amd.index import LocalModelIndex
    from tests import lora_fixtures as lf
    base, factors, full = lf.setup_k3(tmp_path, engine)
    storage = tmp_path / "storage"
    res = run_cli(extract_args(tmp_path, "org/lora_full", "org/extracted", device))
    assert res.exit_code == 0, res.output
    out = storage / "org/extracted"
    assert sorted(p.name for p in out.iterdir()) == ["adapter_config.json", "adapter_model.safetensors", "extraction.json"]
    adapter = LoraAdapter("org/extracted", out)
    index = LocalModelIndex(storage_path=storage)
    asyncio.run(index.add_model("org/base"))
    adapter.check_against("org/base", base_tensor_meta(index, "org/base"))
    targeted = sorted(n for n, _ in lf.TENSORS if any(n.endswith(f".{t}.weight") for t in lf.TARGETS))
    assert sorted(adapter.pairs) == targeted and all(p.rank == 8 and p.scale == 1.0 for p in adapter.pairs.values())
    cfg = json.loads((out / "adapter_config.json").read_text())
    assert cfg["r"] == 8 and cfg["lora_alpha"] == 8 and cfg["use_rslora"] is False and cfg["rank_pattern"] == {}
    assert cfg["target_modules"] == ["q_proj", "v_proj"] and cfg["base_model_name_or_path"] == "org/base"
    rep = json.loads((out / "extraction.json").read_text())
    assert sorted(t["name"] for t in rep["tensors"]) == targeted and rep["skipped"] == []
    for t in rep["tensors"]:                                       # a merged rank-8 adapter, rounded to bf16 once
        assert t["r"] == 8 and t["rho"] == 8 and len(t["sigma"]) == 16 and t["share"] > 0.999, t
        assert abs(t["residual_bound"] - (1 - t["share"]) ** 0.5) < 1e-12
    assert "share" in res.output and "q_proj" in res.output
    # the adapter stands for the finetune: applied, it differs from it in no more elements than bf16 factors explain
    from safetensors.torch import load_file
    got = load_file(str(out / "adapter_model.safetensors"))
    for name in targeted:
        mod = name[:-len(".weight")]
        back = host(engine.lora_apply(on(engine, base[name]), on(engine, got[f"base_model.model.{mod}.lora_A.weight"]),
                                      on(engine, got[f"base_model.model.{mod}.lora_B.weight"]), 1.0))
        assert float((back.float() - full[name].float()).norm() / (full[name].float() - base[name].float()).norm()) < 0.02, name
    # DIR as a finetune_merge entry
    cfgp = lf.write_config(tmp_path, lf.k3_models("org/extracted"), "merged", "ties")
    res = run_cli(["merge", cfgp, "--device", device])
    assert res.exit_code == 0, res.output
    assert sorted(lf.read_outputs(tmp_path / "merged")) == sorted(n for n, _ in lf.TENSORS)
    # the same bytes twice; and an existing adapter is not overwritten
    res = run_cli(extract_args(tmp_path, "org/lora_full", "org/extracted2", device))
    assert res.exit_code == 0, res.output
    for f in ("adapter_model.safetensors", "adapter_config.json", "extraction.json"):
        assert (out / f).read_bytes() == (storage / "org/extracted2" / f).read_bytes(), f
    before = (out / "adapter_model.safetensors").read_bytes()
    res = run_cli(extract_args(tmp_path, "org/lora_full", "org/extracted", device))
    assert res.exit_code != 0 and (out / "adapter_model.safetensors").read_bytes() == before


def check_command_variants(tmp_path, engine, device):
    """a changed norm is skipped and listed; --modules; embed_tokens as embedding-LoRA; the clipped rank's patterns"""
    import asyncio
    import json
    from shardmerge_amd.adapter import LoraAdapter, base_tensor_meta
    from shardmerge_amd.index import LocalModelIndex
    from tests import lora_fixtures as lf
    storage = tmp_path / "storage"
    base = lf.model_tensors(0)
    lf.write_model(storage, "org/base", base)
    ft = dict(lf.model_tensors(1))
    for name in base:                                              # only the norms, the embedding and layer 0's q / k differ
        if not (name.endswith("layernorm.weight") and ".0." in name or "embed_tokens" in name or name.endswith(("0.self_attn.q_proj.weight", "0.self_attn.k_proj.weight"))):
            ft[name] = base[name]
    lf.write_model(storage, "org/ft", ft)
    res = run_cli(extract_args(tmp_path, "org/ft", "org/x", device, rank=96, more=["--dtype", "fp32", "--power-iters", 1]))
    assert res.exit_code == 0, res.output
    out = storage / "org/x"
    rep = json.loads((out / "extraction.json").read_text())
    assert [s["name"] for s in rep["skipped"]] == ["model.layers.0.input_layernorm.weight"] and 0 < rep["skipped"][0]["relative_delta"] < 1
    assert "skipped" in res.output
    assert sorted(t["name"] for t in rep["tensors"]) == ["model.embed_tokens.weight", "model.layers.0.self_attn.k_proj.weight", "model.layers.0.self_attn.q_proj.weight"]
    cfg = json.loads((out / "adapter_config.json").read_text())
    assert cfg["r"] == 96 and cfg["rank_pattern"] == {"model.embed_tokens": 64, "model.layers.0.self_attn.k_proj": 64} == cfg["alpha_pattern"]
    adapter = LoraAdapter("org/x", out)
    index = LocalModelIndex(storage_path=storage)
    asyncio.run(index.add_model("org/base"))
    adapter.check_against("org/base", base_tensor_meta(index, "org/base"))
    emb = adapter.pairs["model.embed_tokens.weight"]
    assert emb.kind == "embedding" and emb.rank == 64 and all(p.scale == 1.0 for p in adapter.pairs.values())
    # at full rank in fp32 the adapter reproduces the finetune's delta
    from safetensors.torch import load_file
    got = load_file(str(out / "adapter_model.safetensors"))
    assert got["base_model.model.model.embed_tokens.lora_embedding_A"].dtype == torch.float32
    back = host(engine.lora_apply(on(engine, base["model.embed_tokens.weight"]), on(engine, got["base_model.model.model.embed_tokens.lora_embedding_A"]),
                                  on(engine, got["base_model.model.model.embed_tokens.lora_embedding_B"]), 1.0, embedding=True))
    assert torch.equal(back, ft["model.embed_tokens.weight"])
    # --modules: by module-name suffix; the others are not read
    res = run_cli(extract_args(tmp_path, "org/ft", "org/y", device, more=["--modules", "q_proj"]))
    assert res.exit_code == 0, res.output
    rep = json.loads((storage / "org/y" / "extraction.json").read_text())
    assert [t["name"] for t in rep["tensors"]] == ["model.layers.0.self_attn.q_proj.weight"] and "model.embed_tokens.weight" in rep["not_selected"]


def check_command_rejections(tmp_path, engine, device, monkeypatch):
    """every rejection raises before DIR exists"""
    import asyncio
    from shardmerge_amd.merge.extract import LoraExtraction
    from tests import lora_fixtures as lf
    lf.setup_k3(tmp_path, engine)
    storage = tmp_path / "storage"
    odd = dict(lf.model_tensors(1))
    odd["lm_head.weight"] = odd["lm_head.weight"].float()
    lf.write_model(storage, "org/odd_dtype", odd)
    odd = dict(lf.model_tensors(1))
    odd["model.norm.weight"] = odd["model.norm.weight"][:64]
    lf.write_model(storage, "org/odd_shape", odd)
    out = storage / "org/never"

    def refused(model, rank=8, match=None):
        with pytest.raises(ValueError, match=match):
            asyncio.run(LoraExtraction(model, "org/base", rank, out, storage, engine=engine).extract(device))
        assert not out.exists()
        res = run_cli(extract_args(tmp_path, model, "org/never", device, rank=rank))
        assert res.exit_code != 0 and not out.exists()
    refused("org/lora", match="adapter directory")
    refused("org/odd_dtype", match="lm_head.weight")
    refused("org/odd_shape", match="model.norm.weight")
    refused("org/ft1", rank=0, match="rank")
    refused("org/ft1", rank=257, match="rank")
    monkeypatch.setenv("WORLD_SIZE", "2")
    refused("org/ft1", match="single process")
    monkeypatch.delenv("WORLD_SIZE")
    lf.write_model(storage, "org/same", lf.model_tensors(0))
    refused("org/same", match="nothing to write")
    refused("org/base", match="both org/base")
