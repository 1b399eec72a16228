"""Checks of operator tsv shared by the emulator tier (tests/test_tsv_host.py) and the GPU tier (tests/test_tsv_gpu.py):
`tsv_apply` through smhip_tsv_probe and Engine.tsv_merge against tests/tsv_oracle.py bit for bit (the tolerance is zero
and derived: every value is an fp32 fma chain, an fp64 sum or a one-rounding fp64 operation in a stated order), a layout
check on exact integers, the properties that define TSV against torch fp64 on the CPU, and the CLI."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

from shardmerge_amd import _lib
from shardmerge_amd.merge.dare import tensor_key
from tests import extract_checks as xc
from tests import harness
from tests import lora_fixtures as lf
from tests import tsv_oracle as to
from tests.extract_checks import bits32, bits64, host, on, pair
from tests.harness import run_cli, ties_models

APPLY_SHAPES = ((1, 1), (3, 5), (17, 33), (130, 257), (257, 130))
APPLY_WIDTHS = (16, 32, 80, 256)
DTYPES = xc.DTYPES
MERGE_SHAPES = ((192, 320), (320, 192))
MERGE_KS = ((1, False), (2, False), (2, True), (3, False), (3, True), (5, False))     # (k, every finetune over its own base)
MERGE_K_IDS = [f"k{k}-{'own_bases' if own else 'shared_base'}" for k, own in MERGE_KS]
KEY = 0x0123456789ABCDEF
ALPHAS = (1.0, 0.5, 0.75, 0.3, 0.6)


def raw(t):
    return host(t).contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- 1. tsv_apply --------------------------------------------------------------------------------------------------
def apply_inputs(rows, cols, Rp, dtype, offset=0, special=False, seed=0):
    g = torch.Generator().manual_seed(1000 + 7 * rows + 3 * cols + Rp + seed)
    flat = lambda n, scale=1.0: (torch.randn(n + offset, generator=g) * scale)
    B, W = flat(rows * Rp), flat(cols * Rp)
    base = flat(rows * cols).to(dtype)
    if special:                                                    # zeros, a denormal, -0
        B[offset::3] = 0.0
        W[offset + 1::5] = -0.0
        B[offset] = 1e-41
        W[offset] = -1e-40
        base[offset::4] = -0.0
    return B[offset:].view(rows, Rp), W[offset:].view(cols, Rp), base[offset:].view(rows, cols)


def check_apply(engine, rows, cols, Rp, dtype, offset=0, special=False, lam=0.7):
    B, W, base = apply_inputs(rows, cols, Rp, dtype, offset, special)
    out, merged = engine.tsv_probe(on(engine, B), on(engine, W), on(engine, base), lam)
    ref_out, ref_merged = to.apply(B.numpy(), W.numpy(), base, lam)
    label = (rows, cols, Rp, str(dtype), offset, special)
    assert np.array_equal(bits32(host(merged).numpy()), bits32(ref_merged)), (label, "merged")
    assert out.dtype == dtype and torch.equal(raw(out), raw(ref_out)), (label, "out")
    out2, merged2 = engine.tsv_probe(on(engine, B), on(engine, W), on(engine, base), lam)
    assert torch.equal(raw(out), raw(out2)) and torch.equal(raw(merged), raw(merged2)), "two calls differ"


def check_apply_integers(engine, rows, cols, Rp):
    """independent of the oracle: small integers, every sum exact in any order; B and W differ, so a transposed or
    permuted operand or output shows"""
    g = torch.Generator().manual_seed(rows + cols)
    B = torch.randint(-3, 4, (rows, Rp), generator=g)
    W = torch.randint(-2, 6, (cols, Rp), generator=g)
    base = torch.randint(-4, 5, (rows, cols), generator=g)
    out, merged = engine.tsv_probe(on(engine, B.float()), on(engine, W.float()), on(engine, base.float()), 2.0)
    ref = B.to(torch.int64) @ W.to(torch.int64).T
    assert torch.equal(host(merged).to(torch.int64), ref), (rows, cols, Rp)
    assert torch.equal(host(out).to(torch.int64), base + 2 * ref), (rows, cols, Rp)


def check_apply_empty_panel(engine):
    """Rp = 0: merged is +0, out is base_out"""
    base = torch.randn(5, 9, generator=torch.Generator().manual_seed(3)).bfloat16()
    empty = torch.zeros(16)[:0]
    out, merged = engine.tsv_probe(on(engine, empty.view(5, 0)), on(engine, empty.view(9, 0)), on(engine, base), 1.0)
    assert torch.equal(raw(out), raw(base)) and not host(merged).view(torch.int32).any()


# ---- 2. the whole function ----------------------------------------------------------------------------------------
def merge_inputs(rows, cols, k, own=False, seed=0, dtype=torch.bfloat16, scale=0.02):
    """k finetunes whose deltas have a decaying spectrum (rank 24 plus noise), over a shared base or their own"""
    g = torch.Generator().manual_seed(77 * rows + k + seed)
    fts, bases = [], []
    shared = torch.randn(rows, cols, generator=g).to(dtype)
    for i in range(k):
        base = torch.randn(rows, cols, generator=g).to(dtype) if own else shared
        d = (torch.randn(rows, 24, generator=g) / torch.arange(1, 25) ** 0.5) @ torch.randn(24, cols, generator=g) / 24 ** 0.5
        d = scale * (d + 0.05 * torch.randn(rows, cols, generator=g))
        fts.append((base.float() + d).to(dtype))
        bases.append(base)
    return fts, bases


def assert_merge_equals(out, rep, delta, ref, label):
    assert torch.equal(raw(out), raw(ref["out"])), (label, "out")
    assert np.array_equal(bits32(host(delta).numpy()), bits32(ref["merged"])), (label, "delta_out")
    got = (rep.width, rep.r, rep.R, rep.Rp, rep.rho, rep.orth_ranks, rep.kept_U, rep.kept_W)
    want = (ref["L"], ref["r"], ref["R"], ref["Rp"], ref["rho"], ref["orth_ranks"], ref["kept_U"], ref["kept_W"])
    assert got == want, (label, got, want)
    for name, a, b in (("sigma", rep.sigma, ref["sigma"]), ("delta_sq", rep.delta_sq, ref["delta_sq"]), ("share", rep.share, ref["share"]),
                       ("mu_U", rep.mu_U, ref["mu_U"]), ("mu_W", rep.mu_W, ref["mu_W"])):
        assert bits64(np.array(a, dtype=np.float64).reshape(-1)).tolist() == bits64(np.array(b, dtype=np.float64).reshape(-1)).tolist(), (label, name)


@functools.lru_cache(maxsize=None)
def merge_case(rows, cols, k, r, q, own=False, variant="", base_out_dtype=torch.bfloat16):
    """inputs and the oracle's result, computed once per process.  variant: "zero_alpha" (entry 1 has alpha 0),
    "identical" (entry 1 is entry 0), "equal_base" (entry 1 is its base: rho = 0)"""
    fts, bases = merge_inputs(rows, cols, k, own)
    alphas = list(ALPHAS[:k])
    if variant == "zero_alpha":
        alphas[1] = 0.0
    if variant == "identical":
        fts[1], bases[1] = fts[0], bases[0]
    if variant == "equal_base":
        fts[1] = bases[1]
    base_out = bases[0].to(base_out_dtype)
    lam = 0.7
    ref = to.merge(fts, bases, alphas, base_out, r, q, lam, KEY)
    return fts, bases, alphas, base_out, lam, ref


def check_merge(engine, rows, cols, k, r, q, own=False, variant="", base_out_dtype=torch.bfloat16):
    fts, bases, alphas, base_out, lam, ref = merge_case(rows, cols, k, r, q, own, variant, base_out_dtype)
    same = {}
    dev = lambda t: same.setdefault(id(t), on(engine, t))          # a shared base stays ONE tensor
    args = ([dev(t) for t in fts], [dev(t) for t in bases], alphas, dev(base_out))
    kw = dict(rank=r, power_iters=q, lam=lam, key=KEY, want_delta=True, layer_name="layers.0.w")
    out, rep, delta = engine.tsv_merge(*args, **kw)
    label = f"{rows}x{cols} k={k} r={r} q={q} own={own} {variant}"
    print(f"{label}: R {rep.R} Rp {rep.Rp} rho {rep.rho} kept {rep.kept_U}/{rep.kept_W} share {[round(s, 4) for s in rep.share]}")
    assert_merge_equals(out, rep, delta, ref, label)
    out2, rep2, delta2 = engine.tsv_merge(*args, **kw)
    assert torch.equal(raw(out), raw(out2)) and torch.equal(raw(delta), raw(delta2)) and rep == rep2, "two calls differ"
    return rep


def check_nonfinite(engine):
    fts, bases = merge_inputs(48, 64, 2)
    for bad in (float("nan"), float("inf"), float("-inf")):
        ft = fts[1].clone()
        ft[5, 7] = bad
        with pytest.raises(ValueError, match=r"model\.layers\.3\.q_proj\.weight.*finetune 1"):
            engine.tsv_merge([on(engine, fts[0]), on(engine, ft)], [on(engine, b) for b in bases], [1.0, 1.0], on(engine, bases[0]),
                             rank=8, layer_name="model.layers.3.q_proj.weight")
    # an inactive entry is not read: its NaN does not matter
    ft = fts[1].clone()
    ft[0, 0] = float("nan")
    out, rep = engine.tsv_merge([on(engine, fts[0]), on(engine, ft)], [on(engine, b) for b in bases], [1.0, 0.0], on(engine, bases[0]), rank=8)
    assert rep.rho == [8, 0] and torch.isfinite(host(out).float()).all()


def check_merge_against(engine, other, rows, cols, k, r, q=2):
    """the device against the emulator library (the shapes whose numpy chain takes more than a few seconds)"""
    fts, bases = merge_inputs(rows, cols, k, seed=1)
    alphas = list(ALPHAS[:k])
    kw = dict(rank=r, power_iters=q, lam=0.7, key=KEY, want_delta=True)
    out, rep, delta = engine.tsv_merge([on(engine, t) for t in fts], [on(engine, bases[0])] * k, alphas, on(engine, bases[0]), **kw)
    out2, rep2, delta2 = other.tsv_merge(fts, [bases[0]] * k, alphas, bases[0], **kw)
    print(f"{rows}x{cols} k={k} r={r}: R {rep.R}, kept {rep.kept_U}/{rep.kept_W}, share {[round(s, 4) for s in rep.share]}")
    assert torch.equal(raw(out), raw(out2)) and torch.equal(raw(delta), raw(delta2))
    assert rep == rep2 and rep.R == k * r


# ---- 3. properties, independent of the oracle ----------------------------------------------------------------------
# Tolerances.  No chain bound is known for the whitened product, so each is 4 x what the numpy restatement of the
# definition (tests/tsv_oracle.py, the function's own arithmetic) deviates from the exact-arithmetic statement on THESE
# cases, measured on the CPU (the figures are in the tests' docstrings and DESIGN.md); none comes from the HIP path.
# Measured (k = 2 / 3 / 5 where three are given; the exact-SVD fp64 form of the definition, tsv_oracle.merge_fp64, gives
# 1e-15 for all of them):
SV_TOL = 4 * 5.6e-8             # |sv_j - s_j| / s_max over the R leading singular values: 4.4e-8 / 4.3e-8 / 5.5e-8
TAIL_TOL = 4 * 5.4e-8           # sv_R / s_max: 3.0e-8 / 4.4e-8 / 5.4e-8
FRO_TOL = 4 * 3.8e-8            # | ||merged||_F^2 - sum s^2 | / sum s^2: 3.7e-8 / 4.7e-9 / 2.8e-8
DUP_TOL = 4 * 1.3e-7            # ||merged(ft, ft) - merged(ft)||_F / ||merged(ft)||_F: 1.25e-7
# ||merged(both) - (merged(0) + merged(1))||_F / ||merged(both)||_F: exactly 0 - the cross Gram is exactly zero, no Jacobi
# rotation mixes the two blocks, and every chain of the joint call is a chain of a separate one plus products of zeros
DISJOINT_TOL = 0.0
PROPERTY_SHAPE = (96, 160)


def property_inputs(k, seed=0):
    """fp32 deltas over a zero base (the inputs ARE the deltas, as in extract_checks.quality_inputs)"""
    rows, cols = PROPERTY_SHAPE
    g = torch.Generator().manual_seed(4000 + k + seed)
    fts = []
    for i in range(k):
        d = (torch.randn(rows, 12, generator=g) / torch.arange(1, 13) ** 0.5) @ torch.randn(12, cols, generator=g) / 12 ** 0.5
        fts.append(0.02 * (d + 0.05 * torch.randn(rows, cols, generator=g)))
    return fts, [torch.zeros(rows, cols)] * k


def tsv_delta(engine, fts, bases, alphas, r=8, q=2):
    same = {}
    dev = lambda t: same.setdefault(id(t), on(engine, t))
    out, rep, delta = engine.tsv_merge([dev(t) for t in fts], [dev(t) for t in bases], alphas, dev(bases[0]), rank=r, power_iters=q,
                                       key=KEY, want_delta=True)
    return host(delta).double(), rep


def singular_value_figures(merged, s):
    """(largest |sv_j - s_j| / s_max over j < R, sv_R / s_max, | ||merged||_F^2 - sum s^2 | / sum s^2)"""
    sv = torch.linalg.svdvals(merged)
    s = torch.sort(torch.tensor(s, dtype=torch.float64), descending=True).values
    R = len(s)
    return (float((sv[:R] - s).abs().max() / s[0]), float(sv[R] / s[0]),
            float(((merged ** 2).sum() - (s ** 2).sum()).abs() / (s ** 2).sum()))


def check_singular_values(engine, k):
    fts, bases = property_inputs(k)
    alphas = list(ALPHAS[:k])
    merged, rep = tsv_delta(engine, fts, bases, alphas)
    s = [a * x for a, sig, rho in zip(alphas, rep.sigma, rep.rho) for x in sig[:rho]]
    dev, tail, fro = singular_value_figures(merged, s)
    print(f"singular values k={k}: R {rep.R}, deviation {dev:.2e} (tol {SV_TOL:.1e}), next {tail:.2e} (tol {TAIL_TOL:.1e}), "
          f"Frobenius {fro:.2e} (tol {FRO_TOL:.1e})")
    assert rep.R == 8 * k == rep.kept_U == rep.kept_W
    assert dev <= SV_TOL and tail <= TAIL_TOL and fro <= FRO_TOL, (k, dev, tail, fro)


def check_duplicates(engine):
    fts, bases = property_inputs(1)
    both, rep = tsv_delta(engine, [fts[0], fts[0]], [bases[0], bases[0]], [1.0, 1.0])
    one, rep1 = tsv_delta(engine, fts, bases, [1.0])
    rel = float(torch.linalg.norm(both - one) / torch.linalg.norm(one))
    task_arithmetic = float(torch.linalg.norm(2 * one - one) / torch.linalg.norm(one))
    print(f"duplicates: relative difference {rel:.2e} (tol {DUP_TOL:.1e}; task arithmetic gives {task_arithmetic:.1f})")
    assert rep.R == 16 and rep.kept_U == rep.kept_W == rep.R // 2 == rep1.R
    assert rel <= DUP_TOL, rel


def check_disjoint_supports(engine):
    """block-diagonal deltas: the cross Gram is exactly zero and the merge is the sum of the separate k = 1 results"""
    rows, cols = PROPERTY_SHAPE
    fts, bases = property_inputs(2, seed=9)
    fts[0][rows // 2:, :] = 0
    fts[0][:, cols // 2:] = 0
    fts[1][:rows // 2, :] = 0
    fts[1][:, :cols // 2] = 0
    both, rep = tsv_delta(engine, fts, bases, [1.0, 0.5])
    a, _ = tsv_delta(engine, fts[:1], bases[:1], [1.0])
    b, _ = tsv_delta(engine, fts[1:], bases[1:], [0.5])
    assert not a[rows // 2:].any() and not a[:, cols // 2:].any() and not b[:rows // 2].any() and not b[:, :cols // 2].any()
    rel = float(torch.linalg.norm(both - (a + b)) / torch.linalg.norm(both))
    print(f"disjoint supports: relative difference {rel:.2e} (tol {DISJOINT_TOL:.1e})")
    assert rep.R == 16 == rep.kept_U == rep.kept_W
    assert rel <= DISJOINT_TOL, rel


def check_truncation(engine, which, rank):
    """k = 1: the rank-r truncation, as good as smhip_lora_extract's (the same margin over the fp64 SVD)"""
    ft, base, D, sv = xc.quality_inputs()[which]
    out, rep, delta = engine.tsv_merge([on(engine, ft)], [on(engine, base)], [1.0], on(engine, base), rank=rank, power_iters=2,
                                       key=tensor_key(0, which), want_delta=True)
    err = torch.linalg.norm(D - host(delta).double())
    best = torch.sqrt((sv[rank:] ** 2).sum())
    ratio = float(err / best)
    print(f"truncation {which} r={rank}: ||D - merged|| / ||D - D_r|| = {ratio:.5f}, share {rep.share[0]:.6f}")
    assert ratio <= 1.02, (which, rank, ratio)
    return ratio


# ---- 4. the C ABI and the engine's argument checks -----------------------------------------------------------------
def check_c_abi(engine):
    fts, bases = merge_inputs(32, 48, 2)
    ft, base = on(engine, fts[0]), on(engine, bases[0])
    out = torch.empty_like(base)
    dll, h = engine.lib.dll, engine.ctx.h
    need = int(dll.smhip_tsv_workspace(32, 48, 2, 8))
    assert need > 0 and dll.smhip_tsv_workspace(32, 48, 2, 0) == 0 and dll.smhip_tsv_workspace(32, 48, 2, 257) == 0
    assert dll.smhip_tsv_workspace(0, 48, 2, 8) == 0 and dll.smhip_tsv_workspace(32, 48, 17, 8) == 0
    ws = engine._xl_workspace(need)

    def call(k=2, alpha=1.0, out_t=out, **over):
        d = _lib.TsvDesc()
        d.k = k
        for i in range(max(0, min(k, 16))):
            d.finetune[i], d.base[i], d.alpha[i] = ft.data_ptr(), base.data_ptr(), alpha
        f = dict(in_dtype=_lib.BF16, base_out=base.data_ptr(), base_out_dtype=_lib.BF16, n=32 * 48, rows=32, cols=48, rank=8,
                 power_iters=1, lam=1.0, key=1, workspace=ws.data_ptr(), workspace_bytes=need)
        f.update(over)
        for key, value in f.items():
            setattr(d, key, value)
        rep = _lib.TsvReport()
        rc = dll.smhip_tsv_merge(h, C.byref(d), out_t.data_ptr(), None, C.byref(rep), engine._stream())
        return rc, dll.smhip_last_error(h).decode(), rep

    rc, msg, rep = call()
    assert rc == _lib.OK and (rep.L, rep.r, rep.R, rep.Rp) == (16, 8, 16, 16) and rep.kept_U == 8, msg
    for kwargs, word in (({"k": 0}, "k out of range"), ({"k": 17}, "k out of range"), ({"alpha": -0.5}, "negative"),
                         ({"alpha": float("nan")}, "alpha"), ({"lam": float("inf")}, "lambda"), ({"rank": 0}, "rank"),
                         ({"rank": 257}, "rank"), ({"power_iters": 5}, "power_iters"), ({"power_iters": -1}, "power_iters"),
                         ({"k": 9, "rank": 32}, "exceeds 256"), ({"rows": 0}, "rows"), ({"cols": 47}, "rows * cols"), ({"in_dtype": 3}, "dtype"),
                         ({"base_out_dtype": -1}, "dtype"), ({"out_t": ft}, "overlaps"), ({"workspace": None}, "workspace"),
                         ({"workspace_bytes": need - 1}, "workspace"), ({"workspace": ws.data_ptr() + 8}, "workspace"),
                         ({"base_out": None}, "null")):
        rc, msg, _ = call(**kwargs)
        assert rc == _lib.ERR_ARG and word in msg and "tsv_merge" in msg, (kwargs, rc, msg)
    assert dll.smhip_tsv_merge(h, None, out.data_ptr(), None, None, None) == _lib.ERR_ARG
    rc, msg, rep = call(n=0, out_t=ft)                              # a no-op, whatever the pointers
    assert rc == _lib.OK and rep.R == 0
    bad_probe = lambda *a: dll.smhip_tsv_probe(h, *a, engine._stream())
    assert bad_probe(ft.data_ptr(), ft.data_ptr(), 4, 4, 8, base.data_ptr(), _lib.BF16, 1.0, out.data_ptr(), None) == _lib.ERR_ARG
    assert bad_probe(ft.data_ptr(), ft.data_ptr(), 4, 4, 272, base.data_ptr(), _lib.BF16, 1.0, out.data_ptr(), None) == _lib.ERR_ARG
    assert bad_probe(None, ft.data_ptr(), 4, 4, 16, base.data_ptr(), _lib.BF16, 1.0, out.data_ptr(), None) == _lib.ERR_ARG
    for kw in (dict(rank=0), dict(rank=300), dict(rank=True), dict(power_iters=5), dict(lam=float("nan"))):
        with pytest.raises(ValueError):
            engine.tsv_merge([ft], [base], [1.0], base, **kw)
    with pytest.raises(ValueError, match="alphas"):
        engine.tsv_merge([ft], [base], [-1.0], base, rank=4)
    with pytest.raises(ValueError, match="at least two dimensions"):
        engine.tsv_merge([ft.reshape(-1)], [base.reshape(-1)], [1.0], base.reshape(-1), rank=4)
    wide = on(engine, torch.zeros(32, 300, dtype=torch.bfloat16))
    out9, rep9 = engine.tsv_merge([wide] * 9, [wide] * 9, [1.0] * 3 + [0.0] * 6, wide, rank=100, layer_name="layers.7")   # 3 x 32 <= 256
    assert rep9.r == 32 and rep9.R == 0 and not host(out9).float().any()
    with pytest.raises(ValueError, match=r"layers\.7.*9 finetunes x rank 32 = 288"):
        engine.tsv_merge([wide] * 9, [wide] * 9, [1.0] * 9, wide, rank=100, layer_name="layers.7")


def check_rank3(engine):
    """a tensor of more than two dimensions is the matrix [shape[0] x the rest]"""
    fts, bases = merge_inputs(48, 60, 2)
    view = lambda t: on(engine, t).view(48, 6, 10)
    out, rep, delta = engine.tsv_merge([view(t) for t in fts], [view(bases[0])] * 2, [1.0, 0.5], view(bases[0]), rank=8, key=KEY, want_delta=True)
    out2, rep2, delta2 = engine.tsv_merge([on(engine, t) for t in fts], [on(engine, bases[0])] * 2, [1.0, 0.5], on(engine, bases[0]), rank=8,
                                          key=KEY, want_delta=True)
    assert tuple(out.shape) == (48, 6, 10) and torch.equal(raw(out).reshape(48, 60), raw(out2)) and rep == rep2


def check_profile(engine, k, q, shape=(320, 192), r=8):
    """the profile names of the header and their launch counts"""
    fts, bases = merge_inputs(*shape, k)
    args = ([on(engine, t) for t in fts], [on(engine, bases[0])] * k, list(ALPHAS[:k]), on(engine, bases[0]))
    engine.ctx.profile(True)
    engine.ctx.profile_reset()
    try:
        engine.tsv_merge(*args, rank=r, power_iters=q, key=KEY)
        table = engine.ctx.profile_table()
    finally:
        engine.ctx.profile(False)
    mm = k * (2 * q + 2)
    want = {"xl_fill": 1, "xl_delta_mm": mm, "xl_fold": mm, "xl_gram": mm + 2, "xl_gram_fold": mm + 2,
            "xl_panel_mm": k * (2 * q + 1) + 2 * k + 1, "geo_gram": k, "geo_gram_fold": k, "tsv_apply": 1}
    assert {n: v[0] for n, v in table.items()} == want, table


# ---- 5. the CLI on the synthetic on-disk model of tests/lora_fixtures.py ------------------------------------------
OPTIONS = {"operator": "tsv", "tsv_rank": 16, "tsv_power_iters": 1, "tsv_lambda": 0.7, "seed": 5}


def write_config(root, third, out_dir, options=OPTIONS, device=None, models=None):
    return harness.write_config(root, models or ties_models(third), out_dir, options, device)


def expected_matrices(base, full, opts):
    """the oracle for the block MATRICES (1-D tensors and passthrough tensors are checked against dare_linear's run)"""
    ft1, ft2 = lf.model_tensors(1), lf.model_tensors(2)
    out = {}
    for name, shape in lf.TENSORS:
        m = re.match(r"model\.layers\.(\d+)\.", name)
        if m is None or len(shape) < 2:
            continue
        entries = [(ft1[name], base[name], 0.5), (ft2[name], ft1[name], 0.3), (full[name], base[name], 0.4)]
        if int(m.group(1)) == 1:
            del entries[1]
        out[name] = to.merge([e[0] for e in entries], [e[1] for e in entries], [e[2] for e in entries], base[name],
                             opts["tsv_rank"], opts["tsv_power_iters"], opts["tsv_lambda"], tensor_key(opts["seed"], name))["out"]
    return out


def check_cli(tmp_path, engine, device=None, third="org/lora_full"):
    """the merge equals the oracle matrix by matrix; everything else equals operator dare_linear at density 1"""
    base, factors, full = lf.setup_k3(tmp_path, engine)
    res = run_cli(write_config(tmp_path, third, "merged", device=device))
    assert res.exit_code == 0, res.output
    got = lf.read_outputs(tmp_path / "merged")
    expected = expected_matrices(base, full, OPTIONS)
    assert len(expected) == 6 and any(not torch.equal(expected[n], base[n]) for n in expected)
    for name in expected:
        assert torch.equal(raw(got[name]), raw(expected[name])), name
    linear = {"operator": "dare_linear", "density": 1.0, "dare_lambda": OPTIONS["tsv_lambda"]}
    res = run_cli(write_config(tmp_path, third, "linear", linear, device=device))
    assert res.exit_code == 0, res.output
    other = lf.read_outputs(tmp_path / "linear")
    assert sorted(other) == sorted(got)
    for name in got:
        if name not in expected:
            assert torch.equal(raw(got[name]), raw(other[name])), name
    readme = (tmp_path / "merged" / "README.md").read_text()
    for word in ("# TSV Merged Model", "TSV (", "rank 16", "power iterations 1", "lambda 0.7", "seed 5"):
        assert word in readme, (word, readme)
    return got
