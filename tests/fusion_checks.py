"""Checks of the pairwise fusion operators shared by the emulator tier (tests/test_fusion_host.py) and the GPU tier
(tests/test_fusion_gpu.py): Engine.fusion_merge and Engine.fusion_fn against tests/fusion_oracle.py, BIT FOR BIT - sm_exp,
sm_log, the row KLs, the quartiles, the threshold, the counts, the gated delta and the output.  The tolerance is zero and
it is derived, not measured: every step of the function is one correctly rounded operation, an exact order statistic or
an integer count in a stated order (include/shardmerge_hip.h, smhip_fusion_merge).  Two checks do not go through the
oracle: the accuracy of the two functions against math.exp / math.log, and the row KL against torch's fp64 log_softmax."""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

from tests import fusion_oracle as fo
from tests.harness import DTYPES, expected_by_tensor, f32_bits, raw

COLS = (1, 7, 8, 9, 2047, 2048, 2049, 4096, 28672)       # 2047..2049: around one full round of 256 lanes x 8
ROWS = (1, 3, 257)
SHAPE = (37, 129)                                         # unaligned rows and a tail octet
FN_TOL = 2.0 ** -50                                       # the issue's cap on the relative error of sm_exp / sm_log


def fusion_inputs(shape, in_dtype=torch.bfloat16, bo_dtype=None, seed=0, sigma=1e-3, own_out=False, device="cpu"):
    """(finetune, base, base_out): a base N(0, 0.02^2), a delta N(0, (sigma * u_r)^2) with a scale u_r per row of the last
    dimension, log-uniform in [0.5, 2] (so that the row KLs differ), all rounded to their dtype"""
    g = torch.Generator(device=device).manual_seed(2000 + seed)
    rn = lambda s: torch.randn(shape, generator=g, device=device, dtype=torch.float32) * s
    bo_dtype = bo_dtype or in_dtype
    base = rn(0.02)
    scale = 0.5 * 4.0 ** torch.rand(tuple(shape[:-1]) + (1,), generator=g, device=device, dtype=torch.float32)
    ft = (base + rn(sigma) * scale).to(in_dtype)
    base = base.to(in_dtype)
    base_out = rn(0.02).to(bo_dtype) if own_out or bo_dtype != in_dtype else base
    return ft, base, base_out


def check(engine, ft, base, base_out, mode="arcee", iqr_mult=1.5, t=None, sane=True, label=""):
    """one call against the oracle, bit for bit; sane (ARCEE): the oracle's result must select something, not everything,
    and have Q3 > Q1 - so that no case passes by selecting nothing.  Returns (report, out, delta, the oracle's dict)"""
    out, rep, delta = engine.fusion_merge(ft, base, base_out, mode=mode, iqr_mult=iqr_mult, t=t, want_delta=True, want_kl=True)
    ref = fo.fusion_merge(ft.cpu(), base.cpu(), base_out.cpu(), mode, iqr_mult=iqr_mult, t=t)
    n = base_out.numel()
    assert out.dtype == base_out.dtype and out.shape == base_out.shape and rep.n == n and rep.mode == mode, label
    if mode == "arcee":
        print(f"{label}: selected {rep.selected} / {ref['selected']} of {n}, quartiles {rep.q1:.4g} {rep.q2:.4g} {rep.q3:.4g}, "
              f"thr {rep.threshold:.4g}, kl {rep.kl_min:.4g} .. {rep.kl_max:.4g}")
        if sane:
            assert 0 < ref["selected"] < n and ref["q3"] > ref["q1"], (label, ref["selected"], n, ref["q1"], ref["q3"])
        kl = rep.kl.cpu().numpy()
        bad = int((kl.view(np.uint32) != ref["kappa"].view(np.uint32)).sum())
        assert bad == 0, f"{label}: {bad} of {kl.size} row KLs differ in their bits"
        for key in ("q1", "q2", "q3", "threshold"):
            assert f32_bits(getattr(rep, key)) == f32_bits(ref[key]), (label, key, getattr(rep, key), ref[key])
        assert rep.selected == ref["selected"], (label, rep.selected, ref["selected"])
        if n:
            assert f32_bits(rep.kl_min) == f32_bits(float(ref["kappa"].min())) and f32_bits(rep.kl_max) == f32_bits(float(ref["kappa"].max())), label
    else:
        print(f"{label}: clipped {rep.clipped} / {ref['clipped']} of {n}")
        assert rep.clipped == ref["clipped"], (label, rep.clipped, ref["clipped"])
    bad = int((raw(delta) != raw(ref["delta"])).sum())
    assert bad == 0, f"{label}: {bad} of {n} gated-delta values differ in their bits"
    bad = int((raw(out) != raw(ref["out"])).sum())
    assert bad == 0, f"{label}: {bad} of {n} output values differ in their bits"
    return rep, out, delta, ref


# ---- sm_exp / sm_log ------------------------------------------------------------------------------------------------------
def exp_grid():
    """0, -2^-60, +-1 ulp around every multiple of ln 2 / 2 down to the cutoff, the cutoff and its neighbours, 10^5 random
    points in [-40, 0]"""
    pts = [0.0, -0.0, -2.0 ** -60, fo.EXP_CUTOFF, np.nextafter(fo.EXP_CUTOFF, 0.0), np.nextafter(fo.EXP_CUTOFF, -100.0), -80.0, -1e300]
    j = 1
    while -j * math.log(2.0) / 2 >= fo.EXP_CUTOFF:
        v = -j * math.log(2.0) / 2
        pts += [v, np.nextafter(v, 0.0), np.nextafter(v, -100.0)]
        j += 1
    rnd = -40.0 * np.random.default_rng(1234).random(100000)
    return np.concatenate([np.array(pts, dtype=np.float64), rnd])


def log_grid():
    """1, 1 + 2^-52, powers of two +- 1 ulp (inside [1, 2^40)), around sqrt 2, 10^5 random points in [1, 2^17]"""
    pts = [1.0, 1.0 + 2.0 ** -52, fo.SQRT2, np.nextafter(fo.SQRT2, 0.0), np.nextafter(fo.SQRT2, 4.0)]
    for e in range(1, 40):
        pts += [2.0 ** e, np.nextafter(2.0 ** e, 0.0), np.nextafter(2.0 ** e, 2.0 ** 41)]
    pts.append(np.nextafter(2.0 ** 40, 0.0))
    rnd = 1.0 + (2.0 ** 17 - 1.0) * np.random.default_rng(4321).random(100000)
    return np.concatenate([np.array(pts, dtype=np.float64), rnd])


def check_functions(engine, device="cpu"):
    """the device (or the emulator's kernel) and the host against the oracle, bit for bit; the accuracy against libm"""
    for op, grid, oracle, exact in (("exp", exp_grid(), fo.sm_exp, math.exp), ("log", log_grid(), fo.sm_log, math.log)):
        want = oracle(grid)
        for on_device in (True, False):
            got = engine.fusion_fn(op, torch.from_numpy(grid), on_device=on_device).numpy()
            bad = int((got.view(np.uint64) != want.view(np.uint64)).sum())
            assert bad == 0, f"sm_{op} (on_device={on_device}): {bad} of {grid.size} values differ from the oracle in their bits"
        ref = np.array([exact(float(v)) for v in grid])
        live = (grid >= fo.EXP_CUTOFF) if op == "exp" else (ref > 0)
        rel = float(np.max(np.abs(want[live] - ref[live]) / ref[live]))
        print(f"sm_{op}: largest relative error against math.{op} on {int(live.sum())} points: {rel:.3e} = 2^{math.log2(rel):.2f}")
        assert rel <= FN_TOL, (op, rel)
        if op == "exp":
            assert want[0] == 1.0 and np.all(want[grid < fo.EXP_CUTOFF] == 0.0) and want[3] > 0.0
        else:
            assert want[0] == 0.0 and not np.signbit(want[0])


# ---- the row KL and the whole call ------------------------------------------------------------------------------------------
def check_shape(engine, C, R, device="cpu"):
    """ARCEE and NEARSWAP on R x C: kl_out, quartiles, threshold, counts, delta and output, bit for bit.  C = 1 gives
    kappa = 0 everywhere (a softmax over one element): no sanity condition there"""
    small = R * C < 512
    ft, base, bo = fusion_inputs((R, C), seed=C % 97 + R, sigma=1e-3 if small or (C + R) % 2 else 1e-4, device=device)
    if small and C > 1:
        ft[R - 1, C // 2] += 0.05                      # a handful of scores has no outlier of its own: plant one
    sane = C > 1
    rep, _, _, ref = check(engine, ft, base, bo, "arcee", sane=sane, label=f"arcee {R}x{C}")
    if C == 1:
        assert rep.selected == 0 and rep.kl_max == 0.0
    check(engine, ft, base, bo, "nearswap", t=5e-4, label=f"nearswap {R}x{C}")


def check_dtypes(engine, in_dtype, bo_dtype, device="cpu"):
    ft, base, bo = fusion_inputs(SHAPE, in_dtype, bo_dtype, seed=11, own_out=True, device=device)
    check(engine, ft, base, bo, "arcee", label=f"arcee {in_dtype}->{bo_dtype}")
    check(engine, ft, base, bo, "nearswap", t=1e-3, label=f"nearswap {in_dtype}->{bo_dtype}")
    ft, base, bo = fusion_inputs(SHAPE, in_dtype, bo_dtype, seed=12, device=device)        # base_out is the base where the dtypes agree
    check(engine, ft, base, bo, "arcee", iqr_mult=0.5, label=f"arcee {in_dtype}->{bo_dtype} shared")


def check_tiny(engine, device="cpu"):
    for n in (1, 2, 4):
        ft, base, bo = fusion_inputs((n,), seed=30 + n, device=device)
        check(engine, ft, base, bo, "arcee", sane=False, label=f"arcee n={n}")
        check(engine, ft, base, bo, "nearswap", t=1e-3, label=f"nearswap n={n}")
    ft, base, bo = fusion_inputs((0,), seed=35, device=device)
    out, rep = engine.fusion_merge(ft, base, bo, mode="arcee")
    assert out.numel() == 0 and rep.selected == 0
    ft, base, bo = fusion_inputs((4, 33, 65), seed=36, own_out=True, device=device)          # rank 3: rows of the last dimension
    check(engine, ft, base, bo, "arcee", label="arcee rank 3")
    check(engine, ft, base, bo, "nearswap", t=1e-3, label="nearswap rank 3")


def check_unaligned(engine, device="cpu"):
    """views offset by one element: the element-wise path of the loader and the store"""
    for dtype in DTYPES:
        for R, C in ((1, 1003), (8, 256), (5, 129)):
            n = R * C
            ft, base, bo = fusion_inputs((n + 5,), dtype, seed=71, own_out=True, device=device)
            cut = lambda t, o: t[o:o + n].view(R, C)
            # (the row scale of fusion_inputs is per flat tensor here: scale the rows by hand)
            f = cut(ft, 1).float()
            b = cut(base, 3).float()
            f = (b + (f - b) * 0.03 * torch.linspace(0.5, 2.0, R, device=f.device).view(R, 1)).to(dtype)
            ftv = torch.empty(n + 1, dtype=dtype, device=f.device)[1:].view(R, C)
            ftv.copy_(f)
            check(engine, ftv, cut(base, 3), cut(bo, 1), "arcee", sane=R > 1, label=f"arcee unaligned {dtype} {R}x{C}")
            check(engine, ftv, cut(base, 3), cut(bo, 1), "nearswap", t=1e-3, label=f"nearswap unaligned {dtype} {R}x{C}")


def check_tied_deltas(engine, device="cpu"):
    """heavily tied bf16 deltas: differences of bf16 weights collide, whole runs of scores are equal"""
    ft, base, bo = fusion_inputs((64, 512), seed=65, sigma=1e-4, device=device)
    rep, _, _, ref = check(engine, ft, base, bo, "arcee", label="tied deltas")
    d = (ft.float() - base.float()).cpu()
    assert d.unique().numel() < d.numel() // 20
    check(engine, ft, base, bo, "nearswap", t=float(d.abs().median()), label="tied deltas, t at a tie")


def check_mostly_zero(engine, device="cpu"):
    """more than three quarters of the deltas zero: Q1 = Q2 = Q3 = thr = 0 and exactly the nonzero scores are selected"""
    ft, base, bo = fusion_inputs((64, 300), seed=66, device=device)
    keep = torch.rand(ft.shape, generator=torch.Generator().manual_seed(5)).to(ft.device) < 0.2
    ft = torch.where(keep, ft, base)
    rep, _, delta, ref = check(engine, ft, base, bo, "arcee", sane=False, label="mostly zero")
    assert (rep.q1, rep.q2, rep.q3, rep.threshold) == (0.0, 0.0, 0.0, 0.0)
    nz = int(((ft.float() - base.float()).cpu() != 0).sum())
    assert 0 < rep.selected == nz == int((delta.cpu() != 0).sum())


def check_identical(engine, device="cpu"):
    """finetune == base: every kappa is 0 EXACTLY, nothing is selected, out is base_out's bytes"""
    for in_dtype, bo_dtype in ((torch.bfloat16, torch.bfloat16), (torch.float32, torch.bfloat16)):
        ft, base, bo = fusion_inputs(SHAPE, in_dtype, bo_dtype, seed=67, own_out=True, device=device)
        rep, out, delta, _ = check(engine, base.clone(), base, bo, "arcee", sane=False, label="identical")
        assert rep.selected == 0 and rep.kl_max == 0.0 and rep.kl_min == 0.0 and not bool(rep.kl.any())
        assert torch.equal(raw(out), raw(bo)) and not bool(delta.any())
    # one row identical among others
    ft, base, bo = fusion_inputs(SHAPE, seed=68, device=device)
    ft[5] = base[5]
    rep, _, _, _ = check(engine, ft, base, bo, "arcee", label="one identical row")
    assert float(rep.kl[5]) == 0.0 and rep.kl_min == 0.0 < rep.kl_max


def check_outliers(engine, device="cpu"):
    """one outlier delta; a row with one weight 80 above the rest (the other terms fall below the exp cutoff)"""
    ft, base, bo = fusion_inputs(SHAPE, torch.float32, seed=69, device=device)
    ft[3, 7] += 0.5
    rep, _, delta, _ = check(engine, ft, base, bo, "arcee", label="one outlier")
    assert float(delta[3, 7]) != 0.0
    ft, base, bo = fusion_inputs((6, 300), torch.float32, seed=70, device=device)
    base[2, 11] += 80.0
    ft[2, 11] += 80.0
    ft[4, 0] += 80.0                                   # ... and in the finetune alone: a large KL
    rep, _, _, ref = check(engine, ft, base, bo, "arcee", label="80 above the rest")
    x = ft[2].double().cpu().numpy()
    assert np.all(fo.sm_exp(x - x.max())[np.arange(300) != 11] == 0.0)      # the cutoff took every other term
    assert float(rep.kl[4]) > 5.0                       # about ln 300: the finetune's row is one spike


def check_iqr(engine, device="cpu"):
    """fusion_iqr 0; the selected sets are nested in fusion_iqr; -1e6 takes everything: dare_linear at density 1"""
    ft, base, bo = fusion_inputs(SHAPE, seed=72, own_out=True, device=device)
    rep0, _, _, ref = check(engine, ft, base, bo, "arcee", iqr_mult=0.0, label="iqr 0")
    assert f32_bits(rep0.threshold) == f32_bits(rep0.q2) and rep0.q3 > rep0.q1
    prev, prev_sel = None, None
    for iqr in (-1e6, -0.5, 0.0, 0.5, 1.5, 3.0):
        _, rep, delta = engine.fusion_merge(ft, base, bo, mode="arcee", iqr_mult=iqr, want_delta=True)
        cur = raw(delta)
        if prev is not None:
            nzm = cur != 0
            assert rep.selected <= prev_sel and torch.equal(cur[nzm], prev[nzm]), iqr
        prev, prev_sel = cur, rep.selected
    assert 0 < prev_sel < bo.numel()
    out, rep, delta = engine.fusion_merge(ft, base, bo, mode="arcee", iqr_mult=-1e6, want_delta=True)
    d_out, _, d_delta = engine.dare_merge([ft], [base], [1.0], bo, density=1.0, lam=1.0, normalize=True, sign_election=False, want_delta=True)
    assert rep.selected == bo.numel() and rep.q3 > rep.q1
    assert torch.equal(raw(out), raw(d_out)) and torch.equal(raw(delta), raw(d_delta))


def check_nearswap_identity(engine, device="cpu"):
    """t >= max |d|: nothing is clipped - dare_linear at density 1 with alpha 1; a small t clips most"""
    ft, base, bo = fusion_inputs(SHAPE, seed=73, own_out=True, device=device)
    tmax = float((ft.float() - base.float()).abs().max())
    out, rep, delta = engine.fusion_merge(ft, base, bo, mode="nearswap", t=tmax, want_delta=True)
    d_out, _, d_delta = engine.dare_merge([ft], [base], [1.0], bo, density=1.0, lam=1.0, normalize=True, sign_election=False, want_delta=True)
    assert rep.clipped == 0 and torch.equal(raw(out), raw(d_out)) and torch.equal(raw(delta), raw(d_delta))
    rep, _, delta, _ = check(engine, ft, base, bo, "nearswap", t=1e-4, label="nearswap small t")
    assert rep.clipped > bo.numel() // 2 and float(delta.abs().max()) == float(np.float32(1e-4))


def check_kl_against_log_softmax(engine, device="cpu"):
    """Independent of the oracle's formula: kl against KL(softmax(x) || softmax(y)) from torch's fp64 log_softmax, with
    the library's exp and log.  Bound per row, from the issue: (C + 128) 2^-52 (1 + max_j |a_j - b_j|) - three ordered
    sums of C terms and function errors of at most 2^-50.  The fp64 kl of the restatement (which the engine reproduces
    bit for bit through kappa, checked here too) is held to it; the engine's fp32 kappa to the bound plus half an ulp of
    its fp32 rounding (2^-24 relative)."""
    for (R, C), sigma in (((33, 129), 1e-3), ((9, 4096), 1e-4), ((3, 28672), 1e-3)):
        ft, base, bo = fusion_inputs((R, C), seed=90 + R, sigma=sigma, device=device)
        _, rep = engine.fusion_merge(ft, base, bo, mode="arcee", want_kl=True)
        kappa, kl, span = fo.row_kl(ft.float().cpu().numpy(), base.float().cpu().numpy())
        assert np.array_equal(rep.kl.cpu().numpy().view(np.uint32), kappa.view(np.uint32))
        lx = torch.log_softmax(ft.double().cpu(), dim=-1)
        ly = torch.log_softmax(base.double().cpu(), dim=-1)
        want = (lx.exp() * (lx - ly)).sum(dim=-1).numpy()
        bound = (C + 128) * 2.0 ** -52 * (1.0 + span)
        err = np.abs(kl - want)
        print(f"{R}x{C}: largest |kl - log_softmax kl| / bound = {float((err / bound).max()):.3g}, smallest kl before the clamp {kl.min():.3g}")
        assert np.all(err <= bound), (R, C, float((err / bound).max()))
        assert np.all(kl > 0.0)                         # no kl is negative before the clamp on these distributions
        got = rep.kl.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(got - np.maximum(want, 0.0)) <= bound * (1.0 + 2.0 ** -24) + np.abs(want) * 2.0 ** -24)


def check_selected_share(engine, device="cpu"):
    """Gaussian bases (sigma 0.02), bf16 deltas (sigma 1e-3 and 1e-4, row-dependent scale): the selected share at
    fusion_iqr 1.5 is 0.13 to 0.17.  (The share is a property of the scale law: with one scale for all rows the scores are
    half-normal and 5.5 % lie above median + 1.5 IQR; fusion_inputs' log-uniform [0.5, 2] is the law used throughout.)"""
    for sigma in (1e-3, 1e-4):
        ft, base, bo = fusion_inputs((96, 1024), seed=95, sigma=sigma, device=device)
        _, rep = engine.fusion_merge(ft, base, bo, mode="arcee")
        share = rep.selected / rep.n
        print(f"sigma {sigma}: selected share {share:.4f}")
        assert 0.13 <= share <= 0.17, (sigma, share)


def check_nonfinite(engine, device="cpu"):
    """NaN / Inf in the finetune, in the base, and in d only (NEARSWAP): ValueError naming the layer and the tensor; the
    context stays usable"""
    name = "model.layers.7.mlp.up_proj.weight"
    for poison in (float("nan"), float("inf"), float("-inf")):
        for which, word in ((0, "the finetune"), (1, "the base")):
            ft, base, bo = fusion_inputs(SHAPE, torch.float32, seed=80, own_out=True, device=device)
            (ft, base)[which].view(-1)[4321] = poison
            with pytest.raises(ValueError, match=re.escape(name) + ".*NaN or Inf in .*" + word):
                engine.fusion_merge(ft, base, bo, mode="arcee", layer_name=name)
            with pytest.raises(ValueError, match=re.escape(name) + ".*NaN or Inf in finetune - base"):
                engine.fusion_merge(ft, base, bo, mode="nearswap", t=1e-3, layer_name=name)
    # d only: finite fp32 weights whose difference overflows
    ft, base, bo = fusion_inputs(SHAPE, torch.float32, seed=81, own_out=True, device=device)
    ft.view(-1)[17], base.view(-1)[17] = 3e38, -3e38
    with pytest.raises(ValueError, match=re.escape(name) + ".*NaN or Inf in finetune - base"):
        engine.fusion_merge(ft, base, bo, mode="nearswap", t=1e-3, layer_name=name)
    ft, base, bo = fusion_inputs(SHAPE, seed=82, device=device)
    check(engine, ft, base, bo, "arcee", label="after an error")


def check_arguments(engine, device="cpu"):
    ft, base, bo = fusion_inputs((8, 8), seed=91, device=device)
    for bad in (0.0, -1e-3, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="nearswap needs t > 0"):
            engine.fusion_merge(ft, base, bo, mode="nearswap", t=bad)
    with pytest.raises(ValueError, match="iqr_mult"):
        engine.fusion_merge(ft, base, bo, mode="arcee", iqr_mult=float("nan"))
    with pytest.raises(ValueError, match="mode"):
        engine.fusion_merge(ft, base, bo, mode="swap")
    with pytest.raises(ValueError, match="shape mismatch"):
        engine.fusion_merge(ft[:4], base, bo, mode="arcee")


def check_determinism(engine, device="cpu"):
    ft, base, bo = fusion_inputs((300, 500), seed=92, own_out=True, device=device)
    a, ra = engine.fusion_merge(ft, base, bo, mode="arcee")
    b, rb = engine.fusion_merge(ft, base, bo, mode="arcee")
    assert torch.equal(raw(a), raw(b)) and ra == rb


CORNERS = [check_tiny, check_unaligned, check_tied_deltas, check_mostly_zero, check_identical, check_outliers, check_iqr,
           check_nearswap_identity, check_kl_against_log_softmax, check_selected_share, check_nonfinite, check_arguments,
           check_determinism]


# ---- profile names and launches ----------------------------------------------------------------------------
PROFILES = [("arcee", {"fusion_rowkl": 1, "fusion_hist": 3, "fusion_select": 3, "fusion_merge": 1}), ("nearswap", {"fusion_merge": 1})]


def check_profile(engine, mode, expected, shape=(40, 50), device="cpu"):
    ft, base, bo = fusion_inputs(shape, seed=6, device=device)
    engine.ctx.profile(True)
    engine.ctx.profile_reset()
    try:
        engine.fusion_merge(ft, base, bo, mode=mode, t=1e-3)
        table = engine.ctx.profile_table()
    finally:
        engine.ctx.profile(False)
    assert {n: table[n][0] for n in table} == expected, table


# ---- the C ABI ------------------------------------------------------------------------------------------------
def check_c_abi(engine, device="cpu"):
    from shardmerge_amd import _lib
    x = torch.zeros(64, dtype=torch.bfloat16, device=device)
    y = torch.zeros(64, dtype=torch.bfloat16, device=device)
    out = torch.zeros(64, dtype=torch.bfloat16, device=device)
    kl = torch.zeros(8, dtype=torch.float32, device=device)
    dll, h = engine.lib.dll, engine.ctx.h

    def call(k=1, mode=_lib.FUSION_NEARSWAP, t=1e-3, iqr=1.5, rows=8, n=64, out_t=out, in_dtype=_lib.BF16, ft=x, base=y, bo=y, kl_out=None):
        d = _lib.FusionDesc()
        d.k = k
        d.finetune[0], d.base[0], d.alpha[0] = (ft.data_ptr() if ft is not None else None), (base.data_ptr() if base is not None else None), 1.0
        d.in_dtype, d.base_out, d.base_out_dtype, d.n = in_dtype, (bo.data_ptr() if bo is not None else None), _lib.BF16, n
        d.mode, d.rows, d.iqr_mult, d.t, d.kl_out = mode, rows, iqr, t, kl_out
        rep = _lib.FusionReport()
        rc = dll.smhip_fusion_merge(h, C.byref(d), out_t.data_ptr() if out_t is not None else None, None, C.byref(rep), None)
        return rc, dll.smhip_last_error(h).decode(), rep

    rc, msg, rep = call()
    assert rc == _lib.OK and rep.clipped == 0, msg
    rc, msg, rep = call(mode=_lib.FUSION_ARCEE, kl_out=kl.data_ptr())
    assert rc == _lib.OK and rep.selected == 0 and rep.threshold == 0.0, msg
    for kwargs, word in (({"t": 0.0}, "t must be"), ({"t": -1.0}, "t must be"), ({"t": float("nan")}, "t must be"),
                         ({"t": float("inf")}, "t must be"), ({"t": 1e-60}, "t must be"), ({"rows": 7}, "rows must divide n"),
                         ({"rows": 0}, "rows must divide n"), ({"k": 2}, "k must be 1"), ({"k": 0}, "k out of range"), ({"mode": 2}, "bad mode"),
                         ({"mode": _lib.FUSION_ARCEE, "iqr": float("nan")}, "iqr_mult"), ({"ft": None}, "null"), ({"base": None}, "null"),
                         ({"bo": None}, "null"), ({"out_t": None}, "null"), ({"out_t": x}, "overlaps"), ({"in_dtype": 3}, "dtype"),
                         ({"mode": _lib.FUSION_ARCEE, "kl_out": out.data_ptr()}, "kl_out")):
        rc, msg, _ = call(**kwargs)
        assert rc == _lib.ERR_ARG and word in msg, (kwargs, rc, msg)
    rc = dll.smhip_fusion_merge(h, None, out.data_ptr(), None, None, None)
    assert rc == _lib.ERR_ARG and "null descriptor" in dll.smhip_last_error(h).decode()
    assert call(n=0, out_t=x)[0] == _lib.OK                     # a no-op, whatever the pointers
    assert dll.smhip_fusion_fn(h, 2, None, None, 0, 0, None) == _lib.ERR_ARG


# ---- the CLI on the synthetic on-disk model of tests/lora_fixtures.py ----------------------------------------
def options(operator):
    return {"operator": operator, "fusion_iqr": 1.0} if operator == "arcee_fusion" else {"operator": operator, "nearswap_t": 2e-3}


def models(second):
    """two entries on disjoint windows: ft1 fuses into layer 0, `second` (an adapter or its checkpoint) into layer 1"""
    return [{"model": "org/ft1", "base": "org/base", "is_input": True, "end_layer": 0},
            {"model": second, "base": "org/base", "is_output": True, "start_layer": 1}]


def expected_outputs(base, full, opts):
    """the oracle tensor by tensor (block tensors) / the provider's tensor (passthrough) for models()"""
    mode = "arcee" if opts["operator"] == "arcee_fusion" else "nearswap"
    def merge(fts, bases, alphas, base_out, name):
        return fo.fusion_merge(
            fts[0], bases[0], base_out, mode, iqr_mult=opts.get("fusion_iqr", 1.5), t=opts.get("nearswap_t"))["out"]

    return expected_by_tensor(base, full, models("org/lora_full"), merge)
