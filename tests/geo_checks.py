"""Checks of the geometric operators (model_stock, nuslerp, slerp) shared by the emulator tier (tests/test_geo_host.py)
and the GPU tier (tests/test_geo_gpu.py): Engine.geo_merge against tests/geo_oracle.py, BIT FOR BIT - output, the fp32
combination, and the report's Gram, cos, t / Omega and coefficients as raw fp64 / fp32 bits.  The tolerance is zero and it
is derived, not measured: the Gram is a sum of exact products in a summation order that the header writes out, every
other step is one correctly rounded IEEE operation or the C library's acos / sin (include/shardmerge_hip.h,
smhip_geo_merge).  The Gram is ALSO held against math.fsum of the exact products, within the a-priori bound of any
summation order, so that an oracle and a kernel with the same mistake do not pass together."""
import math

import pytest
import torch

from tests import geo_oracle
from tests import harness
from tests.harness import ALPHAS, DTYPES, SMALL, expected_by_tensor, f32_bits, f64_bits, make_inputs, raw, ties_models

MODES = geo_oracle.MODES
# (mode, rowwise): the four operator variants
VARIANTS = (("model_stock", False), ("model_stock", True), ("nuslerp", False), ("slerp", False))
VARIANT_IDS = ["model_stock", "model_stock_rowwise", "nuslerp", "slerp"]


def variant_k(mode, k):
    return k if mode == "model_stock" else min(k, 2)


def check(engine, fts, bases, alphas, base_out, mode="model_stock", rowwise=False, label=""):
    """one call against the oracle, bit for bit; returns (the engine's report, the oracle's dict)"""
    out, rep, delta = engine.geo_merge(fts, bases, alphas, base_out, mode=mode, rowwise=rowwise, want_delta=True)
    cpu = lambda ts: [t.cpu() for t in ts]
    ref = geo_oracle.geo_merge(cpu(fts), cpu(bases), alphas, base_out.cpu(), mode=mode, rowwise=rowwise)
    k = len(fts)
    assert out.dtype == base_out.dtype and out.shape == base_out.shape, label
    assert rep.mode == mode and rep.rowwise == bool(rowwise)
    if base_out.numel():
        if rowwise:
            print(f"{label}: t in [{rep.t_min}, {rep.t_max}] mean {rep.t_mean} / oracle [{ref['t_min']}, {ref['t_max']}] mean {ref['t_mean']}")
            for key in ("t_min", "t_max", "t_mean"):
                assert f64_bits(getattr(rep, key)) == f64_bits(ref[key]), (label, key, getattr(rep, key), ref[key])
        else:
            print(f"{label}: cos {rep.cos} / {ref['cos']}, t {rep.t} / {ref['t']}, omega {rep.omega} / {ref['omega']}, "
                  f"c {rep.coefficients} / {ref['c']}")
            for i in range(k):
                for j in range(k):
                    assert f64_bits(rep.gram[i][j]) == f64_bits(ref["G"][i][j]), (label, "G", i, j, rep.gram[i][j], ref["G"][i][j])
            for key in ("cos", "t", "omega"):
                assert f64_bits(getattr(rep, key)) == f64_bits(ref[key]), (label, key, getattr(rep, key), ref[key])
            assert rep.linear == bool(ref["linear"]), (label, rep.linear, ref["linear"])
            assert [f32_bits(c) for c in rep.coefficients] == [f32_bits(c) for c in ref["c"]], (label, rep.coefficients, ref["c"])
    bad = int((raw(delta) != raw(ref["delta"])).sum())
    assert bad == 0, f"{label}: {bad} of {ref['delta'].numel()} values of the combination differ in their bits"
    bad = int((raw(out) != raw(ref["out"])).sum())
    assert bad == 0, f"{label}: {bad} of {ref['out'].numel()} output values differ in their bits"
    return rep, ref


# ---- the parameter grid -------------------------------------------------------------------------------
def check_dtypes(engine, in_dtype, bo_dtype, mode, rowwise, device="cpu"):
    k = variant_k(mode, 3)
    fts, bases, bo = make_inputs(SMALL, k, in_dtype, bo_dtype, seed=11, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:k], bo, mode, rowwise, label=f"{mode} {in_dtype}->{bo_dtype}")
    fts, bases, bo = make_inputs(SMALL, 2, in_dtype, bo_dtype, seed=12, device=device)      # one shared base
    check(engine, fts, bases, ALPHAS[:2], bo, mode, rowwise, label=f"{mode} {in_dtype}->{bo_dtype} shared")


def check_k(engine, k, rowwise, device="cpu"):
    """model_stock at k = 1, 2, 3, 5, 16: one tile of pairs up to k = 4, ten tiles at k = 16; own bases and a shared one"""
    for own in (False, True):
        fts, bases, bo = make_inputs(SMALL, k, seed=20 + k + own, own_bases=own, device=device)
        rep, _ = check(engine, fts, bases, ALPHAS[:k], bo, "model_stock", rowwise, label=f"model_stock k={k} rowwise={rowwise} own={own}")
        if k == 1 and not rowwise:
            assert rep.t == 1.0 and rep.coefficients == [1.0]


def check_pair_k1(engine, device="cpu"):
    """nuslerp / slerp with one entry (a layer window that leaves one): c_0 = 1"""
    fts, bases, bo = make_inputs(SMALL, 1, seed=30, own_bases=True, device=device)
    for mode in ("nuslerp", "slerp"):
        rep, _ = check(engine, fts, bases, [0.3], bo, mode, label=f"{mode} k=1")
        assert rep.coefficients == [1.0] and rep.linear
    out, _ = engine.geo_merge(fts, bases, [0.3], bo, mode="slerp")
    assert torch.equal(raw(out), raw(fts[0].to(bo.dtype)))


def check_shapes(engine, device="cpu"):
    """1-D, rank 3, n not a multiple of 8, C not a multiple of 8 row-wise, rows shorter than an octet, several segments"""
    for shape in ((4099,), (4, 33, 65), (37, 13), (300, 5), (3, 40000), (16, 4096)):
        for mode, rowwise in VARIANTS:
            k = variant_k(mode, 3)
            fts, bases, bo = make_inputs(shape, k, seed=40 + len(shape), own_bases=True, device=device)
            check(engine, fts, bases, ALPHAS[:k], bo, mode, rowwise, label=f"{mode} rowwise={rowwise} shape={shape}")
    for n in (1, 7, 8, 9, 2049):
        fts, bases, bo = make_inputs((n,), 2, seed=71, device=device)
        for mode, rowwise in VARIANTS:
            check(engine, fts, bases, ALPHAS[:2], bo, mode, rowwise, label=f"{mode} n={n}")


def check_unaligned(engine, device="cpu"):
    """views that start at an odd element"""
    for dtype in DTYPES:
        n = 1003
        fts, bases, bo = make_inputs((n + 5,), 2, dtype, seed=70, own_bases=True, device=device)
        cut = lambda t, o: t[o:o + n]
        for mode, rowwise in VARIANTS:
            check(engine, [cut(fts[0], 1), cut(fts[1], 3)], [cut(bases[0], 0), cut(bases[1], 1)], ALPHAS[:2], cut(bo, 1), mode, rowwise,
                  label=f"unaligned {mode} {dtype}")


def check_empty(engine, device="cpu"):
    fts, bases, bo = make_inputs((0,), 2, seed=73, device=device)
    for mode, rowwise in VARIANTS:
        out, rep = engine.geo_merge(fts, bases, [0.5, 0.5], bo, mode=mode, rowwise=rowwise)
        assert out.numel() == 0 and out.dtype == bo.dtype
    fts, bases, bo = make_inputs((0, 8), 2, seed=73, device=device)
    out, rep = engine.geo_merge(fts, bases, [0.5, 0.5], bo, rowwise=True)
    assert out.shape == (0, 8)


# ---- the Gram against exact arithmetic -----------------------------------------------------------------
def check_gram_against_fsum(engine, device="cpu"):
    """|G - exact| <= (n - 1) 2^-53 sum |x_i x_j|: the a-priori bound of recursive summation in ANY order (Higham,
    Accuracy and Stability of Numerical Algorithms, 4.2, first order; the products themselves are exact)"""
    for shape, k, dtype in (((97, 131), 3, torch.bfloat16), ((3, 40000), 2, torch.float32), ((4099,), 4, torch.float16)):
        fts, bases, bo = make_inputs(shape, k, dtype, seed=75, own_bases=True, device=device)
        _, rep = engine.geo_merge(fts, bases, ALPHAS[:k], bo)
        xs = [[float(v) for v in x.tolist()] for x in geo_oracle.vectors([t.cpu() for t in fts], [t.cpu() for t in bases], "model_stock")]
        n = len(xs[0])
        for i in range(k):
            for j in range(i, k):
                prods = [a * b for a, b in zip(xs[i], xs[j])]              # exact in fp64
                exact = math.fsum(prods)
                bound = (n - 1) * 2.0 ** -53 * math.fsum(abs(p) for p in prods)
                err = abs(rep.gram[i][j] - exact)
                print(f"gram {shape} ({i},{j}): {rep.gram[i][j]!r} exact {exact!r} err {err:.3e} bound {bound:.3e}")
                assert err <= bound, (shape, i, j, rep.gram[i][j], exact, err, bound)
                assert rep.gram[j][i] == rep.gram[i][j]


# ---- properties that need no oracle ------------------------------------------------------------------------
def check_disjoint_supports(engine, device="cpu"):
    """deltas with disjoint supports: G_ij = 0, cos = 0, t = 0 - the output of model_stock IS base_out"""
    for rowwise in (False, True):
        fts, bases, bo = make_inputs(SMALL, 3, seed=76, device=device)
        idx = torch.arange(bo.numel(), device=bo.device).view(bo.shape) % 3
        fts = [torch.where(idx == i, fts[i], bases[i]) for i in range(3)]
        out, rep = engine.geo_merge(fts, bases, ALPHAS[:3], bo, rowwise=rowwise)
        assert torch.equal(raw(out), raw(bo))
        if rowwise:
            assert rep.t_min == 0.0 and rep.t_max == 0.0 and rep.t_mean == 0.0
        else:
            assert rep.t == 0.0 and rep.cos == 0.0 and all(rep.gram[i][j] == 0.0 for i in range(3) for j in range(3) if i != j)
            assert all(rep.gram[i][i] > 0.0 for i in range(3)) and rep.coefficients == [0.0, 0.0, 0.0]


def check_row_permutation(engine, device="cpu"):
    """row-wise mode commutes with a permutation of the rows, byte for byte"""
    for shape in ((97, 131), (64, 256)):
        fts, bases, bo = make_inputs(shape, 3, seed=77, own_bases=True, device=device)
        perm = torch.randperm(shape[0], generator=torch.Generator().manual_seed(5)).to(bo.device)
        out, rep = engine.geo_merge(fts, bases, ALPHAS[:3], bo, rowwise=True)
        outp, repp = engine.geo_merge([t[perm].contiguous() for t in fts], [t[perm].contiguous() for t in bases], ALPHAS[:3],
                                      bo[perm].contiguous(), rowwise=True)
        assert torch.equal(raw(outp), raw(out[perm]))
        assert (repp.t_min, repp.t_max) == (rep.t_min, rep.t_max)


def check_nuslerp_endpoint(engine, device="cpu"):
    """alphas (1, 0): tau = 0, c = (1, 0) exactly, the output is base_out + delta_0; (0, 1) the other end"""
    fts, bases, bo = make_inputs(SMALL, 2, seed=78, own_bases=True, device=device)
    for alphas, want in (([1.0, 0.0], [1.0, 0.0]), ([0.0, 2.0], [0.0, 1.0])):
        rep, _ = check(engine, fts, bases, alphas, bo, "nuslerp", label=f"nuslerp alphas {alphas}")
        assert rep.coefficients == want and not rep.linear
        rep, _ = check(engine, fts, bases, alphas, bo, "slerp", label=f"slerp alphas {alphas}")
        assert rep.coefficients == want


def check_slerp_with_itself(engine, device="cpu"):
    """a tensor with itself: cos = 1 > 0.9995, the linear case; s = (1 - tau, tau)"""
    fts, bases, bo = make_inputs(SMALL, 1, seed=79, device=device)
    rep, _ = check(engine, [fts[0], fts[0]], [bases[0], bases[0]], [0.75, 0.25], bo, "slerp", label="slerp with itself")
    assert rep.linear and rep.omega == 0.0 and rep.cos > 0.9995 and rep.coefficients == [0.75, 0.25]
    rep, _ = check(engine, [fts[0], fts[0]], [bases[0], bases[0]], [0.75, 0.25], bo, "nuslerp", label="nuslerp with itself")
    assert rep.linear and rep.coefficients == [0.75, 0.25]


def check_scale_invariance(engine, device="cpu"):
    """one delta times 2 (exact in fp32): every cosine, hence cos and t of model_stock, keep their bits"""
    fts, bases, bo = make_inputs(SMALL, 3, torch.float32, seed=80, device=device)
    zero = [torch.zeros_like(b) for b in bases]
    ds = [f - b for f, b in zip(fts, bases)]
    _, rep = engine.geo_merge(ds, zero, ALPHAS[:3], bo)
    _, rep2 = engine.geo_merge([ds[0], ds[1] * 2.0, ds[2]], zero, ALPHAS[:3], bo)
    assert f64_bits(rep.cos) == f64_bits(rep2.cos) and f64_bits(rep.t) == f64_bits(rep2.t)
    assert rep2.gram[1][1] == 4.0 * rep.gram[1][1] and rep2.gram[0][1] == 2.0 * rep.gram[0][1]


# ---- corners ----------------------------------------------------------------------------------------------
def check_zero_deltas(engine, device="cpu"):
    """every finetune equals its base: every norm is 0, every cosine 0 by definition, t = 0; the pair operators are linear"""
    fts, bases, bo = make_inputs(SMALL, 2, seed=81, own_bases=True, device=device)
    fts = [b.clone() for b in bases]
    for rowwise in (False, True):
        rep, _ = check(engine, fts, bases, [0.5, 0.5], bo, "model_stock", rowwise, label="zero deltas")
        out, _ = engine.geo_merge(fts, bases, [0.5, 0.5], bo, rowwise=rowwise)
        assert torch.equal(raw(out), raw(bo))
    rep, _ = check(engine, fts, bases, [0.5, 0.5], bo, "nuslerp", label="zero deltas nuslerp")
    assert rep.linear and rep.coefficients == [0.5, 0.5]
    fts2, _, _ = make_inputs(SMALL, 2, seed=82, own_bases=True, device=device)       # one zero delta
    rep, _ = check(engine, [fts2[0], bases[1]], bases, [0.5, 0.5], bo, "nuslerp", label="one zero delta")
    assert rep.linear


def check_antiparallel(engine, device="cpu"):
    """k = 2, d_1 = -d_0: G_01 = -G_00 = -G_11 exactly.  With entries +-1 and a square element count the norms are exact,
    cos = -1, den = 1 + cos = 0, t = 0: the output is base_out.  With random entries cos is -1 up to the rounding of the two
    square roots (the header says so): whatever t comes out, it is the oracle's, bit for bit."""
    g = torch.Generator().manual_seed(61)
    d = (torch.randint(0, 2, (64, 256), generator=g).float() * 2 - 1).to(torch.bfloat16).to(device)
    zero = torch.zeros_like(d)
    bo = make_inputs((64, 256), 1, seed=62, device=device)[2]
    for rowwise in (False, True):
        rep, _ = check(engine, [d, -d], [zero, zero], [0.5, 0.5], bo, "model_stock", rowwise, label="antiparallel +-1")
        out, _ = engine.geo_merge([d, -d], [zero, zero], [0.5, 0.5], bo, rowwise=rowwise)
        assert torch.equal(raw(out), raw(bo))
        if rowwise:
            assert (rep.t_min, rep.t_max, rep.t_mean) == (0.0, 0.0, 0.0)
        else:
            assert rep.cos == -1.0 and rep.t == 0.0 and rep.gram[0][1] == -16384.0
    d = torch.randn(SMALL, generator=g).to(torch.bfloat16).to(device)
    zero = torch.zeros_like(d)
    bo = make_inputs(SMALL, 1, seed=62, device=device)[2]
    for rowwise in (False, True):
        rep, _ = check(engine, [d, -d], [zero, zero], [0.5, 0.5], bo, "model_stock", rowwise, label="antiparallel")
        if not rowwise:
            assert rep.gram[0][1] == -rep.gram[0][0] == -rep.gram[1][1] and rep.cos <= -1.0 + 2.0 ** -51
    rep, _ = check(engine, [d, -d], [zero, zero], [0.5, 0.5], bo, "nuslerp", label="antiparallel nuslerp")
    assert rep.linear                     # |cos| > 0.9995


def check_nearly_parallel(engine, device="cpu"):
    """|cos| just above and just below 0.9995: the linear case and the spherical one"""
    g = torch.Generator().manual_seed(83)
    d = torch.randn(SMALL, generator=g)
    e = torch.randn(SMALL, generator=g)
    zero = torch.zeros(SMALL, device=device)
    bo = make_inputs(SMALL, 1, torch.float32, seed=84, device=device)[2]
    for eps, linear in ((0.01, True), (0.05, False)):
        a, b = d.to(device), (d + eps * e).to(device)
        for mode in ("nuslerp", "slerp"):
            rep, _ = check(engine, [a, b], [zero, zero], [0.5, 0.25], bo, mode, label=f"{mode} eps={eps}")
            assert rep.linear is linear and (rep.omega == 0.0) is linear, (eps, rep)
        rep, _ = check(engine, [a, -b], [zero, zero], [0.5, 0.25], bo, "slerp", label=f"slerp negative eps={eps}")
        assert rep.linear is linear and rep.cos < 0


def check_tiny_alpha_sum(engine, device="cpu"):
    """model_stock with alphas that sum to 0: A := 1"""
    fts, bases, bo = make_inputs(SMALL, 2, seed=85, device=device)
    check(engine, fts, bases, [0.5, -0.5], bo, label="A = 0")
    check(engine, fts, bases, [0.5, -0.25], bo, rowwise=True, label="signed alphas")


def check_nonfinite(engine, device="cpu"):
    """a NaN / an Inf in one vector: ValueError naming the tensor and the finetune; the context stays usable"""
    for mode, rowwise in VARIANTS:
        k = variant_k(mode, 3)
        for poison in (float("nan"), float("inf")):
            fts, bases, bo = make_inputs(SMALL, k, seed=86, device=device)
            fts[1] = fts[1].clone()
            fts[1].view(-1)[4321] = poison
            with pytest.raises(ValueError, match=r"model\.layers\.7\.mlp\.up_proj\.weight.*finetune 1\b"):
                engine.geo_merge(fts, bases, ALPHAS[:k], bo, mode=mode, rowwise=rowwise, layer_name="model.layers.7.mlp.up_proj.weight")
        fts, bases, bo = make_inputs(SMALL, k, seed=87, device=device)
        check(engine, fts, bases, ALPHAS[:k], bo, mode, rowwise, label="after an error")
    # Inf - Inf in the delta although no delta element is Inf itself; in weight space the Inf itself
    fts, bases, bo = make_inputs(SMALL, 2, torch.float32, seed=88, own_bases=True, device=device)
    fts[0].view(-1)[5] = float("inf")
    bases[0].view(-1)[5] = float("inf")
    for mode in MODES:
        with pytest.raises(ValueError, match=r"finetune 0\b"):
            engine.geo_merge(fts, bases, ALPHAS[:2], bo, mode=mode)


def check_determinism(engine, device="cpu"):
    fts, bases, bo = make_inputs((300, 500), 2, seed=90, own_bases=True, device=device)
    for mode, rowwise in VARIANTS:
        a, ra = engine.geo_merge(fts, bases, ALPHAS[:2], bo, mode=mode, rowwise=rowwise)
        b, rb = engine.geo_merge(fts, bases, ALPHAS[:2], bo, mode=mode, rowwise=rowwise)
        assert torch.equal(raw(a), raw(b)) and ra == rb


def check_arguments(engine, device="cpu"):
    fts, bases, bo = make_inputs((8, 8), 3, seed=91, device=device)
    with pytest.raises(ValueError, match="mode"):
        engine.geo_merge(fts, bases, ALPHAS[:3], bo, mode="karcher")
    for mode in ("nuslerp", "slerp"):
        with pytest.raises(ValueError, match="at most 2"):
            engine.geo_merge(fts, bases, ALPHAS[:3], bo, mode=mode)
        with pytest.raises(ValueError, match="rowwise"):
            engine.geo_merge(fts[:2], bases[:2], ALPHAS[:2], bo, mode=mode, rowwise=True)
        for alphas in ([-0.5, 1.0], [0.0, 0.0], [float("nan"), 1.0]):
            with pytest.raises(ValueError, match="alphas"):
                engine.geo_merge(fts[:2], bases[:2], alphas, bo, mode=mode)
    with pytest.raises(ValueError, match="shape mismatch"):
        engine.geo_merge([fts[0], fts[1][:4]], bases[:2], [0.5, 0.5], bo)
    with pytest.raises(ValueError, match="supported range"):
        engine.geo_merge([fts[0]] * 17, [bases[0]] * 17, [0.1] * 17, bo)
    with pytest.raises(ValueError, match="alphas"):
        engine.geo_merge(fts, bases, [0.5], bo)


PROPERTIES = [check_disjoint_supports, check_row_permutation, check_nuslerp_endpoint, check_slerp_with_itself, check_scale_invariance]
CORNERS = [check_pair_k1, check_shapes, check_unaligned, check_empty, check_gram_against_fsum, check_zero_deltas, check_antiparallel,
           check_nearly_parallel, check_tiny_alpha_sum, check_nonfinite, check_determinism, check_arguments]


def check_profile(engine, mode, rowwise, k, shape=(40, 50), device="cpu"):
    """profile names and launch counts: ONE geo_gram and ONE geo_combine per call whatever k, the fold for whole-tensor
    calls, the coefficient kernel for row-wise ones"""
    fts, bases, bo = make_inputs(shape, k, seed=6, device=device)
    engine.ctx.profile(True)
    engine.ctx.profile_reset()
    try:
        engine.geo_merge(fts, bases, ALPHAS[:k], bo, mode=mode, rowwise=rowwise)
        table = engine.ctx.profile_table()
    finally:
        engine.ctx.profile(False)
    expected = {"geo_gram": 1, "geo_combine": 1, ("geo_coef" if rowwise else "geo_gram_fold"): 1}
    assert {n: table[n][0] for n in table} == expected


# ---- the CLI on the synthetic on-disk model of tests/lora_fixtures.py ----------------------------------------
README_WORDS = {"model_stock": ("# Model Stock Merged Model", "model_stock:"), "nuslerp": ("# NuSLERP Merged Model", "nuslerp:"),
                "slerp": ("# SLERP Merged Model", "slerp:")}


def options(operator, filter_wise=None):
    opts = {"operator": operator}
    if filter_wise is not None:
        opts["stock_filter_wise"] = filter_wise
    return opts


def geo_models(operator, third):
    """model_stock: layer 0 all three finetunes, layer 1 ft1 and `third`; ft2 is a finetune of ft1 (its own base).
    nuslerp / slerp take two entries: ft1 on every layer, `third` from layer 1 on - layer 0 is left with ONE entry."""
    if operator == "model_stock":
        return ties_models(third)
    return [{"model": "org/ft1", "base": "org/base", "alpha": 0.5, "is_input": True},
            {"model": third, "base": "org/base", "alpha": 0.4, "is_output": True, "start_layer": 1}]


def write_config(root, third, out_dir, opts, device=None):
    return harness.write_config(root, geo_models(opts["operator"], third), out_dir, opts, device)


def expected_outputs(base, full, opts):
    """the oracle tensor by tensor (block tensors) / the provider's tensor (passthrough)"""
    operator = opts["operator"]
    def merge(fts, bases, alphas, base_out, name):
        return geo_oracle.geo_merge(
            fts, bases, alphas, base_out, mode=operator, rowwise=bool(opts.get("stock_filter_wise", 0)))["out"]

    return expected_by_tensor(base, full, geo_models(operator, "org/lora_full"), merge)
