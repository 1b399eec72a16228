"""Checks of the Model Breadcrumbs operators shared by the emulator tier (tests/test_breadcrumbs_host.py) and the GPU
tier (tests/test_breadcrumbs_gpu.py): Engine.breadcrumbs_merge against tests/breadcrumbs_oracle.py, BIT FOR BIT - output,
merged delta, both thresholds, kept and dropped_top counts, k_keep, n_top.  The tolerance is zero and it is derived,
not measured: every step of the function is one correctly rounded fp32 operation or an exact order statistic
(include/shardmerge_hip.h, smhip_breadcrumbs_merge)."""
import math

import pytest
import torch

from tests import breadcrumbs_oracle
from tests import harness
from tests.harness import ALPHAS, DTYPES, SMALL, expected_by_tensor, f32_bits, make_inputs, raw, ties_models

# (density, gamma); the last one has k_keep == 0: thresholds +inf, nothing kept
DENSITY_GAMMA = ((0.9, 0.01), (0.2, 0.01), (0.5, 0.5), (0.9, 0.1), (1.0, 0.0), (0.2, 0.0), (1e-9, 0.3))
MODES = (True, False)                           # sign_election: breadcrumbs_ties, breadcrumbs
INF = float("inf")


def mode_name(sign_election):
    return "breadcrumbs_ties" if sign_election else "breadcrumbs"


def key_of(x: float) -> int:
    """the 31 magnitude bits of an fp32 value: what the radix select orders by"""
    return int.from_bytes(f32_bits(float(x)), "little") & 0x7FFFFFFF


def check(engine, fts, bases, alphas, base_out, density=0.9, gamma=0.01, lam=1.0, normalize=True, sign_election=False, label=""):
    """one call against the oracle, bit for bit; returns the engine's report"""
    kw = dict(density=density, gamma=gamma, lam=lam, normalize=normalize, sign_election=sign_election)
    out, rep, delta = engine.breadcrumbs_merge(fts, bases, alphas, base_out, want_delta=True, **kw)
    cpu = lambda ts: [t.cpu() for t in ts]
    ref, ref_delta, k_keep, n_top, lo, hi, kept, dropped = breadcrumbs_oracle.breadcrumbs_merge(cpu(fts), cpu(bases), alphas, base_out.cpu(), **kw)
    print(f"{label}: k_keep {rep.k_keep} / {k_keep}, n_top {rep.n_top} / {n_top}, kept {rep.kept} / {kept}, "
          f"dropped_top {rep.dropped_top} / {dropped}, lo {rep.thresholds_lo}, hi {rep.thresholds_hi}")
    assert out.dtype == base_out.dtype and out.shape == base_out.shape, label
    assert (rep.k_keep, rep.n_top) == (k_keep, n_top), (label, rep.k_keep, k_keep, rep.n_top, n_top)
    assert [f32_bits(t) for t in rep.thresholds_lo] == [f32_bits(float(t)) for t in lo], (label, rep.thresholds_lo, lo)
    assert [f32_bits(t) for t in rep.thresholds_hi] == [f32_bits(float(t)) for t in hi], (label, rep.thresholds_hi, hi)
    assert rep.kept == kept, (label, rep.kept, kept)
    assert rep.dropped_top == dropped, (label, rep.dropped_top, dropped)
    assert all(d <= n_top for d in rep.dropped_top), (label, rep.dropped_top, n_top)
    bad = int((raw(delta) != raw(ref_delta)).sum())
    assert bad == 0, f"{label}: {bad} of {ref_delta.numel()} merged-delta values differ in their bits"
    bad = int((raw(out) != raw(ref)).sum())
    assert bad == 0, f"{label}: {bad} of {ref.numel()} output values differ in their bits"
    return rep


# ---- the parameter grid -------------------------------------------------------------------------------
def check_dtypes(engine, in_dtype, bo_dtype, sign_election, device="cpu"):
    fts, bases, bo = make_inputs(SMALL, 3, in_dtype, bo_dtype, seed=11, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:3], bo, density=0.2, gamma=0.01, lam=0.7, sign_election=sign_election, label=f"{in_dtype}->{bo_dtype}")
    fts, bases, bo = make_inputs(SMALL, 2, in_dtype, bo_dtype, seed=12, device=device)      # one shared base
    check(engine, fts, bases, ALPHAS[:2], bo, density=0.5, gamma=0.1, normalize=False, sign_election=sign_election,
          label=f"{in_dtype}->{bo_dtype} shared")


def check_k_density_gamma(engine, k, density, gamma, sign_election, device="cpu"):
    for j, (lam, normalize) in enumerate(((1.0, True), (0.7, False))):
        fts, bases, bo = make_inputs(SMALL, k, seed=20 + k + j, own_bases=bool(j), device=device)
        rep = check(engine, fts, bases, ALPHAS[:k], bo, density=density, gamma=gamma, lam=lam, normalize=normalize,
                    sign_election=sign_election,
                    label=f"{mode_name(sign_election)} k={k} density={density} gamma={gamma} lam={lam} normalize={normalize}")
        if density == 1e-9:
            assert rep.k_keep == 0 and rep.kept == [0] * k and rep.dropped_top == [0] * k
            assert all(t == INF for t in rep.thresholds_lo + rep.thresholds_hi)
            out, _ = engine.breadcrumbs_merge(fts, bases, ALPHAS[:k], bo, density=density, gamma=gamma, lam=lam, normalize=normalize,
                                              sign_election=sign_election)
            assert torch.equal(raw(out), raw(bo))
        if gamma == 0.0:
            assert rep.n_top == 0 and rep.dropped_top == [0] * k


def check_lambda_normalize(engine, lam, normalize, sign_election, device="cpu"):
    fts, bases, bo = make_inputs((64, 200), 3, seed=40, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:3], bo, lam=lam, normalize=normalize, sign_election=sign_election,
          label=f"lam={lam} normalize={normalize}")


def check_signed_alphas(engine, device="cpu"):
    for sign_election in MODES:
        for normalize in (True, False):
            fts, bases, bo = make_inputs(SMALL, 4, seed=50, own_bases=True, device=device)
            check(engine, fts, bases, [0.5, -0.3, 0.0, -0.7], bo, density=0.5, gamma=0.05, lam=0.7, normalize=normalize,
                  sign_election=sign_election, label="signed alphas")


# ---- the two identities of the definition ---------------------------------------------------------------------
def check_gamma_zero_is_ties(engine, device="cpu"):
    """gamma == 0 with sign_election == 1 is smhip_ties_merge with the same density, lambda, normalize"""
    for k, own, density, lam, normalize in ((3, True, 0.2, 0.7, True), (5, False, 0.5, 1.0, False), (1, False, 1.0, 1.0, True),
                                            (2, True, 0.01, 1.0, True)):
        fts, bases, bo = make_inputs(SMALL, k, seed=100 + k, own_bases=own, device=device)
        t_out, t_rep, t_delta = engine.ties_merge(fts, bases, ALPHAS[:k], bo, density=density, lam=lam, normalize=normalize, want_delta=True)
        out, rep, delta = engine.breadcrumbs_merge(fts, bases, ALPHAS[:k], bo, density=density, gamma=0.0, lam=lam, normalize=normalize,
                                                   sign_election=True, want_delta=True)
        assert torch.equal(raw(out), raw(t_out)) and torch.equal(raw(delta), raw(t_delta)), (k, density)
        assert rep.k_keep == t_rep.k_keep and rep.kept == t_rep.kept and rep.n_top == 0 and rep.dropped_top == [0] * k
        assert [f32_bits(t) for t in rep.thresholds_lo] == [f32_bits(t) for t in t_rep.thresholds]


def check_all_kept_is_dare_linear(engine, device="cpu"):
    """gamma == 0, density == 1, sign_election == 0 is smhip_dare_merge at density 1, sign_election 0: any key, either rescale"""
    for k, own, lam, normalize in ((3, True, 0.7, True), (5, False, 1.0, False), (1, False, 1.0, True)):
        fts, bases, bo = make_inputs(SMALL, k, seed=100 + k, own_bases=own, device=device)
        out, rep, delta = engine.breadcrumbs_merge(fts, bases, ALPHAS[:k], bo, density=1.0, gamma=0.0, lam=lam, normalize=normalize,
                                                   sign_election=False, want_delta=True)
        for key in (0, 0x0123456789ABCDEF):
            for rescale in (True, False):
                d_out, d_rep, d_delta = engine.dare_merge(fts, bases, ALPHAS[:k], bo, density=1.0, lam=lam, normalize=normalize,
                                                          rescale=rescale, sign_election=False, key=key, want_delta=True)
                assert torch.equal(raw(out), raw(d_out)) and torch.equal(raw(delta), raw(d_delta)), (k, key, rescale)
                assert rep.kept == d_rep.kept


# ---- where the two ranks part ---------------------------------------------------------------------------------
def _thresholds(fts, bases, bo, density, gamma):
    cpu = lambda ts: [t.cpu() for t in ts]
    r = breadcrumbs_oracle.breadcrumbs_merge(cpu(fts), cpu(bases), [1.0] * len(fts), bo.cpu(), density=density, gamma=gamma)
    return [key_of(t) for t in r[4]], [key_of(t) for t in r[5]], r


def check_ranks_part_at_level1(engine, device="cpu"):
    """the two thresholds differ in their first 11 bits: two histogram bins at level 1, two prefixes from then on"""
    fts, bases, bo = make_inputs(SMALL, 2, seed=200, device=device)
    lo, hi, _ = _thresholds(fts, bases, bo, 0.2, 0.01)
    assert all(l >> 20 != h >> 20 for l, h in zip(lo, hi)), (lo, hi)
    for sign_election in MODES:
        check(engine, fts, bases, ALPHAS[:2], bo, density=0.2, gamma=0.01, sign_election=sign_election, label="ranks part at level 1")


def check_ranks_part_at_level2(engine, device="cpu"):
    """both thresholds in one level-1 bin, different 21-bit prefixes: the shared histogram at level 2, two at level 3"""
    fts, bases, bo = make_inputs((256, 512), 2, seed=65, sigma=3e-4, device=device)
    lo, hi, _ = _thresholds(fts, bases, bo, 0.001, 0.0005)
    assert all(l >> 20 == h >> 20 and l >> 10 != h >> 10 for l, h in zip(lo, hi)), ([hex(v) for v in lo], [hex(v) for v in hi])
    for sign_election in MODES:
        check(engine, fts, bases, ALPHAS[:2], bo, density=0.001, gamma=0.0005, sign_election=sign_election, label="ranks part at level 2")


def _bit_pattern_inputs(n, seed, device):
    """a zero base and fp32 finetune values 0x3f800000 + j, j uniform in [0, 1024), random sign"""
    g = torch.Generator().manual_seed(seed)
    fts = []
    for _ in range(2):
        j = torch.randint(0, 1024, (n,), generator=g, dtype=torch.int32)
        sign = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32) << 31        # (wraps to the sign bit)
        fts.append(((j + 0x3F800000) | sign).view(torch.float32).to(device))
    zero = torch.zeros(n, dtype=torch.float32, device=device)
    return fts, [zero, zero], zero


def check_ranks_part_at_level3(engine, device="cpu"):
    """the thresholds share 21 bits and differ in the last 10: one shared histogram at levels 2 AND 3"""
    fts, bases, bo = _bit_pattern_inputs(4096, 210, device)
    lo, hi, _ = _thresholds(fts, bases, bo, 0.2, 0.1)
    assert all(l >> 10 == h >> 10 and l != h for l, h in zip(lo, hi)), ([hex(v) for v in lo], [hex(v) for v in hi])
    for sign_election in MODES:
        rep = check(engine, fts, bases, ALPHAS[:2], bo, density=0.2, gamma=0.1, sign_election=sign_election, label="ranks part at level 3")
        assert all(0 < d <= rep.n_top for d in rep.dropped_top)


def check_ranks_coincide(engine, device="cpu"):
    """tau_lo == tau_hi: deltas drawn from {1, 2, 3} x 2^-10, both ranks fall among the 3 x 2^-10: nothing dropped at the
    top, every such element kept"""
    g = torch.Generator().manual_seed(220)
    n = 4096
    fts = []
    for _ in range(2):
        v = torch.randint(1, 4, (n,), generator=g).float() * 2.0 ** -10
        fts.append((v * (torch.randint(0, 2, (n,), generator=g).float() * 2 - 1)).to(device))
    zero = torch.zeros(n, dtype=torch.float32, device=device)
    lo, hi, r = _thresholds(fts, [zero, zero], zero, 0.1, 0.05)
    assert lo == hi == [key_of(3 * 2.0 ** -10)] * 2, (lo, hi)
    for sign_election in MODES:
        rep = check(engine, fts, [zero, zero], [0.5, 0.25], zero, density=0.1, gamma=0.05, sign_election=sign_election, label="tau_lo == tau_hi")
        assert rep.dropped_top == [0, 0] and all(kept > rep.k_keep for kept in rep.kept)
        assert rep.kept == [int((f.abs() == 3 * 2.0 ** -10).sum()) for f in fts]


# ---- corners ----------------------------------------------------------------------------------------------
def check_default_case_drops_at_the_top(engine, device="cpu"):
    """the upper cut is not vacuous at the small test size: 1 <= dropped_top <= n_top, and the result is not TIES's"""
    fts, bases, bo = make_inputs(SMALL, 3, seed=11, own_bases=True, device=device)
    rep = check(engine, fts, bases, ALPHAS[:3], bo, density=0.2, gamma=0.01, sign_election=True, label="default case")
    assert rep.n_top == 127 and rep.k_keep == 2541
    assert all(1 <= d <= rep.n_top for d in rep.dropped_top) and all(kept >= rep.k_keep for kept in rep.kept)
    out, _ = engine.breadcrumbs_merge(fts, bases, ALPHAS[:3], bo, density=0.2, gamma=0.01, sign_election=True)
    t_out, _ = engine.ties_merge(fts, bases, ALPHAS[:3], bo, density=0.2)
    assert not torch.equal(raw(out), raw(t_out))


def check_zero_delta(engine, device="cpu"):
    """a finetune equal to its base: tau_lo == 0 (and tau_hi), nothing of it kept, nothing dropped at the top"""
    for sign_election in MODES:
        fts, bases, bo = make_inputs(SMALL, 2, seed=60, device=device)
        fts[1] = bases[1].clone()
        rep = check(engine, fts, bases, [0.5, 0.5], bo, density=0.3, gamma=0.02, sign_election=sign_election, label="zero delta")
        assert rep.thresholds_lo[1] == 0.0 and rep.thresholds_hi[1] == 0.0 and rep.kept[1] == 0 and rep.dropped_top[1] == 0
        assert rep.kept[0] >= rep.k_keep > 0


def check_tiny_weight_sum(engine, device="cpu"):
    """weights that make |D| < 1e-8: D is replaced by 1"""
    x = (torch.randn(SMALL, generator=torch.Generator().manual_seed(63)).abs() + 0.5).to(torch.bfloat16).to(device)
    zero = torch.zeros_like(x)
    bo = make_inputs(SMALL, 1, seed=64, device=device)[2]
    for sign_election in MODES:         # breadcrumbs_ties: both entries agree (+), D = 0.5 - 0.5; breadcrumbs: D over all = 0
        check(engine, [x, -x], [zero, zero], [0.5, -0.5], bo, density=1.0, gamma=0.0, sign_election=sign_election, label="D = 0")
        _, _, delta = engine.breadcrumbs_merge([x, -x], [zero, zero], [0.5, -0.5], bo, density=1.0, gamma=0.0,
                                               sign_election=sign_election, want_delta=True)
        assert torch.equal(delta.cpu(), x.float().cpu())              # 0.5 x + 0.5 x over D := 1
        check(engine, [x], [zero], [1e-9], bo, density=0.5, gamma=0.1, sign_election=sign_election, label="D = 1e-9")


def check_ties_exceed_k(engine, device="cpu"):
    """differences of bf16 weights collide: more than k_keep elements lie between the thresholds, all of them are kept"""
    fts, bases, bo = make_inputs((256, 512), 2, seed=65, sigma=3e-4, device=device)
    for sign_election in MODES:
        rep = check(engine, fts, bases, [0.5, 0.5], bo, density=0.2, gamma=0.01, sign_election=sign_election, label="ties")
        assert all(kept > rep.k_keep for kept in rep.kept), (rep.kept, rep.k_keep)


def check_denormals(engine, device="cpu"):
    g = torch.Generator().manual_seed(66)
    ft = (torch.randn(SMALL, generator=g) * 1e-40).to(device)
    assert 0 < float(ft.abs().max()) < 1.2e-38
    zero = torch.zeros_like(ft)
    fb = (torch.randn(SMALL, generator=g) * 1e-39).to(torch.bfloat16).to(device)
    assert 0 < float(fb.float().abs().max()) < 1.2e-38
    bo = make_inputs(SMALL, 1, seed=67, device=device)[2]
    for sign_election in MODES:
        check(engine, [ft, ft * 0.5], [zero, zero], [0.5, 0.75], zero, density=0.5, gamma=0.05, lam=0.7, sign_election=sign_election,
              label="fp32 denormal deltas")
        check(engine, [fb], [torch.zeros_like(fb)], [0.5], bo, density=0.5, gamma=0.05, sign_election=sign_election, label="bf16 denormal deltas")
        check(engine, [fb], [torch.zeros_like(fb)], [0.5], torch.zeros_like(fb), density=0.5, gamma=0.05, sign_election=sign_election,
              label="bf16 denormals onto zero")


def check_unaligned(engine, device="cpu"):
    """views that start at an odd element, and element counts that are not multiples of 8"""
    for dtype in DTYPES:
        for n in (1003, 4096):
            fts, bases, bo = make_inputs((n + 5,), 3, dtype, seed=70, own_bases=True, device=device)
            cut = lambda t, o: t[o:o + n]
            check(engine, [cut(fts[0], 1), cut(fts[1], 3), cut(fts[2], 0)], [cut(bases[0], 0), cut(bases[1], 1), cut(bases[2], 5)],
                  ALPHAS[:3], cut(bo, 1), density=0.2, gamma=0.05, sign_election=dtype != torch.float16, label=f"unaligned {dtype} n={n}")
    for n in (1, 7, 8, 9, 1003, 2049):
        for sign_election in MODES:
            fts, bases, bo = make_inputs((n,), 2, seed=71, device=device)
            check(engine, fts, bases, ALPHAS[:2], bo, density=0.5, gamma=0.2, sign_election=sign_election, label=f"n={n}")


def check_tiny_and_rank3(engine, device="cpu"):
    fts, bases, bo = make_inputs((1,), 2, seed=72, own_bases=True, device=device)
    check(engine, fts, bases, [0.5, 0.5], bo, density=1.0, gamma=0.0, label="1 element")
    check(engine, fts, bases, [0.5, 0.5], bo, density=0.5, gamma=0.5, label="1 element, k_keep = 0")
    fts, bases, bo = make_inputs((0,), 2, seed=73, device=device)
    out, rep = engine.breadcrumbs_merge(fts, bases, [0.5, 0.5], bo)
    assert out.numel() == 0 and out.dtype == bo.dtype and rep.k_keep == 0 and rep.n_top == 0
    assert rep.kept == [0, 0] and rep.dropped_top == [0, 0] and rep.thresholds_lo == [INF, INF] and rep.thresholds_hi == [INF, INF]
    for sign_election in MODES:
        fts, bases, bo = make_inputs((4, 33, 65), 3, seed=74, own_bases=True, device=device)
        check(engine, fts, bases, ALPHAS[:3], bo, sign_election=sign_election, label="rank 3")


def check_nonfinite(engine, device="cpu"):
    """a NaN / an Inf in one finetune: ValueError naming the tensor and the finetune; the context stays usable"""
    for poison in (float("nan"), float("inf"), float("-inf")):
        fts, bases, bo = make_inputs(SMALL, 3, seed=80, device=device)
        fts[1] = fts[1].clone()
        fts[1].view(-1)[4321] = poison
        with pytest.raises(ValueError, match=r"model\.layers\.7\.mlp\.up_proj\.weight.*finetune 1\b"):
            engine.breadcrumbs_merge(fts, bases, ALPHAS[:3], bo, layer_name="model.layers.7.mlp.up_proj.weight")
        fts, bases, bo = make_inputs(SMALL, 3, seed=81, device=device)
        check(engine, fts, bases, ALPHAS[:3], bo, label="after an error")
    # Inf - Inf in the delta although no delta element is Inf itself
    fts, bases, bo = make_inputs(SMALL, 2, torch.float32, seed=82, own_bases=True, device=device)
    fts[0].view(-1)[5] = float("inf")
    bases[0].view(-1)[5] = float("inf")
    with pytest.raises(ValueError, match=r"finetune 0\b"):
        engine.breadcrumbs_merge(fts, bases, ALPHAS[:2], bo, sign_election=True)
    fts, bases, bo = make_inputs(SMALL, 2, seed=83, device=device)
    check(engine, fts, bases, ALPHAS[:2], bo, label="after Inf - Inf")


def check_determinism(engine, device="cpu"):
    fts, bases, bo = make_inputs((300, 500), 3, seed=90, own_bases=True, device=device)
    for sign_election in MODES:
        a, ra = engine.breadcrumbs_merge(fts, bases, ALPHAS[:3], bo, sign_election=sign_election)
        b, rb = engine.breadcrumbs_merge(fts, bases, ALPHAS[:3], bo, sign_election=sign_election)
        assert torch.equal(raw(a), raw(b)) and ra == rb


def check_arguments(engine, device="cpu"):
    fts, bases, bo = make_inputs((8, 8), 2, seed=91, device=device)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="density"):
            engine.breadcrumbs_merge(fts, bases, [0.5, 0.5], bo, density=bad, gamma=0.0)
    for bad in (-0.01, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="gamma"):
            engine.breadcrumbs_merge(fts, bases, [0.5, 0.5], bo, density=0.5, gamma=bad)
    for density, gamma in ((0.9, 0.2), (1.0, 0.01), (0.5, 0.5 + 2.0 ** -52)):
        with pytest.raises(ValueError, match="density.*gamma"):
            engine.breadcrumbs_merge(fts, bases, [0.5, 0.5], bo, density=density, gamma=gamma)
    # the sum is taken in fp64: 0.5 + nextafter(0.5, 1) rounds to 1 and is in range
    rep = check(engine, fts, bases, [0.5, 0.5], bo, density=0.5, gamma=math.nextafter(0.5, 1.0), label="density + gamma rounds to 1")
    assert (rep.k_keep, rep.n_top) == (32, 32)
    with pytest.raises(ValueError, match="shape mismatch"):
        engine.breadcrumbs_merge([fts[0], fts[1][:4]], bases, [0.5, 0.5], bo)
    with pytest.raises(ValueError, match="supported range"):
        engine.breadcrumbs_merge([fts[0]] * 17, [bases[0]] * 17, [0.1] * 17, bo)
    with pytest.raises(ValueError, match="alphas"):
        engine.breadcrumbs_merge(fts, bases, [0.5], bo)


CORNERS = [check_signed_alphas, check_gamma_zero_is_ties, check_all_kept_is_dare_linear, check_ranks_part_at_level1,
           check_ranks_part_at_level2, check_ranks_part_at_level3, check_ranks_coincide, check_default_case_drops_at_the_top,
           check_zero_delta, check_tiny_weight_sum, check_ties_exceed_k, check_denormals, check_unaligned, check_tiny_and_rank3,
           check_nonfinite, check_determinism, check_arguments]


def check_profile(engine, k, expected, shape=(40, 50), device="cpu"):
    """profile names and launch counts: both ranks of every finetune in the same passes"""
    fts, bases, bo = make_inputs(shape, k, seed=6, device=device)
    engine.ctx.profile(True)
    engine.ctx.profile_reset()
    try:
        engine.breadcrumbs_merge(fts, bases, ALPHAS[:k], bo, density=0.5, gamma=0.1)
        table = engine.ctx.profile_table()
    finally:
        engine.ctx.profile(False)
    assert {n: table[n][0] for n in table} == expected


# ---- the CLI on the synthetic on-disk model of tests/lora_fixtures.py ----------------------------------------
def options(operator):
    return {"operator": operator, "density": 0.3, "gamma": 0.05, "breadcrumbs_lambda": 0.7}


def write_config(root, third, out_dir, opts, device=None):
    return harness.write_config(root, ties_models(third), out_dir, opts, device)


def expected_outputs(base, full, opts):
    """the oracle tensor by tensor (block tensors) / the provider's tensor (passthrough)"""
    def merge(fts, bases, alphas, base_out, name):
        return breadcrumbs_oracle.breadcrumbs_merge(
            fts, bases, alphas, base_out, density=opts.get("density", 0.9), gamma=opts.get("gamma", 0.01),
            lam=opts.get("breadcrumbs_lambda", 1.0), normalize=bool(opts.get("breadcrumbs_normalize", 1)),
            sign_election=opts["operator"] == "breadcrumbs_ties")[0]

    return expected_by_tensor(base, full, ties_models("org/lora_full"), merge)
