"""Checks of the TIES operator shared by the emulator tier (tests/test_ties_host.py) and the GPU tier
(tests/test_ties_gpu.py): Engine.ties_merge against tests/ties_oracle.py, BIT FOR BIT - output, merged delta,
thresholds and kept counts.  The tolerance is zero and it is derived, not measured: every step of the function is one
correctly rounded fp32 operation or an exact order statistic (include/shardmerge_hip.h, smhip_ties_merge)."""
import pytest
import torch

from tests import harness, ties_oracle
from tests.harness import ALPHAS, DTYPES, SMALL, expected_by_tensor, f32_bits, make_inputs, raw, ties_models

DENSITIES = (1.0, 0.5, 0.2, 0.01, 1e-9)          # the last one: k_keep == 0, the output is base_out


def check(engine, fts, bases, alphas, base_out, density=0.2, lam=1.0, normalize=True, label=""):
    """one call against the oracle, bit for bit; returns the engine's report"""
    out, rep, delta = engine.ties_merge(fts, bases, alphas, base_out, density=density, lam=lam, normalize=normalize,
                                        want_delta=True)
    cpu = lambda ts: [t.cpu() for t in ts]
    ref, ref_delta, k_keep, taus, kept = ties_oracle.ties_merge(cpu(fts), cpu(bases), alphas, base_out.cpu(), density, lam, normalize)
    assert out.dtype == base_out.dtype and out.shape == base_out.shape, label
    assert rep.k_keep == k_keep, (label, rep.k_keep, k_keep)
    assert [f32_bits(t) for t in rep.thresholds] == [f32_bits(float(t)) for t in taus], (label, rep.thresholds, taus)
    assert rep.kept == kept, (label, rep.kept, kept)
    bad = int((raw(delta) != raw(ref_delta)).sum())
    assert bad == 0, f"{label}: {bad} of {ref_delta.numel()} merged-delta values differ in their bits"
    bad = int((raw(out) != raw(ref)).sum())
    assert bad == 0, f"{label}: {bad} of {ref.numel()} output values differ in their bits"
    return rep


# ---- the parameter grid -------------------------------------------------------------------------------
def check_dtypes(engine, in_dtype, bo_dtype, device="cpu"):
    fts, bases, bo = make_inputs(SMALL, 3, in_dtype, bo_dtype, seed=11, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:3], bo, density=0.2, lam=0.7, label=f"{in_dtype}->{bo_dtype}")
    fts, bases, bo = make_inputs(SMALL, 2, in_dtype, bo_dtype, seed=12, device=device)      # one shared base
    check(engine, fts, bases, ALPHAS[:2], bo, density=0.5, normalize=False, label=f"{in_dtype}->{bo_dtype} shared")


def check_k_density(engine, k, density, device="cpu"):
    for j, (lam, normalize) in enumerate(((1.0, True), (0.7, False))):
        fts, bases, bo = make_inputs(SMALL, k, seed=20 + k + j, own_bases=bool(j), device=device)
        rep = check(engine, fts, bases, ALPHAS[:k], bo, density=density, lam=lam, normalize=normalize,
                    label=f"k={k} density={density} lam={lam} normalize={normalize}")
        if density == 1e-9:
            assert rep.k_keep == 0 and rep.kept == [0] * k and all(t == float("inf") for t in rep.thresholds)
            out, _ = engine.ties_merge(fts, bases, ALPHAS[:k], bo, density=density, lam=lam, normalize=normalize)
            assert torch.equal(raw(out), raw(bo))


def check_lambda_normalize(engine, lam, normalize, device="cpu"):
    fts, bases, bo = make_inputs((64, 200), 3, seed=40, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:3], bo, lam=lam, normalize=normalize, label=f"lam={lam} normalize={normalize}")


def check_signed_alphas(engine, device="cpu"):
    for normalize in (True, False):
        fts, bases, bo = make_inputs(SMALL, 4, seed=50, own_bases=True, device=device)
        check(engine, fts, bases, [0.5, -0.3, 0.0, -0.7], bo, density=0.5, lam=0.7, normalize=normalize, label="signed alphas")


# ---- corners ----------------------------------------------------------------------------------------------
def check_zero_delta(engine, device="cpu"):
    """a finetune equal to its base: tau = 0, nothing of it kept"""
    fts, bases, bo = make_inputs(SMALL, 2, seed=60, device=device)
    fts[1] = bases[1].clone()
    rep = check(engine, fts, bases, [0.5, 0.5], bo, density=0.3, label="zero delta")
    assert rep.thresholds[1] == 0.0 and rep.kept[1] == 0 and rep.kept[0] >= rep.k_keep > 0


def check_opposite_deltas(engine, device="cpu"):
    """exactly opposite deltas with equal weights: S == 0 elects +1, the positive entries survive"""
    d = torch.randn(SMALL, generator=torch.Generator().manual_seed(61)).to(torch.bfloat16).to(device)
    zero = torch.zeros_like(d)
    bo = make_inputs(SMALL, 1, seed=62, device=device)[2]
    check(engine, [d, -d], [zero, zero], [0.5, 0.5], bo, density=1.0, label="opposite deltas")
    out, _, delta = engine.ties_merge([d, -d], [zero, zero], [0.5, 0.5], bo, density=1.0, normalize=True, want_delta=True)
    assert torch.equal(delta.cpu(), d.float().abs().cpu())        # (|d| * 0.5) / 0.5, exact


def check_tiny_weight_sum(engine, device="cpu"):
    """weights that make |D| < 1e-8: D is replaced by 1"""
    x = (torch.randn(SMALL, generator=torch.Generator().manual_seed(63)).abs() + 0.5).to(torch.bfloat16).to(device)
    zero = torch.zeros_like(x)
    bo = make_inputs(SMALL, 1, seed=64, device=device)[2]
    check(engine, [x, -x], [zero, zero], [0.5, -0.5], bo, density=1.0, label="D = 0")        # both agree (+), D = 0.5 - 0.5
    _, _, delta = engine.ties_merge([x, -x], [zero, zero], [0.5, -0.5], bo, density=1.0, want_delta=True)
    assert torch.equal(delta.cpu(), x.float().cpu())              # 0.5 x + 0.5 x over D := 1
    check(engine, [x], [zero], [1e-9], bo, density=0.5, label="D = 1e-9")


def check_ties_exceed_k(engine, device="cpu"):
    """differences of bf16 weights collide: more than k_keep elements reach the threshold, all of them are kept"""
    fts, bases, bo = make_inputs((256, 512), 2, seed=65, sigma=3e-4, device=device)
    rep = check(engine, fts, bases, [0.5, 0.5], bo, density=0.2, label="ties")
    assert all(kept > rep.k_keep for kept in rep.kept), (rep.kept, rep.k_keep)


def check_denormals(engine, device="cpu"):
    g = torch.Generator().manual_seed(66)
    ft = (torch.randn(SMALL, generator=g) * 1e-40).to(device)
    assert 0 < float(ft.abs().max()) < 1.2e-38
    zero = torch.zeros_like(ft)
    check(engine, [ft, ft * 0.5], [zero, zero], [0.5, 0.75], zero, density=0.5, lam=0.7, label="fp32 denormal deltas")
    fb = (torch.randn(SMALL, generator=g) * 1e-39).to(torch.bfloat16).to(device)
    assert 0 < float(fb.float().abs().max()) < 1.2e-38
    bo = make_inputs(SMALL, 1, seed=67, device=device)[2]
    check(engine, [fb], [torch.zeros_like(fb)], [0.5], bo, density=0.5, label="bf16 denormal deltas")
    check(engine, [fb], [torch.zeros_like(fb)], [0.5], torch.zeros_like(fb), density=0.5, label="bf16 denormals onto zero")


def check_unaligned(engine, device="cpu"):
    """views that start at an odd element, and element counts that are not multiples of 8"""
    for dtype in DTYPES:
        for n in (1003, 4096):
            fts, bases, bo = make_inputs((n + 5,), 3, dtype, seed=70, own_bases=True, device=device)
            cut = lambda t, o: t[o:o + n]
            check(engine, [cut(fts[0], 1), cut(fts[1], 3), cut(fts[2], 0)], [cut(bases[0], 0), cut(bases[1], 1), cut(bases[2], 5)],
                  ALPHAS[:3], cut(bo, 1), density=0.2, label=f"unaligned {dtype} n={n}")
    for n in (7, 8, 9, 2049):
        fts, bases, bo = make_inputs((n,), 2, seed=71, device=device)
        check(engine, fts, bases, ALPHAS[:2], bo, density=0.5, label=f"n={n}")


def check_tiny_and_rank3(engine, device="cpu"):
    fts, bases, bo = make_inputs((1,), 2, seed=72, own_bases=True, device=device)
    check(engine, fts, bases, [0.5, 0.5], bo, density=1.0, label="1 element")
    check(engine, fts, bases, [0.5, 0.5], bo, density=0.5, label="1 element, k_keep = 0")
    fts, bases, bo = make_inputs((0,), 2, seed=73, device=device)
    out, rep = engine.ties_merge(fts, bases, [0.5, 0.5], bo)
    assert out.numel() == 0 and out.dtype == bo.dtype and rep.k_keep == 0 and rep.kept == [0, 0]
    fts, bases, bo = make_inputs((4, 33, 65), 3, seed=74, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:3], bo, label="rank 3")


def check_nonfinite(engine, device="cpu"):
    """a NaN / an Inf in one finetune: ValueError naming the tensor and the finetune; the context stays usable"""
    for poison in (float("nan"), float("inf"), float("-inf")):
        fts, bases, bo = make_inputs(SMALL, 3, seed=80, device=device)
        fts[1] = fts[1].clone()
        fts[1].view(-1)[4321] = poison
        with pytest.raises(ValueError, match=r"model\.layers\.7\.mlp\.up_proj\.weight.*finetune 1\b"):
            engine.ties_merge(fts, bases, ALPHAS[:3], bo, layer_name="model.layers.7.mlp.up_proj.weight")
        fts, bases, bo = make_inputs(SMALL, 3, seed=81, device=device)
        check(engine, fts, bases, ALPHAS[:3], bo, label="after an error")
    # Inf - Inf in the delta although no delta element is Inf itself
    fts, bases, bo = make_inputs(SMALL, 2, torch.float32, seed=82, own_bases=True, device=device)
    fts[0].view(-1)[5] = float("inf")
    bases[0].view(-1)[5] = float("inf")
    with pytest.raises(ValueError, match=r"finetune 0\b"):
        engine.ties_merge(fts, bases, ALPHAS[:2], bo)


def check_determinism(engine, device="cpu"):
    fts, bases, bo = make_inputs((300, 500), 3, seed=90, own_bases=True, device=device)
    a, ra = engine.ties_merge(fts, bases, ALPHAS[:3], bo)
    b, rb = engine.ties_merge(fts, bases, ALPHAS[:3], bo)
    assert torch.equal(raw(a), raw(b)) and ra == rb


def check_arguments(engine, device="cpu"):
    fts, bases, bo = make_inputs((8, 8), 2, seed=91, device=device)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="density"):
            engine.ties_merge(fts, bases, [0.5, 0.5], bo, density=bad)
    with pytest.raises(ValueError, match="shape mismatch"):
        engine.ties_merge([fts[0], fts[1][:4]], bases, [0.5, 0.5], bo)
    with pytest.raises(ValueError, match="supported range"):
        engine.ties_merge([fts[0]] * 17, [bases[0]] * 17, [0.1] * 17, bo)
    with pytest.raises(ValueError, match="alphas"):
        engine.ties_merge(fts, bases, [0.5], bo)


# ---- the CLI on the synthetic on-disk model of tests/lora_fixtures.py ----------------------------------------
OPTIONS = {"operator": "ties", "density": 0.3, "ties_lambda": 0.7}


def write_config(root, third, out_dir, options=OPTIONS, device=None):
    return harness.write_config(root, ties_models(third), out_dir, options, device)


def expected_outputs(base, full, options=OPTIONS):
    """the oracle tensor by tensor (block tensors) / the provider's tensor (passthrough)"""
    def merge(fts, bases, alphas, base_out, name):
        return ties_oracle.ties_merge(
            fts, bases, alphas, base_out, options.get("density", 0.2), options.get("ties_lambda", 1.0),
            bool(options.get("ties_normalize", 1)))[0]

    return expected_by_tensor(base, full, ties_models("org/lora_full"), merge)
