"""Checks of the SCE operator shared by the emulator tier (tests/test_sce_host.py) and the GPU tier
(tests/test_sce_gpu.py): Engine.sce_merge against tests/sce_oracle.py, BIT FOR BIT - output, merged delta, nz, k_keep,
the selected count, the threshold's bits, the energies as doubles and the weights' bits.  The tolerance is zero and it is
derived, not measured: every step of the function is one correctly rounded operation or an exact order statistic, in an
order that the header writes out (include/shardmerge_hip.h, smhip_sce_merge)."""
import numpy as np
import pytest
import torch

from tests import harness
from tests import sce_oracle
from tests.harness import ALPHAS, DTYPES, SMALL, expected_by_tensor, f32_bits, f64_bits, make_inputs, raw, ties_models

TOPKS = (1.0, 0.5, 0.1, 0.01, 1e-9)              # the last one: k_keep == 0, the output is base_out
# unequal alphas with one alpha of 0 (SCE takes alphas >= 0)
SCE_ALPHAS = (0.5, 0.0, 0.4, 0.25, 0.6, 0.1, 0.35, 0.45, 0.2, 0.15, 0.55, 0.05, 0.7, 0.3, 0.5, 0.4)
SIZES = (1, 7, 8, 9, 32767, 32768, 32769, 3 * 32768 + 5)     # the octet and segment boundaries of the energy order


def check(engine, fts, bases, alphas, base_out, select_topk=1.0, lam=1.0, label=""):
    """one call against the oracle, bit for bit; returns (the engine's report, the oracle's dict)"""
    out, rep, delta = engine.sce_merge(fts, bases, alphas, base_out, select_topk=select_topk, lam=lam, want_delta=True)
    cpu = lambda ts: [t.cpu() for t in ts]
    ref = sce_oracle.sce_merge(cpu(fts), cpu(bases), alphas, base_out.cpu(), select_topk, lam)
    k = len(fts)
    print(f"{label}: nz {rep.nz} / {ref['nz']}, k_keep {rep.k_keep} / {ref['k_keep']}, selected {rep.selected} / {ref['selected']}, "
          f"threshold {rep.threshold!r} / {ref['threshold']!r}, energies {rep.energies} / {ref['energy']}, weights {rep.weights} / {ref['weight']}")
    assert out.dtype == base_out.dtype and out.shape == base_out.shape, label
    assert (rep.nz, rep.k_keep, rep.selected) == (ref["nz"], ref["k_keep"], ref["selected"]), label
    assert f32_bits(rep.threshold) == f32_bits(ref["threshold"]), (label, rep.threshold, ref["threshold"])
    assert [f64_bits(e) for e in rep.energies] == [f64_bits(e) for e in ref["energy"]], (label, rep.energies, ref["energy"])
    assert [f32_bits(w) for w in rep.weights] == [f32_bits(w) for w in ref["weight"]], (label, rep.weights, ref["weight"])
    assert len(rep.energies) == k and len(rep.weights) == k
    bad = int((raw(delta) != raw(ref["delta"])).sum())
    assert bad == 0, f"{label}: {bad} of {ref['delta'].numel()} merged-delta values differ in their bits"
    bad = int((raw(out) != raw(ref["out"])).sum())
    assert bad == 0, f"{label}: {bad} of {ref['out'].numel()} output values differ in their bits"
    return rep, ref


# ---- the parameter grid -------------------------------------------------------------------------------
def check_dtypes(engine, in_dtype, bo_dtype, device="cpu"):
    fts, bases, bo = make_inputs(SMALL, 3, in_dtype, bo_dtype, seed=11, own_bases=True, device=device)
    check(engine, fts, bases, SCE_ALPHAS[:3], bo, select_topk=0.1, lam=0.7, label=f"{in_dtype}->{bo_dtype}")
    fts, bases, bo = make_inputs(SMALL, 2, in_dtype, bo_dtype, seed=12, device=device)      # one shared base
    check(engine, fts, bases, ALPHAS[:2], bo, select_topk=0.5, label=f"{in_dtype}->{bo_dtype} shared")
    check(engine, fts, bases, ALPHAS[:2], bo, select_topk=1.0, label=f"{in_dtype}->{bo_dtype} shared, no selection")


def check_k_topk(engine, k, topk, device="cpu"):
    """k = 1, 2, 3 (four deltas per octet in registers) and 5, 16 (sixteen); shared bases with lambda 1, own with 0.7"""
    for j, lam in enumerate((1.0, 0.7)):
        fts, bases, bo = make_inputs(SMALL, k, seed=20 + k + j, own_bases=bool(j), device=device)
        alphas = SCE_ALPHAS[:k] if k > 1 else (0.3,)
        rep, ref = check(engine, fts, bases, alphas, bo, select_topk=topk, lam=lam, label=f"k={k} select_topk={topk} lam={lam} own={bool(j)}")
        n = bo.numel()
        if topk == 1.0 or k == 1:                  # the selection is skipped
            assert (rep.nz, rep.k_keep, rep.selected, rep.threshold) == (n, n, n, 0.0)
        elif topk == 1e-9:
            assert rep.k_keep == 0 and rep.selected == 0 and rep.threshold == float("inf") and 0 < rep.nz <= n
            out, _ = engine.sce_merge(fts, bases, alphas, bo, select_topk=topk, lam=lam)
            assert torch.equal(raw(out), raw(bo))
            assert rep.energies == [0.0] * k and [f32_bits(w) for w in rep.weights] == [f32_bits(np.float32(1.0 / k))] * k
        else:
            assert rep.selected >= rep.k_keep > 0 and rep.threshold > 0
        if k == 1:
            assert rep.weights == [1.0]


def check_sizes(engine, n, device="cpu"):
    """element counts around the octet and the 32768-element segment of the energy order, with and without selection"""
    for k, own in ((2, False), (3, True)):
        fts, bases, bo = make_inputs((n,), k, seed=30 + k, own_bases=own, device=device)
        for topk in (0.5, 1.0):
            check(engine, fts, bases, ALPHAS[:k], bo, select_topk=topk, lam=0.7, label=f"n={n} k={k} select_topk={topk}")
    fts, bases, bo = make_inputs((n,), 5, seed=35, device=device)
    check(engine, fts, bases, ALPHAS[:5], bo, select_topk=0.5, label=f"n={n} k=5")


# ---- corners ----------------------------------------------------------------------------------------------
def check_unaligned(engine, device="cpu"):
    """views that start at an odd element"""
    for dtype in DTYPES:
        for n in (1003, 4096):
            fts, bases, bo = make_inputs((n + 5,), 3, dtype, seed=70, own_bases=True, device=device)
            cut = lambda t, o: t[o:o + n]
            for topk in (0.2, 1.0):
                check(engine, [cut(fts[0], 1), cut(fts[1], 3), cut(fts[2], 0)], [cut(bases[0], 0), cut(bases[1], 1), cut(bases[2], 5)],
                      ALPHAS[:3], cut(bo, 1), select_topk=topk, label=f"unaligned {dtype} n={n} select_topk={topk}")


def check_rank3_and_empty(engine, device="cpu"):
    fts, bases, bo = make_inputs((4, 33, 65), 3, seed=74, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:3], bo, select_topk=0.3, label="rank 3")
    check(engine, fts, bases, ALPHAS[:3], bo, select_topk=1.0, label="rank 3, no selection")
    fts, bases, bo = make_inputs((0,), 2, seed=73, device=device)
    for topk, tau in ((0.5, float("inf")), (1.0, 0.0)):
        out, rep = engine.sce_merge(fts, bases, [0.5, 0.5], bo, select_topk=topk)
        assert out.numel() == 0 and out.dtype == bo.dtype
        assert (rep.nz, rep.k_keep, rep.selected, rep.threshold, rep.energies, rep.weights) == (0, 0, 0, tau, [0.0, 0.0], [0.5, 0.5])


def check_zero_delta(engine, device="cpu"):
    """a finetune equal to its base: its energy is 0 and so is its weight; the other's is 1"""
    fts, bases, bo = make_inputs(SMALL, 2, seed=60, device=device)
    fts[1] = bases[1].clone()
    for topk in (0.3, 1.0):
        rep, _ = check(engine, fts, bases, [0.5, 0.5], bo, select_topk=topk, label=f"zero delta select_topk={topk}")
        assert rep.energies[1] == 0.0 and rep.weights == [1.0, 0.0] and rep.energies[0] > 0.0


def check_all_equal(engine, device="cpu"):
    """all finetunes equal: every deviation is 0, q == 0 everywhere, nz == 0, nothing is selected, the output is base_out"""
    fts, bases, bo = make_inputs(SMALL, 1, seed=61, device=device)
    for k in (2, 3, 5):
        rep, _ = check(engine, [fts[0]] * k, [bases[0]] * k, ALPHAS[:k], bo, select_topk=0.5, label=f"all equal k={k}")
        assert (rep.nz, rep.k_keep, rep.selected, rep.threshold) == (0, 0, 0, float("inf"))
        out, _ = engine.sce_merge([fts[0]] * k, [bases[0]] * k, ALPHAS[:k], bo, select_topk=0.5)
        assert torch.equal(raw(out), raw(bo))


def check_nz_rule(engine, device="cpu"):
    """k = 2 on bf16 inputs with a shared base: some elements have equal deltas, q == 0 there, and k_keep counts by nz"""
    fts, bases, bo = make_inputs(SMALL, 2, torch.bfloat16, seed=12, device=device)
    rep, _ = check(engine, fts, bases, [0.5, 0.5], bo, select_topk=0.1, label="nz rule")
    n = bo.numel()
    assert 0 < rep.nz < n, (rep.nz, n)
    assert rep.k_keep == int(0.1 * rep.nz)


def check_ties_exceed_k(engine, device="cpu"):
    """scores on a coarse grid: d_0 = -d_1 = j * 2^-10 with j in 0..7 gives q = 2 d_0^2, eight distinct values over 4096
    elements, so far more elements tie at tau than k_keep asks for - all of them are selected"""
    j = (torch.arange(4096) % 8).float()
    d = (j * 2.0 ** -10).to(torch.bfloat16).to(device)
    zero = torch.zeros_like(d)
    bo = make_inputs((4096,), 1, seed=65, device=device)[2]
    rep, _ = check(engine, [d, -d], [zero, zero], [0.5, 0.5], bo, select_topk=0.2, label="ties at tau")
    assert rep.nz == 4096 - 512 and rep.k_keep == int(0.2 * rep.nz)
    assert rep.selected == 1024 > rep.k_keep, (rep.selected, rep.k_keep)          # j = 7 and j = 6: 512 each
    fts, bases, bo = make_inputs((256, 512), 2, seed=65, sigma=3e-4, device=device)          # differences of bf16 weights collide
    rep, _ = check(engine, fts, bases, [0.5, 0.5], bo, select_topk=0.2, label="ties at tau, random")
    assert rep.selected > rep.k_keep, (rep.selected, rep.k_keep)


def check_opposite_deltas(engine, device="cpu"):
    """exactly opposite deltas: the mean is 0, q = 2 d^2, S == 0 elects +1, the positive entries survive alone: the merged
    delta is |d| w / w = |d| (w = 1/2: the energies are equal)"""
    d = torch.randn(SMALL, generator=torch.Generator().manual_seed(61)).to(torch.bfloat16).to(device)
    zero = torch.zeros_like(d)
    bo = make_inputs(SMALL, 1, seed=62, device=device)[2]
    for topk in (1.0, 0.5):
        rep, ref = check(engine, [d, -d], [zero, zero], [0.5, 0.5], bo, select_topk=topk, label=f"opposite deltas select_topk={topk}")
        assert rep.weights == [0.5, 0.5] and rep.energies[0] == rep.energies[1]
        _, _, delta = engine.sce_merge([d, -d], [zero, zero], [0.5, 0.5], bo, select_topk=topk, want_delta=True)
        want = torch.where(ref["mask"].view(SMALL), d.float().abs().cpu(), torch.zeros(()))
        assert torch.equal(delta.cpu(), want)


def check_denormals(engine, device="cpu"):
    g = torch.Generator().manual_seed(66)
    ft = (torch.randn(SMALL, generator=g) * 1e-20).to(device)                 # squares of deviations are denormal or 0
    zero = torch.zeros_like(ft)
    check(engine, [ft, ft * 0.5], [zero, zero], [0.5, 0.75], zero, select_topk=0.5, lam=0.7, label="fp32, denormal scores")
    ft = (torch.randn(SMALL, generator=g) * 1e-40).to(device)
    assert 0 < float(ft.abs().max()) < 1.2e-38
    rep, _ = check(engine, [ft, ft * 0.5], [zero, zero], [0.5, 0.75], zero, select_topk=0.5, lam=0.7, label="fp32 denormal deltas")
    assert rep.nz == 0                                                        # every square underflows to 0
    check(engine, [ft, ft * 0.5], [zero, zero], [0.5, 0.75], zero, select_topk=1.0, label="fp32 denormal deltas, no selection")
    fb = (torch.randn(SMALL, generator=g) * 1e-39).to(torch.bfloat16).to(device)
    assert 0 < float(fb.float().abs().max()) < 1.2e-38
    bo = make_inputs(SMALL, 1, seed=67, device=device)[2]
    check(engine, [fb, -fb], [torch.zeros_like(fb)] * 2, [0.5, 0.5], bo, select_topk=1.0, label="bf16 denormal deltas")


def check_overflowing_scores(engine, device="cpu"):
    """deltas near 1e20: the squares overflow to +inf, an ordinary score that sorts above all others; the energies are
    finite in fp64"""
    g = torch.Generator().manual_seed(68)
    a = (torch.randn(SMALL, generator=g) * 1e20).to(device)
    b = (torch.randn(SMALL, generator=g) * 1e10).to(device)
    zero = torch.zeros_like(a)
    rep, _ = check(engine, [a, b], [zero, zero], [0.5, 0.5], zero, select_topk=0.5, label="overflowing scores")
    assert rep.threshold == float("inf") and rep.selected >= rep.k_keep > 0


def check_nonfinite(engine, device="cpu"):
    """a NaN / an Inf in one finetune: ValueError naming the tensor and the finetune; the context stays usable"""
    for topk in (0.5, 1.0):
        for poison in (float("nan"), float("inf"), float("-inf")):
            fts, bases, bo = make_inputs(SMALL, 3, seed=80, device=device)
            fts[1] = fts[1].clone()
            fts[1].view(-1)[4321] = poison
            with pytest.raises(ValueError, match=r"model\.layers\.7\.mlp\.up_proj\.weight.*finetune 1\b"):
                engine.sce_merge(fts, bases, ALPHAS[:3], bo, select_topk=topk, layer_name="model.layers.7.mlp.up_proj.weight")
        fts, bases, bo = make_inputs(SMALL, 3, seed=81, device=device)
        check(engine, fts, bases, ALPHAS[:3], bo, select_topk=topk, label="after an error")
    # Inf - Inf in the delta although no delta element is Inf itself
    fts, bases, bo = make_inputs(SMALL, 2, torch.float32, seed=82, own_bases=True, device=device)
    fts[0].view(-1)[5] = float("inf")
    bases[0].view(-1)[5] = float("inf")
    with pytest.raises(ValueError, match=r"finetune 0\b"):
        engine.sce_merge(fts, bases, ALPHAS[:2], bo, select_topk=0.5)
    fts, bases, bo = make_inputs(SMALL, 5, seed=83, device=device)
    fts[4] = fts[4].clone()
    fts[4].view(-1)[12706] = float("nan")
    with pytest.raises(ValueError, match=r"finetune 4\b"):
        engine.sce_merge(fts, bases, ALPHAS[:5], bo, select_topk=0.5)


def check_determinism(engine, device="cpu"):
    fts, bases, bo = make_inputs((300, 500), 3, seed=90, own_bases=True, device=device)
    for topk in (0.1, 1.0):
        a, ra = engine.sce_merge(fts, bases, ALPHAS[:3], bo, select_topk=topk)
        b, rb = engine.sce_merge(fts, bases, ALPHAS[:3], bo, select_topk=topk)
        assert torch.equal(raw(a), raw(b)) and ra == rb


def check_arguments(engine, device="cpu"):
    fts, bases, bo = make_inputs((8, 8), 2, seed=91, device=device)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="select_topk"):
            engine.sce_merge(fts, bases, [0.5, 0.5], bo, select_topk=bad)
    for alphas in ([-0.5, 1.0], [0.0, 0.0], [float("nan"), 1.0], [float("inf"), 1.0]):
        with pytest.raises(ValueError, match="alphas"):
            engine.sce_merge(fts, bases, alphas, bo)
    with pytest.raises(ValueError, match="lam"):
        engine.sce_merge(fts, bases, [0.5, 0.5], bo, lam=float("inf"))
    with pytest.raises(ValueError, match="shape mismatch"):
        engine.sce_merge([fts[0], fts[1][:4]], bases, [0.5, 0.5], bo)
    with pytest.raises(ValueError, match="supported range"):
        engine.sce_merge([fts[0]] * 17, [bases[0]] * 17, [0.1] * 17, bo)
    with pytest.raises(ValueError, match="alphas"):
        engine.sce_merge(fts, bases, [0.5], bo)


# ---- properties that need no oracle ------------------------------------------------------------------------
def check_power_of_two_scaling(engine, device="cpu"):
    """zero bases and bf16 deltas d_i: the call on 2 d_i gives the same selected count and weight bits, a threshold of
    exactly 4 tau and a merged delta of exactly twice the first (every step commutes with a power of two: no overflow, no
    underflow at these magnitudes; the energies scale by 4 exactly and P_i / Z keeps its bits)"""
    fts, bases, _ = make_inputs(SMALL, 3, torch.bfloat16, seed=92, device=device)
    ds = [(f.float() - b.float()).to(torch.bfloat16) for f, b in zip(fts, bases)]
    zero = torch.zeros_like(ds[0])
    for topk in (0.1, 1.0):
        _, rep, delta = engine.sce_merge(ds, [zero] * 3, ALPHAS[:3], zero, select_topk=topk, want_delta=True)
        _, rep2, delta2 = engine.sce_merge([d * 2 for d in ds], [zero] * 3, ALPHAS[:3], zero, select_topk=topk, want_delta=True)
        assert [f32_bits(w) for w in rep2.weights] == [f32_bits(w) for w in rep.weights]
        assert (rep2.nz, rep2.k_keep, rep2.selected) == (rep.nz, rep.k_keep, rep.selected)
        assert rep2.threshold == 4.0 * rep.threshold and rep2.energies == [4.0 * e for e in rep.energies]
        assert torch.equal(raw(delta2), raw(delta * 2.0))


def check_nested_selection(engine, device="cpu"):
    """the selected sets are nested in select_topk: where a smaller share merges something, so does every larger one"""
    fts, bases, bo = make_inputs(SMALL, 3, seed=93, device=device)
    zero_bo = torch.zeros_like(bo)
    prev, prev_sel = None, 0
    for topk in (0.01, 0.1, 0.5, 0.9):
        _, rep, delta = engine.sce_merge(fts, bases, [1.0, 1.0, 1.0], zero_bo, select_topk=topk, want_delta=True)
        cpu = [t.cpu() for t in fts], [t.cpu() for t in bases]
        mask = sce_oracle.select(sce_oracle.deltas(*cpu), topk)[0]
        assert int(mask.sum()) == rep.selected >= prev_sel
        assert not bool((delta.cpu().view(-1) != 0)[~mask].any())            # nothing outside the selection is merged
        if prev is not None:
            assert bool((mask | ~prev).all())                                # prev is a subset of mask
        prev, prev_sel = mask, rep.selected


PROPERTIES = [check_power_of_two_scaling, check_nested_selection]
CORNERS = [check_unaligned, check_rank3_and_empty, check_zero_delta, check_all_equal, check_nz_rule, check_ties_exceed_k,
           check_opposite_deltas, check_denormals, check_overflowing_scores, check_nonfinite, check_determinism, check_arguments]


def check_profile(engine, k, topk, shape=(40, 50), device="cpu"):
    """profile names and launch counts: three levels of ONE selection stream whatever k, none when it is skipped"""
    fts, bases, bo = make_inputs(shape, k, seed=6, device=device)
    engine.ctx.profile(True)
    engine.ctx.profile_reset()
    try:
        engine.sce_merge(fts, bases, ALPHAS[:k], bo, select_topk=topk)
        table = engine.ctx.profile_table()
    finally:
        engine.ctx.profile(False)
    expected = {"sce_energy": 1, "sce_energy_fold": 1, "sce_merge": 1}
    if topk != 1.0 and k > 1:
        expected.update({"sce_hist": 3, "sce_select": 3})
    assert {n: table[n][0] for n in table} == expected


# ---- the CLI on the synthetic on-disk model of tests/lora_fixtures.py ----------------------------------------
OPTIONS = {"operator": "sce", "select_topk": 0.3, "sce_lambda": 0.7}
README_WORDS = ("# SCE Merged Model", "SCE (sce:", "select_topk 0.3", "sce_lambda 0.7")


def write_config(root, third, out_dir, options=OPTIONS, device=None):
    return harness.write_config(root, ties_models(third), out_dir, options, device)


def expected_outputs(base, full, options=OPTIONS):
    """the oracle tensor by tensor (block tensors) / the provider's tensor (passthrough)"""
    def merge(fts, bases, alphas, base_out, name):
        return sce_oracle.sce_merge(
            fts, bases, alphas, base_out, options.get("select_topk", 1.0), options.get("sce_lambda", 1.0))["out"]

    return expected_by_tensor(base, full, ties_models("org/lora_full"), merge)
