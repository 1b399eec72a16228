"""Checks of the PCB operator shared by the emulator tier (tests/test_pcb_host.py) and the GPU tier
(tests/test_pcb_gpu.py): Engine.pcb_merge against tests/pcb_oracle.py, BIT FOR BIT - output, merged delta, lo, hi, t, M
and every count.  The tolerance is zero and it is derived, not measured: every step of the function is one correctly
rounded operation, an exact order statistic or an integer count in a stated order (include/shardmerge_hip.h,
smhip_pcb_merge).  sm_tanh is held to 2^-48 of mpmath's tanh: sm_exp's 2^-52 times the cancellation factor
(1 + e) / (1 - e) <= 16 at the branch point 2^-4.  The function as a whole is held to a torch fp64 restatement of the
paper's form (exp(k s^2) with the factor e^k, torch.tanh clamped at 0, min-max normalisation) in quotient form."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import harness
from tests import pcb_oracle
from tests.harness import ALPHAS, expected_by_tensor, f32_bits, make_inputs, profile_of, raw, ties_models

KS = (1, 2, 3, 4, 5, 16)                        # 4 | 5 straddles the two register variants of the kernels
RATIOS = (0.1, 0.5, 1.0, 1e-9)                  # the last one: q = 1
CLIPS = (0.0, 1e-4, 0.01)                       # r = 0, 0 and 47 at SHAPE
LAMBDAS = (1.0, 0.7)
SHAPE = (37, 129)                               # 4773 elements: unaligned rows and a tail octet
# around one octet, around the span of one work-group of pcb_merge (256 threads x 2 octets) and of a *_hist launch
# (256 x 4 octets), and several work-groups with a tail
SIZES = (1, 7, 8, 9, 4095, 4096, 4097, 8191, 8192, 8193, 2 ** 16 + 5)
EPS = 2.0 ** -24


def check(engine, fts, bases, alphas, base_out, ratio=0.1, clip=1e-4, lam=1.0, label=""):
    """one call against the oracle, bit for bit, and the invariants of the report; returns (report, out, delta, oracle)"""
    kw = dict(ratio=ratio, clip=clip, lam=lam)
    out, rep, delta = engine.pcb_merge(fts, bases, alphas, base_out, want_delta=True, **kw)
    cpu = lambda ts: [t.cpu() for t in ts]
    ref = pcb_oracle.pcb_merge(cpu(fts), cpu(bases), alphas, base_out.cpu(), **kw)
    k, n = len(fts), base_out.numel()
    print(f"{label}: covered {rep.covered} / {ref['covered']}, contested {rep.contested} / {ref['contested']}, "
          f"selected {rep.selected} / {ref['selected']}, positive {rep.positive} / {ref['positive']}, t {rep.t}, M {rep.M}")
    assert out.dtype == base_out.dtype and out.shape == base_out.shape, label
    assert (rep.n, rep.clip_rank, rep.q) == (n, ref["clip_rank"], ref["q"]), (label, rep, ref["clip_rank"], ref["q"])
    for name in ("lo", "hi", "t", "M"):
        got, want = [f32_bits(v) for v in getattr(rep, name)], [f32_bits(float(v)) for v in ref[name]]
        assert got == want, (label, name, getattr(rep, name), ref[name])
    assert rep.positive == ref["positive"], (label, rep.positive, ref["positive"])
    assert rep.selected == ref["selected"], (label, rep.selected, ref["selected"])
    assert rep.covered == ref["covered"] and rep.contested == ref["contested"], (label, rep.covered, rep.contested, ref["covered"], ref["contested"])
    # the invariants
    for i in range(k):
        assert 0.0 <= rep.lo[i] <= rep.hi[i] and 0.0 <= rep.t[i] <= rep.M[i], (label, i, rep)
        assert min(rep.q, rep.positive[i]) <= rep.selected[i] <= rep.positive[i] <= n, (label, i, rep)
        assert (rep.t[i] == 0.0) == (rep.positive[i] < rep.q), (label, i, rep)
    assert rep.contested <= rep.covered <= n, (label, rep)
    bad = int((raw(delta) != raw(ref["delta"])).sum())
    assert bad == 0, f"{label}: {bad} of {n} merged-delta values differ in their bits"
    bad = int((raw(out) != raw(ref["out"])).sum())
    assert bad == 0, f"{label}: {bad} of {n} output values differ in their bits"
    return rep, out, delta, ref


# ---- the parameter grid -------------------------------------------------------------------------------
def check_dtypes(engine, in_dtype, bo_dtype, device="cpu"):
    fts, bases, bo = make_inputs(SHAPE, 3, in_dtype, bo_dtype, seed=11, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:3], bo, ratio=0.3, lam=0.7, label=f"{in_dtype}->{bo_dtype}")
    fts, bases, bo = make_inputs(SHAPE, 2, in_dtype, bo_dtype, seed=12, device=device)      # one shared base
    check(engine, fts, bases, ALPHAS[:2], bo, ratio=0.5, clip=0.01, label=f"{in_dtype}->{bo_dtype} shared")


def check_k(engine, k, own, device="cpu"):
    fts, bases, bo = make_inputs(SHAPE, k, seed=20 + k, own_bases=own, device=device)
    rep, _, _, _ = check(engine, fts, bases, ALPHAS[:k], bo, ratio=0.2, clip=0.001, label=f"k={k} own={own}")
    assert 0 < rep.covered < rep.n and (k == 1 or rep.contested > 0)
    if k == 1:                                  # tv U = tv^2: every nonzero entry agrees with the sum
        assert rep.contested == 0 and rep.selected[0] >= rep.q


def check_options(engine, ratio, clip, lam, device="cpu"):
    fts, bases, bo = make_inputs(SHAPE, 3, seed=40, own_bases=True, device=device)
    rep, _, _, _ = check(engine, fts, bases, ALPHAS[:3], bo, ratio=ratio, clip=clip, lam=lam, label=f"ratio={ratio} clip={clip} lam={lam}")
    n = bo.numel()
    assert rep.q == (1 if ratio == 1e-9 else int(math.floor(ratio * n))) and rep.clip_rank == (47 if clip == 0.01 else 0)
    if ratio == 1.0:                            # more asked than score above 0: the cut is 0 and every positive entry is selected
        assert all(t == 0.0 for t in rep.t) and rep.selected == rep.positive and all(p < n for p in rep.positive)


def check_size(engine, n, device="cpu"):
    for k in (2, 5):
        fts, bases, bo = make_inputs((n,), k, seed=70 + k, device=device)
        check(engine, fts, bases, ALPHAS[:k], bo, ratio=0.3, clip=0.01, label=f"n={n} k={k}")


# ---- corners ----------------------------------------------------------------------------------------------
def check_unaligned(engine, device="cpu"):
    """views of 16-bit tensors that start 2 bytes off a 16-byte boundary: the element-wise path of the loader and the store"""
    for dtype in (torch.bfloat16, torch.float16):
        for n in (1003, 2048):
            fts, bases, bo = make_inputs((n + 5,), 3, dtype, seed=71, own_bases=True, device=device)
            cut = lambda t, o: t[o:o + n]
            check(engine, [cut(fts[0], 1), cut(fts[1], 3), cut(fts[2], 0)], [cut(bases[0], 0), cut(bases[1], 1), cut(bases[2], 5)],
                  ALPHAS[:3], cut(bo, 1), ratio=0.3, label=f"unaligned {dtype} n={n}")


def check_bases(engine, device="cpu"):
    """a base per finetune; one shared base that is also base_out (loaded once)"""
    for k in (3, 5):
        fts, bases, bo = make_inputs(SHAPE, k, seed=50 + k, own_bases=True, device=device)
        check(engine, fts, bases, ALPHAS[:k], bo, ratio=0.3, label=f"own bases k={k}")
        fts, bases, bo = make_inputs(SHAPE, k, seed=52 + k, device=device)
        assert bo is bases[0] and all(b is bases[0] for b in bases)
        check(engine, fts, bases, ALPHAS[:k], bo, ratio=0.3, label=f"out_is_base0 k={k}")


def check_signed_alphas(engine, device="cpu"):
    """negative and zero weights: a zero weight leaves lo = hi = 0 and no positive score; a zero sum is no error"""
    fts, bases, bo = make_inputs(SHAPE, 4, seed=55, own_bases=True, device=device)
    rep, _, _, _ = check(engine, fts, bases, [0.5, -0.3, 0.0, -0.7], bo, ratio=0.5, clip=0.01, lam=0.7, label="signed alphas")
    assert (rep.lo[2], rep.hi[2], rep.positive[2], rep.selected[2]) == (0.0, 0.0, 0, 0)
    check(engine, fts, bases, [-0.5, -0.3, -0.2, -0.7], bo, ratio=0.3, lam=-0.7, label="negative alphas")
    check(engine, fts[:2], bases[:2], [0.5, -0.5], bo, ratio=0.3, label="alphas that sum to zero")


def check_tied_deltas(engine, device="cpu"):
    """differences of bf16 weights collide heavily: ties at lo, hi, t and M"""
    fts, bases, bo = make_inputs((64, 512), 3, seed=65, sigma=3e-4, device=device)
    rep, _, _, _ = check(engine, fts, bases, ALPHAS[:3], bo, ratio=0.2, clip=0.05, label="tied bf16 deltas")
    assert all(s >= rep.q for s in rep.selected)


def check_zero_finetune(engine, device="cpu"):
    """a finetune equal to its base: hi == lo == 0, no score above 0, the others merge as if it were not there"""
    fts, bases, bo = make_inputs(SHAPE, 3, seed=60, device=device)
    fts[1] = bases[1].clone()
    rep, _, delta, _ = check(engine, fts, bases, ALPHAS[:3], bo, ratio=0.3, label="one zero delta")
    assert (rep.lo[1], rep.hi[1], rep.t[1], rep.M[1], rep.positive[1], rep.selected[1]) == (0.0, 0.0, 0.0, 0.0, 0, 0)
    for k in (2, 5):                            # all of them: the output is base_out
        fts, bases, bo = make_inputs(SHAPE, k, seed=61, device=device)
        rep, out, delta, _ = check(engine, [b.clone() for b in bases], bases, ALPHAS[:k], bo, label="zero deltas")
        assert rep.covered == 0 and rep.positive == [0] * k and rep.hi == [0.0] * k
        assert torch.equal(raw(out), raw(bo)) and not bool(delta.any())


def check_constant_magnitude(engine, device="cpu"):
    """one finetune whose delta is +-c everywhere: hi == lo, every score is the same, M == t, every weight is 1"""
    g = torch.Generator().manual_seed(62)
    sign = torch.where(torch.rand(SHAPE, generator=g) < 0.5, -1.0, 1.0)
    d = (sign * 0.00390625).to(torch.bfloat16).to(device)
    zero = torch.zeros_like(d)
    bo = make_inputs(SHAPE, 1, seed=63, device=device)[2]
    rep, _, delta, _ = check(engine, [d], [zero], [0.5], bo, ratio=0.1, label="constant magnitude")
    n = bo.numel()
    assert rep.lo == rep.hi and rep.t == rep.M and rep.M[0] > 0 and rep.selected == [n] and rep.covered == n
    assert torch.equal(delta.cpu(), d.float().cpu() * 0.5)


def check_denormals(engine, device="cpu"):
    """deltas so small that every score falls under 2^-126: nothing is selected, whatever the denormal mode"""
    g = torch.Generator().manual_seed(66)
    ft = (torch.randn(SHAPE, generator=g) * 1e-30).to(device)
    zero = torch.zeros_like(ft)
    rep, out, _, _ = check(engine, [ft, ft * 0.5], [zero, zero], [0.5, 0.75], zero, ratio=0.5, label="scores under 2^-126")
    assert rep.positive == [0, 0] and rep.covered == 0 and not bool(out.any())
    fd = (torch.randn(SHAPE, generator=g) * 1e-40).to(device)
    assert 0 < float(fd.abs().max()) < 1.2e-38
    check(engine, [fd, -fd], [zero, zero], [0.5, 0.25], zero, ratio=0.5, label="fp32 denormal deltas")


def check_nonfinite(engine, device="cpu"):
    """a NaN / an Inf in one finetune: ValueError naming the tensor and the finetune; the context stays usable"""
    for k, poison in ((3, float("inf")), (5, float("nan")), (3, float("-inf"))):
        fts, bases, bo = make_inputs(SHAPE, k, seed=80, device=device)
        fts[1] = fts[1].clone()
        fts[1].view(-1)[4321] = poison
        with pytest.raises(ValueError, match=r"model\.layers\.7\.mlp\.up_proj\.weight.*finetune 1\b"):
            engine.pcb_merge(fts, bases, ALPHAS[:k], bo, layer_name="model.layers.7.mlp.up_proj.weight")
        fts, bases, bo = make_inputs(SHAPE, k, seed=81, device=device)
        check(engine, fts, bases, ALPHAS[:k], bo, label="after an error")


def check_tiny_and_rank3(engine, device="cpu"):
    fts, bases, bo = make_inputs((0,), 2, seed=73, device=device)
    out, rep = engine.pcb_merge(fts, bases, [0.5, 0.5], bo)
    assert out.numel() == 0 and out.dtype == bo.dtype and rep.covered == 0 and rep.selected == [0, 0] and rep.q == 0
    fts, bases, bo = make_inputs((4, 33, 65), 3, seed=74, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:3], bo, ratio=0.3, label="rank 3")


def check_determinism(engine, device="cpu"):
    fts, bases, bo = make_inputs((300, 500), 3, seed=90, own_bases=True, device=device)
    a, ra = engine.pcb_merge(fts, bases, ALPHAS[:3], bo)
    b, rb = engine.pcb_merge(fts, bases, ALPHAS[:3], bo)
    assert torch.equal(raw(a), raw(b)) and ra == rb


def check_arguments(engine, device="cpu"):
    fts, bases, bo = make_inputs((8, 8), 2, seed=91, device=device)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ratio"):
            engine.pcb_merge(fts, bases, [0.5, 0.5], bo, ratio=bad)
    for bad in (-0.1, 0.5, 1.0, float("nan")):
        with pytest.raises(ValueError, match="clip"):
            engine.pcb_merge(fts, bases, [0.5, 0.5], bo, clip=bad)
    with pytest.raises(ValueError, match="lam"):
        engine.pcb_merge(fts, bases, [0.5, 0.5], bo, lam=float("inf"))
    with pytest.raises(ValueError, match="shape mismatch"):
        engine.pcb_merge([fts[0], fts[1][:4]], bases, [0.5, 0.5], bo)
    with pytest.raises(ValueError, match="supported range"):
        engine.pcb_merge([fts[0]] * 17, [bases[0]] * 17, [0.1] * 17, bo)
    with pytest.raises(ValueError, match="alphas"):
        engine.pcb_merge(fts, bases, [0.5], bo)


# ---- properties, through the engine alone ---------------------------------------------------------------------
def check_swap(engine, device="cpu"):
    """k = 2: two-term fp32 sums commute, so the order of the entries does not show in a single byte"""
    for own in (False, True):
        fts, bases, bo = make_inputs(SHAPE, 2, seed=100, own_bases=own, device=device)
        a, ra, da = engine.pcb_merge(fts, bases, [0.5, 0.3], bo, ratio=0.3, clip=0.01, want_delta=True)
        b, rb, db = engine.pcb_merge(fts[::-1], bases[::-1], [0.3, 0.5], bo, ratio=0.3, clip=0.01, want_delta=True)
        assert torch.equal(raw(a), raw(b)) and torch.equal(raw(da), raw(db))
        assert (ra.covered, ra.contested, ra.selected, ra.t) == (rb.covered, rb.contested, rb.selected[::-1], rb.t[::-1])


def check_nested_in_ratio(engine, device="cpu"):
    """the cut falls and the selected sets grow with pcb_ratio; positive[i] does not depend on it"""
    ratios = (0.01, 0.1, 0.3, 0.6, 1.0)
    for k in (1, 3, 5):
        fts, bases, bo = make_inputs(SHAPE, k, seed=110 + k, own_bases=True, device=device)
        reps, deltas = [], []
        for ratio in ratios:
            _, rep, delta = engine.pcb_merge(fts, bases, ALPHAS[:k], bo, ratio=ratio, want_delta=True)
            reps.append(rep)
            deltas.append(delta.cpu())
        for lo, hi in zip(reps, reps[1:]):
            assert lo.positive == hi.positive and lo.M == hi.M and lo.lo == hi.lo and lo.hi == hi.hi
            assert all(a >= b for a, b in zip(lo.t, hi.t)) and all(a <= b for a, b in zip(lo.selected, hi.selected))
            assert lo.covered <= hi.covered and lo.contested <= hi.contested
        assert reps[0].selected[0] < reps[-1].selected[0] == reps[-1].positive[0]
        for lo, hi in zip(deltas, deltas[1:]):      # covered elements stay covered (an element's weights only grow)
            assert bool((hi[lo != 0] != 0).all())


def check_convex(engine, device="cpu"):
    """merged is a convex combination of the clamped entries: |merged| <= max_i |tvc_i| (1 + (k + 2) 2^-24) everywhere"""
    for k, own in ((2, False), (5, True), (16, True)):
        fts, bases, bo = make_inputs(SHAPE, k, seed=120 + k, own_bases=own, device=device)
        alphas = [a if i % 3 else -a for i, a in enumerate(ALPHAS[:k])]
        _, rep, delta = engine.pcb_merge(fts, bases, alphas, bo, ratio=0.4, clip=0.02, want_delta=True)
        top = np.zeros(bo.numel(), dtype=np.float64)
        for i in range(k):
            tv = (fts[i].cpu().float().numpy().reshape(-1) - bases[i].cpu().float().numpy().reshape(-1)) * np.float32(alphas[i])
            c = pcb_oracle.clip_entry(tv, np.float32(rep.lo[i]), np.float32(rep.hi[i]))
            top = np.maximum(top, np.where(tv == 0, 0.0, c.astype(np.float64)))
        merged = np.abs(delta.cpu().numpy().reshape(-1).astype(np.float64))
        assert bool((merged <= top * (1.0 + (k + 2) * EPS)).all()), (k, float((merged / np.maximum(top, 1e-300)).max()))
        assert rep.covered >= int((merged > 0).sum()) > 0         # (a covered element's sum may still cancel to 0)


CORNERS = [check_unaligned, check_bases, check_signed_alphas, check_tied_deltas, check_zero_finetune, check_constant_magnitude,
           check_denormals, check_nonfinite, check_tiny_and_rank3, check_determinism, check_arguments, check_swap,
           check_nested_in_ratio, check_convex]


# ---- profile names and launches ----------------------------------------------------------------------------
PROFILES = [(2, {"stats_hist": 3, "stats_select": 6, "pcb_hist": 3, "pcb_merge": 1}),
            (5, {"stats_hist": 6, "stats_select": 6, "pcb_hist": 6, "pcb_merge": 1})]
PROFILE_IDS = ["k2", "k5"]


def check_profile(engine, k, expected, shape=(40, 50), device="cpu"):
    """three levels of the clip's select (the statistics' kernels, unchanged), three of the scores', one fused pass"""
    fts, bases, bo = make_inputs(shape, k, seed=6, device=device)
    got = profile_of(engine, lambda: engine.pcb_merge(fts, bases, ALPHAS[:k], bo, ratio=0.5))
    assert got == expected, got


# ---- sm_tanh ---------------------------------------------------------------------------------------------------
def tanh_grid():
    """a logarithmic grid from 2^-60 to 30, the neighbourhoods of both branch points, both signs, the zeros"""
    x = np.exp2(np.linspace(-60.0, math.log2(30.0), 3001))
    for b in (pcb_oracle.TANH_SMALL, pcb_oracle.TANH_ONE):
        lo = hi = np.float64(b)
        near = [lo]
        for _ in range(8):
            lo, hi = np.nextafter(lo, 0.0), np.nextafter(hi, np.inf)
            near += [lo, hi]
        x = np.concatenate([x, np.array(near), b * (1.0 + np.linspace(-1e-3, 1e-3, 41))])
    return np.concatenate([x, -x, [0.0, -0.0, 30.0, 1e300, -1e300]])


def check_tanh(engine, on_device):
    import mpmath
    x = tanh_grid()
    y = engine.pcb_fn("tanh", torch.from_numpy(x), on_device=on_device).numpy()
    ref = pcb_oracle.sm_tanh(x)
    assert np.array_equal(y.view(np.uint64), ref.view(np.uint64)), int((y.view(np.uint64) != ref.view(np.uint64)).sum())
    # odd, exactly 0 at 0 (the sign kept), 1 beyond 22.5
    half = (len(x) - 5) // 2
    assert np.array_equal(y[:half].view(np.uint64), (-y[half:2 * half]).view(np.uint64))
    assert y[-5:].view(np.uint64).tolist() == np.array([0.0, -0.0, 1.0, 1.0, -1.0]).view(np.uint64).tolist()
    # against 200-bit mpmath
    mpmath.mp.prec = 200
    worst = 0.0
    for xi, yi in zip(x[:half].tolist(), y[:half].tolist()):
        t = mpmath.tanh(mpmath.mpf(xi))
        worst = max(worst, float(abs((mpmath.mpf(yi) - t) / t)))
    print(f"sm_tanh: largest relative error against mpmath.tanh 2^{math.log2(worst):.2f} over {half} points")
    assert worst <= 2.0 ** -48, math.log2(worst)
    with pytest.raises(ValueError, match="op"):
        engine.pcb_fn("sinh", torch.zeros(1))


# ---- independent of the oracle: the paper's form in torch fp64 --------------------------------------------------
def paper_inputs(n, k, seed, device="cpu"):
    """Gaussian bases (sigma 0.02) with bf16 deltas of sigma 3e-3 (1 + 0.3 i)"""
    g = torch.Generator().manual_seed(2000 + seed)
    base = (torch.randn(n, generator=g) * 0.02).to(torch.bfloat16)
    fts = [(base.float() + torch.randn(n, generator=g) * 3e-3 * (1 + 0.3 * i)).to(torch.bfloat16).to(device) for i in range(k)]
    base = base.to(device)
    return fts, [base] * k, base


def paper_reference(fts, bases, alphas, ratio, clip):
    """-> (num, den, tvc_abs_sum, t / (M - t) max), fp64: torch.sort quantiles at the same indices, exp(k s^2) with the
    factor e^k kept, torch.tanh clamped at 0 from below, min-max normalisation.  Its input is the task vector of step 1."""
    k, n = len(fts), fts[0].numel()
    r, q = pcb_oracle.counts(n, ratio, clip)
    tvs = [((ft.cpu().float() - bs.cpu().float()) * torch.tensor(float(a), dtype=torch.float32)).double().reshape(-1)
           for ft, bs, a in zip(fts, bases, alphas)]
    U = torch.stack(tvs).sum(0)
    num, den, mass, worst = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), 0.0
    for tv in tvs:
        mags = torch.sort(tv.abs()).values
        lo, hi = mags[r], mags[n - 1 - r]
        c = tv.abs().clamp(lo, hi)
        tvc = torch.sign(tv) * c
        s = (c - lo) / (hi - lo)
        S = torch.exp(k * s * s) * torch.tanh(tv * U).clamp(min=0.0)
        t, M = torch.sort(S, descending=True).values[q - 1], S.max()
        scale = torch.where((S >= t) & (S > 0), (S - t) / (M - t), torch.zeros_like(S))
        num, den, mass = num + scale * tvc, den + scale, mass + tvc.abs()
        worst = max(worst, float(t / (M - t)))
    return num, den, mass, worst


def check_paper_form(engine, n, k, ratio=0.1, clip=1e-4, device="cpu"):
    fts, bases, bo = paper_inputs(n, k, seed=k, device=device)
    alphas = [1.0] * k
    _, rep, delta = engine.pcb_merge(fts, bases, alphas, bo, ratio=ratio, clip=clip, want_delta=True)
    num, den, mass, tmt = paper_reference(fts, bases, alphas, ratio, clip)
    merged = delta.cpu().double().reshape(-1)
    covered = den > 0
    judged = covered & (den >= 1e-9)
    skipped = int(covered.sum()) - int(judged.sum())
    eps = EPS * (5.0 + 4.0 * tmt)
    e_num = (eps + (k + 1) * EPS) * mass
    e_den = k * (eps + k * EPS)
    bound = 2.0 * (e_num + merged.abs() * e_den + EPS * num.abs())
    err = (merged * den - num).abs()
    worst = float((err[judged] / bound[judged]).max())
    print(f"paper form n={n} k={k}: t / (M - t) {tmt:.4f}, covered / n {int(covered.sum()) / n:.3f} (engine {rep.covered / n:.3f}), "
          f"selected / n {[s / n for s in rep.selected]}, under the den floor {skipped}, largest error / bound {worst:.4f}")
    assert skipped <= 1e-3 * int(covered.sum()), (skipped, int(covered.sum()))
    assert bool((err[judged] <= bound[judged]).all()), worst
    # (the two counts differ only by entries whose score rounds onto the cut: a weight of 0 here, of an ulp there)
    assert abs(rep.covered - int(covered.sum())) <= 1e-3 * n, (rep.covered, int(covered.sum()))
    return worst


# ---- the C ABI ------------------------------------------------------------------------------------------------
def check_c_abi(engine, device="cpu"):
    from shardmerge_amd import _lib
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(64, generator=g) * 0.01).to(torch.bfloat16).to(device)
    y = torch.zeros(64, dtype=torch.bfloat16, device=device)
    out = torch.zeros(64, dtype=torch.bfloat16, device=device)
    dll, h = engine.lib.dll, engine.ctx.h

    def call(k=1, ratio=0.5, clip=0.0, out_t=out, n=64, in_dtype=_lib.BF16, lam=1.0, alpha=0.5):
        d = _lib.PcbDesc()
        d.k = k
        for i in range(max(0, min(k, 16))):
            d.finetune[i], d.base[i], d.alpha[i] = x.data_ptr(), y.data_ptr(), alpha
        d.in_dtype, d.base_out, d.base_out_dtype, d.n = in_dtype, y.data_ptr(), _lib.BF16, n
        d.ratio, d.clip, d.lam = ratio, clip, lam
        rep = _lib.PcbReport()
        rc = dll.smhip_pcb_merge(h, C.byref(d), out_t.data_ptr(), None, C.byref(rep), None)
        return rc, dll.smhip_last_error(h).decode(), rep

    rc, msg, rep = call()
    assert rc == _lib.OK and rep.q == 32 and rep.clip_rank == 0 and rep.selected[0] >= 32 and 0 < rep.covered <= 64, msg
    assert call(ratio=1.0, clip=0.499)[0] == _lib.OK
    for kwargs, word in (({"k": 0}, "k out of range"), ({"k": 17}, "k out of range"), ({"ratio": 0.0}, "ratio"),
                         ({"ratio": 1.0000001}, "ratio"), ({"ratio": float("nan")}, "ratio"), ({"clip": -1e-9}, "clip"),
                         ({"clip": 0.5}, "clip"), ({"clip": float("nan")}, "clip"), ({"lam": float("inf")}, "lambda"),
                         ({"lam": float("nan")}, "lambda"), ({"alpha": float("nan")}, "alpha"), ({"out_t": x}, "overlaps"),
                         ({"in_dtype": 3}, "dtype")):
        rc, msg, _ = call(**kwargs)
        assert rc == _lib.ERR_ARG and word in msg, (kwargs, rc, msg)
    rc = dll.smhip_pcb_merge(h, None, out.data_ptr(), None, None, None)
    assert rc == _lib.ERR_ARG and "null descriptor" in dll.smhip_last_error(h).decode()
    d = _lib.PcbDesc()
    d.k, d.in_dtype, d.base_out_dtype, d.n, d.ratio, d.clip, d.lam = 1, _lib.BF16, _lib.BF16, 64, 0.5, 0.0, 1.0
    rc = dll.smhip_pcb_merge(h, C.byref(d), out.data_ptr(), None, None, None)
    assert rc == _lib.ERR_ARG and "null" in dll.smhip_last_error(h).decode()
    assert call(n=0, out_t=x)[0] == _lib.OK                     # a no-op, whatever the pointers
    assert dll.smhip_pcb_fn(h, 1, None, None, 0, 0, None) == _lib.ERR_ARG and "bad op" in dll.smhip_last_error(h).decode()
    assert dll.smhip_pcb_fn(h, _lib.PCB_TANH, None, None, 4, 0, None) == _lib.ERR_ARG


# ---- the CLI on the synthetic on-disk model of tests/lora_fixtures.py ----------------------------------------
OPTIONS = {"operator": "pcb", "pcb_ratio": 0.3, "pcb_clip": 0.01, "pcb_lambda": 0.7}


def write_config(root, third, out_dir, opts, device=None):
    return harness.write_config(root, ties_models(third), out_dir, opts, device)


def expected_outputs(base, full, opts, models=None):
    """the oracle tensor by tensor (block tensors) / the provider's tensor (passthrough); the models of ties_models:
    layer 0 has three entries, layer 1 two.  models: the finetune_merge entries, if others."""
    def merge(fts, bases, alphas, base_out, name):
        return pcb_oracle.pcb_merge(
            fts, bases, alphas, base_out, ratio=opts.get("pcb_ratio", 0.1), clip=opts.get("pcb_clip", 0.0001),
            lam=opts.get("pcb_lambda", 1.0))["out"]

    return expected_by_tensor(base, full, models or ties_models("org/lora_full"), merge)
