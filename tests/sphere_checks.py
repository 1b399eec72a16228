"""Checks of the Karcher-mean operators (karcher, multislerp) shared by the emulator tier (tests/test_sphere_host.py) and
the GPU tier (tests/test_sphere_gpu.py).

1. Engine.sphere_merge against tests/sphere_oracle.py BIT FOR BIT: the output, the fp32 combination, the report's G, H, w,
   a, N, tau, iterations, flags and coefficients as raw bits; row-wise every row's coefficients, iteration count and flags.
   The tolerance is zero and it is derived: every step of the definition is one correctly rounded IEEE operation in a
   stated order (include/shardmerge_hip.h, smhip_sphere_merge).
2. sm_acos / sm_sin / sm_cos: host bits == device bits == oracle bits, and an absolute error of at most 2^-40 against
   math.acos / math.sin / math.cos (each good to an ulp), the condition the header derives.
3. Checks that need no oracle - the iteration in tensor space in torch fp64 with math.* trigonometry, slerp / nuslerp at
   k = 2, closed forms, invariances - so that an oracle and a kernel with the same mistake do not pass together."""
import ctypes as C
import math
import struct

import numpy as np
import pytest
import torch

from tests import harness
from tests import sphere_oracle as so
from tests.harness import ALPHAS, DTYPES, SMALL, expected_by_tensor, f32_bits, f64_bits, make_inputs, raw, ties_models

MODES = so.MODES
# (mode, rowwise): the four operator variants
VARIANTS = (("karcher", False), ("karcher", True), ("multislerp", False), ("multislerp", True))
VARIANT_IDS = ["karcher", "karcher_rowwise", "multislerp", "multislerp_rowwise"]
FN_BOUND = 2.0 ** -40


def bits64(xs):
    return [f64_bits(x) for x in xs]


def check(engine, fts, bases, alphas, base_out, mode="karcher", rowwise=False, max_iter=10, tol=1e-5, label=""):
    """one call against the oracle, bit for bit; returns (the engine's report, the oracle's dict)"""
    out, rep, delta = engine.sphere_merge(fts, bases, alphas, base_out, mode=mode, rowwise=rowwise, max_iter=max_iter, tol=tol,
                                          want_delta=True)
    cpu = lambda ts: [t.cpu() for t in ts]
    ref = so.sphere_merge(cpu(fts), cpu(bases), alphas, base_out.cpu(), mode=mode, rowwise=rowwise, max_iter=max_iter, tol=tol)
    k = len(fts)
    assert out.dtype == base_out.dtype and out.shape == base_out.shape, label
    assert rep.mode == mode and rep.rowwise == bool(rowwise)
    if base_out.numel():
        if rowwise:
            print(f"{label}: iterations <= {rep.iters_max}, {rep.rows_unconverged} row(s) not converged, {rep.rows_linear} linear, "
                  f"sum c in [{rep.csum_min}, {rep.csum_max}] mean {rep.csum_mean}")
            got_c, want_c = rep.row_coefficients.numpy().view(np.int32), np.ascontiguousarray(ref["c_rows"]).view(np.int32)
            assert got_c.shape == want_c.shape and np.array_equal(got_c, want_c), (label, "row coefficients", int((got_c != want_c).sum()))
            assert np.array_equal(rep.row_iterations.numpy(), ref["iters_rows"]), (label, "row iterations")
            assert np.array_equal(rep.row_flags.numpy(), ref["flags_rows"]), (label, "row flags")
            for key in ("iters_max", "rows_unconverged", "rows_linear"):
                assert getattr(rep, key) == ref[key], (label, key, getattr(rep, key), ref[key])
            for key in ("csum_min", "csum_max", "csum_mean"):
                assert f64_bits(getattr(rep, key)) == f64_bits(ref[key]), (label, key, getattr(rep, key), ref[key])
        else:
            print(f"{label}: {rep.iterations} iteration(s), tau {rep.tau}, converged {rep.converged}, linear {rep.linear}, c {rep.coefficients}")
            for i in range(k):
                assert bits64(rep.gram[i]) == bits64(ref["G"][i]), (label, "G", i, rep.gram[i], ref["G"][i])
                assert bits64(rep.cosines[i]) == bits64(ref["H"][i]), (label, "H", i, rep.cosines[i], ref["H"][i])
            for got, key in ((rep.weights, "w"), (rep.a, "a")):
                assert bits64(got) == bits64(ref[key]), (label, key, got, ref[key])
            assert f64_bits(rep.length) == f64_bits(ref["N"]) and f64_bits(rep.tau) == f64_bits(ref["tau"]), (label, rep, ref["N"], ref["tau"])
            assert (rep.iterations, rep.converged, rep.linear) == (ref["iterations"], ref["converged"], ref["linear"]), (label, rep)
            assert [f32_bits(c) for c in rep.coefficients] == [f32_bits(c) for c in ref["c"]], (label, rep.coefficients, ref["c"])
    bad = int((raw(delta) != raw(ref["delta"])).sum())
    assert bad == 0, f"{label}: {bad} of {ref['delta'].numel()} values of the combination differ in their bits"
    bad = int((raw(out) != raw(ref["out"])).sum())
    assert bad == 0, f"{label}: {bad} of {ref['out'].numel()} output values differ in their bits"
    return rep, ref


# ---- the parameter grid -------------------------------------------------------------------------------
def check_dtypes(engine, in_dtype, bo_dtype, mode, rowwise, device="cpu"):
    fts, bases, bo = make_inputs(SMALL, 3, in_dtype, bo_dtype, seed=11, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:3], bo, mode, rowwise, label=f"{mode} {in_dtype}->{bo_dtype}")
    fts, bases, bo = make_inputs(SMALL, 2, in_dtype, bo_dtype, seed=12, device=device)      # one shared base
    check(engine, fts, bases, ALPHAS[:2], bo, mode, rowwise, label=f"{mode} {in_dtype}->{bo_dtype} shared")


def check_k(engine, k, mode, rowwise, device="cpu"):
    """k = 1, 2, 3, 5, 16: one tile of pairs up to k = 4 and the register instantiation of sphere_coef, ten tiles and the
    LDS instantiation (256-, 128- and 64-thread work-groups at k = 5, 16); own bases and a shared one"""
    for own in (False, True):
        fts, bases, bo = make_inputs(SMALL, k, seed=20 + k + own, own_bases=own, device=device)
        rep, _ = check(engine, fts, bases, ALPHAS[:k], bo, mode, rowwise, label=f"{mode} k={k} rowwise={rowwise} own={own}")
        if k == 1 and not rowwise:
            assert rep.coefficients == [1.0] and rep.iterations == 0 and rep.converged and not rep.linear


def check_lds_group_sizes(engine, device="cpu"):
    """row-wise k = 7 and 10: the 128-thread work-group of the LDS instantiation at both of its ends (k = 6: the last 256)"""
    for k in (6, 7, 10, 11):
        fts, bases, bo = make_inputs((300, 24), k, seed=33 + k, own_bases=True, device=device)
        check(engine, fts, bases, ALPHAS[:k], bo, "multislerp", True, label=f"row-wise k={k}")


def check_shapes(engine, device="cpu"):
    """1-D, rank 3, n not a multiple of 8, C not a multiple of 8 row-wise, rows shorter than an octet, several segments"""
    for shape in ((4099,), (4, 33, 65), (37, 13), (300, 5), (3, 40000), (16, 4096)):
        for mode, rowwise in VARIANTS:
            fts, bases, bo = make_inputs(shape, 3, seed=40 + len(shape), own_bases=True, device=device)
            check(engine, fts, bases, ALPHAS[:3], bo, mode, rowwise, label=f"{mode} rowwise={rowwise} shape={shape}")
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
        out, rep = engine.sphere_merge(fts, bases, [0.5, 0.5], bo, mode=mode, rowwise=rowwise)
        assert out.numel() == 0 and out.dtype == bo.dtype
    fts, bases, bo = make_inputs((0, 8), 2, seed=73, device=device)
    out, rep = engine.sphere_merge(fts, bases, [0.5, 0.5], bo, rowwise=True)
    assert out.shape == (0, 8)


# ---- the three functions ------------------------------------------------------------------------------------
def function_arguments(op):
    """4096 arguments spread over the domain, its end points, and the values next to them"""
    lo, hi = (-1.0, 1.0) if op == "acos" else (0.0, math.pi)
    g = torch.Generator().manual_seed(17)
    xs = (torch.rand(4096, generator=g, dtype=torch.float64) * (hi - lo) + lo).clamp(lo, hi).tolist() + [lo, hi, 0.0, 0.5 * (lo + hi)]
    if op == "acos":
        xs += [0.5, -0.5, math.nextafter(0.5, 1.0), math.nextafter(-0.5, -1.0)]
        for p in range(1, 53):
            xs += [1.0 - 2.0 ** -p, -(1.0 - 2.0 ** -p), 2.0 ** -p, -(2.0 ** -p)]
    else:
        xs += [math.pi / 2, math.nextafter(math.pi / 2, 4.0), math.nextafter(math.pi / 2, 0.0), math.nextafter(math.pi, 0.0)]
        for p in range(1, 53):
            xs += [2.0 ** -p, math.pi - 2.0 ** -p, math.pi / 2 - 2.0 ** -p, math.pi / 2 + 2.0 ** -p]
        xs += [5e-324, 1e-300, 1e-8, 1e-9]
    assert all(lo <= x <= hi for x in xs)
    return torch.tensor(xs, dtype=torch.float64)


def check_functions(engine, device="cpu"):
    for op in ("acos", "sin", "cos"):
        x = function_arguments(op)
        host = engine.sphere_fn(op, x, on_device=False)
        dev = engine.sphere_fn(op, x, on_device=True)
        ora = torch.from_numpy(so.FNS[op](x.numpy()))
        as_bits = lambda t: t.contiguous().view(torch.int64)
        assert torch.equal(as_bits(host), as_bits(ora)), (op, "host != oracle", int((as_bits(host) != as_bits(ora)).sum()))
        assert torch.equal(as_bits(dev), as_bits(host)), (op, "device != host", int((as_bits(dev) != as_bits(host)).sum()))
        true = torch.tensor([getattr(math, op)(v) for v in x.tolist()], dtype=torch.float64)
        err = float((host - true).abs().max())
        print(f"sm_{op}: {x.numel()} arguments, largest absolute error {err:.3e} = 2^{math.log2(err) if err else float('-inf'):.1f} (bound 2^-40 = {FN_BOUND:.3e})")
        assert err <= FN_BOUND, (op, err)
    assert float(engine.sphere_fn("acos", torch.tensor([1.0]), on_device=False)[0]) == 0.0
    assert float(engine.sphere_fn("acos", torch.tensor([-1.0]), on_device=False)[0]) == math.pi
    assert float(engine.sphere_fn("sin", torch.tensor([0.0]), on_device=False)[0]) == 0.0
    assert float(engine.sphere_fn("cos", torch.tensor([0.0]), on_device=False)[0]) == 1.0
    with pytest.raises(ValueError, match="op"):
        engine.sphere_fn("tan", torch.tensor([0.0]))


# ---- independent of the oracle -----------------------------------------------------------------------------
def correlated_vectors(shape, k, seed, device="cpu"):
    """fp32 random vectors plus a common component: the pairwise cosines are near 1/2"""
    g = torch.Generator().manual_seed(seed)
    common = torch.randn(shape, generator=g)
    return [(torch.randn(shape, generator=g) * (0.7 + 0.2 * i) + common * (1.0 + 0.1 * i)).to(device) for i in range(k)]


def tensor_space_mean(xs, weights, max_iter=50, tol=1e-14):
    """the Karcher mean iterated on the VECTORS in torch fp64 with math.* trigonometry: sum_i w_i |x_i| times the mean
    direction.  Checks that every pairwise cosine lies in [0.2, 0.9]: there fp64 conditioning is harmless."""
    xs = [x.double().reshape(-1) for x in xs]
    norms = [float(x.norm()) for x in xs]
    us = [x / n for x, n in zip(xs, norms)]
    for i in range(len(us)):
        for j in range(i + 1, len(us)):
            assert 0.2 <= float(us[i] @ us[j]) <= 0.9, (i, j, float(us[i] @ us[j]))
    m = sum(w * u for w, u in zip(weights, us))
    m = m / m.norm()
    for _ in range(max_iter):
        t = torch.zeros_like(m)
        for w, u in zip(weights, us):
            d = max(-1.0, min(1.0, float(m @ u)))
            theta = math.acos(d)
            f = 1.0 if theta < 1e-8 else theta / math.sin(theta)
            t = t + (w * f) * (u - d * m)
        tau = float(t.norm())
        if tau < tol:
            break
        m = math.cos(tau) * m + (math.sin(tau) / tau) * t
        m = m / m.norm()
    return sum(w * n for w, n in zip(weights, norms)) * m


def check_against_tensor_space(engine, device="cpu"):
    """|M - R| <= (k + 3) 2^-24 sum_i |c_i x_i| per element, a priori: one fp32 rounding of each coefficient, one of each
    product and k - 1 of the sums make k + 1 units (each relative to a quantity bounded by sum |c_i x_i|); two units are
    left for the second order and for the fp64 residue of the two iterations (4e-16 in the prototype)."""
    shape = (64, 512)
    for k in (2, 3, 5):
        xs = correlated_vectors(shape, k, seed=200 + k, device=device)
        zero = [torch.zeros_like(x) for x in xs]
        bo = torch.zeros(shape, dtype=torch.float32, device=device)
        alphas = ALPHAS[:k]
        weights = [a / sum(alphas) for a in alphas]
        for mode, rowwise in VARIANTS:
            out, rep, M = engine.sphere_merge(xs, zero, alphas, bo, mode=mode, rowwise=rowwise, max_iter=50, tol=1e-14, want_delta=True)
            M = M.cpu().double()
            cpu = [x.cpu() for x in xs]
            if rowwise:
                R = torch.stack([tensor_space_mean([x[r] for x in cpu], weights) for r in range(shape[0])])
                coef = rep.row_coefficients.double()                                    # [R, k]
                scale = sum(coef[:, i:i + 1].abs() * cpu[i].double().abs() for i in range(k))
                assert rep.rows_linear == 0
            else:
                R = tensor_space_mean(cpu, weights).view(shape)
                scale = sum(abs(c) * x.double().abs() for c, x in zip(rep.coefficients, cpu))
                assert not rep.linear
            bound = (k + 3) * 2.0 ** -24 * scale
            ratio = float(((M - R).abs() / bound).max())
            print(f"tensor space k={k} {mode} rowwise={rowwise}: largest |M - R| / bound {ratio:.3f}")
            assert bool(((M - R).abs() <= bound).all()), (k, mode, rowwise, ratio)
            assert torch.equal(raw(out), raw(M.float()))                                 # base_out is 0: out = M


def ulps32(a, b):
    ia, ib = struct.unpack("<i", f32_bits(a))[0], struct.unpack("<i", f32_bits(b))[0]
    return abs(ia - ib)


def check_against_pair_operators(engine, device="cpu"):
    """k = 2: multislerp gives nuslerp's coefficients and karcher slerp's within 1 ulp of fp32 - the first step is exact in
    real arithmetic and the fp64 error is orders below an fp32 ulp.  Both new operators average the LENGTHS linearly, as
    nuslerp does; slerp leaves the length to its two sines, c_i = s_i.  So karcher's coefficients are slerp's where the
    two norms are equal (here: a vector and a signed permutation of it, norms equal to an fp64 rounding), and slerp's
    times N / n_i - within the two fp32 roundings - where they are not."""
    for seed, alphas in ((210, [0.5, 0.3]), (211, [0.2, 0.8]), (212, [1.0, 1.0])):
        fts, bases, bo = make_inputs(SMALL, 2, seed=seed, own_bases=True, device=device)
        g = torch.Generator().manual_seed(seed)
        perm = torch.randperm(bo.numel(), generator=g).to(bo.device)
        sign = (torch.randint(0, 2, (bo.numel(),), generator=g) * 2 - 1).to(bo.device).to(fts[0].dtype)
        twin = (fts[0].reshape(-1)[perm] * sign).view(bo.shape)
        for mode, old, pair in (("multislerp", "nuslerp", fts), ("karcher", "slerp", [fts[0], twin]), ("karcher", "slerp", fts)):
            _, rep = engine.sphere_merge(pair, bases, alphas, bo, mode=mode)
            _, geo = engine.geo_merge(pair, bases, alphas, bo, mode=old)
            assert not geo.linear and not rep.linear and rep.converged and rep.iterations <= 2     # (equal weights start at the mean)
            assert bits64(rep.gram[0]) == bits64(geo.gram[0]) and bits64(rep.gram[1]) == bits64(geo.gram[1])
            norms = [math.sqrt(rep.gram[i][i]) for i in range(2)]
            print(f"{mode} {rep.coefficients} / {old} {geo.coefficients}, norms {norms}")
            if pair is fts and mode == "karcher":
                for c, s, n in zip(rep.coefficients, geo.coefficients, norms):
                    assert abs(c - s * rep.length / n) <= 2.0 ** -23 * abs(c), (rep.coefficients, geo.coefficients, norms)
            else:
                assert all(ulps32(a, b) <= 1 for a, b in zip(rep.coefficients, geo.coefficients)), (mode, rep.coefficients, geo.coefficients)


def check_identical_vectors(engine, device="cpu"):
    """k copies of one vector: c_i = fp32(w_i) and the output is that vector"""
    fts, bases, bo = make_inputs(SMALL, 1, seed=213, device=device)
    zero = torch.zeros_like(fts[0])
    for rowwise in (False, True):
        out, rep = engine.sphere_merge([fts[0]] * 3, [zero] * 3, [0.5, 0.25, 0.25], bo, mode="karcher", rowwise=rowwise)
        assert torch.equal(raw(out), raw(fts[0]))
        if rowwise:
            assert torch.equal(rep.row_coefficients, torch.tensor([0.5, 0.25, 0.25]).expand(SMALL[0], 3)) and rep.rows_unconverged == 0
        else:
            assert rep.coefficients == [0.5, 0.25, 0.25] and rep.converged and not rep.linear


def check_disjoint_supports(engine, device="cpu"):
    """entries +-1 on disjoint supports of equal size, equal weights: exactly orthogonal vectors of equal norm; the mean
    direction is their normalised sum, c_i within 1 fp32 ulp of 1 / sqrt(k)"""
    for k in (2, 3, 5):
        shape = (16, 30 * k)
        g = torch.Generator().manual_seed(214 + k)
        idx = torch.arange(shape[1]).expand(shape) % k
        sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
        xs = [torch.where(idx == i, sign, torch.zeros(shape)).to(device) for i in range(k)]
        zero = [torch.zeros_like(x) for x in xs]
        bo = torch.zeros(shape, device=device)
        want = 1.0 / math.sqrt(k)
        for mode, rowwise in VARIANTS:
            _, rep = engine.sphere_merge(xs, zero, [0.5] * k, bo, mode=mode, rowwise=rowwise)
            cs = rep.row_coefficients.reshape(-1).tolist() if rowwise else rep.coefficients
            assert all(ulps32(c, want) <= 1 for c in cs), (k, mode, rowwise, cs[:k], want)
            if not rowwise:
                assert all(rep.cosines[i][j] == (1.0 if i == j else 0.0) for i in range(k) for j in range(k))


def check_scaling(engine, device="cpu"):
    """every vector times 2^3 (exact in fp32): H, a and every c_i keep their bits"""
    fts, bases, bo = make_inputs(SMALL, 3, torch.float32, seed=215, device=device)
    zero = [torch.zeros_like(b) for b in bases]
    ds = [f - b for f, b in zip(fts, bases)]
    for rowwise in (False, True):
        _, rep = engine.sphere_merge(ds, zero, ALPHAS[:3], bo, mode="multislerp", rowwise=rowwise)
        _, rep8 = engine.sphere_merge([d * 8.0 for d in ds], zero, ALPHAS[:3], bo, mode="multislerp", rowwise=rowwise)
        if rowwise:
            assert torch.equal(raw(rep.row_coefficients), raw(rep8.row_coefficients)) and torch.equal(rep.row_iterations, rep8.row_iterations)
        else:
            assert [bits64(r) for r in rep.cosines] == [bits64(r) for r in rep8.cosines] and bits64(rep.a) == bits64(rep8.a)
            assert [f32_bits(c) for c in rep.coefficients] == [f32_bits(c) for c in rep8.coefficients]
            assert rep8.length == 8.0 * rep.length and rep8.gram[0][1] == 64.0 * rep.gram[0][1]


def check_row_permutation(engine, device="cpu"):
    """row-wise mode commutes with a permutation of the rows, bit for bit"""
    for shape, k in (((97, 131), 3), ((64, 256), 5)):
        fts, bases, bo = make_inputs(shape, k, seed=216, own_bases=True, device=device)
        perm = torch.randperm(shape[0], generator=torch.Generator().manual_seed(5))
        dperm = perm.to(bo.device)
        for mode in MODES:
            out, rep = engine.sphere_merge(fts, bases, ALPHAS[:k], bo, mode=mode, rowwise=True)
            outp, repp = engine.sphere_merge([t[dperm].contiguous() for t in fts], [t[dperm].contiguous() for t in bases], ALPHAS[:k],
                                             bo[dperm].contiguous(), mode=mode, rowwise=True)
            assert torch.equal(raw(outp), raw(out[dperm]))
            assert torch.equal(raw(repp.row_coefficients), raw(rep.row_coefficients[perm]))
            assert torch.equal(repp.row_iterations, rep.row_iterations[perm]) and torch.equal(repp.row_flags, rep.row_flags[perm])


def check_nesting(engine, device="cpu"):
    """one row of n <= 32768 elements is one segment: the row-wise call equals the whole-tensor call bit for bit"""
    for n in (1000, 4099, 32768):
        fts, bases, bo = make_inputs((1, n), 3, seed=217, own_bases=True, device=device)
        for mode in MODES:
            out, rep = engine.sphere_merge(fts, bases, ALPHAS[:3], bo, mode=mode)
            outr, repr_ = engine.sphere_merge(fts, bases, ALPHAS[:3], bo, mode=mode, rowwise=True)
            assert torch.equal(raw(out), raw(outr))
            assert [f32_bits(c) for c in rep.coefficients] == [f32_bits(c) for c in repr_.row_coefficients[0].tolist()]
            assert rep.iterations == int(repr_.row_iterations[0]) == repr_.iters_max


PROPERTIES = [check_against_tensor_space, check_against_pair_operators, check_identical_vectors, check_disjoint_supports, check_scaling,
              check_row_permutation, check_nesting]


# ---- corners ----------------------------------------------------------------------------------------------
def check_zero_vectors(engine, device="cpu"):
    """all vectors zero: c = [0, 0, 0]; all but one zero: that one's c is 1"""
    fts, bases, bo = make_inputs(SMALL, 3, seed=220, own_bases=True, device=device)
    same = [b.clone() for b in bases]
    for rowwise in (False, True):
        rep, _ = check(engine, same, bases, ALPHAS[:3], bo, "multislerp", rowwise, label="zero deltas")
        out, _ = engine.sphere_merge(same, bases, ALPHAS[:3], bo, mode="multislerp", rowwise=rowwise)
        assert torch.equal(raw(out), raw(bo))
        if rowwise:
            assert not rep.row_coefficients.any() and rep.iters_max == 0 and rep.rows_unconverged == 0
        else:
            assert rep.coefficients == [0.0, 0.0, 0.0] and rep.converged and rep.iterations == 0
        rep, _ = check(engine, [same[0], fts[1], same[2]], bases, ALPHAS[:3], bo, "multislerp", rowwise, label="one active delta")
        if rowwise:
            assert torch.equal(rep.row_coefficients, torch.tensor([0.0, 1.0, 0.0]).expand(SMALL[0], 3))
        else:
            assert rep.coefficients == [0.0, 1.0, 0.0] and rep.converged and rep.iterations == 0
    # a tensor whose first rows are zero in one vector: those rows take the two-vector path, the others all three
    x = fts[2].clone()
    x[:5] = bases[2][:5]
    rep, _ = check(engine, [fts[0], fts[1], x], bases, ALPHAS[:3], bo, "multislerp", True, label="zero rows")
    assert not rep.row_coefficients[:5, 2].any() and bool(rep.row_coefficients[5:, 2].all())


def check_antipodal(engine, device="cpu"):
    """x and -x with equal weights: the unit vectors cancel, the LINEAR case.  With entries +-1 and a square element count the
    norms are exact and H_01 = -1, q = 0.  With random entries H_01 is -1 only up to the rounding of the two square roots
    (the header says so) and q may land on either side of 1e-16: whatever comes out, it is the oracle's, bit for bit."""
    g = torch.Generator().manual_seed(221)
    shape = (64, 256)
    d = (torch.randint(0, 2, shape, generator=g).float() * 2 - 1).to(torch.bfloat16).to(device)
    zero = torch.zeros_like(d)
    bo = make_inputs(shape, 1, seed=222, device=device)[2]
    for mode, rowwise in VARIANTS:
        rep, _ = check(engine, [d, -d], [zero, zero], [0.5, 0.5], bo, mode, rowwise, label=f"antipodal +-1 {mode}")
        if rowwise:
            assert rep.rows_linear == shape[0] and torch.equal(rep.row_coefficients, torch.full((shape[0], 2), 0.5))
        else:
            assert rep.linear and not rep.converged and rep.iterations == 0 and rep.coefficients == [0.5, 0.5]
            assert rep.cosines[0][1] == -1.0
        out, _ = engine.sphere_merge([d, -d], [zero, zero], [0.5, 0.5], bo, mode=mode, rowwise=rowwise)
        assert torch.equal(raw(out), raw(torch.zeros_like(bo) if mode == "karcher" else bo))
    d = torch.randn(SMALL, generator=g).to(torch.bfloat16).to(device)
    zero = torch.zeros_like(d)
    bo = make_inputs(SMALL, 1, seed=222, device=device)[2]
    for mode, rowwise in VARIANTS:
        check(engine, [d, -d], [zero, zero], [0.5, 0.5], bo, mode, rowwise, label=f"antipodal {mode}")
        check(engine, [d, -d], [zero, zero], [0.75, 0.25], bo, mode, rowwise, label=f"antipodal {mode}, unequal weights")


def check_zero_alpha(engine, device="cpu"):
    """a zero alpha among positive ones: that vector is inactive, c_i = 0, and the rest is the mean of the others"""
    fts, bases, bo = make_inputs(SMALL, 3, seed=223, own_bases=True, device=device)
    for mode, rowwise in VARIANTS:
        rep, _ = check(engine, fts, bases, [0.5, 0.0, 0.4], bo, mode, rowwise, label=f"zero alpha {mode}")
        out, _ = engine.sphere_merge(fts, bases, [0.5, 0.0, 0.4], bo, mode=mode, rowwise=rowwise)
        out2, rep2 = engine.sphere_merge([fts[0], fts[2]], [bases[0], bases[2]], [0.5, 0.4], bo, mode=mode, rowwise=rowwise)
        assert torch.equal(raw(out), raw(out2))
        if rowwise:
            assert not rep.row_coefficients[:, 1].any() and torch.equal(raw(rep.row_coefficients[:, [0, 2]]), raw(rep2.row_coefficients))
        else:
            assert rep.coefficients[1] == 0.0 and [rep.coefficients[0], rep.coefficients[2]] == rep2.coefficients


def check_tol_zero(engine, device="cpu"):
    """karcher_tol 0: exactly max_iter iterations, reported as not converged"""
    fts, bases, bo = make_inputs(SMALL, 3, seed=224, own_bases=True, device=device)
    for mode, rowwise in VARIANTS:
        for max_iter in (1, 7):
            rep, _ = check(engine, fts, bases, ALPHAS[:3], bo, mode, rowwise, max_iter=max_iter, tol=0.0, label=f"tol 0 {mode}")
            if rowwise:
                assert rep.iters_max == max_iter and bool((rep.row_iterations == max_iter).all()) and rep.rows_unconverged == SMALL[0]
            else:
                assert rep.iterations == max_iter and not rep.converged and not rep.linear
    # identical vectors reach tau == 0 exactly: the step is the identity, not 0 / 0
    rep, _ = check(engine, [fts[0]] * 2, [bases[0]] * 2, [0.5, 0.5], bo, "karcher", max_iter=3, tol=0.0, label="tol 0, identical")
    assert rep.iterations == 3 and not rep.linear and rep.coefficients == [0.5, 0.5]


def check_nonfinite(engine, device="cpu"):
    """a NaN / an Inf in one finetune: ValueError naming the tensor and the finetune; the context stays usable"""
    for mode, rowwise in VARIANTS:
        for poison in (float("nan"), float("inf")):
            fts, bases, bo = make_inputs(SMALL, 3, seed=225, device=device)
            fts[1] = fts[1].clone()
            fts[1].view(-1)[4321] = poison
            with pytest.raises(ValueError, match=r"model\.layers\.7\.mlp\.up_proj\.weight.*finetune 1\b"):
                engine.sphere_merge(fts, bases, ALPHAS[:3], bo, mode=mode, rowwise=rowwise, layer_name="model.layers.7.mlp.up_proj.weight")
        fts, bases, bo = make_inputs(SMALL, 3, seed=226, device=device)
        check(engine, fts, bases, ALPHAS[:3], bo, mode, rowwise, label="after an error")


def check_determinism(engine, device="cpu"):
    fts, bases, bo = make_inputs((300, 500), 3, seed=227, own_bases=True, device=device)
    for mode, rowwise in VARIANTS:
        a, ra = engine.sphere_merge(fts, bases, ALPHAS[:3], bo, mode=mode, rowwise=rowwise)
        b, rb = engine.sphere_merge(fts, bases, ALPHAS[:3], bo, mode=mode, rowwise=rowwise)
        assert torch.equal(raw(a), raw(b))
        if rowwise:
            assert torch.equal(raw(ra.row_coefficients), raw(rb.row_coefficients)) and torch.equal(ra.row_iterations, rb.row_iterations)
            assert (ra.csum_min, ra.csum_max, ra.csum_mean) == (rb.csum_min, rb.csum_max, rb.csum_mean)
        else:
            assert ra == rb


def check_arguments(engine, device="cpu"):
    fts, bases, bo = make_inputs((8, 8), 3, seed=228, device=device)
    with pytest.raises(ValueError, match="mode"):
        engine.sphere_merge(fts, bases, ALPHAS[:3], bo, mode="slerp")
    for alphas in ([-0.5, 1.0, 1.0], [0.0, 0.0, 0.0], [float("nan"), 1.0, 1.0], [float("inf"), 1.0, 1.0]):
        with pytest.raises(ValueError, match="alphas >= 0 with a sum > 0"):
            engine.sphere_merge(fts, bases, alphas, bo)
    for max_iter in (0, 101, 2.5, True):
        with pytest.raises(ValueError, match="max_iter"):
            engine.sphere_merge(fts, bases, ALPHAS[:3], bo, max_iter=max_iter)
    for tol in (-1e-9, 1.0, float("nan")):
        with pytest.raises(ValueError, match="tol"):
            engine.sphere_merge(fts, bases, ALPHAS[:3], bo, tol=tol)
    with pytest.raises(ValueError, match="shape mismatch"):
        engine.sphere_merge([fts[0], fts[1][:4]], bases[:2], [0.5, 0.5], bo)
    with pytest.raises(ValueError, match="supported range"):
        engine.sphere_merge([fts[0]] * 17, [bases[0]] * 17, [0.1] * 17, bo)
    with pytest.raises(ValueError, match="alphas"):
        engine.sphere_merge(fts, bases, [0.5], bo)


CORNERS = [check_lds_group_sizes, check_shapes, check_unaligned, check_empty, check_zero_vectors, check_antipodal, check_zero_alpha,
           check_tol_zero, check_nonfinite, check_determinism, check_arguments]


def check_c_abi(engine):
    """bad arguments through the C ABI (host tensors: the emulator)"""
    from shardmerge_amd import _lib
    x = torch.zeros(64, dtype=torch.bfloat16)
    y = torch.zeros(64, dtype=torch.bfloat16)
    out = torch.zeros(64, dtype=torch.bfloat16)
    dll, h = engine.lib.dll, engine.ctx.h

    def call(k=2, weight_space=0, rowwise=0, rows=1, out_t=out, n=64, in_dtype=_lib.BF16, alpha=0.5, alpha1=None, base=y, max_iter=10, tol=1e-5):
        d = _lib.SphereDesc()
        d.k = k
        for i in range(max(0, min(k, 16))):
            d.finetune[i], d.base[i], d.alpha[i] = x.data_ptr(), (base.data_ptr() if base is not None else None), alpha
        if alpha1 is not None:
            d.alpha[1] = alpha1
        d.in_dtype, d.base_out, d.base_out_dtype, d.n = in_dtype, (base.data_ptr() if base is not None else None), _lib.BF16, n
        d.weight_space, d.rowwise, d.rows, d.max_iter, d.tol = weight_space, rowwise, rows, max_iter, tol
        rep = _lib.SphereReport()
        rc = dll.smhip_sphere_merge(h, C.byref(d), out_t.data_ptr(), None, C.byref(rep), None)
        return rc, dll.smhip_last_error(h).decode(), rep

    rc, msg, rep = call()
    assert rc == _lib.OK and rep.converged == 1 and rep.linear == 0 and rep.iterations == 0, msg      # zero vectors
    assert call(rowwise=1, rows=8)[0] == _lib.OK and call(k=16)[0] == _lib.OK
    assert call(weight_space=1, base=None)[0] == _lib.OK                                          # weight space reads no base
    assert call(tol=0.0, max_iter=100)[0] == _lib.OK
    for kwargs, word in (({"k": 0}, "k out of range"), ({"k": 17}, "k out of range"), ({"alpha": -0.5}, "alphas >= 0"),
                         ({"alpha1": -0.1}, "alphas >= 0"), ({"alpha": 0.0}, "sum > 0"), ({"alpha": float("nan")}, "alpha"),
                         ({"alpha1": float("inf")}, "alpha"), ({"max_iter": 0}, "max_iter"), ({"max_iter": 101}, "max_iter"),
                         ({"tol": float("nan")}, "tol"), ({"tol": 1.0}, "tol"), ({"tol": -1e-3}, "tol"),
                         ({"rows": 0}, "rows"), ({"rows": 7}, "rows"), ({"rowwise": 1, "rows": 5}, "rows"),
                         ({"base": None}, "null"), ({"out_t": x}, "overlaps"), ({"in_dtype": 3}, "dtype")):
        rc, msg, _ = call(**kwargs)
        assert rc == _lib.ERR_ARG and word in msg, (kwargs, rc, msg)
    rc = dll.smhip_sphere_merge(h, None, out.data_ptr(), None, None, None)
    assert rc == _lib.ERR_ARG and "null descriptor" in dll.smhip_last_error(h).decode()
    assert call(n=0, out_t=x, rows=0)[0] == _lib.OK                 # a no-op, whatever the pointers
    v = torch.zeros(4, dtype=torch.float64)
    assert dll.smhip_sphere_fn(h, 3, v.data_ptr(), v.data_ptr(), 4, 0, None) == _lib.ERR_ARG
    assert dll.smhip_sphere_fn(h, 0, None, v.data_ptr(), 4, 0, None) == _lib.ERR_ARG
    assert dll.smhip_sphere_fn(h, 0, None, None, 0, 0, None) == _lib.OK


def check_profile(engine, mode, rowwise, k, shape=(40, 50), device="cpu"):
    """profile names and launch counts: ONE geo_gram and ONE geo_combine per call whatever k, the fold for whole-tensor
    calls, sphere_coef for row-wise ones"""
    fts, bases, bo = make_inputs(shape, k, seed=6, device=device)
    engine.ctx.profile(True)
    engine.ctx.profile_reset()
    try:
        engine.sphere_merge(fts, bases, ALPHAS[:k], bo, mode=mode, rowwise=rowwise)
        table = engine.ctx.profile_table()
    finally:
        engine.ctx.profile(False)
    expected = {"geo_gram": 1, "geo_combine": 1, ("sphere_coef" if rowwise else "geo_gram_fold"): 1}
    assert {n: table[n][0] for n in table} == expected


# ---- the CLI on the synthetic on-disk model of tests/lora_fixtures.py ----------------------------------------
README_WORDS = {"karcher": ("# Karcher Merged Model", "karcher:", "weights [0.416667, 0.25, 0.333333]", "max_iter 10", "tol 1e-05"),
                "multislerp": ("# MultiSLERP Merged Model", "multislerp:", "weights [0.416667, 0.25, 0.333333]", "max_iter 10", "tol 1e-05")}


def options(operator, row_wise=None, **more):
    opts = {"operator": operator, **more}
    if row_wise is not None:
        opts["sphere_row_wise"] = row_wise
    return opts


def write_config(root, third, out_dir, opts, device=None):
    return harness.write_config(root, ties_models(third), out_dir, opts, device)


def expected_outputs(base, full, opts):
    """the oracle tensor by tensor (block tensors) / the provider's tensor (passthrough)"""
    def merge(fts, bases, alphas, base_out, name):
        return so.sphere_merge(
            fts, bases, alphas, base_out, mode=opts["operator"], rowwise=bool(opts.get("sphere_row_wise", 0)),
            max_iter=int(opts.get("karcher_max_iter", 10)), tol=float(opts.get("karcher_tol", 1e-5)))["out"]

    return expected_by_tensor(base, full, ties_models("org/lora_full"), merge)
