"""Checks of operator wudi shared by the emulator tier (tests/test_wudi_host.py) and the GPU tier (tests/test_wudi_gpu.py):
the three kernels through smhip_wudi_gemm and Engine.wudi_merge against tests/wudi_oracle.py bit for bit (every value is an
fp32 fmaf chain in ascending k, an ordered fp64 sum or a one-rounding operation: the tolerance is zero), a layout check on
exact integers, what defines the method against torch fp64, the C ABI, the launch counts and the CLI.  CASES lists them."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from shardmerge_amd import _lib
from tests import dare_oracle, harness
from tests import lora_fixtures as lf
from tests import wudi_oracle as wo
from tests.extract_checks import bits32, bits64, host, on
from tests.harness import raw
from tests.iso_checks import merge_inputs, same_bits

GRAM_R, GRAM_C = (1, 2, 31, 32, 33, 130), (1, 17, 127, 128, 129, 257)      # odd k, the k-block edge; one to three tiles
MN, KS = (1, 17, 128, 129, 257), (1, 31, 32, 33, 130)
ALPHAS = (1.0, 0.7, 1.3, 0.4)
GRAM, RHS, STEP = _lib.WUDI_GRAM, _lib.WUDI_RHS, _lib.WUDI_STEP
POKES = (None, float("nan"), float("inf"), float("-inf"))
t_ = torch.from_numpy


# ---- 1. the kernels alone ---------------------------------------------------------------------------------------------
def pair(engine, rows, cols, dtype, seed, offset=0, pad=0, poke=None):
    """(the fp32 delta, finetune and base on the engine's device): views `offset` elements into their storage, rows `pad`
    elements apart; poke: that value in the middle of the finetune"""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(offset + rows * (cols + pad), generator=g).to(dtype)
    ft = (base.float() + 0.05 * torch.randn(base.numel(), generator=g)).to(dtype)
    view = lambda t: t[offset:].view(rows, cols + pad)[:, :cols]
    if poke is not None:
        view(ft)[rows // 2, cols // 2] = poke
    return (view(ft).float() - view(base).float()).numpy(), view(ft.to(engine.device)), view(base.to(engine.device))


def plane(engine, rows, cols, seed, scale=1.0, offset=0, pad=0):
    flat = torch.randn(offset + rows * (cols + pad), generator=torch.Generator().manual_seed(seed)) * scale
    view = lambda t: t[offset:].view(rows, cols + pad)[:, :cols]
    return view(flat).contiguous().numpy(), view(flat.to(engine.device))


def check_gram(engine, R, C, dtype=torch.bfloat16, offset=0, pad=0, poke=None):
    d, ft, base = pair(engine, R, C, dtype, 7 * R + C, offset, pad, poke)
    s0 = plane(engine, C, C, R + C)[0]
    for prior in (None, s0 + s0.T):                                 # the first task, then a symmetric S to add to
        sh, s = (host(x).numpy() for x in engine.wudi_gemm(GRAM, finetune=ft, base=base, w=0.37, s=None if prior is None else t_(prior)))
        ref_sh, ref_s = wo.gram(d, 0.37, prior)
        assert same_bits(sh, ref_sh) and same_bits(s, ref_s), (R, C, dtype, offset, pad, poke, prior is None)
        assert same_bits(sh.T, ref_sh) and same_bits(s.T, ref_s), (R, C, "Sh or S is not symmetric")


def check_rhs(engine, M, N, K, dtype=torch.bfloat16, offset=0, pad=0, poke=None):
    d, ft, base = pair(engine, M, K, dtype, 5 * M + K, offset, pad, poke)
    b, db = plane(engine, N, K, 3 * N + K, 1.0, offset, pad)
    for prior in (None, plane(engine, M, N, M + N)[0]):
        got = host(engine.wudi_gemm(RHS, finetune=ft, base=base, b=db, p=None if prior is None else t_(prior))).numpy()
        assert same_bits(got, wo.rhs(d, b, prior)), (M, N, K, dtype, offset, pad, poke, prior is None)


def check_step(engine, M, N, K, t=1, offset=0, pad=0, poke=None):
    """non-zero m and v; row 0 has acc == P (a zero row of X and of P) with m == v == 0: the update there is exactly 0"""
    (a, da), (b, db) = plane(engine, M, K, 11 * M + K, 0.1, offset, pad), plane(engine, N, K, 13 * N + K, 0.1, offset, pad)
    p, m, v = (plane(engine, M, N, M + q * N, s)[0] for q, s in ((2, 0.1), (3, 1e-3), (4, 1e-3)))
    x, dx = plane(engine, M, N, M + 5 * N, 0.1, offset, pad)
    v = v * v
    a[0], p[0], m[0], v[0], da[0] = 0.0, 0.0, 0.0, 0.0, 0.0
    if poke is not None:
        a[M // 2, K // 2] = da[M // 2, K // 2] = poke
    got = engine.wudi_gemm(STEP, a=da, b=db, p=t_(p), m=t_(m), v=t_(v), x=dx, t=t, lr=1e-3, want_g=True)
    for name, g, r in zip("mvxg", got, wo.step(a, b, p, m, v, x, 1e-3, t)):
        assert same_bits(host(g).numpy(), r), (M, N, K, t, offset, pad, poke, name)
    assert np.array_equal(bits32(host(got[2]).numpy()[0]), bits32(x[0])), "g == 0, m == v == 0: X must not move"


def check_integers(engine, M, N, K):
    """independent of the oracle: small integers, every sum exact in any order; a transposed or permuted operand or output shows"""
    g = torch.Generator().manual_seed(M + N + K)
    ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g)
    dev, i64 = lambda t, dt=torch.float32: t.to(dt).to(engine.device), lambda t: host(t).to(torch.int64)
    ft, base = ri(-3, 4, K, N), ri(-2, 3, K, N)
    sh, s = engine.wudi_gemm(GRAM, finetune=dev(ft, torch.bfloat16), base=dev(base, torch.bfloat16), w=2.0)
    assert torch.equal(i64(sh), 2 * (ft - base).T @ (ft - base)) and torch.equal(i64(s), i64(sh)), (M, N, K, "gram")
    ft, base, b, p, a = ri(-3, 4, M, K), ri(-2, 3, M, K), ri(-2, 6, N, K), ri(-4, 5, M, N), ri(-3, 4, M, K)
    got = engine.wudi_gemm(RHS, finetune=dev(ft, torch.float16), base=dev(base, torch.float16), b=dev(b), p=p.float())
    assert torch.equal(i64(got), p + (ft - base) @ b.T), (M, N, K, "rhs")
    zeros = torch.zeros(M, N)
    got = engine.wudi_gemm(STEP, a=dev(a), b=dev(b), p=p.float(), m=zeros, v=zeros, x=zeros, want_g=True)
    assert torch.equal(i64(got[3]), 2 * (a @ b.T - p)), (M, N, K, "step")


# ---- 2. the whole function ----------------------------------------------------------------------------------------------
def assert_merge_equals(out, rep, delta, ref, label):
    assert out.dtype == ref["out"].dtype and torch.equal(raw(out), raw(ref["out"])), (label, "out")
    assert np.array_equal(bits32(host(delta).numpy()), bits32(ref["merged"])), (label, "delta_out")
    assert (rep.R, rep.C, rep.active, rep.iterations, rep.zero) == tuple(ref[n] for n in ("R", "C", "active", "iterations", "zero")), (label, rep)
    assert bits32(np.array(rep.w)).tolist() == bits32(np.array(ref["w"])).tolist(), (label, "w", rep.w, ref["w"])
    for name in ("n", "grad_sq_first", "grad_sq_last"):
        assert bits64(np.array(getattr(rep, name)).reshape(-1)).tolist() == bits64(np.array(ref[name]).reshape(-1)).tolist(), (label, name)


@functools.lru_cache(maxsize=None)
def merge_case(shape, k, own=False, in_dtype=torch.bfloat16, bo_dtype=None, variant="", iters=3):
    """inputs and the oracle's result, once per process.  variant: "alpha0" (a zero alpha), "delta0" (finetune 0 is its
    base), "zero" (every finetune is its base)"""
    fts, bases, base_out = merge_inputs(shape, k, own, in_dtype, bo_dtype)
    alphas = list(ALPHAS[:k - 1]) + [0.0 if variant == "alpha0" else ALPHAS[k - 1]]
    fts = list(bases) if variant == "zero" else ([bases[0]] + fts[1:] if variant == "delta0" else fts)
    return fts, bases, alphas, base_out, wo.merge(fts, bases, alphas, base_out, iters, 1e-4, 0.7)


def wudi(engine, fts, bases, alphas, base_out, **kw):
    same = {}
    dev = lambda t: same.setdefault(id(t), on(engine, t))          # a shared base stays ONE tensor
    return engine.wudi_merge([dev(t) for t in fts], [dev(t) for t in bases], alphas, dev(base_out), want_delta=True, **kw)


def check_merge(engine, shape, k, own=False, in_dtype=torch.bfloat16, bo_dtype=None, variant="", iters=3):
    fts, bases, alphas, base_out, ref = merge_case(tuple(shape), k, own, in_dtype, bo_dtype, variant, iters)
    out, rep, delta = wudi(engine, fts, bases, alphas, base_out, iters=iters, lr=1e-4, lam=0.7, layer_name="layers.0.w")
    assert_merge_equals(out, rep, delta, ref, (shape, k, own, in_dtype, bo_dtype, variant, iters))
    if iters == 0 and not rep.zero:
        assert np.array_equal(bits32(host(delta).numpy()), bits32(ref["X0"])), "iters 0: delta_out is iso_sum's X_0"
    out2, rep2, delta2 = wudi(engine, fts, bases, alphas, base_out, iters=iters, lr=1e-4, lam=0.7)
    assert torch.equal(raw(out), raw(out2)) and torch.equal(raw(delta), raw(delta2)) and rep == rep2, "two calls differ"
    return rep


def check_corner_cases(engine):
    assert check_merge(engine, (17, 33), 3, variant="alpha0").active == [0, 1]
    assert check_merge(engine, (33, 17), 3, True, variant="delta0").active == [1, 2]
    rep = check_merge(engine, (130, 40), 2, variant="zero")
    assert rep.zero and rep.active == [] and rep.n == [0.0, 0.0] and rep.grad_sq_first == 0.0
    fts, bases, base_out = merge_inputs((48, 60), 2)                # rank 3: the matrix [shape[0] x the rest]
    view = lambda t: on(engine, t).view(48, 6, 10)
    out, rep, delta = engine.wudi_merge([view(t) for t in fts], [view(bases[0])] * 2, [1.0, 0.5], view(base_out), iters=2, want_delta=True)
    assert tuple(out.shape) == (48, 6, 10) == tuple(delta.shape)
    assert_merge_equals(out.reshape(48, 60), rep, delta.reshape(48, 60), wo.merge(fts, bases, [1.0, 0.5], base_out, 2), "rank 3")
    for bad in POKES[1:]:
        ft = fts[1].clone()
        ft[5, 7] = bad
        with pytest.raises(ValueError, match=r"model\.layers\.3\.q_proj\.weight.*finetune 1"):
            wudi(engine, [fts[0], ft], bases, [1.0, 1.0], base_out, iters=1, layer_name="model.layers.3.q_proj.weight")


# ---- 3. what defines the method, independent of the oracle -----------------------------------------------------------
def check_orthogonal(engine, k):
    """deltas on disjoint column sets: d_i d_j^T = 0, so X_0 S and P are the SAME chain (the other tasks' columns add +0
    and w_i enters both sides through Sh_i alone): g == 0 exactly and X never moves"""
    g = torch.Generator().manual_seed(40 + k)
    base = (torch.randn(130, 257, generator=g) * 0.02).bfloat16()
    cols, fts = torch.randperm(257, generator=g), []
    for i in range(k):
        d = torch.zeros(130, 257)
        d[:, cols[i::k]] = torch.randn(130, len(cols[i::k]), generator=g) * 3e-3 * (1 + 0.3 * i)
        fts.append((base.float() + d).bfloat16())
    x0 = wudi(engine, fts, [base] * k, [1.0] * k, base, iters=0)[2]
    _, rep, delta = wudi(engine, fts, [base] * k, [1.0] * k, base, iters=3)
    assert rep.grad_sq_first == 0.0 == rep.grad_sq_last and torch.equal(raw(delta), raw(x0)) and len(rep.active) == k, rep


def interfering_inputs(seed=3):
    """Gaussian bf16 base, three bf16 deltas of sigma 3e-3 (1 + 0.3 i) that share a common component, 128 x 256; the seed
    was chosen on the CPU, with the oracle alone, so that 5 steps decrease L (tests/test_wudi_host.py asserts it)"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda s: torch.randn(128, 256, generator=g) * s
    base, common = rn(0.02).bfloat16(), rn(1.0)
    return [(base.float() + 3e-3 * (1 + 0.3 * i) * (0.6 * common + 0.8 * rn(1.0))).bfloat16() for i in range(3)], base


def check_interfering(engine):
    fts, base = interfering_inputs()
    deltas = [f.float() - base.float() for f in fts]
    x0 = wudi(engine, fts, [base] * 3, [1.0] * 3, base, iters=0)[2]
    _, rep, delta = wudi(engine, fts, [base] * 3, [1.0] * 3, base, iters=5)
    l0, l5 = wo.loss(host(x0), deltas), wo.loss(host(delta), deltas)
    print(f"interfering: L {l0:.9g} -> {l5:.9g}, grad_sq {rep.grad_sq_first:.6g} -> {rep.grad_sq_last:.6g}")
    assert l5 < l0 and rep.grad_sq_last < rep.grad_sq_first, (l0, l5, rep)


# max |delta_out - X_fp64| of the numpy restatement (tests/wudi_oracle.py, the function's own arithmetic) at 64 x 128,
# k = 2, 3 iterations, lr 1e-5, measured on the CPU: 1.0153e-8; the engine is held to 4 times it.  Adam normalises the
# gradient, so an element whose gradient is at rounding level moves by lr either way: 3 iterations already show ONE such
# element of 8192 with the oracle alone, so only elements with |g_fp64| >= 2^-20 max |g_fp64| at every step are compared
# (tests/test_wudi_host.py asserts that they are at least 99 % of the tensor and that the oracle meets FP64_GAP).
FP64_GAP = 1.016e-8


@functools.lru_cache(maxsize=None)
def fp64_case():
    fts, bases, base_out = merge_inputs((64, 128), 2)
    X64, gs = wo.iterate_fp64([f.float() - b.float() for f, b in zip(fts, bases)], 3, 1e-5)
    mask = functools.reduce(torch.logical_and, [g.abs() >= 2.0 ** -20 * g.abs().max() for g in gs])
    return fts, bases, base_out, X64, mask


def check_against_fp64(engine):
    fts, bases, base_out, X64, mask = fp64_case()
    delta = wudi(engine, fts, bases, [1.0, 1.0], base_out, iters=3, lr=1e-5)[2]
    worst = float((host(delta).double() - X64).abs()[mask].max())
    print(f"fp64 iteration: max |delta_out - X_fp64| {worst:.4e} (tolerance 4 x {FP64_GAP:.3e})")
    assert worst <= 4 * FP64_GAP, (worst, FP64_GAP)


# ---- 5. host logic ------------------------------------------------------------------------------------------------------
def check_profile(engine):
    """per active task one wudi_gram and one wudi_rhs, per step one wudi_step"""
    for k, iters, variant in ((3, 3, "alpha0"), (2, 1, ""), (2, 0, "")):
        fts, bases, alphas, base_out, ref = merge_case((33, 17), k, False, torch.bfloat16, None, variant, iters)
        table = harness.profile_of(engine, lambda: wudi(engine, fts, bases, alphas, base_out, iters=iters, lr=1e-4, lam=0.7))
        a, r = len(ref["active"]), min(iters, 2)
        want = {"geo_gram": k, "geo_gram_fold": k + r, "wudi_gram": a, "wudi_rhs": a, "iso_sum": 1, "wudi_step": iters, "iso_norm": r, "iso_apply": 1}
        assert table == {n: c for n, c in want.items() if c}, table


def check_c_abi(engine):
    fts, bases, _ = merge_inputs((32, 48), 2)
    ft, base, x = on(engine, fts[0]), on(engine, bases[0]), on(engine, torch.ones(8, 8))
    out, y, z = torch.empty_like(base), torch.empty_like(x), torch.zeros_like(x)
    dll, h = engine.lib.dll, engine.ctx.h
    need = int(dll.smhip_wudi_workspace(32, 48))
    assert need >= (2 * 48 * 48 + 5 * 32 * 48) * 4 and dll.smhip_wudi_workspace(0, 48) == 0 == dll.smhip_wudi_workspace(8, 32769)
    ws = engine._xl_workspace(need)

    def merge(out_t=out.data_ptr(), alpha=1.0, ptrs=(ft.data_ptr(), base.data_ptr(), base.data_ptr()), **over):
        d = _lib.WudiDesc()
        d.finetune[0], d.base[0], d.alpha[0], d.finetune[1], d.base[1], d.alpha[1] = ptrs[0], ptrs[1], alpha, ptrs[0], ptrs[1], alpha
        for key, value in {**dict(k=2, in_dtype=_lib.BF16, base_out=ptrs[2], base_out_dtype=_lib.BF16, n=32 * 48, rows=32, cols=48, lam=1.0,
                                  lr=1e-5, iters=2, workspace=ws.data_ptr(), workspace_bytes=need), **over}.items():
            setattr(d, key, value)
        return dll.smhip_wudi_merge(h, C.byref(d), C.c_void_p(out_t), None, None, engine._stream()), dll.smhip_last_error(h).decode()

    def probe(**over):
        d = _lib.WudiGemmDesc()
        for key, value in {**dict(kind=1, M=8, N=8, K=8, finetune=x.data_ptr(), base=z.data_ptr(), dtype=_lib.F32, ld=8, b=x.data_ptr(), ldb=8,
                                  first=1, p=y.data_ptr(), t=1, lr=1e-5), **over}.items():
            setattr(d, key, value)
        return dll.smhip_wudi_gemm(h, C.byref(d), engine._stream()), dll.smhip_last_error(h).decode()

    assert merge()[0] == _lib.OK and merge(n=0, out_t=ft.data_ptr())[0] == _lib.OK and probe()[0] == _lib.OK and bool((host(y) == 8).all())
    # (C > 32768 is rejected before any tensor is read: the pointers are made-up addresses a terabyte apart)
    for fn, name, cases in ((merge, "wudi_merge", (({"k": 17}, "k out of range"), ({"alpha": -1.0}, "alpha"), ({"lam": float("inf")}, "lambda"),
                                                   ({"lr": 0.0}, "lr"), ({"lr": 1.5}, "lr"), ({"iters": -1}, "iters"), ({"iters": 2001}, "iters"),
                                                   ({"cols": 47}, "rows * cols"), ({"out_t": ft.data_ptr()}, "overlaps"), ({"workspace_bytes": need - 1}, "workspace"),
                                                   ({"n": 2 * 32769, "rows": 2, "cols": 32769, "ptrs": (1 << 40, 2 << 40, 3 << 40), "out_t": 4 << 40}, "exceeds 32768"))),
                            (probe, "wudi_gemm", (({"kind": 3}, "kind"), ({"K": 0}, "shape"), ({"kind": 0, "M": 4}, "shape"), ({"dtype": 5}, "dtype"),
                                                  ({"b": None}, "null"), ({"kind": 2}, "null"), ({"p": x.data_ptr()}, "overlaps"), ({"ld": 7}, "pitch")))):
        for kwargs, word in cases:
            rc, msg = fn(**kwargs)
            assert rc == _lib.ERR_ARG and word in msg and name in msg, (kwargs, rc, msg)
    wide = torch.zeros(1, dtype=torch.bfloat16).expand(2, 32769)
    for args, kw in ((([ft], [base], [1.0], base), dict(lr=0.0)), (([ft], [base], [1.0], base), dict(iters=True)), (([ft], [base], [-1.0], base), {}),
                     (([ft.reshape(-1)], [base.reshape(-1)], [1.0], base.reshape(-1)), {}), (([wide] * 2, [wide] * 2, [1.0] * 2, wide), {})):
        with pytest.raises(ValueError, match="wudi_merge"):
            engine.wudi_merge(*args, **kw)


# ---- 6. the CLI on the synthetic on-disk model of tests/lora_fixtures.py ------------------------------------------
OPTIONS = {"operator": "wudi", "wudi_iters": 3, "wudi_lr": 1e-4, "wudi_lambda": 0.7}


def expected_outputs(base, full, models=None):
    """the oracle tensor by tensor: matrices that several entries cover by wudi_oracle.merge, 1-D block tensors and matrices
    of ONE entry by dare_linear at density 1 times lambda, the passthrough tensors from their provider"""
    def merge(fts, bases, alphas, base_out, name):
        if base_out.ndim < 2 or len(fts) == 1:
            return dare_oracle.dare_merge(fts, bases, alphas, base_out, density=1.0, lam=0.7, normalize=True, rescale=True,
                                          sign_election=False, key=0, stream_ids=list(range(len(fts))))[0]
        return wo.merge(fts, bases, alphas, base_out, 3, 1e-4, 0.7)["out"]

    return harness.expected_by_tensor(base, full, models or harness.ties_models("org/lora_full"), merge)


def check_cli(tmp_path, engine, device=None, third="org/lora_full", models=None):
    base, factors, full = lf.setup_k3(tmp_path, engine)
    res = harness.run_cli(harness.write_config(tmp_path, models or harness.ties_models(third), "merged", OPTIONS, device))
    assert res.exit_code == 0, res.output
    harness.assert_outputs(tmp_path / "merged", expected_outputs(base, full, models))
    readme = (tmp_path / "merged" / "README.md").read_text()
    assert all(word in readme for word in ("# WUDI Merged Model", "WUDI (", "iterations 3", "lr 0.0001", "lambda 0.7")), readme


# ---- the checks that both tiers run, by name -------------------------------------------------------------------------
def views_and_special_values(e, dt):
    check_gram(e, 35, 130, dt, offset=1, pad=3), check_gram(e, 64, 136, dt, pad=8)       # (aligned rows, a pitch that is not the width)
    check_rhs(e, 129, 33, 130, dt, offset=1, pad=3), check_rhs(e, 33, 129, 64, dt, pad=8), check_step(e, 129, 33, 35, 3, 1, 3)
    for poke in POKES[1:]:
        check_gram(e, 33, 17, dt, poke=poke), check_rhs(e, 17, 33, 35, dt, poke=poke), check_step(e, 17, 33, 35, poke=poke)


CASES = {f"gram-R{R}": (lambda e, R=R: [check_gram(e, R, c) for c in GRAM_C]) for R in GRAM_R}
CASES.update({f"rhs-step-K{K}": (lambda e, K=K: [(check_rhs(e, M, N, K), check_step(e, M, N, K, 1 + 2 * (i % 2)))
                                                 for i, (M, N) in enumerate(zip(MN + MN, MN + MN[2:] + MN[:2]))]) for K in KS})
CASES.update({f"views-{dt}": functools.partial(views_and_special_values, dt=dt) for dt in harness.DTYPES})
CASES["integers"] = lambda e: [check_integers(e, *s) for s in ((17, 33, 5), (130, 257, 33), (257, 130, 64))]
CASES.update({f"merge-{s[0]}x{s[1]}-iters{it}": (lambda e, s=s, it=it: check_merge(e, s, 2, iters=it)) for s in ((17, 33), (33, 17), (130, 257)) for it in (0, 1, 3)})
CASES.update({f"merge-k{k}-{'own' if own else 'shared'}": (lambda e, k=k, own=own: (check_merge(e, (17, 33), k, own), check_merge(e, (33, 17), k, own)))
              for k in (1, 2, 3, 4) for own in (False, True)})
CASES.update({f"merge-{i}-{o}".replace("torch.", ""): (lambda e, i=i, o=o: check_merge(e, (33, 17), 2, in_dtype=i, bo_dtype=o))
              for i in harness.DTYPES for o in harness.DTYPES})
CASES.update({"merge-corner-cases": check_corner_cases, "orthogonal-k2": lambda e: check_orthogonal(e, 2), "orthogonal-k3": lambda e: check_orthogonal(e, 3),
              "interfering": check_interfering, "fp64": check_against_fp64, "profile": check_profile, "c-abi": check_c_abi})
