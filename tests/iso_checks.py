"""Checks of operator iso_c shared by the emulator tier (tests/test_iso_host.py) and the GPU tier (tests/test_iso_gpu.py):
`iso_gemm` through smhip_iso_gemm and Engine.iso_merge against tests/iso_oracle.py bit for bit (the tolerance is zero and
derived: every value is an fp32 fmaf chain in ascending k, an ordered fp64 sum or a one-rounding operation), a layout check
on exact integers, what defines Iso-C against torch fp64 `linalg.svd`, the properties of the function, and the CLI."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from shardmerge_amd import _lib
from tests import dare_oracle, harness
from tests import iso_oracle as io
from tests import lora_fixtures as lf
from tests.extract_checks import bits32, bits64, host, on
from tests.harness import expected_by_tensor, raw, run_cli, ties_models

# around the MFMA tile (32), the k-block (32) and the work-group tile (128); k is not split, so there is no split edge
GEMM_MN = ((1, 17), (15, 128), (16, 1), (17, 257), (127, 15), (128, 129), (129, 16), (257, 127))
GEMM_K = (1, 3, 4, 5, 31, 32, 33, 130, 515)
GEMM_SYM = ((1, 5), (17, 33), (128, 130), (129, 4), (257, 31))                  # (s, K)
MERGE_SHAPES = ((17, 33), (33, 17), (130, 257), (192, 320), (320, 192), (128, 128))
MERGE_KS = ((1, False), (2, True), (3, False), (3, True), (5, False), (5, True))     # (k, every finetune over its own base)
MERGE_K_IDS = [f"k{k}-{'own_bases' if own else 'shared_base'}" for k, own in MERGE_KS]
ALPHAS = (1.0, 0.7, 1.3, 0.4, 0.9)
DTYPES = harness.DTYPES


def same_bits(got, ref):
    """bit for bit; where the reference is a NaN any NaN will do (the payload of a NaN is not part of the definition)"""
    got, ref = np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    nan = np.isnan(ref)
    return got.shape == ref.shape and np.isnan(got[nan]).all() and np.array_equal(bits32(got[~nan]), bits32(ref[~nan]))


# ---- 1. iso_gemm ---------------------------------------------------------------------------------------------------
def matrix(engine, rows, cols, seed, offset=0, pad=0, special=False, scale=1.0):
    """(the numpy matrix, its view on the engine's device): `offset` elements into its storage, rows `pad` elements apart"""
    g = torch.Generator().manual_seed(seed)
    ld = cols + pad
    flat = torch.randn(offset + rows * ld, generator=g) * scale
    v = flat[offset:].view(rows, ld)[:, :cols]
    if special:                                                     # zeros, -0, denormals
        v[::3, ::2] = 0.0
        v[1::4, 1::3] = -0.0
        v[0, 0] = 1e-41
        v[rows - 1, cols - 1] = -1e-40
    dev = flat.to(engine.device)[offset:].view(rows, ld)[:, :cols]
    return v.contiguous().numpy(), dev


def check_gemm(engine, form, M, N, K, ep=io.PLAIN, offset=0, pad=0, special=False, poke=None):
    a, da = matrix(engine, M, K, 11 * M + K, offset, pad, special)
    b, db = matrix(engine, *((N, K) if form == io.NT else (K, N)), 13 * N + K + 1, offset, pad, special)
    e, de = matrix(engine, M, N, 17 * M + N + 2, offset, pad, special)
    if poke is not None:                                            # a NaN or an Inf in each operand
        for arr, dev in ((a, da), (b, db)):
            arr[arr.shape[0] // 2, arr.shape[1] // 2] = poke
            dev[arr.shape[0] // 2, arr.shape[1] // 2] = poke
    ca, cb = 1.25, -0.3
    got = host(engine.iso_gemm(da, db, form=form, epilogue=ep, ca=ca, cb=cb, e=de if ep else None, ldc=N + pad)).numpy()
    ref = io.gemm(a, b, form, ep, ca, cb, e)
    assert same_bits(got, ref), (form, M, N, K, ep, offset, pad, special, poke)


def check_gemm_sym(engine, s, K, gram=True):
    """the symmetric mode: a a^T, or g g for a symmetric g; the result equals the oracle and its own transpose exactly"""
    a, da = matrix(engine, s, K if gram else s, 19 * s + K)
    if not gram:
        a = io.gemm(a, a)
        da = torch.from_numpy(a).to(engine.device)
    got = host(engine.iso_gemm(da, da, form=io.NT, sym=True, epilogue=io.POLY if not gram else io.PLAIN, ca=0.5, cb=2.0,
                               e=None if gram else da)).numpy()
    ref = io.gemm(a, a, io.NT, io.PLAIN if gram else io.POLY, 0.5, 2.0, a)
    assert np.array_equal(bits32(got), bits32(got.T)), (s, K, gram, "not symmetric")
    assert same_bits(got, ref), (s, K, gram)


def check_gemm_integers(engine, form, M, N, K):
    """independent of the oracle: small integers, every sum exact in any order; a and b differ, so a transposed or
    permuted operand or output shows"""
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randint(-3, 4, (M, K), generator=g)
    b = torch.randint(-2, 6, (N, K) if form == io.NT else (K, N), generator=g)
    e = torch.randint(-4, 5, (M, N), generator=g)
    ref = a.to(torch.int64) @ (b.T if form == io.NT else b).to(torch.int64)
    dev = lambda t: t.float().to(engine.device)
    assert torch.equal(host(engine.iso_gemm(dev(a), dev(b), form=form)).to(torch.int64), ref), (form, M, N, K)
    got = engine.iso_gemm(dev(a), dev(b), form=form, epilogue=io.CUBIC, ca=2.0, cb=-3.0, e=dev(e))
    assert torch.equal(host(got).to(torch.int64), 2 * e - 3 * ref), (form, M, N, K, "cubic")
    got = engine.iso_gemm(dev(a), dev(b), form=form, epilogue=io.POLY, ca=2.0, cb=-3.0, e=dev(e))
    assert torch.equal(host(got).to(torch.int64), 2 * ref - 3 * e), (form, M, N, K, "poly")
    got = engine.iso_gemm(dev(a), dev(b), form=form, epilogue=io.AXPY, ca=2.0, e=dev(e))
    assert torch.equal(host(got).to(torch.int64), 2 * e + ref), (form, M, N, K, "axpy")


# ---- 2. the whole function ----------------------------------------------------------------------------------------
def merge_inputs(shape, k, own=False, in_dtype=torch.bfloat16, bo_dtype=None, seed=0):
    """the issue's inputs: a Gaussian base (sigma 0.02), deltas of sigma 3e-3 (1 + 0.3 i)"""
    g = torch.Generator().manual_seed(5000 + 31 * shape[0] + shape[-1] + k + seed)
    rn = lambda s: torch.randn(shape, generator=g) * s
    shared = rn(0.02).to(in_dtype)
    bases = [rn(0.02).to(in_dtype) if own else shared for _ in range(k)]
    fts = [(bases[i].float() + rn(3e-3 * (1 + 0.3 * i))).to(in_dtype) for i in range(k)]
    base_out = rn(0.02).to(bo_dtype) if (own or (bo_dtype or in_dtype) != in_dtype) else shared
    return fts, bases, base_out


def assert_merge_equals(out, rep, delta, ref, label):
    assert out.dtype == ref["out"].dtype and torch.equal(raw(out), raw(ref["out"])), (label, "out")
    assert np.array_equal(bits32(host(delta).numpy()), bits32(ref["merged"])), (label, "delta_out")
    got = (rep.rows, rep.cols, rep.s, rep.L, rep.transposed, rep.iterations, rep.steps, rep.converged, rep.zero)
    want = (ref["rows"], ref["cols"], ref["s"], ref["L"], ref["transposed"], ref["iterations"], ref["steps"], ref["converged"], ref["zero"])
    assert got == want, (label, got, want)
    for name, a, b in (("nu", rep.nu, ref["nu"]), ("e", rep.e, ref["e"]), ("N", rep.N, ref["N"]), ("sigma_bar", rep.sigma_bar, ref["sigma_bar"])):
        assert bits64(np.array(a).reshape(-1)).tolist() == bits64(np.array(b).reshape(-1)).tolist(), (label, name, a, b)


@functools.lru_cache(maxsize=None)
def merge_case(shape, k, own=False, in_dtype=torch.bfloat16, bo_dtype=None, variant="", tol=1e-4, max_iter=40):
    """inputs and the oracle's result, computed once per process.  variant: "zero" (every finetune is its base),
    "signs" (alphas of both signs and a zero)"""
    fts, bases, base_out = merge_inputs(shape, k, own, in_dtype, bo_dtype)
    alphas = list(ALPHAS[:k])
    if variant == "zero":
        fts = list(bases)
    if variant == "signs":
        alphas = [-0.8, 0.0, 1.1, -0.3, 0.5][:k]
    lam = 0.7
    return fts, bases, alphas, base_out, lam, io.merge(fts, bases, alphas, base_out, lam, tol, max_iter)


def check_merge(engine, shape, k, own=False, in_dtype=torch.bfloat16, bo_dtype=None, variant="", tol=1e-4, max_iter=40):
    fts, bases, alphas, base_out, lam, ref = merge_case(tuple(shape), k, own, in_dtype, bo_dtype, variant, tol, max_iter)
    same = {}
    dev = lambda t: same.setdefault(id(t), on(engine, t))          # a shared base stays ONE tensor
    args = ([dev(t) for t in fts], [dev(t) for t in bases], alphas, dev(base_out))
    kw = dict(lam=lam, tol=tol, max_iter=max_iter, want_delta=True, layer_name="layers.0.w")
    out, rep, delta = engine.iso_merge(*args, **kw)
    label = f"{shape} k={k} own={own} {in_dtype} {bo_dtype} {variant} max_iter={max_iter}"
    print(f"{label}: steps {rep.steps} e {[float(f'{v:.3g}') for v in rep.e]} converged {rep.converged} sigma_bar {rep.sigma_bar:.6g}")
    assert_merge_equals(out, rep, delta, ref, label)
    out2, rep2, delta2 = engine.iso_merge(*args, **kw)
    assert torch.equal(raw(out), raw(out2)) and torch.equal(raw(delta), raw(delta2)) and rep == rep2, "two calls differ"
    return rep


def check_rank3(engine):
    """a tensor of more than two dimensions is the matrix [shape[0] x the rest]"""
    fts, bases, base_out = merge_inputs((48, 60), 2)
    view = lambda t: on(engine, t).view(48, 6, 10)
    out, rep, delta = engine.iso_merge([view(t) for t in fts], [view(bases[0])] * 2, [1.0, 0.5], view(base_out), want_delta=True)
    ref = io.merge(fts, bases, [1.0, 0.5], base_out)
    assert tuple(out.shape) == (48, 6, 10) == tuple(delta.shape) and (rep.rows, rep.cols) == (48, 60)
    assert_merge_equals(out.reshape(48, 60), rep, delta.reshape(48, 60), ref, "rank 3")


def check_nonfinite(engine):
    fts, bases, base_out = merge_inputs((48, 64), 2)
    for bad in (float("nan"), float("inf"), float("-inf")):
        ft = fts[1].clone()
        ft[5, 7] = bad
        with pytest.raises(ValueError, match=r"model\.layers\.3\.q_proj\.weight.*finetune 1"):
            engine.iso_merge([on(engine, fts[0]), on(engine, ft)], [on(engine, b) for b in bases], [1.0, 1.0], on(engine, base_out),
                             layer_name="model.layers.3.q_proj.weight")
    # finite deltas whose weighted sum overflows fp32: nu is not finite
    big = torch.full((48, 64), 3e38)
    with pytest.raises(ValueError, match=r"layers\.9.*not finite"):
        engine.iso_merge([on(engine, big)] * 2, [on(engine, torch.zeros(48, 64))] * 2, [1.0, 1.0], on(engine, big), layer_name="layers.9")


# ---- 3. what defines Iso-C, against torch fp64 linalg.svd ----------------------------------------------------------
# Tolerances: 4 x what the numpy restatement (tests/iso_oracle.py, the function's own arithmetic) deviates from the fp64
# SVD form on THESE cases, measured on the CPU (tests/test_iso_host.py has the figures); none comes from the HIP path.
SVD_CASES = (((128, 512), 3), ((512, 128), 2), ((256, 256), 2))
# (distance, sigma_bar, spread) of iso_oracle.merge; steps qqqcccc, qqqcccc, qqqqqqqccccc
SVD_MEASURED = {((128, 512), 3): (1.016e-6, 3.859e-7, 1.994e-6), ((512, 128), 2): (9.812e-7, 3.667e-7, 1.943e-6),
                ((256, 256), 2): (1.278e-6, 4.931e-9, 1.615e-6)}


def svd_figures(fts, bases, alphas, merged, sigma_bar):
    """(||merged - mean(S) U V^T||_F / ||ref||_F, |sigma_bar - mean(S)| / mean(S), (S_max - S_min) / sigma_bar of merged)"""
    T = sum(float(a) * (f.double() - b.double()) for f, b, a in zip(fts, bases, alphas))
    U, S, Vh = torch.linalg.svd(T, full_matrices=False)
    ref = S.mean() * (U @ Vh)
    own = torch.linalg.svdvals(merged.double())
    return (float(torch.linalg.norm(merged.double() - ref) / torch.linalg.norm(ref)), float(abs(sigma_bar - S.mean()) / S.mean()),
            float((own.max() - own.min()) / sigma_bar))


def check_against_svd(engine, shape, k):
    fts, bases, base_out = merge_inputs(shape, k)
    alphas = list(ALPHAS[:k])
    out, rep, delta = engine.iso_merge([on(engine, t) for t in fts], [on(engine, bases[0])] * k, alphas, on(engine, base_out), want_delta=True)
    figs = svd_figures(fts, bases, alphas, host(delta), rep.sigma_bar)
    tols = [4 * v for v in SVD_MEASURED[(tuple(shape), k)]]
    print(f"{shape} k={k}: steps {rep.steps}, distance {figs[0]:.3e} (tol {tols[0]:.1e}), sigma_bar {figs[1]:.3e} (tol {tols[1]:.1e}), "
          f"spread {figs[2]:.3e} (tol {tols[2]:.1e})")
    assert rep.converged
    assert all(f <= t for f, t in zip(figs, tols)), (shape, k, figs, tols)
    return figs


# ---- 4. properties through the engine ------------------------------------------------------------------------------
def iso(engine, fts, bases, alphas, base_out, **kw):
    same = {}
    dev = lambda t: same.setdefault(id(t), on(engine, t))
    return engine.iso_merge([dev(t) for t in fts], [dev(t) for t in bases], alphas, dev(base_out), want_delta=True, **kw)


def check_transpose(engine):
    fts, bases, base_out = merge_inputs((130, 257), 3, own=True)
    t = lambda x: x.t().contiguous()
    out, rep, delta = iso(engine, fts, bases, list(ALPHAS[:3]), base_out, lam=0.7)
    outT, repT, deltaT = iso(engine, [t(x) for x in fts], [t(x) for x in bases], list(ALPHAS[:3]), t(base_out), lam=0.7)
    assert not rep.transposed and repT.transposed and (repT.rows, repT.cols) == (257, 130)
    assert torch.equal(raw(outT), raw(t(out))) and torch.equal(raw(deltaT), raw(t(delta)))
    assert (rep.steps, rep.e, rep.nu, rep.N, rep.sigma_bar) == (repT.steps, repT.e, repT.nu, repT.N, repT.sigma_bar)


def check_doubled_alphas(engine):
    fts, bases, base_out = merge_inputs((96, 160), 3)
    out, rep, delta = iso(engine, fts, bases, [1.0, 0.7, -1.3], base_out)
    out2, rep2, delta2 = iso(engine, fts, bases, [2.0, 1.4, -2.6], base_out)
    assert torch.equal(raw(host(delta) * 2), raw(delta2))
    assert (rep.steps, rep.e, rep.converged) == (rep2.steps, rep2.e, rep2.converged)
    assert (rep2.nu, rep2.N, rep2.sigma_bar) == (2 * rep.nu, 2 * rep.N, 2 * rep.sigma_bar)


def check_swapped_entries(engine):
    fts, bases, base_out = merge_inputs((96, 160), 2, own=True)
    out, rep, delta = iso(engine, fts, bases, [0.6, 0.6], base_out)
    out2, rep2, delta2 = iso(engine, fts[::-1], bases[::-1], [0.6, 0.6], base_out)
    assert torch.equal(raw(out), raw(out2)) and torch.equal(raw(delta), raw(delta2)) and rep == rep2


def check_partial_permutation(engine, tol=1e-4):
    """k = 1, T = 2^-8 x (a signed partial permutation, 96 x 160): every singular value is 2^-8, so the polar factor is
    2^8 T and e <= tol bounds |q^2 - 1| of the common singular value q of Q: |delta_out - T| <= 2^-8 (tol (2 + tol) + 2^-20),
    the first term exact arithmetic, the second the room for fp32 rounding"""
    g = torch.Generator().manual_seed(12)
    perm = torch.randperm(160, generator=g)[:96]
    T = torch.zeros(96, 160)
    T[torch.arange(96), perm] = (torch.randint(0, 2, (96,), generator=g) * 2 - 1).float() * 2.0 ** -8
    base = (torch.randn(96, 160, generator=g) * 0.02).bfloat16().float()
    out, rep, delta = iso(engine, [base + T], [base], [1.0], base, tol=tol)
    bound = 2.0 ** -8 * (tol * (2 + tol) + 2.0 ** -20)
    worst = float((host(delta).double() - T.double()).abs().max())
    print(f"partial permutation: steps {rep.steps}, e {rep.e[-1]:.3e}, worst |delta_out - T| {worst:.3e} (bound {bound:.3e})")
    assert rep.converged and worst <= bound, (worst, bound)


# |e_fp64 - e_engine| of the numpy restatement at 256 x 1024, k = 3 (steps qqqccc): its last e is 5.906e-5, the residual
# recomputed in fp64 from its delta_out / sigma_bar 5.904e-5
E_GAP = 2.24e-8


def check_large_residual(engine, shape, tol=1e-4):
    """on the device: converged, and e recomputed in torch fp64 from delta_out / sigma_bar stays within tol + 4 E_GAP"""
    g = torch.Generator(device=engine.device).manual_seed(77)
    rn = lambda s: torch.randn(shape, generator=g, device=engine.device) * s
    base = rn(0.02).bfloat16()
    fts = [(base.float() + rn(3e-3 * (1 + 0.3 * i))).bfloat16() for i in range(3)]
    out, rep, delta = engine.iso_merge(fts, [base] * 3, list(ALPHAS[:3]), base, tol=tol, want_delta=True)
    e64 = residual_fp64(delta, rep.sigma_bar)
    print(f"{shape}: steps {rep.steps}, e {rep.e[-1]:.3e}, recomputed in fp64 {e64:.3e} (tol {tol:g} + 4 x {E_GAP:.1e})")
    assert rep.converged and rep.e[-1] <= tol
    assert e64 <= tol + 4 * E_GAP, (shape, e64)


def residual_fp64(delta, sigma_bar):
    Q = delta.double() / sigma_bar
    if Q.shape[0] > Q.shape[1]:
        Q = Q.t()
    G = Q @ Q.t()
    s = G.shape[0]
    return float(torch.linalg.norm(G - torch.eye(s, dtype=torch.float64, device=G.device)) / s ** 0.5)


# ---- 5. host logic ---------------------------------------------------------------------------------------------------
def expected_profile(steps, transposed, zero=False):
    if zero:
        want = {"iso_sum": 1, "iso_norm": 1, "geo_gram_fold": 1, "iso_apply": 1}
    else:
        q, c = steps.count("q"), steps.count("c")
        want = {"iso_sum": 1, "iso_norm": 1, "iso_scale": 1, "iso_gemm_nt": len(steps) + 1 + q, "iso_gemm_nn": q + c,
                "iso_resid": len(steps) + 1, "iso_dot": 1, "geo_gram_fold": len(steps) + 3, "iso_apply": 1}
        if not want["iso_gemm_nn"]:
            del want["iso_gemm_nn"]
    if transposed:
        want["iso_transpose"] = 1 if zero else 2
    return want


def check_profile(engine, shape, k, max_iter=40, zero=False):
    fts, bases, base_out = merge_inputs(shape, k)
    if zero:
        fts = list(bases)
    reps = []
    table = harness.profile_of(engine, lambda: reps.append(iso(engine, fts, bases, list(ALPHAS[:k]), base_out, max_iter=max_iter)[1]))
    rep = reps[0]
    assert rep.zero == zero and table == expected_profile(rep.steps, rep.transposed, zero), (rep.steps, table)
    return rep


def check_c_abi(engine):
    fts, bases, base_out = merge_inputs((32, 48), 2)
    ft, base = on(engine, fts[0]), on(engine, bases[0])
    out = torch.empty_like(base)
    dll, h = engine.lib.dll, engine.ctx.h
    need = int(dll.smhip_iso_workspace(32, 48))
    assert need >= 3 * 32 * 48 * 4 + 2 * 32 * 32 * 4
    assert dll.smhip_iso_workspace(0, 48) == 0 and dll.smhip_iso_workspace(32, -1) == 0
    assert dll.smhip_iso_workspace(16385, 16385) == 0 and dll.smhip_iso_workspace(16384, 100000) > 0
    ws = engine._xl_workspace(need)

    def call(k=2, alpha=1.0, out_t=out, **over):
        d = _lib.IsoDesc()
        d.k = k
        for i in range(max(0, min(k, 16))):
            d.finetune[i], d.base[i], d.alpha[i] = ft.data_ptr(), base.data_ptr(), alpha
        f = dict(in_dtype=_lib.BF16, base_out=base.data_ptr(), base_out_dtype=_lib.BF16, n=32 * 48, rows=32, cols=48, lam=1.0,
                 tol=1e-4, max_iter=40, workspace=ws.data_ptr(), workspace_bytes=need)
        f.update(over)
        for key, value in f.items():
            setattr(d, key, value)
        rep = _lib.IsoReport()
        rc = dll.smhip_iso_merge(h, C.byref(d), out_t.data_ptr(), None, C.byref(rep), engine._stream())
        return rc, dll.smhip_last_error(h).decode(), rep

    rc, msg, rep = call()
    assert rc == _lib.OK and (rep.s, rep.L, rep.transposed, rep.converged) == (32, 48, 0, 1), msg
    for kwargs, word in (({"k": 0}, "k out of range"), ({"k": 17}, "k out of range"), ({"alpha": float("nan")}, "alpha"),
                         ({"lam": float("inf")}, "lambda"), ({"tol": 0.0}, "tol"), ({"tol": 1.5}, "tol"), ({"tol": float("nan")}, "tol"),
                         ({"max_iter": -1}, "max_iter"), ({"max_iter": 201}, "max_iter"), ({"rows": 0}, "rows"),
                         ({"cols": 47}, "rows * cols"), ({"in_dtype": 3}, "dtype"), ({"base_out_dtype": -1}, "dtype"),
                         ({"out_t": ft}, "overlaps"), ({"workspace": None}, "workspace"), ({"workspace_bytes": need - 1}, "workspace"),
                         ({"workspace": ws.data_ptr() + 8}, "workspace"), ({"base_out": None}, "null")):
        rc, msg, _ = call(**kwargs)
        assert rc == _lib.ERR_ARG and word in msg and "iso_merge" in msg, (kwargs, rc, msg)
    # s > 16384 is rejected before any tensor is read: the pointers are made-up addresses a terabyte apart
    d = _lib.IsoDesc()
    d.k, d.finetune[0], d.base[0], d.alpha[0] = 1, 1 << 40, 2 << 40, 1.0
    d.in_dtype = d.base_out_dtype = _lib.BF16
    d.base_out, d.n, d.rows, d.cols, d.lam, d.tol, d.max_iter = 3 << 40, 16385 * 16385, 16385, 16385, 1.0, 1e-4, 40
    d.workspace, d.workspace_bytes = ws.data_ptr(), need
    rc = dll.smhip_iso_merge(h, C.byref(d), C.c_void_p(4 << 40), None, None, engine._stream())
    assert rc == _lib.ERR_ARG and "exceeds 16384" in dll.smhip_last_error(h).decode()
    assert dll.smhip_iso_merge(h, None, out.data_ptr(), None, None, None) == _lib.ERR_ARG
    rc, msg, rep = call(n=0, out_t=ft)                              # a no-op, whatever the pointers
    assert rc == _lib.OK and rep.s == 0 and rep.iterations == 0
    # the probe
    x = on(engine, torch.ones(8, 8))
    y = torch.empty_like(x)

    def probe(**over):
        d = _lib.IsoGemmDesc()
        f = dict(form=0, sym=0, epilogue=0, M=8, N=8, K=8, a=x.data_ptr(), lda=8, b=x.data_ptr(), ldb=8, e=None, lde=0, ca=1.0, cb=1.0,
                 c=y.data_ptr(), ldc=8)
        f.update(over)
        for key, value in f.items():
            setattr(d, key, value)
        return dll.smhip_iso_gemm(h, C.byref(d), engine._stream()), dll.smhip_last_error(h).decode()

    assert probe()[0] == _lib.OK and bool((host(y) == 8).all())
    for kwargs, word in (({"form": 2}, "form"), ({"epilogue": 4}, "epilogue"), ({"M": 0}, "shape"), ({"K": 0}, "shape"), ({"sym": 2}, "sym"),
                         ({"sym": 1, "form": 1}, "sym"), ({"sym": 1, "M": 4}, "sym"), ({"a": None}, "null"), ({"epilogue": 1}, "null"),
                         ({"c": x.data_ptr()}, "overlaps"), ({"lda": 7}, "pitch"), ({"ldc": 7}, "pitch"), ({"a": x.data_ptr() + 2}, "aligned")):
        rc, msg = probe(**kwargs)
        assert rc == _lib.ERR_ARG and word in msg and "iso_gemm" in msg, (kwargs, rc, msg)
    assert dll.smhip_iso_gemm(h, None, None) == _lib.ERR_ARG
    # the engine's own checks
    for kw in (dict(lam=float("nan")), dict(tol=0.0), dict(tol=2.0), dict(max_iter=-1), dict(max_iter=201), dict(max_iter=2.0), dict(max_iter=True)):
        with pytest.raises(ValueError, match="iso_merge"):
            engine.iso_merge([ft], [base], [1.0], base, **kw)
    with pytest.raises(ValueError, match="at least two dimensions"):
        engine.iso_merge([ft.reshape(-1)], [base.reshape(-1)], [1.0], base.reshape(-1))


# ---- 6. the CLI on the synthetic on-disk model of tests/lora_fixtures.py ------------------------------------------
OPTIONS = {"operator": "iso_c", "iso_lambda": 0.7, "iso_tol": 1e-3, "iso_max_iter": 30}


def write_config(root, third, out_dir, options=OPTIONS, device=None, models=None):
    return harness.write_config(root, models or ties_models(third), out_dir, options, device)


def expected_outputs(base, full, opts, models=None):
    """the oracle tensor by tensor: matrices by iso_oracle.merge, 1-D block tensors by dare_linear at density 1, the
    passthrough tensors from their provider"""
    lam, tol, it = opts.get("iso_lambda", 1.0), opts.get("iso_tol", 1e-4), opts.get("iso_max_iter", 40)

    def merge(fts, bases, alphas, base_out, name):
        if base_out.ndim < 2:
            return dare_oracle.dare_merge(fts, bases, alphas, base_out, density=1.0, lam=lam, normalize=True, rescale=True,
                                          sign_election=False, key=0, stream_ids=list(range(len(fts))))[0]
        return io.merge(fts, bases, alphas, base_out, lam, tol, it)["out"]

    return expected_by_tensor(base, full, models or ties_models("org/lora_full"), merge)


def check_cli(tmp_path, engine, device=None, third="org/lora_full"):
    base, factors, full = lf.setup_k3(tmp_path, engine)
    expected = expected_outputs(base, full, OPTIONS)
    assert any(not torch.equal(expected[n], base[n]) for n in expected if "layers" in n)
    res = run_cli(write_config(tmp_path, third, "merged", device=device))
    assert res.exit_code == 0, res.output
    harness.assert_outputs(tmp_path / "merged", expected)
    readme = (tmp_path / "merged" / "README.md").read_text()
    for word in ("# Iso-C Merged Model", "Iso-C (", "lambda 0.7", "tol 0.001", "max_iter 30"):
        assert word in readme, (word, readme)
    return expected
