"""Checks of the bf16x3 product of Iso-C (csrc/sm_iso3.hpp) for the emulator and the GPU tier.  The device is not held to
the emulator's bits in this mode (include/shardmerge_hip.h): exact integers decide the operand layout and the presence
of all six terms, everything else is held to the header's bound against a numpy fp64 product."""
import numpy as np
import torch

from tests import iso_checks as ic
from tests import iso_oracle as io
from tests.extract_checks import bits32, host, on

MN = (1, 31, 33, 129)
KS = (1, 15, 16, 17, 33, 130)
CA, CB = 1.25, -0.3
U = 2.0 ** -23                                      # one addition of an adder that truncates


def product(engine, a, b, form, **kw):
    return host(engine.iso_gemm(on(engine, a), on(engine, b), form=form, gemm="bf16x3", **kw)).double().numpy()


def check_integers(engine, form, M, N, K, swap):
    """odd integers in (2^16, 2^18) - three non-zero pieces - against {-2 .. 2}: every partial sum is below 2^24, so any
    order of addition is exact and the result is the int64 product.  swap: the wide operand is b (the a0 b2 term)"""
    g = torch.Generator().manual_seed(100 * M + 10 * N + K + swap)
    wide = lambda *s: (torch.randint(2 ** 15, 2 ** 17, s, generator=g) * 2 + 1) * (torch.randint(0, 2, s, generator=g) * 2 - 1)
    small = lambda *s: torch.randint(-2, 3, s, generator=g)
    bs = (N, K) if form == io.NT else (K, N)
    a, b = (small(M, K), wide(*bs)) if swap else (wide(M, K), small(*bs))
    ref = a @ (b.T if form == io.NT else b)
    got = product(engine, a.float(), b.float(), form)
    assert np.array_equal(got.astype(np.int64), ref.numpy()), (form, M, N, K, swap)


def operand(rows, cols, seed, offset=0):
    """Gaussian values scaled by 2^-j, j in 0..20, their magnitudes held to [2^-20, 1]; a view `offset` elements into its
    storage (not 16-byte aligned; an odd `cols` is an odd pitch)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(offset + rows * cols, generator=g) * 2.0 ** -torch.randint(0, 21, (offset + rows * cols,), generator=g).float()
    return torch.copysign(x.abs().clamp(2.0 ** -20, 1.0), x)[offset:].view(rows, cols)


def check_bound(engine, form, M, N, K, ep=io.PLAIN, sym=False, offset=0):
    """|C - C64| <= (6 K + 1) 2^-23 (|A| |B|) per element; an epilogue's two rounded operations add 2^-23 of what they
    add up.  Returns the worst share of the bound met"""
    a = operand(M, K, 7 * M + K, offset)
    b = a if sym else operand(*((N, K) if form == io.NT else (K, N)), 11 * N + K + 1, offset)
    e = operand(M, N, 13 * M + N + 2, offset)
    a64, b64, e64 = (t.double().numpy() for t in (a, b, e))
    b64 = b64.T if form == io.NT else b64
    c64, bound = a64 @ b64, (6 * K + 1) * U * (np.abs(a64) @ np.abs(b64))
    got = product(engine, a, b, form, sym=sym, epilogue=ep, ca=CA, cb=CB, e=on(engine, e) if ep else None)
    if ep:
        wa, we = {io.POLY: (CA, CB), io.AXPY: (1.0, CA), io.CUBIC: (CB, CA)}[ep]          # the weights of acc and of e
        bound = abs(wa) * bound + U * (abs(wa) * (np.abs(c64) + bound) + np.abs(we * e64))
        c64 = wa * c64 + we * e64
    share = float((np.abs(got - c64) / bound).max())
    print(f"form {form} {M}x{N}x{K} ep {ep} sym {sym} offset {offset}: worst share of the bound {share:.4f}")
    assert share <= 1.0, (form, M, N, K, ep, sym, share)
    if sym:
        assert np.array_equal(bits32(got), bits32(got.T)), (M, K, "not symmetric")
    return share


def check_merge(engine, ref_engine, shape):
    """gemm="bf16x3" converges, and its three deviations from torch fp64 linalg.svd's mean(S) U V^T stay within 4 x those
    of the fp32 path on the same inputs (ref_engine: the emulator where the shape allows)"""
    fts, bases, base_out = ic.merge_inputs(shape, 2)
    figs = {}
    for mode, eng in (("fp32", ref_engine), ("bf16x3", engine)):
        args = ([on(eng, t) for t in fts], [on(eng, bases[0])] * 2, [1.0, 0.7], on(eng, base_out))
        out, rep, delta = eng.iso_merge(*args, want_delta=True, gemm=mode, layer_name="layers.0.w")
        assert rep.converged and rep.iterations <= 40, (mode, rep.steps)
        figs[mode] = ic.svd_figures(fts, bases, [1.0, 0.7], host(delta), rep.sigma_bar)
        print(f"{shape} {mode}: steps {rep.steps}, distance {figs[mode][0]:.3e}, sigma_bar {figs[mode][1]:.3e}, spread {figs[mode][2]:.3e}")
    assert all(s <= 4 * f for s, f in zip(figs["bf16x3"], figs["fp32"])), (shape, figs)
    return figs


def _cases():
    """the product's cases by name, each a call on an engine"""
    out = {}
    for form, tag in ((io.NT, "nt"), (io.NN, "nn")):
        for swap in (False, True):
            out[f"integers-{tag}-{'b' if swap else 'a'}_wide"] = lambda e, f=form, s=swap: [
                check_integers(e, f, M, N, K, s) for M, N, K in ((33, 31, 17), (129, 33, 16), (1, 129, 9))]
        for K in KS:
            out[f"bound-{tag}-K{K}"] = lambda e, f=form, K=K: max(check_bound(e, f, M, N, K) for M in MN for N in MN)
        out[f"bound-{tag}-epilogue"] = lambda e, f=form: check_bound(e, f, 129, 33, 130, ep=io.POLY if f == io.NT else io.CUBIC)
        out[f"bound-{tag}-odd_pitch_view"] = lambda e, f=form: check_bound(e, f, 33, 31, 17, ep=io.AXPY, offset=1)
    out["symmetric-129x129x130"] = lambda e: check_bound(e, io.NT, 129, 129, 130, sym=True)
    return out


CASES = _cases()
