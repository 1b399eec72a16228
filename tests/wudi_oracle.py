"""smhip_wudi_merge and the three kernels of smhip_wudi_gemm restated in numpy from the text of include/shardmerge_hip.h:
iso_oracle's fmaf chains in ascending k and ordered fp64 sums, one IEEE operation per step; the HIP path and the emulator
must equal this bit for bit.  ``iterate_fp64`` and ``loss`` are the same iteration and the objective in torch fp64: what
the property tests measure against.  Test infrastructure of that feature."""
import numpy as np
import torch

from tests import extract_oracle as xo
from tests import iso_oracle as io

f32, f64 = np.float32, np.float64
B1, B2, EPS = f32(0.9), f32(0.999), f32(1e-8)
C1, C2 = f32(f64(1.0) - f64(0.9)), f32(f64(1.0) - f64(0.999))


def schedule(lr, t):
    """(s_t, q_t) of step t: the powers by repeated fp64 products"""
    b1t = b2t = f64(1.0)
    for _ in range(t):
        b1t, b2t = b1t * f64(0.9), b2t * f64(0.999)
    return f32(f64(lr) / (f64(1.0) - b1t)), f32(f64(1.0) / np.sqrt(f64(1.0) - b2t))


def gram(d, w, s=None):
    """d [K x N] fp32 -> (Sh, S): Sh = w d^T d; S = Sh, or s + Sh"""
    with np.errstate(all="ignore"):
        sh = f32(w) * io.gemm(d.T, d.T)
        return sh, (sh if s is None else np.asarray(s, dtype=f32) + sh)


def rhs(d, b, p=None):
    """d [M x K], b [N x K] -> the chains d b^T, or p + them"""
    with np.errstate(all="ignore"):
        acc = io.gemm(d, b)
        return acc if p is None else np.asarray(p, dtype=f32) + acc


def step(a, b, p, m, v, x, lr, t):
    """step 7 on acc = a b^T -> (m', v', X', g)"""
    st, qt = schedule(lr, t)
    one = lambda c: np.full((1, 1), c, dtype=f32)
    with np.errstate(all="ignore"):
        g = f32(2.0) * (io.gemm(a, b) - p)
        m1 = xo.fma32(one(B1), m, C1 * g)
        v1 = xo.fma32(one(B2), v, (C2 * g) * g)
        return m1, v1, x - st * (m1 / (np.sqrt(v1) * qt + EPS)), g


def merge(finetunes, bases, alphas, base_out: torch.Tensor, iters=300, lr=1e-5, lam=1.0):
    """-> dict: out, merged, X0 and every field of the report"""
    shape = base_out.shape
    R, C = shape[0], int(np.prod(shape[1:]))
    with np.errstate(all="ignore"):
        ds = [xo.delta(ft, bs).reshape(R, C) for ft, bs in zip(finetunes, bases)]
    bad = [i for i, d in enumerate(ds) if not np.isfinite(d).all()]
    if bad:
        raise ValueError(f"NaN or Inf in finetune - base of finetune {', '.join(map(str, bad))}")
    n = [io.ordered_sum(d.astype(f64) ** 2) for d in ds]
    active = [i for i in range(len(ds)) if float(alphas[i]) != 0.0 and n[i] != 0.0]
    w = [float(f32(f64(alphas[i]) / f64(n[i]))) if i in active else 0.0 for i in range(len(ds))]
    rep = {"R": R, "C": C, "active": active, "n": n, "w": w, "iterations": iters, "zero": not active, "grad_sq_first": 0.0,
           "grad_sq_last": 0.0}
    X = np.zeros((R, C), dtype=f32)
    if active:
        S = P = None
        for i in active:
            sh, S = gram(ds[i], w[i], S)
            P = rhs(ds[i], sh, P)
        X = rep["X0"] = io.task_sum(finetunes, bases, alphas)[0]
        m, v = np.zeros_like(X), np.zeros_like(X)
        for t in range(1, iters + 1):
            m, v, X, g = step(X, S, P, m, v, X, lr, t)
            if t in (1, iters):
                rep["grad_sq_last"] = io.ordered_sum(g.astype(f64) ** 2)
                rep["grad_sq_first"] = rep["grad_sq_last"] if t == 1 else rep["grad_sq_first"]
    out32 = xo.fma32(np.full((1, 1), lam, dtype=f32), X, base_out.float().numpy().reshape(R, C))
    rep["merged"] = X.reshape(shape)
    rep["out"] = torch.from_numpy(out32).to(base_out.dtype).reshape(shape)
    return rep


def loss(X, deltas) -> float:
    """L(X) = sum_i ||(X - d_i) d_i^T||_F^2 / ||d_i||_F^2 in torch fp64"""
    X = torch.as_tensor(X).double()
    return float(sum(torch.linalg.norm((X - d.double()) @ d.double().T) ** 2 / torch.linalg.norm(d.double()) ** 2 for d in deltas))


def iterate_fp64(deltas, iters, lr):
    """the same iteration in torch fp64 with alphas 1: deltas, products and Adam, the same constants -> (X, [g_1 .. g_iters])"""
    ds = [d.double() for d in deltas]
    S = sum(d.T @ d / (d * d).sum() for d in ds)
    P = sum(d @ (d.T @ d) / (d * d).sum() for d in ds)
    X = sum(ds)
    m, v, gs = torch.zeros_like(X), torch.zeros_like(X), []
    for t in range(1, iters + 1):
        g = 2.0 * (X @ S - P)
        m = 0.9 * m + (1.0 - 0.9) * g
        v = 0.999 * v + (1.0 - 0.999) * g * g
        X = X - lr / (1.0 - 0.9 ** t) * m / (v.sqrt() / (1.0 - 0.999 ** t) ** 0.5 + 1e-8)
        gs.append(g)
    return X, gs
