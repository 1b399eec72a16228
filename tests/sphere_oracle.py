"""A restatement of smhip_sphere_merge (include/shardmerge_hip.h: karcher, multislerp) in numpy fp64, written from the
header's text.  Steps 1, 2 and 4 - the vectors, the ordered fp64 Gram, the fp32 combination - are those of
smhip_geo_merge and come from tests/geo_oracle.py by import.  Step 3 is restated here one IEEE operation per line (numpy
float64 never fuses), vectorised over the rows with per-row stop masks: a whole-tensor call is one row.  sm_acos /
sm_sin / sm_cos are restated from the header's description (the series, their lengths, the reductions) with the
coefficients computed HERE as exact rationals rounded to fp64, not copied from the kernel source."""
import math
from fractions import Fraction

import numpy as np
import torch

from tests import geo_oracle

MODES = ("karcher", "multislerp")
PI, PIO2 = math.pi, math.pi / 2            # fp64(pi), fp64(pi / 2)
SMALL, QMIN = 1e-8, 1e-16
CONVERGED, LINEAR = 1, 2

# asin: (2m)! / (4^m (m!)^2 (2m + 1)), m = 0..23; sin: (-1)^m / (2m + 1)!, m = 0..11; cos: (-1)^m / (2m)!, m = 0..12
ASIN = [float(Fraction(math.factorial(2 * m), 4 ** m * math.factorial(m) ** 2 * (2 * m + 1))) for m in range(24)]
SIN = [float(Fraction((-1) ** m, math.factorial(2 * m + 1))) for m in range(12)]
COS = [float(Fraction((-1) ** m, math.factorial(2 * m))) for m in range(13)]


def _horner(c, z):
    p = np.full_like(z, c[-1])
    for ci in reversed(c[:-1]):
        p = p * z
        p = p + ci
    return p


def _asin_half(z):
    z2 = z * z
    return z * _horner(ASIN, z2)


def sm_acos(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        up = (1.0 + (-x)) * 0.5
        hi = 2.0 * _asin_half(np.sqrt(up))
        dn = (1.0 + x) * 0.5
        lo = 2.0 * _asin_half(np.sqrt(dn))
        lo = PI + (-lo)
        mid = PIO2 + (-_asin_half(x))
        return np.where(x > 0.5, hi, np.where(x < -0.5, lo, mid))


def _reflect(x):
    x = np.asarray(x, dtype=np.float64)
    up = x > PIO2
    return up, np.where(up, PI + (-x), x)


def sm_sin(x):
    with np.errstate(all="ignore"):
        _, y = _reflect(x)
        y2 = y * y
        return y * _horner(SIN, y2)


def sm_cos(x):
    with np.errstate(all="ignore"):
        up, y = _reflect(x)
        y2 = y * y
        v = _horner(COS, y2)
        return np.where(up, -v, v)


FNS = {"acos": sm_acos, "sin": sm_sin, "cos": sm_cos}


def _quad(H, v):
    k = v.shape[1]
    Q = np.zeros(v.shape[0])
    for i in range(k):
        r = np.zeros(v.shape[0])
        for j in range(k):
            r = r + H[:, i, j] * v[:, j]
        Q = Q + v[:, i] * r
    return Q


def coefficients(G, alphas, max_iter=10, tol=1e-5):
    """step 3 for R Grams at once.  G: float64 [R][k][k].  -> dict(c fp32 [R][k], a, w, H, N, iterations, flags, tau)"""
    G = np.asarray(G, dtype=np.float64)
    R, k = G.shape[0], G.shape[1]
    A = 0.0
    for al in alphas:
        A = A + float(al)
    assert all(float(al) >= 0 for al in alphas) and A > 0
    with np.errstate(all="ignore"):
        n = np.sqrt(np.stack([G[:, i, i] for i in range(k)], axis=1))
        w0 = np.array([float(al) / A for al in alphas])
        active = (n > 0.0) & (w0 > 0.0)[None, :]
        W = np.zeros(R)
        for i in range(k):
            W = np.where(active[:, i], W + w0[i], W)
        nact = active.sum(axis=1)
        w = np.where(active, w0[None, :] / W[:, None], 0.0)
        N = np.zeros(R)
        for i in range(k):
            N = N + w[:, i] * n[:, i]
        H = np.zeros((R, k, k))
        for i in range(k):
            H[:, i, i] = 1.0
            for j in range(i + 1, k):
                p = n[:, i] * n[:, j]
                c = G[:, i, j] / p
                c = np.where(c > 1.0, 1.0, np.where(c < -1.0, -1.0, c))
                H[:, i, j] = H[:, j, i] = np.where((p == 0.0) | ~np.isfinite(p), 0.0, c)
        a = w.copy()
        iterations = np.zeros(R, dtype=np.int32)
        flags = np.zeros(R, dtype=np.int32)
        tau_out = np.zeros(R)
        coef = np.zeros((R, k), dtype=np.float32)
        done = nact <= 1
        flags[done] = CONVERGED
        coef[done] = a[done].astype(np.float32)
        q = _quad(H, a)
        lin = ~done & (~(q > QMIN) | ~np.isfinite(q))
        flags[lin] = LINEAR
        done = done | lin
        a = np.where(done[:, None], a, a / np.sqrt(q)[:, None])
        for it in range(max_iter):
            live = ~done
            if not live.any():
                break
            iterations[live] = it + 1
            g = np.zeros(R)
            t = np.zeros((R, k))
            for j in range(k):
                d = np.zeros(R)
                for i in range(k):
                    d = d + a[:, i] * H[:, i, j]
                d = np.where(d > 1.0, 1.0, np.where(d < -1.0, -1.0, d))
                th = sm_acos(d)
                sn = sm_sin(th)
                f = np.where(th < SMALL, 1.0, np.where(sn < SMALL, 0.0, th / sn))
                p = w[:, j] * f
                t[:, j] = p
                g = g + p * d
            for i in range(k):
                t[:, i] = t[:, i] + (-(a[:, i] * g))
            tau2 = _quad(H, t)
            bad = live & ~np.isfinite(tau2)
            flags[bad] = LINEAR
            done = done | bad
            live = live & ~bad
            tau = np.sqrt(np.where(tau2 > 0.0, tau2, 0.0))
            tau = np.where(tau > PI, PI, tau)
            tau_out[live] = tau[live]
            conv = live & (tau < tol)
            flags[conv] = CONVERGED
            done = done | conv
            live = live & ~conv
            cs = sm_cos(tau)
            sc = np.where(tau < SMALL, 1.0, sm_sin(tau) / tau)
            an = np.empty_like(a)
            for i in range(k):
                an[:, i] = cs * a[:, i] + sc * t[:, i]
            q = _quad(H, an)
            bad = live & (~(q > QMIN) | ~np.isfinite(q))
            flags[bad] = LINEAR
            a = np.where(bad[:, None], an, a)
            done = done | bad
            live = live & ~bad
            a = np.where(live[:, None], an / np.sqrt(q)[:, None], a)
        linear = (flags & LINEAR) != 0
        coef[linear] = w[linear].astype(np.float32)
        normal = ~linear & (nact > 1)
        c = np.where(w > 0.0, (a * N[:, None]) / n, 0.0).astype(np.float32)
        coef[normal] = c[normal]
    return {"c": coef, "a": a, "w": w, "H": H, "N": N, "iterations": iterations, "flags": flags, "tau": tau_out}


def sphere_merge(fts, bases, alphas, base_out, mode="karcher", rowwise=False, max_iter=10, tol=1e-5):
    """-> dict(out, delta, ...): whole tensor G, H, w, a, N, c, iterations, tau, converged, linear; row-wise c_rows,
    iters_rows, flags_rows, iters_max, rows_unconverged, rows_linear, csum_min, csum_max, csum_mean"""
    assert mode in MODES
    k, shape = len(fts), tuple(base_out.shape)
    n = base_out.numel()
    geo_mode = "slerp" if mode == "karcher" else "nuslerp"          # weight space / delta space
    xs = geo_oracle.vectors(fts, bases, geo_mode)
    for i, x in enumerate(xs):
        if not bool(torch.isfinite(x).all()):
            raise ValueError(f"non-finite vector of finetune {i}")
    if n == 0:
        return {"out": torch.empty(shape, dtype=base_out.dtype), "delta": torch.empty(shape, dtype=torch.float32)}
    if rowwise:
        R = shape[0] if len(shape) > 1 else 1
        res = coefficients(geo_oracle.gram_rows(xs, R), alphas, max_iter, tol)
        view = (R,) + (1,) * (len(shape) - 1) if len(shape) > 1 else (1,)
        coefs = [torch.from_numpy(np.ascontiguousarray(res["c"][:, i])).view(view) for i in range(k)]
        out, M = geo_oracle.combine(xs, coefs, base_out, geo_mode, shape)
        sums = []
        for r in range(R):
            s = 0.0
            for i in range(k):
                s = s + float(res["c"][r, i])
            sums.append(s)
        total = 0.0
        for s in sums:
            total = total + s
        return {"out": out, "delta": M, "c_rows": res["c"], "iters_rows": res["iterations"], "flags_rows": res["flags"],
                "iters_max": int(res["iterations"].max()), "rows_unconverged": int(((res["flags"] & CONVERGED) == 0).sum()),
                "rows_linear": int(((res["flags"] & LINEAR) != 0).sum()),
                "csum_min": min(sums), "csum_max": max(sums), "csum_mean": total / float(R)}
    G = geo_oracle.gram_whole(xs)
    res = coefficients(np.array([G], dtype=np.float64), alphas, max_iter, tol)
    c = [np.float32(v) for v in res["c"][0]]
    out, M = geo_oracle.combine(xs, c, base_out, geo_mode, shape)
    return {"out": out, "delta": M, "G": G, "H": res["H"][0].tolist(), "w": res["w"][0].tolist(), "a": res["a"][0].tolist(),
            "N": float(res["N"][0]), "c": [float(v) for v in c], "iterations": int(res["iterations"][0]), "tau": float(res["tau"][0]),
            "converged": bool(res["flags"][0] & CONVERGED), "linear": bool(res["flags"][0] & LINEAR)}
