"""smhip_tsv_merge restated in numpy from the text of include/shardmerge_hip.h, on the primitives of
tests/extract_oracle.py (the exact fp32 fma, the delta products, the ordered fp64 Gram, the Jacobi eigensolver).  The HIP
path and the emulator must equal this bit for bit.  ``merge_fp64`` evaluates the same definition in plain fp64 (LAPACK
SVD and eigh): the distance between the two is what the property tests' tolerances are measured from.  Test
infrastructure of that feature."""
import numpy as np
import torch

from tests import extract_oracle as xo
from tests import geo_oracle

MAX_R = 256


def chain_order(Rp):
    """the k of every chain position: inside a block of 16, k0 + 4 g + j in the order j = 0..3 outside, g = 0..3 inside"""
    return [b + 4 * g + j for b in range(0, Rp, 16) for j in range(4) for g in range(4)]


def apply(B, W, base_out: torch.Tensor, lam):
    """tsv_apply: B [rows x Rp], W [cols x Rp] fp32 -> (out in base_out's dtype, merged fp32)"""
    rows, cols = base_out.shape
    acc = np.zeros((rows, cols), dtype=np.float32)
    for k in chain_order(B.shape[1]):
        acc = xo.fma32(B[:, k:k + 1], W[:, k][None, :], acc)
    base32 = base_out.float().numpy()
    out32 = xo.fma32(np.full((1, 1), np.float32(lam)), acc, base32)
    return torch.from_numpy(out32).to(base_out.dtype), acc


def range_finder(D, omega, power_iters):
    """steps 2 - 4 of smhip_lora_extract -> (Q, C, orth ranks)"""
    ranks = []

    def orth_(Y):
        Q, kept = xo.orth(Y)
        ranks.append(kept)
        return Q
    Y = xo.delta_mm(D, omega, 0)
    for _ in range(power_iters):
        Z = xo.delta_mm(D, orth_(Y), 1)
        Y = xo.delta_mm(D, orth_(Z), 0)
    Q = orth_(Y)
    return Q, xo.delta_mm(D, Q, 1), ranks


def whiten(P, R):
    """-> (S [R x R] fp64, mu [R], kept)"""
    mu, E = xo.sym_eig(xo.gram(P)[:R, :R])
    S = np.zeros((R, R), dtype=np.float64)
    cut = np.float64(1e-6) * mu[0]
    kept = 0
    with np.errstate(all="ignore"):
        for j in range(R):
            if mu[j] > cut:
                kept += 1
                S = S + np.outer(E[:, j], E[:, j]) / np.sqrt(mu[j])
    return S, mu, kept


def merge(finetunes, bases, alphas, base_out: torch.Tensor, rank, power_iters, lam, key):
    """-> dict: out, merged, and every field of the report"""
    rows, cols = base_out.shape
    k = len(finetunes)
    r = min(rank, rows, cols)
    L = xo.panel_width(rows, cols, r)
    omega = xo.fill(cols, L, key)
    rep = {"L": L, "r": r, "rho": [0] * k, "sigma": [[0.0] * r for _ in range(k)], "delta_sq": [0.0] * k, "share": [0.0] * k,
           "orth_ranks": [[] for _ in range(k)], "mu_U": [], "mu_W": [], "kept_U": 0, "kept_W": 0}
    Us, Ws, s = [], [], []
    for i in range(k):
        if float(alphas[i]) == 0.0:
            continue
        D = xo.delta(finetunes[i], bases[i])
        if not np.isfinite(D).all():
            raise ValueError(f"NaN or Inf in finetune {i}")
        Q, Cm, ranks = range_finder(D, omega, power_iters)
        lam_, V = xo.sym_eig(xo.gram(Cm))
        sigma = np.sqrt(np.maximum(lam_, 0.0))
        cut = np.float64(1e-12) * lam_[0]
        rho, total = 0, np.float64(0.0)
        for j in range(r):
            total = total + max(lam_[j], np.float64(0.0))
            if lam_[j] > cut and rho == j:
                rho += 1
        delta_sq = geo_oracle.gram_whole([torch.from_numpy(D).reshape(-1)])[0][0]
        rep["rho"][i], rep["sigma"][i], rep["orth_ranks"][i] = rho, [float(v) for v in sigma[:r]], ranks
        rep["delta_sq"][i] = float(delta_sq)
        rep["share"][i] = float(total / delta_sq) if delta_sq > 0 else 0.0
        if rho:
            Us.append(xo.panel_mm(Q, V[:, :rho].astype(np.float32)))
            Ws.append(xo.panel_mm(Cm, (V[:, :rho] / sigma[None, :rho]).astype(np.float32)))
        s += [np.float64(alphas[i]) * sigma[j] for j in range(rho)]
    R = sum(rep["rho"])
    Rp = xo.ceil16(R)
    rep["R"], rep["Rp"] = R, Rp
    U = np.zeros((rows, Rp), dtype=np.float32)
    W = np.zeros((cols, Rp), dtype=np.float32)
    B = np.zeros((rows, Rp), dtype=np.float32)
    if R:
        U[:, :R] = np.concatenate(Us, axis=1)
        W[:, :R] = np.concatenate(Ws, axis=1)
        SU, mu_U, rep["kept_U"] = whiten(U, R)
        SW, mu_W, rep["kept_W"] = whiten(W, R)
        rep["mu_U"], rep["mu_W"] = [float(v) for v in mu_U], [float(v) for v in mu_W]
        M = np.zeros((R, R), dtype=np.float64)
        for c in range(R):
            M = M + (SU[:, c:c + 1] * s[c]) * SW[c:c + 1, :]
        M32 = np.zeros((Rp, Rp), dtype=np.float32)
        M32[:R, :R] = M.astype(np.float32)
        B = xo.panel_mm(U, M32)
    rep["out"], rep["merged"] = apply(B, W, base_out, lam)
    rep["s"] = [float(v) for v in s]
    return rep


def merge_fp64(finetunes, bases, alphas, rank):
    """the definition in exact-SVD form, fp64 throughout: the r leading triplets of every delta by LAPACK, Loewdin
    whitening with the same 1e-6 cutoff, the merged delta.  -> (merged fp64, s sorted descending)"""
    Us, Ws, s = [], [], []
    for ft, bs, a in zip(finetunes, bases, alphas):
        if float(a) == 0.0:
            continue
        D = xo.delta(ft, bs).astype(np.float64)
        u, sv, vt = np.linalg.svd(D, full_matrices=False)
        r = min(rank, len(sv))
        rho = int(np.sum(sv[:r] ** 2 > 1e-12 * sv[0] ** 2)) if sv[0] > 0 else 0
        Us.append(u[:, :rho]); Ws.append(vt[:rho].T); s += list(float(a) * sv[:rho])
    rows, cols = finetunes[0].shape
    if not s:
        return np.zeros((rows, cols)), np.zeros(0)
    U, W = np.concatenate(Us, axis=1), np.concatenate(Ws, axis=1)

    def inv_sqrt(P):
        mu, E = np.linalg.eigh(P.T @ P)
        keep = mu > 1e-6 * mu.max()
        return (E[:, keep] / np.sqrt(mu[keep])) @ E[:, keep].T
    M = inv_sqrt(U) @ np.diag(s) @ inv_sqrt(W)
    return U @ M @ W.T, np.sort(np.array(s))[::-1]
