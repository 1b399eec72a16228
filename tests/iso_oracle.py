"""smhip_iso_merge and smhip_iso_gemm restated in numpy from the text of include/shardmerge_hip.h: the exact fp32 fma of
tests/extract_oracle.py, the fmaf chains in ascending k, the ordered fp64 sums (segments, 256 lanes of octets, the binary
tree, segments in index order) with one IEEE operation per step.  The HIP path and the emulator must equal this bit for
bit.  ``merge_fp64`` is the paper's form on LAPACK's fp64 SVD: the distance between the two is what the property tests'
tolerances are measured from.  Test infrastructure of that feature."""
import numpy as np
import torch

from tests import extract_oracle as xo

SEG, LANES = 32768, 256
A5, B5, C5 = (np.float32(float.fromhex(h)) for h in ("0x1.b8e56p+1", "-0x1.31999ap+2", "0x1.040832p+1"))
A3, B3 = np.float32(1.5), np.float32(-0.5)
QUINTIC_ABOVE = 0.35
NT, NN = 0, 1
PLAIN, POLY, AXPY, CUBIC = range(4)


def _s(v):
    return np.full((1, 1), np.float32(v), dtype=np.float32)


def gemm(a, b, form=NT, epilogue=PLAIN, ca=0.0, cb=0.0, e=None):
    """a [M x K]; b [N x K] (NT) or [K x N] (NN) -> ep(a b^T) or ep(a b): one fmaf chain per element from +0 in ascending
    k, and one step fmaf(+0, +0, acc) when K is odd"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    bt = np.ascontiguousarray(b if form == NN else b.T, dtype=np.float32)       # [K x N]
    M, K = a.shape
    acc = np.zeros((M, bt.shape[1]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(K):
            acc = xo.fma32(a[:, k:k + 1], bt[k:k + 1, :], acc)
        if K & 1:
            acc = acc + np.float32(0.0)
        if epilogue == PLAIN:
            return acc
        e = np.asarray(e, dtype=np.float32)
        if epilogue == POLY:
            return xo.fma32(_s(ca), acc, np.float32(cb) * e)
        if epilogue == AXPY:
            return xo.fma32(_s(ca), e, acc)
        return xo.fma32(_s(ca), e, np.float32(cb) * acc)


def ordered_sum(terms) -> float:
    """terms: the fp64 addends of a row-major matrix, flat -> the ordered sum"""
    t = np.asarray(terms, dtype=np.float64).reshape(-1)
    n = t.size
    nseg = -(-n // SEG)
    p = np.zeros(nseg * SEG, dtype=np.float64)
    p[:n] = t                                       # (a missing element adds +0: no lane is ever -0)
    per = SEG // 8 // LANES
    x = p.reshape(nseg, per, LANES, 8)
    lanes = np.zeros((nseg, LANES), dtype=np.float64)
    with np.errstate(all="ignore"):
        for q in range(per):
            for el in range(8):
                lanes = lanes + x[:, q, :, el]
        h = LANES // 2
        while h >= 1:
            lanes = lanes[:, :h] + lanes[:, h:2 * h]
            h //= 2
        total = np.float64(0.0)
        for v in lanes[:, 0]:
            total = total + v
    return float(total)


def task_sum(finetunes, bases, alphas):
    """step 1 -> T fp32 [rows x cols] and the finetunes with a non-finite delta"""
    shape = finetunes[0].shape
    T = np.zeros((shape[0], int(np.prod(shape[1:]))), dtype=np.float32)
    bad = []
    with np.errstate(all="ignore"):
        for i, (ft, bs, al) in enumerate(zip(finetunes, bases, alphas)):
            d = xo.delta(ft, bs).reshape(T.shape)
            if not np.isfinite(d).all():
                bad.append(i)
            T = T + d * np.float32(al)
    return T, bad


def resid(G):
    s = G.shape[0]
    with np.errstate(all="ignore"):
        d = G.astype(np.float64) - np.eye(s, dtype=np.float64)
        return float(np.sqrt(np.float64(ordered_sum(d * d)) / np.float64(s)))


def merge(finetunes, bases, alphas, base_out: torch.Tensor, lam=1.0, tol=1e-4, max_iter=40):
    """-> dict: out, merged, Q (oriented, [s x L]) and every field of the report"""
    shape = base_out.shape
    T, bad = task_sum(finetunes, bases, alphas)
    if bad:
        raise ValueError(f"NaN or Inf in finetune - base of finetune {', '.join(map(str, bad))}")
    rows, cols = T.shape
    tr = rows > cols
    X = np.ascontiguousarray(T.T if tr else T)
    s, L = X.shape
    rep = {"rows": rows, "cols": cols, "s": s, "L": L, "transposed": tr, "iterations": 0, "steps": "", "e": [], "converged": False,
           "N": 0.0, "sigma_bar": 0.0, "zero": False}
    Xd = X.astype(np.float64)
    nu = float(np.sqrt(np.float64(ordered_sum(Xd * Xd))))
    rep["nu"] = nu
    if not np.isfinite(nu):
        raise ValueError("the sum of the weighted deltas is not finite")
    if nu == 0.0:
        rep["zero"] = True
        Q = np.zeros_like(X)
        sig = np.float32(0.0)
    else:
        with np.errstate(all="ignore"):
            Q = X * np.float32(np.float64(1.0) / np.float64(nu))
        t, cubic, prev = 0, False, 0.0
        while True:
            G = gemm(Q, Q)
            e = resid(G)
            rep["e"].append(e)
            if not np.isfinite(e):
                raise ValueError("the iteration left the finite numbers")
            if e <= tol:
                rep["converged"] = True
                break
            if t == max_iter:
                break
            if not e > QUINTIC_ABOVE or (t > 0 and not e < prev):
                cubic = True                    # the quintic phase ends for good
            prev = e
            if not cubic:
                P =gemm(G, G, NT, POLY, C5, B5, G)
                Q = gemm(P, Q, NN, AXPY, A5, 0.0, Q)
                rep["steps"] += "q"
            else:
                Q = gemm(G, Q, NN, CUBIC, A3, B3, Q)
                rep["steps"] += "c"
            t += 1
        rep["iterations"] = t
        N = ordered_sum(Q.astype(np.float64) * Xd)
        rep["N"] = N
        rep["sigma_bar"] = float(np.float64(N) / np.float64(s))
        if not np.isfinite(N):
            raise ValueError("the mean singular value is not finite")
        sig = np.float32(rep["sigma_bar"])
    with np.errstate(all="ignore"):
        merged = np.float32(sig) * Q
    merged = np.ascontiguousarray(merged.T if tr else merged)
    out32 = xo.fma32(_s(lam), merged, base_out.float().numpy().reshape(rows, cols))
    rep["Q"] = Q
    rep["merged"] = merged.reshape(shape)
    rep["out"] = torch.from_numpy(out32).to(base_out.dtype).reshape(shape)
    return rep


def merge_fp64(finetunes, bases, alphas):
    """the paper's form in fp64: T = U S V^T by LAPACK -> (mean(S) U V^T, mean(S), S)"""
    shape = finetunes[0].shape
    T = np.zeros((shape[0], int(np.prod(shape[1:]))), dtype=np.float64)
    for ft, bs, al in zip(finetunes, bases, alphas):
        T += float(al) * xo.delta(ft, bs).reshape(T.shape).astype(np.float64)
    U, S, Vt = np.linalg.svd(T, full_matrices=False)
    return S.mean() * (U @ Vt), float(S.mean()), S
