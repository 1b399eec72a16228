"""smhip_lora_extract restated in numpy from the text of include/shardmerge_hip.h: the Rademacher panel, the two delta
products in their stated chain orders with an EXACT fp32 fma (an fp64 product, TwoSum, round to odd, one cast), the
ordered fp64 Gram, the Jacobi eigensolver one rounded operation at a time, the factors.  The HIP path and the emulator
must equal this bit for bit.  Test infrastructure of that feature."""
import numpy as np
import torch

from tests import dare_oracle, geo_oracle

SEG = 512            # reduction segment of a delta product
GSEG = 256           # rows per segment of a Gram
EIG_SWEEPS = 60
ONE = np.uint64(1)


def ceil16(v):
    return (v + 15) // 16 * 16


def panel_width(rows, cols, rank):
    return min(ceil16(rank + 8), ceil16(min(rows, cols)))


# ---- the exact fp32 fma ----
def fma32(a, b, c):
    """fp32(a * b + c) with ONE rounding, elementwise on float32 arrays.  p = a * b is exact in fp64 (24 + 24 bits);
    s = fl64(p + c) and its error e by TwoSum; where e != 0 and s is even, s moves one ulp towards e (round to odd), so
    that the cast to fp32 sees the sticky bit and cannot round twice."""
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c = c.astype(np.float64)
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (e != 0) & ((s.view(np.uint64) & ONE) == 0)
        if fix.any():
            # towards e: away from zero when e has s's sign (s is never 0 here: then e would be 0)
            up = (e > 0) == (s > 0)
            bits = s.view(np.uint64).copy()
            bits[fix & up] += ONE
            bits[fix & ~up] -= ONE
            s = bits.view(np.float64)
        return s.astype(np.float32)


def fma32_selfcheck():
    """known cases of double rounding: float32(float64(a) * b + c) is wrong on them"""
    a = np.float32(1 + 2.0 ** -12)
    cases = [(a, a, np.float32(2.0 ** -60)), (np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23), np.float32(-1.0)),
             (np.float32(3.0), np.float32(1 / 3), np.float32(2.0 ** -40))]
    from fractions import Fraction
    for x, y, z in cases:
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo = np.float32(float(exact))                       # Python rounds a Fraction correctly to fp64, not fp32: search
        cand = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cand, key=lambda v: (abs(Fraction(float(v)) - exact), int(v.view(np.uint32)) & 1))
        got = fma32(np.array([x]), np.array([y]), np.array([z]))[0]
        assert got == best, (x, y, z, got, best)


# ---- the primitives ----
def fill(nrows, L, key):
    n = nrows * L
    nblk = (n + 127) // 128
    blk = np.arange(nblk, dtype=np.uint64)
    zero = np.zeros(nblk, dtype=np.uint64)
    w = dare_oracle.philox4x32_10(blk & dare_oracle.LO, blk >> dare_oracle.S32, zero, zero, key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF)
    words = np.stack(w, axis=1).reshape(-1)                                     # word (e >> 5): block-major, 4 per block
    bits = (words[:, None] >> np.arange(32, dtype=np.uint64)[None, :]) & ONE    # bit e & 31
    return np.where(bits.reshape(-1)[:n] == 0, np.float32(1), np.float32(-1)).reshape(nrows, L)


def delta(finetune: torch.Tensor, base: torch.Tensor) -> np.ndarray:
    return (finetune.float() - base.float()).numpy()


def delta_mm(D, X, trans):
    """D [rows x cols] fp32, X [K x L] fp32 -> [M x L] fp32 (the fold included)"""
    A = D.T if trans else D                       # [M x K]
    M, K = A.shape
    L = X.shape[1]
    step = 4 if trans else 32
    out = np.zeros((M, L), dtype=np.float32)
    for ks in range(0, K, SEG):
        ke = min(K, ks + SEG)
        n = -(-(ke - ks) // step) * step
        Ap = np.zeros((M, n), dtype=np.float32)
        Xp = np.zeros((n, L), dtype=np.float32)
        Ap[:, :ke - ks] = A[:, ks:ke]
        Xp[:ke - ks] = X[ks:ke]
        if trans:
            order = range(n)
        else:                                     # inside a block of 32: j = 0..7 outside, g = 0..3 inside, k = 8 g + j
            order = [b + 8 * g + j for b in range(0, n, 32) for j in range(8) for g in range(4)]
        acc = np.zeros((M, L), dtype=np.float32)
        for k in order:
            acc = fma32(Ap[:, k:k + 1], Xp[k:k + 1, :], acc)
        with np.errstate(all="ignore"):
            out = out + acc                       # the fold: segments in index order, fp32
    return out


def gram(P):
    """[m x L] fp32 -> [L x L] float64"""
    m, L = P.shape
    Pd = P.astype(np.float64)
    G = np.zeros((L, L), dtype=np.float64)
    with np.errstate(all="ignore"):
        for r0 in range(0, m, GSEG):
            r1 = min(m, r0 + GSEG)
            s = []
            for c in range(4):
                acc = np.zeros((L, L), dtype=np.float64)
                for r in range(r0 + c, r1, 4):
                    acc = acc + np.outer(Pd[r], Pd[r])
                s.append(acc)
            G = G + ((s[0] + s[2]) + (s[1] + s[3]))
    return G


def panel_mm(P, T):
    m, L = P.shape
    acc = np.zeros((m, T.shape[1]), dtype=np.float32)
    for k in range(L):
        acc = fma32(P[:, k:k + 1], T[k:k + 1, :], acc)
    return acc


def sym_eig(G):
    """-> (lam [n] descending, V [n x n] with eigenvector i in column i)"""
    a = np.array(G, dtype=np.float64)
    n = a.shape[0]
    v = np.eye(n, dtype=np.float64)
    scale = np.float64(0.0)
    for i in range(n):
        scale = scale + abs(a[i, i])
    thr = scale * np.float64(2.0 ** -70)
    with np.errstate(all="ignore"):
        for _ in range(EIG_SWEEPS):
            rotated = False
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = a[p, q]
                    if not abs(apq) > thr:
                        continue
                    rotated = True
                    app, aqq = a[p, p], a[q, q]
                    theta = (aqq - app) / (np.float64(2.0) * apq)
                    den = abs(theta) + np.sqrt(theta * theta + np.float64(1.0))
                    t = (np.float64(-1.0) if theta < 0 else np.float64(1.0)) / den
                    c = np.float64(1.0) / np.sqrt(t * t + np.float64(1.0))
                    s = t * c
                    rp, rq = a[p].copy(), a[q].copy()
                    new_p = c * rp - s * rq
                    new_q = s * rp + c * rq
                    a[p] = new_p; a[:, p] = new_p
                    a[q] = new_q; a[:, q] = new_q
                    tap = t * apq
                    a[p, p] = app - tap
                    a[q, q] = aqq + tap
                    a[p, q] = a[q, p] = 0.0
                    vp, vq = v[:, p].copy(), v[:, q].copy()
                    v[:, p] = c * vp - s * vq
                    v[:, q] = s * vp + c * vq
            if not rotated:
                break
    d = np.diag(a).copy()
    order = sorted(range(n), key=lambda i: (-d[i], i)) if not np.isnan(d).any() else list(range(n))
    lam = d[order]
    V = v[:, order].copy()
    for i in range(n):
        big = int(np.argmax(np.abs(V[:, i])))         # the first of the largest
        if V[big, i] < 0:
            V[:, i] = -V[:, i]
    return lam, V


def orth(Y):
    """-> (Q, kept rank)"""
    L = Y.shape[1]
    lam, V = sym_eig(gram(Y))
    cut = np.float64(1e-12) * lam[0]
    T = np.zeros((L, L), dtype=np.float32)
    kept = 0
    for i in range(L):
        if lam[i] > cut:
            kept += 1
            T[:, i] = (V[:, i] / np.sqrt(lam[i])).astype(np.float32)
    return panel_mm(Y, T), kept


def extract(finetune: torch.Tensor, base: torch.Tensor, rank: int, power_iters: int, key: int):
    """-> dict: a32 [rank x cols] and b32 [rows x rank] BEFORE the rounding into the factor dtype (fp32), sigma [L], rho,
    orth_ranks, delta_sq, share, L"""
    D = delta(finetune, base)
    rows, cols = D.shape
    L = panel_width(rows, cols, rank)
    ranks = []

    def orth_(Y):
        Q, kept = orth(Y)
        ranks.append(kept)
        return Q
    Y = delta_mm(D, fill(cols, L, key), 0)
    for _ in range(power_iters):
        Z = delta_mm(D, orth_(Y), 1)
        Y = delta_mm(D, orth_(Z), 0)
    Q = orth_(Y)
    Cm = delta_mm(D, Q, 1)
    lam, V = sym_eig(gram(Cm))
    sigma = np.sqrt(np.maximum(lam, 0.0))
    n = min(rank, L)
    cut = np.float64(1e-12) * lam[0]
    rho, total = 0, np.float64(0.0)
    Tb = np.zeros((L, rank), dtype=np.float32)
    Ta = np.zeros((L, rank), dtype=np.float32)
    for i in range(n):
        total = total + max(lam[i], np.float64(0.0))
        if lam[i] > cut:
            rho += 1
            s = np.sqrt(sigma[i])
            Tb[:, i] = (V[:, i] * s).astype(np.float32)
            Ta[:, i] = (V[:, i] / s).astype(np.float32)
    delta_sq = geo_oracle.gram_whole([torch.from_numpy(D).reshape(-1)])[0][0]
    return {"b32": panel_mm(Q, Tb), "a32": np.ascontiguousarray(panel_mm(Cm, Ta).T), "sigma": sigma, "rho": rho,
            "orth_ranks": ranks, "delta_sq": float(delta_sq), "share": float(total / delta_sq) if delta_sq > 0 else 0.0, "L": L}


def round_factor(x32: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    return torch.from_numpy(x32).to(dtype)
