"""A restatement of smhip_geo_merge (include/shardmerge_hip.h: Model Stock, NuSLERP, SLERP) in torch / numpy / math,
written from the header's text: the vectors, the fp64 Gram in the header's summation order (segments, 256 lanes of
octets, the binary tree, segments in index order), the coefficients in fp64 with one IEEE operation per step (Python
floats and numpy float64 never fuse), one rounding to fp32, and the fp32 combination.  ``math.acos`` / ``math.sin`` are
the C library's, as the header asks."""
import math

import numpy as np
import torch

SEG = 32768          # elements per segment of a whole-tensor Gram
LANES = 256
MODES = ("model_stock", "nuslerp", "slerp")


def vectors(fts, bases, mode):
    """step 1: x_i in fp32 (flat)"""
    if mode == "slerp":
        return [f.float().reshape(-1) for f in fts]
    return [(f.float() - b.float()).reshape(-1) for f, b in zip(fts, bases)]


def _segment_sums(a, b, seg_len):
    """a, b: fp32 [S * seg_len] (S segments, the last one zero-padded: a missing element adds nothing, and a product +0
    leaves a lane unchanged since no lane is ever -0).  The value of each segment -> float64 [S]."""
    S = a.numel() // seg_len
    noct = -(-seg_len // 8)
    per = -(-noct // LANES)                       # octets per lane
    out = np.empty(S, dtype=np.float64)
    step = max(1, (1 << 24) // max(seg_len, 1))   # segments per slab (bounded memory)
    for s0 in range(0, S, step):
        s1 = min(S, s0 + step)
        pa = torch.zeros(s1 - s0, per * LANES * 8, dtype=torch.float64)
        pb = torch.zeros_like(pa)
        pa[:, :seg_len] = a[s0 * seg_len:s1 * seg_len].view(s1 - s0, seg_len).double()
        pb[:, :seg_len] = b[s0 * seg_len:s1 * seg_len].view(s1 - s0, seg_len).double()
        # exact products (24 x 24 bits fit 53), as [segment][q][e][lane]: octet q * 256 + lane, element e of it
        prod = (pa * pb).view(s1 - s0, per, LANES, 8).permute(0, 1, 3, 2).contiguous()
        lanes = torch.zeros(s1 - s0, LANES, dtype=torch.float64)
        for q in range(per):                                    # a lane's elements in ascending index order
            for e in range(8):
                lanes = lanes + prod[:, q, e, :]
        s = LANES // 2
        while s >= 1:                                           # the tree: p_t = p_t + p_(t+s), t < s
            lanes = lanes[:, :s] + lanes[:, s:2 * s]
            s //= 2
        out[s0:s1] = lanes[:, 0].numpy()
    return out


def gram_whole(xs):
    """step 2, whole tensor: G as a k x k list of Python floats (both triangles)"""
    k, n = len(xs), xs[0].numel()
    nseg = -(-n // SEG)
    padded = []
    for x in xs:
        p = torch.zeros(nseg * SEG, dtype=torch.float32)
        p[:n] = x
        padded.append(p)
    G = [[0.0] * k for _ in range(k)]
    for i in range(k):
        for j in range(i, k):
            g = 0.0
            for v in _segment_sums(padded[i], padded[j], SEG).tolist():     # the segments in index order
                g = g + v
            G[i][j] = G[j][i] = g
    return G


def gram_rows(xs, R):
    """step 2, row-wise: float64 [R][k][k]"""
    k, n = len(xs), xs[0].numel()
    C = n // R
    G = np.zeros((R, k, k), dtype=np.float64)
    for i in range(k):
        for j in range(i, k):
            G[:, i, j] = G[:, j, i] = _segment_sums(xs[i], xs[j], C)
    return G


def cos_ij(G, i, j):
    ni, nj = math.sqrt(G[i][i]), math.sqrt(G[j][j])
    p = ni * nj
    if p == 0.0 or not math.isfinite(p):
        return 0.0
    return max(-1.0, min(1.0, G[i][j] / p))


def stock_t(G, k):
    """(cos, t) of MODEL_STOCK"""
    if k == 1:
        return 0.0, 1.0
    total = 0.0
    for i in range(k):
        for j in range(i + 1, k):
            total = total + cos_ij(G, i, j)
    cos = total / float(k * (k - 1) // 2)
    den = 1.0 + float(k - 1) * cos
    if not den > 0.0:
        return cos, 0.0
    t = (float(k) * cos) / den
    return cos, (t if math.isfinite(t) else 0.0)


def alpha_sum(alphas):
    A = 0.0
    for a in alphas:
        A = A + float(a)
    return 1.0 if abs(A) < 1e-8 else A


def f32(x):
    return np.float32(x)


def stock_coefficients(t, alphas):
    A = alpha_sum(alphas)
    return [f32((t * float(a)) / A) for a in alphas]


def slerp_coefficients(G, alphas, mode):
    """(cos_01, tau, omega, linear, [c_0, c_1]) of NUSLERP / SLERP at k = 2"""
    a0, a1 = float(alphas[0]), float(alphas[1])
    tau = a1 / (a0 + a1)
    n0, n1 = math.sqrt(G[0][0]), math.sqrt(G[1][1])
    cos = cos_ij(G, 0, 1)
    linear = n0 == 0.0 or n1 == 0.0 or abs(cos) > 0.9995
    one_tau = 1.0 - tau
    if linear:
        omega, s0, s1 = 0.0, one_tau, tau
    else:
        omega = math.acos(cos)
        so = math.sin(omega)
        s0 = math.sin(one_tau * omega) / so
        s1 = math.sin(tau * omega) / so
    if mode == "nuslerp" and not linear:
        N = one_tau * n0 + tau * n1
        c = [f32((s0 * N) / n0), f32((s1 * N) / n1)]
    else:
        c = [f32(s0), f32(s1)]
    return cos, tau, omega, linear, c


def combine(xs, coefs, base_out, mode, shape):
    """step 4: (out in base_out's dtype, M in fp32); coefs[i]: an fp32 scalar or an fp32 tensor broadcast over the rows"""
    M = torch.zeros(shape, dtype=torch.float32)
    for x, c in zip(xs, coefs):
        c = c if isinstance(c, torch.Tensor) else torch.tensor(float(c), dtype=torch.float32)
        M = M + c * x.view(shape)                  # fl32 product, then fl32 sum: two torch ops, never fused
    if mode == "slerp":
        return M.to(base_out.dtype), M
    return (base_out.float() + M).to(base_out.dtype), M


def geo_merge(fts, bases, alphas, base_out, mode="model_stock", rowwise=False):
    """-> dict(out, delta, G, cos, t, omega, linear, c) for whole-tensor calls; dict(out, delta, t_rows, t_min, t_max,
    t_mean) for row-wise ones"""
    assert mode in MODES
    k, shape = len(fts), tuple(base_out.shape)
    n = base_out.numel()
    xs = vectors(fts, bases, mode)
    for i, x in enumerate(xs):
        if not bool(torch.isfinite(x).all()):
            raise ValueError(f"non-finite vector of finetune {i}")
    if n == 0:
        return {"out": torch.empty(shape, dtype=base_out.dtype), "delta": torch.empty(shape, dtype=torch.float32)}
    if rowwise:
        assert mode == "model_stock"
        R = shape[0] if len(shape) > 1 else 1
        G = gram_rows(xs, R)
        ts = [stock_t(G[r].tolist(), k)[1] for r in range(R)]
        rows = [stock_coefficients(t, alphas) for t in ts]
        view = (R,) + (1,) * (len(shape) - 1) if len(shape) > 1 else (1,)
        coefs = [torch.tensor(np.array([row[i] for row in rows], dtype=np.float32)).view(view) for i in range(k)]
        out, M = combine(xs, coefs, base_out, mode, shape)
        total = 0.0
        for t in ts:
            total = total + t
        return {"out": out, "delta": M, "t_rows": ts, "t_min": min(ts), "t_max": max(ts), "t_mean": total / float(R)}
    G = gram_whole(xs)
    if mode == "model_stock":
        cos, t = stock_t(G, k)
        omega, linear, c = 0.0, False, stock_coefficients(t, alphas)
    elif k == 1:
        cos, t, omega, linear, c = 0.0, 0.0, 0.0, True, [f32(1.0)]
    else:
        assert k == 2
        cos, t, omega, linear, c = slerp_coefficients(G, alphas, mode)
    out, M = combine(xs, c, base_out, mode, shape)
    return {"out": out, "delta": M, "G": G, "cos": cos, "t": t, "omega": omega, "linear": linear, "c": [float(v) for v in c]}
