"""A plain numpy restatement of smhip_fusion_merge (include/shardmerge_hip.h): sm_exp and sm_log of csrc/sm_fusion.hpp one
rounded fp64 operation at a time, the row sums in the stated order (octet o of a row to lane o % 256, a lane in ascending
index from +0, the binary tree over the 256 lanes), the scores, the three exact quartiles, the gate and the clamp.  numpy
rounds every array operation once and fuses nothing, so this file IS the definition executed literally."""
import numpy as np
import torch

LN2_HI, LN2_LO = float.fromhex("0x1.62e42fee00000p-1"), float.fromhex("0x1.a39ef35793c76p-33")
INV_LN2, SQRT2 = float.fromhex("0x1.71547652b82fep+0"), float.fromhex("0x1.6a09e667f3bcdp+0")
EXP_CUTOFF = -45.0
EXP_C = [float.fromhex(h) for h in (
    "0x1.0000000000000p+0", "0x1.0000000000000p+0", "0x1.0000000000000p-1", "0x1.5555555555555p-3",
    "0x1.5555555555555p-5", "0x1.1111111111111p-7", "0x1.6c16c16c16c17p-10", "0x1.a01a01a01a01ap-13",
    "0x1.a01a01a01a01ap-16", "0x1.71de3a556c734p-19", "0x1.27e4fb7789f5cp-22", "0x1.ae64567f544e4p-26",
    "0x1.1eed8eff8d898p-29", "0x1.6124613a86d09p-33", "0x1.93974a8c07c9dp-37")]
LOG_C = [float.fromhex(h) for h in (
    "0x1.0000000000000p+0", "0x1.5555555555555p-2", "0x1.999999999999ap-3", "0x1.2492492492492p-3",
    "0x1.c71c71c71c71cp-4", "0x1.745d1745d1746p-4", "0x1.3b13b13b13b14p-4", "0x1.1111111111111p-4",
    "0x1.e1e1e1e1e1e1ep-5", "0x1.af286bca1af28p-5", "0x1.8618618618618p-5", "0x1.642c8590b2164p-5",
    "0x1.47ae147ae147bp-5")]
LANES = 256


def _horner(c, z):
    p = np.full_like(z, c[-1])
    for ci in reversed(c[:-1]):
        p = p * z
        p = p + ci
    return p


def sm_exp(a):
    """e^a on (-inf, 0], +0 below EXP_CUTOFF"""
    a = np.asarray(a, dtype=np.float64)
    live = a >= EXP_CUTOFF
    x = np.where(live, a, 0.0)
    t = x * INV_LN2
    kd = np.floor(t + 0.5)
    hi = kd * LN2_HI
    lo = kd * LN2_LO
    r = x - hi
    r = r - lo
    y = _horner(EXP_C, r) * np.ldexp(1.0, kd.astype(np.int64))
    return np.where(live, y, 0.0)


def sm_log(S):
    """ln S on [1, 2^40)"""
    S = np.ascontiguousarray(S, dtype=np.float64)
    u = S.view(np.uint64)
    e = ((u >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64) - 1023
    m = ((u & np.uint64(0x000fffffffffffff)) | np.uint64(0x3ff0000000000000)).view(np.float64)
    big = m > SQRT2
    m = np.where(big, m * 0.5, m)
    e = e + big.astype(np.int64)
    f = m - 1.0
    s = f / (2.0 + f)
    lm = (2.0 * s) * _horner(LOG_C, s * s)
    ed = e.astype(np.float64)
    return ed * LN2_HI + (lm + ed * LN2_LO)


def _row_sum(v):
    """[R, C] fp64 -> [R]: the row order of smhip_geo_merge step 2 (a padding +0 leaves a sum that started at +0 as it is)"""
    R, C = v.shape
    noct = (C + 7) // 8
    rounds = (noct + LANES - 1) // LANES
    pad = np.zeros((R, rounds * LANES * 8), dtype=np.float64)
    pad[:, :C] = v
    pad = pad.reshape(R, rounds, LANES, 8)
    acc = np.zeros((R, LANES), dtype=np.float64)
    for r in range(rounds):
        for e in range(8):
            acc = acc + pad[:, r, :, e]
    s = LANES // 2
    while s:
        acc = acc[:, :s] + acc[:, s:2 * s]
        s //= 2
    return acc[:, 0]


def row_kl(x, y, rows_per_step=64):
    """x, y: float32 [R, C] -> (kappa float32 [R], kl float64 [R] before the clamp, max_j |a_j - b_j| [R])"""
    R, C = x.shape
    kl = np.empty(R, dtype=np.float64)
    span = np.empty(R, dtype=np.float64)
    step = max(1, min(R, rows_per_step * 4096 // max(C, 1) + 1))
    for r0 in range(0, R, step):
        xs, ys = x[r0:r0 + step].astype(np.float64), y[r0:r0 + step].astype(np.float64)
        a = xs - xs.max(axis=1, keepdims=True)
        b = ys - ys.max(axis=1, keepdims=True)
        ea, eb = sm_exp(a), sm_exp(b)
        diff = a - b
        sa, sb, u = _row_sum(ea), _row_sum(eb), _row_sum(ea * diff)
        kl[r0:r0 + step] = u / sa - (sm_log(sa) - sm_log(sb))
        span[r0:r0 + step] = np.abs(diff).max(axis=1)
    kappa = np.where(kl > 0.0, kl, 0.0).astype(np.float32)
    return kappa, kl, span


def _f32(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().to(torch.float32).contiguous().numpy()


def fusion_merge(ft, base, base_out, mode, iqr_mult=1.5, t=None):
    """-> dict(out, delta, and arcee: kappa, kl, span, q1, q2, q3, threshold, selected; nearswap: clipped)"""
    shape = tuple(base_out.shape)
    n = base_out.numel()
    x, y, bo = _f32(ft).reshape(-1), _f32(base).reshape(-1), _f32(base_out).reshape(-1)
    d = x - y
    res = {}
    if mode == "nearswap":
        t32 = np.float32(t)
        M = np.where(d > t32, t32, np.where(d < -t32, -t32, d)).astype(np.float32)
        res["clipped"] = int((np.abs(d) > t32).sum())
    else:
        C = shape[-1] if len(shape) else 1
        R = n // C if C else 0
        if n:
            kappa, kl, span = row_kl(x.reshape(R, C), y.reshape(R, C))
            s = (np.abs(d).reshape(R, C) * kappa[:, None]).astype(np.float32).reshape(-1)
            keys = np.sort(s.view(np.uint32) & np.uint32(0x7fffffff))
            q1, q2, q3 = (keys[int(rho)].reshape(1).view(np.float32)[0] for rho in ((n - 1) // 4, (n - 1) // 2, 3 * (n - 1) // 4))
            thr = np.float32(q2 + np.float32(np.float32(iqr_mult) * np.float32(q3 - q1)))
            sel = s > thr
            M = np.where(sel, d, np.float32(0.0)).astype(np.float32)
            res.update(kappa=kappa, kl=kl, span=span, q1=float(q1), q2=float(q2), q3=float(q3), threshold=float(thr),
                       selected=int(sel.sum()))
        else:
            M = d
            res.update(kappa=np.zeros(0, np.float32), kl=np.zeros(0), span=np.zeros(0), q1=0.0, q2=0.0, q3=0.0, threshold=0.0, selected=0)
    r = bo + M
    res["delta"] = torch.from_numpy(np.ascontiguousarray(M)).reshape(shape)
    res["out"] = torch.from_numpy(np.ascontiguousarray(r)).reshape(shape).to(base_out.dtype)
    return res
