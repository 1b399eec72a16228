"""A plain numpy restatement of smhip_pcb_merge (include/shardmerge_hip.h): sm_tanh of csrc/sm_pcb.hpp one rounded fp64
operation at a time (sm_exp is tests/fusion_oracle.py's), the clip's order statistics by a partition (the values a sort
would place there), the scores, their two order statistics likewise, the weights and the two fp32 sums with the loop
over the finetunes explicit.
numpy rounds every array operation once and fuses nothing, so this file IS the definition executed literally."""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from tests.fusion_oracle import _horner, sm_exp

F32, F64 = np.float32, np.float64
TANH_SMALL, TANH_ONE = 2.0 ** -4, 22.5
SCORE_MIN = 2.0 ** -126
TANH_C = [float.fromhex(h) for h in (
    "0x1.0000000000000p+0", "-0x1.5555555555555p-2", "0x1.1111111111111p-3", "-0x1.ba1ba1ba1ba1cp-5",
    "0x1.664f4882c10fap-6", "-0x1.226e355e6c23dp-7", "0x1.d6d3d0e157de0p-9", "-0x1.7da36452b75e3p-10",
    "0x1.3558248036744p-11")]


def sm_tanh(x):
    """tanh x: the odd series below 2^-4, (1 - e) / (1 + e) with e = sm_exp(-2 |x|) up to 22.5, +-1 beyond"""
    x = np.atleast_1d(np.asarray(x, dtype=F64))
    ax = np.abs(x)
    y = np.copysign(1.0, x)                                       # beyond 22.5, and a NaN
    small, mid = ax < TANH_SMALL, (ax >= TANH_SMALL) & (ax <= TANH_ONE)
    xs = x[small]
    y[small] = xs * _horner(TANH_C, xs * xs)
    e = sm_exp(-2.0 * ax[mid])
    y[mid] = np.copysign((1.0 - e) / (1.0 + e), x[mid])
    return y


def _f32(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().to(torch.float32).contiguous().numpy().reshape(-1)


def counts(n, ratio, clip):
    """(r, q) of steps 2 and 6"""
    r = int(math.floor(float(clip) * float(n)))
    q = n if float(ratio) == 1.0 else max(1, int(math.floor(float(ratio) * float(n))))
    return r, q


def clip_entry(tv, lo, hi):
    a = np.abs(tv)
    c = np.where(a < lo, lo, a)
    return np.where(c > hi, hi, c)


def score(tv, U, lo, hi, k):
    """steps 3 - 5 for one finetune: tv, U float32 arrays, lo <= hi float32 scalars -> S float32.  Only the entries with
    tv U > 0 are evaluated: elsewhere sm_tanh is <= 0, so is the product, and the score is +0 by step 5."""
    x = tv.astype(F64) * U.astype(F64)
    live = x > 0
    x, c = x[live], clip_entry(tv[live], lo, hi)
    if hi == lo:
        s = np.zeros(c.shape, dtype=F64)
    else:
        span = F64(hi) - F64(lo)
        s = (c.astype(F64) - F64(lo)) / span
    intra = sm_exp(F64(k) * (s * s - 1.0))
    p = intra * sm_tanh(x)
    S = np.zeros(tv.shape, dtype=F32)
    S[live] = np.where(p >= SCORE_MIN, p, 0.0).astype(F32)
    return S


def pcb_merge(finetunes, bases, alphas, base_out, ratio=0.1, clip=0.0001, lam=1.0):
    """-> dict(out in base_out's dtype, delta fp32 (merged, before lambda), lo, hi, t, M [k] float32, positive, selected
    [k], covered, contested, clip_rank, q, and per finetune tv, tvc, S, scale for the property checks)"""
    k, n, shape = len(finetunes), base_out.numel(), tuple(base_out.shape)
    r, q = counts(n, ratio, clip)
    res = dict(clip_rank=r, q=q if n else 0, lo=[], hi=[], t=[], M=[], positive=[], selected=[], tv=[], tvc=[], S=[], scale=[])
    bo = _f32(base_out)
    if n == 0:
        res.update(covered=0, contested=0, delta=torch.zeros(shape), out=base_out.clone(),
                   lo=[F32(0)] * k, hi=[F32(0)] * k, t=[F32(0)] * k, M=[F32(0)] * k, positive=[0] * k, selected=[0] * k)
        return res
    # 1: the weighted entries, and their sum in index order
    U = np.zeros(n, dtype=F32)
    for ft, bs, alpha in zip(finetunes, bases, alphas):
        d = _f32(ft) - _f32(bs)
        if not np.isfinite(d).all():
            raise ValueError("non-finite delta")
        tv = d * F32(alpha)
        res["tv"].append(tv)
        U = U + tv

    def one(tv):
        # 2: the clip bounds are exact order statistics of |tv| (a partition places them as a sort would)
        mags = np.partition(np.abs(tv), sorted({r, n - 1 - r}))
        lo, hi = mags[r], mags[n - 1 - r]
        # 3 - 5
        S = score(tv, U, lo, hi, k)
        # 6: the q-th largest and the largest score
        t, M = np.partition(S, n - q)[n - q], S.max()
        with np.errstate(divide="ignore", invalid="ignore"):
            ramp = (S - t) / (M - t)
        scale = np.where((S < t) | (S == 0), F32(0), np.where(M == t, F32(1), ramp)).astype(F32)
        c = clip_entry(tv, lo, hi)
        tvc = np.where(tv == 0, F32(0), np.copysign(c, tv)).astype(F32)
        return lo, hi, t, M, int((S > 0).sum()), int(((S >= t) & (S > 0)).sum()), tvc, S, scale

    # (the finetunes are independent up to here: threads only shorten the wait, the sums below run in index order)
    with ThreadPoolExecutor(max_workers=min(k, 16)) as pool:
        per = list(pool.map(one, res["tv"]))
    num, den = np.zeros(n, dtype=F32), np.zeros(n, dtype=F32)
    weighted = np.zeros(n, dtype=np.int64)
    for lo, hi, t, M, positive, selected, tvc, S, scale in per:
        # 7
        num = num + scale * tvc
        den = den + scale
        weighted = weighted + (scale > 0)
        res["lo"].append(lo); res["hi"].append(hi); res["t"].append(t); res["M"].append(M)
        res["positive"].append(positive); res["selected"].append(selected)
        res["tvc"].append(tvc); res["S"].append(S); res["scale"].append(scale)
    merged = num / np.maximum(den, F32(1e-12))
    out = bo + F32(lam) * merged
    res.update(covered=int((den > 0).sum()), contested=int((weighted >= 2).sum()),
               delta=torch.from_numpy(np.ascontiguousarray(merged)).reshape(shape),
               out=torch.from_numpy(np.ascontiguousarray(out)).reshape(shape).to(base_out.dtype))
    return res
