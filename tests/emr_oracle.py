"""A restatement of smhip_emr_merge, smhip_emr_mask and smhip_emr_apply (include/shardmerge_hip.h: EMR-Merging) in numpy
and torch on the CPU, written from the header's text: the fp32 deltas, their fp32 sum in entry order, the election with
max in place of the sum, the mask by comparing signs, the seven fp64 sums of a row in the delta pack's order
(tests/dpack_oracle.py: octet o to lane o % 256, ascending within the lane, the binary tree, rows in order), the rescaler
and the residual with one IEEE operation per step (numpy scalars and Python floats never fuse), and the three roundings
of apply.  The HIP path must equal this bit for bit.  Test infrastructure of that feature."""
from types import SimpleNamespace

import numpy as np
import torch

from tests.dpack_oracle import in_order, pack_bits, row_sums, unpack_bits, view_rows

CODES = (torch.bfloat16, torch.float16, torch.float32)


def _in_dtype(tensors):
    """one input dtype per call; mixed dtypes are promoted to fp32, never demoted (the engine's rule)"""
    dtypes = {t.dtype for t in tensors}
    dt = next(iter(dtypes)) if len(dtypes) == 1 else torch.float32
    return dt if dt in CODES else torch.float32


def _f32(t, dt):
    return t.to(dt).to(torch.float32).contiguous().numpy()


def emr_merge(fts, bases, base_out, lam=1.0):
    """-> dict(out, delta: torch tensors; the report's fields)"""
    dt = _in_dtype(list(fts) + list(bases))
    k, n = len(fts), base_out.numel()
    d = [(_f32(f, dt) - _f32(b, dt)).reshape(-1) for f, b in zip(fts, bases)]              # step 1: one rounded subtraction
    S = np.zeros(n, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for di in d:                                                                       # step 2: fp32, in entry order
            S = S + di
    if any(not np.isfinite(di).all() for di in d) or not np.isfinite(S).all():
        raise ValueError("non-finite delta or sum")
    pos = S >= 0
    eps = np.zeros(n, dtype=np.float32)
    w = np.full(n, -1, dtype=np.int64)
    agree = []
    for i, di in enumerate(d):                                                             # step 3
        cand = np.where(pos, di > 0, di < 0)
        better = cand & (np.abs(di) > eps)                                                 # strictly: the smallest i that attains it
        eps = np.where(better, np.abs(di), eps)
        w = np.where(better, i, w)
        agree.append(int(cand.sum()))
    tau = np.where(eps == 0, np.float32(0.0), np.where(pos, eps, -eps)).astype(np.float32)  # step 4
    dl = (np.float32(lam) * tau).astype(np.float32)                                        # step 5: two roundings and the cast
    bo_dt = base_out.dtype if base_out.dtype in CODES else torch.float32
    r = _f32(base_out, bo_dt).reshape(-1) + dl
    out = torch.from_numpy(r).to(bo_dt).reshape(base_out.shape)
    some_pos = np.zeros(n, dtype=bool)
    some_neg = np.zeros(n, dtype=bool)
    for di in d:
        some_pos |= di > 0
        some_neg |= di < 0
    return dict(out=out, delta=torch.from_numpy(dl).reshape(base_out.shape), tau=tau, d=d, S=S, n=n,
                elected_pos=int(((eps > 0) & pos).sum()), elected_neg=int(((eps > 0) & ~pos).sum()), zero=int((eps == 0).sum()),
                contested=int((some_pos & some_neg).sum()), winner=[int((w == i).sum()) for i in range(k)], agree=agree)


def scale_of(A, B):
    return np.float32(0.0) if B == 0 else np.float32(float(A) / float(B))


def resid_of(D2, X, U2, l32):
    lam = float(l32)
    e = (float(D2) - 2.0 * (lam * float(X))) + (lam * lam) * float(U2)
    return e if e > 0.0 else 0.0


def emr_mask(ft, base, unified):
    """-> SimpleNamespace(mask, scale: torch tensors; the report's fields)"""
    dt = _in_dtype([ft, base, unified])
    R, C = view_rows(ft.shape)
    b = _f32(base, dt).reshape(R, C)
    d = _f32(ft, dt).reshape(R, C) - b
    u = _f32(unified, dt).reshape(R, C) - b
    if not np.isfinite(d).all() or not np.isfinite(u).all():
        raise ValueError("non-finite delta")
    m = ((d > 0) & (u > 0)) | ((d < 0) & (u < 0))                                          # signs compared, no product
    d64, u64 = d.astype(np.float64), u.astype(np.float64)
    total = lambda v: in_order(row_sums(v)) if R * C else 0.0
    A = total(np.abs(d64))
    B = total(np.where(m, np.abs(u64), 0.0))
    D2 = total(d64 * d64)
    X = total(np.where(m, d64 * u64, 0.0))                                                 # (>= 0 where m: the signs agree)
    U2 = total(np.where(m, u64 * u64, 0.0))
    lam = scale_of(A, B)
    return SimpleNamespace(mask=torch.from_numpy(pack_bits(m)), scale=torch.from_numpy(np.array([lam], dtype=np.float32)),
                           rows=R, cols=C, A=A, B=B, D2=D2, X=X, U2=U2, c=int(m.sum()), nonzero=int((d != 0).sum()),
                           lam=float(lam), delta_sq=D2, resid_sq=resid_of(D2, X, U2, lam))


def emr_apply(base, unified, mask, scale):
    """-> the task's tensor in base's dtype"""
    R, C = view_rows(base.shape)
    bits = torch.from_numpy(unpack_bits(mask.numpy(), C)) if R * C else torch.zeros((R, C), dtype=torch.bool)
    b = base.reshape(R, C).to(torch.float32)
    u = unified.reshape(R, C).to(torch.float32) - b                                        # one rounding each
    t = scale.to(torch.float32).reshape(1, 1) * u
    moved = (b + t).to(base.dtype)
    return torch.where(bits, moved, base.reshape(R, C)).reshape(base.shape)
