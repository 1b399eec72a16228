"""A restatement of smhip_dpack_pack and smhip_dpack_apply (include/shardmerge_hip.h: the delta pack) in numpy and
torch on the CPU, written from the header's text: the fp32 delta, the exact order statistic of the trim, the bit planes,
the fp64 sums of a row in the header's order (octet o to lane o % 256, ascending within the lane, the binary tree), the
scale and the residual with one IEEE operation per step (numpy float64 and Python floats never fuse), and the one fp32
addition and one rounding of apply.  The HIP path must equal this bit for bit.  Test infrastructure of that feature."""
import math
from types import SimpleNamespace

import numpy as np
import torch

LANES = 256


def view_rows(shape):
    """R = shape[0] rows of the rest; a 0-D or 1-D tensor is one row"""
    shape = tuple(shape)
    if len(shape) <= 1:
        return 1, int(np.prod(shape, dtype=np.int64)) if shape else 1
    return shape[0], int(np.prod(shape[1:], dtype=np.int64))


def row_sums(v):
    """v: float64 [R, C], every value >= +0.  Step 4's sum of each row -> float64 [R] (a missing element adds +0, which
    leaves a lane unchanged)"""
    R, C = v.shape
    per = max(1, -(-(-(-C // 8)) // LANES))              # octets per lane
    pad = np.zeros((R, per * LANES * 8), dtype=np.float64)
    pad[:, :C] = v
    oct_ = pad.reshape(R, per, LANES, 8)                 # [row][q][lane][e]: octet q * 256 + lane, element e of it
    lanes = np.zeros((R, LANES), dtype=np.float64)
    for q in range(per):                                 # a lane's elements in ascending index order
        for e in range(8):
            lanes = lanes + oct_[:, q, :, e]
    s = LANES // 2
    while s >= 1:                                        # the tree: v_t = v_t + v_(t+s), t < s
        lanes = lanes[:, :s] + lanes[:, s:2 * s]
        s //= 2
    return lanes[:, 0].copy()


def in_order(values):
    """((0 + v_0) + v_1) + ... in fp64"""
    t = 0.0
    for v in values:
        t = t + float(v)
    return t


def scale_of(A, c):
    return np.float32(0.0) if c == 0 else np.float32(float(A) / float(c))


def resid_of(A, Q, c, s32):
    s = float(s32)
    e = (float(Q) - 2.0 * (s * float(A))) + float(c) * (s * s)
    return e if e > 0.0 else 0.0


def pack_bits(b):
    """bool [R, C] -> uint8 [R, ceil(C / 8)], bit c % 8 of byte c / 8"""
    R, C = b.shape
    pb = -(-C // 8)
    pad = np.zeros((R, pb * 8), dtype=np.uint8)
    pad[:, :C] = b
    w = (1 << np.arange(8)).astype(np.uint16)
    return (pad.reshape(R, pb, 8).astype(np.uint16) * w).sum(axis=2).astype(np.uint8)


def unpack_bits(p, C):
    """uint8 [R, PB] -> bool [R, C]"""
    p = np.asarray(p, dtype=np.uint8)
    bits = (p[:, :, None] >> np.arange(8, dtype=np.uint8)) & 1
    return bits.reshape(p.shape[0], p.shape[1] * 8)[:, :C].astype(bool)


def delta(ft, base):
    """step 1: fl32(fp32(ft) - fp32(base)) as numpy [R, C]"""
    dt = ft.dtype if ft.dtype == base.dtype else torch.float32
    R, C = view_rows(ft.shape)
    d = ft.to(dt).to(torch.float32) - base.to(dt).to(torch.float32)
    return d.reshape(R, C).numpy()


def pack(ft, base, bits=1, density=1.0, scale="row"):
    """-> SimpleNamespace(sign, mask | None, scale: torch tensors; the report's fields)"""
    d = delta(ft, base)
    if not np.isfinite(d).all():
        raise ValueError("non-finite delta")
    R, C = d.shape
    n = R * C
    mag = np.abs(d)
    if bits == 1:
        k_keep, tau, kept = n, np.float32(0.0), np.ones((R, C), dtype=bool)
    else:
        k_keep = n if density == 1 else int(math.floor(density * n))
        if k_keep == 0:
            tau = np.float32(np.inf)
        else:
            tau = np.partition(mag.reshape(-1), n - k_keep)[n - k_keep]
        kept = (mag >= tau) & (d != 0)
    sign = pack_bits(kept & (d < 0))
    mask = pack_bits(kept) if bits == 2 else None
    d64 = d.astype(np.float64)
    A = row_sums(np.where(kept, np.abs(d64), 0.0))
    Q = row_sums(np.where(kept, d64 * d64, 0.0))
    Z = row_sums(np.where(kept, 0.0, d64 * d64))
    c = kept.sum(axis=1).astype(np.int64)
    nz = int((d != 0).sum())
    if scale == "tensor":
        A, Q, Z, c = [in_order(A)], [in_order(Q)], [in_order(Z)], [int(c.sum())]
    s = np.array([scale_of(A[r], c[r]) for r in range(len(c))], dtype=np.float32)
    resid_sq = in_order(float(Z[r]) + resid_of(A[r], Q[r], c[r], s[r]) for r in range(len(c)))
    delta_sq = in_order(float(Q[r]) + float(Z[r]) for r in range(len(c)))
    if n == 0:
        s = np.zeros(1 if scale == "tensor" else R, dtype=np.float32)
        resid_sq = delta_sq = 0.0
    return SimpleNamespace(sign=torch.from_numpy(sign), mask=torch.from_numpy(mask) if mask is not None else None,
                           scale=torch.from_numpy(s), rows=R, cols=C, bits=bits, k_keep=k_keep, threshold=float(tau),
                           kept=int(kept.sum()), nonzero=nz, delta_sq=delta_sq, resid_sq=resid_sq)


def apply(base, sign, mask, scale):
    """-> the finetune tensor in base's dtype"""
    R, C = view_rows(base.shape)
    sg = torch.from_numpy(unpack_bits(sign.numpy(), C))
    kept = torch.from_numpy(unpack_bits(mask.numpy(), C)) if mask is not None else torch.ones(R, C, dtype=torch.bool)
    s = scale.to(torch.float32).reshape(-1, 1).expand(R, 1) if scale.numel() == 1 else scale.to(torch.float32).reshape(R, 1)
    b = base.reshape(R, C)
    moved = (b.to(torch.float32) + torch.where(sg, -s, s)).to(base.dtype)        # one fp32 addition, one rounding
    return torch.where(kept, moved, b).reshape(base.shape)
