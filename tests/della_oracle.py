"""The DELLA operators restated in numpy / torch on the CPU (include/shardmerge_hip.h, smhip_della_merge): the rank of each
magnitude within its row by sorting the integer magnitude bits (equal magnitudes share a rank), the threshold in
np.float64 one operation at a time, the draws of tests/dare_oracle.py, and the fp32 chain of that oracle with a
threshold and a rescale per element.  The HIP path must equal this bit for bit.  Test infrastructure of that feature."""
import numpy as np
import torch

from tests import dare_oracle

MAX_COLS = 32768


def magnitude_bits(d: torch.Tensor) -> np.ndarray:
    """the 31 magnitude bits of an fp32 tensor as uint32"""
    return d.contiguous().view(torch.int32).numpy().view(np.uint32) & np.uint32(0x7FFFFFFF)


def ranks(mag: np.ndarray) -> np.ndarray:
    """[R, c] magnitude bits -> [R, c]: how many elements of the row are strictly smaller"""
    out = np.empty(mag.shape, dtype=np.int64)
    for r in range(mag.shape[0]):
        out[r] = np.searchsorted(np.sort(mag[r]), mag[r], side="left")
    return out


def thresholds_of_ranks(r: np.ndarray, c: int, density: float, epsilon: float) -> np.ndarray:
    """step 4: every operation in np.float64, rounded once, in the stated order -> uint32"""
    if density == 1:
        return np.full(r.shape, 65536, dtype=np.uint32)
    if epsilon == 0:
        return np.full(r.shape, dare_oracle.threshold(density), dtype=np.uint32)
    p_lo = np.float64(density) - np.float64(epsilon)
    w = np.float64(2.0) * np.float64(epsilon)
    if c == 1:
        p = np.full(r.shape, p_lo, dtype=np.float64)
    else:
        num = w * r.astype(np.float64)
        q = num / np.float64(c - 1)
        p = p_lo + q
    return np.minimum(np.floor(p * np.float64(65536.0)), 65535.0).astype(np.uint32)


def check_arguments(density: float, epsilon: float) -> None:
    if not (0.0 < density <= 1.0) or not (epsilon >= 0.0):
        raise ValueError("density / epsilon out of range")
    if density == 1.0:
        if epsilon != 0.0:
            raise ValueError("density 1 requires epsilon 0")
        return
    if epsilon == 0.0:
        if dare_oracle.threshold(density) < 1:
            raise ValueError("density below 2^-16")
        return
    if not (np.float64(density) + np.float64(epsilon) < 1.0) or not (np.floor((np.float64(density) - np.float64(epsilon)) * 65536.0) >= 1):
        raise ValueError("density, epsilon: the window leaves (2^-16, 1)")


def della_merge(finetunes, bases, alphas, base_out, density=0.5, epsilon=0.15, lam=1.0, normalize=True, rescale=True,
                sign_election=True, key=0, stream_ids=None):
    """-> (out in base_out's dtype, merged delta fp32, thresholds int32 [k, *shape], T_lo, T_hi, kept counts)"""
    f32 = torch.float32
    check_arguments(float(density), float(epsilon))
    n = base_out.numel()
    shape = tuple(base_out.shape)
    c = shape[-1] if len(shape) else 1
    R = n // c if c else 0
    if epsilon > 0 and c > MAX_COLS:
        raise ValueError(f"rows of {c} elements exceed {MAX_COLS}")
    stream_ids = list(range(len(finetunes))) if stream_ids is None else stream_ids
    ends = thresholds_of_ranks(np.array([0, max(c - 1, 0)], dtype=np.int64), max(c, 1), density, epsilon)
    zero = torch.zeros((), dtype=f32)
    S = torch.zeros(n, dtype=f32)
    tvs, al32, kept, Ts = [], [], [], []
    for ft, bs, alpha, sid in zip(finetunes, bases, alphas, stream_ids):
        d = ft.to(f32).reshape(-1) - bs.to(f32).reshape(-1)
        if not bool(torch.isfinite(d).all()):
            raise ValueError("non-finite delta")
        if epsilon == 0 or density == 1 or n == 0:
            T = thresholds_of_ranks(np.zeros(n, dtype=np.int64), max(c, 1), density, 0.0 if n else epsilon)
        else:
            T = thresholds_of_ranks(ranks(magnitude_bits(d).reshape(R, c)), c, density, epsilon).reshape(-1)
        Ts.append(torch.from_numpy(T.astype(np.int32)).reshape(shape))
        h = dare_oracle.draws(key, sid, 0, (n + 7) >> 3)[:n].astype(np.uint32)
        keep = torch.from_numpy(h < T) & (d != 0)
        s = torch.from_numpy((np.float64(65536.0) / T.astype(np.float64)).astype(np.float32)) if rescale else torch.ones(n, dtype=f32)
        a = torch.tensor(float(alpha), dtype=f32)
        tv = torch.where(keep, (d * s) * a, zero)
        kept.append(int(keep.sum()))
        S = S + tv
        al32.append(a)
        if sign_election:
            tvs.append(tv)
    if sign_election:
        pos = S >= 0
        M, D = torch.zeros(n, dtype=f32), torch.zeros(n, dtype=f32)
        for tv, a in zip(tvs, al32):
            m = torch.where(pos, tv > 0, tv < 0)
            M = M + torch.where(m, tv, zero)
            D = D + torch.where(m, a, zero)
    else:
        M = S
        D = torch.zeros((), dtype=f32)
        for a in al32:
            D = D + a
    if normalize:
        D = torch.where(D.abs() < torch.tensor(1e-8, dtype=f32), torch.ones((), dtype=f32), D)
        M = M / D
    delta = torch.tensor(float(lam), dtype=f32) * M
    out = (base_out.to(f32).reshape(-1) + delta).to(base_out.dtype)
    thresholds = torch.stack(Ts) if Ts else torch.zeros((0,) + shape, dtype=torch.int32)
    return out.reshape(shape), delta.reshape(shape), thresholds, int(ends[0]), int(ends[1]), kept
