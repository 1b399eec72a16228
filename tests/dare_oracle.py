"""The DARE operators restated in numpy / torch on the CPU (include/shardmerge_hip.h, smhip_dare_merge): Philox4x32-10
with uint64 products, the 16-bit draws, and the fp32 chain with explicit loops over the finetunes, so no reduction
order is left to a library: the HIP path must equal this bit for bit.  The generator is first held to its published
known-answer vectors (tests/test_dare_host.py).  Test infrastructure of that feature."""
import hashlib

import numpy as np
import torch

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
CHUNK_OCTETS = 1 << 22          # octets whose mask is generated at once (several uint64 arrays of this length)

# (counter, key, output) of Philox4x32-10 as published with the generator (Random123 known-answer tests)
KNOWN_ANSWERS = (
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """counters: uint64 arrays holding 32-bit words; the key: two Python ints.  -> four uint64 arrays of 32-bit words"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    for _ in range(10):
        p0 = M0 * c0                      # < 2^64: exact in uint64
        p1 = M1 * c2
        n0 = (p1 >> S32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> S32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & LO, n2, p0 & LO
        k0 = (k0 + W0) & 0xFFFFFFFF
        k1 = (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def draws(key: int, stream_id: int, first_octet: int, n_octets: int) -> np.ndarray:
    """the 16-bit draws h of the 8 * n_octets elements from element 8 * first_octet on, uint16"""
    oct_ = np.arange(first_octet, first_octet + n_octets, dtype=np.uint64)
    zero = np.zeros(n_octets, dtype=np.uint64)
    blk = philox4x32_10(oct_ & LO, oct_ >> S32, zero + np.uint64(stream_id), zero, key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF)
    h = np.empty((n_octets, 8), dtype=np.uint16)
    for w in range(4):
        h[:, 2 * w] = (blk[w] & np.uint64(0xFFFF)).astype(np.uint16)
        h[:, 2 * w + 1] = (blk[w] >> np.uint64(16)).astype(np.uint16)
    return h.reshape(-1)


def threshold(density: float) -> int:
    return 65536 if density == 1 else int(float(density) * 65536.0)


def mask(key: int, stream_id: int, n: int, T: int, first: int = 0) -> torch.Tensor:
    """bool [n]: h < T for the elements first .. first + n - 1, generated in chunks"""
    out = torch.empty(n, dtype=torch.bool)
    o0, o1 = first >> 3, (first + n + 7) >> 3
    for a in range(o0, o1, CHUNK_OCTETS):
        b = min(o1, a + CHUNK_OCTETS)
        m = draws(key, stream_id, a, b - a).astype(np.uint32) < np.uint32(T)
        lo, hi = max(first, 8 * a), min(first + n, 8 * b)
        out[lo - first:hi - first] = torch.from_numpy(m[lo - 8 * a:hi - 8 * a])
    return out


def keep_bit(key: int, stream_id: int, j: int, T: int) -> bool:
    """one element of any 64-bit index"""
    return bool(draws(key, stream_id, j >> 3, 1)[j & 7] < T)


def tensor_key(seed: int, tensor_name: str) -> int:
    return int.from_bytes(hashlib.sha256(f"{seed}\n{tensor_name}".encode()).digest()[:8], "little")


def dare_merge(finetunes, bases, alphas, base_out, density=0.2, lam=1.0, normalize=True, rescale=True, sign_election=True,
               key=0, stream_ids=None):
    """-> (out in base_out's dtype, merged delta fp32, T, kept counts)"""
    f32 = torch.float32
    n = base_out.numel()
    T = threshold(density)
    if T == 0:
        raise ValueError("density below 2^-16")
    stream_ids = list(range(len(finetunes))) if stream_ids is None else stream_ids
    r = torch.tensor(65536.0 / T if rescale else 1.0, dtype=f32)          # the fp64 quotient rounded once
    zero = torch.zeros((), dtype=f32)
    S = torch.zeros(n, dtype=f32)
    tvs, al32, kept = [], [], []
    for ft, bs, alpha, sid in zip(finetunes, bases, alphas, stream_ids):
        d = ft.to(f32).reshape(-1) - bs.to(f32).reshape(-1)
        if not bool(torch.isfinite(d).all()):
            raise ValueError("non-finite delta")
        keep = mask(key, sid, n, T) & (d != 0)
        a = torch.tensor(float(alpha), dtype=f32)
        tv = torch.where(keep, (d * r) * a, zero)
        del d
        kept.append(int(keep.sum()))
        del keep
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
    return out.reshape(base_out.shape), delta.reshape(base_out.shape), T, kept
