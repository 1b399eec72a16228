"""The CABS operator restated in numpy on the CPU (include/shardmerge_hip.h, smhip_cabs_merge), written from the
header's steps 1 to 7: a sort per group, ties by >=, the fp32 steps through np.float32 arrays, one rounded operation
per line.  Every step is an integer function, an exact order statistic or a correctly rounded fp32 operation and the
loop over the finetunes is explicit, so no reduction order is left to a library: the HIP path must equal this bit for
bit.  Test infrastructure of that feature."""
import numpy as np
import torch

F32 = np.float32


def view_of(shape):
    """(R, C): rows of the last dimension, a 0-D or 1-D tensor is one row"""
    shape = tuple(int(v) for v in shape)
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    C = shape[-1] if shape else 1
    return ((n // C) if C else 1) or 1, C


def quotas(C, n_keep, group):
    """[G]: the quota of every group of a row, ceil(N m' / M) in integers"""
    G = (C + group - 1) // group
    mlen = np.minimum(C - np.arange(G, dtype=np.int64) * group, group)
    return (n_keep * mlen + group - 1) // group


def cabs_merge(finetunes, bases, alphas, base_out, n_keep, group, conflict_aware=True, lam=1.0):
    """-> dict(out in base_out's dtype, delta fp32, mask int32 (bit i: finetune i kept the element), groups, kept [k],
    short_groups [k], surplus [k], covered, overlap)"""
    k, n, shape = len(finetunes), base_out.numel(), tuple(base_out.shape)
    N, M = int(n_keep), int(group)
    if n == 0:
        return dict(out=base_out.clone(), delta=torch.zeros(shape, dtype=torch.float32), mask=torch.zeros(shape, dtype=torch.int32),
                    groups=0, kept=[0] * k, short_groups=[0] * k, surplus=[0] * k, covered=0, overlap=0)
    R, C = view_of(shape)
    G = (C + M - 1) // M
    q = quotas(C, N, M)[None, :]                                    # [1, G]
    pad = G * M - C
    to_np = lambda t: t.detach().cpu().to(torch.float32).reshape(R, C).numpy()
    Msum = np.zeros((R, C), dtype=F32)
    mask = np.zeros((R, C), dtype=np.int32)
    taken = np.zeros((R, C), dtype=bool)
    kept_n, short_n, surplus_n = [], [], []
    for i, (ft, bs, alpha) in enumerate(zip(finetunes, bases, alphas)):
        # 1: the delta
        d = to_np(ft) - to_np(bs)
        assert d.dtype == F32
        if not np.isfinite(d).all():
            raise ValueError(f"non-finite delta in finetune {i}")
        # 3: the candidates and the cut of every group
        key = (d.view(np.uint32) & np.uint32(0x7FFFFFFF)).astype(np.int32)         # 31 bits: order as signed integers
        cand = d != 0
        if conflict_aware:
            cand &= ~taken
        ck = np.where(cand, key, 0)                                 # a candidate's key is at least 1
        grouped = np.pad(ck, ((0, 0), (0, pad))).reshape(R, G, M)
        ordered = np.sort(grouped, axis=2)                          # ascending: the q-th largest is at M - q
        c = (grouped != 0).sum(axis=2)
        tau = np.take_along_axis(ordered, np.broadcast_to((M - q)[:, :, None], (R, G, 1)), axis=2)[:, :, 0]
        tau = np.where(c <= q, 1, tau)                              # at most q candidates: every one is kept
        keep_g = (grouped != 0) & (grouped >= tau[:, :, None])
        kc = keep_g.sum(axis=2)
        kept = keep_g.reshape(R, G * M)[:, :C]
        kept_n.append(int(kc.sum()))
        short_n.append(int((c < q).sum()))
        surplus_n.append(int(np.maximum(kc - q, 0).sum()))
        # 4: the weighted entry and the running sum
        tv = np.where(kept, d * F32(alpha), F32(0))
        assert tv.dtype == F32
        Msum = Msum + tv
        mask |= kept.astype(np.int32) << i
        taken |= kept
    # 5: the output
    delta = F32(lam) * Msum
    assert delta.dtype == F32
    out = base_out.detach().cpu().to(torch.float32).reshape(R, C).numpy() + delta
    out = torch.from_numpy(out).to(base_out.dtype).reshape(shape)
    bits = np.zeros((R, C), dtype=np.int64)
    for i in range(k):
        bits += (mask >> i) & 1
    return dict(out=out, delta=torch.from_numpy(delta).reshape(shape), mask=torch.from_numpy(mask).reshape(shape), groups=R * G,
                kept=kept_n, short_groups=short_n, surplus=surplus_n, covered=int((bits >= 1).sum()), overlap=int((bits >= 2).sum()))
