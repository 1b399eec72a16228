"""The Consensus operators restated in torch on the CPU (include/shardmerge_hip.h, smhip_consensus_merge), written from
the header, one rounded fp32 operation per line.  Every step is a correctly rounded fp32 operation, a comparison, an
integer count or (the TIES flavour) an exact order statistic, and the loops over the finetunes are explicit, so no
reduction order is left to a library: the HIP path must equal this bit for bit.  Test infrastructure of that feature."""
import torch

from tests import ties_oracle

F32 = torch.float32


def consensus_merge(finetunes, bases, alphas, base_out, ties=False, density=0.2, mask_lambda=0.4, consensus_k=2, lam=1.0,
                    normalize=True):
    """-> dict(out in base_out's dtype, delta fp32, masked [k], agree [k + 1], selected, k_keep, thresholds, kept)"""
    k, n = len(finetunes), base_out.numel()
    zero, one = torch.zeros((), dtype=F32), torch.ones((), dtype=F32)
    # 1, 2: the deltas and the weighted entries of EVERY element
    tvs, al32 = [], []
    for ft, bs, alpha in zip(finetunes, bases, alphas):
        d = ft.to(F32).reshape(-1) - bs.to(F32).reshape(-1)
        if not bool(torch.isfinite(d).all()):
            raise ValueError("non-finite delta")
        a = torch.tensor(float(alpha), dtype=F32)
        tvs.append(d * a)
        al32.append(a)
    # 3: the multi-task vector
    k_keep, taus, kept = 0, [], []
    if ties:
        flat = torch.zeros(n, dtype=F32)                # M of smhip_ties_merge steps 2 - 6: lambda 1 onto a zero base is M itself
        _, U, k_keep, taus, kept = ties_oracle.ties_merge(finetunes, bases, alphas, flat, density, 1.0, normalize)
        U = U.reshape(-1)
    else:
        U = torch.zeros(n, dtype=F32)
        for tv in tvs:
            U = U + tv
    # 4, 5: the masks and their count
    ml = torch.tensor(float(mask_lambda), dtype=F32)
    c = torch.zeros(n, dtype=torch.int64)
    masked = []
    for tv in tvs:
        rest = U - tv
        rhs = ml * rest.abs()
        m = tv.abs() >= rhs
        masked.append(int(m.sum()))
        c = c + m.to(torch.int64)
    need = min(int(consensus_k), k)
    selected = c >= need
    agree = [int((c == j).sum()) for j in range(k + 1)]
    # 6: the merged delta
    M = U
    if not ties and normalize:
        D = torch.zeros((), dtype=F32)
        for a in al32:
            D = D + a
        if bool(D.abs() < torch.tensor(1e-8, dtype=F32)):
            D = one
        M = U / D
    M = torch.where(selected, M, zero)
    # 7: the output
    delta = torch.tensor(float(lam), dtype=F32) * M
    out = (base_out.to(F32).reshape(-1) + delta).to(base_out.dtype)
    return dict(out=out.reshape(base_out.shape), delta=delta.reshape(base_out.shape), masked=masked, agree=agree,
                selected=int(selected.sum()), k_keep=k_keep, thresholds=taus, kept=kept)
