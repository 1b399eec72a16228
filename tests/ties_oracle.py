"""The TIES operator restated in torch on the CPU (include/shardmerge_hip.h, smhip_ties_merge).  Every step is one
correctly rounded fp32 operation or an exact order statistic and the loops over the finetunes are explicit, so no
reduction order is left to a library: the HIP path must equal this bit for bit.  Test infrastructure of that feature."""
import torch


def ties_merge(finetunes, bases, alphas, base_out, density=0.2, lam=1.0, normalize=True):
    """-> (out in base_out's dtype, merged delta fp32, k_keep, thresholds [fp32 tensors], kept counts)"""
    f32 = torch.float32
    n = base_out.numel()
    k_keep = n if density == 1 else int(density * n)
    tvs, al32, taus, kept = [], [], [], []
    for ft, bs, alpha in zip(finetunes, bases, alphas):
        d = ft.to(f32).reshape(-1) - bs.to(f32).reshape(-1)
        if not bool(torch.isfinite(d).all()):
            raise ValueError("non-finite delta")
        mag = d.abs()
        tau = torch.kthvalue(mag, n - k_keep + 1).values if 0 < k_keep else torch.tensor(float("inf"), dtype=f32)
        if n == 0:
            tau = torch.tensor(float("inf"), dtype=f32)
        keep = (mag >= tau) & (d != 0)
        a = torch.tensor(float(alpha), dtype=f32)
        tvs.append(torch.where(keep, d * a, torch.zeros((), dtype=f32)))
        al32.append(a)
        taus.append(tau)
        kept.append(int(keep.sum()))
    S = torch.zeros(n, dtype=f32)
    for tv in tvs:
        S = S + tv
    pos = S >= 0
    M, D = torch.zeros(n, dtype=f32), torch.zeros(n, dtype=f32)
    zero = torch.zeros((), dtype=f32)
    for tv, a in zip(tvs, al32):
        m = torch.where(pos, tv > 0, tv < 0)
        M = M + torch.where(m, tv, zero)
        D = D + torch.where(m, a, zero)
    if normalize:
        D = torch.where(D.abs() < torch.tensor(1e-8, dtype=f32), torch.ones((), dtype=f32), D)
        M = M / D
    delta = torch.tensor(float(lam), dtype=f32) * M
    out = (base_out.to(f32).reshape(-1) + delta).to(base_out.dtype)
    return out.reshape(base_out.shape), delta.reshape(base_out.shape), k_keep, taus, kept
