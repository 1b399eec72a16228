"""The Model Breadcrumbs operators restated in torch on the CPU (include/shardmerge_hip.h, smhip_breadcrumbs_merge).
Every step is one correctly rounded fp32 operation or an exact order statistic (``kthvalue``) and the loops over the
finetunes are explicit, so no reduction order is left to a library: the HIP path must equal this bit for bit.  Test
infrastructure of that feature."""
import math

import torch


def counts(n, density, gamma):
    """(k_keep, n_top) in fp64, as the header states them"""
    k_keep = n if density == 1 else int(math.floor(float(density) * n))
    n_top = min(int(math.floor(float(gamma) * n)), n - k_keep)
    return k_keep, n_top


def breadcrumbs_merge(finetunes, bases, alphas, base_out, density=0.9, gamma=0.01, lam=1.0, normalize=True, sign_election=False):
    """-> (out in base_out's dtype, merged delta fp32, k_keep, n_top, thresholds_lo, thresholds_hi [fp32 tensors], kept
    counts, dropped_top counts)"""
    f32 = torch.float32
    n = base_out.numel()
    k_keep, n_top = counts(n, density, gamma)
    inf = torch.tensor(float("inf"), dtype=f32)
    zero = torch.zeros((), dtype=f32)
    tvs, al32, taus_lo, taus_hi, kept, dropped = [], [], [], [], [], []
    for ft, bs, alpha in zip(finetunes, bases, alphas):
        d = ft.to(f32).reshape(-1) - bs.to(f32).reshape(-1)
        if not bool(torch.isfinite(d).all()):
            raise ValueError("non-finite delta")
        mag = d.abs()
        if k_keep > 0:
            # the r-th largest of n is the (n - r + 1)-th smallest
            tau_hi = torch.kthvalue(mag, n - (n_top + 1) + 1).values
            tau_lo = torch.kthvalue(mag, n - (n_top + k_keep) + 1).values
        else:
            tau_hi, tau_lo = inf, inf
        keep = (mag >= tau_lo) & (mag <= tau_hi) & (d != 0)
        a = torch.tensor(float(alpha), dtype=f32)
        tvs.append(torch.where(keep, d * a, zero))
        al32.append(a)
        taus_lo.append(tau_lo)
        taus_hi.append(tau_hi)
        kept.append(int(keep.sum()))
        dropped.append(int((mag > tau_hi).sum()))
    S = torch.zeros(n, dtype=f32)
    for tv in tvs:
        S = S + tv
    if sign_election:                       # steps 4-6 of smhip_ties_merge
        pos = S >= 0
        M, D = torch.zeros(n, dtype=f32), torch.zeros(n, dtype=f32)
        for tv, a in zip(tvs, al32):
            m = torch.where(pos, tv > 0, tv < 0)
            M = M + torch.where(m, tv, zero)
            D = D + torch.where(m, a, zero)
    else:                                   # step 5 of smhip_dare_merge, dare_linear
        M = S
        D = torch.zeros((), dtype=f32)
        for a in al32:
            D = D + a
        D = D.expand(n)
    if normalize:
        D = torch.where(D.abs() < torch.tensor(1e-8, dtype=f32), torch.ones((), dtype=f32), D)
        M = M / D
    delta = torch.tensor(float(lam), dtype=f32) * M
    out = (base_out.to(f32).reshape(-1) + delta).to(base_out.dtype)
    return (out.reshape(base_out.shape), delta.reshape(base_out.shape), k_keep, n_top, taus_lo, taus_hi, kept, dropped)
