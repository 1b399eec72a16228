"""The SCE operator restated in torch / numpy / Python floats on the CPU (include/shardmerge_hip.h, smhip_sce_merge),
written from the header's text.  The loops over the finetunes are explicit, every fp32 step is one torch operation (never
fused), the threshold is torch.kthvalue's exact order statistic, the energies are summed in the header's order (segments,
256 lanes of octets, the binary tree, segments in index order: tests/geo_oracle.py's), and P, Z and the weights are Python
floats, one IEEE operation each.  The HIP path must equal this bit for bit.  Test infrastructure of that feature."""
import math

import numpy as np
import torch

from tests import geo_oracle

F32 = torch.float32


def deltas(finetunes, bases):
    """step 1: d_i in fp32 (flat)"""
    return [f.to(F32).reshape(-1) - b.to(F32).reshape(-1) for f, b in zip(finetunes, bases)]


def scores(ds):
    """step 2: q, the sum of squared deviations across the finetunes, one rounded fp32 operation per step"""
    k = len(ds)
    s = torch.zeros_like(ds[0])
    for d in ds:
        s = s + d
    mean = s / torch.full_like(s, float(k))           # (tensor by tensor: an IEEE division, never a product with 1 / k)
    q = torch.zeros_like(s)
    for d in ds:
        e = d - mean
        q = q + e * e
    return q


def select(ds, select_topk):
    """step 2: (mask or None when every element is selected, nz, k_keep, selected, tau as a float)"""
    k, n = len(ds), ds[0].numel()
    if select_topk == 1 or k == 1:
        return None, n, n, n, 0.0
    q = scores(ds)
    assert not bool(torch.isnan(q).any())
    nz = int((q > 0).sum())
    k_keep = int(math.floor(float(select_topk) * float(nz)))
    if k_keep == 0:
        return torch.zeros(n, dtype=torch.bool), nz, 0, 0, float("inf")
    tau = torch.kthvalue(q, n - k_keep + 1).values    # the k_keep-th largest
    mask = (q >= tau) & (q > 0)
    return mask, nz, k_keep, int(mask.sum()), float(tau)


def energy(x):
    """step 3: sum of x^2 in fp64 in the order of step 2 of smhip_geo_merge, as a Python float"""
    if x.numel() == 0:
        return 0.0
    return geo_oracle.gram_whole([x])[0][0]


def weights(alphas, energies):
    """step 3: w_i as numpy float32"""
    k = len(alphas)
    P = [float(a) * E for a, E in zip(alphas, energies)]
    Z = 0.0
    for p in P:
        Z = Z + p
    if Z > 0.0 and math.isfinite(Z):
        return [np.float32(p / Z) for p in P]
    return [np.float32(1.0 / float(k)) for _ in P]


def sce_merge(finetunes, bases, alphas, base_out, select_topk=1.0, lam=1.0):
    """-> dict(out in base_out's dtype, delta fp32, nz, k_keep, selected, threshold, energy [floats], weight [floats], mask)"""
    shape, n = tuple(base_out.shape), base_out.numel()
    ds = deltas(finetunes, bases)
    for i, d in enumerate(ds):
        if not bool(torch.isfinite(d).all()):
            raise ValueError(f"non-finite delta of finetune {i}")
    mask, nz, k_keep, selected, tau = select(ds, select_topk)
    zero = torch.zeros((), dtype=F32)
    xs = ds if mask is None else [torch.where(mask, d, zero) for d in ds]
    E = [energy(x) for x in xs]
    w = weights(alphas, E)
    S = torch.zeros(n, dtype=F32)
    for x in xs:
        S = S + x
    pos = S >= 0
    M, D = torch.zeros(n, dtype=F32), torch.zeros(n, dtype=F32)
    for x, wi in zip(xs, w):
        wt = torch.tensor(float(wi), dtype=F32)
        m = torch.where(pos, x > 0, x < 0)
        M = M + torch.where(m, x * wt, zero)
        D = D + torch.where(m, wt, zero)
    D = torch.where(D.abs() < torch.tensor(1e-8, dtype=F32), torch.ones((), dtype=F32), D)
    M = M / D
    delta = torch.tensor(float(lam), dtype=F32) * M
    out = (base_out.to(F32).reshape(-1) + delta).to(base_out.dtype)
    return {"out": out.reshape(shape), "delta": delta.reshape(shape), "nz": nz, "k_keep": k_keep, "selected": selected,
            "threshold": tau, "energy": E, "weight": [float(v) for v in w],
            "mask": torch.ones(n, dtype=torch.bool) if mask is None else mask}
