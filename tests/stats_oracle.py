"""A restatement of smhip_delta_stats (include/shardmerge_hip.h, steps 1-5) in torch / numpy, written from the header's
text: the deltas in fp32, the Gram and the kept energies in the header's fp64 summation order (the Gram routine of
tests/geo_oracle.py, imported), the thresholds from a sort, the election with one rounded fp32 operation per step and
an explicit loop over the finetunes, the counts as integer sums.  Test infrastructure of that feature."""
import torch

from tests import geo_oracle


def delta_stats(finetunes, bases, alphas, densities):
    """-> dict of the report's fields: Python ints, floats (tau rounded to fp32 already) and lists of them"""
    f32 = torch.float32
    k = len(finetunes)
    ds = [ft.to(f32).reshape(-1) - bs.to(f32).reshape(-1) for ft, bs in zip(finetunes, bases)]
    n = ds[0].numel()
    bad = [i for i, d in enumerate(ds) if not bool(torch.isfinite(d).all())]
    if bad:
        raise ValueError(f"non-finite delta in finetunes {bad}")
    zero = torch.zeros((), dtype=f32)
    rep = {"n": n, "nonzero": [int((d != 0).sum()) for d in ds], "gram": geo_oracle.gram_whole(ds),
           "k_keep": [], "thresholds": [], "kept": [], "energy": [], "opposed": [], "alone": [], "cover": [], "conflict": []}
    order = [torch.sort(d.abs(), descending=True).values for d in ds]
    for rho in densities:
        k_keep = n if rho == 1 else int(float(rho) * float(n))              # floor of the fp64 product
        keeps, taus, tvs = [], [], []
        for i, d in enumerate(ds):
            tau = order[i][k_keep - 1] if k_keep > 0 else torch.tensor(float("inf"), dtype=f32)
            keep = (d.abs() >= tau) & (d != 0)
            keeps.append(keep)
            taus.append(float(tau))
            tvs.append(torch.where(keep, d * torch.tensor(float(alphas[i]), dtype=f32), zero))
        S = torch.zeros(n, dtype=f32)
        for tv in tvs:
            S = S + tv
        pos = S >= 0
        c = torch.zeros(n, dtype=torch.int64)
        any_pos, any_neg = torch.zeros(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool)
        for keep, tv in zip(keeps, tvs):
            c += keep
            any_pos |= tv > 0
            any_neg |= tv < 0
        rep["k_keep"].append(k_keep)
        rep["thresholds"].append(taus)
        rep["kept"].append([int(keep.sum()) for keep in keeps])
        rep["energy"].append([geo_oracle.gram_whole([torch.where(keep, d, zero)])[0][0] for keep, d in zip(keeps, ds)])
        rep["opposed"].append([int((keep & ~torch.where(pos, tv > 0, tv < 0)).sum()) for keep, tv in zip(keeps, tvs)])
        rep["alone"].append([int((keep & (c == 1)).sum()) for keep in keeps])
        rep["cover"].append(torch.bincount(c, minlength=k + 1).tolist())
        rep["conflict"].append(int((any_pos & any_neg).sum()))
    return rep
