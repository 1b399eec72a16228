"""A plain numpy restatement of smhip_widen_merge (include/shardmerge_hip.h): the column sums by a loop over the rows
in the stated order (segments of 512 rows, 8 sub-lanes, the binary tree, the segments in index order), the two
divergences one rounded fp64 operation at a time, the ranks by np.searchsorted on the sorted keys (the number of
strictly smaller values, whatever the sort did with ties), the softmax with the loop over the finetunes explicit and the
fp32 combination.  sm_exp is not restated: ``exp`` is the library's own, through smhip_fusion_fn on the host
(``exp_of(engine)``), which tests/test_fusion_host.py holds to its numpy restatement and to mpmath.
numpy rounds every array operation once and fuses nothing, so this file IS the definition executed literally."""
import numpy as np
import torch

F32, F64 = np.float32, np.float64
SEG_ROWS, SUB = 512, 8
MAX_COLS = 65536


def exp_of(engine):
    """sm_exp over an fp64 numpy array, evaluated on the host by the engine's library"""
    def exp(x):
        x = np.ascontiguousarray(x, dtype=F64)
        return engine.fusion_fn("exp", torch.from_numpy(x.reshape(-1)), on_device=False).numpy().reshape(x.shape)
    return exp


def view(shape):
    shape = tuple(int(v) for v in shape)
    if len(shape) < 2:
        return 1, int(np.prod(shape, dtype=np.int64))
    return shape[0], int(np.prod(shape[1:], dtype=np.int64))


def _f32(t: torch.Tensor, R, C) -> np.ndarray:
    return t.detach().cpu().to(torch.float32).contiguous().numpy().reshape(R, C)


def column_sum(a, b):
    """sum_r a[r, :] * b[r, :] for fp32 arrays [R, C], in fp64, in the order of step 1"""
    R, C = a.shape
    a, b = a.astype(F64), b.astype(F64)
    total = np.zeros(C, dtype=F64)
    for g0 in range(0, R, SEG_ROWS):
        rows = min(SEG_ROWS, R - g0)
        lane = [np.zeros(C, dtype=F64) for _ in range(SUB)]
        for rho in range(rows):
            lane[rho % SUB] = lane[rho % SUB] + a[g0 + rho] * b[g0 + rho]      # (the product is exact)
        s = SUB // 2
        while s:
            for u in range(s):
                lane[u] = lane[u] + lane[u + s]
            s //= 2
        total = total + lane[0]
    return total


def divergences(P, B, X):
    """step 2: (m, d) from the three sums of every column"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = np.abs(np.sqrt(P) - np.sqrt(B))
        den = np.sqrt(P * B)
        c = np.minimum(1.0, np.maximum(-1.0, X / den))
        d = 1.0 - c
    odd = (den == 0) | ~np.isfinite(den)
    d = np.where(odd, np.where(P == B, 0.0, 1.0), d)
    return m, d


def ranks(stat):
    """step 3: the number of strictly smaller values, per column"""
    return np.searchsorted(np.sort(stat), stat, side="left").astype(np.int64)


def widen_merge(finetunes, bases, alphas, base_out, *, ratio=1.0, calibration=1.0, lam=1.0, exp):
    """-> dict(out in base_out's dtype, delta fp32 (lambda * M), rows, cols, vector_mode, stat fp64 [k, 2, C], rank int64
    [k, 2, C], weight fp32 [k, C], mu [k][2], calibrated [k][2], sums [k] of (P, B, X) in matrix mode)"""
    k, shape = len(finetunes), tuple(base_out.shape)
    R, C = view(shape)
    n = R * C
    res = dict(rows=R if n else 0, cols=C if n else 0, vector_mode=bool(n and R == 1), sums=[])
    if n == 0:
        res.update(out=base_out.clone(), delta=torch.zeros(shape), stat=np.zeros((k, 2, 0)), rank=np.zeros((k, 2, 0), dtype=np.int64),
                   weight=np.zeros((k, 0), dtype=F32), mu=[[0.0, 0.0]] * k, calibrated=[[0, 0]] * k)
        return res
    assert C <= MAX_COLS
    ns = 1 if R == 1 else 2
    f = [_f32(t, R, C) for t in finetunes]
    b = [_f32(t, R, C) for t in bases]
    stat = np.zeros((k, 2, C), dtype=F64)
    rank = np.zeros((k, 2, C), dtype=np.int64)
    bad = []
    for i in range(k):
        if R == 1:
            stat[i, 0] = np.abs(f[i][0] - b[i][0]).astype(F64)
            if not np.isfinite(stat[i, 0]).all():
                bad.append(i)
        else:
            P, B, X = column_sum(f[i], f[i]), column_sum(b[i], b[i]), column_sum(f[i], b[i])
            res["sums"].append((P, B, X))
            if not (np.isfinite(P).all() and np.isfinite(B).all()):
                bad.append(i)
            stat[i, 0], stat[i, 1] = divergences(P, B, X)
    if bad:
        raise ValueError(f"non-finite finetune or base: {bad}")
    Cd = F64(C)
    mu = np.zeros((k, 2), dtype=F64)
    for i in range(k):
        for s in range(ns):
            rank[i, s] = ranks(stat[i, s])
            mu[i, s] = (F64(int(rank[i, s].sum())) / Cd) / Cd
    sigma = rank.astype(F64) / Cd
    # step 4
    score = np.zeros((k, 2, C), dtype=F64)
    calibrated = np.zeros((k, 2), dtype=np.int64)
    for s in range(ns):
        smax = sigma[:, s].max(axis=0)
        e = [exp(sigma[i, s] - smax) for i in range(k)]
        Z = np.zeros(C, dtype=F64)
        for i in range(k):
            Z = Z + e[i]
        for i in range(k):
            cal = sigma[i, s] > F64(ratio) * mu[i, s]
            score[i, s] = np.where(cal, F64(calibration), e[i] / Z)
            calibrated[i, s] = int(cal.sum())
    # step 5
    weight = np.zeros((k, C), dtype=F32)
    for i in range(k):
        h = 0.5 * (score[i, 0] + score[i, 1]) if ns == 2 else score[i, 0]
        weight[i] = (F64(alphas[i]) * h).astype(F32)
    # step 6
    M = np.zeros((R, C), dtype=F32)
    for i in range(k):
        M = M + weight[i][None, :] * (f[i] - b[i])
    delta = F32(lam) * M
    out = _f32(base_out, R, C) + delta
    res.update(stat=stat, rank=rank, weight=weight, mu=mu.tolist(), calibrated=calibrated.tolist(),
               delta=torch.from_numpy(np.ascontiguousarray(delta)).reshape(shape),
               out=torch.from_numpy(np.ascontiguousarray(out)).reshape(shape).to(base_out.dtype))
    return res
