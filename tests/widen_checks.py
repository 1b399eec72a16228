"""Checks of the WIDEN operator shared by the emulator tier (tests/test_widen_host.py) and the GPU tier
(tests/test_widen_gpu.py): Engine.widen_merge against tests/widen_oracle.py, BIT FOR BIT - output, delta_out, every
column's statistics, ranks and weights, mu and calibrated.  The tolerance is zero and it is derived, not measured: every
step of the function is one correctly rounded operation, an integer count or a sum in an order that is a function of the
shape alone (include/shardmerge_hip.h, smhip_widen_merge).  Independently of that oracle the function is held to the
paper's form in torch fp64 and its column sums to math.fsum of the exact products."""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

from tests import harness
from tests import widen_oracle as wo
from tests.harness import ALPHAS, DTYPES, expected_by_tensor, make_inputs, profile_of, raw, ties_models

KS = (1, 2, 4, 5, 16)                           # 4 | 5 straddles the two register variants of widen_combine
ROWS = (1, 2, 7, 8, 9, 511, 512, 513, 1025)     # around the sub-lanes (8) and the segments (512)
COLS = (1, 7, 8, 9, 255, 256, 257, 4544)        # around the octet and the work-group (256 columns); 4544 % 256 != 0
RATIOS = (-1.0, 0.0, 0.5, 1.0, 1.5, 3.0)
CALIBRATIONS = (0.0, 0.5, 1.0, 2.0)
LAMBDAS = (0.7, 1.0)
SHAPE = (37, 129)                               # unaligned rows and a tail octet
EPS = 2.0 ** -24


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check(engine, fts, bases, alphas, base_out, ratio=1.0, calibration=1.0, lam=1.0, label=""):
    """one call against the oracle, bit for bit, and the invariants of the report; returns (report, out, delta, oracle)"""
    kw = dict(ratio=ratio, calibration=calibration, lam=lam)
    out, rep, delta = engine.widen_merge(fts, bases, alphas, base_out, want_stats=True, want_delta=True, **kw)
    cpu = lambda ts: [t.cpu() for t in ts]
    ref = wo.widen_merge(cpu(fts), cpu(bases), alphas, base_out.cpu(), exp=wo.exp_of(engine), **kw)
    k, n = len(fts), base_out.numel()
    print(f"{label}: {rep.rows} x {rep.cols} vector {rep.vector_mode}, mu {rep.mu}, calibrated {rep.calibrated}")
    assert out.dtype == base_out.dtype and out.shape == base_out.shape, label
    assert (rep.rows, rep.cols, rep.vector_mode) == (ref["rows"], ref["cols"], ref["vector_mode"]), (label, rep)
    bad = int((u64(rep.stat.numpy()) != u64(ref["stat"])).sum())
    assert bad == 0, f"{label}: {bad} statistics differ in their bits"
    bad = int((rep.rank.numpy() != ref["rank"]).sum())
    assert bad == 0, f"{label}: {bad} ranks differ"
    bad = int((rep.weight.numpy().view(np.uint32) != ref["weight"].view(np.uint32)).sum())
    assert bad == 0, f"{label}: {bad} weights differ in their bits"
    assert u64(np.array(rep.mu)).tolist() == u64(np.array(ref["mu"])).tolist(), (label, rep.mu, ref["mu"])
    assert rep.calibrated == ref["calibrated"], (label, rep.calibrated, ref["calibrated"])
    bad = int((raw(delta) != raw(ref["delta"])).sum())
    assert bad == 0, f"{label}: {bad} of {n} delta_out values differ in their bits"
    bad = int((raw(out) != raw(ref["out"])).sum())
    assert bad == 0, f"{label}: {bad} of {n} output values differ in their bits"
    # the invariants: statistics finite and >= +0 (no sign bit), ranks below C, 0 <= w / alpha <= max(1, calibration)
    if n:
        stat = rep.stat.numpy()
        assert np.isfinite(stat).all() and not np.signbit(stat).any(), label
        assert int(rep.rank.min()) >= 0 and int(rep.rank.max()) < rep.cols, label
        top = max(1.0, calibration) * (1.0 + 2 * EPS)
        for i in range(k):
            q = rep.weight[i].double().numpy() / alphas[i] if alphas[i] else rep.weight[i].double().numpy()
            assert (q >= 0).all() and (q <= (top if alphas[i] else 0.0)).all(), (label, i, float(q.min()), float(q.max()))
            assert all(0 <= c <= rep.cols for c in rep.calibrated[i]) and all(0.0 <= m < 1.0 for m in rep.mu[i]), (label, rep)
    return rep, out, delta, ref


# ---- the parameter grid -------------------------------------------------------------------------------
def check_rows(engine, R, device="cpu"):
    """rows around the sub-lane and segment edges: an aligned width (16-byte loads) and an odd one"""
    for C_, k, own in ((40, 3, True), (19, 2, False)):
        fts, bases, bo = make_inputs((R, C_), k, seed=R % 89 + C_, own_bases=own, device=device)
        rep, _, _, _ = check(engine, fts, bases, ALPHAS[:k], bo, lam=0.7, label=f"R={R} C={C_} k={k}")
        assert rep.vector_mode == (R == 1)


def check_cols(engine, C_, device="cpu"):
    for R, k in ((10, 2), (1, 3)):
        fts, bases, bo = make_inputs((R, C_), k, seed=C_ % 83 + R, own_bases=True, device=device)
        check(engine, fts, bases, ALPHAS[:k], bo, calibration=0.5, label=f"R={R} C={C_} k={k}")


def check_k(engine, k, own, device="cpu"):
    fts, bases, bo = make_inputs(SHAPE, k, seed=20 + k, own_bases=own, device=device)
    rep, _, _, _ = check(engine, fts, bases, ALPHAS[:k], bo, calibration=0.5, lam=0.7, label=f"k={k} own={own}")
    assert all(0 < c < rep.cols for row in rep.calibrated for c in row)


def check_dtypes(engine, in_dtype, bo_dtype, device="cpu"):
    fts, bases, bo = make_inputs(SHAPE, 3, in_dtype, bo_dtype, seed=11, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:3], bo, calibration=0.5, lam=0.7, label=f"{in_dtype}->{bo_dtype}")
    fts, bases, bo = make_inputs((16, 64), 2, in_dtype, bo_dtype, seed=12, device=device)      # one shared base, 16-byte loads
    check(engine, fts, bases, ALPHAS[:2], bo, ratio=0.5, label=f"{in_dtype}->{bo_dtype} shared")


def check_options(engine, ratio, calibration, lam, device="cpu"):
    fts, bases, bo = make_inputs(SHAPE, 3, seed=40, own_bases=True, device=device)
    rep, _, _, _ = check(engine, fts, bases, ALPHAS[:3], bo, ratio=ratio, calibration=calibration, lam=lam,
                         label=f"ratio={ratio} calibration={calibration} lam={lam}")
    if ratio < 0:
        assert rep.calibrated == [[rep.cols, rep.cols]] * 3
    if ratio == 0:                                  # every column but the lowest-ranked
        assert rep.calibrated == [[rep.cols - 1, rep.cols - 1]] * 3


# ---- corners ----------------------------------------------------------------------------------------------
def check_unaligned(engine, device="cpu"):
    """views that start off a 16-byte boundary: the element-wise path of the loaders and the store"""
    R, C_ = 12, 88
    n = R * C_
    for dtype in DTYPES:
        fts, bases, bo = make_inputs((n + 5,), 3, dtype, seed=71, own_bases=True, device=device)
        cut = lambda t, o: t[o:o + n].view(R, C_)
        check(engine, [cut(fts[0], 1), cut(fts[1], 3), cut(fts[2], 0)], [cut(bases[0], 0), cut(bases[1], 1), cut(bases[2], 5)],
              ALPHAS[:3], cut(bo, 1), calibration=0.5, label=f"unaligned {dtype}")


def check_bases(engine, device="cpu"):
    """a base per finetune; one shared base that is also base_out (loaded once)"""
    for k in (3, 5):
        fts, bases, bo = make_inputs((24, 72), k, seed=52 + k, device=device)
        assert bo is bases[0] and all(b is bases[0] for b in bases)
        check(engine, fts, bases, ALPHAS[:k], bo, calibration=0.5, label=f"out_is_base0 k={k}")


def check_signed_alphas(engine, device="cpu"):
    """negative and zero weights, a zero sum: nothing divides by the alphas, and the statistics do not depend on them"""
    fts, bases, bo = make_inputs(SHAPE, 4, seed=55, own_bases=True, device=device)
    a, _, _, _ = check(engine, fts, bases, [0.5, -0.3, 0.0, -0.7], bo, calibration=0.5, lam=0.7, label="signed alphas")
    b, _, _, _ = check(engine, fts, bases, [-0.5, -0.3, -0.2, -0.7], bo, calibration=0.5, lam=-0.7, label="negative alphas")
    assert torch.equal(a.rank, b.rank) and a.mu == b.mu and a.calibrated == b.calibrated and not bool(a.weight[2].any())
    check(engine, fts[:2], bases[:2], [0.5, -0.5], bo, label="alphas that sum to zero")


def check_zero_finetunes(engine, device="cpu"):
    """finetunes equal to their bases: every statistic +0, every rank 0, mu 0, nothing calibrated at ratio >= 0, the
    softmax weights alpha / k; the output is base_out"""
    for shape in (SHAPE, (1, 77)):
        for k in (1, 2, 4):
            fts, bases, bo = make_inputs(shape, k, seed=61, own_bases=True, device=device)
            rep, out, delta, _ = check(engine, [b.clone() for b in bases], bases, [0.5] * k, bo, calibration=2.0, label=f"zero deltas k={k}")
            assert not bool(rep.stat.any()) and not bool(rep.rank.any()) and rep.mu == [[0.0, 0.0]] * k and rep.calibrated == [[0, 0]] * k
            assert bool((rep.weight == np.float32(0.5 * (1.0 / k))).all())
            assert torch.equal(raw(out), raw(bo)) and not bool(delta.any())
    # one of three
    fts, bases, bo = make_inputs(SHAPE, 3, seed=60, device=device)
    fts[1] = bases[1].clone()
    rep, _, _, _ = check(engine, fts, bases, ALPHAS[:3], bo, label="one zero delta")
    assert not bool(rep.stat[1].any()) and not bool(rep.rank[1].any()) and rep.mu[1] == [0.0, 0.0] and rep.calibrated[1] == [0, 0]


def check_untouched_columns(engine, device="cpu"):
    """columns a finetune did not touch among touched ones: P == B == X there, so d = +0 and m = +0 exactly and the
    columns share rank 0"""
    for R in (64, 600):
        fts, bases, bo = make_inputs((R, 96), 3, seed=62, device=device)
        keep = torch.arange(96, device=bo.device) % 3 == 1
        fts[0] = torch.where(keep[None, :], bases[0], fts[0])
        rep, _, _, _ = check(engine, fts, bases, ALPHAS[:3], bo, calibration=0.5, label=f"untouched columns R={R}")
        keep = keep.cpu()
        assert not bool(rep.stat[0][:, keep].any()) and not bool(rep.rank[0][:, keep].any())
        assert bool((rep.stat[0][:, ~keep] > 0).all()) and bool((rep.rank[0][:, ~keep] >= int(keep.sum())).all())


def check_tied_columns(engine, device="cpu"):
    """heavily tied statistics: two finetunes that are copies of each other, and columns duplicated within a tensor"""
    fts, bases, bo = make_inputs((40, 64), 3, seed=63, device=device)
    fts[2] = fts[0].clone()
    for t in fts + [bases[0]]:
        t[:, 32:] = t[:, :32]                      # (bases are one tensor: base_out too)
    rep, _, _, _ = check(engine, fts, bases, ALPHAS[:3], bo, calibration=0.5, label="tied columns")
    assert torch.equal(rep.rank[0], rep.rank[2]) and torch.equal(rep.rank[:, :, :32], rep.rank[:, :, 32:])
    assert int(rep.rank.max()) <= 62 and bool((rep.rank % 2 == 0).all())
    # vector mode: differences of bf16 values collide
    fts, bases, bo = make_inputs((1, 4096), 2, seed=65, sigma=3e-4, device=device)
    rep, _, _, _ = check(engine, fts, bases, ALPHAS[:2], bo, label="tied |delta|")
    assert len(np.unique(rep.rank[0, 0].numpy())) < 2048


def check_zero_columns(engine, device="cpu"):
    """a column that is zero in the base alone (den == 0, P != B: d = 1) and in both (P == B == 0: d = +0)"""
    fts, bases, bo = make_inputs((20, 48), 2, seed=64, own_bases=True, device=device)
    bases[0][:, 5] = 0
    bases[1][:, 7] = 0
    fts[1][:, 7] = 0
    rep, _, _, _ = check(engine, fts, bases, ALPHAS[:2], bo, calibration=0.5, label="zero columns")
    assert float(rep.stat[0, 1, 5]) == 1.0 and float(rep.stat[0, 0, 5]) > 0
    assert float(rep.stat[1, 1, 7]) == 0.0 and float(rep.stat[1, 0, 7]) == 0.0 and int(rep.rank[1, 1, 7]) == 0


def check_nonfinite(engine, device="cpu"):
    """a NaN / an Inf in a finetune or in a base: ValueError naming the tensor and the finetunes; the context stays usable"""
    name = "model.layers.7.mlp.up_proj.weight"
    for shape in (SHAPE, (1, 300), (600, 24)):
        n = shape[0] * shape[1]
        for k, poison, in_base in ((3, float("inf"), False), (5, float("nan"), False), (3, float("-inf"), True), (2, float("nan"), True)):
            fts, bases, bo = make_inputs(shape, k, seed=80, own_bases=True, device=device)
            (bases if in_base else fts)[1].view(-1)[n - 3] = poison
            with pytest.raises(ValueError, match=rf"{re.escape(name)}.*finetune 1\b"):
                engine.widen_merge(fts, bases, ALPHAS[:k], bo, layer_name=name)
        fts, bases, bo = make_inputs(shape, 3, seed=80, own_bases=True, device=device)
        fts[0].view(-1)[0] = float("nan")
        bases[2].view(-1)[n // 2] = float("inf")
        with pytest.raises(ValueError, match=r"finetune 0, 2\b"):
            engine.widen_merge(fts, bases, ALPHAS[:3], bo, layer_name=name)
        fts, bases, bo = make_inputs(shape, 3, seed=81, device=device)
        check(engine, fts, bases, ALPHAS[:3], bo, label="after an error")


def check_tiny_and_rank3(engine, device="cpu"):
    fts, bases, bo = make_inputs((0,), 2, seed=73, device=device)
    out, rep = engine.widen_merge(fts, bases, [0.5, 0.5], bo)
    assert out.numel() == 0 and out.dtype == bo.dtype and (rep.rows, rep.cols) == (0, 0) and rep.calibrated == [[0, 0], [0, 0]]
    fts, bases, bo = make_inputs((4, 33, 65), 3, seed=74, own_bases=True, device=device)
    rep, _, _, _ = check(engine, fts, bases, ALPHAS[:3], bo, calibration=0.5, label="rank 3")
    assert (rep.rows, rep.cols, rep.vector_mode) == (4, 33 * 65, False)
    fts, bases, bo = make_inputs((300,), 2, seed=75, own_bases=True, device=device)       # a 1-D tensor is one row
    rep, _, _, _ = check(engine, fts, bases, ALPHAS[:2], bo, label="1-D")
    assert (rep.rows, rep.cols, rep.vector_mode) == (1, 300, True)
    fts, bases, bo = make_inputs((1, 1), 2, seed=76, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:2], bo, label="1 x 1")


def check_determinism(engine, device="cpu"):
    fts, bases, bo = make_inputs((600, 500), 3, seed=90, own_bases=True, device=device)
    a, ra = engine.widen_merge(fts, bases, ALPHAS[:3], bo)
    b, rb = engine.widen_merge(fts, bases, ALPHAS[:3], bo)
    assert torch.equal(raw(a), raw(b)) and ra == rb


def check_arguments(engine, device="cpu"):
    fts, bases, bo = make_inputs((8, 8), 2, seed=91, device=device)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ratio"):
            engine.widen_merge(fts, bases, [0.5, 0.5], bo, ratio=bad)
    for bad in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="calibration"):
            engine.widen_merge(fts, bases, [0.5, 0.5], bo, calibration=bad)
    with pytest.raises(ValueError, match="lam"):
        engine.widen_merge(fts, bases, [0.5, 0.5], bo, lam=float("inf"))
    with pytest.raises(ValueError, match="shape mismatch"):
        engine.widen_merge([fts[0], fts[1][:4]], bases, [0.5, 0.5], bo)
    with pytest.raises(ValueError, match="supported range"):
        engine.widen_merge([fts[0]] * 17, [bases[0]] * 17, [0.1] * 17, bo)
    with pytest.raises(ValueError, match="alphas"):
        engine.widen_merge(fts, bases, [0.5], bo)
    wide = torch.zeros((1, 65537), dtype=torch.bfloat16, device=device)
    with pytest.raises(ValueError, match="65537 columns, at most 65536"):
        engine.widen_merge([wide], [wide], [1.0], wide, layer_name="wide")


# ---- properties, through the engine alone ---------------------------------------------------------------------
def _stats_call(engine, fts, bases, alphas, bo, **kw):
    out, rep, delta = engine.widen_merge(fts, bases, alphas, bo, want_stats=True, want_delta=True, **kw)
    return out, rep, delta.cpu()


def check_column_permutation(engine, device="cpu"):
    """permuting the columns of all inputs permutes the output's columns: a column's sums never see another column and the
    ranks are order-free"""
    for shape, k in (((530, 72), 3), ((1, 300), 2), ((9, 131), 5)):
        fts, bases, bo = make_inputs(shape, k, seed=100 + k, own_bases=True, device=device)
        perm = torch.randperm(shape[1], generator=torch.Generator().manual_seed(5)).to(bo.device)
        p = lambda t: t[:, perm].contiguous()
        a, ra, da = _stats_call(engine, fts, bases, ALPHAS[:k], bo, calibration=0.5, lam=0.7)
        b, rb, db = _stats_call(engine, [p(t) for t in fts], [p(t) for t in bases], ALPHAS[:k], p(bo), calibration=0.5, lam=0.7)
        perm = perm.cpu()
        assert torch.equal(raw(a.cpu()[:, perm]), raw(b)) and torch.equal(raw(da[:, perm]), raw(db))
        assert torch.equal(ra.rank[:, :, perm], rb.rank) and torch.equal(ra.weight[:, perm].view(torch.int32), rb.weight.view(torch.int32))
        assert ra.mu == rb.mu and ra.calibrated == rb.calibrated


def check_swap(engine, device="cpu"):
    """k = 2: two-term sums commute, so the order of the entries does not show in a single byte"""
    for shape, own in ((SHAPE, False), (SHAPE, True), ((1, 99), True)):
        fts, bases, bo = make_inputs(shape, 2, seed=110, own_bases=own, device=device)
        a, ra, da = _stats_call(engine, fts, bases, [0.5, 0.3], bo, calibration=0.5)
        b, rb, db = _stats_call(engine, fts[::-1], bases[::-1], [0.3, 0.5], bo, calibration=0.5)
        assert torch.equal(raw(a), raw(b)) and torch.equal(raw(da), raw(db))
        assert ra.mu == rb.mu[::-1] and ra.calibrated == rb.calibrated[::-1] and torch.equal(ra.rank, rb.rank.flip(0))


def check_scale_by_two(engine, device="cpu"):
    """fp32 inputs, every finetune and base times 2: every rank and weight unchanged, delta_out doubled"""
    for shape in ((520, 40), (1, 200)):
        fts, bases, bo = make_inputs(shape, 3, torch.float32, seed=120, own_bases=True, device=device)
        a, ra, da = _stats_call(engine, fts, bases, ALPHAS[:3], bo, calibration=0.5, lam=0.7)
        b, rb, db = _stats_call(engine, [2 * t for t in fts], [2 * t for t in bases], ALPHAS[:3], bo, calibration=0.5, lam=0.7)
        assert torch.equal(ra.rank, rb.rank) and torch.equal(ra.weight.view(torch.int32), rb.weight.view(torch.int32))
        assert ra.mu == rb.mu and ra.calibrated == rb.calibrated
        assert torch.equal(raw(2 * da), raw(db)) and torch.equal(u64_t(2 * ra.stat[:, 0]), u64_t(rb.stat[:, 0]))
        assert torch.equal(u64_t(ra.stat[:, 1]), u64_t(rb.stat[:, 1]))


def u64_t(t):
    return t.contiguous().view(torch.int64)


def _dare_linear(engine, fts, bases, alphas, bo, lam):
    k = len(fts)
    out, _, delta = engine.dare_merge(fts, bases, alphas, bo, density=1.0, lam=lam, normalize=False, rescale=True,
                                      sign_election=False, key=0, stream_ids=list(range(k)), want_delta=True)
    return out, delta.cpu()


def check_dare_linear_identities(engine, device="cpu"):
    """k = 1 with calibration 1 (any ratio), and any k with ratio -1 and calibration 1, are dare_linear at density 1 without
    normalize; with ratio 0 the columns whose ranks are all positive are"""
    for shape in (SHAPE, (1, 200), (600, 24)):
        fts, bases, bo = make_inputs(shape, 1, seed=130, own_bases=True, device=device)
        want, dwant = _dare_linear(engine, fts, bases, [0.6], bo, 0.7)
        for ratio in RATIOS:
            out, rep, delta = _stats_call(engine, fts, bases, [0.6], bo, ratio=ratio, calibration=1.0, lam=0.7)
            assert torch.equal(raw(out), raw(want)) and torch.equal(raw(delta), raw(dwant)), (shape, ratio)
        for k, own in ((2, False), (5, True), (16, True)):
            alphas = [a if i % 3 else -a for i, a in enumerate(ALPHAS[:k])]
            fts, bases, bo = make_inputs(shape, k, seed=130 + k, own_bases=own, device=device)
            want, dwant = _dare_linear(engine, fts, bases, alphas, bo, 0.7)
            out, rep, delta = _stats_call(engine, fts, bases, alphas, bo, ratio=-1.0, calibration=1.0, lam=0.7)
            assert all(m > 0 for row in rep.mu for m in row[:1 if rep.vector_mode else 2])      # the statistics are not all equal
            assert torch.equal(raw(out), raw(want)) and torch.equal(raw(delta), raw(dwant)), (shape, k)
            out, rep, delta = _stats_call(engine, fts, bases, alphas, bo, ratio=0.0, calibration=1.0, lam=0.7)
            ns = 1 if rep.vector_mode else 2
            positive = (rep.rank[:, :ns] > 0).all(dim=0).all(dim=0)
            assert 0 < int(positive.sum()) < rep.cols
            view = lambda t: t.reshape(rep.rows, rep.cols)[:, positive]
            assert torch.equal(raw(view(delta)), raw(view(dwant))), (shape, k)
            if not rep.vector_mode:             # (in vector mode the lowest rank is a delta of 0, which no weight shows)
                assert not torch.equal(raw(delta), raw(dwant))


def check_calibrated_sets(engine, device="cpu"):
    """calibrated does not depend on widen_calibration; the calibrated sets grow as widen_ratio falls"""
    for shape, k in ((SHAPE, 3), ((1, 300), 2)):
        fts, bases, bo = make_inputs(shape, k, seed=140, own_bases=True, device=device)
        reps = {}
        for ratio in sorted(RATIOS):
            per = [_stats_call(engine, fts, bases, ALPHAS[:k], bo, ratio=ratio, calibration=c)[1] for c in CALIBRATIONS]
            assert all(r.calibrated == per[0].calibrated and r.mu == per[0].mu for r in per)
            reps[ratio] = per
        # the sets themselves, through the weights at calibration 2 (index 3), which no softmax value reaches: a column's
        # w / alpha is 2 with every statistic calibrated, in [1, 1.5] with one of two, below 1 with none
        def calibrated_stats(rep):
            h = rep.weight.double() / torch.tensor(ALPHAS[:k], dtype=torch.float64)[:, None]
            return (h >= 1.0).to(torch.int64) + (h >= 1.75).to(torch.int64) if not rep.vector_mode else (h >= 1.0).to(torch.int64)
        for lo, hi in zip(sorted(RATIOS), sorted(RATIOS)[1:]):
            a, b = reps[lo], reps[hi]
            assert all(x >= y for ra, rb in zip(a[0].calibrated, b[0].calibrated) for x, y in zip(ra, rb))
            assert bool((calibrated_stats(a[3]) >= calibrated_stats(b[3])).all())
            assert [int(c.sum()) for c in calibrated_stats(a[3])] == [sum(row) for row in a[3].calibrated]
        assert reps[-1.0][0].calibrated[0][0] == reps[1.0][0].cols > reps[3.0][0].calibrated[0][0]


CORNERS = [check_unaligned, check_bases, check_signed_alphas, check_zero_finetunes, check_untouched_columns, check_tied_columns,
           check_zero_columns, check_nonfinite, check_tiny_and_rank3, check_determinism, check_arguments, check_column_permutation,
           check_swap, check_scale_by_two, check_dare_linear_identities, check_calibrated_sets]


# ---- profile names and launches ----------------------------------------------------------------------------
PROFILES = [((40, 50), 2, {"widen_colstats": 1, "widen_colfold": 1, "widen_rank": 1, "widen_coef": 1, "widen_combine": 1}),
            ((40, 50), 5, {"widen_colstats": 1, "widen_colfold": 1, "widen_rank": 1, "widen_coef": 1, "widen_combine": 1}),
            ((1, 500), 3, {"widen_colfold": 1, "widen_rank": 1, "widen_coef": 1, "widen_combine": 1})]
PROFILE_IDS = ["matrix_k2", "matrix_k5", "vector_k3"]


def check_profile(engine, shape, k, expected, device="cpu"):
    """five kernels in matrix mode, four in vector mode, one launch each whatever k"""
    fts, bases, bo = make_inputs(shape, k, seed=6, device=device)
    got = profile_of(engine, lambda: engine.widen_merge(fts, bases, ALPHAS[:k], bo))
    assert got == expected, got


# ---- independent of the oracle: the column sums against math.fsum ------------------------------------------
def check_sums_against_fsum(engine, shape=(1030, 257), device="cpu"):
    """P, B and X of eight sampled columns stay within (R - 1) 2^-53 sum |terms| of math.fsum of the exact products (the
    Gram's bound).  The sums are the oracle's, which `check` ties to the engine's m and d bit for bit."""
    fts, bases, bo = make_inputs(shape, 2, torch.float32, seed=150, own_bases=True, device=device)   # (sums of bf16 products would be exact)
    _, _, _, ref = check(engine, fts, bases, ALPHAS[:2], bo, label="fsum")
    R, C_ = shape
    cols = np.random.default_rng(3).choice(C_, 8, replace=False)
    worst = 0.0
    for i in range(2):
        f, b = fts[i].cpu().double().numpy(), bases[i].cpu().double().numpy()
        for got, x, y in zip(ref["sums"][i], (f, b, f), (f, b, b)):
            for j in cols:
                terms = (x[:, j] * y[:, j]).tolist()                      # exact: products of fp32 values in fp64
                exact, mass = math.fsum(terms), math.fsum(abs(t) for t in terms)
                bound = (R - 1) * 2.0 ** -53 * mass
                assert abs(float(got[j]) - exact) <= bound, (i, j, float(got[j]), exact, bound)
                worst = max(worst, abs(float(got[j]) - exact) / bound)
    print(f"column sums against fsum: largest error / bound {worst:.4f}")


# ---- independent of the oracle: the paper's form in torch fp64 --------------------------------------------------
PAPER_CASES = [((512, 1024), 2), ((1024, 4096), 3), ((300, 4544), 2)]


def paper_inputs(shape, k, seed, device="cpu"):
    """Gaussian bases (sigma 0.02) with bf16 deltas of sigma 3e-3 (1 + 0.3 i), times a per-column scale log-uniform in
    about [0.5, 2]"""
    g = torch.Generator().manual_seed(3000 + seed)
    base = (torch.randn(shape, generator=g) * 0.02).to(torch.bfloat16)
    fts = []
    for i in range(k):
        scale = torch.exp2(torch.rand(shape[1], generator=g) * 2.0 - 1.0)
        fts.append((base.float() + torch.randn(shape, generator=g) * 3e-3 * (1 + 0.3 * i) * scale[None, :]).to(torch.bfloat16).to(device))
    base = base.to(device)
    return fts, [base] * k, base


def paper_reference(fts, bases, alphas, ratio, calibration):
    """-> (stats [k][2] fp64 [C], ranks [k][2], weights [k] fp64 [C], merged fp64 [R, C], mass): torch.norm(dim=0), W / norm,
    1 - cosine_similarity(dim=0), stable argsort, torch.softmax, the mean cut, 0.5 (m + d), the weighted sum"""
    k = len(fts)
    C_ = fts[0].shape[1]
    stats, ranks, sig = [], [], []
    for ft, bs in zip(fts, bases):
        W, B = ft.cpu().double(), bs.cpu().double()
        nw, nb = torch.norm(W, dim=0), torch.norm(B, dim=0)
        m = (nw - nb).abs()
        d = 1.0 - torch.cosine_similarity(W / nw, B / nb, dim=0)
        per = []
        for s in (m, d):
            order = torch.argsort(s, stable=True)
            r = torch.empty(C_, dtype=torch.int64)
            r[order] = torch.arange(C_)
            per.append(r)
        stats.append((m, d)); ranks.append(per); sig.append([r.double() / C_ for r in per])
    scores = []
    for s in range(2):
        p = torch.softmax(torch.stack([sig[i][s] for i in range(k)]), dim=0)
        for i in range(k):
            cut = sig[i][s] > ratio * sig[i][s].mean()
            p[i] = torch.where(cut, torch.full_like(p[i], calibration), p[i])
        scores.append(p)
    weights = [alphas[i] * 0.5 * (scores[0][i] + scores[1][i]) for i in range(k)]
    merged = torch.zeros(fts[0].shape, dtype=torch.float64)
    mass = torch.zeros_like(merged)
    for i in range(k):
        x = fts[i].cpu().double() - bases[i].cpu().double()
        merged += weights[i][None, :] * x
        mass += (weights[i][None, :] * x).abs()
    return stats, ranks, weights, merged, mass


def uncertain_columns(stats, bases, R):
    """columns one of whose statistics lies within 2 (R + 16) 2^-52 max(1, max_j sqrt(B)) of another column's"""
    C_ = stats[0][0].numel()
    bad = torch.zeros(C_, dtype=torch.bool)
    for (m, d), bs in zip(stats, bases):
        tol = 2.0 * (R + 16) * 2.0 ** -52 * max(1.0, float(torch.norm(bs.cpu().double(), dim=0).max()))
        for s in (m, d):
            v, order = torch.sort(s)
            close = (v[1:] - v[:-1]) <= tol
            near = torch.zeros(C_, dtype=torch.bool)
            near[1:] |= close
            near[:-1] |= close
            bad[order[near]] = True
    return bad


def check_paper_form(engine, shape, k, ratio=1.0, calibration=1.0, device="cpu"):
    fts, bases, bo = paper_inputs(shape, k, seed=k, device=device)
    alphas = list(ALPHAS[:k])
    _, rep, delta = engine.widen_merge(fts, bases, alphas, bo, ratio=ratio, calibration=calibration, want_stats=True, want_delta=True)
    stats, ranks, weights, merged, mass = paper_reference(fts, bases, alphas, ratio, calibration)
    R, C_ = shape
    bad = uncertain_columns(stats, bases, R)
    good = ~bad
    dworst = max(float((rep.stat[i, 1] - stats[i][1]).abs().max()) for i in range(k))
    print(f"paper form {shape} k={k}: uncertain columns {int(bad.sum())} of {C_}, largest |d - d_ref| {dworst:.3g}")
    assert int(bad.sum()) <= 1e-3 * C_, int(bad.sum())
    wworst = 0.0
    for i in range(k):
        for s in range(2):
            assert torch.equal(rep.rank[i, s][good], ranks[i][s][good]), (i, s, int((rep.rank[i, s] != ranks[i][s]).sum()))
        w, wr = rep.weight[i].double()[good], weights[i][good]
        assert bool(((w - wr).abs() <= 2.0 ** -22 * wr.abs()).all()), (i, float(((w - wr).abs() / wr.abs()).max()))
        wworst = max(wworst, float(((w - wr).abs() / wr.abs()).max()))
    err = (delta.cpu().double() - merged).abs()[:, good]
    bound = ((k + 2) * EPS * mass)[:, good]
    live = bound > 0
    print(f"  largest |w - w_ref| / |w_ref| 2^{math.log2(max(wworst, 1e-300)):.2f}, largest delta error / bound "
          f"{float((err[live] / bound[live]).max()):.4f}")
    assert bool((err <= bound).all()), float((err[live] / bound[live]).max())


# ---- model shapes: the device against the emulator ---------------------------------------------------------
def check_equals_emulator(engine, emul, shape, k, device):
    fts, bases, bo = make_inputs(shape, k, seed=sum(shape) % 97, device=device)
    kw = dict(calibration=0.5, lam=0.7, want_stats=True, want_delta=True)
    out, rep, delta = engine.widen_merge(fts, bases, ALPHAS[:k], bo, **kw)
    cpu = lambda ts: [t.cpu() for t in ts]
    cb = cpu(bases[:1]) * k
    eout, erep, edelta = emul.widen_merge(cpu(fts), cb, ALPHAS[:k], cb[0], **kw)
    assert torch.equal(raw(out), raw(eout)) and torch.equal(raw(delta), raw(edelta))
    assert torch.equal(u64_t(rep.stat), u64_t(erep.stat)) and torch.equal(rep.rank, erep.rank)
    assert torch.equal(rep.weight.view(torch.int32), erep.weight.view(torch.int32))
    assert rep.mu == erep.mu and rep.calibrated == erep.calibrated


# ---- the C ABI ------------------------------------------------------------------------------------------------
def check_c_abi(engine, device="cpu"):
    from shardmerge_amd import _lib
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(64, generator=g) * 0.01).to(torch.bfloat16).to(device)
    y = torch.zeros(64, dtype=torch.bfloat16, device=device)
    out = torch.zeros(64, dtype=torch.bfloat16, device=device)
    dll, h = engine.lib.dll, engine.ctx.h

    def call(k=1, rows=8, ratio=1.0, calibration=1.0, out_t=out, n=64, in_dtype=_lib.BF16, lam=1.0, alpha=0.5):
        d = _lib.WidenDesc()
        d.k = k
        for i in range(max(0, min(k, 16))):
            d.finetune[i], d.base[i], d.alpha[i] = x.data_ptr(), y.data_ptr(), alpha
        d.in_dtype, d.base_out, d.base_out_dtype, d.n, d.rows = in_dtype, y.data_ptr(), _lib.BF16, n, rows
        d.ratio, d.calibration, d.lam = ratio, calibration, lam
        rep = _lib.WidenReport()
        rc = dll.smhip_widen_merge(h, C.byref(d), out_t.data_ptr(), None, None, None, None, C.byref(rep), None)
        return rc, dll.smhip_last_error(h).decode(), rep

    rc, msg, rep = call()
    assert rc == _lib.OK and (rep.rows, rep.cols, rep.vector_mode) == (8, 8, 0), msg
    rc, msg, rep = call(rows=1, calibration=0.0, ratio=-1e6)
    assert rc == _lib.OK and (rep.rows, rep.cols, rep.vector_mode) == (1, 64, 1) and rep.calibrated[0][0] == 64, msg
    for kwargs, word in (({"k": 0}, "k out of range"), ({"k": 17}, "k out of range"), ({"rows": 0}, "rows must divide n"),
                         ({"rows": 7}, "rows must divide n"), ({"rows": 128}, "rows must divide n"), ({"calibration": -1e-9}, "calibration"),
                         ({"calibration": float("nan")}, "calibration"), ({"calibration": float("inf")}, "calibration"),
                         ({"ratio": float("nan")}, "ratio"), ({"ratio": float("inf")}, "ratio"), ({"lam": float("inf")}, "lambda"),
                         ({"alpha": float("nan")}, "alpha"), ({"out_t": x}, "overlaps"), ({"in_dtype": 3}, "dtype")):
        rc, msg, _ = call(**kwargs)
        assert rc == _lib.ERR_ARG and word in msg, (kwargs, rc, msg)
    # C too large: the check needs no memory behind the pointers' ends (rows = 1, n = 65537 is refused before any launch)
    big = torch.zeros(65537, dtype=torch.bfloat16, device=device)
    d = _lib.WidenDesc()
    d.k, d.in_dtype, d.base_out_dtype, d.n, d.rows, d.ratio, d.calibration, d.lam = 1, _lib.BF16, _lib.BF16, 65537, 1, 1.0, 1.0, 1.0
    d.finetune[0], d.base[0], d.base_out, d.alpha[0] = big.data_ptr(), big.data_ptr(), big.data_ptr(), 1.0
    big_out = torch.zeros(65537, dtype=torch.bfloat16, device=device)
    rc = dll.smhip_widen_merge(h, C.byref(d), big_out.data_ptr(), None, None, None, None, None, None)
    assert rc == _lib.ERR_ARG and "more than 65536 columns" in dll.smhip_last_error(h).decode()
    d.rows, d.n = 2, 2 * 65536                               # 65536 columns are accepted (the tensors are too short: n is not run)
    rc = dll.smhip_widen_merge(h, None, out.data_ptr(), None, None, None, None, None, None)
    assert rc == _lib.ERR_ARG and "null descriptor" in dll.smhip_last_error(h).decode()
    assert call(n=0, out_t=x)[0] == _lib.OK                     # a no-op, whatever the pointers


# ---- the CLI on the synthetic on-disk model of tests/lora_fixtures.py ----------------------------------------
OPTIONS = {"operator": "widen", "widen_ratio": 0.5, "widen_calibration": 0.8, "widen_lambda": 0.7}


def write_config(root, third, out_dir, opts, device=None):
    return harness.write_config(root, ties_models(third), out_dir, opts, device)


def expected_outputs(engine, base, full, opts, models=None):
    """the oracle tensor by tensor (block tensors) / the provider's tensor (passthrough); the models of ties_models:
    layer 0 has three entries, layer 1 two.  models: the finetune_merge entries, if others."""
    def merge(fts, bases, alphas, base_out, name):
        return wo.widen_merge(
            fts, bases, alphas, base_out, ratio=opts.get("widen_ratio", 1.0), calibration=opts.get("widen_calibration", 1.0),
            lam=opts.get("widen_lambda", 1.0), exp=wo.exp_of(engine))["out"]

    return expected_by_tensor(base, full, models or ties_models("org/lora_full"), merge)
