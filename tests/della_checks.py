"""Checks of the DELLA operators shared by the emulator tier (tests/test_della_host.py) and the GPU tier
(tests/test_della_gpu.py): Engine.della_merge against tests/della_oracle.py, BIT FOR BIT - output, merged delta, the
per-element thresholds, T_lo, T_hi and the kept counts.  The tolerance is zero and it is derived, not measured: every step
of the function is an integer function, an exact count or one correctly rounded operation (include/shardmerge_hip.h,
smhip_della_merge)."""
import math

import numpy as np
import pytest
import torch

from tests import dare_oracle, della_oracle
from tests import harness
from tests.dare_checks import KEY, STAT_KEY, STAT_STREAMS, dare_models, stream_ids
from tests.harness import ALPHAS, DTYPES, SMALL, expected_by_tensor, make_inputs, raw

WINDOWS = ((0.5, 0.15), (0.2, 0.1), (0.7, 0.29), (0.5, 0.0), (1.0, 0.0), (2.0 ** -15 + 0.01, 0.01))   # the last one: T_lo == 2
MODES = (True, False)                           # sign_election: della, della_linear
ROW_LENGTHS = (1, 2, 7, 8, 9, 255, 256, 257, 1000, 4096, 4097, 32768)
STAT_WINDOWS = ((0.5, 0.15), (0.2, 0.1), (0.7, 0.29), (0.5, 0.0))
STAT_SHAPE = (256, 4096)


def mode_name(sign_election):
    return "della" if sign_election else "della_linear"


def check(engine, fts, bases, alphas, base_out, density=0.5, epsilon=0.15, lam=1.0, normalize=True, rescale=True,
          sign_election=True, key=KEY, stream_ids=None, label=""):
    """one call against the oracle, bit for bit; returns (the engine's report, the oracle's thresholds)"""
    kw = dict(density=density, epsilon=epsilon, lam=lam, normalize=normalize, rescale=rescale, sign_election=sign_election,
              key=key, stream_ids=stream_ids)
    out, rep, delta, thr = engine.della_merge(fts, bases, alphas, base_out, want_delta=True, want_thresholds=True, **kw)
    cpu = lambda ts: [t.cpu() for t in ts]
    ref, ref_delta, ref_thr, T_lo, T_hi, kept = della_oracle.della_merge(cpu(fts), cpu(bases), alphas, base_out.cpu(), **kw)
    print(f"{label}: T {rep.threshold_lo}..{rep.threshold_hi} / {T_lo}..{T_hi}, kept {rep.kept} / {kept}")
    assert out.dtype == base_out.dtype and out.shape == base_out.shape, label
    assert (rep.threshold_lo, rep.threshold_hi) == (T_lo, T_hi), (label, rep, T_lo, T_hi)
    assert thr.shape == ref_thr.shape, label
    bad = int((thr.cpu() != ref_thr).sum())
    assert bad == 0, f"{label}: {bad} of {ref_thr.numel()} thresholds differ"
    assert rep.kept == kept, (label, rep.kept, kept)
    bad = int((raw(delta) != raw(ref_delta)).sum())
    assert bad == 0, f"{label}: {bad} of {ref_delta.numel()} merged-delta values differ in their bits"
    bad = int((raw(out) != raw(ref)).sum())
    assert bad == 0, f"{label}: {bad} of {ref.numel()} output values differ in their bits"
    return rep, ref_thr


# ---- the parameter grid -------------------------------------------------------------------------------
def check_dtypes(engine, in_dtype, bo_dtype, sign_election, device="cpu"):
    fts, bases, bo = make_inputs(SMALL, 3, in_dtype, bo_dtype, seed=11, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:3], bo, density=0.2, epsilon=0.1, lam=0.7, sign_election=sign_election, label=f"{in_dtype}->{bo_dtype}")
    fts, bases, bo = make_inputs(SMALL, 2, in_dtype, bo_dtype, seed=12, device=device)      # one shared base
    check(engine, fts, bases, ALPHAS[:2], bo, normalize=False, sign_election=sign_election, label=f"{in_dtype}->{bo_dtype} shared")


def check_k_window(engine, k, window, sign_election, device="cpu"):
    density, epsilon = window
    for j, (lam, normalize) in enumerate(((1.0, True), (0.7, False))):
        fts, bases, bo = make_inputs(SMALL, k, seed=20 + k + j, own_bases=bool(j), device=device)
        rep, thr = check(engine, fts, bases, ALPHAS[:k], bo, density=density, epsilon=epsilon, lam=lam, normalize=normalize,
                         sign_election=sign_election, stream_ids=list(range(3, 3 + k)),
                         label=f"{mode_name(sign_election)} k={k} density={density} epsilon={epsilon} lam={lam} normalize={normalize}")
        if window == WINDOWS[-1]:
            assert rep.threshold_lo == 2
        if epsilon > 0 and bo.dtype == torch.bfloat16:      # the bf16 deltas tie heavily: fewer ranks than elements, more than a handful
            distinct = len(np.unique(thr[0][0].numpy()))
            assert 8 < distinct < SMALL[1], distinct


def check_options(engine, lam, normalize, rescale, sign_election, device="cpu"):
    fts, bases, bo = make_inputs((64, 200), 3, seed=40, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:3], bo, lam=lam, normalize=normalize, rescale=rescale, sign_election=sign_election,
          label=f"lam={lam} normalize={normalize} rescale={rescale}")


def check_signed_alphas(engine, device="cpu"):
    for sign_election in MODES:
        for normalize in (True, False):
            fts, bases, bo = make_inputs(SMALL, 4, seed=50, own_bases=True, device=device)
            check(engine, fts, bases, [0.5, -0.3, 0.0, -0.7], bo, lam=0.7, normalize=normalize, sign_election=sign_election, label="signed alphas")


# ---- row lengths where the sort and the lower bound can go wrong --------------------------------------------------
def check_row_length(engine, c, device="cpu"):
    for j, in_dtype in enumerate((torch.bfloat16, torch.float32)):
        fts, bases, bo = make_inputs((3, c), 2, in_dtype, seed=200 + j, own_bases=bool(j), device=device)
        rep, thr = check(engine, fts, bases, ALPHAS[:2], bo, sign_election=bool(j), label=f"c={c} {in_dtype}")
        if c == 1:
            assert rep.threshold_lo == rep.threshold_hi == math.floor(0.35 * 65536)
        if in_dtype == torch.float32 and c > 1:       # distinct magnitudes (almost surely): every rank occurs, both ends of the window
            assert int(thr.min()) == rep.threshold_lo and int(thr.max()) == rep.threshold_hi


def check_row_too_long(engine, device="cpu"):
    fts, bases, bo = make_inputs((2, della_oracle.MAX_COLS + 1), 1, seed=210, device=device)
    with pytest.raises(ValueError, match=r"model\.layers\.3\.mlp.*32769.*32768"):
        engine.della_merge(fts, bases, [1.0], bo, layer_name="model.layers.3.mlp.up_proj.weight")
    check(engine, fts, bases, [1.0], bo, epsilon=0.0, label="c = 32769 without a window")        # nothing is ranked: any row length
    fts, bases, bo = make_inputs((della_oracle.MAX_COLS + 1,), 1, seed=211, device=device)       # a 1-D tensor is one row
    with pytest.raises(ValueError, match="32769"):
        engine.della_merge(fts, bases, [1.0], bo)


# ---- row contents -------------------------------------------------------------------------------------------
def check_row_contents(engine, device="cpu"):
    c = 300
    g = torch.Generator().manual_seed(220)
    mags = torch.rand(c, generator=g) + 0.5
    signs = torch.where(torch.rand(c, generator=g) < 0.5, -1.0, 1.0)
    rows = [torch.full((c,), 0.75) * signs,                              # equal magnitudes, mixed signs: every rank 0
            torch.zeros(c),                                              # all zero: rank 0, nothing kept
            torch.sort(mags).values * signs,                             # ascending
            torch.sort(mags, descending=True).values * signs,            # descending
            torch.where(torch.arange(c) % 3 == 0, 0.0, 1.0) * mags * signs,   # a third zero
            torch.cat([torch.zeros(c // 2), -torch.zeros(c - c // 2)])]  # +0 and -0
    d = torch.stack(rows).to(device)
    zero = torch.zeros_like(d)
    for sign_election in MODES:
        rep, thr = check(engine, [d, d * 0.5], [zero, zero], [0.5, 0.75], zero, lam=0.7, sign_election=sign_election, label="row contents")
        t = thr[0]
        assert bool((t[0] == rep.threshold_lo).all()) and bool((t[1] == rep.threshold_lo).all()) and bool((t[5] == rep.threshold_lo).all())
        assert bool((t[2][1:] >= t[2][:-1]).all()) and bool((t[3][1:] <= t[3][:-1]).all())
        assert int(t[2][0]) == rep.threshold_lo and int(t[2][-1]) == rep.threshold_hi and int(t[3][0]) == rep.threshold_hi
        assert bool((t[4][::3] == rep.threshold_lo).all()) and int(t[4].max()) == rep.threshold_hi
    out, rep, delta = engine.della_merge([d[1:2]], [zero[1:2]], [1.0], zero[1:2], want_delta=True)
    assert rep.kept == [0] and not bool(delta.any())


def check_zero_delta(engine, device="cpu"):
    """a finetune equal to its base: nothing of it is kept, whatever the mask"""
    for sign_election in MODES:
        fts, bases, bo = make_inputs(SMALL, 2, seed=60, device=device)
        fts[1] = bases[1].clone()
        rep, _ = check(engine, fts, bases, [0.5, 0.5], bo, density=0.3, epsilon=0.1, sign_election=sign_election, label="zero delta")
        assert rep.kept[1] == 0 and rep.kept[0] > 0


def check_denormals(engine, device="cpu"):
    g = torch.Generator().manual_seed(66)
    ft = (torch.randn(SMALL, generator=g) * 1e-40).to(device)
    zero = torch.zeros_like(ft)
    for sign_election in MODES:
        check(engine, [ft, ft * 0.5], [zero, zero], [0.5, 0.75], zero, lam=0.7, sign_election=sign_election, label="fp32 denormal deltas")


def check_unaligned_and_rank3(engine, device="cpu"):
    """views that start at an odd element; rank-3 tensors (the row is the last dimension); n == 0"""
    for dtype in DTYPES:
        fts, bases, bo = make_inputs((7, 1003 + 5), 3, dtype, seed=70, own_bases=True, device=device)
        cut = lambda t, o: t.reshape(-1)[o:o + 7 * 1003].reshape(7, 1003)
        check(engine, [cut(fts[0], 1), cut(fts[1], 3), cut(fts[2], 0)], [cut(bases[0], 0), cut(bases[1], 1), cut(bases[2], 5)],
              ALPHAS[:3], cut(bo, 1), sign_election=dtype != torch.float16, label=f"unaligned {dtype}")
    for sign_election in MODES:
        fts, bases, bo = make_inputs((4, 33, 65), 3, seed=74, own_bases=True, device=device)
        check(engine, fts, bases, ALPHAS[:3], bo, sign_election=sign_election, label="rank 3")
        fts, bases, bo = make_inputs((1003,), 2, seed=75, device=device)
        check(engine, fts, bases, ALPHAS[:2], bo, sign_election=sign_election, label="1-D: one row")
    fts, bases, bo = make_inputs((0,), 2, seed=73, device=device)
    out, rep = engine.della_merge(fts, bases, [0.5, 0.5], bo)
    assert out.numel() == 0 and out.dtype == bo.dtype and rep.kept == [0, 0]


def check_nonfinite(engine, device="cpu"):
    """a NaN / an Inf in one finetune: ValueError naming the tensor and the finetune; the context stays usable"""
    for poison in (float("nan"), float("inf"), float("-inf")):
        for epsilon in (0.15, 0.0):
            fts, bases, bo = make_inputs(SMALL, 3, seed=80, device=device)
            fts[1] = fts[1].clone()
            fts[1].view(-1)[4321] = poison
            with pytest.raises(ValueError, match=r"model\.layers\.7\.mlp\.up_proj\.weight.*finetune 1\b") as err:
                engine.della_merge(fts, bases, ALPHAS[:3], bo, epsilon=epsilon, layer_name="model.layers.7.mlp.up_proj.weight")
            # (epsilon == 0 runs DARE's pass: the text still names this entry point)
            assert str(err.value).endswith(": della_merge: NaN or Inf in finetune - base of finetune 1"), err.value
        fts, bases, bo = make_inputs(SMALL, 3, seed=81, device=device)
        check(engine, fts, bases, ALPHAS[:3], bo, label="after an error")
    fts, bases, bo = make_inputs(SMALL, 2, torch.float32, seed=82, own_bases=True, device=device)
    fts[0].view(-1)[5] = float("inf")
    bases[0].view(-1)[5] = float("inf")
    with pytest.raises(ValueError, match=r"finetune 0\b"):
        engine.della_merge(fts, bases, ALPHAS[:2], bo, sign_election=False)


BAD_WINDOWS = ((0.0, 0.0), (-0.1, 0.0), (1.5, 0.0), (float("nan"), 0.1), (0.5, float("nan")), (0.5, -0.01), (1.0, 0.1), (0.9, 0.1),
               (0.5, 0.5), (0.1, 0.1), (0.1 + 2.0 ** -17, 0.1), (2.0 ** -17, 0.0))


def check_arguments(engine, device="cpu"):
    fts, bases, bo = make_inputs((8, 8), 2, seed=91, device=device)
    for density, epsilon in BAD_WINDOWS:
        with pytest.raises(ValueError, match="density|epsilon"):
            engine.della_merge(fts, bases, [0.5, 0.5], bo, density=density, epsilon=epsilon)
        with pytest.raises(ValueError):
            della_oracle.check_arguments(density, epsilon)
    for density, epsilon in WINDOWS + ((0.1 + 2.0 ** -16, 0.1), (2.0 ** -16, 0.0)):
        engine.della_merge(fts, bases, [0.5, 0.5], bo, density=density, epsilon=epsilon)
    with pytest.raises(ValueError, match="shape mismatch"):
        engine.della_merge([fts[0], fts[1][:4]], bases, [0.5, 0.5], bo)
    with pytest.raises(ValueError, match="supported range"):
        engine.della_merge([fts[0]] * 17, [bases[0]] * 17, [0.1] * 17, bo)
    with pytest.raises(ValueError, match="alphas"):
        engine.della_merge(fts, bases, [0.5], bo)
    with pytest.raises(ValueError, match="stream_ids"):
        engine.della_merge(fts, bases, [0.5, 0.5], bo, stream_ids=[0, 2 ** 32])
    for bad in (-1, 2 ** 64, 1.5, True):
        with pytest.raises(ValueError, match="key"):
            engine.della_merge(fts, bases, [0.5, 0.5], bo, key=bad)


# ---- the identity and the properties of the definition ------------------------------------------------------------
def profiled(engine, call):
    engine.ctx.profile(True)
    engine.ctx.profile_reset()
    try:
        res = call()
        table = engine.ctx.profile_table()
    finally:
        engine.ctx.profile(False)
    return res, {n: table[n][0] for n in table}


def check_epsilon_zero_is_dare(engine, device="cpu"):
    """epsilon == 0: smhip_dare_merge bit for bit, for both modes and any key, and nothing is ranked"""
    for k, own, lam, normalize, density in ((3, True, 0.7, True, 0.5), (5, False, 1.0, False, 0.2), (1, False, 1.0, True, 1.0)):
        fts, bases, bo = make_inputs(SMALL, k, seed=100 + k, own_bases=own, device=device)
        for sign_election in MODES:
            for key in (0, KEY, 2 ** 64 - 1):
                for rescale in (True, False):
                    kw = dict(density=density, lam=lam, normalize=normalize, rescale=rescale, sign_election=sign_election, key=key,
                              stream_ids=list(range(2, 2 + k)), want_delta=True)
                    d_out, d_rep, d_delta = engine.dare_merge(fts, bases, ALPHAS[:k], bo, **kw)
                    (out, rep, delta), launches = profiled(engine, lambda: engine.della_merge(fts, bases, ALPHAS[:k], bo, epsilon=0.0, **kw))
                    assert rep.threshold_lo == rep.threshold_hi == d_rep.threshold and rep.kept == d_rep.kept
                    assert torch.equal(raw(out), raw(d_out)) and torch.equal(raw(delta), raw(d_delta)), (k, key)
                    assert launches == {"dare_merge": 1}, launches


def check_order_independence(engine, device="cpu"):
    """permuting the elements within each row (inputs together) permutes the thresholds and nothing else"""
    fts, bases, bo = make_inputs((40, 333), 2, seed=230, own_bases=True, device=device)
    perm = torch.randperm(333, generator=torch.Generator().manual_seed(231)).to(device)
    _, _, thr = engine.della_merge(fts, bases, ALPHAS[:2], bo, want_thresholds=True)
    pm = lambda ts: [t[:, perm].contiguous() for t in ts]
    _, _, thr_p = engine.della_merge(pm(fts), pm(bases), ALPHAS[:2], bo[:, perm].contiguous(), want_thresholds=True)
    assert torch.equal(thr[:, :, perm], thr_p)
    assert len(torch.unique(thr)) > 50


def check_monotone_and_nested(engine, device="cpu"):
    """within a row T does not decrease with the magnitude; the kept sets are nested in density at a fixed epsilon"""
    fts, bases, bo = make_inputs((30, 500), 1, torch.float32, seed=110, device=device)
    call = lambda density: engine.della_merge(fts, bases, [1.0], bo, density=density, epsilon=0.1, normalize=False, rescale=False,
                                              sign_election=False, key=KEY, stream_ids=[5], want_delta=True, want_thresholds=True)
    _, ra, a, ta = call(0.2)
    _, rb, b, tb = call(0.4)
    mag = (fts[0].float() - bases[0].float()).abs().cpu()
    order = torch.argsort(mag, dim=1)
    sorted_t = torch.gather(ta[0].cpu(), 1, order)
    assert bool((sorted_t[:, 1:] >= sorted_t[:, :-1]).all())
    assert bool((tb >= ta).all())
    a, b = raw(a), raw(b)
    nz = a != 0
    assert 0 < ra.kept[0] < rb.kept[0]
    assert int(nz.sum()) == ra.kept[0] and int((b != 0).sum()) == rb.kept[0]
    assert torch.equal(a[nz], b[nz])


def check_slabs(engine, device="cpu"):
    """slabs of 1, 7 and 64 rows give the bytes of one slab: the mask is indexed in the tensor, not in the slab"""
    fts, bases, bo = make_inputs((64, 1000), 3, seed=240, own_bases=True, device=device)
    fts2, bases2, bo2 = make_inputs((13, 131), 2, seed=241, device=device)           # rows that start inside an octet
    big, small = [], []
    try:
        for rows in (0, 1, 7, 64):
            engine.ctx.debug_option("della_slab_rows", rows)
            res, launches = profiled(engine, lambda: engine.della_merge(fts, bases, ALPHAS[:3], bo, key=KEY, want_delta=True, want_thresholds=True))
            slabs = 1 if rows == 0 else -(-64 // rows)
            assert launches == {"della_table": 1, "della_rank": slabs, "della_merge": slabs}, (rows, launches)
            big.append(res)
            small.append(engine.della_merge(fts2, bases2, ALPHAS[:2], bo2, key=KEY, sign_election=False, want_delta=True, want_thresholds=True))
    finally:
        engine.ctx.debug_option("della_slab_rows", 0)
    for results in (big, small):
        ref = results[0]
        for res in results[1:]:
            assert res[1] == ref[1]
            assert torch.equal(raw(res[0]), raw(ref[0])) and torch.equal(raw(res[2]), raw(ref[2])) and torch.equal(res[3], ref[3])
    check(engine, fts, bases, ALPHAS[:3], bo, key=KEY, label="slabs: the default against the oracle")
    try:
        engine.ctx.debug_option("della_slab_rows", 3)
        check(engine, fts2, bases2, ALPHAS[:2], bo2, key=KEY, sign_election=False, label="slabs of 3 rows of 131 against the oracle")
    finally:
        engine.ctx.debug_option("della_slab_rows", 0)


def check_determinism(engine, device="cpu"):
    """the same call twice: the same bytes; another stream or key: another mask, the same thresholds"""
    fts, bases, bo = make_inputs((30, 500), 3, seed=90, own_bases=True, device=device)
    a, ra = engine.della_merge(fts, bases, ALPHAS[:3], bo, key=KEY)
    b, rb = engine.della_merge(fts, bases, ALPHAS[:3], bo, key=KEY)
    assert torch.equal(raw(a), raw(b)) and ra == rb
    one = lambda key, sid: engine.della_merge(fts[:1], bases[:1], [1.0], bo, normalize=False, rescale=False, sign_election=False, key=key,
                                              stream_ids=[sid], want_delta=True, want_thresholds=True)[2:]
    ref, ref_t = one(KEY, 0)
    for key, sid in ((KEY, 1), (KEY + 1, 0)):
        other, other_t = one(key, sid)
        assert torch.equal(ref_t, other_t)
        differ = int(((ref != 0) != (other != 0)).sum())
        assert differ > ref.numel() // 4, differ


def check_statistics(engine, window, device="cpu"):
    """256 x 4096 non-zero deltas of distinct magnitudes: the kept share within 6 sigma of mean(T / 65536), the kept share
    of the upper half of the ranks minus that of the lower half within 6 sigma of its expectation (sums of independent
    Bernoulli variables of probability q = T / 65536: the variance is the sum of q (1 - q))"""
    density, epsilon = window
    R, c = STAT_SHAPE
    n = R * c
    d = (torch.rand(n, generator=torch.Generator().manual_seed(140)) + 0.5).reshape(R, c).to(device)
    zero = torch.zeros_like(d)
    upper = torch.from_numpy(della_oracle.ranks(della_oracle.magnitude_bits(d.cpu())) >= c // 2).reshape(-1)      # the upper half of the ranks
    for sid in STAT_STREAMS:
        _, rep, delta, thr = engine.della_merge([d], [zero], [1.0], zero, density=density, epsilon=epsilon, normalize=False, rescale=False,
                                                sign_election=False, key=STAT_KEY, stream_ids=[sid], want_delta=True, want_thresholds=True)
        m = (delta.cpu() != 0).reshape(-1)
        q = thr[0].cpu().reshape(-1).double() / 65536.0
        assert rep.kept == [int(m.sum())]
        h = torch.from_numpy(dare_oracle.draws(STAT_KEY, sid, 0, n >> 3).astype(np.int32))
        assert torch.equal(m, h < thr[0].cpu().reshape(-1))
        sigma = math.sqrt(float((q * (1 - q)).sum())) / n
        dev = abs(rep.kept[0] / n - float(q.mean()))
        print(f"window {window} stream {sid}: kept {rep.kept[0] / n:.7f}, mean q {float(q.mean()):.7f}, {dev / sigma:.2f} sigma")
        assert dev <= 6 * sigma
        nu, nl = int(upper.sum()), int((~upper).sum())
        gap = float(m[upper].sum()) / nu - float(m[~upper].sum()) / nl
        expect = float(q[upper].mean() - q[~upper].mean())
        sigma = math.sqrt(float((q[upper] * (1 - q[upper])).sum()) / nu ** 2 + float((q[~upper] * (1 - q[~upper])).sum()) / nl ** 2)
        print(f"window {window} stream {sid}: upper - lower {gap:.7f}, expected {expect:.7f}, {abs(gap - expect) / sigma:.2f} sigma")
        assert abs(gap - expect) <= 6 * sigma


# ---- the CLI on the synthetic on-disk model of tests/lora_fixtures.py ----------------------------------------
def options(operator):
    return {"operator": operator, "density": 0.4, "epsilon": 0.2, "della_lambda": 0.7, "seed": 2 ** 62 + 12345}


def write_config(root, third, out_dir, opts, device=None):
    return harness.write_config(root, dare_models(third), out_dir, opts, device)


def expected_outputs(base, full, opts):
    """the oracle tensor by tensor (block tensors) / the provider's tensor (passthrough)"""
    models = dare_models("org/lora_full")
    def merge(fts, bases, alphas, base_out, name):
        return della_oracle.della_merge(
            fts, bases, alphas, base_out, density=opts.get("density", 0.5), epsilon=opts.get("epsilon", 0.15),
            lam=opts.get("della_lambda", 1.0), normalize=bool(opts.get("della_normalize", 1)),
            rescale=bool(opts.get("della_rescale", 1)), sign_election=opts["operator"] == "della",
            key=dare_oracle.tensor_key(opts.get("seed", 0), name), stream_ids=stream_ids(models, name))[0]

    return expected_by_tensor(base, full, models, merge)
