"""Checks of the CABS operator shared by the emulator tier (tests/test_cabs_host.py) and the GPU tier
(tests/test_cabs_gpu.py): Engine.cabs_merge against tests/cabs_oracle.py, BIT FOR BIT - output, merged delta, the kept
bits of every element and every field of the report.  The tolerance is zero and it is derived, not measured: every step
of the function is an integer function, an exact order statistic or one correctly rounded fp32 operation
(include/shardmerge_hip.h, smhip_cabs_merge)."""
import ctypes as C

import pytest
import torch

from tests import cabs_oracle
from tests import harness
from tests.harness import ALPHAS, expected_by_tensor, make_inputs, profile_of, raw, ties_models

COLS = (1, 3, 7, 8, 9, 63, 64, 65, 133, 511, 512, 513, 1025, 2053, 4544)    # around the group, octet and work-group edges
GROUPS = (4, 8, 16, 64, 512)
LAMBDAS = (1.0, 0.7, -0.5)
KS = (1, 2, 3, 4, 5, 16)                        # 4 | 5 straddles the two register variants of the kernel
OPTIONS = {"operator": "cabs", "cabs_n": 8, "cabs_m": 32, "cabs_conflict_aware": 1, "cabs_lambda": 0.7}


def n_keeps(M):
    return sorted({1, M // 4, M - 1, M})


def check(engine, fts, bases, alphas, base_out, n_keep=16, group=64, conflict_aware=True, lam=1.0, label=""):
    """one call against the oracle, bit for bit, and the invariants of the report; returns (report, out, delta)"""
    kw = dict(n_keep=n_keep, group=group, conflict_aware=conflict_aware, lam=lam)
    out, rep, delta = engine.cabs_merge(fts, bases, alphas, base_out, want_delta=True, want_mask=True, **kw)
    cpu = lambda ts: [t.cpu() for t in ts]
    ref = cabs_oracle.cabs_merge(cpu(fts), cpu(bases), alphas, base_out.cpu(), **kw)
    k, n = len(fts), base_out.numel()
    print(f"{label}: kept {rep.kept} / {ref['kept']}, short {rep.short_groups} / {ref['short_groups']}, surplus {rep.surplus} / "
          f"{ref['surplus']}, covered {rep.covered} / {ref['covered']}, overlap {rep.overlap} / {ref['overlap']}")
    assert out.dtype == base_out.dtype and out.shape == base_out.shape, label
    R, Cc = cabs_oracle.view_of(base_out.shape)
    assert (rep.n, rep.rows, rep.cols, rep.n_keep, rep.group, rep.conflict_aware) == (n, R, Cc, n_keep, group, conflict_aware), label
    for f in ("groups", "kept", "short_groups", "surplus", "covered", "overlap"):
        assert getattr(rep, f) == ref[f], (label, f, getattr(rep, f), ref[f])
    mask = rep.mask.cpu()
    bad = int((mask != ref["mask"]).sum())
    assert bad == 0, f"{label}: {bad} of {n} kept masks differ"
    bad = int((raw(delta) != raw(ref["delta"])).sum())
    assert bad == 0, f"{label}: {bad} of {n} merged-delta values differ in their bits"
    bad = int((raw(out) != raw(ref["out"])).sum())
    assert bad == 0, f"{label}: {bad} of {n} output values differ in their bits"
    # the invariants, on what the engine reported
    bits = sum(((mask >> i) & 1) for i in range(k))
    assert [int(((mask >> i) & 1).sum()) for i in range(k)] == rep.kept, label
    assert rep.covered == int((bits >= 1).sum()) and rep.overlap == int((bits >= 2).sum()), label
    if conflict_aware:
        assert rep.overlap == 0 and rep.covered == sum(rep.kept) and int(bits.max()) <= 1, label
    else:
        assert sum(rep.kept) == rep.covered + int((bits - 1).clamp(min=0).sum()), label
    quota = R * int(cabs_oracle.quotas(Cc, n_keep, group).sum())
    assert rep.groups == R * ((Cc + group - 1) // group), label
    for i in range(k):
        assert rep.kept[i] - rep.surplus[i] <= quota, (label, i, rep.kept[i], rep.surplus[i], quota)
        if rep.short_groups[i] == 0:
            assert rep.kept[i] - rep.surplus[i] == quota, (label, i, rep.kept[i], rep.surplus[i], quota)
    return rep, out, delta


# ---- row lengths, the option grid, the finetune count -------------------------------------------------------------
def check_cols(engine, Cc, device="cpu"):
    """M = 64, N = 16 at a row length around the group, octet and work-group edges; several rows where that stays small"""
    for R in ((1, 2, 5) if Cc <= 1025 else (1, 3)):
        fts, bases, bo = make_inputs((R, Cc), 3, seed=R + Cc, own_bases=R == 2, device=device)
        check(engine, fts, bases, ALPHAS[:3], bo, 16, 64, label=f"{R} x {Cc}")


def check_many_rows(engine, device="cpu"):
    for Cc, M, N in ((9, 64, 16), (3, 4, 1), (20, 16, 4)):
        fts, bases, bo = make_inputs((257, Cc), 2, seed=Cc, device=device)
        check(engine, fts, bases, ALPHAS[:2], bo, N, M, label=f"257 x {Cc} {N}:{M}")


def check_ranks(engine, device="cpu"):
    """a rank-3 tensor (rows of its last dimension) and a 1-D tensor (one row)"""
    fts, bases, bo = make_inputs((4, 33, 65), 3, seed=74, own_bases=True, device=device)
    rep, _, _ = check(engine, fts, bases, ALPHAS[:3], bo, 16, 64, label="rank 3")
    assert (rep.rows, rep.cols, rep.groups) == (132, 65, 264)
    fts, bases, bo = make_inputs((2053,), 3, seed=75, device=device)
    rep, _, _ = check(engine, fts, bases, ALPHAS[:3], bo, 16, 64, label="1-D")
    assert (rep.rows, rep.cols, rep.groups) == (1, 2053, 33)


def check_options(engine, M, conflict_aware, Cc, device="cpu"):
    """every N and lambda of the grid at one group, at a row length with a tail group"""
    fts, bases, bo = make_inputs((3, Cc), 3, seed=M, own_bases=M == 16, device=device)
    for N in n_keeps(M):
        for lam in LAMBDAS:
            check(engine, fts, bases, ALPHAS[:3], bo, N, M, conflict_aware, lam, label=f"{N}:{M} ca={conflict_aware} lam={lam}")


def check_k(engine, k, own, device="cpu"):
    fts, bases, bo = make_inputs((5, 333), k, seed=20 + k, own_bases=own, device=device)
    for ca in (True, False):
        check(engine, fts, bases, ALPHAS[:k], bo, 16, 64, ca, label=f"k={k} own={own} ca={ca}")
        check(engine, fts, bases, [(-1) ** i * (0.0 if i == 1 else ALPHAS[i]) for i in range(k)], bo, 3, 8, ca, lam=0.7,
              label=f"k={k} signed and zero alphas ca={ca}")


def check_dtypes(engine, in_dtype, bo_dtype, device="cpu"):
    fts, bases, bo = make_inputs((37, 129), 3, in_dtype, bo_dtype, seed=11, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:3], bo, 16, 64, lam=0.7, label=f"{in_dtype}->{bo_dtype}")
    fts, bases, bo = make_inputs((16, 128), 2, in_dtype, bo_dtype, seed=12, device=device)      # one shared base, the 16-byte path
    check(engine, fts, bases, ALPHAS[:2], bo, 2, 8, conflict_aware=False, label=f"{in_dtype}->{bo_dtype} shared")


# ---- corners --------------------------------------------------------------------------------------------------
def check_unaligned(engine, device="cpu"):
    """views that start off a 16-byte boundary, with C % 8 == 0: the element-wise path of the loader and the stores"""
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        R, Cc = 6, 128
        n = R * Cc
        fts, bases, bo = make_inputs((n + 5,), 3, dtype, seed=71, own_bases=True, device=device)
        cut = lambda t, o: t[o:o + n].view(R, Cc)
        check(engine, [cut(fts[0], 1), cut(fts[1], 3), cut(fts[2], 0)], [cut(bases[0], 0), cut(bases[1], 1), cut(bases[2], 5)],
              ALPHAS[:3], cut(bo, 1), 16, 64, label=f"unaligned {dtype}")


def tied_inputs(shape, k, device="cpu"):
    """bf16 finetunes of a bf16 base: a delta is a small multiple of the base's ulp, so the cut value is shared by many"""
    g = torch.Generator().manual_seed(4242)
    base = (torch.randn(shape, generator=g) * 0.02).to(torch.bfloat16)
    fts = [(base.float() + torch.randn(shape, generator=g) * 3e-3 * (1 + 0.3 * i)).to(torch.bfloat16).to(device) for i in range(k)]
    base = base.to(device)
    return fts, [base] * k, base


def check_tied(engine, shape=(32, 1024), device="cpu"):
    """heavily tied deltas: a large share of the groups keeps more than its quota, so the tie rule carries the case"""
    fts, bases, bo = tied_inputs(shape, 2, device)
    for ca in (True, False):
        rep, _, _ = check(engine, fts, bases, [0.5, 0.3], bo, 64, 256, ca, label=f"tied bf16 ca={ca}")
        assert rep.surplus[0] > rep.groups // 10, (rep.surplus, rep.groups)


def check_finetune_equal_to_its_base(engine, device="cpu"):
    """no candidate anywhere: every group is short, nothing is kept, and the next finetune sees an untouched tensor"""
    fts, bases, bo = make_inputs((7, 200), 3, seed=60, device=device)
    fts[0] = bases[0].clone()
    rep, _, _ = check(engine, fts, bases, ALPHAS[:3], bo, 16, 64, label="ft0 == base")
    assert rep.kept[0] == 0 and rep.short_groups[0] == rep.groups and rep.surplus[0] == 0 and rep.kept[1] > 0
    fts = [b.clone() for b in bases]
    rep, out, delta = check(engine, fts, bases, ALPHAS[:3], bo, 16, 64, label="all == base")
    assert rep.covered == 0 and torch.equal(raw(out), raw(bo)) and not bool(delta.any())


def check_sparse_groups(engine, device="cpu"):
    """deltas that are zero in most places: groups with fewer than q non-zero entries keep all of them and are short"""
    fts, bases, bo = make_inputs((9, 260), 3, torch.float32, seed=61, own_bases=True, device=device)
    g = torch.Generator().manual_seed(7)
    for i in range(3):
        hole = (torch.rand((9, 260), generator=g) < 0.9).to(device)
        fts[i] = torch.where(hole, bases[i], fts[i])
    rep, _, _ = check(engine, fts, bases, ALPHAS[:3], bo, 16, 64, label="sparse deltas")
    assert all(0 < s for s in rep.short_groups) and all(s == 0 for s in rep.surplus)
    check(engine, fts, bases, ALPHAS[:3], bo, 2, 4, conflict_aware=False, label="sparse deltas 2:4")


def check_later_finetunes_run_short(engine, device="cpu"):
    """K N > M: the earlier finetunes use the groups up"""
    fts, bases, bo = make_inputs((4, 128), 5, torch.float32, seed=62, device=device)     # (fp32: no zero delta, no tie)
    rep, _, _ = check(engine, fts, bases, ALPHAS[:5], bo, 48, 64, label="5 x 48 > 64")
    G = rep.groups
    assert rep.short_groups == [0, G, G, G, G] and rep.kept == [48 * G, 16 * G, 0, 0, 0]
    rep, _, _ = check(engine, fts, bases, ALPHAS[:5], bo, 7, 8, label="5 x 7 > 8")
    G = rep.groups
    assert rep.short_groups == [0, G, G, G, G] and rep.kept == [7 * G, G, 0, 0, 0]


def check_nonfinite(engine, device="cpu"):
    """a NaN / an Inf in a finetune or in a base: ValueError naming the tensor and the finetunes; the context stays usable"""
    name = "model.layers.7.mlp.up_proj.weight"
    for k, M, poison in ((3, 64, float("inf")), (5, 64, float("nan")), (3, 8, float("-inf"))):
        fts, bases, bo = make_inputs((37, 129), k, seed=80, device=device)
        fts[1] = fts[1].clone()
        fts[1].view(-1)[4321] = poison
        with pytest.raises(ValueError, match=rf"model\.layers\.7\.mlp\.up_proj\.weight.*finetune 1\b"):
            engine.cabs_merge(fts, bases, ALPHAS[:k], bo, n_keep=M // 4, group=M, layer_name=name)
        fts, bases, bo = make_inputs((37, 129), k, seed=81, own_bases=True, device=device)
        bases[2] = bases[2].clone()
        bases[2].view(-1)[17] = poison
        with pytest.raises(ValueError, match=rf"model\.layers\.7\.mlp\.up_proj\.weight.*finetune 2\b"):
            engine.cabs_merge(fts, bases, ALPHAS[:k], bo, n_keep=M // 4, group=M, layer_name=name)
        fts, bases, bo = make_inputs((37, 129), k, seed=82, device=device)
        bases = [bases[0].clone()] * k                                # the shared base: every finetune is named
        bases[0].view(-1)[5] = poison
        with pytest.raises(ValueError, match=r"finetune 0, 1, 2"):
            engine.cabs_merge(fts, bases, ALPHAS[:k], bo, n_keep=M // 4, group=M, layer_name=name)
        fts, bases, bo = make_inputs((37, 129), k, seed=83, device=device)
        check(engine, fts, bases, ALPHAS[:k], bo, M // 4, M, label="after an error")


def check_empty(engine, device="cpu"):
    fts, bases, bo = make_inputs((0,), 2, seed=73, device=device)
    out, rep = engine.cabs_merge(fts, bases, [0.5, 0.5], bo, n_keep=16, group=64, want_mask=True)
    assert out.numel() == 0 and out.dtype == bo.dtype and rep.mask.numel() == 0
    assert (rep.groups, rep.kept, rep.short_groups, rep.surplus, rep.covered, rep.overlap) == (0, [0, 0], [0, 0], [0, 0], 0, 0)
    fts, bases, bo = make_inputs((3, 0), 2, seed=73, device=device)
    assert engine.cabs_merge(fts, bases, [0.5, 0.5], bo, n_keep=16, group=64)[0].shape == (3, 0)


def check_determinism(engine, device="cpu"):
    fts, bases, bo = make_inputs((30, 500), 3, seed=90, own_bases=True, device=device)
    a, ra = engine.cabs_merge(fts, bases, ALPHAS[:3], bo, n_keep=16, group=64)
    b, rb = engine.cabs_merge(fts, bases, ALPHAS[:3], bo, n_keep=16, group=64)
    assert torch.equal(raw(a), raw(b)) and ra == rb


# ---- the identities, bit for bit through the same engine ------------------------------------------------------------
def check_full_quota_is_dare_linear(engine, device="cpu"):
    """conflict_aware 0 with N == M keeps every non-zero entry: dare_linear at density 1 without normalisation"""
    for k, own, lam, M in ((3, True, 0.7, 64), (5, False, 1.0, 8), (1, False, 1.0, 4), (16, True, -0.5, 512)):
        fts, bases, bo = make_inputs((37, 129), k, seed=100 + k, own_bases=own, device=device)
        out, rep, delta = engine.cabs_merge(fts, bases, ALPHAS[:k], bo, n_keep=M, group=M, conflict_aware=False, lam=lam, want_delta=True)
        d_out, _, d_delta = engine.dare_merge(fts, bases, ALPHAS[:k], bo, density=1.0, lam=lam, normalize=False, sign_election=False,
                                              want_delta=True)
        assert torch.equal(raw(out), raw(d_out)) and torch.equal(raw(delta), raw(d_delta)), k
        assert rep.surplus == [0] * k


def check_one_group_is_breadcrumbs(engine, device="cpu"):
    """R = 1, C = M = 512, N = 128, conflict_aware 0: the group is the tensor and the cut is breadcrumbs' at gamma 0,
    density 0.25 (floor(0.25 * 512) = 128 exactly), without normalisation"""
    for k, own, lam in ((1, False, 1.0), (3, True, 0.7), (5, False, -0.5)):
        fts, bases, bo = make_inputs((512,), k, seed=120 + k, own_bases=own, device=device)
        out, rep, delta = engine.cabs_merge(fts, bases, ALPHAS[:k], bo, n_keep=128, group=512, conflict_aware=False, lam=lam, want_delta=True)
        b_out, b_rep, b_delta = engine.breadcrumbs_merge(fts, bases, ALPHAS[:k], bo, density=0.25, gamma=0.0, lam=lam, normalize=False,
                                                         sign_election=False, want_delta=True)
        assert torch.equal(raw(out), raw(b_out)) and torch.equal(raw(delta), raw(b_delta)), k
        assert rep.kept == b_rep.kept


def check_k1_ignores_conflict_aware(engine, device="cpu"):
    fts, bases, bo = make_inputs((37, 129), 1, seed=130, device=device)
    a, ra, da = engine.cabs_merge(fts, bases, [0.5], bo, n_keep=16, group=64, conflict_aware=True, want_delta=True)
    b, rb, db = engine.cabs_merge(fts, bases, [0.5], bo, n_keep=16, group=64, conflict_aware=False, want_delta=True)
    assert torch.equal(raw(a), raw(b)) and torch.equal(raw(da), raw(db)) and ra.kept == rb.kept


def check_first_entry_alone(engine, device="cpu"):
    """alphas (1, 0, ..., 0): the output depends neither on conflict_aware nor on the other finetunes' tensors"""
    fts, bases, bo = make_inputs((37, 129), 4, seed=131, device=device)
    other, _, _ = make_inputs((37, 129), 4, seed=132, device=device)
    alone = engine.cabs_merge(fts[:1], bases[:1], [1.0], bo, n_keep=16, group=64)[0]
    for ca in (True, False):
        for rest in (fts[1:], other[1:]):
            out = engine.cabs_merge([fts[0]] + list(rest), bases, [1.0, 0.0, 0.0, 0.0], bo, n_keep=16, group=64, conflict_aware=ca)[0]
            assert torch.equal(raw(out), raw(alone)), ca


def check_kept_set_grows_with_n(engine, device="cpu"):
    fts, bases, bo = make_inputs((9, 300), 3, seed=133, device=device)
    masks = []
    for N in (1, 2, 16, 17, 63, 64):
        _, rep = engine.cabs_merge(fts, bases, ALPHAS[:3], bo, n_keep=N, group=64, want_mask=True)
        masks.append(rep.mask.cpu() & 1)
    for lo, hi in zip(masks, masks[1:]):
        assert bool(((lo & hi) == lo).all()) and int(hi.sum()) > int(lo.sum())


def check_arguments(engine, device="cpu"):
    fts, bases, bo = make_inputs((8, 8), 2, seed=91, device=device)
    for bad in (0, 2, 3, 6, 48, 1024, 64.0, True, "64"):
        with pytest.raises(ValueError, match="group"):
            engine.cabs_merge(fts, bases, [0.5, 0.5], bo, n_keep=1, group=bad)
    for bad in (0, -1, 65, 2.0, True):
        with pytest.raises(ValueError, match="n_keep"):
            engine.cabs_merge(fts, bases, [0.5, 0.5], bo, n_keep=bad, group=64)
    with pytest.raises(ValueError, match="lam"):
        engine.cabs_merge(fts, bases, [0.5, 0.5], bo, n_keep=1, group=4, lam=float("inf"))
    with pytest.raises(ValueError, match="shape mismatch"):
        engine.cabs_merge([fts[0], fts[1][:4]], bases, [0.5, 0.5], bo, n_keep=1, group=4)
    with pytest.raises(ValueError, match="supported range"):
        engine.cabs_merge([fts[0]] * 17, [bases[0]] * 17, [0.1] * 17, bo, n_keep=1, group=4)
    with pytest.raises(ValueError, match="alphas"):
        engine.cabs_merge(fts, bases, [0.5], bo, n_keep=1, group=4)


CORNERS = [check_many_rows, check_ranks, check_unaligned, check_tied, check_finetune_equal_to_its_base, check_sparse_groups,
           check_later_finetunes_run_short, check_nonfinite, check_empty, check_determinism, check_full_quota_is_dare_linear,
           check_one_group_is_breadcrumbs, check_k1_ignores_conflict_aware, check_first_entry_alone, check_kept_set_grows_with_n,
           check_arguments]


# ---- the paper's form, in torch, independent of the oracle ---------------------------------------------------------
PAPER_CASES = [((512, 1024), 2, 64, 256), ((300, 4544), 3, 128, 512), ((1024, 4096), 3, 16, 64)]
PAPER_CAP = 1e-3                                # groups left out at most: those where the cut value is not unique


def paper_inputs(shape, k, device="cpu"):
    """fp32 Gaussian bases of sigma 0.02, fp32 deltas of sigma 3e-3 (1 + 0.3 i)"""
    g = torch.Generator().manual_seed(99)
    base = (torch.randn(shape, generator=g) * 0.02).to(device)
    fts = [(base.cpu() + torch.randn(shape, generator=g) * (3e-3 * (1 + 0.3 * i))).to(device) for i in range(k)]
    return fts, [base] * k, base


def paper_form(fts, bases, alphas, base_out, N, M, lam):
    """For the finetunes in turn: |d| with what is taken masked out, reshaped to groups, torch.topk(n), scattered; then
    the weighted sum in fp32.  -> (out, delta, ambiguous [R, G]: groups where the cut value occurs more than once among
    a finetune's candidates, so that topk's choice is arbitrary)"""
    R, Cc = base_out.shape
    G = (Cc + M - 1) // M
    taken = torch.zeros((R, Cc), dtype=torch.bool, device=base_out.device)
    ambiguous = torch.zeros((R, G), dtype=torch.bool, device=base_out.device)
    Msum = torch.zeros((R, Cc), dtype=torch.float32, device=base_out.device)
    for ft, bs, alpha in zip(fts, bases, alphas):
        d = ft.float() - bs.float()
        mag = torch.where(taken, torch.full_like(d, -1.0), d.abs())
        kept = torch.zeros_like(taken)
        full = (Cc // M) * M
        for c0, c1, m in ((0, full, M), (full, Cc, Cc - full)):          # the full groups, then the tail group
            if c1 == c0:
                continue
            q = (N * m + M - 1) // M
            grp = mag[:, c0:c1].reshape(R, -1, m)
            vals, idx = torch.topk(grp, q, dim=2)
            sel = torch.zeros_like(grp, dtype=torch.bool).scatter_(2, idx, torch.ones_like(idx, dtype=torch.bool)) & (grp > 0)
            kept[:, c0:c1] = sel.reshape(R, c1 - c0)
            cut = vals[:, :, -1:]
            ambiguous[:, c0 // M:c0 // M + grp.shape[1]] |= (grp == cut).sum(dim=2) > 1
        Msum = Msum + torch.where(kept, d * torch.tensor(float(alpha), dtype=torch.float32, device=d.device), torch.zeros_like(d))
        taken |= kept
    delta = torch.tensor(float(lam), dtype=torch.float32, device=Msum.device) * Msum
    return (base_out.float() + delta).to(base_out.dtype), delta, ambiguous


def check_paper_form(engine, shape, k, N, M, device="cpu"):
    fts, bases, bo = paper_inputs(shape, k, device)
    out, rep, delta = engine.cabs_merge(fts, bases, ALPHAS[:k], bo, n_keep=N, group=M, conflict_aware=True, lam=0.7, want_delta=True)
    p_out, p_delta, ambiguous = paper_form(fts, bases, ALPHAS[:k], bo, N, M, 0.7)
    R, Cc = shape
    left_out = int(ambiguous.sum())
    print(f"paper form {shape} k={k} {N}:{M}: {left_out} of {ambiguous.numel()} groups left out (cut value not unique)")
    assert ambiguous.numel() == rep.groups
    assert left_out <= PAPER_CAP * ambiguous.numel(), (left_out, ambiguous.numel())
    use = (~ambiguous).repeat_interleave(M, dim=1)[:, :Cc].cpu()
    assert torch.equal(raw(delta)[use], raw(p_delta)[use])
    assert torch.equal(raw(out)[use], raw(p_out)[use])
    assert rep.overlap == 0


# ---- profile names --------------------------------------------------------------------------------------------------
PROFILES = [(2, {"cabs_merge": 1}), (4, {"cabs_merge": 1}), (5, {"cabs_merge_any": 1}), (16, {"cabs_merge_any": 1})]


def check_profile(engine, k, expected, device="cpu"):
    """one fused launch, whatever the group: no histogram launch, no select"""
    for M in (4, 64):
        fts, bases, bo = make_inputs((40, 50), k, seed=6, device=device)
        got = profile_of(engine, lambda: engine.cabs_merge(fts, bases, ALPHAS[:k], bo, n_keep=M // 4, group=M))
        assert got == expected, got


# ---- the C ABI --------------------------------------------------------------------------------------------------------
def check_c_abi(engine, device="cpu"):
    from shardmerge_amd import _lib
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(64, generator=g) + 2).to(torch.bfloat16).to(device)
    y = torch.zeros(64, dtype=torch.bfloat16, device=device)
    out = torch.zeros(64, dtype=torch.bfloat16, device=device)
    mask = torch.zeros(64, dtype=torch.int16, device=device)
    dll, h = engine.lib.dll, engine.ctx.h

    def call(k=1, n_keep=2, group=8, ca=1, out_t=out, mask_t=None, n=64, rows=4, in_dtype=_lib.BF16, lam=1.0, alpha=0.5):
        d = _lib.CabsDesc()
        d.k = k
        for i in range(max(0, min(k, 16))):
            d.finetune[i], d.base[i], d.alpha[i] = x.data_ptr(), y.data_ptr(), alpha
        d.in_dtype, d.base_out, d.base_out_dtype, d.n, d.rows = in_dtype, y.data_ptr(), _lib.BF16, n, rows
        d.n_keep, d.group, d.conflict_aware, d.lam = n_keep, group, ca, lam
        rep = _lib.CabsReport()
        rc = dll.smhip_cabs_merge(h, C.byref(d), out_t.data_ptr(), None, mask_t.data_ptr() if mask_t is not None else None,
                                  C.byref(rep), None)
        return rc, dll.smhip_last_error(h).decode(), rep

    rc, msg, rep = call(mask_t=mask)
    assert rc == _lib.OK and rep.groups == 8 and rep.kept[0] >= 16 and rep.covered == rep.kept[0] and rep.overlap == 0, msg
    assert int((mask.cpu() != 0).sum()) == rep.kept[0]
    rc, msg, rep = call(k=2, ca=0, n_keep=8)
    assert rc == _lib.OK and rep.kept[0] == rep.kept[1] == 64 and rep.overlap == 64, msg
    for kwargs, word in (({"k": 0}, "k out of range"), ({"k": 17}, "k out of range"), ({"group": 2}, "group"), ({"group": 48}, "group"),
                         ({"group": 1024}, "group"), ({"group": 0}, "group"), ({"group": -8}, "group"), ({"n_keep": 0}, "n_keep"),
                         ({"n_keep": 9}, "n_keep"), ({"ca": 2}, "conflict_aware"), ({"ca": -1}, "conflict_aware"),
                         ({"lam": float("inf")}, "lambda"), ({"lam": float("nan")}, "lambda"), ({"alpha": float("nan")}, "alpha"),
                         ({"out_t": x}, "overlaps"), ({"in_dtype": 3}, "dtype"), ({"rows": 0}, "rows"), ({"rows": 5}, "rows"),
                         ({"mask_t": out}, "mask_out"), ({"mask_t": x}, "mask_out")):
        rc, msg, _ = call(**kwargs)
        assert rc == _lib.ERR_ARG and word in msg, (kwargs, rc, msg)
    rc = dll.smhip_cabs_merge(h, None, out.data_ptr(), None, None, None, None)
    assert rc == _lib.ERR_ARG and "null descriptor" in dll.smhip_last_error(h).decode()
    assert call(n=0, out_t=x)[0] == _lib.OK                     # a no-op, whatever the pointers


# ---- the CLI on the synthetic on-disk model of tests/lora_fixtures.py ----------------------------------------
def write_config(root, third, out_dir, opts, device=None):
    return harness.write_config(root, ties_models(third), out_dir, opts, device)


def expected_outputs(base, full, opts, models=None):
    """the oracle tensor by tensor (block tensors) / the provider's tensor (passthrough); the models of ties_models:
    layer 0 has three entries, layer 1 two, in the order of finetune_merge"""
    def merge(fts, bases, alphas, base_out, name):
        return cabs_oracle.cabs_merge(fts, bases, alphas, base_out, int(opts.get("cabs_n", 64)), int(opts.get("cabs_m", 256)),
                                      bool(opts.get("cabs_conflict_aware", 1)), opts.get("cabs_lambda", 1.0))["out"]

    return expected_by_tensor(base, full, models or ties_models("org/lora_full"), merge)
