"""Checks of EMR-Merging shared by the emulator tier (tests/test_emr_host.py) and the GPU tier (tests/test_emr_gpu.py):
Engine.emr_merge, Engine.emr_mask and Engine.emr_apply against tests/emr_oracle.py, BIT FOR BIT - output, merged delta,
every counter, the mask plane, all seven sums, the rescaler, the residual, the applied tensor.  The tolerance is zero and
it is derived, not measured: every step of the three functions is one correctly rounded operation, a comparison or an
integer count (include/shardmerge_hip.h, smhip_emr_merge / smhip_emr_mask / smhip_emr_apply).  Then the identities with
the existing operators through the same engine, the paper's form in torch fp64 (independent of the oracle), and the
command and the pack on the on-disk model of tests/lora_fixtures.py."""
import asyncio
import ctypes as C
import json
import math

import pytest
import torch

from tests import emr_oracle as eo
from tests import harness
from tests.dpack_oracle import unpack_bits
from tests.harness import DTYPES, KS, SMALL, f32_bits, f64_bits, make_inputs, profile_of, raw

SIZES = (0, 1, 7, 8, 9, 2047, 2048, 2049, 2 ** 16 + 5)    # around one octet, around one work-group of 256 octets, several
LAMBDAS = (1.0, 0.5, -1.0)
COLS = (1, 7, 8, 9, 2047, 2048, 2056, 4104)                # a row's lanes wrap at 2048 elements
ROWS = (1, 2, 3, 257)
MERGE_FIELDS = ("n", "elected_pos", "elected_neg", "zero", "contested", "winner", "agree")
MASK_INTS = ("rows", "cols", "c", "nonzero")
MASK_SUMS = ("A", "B", "D2", "X", "U2", "delta_sq", "resid_sq")


def cpu(ts):
    return [t.cpu() for t in ts]


# ---- one call against the oracle ---------------------------------------------------------------------------------------
def check(engine, fts, bases, base_out, lam=1.0, label=""):
    """emr_merge against the oracle, bit for bit, and the invariants of the report; returns (report, out, delta, ref)"""
    out, rep, delta = engine.emr_merge(fts, bases, base_out, lam=lam, want_delta=True, layer_name=label or "layer")
    ref = eo.emr_merge(cpu(fts), cpu(bases), base_out.cpu(), lam=lam)
    n = base_out.numel()
    print(f"{label}: {rep} / contested {ref['contested']}")
    assert out.dtype == base_out.dtype and out.shape == base_out.shape and delta.dtype == torch.float32, label
    for f in MERGE_FIELDS:
        assert getattr(rep, f) == ref[f], (label, f, getattr(rep, f), ref[f])
    assert sum(rep.winner) + rep.zero == n and rep.elected_pos + rep.elected_neg + rep.zero == n, (label, rep)
    assert all(w <= a for w, a in zip(rep.winner, rep.agree)), (label, rep)
    bad = int((raw(delta) != raw(ref["delta"])).sum())
    assert bad == 0, f"{label}: {bad} of {n} merged-delta values differ in their bits"
    bad = int((raw(out) != raw(ref["out"])).sum())
    assert bad == 0, f"{label}: {bad} of {n} output values differ in their bits"
    return rep, out, delta, ref


def check_mask(engine, ft, base, uni, label=""):
    """emr_mask and emr_apply against the oracle, bit for bit; returns (mask, scale, report, applied)"""
    mask, scale, rep = engine.emr_mask(ft, base, uni, name=label or "tensor")
    ref = eo.emr_mask(ft.cpu(), base.cpu(), uni.cpu())
    print(f"{label}: {rep}")
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == tuple(ref.mask.shape) and tuple(scale.shape) == (1,), label
    bad = int((mask.cpu() != ref.mask).sum())
    assert bad == 0, f"{label}: {bad} of {mask.numel()} plane bytes differ"
    for f in MASK_INTS:
        assert getattr(rep, f) == getattr(ref, f), (label, f, getattr(rep, f), getattr(ref, f))
    for f in MASK_SUMS:
        assert f64_bits(getattr(rep, f)) == f64_bits(getattr(ref, f)), (label, f, getattr(rep, f), getattr(ref, f))
    assert f32_bits(rep.lam) == f32_bits(ref.lam) and torch.equal(raw(scale), raw(ref.scale)), (label, rep.lam, ref.lam)
    got = engine.emr_apply(base, uni, mask, scale)
    want = eo.emr_apply(base.cpu(), uni.cpu(), ref.mask, ref.scale)
    assert got.dtype == base.dtype and got.shape == base.shape, label
    bad = int((raw(got) != raw(want)).sum())
    assert bad == 0, f"{label}: {bad} of {base.numel()} applied values differ in their bits"
    return mask, scale, rep, got


def triple(shape, dtype=torch.bfloat16, seed=0, device="cpu"):
    """(finetune, base, unified): the unified model is the oracle's merge of the finetune and a second one"""
    fts, bases, bo = make_inputs(shape, 2, dtype, seed=seed, device=device)
    uni = eo.emr_merge(cpu(fts), cpu(bases), bo.cpu())["out"].to(device)
    return fts[0], bases[0], uni


# ---- emr_merge: the parameter grid -----------------------------------------------------------------------------------------
def check_k(engine, k, own, lam, device="cpu"):
    fts, bases, bo = make_inputs(SMALL, k, seed=20 + k, own_bases=own, device=device)
    check(engine, fts, bases, bo, lam=lam, label=f"k={k} own={own} lam={lam}")


def check_size(engine, n, device="cpu"):
    for k in (2, 5):
        fts, bases, bo = make_inputs((n,), k, seed=70 + k, own_bases=k == 5, device=device)
        rep, out, _, _ = check(engine, fts, bases, bo, label=f"n={n} k={k}")
        assert rep.n == n and out.numel() == n


def check_dtypes(engine, in_dtype, bo_dtype, device="cpu"):
    fts, bases, bo = make_inputs(SMALL, 3, in_dtype, bo_dtype, seed=11, own_bases=True, device=device)
    check(engine, fts, bases, bo, lam=0.5, label=f"{in_dtype}->{bo_dtype}")
    fts, bases, bo = make_inputs(SMALL, 2, in_dtype, bo_dtype, seed=12, device=device)      # one shared base
    check(engine, fts, bases, bo, label=f"{in_dtype}->{bo_dtype} shared")


def check_unaligned(engine, device="cpu"):
    """views that start one element (and more) off a 16-byte boundary: the element-wise path of the loader and the store"""
    for dtype in DTYPES:
        for n in (1003, 2048):
            fts, bases, bo = make_inputs((n + 5,), 3, dtype, seed=71, own_bases=True, device=device)
            cut = lambda t, o: t[o:o + n]
            check(engine, [cut(fts[0], 1), cut(fts[1], 3), cut(fts[2], 0)], [cut(bases[0], 0), cut(bases[1], 1), cut(bases[2], 5)],
                  cut(bo, 1), label=f"unaligned {dtype} n={n}")
            fts, bases, bo = make_inputs((n + 5,), 2, dtype, seed=72, device=device)       # a shared base that is base_out, off by one
            check(engine, [cut(fts[0], 1), cut(fts[1], 1)], [cut(bases[0], 1)] * 2, cut(bases[0], 1), label=f"unaligned shared {dtype} n={n}")


def tied_inputs(k, shape=SMALL, seed=0, device="cpu"):
    """bf16 deltas that are small multiples of an ulp: bases in [1.25, 1.75) (one binade, ulp 2^-7), deltas j ulp, |j| <= 2"""
    g = torch.Generator().manual_seed(3000 + seed)
    base = (1.25 + 0.5 * torch.rand(shape, generator=g)).to(torch.bfloat16)
    fts = [(base.float() + torch.randint(-2, 3, shape, generator=g).float() * 2.0 ** -7).to(torch.bfloat16) for _ in range(k)]
    return [f.to(device) for f in fts], [base.to(device)] * k, base.to(device)


def check_heavy_ties(engine, device="cpu"):
    """S == 0 with non-zero entries occurs and elects plus; equal magnitudes go to the first entry"""
    for k in (2, 3, 5, 16):
        fts, bases, bo = tied_inputs(k, seed=k, device=device)
        rep, _, delta, ref = check(engine, fts, bases, bo, label=f"heavy ties k={k}")
        zero_sum = (ref["S"] == 0) & (sum((d != 0) for d in ref["d"]) > 0)
        assert int(zero_sum.sum()) > 0, "the inputs hold no zero sum with non-zero entries"
        assert bool((delta.cpu().reshape(-1).numpy()[zero_sum] > 0).all())             # a zero sum elects plus
        assert rep.winner[0] > rep.winner[-1]                                          # the first of equal magnitudes wins


def check_equal_finetunes(engine, device="cpu"):
    """a finetune equal to its base never wins or agrees; all finetunes equal to their bases: the output is base_out"""
    fts, bases, bo = make_inputs(SMALL, 3, seed=60, device=device)
    fts[1] = bases[1].clone()
    rep, _, _, _ = check(engine, fts, bases, bo, label="one finetune is its base")
    assert rep.winner[1] == 0 and rep.agree[1] == 0
    fts = [b.clone() for b in bases]
    rep, out, delta, _ = check(engine, fts, bases, bo, label="zero deltas")
    n = bo.numel()
    assert rep.zero == n and rep.contested == 0 and rep.winner == [0] * 3 and rep.agree == [0] * 3
    assert torch.equal(raw(out), raw(bo)) and not bool(delta.any()) and not bool(torch.signbit(delta).any())


def check_denormals(engine, device="cpu"):
    g = torch.Generator().manual_seed(66)
    ft = (torch.randn(SMALL, generator=g) * 1e-40).to(device)
    assert 0 < float(ft.abs().max()) < 1.2e-38
    zero = torch.zeros_like(ft)
    check(engine, [ft, ft * 0.5, -ft], [zero] * 3, zero, lam=0.5, label="fp32 denormal deltas")


def check_nonfinite(engine, device="cpu"):
    """a NaN / an Inf in a finetune or in a base: ValueError naming the tensor and the finetune; the context stays usable"""
    name = "model.layers.7.mlp.up_proj.weight"
    for k, poison, in_base in ((3, float("inf"), False), (5, float("nan"), False), (3, float("-inf"), True), (2, float("nan"), True)):
        fts, bases, bo = make_inputs(SMALL, k, seed=80, own_bases=True, device=device)
        target = bases if in_base else fts
        target[1] = target[1].clone()
        target[1].view(-1)[4321] = poison
        with pytest.raises(ValueError, match=r"model\.layers\.7\.mlp\.up_proj\.weight.*finetune 1\b"):
            engine.emr_merge(fts, bases, bo, layer_name=name)
        fts, bases, bo = make_inputs(SMALL, k, seed=81, device=device)
        check(engine, fts, bases, bo, label="after an error")
    # finite deltas whose fp32 sum overflows
    big = torch.full((64,), 3e38, dtype=torch.float32, device=device)
    zero = torch.zeros_like(big)
    with pytest.raises(ValueError, match=rf"{name}.*sum"):
        engine.emr_merge([big, big], [zero, zero], zero, layer_name=name)


def check_rank3_and_determinism(engine, device="cpu"):
    fts, bases, bo = make_inputs((4, 33, 65), 3, seed=74, own_bases=True, device=device)
    check(engine, fts, bases, bo, label="rank 3")
    fts, bases, bo = make_inputs((300, 500), 3, seed=90, own_bases=True, device=device)
    a, ra = engine.emr_merge(fts, bases, bo)
    b, rb = engine.emr_merge(fts, bases, bo)
    assert torch.equal(raw(a), raw(b)) and ra == rb


def check_arguments(engine, device="cpu"):
    fts, bases, bo = make_inputs((8, 8), 2, seed=91, device=device)
    for bad in (float("inf"), float("nan"), "1", True, None):
        with pytest.raises(ValueError, match="lam"):
            engine.emr_merge(fts, bases, bo, lam=bad)
    with pytest.raises(ValueError, match="shape mismatch"):
        engine.emr_merge([fts[0], fts[1][:4]], bases, bo)
    with pytest.raises(ValueError, match="supported range"):
        engine.emr_merge([fts[0]] * 17, [bases[0]] * 17, bo)
    with pytest.raises(ValueError, match="bases"):
        engine.emr_merge(fts, bases[:1], bo)
    ft, base, uni = triple((8, 8), seed=92, device=device)
    with pytest.raises(ValueError, match="emr_mask: shape mismatch in T"):
        engine.emr_mask(ft, base, uni[:4], name="T")
    mask, scale, _ = engine.emr_mask(ft, base, uni)
    for kwargs, word in ((dict(mask=mask[:4]), "mask"), (dict(mask=mask.to(torch.int8)), "mask"), (dict(scale=torch.zeros(2)), "scale"),
                         (dict(scale=scale.double()), "scale"), (dict(unified=uni.float()), "unified"), (dict(unified=uni[:4]), "unified"),
                         (dict(base=base.to(torch.int32), unified=uni.to(torch.int32)), "base")):
        args = dict(base=base, unified=uni, mask=mask, scale=scale)
        args.update(kwargs)
        with pytest.raises(ValueError, match=f"emr_apply: {word}"):
            engine.emr_apply(args["base"], args["unified"], args["mask"], args["scale"])


# ---- the identities and properties through the engine ----------------------------------------------------------------------
def check_k1_is_dare_linear(engine, device="cpu"):
    """one entry: the delta itself - dare_linear at density 1 with alpha 1 and the same lambda"""
    for own, lam, dtype in ((False, 1.0, torch.bfloat16), (True, 0.5, torch.float16), (True, -1.0, torch.float32)):
        fts, bases, bo = make_inputs(SMALL, 1, dtype, seed=100, own_bases=own, device=device)
        out, rep, delta = engine.emr_merge(fts, bases, bo, lam=lam, want_delta=True)
        d_out, _, d_delta = engine.dare_merge(fts, bases, [1.0], bo, density=1.0, lam=lam, normalize=True, sign_election=False, want_delta=True)
        assert torch.equal(raw(out), raw(d_out)) and torch.equal(raw(delta), raw(d_delta)), (own, lam)
        assert rep.contested == 0 and rep.winner == rep.agree


def check_swap_and_copies(engine, device="cpu"):
    """k = 2 with the entries swapped gives the same bytes; three copies of one finetune give the k = 1 output"""
    for own in (False, True):
        fts, bases, bo = make_inputs(SMALL, 2, seed=101, own_bases=own, device=device)
        a, ra, da = engine.emr_merge(fts, bases, bo, want_delta=True)
        b, rb, db = engine.emr_merge(fts[::-1], bases[::-1], bo, want_delta=True)
        assert torch.equal(raw(a), raw(b)) and torch.equal(raw(da), raw(db))
        assert (ra.elected_pos, ra.elected_neg, ra.zero, ra.contested, ra.agree) == (rb.elected_pos, rb.elected_neg, rb.zero, rb.contested, rb.agree[::-1])
    fts, bases, bo = tied_inputs(2, seed=7, device=device)                         # with equal magnitudes and zero sums too
    a = engine.emr_merge(fts, bases, bo)[0]
    b = engine.emr_merge(fts[::-1], bases, bo)[0]
    assert torch.equal(raw(a), raw(b))
    fts, bases, bo = make_inputs(SMALL, 1, seed=102, own_bases=True, device=device)
    one, r1 = engine.emr_merge(fts, bases, bo, lam=0.5)
    three, r3 = engine.emr_merge(fts * 3, bases * 3, bo, lam=0.5)
    assert torch.equal(raw(one), raw(three)) and r3.winner == [r1.winner[0], 0, 0] and r3.agree == r1.agree * 3


def check_elements_of_the_inputs(engine, device="cpu"):
    """lambda 1, a shared base that is base_out: every element of delta_out is +0 or some d_i, every element of out is an
    element of a finetune or of the base, and fp32(out) - fp32(base) gives delta_out back - bit for bit, everywhere.
    (The seed is one at which no input holds a negative zero: a finetune's -0 that is elected comes out as base + (-0 - base)
    = +0, equal in value and not in its bits; seed 203 holds one such fp16 element in 524288 at k = 3.)"""
    for dtype in DTYPES:
        for k in (2, 3, 5):
            fts, bases, bo = make_inputs((512, 1024), k, dtype, seed=201)            # drawn on the CPU: the same inputs on both tiers
            assert not any(bool(((t == 0) & torch.signbit(t)).any()) for t in fts + [bo])
            fts, bo = [f.to(device) for f in fts], bo.to(device)
            bases = [bo] * k
            out, rep, delta = engine.emr_merge(fts, bases, bo, want_delta=True)
            d = torch.stack([f.float() - bo.float() for f in fts])
            zero = raw(delta) == 0
            is_entry = (raw(delta).unsqueeze(0) == raw(d)).any(0)
            assert bool((zero | is_entry).all()), (dtype, k)
            assert not bool(torch.signbit(delta[delta == 0]).any())
            of_inputs = (raw(out).unsqueeze(0) == torch.stack([raw(f) for f in fts] + [raw(bo)])).any(0)
            assert bool(of_inputs.all()), (dtype, k, int((~of_inputs).sum()))
            assert torch.equal(raw(out.float() - bo.float()), raw(delta)), (dtype, k)


def check_mask_counts_agree(engine, device="cpu"):
    """the two kernels on the same inputs: emr_mask(f_i, base, out).c == agree[i] of the emr_merge report"""
    for dtype in DTYPES:
        for k in (2, 3, 5):
            fts, bases, bo = make_inputs(SMALL, k, dtype, seed=300 + k, device=device)
            out, rep = engine.emr_merge(fts, bases, bo)
            for i in range(k):
                _, _, mr = engine.emr_mask(fts[i], bo, out)
                assert mr.c == rep.agree[i], (dtype, k, i, mr.c, rep.agree)


def check_k1_round_trip(engine, device="cpu"):
    """one entry: the unified model is the finetune, lambda is exactly 1, the residual 0, apply returns the finetune"""
    for dtype in DTYPES:
        fts, bases, bo = make_inputs(SMALL, 1, dtype, seed=400, device=device)
        out, _ = engine.emr_merge(fts, bases, bo)
        assert torch.equal(raw(out), raw(fts[0]))
        mask, scale, rep, got = check_mask(engine, fts[0], bo, out, label=f"round trip {dtype}")
        assert f32_bits(rep.lam) == f32_bits(1.0) and rep.resid_sq == 0.0 and rep.c == rep.nonzero
        assert torch.equal(raw(got), raw(fts[0]))


MERGE_CORNERS = [check_unaligned, check_heavy_ties, check_equal_finetunes, check_denormals, check_nonfinite, check_rank3_and_determinism,
                 check_arguments, check_k1_is_dare_linear, check_swap_and_copies, check_elements_of_the_inputs, check_mask_counts_agree,
                 check_k1_round_trip]


# ---- emr_mask / emr_apply -----------------------------------------------------------------------------------------------------
def check_cols(engine, cols, device="cpu"):
    for rows in (1, 3):
        ft, base, uni = triple((rows, cols), seed=cols % 89, device=device)
        check_mask(engine, ft, base, uni, label=f"{rows} x {cols}")


def check_rows(engine, rows, device="cpu"):
    for cols in (9, 136):
        ft, base, uni = triple((rows, cols), seed=rows % 89, device=device)
        check_mask(engine, ft, base, uni, label=f"{rows} x {cols}")


def check_mask_dtypes(engine, dtype, device="cpu"):
    ft, base, uni = triple(SMALL, dtype, seed=13, device=device)
    check_mask(engine, ft, base, uni, label=f"{dtype}")
    ft, base, uni = triple((16, 256), dtype, seed=14, device=device)                 # every octet a 16-byte access
    check_mask(engine, ft, base, uni, label=f"{dtype} aligned")


def check_mask_ranks(engine, device="cpu"):
    for shape in ((4, 33, 65), (1003,), (2048,), ()):
        ft, base, uni = triple(shape, seed=15 + len(shape), device=device)
        mask, _, rep, _ = check_mask(engine, ft, base, uni, label=f"shape {shape}")
        if len(shape) <= 1:
            assert rep.rows == 1 and mask.shape[0] == 1


def check_mask_offset_views(engine, device="cpu"):
    for dtype in DTYPES:
        for rows, cols in ((5, 200), (3, 131)):
            n = rows * cols
            ft, base, uni = triple((n + 5,), dtype, seed=16, device=device)
            cut = lambda t, o: t[o:o + n].reshape(rows, cols)
            check_mask(engine, cut(ft, 1), cut(base, 3), cut(uni, 0), label=f"offset views {dtype} {rows} x {cols}")


def check_mask_degenerate(engine, device="cpu"):
    """the unified model equal to the base: B == 0, lambda +0, an empty mask, apply returns the base; the model equal to the
    unified model: lambda exactly 1 and a zero residual"""
    ft, base, _ = triple(SMALL, seed=17, device=device)
    mask, scale, rep, got = check_mask(engine, ft, base, base.clone(), label="unified == base")
    assert rep.B == 0.0 and rep.c == 0 and f32_bits(rep.lam) == f32_bits(0.0) and not bool(mask.any())
    assert rep.resid_sq == rep.delta_sq > 0 and torch.equal(raw(got), raw(base))
    mask, scale, rep, got = check_mask(engine, ft, base, ft.clone(), label="model == unified")
    assert f32_bits(rep.lam) == f32_bits(1.0) and rep.resid_sq == 0.0 and torch.equal(raw(got), raw(ft))
    mask, scale, rep, got = check_mask(engine, base.clone(), base, ft, label="model == base")
    assert rep.A == 0.0 and rep.nonzero == 0 and rep.c == 0 and f32_bits(rep.lam) == f32_bits(0.0)
    e = torch.zeros((0, 8), dtype=torch.bfloat16, device=device)
    mask, scale, rep = engine.emr_mask(e, e, e)
    assert mask.numel() == 0 and f32_bits(float(scale[0])) == f32_bits(0.0) and rep.c == 0 and rep.resid_sq == 0.0
    assert engine.emr_apply(e, e, mask, scale).shape == e.shape


def check_mask_nonfinite(engine, device="cpu"):
    for where, word in ((0, "finetune - base"), (1, "finetune - base"), (2, "unified - base")):
        for poison in (float("nan"), float("inf")):
            ts = [t.clone() for t in triple(SMALL, seed=18, device=device)]
            ts[where].view(-1)[777] = poison
            if where == 1:
                ts[2].view(-1)[777] = poison                           # NaN - NaN and Inf - Inf are both NaN: the first message
            with pytest.raises(ValueError, match=rf"model\.norm\.weight.*{word}"):
                engine.emr_mask(ts[0], ts[1], ts[2], name="model.norm.weight")
    ft, base, uni = triple(SMALL, seed=19, device=device)
    check_mask(engine, ft, base, uni, label="after an error")


def check_mask_underflow(engine, device="cpu"):
    """deltas whose product underflows to zero still compare by sign"""
    d = torch.tensor([1e-30, -1e-30, 1e-30, -1e-30, 1e-42, 0.0, -0.0, 1e-42], dtype=torch.float32, device=device)
    u = torch.tensor([1e-30, 1e-30, -1e-30, -1e-30, 1e-42, 1e-30, -1e-30, 0.0], dtype=torch.float32, device=device)
    zero = torch.zeros_like(d)
    mask, _, rep, _ = check_mask(engine, d, zero, u, label="underflow")
    assert int(mask[0, 0]) == 0b00011001 and rep.c == 3


MASK_CORNERS = [check_mask_ranks, check_mask_offset_views, check_mask_degenerate, check_mask_nonfinite, check_mask_underflow]


# ---- launches and the C ABI ---------------------------------------------------------------------------------------------------------
def check_profile(engine, device="cpu"):
    for k in (2, 5):
        fts, bases, bo = make_inputs((40, 50), k, seed=6, device=device)
        assert profile_of(engine, lambda: engine.emr_merge(fts, bases, bo)) == {"emr_merge": 1}
    ft, base, uni = triple((40, 50), seed=6, device=device)
    assert profile_of(engine, lambda: engine.emr_mask(ft, base, uni)) == {"emr_mask": 1, "geo_gram_fold": 1}
    mask, scale, _ = engine.emr_mask(ft, base, uni)
    assert profile_of(engine, lambda: engine.emr_apply(base, uni, mask, scale)) == {"emr_apply": 1}


def check_c_abi(engine, device="cpu"):
    from shardmerge_amd import _lib
    x = torch.zeros(64, dtype=torch.bfloat16, device=device)
    y = torch.zeros(64, dtype=torch.bfloat16, device=device)
    out = torch.zeros(64, dtype=torch.bfloat16, device=device)
    plane = torch.zeros(8, dtype=torch.uint8, device=device)
    sc = torch.zeros(1, dtype=torch.float32, device=device)
    dll, h = engine.lib.dll, engine.ctx.h
    err = lambda: dll.smhip_last_error(h).decode()

    def merge(k=1, out_t=out, n=64, in_dtype=_lib.BF16, lam=1.0):
        d = _lib.EmrDesc()
        d.k = k
        for i in range(max(0, min(k, 16))):
            d.finetune[i], d.base[i] = x.data_ptr(), y.data_ptr()
        d.in_dtype, d.base_out, d.base_out_dtype, d.n, d.lam = in_dtype, y.data_ptr(), _lib.BF16, n, lam
        rep = _lib.EmrReport()
        return dll.smhip_emr_merge(h, C.byref(d), out_t.data_ptr(), None, C.byref(rep), None), err(), rep

    rc, msg, rep = merge()
    assert rc == _lib.OK and rep.n == 64 and rep.zero == 64 and rep.winner[0] == 0, msg
    for kwargs, word in (({"k": 0}, "k out of range"), ({"k": 17}, "k out of range"), ({"lam": float("inf")}, "lambda"),
                         ({"lam": float("nan")}, "lambda"), ({"out_t": x}, "overlaps"), ({"in_dtype": 3}, "dtype")):
        rc, msg, _ = merge(**kwargs)
        assert rc == _lib.ERR_ARG and "emr_merge" in msg and word in msg, (kwargs, rc, msg)
    assert dll.smhip_emr_merge(h, None, out.data_ptr(), None, None, None) == _lib.ERR_ARG and "null descriptor" in err()
    assert merge(n=0, out_t=x)[0] == _lib.OK                     # a no-op, whatever the pointers

    def mask(ft=x, uni=out, plane_t=plane, scale_t=sc, dtype=_lib.BF16):
        d = _lib.EmrMaskDesc(ft.data_ptr(), y.data_ptr(), uni.data_ptr(), dtype, 1, 64)
        rep = _lib.EmrMaskReport()
        return dll.smhip_emr_mask(h, C.byref(d), plane_t.data_ptr() if plane_t is not None else None,
                                  scale_t.data_ptr() if scale_t is not None else None, C.byref(rep), None), err(), rep

    rc, msg, rep = mask()
    assert rc == _lib.OK and rep.cols == 64 and rep.c == 0, msg
    for kwargs, word in (({"dtype": 3}, "dtype"), ({"plane_t": None}, "null"), ({"scale_t": None}, "null"),
                         ({"plane_t": x.view(torch.uint8)}, "overlaps")):
        rc, msg, _ = mask(**kwargs)
        assert rc == _lib.ERR_ARG and "emr_mask" in msg and word in msg, (kwargs, rc, msg)
    assert dll.smhip_emr_mask(h, None, plane.data_ptr(), sc.data_ptr(), None, None) == _lib.ERR_ARG and "null descriptor" in err()

    def apply(out_t=out, uni=x, dtype=_lib.BF16, plane_t=plane):
        d = _lib.EmrApplyDesc(y.data_ptr(), uni.data_ptr(), dtype, 1, 64, plane_t.data_ptr() if plane_t is not None else None, sc.data_ptr())
        return dll.smhip_emr_apply(h, C.byref(d), out_t.data_ptr(), None), err()

    assert apply()[0] == _lib.OK
    for kwargs, word in (({"dtype": 3}, "dtype"), ({"plane_t": None}, "null"), ({"out_t": x}, "overlaps")):
        rc, msg = apply(**kwargs)
        assert rc == _lib.ERR_ARG and "emr_apply" in msg and word in msg, (kwargs, rc, msg)
    assert dll.smhip_emr_apply(h, None, out.data_ptr(), None) == _lib.ERR_ARG and "null descriptor" in err()


# ---- independent of the oracle: the paper's form in torch fp64 ---------------------------------------------------------------------
def paper_inputs(k, shape=(512, 1024), device="cpu"):
    g = torch.Generator().manual_seed(5000 + k)
    base = (torch.randn(shape, generator=g) * 0.02).to(torch.bfloat16)
    fts = [(base.float() + torch.randn(shape, generator=g) * (3e-3 * (1 + 0.3 * i))).to(torch.bfloat16) for i in range(k)]
    return [f.to(device) for f in fts], base.to(device)


def check_paper_form(engine, k, device="cpu"):
    """elect as the paper writes it - the stacked sum, the flag with >= 0, the running where(abs > max) - the masks and
    sum |tau| / sum |M tau_uni|, all in fp64.  An element is UNCERTAIN where the sign of the fp64 sum differs from the fp32
    sum's: at most 0.1 % may be (the reference alone gives none on these inputs).  Everywhere else tau and every mask bit
    are equal.  lambda: within 2^-23 |lambda_ref| - one fp32 rounding (2^-24) plus an ordered fp64 sum of n non-negative
    terms on either side (n 2^-53 each), far below the other 2^-24.  resid_sq: within (n + 8) 2^-53 (D2 + 2 lambda X +
    lambda^2 U2) of the residual recomputed in fp64 from the unpacked mask - n additions of non-negative terms per sum and
    the handful of operations that combine them."""
    fts, base = paper_inputs(k, device=device)
    n = base.numel()
    out, rep, delta = engine.emr_merge(fts, [base] * k, base, want_delta=True)
    b64 = base.cpu().double()
    tv = torch.stack([f.cpu().double() - b64 for f in fts])
    s64 = tv.sum(0)
    s32 = torch.zeros(base.shape, dtype=torch.float32)
    for i in range(k):
        s32 = s32 + tv[i].float()
    uncertain = (s64 >= 0) != (s32 >= 0)
    print(f"k={k}: uncertain {int(uncertain.sum())} of {n}")
    assert int(uncertain.sum()) <= n // 1000
    flag = torch.where(s64 >= 0, 1.0, -1.0).double()
    top = torch.zeros_like(s64)
    for i in range(k):
        agrees = tv[i] * flag > 0
        top = torch.where(agrees & (tv[i].abs() > top), tv[i].abs(), top)
    tau = top * flag
    sure = ~uncertain
    # (tau rounded once to fp32, as the function's d_i is: a bf16 difference whose operands lie more than 16 binades apart
    #  does not fit fp32's 24 bits, and rounding is monotonic, so it commutes with the maximum)
    assert torch.equal(delta.cpu()[sure], tau.float()[sure])
    for i in range(k):
        mask, scale, mr = engine.emr_mask(fts[i], base, out)
        m_ref = tv[i] * tau > 0
        got = torch.from_numpy(unpack_bits(mask.cpu().numpy(), base.shape[1])).reshape(base.shape)
        assert torch.equal(got[sure], m_ref[sure]), (k, i)
        lam_ref = float(tv[i].abs().sum() / (m_ref * tau).abs().sum())
        print(f"k={k} i={i}: lambda {mr.lam!r} ref {lam_ref!r}")
        assert abs(mr.lam - lam_ref) <= 2.0 ** -23 * abs(lam_ref), (k, i, mr.lam, lam_ref)
        u = out.cpu().double() - b64
        resid = float(((tv[i] - mr.lam * got.double() * u) ** 2).sum())
        bound = (n + 8) * 2.0 ** -53 * (mr.D2 + 2 * mr.lam * mr.X + mr.lam ** 2 * mr.U2)
        print(f"k={k} i={i}: resid_sq {mr.resid_sq!r} recomputed {resid!r} bound {bound!r}")
        assert abs(mr.resid_sq - resid) <= bound, (k, i, mr.resid_sq, resid, bound)


# ---- the command and the pack on the on-disk model of tests/lora_fixtures.py --------------------------------------------------------
OPTIONS = {"operator": "emr", "emr_lambda": 1.0}
PACK_FILES = ["emr_config.json", "emr_model.safetensors", "emr_task.json"]
ONE_ENTRY = {"operator": "dare_linear", "density": 1.0}
TASKS = ("org/ft1", "org/ft2")


def run_cli(args):
    from click.testing import CliRunner
    from shardmerge_amd.__main__ import cli
    return CliRunner().invoke(cli, [str(a) for a in args])


def task_args(root, model, out, device, more=(), base="org/base", unified="org/uni"):
    return ["emr-task", model, "--base", base, "--unified", unified, "--out", root / "storage" / out, "--storage-dir", root / "storage",
            "--device", device, *more]


def emr_models():
    """two finetunes of one base: ft1 provides the embedding, ft2 the output layers"""
    return [{"model": "org/ft1", "base": "org/base", "is_input": True}, {"model": "org/ft2", "base": "org/base", "is_output": True}]


def expected_unified(base, lam=1.0):
    from tests import lora_fixtures as lf

    def merge(fts, bases, alphas, base_out, name):
        return eo.emr_merge(fts, bases, base_out, lam=lam)["out"]
    return harness.expected_by_tensor(base, lf.model_tensors(2), emr_models(), merge)


def oracle_task(base, ft, uni, scale="model", full=()):
    """the tensors an EMR pack of `ft` stands for, by the oracle, in the model's layer order: emr_apply where masked, ft's own
    tensor where stored whole, the base's where nothing differs; returns (tensors, {name: what is stored}, lambda of the model)"""
    from shardmerge_amd.index import order_weights
    names = order_weights(list(ft))
    kinds, refs = {}, {}
    for name in names:
        if torch.equal(raw(ft[name]), raw(base[name])):
            continue
        if torch.equal(raw(uni[name]), raw(base[name])) or any(name.endswith(s) for s in full):
            kinds[name] = "full"
            continue
        kinds[name] = "masked"
        refs[name] = eo.emr_mask(ft[name], base[name], uni[name])
    A = B = 0.0
    for name in names:
        if name in refs:
            A, B = A + refs[name].A, B + refs[name].B
    lam = eo.scale_of(A, B)
    out = {}
    for name in names:
        if name not in kinds:
            out[name] = base[name]
        elif kinds[name] == "full":
            out[name] = ft[name]
        else:
            sc = torch.tensor([float(lam)], dtype=torch.float32) if scale == "model" else refs[name].scale
            out[name] = eo.emr_apply(base[name], uni[name], refs[name].mask, sc)
    return out, kinds, refs, float(lam)


def setup_unified(tmp_path, engine, device):
    """the k3 storage, the emr merge of ft1 and ft2 run twice (the same bytes, the oracle's tensors), its output placed in the
    storage directory as org/uni; returns (base, the unified model's tensors)"""
    from tests import lora_fixtures as lf
    base, _, _ = lf.setup_k3(tmp_path, engine)
    expected = expected_unified(base)
    cfg = harness.write_config(tmp_path, emr_models(), "merged", OPTIONS, device)
    res = harness.run_cli(cfg)
    assert res.exit_code == 0, res.output
    harness.assert_outputs(tmp_path / "merged", expected)
    readme = (tmp_path / "merged" / "README.md").read_text()
    for word in ("# EMR Merged Model", "EMR-Merging", "lambda 1", "org/ft1"):
        assert word in readme, (word, readme)
    res = harness.run_cli(harness.write_config(tmp_path, emr_models(), "merged2", OPTIONS, device))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged2", tmp_path / "merged")
    res = harness.run_cli(cfg, "analyze")
    assert res.exit_code == 0, res.output
    lf.write_model(tmp_path / "storage", "org/uni", expected)
    return base, expected


def pack_entry(pack, **flags):
    return [{"model": pack, "base": "org/base", "is_input": True, "is_output": True, **flags}]


def check_end_to_end(tmp_path, engine, device):
    """emr merge -> the unified model in storage -> emr-task per finetune -> a one-entry dare_linear merge of each pack equals
    the oracle's emr_apply tensors; the files, the config, the report, analyze, an existing pack"""
    from safetensors.torch import load_file
    from shardmerge_amd.emrpack import EmrPack, is_emr_dir
    from shardmerge_amd.index import LocalModelIndex
    from tests import lora_fixtures as lf
    base, uni = setup_unified(tmp_path, engine, device)
    storage = tmp_path / "storage"
    for t, which in enumerate((1, 2)):
        ft = lf.model_tensors(which)
        pack_uri = f"org/task{which}"
        res = run_cli(task_args(tmp_path, TASKS[t], pack_uri, device))
        assert res.exit_code == 0, res.output
        out = storage / pack_uri
        assert sorted(p.name for p in out.iterdir()) == PACK_FILES and is_emr_dir(out)
        assert "residual" in res.output and "q_proj" in res.output and "lambda" in res.output
        want, kinds, refs, lam = oracle_task(base, ft, uni)
        # the passthrough tensors the merge took from the other finetune or from this one are stored whole or masked
        pack = EmrPack(pack_uri, out)
        assert {n: x.kind for n, x in pack.tensors.items()} == kinds and pack.unified == "org/uni"
        cfg = json.loads((out / "emr_config.json").read_text())
        assert (cfg["format"], cfg["version"], cfg["base_model_name_or_path"], cfg["unified_model_name_or_path"], cfg["scale"]) == \
            ("shardmerge-emr", 1, "org/base", "org/uni", "model")
        assert cfg["tensors"] == {n: {"shape": list(ft[n].shape), "dtype": "BF16"} for n in kinds}
        got = load_file(str(out / "emr_model.safetensors"))
        rep = json.loads((out / "emr_task.json").read_text())
        index = LocalModelIndex(storage_path=storage)
        asyncio.run(index.add_model("org/base"))
        asyncio.run(index.add_model(pack_uri))
        assert index.emr(pack_uri) is not None and index.pack(pack_uri) is None and index.adapter(pack_uri) is None
        assert [x["name"] for x in rep["tensors"]] == [n for n in index.get_layer_order("org/base") if n in kinds]
        assert f32_bits(rep["lambda"]) == f32_bits(lam)
        for x in rep["tensors"]:
            name = x["name"]
            if kinds[name] == "full":
                assert x["stored"] == "full" and torch.equal(raw(got[f"{name}.full"]), raw(ft[name]))
                continue
            r = refs[name]
            assert torch.equal(got[f"{name}.mask"], r.mask) and f32_bits(float(got[f"{name}.scale"][0])) == f32_bits(lam)
            assert (x["c"], x["nonzero"], x["shape"]) == (r.c, r.nonzero, list(ft[name].shape)) and f32_bits(x["lambda"]) == f32_bits(lam)
            resid = eo.resid_of(r.D2, r.X, r.U2, lam)
            assert x["resid_sq"] == resid and x["relative_residual"] == math.sqrt(resid / r.D2)
            assert x["bytes"] == r.mask.numel() + 4
        assert rep["totals"]["bytes"] == sum(x["bytes"] for x in rep["tensors"]) == sum(v.numel() * v.element_size() for v in got.values())
        # the pack as the one entry of a dare_linear merge at density 1: the task's model
        cfgp = harness.write_config(tmp_path, pack_entry(pack_uri), f"task{which}", ONE_ENTRY, device)
        res = harness.run_cli(cfgp)
        assert res.exit_code == 0, res.output
        harness.assert_outputs(tmp_path / f"task{which}", want)
        res = harness.run_cli(cfgp, "analyze")
        assert res.exit_code == 0, res.output
    # an existing pack is not overwritten
    before = (storage / "org/task1" / "emr_model.safetensors").read_bytes()
    res = run_cli(task_args(tmp_path, "org/ft1", "org/task1", device))
    assert res.exit_code != 0 and (storage / "org/task1" / "emr_model.safetensors").read_bytes() == before
    return base, uni


def check_forms(tmp_path, engine, device):
    """--scale tensor and --full: a rescaler per tensor, the named tensors stored whole; the pack next to a full finetune in a
    ties merge equals the merge of the oracle's tensors"""
    from tests import lora_fixtures as lf
    from tests import ties_oracle
    base, uni = setup_unified(tmp_path, engine, device)
    ft = lf.model_tensors(1)
    res = run_cli(task_args(tmp_path, "org/ft1", "org/task", device, ("--scale", "tensor", "--full", "k_proj.weight,input_layernorm.weight")))
    assert res.exit_code == 0, res.output
    want, kinds, refs, _ = oracle_task(base, ft, uni, scale="tensor", full=("k_proj.weight", "input_layernorm.weight"))
    assert sorted(n for n, k in kinds.items() if k == "full" and "layers" in n) == sorted(n for n, _ in lf.TENSORS if "k_proj" in n or "layernorm" in n)
    rep = json.loads((tmp_path / "storage" / "org/task" / "emr_task.json").read_text())
    assert {x["name"]: x["stored"] for x in rep["tensors"]} == kinds and rep["lambda"] is None
    for x in rep["tensors"]:
        if x["stored"] == "masked":
            assert f32_bits(x["lambda"]) == f32_bits(refs[x["name"]].lam) and x["resid_sq"] == refs[x["name"]].resid_sq
    res = harness.run_cli(harness.write_config(tmp_path, pack_entry("org/task"), "task", ONE_ENTRY, device))
    assert res.exit_code == 0, res.output
    harness.assert_outputs(tmp_path / "task", want)
    opts = {"operator": "ties", "density": 0.3, "ties_lambda": 0.7}
    models = [{"model": "org/task", "base": "org/base", "alpha": 0.5, "is_input": True},
              {"model": "org/ft2", "base": "org/base", "alpha": 0.4, "is_output": True}]
    res = harness.run_cli(harness.write_config(tmp_path, models, "merged_ties", opts, device))
    assert res.exit_code == 0, res.output
    got = lf.read_outputs(tmp_path / "merged_ties")
    emb = "model.embed_tokens.weight"
    assert torch.equal(raw(got[emb]), raw(want[emb]))
    ft2 = lf.model_tensors(2)
    for name in ("model.layers.1.self_attn.q_proj.weight", "model.layers.0.self_attn.k_proj.weight"):
        ref = ties_oracle.ties_merge([want[name], ft2[name]], [base[name]] * 2, [0.5, 0.4], base[name], 0.3, 0.7, True)[0]
        assert torch.equal(raw(got[name]), raw(ref)), name


def check_stamp(tmp_path, engine, device):
    """a resume after the pack has changed must not reuse old shards: the stamp hashes its config bytes and its header"""
    from safetensors.torch import load_file, save_file
    from shardmerge_amd import distributed
    from shardmerge_amd.config import MergeConfig
    setup_unified(tmp_path, engine, device)
    assert run_cli(task_args(tmp_path, "org/ft1", "org/task", device)).exit_code == 0
    pack = tmp_path / "storage" / "org/task"
    cfg = MergeConfig.from_yaml(harness.write_config(tmp_path, pack_entry("org/task"), "out", ONE_ENTRY, device))
    s0 = distributed.config_stamp(cfg)
    assert s0 == distributed.config_stamp(cfg)
    assert s0 != distributed.config_stamp(MergeConfig.from_yaml(harness.write_config(tmp_path, pack_entry("org/ft1"), "out", ONE_ENTRY, device)))
    text = (pack / "emr_config.json").read_text()
    (pack / "emr_config.json").write_text(text + "\n")
    s1 = distributed.config_stamp(cfg)
    (pack / "emr_config.json").write_text(text)
    tensors = load_file(str(pack / "emr_model.safetensors"))
    save_file(tensors, str(pack / "emr_model.safetensors"), metadata={"format": "pt", "note": "rewritten"})
    s2 = distributed.config_stamp(cfg)
    assert len({s0, s1, s2}) == 3


def write_pack(storage, uri, stored, tensor_meta, **config):
    from safetensors.torch import save_file
    d = storage / uri
    d.mkdir(parents=True, exist_ok=True)
    save_file({k: v.contiguous() for k, v in stored.items()}, str(d / "emr_model.safetensors"), metadata={"format": "pt"})
    cfg = {"format": "shardmerge-emr", "version": 1, "base_model_name_or_path": "org/base", "unified_model_name_or_path": "org/ft2",
           "scale": "model", "tensors": tensor_meta}
    cfg.update(config)
    (d / "emr_config.json").write_text(json.dumps(cfg))


def check_reader_rejections(tmp_path, engine, device):
    """every pack the reader rejects: EmrPackError naming the pack and the key or field, and `merge` ends before an output
    exists; a pack or an adapter as the base or as the unified model of an EMR entry"""
    from shardmerge_amd.adapter import base_tensor_meta
    from shardmerge_amd.config import MergeConfig
    from shardmerge_amd.emrpack import EmrPack, EmrPackError, is_emr_dir
    from shardmerge_amd.index import LocalModelIndex
    from shardmerge_amd.merge import operator_class
    from tests import lora_fixtures as lf
    base, _, _ = lf.setup_k3(tmp_path, engine)
    storage = tmp_path / "storage"
    q, n1 = "model.layers.0.self_attn.q_proj.weight", "model.norm.weight"
    good = {f"{q}.mask": torch.zeros(128, 16, dtype=torch.uint8), f"{q}.scale": torch.ones(1), f"{n1}.full": base[n1]}
    meta = {q: {"shape": [128, 128], "dtype": "BF16"}, n1: {"shape": [128], "dtype": "BF16"}}
    write_pack(storage, "org/good", good, meta)
    EmrPack("org/good", storage / "org/good")
    res = harness.run_cli(harness.write_config(tmp_path, pack_entry("org/good"), "fine", ONE_ENTRY, device))
    assert res.exit_code == 0, res.output
    # a directory that also holds delta_config.json is no EMR pack
    write_pack(storage, "org/both_kinds", good, meta)
    (storage / "org/both_kinds" / "delta_config.json").write_text("{}")
    assert is_emr_dir(storage / "org/good") and not is_emr_dir(storage / "org/both_kinds")

    def refused(uri, stored, match, meta=meta, direct=True, **config):
        write_pack(storage, uri, stored, meta, **config)
        if direct:
            with pytest.raises(EmrPackError, match=match):
                EmrPack(uri, storage / uri)
        res = harness.run_cli(harness.write_config(tmp_path, pack_entry(uri), "never", ONE_ENTRY, device))
        assert res.exit_code != 0 and not (tmp_path / "never").exists(), uri
        return res

    drop = lambda *keys: {k: v for k, v in good.items() if k not in keys}
    refused("org/bad_version", good, r"org/bad_version.*version 2", version=2)
    refused("org/bad_format", good, r"org/bad_format.*format", format="shardmerge-delta")
    refused("org/bad_scale_mode", good, r"org/bad_scale_mode.*scale 'row'", scale="row")
    refused("org/no_unified", good, r"org/no_unified.*unified_model_name_or_path", unified_model_name_or_path=None)
    refused("org/no_base", good, r"org/no_base.*base_model_name_or_path", base_model_name_or_path=3)
    refused("org/bad_suffix", {**good, f"{q}.sign": torch.zeros(3)}, rf"org/bad_suffix.*{q}\.sign.*suffix")
    refused("org/no_scale", drop(f"{q}.scale"), rf"org/no_scale.*{q}\.mask.*scale")
    refused("org/no_mask", drop(f"{q}.mask"), rf"org/no_mask.*{q}\.mask")
    refused("org/bad_plane", {**good, f"{q}.mask": torch.zeros(128, 15, dtype=torch.uint8)}, rf"org/bad_plane.*{q}\.mask.*\[128, 16\]")
    refused("org/bad_plane_dtype", {**good, f"{q}.mask": torch.zeros(128, 16, dtype=torch.int8)}, rf"org/bad_plane_dtype.*{q}\.mask.*U8")
    refused("org/bad_scale", {**good, f"{q}.scale": torch.zeros(128)}, rf"org/bad_scale.*{q}\.scale.*\[1\]")
    refused("org/bad_scale_dtype", {**good, f"{q}.scale": torch.zeros(1, dtype=torch.float16)}, rf"org/bad_scale_dtype.*{q}\.scale.*F32")
    refused("org/both", {**good, f"{q}.full": base[q]}, rf"org/both.*{q}\.full.*{q}\.(mask|scale)")
    refused("org/undeclared", good, rf"org/undeclared.*{n1}", meta={q: meta[q]})
    refused("org/bad_tensors", good, r"org/bad_tensors.*tensors", tensors=[1])
    # what only the shard headers of the base and of the unified model show (check_against, in initialize())
    refused("org/bad_shape", {**drop(f"{n1}.full"), f"{n1}.full": base[n1][:64]}, None, direct=False,
            meta={q: meta[q], n1: {"shape": [64], "dtype": "BF16"}})
    index = LocalModelIndex(storage_path=storage)
    asyncio.run(index.add_model("org/base"))
    with pytest.raises(EmrPackError, match=rf"org/bad_shape.*{n1}\.full.*base org/base"):
        EmrPack("org/bad_shape", storage / "org/bad_shape").check_against("org/base", base_tensor_meta(index, "org/base"))
    other = "model.layers.9.self_attn.q_proj.weight"
    write_pack(storage, "org/unknown", {f"{other}.full": base[q]}, {other: {"shape": [128, 128], "dtype": "BF16"}})
    with pytest.raises(EmrPackError, match=rf"org/unknown.*{other}\.full.*unified model org/base"):
        EmrPack("org/unknown", storage / "org/unknown").check_against("org/base", base_tensor_meta(index, "org/base"), what="unified model")
    odd = dict(lf.model_tensors(2))
    odd[q] = odd[q].float()
    lf.write_model(storage, "org/odd_uni", odd)
    write_pack(storage, "org/on_odd", good, meta, unified_model_name_or_path="org/odd_uni")
    write_pack(storage, "org/dpack", {f"{q}.sign": torch.zeros(128, 16, dtype=torch.uint8), f"{q}.scale": torch.zeros(128)}, {})
    (storage / "org/dpack" / "emr_config.json").unlink()
    (storage / "org/dpack" / "emr_model.safetensors").rename(storage / "org/dpack" / "delta_model.safetensors")
    (storage / "org/dpack" / "delta_config.json").write_text(json.dumps(
        {"format": "shardmerge-delta", "version": 1, "base_model_name_or_path": "org/base", "bits": 1, "density": 1.0, "scale": "row",
         "tensors": {q: meta[q]}}))

    def initialize(models):
        res = harness.run_cli(harness.write_config(tmp_path, models, "never", ONE_ENTRY, device))
        assert res.exit_code != 0 and not (tmp_path / "never").exists()
        cfg = MergeConfig.from_yaml(tmp_path / "never.yaml")
        return asyncio.run(operator_class(cfg.operator)(config=cfg, index_manager=LocalModelIndex(storage_path=storage)).initialize())

    with pytest.raises(EmrPackError, match=rf"org/on_odd.*{q}\.mask.*unified model org/odd_uni"):
        initialize(pack_entry("org/on_odd"))
    for bad, what in (("org/good", "an EMR pack"), ("org/dpack", "a delta pack"), ("org/lora", "an adapter")):
        with pytest.raises(ValueError, match=rf"org/good: the base of an EMR pack entry must be a full model, {bad} is {what}"):
            initialize([{"model": "org/good", "base": bad, "is_input": True, "is_output": True}])
        write_pack(storage, "org/on_bad", good, meta, unified_model_name_or_path=bad)
        with pytest.raises(ValueError, match=rf"org/on_bad: the unified model of an EMR pack entry must be a full model, {bad} is {what}"):
            initialize(pack_entry("org/on_bad"))


def check_command_rejections(tmp_path, engine, device, monkeypatch):
    """everything emr-task rejects is rejected before DIR exists; extract-lora and compress-delta take no EMR pack"""
    from shardmerge_amd.merge.compress import DeltaCompression
    from shardmerge_amd.merge.emr_task import EmrTask
    from shardmerge_amd.merge.extract import LoraExtraction
    from tests import dpack_checks as dc
    from tests import lora_fixtures as lf
    setup_unified(tmp_path, engine, device)
    storage = tmp_path / "storage"
    assert run_cli(task_args(tmp_path, "org/ft1", "org/task", device)).exit_code == 0
    assert dc.run_cli(dc.compress_args(tmp_path, "org/ft1", "org/dpack", device, ("--bits", 1))).exit_code == 0
    odd = dict(lf.model_tensors(1))
    odd["lm_head.weight"] = odd["lm_head.weight"].float()
    lf.write_model(storage, "org/odd_dtype", odd)
    odd = dict(lf.model_tensors(1))
    odd["model.norm.weight"] = odd["model.norm.weight"][:64]
    lf.write_model(storage, "org/odd_shape", odd)
    odd = dict(lf.model_tensors(1))
    del odd["lm_head.weight"]
    (storage / "org/fewer").mkdir(parents=True)
    from safetensors.torch import save_file
    save_file(odd, str(storage / "org/fewer" / "model.safetensors"), metadata={"format": "pt"})
    (storage / "org/fewer" / "model.safetensors.index.json").write_text(json.dumps(
        {"metadata": {}, "weight_map": {n: "model.safetensors" for n in odd}}))
    out = storage / "org/never"

    def refused(match, model="org/ft1", base="org/base", unified="org/uni", scale="model"):
        with pytest.raises(ValueError, match=match):
            asyncio.run(EmrTask(model, base, unified, out, storage, scale, engine=engine).run(device))
        assert not out.exists()
        res = run_cli(task_args(tmp_path, model, "org/never", device, ("--scale", scale), base=base, unified=unified))
        assert res.exit_code != 0 and not out.exists()

    for slot in ("model", "base", "unified"):
        refused("org/lora is an adapter", **{slot: "org/lora"})
        refused("org/dpack is a delta pack", **{slot: "org/dpack"})
        refused("org/task is itself an EMR pack", **{slot: "org/task"})
        refused("lm_head.weight", **{slot: "org/odd_dtype"})
        refused("model.norm.weight", **{slot: "org/odd_shape"})
        refused("do not hold the same tensors.*lm_head.weight", **{slot: "org/fewer"})
    refused("--scale 'row'", scale="row")
    refused("MODEL and --base are both org/base", model="org/base")
    refused("--base and --unified are both org/base", unified="org/base")
    monkeypatch.setenv("WORLD_SIZE", "2")
    refused("single process")
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(ValueError, match="already holds an EMR pack"):
        asyncio.run(EmrTask("org/ft1", "org/base", "org/uni", storage / "org/task", storage, engine=engine).run(device))
    with pytest.raises(ValueError, match="--full ' , ' names no suffix"):
        from shardmerge_amd.merge.emr_task import parse_suffixes
        parse_suffixes(" , ")
    for model, base in (("org/task", "org/base"), ("org/ft1", "org/task")):
        with pytest.raises(ValueError, match="extract-lora: org/task is an EMR pack"):
            asyncio.run(LoraExtraction(model, base, 8, out, storage, engine=engine).extract(device))
        with pytest.raises(ValueError, match="compress-delta: org/task is an EMR pack"):
            asyncio.run(DeltaCompression(model, base, out, storage, 1, engine=engine).compress(device))
        assert not out.exists()
