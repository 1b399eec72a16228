"""Checks of the Consensus operators shared by the emulator tier (tests/test_consensus_host.py) and the GPU tier
(tests/test_consensus_gpu.py): Engine.consensus_merge against tests/consensus_oracle.py, BIT FOR BIT - output, merged
delta, masked / agree / selected counts and, for the TIES flavour, k_keep, thresholds and kept counts.  The tolerance is
zero and it is derived, not measured: every step of the function is one correctly rounded fp32 operation, a comparison,
an integer count or an exact order statistic (include/shardmerge_hip.h, smhip_consensus_merge)."""
import ctypes as C

import pytest
import torch

from tests import consensus_oracle
from tests import harness
from tests.harness import ALPHAS, expected_by_tensor, f32_bits, make_inputs, profile_of, raw, ties_models

FLAVOURS = (False, True)                        # ties: consensus_ta, consensus_ties
FLAVOUR_IDS = ["consensus_ta", "consensus_ties"]
KS = (1, 2, 3, 4, 5, 16)                        # 4 | 5 straddles the two register variants of the kernel
CONSENSUS_KS = (1, 2, "k", 16)
MASK_LAMBDAS = (0.0, 0.4, 1.0, 3.0)
SHAPE = (37, 129)                               # 4773 elements: unaligned rows and a tail octet
SIZES = (1, 7, 8, 9, 2047, 2048, 2049)          # around one octet and around one work-group of 256 octets


def name_of(ties):
    return "consensus_ties" if ties else "consensus_ta"


def check(engine, fts, bases, alphas, base_out, ties=False, density=0.2, mask_lambda=0.4, consensus_k=2, lam=1.0, normalize=True,
          label=""):
    """one call against the oracle, bit for bit, and the invariants of the report; returns (report, out, delta)"""
    kw = dict(ties=ties, density=density, mask_lambda=mask_lambda, consensus_k=consensus_k, lam=lam, normalize=normalize)
    out, rep, delta = engine.consensus_merge(fts, bases, alphas, base_out, want_delta=True, **kw)
    cpu = lambda ts: [t.cpu() for t in ts]
    ref = consensus_oracle.consensus_merge(cpu(fts), cpu(bases), alphas, base_out.cpu(), **kw)
    k, n = len(fts), base_out.numel()
    print(f"{label}: selected {rep.selected} / {ref['selected']}, agree {rep.agree} / {ref['agree']}, masked {rep.masked} / {ref['masked']}")
    assert out.dtype == base_out.dtype and out.shape == base_out.shape, label
    assert rep.n == n and rep.ties == ties, label
    assert rep.masked == ref["masked"], (label, rep.masked, ref["masked"])
    assert rep.agree == ref["agree"], (label, rep.agree, ref["agree"])
    assert rep.selected == ref["selected"], (label, rep.selected, ref["selected"])
    assert rep.k_keep == ref["k_keep"], (label, rep.k_keep, ref["k_keep"])
    assert [f32_bits(t) for t in rep.thresholds] == [f32_bits(float(t)) for t in ref["thresholds"]], (label, rep.thresholds, ref["thresholds"])
    assert rep.kept == ref["kept"], (label, rep.kept, ref["kept"])
    # the invariants
    need = min(consensus_k, k)
    assert sum(rep.agree) == n, (label, rep.agree, n)
    assert rep.selected == sum(rep.agree[need:]), (label, rep.selected, rep.agree, need)
    assert sum(c * a for c, a in enumerate(rep.agree)) == sum(rep.masked), (label, rep.agree, rep.masked)
    bad = int((raw(delta) != raw(ref["delta"])).sum())
    assert bad == 0, f"{label}: {bad} of {n} merged-delta values differ in their bits"
    bad = int((raw(out) != raw(ref["out"])).sum())
    assert bad == 0, f"{label}: {bad} of {n} output values differ in their bits"
    return rep, out, delta


# ---- the parameter grid -------------------------------------------------------------------------------
def check_dtypes(engine, in_dtype, bo_dtype, ties, device="cpu"):
    fts, bases, bo = make_inputs(SHAPE, 3, in_dtype, bo_dtype, seed=11, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:3], bo, ties=ties, lam=0.7, label=f"{in_dtype}->{bo_dtype}")
    fts, bases, bo = make_inputs(SHAPE, 2, in_dtype, bo_dtype, seed=12, device=device)      # one shared base
    check(engine, fts, bases, ALPHAS[:2], bo, ties=ties, density=0.5, normalize=False, label=f"{in_dtype}->{bo_dtype} shared")


def check_k_options(engine, k, consensus_k, mask_lambda, ties, device="cpu"):
    ck = k if consensus_k == "k" else consensus_k
    own = (k + ck) % 2 == 1
    fts, bases, bo = make_inputs(SHAPE, k, seed=20 + k, own_bases=own, device=device)
    rep, _, _ = check(engine, fts, bases, ALPHAS[:k], bo, ties=ties, mask_lambda=mask_lambda, consensus_k=ck,
                      label=f"{name_of(ties)} k={k} consensus_k={ck} mask_lambda={mask_lambda}")
    if mask_lambda == 0.0:
        assert rep.masked == [bo.numel()] * k and rep.selected == bo.numel()
    if k == 1 and not ties:
        assert rep.selected == bo.numel()           # U - tv_0 == 0: one entry is taken as it is


def check_lambda_normalize(engine, lam, normalize, ties, device="cpu"):
    for k in (3, 5):
        fts, bases, bo = make_inputs(SHAPE, k, seed=40 + k, own_bases=True, device=device)
        check(engine, fts, bases, ALPHAS[:k], bo, ties=ties, lam=lam, normalize=normalize, label=f"k={k} lam={lam} normalize={normalize}")


def check_size(engine, n, ties, device="cpu"):
    for k in (2, 5):
        fts, bases, bo = make_inputs((n,), k, seed=70 + k, device=device)
        check(engine, fts, bases, ALPHAS[:k], bo, ties=ties, density=0.5, label=f"n={n} k={k}")


# ---- corners ----------------------------------------------------------------------------------------------
def check_unaligned(engine, device="cpu"):
    """views of 16-bit tensors that start 2 bytes off a 16-byte boundary: the element-wise path of the loader and the store"""
    for dtype in (torch.bfloat16, torch.float16):
        for n in (1003, 2048):
            for ties in FLAVOURS:
                fts, bases, bo = make_inputs((n + 5,), 3, dtype, seed=71, own_bases=True, device=device)
                cut = lambda t, o: t[o:o + n]
                check(engine, [cut(fts[0], 1), cut(fts[1], 3), cut(fts[2], 0)], [cut(bases[0], 0), cut(bases[1], 1), cut(bases[2], 5)],
                      ALPHAS[:3], cut(bo, 1), ties=ties, label=f"unaligned {dtype} n={n}")


def check_bases(engine, device="cpu"):
    """a base per finetune; one shared base that is also base_out (loaded once)"""
    for ties in FLAVOURS:
        for k in (3, 5):
            fts, bases, bo = make_inputs(SHAPE, k, seed=50 + k, own_bases=True, device=device)
            check(engine, fts, bases, ALPHAS[:k], bo, ties=ties, label=f"own bases k={k}")
            fts, bases, bo = make_inputs(SHAPE, k, seed=52 + k, device=device)
            assert bo is bases[0] and all(b is bases[0] for b in bases)
            check(engine, fts, bases, ALPHAS[:k], bo, ties=ties, label=f"out_is_base0 k={k}")


def check_signed_alphas(engine, device="cpu"):
    for ties in FLAVOURS:
        for normalize in (True, False):
            fts, bases, bo = make_inputs(SHAPE, 4, seed=55, own_bases=True, device=device)
            check(engine, fts, bases, [0.5, -0.3, 0.0, -0.7], bo, ties=ties, density=0.5, lam=0.7, normalize=normalize, label="signed alphas")
            check(engine, fts, bases, [-0.5, -0.3, -0.2, -0.7], bo, ties=ties, lam=-0.7, normalize=normalize, label="negative alphas")


def check_tiny_weight_sum(engine, device="cpu"):
    """alphas whose sum cancels: |D| < 1e-8 and D is replaced by 1"""
    for ties in FLAVOURS:
        fts, bases, bo = make_inputs(SHAPE, 2, seed=56, own_bases=True, device=device)
        check(engine, fts, bases, [0.5, -0.5], bo, ties=ties, density=1.0, consensus_k=1, label="D = 0")
        fts, bases, bo = make_inputs(SHAPE, 1, seed=57, device=device)
        check(engine, fts, bases, [1e-9], bo, ties=ties, density=0.5, label="D = 1e-9")


def check_zero_deltas(engine, device="cpu"):
    """every finetune equals its base: every mask is set (0 >= 0), agree[k] == n, the output is base_out"""
    for ties in FLAVOURS:
        for k in (2, 5):
            fts, bases, bo = make_inputs(SHAPE, k, seed=60, device=device)
            fts = [b.clone() for b in bases]
            rep, out, delta = check(engine, fts, bases, ALPHAS[:k], bo, ties=ties, mask_lambda=3.0, consensus_k=k, label="zero deltas")
            n = bo.numel()
            assert rep.agree == [0] * k + [n] and rep.masked == [n] * k and rep.selected == n
            assert torch.equal(raw(out), raw(bo)) and not bool(delta.any())


def check_denormals(engine, device="cpu"):
    g = torch.Generator().manual_seed(66)
    ft = (torch.randn(SHAPE, generator=g) * 1e-40).to(device)
    assert 0 < float(ft.abs().max()) < 1.2e-38
    zero = torch.zeros_like(ft)
    fb = (torch.randn(SHAPE, generator=g) * 1e-39).to(torch.bfloat16).to(device)
    assert 0 < float(fb.float().abs().max()) < 1.2e-38
    bo = make_inputs(SHAPE, 1, seed=67, device=device)[2]
    for ties in FLAVOURS:
        check(engine, [ft, ft * 0.5, -ft], [zero] * 3, [0.5, 0.75, 0.25], zero, ties=ties, density=0.5, lam=0.7, label="fp32 denormal deltas")
        check(engine, [fb, -fb], [torch.zeros_like(fb)] * 2, [0.5, 0.25], bo, ties=ties, density=0.5, label="bf16 denormal deltas")


def check_tied_finetunes(engine, device="cpu"):
    """ft_1 == ft_0 with equal weights, k = 2, mask_lambda = 1: |tv| >= |U - tv| holds with EQUALITY, and >= decides"""
    fts, bases, bo = make_inputs(SHAPE, 1, seed=68, device=device)
    n = bo.numel()
    rep, _, _ = check(engine, [fts[0], fts[0]], [bases[0], bases[0]], [0.5, 0.5], bo, ties=False, mask_lambda=1.0, consensus_k=2,
                      label="tied finetunes")
    assert rep.agree == [0, 0, n] and rep.selected == n           # (U - tv = tv exactly: 2 tv - tv)
    rep, _, _ = check(engine, [fts[0], fts[0]], [bases[0], bases[0]], [0.5, 0.5], bo, ties=True, density=1.0, normalize=False,
                      mask_lambda=1.0, consensus_k=2, label="tied finetunes, ties")
    assert rep.agree == [0, 0, n] and rep.selected == n
    # a hair above 1 and the equality fails wherever the delta is not zero
    zeros = int((fts[0].float() - bases[0].float() == 0).sum())
    rep, _, _ = check(engine, [fts[0], fts[0]], [bases[0], bases[0]], [0.5, 0.5], bo, ties=False, mask_lambda=1.0000001, consensus_k=2,
                      label="tied finetunes, mask_lambda > 1")
    assert rep.agree == [n - zeros, 0, zeros]


def check_nonfinite(engine, device="cpu"):
    """a NaN / an Inf in one finetune: ValueError naming the tensor and the finetune; the context stays usable"""
    for ties in FLAVOURS:
        for k, poison in ((3, float("inf")), (5, float("nan")), (3, float("-inf"))):
            fts, bases, bo = make_inputs(SHAPE, k, seed=80, device=device)
            fts[1] = fts[1].clone()
            fts[1].view(-1)[4321] = poison
            with pytest.raises(ValueError, match=r"model\.layers\.7\.mlp\.up_proj\.weight.*finetune 1\b"):
                engine.consensus_merge(fts, bases, ALPHAS[:k], bo, ties=ties, layer_name="model.layers.7.mlp.up_proj.weight")
            fts, bases, bo = make_inputs(SHAPE, k, seed=81, device=device)
            check(engine, fts, bases, ALPHAS[:k], bo, ties=ties, label="after an error")


def check_tiny_and_rank3(engine, device="cpu"):
    for ties in FLAVOURS:
        fts, bases, bo = make_inputs((0,), 2, seed=73, device=device)
        out, rep = engine.consensus_merge(fts, bases, [0.5, 0.5], bo, ties=ties)
        assert out.numel() == 0 and out.dtype == bo.dtype and rep.selected == 0 and rep.agree == [0, 0, 0] and rep.masked == [0, 0]
        fts, bases, bo = make_inputs((4, 33, 65), 3, seed=74, own_bases=True, device=device)
        check(engine, fts, bases, ALPHAS[:3], bo, ties=ties, label="rank 3")


def check_determinism(engine, device="cpu"):
    fts, bases, bo = make_inputs((300, 500), 3, seed=90, own_bases=True, device=device)
    for ties in FLAVOURS:
        a, ra = engine.consensus_merge(fts, bases, ALPHAS[:3], bo, ties=ties)
        b, rb = engine.consensus_merge(fts, bases, ALPHAS[:3], bo, ties=ties)
        assert torch.equal(raw(a), raw(b)) and ra == rb


# ---- the identities with the existing operators, through the same engine ----------------------------------------
def check_ta_is_dare_linear(engine, device="cpu"):
    """mask_lambda 0, consensus_k 1: every mask is set, everything selected - dare_linear at density 1"""
    for k, own, lam, normalize in ((3, True, 0.7, True), (5, False, 1.0, False), (1, False, 1.0, True), (16, True, 1.0, True)):
        fts, bases, bo = make_inputs(SHAPE, k, seed=100 + k, own_bases=own, device=device)
        out, rep, delta = engine.consensus_merge(fts, bases, ALPHAS[:k], bo, ties=False, mask_lambda=0.0, consensus_k=1, lam=lam,
                                                 normalize=normalize, want_delta=True)
        d_out, _, d_delta = engine.dare_merge(fts, bases, ALPHAS[:k], bo, density=1.0, lam=lam, normalize=normalize,
                                              sign_election=False, want_delta=True)
        assert torch.equal(raw(out), raw(d_out)) and torch.equal(raw(delta), raw(d_delta)), k
        assert rep.selected == bo.numel()


def check_ties_is_ties(engine, device="cpu"):
    """mask_lambda 0, consensus_k 1 on top of TIES: smhip_ties_merge at the same density, report included"""
    for k, own, density, lam, normalize in ((3, True, 0.2, 0.7, True), (5, False, 0.5, 1.0, False), (1, False, 1.0, 1.0, True),
                                            (2, True, 0.01, 1.0, True)):
        fts, bases, bo = make_inputs(SHAPE, k, seed=100 + k, own_bases=own, device=device)
        out, rep, delta = engine.consensus_merge(fts, bases, ALPHAS[:k], bo, ties=True, density=density, mask_lambda=0.0,
                                                 consensus_k=1, lam=lam, normalize=normalize, want_delta=True)
        t_out, t_rep, t_delta = engine.ties_merge(fts, bases, ALPHAS[:k], bo, density=density, lam=lam, normalize=normalize, want_delta=True)
        assert torch.equal(raw(out), raw(t_out)) and torch.equal(raw(delta), raw(t_delta)), (k, density)
        assert rep.k_keep == t_rep.k_keep and rep.kept == t_rep.kept
        assert [f32_bits(t) for t in rep.thresholds] == [f32_bits(t) for t in t_rep.thresholds]


def check_nested_in_consensus_k(engine, device="cpu"):
    """the selected sets are nested: wherever the delta at consensus_k + 1 is nonzero it equals the delta at consensus_k"""
    for ties in FLAVOURS:
        for k in (3, 5):
            fts, bases, bo = make_inputs(SHAPE, k, seed=110 + k, own_bases=True, device=device)
            deltas, selected = [], []
            for ck in range(1, k + 1):
                _, rep, delta = engine.consensus_merge(fts, bases, ALPHAS[:k], bo, ties=ties, consensus_k=ck, want_delta=True)
                deltas.append(raw(delta))
                selected.append(rep.selected)
            assert selected == sorted(selected, reverse=True) and selected[0] > selected[-1] > 0, selected
            for lo, hi in zip(deltas, deltas[1:]):
                nz = hi != 0
                assert torch.equal(hi[nz], lo[nz])


def check_arguments(engine, device="cpu"):
    fts, bases, bo = make_inputs((8, 8), 2, seed=91, device=device)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="density"):
            engine.consensus_merge(fts, bases, [0.5, 0.5], bo, ties=True, density=bad)
        engine.consensus_merge(fts, bases, [0.5, 0.5], bo, ties=False, density=bad)        # consensus_ta takes no density
    for bad in (-0.1, 1e7, float("nan")):
        with pytest.raises(ValueError, match="mask_lambda"):
            engine.consensus_merge(fts, bases, [0.5, 0.5], bo, mask_lambda=bad)
    for bad in (0, 17, 2.0, True):
        with pytest.raises(ValueError, match="consensus_k"):
            engine.consensus_merge(fts, bases, [0.5, 0.5], bo, consensus_k=bad)
    with pytest.raises(ValueError, match="lam"):
        engine.consensus_merge(fts, bases, [0.5, 0.5], bo, lam=float("inf"))
    with pytest.raises(ValueError, match="shape mismatch"):
        engine.consensus_merge([fts[0], fts[1][:4]], bases, [0.5, 0.5], bo)
    with pytest.raises(ValueError, match="supported range"):
        engine.consensus_merge([fts[0]] * 17, [bases[0]] * 17, [0.1] * 17, bo)
    with pytest.raises(ValueError, match="alphas"):
        engine.consensus_merge(fts, bases, [0.5], bo)


CORNERS = [check_unaligned, check_bases, check_signed_alphas, check_tiny_weight_sum, check_zero_deltas, check_denormals,
           check_tied_finetunes, check_nonfinite, check_tiny_and_rank3, check_determinism, check_ta_is_dare_linear, check_ties_is_ties,
           check_nested_in_consensus_k, check_arguments]


# ---- profile names and launches ----------------------------------------------------------------------------
PROFILES = [(False, 2, {"consensus_merge": 1}), (False, 5, {"consensus_merge": 1}),
            (True, 2, {"ties_hist": 3, "ties_select": 3, "consensus_merge": 1}),
            (True, 5, {"ties_hist": 6, "ties_select": 3, "consensus_merge": 1})]
PROFILE_IDS = ["ta-k2", "ta-k5", "ties-k2", "ties-k5"]


def check_profile(engine, ties, k, expected, shape=(40, 50), device="cpu"):
    """one fused launch; the TIES flavour adds exactly the selection launches that ties_merge makes at the same k"""
    fts, bases, bo = make_inputs(shape, k, seed=6, device=device)
    got = profile_of(engine, lambda: engine.consensus_merge(fts, bases, ALPHAS[:k], bo, ties=ties, density=0.5))
    assert got == expected, got
    if ties:
        of_ties = profile_of(engine, lambda: engine.ties_merge(fts, bases, ALPHAS[:k], bo, density=0.5))
        assert {n: c for n, c in got.items() if n != "consensus_merge"} == {n: c for n, c in of_ties.items() if n != "ties_merge"}


# ---- the C ABI ------------------------------------------------------------------------------------------------
def check_c_abi(engine, device="cpu"):
    from shardmerge_amd import _lib
    x = torch.zeros(64, dtype=torch.bfloat16, device=device)
    y = torch.zeros(64, dtype=torch.bfloat16, device=device)
    out = torch.zeros(64, dtype=torch.bfloat16, device=device)
    dll, h = engine.lib.dll, engine.ctx.h

    def call(k=1, density=0.2, ties=0, mask_lambda=0.4, consensus_k=2, out_t=out, n=64, in_dtype=_lib.BF16, lam=1.0, alpha=0.5):
        d = _lib.ConsensusDesc()
        d.k = k
        for i in range(max(0, min(k, 16))):
            d.finetune[i], d.base[i], d.alpha[i] = x.data_ptr(), y.data_ptr(), alpha
        d.in_dtype, d.base_out, d.base_out_dtype, d.n = in_dtype, y.data_ptr(), _lib.BF16, n
        d.density, d.lam, d.normalize = density, lam, 1
        d.mask_lambda, d.consensus_k, d.ties = mask_lambda, consensus_k, ties
        rep = _lib.ConsensusReport()
        rc = dll.smhip_consensus_merge(h, C.byref(d), out_t.data_ptr(), None, C.byref(rep), None)
        return rc, dll.smhip_last_error(h).decode(), rep

    rc, msg, rep = call()
    assert rc == _lib.OK and rep.selected == 64 and rep.agree[1] == 64 and rep.masked[0] == 64 and rep.k_keep == 0, msg
    rc, msg, rep = call(ties=1, density=0.5)
    assert rc == _lib.OK and rep.k_keep == 32 and rep.selected == 64, msg
    assert call(ties=0, density=0.0)[0] == _lib.OK              # consensus_ta reads no density
    for kwargs, word in (({"k": 0}, "k out of range"), ({"k": 17}, "k out of range"), ({"consensus_k": 0}, "consensus_k"),
                         ({"consensus_k": 17}, "consensus_k"), ({"mask_lambda": -0.1}, "mask_lambda"),
                         ({"mask_lambda": float("nan")}, "mask_lambda"), ({"mask_lambda": 1.0000001e6}, "mask_lambda"),
                         ({"ties": 1, "density": 0.0}, "density"), ({"ties": 1, "density": 1.01}, "density"),
                         ({"ties": 1, "density": float("nan")}, "density"), ({"lam": float("inf")}, "lambda"),
                         ({"lam": float("nan")}, "lambda"), ({"alpha": float("nan")}, "alpha"), ({"out_t": x}, "overlaps"),
                         ({"in_dtype": 3}, "dtype")):
        rc, msg, _ = call(**kwargs)
        assert rc == _lib.ERR_ARG and word in msg, (kwargs, rc, msg)
    rc = dll.smhip_consensus_merge(h, None, out.data_ptr(), None, None, None)
    assert rc == _lib.ERR_ARG and "null descriptor" in dll.smhip_last_error(h).decode()
    assert call(n=0, out_t=x)[0] == _lib.OK                     # a no-op, whatever the pointers


# ---- the CLI on the synthetic on-disk model of tests/lora_fixtures.py ----------------------------------------
def options(operator):
    opts = {"operator": operator, "mask_lambda": 0.6, "consensus_k": 2, "consensus_lambda": 0.7}
    if operator == "consensus_ties":
        opts["density"] = 0.3
    return opts


def write_config(root, third, out_dir, opts, device=None):
    return harness.write_config(root, ties_models(third), out_dir, opts, device)


def expected_outputs(base, full, opts):
    """the oracle tensor by tensor (block tensors) / the provider's tensor (passthrough); the models of ties_models:
    layer 0 has three entries, layer 1 two"""
    def merge(fts, bases, alphas, base_out, name):
        return consensus_oracle.consensus_merge(
            fts, bases, alphas, base_out, ties=opts["operator"] == "consensus_ties", density=opts.get("density", 0.2),
            mask_lambda=opts.get("mask_lambda", 0.4), consensus_k=opts.get("consensus_k", 2), lam=opts.get("consensus_lambda", 1.0),
            normalize=bool(opts.get("consensus_normalize", 1)))["out"]

    return expected_by_tensor(base, full, ties_models("org/lora_full"), merge)
