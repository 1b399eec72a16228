"""Checks of the DARE operators shared by the emulator tier (tests/test_dare_host.py) and the GPU tier
(tests/test_dare_gpu.py): Engine.dare_merge against tests/dare_oracle.py, BIT FOR BIT - output, merged delta, T and
kept counts.  The tolerance is zero and it is derived, not measured: every step of the function is an integer function
or one correctly rounded fp32 operation (include/shardmerge_hip.h, smhip_dare_merge)."""
import math

import pytest
import torch

from tests import dare_oracle
from tests import harness
from tests.harness import ALPHAS, DTYPES, SMALL, covering, expected_by_tensor, layer_of, make_inputs, raw, ties_models

DENSITIES = (1.0, 0.5, 0.2, 0.01, 2.0 ** -16)   # the last one: T = 1, the smallest density there is
MODES = (True, False)                           # sign_election: dare_ties, dare_linear
KEY = 0x0123456789ABCDEF
# one 2^20-element statistics check: the key and the streams were fixed after the CPU oracle passed with them (the
# mask is deterministic: the check passes always or never)
STAT_KEY, STAT_STREAMS, STAT_N = (456 << 32) | 123, (3, 4), 1 << 20


def mode_name(sign_election):
    return "dare_ties" if sign_election else "dare_linear"


def check(engine, fts, bases, alphas, base_out, density=0.2, lam=1.0, normalize=True, rescale=True, sign_election=True,
          key=KEY, stream_ids=None, label=""):
    """one call against the oracle, bit for bit; returns the engine's report"""
    kw = dict(density=density, lam=lam, normalize=normalize, rescale=rescale, sign_election=sign_election, key=key,
              stream_ids=stream_ids)
    out, rep, delta = engine.dare_merge(fts, bases, alphas, base_out, want_delta=True, **kw)
    cpu = lambda ts: [t.cpu() for t in ts]
    ref, ref_delta, T, kept = dare_oracle.dare_merge(cpu(fts), cpu(bases), alphas, base_out.cpu(), **kw)
    print(f"{label}: T {rep.threshold} / {T}, kept {rep.kept} / {kept}")
    assert out.dtype == base_out.dtype and out.shape == base_out.shape, label
    assert rep.threshold == T and rep.density == T / 65536.0, (label, rep.threshold, T)
    assert rep.kept == kept, (label, rep.kept, kept)
    bad = int((raw(delta) != raw(ref_delta)).sum())
    assert bad == 0, f"{label}: {bad} of {ref_delta.numel()} merged-delta values differ in their bits"
    bad = int((raw(out) != raw(ref)).sum())
    assert bad == 0, f"{label}: {bad} of {ref.numel()} output values differ in their bits"
    return rep


# ---- the parameter grid -------------------------------------------------------------------------------
def check_dtypes(engine, in_dtype, bo_dtype, sign_election, device="cpu"):
    fts, bases, bo = make_inputs(SMALL, 3, in_dtype, bo_dtype, seed=11, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:3], bo, density=0.2, lam=0.7, sign_election=sign_election, label=f"{in_dtype}->{bo_dtype}")
    fts, bases, bo = make_inputs(SMALL, 2, in_dtype, bo_dtype, seed=12, device=device)      # one shared base
    check(engine, fts, bases, ALPHAS[:2], bo, density=0.5, normalize=False, sign_election=sign_election,
          label=f"{in_dtype}->{bo_dtype} shared")


def check_k_density(engine, k, density, sign_election, device="cpu"):
    for j, (lam, normalize) in enumerate(((1.0, True), (0.7, False))):
        fts, bases, bo = make_inputs(SMALL, k, seed=20 + k + j, own_bases=bool(j), device=device)
        rep = check(engine, fts, bases, ALPHAS[:k], bo, density=density, lam=lam, normalize=normalize, sign_election=sign_election,
                    stream_ids=list(range(3, 3 + k)), label=f"{mode_name(sign_election)} k={k} density={density} lam={lam} normalize={normalize}")
        assert rep.threshold == (65536 if density == 1.0 else math.floor(density * 65536))


def check_options(engine, lam, normalize, rescale, sign_election, device="cpu"):
    fts, bases, bo = make_inputs((64, 200), 3, seed=40, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:3], bo, lam=lam, normalize=normalize, rescale=rescale, sign_election=sign_election,
          label=f"lam={lam} normalize={normalize} rescale={rescale}")


def check_signed_alphas(engine, device="cpu"):
    for sign_election in MODES:
        for normalize in (True, False):
            fts, bases, bo = make_inputs(SMALL, 4, seed=50, own_bases=True, device=device)
            check(engine, fts, bases, [0.5, -0.3, 0.0, -0.7], bo, density=0.5, lam=0.7, normalize=normalize,
                  sign_election=sign_election, label="signed alphas")


# ---- corners ----------------------------------------------------------------------------------------------
def check_zero_delta(engine, device="cpu"):
    """a finetune equal to its base: nothing of it is kept, whatever the mask"""
    for sign_election in MODES:
        fts, bases, bo = make_inputs(SMALL, 2, seed=60, device=device)
        fts[1] = bases[1].clone()
        rep = check(engine, fts, bases, [0.5, 0.5], bo, density=0.3, sign_election=sign_election, label="zero delta")
        assert rep.kept[1] == 0 and rep.kept[0] > 0
        rep = check(engine, fts, bases, [0.5, 0.5], bo, density=1.0, sign_election=sign_election, label="zero delta, density 1")
        assert rep.kept[1] == 0


def check_tiny_weight_sum(engine, device="cpu"):
    """weights that make |D| < 1e-8: D is replaced by 1"""
    x = (torch.randn(SMALL, generator=torch.Generator().manual_seed(63)).abs() + 0.5).to(torch.bfloat16).to(device)
    zero = torch.zeros_like(x)
    bo = make_inputs(SMALL, 1, seed=64, device=device)[2]
    for sign_election in MODES:         # dare_ties: both entries agree (+), D = 0.5 - 0.5; dare_linear: D over all = 0
        check(engine, [x, -x], [zero, zero], [0.5, -0.5], bo, density=1.0, sign_election=sign_election, label="D = 0")
        _, _, delta = engine.dare_merge([x, -x], [zero, zero], [0.5, -0.5], bo, density=1.0, sign_election=sign_election, want_delta=True)
        assert torch.equal(delta.cpu(), x.float().cpu())              # 0.5 x + 0.5 x over D := 1
        check(engine, [x], [zero], [1e-9], bo, density=0.5, sign_election=sign_election, label="D = 1e-9")


def check_denormals(engine, device="cpu"):
    g = torch.Generator().manual_seed(66)
    ft = (torch.randn(SMALL, generator=g) * 1e-40).to(device)
    zero = torch.zeros_like(ft)
    for sign_election in MODES:
        check(engine, [ft, ft * 0.5], [zero, zero], [0.5, 0.75], zero, density=0.5, lam=0.7, sign_election=sign_election,
              label="fp32 denormal deltas")


def check_unaligned(engine, device="cpu"):
    """views that start at an odd element, and element counts that are not multiples of 8, n < 8 included"""
    for dtype in DTYPES:
        for n in (1003, 4096):
            fts, bases, bo = make_inputs((n + 5,), 3, dtype, seed=70, own_bases=True, device=device)
            cut = lambda t, o: t[o:o + n]
            check(engine, [cut(fts[0], 1), cut(fts[1], 3), cut(fts[2], 0)], [cut(bases[0], 0), cut(bases[1], 1), cut(bases[2], 5)],
                  ALPHAS[:3], cut(bo, 1), density=0.2, sign_election=dtype != torch.float16, label=f"unaligned {dtype} n={n}")
    for n in (1, 3, 7, 8, 9, 2049):
        for sign_election in MODES:
            fts, bases, bo = make_inputs((n,), 2, seed=71, device=device)
            check(engine, fts, bases, ALPHAS[:2], bo, density=0.5, sign_election=sign_election, label=f"n={n}")


def check_tiny_and_rank3(engine, device="cpu"):
    fts, bases, bo = make_inputs((0,), 2, seed=73, device=device)
    out, rep = engine.dare_merge(fts, bases, [0.5, 0.5], bo)
    assert out.numel() == 0 and out.dtype == bo.dtype and rep.threshold == 13107 and rep.kept == [0, 0]
    for sign_election in MODES:
        fts, bases, bo = make_inputs((4, 33, 65), 3, seed=74, own_bases=True, device=device)
        check(engine, fts, bases, ALPHAS[:3], bo, sign_election=sign_election, label="rank 3")


def check_nonfinite(engine, device="cpu"):
    """a NaN / an Inf in one finetune: ValueError naming the tensor and the finetune; the context stays usable"""
    for poison in (float("nan"), float("inf"), float("-inf")):
        fts, bases, bo = make_inputs(SMALL, 3, seed=80, device=device)
        fts[1] = fts[1].clone()
        fts[1].view(-1)[4321] = poison
        with pytest.raises(ValueError, match=r"model\.layers\.7\.mlp\.up_proj\.weight.*finetune 1\b"):
            engine.dare_merge(fts, bases, ALPHAS[:3], bo, density=0.01, layer_name="model.layers.7.mlp.up_proj.weight")
        fts, bases, bo = make_inputs(SMALL, 3, seed=81, device=device)
        check(engine, fts, bases, ALPHAS[:3], bo, label="after an error")
    # Inf - Inf in the delta although no delta element is Inf itself
    fts, bases, bo = make_inputs(SMALL, 2, torch.float32, seed=82, own_bases=True, device=device)
    fts[0].view(-1)[5] = float("inf")
    bases[0].view(-1)[5] = float("inf")
    with pytest.raises(ValueError, match=r"finetune 0\b"):
        engine.dare_merge(fts, bases, ALPHAS[:2], bo, sign_election=False)


def check_arguments(engine, device="cpu"):
    fts, bases, bo = make_inputs((8, 8), 2, seed=91, device=device)
    for bad in (0.0, -0.1, 1.5, float("nan"), 2.0 ** -17, math.nextafter(2.0 ** -16, 0.0)):
        with pytest.raises(ValueError, match="density"):
            engine.dare_merge(fts, bases, [0.5, 0.5], bo, density=bad)
    with pytest.raises(ValueError, match="shape mismatch"):
        engine.dare_merge([fts[0], fts[1][:4]], bases, [0.5, 0.5], bo)
    with pytest.raises(ValueError, match="supported range"):
        engine.dare_merge([fts[0]] * 17, [bases[0]] * 17, [0.1] * 17, bo)
    with pytest.raises(ValueError, match="alphas"):
        engine.dare_merge(fts, bases, [0.5], bo)
    with pytest.raises(ValueError, match="stream_ids"):
        engine.dare_merge(fts, bases, [0.5, 0.5], bo, stream_ids=[0])
    with pytest.raises(ValueError, match="stream_ids"):
        engine.dare_merge(fts, bases, [0.5, 0.5], bo, stream_ids=[0, 2 ** 32])
    for bad in (-1, 2 ** 64, 1.5, True):
        with pytest.raises(ValueError, match="key"):
            engine.dare_merge(fts, bases, [0.5, 0.5], bo, key=bad)


# ---- the two identities of the definition ---------------------------------------------------------------------
def check_density_one_is_ties(engine, device="cpu"):
    """dare_ties at density 1 (T = 65536, r = 1) is smhip_ties_merge at density 1, for any key"""
    for k, own, lam, normalize in ((3, True, 0.7, True), (5, False, 1.0, False), (1, False, 1.0, True)):
        fts, bases, bo = make_inputs(SMALL, k, seed=100 + k, own_bases=own, device=device)
        t_out, _, t_delta = engine.ties_merge(fts, bases, ALPHAS[:k], bo, density=1.0, lam=lam, normalize=normalize, want_delta=True)
        for key in (0, KEY, 2 ** 64 - 1):
            for rescale in (True, False):
                out, rep, delta = engine.dare_merge(fts, bases, ALPHAS[:k], bo, density=1.0, lam=lam, normalize=normalize, rescale=rescale,
                                                    sign_election=True, key=key, want_delta=True)
                assert rep.threshold == 65536
                assert torch.equal(raw(out), raw(t_out)) and torch.equal(raw(delta), raw(t_delta)), (k, key)


def check_nested_masks(engine, device="cpu"):
    """rescale = 0: the kept set at density 0.1 is a subset of the kept set at 0.3 (same key, same stream)"""
    fts, bases, bo = make_inputs((300, 500), 1, torch.float32, seed=110, device=device)
    call = lambda density: engine.dare_merge(fts, bases, [1.0], bo, density=density, normalize=False, rescale=False,
                                             sign_election=False, key=KEY, stream_ids=[5], want_delta=True)
    _, ra, a = call(0.1)
    _, rb, b = call(0.3)
    a, b = raw(a), raw(b)
    nz = a != 0
    assert 0 < ra.kept[0] < rb.kept[0]
    assert int(nz.sum()) == ra.kept[0] and int((b != 0).sum()) == rb.kept[0]
    assert torch.equal(a[nz], b[nz])


# ---- the mask is a function of (key, stream, index) only --------------------------------------------------
def check_determinism(engine, device="cpu"):
    fts, bases, bo = make_inputs((300, 500), 3, seed=90, own_bases=True, device=device)
    a, ra = engine.dare_merge(fts, bases, ALPHAS[:3], bo, key=KEY)
    b, rb = engine.dare_merge(fts, bases, ALPHAS[:3], bo, key=KEY)
    assert torch.equal(raw(a), raw(b)) and ra == rb


def check_slices(engine, device="cpu"):
    """the result of the first m elements does not depend on what follows them: another grid, the same mask"""
    n = 70000
    fts, bases, bo = make_inputs((n,), 2, seed=120, own_bases=True, device=device)
    for sign_election in MODES:
        full, _, fd = engine.dare_merge(fts, bases, ALPHAS[:2], bo, sign_election=sign_election, key=KEY, want_delta=True)
        for m in (8, 4096, 33333, 69999):
            cut = lambda ts: [t[:m] for t in ts]
            part, _, pd = engine.dare_merge(cut(fts), cut(bases), ALPHAS[:2], bo[:m], sign_election=sign_election, key=KEY, want_delta=True)
            assert torch.equal(raw(part), raw(full[:m])) and torch.equal(raw(pd), raw(fd[:m])), m


def check_streams_and_keys(engine, device="cpu"):
    """another stream id, another key: another mask; two finetunes with the same delta keep different sets"""
    fts, bases, bo = make_inputs((300, 500), 1, torch.float32, seed=130, device=device)
    call = lambda key, sid: raw(engine.dare_merge(fts, bases, [1.0], bo, density=0.5, normalize=False, rescale=False, sign_election=False,
                                                  key=key, stream_ids=[sid], want_delta=True)[2]) != 0
    ref = call(KEY, 0)
    n = ref.numel()
    for other in (call(KEY, 1), call(KEY + 1, 0), call(KEY ^ (1 << 63), 0)):
        differ = int((ref != other).sum())
        assert abs(differ / n - 0.5) < 6 * math.sqrt(0.25 / n), differ         # independent masks at density 1/2 differ in half
    # the same delta twice, streams 0 and 1: the merged delta is d where exactly one kept it, 2 d where both did
    d = (fts[0] - bases[0]).cpu()
    _, rep, delta = engine.dare_merge([fts[0], fts[0]], [bases[0], bases[0]], [1.0, 1.0], bo, density=0.5, normalize=False, rescale=False,
                                      sign_election=False, key=KEY, stream_ids=[0, 1], want_delta=True)
    m0, m1 = call(KEY, 0), call(KEY, 1)
    assert not torch.equal(m0, m1)
    zero = torch.zeros((), dtype=d.dtype)
    expect = torch.where(m0.view(d.shape), d, zero) + torch.where(m1.view(d.shape), d, zero)
    assert torch.equal(raw(delta), raw(expect))
    assert rep.kept == [int(m0.sum()), int(m1.sum())]


def check_statistics(engine, density, device="cpu"):
    """2^20 non-zero deltas: kept / n within 6 sigma of q = T / 65536, the overlap of two streams within 6 sigma of q^2"""
    n = STAT_N
    g = torch.Generator().manual_seed(140)
    d = (torch.rand(n, generator=g) + 0.5).to(device)          # no zero among them
    zero = torch.zeros_like(d)
    T = dare_oracle.threshold(density)
    q = T / 65536.0
    kept = []
    for sid in STAT_STREAMS:
        _, rep, delta = engine.dare_merge([d], [zero], [1.0], zero, density=density, normalize=False, rescale=False, sign_election=False,
                                          key=STAT_KEY, stream_ids=[sid], want_delta=True)
        m = delta.cpu() != 0
        assert rep.threshold == T and rep.kept == [int(m.sum())]
        assert torch.equal(m, dare_oracle.mask(STAT_KEY, sid, n, T))
        bound = 6 * math.sqrt(q * (1 - q) / n)
        print(f"density {density}: stream {sid} kept {rep.kept[0] / n:.7f}, q {q:.7f}, bound {bound:.3g}")
        assert abs(rep.kept[0] / n - q) <= bound
        kept.append(m)
    overlap = int((kept[0] & kept[1]).sum()) / n
    bound = 6 * math.sqrt(q * q * (1 - q * q) / n)
    print(f"density {density}: overlap {overlap:.7f}, q^2 {q * q:.7f}, bound {bound:.3g}")
    assert abs(overlap - q * q) <= bound


# ---- the CLI on the synthetic on-disk model of tests/lora_fixtures.py ----------------------------------------
def options(operator):
    return {"operator": operator, "density": 0.3, "dare_lambda": 0.7, "seed": 2 ** 62 + 12345}


def dare_models(third):
    """ties_models: layer 0: all three entries; layer 1: entries 0 and 2 (entry 1's window ends at layer 0), so on layer 1
    the third entry is the SECOND covering finetune while its stream id stays 2"""
    return ties_models(third)


def stream_ids(models, name):
    """a finetune's stream id is its position among ALL the entries, whichever of them cover the tensor's layer"""
    return [i for i, _ in covering(models, layer_of(name))]


def write_config(root, third, out_dir, opts, device=None):
    return harness.write_config(root, dare_models(third), out_dir, opts, device)


def expected_outputs(base, full, opts):
    """the oracle tensor by tensor (block tensors) / the provider's tensor (passthrough)"""
    models = dare_models("org/lora_full")
    def merge(fts, bases, alphas, base_out, name):
        return dare_oracle.dare_merge(
            fts, bases, alphas, base_out, density=opts.get("density", 0.2), lam=opts.get("dare_lambda", 1.0),
            normalize=bool(opts.get("dare_normalize", 1)), rescale=bool(opts.get("dare_rescale", 1)),
            sign_election=opts["operator"] == "dare_ties", key=dare_oracle.tensor_key(opts.get("seed", 0), name),
            stream_ids=stream_ids(models, name))[0]

    return expected_by_tensor(base, full, models, merge)
