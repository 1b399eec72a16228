"""Per-bin conformance of the 2-D transform and of the merge-only transform paths, shared by the two tiers:

  * tests/test_transform_host.py (no GPU): the kernel bodies in the CPU work-group emulator (tests/emul);
  * tests/test_transform_gpu.py (-m gpu): the same checks through libshardmerge_hip.so on a real MI355X;
  * tools/transform_report.py prints what the checks measure (profiles/transform_conformance*.txt).

The criterion.  The reference of an fp32 input x, used exactly as given, is torch.fft.fftn(x.double());
of a spectrum s it is ifftn(s.to(complex128)).real.  For an implementation `impl`

    e(impl, x) = max_k max(0, |impl(x)_k - ref_k| - 2^-22 |ref_k|) / scale(x)

scale = ||x||_1 for sparse inputs (impulses), sqrt(n) ||x||_2 for dense ones; for the inverse ||s||_1 / n and
||s||_2 / sqrt(n); for the round trip ifft(fft(x)) - x the inverse's dense scale of x's spectrum, ||x||_2.  The
2^-22 |ref_k| term lets a bin be off by four fp32 ulps of its own magnitude (else the DC bin of an input with a large
mean decides everything); the sparse families of the plain transforms go without it (ALLOWANCE).

NO tolerance is a literal: for each shape and family E_ref is the maximum over the family's inputs of
e(torch's fp32 FFT, x), computed on the spot, and every input must meet e(kernel, x) <= MARGIN * E_ref.
MARGIN = 4 is two bits: two correct fp32 FFTs of different factorisations (radix 16 / 32 stages and an r2c post-step
here, radix 4 / 5 and generic passes in pocketfft) differ by small factors either way; a short-rounded or drifting
twiddle table costs four bits or more.

The merge-only paths (the folded kernels, k_dftp, the transposed merge, the batched rank-3 passes, the R = 1 column
kernels of 1-D tensors) are reached through Engine.merge_layer([d, 0], [0, 0], ...): the second delta is exactly
zero, the Arithmetic-FFT branch runs and (quirk Q3) leaves i * Im F_d, i.e. the odd part of d, times target_norm / ||d||.  The closed form is evaluated in fp64
with the scalar of the ORACLE's trace; E_ref is the per-element error of the fp32 oracle (oracle/spectral_oracle.py)
against that closed form on the same inputs.

Known limit.  The closed form discards the Re plane after the blend: a defect confined to the Re output of the last
forward stage of a merge-only kernel stays covered by the noise-based parity tests only.  Of the folded kernels the
K = 2 arithmetic branch launches KF1Q, KF2Q and KI1x2Q; KF2SQ (the single-signal column pass of K >= 3 SLERP rounds) and
KI1x1Q (512-thread column plans, which no folded shape has) are not on its way, and neither is k_pair1d, which is a
SLERP pair merge: those three stay with the noise-based tests.
"""
import math

import torch

from oracle import spectral_oracle as so

MARGIN = 4.0
ULPS4 = 2.0 ** -22
# family -> the allowance where it is not ULPS4.  The transform of ONE impulse (one spectral bin) has the magnitude of the
# scale in every bin, so no bin can decide everything, and torch's own error stays below four ulps there: with the
# allowance E_ref comes out as 0 (it did at 1024, 2048, 3072, 3584, 2304, ...) and a multiple of it says nothing.  The
# sparse families therefore compare the plain errors, max |impl - ref| / scale, with the same margin.
ALLOWANCE = {"sparse": 0.0, "inv_sparse": 0.0}

# SM_STATIC_PLANS of shardmerge_amd/csrc/sm_plans.hpp, restated (the library does not list them; every one must be
# length_supported: test_transform_host.py)
STATIC_LENGTHS = (1024, 2048, 4096, 8192, 16384, 14336, 28672, 3072, 3584, 5120, 6144, 7168, 12288, 13824, 27648, 2304,
                  256, 512, 64, 128)
RUNTIME_LENGTHS = (1408, 832, 1536, 2560, 96)          # 11 * 128, 13 * 64, ...: planned at run time
CHIRP_SHAPES = ((2, 34), (2, 1136), (2, 4544))         # row lengths without a plan: the chirp-z row passes
ONE_D_SHAPES = ((4096,), (77,), (1, 64))
MISALIGNED_LENGTHS = (1024, 28672)
PACKED_FLAGS = ("-DSM_ROW_PACK_BIG=2", "-DSM_I1_PACK=2", "-DSM_F1Q_PACK=2", "-DSM_F2_PACK=2", "-DSM_F2S_PACK=2",
                "-DSM_ROW_PACK_MAX_T=0")               # the build of test_complex_packed_engine_mode
PACKED_LENGTHS = (8192, 14336, 7168, 3072, 5120, 13824, 2304, 1408)


def fn_shapes():
    """[(shape, tested axis)] of section 3: every static length and the run-time planned ones in both orientations,
    the chirp-z row lengths, the 1-D tensors"""
    out = []
    for n in STATIC_LENGTHS + RUNTIME_LENGTHS:
        out += [((2, n), 1), ((n, 2), 0)]
    out += [(s, 1) for s in CHIRP_SHAPES]
    out += [(s, len(s) - 1) for s in ONE_D_SHAPES]
    return out


def shape_id(shape):
    return "x".join(map(str, shape))


# ---- the criterion ------------------------------------------------------------------------------------------------
def excess(got: torch.Tensor, ref: torch.Tensor, scale: float, family: str = "") -> float:
    """e(impl, x) of the module docstring; got: the implementation's output, ref: the fp64 reference"""
    got = got.detach().cpu()
    got = got.to(torch.complex128) if got.is_complex() else got.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    over = ((got - ref).abs() - ALLOWANCE.get(family, ULPS4) * ref.abs()).clamp_(min=0)
    worst = float(over.max())
    assert math.isfinite(worst), "non-finite output"
    return worst / scale


def ref_fft(x):
    x = x.double()
    return torch.fft.fft(x) if x.ndim == 1 else torch.fft.fftn(x, dim=(-2, -1))


def ref_ifft(s):
    s = s.to(torch.complex128)
    return (torch.fft.ifft(s) if s.ndim == 1 else torch.fft.ifftn(s, dim=(-2, -1))).real


def l1(t):
    return float(t.abs().double().sum())


def l2(t):
    return float(t.abs().double().pow(2).sum().sqrt())


def pooled(records):
    """[(family, name, e_kernel, e_ref)] -> {family: (worst e_kernel, E_ref)}"""
    out = {}
    for fam, _, ek, er in records:
        a, b = out.get(fam, (0.0, 0.0))
        out[fam] = (max(a, ek), max(b, er))
    return out


def assert_records(records, what, margins=None):
    """every input of a family within MARGIN * E_ref, E_ref the family's maximum of the reference implementation's e;
    margins: {family: its own stated margin} of the one case that has one (direct_sum_margin)"""
    pool = pooled(records)
    margin = lambda fam: (margins or {}).get(fam, MARGIN)
    for fam, name, ek, er in records:
        print(f"{what} {fam:9s} {name:24s} e(kernel) {ek:.3e}  e(ref) {er:.3e}  E_ref {pool[fam][1]:.3e}")
    bad = [(fam, name, ek, pool[fam][1]) for fam, name, ek, _ in records if not ek <= margin(fam) * pool[fam][1]]
    assert not bad, f"{what}: e(kernel) > margin * E_ref for (family, input, e(kernel), E_ref) = {bad}"


# ---- inputs: computed in fp64, rounded once; the rounded tensor is the input of both sides -------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, g):
    return torch.randn(shape, generator=g, dtype=torch.float64)


def tone_frequencies(n):
    fs = []
    for f in (1, 37 if n >= 100 else 3, n // 4, n // 2 - 1):
        if 0 < f < n and f not in fs:
            fs.append(f)
    return fs


def impulse_indices(n, seed):
    idx = [i for i in (1, 2, 3, 5, 7, 16, 17, n // 2, n // 2 + 1, n - 1) if 0 <= i < n]
    idx += [int(i) for i in torch.randint(0, n, (4,), generator=_gen(seed))]
    return sorted(set(idx))


def sparse_inputs(shape, axis, seed):
    """unit impulses along the tested axis; the other index is 1 (0 where that axis has one entry)"""
    out = []
    for i in impulse_indices(shape[axis], seed):
        x = torch.zeros(shape, dtype=torch.float32)
        pos = [min(1, s - 1) for s in shape]
        pos[axis] = i
        x[tuple(pos)] = 1.0
        out.append((f"impulse@{i}", x))
    return out


def noise_inputs(shape, seed):
    """the four noise members of the dense family: Gaussian, large mean, heavy-tailed, bf16-rounded"""
    g = _gen(seed)
    noise = _randn(shape, g)
    mean = 1.0 + 0.003 * _randn(shape, g)
    heavy = _randn(shape, g)
    n = heavy.numel()
    hit = torch.randperm(n, generator=g)[:max(1, n // 1000)]                  # 0.1 % of the entries, at least one
    heavy.view(-1)[hit] *= 100.0
    bf16 = _randn(shape, g).to(torch.bfloat16)
    return [("noise", noise.float()), ("mean", mean.float()), ("heavy", heavy.float()), ("bf16", bf16.float())]


def dense_inputs(shape, axis, seed):
    """real tones along the tested axis (every bin away from +-f must stay under the tolerance: leakage) with the
    amplitudes 1, 1/2, ... along the other axis, then the noise members"""
    n = shape[axis]
    view = [1] * len(shape)
    view[axis] = n
    idx = torch.arange(n, dtype=torch.float64).view(view)
    amp = torch.ones(shape, dtype=torch.float64)
    if len(shape) == 2:
        other = torch.arange(shape[1 - axis], dtype=torch.float64)
        amp = amp * (0.5 ** other).view([-1, 1] if axis == 1 else [1, -1])
    out = []
    for f in tone_frequencies(n):
        ph = 2.0 * math.pi * f * idx / n
        out.append((f"cos{f}", (torch.cos(ph) * amp).float()))
        out.append((f"sin{f}", (torch.sin(ph) * amp).float()))
    return out + noise_inputs(shape, seed)


def _positions(shape, seed):
    """spectral bins for the single-bin inverse: the self-conjugate ones, then others"""
    if len(shape) == 1:
        n = shape[0]
        pos = [(0,), (n // 2,), (1 % n,), (n - 1,), (n // 3,)]
        pos += [(int(i),) for i in torch.randint(0, n, (2,), generator=_gen(seed))]
    else:
        r, c = shape
        pos = [(0, 0), (r // 2, 0), (0, c // 2), (r // 2, c // 2), (1 % r, 1 % c), (r - 1, c - 1), (r // 3, (c // 3 + 1) % c)]
        g = _gen(seed)
        pos += [(int(torch.randint(0, r, (1,), generator=g)), int(torch.randint(0, c, (1,), generator=g))) for _ in range(2)]
    seen, out = set(), []
    for p in pos:
        if p not in seen:
            seen.add(p)
            out.append(p)
    return out


def inverse_sparse_inputs(shape, seed):
    out = []
    for p in _positions(shape, seed):
        s = torch.zeros(shape, dtype=torch.complex64)
        s[p] = 1.0 + 2.0j
        out.append(("bin@" + ",".join(map(str, p)), s))
    return out


def inverse_dense_inputs(shape, seed):
    g = _gen(seed)
    gauss = torch.complex(_randn(shape, g), _randn(shape, g)).to(torch.complex64)            # not Hermitian
    herm = ref_fft(_randn(shape, g).float()).to(torch.complex64)
    for p in _positions(shape, seed)[:2 if len(shape) == 1 else 4]:                        # the self-conjugate bins
        herm[p] = herm[p].real + 1j * (0.5 + herm[p].real.abs())
    return [("gauss", gauss), ("herm+imag", herm)]


# ---- section 3: fft_transform / ifft_transform -----------------------------------------------------------------------
BATCH = 16          # the other length of a batched call: one input of the family per row (column)
BATCH_FROM = 1024   # the emulator tier batches from this length on (one work-group per bin column, tens of us each)


def emulator_batched(shape, axis):
    return len(shape) == 2 and min(shape) > 1 and shape[axis] >= BATCH_FROM


def _stacked(lines, n, axis, name):
    """[(name, (n,) line)] -> one [BATCH x n] (axis 1) or [n x BATCH] (axis 0) tensor, line i at the other index i"""
    assert len(lines) <= BATCH
    x = torch.zeros((BATCH, n), dtype=lines[0][1].dtype)
    for i, (_, line) in enumerate(lines):
        x[i] = line
    return [(name, x if axis == 1 else x.T.contiguous())]


def family_inputs(shape, axis, seed, batched):
    """{family: [(input, tensor)]}.  batched (2-D shapes only): members of like scale share ONE tensor, [BATCH x n] or
    [n x BATCH] with one member per row (column) - the impulses, the tones, the Gaussian and the bf16 noise - and the
    single spectral bins share one spectrum; the reference is the fp64 transform of the same tensor, so the check is
    unchanged.  The large-mean and the heavy-tailed input keep a call of their own: in a shared tensor their norm would
    set the scale the tones' leakage bins are judged by."""
    if not batched:
        return {"sparse": sparse_inputs(shape, axis, seed), "dense": dense_inputs(shape, axis, seed),
                "inv_sparse": inverse_sparse_inputs(shape, seed + 1), "inv_dense": inverse_dense_inputs(shape, seed + 2)}
    n = shape[axis]
    full = (BATCH, n) if axis == 1 else (n, BATCH)
    bins = torch.zeros(full, dtype=torch.complex64)
    for p in _positions(full, seed + 1):
        bins[p] = 1.0 + 2.0j
    lines = dense_inputs((n,), 0, seed)
    pick = lambda names: [m for m in lines if m[0] in names]
    tones = [m for m in lines if m[0][:3] in ("cos", "sin")]
    own = [m for m in dense_inputs(shape, axis, seed) if m[0] in ("mean", "heavy")]
    return {"sparse": _stacked(sparse_inputs((n,), 0, seed), n, axis, "impulses"),
            "dense": _stacked(tones, n, axis, "tones") + _stacked(pick(("noise", "bf16")), n, axis, "noise+bf16") + own,
            "inv_sparse": [("bins", bins)], "inv_dense": inverse_dense_inputs(full, seed + 2)}


def transform_records(fft, ifft, shape, axis, seed=None, place=lambda t: t, batched=False):
    """[(family, input, e(kernel), e(torch fp32))] of one shape.  fft / ifft: the implementation under test (tensor ->
    tensor); place: how an input reaches it (the misaligned views)"""
    seed = seed if seed is not None else 7919 * shape[axis] + axis
    inputs = family_inputs(shape, axis, seed, batched)
    rec = []
    for fam in ("sparse", "dense"):
        for name, x in inputs[fam]:
            ref = ref_fft(x)
            scale = l1(x) if fam == "sparse" else math.sqrt(x.numel()) * l2(x)
            spec = fft(place(x))
            rec.append((fam, name, excess(spec, ref, scale, fam), excess(so.fft_transform(x), ref, scale, fam)))
            if fam == "dense":                                     # the round trip ifft(fft(x)) - x
                rec.append(("roundtrip", name, excess(ifft(spec), x.double(), l2(x)),
                            excess(so.ifft_transform(so.fft_transform(x)), x.double(), l2(x))))
    for fam in ("inv_sparse", "inv_dense"):
        for name, s in inputs[fam]:
            ref = ref_ifft(s)
            scale = l1(s) / s.numel() if fam == "inv_sparse" else l2(s) / math.sqrt(s.numel())
            rec.append((fam, name, excess(ifft(place(s)), ref, scale, fam), excess(so.ifft_transform(s), ref, scale, fam)))
    return rec


def engine_records(engine, shape, axis, place=lambda t: t, batched=False):
    return transform_records(engine.fft_transform, engine.ifft_transform, shape, axis, place=place, batched=batched)


def check_transforms(engine, shape, axis, batched=False):
    assert_records(engine_records(engine, shape, axis, batched=batched), f"{shape_id(shape)}")


def misaligned_on(engine):
    """place(): the same values in a contiguous view of the engine's device that is not 16-byte aligned (8 bytes in),
    as test_misaligned_inputs_take_the_elementwise_path builds it.  That such a view takes the element-wise, run-time
    planned kernels is the host's decision (aligned16() in run_f1 / run_inverse, sm_pipeline.hpp); those kernels carry
    the profile names of the vector ones and in the emulator compute the same bits, so nothing the library reports can
    show which ran - this case holds the result of such a call to the bound, whichever kernel produced it."""
    def place(t):
        flat = torch.view_as_real(t).reshape(-1) if t.is_complex() else t.reshape(-1)
        big = torch.zeros(flat.numel() + 2, dtype=flat.dtype, device=engine.device)
        big[2:] = flat.to(engine.device)
        v = big[2:]
        v = torch.view_as_complex(v.view(-1, 2)) if t.is_complex() else v
        v = v.view(t.shape)
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
        return v
    return place


def check_misaligned_transforms(engine, n, batched=False):
    for shape, axis in (((2, n), 1), ((n, 2), 0)):
        assert_records(engine_records(engine, shape, axis, place=misaligned_on(engine), batched=batched),
                       f"misaligned {shape_id(shape)}")


# ---- section 4: the merge-only paths through the arithmetic-branch closed form ------------------------------------------
FOLDED_SHAPES = ((8192, 128), (14336, 128), (16384, 128), (28672, 128))        # C = 128: the smallest fold_shape accepts
UNHOOKED_DEVICE_SHAPES = ((28672, 128), (14336, 128))


def _as3(shape):
    """(batch, R, C) of a 1-D, 2-D or rank-3 shape; a 1-D tensor is one column of R entries here"""
    if len(shape) == 1:
        return 1, shape[0], 1
    if len(shape) == 2:
        return 1, shape[0], shape[1]
    return shape


def _mirror(d):
    """d[-r, -c] per slice (d[-i] for a 1-D tensor)"""
    dims = (0,) if d.ndim == 1 else (-2, -1)
    return torch.roll(torch.flip(d, dims=dims), shifts=[1] * len(dims), dims=dims)


def merge_inputs(shape, seed):
    """{family: [(name, fp32 field)]}: the families of section 2 as fields of `shape` (every slice of a rank-3 shape its
    own), one exactly even field (its exact result is zero) and five impulses"""
    b, r, c = _as3(shape)
    i = torch.arange(r, dtype=torch.float64).view(1, r, 1)
    j = torch.arange(c, dtype=torch.float64).view(1, 1, c)
    sl = torch.arange(b, dtype=torch.float64).view(b, 1, 1)
    amp = 0.5 ** sl
    phase = lambda f: 2.0 * math.pi * ((f + sl) * i / r + 5.0 * j / c)          # slice s: frequency f + s
    dense = []
    for f in tone_frequencies(r):
        dense.append((f"cos{f}", torch.cos(phase(f)) * amp))
        dense.append((f"sin{f}", torch.sin(phase(f)) * amp))
    dense += [(name, x.double().view(b, r, c)) for name, x in noise_inputs((b, r, c), seed)]
    even = torch.cos(phase(37 if r > 37 else 3)) * amp
    dense.append(("even", 0.5 * (even + _mirror(even))))                       # exactly even in fp64 and after rounding
    sparse = []
    for p in ((1, 1), (r - 1, c - 1), (r // 4 + 1, 5), (3, c // 2), (r // 2 + 1, c // 2 + 1)):
        p = (p[0] % r, p[1] % c)
        x = torch.zeros((b, r, c), dtype=torch.float64)
        x[:, p[0], p[1]] = amp.view(b)
        sparse.append((f"impulse@{p[0]},{p[1]}" if c > 1 else f"impulse@{p[0]}", x))
    fin = lambda fam: [(name, x.float().view(shape).contiguous()) for name, x in fam]
    out = {"dense": fin(dense), "sparse": fin(sparse)}
    for fam in out.values():
        for name, x in fam:
            assert float(x.abs().max()) > 0, name
    return out


def arith_closed_form(d):
    """(expected merged delta in fp64, the oracle's merged delta, the oracle's trace, the scalar) of
    merge_layer([d, 0], [0, 0], ..)"""
    z = torch.zeros_like(d)
    tr = so.LayerTrace()
    with so.exact_norms():
        so.merge_layer([d, z], [z, z], [0.3, 0.5], z, trace=tr)
    assert tr.branches == ["arith"]
    scalar = tr.target_norm / tr.step_norms[0][0]                  # the oracle's a * (target_norm / ||a||)
    dd = d.double()
    return 0.5 * (dd - _mirror(dd)) * scalar, tr.merged_delta, tr, scalar


def engine_arith(engine, d, options=None):
    """(merged delta on the CPU, report, {kernel: launches}) of the engine's merge_layer([d, 0], [0, 0], ..) with the debug
    options {key: (value, value to restore)} set"""
    z = torch.zeros_like(d)
    options = options or {}
    for key, (value, _) in options.items():
        engine.ctx.debug_option(key, value)
    engine.ctx.profile(True)
    engine.ctx.profile_reset()
    try:
        out, rep, delta = engine.merge_layer([d, z], [z, z], [0.3, 0.5], z, want_delta=True, norm_mode="exact")
        delta = delta.cpu()
        table = engine.ctx.profile_table()
    finally:
        engine.ctx.profile(False)
        for key, (_, restore) in options.items():
            engine.ctx.debug_option(key, restore)
    assert rep.branches == ["arith"]
    return delta, rep, {name: table[name][0] for name in table if table[name][0]}


def check_report_norms(rep, tr):
    """the report's norms against the oracle's trace (exact norms on both sides): 2e-6 relative, what the fp32 norms of
    the trace and the reference's own fp32 arithmetic on them leave"""
    assert abs(rep.target_norm - tr.target_norm) <= 2e-6 * tr.target_norm
    assert abs(rep.delta_norms[0] - tr.step_norms[0][0]) <= 2e-6 * tr.step_norms[0][0] and rep.delta_norms[1] == 0.0


def merge_records(engine, shape, variants, seed=None):
    """variants: {label: debug options}.  -> ({label: [(family, input, e(kernel), e(oracle))]}, {label: {input: delta}},
    {label: launches of the last input})"""
    seed = seed if seed is not None else 104729 + sum(shape)
    rec = {v: [] for v in variants}
    deltas = {v: {} for v in variants}
    launches = {}
    for fam, inputs in merge_inputs(shape, seed).items():
        for name, d in inputs:
            expect, oracle_delta, tr, scalar = arith_closed_form(d)
            scale = scalar * (l1(d) if fam == "sparse" else l2(d))
            e_ref = excess(oracle_delta, expect, scale)
            for v, options in variants.items():
                delta, rep, launches[v] = engine_arith(engine, d, options)
                assert delta.shape == d.shape and delta.dtype == torch.float32
                check_report_norms(rep, tr)
                rec[v].append((fam, name, excess(delta, expect, scale), e_ref))
                deltas[v][name] = delta
    return rec, deltas, launches


def differ_in_bits(da, db):
    """two variants' deltas are not the same bits on at least one input: both paths ran"""
    return any(not torch.equal(da[name].view(torch.int32), db[name].view(torch.int32)) for name in da)


FOLD_ON = {"fold_min_rows": (8192, 0)}
FOLD_OFF = {"fold_min_rows": (8192, 0), "fold_columns": (0, 1)}


def check_folded(engine, shape):
    """the folded column pass (KF1Q, KF2Q, KI1x2Q) and the plain one on the same inputs: both meet the bound, and they are
    different code.  The folded kernels share their profile names with the plain ones, so the launch names below only
    show that the multi-kernel arithmetic path ran; that the FOLDED kernels ran is shown by the two variants' deltas
    differing in bits.  KF2SQ and KI1x1Q are not reachable from this branch (module docstring)."""
    rec, deltas, launches = merge_records(engine, shape, {"folded": FOLD_ON, "plain": FOLD_OFF})
    for v in rec:
        assert_records(rec[v], f"{shape_id(shape)} {v}")
        assert {"f1_rows_fwd", "f2_cols_fwd", "blend", "i1_cols_inv", "i2_rows_inv"} <= set(launches[v]), launches[v]
    assert differ_in_bits(deltas["folded"], deltas["plain"]), "fold_columns = 0 changed nothing: the folded path did not run"


def check_unhooked_folded(engine, shape):
    """the shapes that fold without any hook, as the product runs them"""
    rec, deltas, _ = merge_records(engine, shape, {"default": {}, "plain": {"fold_columns": (0, 1)}})
    for v in rec:
        assert_records(rec[v], f"{shape_id(shape)} {v}")
    assert differ_in_bits(deltas["default"], deltas["plain"]), "the default path of this shape is not the folded one"


def direct_sum_margin(p):
    """The one stated exception to MARGIN.  A column length p * M with p > DFTP_PAIR_MAX_P = 126 combines its
    p row blocks by DIRECT p-term fp32 sums (k_dftp), forward and inverse.  For an impulse all p terms of the inverse sum
    are coherent, and a sequential sum of p equal terms carries a relative rounding error of ~ 2^-24 sqrt(p) (measured
    on a plain fp32 model of the 167-term sum: rms 3.0e-7, max 1.4e-6), where the log2(p) levels of an FFT - the
    reference - carry ~ 2^-24 sqrt(log2 p).  The sparse family of such a shape is therefore held to
    sqrt(p / log2 p) times the reference's error, with one bit on top where MARGIN has two (the model already accounts
    for the difference between the two summations, which is most of what MARGIN's two bits are for):
    2 * sqrt(p / log2 p) = 9.5 at p = 167, against 4.2 measured on the device and 2.9 in the emulator.  At this shape
    the sparse family therefore sees a loss of about three and a half bits, not of two."""
    return 2.0 * math.sqrt(p / math.log2(p))


# (id, shape, {label: options}, kernels that must have run per label, labels whose bits must differ)
def path_cases():
    cases = []
    for p in (2, 4, 8):
        cases.append((f"force_split{p}", (256, 128), {"plain": {}, "split": {"force_split": (p, 0)}},
                      {"split": {"dft_across_slices"}}, ("plain", "split")))
    # k_dftp_pairs (p <= 126) and the generic k_dftp share a profile name: that the dftp_pairs hook switches kernels is
    # shown by the two variants' bits; 34 = 17 * 2, 76 = 19 * 4 (M > 2)
    for shape in ((34, 64), (76, 96)):
        cases.append((f"rough_column_{shape_id(shape)}", shape,
                      {"pairs": {"dftp_pairs": (1, 1)}, "single": {"dftp_pairs": (0, 1)}},
                      {"pairs": {"dft_across_slices"}, "single": {"dft_across_slices"}}, ("pairs", "single")))
    # 668 = 167 * 4: p > DFTP_PAIR_MAX_P, the generic kernel whatever the hook says - one variant
    cases.append(("rough_column_668x32", (668, 32), {"default": {}}, {"default": {"dft_across_slices"}}, None))
    cases.append(("transposed_64x34", (64, 34), {"default": {}}, {"default": {"transpose", "dft_across_slices"}}, None))
    cases.append(("both_rough_34x38", (34, 38), {"default": {}}, {"default": {"dft_across_slices"}}, None))
    cases.append(("force_bluestein_64x96", (64, 96), {"plain": {}, "chirp": {"force_bluestein": (1, 0)}}, {}, ("plain", "chirp")))
    cases.append(("rank3_3x64x128", (3, 64, 128), {"default": {}}, {"default": {"f2_cols_fwd", "i1_cols_inv"}}, None))
    # 1-D tensors, at the lengths the issue names for pair_1d: the arithmetic branch runs the R = 1 column kernels
    # (k_f2_r1, k_i1_r1) around the row passes.  k_pair1d itself is a SLERP pair merge (pair1d_ok is consulted on that
    # branch only) and no closed form reaches it: these cases do NOT cover it
    for shape in ((4096,), (77,)):
        cases.append((f"one_d_{shape[0]}", shape, {"default": {}}, {"default": {"f2_cols_fwd", "i1_cols_inv"}}, None))
    return cases


PATH_CASES = path_cases()
PATH_CASE_IDS = [c[0] for c in PATH_CASES]


def check_path(engine, cid):
    _, shape, variants, must_run, differ = [c for c in PATH_CASES if c[0] == cid][0]
    rec, deltas, launches = merge_records(engine, shape, variants)
    margins = {"sparse": direct_sum_margin(167)} if cid == "rough_column_668x32" else None         # 668 = 167 * 4
    for v in rec:
        assert_records(rec[v], f"{cid} {v}", margins)
        assert must_run.get(v, set()) <= set(launches[v]), (v, launches[v])
    if cid.startswith("force_split"):
        assert "dft_across_slices" not in launches["plain"]
    if differ:
        assert differ_in_bits(deltas[differ[0]], deltas[differ[1]]), f"{cid}: the hook changed nothing"


# ---- section 5: the check bites where the old one did not -------------------------------------------------------------
def dit_fft(x: torch.Tensor, last_stage=None) -> torch.Tensor:
    """a plain fp64 radix-2 decimation-in-time DFT of a 1-D tensor of 2^k entries; last_stage(w) -> the twiddles
    w^0 .. w^(n/2-1) the LAST stage multiplies by (the defect models perturb them)"""
    n = x.numel()
    bits = n.bit_length() - 1
    assert 1 << bits == n
    rev = torch.zeros(n, dtype=torch.long)
    for b in range(bits):
        rev |= ((torch.arange(n) >> b) & 1) << (bits - 1 - b)
    y = x.to(torch.complex128)[rev]
    m = 1
    while m < n:
        ang = -math.pi * torch.arange(m, dtype=torch.float64) / m
        w = torch.complex(torch.cos(ang), torch.sin(ang))
        if 2 * m == n and last_stage is not None:
            w = last_stage(w)
        y = y.view(-1, 2, m)
        t = y[:, 1, :] * w
        y = torch.stack((y[:, 0, :] + t, y[:, 0, :] - t), dim=1).reshape(-1)
        m *= 2
    return y


def one_twiddle_off(m, rel):
    """defect model (a): w^m off by `rel` relative"""
    def f(w):
        w = w.clone()
        w[m] = w[m] * (1.0 + rel)
        return w
    return f


def phase_drift(eps):
    """defect model (b): a phase error proportional to the index, eps at the end of the table"""
    def f(w):
        k = torch.arange(w.numel(), dtype=torch.float64) / w.numel()
        return w * torch.complex(torch.cos(eps * k), torch.sin(eps * k))
    return f


def old_criterion_passes(fft, n, tol=3e-6):
    """test_static_and_dynamic_plan_lengths' comparison: Gaussian noise, one normwise ratio against torch's fp32 FFT"""
    x = torch.randn(n, generator=_gen(n))
    return so.rel_err(torch.view_as_real(fft(x)), torch.view_as_real(so.fft_transform(x))) < tol


def largest_passing_defect(model, n):
    """the largest power of two at which the old criterion still accepts the defective transform"""
    for e in range(0, -60, -1):
        fft = lambda x, e=e: dit_fft(x, model(2.0 ** e)).to(torch.complex64)
        if old_criterion_passes(fft, n):
            return 2.0 ** e, fft
    raise AssertionError("the old criterion rejects every magnitude")


def rejected_inputs(fft, n):
    """the members of the forward families on which the new check rejects `fft`"""
    good = lambda x: dit_fft(x).to(torch.complex64)
    rec = transform_records(fft, lambda s: so.ifft_transform(s), (n,), 0)
    pool = pooled(rec)
    sane = transform_records(good, lambda s: so.ifft_transform(s), (n,), 0)
    assert all(ek <= MARGIN * pooled(sane)[fam][1] for fam, _, ek, _ in sane if fam in ("sparse", "dense")), \
        "the unperturbed DFT does not pass its own check"
    return [(fam, name) for fam, name, ek, _ in rec if fam in ("sparse", "dense") and not ek <= MARGIN * pool[fam][1]]
