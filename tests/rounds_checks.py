"""Every streaming kernel that DeltaHost launches (csrc/sm_delta_host.hpp), at round counts that its operator's own tests
never reach.  Shared by the emulator tier (tests/test_rounds_host.py) and the GPU tier (tests/test_rounds_gpu.py).

Those kernels loop `for (q = 0; q < p.chunks; ++q)` over rounds of 256 units per work-group and carry state from round
to round: lane counters, LDS histograms and their flush, staged scale bytes, the `break` of octet_at, the branches of
the last round.  A tensor small enough for a CPU oracle leaves `chunks` at the kernel's minimum, so the test hook
"stream_chunks" of smhip_debug_option forces the count.  A case is one call of an operator's own X_checks.check - its
oracle and its tolerance, which is zero throughout - and asserts under the forced count:
  (a) that check passes;
  (b) everything the engine returned - outputs, side outputs, every field of the reports - has the bytes of the same
      call with the option at 0 (no result depends on the round count: none of these kernels adds floating point
      values across rounds in an order the count could change);
  (c) "stream_chunks_applied" rose, the kernels the case is named for ran, and the launch counts are those of the
      option at 0.
The geometry, from stream_grid: SMALL is 1589 octets, which 1, 2, 3 and 7 rounds split into 7, 4, 3 and 1 work-groups;
at 2 and 3 rounds the last work-group has rounds wholly past the end, at 7 the last round is partial, from 3 on a
staging set and the per-lane state are reused.  The row-octet kernels see 97 x 17 = 1649 units (the same grids), CABS
97 x 3 x 8 = 2328."""
import dataclasses
import struct
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from tests import (breadcrumbs_checks, cabs_checks, consensus_checks, dare_checks, della_checks, dpack_checks, emr_checks,
                   fp8_checks, fusion_checks, geo_checks, iso_checks, mx4_checks, pcb_checks, sce_checks, sphere_checks,
                   stats_checks, ties_checks)
from tests.harness import ALPHAS, DTYPES, SMALL, make_inputs, profile_of, raw

COUNTS = (1, 2, 3, 7)
MX4_SHAPES = ((3, 8224), (257, 2080))            # 771 blocks: at 3 rounds a second work-group of 3 blocks, a partial
MX4_ONE_GROUP = 66                               # 16-byte scale store and two empty rounds; 16705 blocks: 66 rounds, one work-group

# The kernels whose parameter block has a `chunks` field that DeltaHost fills: the launches of sm_delta_host.hpp whose
# grid is stream_grid(units, block, chunks), by the names of their tags (an ...Any instantiation shares its name but for
# CABS).  delta_inputs serves ties, crumbs, dare, geo_combine, sce, consensus, fusion, pcb and emr _merge; hist_grid the
# _hist kernels; the rest have a call of their own.  WHEN YOU ADD a kernel that reads a chunks field filled through
# DeltaHost::stream_chunks, add its name here and a case to CASES: test_table_is_complete holds the two together.
KERNELS = ("ties_hist", "ties_merge", "crumbs_hist", "crumbs_merge", "dare_merge", "della_merge", "geo_combine",
           "sce_hist", "sce_merge", "consensus_merge", "stats_hist", "fusion_hist", "fusion_merge", "pcb_hist", "pcb_merge",
           "cabs_merge", "cabs_merge_any", "iso_sum", "iso_apply", "dpack_apply", "fp8_dequant", "mx4_quant", "mx4_dequant",
           "emr_merge", "emr_apply")


@contextmanager
def forced_chunks(engine, c):
    """every streaming kernel of DeltaHost runs c rounds per work-group (0: as always); the option is 0 afterwards"""
    engine.ctx.debug_option("stream_chunks", c)
    try:
        yield
    finally:
        engine.ctx.debug_option("stream_chunks", 0)


class Recording:
    """the engine, keeping what each of its calls returned"""

    def __init__(self, engine):
        self._engine, self.results = engine, []

    def __getattr__(self, name):
        attr = getattr(self._engine, name)
        if name.startswith("_") or not callable(attr):
            return attr

        def call(*args, **kw):
            res = attr(*args, **kw)
            self.results.append((name, res))
            return res
        return call


def freeze(x):
    """a returned value as something == compares byte for byte: tensors and floats as their bytes, reports field by field"""
    if isinstance(x, torch.Tensor):
        return ("tensor", str(x.dtype), tuple(x.shape), x.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    if isinstance(x, (np.ndarray, np.generic)):
        return ("numpy", str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes())
    if dataclasses.is_dataclass(x) and not isinstance(x, type):
        return (type(x).__name__,) + tuple((f.name, freeze(getattr(x, f.name))) for f in dataclasses.fields(x))
    if isinstance(x, float):
        return ("float", struct.pack("<d", x))
    if isinstance(x, (list, tuple)):
        return tuple(freeze(v) for v in x)
    if isinstance(x, dict):
        return tuple((k, freeze(v)) for k, v in sorted(x.items()))
    return x


def assert_same_results(got, want, label):
    assert [n for n, _ in got] == [n for n, _ in want], label
    for j, ((name, a), (_, b)) in enumerate(zip(got, want)):
        assert freeze(a) == freeze(b), f"{label}: call {j}, {name}: the result differs from that of the option at 0"


# ---- the table ------------------------------------------------------------------------------------------------------
def std(k, device, seed, own=True, shape=SMALL):
    fts, bases, bo = make_inputs(shape, k, seed=seed, own_bases=own, device=device)
    return fts, bases, ALPHAS[:k], bo


def emr_in(k, device, seed):
    fts, bases, _, bo = std(k, device, seed)
    return fts, bases, bo


def cabs(e, d, k):
    # (group 64: 8 lanes per team and tail groups of 3 columns; the teams' LDS and the kept counters cross the rounds)
    cabs_checks.check(e, *std(k, d, 340 + k), n_keep=16, group=64, label=f"cabs k={k}")
    cabs_checks.check(e, *std(k, d, 350 + k, own=False), n_keep=2, group=4, conflict_aware=False, label=f"cabs 2:4 k={k}")


def dpack(e, d):
    for bits, density, scale in ((1, 1.0, "row"), (2, 0.3, "tensor")):
        dpack_checks.check(e, *dpack_checks.pair(SMALL, seed=360 + bits, device=d), bits=bits, density=density, scale=scale,
                           label=f"dpack {bits} bit")


def geo(e, d):
    for mode, rowwise in geo_checks.VARIANTS:
        geo_checks.check(e, *std(3 if mode == "model_stock" else 2, d, 310), mode=mode, rowwise=rowwise, label=f"{mode} rowwise={rowwise}")


def sphere(e, d):
    for mode, rowwise in sphere_checks.VARIANTS:
        sphere_checks.check(e, *std(3, d, 311), mode=mode, rowwise=rowwise, label=f"{mode} rowwise={rowwise}")


def emr_apply(e, d):
    emr_checks.check_mask(e, *emr_checks.triple(SMALL, seed=370, device=d), label="emr mask and apply")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    kernels: tuple               # the names of KERNELS that the case launches, exactly
    run: object                  # run(engine, device)


# k = 3 | 5: the register and the ...Any instantiation (SCE, Consensus, PCB, CABS, EMR: k <= 4 | more); 16: four groups of
# _hist launches.  The hist side (hist_grid: 4 rounds by default) and the merge side (2) of a call take the same forced count
CASES = (
    Case("ties-k3", ("ties_hist", "ties_merge"), lambda e, d: ties_checks.check(e, *std(3, d, 301), density=0.2, lam=0.7, label="ties k=3")),
    Case("ties-k16", ("ties_hist", "ties_merge"), lambda e, d: ties_checks.check(e, *std(16, d, 302, own=False), density=0.5, label="ties k=16")),
    Case("breadcrumbs-k3", ("crumbs_hist", "crumbs_merge"),
         lambda e, d: breadcrumbs_checks.check(e, *std(3, d, 303), density=0.8, gamma=0.05, sign_election=True, label="breadcrumbs k=3")),
    Case("dare-k3", ("dare_merge",), lambda e, d: dare_checks.check(e, *std(3, d, 304), density=0.3, stream_ids=[3, 4, 5], label="dare k=3")),
    Case("dare-k5", ("dare_merge",), lambda e, d: dare_checks.check(e, *std(5, d, 305), density=0.5, sign_election=False, label="dare k=5")),
    Case("della-k3", ("della_merge",), lambda e, d: della_checks.check(e, *std(3, d, 306), density=0.5, epsilon=0.15, label="della k=3")),
    Case("geo", ("geo_combine",), geo),
    Case("sphere", ("geo_combine",), sphere),
    Case("sce-k3", ("sce_hist", "sce_merge"), lambda e, d: sce_checks.check(e, *std(3, d, 312), select_topk=0.3, lam=0.7, label="sce k=3")),
    Case("sce-k5", ("sce_hist", "sce_merge"), lambda e, d: sce_checks.check(e, *std(5, d, 313), select_topk=0.3, label="sce k=5")),
    Case("consensus-ta-k3", ("consensus_merge",), lambda e, d: consensus_checks.check(e, *std(3, d, 314), ties=False, label="consensus_ta k=3")),
    Case("consensus-ta-k5", ("consensus_merge",), lambda e, d: consensus_checks.check(e, *std(5, d, 315), ties=False, label="consensus_ta k=5")),
    Case("consensus-ties-k3", ("ties_hist", "consensus_merge"), lambda e, d: consensus_checks.check(e, *std(3, d, 316), ties=True, label="consensus_ties k=3")),
    Case("consensus-ties-k5", ("ties_hist", "consensus_merge"), lambda e, d: consensus_checks.check(e, *std(5, d, 317), ties=True, label="consensus_ties k=5")),
    # (the fused pass of the statistics walks segments, not rounds: its histogram side is all there is)
    Case("stats-k3", ("stats_hist",), lambda e, d: stats_checks.check(e, *std(3, d, 318)[:3], stats_checks.DENS4, label="stats k=3")),
    Case("stats-k5", ("stats_hist",), lambda e, d: stats_checks.check(e, *std(5, d, 319)[:3], stats_checks.DENS_MIXED, label="stats k=5")),
    Case("fusion-arcee", ("fusion_hist", "fusion_merge"),
         lambda e, d: fusion_checks.check(e, *fusion_checks.fusion_inputs(SMALL, seed=320, device=d), mode="arcee", label="arcee")),
    Case("fusion-nearswap", ("fusion_merge",),
         lambda e, d: fusion_checks.check(e, *fusion_checks.fusion_inputs(SMALL, seed=321, own_out=True, device=d), mode="nearswap", t=1e-3, label="nearswap")),
    Case("pcb-k3", ("stats_hist", "pcb_hist", "pcb_merge"), lambda e, d: pcb_checks.check(e, *std(3, d, 330), ratio=0.1, label="pcb k=3")),
    Case("pcb-k5", ("stats_hist", "pcb_hist", "pcb_merge"), lambda e, d: pcb_checks.check(e, *std(5, d, 331), ratio=0.3, lam=0.7, label="pcb k=5")),
    Case("cabs-k3", ("cabs_merge",), lambda e, d: cabs(e, d, 3)),
    Case("cabs-k5", ("cabs_merge_any",), lambda e, d: cabs(e, d, 5)),
    Case("iso-k3", ("iso_sum", "iso_apply"), lambda e, d: iso_checks.check_merge(e, SMALL, 3, own=True)),
    Case("dpack", ("ties_hist", "dpack_apply"), dpack),            # (the 2-bit pack selects with the thresholds of TIES)
    Case("fp8", ("fp8_dequant",), lambda e, d: fp8_checks.check(e, fp8_checks.weights(SMALL, seed=7, device=d), "fp8 97x131")),
    Case("emr-k3", ("emr_merge",), lambda e, d: emr_checks.check(e, *emr_in(3, d, 371), lam=0.5, label="emr k=3")),
    Case("emr-k5", ("emr_merge",), lambda e, d: emr_checks.check(e, *emr_in(5, d, 372), label="emr k=5")),
    Case("emr-apply", ("emr_apply",), emr_apply),
) + tuple(
    Case(f"mx4-{r}x{c}-{str(dt).split('.')[-1]}", ("mx4_quant", "mx4_dequant"),
         lambda e, d, shape=(r, c), dt=dt: mx4_checks.check(e, mx4_checks.weights(shape, dt, seed=sum(shape) % 89, device=d), f"mx4 {shape} {dt}"))
    for r, c in MX4_SHAPES for dt in DTYPES)
BY_NAME = {c.name: c for c in CASES}
CASE_COUNTS = [(c.name, n) for c in CASES for n in COUNTS + ((MX4_ONE_GROUP,) if c.name.startswith("mx4-257x") else ())]

_at_zero = {}


def run_recorded(engine, case, device):
    """(what the case's engine calls returned, {kernel: launches}, stream_chunks_applied afterwards)"""
    rec = Recording(engine)
    prof = profile_of(engine, lambda: case.run(rec, device))
    return rec.results, prof, engine.ctx.debug_query("stream_chunks_applied")


def at_zero(engine, case, device):
    """the case with the option at 0: run once per tier, kept unchanged for every forced count"""
    key = (str(device), case.name)
    if key not in _at_zero:
        engine.ctx.debug_option("stream_chunks", 0)
        results, prof, applied = run_recorded(engine, case, device)
        assert applied == 0, "the option is 0 and a round count was forced"
        _at_zero[key] = (results, prof)
    return _at_zero[key]


def check_case(engine, name, c, device="cpu"):
    case = BY_NAME[name]
    want, want_prof = at_zero(engine, case, device)
    with forced_chunks(engine, c):
        got, prof, applied = run_recorded(engine, case, device)                  # (a): the operator's own check, inside
    assert_same_results(got, want, f"{name} at {c} rounds")                       # (b)
    assert applied >= 1, f"{name}: no launch took the forced round count"         # (c)
    assert tuple(n for n in KERNELS if n in prof) == case.kernels, (name, sorted(prof))
    assert prof == want_prof, (name, c, prof, want_prof)
    assert engine.ctx.debug_query("stream_chunks_applied") == 0


def check_table_is_complete():
    seen = {k for case in CASES for k in case.kernels}
    assert seen == set(KERNELS) and len(set(KERNELS)) == len(KERNELS), sorted(seen ^ set(KERNELS))
    assert len(BY_NAME) == len(CASES)


# ---- the hook itself -------------------------------------------------------------------------------------------------
def check_hook(engine, device="cpu"):
    """the counter counts since the option was set, 0 restores the default, a count above the cap is the cap, the launch
    counts of a TIES and an MXFP4 call do not depend on the option"""
    args = std(3, device, 380)
    x = mx4_checks.weights((3, 8224), seed=3, device=device)
    ties = {"ties_hist": 3, "ties_select": 3, "ties_merge": 1}
    assert profile_of(engine, lambda: engine.ties_merge(*args, density=0.2)) == ties
    assert profile_of(engine, lambda: engine.mx4_quant(x)) == {"mx4_quant": 1}
    assert engine.ctx.debug_query("stream_chunks_applied") == 0
    with forced_chunks(engine, 3):
        assert profile_of(engine, lambda: engine.ties_merge(*args, density=0.2)) == ties
        assert engine.ctx.debug_query("stream_chunks_applied") == 2           # the histogram side and the merge side
        assert profile_of(engine, lambda: engine.mx4_quant(x)) == {"mx4_quant": 1}
        assert engine.ctx.debug_query("stream_chunks_applied") == 3
        engine.ctx.debug_option("stream_chunks", 3)                           # setting it starts the count again
        assert engine.ctx.debug_query("stream_chunks_applied") == 0
    engine.mx4_quant(x)
    assert engine.ctx.debug_query("stream_chunks_applied") == 0
    want = engine.mx4_quant(x)
    with forced_chunks(engine, 10 ** 6):                                      # 4096 rounds, one work-group, all but four empty
        got = engine.mx4_quant(x)
        assert engine.ctx.debug_query("stream_chunks_applied") == 1
    assert freeze(got) == freeze(want)
    with forced_chunks(engine, -5):                                           # (a negative count is 0)
        engine.mx4_quant(x)
        assert engine.ctx.debug_query("stream_chunks_applied") == 0


# ---- errors and edges ------------------------------------------------------------------------------------------------
def check_views(engine, device="cpu"):
    """the views that start one element into their storage: the element-by-element path of both MXFP4 kernels loops too"""
    with forced_chunks(engine, 3):
        prof = profile_of(engine, lambda: mx4_checks.check_views(engine, device=device))
        assert engine.ctx.debug_query("stream_chunks_applied") >= 1 and {"mx4_quant", "mx4_dequant"} <= set(prof)


def check_after_an_error(engine, device="cpu"):
    """a call that fails under a forced count leaves nothing behind: the next one is correct"""
    with forced_chunks(engine, 3):
        for dtype in DTYPES:
            x = mx4_checks.weights((3, 8224), dtype, seed=41, device=device)
            x[2, 8223] = float("nan")                                         # in the second work-group's three blocks
            with pytest.raises(ValueError, match=r"layers\.7\.up_proj"):
                engine.mx4_quant(x, layer_name="layers.7.up_proj")
            mx4_checks.check(engine, mx4_checks.weights((3, 8224), dtype, seed=42, device=device), f"after an error {dtype}")
        codes, sc, _ = engine.mx4_quant(mx4_checks.weights((3, 8224), seed=43, device=device))
        sc[2, 256] = 0xFF
        with pytest.raises(ValueError, match=r"NaN scale code in model\.norm"):
            engine.mx4_dequant(codes, sc, torch.bfloat16, layer_name="model.norm")
        mx4_checks.check(engine, mx4_checks.weights((3, 8224), seed=44, device=device), "after a NaN scale")
        assert engine.ctx.debug_query("stream_chunks_applied") >= 1


def check_empty(engine, device="cpu"):
    """an empty tensor under a forced count: what it returns today, and no launch"""
    def calls():
        x = mx4_checks.weights((3, 64), seed=26, device=device)
        fts, bases, alphas, bo = std(2, device, 390, shape=(0,))
        e = engine.mx4_quant(x[:0])
        res = [e, engine.mx4_dequant(e[0], e[1], torch.float32),
               engine.ties_merge(fts, bases, alphas, bo, density=0.5, want_delta=True),
               engine.dare_merge(fts, bases, alphas, bo, density=0.5, want_delta=True),
               engine.emr_merge(fts, bases, bo, want_delta=True),
               engine.delta_stats(fts, bases, alphas, (0.5,))]
        assert res[0][0].numel() == 0 and res[0][2].blocks == 0 and res[1].numel() == 0 and res[2][0].numel() == 0
        return res
    want = calls()
    with forced_chunks(engine, 3):
        got = []
        assert profile_of(engine, lambda: got.extend(calls())) == {}
        assert engine.ctx.debug_query("stream_chunks_applied") == 0
    assert freeze(got) == freeze(want)


# ---- device only: the two quantised formats at model-like shapes against the emulator under the same count ----------
DEVICE_SHAPES = ((300, 4544), (2048, 4096))
DEVICE_COUNTS = (3, 5)


def check_device_against_emulator(engine, shape, c):
    from tests.emul.loader import emul_engine
    emul = emul_engine()
    x = mx4_checks.weights(shape, seed=sum(shape) % 97, device=engine.device)
    y = fp8_checks.weights(shape, seed=sum(shape) % 97, device=engine.device)
    with forced_chunks(engine, c), forced_chunks(emul, c):
        codes, sc, rep = engine.mx4_quant(x)
        ecodes, esc, erep = emul.mx4_quant(x.cpu())
        assert torch.equal(ecodes, codes.cpu()) and torch.equal(esc, sc.cpu()) and erep == rep
        assert torch.equal(raw(emul.mx4_dequant(ecodes, esc, torch.bfloat16)), raw(engine.mx4_dequant(codes, sc, torch.bfloat16)))
        f8, inv, _ = engine.fp8_quant(y)
        assert torch.equal(raw(emul.fp8_dequant(f8.cpu(), inv.cpu(), torch.bfloat16)), raw(engine.fp8_dequant(f8, inv, torch.bfloat16)))
        assert engine.ctx.debug_query("stream_chunks_applied") == 3 == emul.ctx.debug_query("stream_chunks_applied")
