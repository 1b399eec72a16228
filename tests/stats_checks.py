"""Checks of the task-vector statistics shared by the emulator tier (tests/test_stats_host.py) and the GPU tier
(tests/test_stats_gpu.py): Engine.delta_stats against tests/stats_oracle.py.  EVERY field of the report is compared with
== - the integers, and the bits of the floats (thresholds) and doubles (Gram, energies).  The tolerance is zero and it is
derived, not measured: every value is an integer, an exact order statistic or an fp64 sum in a stated order
(include/shardmerge_hip.h, smhip_delta_stats)."""
import ctypes as C
import json
import re
import struct

import pytest
import torch
from click.testing import CliRunner

from tests import harness
from tests import lora_fixtures as lf
from tests import stats_oracle
from tests.harness import ALPHAS, f32_bits, make_inputs, profile_of, ties_models

FIELDS = ("nonzero", "gram", "k_keep", "thresholds", "kept", "energy", "opposed", "alone", "cover", "conflict")
SEG = 32768
SIZES = (1, 7, 8, 9, 2047, SEG - 1, SEG, SEG + 1, 2 * SEG + 8 * 256 + 3)     # octet and segment edges
KS = (1, 2, 4, 5, 16)                           # 4 | 5 straddles the two instantiations of stats_pass
MS = (1, 4)
DENS4 = (0.05, 0.1, 0.2, 0.5)                   # the command's default
DENS_MIXED = (0.5, 1.0, 0.5, 1e-9)              # a duplicate, density 1, and a k_keep of 0, out of order
SHAPE = (37, 129)                               # 4773 elements: unaligned rows and a tail octet


def report_f64_bits(x: float) -> bytes:
    """the value packed as it stands, without the float() of harness.f64_bits: what float() would parse, a string say, is an error here"""
    return struct.pack("<d", x)


def bits(field, value):
    """a field of a report as something == compares exactly: floats as their bits (fp32 for the thresholds)"""
    if field == "thresholds":
        return [[f32_bits(v) for v in row] for row in value]
    if field in ("gram", "energy"):
        return [[report_f64_bits(v) for v in row] for row in value]
    return value


def assert_identities(rep, label=""):
    k = len(rep.nonzero)
    for q in range(len(rep.densities)):
        assert sum(rep.cover[q]) == rep.n, (label, q, rep.cover[q], rep.n)
        assert sum(c * v for c, v in enumerate(rep.cover[q])) == sum(rep.kept[q]), (label, q, rep.cover[q], rep.kept[q])
        assert sum(rep.alone[q]) == rep.cover[q][1], (label, q, rep.alone[q], rep.cover[q])
        for i in range(k):
            assert rep.opposed[q][i] <= rep.kept[q][i] <= rep.nonzero[i], (label, q, i)
            if rep.densities[q] == 1.0:
                assert report_f64_bits(rep.energy[q][i]) == report_f64_bits(rep.gram[i][i]), (label, q, i, rep.energy[q][i], rep.gram[i][i])
                assert rep.kept[q][i] == rep.nonzero[i]
    assert all(rep.gram[i][j] == rep.gram[j][i] for i in range(k) for j in range(k))


def check(engine, fts, bases, alphas, densities, label=""):
    """one call against the oracle, every field bit for bit, and the identities; returns the report"""
    rep = engine.delta_stats(fts, bases, alphas, densities, layer_name=label or None)
    cpu = lambda ts: [t.cpu() for t in ts]
    ref = stats_oracle.delta_stats(cpu(fts), cpu(bases), alphas, densities)
    print(f"{label}: n {rep.n}, k_keep {rep.k_keep}, kept {rep.kept}, conflict {rep.conflict} / {ref['conflict']}")
    assert rep.n == ref["n"] == fts[0].numel() and rep.densities == [float(x) for x in densities], label
    for f in FIELDS:
        assert bits(f, getattr(rep, f)) == bits(f, ref[f]), (label, f, getattr(rep, f), ref[f])
    assert_identities(rep, label)
    return rep


# ---- the parameter grid -------------------------------------------------------------------------------
def check_size(engine, n, device="cpu"):
    fts, bases, _ = make_inputs((n,), 2, seed=70 + n % 13, device=device)
    check(engine, fts, bases, ALPHAS[:2], DENS4, label=f"n={n} k=2 m=4")
    fts, bases, _ = make_inputs((n,), 5, seed=71 + n % 13, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:5], (0.3,), label=f"n={n} k=5 m=1")
    check(engine, fts, bases, ALPHAS[:5], DENS_MIXED, label=f"n={n} k=5 mixed densities")


def check_k_m(engine, k, m, device="cpu"):
    for own in (False, True):
        fts, bases, _ = make_inputs(SHAPE, k, seed=20 + k + m, own_bases=own, device=device)
        check(engine, fts, bases, ALPHAS[:k], DENS4[:m], label=f"k={k} m={m} own_bases={own}")


def check_dtypes(engine, in_dtype, device="cpu"):
    fts, bases, _ = make_inputs(SHAPE, 3, in_dtype, seed=11, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:3], DENS4, label=f"{in_dtype} own bases")
    fts, bases, _ = make_inputs(SHAPE, 2, in_dtype, seed=12, device=device)
    check(engine, fts, bases, ALPHAS[:2], DENS_MIXED, label=f"{in_dtype} shared base")


# ---- corners ----------------------------------------------------------------------------------------------
def check_unaligned(engine, device="cpu"):
    """views that start one element off a 16-byte boundary: the element-wise path of the loader"""
    for dtype in (torch.bfloat16, torch.float32):
        for n in (1003, SEG + 9):
            for k in (3, 5):
                fts, bases, _ = make_inputs((n + 5,), k, dtype, seed=71, own_bases=True, device=device)
                cut = lambda t, o: t[o:o + n]
                check(engine, [cut(f, 1) for f in fts], [cut(b, 1 if i else 0) for i, b in enumerate(bases)], ALPHAS[:k], DENS4,
                      label=f"unaligned {dtype} n={n} k={k}")


def check_duplicate_zero_and_one(engine, device="cpu"):
    """duplicate densities share every histogram to the end; k_keep == 0 is tau = +inf and an empty report; density 1
    keeps every nonzero entry"""
    for k in (3, 5):
        fts, bases, _ = make_inputs(SHAPE, k, seed=30 + k, device=device)
        n = fts[0].numel()
        rep = check(engine, fts, bases, ALPHAS[:k], DENS_MIXED, label=f"mixed densities k={k}")
        assert rep.k_keep == [n // 2, n, n // 2, 0]
        for f in ("thresholds", "kept", "energy", "opposed", "alone", "cover"):
            assert bits(f, getattr(rep, f))[0] == bits(f, getattr(rep, f))[2], f
        assert rep.conflict[0] == rep.conflict[2]
        assert rep.thresholds[3] == [float("inf")] * k and rep.kept[3] == [0] * k and rep.energy[3] == [0.0] * k
        assert rep.cover[3] == [n] + [0] * k and rep.conflict[3] == 0 and rep.opposed[3] == [0] * k and rep.alone[3] == [0] * k
        rep = check(engine, fts, bases, ALPHAS[:k], (0.2, 0.2, 0.2, 0.2), label=f"four equal densities k={k}")
        assert rep.kept[0] == rep.kept[1] == rep.kept[2] == rep.kept[3] and min(rep.kept[0]) >= rep.k_keep[0] > 0


def check_signed_alphas(engine, device="cpu"):
    """a negative alpha flips its finetune's side of the election; a zero alpha's kept entries are tv = 0: they agree
    with nothing (opposed, all of them) and take no side (never a conflict)"""
    fts, bases, _ = make_inputs(SHAPE, 4, seed=55, own_bases=True, device=device)
    rep = check(engine, fts, bases, [0.5, -0.3, 0.0, -0.7], DENS4, label="signed alphas")
    for q in range(4):
        assert rep.opposed[q][2] == rep.kept[q][2] > 0
    check(engine, fts, bases, [-0.5, -0.3, -0.2, -0.7], DENS4, label="negative alphas")
    for k in (1, 5):
        rep = check(engine, fts[:1] * k, bases[:1] * k, [0.0] * k, (0.5, 1.0), label=f"zero alphas k={k}")
        assert rep.conflict == [0, 0] and rep.opposed == rep.kept


def check_zero_delta(engine, device="cpu"):
    """one finetune equals its base: nothing of it is nonzero or kept, its threshold is 0; all of them: an empty report"""
    for k in (3, 5):
        fts, bases, _ = make_inputs(SHAPE, k, seed=60, device=device)
        n = fts[0].numel()
        fts[1] = bases[1].clone()
        rep = check(engine, fts, bases, ALPHAS[:k], DENS_MIXED, label=f"one zero delta k={k}")
        assert rep.nonzero[1] == 0 and all(row[1] == 0 for row in rep.kept) and rep.gram[1] == [0.0] * k
        assert rep.thresholds[0][1] == 0.0 and rep.thresholds[3][1] == float("inf")
        rep = check(engine, [b.clone() for b in bases], bases, ALPHAS[:k], (0.5, 1.0), label=f"all zero deltas k={k}")
        assert rep.nonzero == [0] * k and rep.cover == [[n] + [0] * k] * 2 and rep.conflict == [0, 0]


def check_tied_bf16(engine, device="cpu"):
    """sigma 3e-3 on bf16 weights: a few hundred distinct magnitudes, so the thresholds tie heavily and kept > k_keep"""
    n = 2 * SEG + 777
    for k in (2, 5):
        fts, bases, _ = make_inputs((n,), k, torch.bfloat16, seed=65, sigma=3e-3, device=device)
        rep = check(engine, fts, bases, ALPHAS[:k], DENS4, label=f"tied bf16 k={k}")
        assert any(rep.kept[q][i] > rep.k_keep[q] for q in range(4) for i in range(k)), (rep.kept, rep.k_keep)


def check_denormals(engine, device="cpu"):
    g = torch.Generator().manual_seed(66)
    ft = (torch.randn(SHAPE, generator=g) * 1e-40).to(device)
    assert 0 < float(ft.abs().max()) < 1.2e-38
    zero = torch.zeros_like(ft)
    check(engine, [ft, ft * 0.5, -ft], [zero] * 3, [0.5, 0.75, 0.25], DENS4, label="fp32 denormal deltas")


def check_nonfinite(engine, device="cpu"):
    """a NaN / an Inf in one finetune: ValueError naming the tensor and the finetune; the context stays usable"""
    for k, poison in ((3, float("inf")), (5, float("nan")), (3, float("-inf"))):
        fts, bases, _ = make_inputs(SHAPE, k, seed=80, device=device)
        fts[1] = fts[1].clone()
        fts[1].view(-1)[4321] = poison
        with pytest.raises(ValueError, match=r"model\.layers\.7\.mlp\.up_proj\.weight.*finetune 1\b"):
            engine.delta_stats(fts, bases, ALPHAS[:k], DENS4, layer_name="model.layers.7.mlp.up_proj.weight")
        fts, bases, _ = make_inputs(SHAPE, k, seed=81, device=device)
        check(engine, fts, bases, ALPHAS[:k], DENS4, label="after an error")


def check_tiny_and_rank3(engine, device="cpu"):
    fts, bases, _ = make_inputs((0,), 2, seed=73, device=device)
    rep = engine.delta_stats(fts, bases, [0.5, 0.5], (0.5, 1.0))
    assert rep.n == 0 and rep.thresholds == [[float("inf")] * 2] * 2 and rep.k_keep == [0, 0] and rep.cover == [[0, 0, 0]] * 2
    assert rep.nonzero == [0, 0] and rep.gram == [[0.0, 0.0]] * 2 and rep.kept == rep.opposed == rep.alone == [[0, 0]] * 2
    assert rep.energy == [[0.0, 0.0]] * 2 and rep.conflict == [0, 0]
    fts, bases, _ = make_inputs((4, 33, 65), 3, seed=74, own_bases=True, device=device)
    check(engine, fts, bases, ALPHAS[:3], DENS4, label="rank 3")


def check_determinism(engine, device="cpu"):
    fts, bases, _ = make_inputs((300, 500), 3, seed=90, own_bases=True, device=device)
    assert engine.delta_stats(fts, bases, ALPHAS[:3], DENS4) == engine.delta_stats(fts, bases, ALPHAS[:3], DENS4)


def check_identities_with_the_operators(engine, device="cpu"):
    """through the same engine: thresholds and kept are ties_merge's at each density, the Gram is geo_merge's"""
    for k, own, shape in ((3, True, SHAPE), (5, False, SHAPE), (1, False, SHAPE), (16, True, SHAPE), (2, False, (SEG + 100,))):
        fts, bases, bo = make_inputs(shape, k, seed=100 + k, own_bases=own, device=device)
        rep = engine.delta_stats(fts, bases, ALPHAS[:k], DENS_MIXED)
        assert_identities(rep, f"k={k}")
        for q, rho in enumerate(DENS_MIXED):
            _, t_rep = engine.ties_merge(fts, bases, ALPHAS[:k], bo, density=rho)
            assert rep.k_keep[q] == t_rep.k_keep and rep.kept[q] == t_rep.kept, (k, rho)
            assert [f32_bits(t) for t in rep.thresholds[q]] == [f32_bits(t) for t in t_rep.thresholds], (k, rho)
        _, g_rep = engine.geo_merge(fts, bases, ALPHAS[:k], bo, mode="model_stock")
        assert bits("gram", rep.gram) == bits("gram", g_rep.gram), k


def check_arguments(engine, device="cpu"):
    fts, bases, _ = make_inputs((8, 8), 2, seed=91, device=device)
    for bad in ((0.0,), (-0.1,), (1.5,), (float("nan"),), (0.2, 0.0)):
        with pytest.raises(ValueError, match="density"):
            engine.delta_stats(fts, bases, [0.5, 0.5], bad)
    for bad in ((), (0.1,) * 5):
        with pytest.raises(ValueError, match="densities"):
            engine.delta_stats(fts, bases, [0.5, 0.5], bad)
    with pytest.raises(ValueError, match="shape mismatch"):
        engine.delta_stats([fts[0], fts[1][:4]], bases, [0.5, 0.5], DENS4)
    with pytest.raises(ValueError, match="supported range"):
        engine.delta_stats([fts[0]] * 17, [bases[0]] * 17, [0.1] * 17, DENS4)
    with pytest.raises(ValueError, match="alphas"):
        engine.delta_stats(fts, bases, [0.5], DENS4)


CORNERS = [check_unaligned, check_duplicate_zero_and_one, check_signed_alphas, check_zero_delta, check_tied_bf16, check_denormals,
           check_nonfinite, check_tiny_and_rank3, check_determinism, check_identities_with_the_operators, check_arguments]


# ---- profile names and launches ----------------------------------------------------------------------------
def check_profile(engine, k, m, shape=(40, 50), device="cpu"):
    """three stats_hist launches per group of four finetunes and three stats_select launches, whatever m; the Gram through
    geo_gram's own launches; one fused pass and its fold"""
    fts, bases, _ = make_inputs(shape, k, seed=6, device=device)
    got = profile_of(engine, lambda: engine.delta_stats(fts, bases, ALPHAS[:k], DENS4[:m]))
    assert got == {"stats_hist": 3 * ((k + 3) // 4), "stats_select": 3, "geo_gram": 1, "geo_gram_fold": 1, "stats_pass": 1, "stats_fold": 1}, got


# ---- the C ABI ------------------------------------------------------------------------------------------------
def check_c_abi(engine, device="cpu"):
    from shardmerge_amd import _lib
    x = torch.ones(64, dtype=torch.bfloat16, device=device)
    y = torch.zeros(64, dtype=torch.bfloat16, device=device)
    dll, h = engine.lib.dll, engine.ctx.h

    def call(k=1, m=1, density=0.5, n=64, in_dtype=_lib.BF16, alpha=0.5, ft=x, with_report=True):
        d = _lib.StatsDesc()
        d.k, d.m, d.in_dtype, d.n = k, m, in_dtype, n
        for i in range(max(0, min(k, 16))):
            d.finetune[i], d.base[i], d.alpha[i] = (ft.data_ptr() if ft is not None else None), y.data_ptr(), alpha
        for q in range(max(0, min(m, 4))):
            d.density[q] = density
        rep = _lib.StatsReport()
        rc = dll.smhip_delta_stats(h, C.byref(d), C.byref(rep) if with_report else None, None)
        return rc, dll.smhip_last_error(h).decode(), rep

    rc, msg, rep = call()
    assert rc == _lib.OK and rep.k_keep[0] == 32 and rep.kept[0][0] == 64 and rep.nonzero[0] == 64 and rep.G[0][0] == 64.0, msg
    assert rep.cover[0][1] == 64 and rep.alone[0][0] == 64 and rep.opposed[0][0] == 0 and rep.energy[0][0] == 64.0 and rep.tau[0][0] == 1.0
    for kwargs, word in (({"k": 0}, "k out of range"), ({"k": 17}, "k out of range"), ({"m": 0}, "m out of range"), ({"m": 5}, "m out of range"),
                         ({"density": 0.0}, "density"), ({"density": 1.01}, "density"), ({"density": float("nan")}, "density"),
                         ({"alpha": float("nan")}, "alpha"), ({"alpha": float("inf")}, "alpha"), ({"in_dtype": 3}, "dtype"),
                         ({"ft": None}, "null model tensor"), ({"with_report": False}, "null report")):
        rc, msg, _ = call(**kwargs)
        assert rc == _lib.ERR_ARG and word in msg, (kwargs, rc, msg)
    rc = dll.smhip_delta_stats(h, None, C.byref(_lib.StatsReport()), None)
    assert rc == _lib.ERR_ARG and "null descriptor" in dll.smhip_last_error(h).decode()
    rc, msg, rep = call(n=0, ft=None, m=2)
    assert rc == _lib.OK and rep.tau[0][0] == float("inf") and rep.tau[1][0] == float("inf") and rep.cover[0][0] == 0, msg


# ---- the model-shaped cases of the GPU tier ----------------------------------------------------------------
def check_model_shape(engine, shape, k, own, densities, device="cpu"):
    """Gaussian deltas: the report cannot be empty - at rho < 1 every finetune keeps some and not all, and some elements conflict"""
    fts, bases, _ = make_inputs(shape, k, seed=7 + k, own_bases=own, device=device)
    rep = check(engine, fts, bases, ALPHAS[:k], densities, label=f"{shape} k={k}")
    for q, rho in enumerate(densities):
        if rho < 1.0:
            assert 0 < rep.conflict[q] < rep.n or k == 1, (q, rep.conflict)
            assert all(0 < kept < rep.n for kept in rep.kept[q]), (q, rep.kept[q])
    return rep


# ---- the CLI on the synthetic on-disk model of tests/lora_fixtures.py ----------------------------------------
def write_config(root, third, out_dir, options=None, device=None, models=None):
    return harness.write_config(root, models or ties_models(third), out_dir, options or None, device)


def run_cli(args):
    from shardmerge_amd.__main__ import cli
    return CliRunner().invoke(cli, [str(a) for a in args])


def expected_records(base, full, densities, windows=True):
    """the oracle tensor by tensor, in the order merge takes the tensors: the models of harness.ties_models - layer 0
    has three entries, layer 1 two (windows) - or all three everywhere"""
    ft1, ft2 = lf.model_tensors(1), lf.model_tensors(2)
    out = []
    for name, shape in lf.TENSORS:
        m = re.match(r"model\.layers\.(\d+)\.", name)
        if m is None:
            continue
        entries = [(0, ft1[name], base[name], 0.5)] + ([(1, ft2[name], ft1[name], 0.3)] if int(m.group(1)) == 0 or not windows else []) + \
                  [(2, full[name], base[name], 0.4)]
        ref = stats_oracle.delta_stats([e[1] for e in entries], [e[2] for e in entries], [e[3] for e in entries], densities)
        out.append({"name": name, "shape": list(shape), "entries": [e[0] for e in entries], **ref})
    return out


def assert_report(path, expected, densities):
    doc = json.loads(path.read_text())
    assert doc["densities"] == [float(x) for x in densities] and doc["output_base_model"] == "org/base"
    assert [m["model"] for m in doc["models"]][:2] == ["org/ft1", "org/ft2"] and [m["alpha"] for m in doc["models"]] == [0.5, 0.3, 0.4]
    # the tensors come in the order merge takes them (shards by file name, a shard's tensors in layer order)
    assert sorted(t["name"] for t in doc["tensors"]) == sorted(t["name"] for t in expected)
    by_name = {t["name"]: t for t in expected}
    expected = [by_name[t["name"]] for t in doc["tensors"]]
    shard_of = {n: s for s, items in lf.SHARDS.items() for n, _ in items}
    assert [shard_of[t["name"]] for t in expected] == sorted(shard_of[t["name"]] for t in expected)
    for got, ref in zip(doc["tensors"], expected):
        assert got["shape"] == ref["shape"] and got["n"] == ref["n"] and got["entries"] == ref["entries"], got["name"]
        for f in FIELDS:
            assert bits(f, got[f]) == bits(f, ref[f]), (got["name"], f, got[f], ref[f])
    assert sorted(p["name"] for p in doc["passthrough"]) == sorted(n for n, _ in lf.TENSORS if "layers" not in n)
    # the model record: integers summed exactly, the doubles added in tensor order
    rec, K, m = doc["model"], 3, len(densities)
    assert rec["n"] == sum(t["n"] for t in expected)
    want_nz, want_g, want_kept, want_e = [0] * K, [[0.0] * K for _ in range(K)], [[0] * K for _ in range(m)], [[0.0] * K for _ in range(m)]
    for t in expected:
        for a, i in enumerate(t["entries"]):
            want_nz[i] += t["nonzero"][a]
            for b, j in enumerate(t["entries"]):
                want_g[i][j] = want_g[i][j] + t["gram"][a][b]
            for q in range(m):
                want_kept[q][i] += t["kept"][q][a]
                want_e[q][i] = want_e[q][i] + t["energy"][q][a]
    assert rec["nonzero"] == want_nz and rec["kept"] == want_kept
    assert bits("gram", rec["gram"]) == bits("gram", want_g) and bits("energy", rec["energy"]) == bits("energy", want_e)
    assert rec["conflict"] == [sum(t["conflict"][q] for t in expected) for q in range(m)]
    for q in range(m):
        assert sum(rec["cover"][q]) == rec["n"]
    return doc
