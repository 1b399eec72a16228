"""Checks of the fused EMR pass shared by the emulator tier (tests/test_emr_fused_host.py) and the GPU tier
(tests/test_emr_fused_gpu.py): Engine.emr_merge_masks (smhip_emr_merge_masks, include/shardmerge_hip.h) against the
composition that IS its specification - emr_merge, then emr_mask(f_i, b_i, out) for every entry - once by
tests/emr_oracle.py and once through the same engine's two existing calls, BIT FOR BIT: out, the merged delta, every
counter, all k planes, all 7k sums, every rescaler, the residuals.  The tolerance is zero and it is derived, not measured:
both sides are the same sequence of correctly rounded operations, comparisons and integer counts.  Then the identities
through the engine, the launches, the C ABI, and `merge --emr-packs` on the on-disk model of tests/lora_fixtures.py
against what `emr-task` writes afterwards."""
import asyncio
import ctypes as C
import json

import pytest
import torch

from tests import emr_checks as ec
from tests import emr_oracle as eo
from tests import harness
from tests.harness import DTYPES, SMALL, f32_bits, f64_bits, make_inputs, profile_of, raw

FOLD_ROWS = 64                                             # EMR_FOLD_ROWS of csrc/sm_emr_fused.hpp: rows per staged block of emr_fold
COLS = ec.COLS                                             # a row's lanes wrap at 2048 elements; the octet's edge
ROWS = ec.ROWS
FOLD_EDGE_ROWS = (FOLD_ROWS - 1, FOLD_ROWS, FOLD_ROWS + 1, 3 * FOLD_ROWS + 5)
KS = (1, 2, 3, 4, 5, 8, 16)                                # the 4-task register group and the k <= 4 / k <= 16 switch
LAMBDAS = ec.LAMBDAS


def cpu(ts):
    return [t.cpu() for t in ts]


def same_mask_report(got, want, label):
    for f in ec.MASK_INTS:
        assert getattr(got, f) == getattr(want, f), (label, f, getattr(got, f), getattr(want, f))
    for f in ec.MASK_SUMS:
        assert f64_bits(getattr(got, f)) == f64_bits(getattr(want, f)), (label, f, getattr(got, f), getattr(want, f))
    assert f32_bits(got.lam) == f32_bits(want.lam), (label, got.lam, want.lam)


def check(engine, fts, bases, base_out, lam=1.0, label="", through_engine=True):
    """one fused call against the oracle's composition and against the engine's own two calls; returns the call's result"""
    k, n = len(fts), base_out.numel()
    out, rep, masks, scales, mreps, delta = engine.emr_merge_masks(fts, bases, base_out, lam=lam, want_delta=True,
                                                                   layer_name=label or "layer")
    ref = eo.emr_merge(cpu(fts), cpu(bases), base_out.cpu(), lam=lam)
    print(f"{label}: {rep}")
    assert out.dtype == base_out.dtype and out.shape == base_out.shape and delta.dtype == torch.float32, label
    for f in ec.MERGE_FIELDS:
        assert getattr(rep, f) == ref[f], (label, f, getattr(rep, f), ref[f])
    bad = int((raw(delta) != raw(ref["delta"])).sum())
    assert bad == 0, f"{label}: {bad} of {n} merged-delta values differ in their bits"
    bad = int((raw(out) != raw(ref["out"])).sum())
    assert bad == 0, f"{label}: {bad} of {n} output values differ in their bits"
    assert len(masks) == len(scales) == len(mreps) == k
    for i in range(k):
        want = eo.emr_mask(fts[i].cpu(), bases[i].cpu(), ref["out"])
        print(f"{label} entry {i}: {mreps[i]}")
        assert masks[i].dtype == torch.uint8 and tuple(masks[i].shape) == tuple(want.mask.shape), (label, i)
        assert scales[i].dtype == torch.float32 and tuple(scales[i].shape) == (1,), (label, i)
        bad = int((masks[i].cpu() != want.mask).sum())
        assert bad == 0, f"{label} entry {i}: {bad} of {want.mask.numel()} plane bytes differ"
        same_mask_report(mreps[i], want, f"{label} entry {i}")
        assert torch.equal(raw(scales[i]), raw(want.scale)), (label, i)
    if through_engine:
        out2, rep2, delta2 = engine.emr_merge(fts, bases, base_out, lam=lam, want_delta=True)
        assert torch.equal(raw(out2), raw(out)) and torch.equal(raw(delta2), raw(delta)) and rep2 == rep, label
        for i in range(k):
            m2, s2, r2 = engine.emr_mask(fts[i], bases[i], out2)
            assert torch.equal(m2.cpu(), masks[i].cpu()) and torch.equal(raw(s2), raw(scales[i])) and r2 == mreps[i], (label, i)
    return out, rep, masks, scales, mreps, delta


# ---- the grid ---------------------------------------------------------------------------------------------------------
def check_cols(engine, cols, device="cpu"):
    for k, own in ((3, False), (5, True)):
        fts, bases, bo = make_inputs((3, cols), k, seed=cols % 89 + k, own_bases=own, device=device)
        check(engine, fts, bases, bo, label=f"3 x {cols} k={k}")


def check_rows(engine, rows, device="cpu"):
    for k, own in ((2, True), (5, False)):
        fts, bases, bo = make_inputs((rows, 131), k, seed=rows % 89 + k, own_bases=own, device=device)
        check(engine, fts, bases, bo, label=f"{rows} x 131 k={k}")


def check_fold_rows(engine, rows, device="cpu"):
    """many rows of one octet: the staged blocks of emr_fold, their edge and the carried sum"""
    for k in (2, 16):
        fts, bases, bo = make_inputs((rows, 8), k, seed=rows % 89 + k, device=device)
        check(engine, fts, bases, bo, label=f"{rows} x 8 k={k}")


def check_k(engine, k, own, lam, device="cpu"):
    fts, bases, bo = make_inputs(SMALL, k, seed=20 + k, own_bases=own, device=device)
    check(engine, fts, bases, bo, lam=lam, label=f"k={k} own={own} lam={lam}")


def check_dtypes(engine, in_dtype, bo_dtype, device="cpu"):
    fts, bases, bo = make_inputs(SMALL, 3, in_dtype, bo_dtype, seed=11, own_bases=True, device=device)
    check(engine, fts, bases, bo, lam=0.5, label=f"{in_dtype}->{bo_dtype}")
    fts, bases, bo = make_inputs((16, 256), 5, in_dtype, bo_dtype, seed=12, device=device)   # one shared base, 16-byte accesses
    check(engine, fts, bases, bo, label=f"{in_dtype}->{bo_dtype} shared")


def check_base_out_is_no_base(engine, device="cpu"):
    """shared bases and a base_out that is none of them"""
    for k in (2, 5):
        fts, bases, _ = make_inputs(SMALL, k, seed=30 + k, device=device)
        other = make_inputs(SMALL, 1, seed=40 + k, device=device)[2]
        check(engine, fts, bases, other, label=f"base_out is no base k={k}")


def check_offset_views(engine, device="cpu"):
    """views that start one element (and more) off a 16-byte boundary: element by element, loads and stores"""
    for dtype in DTYPES:
        for rows, cols, k in ((5, 200, 3), (3, 131, 5)):
            n = rows * cols
            fts, bases, bo = make_inputs((n + 5,), k, dtype, seed=71, own_bases=True, device=device)
            cut = lambda t, o: t[o:o + n].reshape(rows, cols)
            check(engine, [cut(f, (i + 1) % 4) for i, f in enumerate(fts)], [cut(b, (i + 3) % 5) for i, b in enumerate(bases)],
                  cut(bo, 1), label=f"offset views {dtype} {rows} x {cols}")
            fts, bases, bo = make_inputs((n + 5,), 2, dtype, seed=72, device=device)        # a shared base that is base_out, off by one
            check(engine, [cut(fts[0], 1), cut(fts[1], 1)], [cut(bases[0], 1)] * 2, cut(bases[0], 1),
                  label=f"offset shared {dtype} {rows} x {cols}")


def check_heavy_ties(engine, device="cpu"):
    for k in (2, 3, 5, 16):
        fts, bases, bo = ec.tied_inputs(k, seed=k, device=device)
        check(engine, fts, bases, bo, label=f"heavy ties k={k}")


def check_equal_finetunes(engine, device="cpu"):
    """a finetune equal to its base: an all-zero plane and a rescaler of +0; all finetunes equal: every plane is the same"""
    for k in (3, 5):
        fts, bases, bo = make_inputs(SMALL, k, seed=60, device=device)
        fts[1] = bases[1].clone()
        _, rep, masks, scales, mreps, _ = check(engine, fts, bases, bo, label=f"one finetune is its base k={k}")
        assert not bool(masks[1].any()) and f32_bits(float(scales[1][0])) == f32_bits(0.0) and mreps[1].A == 0.0 and mreps[1].nonzero == 0
        fts = [fts[0]] * k
        out, rep, masks, scales, mreps, _ = check(engine, fts, bases, bo, label=f"all finetunes equal k={k}")
        assert torch.equal(raw(out), raw(fts[0])) and all(torch.equal(m, masks[0]) for m in masks)
        assert all(f32_bits(r.lam) == f32_bits(1.0) and r.resid_sq == 0.0 for r in mreps)


def check_nonfinite(engine, device="cpu"):
    """the three errors in their order of precedence; the context stays usable"""
    name = "model.layers.7.mlp.up_proj.weight"
    for k in (3, 5):
        for poison in (float("inf"), float("nan")):
            fts, bases, bo = make_inputs(SMALL, k, seed=80, own_bases=True, device=device)
            fts[2], fts[1] = fts[2].clone(), fts[1].clone()
            fts[2].view(-1)[4321] = poison
            fts[1].view(-1)[77] = poison
            with pytest.raises(ValueError, match=rf"{name}.*finetune - base of finetune 1$"):
                engine.emr_merge_masks(fts, bases, bo, layer_name=name)
        # a non-finite base_out: every delta and the sum are finite, out - base_i is not
        fts, bases, bo = make_inputs(SMALL, k, seed=81, own_bases=True, device=device)
        bo = bo.clone()
        bo.view(-1)[99] = float("inf")
        with pytest.raises(ValueError, match=rf"{name}.*unified - base of entry 0$"):
            engine.emr_merge_masks(fts, bases, bo, layer_name=name)
        fts, bases, bo = make_inputs(SMALL, k, seed=82, device=device)
        check(engine, fts, bases, bo, label="after an error")
    big = torch.full((64,), 3e38, dtype=torch.float32, device=device)
    zero = torch.zeros_like(big)
    with pytest.raises(ValueError, match=rf"{name}.*sum"):
        engine.emr_merge_masks([big, big], [zero, zero], zero, layer_name=name)


def check_ranks_empty_and_determinism(engine, device="cpu"):
    for shape, k in (((4, 33, 65), 3), ((1003,), 5), ((2048,), 2), ((), 3)):
        fts, bases, bo = make_inputs(shape, k, seed=74 + len(shape), own_bases=True, device=device)
        _, _, masks, _, mreps, _ = check(engine, fts, bases, bo, label=f"shape {shape}")
        if len(shape) <= 1:
            assert mreps[0].rows == 1 and masks[0].shape[0] == 1
    e = torch.zeros((0, 8), dtype=torch.bfloat16, device=device)
    for k in (2, 5):
        out, rep, masks, scales, mreps, delta = engine.emr_merge_masks([e] * k, [e] * k, e, want_delta=True)
        assert out.shape == e.shape and rep.n == 0 and all(m.numel() == 0 for m in masks)
        assert all(f32_bits(float(s[0])) == f32_bits(0.0) for s in scales) and all(r.c == 0 and r.resid_sq == 0.0 for r in mreps)
    for k in (3, 5):
        fts, bases, bo = make_inputs((300, 500), k, seed=90, own_bases=True, device=device)
        a = engine.emr_merge_masks(fts, bases, bo)
        b = engine.emr_merge_masks(fts, bases, bo)
        assert torch.equal(raw(a[0]), raw(b[0])) and a[1] == b[1] and a[4] == b[4]
        assert all(torch.equal(x, y) for x, y in zip(a[2], b[2])) and all(torch.equal(raw(x), raw(y)) for x, y in zip(a[3], b[3]))


def check_arguments(engine, device="cpu"):
    fts, bases, bo = make_inputs((8, 8), 2, seed=91, device=device)
    for bad in (float("inf"), float("nan"), "1", True, None):
        with pytest.raises(ValueError, match="lam"):
            engine.emr_merge_masks(fts, bases, bo, lam=bad)
    with pytest.raises(ValueError, match="shape mismatch"):
        engine.emr_merge_masks([fts[0], fts[1][:4]], bases, bo)
    with pytest.raises(ValueError, match="supported range"):
        engine.emr_merge_masks([fts[0]] * 17, [bases[0]] * 17, bo)
    with pytest.raises(ValueError, match="bases"):
        engine.emr_merge_masks(fts, bases[:1], bo)
    assert len(engine.emr_merge_masks(fts, bases, bo)) == 5 and len(engine.emr_merge_masks(fts, bases, bo, want_delta=True)) == 6


# ---- identities through the engine -----------------------------------------------------------------------------------------
def check_k1_round_trip(engine, device="cpu"):
    """one entry, lambda 1, base_out the base: the rescaler is exactly 1 and emr_apply returns the finetune"""
    for dtype in DTYPES:
        fts, bases, bo = make_inputs(SMALL, 1, dtype, seed=400, device=device)
        out, rep, masks, scales, mreps, _ = check(engine, fts, bases, bo, label=f"round trip {dtype}")
        assert torch.equal(raw(out), raw(fts[0])) and f32_bits(float(scales[0][0])) == f32_bits(1.0) and mreps[0].resid_sq == 0.0
        assert torch.equal(raw(engine.emr_apply(bo, out, masks[0], scales[0])), raw(fts[0]))


def check_mask_counts_agree(engine, device="cpu"):
    """lambda 1 on a shared base that is base_out: unified - base is the elected entry, so entry i's mask bits are the
    elements where its non-zero delta has the elected sign - mask_reports[i].c == report.agree[i] (the inputs of
    emr_checks.check_mask_counts_agree, at which no elected entry is lost to out's rounding)"""
    for dtype in DTYPES:
        for k in (2, 3, 5):
            fts, bases, bo = make_inputs(SMALL, k, dtype, seed=300 + k, device=device)
            _, rep, _, _, mreps = engine.emr_merge_masks(fts, bases, bo)
            assert [r.c for r in mreps] == rep.agree, (dtype, k, [r.c for r in mreps], rep.agree)


def check_swap(engine, device="cpu"):
    """swapping two entries swaps their planes, rescalers and reports and leaves out unchanged"""
    for k, own in ((2, False), (3, True), (5, True)):
        fts, bases, bo = make_inputs(SMALL, k, seed=101, own_bases=own, device=device)
        a = engine.emr_merge_masks(fts, bases, bo)
        perm = [1, 0] + list(range(2, k))
        b = engine.emr_merge_masks([fts[i] for i in perm], [bases[i] for i in perm], bo)
        assert torch.equal(raw(a[0]), raw(b[0]))
        for i in range(k):
            assert torch.equal(a[2][perm[i]], b[2][i]) and torch.equal(raw(a[3][perm[i]]), raw(b[3][i])) and a[4][perm[i]] == b[4][i], (k, i)


CORNERS = [check_base_out_is_no_base, check_offset_views, check_heavy_ties, check_equal_finetunes, check_nonfinite,
           check_ranks_empty_and_determinism, check_arguments, check_k1_round_trip, check_mask_counts_agree, check_swap]


# ---- launches and the C ABI ---------------------------------------------------------------------------------------------------
def check_profile(engine, device="cpu"):
    for k in (1, 2, 4, 5, 16):
        fts, bases, bo = make_inputs((40, 50), k, seed=6, device=device)
        assert profile_of(engine, lambda: engine.emr_merge_masks(fts, bases, bo)) == {"emr_merge_mask": 1, "emr_fold": 1}, k


def check_fold_hook(engine, device="cpu"):
    """the debug option that folds with geo_gram_fold: the other launch, the same bits"""
    fts, bases, bo = make_inputs((3 * FOLD_ROWS + 5, 24), 5, seed=7, device=device)
    a = engine.emr_merge_masks(fts, bases, bo)
    engine.ctx.debug_option("emr_fused_geo_fold", 1)
    try:
        assert profile_of(engine, lambda: engine.emr_merge_masks(fts, bases, bo)) == {"emr_merge_mask": 1, "geo_gram_fold": 1}
        b = engine.emr_merge_masks(fts, bases, bo)
    finally:
        engine.ctx.debug_option("emr_fused_geo_fold", 0)
    assert a[4] == b[4] and all(torch.equal(raw(x), raw(y)) for x, y in zip(a[3], b[3]))


def check_c_abi(engine, device="cpu"):
    from shardmerge_amd import _lib
    x = torch.zeros(64, dtype=torch.bfloat16, device=device)
    y = torch.zeros(64, dtype=torch.bfloat16, device=device)
    out = torch.zeros(64, dtype=torch.bfloat16, device=device)
    planes = torch.zeros((2, 8), dtype=torch.uint8, device=device)
    sc = torch.zeros(2, dtype=torch.float32, device=device)
    dll, h = engine.lib.dll, engine.ctx.h
    err = lambda: dll.smhip_last_error(h).decode()

    def call(k=2, out_t=out, n=64, rows=1, cols=64, in_dtype=_lib.BF16, lam=1.0, masks="ok", scales="ok", plane0=None, scale0=None):
        d = _lib.EmrDesc()
        d.k = k
        for i in range(max(0, min(k, 16))):
            d.finetune[i], d.base[i] = x.data_ptr(), y.data_ptr()
        d.in_dtype, d.base_out, d.base_out_dtype, d.n, d.lam = in_dtype, y.data_ptr(), _lib.BF16, n, lam
        mp = (C.c_void_p * 16)(*[planes[i % 2].data_ptr() for i in range(2)])
        sp = (C.c_void_p * 16)(*[sc[i:i + 1].data_ptr() for i in range(2)])
        if plane0 is not None:
            mp[0] = plane0
        if scale0 is not None:
            sp[0] = scale0
        rep, mreps = _lib.EmrReport(), (_lib.EmrMaskReport * 16)()
        rc = dll.smhip_emr_merge_masks(h, C.byref(d), rows, cols, out_t.data_ptr(), None, mp if masks == "ok" else None,
                                       sp if scales == "ok" else None, C.byref(rep), mreps, None)
        return rc, err(), rep, mreps

    rc, msg, rep, mreps = call()
    assert rc == _lib.OK and rep.n == 64 and rep.zero == 64 and mreps[1].cols == 64 and mreps[1].c == 0, msg
    cases = (({"k": 0}, "k out of range"), ({"k": 17}, "k out of range"), ({"lam": float("inf")}, "lambda"),
             ({"lam": float("nan")}, "lambda"), ({"out_t": x}, "overlaps"), ({"in_dtype": 3}, "dtype"),
             ({"rows": 2}, "rows * cols"), ({"masks": None}, "null"), ({"scales": None}, "null"),
             ({"plane0": 0}, "null"), ({"scale0": 0}, "null"), ({"plane0": x.data_ptr()}, "overlaps"),
             ({"scale0": out.data_ptr()}, "overlaps"), ({"plane0": planes[1].data_ptr()}, "overlaps"),
             ({"scale0": sc.data_ptr() + 2}, "aligned"))
    for kwargs, word in cases:
        rc, msg, _, _ = call(**kwargs)
        assert rc == _lib.ERR_ARG and "emr_merge_masks" in msg and word in msg, (kwargs, rc, msg)
    assert dll.smhip_emr_merge_masks(h, None, 1, 64, out.data_ptr(), None, None, None, None, None, None) == _lib.ERR_ARG \
        and "null descriptor" in err()
    # none of the rejected calls launched anything
    def rejected():
        for kwargs, _ in cases:
            call(**kwargs)
    assert profile_of(engine, rejected) == {}
    assert call(n=0, rows=0, cols=64)[0] == _lib.OK                 # no element: nothing is launched, the rescalers are +0


# ---- `merge --emr-packs` on the on-disk model of tests/lora_fixtures.py -------------------------------------------------------
def merge_cli(cfg_path, *more):
    from click.testing import CliRunner
    from shardmerge_amd.__main__ import cli
    return CliRunner().invoke(cli, ["merge", str(cfg_path), *[str(a) for a in more]])


def same_pack_dirs(a, b):
    """the same safetensors keys and bytes, emr_config.json and emr_task.json equal as JSON (floats included)"""
    from safetensors.torch import load_file
    assert sorted(p.name for p in a.iterdir()) == sorted(p.name for p in b.iterdir()) == ec.PACK_FILES, (a, b)
    ta, tb = load_file(str(a / "emr_model.safetensors")), load_file(str(b / "emr_model.safetensors"))
    assert sorted(ta) == sorted(tb), (sorted(ta), sorted(tb))
    for key in ta:
        assert ta[key].dtype == tb[key].dtype and ta[key].shape == tb[key].shape, key
        assert torch.equal(ta[key].reshape(-1).view(torch.uint8), tb[key].reshape(-1).view(torch.uint8)), key
    for doc in ("emr_config.json", "emr_task.json"):
        assert json.loads((a / doc).read_text()) == json.loads((b / doc).read_text()), doc


def merge_with_packs(tmp_path, engine, device, more=(), out="storage/org/uni"):
    """the k3 storage, the plain emr merge and the merge that writes its packs (its output at storage/org/uni); returns
    (base, the unified model's tensors by the oracle)"""
    from tests import lora_fixtures as lf
    base, _, _ = lf.setup_k3(tmp_path, engine)
    expected = ec.expected_unified(base)
    res = harness.run_cli(harness.write_config(tmp_path, ec.emr_models(), "plain", ec.OPTIONS, device))
    assert res.exit_code == 0, res.output
    cfg = harness.write_config(tmp_path, ec.emr_models(), out, ec.OPTIONS, device)
    res = merge_cli(cfg, "--emr-packs", tmp_path / "storage", "--emr-unified", "org/uni", *more)
    assert res.exit_code == 0, res.output
    harness.assert_outputs(tmp_path / out, expected)
    lf.assert_same_outputs(tmp_path / out, tmp_path / "plain")            # the options change no byte of the output
    readme = (tmp_path / out / "README.md").read_text()
    for word in ("# EMR Merged Model", "EMR packs written", "org/ft1-emr", "org/ft2-emr", "org/uni"):
        assert word in readme, (word, readme)
    return base, expected


def check_packs_end_to_end(tmp_path, engine, device):
    """each pack the merge wrote equals the directory emr-task writes afterwards from (finetune, base, the merge's
    output), and as the one entry of a dare_linear merge it gives the oracle's task tensors"""
    from tests import lora_fixtures as lf
    base, uni = merge_with_packs(tmp_path, engine, device)
    storage = tmp_path / "storage"
    for which in (1, 2):
        res = ec.run_cli(ec.task_args(tmp_path, f"org/ft{which}", f"org/task{which}", device))
        assert res.exit_code == 0, res.output
        same_pack_dirs(storage / f"org/ft{which}-emr", storage / f"org/task{which}")
        want = ec.oracle_task(base, lf.model_tensors(which), uni)[0]
        res = harness.run_cli(harness.write_config(tmp_path, ec.pack_entry(f"org/ft{which}-emr"), f"task{which}", ec.ONE_ENTRY, device))
        assert res.exit_code == 0, res.output
        harness.assert_outputs(tmp_path / f"task{which}", want)


def check_pack_forms(tmp_path, engine, device):
    """--emr-scale tensor with --emr-full, against emr-task's --scale tensor --full and the oracle"""
    from tests import lora_fixtures as lf
    full = "k_proj.weight,input_layernorm.weight"
    base, uni = merge_with_packs(tmp_path, engine, device, ("--emr-scale", "tensor", "--emr-full", full))
    storage = tmp_path / "storage"
    for which in (1, 2):
        res = ec.run_cli(ec.task_args(tmp_path, f"org/ft{which}", f"org/task{which}", device, ("--scale", "tensor", "--full", full)))
        assert res.exit_code == 0, res.output
        same_pack_dirs(storage / f"org/ft{which}-emr", storage / f"org/task{which}")
        rep = json.loads((storage / f"org/ft{which}-emr" / "emr_task.json").read_text())
        want, kinds, _, _ = ec.oracle_task(base, lf.model_tensors(which), uni, scale="tensor", full=tuple(full.split(",")))
        assert {x["name"]: x["stored"] for x in rep["tensors"]} == kinds and rep["lambda"] is None and rep["scale"] == "tensor"
        res = harness.run_cli(harness.write_config(tmp_path, ec.pack_entry(f"org/ft{which}-emr"), f"task{which}", ec.ONE_ENTRY, device))
        assert res.exit_code == 0, res.output
        harness.assert_outputs(tmp_path / f"task{which}", want)


def check_pack_rejections(tmp_path, engine, device, monkeypatch):
    """every rejection exits non-zero, names the option and the cause, and leaves no pack directory and no output shard"""
    import yaml
    from tests import dpack_checks as dc
    from tests import lora_fixtures as lf
    lf.setup_k3(tmp_path, engine)
    storage = tmp_path / "storage"
    assert dc.run_cli(dc.compress_args(tmp_path, "org/ft1", "org/dpack", device, ("--bits", 1))).exit_code == 0
    lf.write_model(storage, "org/uni_old", ec.expected_unified(lf.model_tensors(0)))
    assert ec.run_cli(ec.task_args(tmp_path, "org/ft1", "org/task", device, unified="org/uni_old")).exit_code == 0
    odd = {n: t.float() for n, t in lf.model_tensors(2).items()}
    lf.write_model(storage, "org/ft2_f32", odd)
    packs = ("--emr-packs", storage, "--emr-unified", "org/uni")
    before = sorted(p for p in storage.rglob("*") if p.is_file())

    def refused(word, more=packs, models=None, options=ec.OPTIONS, edit=None):
        cfg = harness.write_config(tmp_path, models or ec.emr_models(), "never", options, device)
        if edit:
            doc = yaml.safe_load(cfg.read_text())
            edit(doc)
            cfg.write_text(yaml.safe_dump(doc))
        res = merge_cli(cfg, *more)
        assert res.exit_code != 0, (word, res.output)
        assert not list((tmp_path / "never").glob("*.safetensors")), word
        assert sorted(p for p in storage.rglob("*") if p.is_file()) == before, word
        return res

    import logging
    seen = []

    class Keep(logging.Handler):
        def emit(self, record):
            seen.append(record)
    handler = Keep()
    logging.getLogger().addHandler(handler)
    try:
        def said(word):
            text = " ".join(r.getMessage() for r in seen)
            assert word in text, (word, text[-600:])
            seen.clear()

        entry = lambda model, **kw: {"model": model, "base": "org/base", **kw}
        two = lambda second, **kw: [entry("org/ft1", is_input=True), entry(second, is_output=True, **kw)]
        refused("operator", options={"operator": "dare_linear", "density": 1.0}); said("--emr-packs requires operator: emr")
        refused("unified", more=("--emr-packs", storage)); said("--emr-packs requires --emr-unified")
        for opt in (("--emr-unified", "org/uni"), ("--emr-scale", "tensor"), ("--emr-full", "k_proj.weight")):
            refused(opt[0], more=opt); said(f"{opt[0]} is accepted only with --emr-packs")
        refused("adapter", models=two("org/lora")); said("org/lora is an adapter")
        refused("delta pack", models=two("org/dpack")); said("org/dpack is a delta pack")
        refused("EMR pack", models=two("org/task")); said("org/task is an EMR pack")
        refused("window", models=two("org/ft2", end_layer=0)); said("org/ft2 has a layer window")
        refused("window", models=two("org/ft2", start_layer=1)); said("org/ft2 has a layer window")
        refused("twice", models=[entry("org/ft1", is_input=True), entry("org/ft1", is_output=True)]); said("two entries are org/ft1")
        refused("dtype", edit=lambda doc: doc.update(output_dtype="float32")); said("output_dtype float32 differs from the dtype of")
        refused("dtype", models=two("org/ft2_f32")); said("differs from the dtype of org/ft2_f32")
        for name in ("org/ft1", "org/base"):
            refused("unified", more=("--emr-packs", storage, "--emr-unified", name)); said(f"--emr-unified {name} is")
        refused("full", more=packs + ("--emr-full", " , ")); said("--emr-full ' , ' names no suffix")
        monkeypatch.setenv("WORLD_SIZE", "2")
        refused("ranks"); said("single process")
        monkeypatch.delenv("WORLD_SIZE")
        for var in ("SHARDMERGE_FORCE_DIST", "SHARDMERGE_INPLACE"):
            monkeypatch.setenv(var, "1")
            refused(var); said(f"unset {var}")
            monkeypatch.delenv(var)
        # an existing pack in a target directory; an output directory with finished shards
        res = merge_cli(harness.write_config(tmp_path, ec.emr_models(), "first", ec.OPTIONS, device), "--emr-packs", tmp_path / "packs",
                        "--emr-unified", "org/uni")
        assert res.exit_code == 0, res.output
        seen.clear()
        kept = (tmp_path / "packs" / "org/ft2-emr" / "emr_model.safetensors").read_bytes()
        refused("existing", more=("--emr-packs", tmp_path / "packs", "--emr-unified", "org/uni")); said("already holds an EMR pack")
        assert (tmp_path / "packs" / "org/ft2-emr" / "emr_model.safetensors").read_bytes() == kept
        res = merge_cli(harness.write_config(tmp_path, ec.emr_models(), "first", ec.OPTIONS, device), *packs)
        assert res.exit_code != 0 and not (storage / "org/ft1-emr").exists() and not (storage / "org/ft2-emr").exists()
        said("holds the finished shard")
    finally:
        logging.getLogger().removeHandler(handler)


def check_reads(tmp_path, engine, monkeypatch):
    """host logic: with packs every (model, tensor) pair is read exactly once, a block tensor's reads are the plain merge's
    and only the passthrough tensors bring every entry's finetune and base in; with the prefetching loader its schedule
    (_layer_requests) covers every read, so none falls through to the index"""
    from shardmerge_amd.config import MergeConfig
    from shardmerge_amd.index import LocalModelIndex
    from shardmerge_amd.merge.emr import EmrMerge
    from shardmerge_amd.merge.emr_packs import EmrPackMerge, EmrPackOptions
    from tests import lora_fixtures as lf
    lf.setup_k3(tmp_path, engine)
    storage = tmp_path / "storage"

    class Counting(LocalModelIndex):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.reads = []

        def load_tensor(self, uri, name):
            self.reads.append((uri, name))
            return super().load_tensor(uri, name)

    def run(cls, out, prefetch, **kw):
        monkeypatch.setenv("SHARDMERGE_PREFETCH", prefetch)
        cfg = MergeConfig.from_yaml(harness.write_config(tmp_path, ec.emr_models(), out, ec.OPTIONS, "cpu"))
        index = Counting(storage_path=storage)
        asyncio.run(cls(config=cfg, index_manager=index, engine=engine, **kw).merge("cpu"))
        return index.reads

    options = lambda d: {"emr_pack_options": EmrPackOptions(tmp_path / d, "org/uni")}
    plain = run(EmrMerge, "plain", "0")
    packed = run(EmrPackMerge, "packed", "0", **options("packs0"))
    assert len(packed) == len(set(packed)), sorted(r for r in packed if packed.count(r) > 1)
    block = lambda reads: sorted(r for r in reads if harness.layer_of(r[1]) is not None)
    assert block(packed) == block(plain)
    names = [n for n, _ in lf.TENSORS if harness.layer_of(n) is None]
    assert sorted(r for r in packed if harness.layer_of(r[1]) is None) == sorted((u, n) for n in names for u in ("org/base", "org/ft1", "org/ft2"))
    assert sorted(r for r in plain if harness.layer_of(r[1]) is None) == sorted([("org/ft1", names[0])] + [("org/ft2", n) for n in names[1:]])
    assert run(EmrPackMerge, "packed1", "1", **options("packs1")) == []
    lf.assert_same_outputs(tmp_path / "packed1", tmp_path / "plain")
    for which in (1, 2):
        same_pack_dirs(tmp_path / "packs0" / f"org/ft{which}-emr", tmp_path / "packs1" / f"org/ft{which}-emr")
