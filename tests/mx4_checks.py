"""Checks of MXFP4 shared by the emulator tier (tests/test_mx4_host.py) and the GPU tier (tests/test_mx4_gpu.py): the
engine against a plain restatement of include/shardmerge_hip.h (smhip_mx4_quant), BIT FOR BIT.  The restatement works
in fp64 with numpy.frexp / ldexp - exact for power-of-two scalings of 24-bit values - and picks the nearest of the eight
magnitudes by the seven midpoints.  The tolerance is zero: every step of the function is exact or an integer function."""
import json

import numpy as np
import pytest
import torch

from tests.harness import DTYPES, raw

ROWS = (1, 3, 257)
COLS = (32, 64, 2016, 2080, 8224)      # one block; 63 and 65 blocks around the wave; 257 around the work-group
MAGS = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
MIDS = (MAGS[:-1] + MAGS[1:]) / 2


def to_e2m1(v):
    """the code of every scaled value: the midpoints it passes, a tie going up to an even code only; NaN saturates"""
    a = np.abs(v)[..., None]
    code = np.where(np.arange(7) % 2 == 1, a >= MIDS, a > MIDS).sum(-1)
    return (np.where(np.isnan(v), 7, code) | (np.signbit(v) << 3)).astype(np.uint8)


def scale_of(a):
    """amax_to_e8m0: floor(log2 a) - 2 + 127, at least 0; 0 for a zero"""
    return np.where(a > 0, np.clip(np.frexp(a)[1] + 124, 0, None), 0).astype(np.int64)


def restate(x):
    """(codes [R, C / 2], scales [R, C / 32], saturated, zero blocks) of a 2-D CPU tensor"""
    R, C = x.shape
    xd = x.double().numpy().reshape(R, C // 32, 32)
    a = np.abs(xd).max(-1)
    s = scale_of(a)
    v = np.ldexp(xd, (127 - s)[..., None])
    c = to_e2m1(v).reshape(R, C)
    return c[:, 0::2] | (c[:, 1::2] << 4), s.astype(np.uint8), int((np.abs(v) >= 7).sum()), int((a == 0).sum())


def decode(codes, scales):
    """the fp64 values of codes [R, C / 2] and scales [R, C / 32] (numpy uint8): exact"""
    c = np.stack([codes & 15, codes >> 4], -1).reshape(codes.shape[0], -1)
    mag = np.copysign(MAGS[c & 7], np.where(c & 8, -1.0, 1.0))
    return np.ldexp(mag, np.repeat(scales.astype(np.int64) - 127, 32, axis=1))


def weights(shape, dtype=torch.bfloat16, seed=0, device="cpu"):
    """Gaussian blocks scaled by powers of two from 2^-12 to 2^12: neighbouring scales differ, some elements saturate"""
    g = torch.Generator().manual_seed(7000 + seed)
    x = torch.randn(shape, generator=g).view(shape[0], -1, 32)
    x = x * torch.exp2(torch.randint(-12, 13, x.shape[:2], generator=g).float())[..., None]
    return x.view(shape).to(dtype).to(device)


def check(engine, x, label="", out_dtypes=DTYPES):
    """quant and dequant against the restatement, bit for bit; returns (codes, scales, report)"""
    codes, sc, rep = engine.mx4_quant(x, layer_name=label)
    rc, rs, sat, zeros = restate(x.cpu())
    assert codes.dtype == sc.dtype == torch.uint8 and codes.shape == rc.shape and sc.shape == rs.shape, label
    assert np.array_equal(codes.cpu().numpy(), rc), f"{label}: {int((codes.cpu().numpy() != rc).sum())} of {rc.size} code bytes differ"
    assert np.array_equal(sc.cpu().numpy(), rs), f"{label}: scales differ"
    assert (rep.rows, rep.cols, rep.blocks, rep.zero_blocks, rep.saturated, rep.nonfinite) == (*x.shape, rs.size, zeros, sat, 0), (label, rep)
    for dtype in out_dtypes:
        out = engine.mx4_dequant(codes, sc, dtype, layer_name=label)
        exp = torch.from_numpy(decode(rc, rs).astype(np.float32)).to(dtype)             # (exact, then the one cast)
        assert out.dtype == dtype and out.shape == x.shape, label
        bad = int((raw(out) != raw(exp)).sum())
        assert bad == 0, f"{label} -> {dtype}: {bad} of {exp.numel()} dequantised values differ in their bits"
    return codes, sc, rep


# ---- 1: the conversions, exhaustively --------------------------------------------------------------------------
def check_conversions(engine):
    bf16 = (torch.arange(65536, dtype=torch.int32) - 32768).to(torch.int16).view(torch.bfloat16).float()
    mid = torch.from_numpy(MIDS).float()
    near = torch.cat([mid, torch.nextafter(mid, torch.tensor(9.0)), torch.nextafter(mid, torch.tensor(-9.0))])
    for v in (bf16, torch.cat([near, -near])):
        got, want = engine.mx4_fn("f32_to_e2m1", v).numpy(), to_e2m1(v.double().numpy())
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"f32_to_e2m1({v[bad[0]].item()!r}) = {got[bad[0]]:#x}, expected {want[bad[0]]:#x}"
    codes = torch.arange(16, dtype=torch.uint8)
    want = torch.from_numpy(np.copysign(MAGS[codes.numpy() & 7], np.where(codes.numpy() & 8, -1.0, 1.0))).float()
    assert torch.equal(raw(engine.mx4_fn("e2m1_to_f32", codes)), raw(want)), "e2m1_to_f32 differs on some code"
    s = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    got = engine.mx4_fn("e8m0_to_f32", s)
    assert torch.equal(raw(got[:255]), raw(torch.from_numpy(np.ldexp(1.0, np.arange(255) - 127).astype(np.float32))))
    assert bool(got[255].isnan()) and torch.equal(raw(got), raw(engine.mx4_fn("e8m0_to_f32", s, on_device=False)))
    assert torch.equal(engine.mx4_fn("f32_to_e2m1", bf16, on_device=False), engine.mx4_fn("f32_to_e2m1", bf16))
    a = torch.cat([bf16[bf16.isfinite()], torch.tensor([2.0 ** -149, 2.0 ** -127, 2.0 ** -126, 1.5 * 2.0 ** -124, 2.0 ** -123])])
    assert np.array_equal(engine.mx4_fn("amax_to_e8m0", a).numpy(), scale_of(a.double().abs().numpy()).astype(np.uint8))


# ---- 2: the shapes -----------------------------------------------------------------------------------------------
def check_shapes(engine, rows, dtype, device="cpu"):
    for j, cols in enumerate(COLS):
        check(engine, weights((rows, cols), dtype, seed=j, device=device), f"{rows}x{cols} {dtype}")


def check_views(engine, device="cpu"):
    """views that start one element (one byte) into their storage: no 16-byte access fits, the bytes are the same"""
    for dtype in DTYPES:
        rows, cols = 3, 8224
        flat = weights((1, rows * cols + 32), dtype, seed=11, device=device).view(-1)
        x = flat[1:1 + rows * cols].view(rows, cols)
        codes, sc, _ = check(engine, x, f"offset view {dtype}", out_dtypes=(dtype,))
        shifted = torch.zeros(codes.numel() + sc.numel() + 2, dtype=torch.uint8, device=codes.device)
        c1, s1 = shifted[1:1 + codes.numel()].view(codes.shape), shifted[1 + codes.numel():-1].view(sc.shape)
        c1.copy_(codes), s1.copy_(sc)
        assert torch.equal(raw(engine.mx4_dequant(c1, s1, dtype)), raw(engine.mx4_dequant(codes, sc, dtype)))


# ---- 3: the corners ----------------------------------------------------------------------------------------------
def corner_zero_block(engine, device):
    x = weights((3, 96), torch.float32, seed=20, device=device)
    x[1, 32:64] = 0.0
    x[1, 35] = -0.0
    codes, sc, rep = check(engine, x, "zero block")
    assert int(sc[1, 1]) == 0 and rep.zero_blocks == 1
    assert codes[1, 16:32].cpu().tolist() == [0, 0x80] + [0] * 14      # -0 keeps its sign bit: element 3, a high nibble


def corner_denormals(engine, device):
    g = torch.Generator().manual_seed(21)
    x = (torch.randint(-(2 ** 23) + 1, 2 ** 23, (2, 64), generator=g).double() * 2.0 ** -149).float().to(device)
    x[0, 5] = 2.0 ** -126                                               # a normal maximum beside denormal elements
    _, sc, rep = check(engine, x, "fp32 denormals")
    assert int(sc.max()) == 0 and rep.zero_blocks == 0
    check(engine, x.bfloat16(), "bf16 denormals")


def corner_scale_step(engine, device):
    """a exactly 6, just above 6, just below 8 and 8, times 1 and 2^10: (scale code, the maximum's code, saturated)"""
    for k in (0, 10):
        for a, want in ((6.0, (127, 7, 0)), (float(np.nextafter(np.float32(6), np.float32(9))), (127, 7, 0)),
                        (float(np.nextafter(np.float32(8), np.float32(0))), (127, 7, 1)), (8.0, (128, 6, 0))):
            x = torch.zeros(1, 64, device=device)
            x[0, 33], x[0, 34] = -a * 2.0 ** k, 2.5 * 2.0 ** k
            codes, sc, rep = check(engine, x, f"a = {a!r} 2^{k}")
            assert (int(sc[0, 1]), int(codes[0, 16]) >> 4, rep.saturated) == (want[0] + k, 8 | want[1], want[2]), (a, k)
            assert int(sc[0, 0]) == 0 and rep.zero_blocks == 1


def corner_nonfinite(engine, device):
    for poison in (float("nan"), float("inf"), float("-inf")):
        for dtype in DTYPES:
            x = weights((3, 2080), dtype, seed=23, device=device)
            x[2, 2079] = poison
            with pytest.raises(ValueError, match=r"model\.layers\.7\.mlp\.up_proj\.weight"):
                engine.mx4_quant(x, layer_name="model.layers.7.mlp.up_proj.weight")
    codes, sc, _ = check(engine, weights((3, 2080), seed=24, device=device), "after an error")
    sc[2, 64] = 0xFF
    with pytest.raises(ValueError, match=r"NaN scale code in model\.norm"):
        engine.mx4_dequant(codes, sc, torch.bfloat16, layer_name="model.norm")


def corner_arguments(engine, device):
    from tests.harness import profile_of
    x = weights((3, 64), seed=26, device=device)
    codes, sc, _ = engine.mx4_quant(x)

    def bad_calls():
        for call, what in ((lambda: engine.mx4_quant(x[:, :48].contiguous(), layer_name="w48"), r"w48.*48 columns"),
                           (lambda: engine.mx4_quant(x.view(-1), layer_name="flat"), r"flat.*2-D"),
                           (lambda: engine.mx4_quant(x.double(), layer_name="f64"), r"f64.*float64"),
                           (lambda: engine.mx4_dequant(codes, sc[:, :1], torch.bfloat16, layer_name="w"), r"scales of w.*\[3, 1\].*\[3, 2\] expected"),
                           (lambda: engine.mx4_dequant(codes[:, :24], sc, torch.bfloat16, layer_name="w"), r"codes of w"),
                           (lambda: engine.mx4_dequant(codes, sc, torch.float64, layer_name="w"), r"dtype of w"),
                           (lambda: engine.mx4_dequant(own, sc, torch.bfloat16, out=over, layer_name="w"), r"w: .*overlaps")):
            with pytest.raises(ValueError, match=what):
                call()

    buf = torch.zeros(3 * 64 * 2, dtype=torch.uint8, device=codes.device)      # the output laid over its own codes
    own, over = buf[:codes.numel()].view(codes.shape), buf.view(torch.bfloat16).view(3, 64)
    assert profile_of(engine, bad_calls) == {}
    assert profile_of(engine, lambda: engine.mx4_quant(x)) == {"mx4_quant": 1}
    assert profile_of(engine, lambda: engine.mx4_dequant(codes, sc, torch.float16)) == {"mx4_dequant": 1}
    e = engine.mx4_quant(x[:0])
    assert e[0].numel() == 0 and e[2].blocks == 0 and engine.mx4_dequant(e[0], e[1], torch.float32).numel() == 0


CORNERS = [corner_zero_block, corner_denormals, corner_scale_step, corner_nonfinite, corner_arguments]


# ---- 4: independently of the restatement, in fp64, every element -------------------------------------------------
def check_error_bound(engine, device="cpu"):
    """|x - dq| <= a / 4 where the element did not saturate and < a / 2 where it did, a the block's maximum: the scale
    is at most a / 4 and the widest gap of the grid is 2 scales; a saturated element lies in [7, 8) scales, stored as 6"""
    for dtype in DTYPES:
        x = weights((257, 2080), dtype, seed=30, device=device)
        codes, sc, rep = engine.mx4_quant(x)
        xd = x.cpu().double().numpy()
        a = np.repeat(np.abs(xd).reshape(257, -1, 32).max(-1), 32, axis=1)
        scale = np.ldexp(1.0, np.repeat(sc.cpu().numpy().astype(np.int64) - 127, 32, axis=1))
        sat = np.abs(xd) >= 7 * scale
        err = np.abs(xd - decode(codes.cpu().numpy(), sc.cpu().numpy()))
        print(f"error bound {dtype}: worst |x - dq| / a = {(err / a).max():.6f}, {int(sat.sum())} saturated")
        assert int(sat.sum()) == rep.saturated > 0
        assert bool((err[~sat] <= a[~sat] / 4).all()) and bool((err[sat] < a[sat] / 2).all())


# ---- 5: through the public interface, on the on-disk model of tests/lora_fixtures.py -----------------------------
def run_cli(args):
    from click.testing import CliRunner
    from shardmerge_amd.__main__ import cli
    return CliRunner().invoke(cli, [str(a) for a in args])


def check_commands_and_merge(tmp_path, engine, device):
    """a quantize-mxfp4 output as a finetune_merge entry merges, byte for byte, like its dequantize-mxfp4 output"""
    import asyncio
    from safetensors.torch import load_file, save_file
    from shardmerge_amd import distributed
    from shardmerge_amd.config import MergeConfig
    from shardmerge_amd.index import LocalModelIndex
    from shardmerge_amd.merge import operator_class
    from tests import harness, lora_fixtures as lf
    lf.setup_k3(tmp_path, engine)
    storage = tmp_path / "storage"
    q4 = storage / "org/ft1-mx4"
    for args in (["quantize-mxfp4", "org/ft1", "--out", q4], ["dequantize-mxfp4", "org/ft1-mx4", "--out", storage / "org/ft1-back", "--dtype", "bf16"]):
        res = run_cli(args + ["--storage-dir", storage, "--device", device])
        assert res.exit_code == 0, res.output
    ft1 = lf.model_tensors(1)
    got = {}
    for f in sorted(q4.glob("*.safetensors")):
        got.update(load_file(str(f)))
    quantised = [n for n, t in ft1.items() if t.ndim == 2 and n.endswith(".weight") and n.split(".")[-2].endswith("_proj")]
    assert quantised and sorted(got) == sorted(list(ft1) + [f"{n}_scale" for n in quantised])
    for n, t in ft1.items():
        assert all(np.array_equal(got[k].numpy(), w) for k, w in zip((n, f"{n}_scale"), restate(t))) if n in quantised \
            else torch.equal(raw(got[n]), raw(t)), n
    qc = json.loads((q4 / "config.json").read_text())["quantization_config"]
    assert qc == {"quant_method": "mxfp4", "weight_block_size": [1, 32], "scale_format": "e8m0",
                  "modules_to_not_convert": sorted({n.rsplit(".", 1)[0] for n in set(ft1) - set(quantised)})}
    index = LocalModelIndex(storage_path=storage)
    asyncio.run(index.add_model("org/ft1-mx4"))
    assert index.mx4("org/ft1-mx4") is not None
    for options in ({"operator": "dare_linear", "density": 1.0}, {"operator": "ties", "density": 0.3, "ties_lambda": 0.7}):
        outs = []
        for entry in ("org/ft1-mx4", "org/ft1-back"):
            models = [{"model": entry, "base": "org/base", "alpha": 0.5, "is_input": True},
                      {"model": "org/ft2", "base": "org/base", "alpha": 0.4, "is_output": True}]
            out = f"merged-{options['operator']}-{entry[-4:]}"
            res = harness.run_cli(harness.write_config(tmp_path, models, out, options, device))
            assert res.exit_code == 0, res.output
            assert harness.run_cli(tmp_path / f"{out}.yaml", "analyze").exit_code == 0
            outs.append(tmp_path / out)
        lf.assert_same_outputs(outs[0], outs[1])
        assert not all(torch.equal(raw(a), raw(b)) for a, b in
                       zip(lf.read_outputs(outs[0]).values(), lf.read_outputs(storage / "org/base").values()))
    # an MXFP4 checkpoint as base or output_base_model: rejected in initialize(), nothing written
    for models, obm in (([{"model": "org/ft2", "base": "org/ft1-mx4", "alpha": 0.5, "is_input": True, "is_output": True}], "org/base"),
                        ([{"model": "org/ft2", "base": "org/base", "alpha": 0.5, "is_input": True, "is_output": True}], "org/ft1-mx4")):
        p = harness.write_config(tmp_path, models, "never", {"operator": "ties", "density": 0.3}, device)
        p.write_text(p.read_text().replace("output_base_model: org/base", f"output_base_model: {obm}"))
        cfg = MergeConfig.from_yaml(p)
        with pytest.raises(ValueError, match=r"org/ft1-mx4.*dequantize-mxfp4"):
            asyncio.run(operator_class(cfg.operator)(config=cfg, index_manager=LocalModelIndex(storage_path=storage)).initialize())
        assert harness.run_cli(p).exit_code != 0 and not (tmp_path / "never").exists()
    # the commands' rejections: a DIR that is not empty, a checkpoint quantised twice, a 16-bit model dequantised
    for args in (["quantize-mxfp4", "org/ft2", "--out", q4], ["quantize-mxfp4", "org/ft1-mx4", "--out", storage / "x"],
                 ["dequantize-mxfp4", "org/ft2", "--out", storage / "x"]):
        assert run_cli(args + ["--storage-dir", storage, "--device", device]).exit_code != 0 and not (storage / "x").exists()
    models = [{"model": "org/ft1-mx4", "base": "org/base", "alpha": 0.5, "is_input": True, "is_output": True}]
    cfg = MergeConfig.from_yaml(harness.write_config(tmp_path, models, "stamp", {"operator": "ties", "density": 0.3}, device))
    s0 = distributed.config_stamp(cfg)
    shard = sorted(q4.glob("*.safetensors"))[0]
    save_file(load_file(str(shard)), str(shard), metadata={"format": "pt", "note": "rewritten"})
    assert s0 != distributed.config_stamp(cfg)
    # a mis-shaped and a missing scale, another block size and scale format: rejected naming the model and the tensor or field
    tensors = load_file(str(shard))
    name = next(n for n in tensors if n.endswith("_scale"))
    for doc, what in (({**tensors, name: tensors[name][:, :1].contiguous()}, name), ({k: v for k, v in tensors.items() if k != name}, f"no {name}")):
        save_file(doc, str(shard), metadata={"format": "pt"})
        with pytest.raises(ValueError, match=rf"org/ft1-mx4.*{what}"):
            asyncio.run(LocalModelIndex(storage_path=storage).add_model("org/ft1-mx4"))
    written = (q4 / "config.json").read_text()
    for field, value in (("weight_block_size", [1, 16]), ("scale_format", "fp32")):
        doc = json.loads(written)
        doc["quantization_config"][field] = value
        (q4 / "config.json").write_text(json.dumps(doc))
        with pytest.raises(ValueError, match=rf"org/ft1-mx4.*{field}"):
            asyncio.run(LocalModelIndex(storage_path=storage).add_model("org/ft1-mx4"))


ODDS = ("model.layers.0.mlp.up_proj.weight", "model.layers.1.mlp.up_proj.weight")      # (every layer has the same tensors)
ODD = ODDS[1]                                         # a named module's weight of 80 columns: two blocks and a half


def add_odd_weight(storage, src, dst, which):
    """a copy of the model `src` as `dst` with the tensors ODDS added to its last shard (which = 0: the base's; 1, 2: a
    finetune's); the shared tensors of tests/lora_fixtures.py stay as they are.  Returns the tensor"""
    import shutil
    from safetensors.torch import load_file, save_file
    from tests import lora_fixtures as lf
    shutil.copytree(storage / src, storage / dst)
    index = storage / dst / "model.safetensors.index.json"
    doc = json.loads(index.read_text())
    shard = sorted(set(doc["weight_map"].values()))[-1]
    tensors = load_file(str(storage / dst / shard))
    for j, name in enumerate(ODDS):
        t = lf.randn((64, 80), 900 + j, 0.02)
        tensors[name] = (t + lf.randn((64, 80), 900 + 10 * which + j, 0.003) if which else t).to(torch.bfloat16)
        doc["weight_map"][name] = shard
    save_file(tensors, str(storage / dst / shard), metadata={"format": "pt"})
    index.write_text(json.dumps(doc))
    return {name: tensors[name] for name in ODDS}


def check_odd_columns(tmp_path, engine, device):
    """a named module's weight whose column count is no multiple of 32: `quantize-mxfp4` copies it byte for byte, writes no
    scale for it and lists its module under modules_to_not_convert; `dequantize-mxfp4` and a merge of the result succeed"""
    import asyncio
    from safetensors.torch import load_file
    from shardmerge_amd.index import LocalModelIndex
    from tests import harness, lora_fixtures as lf
    lf.setup_k3(tmp_path, engine)
    storage = tmp_path / "storage"
    odd = [add_odd_weight(storage, f"org/{m}", f"org/{m}-odd", which) for which, m in enumerate(("base", "ft1", "ft2"))]
    assert odd[1][ODD].shape[1] % 32 != 0 and not torch.equal(odd[1][ODD], odd[0][ODD])
    q4, back = storage / "org/ft1-odd-mx4", storage / "org/ft1-odd-back"
    for args in (["quantize-mxfp4", "org/ft1-odd", "--out", q4], ["dequantize-mxfp4", "org/ft1-odd-mx4", "--out", back, "--dtype", "bf16"]):
        res = run_cli(args + ["--storage-dir", storage, "--device", device])
        assert res.exit_code == 0, res.output
    ft1 = dict(lf.model_tensors(1), **odd[1])
    got = {}
    for f in sorted(q4.glob("*.safetensors")):
        got.update(load_file(str(f)))
    quantised = [n for n, t in ft1.items() if t.ndim == 2 and n.split(".")[-2].endswith("_proj") and n not in ODDS]
    assert len(quantised) == 6 and sorted(got) == sorted(list(ft1) + [f"{n}_scale" for n in quantised])     # no scale for ODD
    for n in ODDS:
        assert got[n].dtype == torch.bfloat16 and got[n].shape == odd[1][n].shape and torch.equal(raw(got[n]), raw(odd[1][n])), n
    for n in quantised:
        assert all(np.array_equal(got[k].numpy(), w) for k, w in zip((n, f"{n}_scale"), restate(ft1[n]))), n
    qc = json.loads((q4 / "config.json").read_text())["quantization_config"]
    assert all(n.rsplit(".", 1)[0] in qc["modules_to_not_convert"] for n in ODDS)
    assert qc["modules_to_not_convert"] == sorted({n.rsplit(".", 1)[0] for n in set(ft1) - set(quantised)})
    restored = {}
    for f in sorted(back.glob("*.safetensors")):
        restored.update(load_file(str(f)))
    assert sorted(restored) == sorted(ft1) and all(torch.equal(raw(restored[n]), raw(odd[1][n])) for n in ODDS)
    index = LocalModelIndex(storage_path=storage)
    asyncio.run(index.add_model("org/ft1-odd-mx4"))
    assert index.mx4("org/ft1-odd-mx4") is not None and ODD not in index.mx4("org/ft1-odd-mx4").scale_keys
    outs = []
    for entry in ("org/ft1-odd-mx4", "org/ft1-odd-back", "org/ft1-odd"):
        models = [{"model": entry, "base": "org/base-odd", "alpha": 0.5, "is_input": True},
                  {"model": "org/ft2-odd", "base": "org/base-odd", "alpha": 0.4, "is_output": True}]
        p = harness.write_config(tmp_path, models, f"merged-{entry[-3:]}", {"operator": "ties", "density": 0.3, "ties_lambda": 0.7}, device)
        p.write_text(p.read_text().replace("output_base_model: org/base", "output_base_model: org/base-odd"))
        res = harness.run_cli(p)
        assert res.exit_code == 0, res.output
        outs.append(lf.read_outputs(tmp_path / f"merged-{entry[-3:]}"))
    assert sorted(outs[0]) == sorted(outs[1]) == sorted(ft1) and all(torch.equal(raw(outs[0][n]), raw(outs[1][n])) for n in ft1)
    # the copied tensor merges as the model that was never quantised does, and it does merge: the output is not the base's
    assert torch.equal(raw(outs[0][ODD]), raw(outs[2][ODD])) and not torch.equal(raw(outs[0][ODD]), raw(odd[0][ODD]))
