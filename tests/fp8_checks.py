"""Checks of block-scaled FP8 shared by the emulator tier (tests/test_fp8_host.py) and the GPU tier
(tests/test_fp8_gpu.py): Engine.fp8_fn, fp8_quant and fp8_dequant against torch on the CPU, BIT FOR BIT.  The tolerance
is zero and it is derived: the block maximum is exact, the scale and every code are one rounded fp32 division each and
the conversion is round-to-nearest-even on a stated grid (include/shardmerge_hip.h, smhip_fp8_quant), which is what
`a / 448`, `(x / s).to(torch.float8_e4m3fn)` and `(q.float() * s).to(dtype)` compute on the CPU - torch's conversion
agrees with f32_to_e4m3 for every |v| < 464 and |x / s| <= 448 (1 + 2^-23).  Then, independently of that restatement,
the error bound of the format in fp64."""
import json
import math

import pytest
import torch

from tests.harness import DTYPES, f32_bits, raw

ROWS = (1, 127, 128, 129, 257)
COLS = (1, 7, 8, 9, 120, 127, 128, 129, 136, 264)
F8 = torch.float8_e4m3fn
TINY = 2.0 ** -126


def restate(x):
    """(codes as uint8, scale_inv, the scale of every element, the blocks' maxima) of a 2-D CPU tensor: the three lines of torch"""
    R, C = x.shape
    br, bc = -(-R // 128), -(-C // 128)
    pad = torch.zeros(br * 128, bc * 128)
    pad[:R, :C] = x.float().abs()
    a = pad.view(br, 128, bc, 128).amax(dim=(1, 3))
    s = torch.clamp(a / 448, min=TINY)
    sb = s.repeat_interleave(128, 0).repeat_interleave(128, 1)[:R, :C]
    return (x.float() / sb).to(F8).view(torch.uint8), s, sb, a


def weights(shape, dtype=torch.bfloat16, seed=0, device="cpu"):
    """Gaussian data at sigma 0.02; the first block is scaled by 2^10 and the last by 2^-10, so the scales differ by
    block and a lookup into the wrong block shows"""
    g = torch.Generator().manual_seed(4000 + seed)
    x = torch.randn(shape, generator=g) * 0.02
    x[:128, :128] *= 2.0 ** 10
    x[-(((shape[0] - 1) % 128) + 1):, -(((shape[1] - 1) % 128) + 1):] *= 2.0 ** -10
    return x.to(dtype).to(device)


def check(engine, x, label="", out_dtypes=DTYPES):
    """quant and dequant against the restatement, bit for bit; returns (codes, scale_inv, report)"""
    codes, sc, rep = engine.fp8_quant(x, name=label)
    rc, rs, sb, a = restate(x.cpu())
    assert codes.dtype == F8 and codes.shape == x.shape and sc.dtype == torch.float32 and sc.shape == rs.shape, label
    bad = int((codes.cpu().view(torch.uint8) != rc).sum())
    assert bad == 0, f"{label}: {bad} of {rc.numel()} codes differ"
    assert torch.equal(raw(sc), raw(rs)), f"{label}: scales differ in their bits"
    assert (rep.rows, rep.cols, rep.blocks, rep.zero_blocks, f32_bits(rep.amax), rep.flags) == \
        (x.shape[0], x.shape[1], rs.numel(), int((a == 0).sum()), f32_bits(a.max().item()), 0), (label, rep)
    for dtype in out_dtypes:
        out = engine.fp8_dequant(codes, sc, dtype, name=label)
        exp = (rc.view(F8).float() * sb).to(dtype)
        assert out.dtype == dtype and out.shape == x.shape, label
        bad = int((raw(out) != raw(exp)).sum())
        assert bad == 0, f"{label} -> {dtype}: {bad} of {exp.numel()} dequantised values differ in their bits"
    return codes, sc, rep


# ---- 1: the conversions, exhaustively --------------------------------------------------------------------------
def check_conversions(engine, device="cpu"):
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    dec = engine.fp8_fn("e4m3_to_f32", codes)
    assert torch.equal(raw(dec), raw(codes.view(F8).float())), "e4m3_to_f32 differs from torch on some code"
    grid = codes[:127].view(F8).float()                                  # the non-negative finite values, ascending
    mid = ((grid[:-1].double() + grid[1:].double()) / 2).float()        # exact: one more mantissa bit
    assert mid.numel() == 126 and torch.equal(mid.double() * 2, grid[:-1].double() + grid[1:].double())
    up, down = torch.nextafter(mid, torch.tensor(math.inf)), torch.nextafter(mid, torch.tensor(-math.inf))
    pos = torch.cat([mid, up, down])
    bf16 = (torch.arange(65536, dtype=torch.int32) - 32768).to(torch.int16).view(torch.bfloat16).float()
    for v in (bf16, torch.cat([pos, -pos])):
        got = engine.fp8_fn("f32_to_e4m3", v)
        a = v.abs()
        want = torch.where(a < 464, v.clamp(-463, 463).to(F8).view(torch.uint8),
                           torch.where(v < 0, torch.tensor(0xFE, dtype=torch.uint8), torch.tensor(0x7E, dtype=torch.uint8)))
        want = torch.where(v.isnan(), torch.tensor(0x7F, dtype=torch.uint8), want)
        bad = (got != want).nonzero().flatten()
        assert bad.numel() == 0, f"f32_to_e4m3({v[bad[0]].item()!r}) = {int(got[bad[0]]):#x}, expected {int(want[bad[0]]):#x}"
    host = engine.fp8_fn("f32_to_e4m3", bf16, on_device=False)
    assert torch.equal(host, engine.fp8_fn("f32_to_e4m3", bf16))


# ---- 2: the grid -------------------------------------------------------------------------------------------------
def check_grid(engine, rows, dtype, device="cpu"):
    for j, cols in enumerate(COLS):
        check(engine, weights((rows, cols), dtype, seed=j, device=device), f"{rows}x{cols} {dtype}")


def check_views(engine, device="cpu"):
    """a view that starts one element into its storage (no vector access fits) with a row pitch that is no multiple of
    8, and one of a pitch that is: every path of both kernels against the same restatement"""
    for dtype in DTYPES:
        for rows, cols in ((129, 136), (130, 129)):
            flat = weights((1, rows * cols + 8), dtype, seed=11, device=device).view(-1)
            x = flat[1:1 + rows * cols].view(rows, cols)
            codes, sc, _ = check(engine, x, f"offset view {dtype} {rows}x{cols}", out_dtypes=(dtype,))
            shifted = torch.zeros(rows * cols + 8, dtype=torch.uint8, device=codes.device)
            shifted[1:1 + rows * cols] = codes.view(torch.uint8).view(-1)
            out = engine.fp8_dequant(shifted[1:1 + rows * cols].view(rows, cols).view(F8), sc, dtype)
            assert torch.equal(raw(out), raw(engine.fp8_dequant(codes, sc, dtype)))


# ---- 3: the corners ----------------------------------------------------------------------------------------------
def corner_zero_block(engine, device):
    x = weights((129, 256), torch.float32, seed=20, device=device)
    x[:128, 128:] = 0.0
    x[5, 130] = -0.0
    codes, sc, rep = check(engine, x, "zero block")
    assert f32_bits(float(sc[0, 1])) == f32_bits(TINY) and rep.zero_blocks == 1
    assert int((codes[:128, 128:].cpu().view(torch.uint8) & 0x7F).sum()) == 0


def corner_smallest_denormal(engine, device):
    x = torch.zeros(128, 128, device=device)
    x[17, 93] = 2.0 ** -149
    codes, sc, rep = check(engine, x, "smallest denormal")
    assert f32_bits(float(sc[0, 0])) == f32_bits(TINY) and rep.zero_blocks == 0 and rep.amax == 2.0 ** -149
    assert int(codes.cpu().view(torch.uint8).sum()) == 0


def corner_amax(engine, device):
    for dtype in DTYPES:
        x = torch.zeros(128, 136, dtype=dtype, device=device)
        x[0, 0], x[127, 127], x[64, 3], x[1, 130] = 0.75, -0.75, 0.375, 3.0
        codes, sc, rep = check(engine, x, f"amax {dtype}")
        c = codes.cpu().view(torch.uint8)
        assert (int(c[0, 0]), int(c[127, 127]), int(c[64, 3]), int(c[1, 130])) == (0x7E, 0xFE, 0x76, 0x7E) and rep.amax == 3.0


def corner_nonfinite(engine, device):
    for poison in (float("nan"), float("inf"), float("-inf")):
        for dtype in DTYPES:
            x = weights((130, 136), dtype, seed=23, device=device)
            x[129, 131] = poison
            with pytest.raises(ValueError, match=r"model\.layers\.7\.mlp\.up_proj\.weight"):
                engine.fp8_quant(x, name="model.layers.7.mlp.up_proj.weight")
    check(engine, weights((130, 136), seed=24, device=device), "after an error")


def corner_nan_code(engine, device):
    codes, sc, _ = engine.fp8_quant(weights((130, 136), seed=25, device=device))
    for nan, at in ((0x7F, (129, 135)), (0xFF, (0, 0))):
        c = codes.clone().view(torch.uint8)
        c[at] = nan
        with pytest.raises(ValueError, match=r"NaN code in model\.norm"):
            engine.fp8_dequant(c.view(F8), sc, torch.bfloat16, name="model.norm")
    engine.fp8_dequant(codes, sc, torch.bfloat16)


def corner_arguments(engine, device):
    from tests.harness import profile_of
    x = weights((130, 136), seed=26, device=device)
    codes, sc, _ = engine.fp8_quant(x)

    def bad_calls():
        with pytest.raises(ValueError, match=r"scale_inv.*\[2, 1\].*\[2, 2\] expected"):
            engine.fp8_dequant(codes, sc[:, :1], torch.bfloat16)
        with pytest.raises(ValueError, match="scale_inv"):
            engine.fp8_dequant(codes, sc.double(), torch.bfloat16)
        with pytest.raises(ValueError, match="64 x 64 is not 128 x 128"):
            engine.fp8_quant(x, block=(64, 64))
        with pytest.raises(ValueError, match="128 x 64 is not 128 x 128"):
            engine.fp8_dequant(codes, sc, torch.bfloat16, block=(128, 64))
        with pytest.raises(ValueError, match="dtype"):
            engine.fp8_dequant(codes, sc, torch.float64)
        with pytest.raises(ValueError, match="2-D"):
            engine.fp8_quant(x.view(-1))

    assert profile_of(engine, bad_calls) == {}
    assert profile_of(engine, lambda: engine.fp8_quant(x)) == {"fp8_quant": 1}
    assert profile_of(engine, lambda: engine.fp8_dequant(codes, sc, torch.float16)) == {"fp8_dequant": 1}
    e = engine.fp8_quant(x[:0])
    assert e[0].numel() == 0 and e[2].blocks == 0 and engine.fp8_dequant(e[0], e[1], torch.float32).numel() == 0


CORNERS = [corner_zero_block, corner_smallest_denormal, corner_amax, corner_nonfinite, corner_nan_code, corner_arguments]


# ---- 4: independently of the restatement, in fp64 ----------------------------------------------------------------
def check_error_bound(engine, device="cpu"):
    """|x - e4m3_to_f32(code) s| <= max(2^-4 |x|, 2^-10 s) (1 + 2^-20): half an ulp of three mantissa bits, or half the
    subnormal step; the roundings of the fp32 division and product are inside the margin.  The block maximum is
    reproduced within 2^-23 relative (its code is +-448 exactly and s 448 is a / 448 * 448)."""
    for dtype in DTYPES:
        x = weights((257, 264), dtype, seed=30, device=device)
        codes, sc, _ = engine.fp8_quant(x)
        xd = x.cpu().double()
        s = sc.cpu().double().repeat_interleave(128, 0).repeat_interleave(128, 1)[:257, :264]
        dq = engine.fp8_fn("e4m3_to_f32", codes.cpu().view(torch.uint8).view(-1)).view(257, 264).double() * s
        bound = torch.maximum(2.0 ** -4 * xd.abs(), 2.0 ** -10 * s) * (1 + 2.0 ** -20)
        worst = ((xd - dq).abs() / bound).max().item()
        print(f"error bound {dtype}: worst |x - dq| / bound = {worst:.6f}")
        assert worst <= 1.0
        pad = torch.zeros(3 * 128, 3 * 128, dtype=torch.float64)
        pad[:257, :264] = xd.abs()
        a = pad.view(3, 128, 3, 128).amax(dim=(1, 3))
        pad[:257, :264] = dq.abs()
        got = pad.view(3, 128, 3, 128).amax(dim=(1, 3))
        assert bool(((got - a).abs() <= 2.0 ** -23 * a).all())


# ---- 5: through the public interface, on the on-disk model of tests/lora_fixtures.py -----------------------------
MODULES = "q_proj,k_proj,v_proj,o_proj,gate_proj,up_proj,down_proj"


def run_cli(args):
    from click.testing import CliRunner
    from shardmerge_amd.__main__ import cli
    return CliRunner().invoke(cli, [str(a) for a in args])


def check_commands_and_merge(tmp_path, engine, device):
    """quantize-fp8 of a finetune; the result as a finetune_merge entry under dare_linear at density 1 and under ties
    equals, byte for byte, the same merge with the entry replaced by its dequantize-fp8 output"""
    import asyncio
    from safetensors.torch import load_file
    from shardmerge_amd.config import MergeConfig
    from shardmerge_amd.index import LocalModelIndex
    from shardmerge_amd.merge import operator_class
    from tests import harness
    from tests import lora_fixtures as lf
    lf.setup_k3(tmp_path, engine)
    storage = tmp_path / "storage"
    res = run_cli(["quantize-fp8", "org/ft1", "--out", storage / "org/ft1-fp8", "--storage-dir", storage, "--device", device])
    assert res.exit_code == 0, res.output
    res = run_cli(["dequantize-fp8", "org/ft1-fp8", "--out", storage / "org/ft1-back", "--storage-dir", storage,
                   "--dtype", "bf16", "--device", device])
    assert res.exit_code == 0, res.output
    # the written shards and the config block
    ft1 = lf.model_tensors(1)
    got = {}
    for f in sorted((storage / "org/ft1-fp8").glob("*.safetensors")):
        got.update(load_file(str(f)))
    quantised = [n for n, t in ft1.items() if t.ndim == 2 and n.endswith(".weight") and n.split(".")[-2] in MODULES.split(",")]
    assert quantised and sorted(got) == sorted(list(ft1) + [f"{n}_scale_inv" for n in quantised])
    for n in quantised:
        rc, rs = restate(ft1[n])[:2]
        assert got[n].dtype == F8 and torch.equal(got[n].view(torch.uint8), rc) and torch.equal(raw(got[f"{n}_scale_inv"]), raw(rs))
    for n in set(ft1) - set(quantised):
        assert torch.equal(raw(got[n]), raw(ft1[n])), n
    qc = json.loads((storage / "org/ft1-fp8" / "config.json").read_text())["quantization_config"]
    assert (qc["quant_method"], qc["fmt"], qc["weight_block_size"], qc["activation_scheme"]) == ("fp8", "e4m3", [128, 128], "dynamic")
    assert sorted(qc["modules_to_not_convert"]) == sorted({n.rsplit(".", 1)[0] for n in set(ft1) - set(quantised)})
    index = LocalModelIndex(storage_path=storage)
    asyncio.run(index.add_model("org/ft1-fp8"))
    assert index.fp8("org/ft1-fp8") is not None and index.fp8("org/ft1-back") is None
    # the merges
    for options in ({"operator": "dare_linear", "density": 1.0}, {"operator": "ties", "density": 0.3, "ties_lambda": 0.7}):
        outs = []
        for entry in ("org/ft1-fp8", "org/ft1-back"):
            models = [{"model": entry, "base": "org/base", "alpha": 0.5, "is_input": True},
                      {"model": "org/ft2", "base": "org/base", "alpha": 0.4, "is_output": True}]
            out = f"merged-{options['operator']}-{entry[-4:]}"
            res = harness.run_cli(harness.write_config(tmp_path, models, out, options, device))
            assert res.exit_code == 0, res.output
            assert harness.run_cli(tmp_path / f"{out}.yaml", "analyze").exit_code == 0
            outs.append(tmp_path / out)
        lf.assert_same_outputs(outs[0], outs[1])
        assert not all(torch.equal(raw(a), raw(b)) for a, b in
                       zip(lf.read_outputs(outs[0]).values(), lf.read_outputs(tmp_path / "storage" / "org/base").values()))
    # an FP8 checkpoint as base or output_base_model: rejected in initialize(), nothing written
    for models, obm in (([{"model": "org/ft2", "base": "org/ft1-fp8", "alpha": 0.5, "is_input": True, "is_output": True}], "org/base"),
                        ([{"model": "org/ft2", "base": "org/base", "alpha": 0.5, "is_input": True, "is_output": True}], "org/ft1-fp8")):
        p = harness.write_config(tmp_path, models, "never", {"operator": "ties", "density": 0.3}, device)
        doc = p.read_text().replace("output_base_model: org/base", f"output_base_model: {obm}")
        p.write_text(doc)
        cfg = MergeConfig.from_yaml(p)
        with pytest.raises(ValueError, match=r"org/ft1-fp8.*dequantize-fp8"):
            asyncio.run(operator_class(cfg.operator)(config=cfg, index_manager=LocalModelIndex(storage_path=storage)).initialize())
        res = harness.run_cli(p)
        assert res.exit_code != 0 and not (tmp_path / "never").exists()
    # the stamp follows the scales
    from shardmerge_amd import distributed
    models = [{"model": "org/ft1-fp8", "base": "org/base", "alpha": 0.5, "is_input": True, "is_output": True}]
    cfg = MergeConfig.from_yaml(harness.write_config(tmp_path, models, "stamp", {"operator": "ties", "density": 0.3}, device))
    s0 = distributed.config_stamp(cfg)
    res = run_cli(["quantize-fp8", "org/ft2", "--out", storage / "org/ft1-fp8", "--storage-dir", storage, "--device", device])
    assert res.exit_code != 0                                     # an existing directory is not overwritten
    assert s0 == distributed.config_stamp(cfg)
    from safetensors.torch import save_file
    shard = sorted((storage / "org/ft1-fp8").glob("*.safetensors"))[0]
    save_file(load_file(str(shard)), str(shard), metadata={"format": "pt", "note": "rewritten"})
    assert s0 != distributed.config_stamp(cfg)
