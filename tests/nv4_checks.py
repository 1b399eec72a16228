"""Checks of NVFP4 shared by the emulator tier (tests/test_nv4_host.py) and the GPU tier (tests/test_nv4_gpu.py): the
engine against a plain restatement of include/shardmerge_hip.h (smhip_nv4_quant), BIT FOR BIT.  The restatement carries
every fp32 operation out as numpy.float32, does the E4M3 step with torch.float8_e4m3fn and picks the nearest of the eight
E2M1 magnitudes by the seven midpoints in fp64.  The tolerance is zero: every step is exact or one rounded operation.
The error bound |x - dq| <= d (1 + 2^-20) on every element that did not saturate is derived - half the widest gap of the
grid, 2, times d, and the roundings of q and of the product - and checked in fp64 on every case."""
import json

import numpy as np
import pytest
import torch

from tests.harness import DTYPES, raw
from tests.mx4_checks import MAGS, to_e2m1

F = np.float32
ROWS = (1, 3, 257)
COLS = (16, 32, 48, 2032, 8208)        # one block; a pair; a lone block behind a pair; 127 and 513 blocks: a partial round
WORST = {"share": 0.0}                  # the largest |x - dq| / d met by check(), for the README


def restate(x):
    """a 2-D CPU tensor as (codes [R, C / 2], scale codes [R, C / 16], g, d [R, C / 16], report fields)"""
    R, C = x.shape
    xb = x.float().numpy().reshape(R, C // 16, 16)                      # the exact promotion
    A = np.abs(xb).max() if xb.size else F(0)
    g = np.maximum(F(A) / F(2688), F(2.0 ** -126))
    a = np.abs(xb).max(-1)
    t = (a / F(6)) / g
    sc = torch.from_numpy(np.minimum(t, F(448))).to(torch.float8_e4m3fn)
    d = sc.float().numpy() * g
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.abs(xb) / d[..., None]
    dead = np.broadcast_to((d == 0)[..., None], q.shape)
    c = np.where(dead, np.signbit(xb) << 3, to_e2m1(np.copysign(q, xb).astype(np.float64))).astype(np.uint8).reshape(R, C)
    fields = dict(blocks=a.size, zero_blocks=int((a == 0).sum()), zero_scale_blocks=int(((a != 0) & (d == 0)).sum()),
                  saturated=int(((q >= 7) & ~dead).sum()), nonfinite=0)
    return c[:, 0::2] | (c[:, 1::2] << 4), sc.view(torch.uint8).numpy(), g, d, fields


def decode(codes, d):
    """the fp32 product of every code with its block's d (numpy): one rounded operation"""
    c = np.stack([codes & 15, codes >> 4], -1).reshape(codes.shape[0], -1)
    mag = np.copysign(MAGS[c & 7], np.where(c & 8, -1.0, 1.0)).astype(F)
    return mag * np.repeat(d, 16, axis=1)


def weights(shape, dtype=torch.bfloat16, seed=0, device="cpu"):
    """Gaussian blocks scaled by powers of two from 2^-7 to 2^7, one element of each at least 2^e: neighbouring scales
    differ, some block scales are E4M3 subnormals that round down (saturation), none underflows (t >= 448 2^-17)"""
    g = torch.Generator().manual_seed(9000 + seed)
    x = torch.randn(shape, generator=g).view(shape[0], -1, 16)
    x[..., 3] = torch.where(x[..., 3] < 0, x[..., 3] - 1, x[..., 3] + 1)
    x = x * torch.exp2(torch.randint(-7, 8, x.shape[:2], generator=g).float())[..., None]
    return x.view(shape).to(dtype).to(device)


def check(engine, x, label="", out_dtypes=DTYPES):
    """quant and dequant against the restatement, bit for bit, and the error bound; returns (codes, scales, g, report)"""
    codes, sc, g, rep = engine.nv4_quant(x, layer_name=label)
    rc, rs, rg, d, fields = restate(x.cpu())
    assert codes.dtype == torch.uint8 and sc.dtype == torch.float8_e4m3fn and g.dtype == torch.float32 and g.shape == (), label
    assert codes.shape == rc.shape and sc.shape == rs.shape, label
    assert F(g.item()).tobytes() == F(rg).tobytes(), f"{label}: g {g.item()!r}, expected {rg!r}"
    assert np.array_equal(sc.cpu().view(torch.uint8).numpy(), rs), f"{label}: scales differ"
    assert np.array_equal(codes.cpu().numpy(), rc), f"{label}: {int((codes.cpu().numpy() != rc).sum())} of {rc.size} code bytes differ"
    got = {k: getattr(rep, k) for k in fields}
    assert (rep.rows, rep.cols) == tuple(x.shape) and got == fields, (label, got, fields)
    dq = decode(rc, d)
    for dtype in out_dtypes:
        out = engine.nv4_dequant(codes, sc, g, dtype, layer_name=label)
        exp = torch.from_numpy(dq).to(dtype)                                    # (the one cast)
        assert out.dtype == dtype and out.shape == x.shape, label
        bad = int((raw(out) != raw(exp)).sum())
        assert bad == 0, f"{label} -> {dtype}: {bad} of {exp.numel()} dequantised values differ in their bits"
    # the bound, in fp64, on every element that did not saturate (a block with d == 0 has no quotient: its elements are
    # below 3 2^-9 g, half the widest gap times the smallest scale that is not zero)
    xd, dd = x.cpu().double().numpy(), np.repeat(d.astype(np.float64), 16, axis=1)
    err = np.abs(xd - dq.astype(np.float64))
    live = (dd > 0) & (np.abs(xd) < 7 * dd)
    assert bool((err[live] <= dd[live] * (1 + 2.0 ** -20)).all()), f"{label}: |x - dq| exceeds d"
    assert bool((np.abs(xd[dd == 0]) <= 3 * 2.0 ** -9 * float(rg) * (1 + 2.0 ** -20)).all()), label
    if live.any():
        WORST["share"] = max(WORST["share"], float((err[live] / dd[live]).max()))
    return codes, sc, g, rep


# ---- 1 and 3: the shapes ---------------------------------------------------------------------------------------------
def check_shapes(engine, rows, dtype, device="cpu"):
    for j, cols in enumerate(COLS):
        check(engine, weights((rows, cols), dtype, seed=j, device=device), f"{rows}x{cols} {dtype}")
    print(f"worst |x - dq| / d so far: {WORST['share']:.6f}")


def check_views(engine, device="cpu"):
    """views that start one element (one byte) into their storage: no 16-byte access fits, the bytes are the same"""
    for dtype in DTYPES:
        rows, cols = 3, 8208
        flat = weights((1, rows * cols + 16), dtype, seed=11, device=device).view(-1)
        codes, sc, g, _ = check(engine, flat[1:1 + rows * cols].view(rows, cols), f"offset view {dtype}", out_dtypes=(dtype,))
        shifted = torch.zeros(codes.numel() + sc.numel() + 2, dtype=torch.uint8, device=codes.device)
        c1, s1 = shifted[1:1 + codes.numel()].view(codes.shape), shifted[1 + codes.numel():-1].view(sc.shape)
        c1.copy_(codes), s1.copy_(sc.view(torch.uint8))
        assert torch.equal(raw(engine.nv4_dequant(c1, s1, g, dtype)), raw(engine.nv4_dequant(codes, sc, g, dtype)))


def check_rounds(engine, device="cpu"):
    """the same bytes at forced round counts: 1, 2 and 3 rounds per work-group (the staged scale sets alternate)"""
    x = weights((3, 8208), seed=12, device=device)
    want = check(engine, x, "rounds 0")
    for c in (1, 2, 3):
        engine.ctx.debug_option("stream_chunks", c)
        try:
            got = check(engine, x, f"rounds {c}", out_dtypes=(torch.bfloat16,))
            assert engine.ctx.debug_query("stream_chunks_applied") == 3     # nv4_amax, nv4_quant, nv4_dequant
        finally:
            engine.ctx.debug_option("stream_chunks", 0)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.uint8), want[1].view(torch.uint8)) and got[2:] == want[2:]


# ---- 2: the corners --------------------------------------------------------------------------------------------------
def corner_zero_tensor(engine, device):
    codes, sc, g, rep = check(engine, torch.zeros(3, 48, device=device), "zeros")
    assert g.item() == 2.0 ** -126 and rep.zero_blocks == rep.blocks == 9 and not codes.any() and not sc.view(torch.uint8).any()


def corner_zero_block(engine, device):
    x = weights((3, 48), torch.float32, seed=20, device=device)
    x[1, 16:32] = 0.0
    x[1, 19] = -0.0
    codes, sc, _, rep = check(engine, x, "zero block")
    assert sc.view(torch.uint8)[1, 1].item() == 0 and (rep.zero_blocks, rep.zero_scale_blocks) == (1, 0)
    assert codes[1, 8:16].cpu().tolist() == [0, 0x80] + [0] * 6        # -0 keeps its sign bit: element 3, a high nibble


def corner_scale_underflow(engine, device):
    """a block so small against A that t < 2^-10: its scale code is 0, d == 0, every code is 0"""
    x = torch.zeros(1, 48, device=device)
    x[0, 0], x[0, 16:32] = 2688.0, 0.004                                # g = 1; t = 0.004 / 6 < 2^-10
    codes, sc, g, rep = check(engine, x, "scale underflow")
    assert g.item() == 1.0 and (rep.zero_blocks, rep.zero_scale_blocks) == (1, 1) and not codes[0, 8:16].any()


def corner_subnormal_scale(engine, device):
    """t = 1.25 2^-9 is an E4M3 subnormal that rounds DOWN to 2^-9: the maximum's quotient is 7.5 and saturates"""
    x = torch.zeros(1, 32, device=device)
    x[0, 0], x[0, 16], x[0, 17] = 2688.0, -7.5 * 2.0 ** -9, 2.0 ** -9
    codes, sc, _, rep = check(engine, x, "subnormal scale")
    assert sc.view(torch.uint8)[0, 1].item() == 1 and rep.saturated == 1 and codes[0, 8].item() == 0x2F   # -6 low, +1 high


def corner_block_max_is_amax(engine, device):
    x = weights((3, 64), seed=22, device=device)
    x[2, 37] = -1.0e4
    codes, sc, _, rep = check(engine, x, "a == A")
    assert sc.view(torch.uint8)[2, 2].item() == 0x7E and codes[2, 18].item() >> 4 == 0xF and rep.saturated == 0


def corner_errors(engine, device):
    name = "model.layers.7.mlp.up_proj.weight"
    for poison in (float("nan"), float("inf"), float("-inf")):
        for dtype in DTYPES:
            x = weights((3, 2032), dtype, seed=23, device=device)
            x[2, 2031] = poison
            with pytest.raises(ValueError, match=r"model\.layers\.7\.mlp\.up_proj\.weight"):
                engine.nv4_quant(x, layer_name=name)
    x = weights((3, 2032), seed=24, device=device)
    codes, sc, g, _ = check(engine, x, "after an error")
    bad = sc.clone()
    bad.view(torch.uint8)[2, 126] = 0xFF
    for call, what in ((lambda: engine.nv4_dequant(codes, bad, g, layer_name=name), r"NaN scale code in model\.layers\.7"),
                       (lambda: engine.nv4_dequant(codes, sc, 0.0, layer_name=name), r"up_proj\.weight.*not finite and positive"),
                       (lambda: engine.nv4_dequant(codes, sc, float("inf"), layer_name=name), r"up_proj\.weight.*not finite and positive"),
                       (lambda: engine.nv4_quant(x[:, :24].contiguous(), layer_name="w24"), r"w24.*24 columns"),
                       (lambda: engine.nv4_dequant(codes, sc[:, :1], g, layer_name="w"), r"scales of w.*\[3, 1\].*\[3, 127\] expected")):
        with pytest.raises(ValueError, match=what):
            call()


CORNERS = [corner_zero_tensor, corner_zero_block, corner_scale_underflow, corner_subnormal_scale, corner_block_max_is_amax,
           corner_errors]


# ---- 4: through the public interface, on the on-disk model of tests/lora_fixtures.py ---------------------------------
def run_cli(args):
    from click.testing import CliRunner
    from shardmerge_amd.__main__ import cli
    return CliRunner().invoke(cli, [str(a) for a in args])


def check_commands_and_merge(tmp_path, engine, device):
    """a quantize-nvfp4 output as a finetune_merge entry merges, byte for byte, like its dequantize-nvfp4 output"""
    import asyncio
    from safetensors.torch import load_file, save_file
    from shardmerge_amd import distributed
    from shardmerge_amd.config import MergeConfig
    from shardmerge_amd.index import LocalModelIndex
    from shardmerge_amd.merge import operator_class
    from tests import harness, lora_fixtures as lf
    lf.setup_k3(tmp_path, engine)
    storage = tmp_path / "storage"
    q4 = storage / "org/ft1-nv4"
    for args in (["quantize-nvfp4", "org/ft1", "--out", q4], ["dequantize-nvfp4", "org/ft1-nv4", "--out", storage / "org/ft1-back", "--dtype", "bf16"],
                 ["quantize-fp8", "org/ft2", "--out", storage / "org/ft2-fp8"]):
        res = run_cli(args + ["--storage-dir", storage, "--device", device])
        assert res.exit_code == 0, res.output
    ft1 = lf.model_tensors(1)
    got = {}
    for f in sorted(q4.glob("*.safetensors")):
        got.update(load_file(str(f)))
    quantised = [n for n, t in ft1.items() if t.ndim == 2 and n.endswith(".weight") and n.split(".")[-2].endswith("_proj")]
    assert quantised and sorted(got) == sorted(list(ft1) + [f"{n}_scale{s}" for n in quantised for s in ("", "_2")])
    for n, t in ft1.items():
        if n in quantised:
            rc, rs, rg, _, _ = restate(t)
            assert np.array_equal(got[n].numpy(), rc) and np.array_equal(got[f"{n}_scale"].view(torch.uint8).numpy(), rs), n
            assert got[f"{n}_scale_2"].dtype == torch.float32 and got[f"{n}_scale_2"].item() == float(rg), n
        else:
            assert torch.equal(raw(got[n]), raw(t)), n
    qc = json.loads((q4 / "config.json").read_text())["quantization_config"]
    assert qc == {"quant_method": "modelopt", "quant_algo": "NVFP4", "group_size": 16,
                  "ignore": sorted({n.rsplit(".", 1)[0] for n in set(ft1) - set(quantised)})}
    index = LocalModelIndex(storage_path=storage)
    asyncio.run(index.add_model("org/ft1-nv4")), asyncio.run(index.add_model("org/ft2-fp8"))
    assert index.nv4("org/ft1-nv4") is not None and index.fp8("org/ft1-nv4") is None
    assert index.fp8("org/ft2-fp8") is not None and index.nv4("org/ft2-fp8") is None      # an FP8 checkpoint stays one
    for options in ({"operator": "dare_linear", "density": 1.0}, {"operator": "ties", "density": 0.3, "ties_lambda": 0.7}):
        outs = []
        for entry in ("org/ft1-nv4", "org/ft1-back"):
            models = [{"model": entry, "base": "org/base", "alpha": 0.5, "is_input": True},
                      {"model": "org/ft2", "base": "org/base", "alpha": 0.4, "is_output": True}]
            out = f"merged-{options['operator']}-{entry[-4:]}"
            res = harness.run_cli(harness.write_config(tmp_path, models, out, options, device))
            assert res.exit_code == 0, res.output
            outs.append(tmp_path / out)
        lf.assert_same_outputs(outs[0], outs[1])
        assert not all(torch.equal(raw(a), raw(b)) for a, b in
                       zip(lf.read_outputs(outs[0]).values(), lf.read_outputs(storage / "org/base").values()))
    # an NVFP4 checkpoint as base or output_base_model: rejected in initialize(), nothing written
    for models, obm in (([{"model": "org/ft2", "base": "org/ft1-nv4", "alpha": 0.5, "is_input": True, "is_output": True}], "org/base"),
                        ([{"model": "org/ft2", "base": "org/base", "alpha": 0.5, "is_input": True, "is_output": True}], "org/ft1-nv4")):
        p = harness.write_config(tmp_path, models, "never", {"operator": "ties", "density": 0.3}, device)
        p.write_text(p.read_text().replace("output_base_model: org/base", f"output_base_model: {obm}"))
        cfg = MergeConfig.from_yaml(p)
        with pytest.raises(ValueError, match=r"org/ft1-nv4.*dequantize-nvfp4"):
            asyncio.run(operator_class(cfg.operator)(config=cfg, index_manager=LocalModelIndex(storage_path=storage)).initialize())
        assert harness.run_cli(p).exit_code != 0 and not (tmp_path / "never").exists()
    models = [{"model": "org/ft1-nv4", "base": "org/base", "alpha": 0.5, "is_input": True, "is_output": True}]
    cfg = MergeConfig.from_yaml(harness.write_config(tmp_path, models, "stamp", {"operator": "ties", "density": 0.3}, device))
    s0 = distributed.config_stamp(cfg)
    shard = sorted(q4.glob("*.safetensors"))[0]
    save_file(load_file(str(shard)), str(shard), metadata={"format": "pt", "note": "rewritten"})
    assert s0 != distributed.config_stamp(cfg)
    # a mis-shaped and a missing scale, an FP8 and an MXFP4 weight mixed in, another group size: rejected naming the
    # model and the tensor or field
    tensors = load_file(str(shard))
    name = next(n for n in tensors if n.endswith("_scale"))
    fp8w = {"extra.weight": torch.zeros(4, 4).to(torch.float8_e4m3fn), "extra.weight_scale_inv": torch.ones(1, 1)}
    for doc, what in (({**tensors, name: tensors[name][:, :1].contiguous()}, name), ({k: v for k, v in tensors.items() if k != name}, f"no {name}"),
                      ({k: v for k, v in tensors.items() if k != name + "_2"}, f"no {name}_2"), ({**tensors, **fp8w}, "extra.weight.*mixed"),
                      ({**tensors, name: tensors[name].view(torch.uint8)}, f"{name}.*mixed")):
        save_file(doc, str(shard), metadata={"format": "pt"})
        with pytest.raises(ValueError, match=rf"org/ft1-nv4.*{what}"):
            asyncio.run(LocalModelIndex(storage_path=storage).add_model("org/ft1-nv4"))
    save_file(tensors, str(shard), metadata={"format": "pt"})
    doc = json.loads((q4 / "config.json").read_text())
    doc["quantization_config"]["group_size"] = 32
    (q4 / "config.json").write_text(json.dumps(doc))
    with pytest.raises(ValueError, match=r"org/ft1-nv4.*group_size"):
        asyncio.run(LocalModelIndex(storage_path=storage).add_model("org/ft1-nv4"))
