"""Checks of GPTQ-layout INT4 shared by the emulator tier (tests/test_gptq_host.py) and the GPU tier
(tests/test_gptq_gpu.py): the engine against a plain restatement of include/shardmerge_hip.h (smhip_gptq_quant,
smhip_gptq_dequant), BIT FOR BIT.  The restatement carries every operation out as numpy.float32 / numpy.float16 and packs
with integer shifts.  The tolerance is zero: every step is exact or one rounded operation.
The error bound, derived in the header, on the fp32 value dq = (q - z) s16, checked in fp64 on every element: s16 / 2 where
the element was not clipped; s16 (1/2 + 15 * 2^-11) where it was and s16 is a normal fp16 number no clamp moved (the fp16
rounding of s stretches the range); s16 / 2 + 15 * 2^-25 where s16 is subnormal or was raised to 2^-24; each times
1 + 2^-17 for the fp32 roundings.  A clipped element of a group whose scale the upper clamp lowered has no bound."""
import json

import numpy as np
import pytest
import torch

from tests.harness import DTYPES, raw

F = np.float32
GROUPS = (32, 64, 128)
ROWS = (8, 72, 136)                     # a partial tile; a second, partial tile; a third
SHIFTS = (4 * np.arange(8)).astype(np.uint32)
WORST = {"share": 0.0, "clipped_share": 0.0}   # the largest |x - dq| / (s16 / 2) met by check(), for the README


def pack8(v):
    """[..., 8 n] integers 0 .. 15 as [..., n] words, element e of an octet at bits 4 e"""
    v = v.astype(np.uint32).reshape(v.shape[:-1] + (-1, 8))
    return (v << SHIFTS).sum(-1, dtype=np.uint32).view(np.int32)


def restate(x, g):
    """a 2-D CPU tensor as (qweight [C / 8, R], qzeros [C / g, R / 8], scales [C / g, R], g_idx, dq [R, C] fp32, s, report)"""
    R, C = x.shape
    xg = x.float().numpy().reshape(R, C // g, g)                        # the exact promotion
    mn, mx = np.minimum(xg.min(-1), F(0)), np.maximum(xg.max(-1), F(0))
    with np.errstate(over="ignore", divide="ignore"):
        s = (mx - mn) / F(15)
        h = s.astype(np.float16)
        s16h = np.clip(h, np.float16(2.0 ** -24), np.float16(65504))
        s16 = s16h.astype(F)
        z = np.clip(np.rint((F(0) - mn) / s16), 0, 15)
        t = np.rint(xg / s16[..., None]) + z[..., None]
    q = np.clip(t, 0, 15)
    zero = (mn == 0) & (mx == 0)
    fields = dict(groups=R * C // g, zero_groups=int(zero.sum()), scale_clamped=int(((s16h != h) & ~zero).sum()),
                  clipped=int(((t < 0) | (t > 15)).sum()), nonfinite=0)
    dq = ((q - z[..., None]).astype(F) * s16[..., None]).reshape(R, C)
    clipped = ((t < 0) | (t > 15)).reshape(R, C)
    return (np.ascontiguousarray(pack8(q.reshape(R, C)).T), pack8((z.T.astype(np.int64) - 1) & 15), np.ascontiguousarray(s16h.T),
            (np.arange(C) // g).astype(np.int32), dq, (s, s16, clipped), fields)


def weights(shape, g, dtype=torch.bfloat16, seed=0, device="cpu"):
    """Gaussian groups scaled by powers of two from 2^-9 to 2^3 and shifted off centre, so neighbouring scales and
    zero-points differ and the fp16 rounding of some scales clips an extreme; every 7th group one-sided"""
    gen = torch.Generator().manual_seed(9100 + seed)
    x = torch.randn(shape, generator=gen).view(shape[0], -1, g)
    x = (x + torch.randn(x.shape[:2], generator=gen)[..., None]) * torch.exp2(torch.randint(-9, 4, x.shape[:2], generator=gen).float())[..., None]
    x.view(-1, g)[::7] = x.view(-1, g)[::7].abs()
    return x.view(shape).to(dtype).to(device)


def check(engine, x, g, label="", out_dtypes=DTYPES):
    """quant and dequant against the restatement, bit for bit, and the error bound; returns what gptq_quant returned"""
    got = engine.gptq_quant(x, g, layer_name=label)
    qweight, qzeros, scales, g_idx, rep = got
    rw, rz, rs, rg, dq, (s, s16, clipped), fields = restate(x.cpu(), g)
    assert (qweight.dtype, qzeros.dtype, scales.dtype, g_idx.dtype) == (torch.int32, torch.int32, torch.float16, torch.int32), label
    for name, a, b in (("qweight", qweight, rw), ("qzeros", qzeros, rz), ("scales", scales.view(torch.int16), rs.view(np.int16)), ("g_idx", g_idx, rg)):
        assert tuple(a.shape) == b.shape, (label, name, a.shape, b.shape)
        assert np.array_equal(a.cpu().numpy(), b), f"{label}: {int((a.cpu().numpy() != b).sum())} of {b.size} words of {name} differ"
    seen = {k: getattr(rep, k) for k in fields}
    assert (rep.rows, rep.cols, rep.group_size) == (*x.shape, g) and seen == fields, (label, seen, fields)
    for dtype in out_dtypes:
        out = engine.gptq_dequant(qweight, qzeros, scales, g_idx, dtype, layer_name=label)
        exp = torch.from_numpy(dq).to(dtype)                                    # (the one cast)
        assert out.dtype == dtype and out.shape == x.shape, label
        bad = int((raw(out) != raw(exp)).sum())
        assert bad == 0, f"{label} -> {dtype}: {bad} of {exp.numel()} dequantised values differ in their bits"
    # the bound, in fp64, on every element
    rep64 = lambda a: np.repeat(a.astype(np.float64), g, axis=1)
    err, sd, hd = np.abs(x.cpu().double().numpy() - dq.astype(np.float64)), rep64(s), rep64(s16)
    normal = (hd >= 2.0 ** -14) & (np.abs(sd - hd) <= hd * 2.0 ** -11)          # a normal fp16 number no clamp moved
    bound = np.where(~clipped, hd / 2, np.where(normal, hd * (0.5 + 15 * 2.0 ** -11), hd / 2 + 15 * 2.0 ** -25))
    held = ~clipped | (sd <= 65520.0)                                           # (above: the upper clamp, no bound)
    print(f"{label}: worst |x - dq| / (s16 / 2): not clipped {(err / hd * 2)[~clipped].max(initial=0):.6f}, "
          f"clipped {(err / hd * 2)[clipped & held].max(initial=0):.6f} of {int(clipped.sum())}")
    assert bool((err[held] <= bound[held] * (1 + 2.0 ** -17)).all()), f"{label}: |x - dq| exceeds its bound"
    WORST["share"] = max(WORST["share"], float((err / hd * 2)[~clipped].max(initial=0)))
    WORST["clipped_share"] = max(WORST["clipped_share"], float((err / hd * 2)[clipped & held].max(initial=0)))
    return got


# ---- the conversions -------------------------------------------------------------------------------------------------
def check_shapes(engine, g, dtype, device="cpu"):
    for i, rows in enumerate(ROWS):
        for j, cols in enumerate((g, 3 * g, 17 * g)):
            check(engine, weights((rows, cols), g, dtype, seed=3 * i + j, device=device), g, f"{rows}x{cols} g{g} {dtype}")
    print(f"worst shares so far: {WORST}")


def check_views(engine, device="cpu"):
    """views that start one element into their storage: no 16-byte access fits, the bytes are the same"""
    rows, cols, g = 72, 192, 64
    for dtype in DTYPES:
        flat = weights((1, rows * cols + 64), g, dtype, seed=11, device=device).view(-1)
        four = check(engine, flat[1:1 + rows * cols].view(rows, cols), g, f"offset view {dtype}", out_dtypes=(dtype,))[:4]
        shifted = [torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view(t.shape).copy_(t) for t in four]
        out = torch.zeros(rows * cols + 1, dtype=dtype, device=four[0].device)[1:].view(rows, cols)
        engine.gptq_dequant(*shifted, dtype, out=out)
        assert torch.equal(raw(out), raw(engine.gptq_dequant(*four, dtype)))


def check_rounds(engine, device="cpu"):
    """the same bytes at forced round counts: 1, 2 and 3 tiles per work-group (the dequantiser's LDS sets alternate)"""
    x = weights((136, 17 * 32), 32, seed=12, device=device)
    want = check(engine, x, 32, "rounds 0")
    for c in (1, 2, 3):
        engine.ctx.debug_option("stream_chunks", c)
        try:
            got = check(engine, x, 32, f"rounds {c}", out_dtypes=(torch.bfloat16,))
            assert engine.ctx.debug_query("stream_chunks_applied") == 2     # gptq_quant, gptq_dequant
        finally:
            engine.ctx.debug_option("stream_chunks", 0)
        assert all(torch.equal(a, b) for a, b in zip(got[:4], want[:4])) and got[4] == want[4]


# ---- the corners -----------------------------------------------------------------------------------------------------
def corner_zero_group(engine, device):
    x = weights((8, 96), 32, torch.float32, seed=20, device=device)
    x[3, 32:64] = 0.0
    x[3, 40] = -0.0
    qweight, qzeros, scales, _, rep = check(engine, x, 32, "zero group")
    assert scales.view(torch.int16)[1, 3].item() == 1 and (rep.zero_groups, rep.scale_clamped) == (1, 0)    # 2^-24
    assert (qzeros[1, 0].item() >> 12) & 15 == 15 and not ((qweight[4:8, 3]) != 0).any()                      # z = 0 is stored as 15


def corner_one_sided(engine, device):
    """an all-positive group has z = 0 (stored nibble 15), an all-negative one z = 15 (stored 14)"""
    x = weights((8, 64), 32, torch.float32, seed=21, device=device).abs() + 0.25
    x[:, 32:] = -x[:, 32:]
    _, qzeros, _, _, _ = check(engine, x, 32, "one-sided")
    assert qzeros.cpu().numpy().view(np.uint32).tolist() == [[0xFFFFFFFF], [0xEEEEEEEE]]


def corner_scale_clamps(engine, device):
    """s below 2^-25 is raised to 2^-24, s above 65504 lowered to it: there the extremes clip"""
    x = torch.zeros(8, 64, device=device)
    x[:, :32] = torch.linspace(-1e-9, 2e-9, 32, device=device)
    x[:, 32:] = torch.linspace(-3e6, 3e6, 32, device=device)
    _, _, scales, _, rep = check(engine, x, 32, "clamps")
    assert scales.view(torch.int16).tolist() == [[1] * 8, [0x7BFF] * 8] and rep.scale_clamped == 16 and rep.clipped > 0


def corner_midpoints(engine, device):
    """s16 = 1 and z = 0: a quotient exactly between two codes goes to the even one"""
    x = torch.zeros(8, 32, device=device)
    x[:, :8] = torch.tensor([15.0, 0.5, 1.5, 2.5, 3.5, 13.5, 14.5, 0.0], device=device)
    qweight, _, scales, _, rep = check(engine, x, 32, "midpoints")
    assert scales[0, 0].item() == 1.0 and int(qweight.cpu().numpy().view(np.uint32)[0, 0]) == 0x0EE4220F and rep.clipped == 0


def corner_symmetric(engine, device):
    """a hand-packed symmetric checkpoint: zero words 0x77777777 read as z = 8"""
    gen = torch.Generator().manual_seed(22)
    q = torch.randint(0, 16, (16, 64), generator=gen)
    scales = (torch.rand(2, 16, generator=gen) + 0.5).to(torch.float16)
    qweight = torch.from_numpy(np.ascontiguousarray(pack8(q.numpy()).T))
    qzeros = torch.full((2, 2), 0x77777777, dtype=torch.int32)
    g_idx = torch.arange(64, dtype=torch.int32) // 32
    out = engine.gptq_dequant(qweight.to(device), qzeros.to(device), scales.to(device), g_idx.to(device), torch.float32)
    assert torch.equal(out.cpu(), (q - 8).float() * scales.float().T.repeat_interleave(32, dim=1))


def corner_errors(engine, device):
    name = "model.layers.7.mlp.up_proj.weight"
    match = r"model\.layers\.7\.mlp\.up_proj\.weight"
    for poison in (float("nan"), float("inf"), float("-inf")):
        for dtype in DTYPES:
            x = weights((72, 192), 64, dtype, seed=23, device=device)
            x[71, 191] = poison
            with pytest.raises(ValueError, match="Non-finite value in " + match):
                engine.gptq_quant(x, 64, layer_name=name)
    x = weights((72, 192), 64, seed=24, device=device)
    qweight, qzeros, scales, g_idx, _ = check(engine, x, 64, "after an error")
    for poison in (float("nan"), float("inf")):
        bad = scales.clone()
        bad[2, 71] = poison
        with pytest.raises(ValueError, match="Non-finite scale in " + match):
            engine.gptq_dequant(qweight, qzeros, bad, g_idx, layer_name=name)
    permuted = g_idx.clone()
    permuted[[5, 100]] = permuted[[100, 5]]
    for call, what in ((lambda: engine.gptq_dequant(qweight, qzeros, scales, permuted, layer_name=name), match + ".*act-order"),
                       (lambda: engine.gptq_quant(x[:12, :48].contiguous(), 32, layer_name="w12"), r"w12.*\[12, 48\]"),
                       (lambda: engine.gptq_quant(x, 48, layer_name="w"), r"group size 48 for w"),
                       (lambda: engine.gptq_dequant(qweight, qzeros[:, :8], scales, g_idx, layer_name="w"), r"qzeros of w.*\[3, 8\].*\[3, 9\] expected"),
                       (lambda: engine.gptq_dequant(qweight, qzeros, scales[:, :64], g_idx, layer_name="w"), r"scales of w.*\[3, 64\]"),
                       (lambda: engine.gptq_dequant(qweight, qzeros, scales, g_idx[:-1], layer_name="w"), r"g_idx of w.*\[191\]")):
        with pytest.raises(ValueError, match=what):
            call()


CORNERS = [corner_zero_group, corner_one_sided, corner_scale_clamps, corner_midpoints, corner_symmetric, corner_errors]


# ---- through the public interface, on the on-disk model of tests/lora_fixtures.py ------------------------------------
def check_commands_and_merge(tmp_path, engine, device):
    """a quantize-gptq output as a finetune_merge entry merges, byte for byte, like its dequantize-gptq output"""
    import asyncio
    from safetensors.torch import load_file, save_file
    from shardmerge_amd import distributed
    from shardmerge_amd.config import MergeConfig
    from shardmerge_amd.index import LocalModelIndex
    from shardmerge_amd.merge import operator_class
    from tests import harness, lora_fixtures as lf
    from tests.nv4_checks import run_cli
    lf.setup_k3(tmp_path, engine)
    storage = tmp_path / "storage"
    q4 = storage / "org/ft1-gptq"
    for args in (["quantize-gptq", "org/ft1", "--out", q4, "--group-size", "64"],
                 ["dequantize-gptq", "org/ft1-gptq", "--out", storage / "org/ft1-back", "--dtype", "bf16"],
                 ["quantize-nvfp4", "org/ft2", "--out", storage / "org/ft2-nv4"], ["quantize-fp8", "org/ft2", "--out", storage / "org/ft2-fp8"]):
        res = run_cli(args + ["--storage-dir", storage, "--device", device])
        assert res.exit_code == 0, res.output
    ft1 = lf.model_tensors(1)
    got = {}
    for f in sorted(q4.glob("*.safetensors")):
        got.update(load_file(str(f)))
    quantised = [n[:-len("weight")] for n, t in ft1.items() if t.ndim == 2 and n.endswith(".weight") and n.split(".")[-2].endswith("_proj")]
    plain = [n for n in ft1 if n[:-len("weight")] not in quantised]
    assert quantised and sorted(got) == sorted(plain + [s + k for s in quantised for k in ("qweight", "qzeros", "scales", "g_idx")])
    for stem in quantised:
        rw, rz, rs, rg = restate(ft1[stem + "weight"], 64)[:4]
        for k, ref in (("qweight", rw), ("qzeros", rz), ("scales", rs), ("g_idx", rg)):
            assert np.array_equal(got[stem + k].numpy(), ref), stem + k
    assert all(torch.equal(raw(got[n]), raw(ft1[n])) for n in plain)
    qc = json.loads((q4 / "config.json").read_text())["quantization_config"]
    assert {k: qc[k] for k in ("quant_method", "bits", "group_size", "desc_act", "sym")} == \
        {"quant_method": "gptq", "bits": 4, "group_size": 64, "desc_act": False, "sym": False}
    index = LocalModelIndex(storage_path=storage)
    for uri in ("org/ft1-gptq", "org/ft2-nv4", "org/ft2-fp8", "org/ft1"):
        asyncio.run(index.add_model(uri))
    kinds = {uri: [k for k in ("gptq", "nv4", "fp8", "mx4") if getattr(index, k)(uri) is not None] for uri in index.model_indexes}
    assert kinds == {"org/ft1-gptq": ["gptq"], "org/ft2-nv4": ["nv4"], "org/ft2-fp8": ["fp8"], "org/ft1": []}
    for options in ({"operator": "dare_linear", "density": 1.0}, {"operator": "ties", "density": 0.3, "ties_lambda": 0.7}):
        outs = []
        for entry in ("org/ft1-gptq", "org/ft1-back"):
            models = [{"model": entry, "base": "org/base", "alpha": 0.5, "is_input": True},
                      {"model": "org/ft2", "base": "org/base", "alpha": 0.4, "is_output": True}]
            out = f"merged-{options['operator']}-{entry[-4:]}"
            res = harness.run_cli(harness.write_config(tmp_path, models, out, options, device))
            assert res.exit_code == 0, res.output
            outs.append(tmp_path / out)
        lf.assert_same_outputs(outs[0], outs[1])
        assert not all(torch.equal(raw(a), raw(b)) for a, b in
                       zip(lf.read_outputs(outs[0]).values(), lf.read_outputs(storage / "org/base").values()))
    # a GPTQ checkpoint as base or output_base_model: rejected in initialize(), nothing written
    for models, obm in (([{"model": "org/ft2", "base": "org/ft1-gptq", "alpha": 0.5, "is_input": True, "is_output": True}], "org/base"),
                        ([{"model": "org/ft2", "base": "org/base", "alpha": 0.5, "is_input": True, "is_output": True}], "org/ft1-gptq")):
        p = harness.write_config(tmp_path, models, "never", {"operator": "ties", "density": 0.3}, device)
        p.write_text(p.read_text().replace("output_base_model: org/base", f"output_base_model: {obm}"))
        cfg = MergeConfig.from_yaml(p)
        with pytest.raises(ValueError, match=r"org/ft1-gptq.*dequantize-gptq"):
            asyncio.run(operator_class(cfg.operator)(config=cfg, index_manager=LocalModelIndex(storage_path=storage)).initialize())
        assert harness.run_cli(p).exit_code != 0 and not (tmp_path / "never").exists()
    models = [{"model": "org/ft1-gptq", "base": "org/base", "alpha": 0.5, "is_input": True, "is_output": True}]
    cfg = MergeConfig.from_yaml(harness.write_config(tmp_path, models, "stamp", {"operator": "ties", "density": 0.3}, device))
    s0 = distributed.config_stamp(cfg)
    shard = sorted(q4.glob("*.safetensors"))[0]
    save_file(load_file(str(shard)), str(shard), metadata={"format": "pt", "note": "rewritten"})
    assert s0 != distributed.config_stamp(cfg)
    # what the detector rejects, naming the model and the tensor or field
    tensors = load_file(str(shard))
    name = next(n for n in tensors if n.endswith(".qzeros"))
    for doc, what in (({**tensors, name: tensors[name][:, :1].contiguous()}, name), ({k: v for k, v in tensors.items() if k != name}, f"no {name}"),
                      ({**tensors, name: tensors[name].to(torch.int64)}, f"{name} is I64")):
        save_file(doc, str(shard), metadata={"format": "pt"})
        with pytest.raises(ValueError, match=rf"org/ft1-gptq.*{what}"):
            asyncio.run(LocalModelIndex(storage_path=storage).add_model("org/ft1-gptq"))
    save_file(tensors, str(shard), metadata={"format": "pt"})
    config = json.loads((q4 / "config.json").read_text())
    for field, value in (("bits", 8), ("desc_act", True), ("checkpoint_format", "gptq_v2"), ("group_size", 16)):
        doc = json.loads(json.dumps(config))
        doc["quantization_config"][field] = value
        (q4 / "config.json").write_text(json.dumps(doc))
        with pytest.raises(ValueError, match=rf"org/ft1-gptq.*{field}"):
            asyncio.run(LocalModelIndex(storage_path=storage).add_model("org/ft1-gptq"))
