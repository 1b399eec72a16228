"""Checks of the delta pack shared by the emulator tier (tests/test_dpack_host.py) and the GPU tier
(tests/test_dpack_gpu.py): Engine.delta_pack and Engine.delta_apply against tests/dpack_oracle.py, BIT FOR BIT - the
planes, the scales, every report field and the rebuilt tensor.  The tolerance is zero and it is derived, not measured:
every step of the function is an exact order statistic, an integer function or one correctly rounded operation in a
stated order (include/shardmerge_hip.h, smhip_dpack_pack).  Then, independently of that oracle, in torch fp64: the
residual recomputed from the unpacked planes, the optimality of the scale, and the 1-bit residual of a Gaussian."""
import math

import pytest
import torch

from tests import dpack_oracle as po
from tests.harness import DTYPES, f32_bits, f64_bits, make_inputs, raw

COLS = (1, 7, 8, 9, 2047, 2048, 2056, 4104)      # a row's lanes wrap at 2048 elements
ROWS = (1, 2, 3, 257)
# (bits, density): the last one asks for k_keep == 0 at every shape of these tests
FORMS = ((1, 1.0), (2, 1.0), (2, 0.5), (2, 0.2), (2, 1e-9))
SCALES = ("row", "tensor")


def pair(shape, dtype=torch.bfloat16, seed=0, sigma=3e-3, device="cpu"):
    fts, bases, _ = make_inputs(shape, 1, dtype, seed=seed, sigma=sigma, device=device)
    return fts[0], bases[0]


def check(engine, ft, base, bits=1, density=1.0, scale="row", label=""):
    """pack and apply against the oracle, bit for bit; returns (sign, mask, scale, report, rebuilt)"""
    sign, mask, sc, rep = engine.delta_pack(ft, base, bits=bits, density=density, scale=scale, name=label)
    ref = po.pack(ft.cpu(), base.cpu(), bits, density, scale)
    assert sign.dtype == torch.uint8 and tuple(sign.shape) == tuple(ref.sign.shape), label
    assert torch.equal(sign.cpu(), ref.sign), f"{label}: sign plane differs"
    assert (mask is None) == (bits == 1), label
    if mask is not None:
        assert torch.equal(mask.cpu(), ref.mask), f"{label}: mask plane differs"
    assert sc.dtype == torch.float32 and tuple(sc.shape) == tuple(ref.scale.shape), label
    assert torch.equal(raw(sc), raw(ref.scale)), f"{label}: scales differ in their bits"
    got = (rep.rows, rep.cols, rep.bits, rep.k_keep, f32_bits(rep.threshold), rep.kept, rep.nonzero,
           f64_bits(rep.delta_sq), f64_bits(rep.resid_sq))
    want = (ref.rows, ref.cols, ref.bits, ref.k_keep, f32_bits(ref.threshold), ref.kept, ref.nonzero,
            f64_bits(ref.delta_sq), f64_bits(ref.resid_sq))
    assert got == want, (label, rep, ref)
    out = engine.delta_apply(base, sign, mask, sc)
    exp = po.apply(base.cpu(), ref.sign, ref.mask, ref.scale)
    assert out.dtype == base.dtype and out.shape == base.shape, label
    bad = int((raw(out) != raw(exp)).sum())
    assert bad == 0, f"{label}: {bad} of {exp.numel()} rebuilt values differ in their bits"
    return sign, mask, sc, rep, out


# ---- the grid ------------------------------------------------------------------------------------------------
def check_cols(engine, cols, device="cpu"):
    """every column count at three rows, every form, both scales"""
    for j, (bits, density) in enumerate(FORMS):
        for scale in SCALES:
            ft, base = pair((3, cols), seed=100 + j, device=device)
            rep = check(engine, ft, base, bits, density, scale, f"3x{cols} bits={bits} density={density} {scale}")[3]
            if density == 1e-9:
                assert rep.k_keep == 0 and rep.kept == 0 and rep.threshold == float("inf")


def check_rows(engine, rows, device="cpu"):
    for cols in (9, 2056):
        for bits, density in ((1, 1.0), (2, 0.2)):
            for scale in SCALES:
                ft, base = pair((rows, cols), seed=110 + rows % 7, device=device)
                check(engine, ft, base, bits, density, scale, f"{rows}x{cols} bits={bits} {scale}")


def check_dtypes(engine, dtype, device="cpu"):
    for bits, density in ((1, 1.0), (2, 0.5)):
        ft, base = pair((5, 2047), dtype, seed=120, device=device)
        check(engine, ft, base, bits, density, "row", f"{dtype} bits={bits}")
        ft, base = pair((4, 2048), dtype, seed=121, device=device)
        check(engine, ft, base, bits, density, "tensor", f"{dtype} bits={bits} aligned")
    # a finetune and a base of two dtypes: both promoted to fp32, the planes still fit the shape
    ft, base = pair((3, 100), dtype, seed=122, device=device)
    sign, mask, sc, rep = engine.delta_pack(ft, base.float(), bits=2, density=0.5)
    ref = po.pack(ft.cpu(), base.cpu().float(), 2, 0.5, "row")
    assert torch.equal(sign.cpu(), ref.sign) and torch.equal(mask.cpu(), ref.mask) and torch.equal(raw(sc), raw(ref.scale))


def check_rank3_and_1d(engine, device="cpu"):
    ft, base = pair((4, 33, 65), seed=130, device=device)
    for bits, density in ((1, 1.0), (2, 0.2)):
        rep = check(engine, ft, base, bits, density, "row", f"rank 3 bits={bits}")[3]
        assert (rep.rows, rep.cols) == (4, 33 * 65)
    for n in (1, 9, 5000):
        ft, base = pair((n,), seed=131, device=device)
        for scale in SCALES:
            rep = check(engine, ft, base, 2, 0.5, scale, f"1-D n={n} {scale}")[3]
            assert (rep.rows, rep.cols) == (1, n)
    ft, base = pair((), seed=132, device=device)
    assert check(engine, ft, base, 1, 1.0, "row", "0-D")[3].cols == 1


def check_offset_views(engine, device="cpu"):
    """views that start one element into their storage: no pointer is 16-byte aligned"""
    for dtype in DTYPES:
        for rows, cols in ((3, 2048), (2, 2047)):
            n = rows * cols
            ft, base = pair((n + 8,), dtype, seed=140, device=device)
            cut = lambda t, o: t[o:o + n].view(rows, cols)
            for fo, bo in ((1, 1), (1, 0), (0, 1)):
                check(engine, cut(ft, fo), cut(base, bo), 2, 0.5, "row", f"offset views {dtype} {rows}x{cols} {fo}/{bo}")
                check(engine, cut(ft, fo), cut(base, bo), 1, 1.0, "tensor", f"offset views {dtype} {rows}x{cols} {fo}/{bo} 1-bit")


def check_heavy_ties(engine, device="cpu"):
    """differences of bf16 weights collide: far more than k_keep elements reach the threshold, all of them are kept"""
    ft, base = pair((64, 2056), seed=150, sigma=3e-4, device=device)
    for scale in SCALES:
        rep = check(engine, ft, base, 2, 0.2, scale, f"ties {scale}")[3]
        assert rep.kept > rep.k_keep > 0


def check_equal_to_base(engine, device="cpu"):
    """a finetune equal to its base: the scales are +0; under 2 bits nothing is kept and apply returns the base bit for
    bit, a -0 included"""
    for dtype in DTYPES:
        _, base = pair((5, 2049), dtype, seed=160, device=device)
        base = base.clone()
        base.view(-1)[::7] = -0.0
        for bits, density in ((2, 1.0), (2, 0.5), (1, 1.0)):
            for scale in SCALES:
                sign, mask, sc, rep, out = check(engine, base.clone(), base, bits, density, scale, f"zero delta {dtype} bits={bits}")
                assert rep.nonzero == 0 and rep.delta_sq == 0.0 and rep.resid_sq == 0.0
                assert all(f32_bits(float(v)) == f32_bits(0.0) for v in sc.cpu())
                assert int(sign.cpu().sum()) == 0
                if bits == 2:
                    assert rep.kept == 0 and rep.threshold == 0.0 and int(mask.cpu().sum()) == 0
                    assert torch.equal(raw(out), raw(base)), "apply moved an element of a zero-delta pack"
                else:                                    # every element is kept: base + 0, which IEEE makes +0 of a -0
                    assert rep.kept == base.numel() and torch.equal(out.cpu(), base.cpu())


def check_empty_row(engine, device="cpu"):
    """rows without a kept entry beside rows with some: their scale is +0 and they come back as the base"""
    ft, base = pair((6, 2056), seed=170, device=device)
    ft = ft.clone()
    ft[1], ft[4] = base[1], base[4]
    ft[2] = (base[2].view(torch.int16) + 1).view(base.dtype)        # one ulp away from zero: non-zero deltas under the threshold
    sign, mask, sc, rep, out = check(engine, ft, base, 2, 0.3, "row", "empty rows")
    assert float(sc[1]) == 0.0 and float(sc[4]) == 0.0
    assert torch.equal(raw(out[1]), raw(base[1])) and torch.equal(raw(out[4]), raw(base[4]))
    check(engine, ft, base, 2, 0.3, "tensor", "empty rows, tensor scale")


def check_nonfinite(engine, device="cpu"):
    """a NaN / an Inf in the finetune or in the base: ValueError naming the tensor; the context stays usable"""
    for bits, density in ((1, 1.0), (2, 0.5)):
        for poison in (float("nan"), float("inf"), float("-inf")):
            for in_base in (False, True):
                ft, base = pair((7, 1000), seed=180, device=device)
                ft, base = ft.clone(), base.clone()
                (base if in_base else ft).view(-1)[4321] = poison
                with pytest.raises(ValueError, match=r"model\.layers\.7\.mlp\.up_proj\.weight"):
                    engine.delta_pack(ft, base, bits=bits, density=density, name="model.layers.7.mlp.up_proj.weight")
        ft, base = pair((7, 1000), seed=181, device=device)
        check(engine, ft, base, bits, density, "row", "after an error")
    ft, base = pair((7, 1000), torch.float32, seed=182, device=device)          # Inf - Inf
    ft.view(-1)[5] = float("inf")
    base.view(-1)[5] = float("inf")
    with pytest.raises(ValueError, match="Non-finite delta in w"):
        engine.delta_pack(ft, base, name="w")


def check_empty(engine, device="cpu"):
    for shape in ((0,), (3, 0), (0, 5)):
        ft, base = pair(shape, seed=190, device=device)
        for bits, density in ((1, 1.0), (2, 0.5)):
            for scale in SCALES:
                sign, mask, sc, rep, out = check(engine, ft, base, bits, density, scale, f"n = 0 {shape} bits={bits} {scale}")
                assert rep.kept == 0 and rep.k_keep == 0 and out.numel() == 0
                assert rep.threshold == (float("inf") if bits == 2 else 0.0)


def check_determinism(engine, device="cpu"):
    ft, base = pair((300, 520), seed=200, device=device)
    a = engine.delta_pack(ft, base, bits=2, density=0.3)
    b = engine.delta_pack(ft, base, bits=2, density=0.3)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def check_arguments(engine, device="cpu"):
    """every argument error is a ValueError before any launch"""
    from tests.harness import profile_of
    ft, base = pair((8, 16), seed=210, device=device)
    sign, mask, sc, _ = engine.delta_pack(ft, base, bits=2, density=0.5)

    def bad_calls():
        for bits in (0, 3, True, 1.0, "1"):
            with pytest.raises(ValueError, match="bits"):
                engine.delta_pack(ft, base, bits=bits)
        for density in (0.0, -0.1, 1.5, float("nan"), None):
            with pytest.raises(ValueError, match="density"):
                engine.delta_pack(ft, base, bits=2, density=density)
        with pytest.raises(ValueError, match="bits = 1.*density"):
            engine.delta_pack(ft, base, bits=1, density=0.5)
        with pytest.raises(ValueError, match="scale"):
            engine.delta_pack(ft, base, scale="column")
        with pytest.raises(ValueError, match="shape mismatch in w"):
            engine.delta_pack(ft, base[:4], name="w")
        with pytest.raises(ValueError, match="sign"):
            engine.delta_apply(base, sign[:, :1], mask, sc)
        with pytest.raises(ValueError, match="mask"):
            engine.delta_apply(base, sign, mask.to(torch.int32), sc)
        with pytest.raises(ValueError, match="scale"):
            engine.delta_apply(base, sign, mask, sc[:3])
        with pytest.raises(ValueError, match="scale"):
            engine.delta_apply(base, sign, mask, sc.double())
        with pytest.raises(ValueError, match="base"):
            engine.delta_apply(base.double(), sign, mask, sc)

    assert profile_of(engine, bad_calls) == {}


def check_launches(engine, device="cpu"):
    """the selection is TIES's kernels, the folds are geo_gram_fold; a 1-bit pack selects nothing"""
    from tests.harness import profile_of
    ft, base = pair((64, 520), seed=220, device=device)
    assert profile_of(engine, lambda: engine.delta_pack(ft, base, bits=2, density=0.5)) == \
        {"ties_hist": 3, "ties_select": 3, "dpack_pack": 1, "geo_gram_fold": 2, "dpack_scale": 1}
    assert profile_of(engine, lambda: engine.delta_pack(ft, base, bits=2, density=1e-9)) == \
        {"ties_hist": 1, "ties_select": 3, "dpack_pack": 1, "geo_gram_fold": 2, "dpack_scale": 1}
    assert profile_of(engine, lambda: engine.delta_pack(ft, base, bits=1)) == {"dpack_pack": 1, "geo_gram_fold": 2, "dpack_scale": 1}
    sign, mask, sc, _ = engine.delta_pack(ft, base, bits=1)
    assert profile_of(engine, lambda: engine.delta_apply(base, sign, mask, sc)) == {"dpack_apply": 1}


# ---- independently of the oracle, in torch fp64 -----------------------------------------------------------------
def unpacked(ft, base, sign, mask, sc):
    """(d, q, kept) in fp64 from the planes: q = +-s where kept, 0 elsewhere"""
    R, C = po.view_rows(ft.shape)
    d = (ft.cpu().float() - base.cpu().float()).double().reshape(R, C)
    bits = lambda p: ((p.cpu().to(torch.int32).unsqueeze(-1) >> torch.arange(8)) & 1).reshape(R, -1)[:, :C].bool()
    kept = bits(mask) if mask is not None else torch.ones(R, C, dtype=torch.bool)
    s = sc.cpu().double().reshape(-1, 1).expand(R, 1) if sc.numel() == 1 else sc.cpu().double().reshape(R, 1)
    q = torch.where(kept, torch.where(bits(sign), -s, s), torch.zeros((), dtype=torch.float64))
    return d, q, kept, s


def check_residual(engine, device="cpu"):
    """||d - q||^2 recomputed from the planes equals resid_sq within the a-priori bound of the ordered sums and the
    formula: (n + 8) 2^-53 (Z + Q + 2 s A + c s^2)"""
    for shape, dtype in (((37, 2056), torch.bfloat16), ((64, 1000), torch.float32)):
        for bits, density in ((1, 1.0), (2, 0.5), (2, 0.2)):
            for scale in SCALES:
                ft, base = pair(shape, dtype, seed=230, device=device)
                sign, mask, sc, rep = engine.delta_pack(ft, base, bits=bits, density=density, scale=scale)
                d, q, kept, s = unpacked(ft, base, sign, mask, sc)
                direct = float(((d - q) ** 2).sum())
                n = d.numel()
                Z, Q = float((d[~kept] ** 2).sum()), float((d[kept] ** 2).sum())
                sA = float((s.expand_as(d)[kept] * d[kept].abs()).sum())
                cs2 = float((s.expand_as(d)[kept] ** 2).sum())
                bound = (n + 8) * 2.0 ** -53 * (Z + Q + 2 * sA + cs2)
                print(f"residual {shape} {dtype} bits={bits} density={density} {scale}: |{direct} - {rep.resid_sq}| = "
                      f"{abs(direct - rep.resid_sq):.3e}, bound {bound:.3e}")
                assert abs(direct - rep.resid_sq) <= bound
                # (two sums of n non-negative terms, each within (n - 1) 2^-53 of the exact one)
                assert abs(float((d ** 2).sum()) - rep.delta_sq) <= 2 * (n + 8) * 2.0 ** -53 * (Z + Q)
                assert rep.kept == int(kept.sum()) and rep.nonzero == int((d != 0).sum())


def check_scale_optimal(engine, device="cpu"):
    """s (1 +- 2^-10) gives a strictly larger residual over the kept entries: the gap is c s^2 2^-20, the rounding of
    s to fp32 and of the fp64 sums at most c s^2 2^-33"""
    ft, base = pair((16, 2056), torch.float32, seed=240, device=device)
    for bits, density in ((1, 1.0), (2, 0.3)):
        for scale in SCALES:
            sign, mask, sc, rep = engine.delta_pack(ft, base, bits=bits, density=density, scale=scale)
            d, q, kept, s = unpacked(ft, base, sign, mask, sc)
            best = float(((d - q) ** 2).sum())
            for f in (1 + 2.0 ** -10, 1 - 2.0 ** -10):
                assert float(((d - q * f) ** 2).sum()) > best, (bits, scale, f)


def check_gaussian_one_bit(engine, device="cpu"):
    """fp32 Gaussian deltas, sigma 3e-3 on a base of sigma 0.02, n = 2^18: the 1-bit relative residual is within 1 % of
    sqrt(1 - 2 / pi)"""
    ft, base = pair((1 << 18,), torch.float32, seed=250, device=device)
    for scale in SCALES:
        rep = engine.delta_pack(ft, base, bits=1, scale=scale)[3]
        print(f"1-bit Gaussian {scale}: {rep.rel_residual} vs {math.sqrt(1 - 2 / math.pi)}")
        assert abs(rep.rel_residual / math.sqrt(1 - 2 / math.pi) - 1) < 0.01


# ---- identities through the engine, bit for bit --------------------------------------------------------------------
def check_reconstruction(engine, device="cpu"):
    """an fp32 base of multiples of 2^-10 with deltas in {-2^-7, 0, +2^-7}: 2 bits at density 1, then apply, give the
    finetune back; packing the result again gives the same planes and scale"""
    g = torch.Generator().manual_seed(260)
    base = (torch.randint(-2048, 2048, (9, 1003), generator=g).float() * 2.0 ** -10).to(device)
    ft = base + (torch.randint(-1, 2, (9, 1003), generator=g).float() * 2.0 ** -7).to(device)
    for scale in SCALES:
        sign, mask, sc, rep = engine.delta_pack(ft, base, bits=2, density=1.0, scale=scale)
        assert rep.resid_sq == 0.0 and all(float(v) == 2.0 ** -7 for v in sc.cpu())
        out = engine.delta_apply(base, sign, mask, sc)
        assert torch.equal(raw(out), raw(ft))
        again = engine.delta_pack(out, base, bits=2, density=1.0, scale=scale)
        assert torch.equal(again[0], sign) and torch.equal(again[1], mask) and torch.equal(raw(again[2]), raw(sc))


def check_against_stats_and_ties(engine, device="cpu"):
    """2 bits: the kept count and the threshold are delta_stats's and ties_merge's at the same density, and the kept set
    is where a ties merge of this one finetune moves the base"""
    ft, base = pair((33, 1000), seed=270, device=device)
    for density in (1.0, 0.5, 0.2, 0.01):
        sign, mask, sc, rep = engine.delta_pack(ft, base, bits=2, density=density)
        st = engine.delta_stats([ft], [base], [1.0], [density])
        assert (rep.k_keep, rep.kept, rep.nonzero) == (st.k_keep[0], st.kept[0][0], st.nonzero[0])
        assert f32_bits(rep.threshold) == f32_bits(st.thresholds[0][0])
        _, trep, delta = engine.ties_merge([ft], [base], [1.0], base, density=density, normalize=False, want_delta=True)
        assert (trep.k_keep, trep.kept[0]) == (rep.k_keep, rep.kept) and f32_bits(trep.thresholds[0]) == f32_bits(rep.threshold)
        kept = torch.from_numpy(po.unpack_bits(mask.cpu().numpy(), 1000))
        assert torch.equal(kept, delta.cpu() != 0)


def check_nested(engine, device="cpu"):
    """the kept sets are nested in the density, and the signs agree where both keep"""
    ft, base = pair((17, 2056), seed=280, device=device)
    prev = None
    for density in (0.05, 0.2, 0.5, 1.0):
        sign, mask, _, _ = engine.delta_pack(ft, base, bits=2, density=density)
        m, s = mask.cpu().to(torch.int32), sign.cpu().to(torch.int32)
        if prev is not None:
            assert int((prev[0] & ~m).sum()) == 0 and torch.equal(prev[1], s & prev[0])
        prev = (m, s)
    one = engine.delta_pack(ft, base, bits=1)[0].cpu().to(torch.int32)
    assert torch.equal(prev[1], one)                 # density 1 keeps every non-zero delta: its signs are the 1-bit plane's


CORNERS = [check_rank3_and_1d, check_offset_views, check_heavy_ties, check_equal_to_base, check_empty_row, check_nonfinite,
           check_empty, check_determinism, check_arguments, check_launches, check_residual, check_scale_optimal,
           check_gaussian_one_bit, check_reconstruction, check_against_stats_and_ties, check_nested]


# ---- end to end on the on-disk model of tests/lora_fixtures.py ---------------------------------------------------------
OPTIONS = {"operator": "ties", "density": 0.3, "ties_lambda": 0.7}
PACK_FILES = ["compression.json", "delta_config.json", "delta_model.safetensors"]


def run_cli(args):
    from click.testing import CliRunner
    from shardmerge_amd.__main__ import cli
    return CliRunner().invoke(cli, [str(a) for a in args])


def compress_args(root, model, out, device, more=("--bits", 2, "--density", 0.5), base="org/base"):
    return ["compress-delta", model, "--base", base, "--out", root / "storage" / out, "--storage-dir", root / "storage",
            "--device", device, *more]


def oracle_finetune(base, ft, bits, density, scale, packed=lambda name, t: t.ndim >= 2):
    """the tensors a pack of `ft` on `base` stands for, by the oracle: apply(pack) where packed, ft's own tensor where
    stored whole, the base's where nothing differs"""
    out = {}
    for name, t in ft.items():
        if torch.equal(raw(t), raw(base[name])):
            out[name] = base[name]
        elif packed(name, t):
            ref = po.pack(t, base[name], bits, density, scale)
            out[name] = po.apply(base[name], ref.sign, ref.mask, ref.scale)
        else:
            out[name] = t
    return out


def pack_models(pack):
    from tests.harness import ties_models
    return ties_models(pack)


def expected_outputs(base, pack_full):
    from tests import ties_oracle
    from tests.harness import expected_by_tensor

    def merge(fts, bases, alphas, base_out, name):
        return ties_oracle.ties_merge(fts, bases, alphas, base_out, OPTIONS["density"], OPTIONS["ties_lambda"], True)[0]

    return expected_by_tensor(base, pack_full, pack_models("org/pack"), merge)


def setup_pack(tmp_path, engine, device, more=("--bits", 2, "--density", 0.5), out="org/pack"):
    """the k3 storage and org/pack = compress-delta of a third full finetune; returns (base, that finetune, the CLI result)"""
    from tests import lora_fixtures as lf
    base, _, _ = lf.setup_k3(tmp_path, engine)
    ft3 = dict(lf.model_tensors(2))
    for ti, (name, shape) in enumerate(lf.TENSORS):            # a finetune of its own; lm_head and layer 1's norm stay the base's
        ft3[name] = (base[name].float() + lf.randn(shape, 900 + ti, 0.003)).to(torch.bfloat16)
    ft3["lm_head.weight"] = base["lm_head.weight"]
    ft3["model.layers.1.input_layernorm.weight"] = base["model.layers.1.input_layernorm.weight"]
    lf.write_model(tmp_path / "storage", "org/ft3", ft3)
    res = run_cli(compress_args(tmp_path, "org/ft3", out, device, more))
    assert res.exit_code == 0, res.output
    return base, ft3, res


def check_command(tmp_path, engine, device):
    """compress-delta runs, the reader accepts DIR, compression.json agrees with the engine's reports, a ties merge with
    the pack as an entry equals the merge of the oracle's delta_apply tensors, twice with the same bytes"""
    import asyncio
    import json
    from safetensors.torch import load_file
    from shardmerge_amd.adapter import base_tensor_meta
    from shardmerge_amd.deltapack import DeltaPack, is_pack_dir
    from shardmerge_amd.index import LocalModelIndex
    from tests import harness
    from tests import lora_fixtures as lf
    base, ft3, res = setup_pack(tmp_path, engine, device)
    storage = tmp_path / "storage"
    out = storage / "org/pack"
    assert sorted(p.name for p in out.iterdir()) == PACK_FILES and is_pack_dir(out)
    assert "residual" in res.output and "q_proj" in res.output
    pack = DeltaPack("org/pack", out)
    index = LocalModelIndex(storage_path=storage)
    asyncio.run(index.add_model("org/base"))
    asyncio.run(index.add_model("org/pack"))
    pack.check_against("org/base", base_tensor_meta(index, "org/base"))
    assert index.pack("org/pack") is not None and index.adapter("org/pack") is None
    changed = [n for n, _ in lf.TENSORS if not torch.equal(raw(ft3[n]), raw(base[n]))]
    assert sorted(pack.tensors) == sorted(changed)
    assert {n: t.kind for n, t in pack.tensors.items()} == {n: "packed" if ft3[n].ndim >= 2 else "full" for n in changed}
    cfg = json.loads((out / "delta_config.json").read_text())
    assert (cfg["format"], cfg["version"], cfg["base_model_name_or_path"], cfg["bits"], cfg["density"], cfg["scale"]) == \
        ("shardmerge-delta", 1, "org/base", 2, 0.5, "row")
    got = load_file(str(out / "delta_model.safetensors"))
    rep = json.loads((out / "compression.json").read_text())
    assert [t["name"] for t in rep["tensors"]] == [n for n in index.get_layer_order("org/base") if n in changed]
    assert sorted(rep["unchanged"]) == sorted(n for n, _ in lf.TENSORS if n not in changed)
    for t in rep["tensors"]:
        name = t["name"]
        if ft3[name].ndim < 2:
            assert t["stored"] == "full" and torch.equal(raw(got[f"{name}.full"]), raw(ft3[name]))
            continue
        dev = lambda x: x.to(engine.device)
        sign, mask, sc, r = engine.delta_pack(dev(ft3[name]), dev(base[name]), bits=2, density=0.5)
        assert torch.equal(got[f"{name}.sign"], sign.cpu()) and torch.equal(got[f"{name}.mask"], mask.cpu())
        assert torch.equal(raw(got[f"{name}.scale"]), raw(sc))
        assert (t["kept"], t["k_keep"], t["nonzero"], t["threshold"], t["delta_sq"], t["resid_sq"]) == \
            (r.kept, r.k_keep, r.nonzero, r.threshold, r.delta_sq, r.resid_sq)
        assert t["relative_residual"] == math.sqrt(r.resid_sq / r.delta_sq)
        assert t["bytes"] == 2 * sign.numel() + 4 * sc.numel() and t["shape"] == list(ft3[name].shape)
    assert rep["totals"]["bytes"] == sum(t["bytes"] for t in rep["tensors"]) == sum(v.numel() * v.element_size() for v in got.values())
    # the pack as a finetune_merge entry
    expected = expected_outputs(base, oracle_finetune(base, ft3, 2, 0.5, "row"))
    cfgp = harness.write_config(tmp_path, pack_models("org/pack"), "merged", OPTIONS, device)
    res = harness.run_cli(cfgp)
    assert res.exit_code == 0, res.output
    harness.assert_outputs(tmp_path / "merged", expected)
    res = harness.run_cli(harness.write_config(tmp_path, pack_models("org/pack"), "merged2", OPTIONS, device))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged2", tmp_path / "merged")
    # analyze accepts the config
    res = harness.run_cli(cfgp, "analyze")
    assert res.exit_code == 0, res.output
    # the same pack twice; an existing pack is not overwritten
    res = run_cli(compress_args(tmp_path, "org/ft3", "org/pack_again", device))
    assert res.exit_code == 0, res.output
    for f in PACK_FILES:
        assert (out / f).read_bytes() == (storage / "org/pack_again" / f).read_bytes(), f
    before = (out / "delta_model.safetensors").read_bytes()
    res = run_cli(compress_args(tmp_path, "org/ft3", "org/pack", device))
    assert res.exit_code != 0 and (out / "delta_model.safetensors").read_bytes() == before
    return base, ft3, expected


def check_command_forms(tmp_path, engine, device):
    """a 1-bit pack with a scale per tensor and --modules: the other changed tensors are stored whole; flagged is_input
    the pack provides the embedding"""
    import json
    from tests import harness
    from tests import lora_fixtures as lf
    base, ft3, _ = setup_pack(tmp_path, engine, device, more=("--bits", 1, "--scale", "tensor", "--modules", "q_proj,embed_tokens"))
    rep = json.loads((tmp_path / "storage" / "org/pack" / "compression.json").read_text())
    packed = lambda name, t: t.ndim >= 2 and ("q_proj" in name or "embed_tokens" in name)
    assert {t["name"]: t["stored"] for t in rep["tensors"]} == \
        {n: "packed" if packed(n, ft3[n]) else "full" for n, _ in lf.TENSORS if not torch.equal(raw(ft3[n]), raw(base[n]))}
    full = oracle_finetune(base, ft3, 1, 1.0, "tensor", packed)
    models = [{"model": "org/pack", "base": "org/base", "alpha": 0.5, "is_input": True},
              {"model": "org/ft1", "base": "org/base", "alpha": 0.4, "is_output": True}]
    res = harness.run_cli(harness.write_config(tmp_path, models, "merged", OPTIONS, device))
    assert res.exit_code == 0, res.output
    got = lf.read_outputs(tmp_path / "merged")
    emb = "model.embed_tokens.weight"
    assert torch.equal(raw(got[emb]), raw(full[emb])) and not torch.equal(raw(got[emb]), raw(base[emb]))
    assert torch.equal(raw(got["lm_head.weight"]), raw(lf.model_tensors(1)["lm_head.weight"]))
    from tests import ties_oracle
    name = "model.layers.1.self_attn.k_proj.weight"             # stored whole: the finetune's own tensor enters the merge
    want = ties_oracle.ties_merge([ft3[name], lf.model_tensors(1)[name]], [base[name]] * 2, [0.5, 0.4], base[name], 0.3, 0.7, True)[0]
    assert torch.equal(raw(got[name]), raw(want))


def check_stamp(tmp_path, engine, device):
    """a resume after the pack has changed must not reuse old shards: the stamp hashes its config bytes and its header"""
    from safetensors.torch import load_file, save_file
    from shardmerge_amd import distributed
    from shardmerge_amd.config import MergeConfig
    from tests import harness
    setup_pack(tmp_path, engine, device)
    pack = tmp_path / "storage" / "org/pack"
    cfg = MergeConfig.from_yaml(harness.write_config(tmp_path, pack_models("org/pack"), "merged", OPTIONS, device))
    s0 = distributed.config_stamp(cfg)
    assert s0 == distributed.config_stamp(cfg)
    assert s0 != distributed.config_stamp(MergeConfig.from_yaml(harness.write_config(tmp_path, pack_models("org/ft3"), "merged", OPTIONS, device)))
    text = (pack / "delta_config.json").read_text()
    (pack / "delta_config.json").write_text(text + "\n")
    s1 = distributed.config_stamp(cfg)
    (pack / "delta_config.json").write_text(text)
    tensors = load_file(str(pack / "delta_model.safetensors"))
    save_file(tensors, str(pack / "delta_model.safetensors"), metadata={"format": "pt", "note": "rewritten"})
    s2 = distributed.config_stamp(cfg)
    assert len({s0, s1, s2}) == 3


def write_pack(storage, uri, tensors, tensor_meta, **config):
    import json
    from safetensors.torch import save_file
    d = storage / uri
    d.mkdir(parents=True, exist_ok=True)
    save_file({k: v.contiguous() for k, v in tensors.items()}, str(d / "delta_model.safetensors"), metadata={"format": "pt"})
    cfg = {"format": "shardmerge-delta", "version": 1, "base_model_name_or_path": "org/base", "bits": 2, "density": 0.5,
           "scale": "row", "tensors": tensor_meta}
    cfg.update(config)
    (d / "delta_config.json").write_text(json.dumps(cfg))


def check_reader_rejections(tmp_path, engine, device):
    """every pack the reader rejects: DeltaPackError naming the pack and the key or field, and `merge` ends before an
    output exists"""
    from shardmerge_amd.deltapack import DeltaPack, DeltaPackError
    from tests import harness
    from tests import lora_fixtures as lf
    base, _, _ = lf.setup_k3(tmp_path, engine)
    storage = tmp_path / "storage"
    q, n1 = "model.layers.0.self_attn.q_proj.weight", "model.norm.weight"
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    good = {f"{q}.sign": u8(128, 16), f"{q}.mask": u8(128, 16), f"{q}.scale": torch.zeros(128), f"{n1}.full": base[n1]}
    meta = {q: {"shape": [128, 128], "dtype": "BF16"}, n1: {"shape": [128], "dtype": "BF16"}}
    write_pack(storage, "org/good", good, meta)
    DeltaPack("org/good", storage / "org/good")

    def refused(uri, tensors, match, meta=meta, direct=True, **config):
        write_pack(storage, uri, tensors, meta, **config)
        if direct:
            with pytest.raises(DeltaPackError, match=match):
                DeltaPack(uri, storage / uri)
        res = harness.run_cli(harness.write_config(tmp_path, pack_models(uri), "never", OPTIONS, device))
        assert res.exit_code != 0 and not (tmp_path / "never").exists(), uri
        return res

    drop = lambda *keys: {k: v for k, v in good.items() if k not in keys}
    refused("org/bad_version", good, r"org/bad_version.*version 2", version=2)
    refused("org/bad_format", good, r"org/bad_format.*format", format="other")
    refused("org/bad_suffix", {**good, f"{q}.bias": torch.zeros(3)}, rf"org/bad_suffix.*{q}\.bias.*suffix")
    refused("org/no_scale", drop(f"{q}.scale"), rf"org/no_scale.*{q}\.sign.*scale")
    refused("org/no_mask", drop(f"{q}.mask"), rf"org/no_mask.*{q}\.sign.*mask")
    refused("org/no_sign", drop(f"{q}.sign"), rf"org/no_sign.*{q}\.sign")
    refused("org/mask_1bit", good, rf"org/mask_1bit.*{q}\.mask", bits=1, density=1.0)
    refused("org/bad_plane", {**good, f"{q}.sign": u8(128, 15)}, rf"org/bad_plane.*{q}\.sign.*\[128, 16\]")
    refused("org/bad_plane_dtype", {**good, f"{q}.mask": torch.zeros(128, 16, dtype=torch.int8)}, rf"org/bad_plane_dtype.*{q}\.mask.*U8")
    refused("org/bad_scale", {**good, f"{q}.scale": torch.zeros(1)}, rf"org/bad_scale.*{q}\.scale.*\[128\]")
    refused("org/bad_scale_dtype", {**good, f"{q}.scale": torch.zeros(128, dtype=torch.float16)}, rf"org/bad_scale_dtype.*{q}\.scale.*F32")
    refused("org/both", {**good, f"{q}.full": base[q]}, rf"org/both.*{q}\.full.*{q}\.(sign|mask|scale)")
    refused("org/bad_density", good, r"org/bad_density.*density", density=0.0)
    refused("org/bad_bits", good, r"org/bad_bits.*bits", bits=3)
    refused("org/undeclared", good, rf"org/undeclared.*{n1}", meta={q: meta[q]})
    # what only the base's shard headers show (check_against, in initialize())
    res = refused("org/bad_shape", {**drop(f"{n1}.full"), f"{n1}.full": base[n1][:64]}, None, direct=False,
                  meta={q: meta[q], n1: {"shape": [64], "dtype": "BF16"}})
    assert "org/bad_shape" in str(res.exception) + res.output or res.exception is not None
    other = "model.layers.9.self_attn.q_proj.weight"
    write_pack(storage, "org/unknown", {f"{other}.full": base[q]}, {other: {"shape": [128, 128], "dtype": "BF16"}})
    from shardmerge_amd.adapter import base_tensor_meta
    from shardmerge_amd.index import LocalModelIndex
    import asyncio
    index = LocalModelIndex(storage_path=storage)
    asyncio.run(index.add_model("org/base"))
    with pytest.raises(DeltaPackError, match=rf"org/unknown.*{other}\.full.*org/base"):
        DeltaPack("org/unknown", storage / "org/unknown").check_against("org/base", base_tensor_meta(index, "org/base"))
    with pytest.raises(DeltaPackError, match=rf"org/bad_shape.*{n1}\.full.*org/base"):
        DeltaPack("org/bad_shape", storage / "org/bad_shape").check_against("org/base", base_tensor_meta(index, "org/base"))
    # a pack or an adapter as the base of a pack entry
    for bad_base, what in (("org/good", "a delta pack"), ("org/lora", "an adapter")):
        models = [{"model": "org/good", "base": bad_base, "alpha": 0.5, "is_input": True, "is_output": True}]
        res = harness.run_cli(harness.write_config(tmp_path, models, "never", OPTIONS, device))
        assert res.exit_code != 0 and not (tmp_path / "never").exists()
        from shardmerge_amd.config import MergeConfig
        from shardmerge_amd.merge import operator_class
        cfg = MergeConfig.from_yaml(tmp_path / "never.yaml")
        with pytest.raises(ValueError, match=rf"org/good.*{bad_base} is {what}"):
            asyncio.run(operator_class(cfg.operator)(config=cfg, index_manager=LocalModelIndex(storage_path=storage)).initialize())


def check_command_rejections(tmp_path, engine, device, monkeypatch):
    """everything compress-delta and extract-lora reject is rejected before DIR exists"""
    import asyncio
    from shardmerge_amd.merge.compress import DeltaCompression
    from shardmerge_amd.merge.extract import LoraExtraction
    from tests import lora_fixtures as lf
    setup_pack(tmp_path, engine, device)
    storage = tmp_path / "storage"
    odd = dict(lf.model_tensors(1))
    odd["lm_head.weight"] = odd["lm_head.weight"].float()
    lf.write_model(storage, "org/odd_dtype", odd)
    odd = dict(lf.model_tensors(1))
    odd["model.norm.weight"] = odd["model.norm.weight"][:64]
    lf.write_model(storage, "org/odd_shape", odd)
    out = storage / "org/never"

    def refused(model, match, base="org/base", bits=2, density=0.5, more=None):
        with pytest.raises(ValueError, match=match):
            asyncio.run(DeltaCompression(model, base, out, storage, bits, density, engine=engine).compress(device))
        assert not out.exists()
        more = more if more is not None else ["--bits", bits] + (["--density", density] if density is not None else [])
        res = run_cli(compress_args(tmp_path, model, "org/never", device, more, base=base))
        assert res.exit_code != 0 and not out.exists()
    refused("org/lora", "org/lora is an adapter")
    refused("org/pack", "org/pack is itself a delta pack")
    refused("org/ft1", "org/lora is an adapter", base="org/lora")
    refused("org/ft1", "org/pack is itself a delta pack", base="org/pack")
    refused("org/odd_dtype", "lm_head.weight")
    refused("org/odd_shape", "model.norm.weight")
    refused("org/ft1", "--bits 2 needs --density", density=None)
    refused("org/ft1", "--bits 1.*--density", bits=1, density=0.5)
    refused("org/ft1", "--bits", bits=3)
    refused("org/ft1", "--density", density=1.5)
    monkeypatch.setenv("WORLD_SIZE", "2")
    refused("org/ft1", "single process")
    monkeypatch.delenv("WORLD_SIZE")
    refused("org/base", "both org/base")
    with pytest.raises(ValueError, match="already holds a delta pack"):
        asyncio.run(DeltaCompression("org/ft1", "org/base", storage / "org/pack", storage, 1, engine=engine).compress(device))
    # extract-lora takes no pack, as MODEL or as BASE
    for model, base in (("org/pack", "org/base"), ("org/ft1", "org/pack")):
        with pytest.raises(ValueError, match="org/pack is a delta pack"):
            asyncio.run(LoraExtraction(model, base, 8, out, storage, engine=engine).extract(device))
        assert not out.exists()
