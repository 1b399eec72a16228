"""DoRA and embedding-LoRA adapters on the MI355X: smhip_adapter_apply against fp64 at model shapes, bitwise
repeatability, merge_layer on a DoRA finetune, and the CLI end to end with a DoRA + embedding adapter entry."""
import math

import pytest
import torch
from click.testing import CliRunner

from tests import dora_fixtures as df
from tests import lora_fixtures as lf
from tests.harness import eng  # noqa: F401
from tests.test_dora_host import check_against_fp64, dora_slack

pytestmark = pytest.mark.gpu

SHAPES = [(4096, 4096), (14336, 4096), (4096, 14336), (28672, 8192), (1024, 8192), (4544, 4544), (11008, 4096),
          (1, 4096), (3, 5)]
RANKS = {s: [16, 256] for s in SHAPES}
RANKS[(4544, 4544)] = RANKS[(3, 5)] = [7, 16, 256]
DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _inputs(rows, cols, rank, fd, rel, g, dev):
    """base ~ N(0, 0.02^2); factors scaled so that s * B @ A has ~ rel times the base's size (s = 2); m ~ U(0.5, 1.5)"""
    s = 2.0
    sig = math.sqrt(0.02 * rel / (s * math.sqrt(rank)))
    base = torch.randn(rows, cols, generator=g, device=dev) * 0.02
    a = (torch.randn(rank, cols, generator=g, device=dev) * sig).to(fd)
    b = (torch.randn(rows, rank, generator=g, device=dev) * sig).to(fd)
    m = torch.rand(rows, generator=g, device=dev) + 0.5
    return base, a, b, s, m


@pytest.mark.parametrize("bd", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dora_apply_against_fp64(eng, shape, bd):
    rows, cols = shape
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(rows * 11 + cols)
    diffs = total = 0
    for rank in RANKS[shape]:
        for fd in DTYPES:
            for rel in (1.0, 0.01):
                base32, a, b, s, m = _inputs(rows, cols, rank, fd, rel, g, dev)
                base = base32.to(bd)
                del base32
                md = torch.bfloat16 if fd == torch.bfloat16 else torch.float32
                m = m.to(md)
                out = eng.lora_apply(base, a, b, s, magnitude=m)
                again = eng.lora_apply(base, a, b, s, magnitude=m)
                assert torch.equal(_bits(out), _bits(again)), (shape, rank, fd, rel)
                del again
                e, f = df.dora_ref(base, a, b, s, m)
                n = check_against_fp64(out, e, dora_slack(a, b, s, fd, f), bd)
                if bd != torch.float32:
                    diffs += n
                    total += out.numel()
                del e, f, out, base, a, b, m
    if bd != torch.float32 and total >= 4096 * 30:
        assert diffs <= 1e-3 * total, (shape, bd, diffs, total)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("rows", [32000, 128256])
@pytest.mark.parametrize("rank", [16, 64])
def test_embedding_apply_against_fp64(eng, rows, rank):
    cols = 4096
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(rows + rank)
    diffs = total = 0
    base = (torch.randn(rows, cols, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    a = (torch.randn(rank, rows, generator=g, device=dev) * 0.05).to(torch.bfloat16)     # lora_embedding_A
    b = (torch.randn(cols, rank, generator=g, device=dev) * 0.05).to(torch.bfloat16)     # lora_embedding_B
    out = eng.lora_apply(base, a, b, 2.0, embedding=True)
    assert torch.equal(_bits(out), _bits(eng.lora_apply(base, a, b, 2.0, embedding=True)))
    # the embedding layout is plain LoRA with the factors' roles transposed
    assert torch.equal(_bits(out), _bits(eng.lora_apply(base, b.T.contiguous(), a.T.contiguous(), 2.0)))
    for r0 in range(0, rows, 16384):                       # (fp64 reference in slices of rows)
        sl = slice(r0, min(rows, r0 + 16384))
        e, _ = df.dora_ref(base[sl], a[:, sl], b, 2.0, None, embedding=True)
        diffs += check_against_fp64(out[sl], e, dora_slack(a[:, sl], b, 2.0, torch.bfloat16, None, embedding=True),
                                    torch.bfloat16)
        total += e.numel()
        del e
    assert diffs <= 1e-3 * total, (diffs, total)
    torch.cuda.empty_cache()


def test_no_magnitude_through_the_new_entry_equals_lora_apply(eng):
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(3)
    for bd in DTYPES:
        base, a, b, s, _ = _inputs(4544, 4544, 16, torch.bfloat16, 1.0, g, dev)
        base = base.to(bd)
        assert torch.equal(_bits(eng.adapter_apply(base, a, b, s)), _bits(eng.lora_apply(base, a, b, s)))


def test_zero_norm_row_raises_naming_the_row(eng):
    from shardmerge_amd._lib import ERR_ROW_NORM, SmhipError
    dev = eng.device
    base = torch.randn(4096, 4096, device=dev) * 0.02
    a, b = torch.randn(16, 4096, device=dev) * 0.05, torch.randn(4096, 16, device=dev) * 0.05
    base[1234] = 0
    b[1234] = 0
    m = torch.ones(4096, device=dev)
    m[3000] = float("nan")
    with pytest.raises(SmhipError, match=r"row 1234 .*\(2 of 4096 rows\)") as ei:
        eng.lora_apply(base.to(torch.bfloat16), a.to(torch.bfloat16), b.to(torch.bfloat16), 2.0, magnitude=m)
    assert ei.value.code == ERR_ROW_NORM


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("norm_mode", ["reference_cpu", "exact"])
def test_merge_layer_on_dora_finetune_equals_reuploaded(eng, k, norm_mode):
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(8192 + k)
    base = (torch.randn(4096, 4096, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    fts = [(base.float() + torch.randn(4096, 4096, generator=g, device=dev) * 0.003).to(torch.bfloat16)
           for _ in range(k - 1)]
    a = (torch.randn(16, 4096, generator=g, device=dev) * 0.05).to(torch.bfloat16)
    b = (torch.randn(4096, 16, generator=g, device=dev) * 0.05).to(torch.bfloat16)
    m = base.float().norm(dim=1) * (1 + 0.1 * torch.randn(4096, generator=g, device=dev))
    ft_dora = eng.lora_apply(base, a, b, 2.0, magnitude=m)
    ft_copy = ft_dora.cpu().to(dev)
    alphas = [0.5, 0.3, 0.2][:k]
    out1, rep1 = eng.merge_layer(fts + [ft_dora], [base] * k, alphas, base, norm_mode=norm_mode)
    out2, rep2 = eng.merge_layer(fts + [ft_copy], [base] * k, alphas, base, norm_mode=norm_mode)
    torch.cuda.synchronize()
    assert rep1.branches == rep2.branches
    assert torch.equal(out1.view(torch.uint8), out2.view(torch.uint8))


@pytest.mark.parametrize("inplace", [False, True])
def test_cli_on_device_dora_adapter_entry_equals_materialised_checkpoint(tmp_path, eng, monkeypatch, inplace):
    from shardmerge_amd.__main__ import cli
    if inplace:
        monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    df.setup_k3(tmp_path, eng)
    for adapter, out in (("org/dora", "merged_adapter"), ("org/dora_full", "merged_full")):
        res = CliRunner().invoke(cli, ["merge", str(lf.write_config(tmp_path, df.k3_models_input(adapter), out))])
        assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged_full", file_bytes=not inplace)
