"""LoRA adapters as finetunes on the MI355X: smhip_lora_apply against fp64 at model shapes, merge_layer on an
adapter-derived finetune, and the CLI end to end with an adapter entry (single process and in-place shards)."""
import math

import pytest
import torch
from click.testing import CliRunner

from tests import lora_fixtures as lf
from tests.harness import eng  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = [(4096, 4096), (14336, 4096), (4096, 14336), (28672, 8192), (1024, 8192), (4544, 4544), (11008, 4096),
          (1, 4096), (3, 5)]
RANKS = [1, 7, 16, 64, 256]
DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _inputs(rows, cols, rank, fd, rel, g, dev):
    """base ~ N(0, 0.02^2); factors scaled so that s * B @ A has ~ rel times the base's size (s = 2)"""
    s = 2.0
    sig = math.sqrt(0.02 * rel / (s * math.sqrt(rank)))
    base = torch.randn(rows, cols, generator=g, device=dev) * 0.02
    a = (torch.randn(rank, cols, generator=g, device=dev) * sig).to(fd)
    b = (torch.randn(rows, rank, generator=g, device=dev) * sig).to(fd)
    return base, a, b, s


def _spacing(r):
    """distance from |r| to the next value of r's 16-bit dtype (fp64)"""
    mant, tiny = (7, 2.0 ** -133) if r.dtype == torch.bfloat16 else (10, 2.0 ** -24)
    _, e = torch.frexp(r.double())
    return torch.ldexp(torch.ones_like(r, dtype=torch.float64), e - 1 - mant).clamp_min(tiny)


@pytest.mark.parametrize("bd", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_lora_apply_against_fp64(eng, shape, bd):
    rows, cols = shape
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(rows * 7 + cols)
    diffs = total = 0
    for rank in RANKS:
        for fd in DTYPES:
            for rel in (1.0, 0.01):
                base32, a, b, s = _inputs(rows, cols, rank, fd, rel, g, dev)
                base = base32.to(bd)
                del base32
                out = eng.lora_apply(base, a, b, s)
                again = eng.lora_apply(base, a, b, s)
                assert torch.equal(out.view(torch.uint8) if bd != torch.float32 else out.view(torch.int32),
                                   again.view(torch.uint8) if bd != torch.float32 else again.view(torch.int32))
                del again
                sf = float(torch.tensor(s, dtype=torch.float32))
                e = base.double() + sf * (b.double() @ a.double())
                if bd == torch.float32:
                    bound = 2.0 ** -24 * e.abs() + (rank + 2) * 2.0 ** -24 * sf * (b.double().abs() @ a.double().abs())
                    bad = ((out.double() - e).abs() > bound).sum().item()
                    assert bad == 0, (shape, rank, fd, rel, bad)
                    del bound
                else:
                    # one ulp of the once-rounded value, plus what the fp32 sum of the contract may lose where the
                    # result cancels against the base (16-bit factors; fp32 factors are summed in fp64 and need none)
                    r = e.to(bd)
                    acc_err = 0.0 if fd == torch.float32 else (rank + 2) * 2.0 ** -24 * sf * (b.double().abs() @ a.double().abs())
                    ulps = (((out.double() - r.double()).abs() - acc_err).clamp_min(0) / _spacing(r)).max().item()
                    assert ulps <= 1.0 + 1e-9, (shape, rank, fd, rel, ulps)     # (the device's fp64 division)
                    del acc_err
                    diffs += (out != r).sum().item()
                    total += out.numel()
                    del r
                del e, out, base, a, b
    if bd != torch.float32 and total >= 4096 * 30:      # (a fraction of a few dozen elements says nothing)
        assert diffs <= 1e-3 * total, (shape, bd, diffs, total)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("norm_mode", ["reference_cpu", "exact"])
def test_merge_layer_on_adapter_finetune_equals_reuploaded(eng, k, norm_mode):
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(4096 + k)
    base = (torch.randn(4096, 4096, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    fts = [(base.float() + torch.randn(4096, 4096, generator=g, device=dev) * 0.003).to(torch.bfloat16)
           for _ in range(k - 1)]
    a = (torch.randn(16, 4096, generator=g, device=dev) * 0.05).to(torch.bfloat16)
    b = (torch.randn(4096, 16, generator=g, device=dev) * 0.05).to(torch.bfloat16)
    ft_lora = eng.lora_apply(base, a, b, 2.0)
    ft_copy = ft_lora.cpu().to(dev)
    alphas = [0.5, 0.3, 0.2][:k]
    out1, rep1 = eng.merge_layer(fts + [ft_lora], [base] * k, alphas, base, norm_mode=norm_mode)
    out2, rep2 = eng.merge_layer(fts + [ft_copy], [base] * k, alphas, base, norm_mode=norm_mode)
    torch.cuda.synchronize()
    assert rep1.branches == rep2.branches
    assert torch.equal(out1.view(torch.uint8), out2.view(torch.uint8))


@pytest.mark.parametrize("inplace", [False, True])
def test_cli_on_device_adapter_entry_equals_materialised_checkpoint(tmp_path, eng, monkeypatch, inplace):
    from shardmerge_amd.__main__ import cli
    if inplace:
        monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    lf.setup_k3(tmp_path, eng)
    for cfg, out in ((lf.write_config(tmp_path, lf.k3_models("org/lora"), "merged_adapter"), "merged_adapter"),
                     (lf.write_config(tmp_path, lf.k3_models("org/lora_full"), "merged_full"), "merged_full")):
        res = CliRunner().invoke(cli, ["merge", str(cfg)])
        assert res.exit_code == 0, res.output
    # (the in-place shards carry a stamp of their configuration, which names the models: compare the tensors there)
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged_full", file_bytes=not inplace)
