"""operator: wudi on the MI355X: the checks of tests/wudi_checks.py on the device - the three GEMM kernels of
csrc/sm_wudi.hpp on v_mfma_f32_32x32x2_f32 and the whole function bit for bit against tests/wudi_oracle.py, what defines
the method against torch fp64, the C ABI and the launch counts - then two model-shaped cases (256 x 1024: eight tiles along
n, 32 k-blocks; 300 x 568: unaligned edges) against the emulator library that build() produces, and the CLI on the device.
No case runs more than 5 iterations or is larger than 512 x 2048."""
import pytest
import torch

from tests import wudi_checks as wc
from tests.harness import eng  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", wc.CASES)
def test_engine(eng, case):
    wc.CASES[case](eng)


@pytest.mark.parametrize("shape", [(256, 1024), (300, 568)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_model_shape_against_the_emulator(eng, shape):
    from tests.emul.loader import emul_engine
    fts, bases, base_out = wc.merge_inputs(shape, 3)
    got, want = (wc.wudi(e, fts, bases, list(wc.ALPHAS[:3]), base_out, iters=2, lr=1e-4, lam=0.7) for e in (eng, emul_engine()))
    assert torch.equal(wc.raw(got[0]), wc.raw(want[0])) and torch.equal(wc.raw(got[2]), wc.raw(want[2])) and got[1] == want[1], shape


@pytest.mark.parametrize("inplace", [False, True], ids=["single_process", "inplace"])
def test_cli_on_the_device(tmp_path, eng, monkeypatch, inplace):
    if inplace:
        monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    wc.check_cli(tmp_path, eng, device="cuda", third="org/lora")
