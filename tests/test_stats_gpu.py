"""analyze / Engine.delta_stats on the MI355X: the kernels of csrc/sm_stats.hpp (and geo_gram's) against
tests/stats_oracle.py, every report field bit for bit (tests/stats_checks.py) - the grid and the corners of the emulator
tier, model-shaped cases (the smallest at which the device path differs from the emulator's: many work-groups, several
octets per thread; none above 4096 x 4096, the CPU oracle takes seconds), and the CLI on the device."""
import pytest
import torch

from tests import lora_fixtures as lf
from tests import stats_checks as sc
from tests.harness import DTYPES, eng  # noqa: F401

pytestmark = pytest.mark.gpu

# (shape, k, own bases, densities); the last: histograms that span many work-groups
MODEL_SHAPES = [((1024, 4096), 3, False, sc.DENS4), ((300, 4544), 3, False, (0.5, 1.0, 0.5, 0.01)), ((128, 11008), 5, False, sc.DENS4),
                ((1, 4096), 3, False, sc.DENS4), ((2048, 4096), 16, True, (0.2,)), ((4096, 4096), 3, False, (0.2, 0.05))]


@pytest.mark.parametrize("n", sc.SIZES)
def test_sizes(eng, n):
    sc.check_size(eng, n, device=eng.device)


@pytest.mark.parametrize("m", sc.MS)
@pytest.mark.parametrize("k", sc.KS)
def test_k_and_m(eng, k, m):
    sc.check_k_m(eng, k, m, device=eng.device)


@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(eng, in_dtype):
    sc.check_dtypes(eng, in_dtype, device=eng.device)


@pytest.mark.parametrize("check", sc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(eng, check):
    check(eng, device=eng.device)


@pytest.mark.parametrize("shape,k,own,densities", MODEL_SHAPES, ids=["x".join(map(str, s)) + f"-k{k}" for s, k, _, _ in MODEL_SHAPES])
def test_model_shape(eng, shape, k, own, densities):
    sc.check_model_shape(eng, shape, k, own, densities, device=eng.device)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("m", sc.MS)
@pytest.mark.parametrize("k", (2, 5))
def test_profile_names_and_launches(eng, k, m):
    sc.check_profile(eng, k, m, shape=(1024, 1024), device=eng.device)


def test_c_abi_rejects_bad_arguments(eng):
    sc.check_c_abi(eng, device=eng.device)


def test_cli_on_the_device(tmp_path, eng):
    base, factors, full = lf.setup_k3(tmp_path, eng)
    res = sc.run_cli(["analyze", sc.write_config(tmp_path, "org/lora", "merged", {"operator": "ties"}, device="cuda")])
    assert res.exit_code == 0, res.output
    assert sorted(p.name for p in (tmp_path / "merged").iterdir()) == ["analysis.json"]
    sc.assert_report(tmp_path / "merged" / "analysis.json", sc.expected_records(base, full, sc.DENS4), sc.DENS4)
    assert "opposed/kept" in res.output
