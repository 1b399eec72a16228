"""operator: della / della_linear on the MI355X: the kernels of csrc/sm_della.hpp against tests/della_oracle.py, bit for
bit (tests/della_checks.py) - the grid, the row lengths and the corners of the emulator tier, the identity, the
statistics, the launch counts, model-shaped cases cut to a few hundred rows (each once, alternating the two modes), and
the CLI on the device."""
import pytest
import torch

from tests import della_checks as dc
from tests import lora_fixtures as lf
from tests.harness import ALPHAS, DTYPES, KS, assert_outputs, eng, make_inputs, run_cli  # noqa: F401

pytestmark = pytest.mark.gpu

MODE_IDS = ["della", "della_linear"]
# (shape, k): more work-groups than CUs; the longest real row, no power of two; ...; the LDS limit; one row
MODEL_SHAPES = (((1024, 4096), 3), ((256, 28672), 2), ((128, 11008), 3), ((300, 4544), 3), ((16, 32768), 2), ((1, 4096), 3))


@pytest.mark.parametrize("sign_election", dc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(eng, in_dtype, bo_dtype, sign_election):
    dc.check_dtypes(eng, in_dtype, bo_dtype, sign_election, device=eng.device)


@pytest.mark.parametrize("sign_election", dc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("window", dc.WINDOWS, ids=lambda w: f"{w[0]:.4g}-{w[1]:g}")
@pytest.mark.parametrize("k", KS)
def test_k_and_window(eng, k, window, sign_election):
    dc.check_k_window(eng, k, window, sign_election, device=eng.device)


@pytest.mark.parametrize("sign_election", dc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("rescale", [True, False])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("lam", [1.0, 0.7])
def test_lambda_normalize_rescale(eng, lam, normalize, rescale, sign_election):
    dc.check_options(eng, lam, normalize, rescale, sign_election, device=eng.device)


@pytest.mark.parametrize("c", dc.ROW_LENGTHS)
def test_row_length(eng, c):
    dc.check_row_length(eng, c, device=eng.device)


CORNERS = [dc.check_signed_alphas, dc.check_row_too_long, dc.check_row_contents, dc.check_zero_delta, dc.check_denormals,
           dc.check_unaligned_and_rank3, dc.check_nonfinite, dc.check_arguments, dc.check_epsilon_zero_is_dare,
           dc.check_order_independence, dc.check_monotone_and_nested, dc.check_slabs, dc.check_determinism]


@pytest.mark.parametrize("check", CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(eng, check):
    check(eng, device=eng.device)


@pytest.mark.parametrize("window", dc.STAT_WINDOWS, ids=lambda w: f"{w[0]:g}-{w[1]:g}")
def test_statistics(eng, window):
    dc.check_statistics(eng, window, device=eng.device)


@pytest.mark.parametrize("case", list(enumerate(MODEL_SHAPES)), ids=lambda c: "x".join(map(str, c[1][0])) + f"-k{c[1][1]}-" + MODE_IDS[c[0] % 2])
def test_model_shape(eng, case):
    i, (shape, k) = case
    fts, bases, bo = make_inputs(shape, k, seed=sum(shape) % 97, device=eng.device)
    rep, _ = dc.check(eng, fts, bases, ALPHAS[:k], bo, lam=0.7, sign_election=i % 2 == 0, label=f"{shape} k={k}")
    assert (rep.threshold_lo, rep.threshold_hi) == (22937, 42598) and all(0 < kept < bo.numel() for kept in rep.kept)
    del fts, bases, bo
    torch.cuda.empty_cache()


def test_model_shape_with_own_bases(eng):
    fts, bases, bo = make_inputs((512, 4096), 3, torch.bfloat16, torch.float32, seed=3, own_bases=True, device=eng.device)
    dc.check(eng, fts, bases, [0.5, -0.3, 0.4], bo, density=0.2, epsilon=0.1, normalize=False, sign_election=False, stream_ids=[0, 2, 5],
             label="512 x 4096, own bases, fp32 output")


def test_profile_names_and_launches(eng):
    fts, bases, bo = make_inputs((1024, 1024), 2, seed=4, device=eng.device)
    _, launches = dc.profiled(eng, lambda: eng.della_merge(fts, bases, ALPHAS[:2], bo))
    assert launches == {"della_table": 1, "della_rank": 1, "della_merge": 1}
    _, launches = dc.profiled(eng, lambda: eng.della_merge(fts, bases, ALPHAS[:2], bo, epsilon=0.0))
    assert launches == {"dare_merge": 1}
    _, launches = dc.profiled(eng, lambda: eng.della_merge(fts, bases, ALPHAS[:2], bo, density=1.0, epsilon=0.0, want_thresholds=True))
    assert launches == {"dare_merge": 1}
    _, launches = dc.profiled(eng, lambda: eng.della_merge(fts, bases, ALPHAS[:2], bo, epsilon=0.0, want_thresholds=True))
    assert launches == {"della_table": 1, "dare_merge": 1}      # (the uniform threshold, written for the debugging output only)


@pytest.mark.parametrize("operator", ["della", "della_linear"])
@pytest.mark.parametrize("inplace", [False, True], ids=["single_process", "inplace"])
def test_cli_on_the_device(tmp_path, eng, monkeypatch, inplace, operator):
    if inplace:
        monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    base, factors, full = lf.setup_k3(tmp_path, eng)
    opts = dc.options(operator)
    res = run_cli(dc.write_config(tmp_path, "org/lora", "merged", opts, device="cuda"))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", dc.expected_outputs(base, full, opts))
    assert "DELLA" in (tmp_path / "merged" / "README.md").read_text()
