"""Emulator tier of the per-bin transform conformance (tests/transform_checks.py): the kernel bodies and the host
orchestration in the CPU work-group emulator, against the fp64 DFT, with torch's fp32 FFT / the fp32 oracle measuring the
tolerance on the same inputs.

The emulator runs one work-group per bin column at tens of microseconds each, whatever the other length is: from
BATCH_FROM points on the inputs of a family share one call ([16 x n] / [n x 16], one member per row / column); the device
tier runs every input in a call of its own at every length.  The folded shapes run the whole input list here too (one to
two minutes for the longest)."""
import pytest
import torch

from tests import transform_checks as tc
from tests.harness import REPO, emul  # noqa: F401  (pytest registers the fixture in this module)

_batched = tc.emulator_batched


def test_restated_static_lengths_are_the_plans_of_the_library(emul):
    """STATIC_LENGTHS restates SM_STATIC_PLANS: the same twenty lengths as sm_plans.hpp lists, each one supported"""
    import re
    text = (REPO / "shardmerge_amd" / "csrc" / "sm_plans.hpp").read_text()
    listed = [int(n) for n in re.findall(r"X\(SPlan<(\d+),", text)]
    assert len(tc.STATIC_LENGTHS) == 20 and sorted(listed) == sorted(tc.STATIC_LENGTHS)
    for n in tc.STATIC_LENGTHS + tc.RUNTIME_LENGTHS:
        assert emul.lib.length_supported(n), n
    for shape in tc.CHIRP_SHAPES:
        assert not emul.lib.length_supported(shape[1]) and emul.lib.shape_supported(*shape), shape


@pytest.mark.parametrize("shape,axis", tc.fn_shapes(), ids=lambda v: tc.shape_id(v) if isinstance(v, tuple) else None)
def test_transforms_per_bin(emul, shape, axis):
    tc.check_transforms(emul, shape, axis, batched=_batched(shape, axis))


@pytest.mark.parametrize("n", tc.MISALIGNED_LENGTHS)
def test_misaligned_views_per_bin(emul, n):
    """the element-wise path of a view that is not 16-byte aligned"""
    tc.check_misaligned_transforms(emul, n, batched=n >= tc.BATCH_FROM)


def test_complex_packed_variant_per_bin():
    """fft_engine.hpp's PACK mode 2 (the alternate emulator build of test_complex_packed_engine_mode), at its lengths"""
    from tests.emul.loader import emul_engine_variant
    eng = emul_engine_variant(list(tc.PACKED_FLAGS), "cpx")
    for n in tc.PACKED_LENGTHS:
        for shape, axis in (((2, n), 1), ((n, 2), 0)):
            tc.check_transforms(eng, shape, axis, batched=True)


@pytest.mark.parametrize("shape", tc.FOLDED_SHAPES, ids=tc.shape_id)
def test_folded_column_pass_closed_form(emul, shape):
    tc.check_folded(emul, shape)


@pytest.mark.parametrize("cid", tc.PATH_CASE_IDS)
def test_merge_only_paths_closed_form(emul, cid):
    tc.check_path(emul, cid)


# ---- the check bites where the old one did not (CPU only: a perturbed fp64 DFT, no kernel is edited) -------------------
@pytest.mark.parametrize("model", [lambda mag: tc.one_twiddle_off(1365, mag), tc.phase_drift], ids=["one_twiddle", "phase_drift"])
def test_defective_dft_passes_the_old_criterion_and_fails_the_new(model):
    """n = 8192, a defect in the last stage's twiddles as large as the old criterion (Gaussian noise, normwise 3e-6
    against torch's fp32 FFT) lets pass: the per-bin check rejects it on a member of its families"""
    n = 8192
    mag, fft = tc.largest_passing_defect(model, n)
    assert tc.old_criterion_passes(fft, n)
    assert mag >= 2.0 ** -20, mag                       # a defect of 1e-6 and more, far beyond fp32 rounding
    rejected = tc.rejected_inputs(fft, n)
    print(f"defect magnitude 2^{int(torch.log2(torch.tensor(mag)))}: rejected on {rejected}")
    assert rejected
