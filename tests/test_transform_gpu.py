"""Device tier of the per-bin transform conformance (tests/transform_checks.py): the same checks through
libshardmerge_hip.so on a real MI355X, every input in a call of its own, the whole input list at every folded shape, and
the two shapes that fold without a hook as the product runs them."""
import pytest

from tests import transform_checks as tc
from tests.harness import eng  # noqa: F401  (pytest registers the fixture in this module)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape,axis", tc.fn_shapes(), ids=lambda v: tc.shape_id(v) if isinstance(v, tuple) else None)
def test_transforms_per_bin_on_device(eng, shape, axis):
    tc.check_transforms(eng, shape, axis)


@pytest.mark.parametrize("n", tc.MISALIGNED_LENGTHS)
def test_misaligned_views_per_bin_on_device(eng, n):
    """the element-wise path of a device view that is not 16-byte aligned"""
    tc.check_misaligned_transforms(eng, n)


@pytest.mark.parametrize("shape", tc.FOLDED_SHAPES, ids=tc.shape_id)
def test_folded_column_pass_closed_form_on_device(eng, shape):
    tc.check_folded(eng, shape)


@pytest.mark.parametrize("shape", tc.UNHOOKED_DEVICE_SHAPES, ids=tc.shape_id)
def test_shapes_that_fold_by_themselves_closed_form_on_device(eng, shape):
    tc.check_unhooked_folded(eng, shape)


@pytest.mark.parametrize("cid", tc.PATH_CASE_IDS)
def test_merge_only_paths_closed_form_on_device(eng, cid):
    tc.check_path(eng, cid)
