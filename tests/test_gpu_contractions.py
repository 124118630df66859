"""The contraction kernels around the fp16 two-piece family against float64 numpy (cases, references and judges:
tests/contraction_cases.py): gemm_plain_kernel in its eight forms, fwd_narrow_in_kernel at every lanes-per-row setting and the
launches it declines, gemm_split_kernel in its six forms in fp32 and in bf16 storage, gconv_fwd_kernel in bf16 storage and as the
fp32 128 x 128 tile, and every (storage, kernel, tile) form of the weight gradient with both slab reductions.  Each case asserts the
exact plan tuple the library reports before it judges; the plans are those of the default environment."""
import pytest

from tests import contraction_cases as K

pytestmark = pytest.mark.gpu

_name = lambda c: c["name"]


@pytest.mark.parametrize("case", K.PLAIN_CASES, ids=_name)
def test_plain_forward(case):
    K.run_fwd(case)


@pytest.mark.parametrize("case", K.NARROW_CASES, ids=_name)
def test_narrow_in_forward(case):
    """The narrow kernel, the launches it declines (the plan still answers 4, gemm_plain_kernel runs) and its neighbours."""
    K.run_fwd(case)


@pytest.mark.parametrize("case", K.SPLIT_CASES, ids=_name)
def test_split_forward(case):
    K.run_fwd(case)


@pytest.mark.parametrize("case", K.SPLIT_BF16_CASES, ids=_name)
def test_split_forward_bf16(case):
    K.run_fwd(case)


@pytest.mark.parametrize("case", K.GENERIC_CASES, ids=_name)
def test_generic_forward(case):
    K.run_fwd(case)


@pytest.mark.parametrize("case", K.VIEW_CASES, ids=_name)
def test_channel_offset_views_next_to_nan(case):
    """Sources = channel-offset slices of buffers whose other columns hold NaN, output = a slice of a sentinel-filled buffer: the
    family is still taken, the result is finite and within the bar, nothing is written outside the view."""
    K.run_fwd(case)


@pytest.mark.parametrize("case", K.DW_CASES, ids=_name)
def test_weight_gradient(case):
    K.run_dw(case)


@pytest.mark.parametrize("case", K.DW_BF16_CASES, ids=_name)
def test_weight_gradient_bf16(case):
    K.run_dw(case)
