"""CPU test of the localised error metrics of tests/test_gemm_grad_forms_gpu.py (worst_block / worst_row): the standing proof that they see a fault which the
whole-tensor rel-L2 at the same bound does not.  It lives in a file of its own because the two GPU files mark every test they hold `gpu`.

The arithmetic.  One row of R with relative error d adds d / sqrt(R) to the whole-tensor rel-L2, in quadrature with the rounding of the other rows (one bf16
rounding of N(0,1) data: 1.6e-3).  Under the bf16 bound of 4e-3 that leaves sqrt(4e-3^2 - 1.6e-3^2) = 3.7e-3:
  * a row REPLACED by an independent N(0,1) row (d = sqrt 2, worst_row >= 1) stays invisible only from R = 2 / 3.7e-3^2 = 148,000 rows up - the first case uses
    262,144 rows (of 32 columns, the final layer's width: the column count does not enter).  At (4096, 1152) such a row reads 2.2e-2 in the whole tensor;
  * at (4096, 1152) the invisible row errors are those up to d = 0.23: the second case damages one row by 20 % (50 x the bound) and the whole tensor still passes.
A 128 x 128 block of a (4096, 1152) fp32 pair is 1 / 288 of the energy: under the fp32 bound of 2e-5 a block error of up to 3.4e-4 is invisible; the third case
damages one block by 2e-4 (10 x the bound)."""
import torch

from conftest import rel_l2
from test_gemm_grad_forms_gpu import F32_TOL, worst_block, worst_row

BF16_BOUND = 4e-3         # BF16_TOL of the default (bf16-operand) build; this test rounds to bf16 whatever PXA_OPERAND_DTYPE says


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_worst_row_sees_a_replaced_row_that_the_whole_tensor_metric_hides():
    ref = _randn(262144, 32, seed=1)
    got = ref.to(torch.bfloat16).float()
    assert worst_row(got, ref) < BF16_BOUND                       # a correct result passes both metrics
    got[123457] = _randn(32, seed=2)
    assert rel_l2(got, ref) < BF16_BOUND
    assert worst_row(got, ref) >= 1.0


def test_worst_row_sees_a_damaged_row_at_4096_x_1152():
    ref = _randn(4096, 1152, seed=1)
    got = ref.to(torch.bfloat16).float()
    assert worst_row(got, ref) < BF16_BOUND
    got[4095] = ref[4095] + 0.2 * _randn(1152, seed=2)
    assert rel_l2(got, ref) < BF16_BOUND
    assert worst_row(got, ref) >= 0.19 and worst_row(got, ref) == worst_block(got, ref, 1, 1152)


def test_worst_block_sees_a_damaged_tile_of_an_fp32_pair():
    ref = _randn(4096, 1152, seed=1).double()
    got = ref.float()
    assert worst_block(got, ref, 128, 128) < F32_TOL and worst_row(got, ref) < F32_TOL
    got[3968:4096, 1024:1152] += 2e-4 * _randn(128, 128, seed=2)   # the last tile in both directions
    assert rel_l2(got, ref) < F32_TOL
    assert worst_block(got, ref, 128, 128) >= 1.9e-4
    # ragged last blocks count: with 100 x 100 blocks the damage sits in the partial blocks of the last block row and column
    assert worst_block(got, ref, 100, 100) >= 1.9e-4 and abs(worst_block(got, ref, 4096, 1152) / rel_l2(got, ref) - 1) < 1e-9
