"""ops.gemm in the five forms T5Encoder.forward calls it per block (pixart_sigma_amd/t5/encoder.py), at row counts and widths where pxa_gemm's dispatch
(csrc/gemm.hip: choose_gemm) gives them the kernels a real batch reaches: M >= 1024 and N >= 1024, so the persistent 256 x 256 kernel for the 16-bit outputs
and the 256 x 256 two-stage kernel with the direct epilogue for the fp32 residual.  tests/test_t5_kernels_gpu.py and tests/test_t5_model_gpu.py stay below
that threshold at every GEMM (N = 128 .. 384), so what they check is the 128 x 128 kernel.  tools/extract_t5_features.py defaults to 8 prompts of 300 tokens:
M = 2400 rows = 9 x 256 + 96, never a multiple of the tile.

Shapes.  (d_model, inner, d_ff) = (1024, 1024, 1280) at M = 1120 = 4 x 256 + 96 (the remainder of 2400: the second 128-row wave row of the last tile is wholly
out of range) and M = 1200 = 4 x 256 + 176 (partly in range); one case per call at T5-XXL's widths (4096, 4096, 10240) with M = 2400: 480 / 400 output tiles
on 256 CUs, so a workgroup of the persistent kernel takes a second item, and 160 k-tiles into one fp32 accumulator for wff; M = 900 and 300 (the last, smaller
batch of a prompt file) for one 16-bit and one fp32 form below the threshold.  Each test asserts through ops.gemm_plan the instance it is there for.

Reference everywhere: the fp64 product of the operand-rounded inputs, on the GPU.  Bounds, helpers and guard bands are those of tests/test_gemm_grad_forms_gpu.py
(none new): 16-bit outputs BF16_TOL for the whole tensor, the worst row and the worst 64 x 64 block (a wave's store tile); the fp32 residual 2e-5 for the whole
tensor, the worst 128 x 128 block and the worst row of (x - x0) against n x the product after the n-th accumulating call.  Every output is a view between
GUARD = 256 rows (and, where stated, columns) of a bit pattern compared afterwards: SENTINEL16 around stored outputs, -0.0 around the residual (a masked
lane's stray + 0.0 clears the sign), NaN around h0, which is wi1's aux operand: an aux row at or past M that reaches a stored value shows.  The A operands lie
between NaN rows as well.  g is held against gelu_tanh(x W0^T) * (x W1^T), so it carries h0's rounding and its own: about sqrt(2) x one rounding.

Census: encoder.py line -> test
  qkv = gemm(xn, wqkv, NT)                                   test_wqkv_packed_output            gemm_pers_kernel<0,0,0,false>
  gemm(a, wo, NT, out_f32=x, accumulate=True)                test_residual_projections[wo]      gemm_glds_kernel<0,256,256,2,4,0,false>, accumulate mode 2
  h0 = gemm(xn, wi0, NT, act=GELU)                           test_gated_gelu_chain (h0)         gemm_pers_kernel<0,7,0,false>
  g = gemm(xn, wi1, NT, act=MUL_AUX, aux=h0)                 test_gated_gelu_chain (g)          gemm_pers_kernel<0,3,0,false>
  gemm(g, wff, NT, out_f32=x, accumulate=True)               test_residual_projections[wff]     gemm_glds_kernel<0,256,256,2,4,0,false>, accumulate mode 2
  the residual with ld_f32 > N (a C-ABI caller's slice)      test_residual_column_slice
  wi1 and wo at M = 900 / 300                                test_below_the_row_threshold       gemm_glds_kernel<0,128,128,2,2,1,false> / <0,128,128,2,2,0,false>
  all of the above under the fp16-operand library            test_f16_build_runs_this_file

Measured on an MI355X, per case and build: the table MEASURED below (every figure is also written by record_parity)."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from conftest import ROOT, record_parity  # noqa: E402
from test_kernels_gpu import BF16_TOL, _gpu_rnd, _opd, bf, ops  # noqa: E402,F401
from test_gemm_grad_forms_gpu import (GUARD, MINUS_ZERO32, SENTINEL16, Banded, accumulate_twice, check_16, plan_of, worst_block)  # noqa: E402

MEASURED = """
rel-L2 against fp64 on an MI355X; every guard band intact, every plan as named.  16-bit outputs: worst 64 x 64 block / worst row (bound 4e-3 with bf16 operands,
5e-4 with fp16 operands); fp32 residual: worst 128 x 128 block / worst row of the two calls (bound 2e-5).
  output  case      bf16 operands          fp16 operands
  wqkv    M1120     1.76e-3 / 1.76e-3      2.17e-4 / 2.18e-4
          M1200     1.73e-3 / 1.76e-3      2.17e-4 / 2.18e-4
          xxl       1.77e-3 / 1.71e-3      2.21e-4 / 2.14e-4
  h0      M1120     1.79e-3 / 1.89e-3      2.24e-4 / 2.32e-4
          M1200     1.76e-3 / 1.89e-3      2.24e-4 / 2.32e-4
          xxl       1.85e-3 / 1.74e-3      2.30e-4 / 2.18e-4
          M900      1.86e-3 / 1.89e-3      2.43e-4 / 2.32e-4
          M300      1.75e-3 / 1.81e-3      2.26e-4 / 2.32e-4
  g       M1120     2.72e-3 / 3.18e-3      3.53e-4 / 3.76e-4
          M1200     2.72e-3 / 3.18e-3      3.37e-4 / 3.76e-4
          xxl       2.82e-3 / 2.57e-3      3.44e-4 / 3.23e-4
          M900      3.02e-3 / 3.18e-3      4.01e-4 / 3.61e-4
          M300      2.69e-3 / 2.95e-3      3.30e-4 / 3.56e-4
  wo      M1120     1.9e-7 / 2.2e-7        2.2e-7 / 2.4e-7
          M1200     1.9e-7 / 2.2e-7        2.2e-7 / 2.4e-7
          xxl       4.1e-7 / 4.3e-7        4.2e-7 / 4.3e-7
          M900      2.1e-7 / 2.2e-7        2.4e-7 / 2.4e-7
          M300      1.9e-7 / 2.1e-7        2.1e-7 / 2.3e-7
  wff     M1120     2.2e-7 / 2.5e-7        2.4e-7 / 2.6e-7      (the same with ld_f32 > N)
          M1200     2.2e-7 / 2.5e-7        2.4e-7 / 2.6e-7      (the same with ld_f32 > N)
          xxl       6.6e-7 / 6.9e-7        6.6e-7 / 6.8e-7
g carries two roundings (h0's and its own): whole tensor 2.35e-3 (bf16) / 2.94e-4 (fp16) = sqrt(2) x the 1.66e-3 / 2.08e-4 of one; its worst row and its worst
ragged block (M = 900 leaves 4 rows to the last 64-row block) are where a bound is closest: 80 %.
"""

# (M, d_model, inner, d_ff)
SMALL = [(1120, 1024, 1024, 1280), (1200, 1024, 1024, 1280)]
XXL = (2400, 4096, 4096, 10240)
SHAPES = SMALL + [XXL]
IDS = ["M1120", "M1200", "xxl_M2400"]
PERS_PLAIN, PERS_GELU, PERS_GENERIC = "gemm_pers_kernel<0,0,0,false>", "gemm_pers_kernel<0,7,0,false>", "gemm_pers_kernel<0,3,0,false>"
GLDS_256_DIRECT, GLDS_128_DIRECT, GLDS_128_STAGED = ("gemm_glds_kernel<0,256,256,2,4,0,false>", "gemm_glds_kernel<0,128,128,2,2,0,false>",
                                                      "gemm_glds_kernel<0,128,128,2,2,1,false>")


def nan16():
    """the bits of a quiet NaN in the operand type"""
    return 0x7E00 if _opd() == torch.float16 else 0x7FC0


def operand(rows, cols, seed):
    """an A operand as the encoder has it (a contiguous 16-bit (rows, cols) tensor of N(0, 1) values), between NaN rows"""
    t = Banded(rows, cols, _opd(), nan16())
    t.view.copy_(bf(_gpu_rnd(rows, cols, seed=seed)))
    return t.view


def weight(N, K, seed):
    return bf(_gpu_rnd(N, K, scale=K ** -0.5, seed=seed))


def check_16_blocks(label, got, ref):
    """check_16 (whole tensor, worst row) and the worst 64 x 64 block, all at BF16_TOL"""
    check_16(label, got, ref)
    eb = worst_block(got, ref, 64, 64)
    print(f"[{label}] worst 64x64 block {eb:.2e}")
    record_parity(f"{label} worst 64x64 block", eb, BF16_TOL)
    assert eb < BF16_TOL, (label, eb, BF16_TOL)


def assert_edges(M, N):
    """the shape conditions of choose_gemm's branch for the encoder's forms above the threshold, and the raggedness the case is there for"""
    assert M >= 1024 and N >= 1024 and N % 256 == 0 and M % 256 != 0
    if M == 1120:
        assert M % 256 == 96 and M % 256 <= 128
    if M == 1200:
        assert 128 < M % 256 < 256
    if M == 2400:
        assert M % 256 == 96


# ------------------------------------------------------------------------------------------------ wqkv
@pytest.mark.parametrize("M,D,inner,dff", SHAPES, ids=IDS)
def test_wqkv_packed_output(ops, M, D, inner, dff):
    """qkv = gemm(xn, wqkv, NT): the packed (M, 3 inner) output, here a view between SENTINEL16 rows and columns."""
    N, K = 3 * inner, D
    assert_edges(M, N)
    xn, w = operand(M, K, 1), weight(N, K, 2)
    out = Banded(M, N, _opd(), SENTINEL16, col_bands=True)
    out.view.fill_(float("nan"))
    plan = plan_of(ops, xn, w, ops.NT, out=out.view)
    assert (plan["kernel"], plan["split"], plan["try_nt4"]) == (PERS_PLAIN, 1, 1), plan
    if M == 2400:
        assert ((M + 255) // 256) * (N // 256) == 480
    got = ops.gemm(xn, w, ops.NT, out=out.view)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.view.data_ptr()
    out.assert_intact(f"t5 wqkv {M}x{N} K={K}")
    check_16_blocks(f"t5 wqkv {M}x{N} K={K}", out.view, xn.double() @ w.double().t())


# ------------------------------------------------------------------------------------------------ wi0 -> wi1
def gated_gelu(ops, label, M, N, K, kernels):
    xn, w0, w1 = operand(M, K, 1), weight(N, K, 2), weight(N, K, 3)
    h0, g = Banded(M, N, _opd(), nan16()), Banded(M, N, _opd(), SENTINEL16)
    h0.view.fill_(float("nan"))
    g.view.fill_(float("nan"))
    call0, call1 = dict(act=ops.ACT_GELU, out=h0.view), dict(act=ops.ACT_MUL_AUX, aux=h0.view, out=g.view)
    assert (plan_of(ops, xn, w0, ops.NT, **call0)["kernel"], plan_of(ops, xn, w1, ops.NT, **call1)["kernel"]) == kernels
    ops.gemm(xn, w0, ops.NT, **call0)
    ops.gemm(xn, w1, ops.NT, **call1)
    torch.cuda.synchronize()
    h0.assert_intact(f"{label} h0")
    g.assert_intact(f"{label} g")
    want_h = F.gelu(xn.double() @ w0.double().t(), approximate="tanh")
    check_16_blocks(f"{label} h0 = gelu(x W0^T)", h0.view, want_h)
    want_h *= xn.double() @ w1.double().t()
    check_16_blocks(f"{label} g = gelu(x W0^T) * (x W1^T)", g.view, want_h)


@pytest.mark.parametrize("M,D,inner,dff", SHAPES, ids=IDS)
def test_gated_gelu_chain(ops, M, D, inner, dff):
    """h0 = gemm(xn, wi0, NT, act=GELU) without a bias and with one output (the persistent kernel's GELU flavour), then g = gemm(xn, wi1, NT, act=MUL_AUX,
    aux=h0) without column sums (its run-time generic flavour), chained as the encoder chains them; h0 lies between NaN rows when wi1 reads it."""
    assert_edges(M, dff)
    if M == 2400:
        assert ((M + 255) // 256) * (dff // 256) == 400
    gated_gelu(ops, f"t5 wi {M}x{dff} K={D}", M, dff, D, (PERS_GELU, PERS_GENERIC))


# ------------------------------------------------------------------------------------------------ wo / wff
def residual(ops, label, M, N, K, kernel, col_bands=False):
    """x (fp32, N(0, 1), between -0.0 bands) += a W^T, twice: (x - x0) against n x the fp64 product after each call"""
    a, w = operand(M, K, 1), weight(N, K, 2)
    x = Banded(M, N, torch.float32, MINUS_ZERO32, col_bands=col_bands)
    plan = plan_of(ops, a, w, ops.NT, out_f32=x.view, accumulate=True)
    assert (plan["kernel"], plan["split"], plan["k_per_split"], plan["accumulate"], plan["splitk_reduce"]) == (kernel, 1, K, 2, 0), plan
    accumulate_twice(ops, label, a, w, ops.NT, x, a.double() @ w.double().t(), split_k=1, poison=False)


@pytest.mark.parametrize("which", ["wo", "wff"])
@pytest.mark.parametrize("M,D,inner,dff", SHAPES, ids=IDS)
def test_residual_projections(ops, M, D, inner, dff, which):
    """gemm(a, wo, NT, out_f32=x, accumulate=True) with K = inner and gemm(g, wff, NT, out_f32=x, accumulate=True) with K = d_ff: the fp32 residual stream is
    read and written in place by one k-slice (accumulate mode 2) of the 256 x 256 two-stage kernel's direct epilogue."""
    K = inner if which == "wo" else dff
    assert_edges(M, D)
    if (M, which) == (2400, "wff"):
        assert K // 64 == 160
    residual(ops, f"t5 {which} {M}x{D} K={K}", M, D, K, GLDS_256_DIRECT)


@pytest.mark.parametrize("M,D,inner,dff", SMALL, ids=IDS[:2])
def test_residual_column_slice(ops, M, D, inner, dff):
    """the same call with ld_f32 > N: the residual is a column slice of a wider fp32 tensor, -0.0 on all four sides"""
    assert_edges(M, D)
    residual(ops, f"t5 wff {M}x{D} K={dff} ld={D + 2 * GUARD}", M, D, dff, GLDS_256_DIRECT, col_bands=True)


# ------------------------------------------------------------------------------------------------ below the threshold
@pytest.mark.parametrize("M", [900, 300])
def test_below_the_row_threshold(ops, M):
    """M < 1024 at the same widths: the 128 x 128 two-stage kernel, staged epilogue for wi0 / wi1, direct for the residual; 900 = 7 x 128 + 4, 300 = 2 x 128 + 44"""
    _, D, inner, dff = SMALL[0]
    assert M < 1024 <= min(D, dff) and M % 128 != 0
    gated_gelu(ops, f"t5 wi {M}x{dff} K={D}", M, dff, D, (GLDS_128_STAGED, GLDS_128_STAGED))
    residual(ops, f"t5 wo {M}x{D} K={inner}", M, D, inner, GLDS_128_DIRECT)


# ------------------------------------------------------------------------------------------------ the fp16-operand build
def test_f16_build_runs_this_file():
    """This file again, in a fresh process under the fp16-operand library (one operand type per process; the GEMM build bench.py times, and these instances
    are shared with the denoiser), with BF16_TOL of that build."""
    env = dict(os.environ, PXA_OPERAND_DTYPE="f16")
    env.pop("PXA_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-s", "-p", "no:cacheprovider", "-k", "not f16_build"],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    tail = "\n".join(ln for ln in r.stdout.splitlines() if ("passed" in ln or "failed" in ln or "FAILED" in ln or "Error" in ln))
    print("\n[f16 build] " + tail.replace("\n", "\n[f16 build] "))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert "skipped" not in tail and "passed" in tail, tail
