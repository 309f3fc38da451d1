"""The FP8 weight kernels of csrc/gemm_w8.hip on the GPU: pxa_fp8_quant_rows bit for bit against the torch statement of tests/t5_fp8_refs.py,
pxa_fp8_dequant_rows bit for bit against (q.float() * s[:, None]).to(operand), and pxa_gemm_w8 in the five forms T5Encoder calls it per block.

GEMM reference: the fp64 product, on the GPU, of the 16-bit activations and scale * q taken in fp64.  Bounds are the project's own (tests/test_t5_gemm_forms_gpu.py):
BF16_TOL for 16-bit outputs over the whole tensor, the worst row and the worst 64 x 64 block; 2e-5 for the fp32 residual after each of two accumulating calls
(accumulate_twice).  They apply unchanged because the kernel multiplies the same 16-bit-representable operands into fp32 that pxa_gemm does.  Row counts are the
ones a 64-row tile of 16-row MFMA blocks can get wrong: 1, 15, 16, 17, 64, 65, 77, 300 and pxa_gemm_w8_max_m(); widths (N, K) = (128, 64) one k-step, (136, 80)
ragged in both (N: half a wave's 16 columns; K: 5 pieces of 16 in a chunk of 128), (384, 1040) = 8 chunks + 16, (1280, 1024), (1024, 1280), and one case per call
form at XXL widths with M = 300.  Each launch is held against the fp64 value of ITS operands: g = (x W1^T) * h0 against the fp64 product times the h0 the launch read (h0 itself against
gelu(x W0^T)), so every bound is the bound of one rounding; against gelu(x W0^T) * (x W1^T) g carries two (whole tensor 2.36e-3 = sqrt(2) x 1.66e-3 with bf16
operands, as pxa_gemm's), and at N = 128 the worst of 2048 rows of 128 such elements measured 4.6e-3 - a statement about 128 roundings, not about the kernel;
that figure is recorded, not bounded.  Scales are 2^-12 .. 2^2 per row, so a kernel that applies another row's scale is off by orders of magnitude.  Outputs are views
between GUARD rows and columns of a sentinel, h0 (the aux operand) and the A operands lie between NaN rows, the residual between -0.0 bands.  Every launch is
made twice and the two results compared bit for bit; every test asserts through gemm_w8_plan the instance (columns per wave, epilogue) and split = 1.

The file runs once more under the fp16-operand library in a child process (test_f16_build_runs_this_file).

Measured on an MI355X, bf16 build (every figure is also written by record_parity): 16-bit outputs whole tensor 1.64 - 1.67e-3 everywhere; XXL wqkv worst row
1.78e-3 / worst 64 x 64 block 1.93e-3, h0 1.83e-3 / 2.10e-3, g 1.77e-3 / 1.85e-3; the closest a bound comes is the worst of 2048 rows of 136 elements, h0
3.50e-3 (bound 4e-3).  Residual after two calls: 4e-8 (K = 80), 2.1e-7 (XXL wo), 3.8e-7 (XXL wff, 80 chunks), worst row 4.6e-7 (bound 2e-5).  Quantiser and
dequantiser bit-equal in both builds."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import t5_fp8_refs as R  # noqa: E402
from conftest import ROOT, record_parity, rel_l2  # noqa: E402
from test_kernels_gpu import BF16_TOL, _gpu_rnd, _opd, bf, ops  # noqa: E402,F401
from test_gemm_grad_forms_gpu import GUARD, MINUS_ZERO32, SENTINEL16, Banded, accumulate_twice  # noqa: E402
from test_t5_gemm_forms_gpu import check_16_blocks, nan16, operand  # noqa: E402

FP8 = torch.float8_e4m3fn
STORE, GELU, MUL_AUX, ADD_F32 = 0, 1, 2, 3
CUS = 256


# ------------------------------------------------------------------------------------------------ quantiser
def special_rows(K):
    """rows 0 .. 2 of every quantiser case: zeros; a maximum of exactly 448 * 2^-3; a row of scale 1 with exact ties between two codes (to the even one),
    values at and below half the smallest subnormal step 2^-9, and -0.0"""
    g = torch.Generator().manual_seed(7)
    r = torch.zeros(3, K)
    r[1] = torch.randn(K, generator=g) * 0.05
    r[1, 0] = 448 * 2.0 ** -3
    r[2, :12] = torch.tensor([448.0, 1.0625, 1.1875, -1.0625, 17.0, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -11, -2.0 ** -12, -0.0, 0.0, -27.0])
    return r


@pytest.mark.parametrize("src_f32", [False, True], ids=["operand", "fp32"])
@pytest.mark.parametrize("N,K", [(5, 80), (3, 4096), (130, 1040)])
def test_quantiser_is_the_torch_statement_bit_for_bit(ops, N, K, src_f32):
    dt = torch.float32 if src_f32 else _opd()
    g = torch.Generator().manual_seed(N + K)
    w = torch.randn(N, K, generator=g) * K ** -0.5 * torch.exp2(torch.randint(-6, 7, (N, 1), generator=g).float())
    w[:3] = special_rows(K)
    w = w.to(dt)
    ld, ldq, big = K + 16, K + 32, 6.0e4
    src = torch.full((N, ld), big, dtype=dt)                        # behind every row: values that would move the row's maximum if they were read
    src[:, :K] = w
    src = src.cuda()
    qbuf = torch.full((N + 2, ldq), 0xA5, dtype=torch.uint8, device="cuda")
    sbuf = torch.full((N + 8,), -7.0, device="cuda")
    q, s = ops.fp8_quant_rows(src[:, :K], q=qbuf[1:N + 1, :K].view(FP8), scale=sbuf[4:N + 4])
    torch.cuda.synchronize()
    want_q, want_s = R.quant_rows(w)
    assert torch.equal(sbuf[4:N + 4].cpu(), want_s), (sbuf[4:N + 4].cpu()[:8], want_s[:8])
    got = qbuf[1:N + 1, :K].cpu()
    bad = got != want_q.view(torch.uint8)
    assert not bad.any(), f"{int(bad.sum())} codes differ, first at {bad.nonzero()[0].tolist()}: {got[bad][:4].tolist()} vs {want_q.view(torch.uint8)[bad][:4].tolist()}"
    assert (qbuf[0] == 0xA5).all() and (qbuf[N + 1] == 0xA5).all() and (qbuf[1:N + 1, K:] == 0xA5).all(), "bytes outside q were written"
    assert (sbuf[:4] == -7).all() and (sbuf[N + 4:] == -7).all(), "scales outside [0, N) were written"
    assert want_s[0] == 1 and want_s[1] == 2.0 ** -3 and want_s[2] == 1 and not ((got & 0x7F) == 0x7F).any()
    assert got[2, :11].tolist() == [0x7E, 0x38, 0x3A, 0xB8, 0x58, 0x00, 0x02, 0x00, 0x80, 0x80, 0x00]         # ties to the even code; tiny values to a signed zero
    q2, s2 = ops.fp8_quant_rows(src[:, :K])                          # allocated outputs, again: the same bits
    assert torch.equal(q2.view(torch.uint8), qbuf[1:N + 1, :K]) and torch.equal(s2, sbuf[4:N + 4])


# ------------------------------------------------------------------------------------------------ dequantiser
def test_dequantiser_on_every_code_is_the_torch_statement_bit_for_bit(ops):
    codes = torch.arange(256, dtype=torch.uint8)
    codes[(codes & 0x7F) == 0x7F] = 0                               # the 254 codes that are numbers
    assert len(set(codes.tolist())) == 254
    scales = torch.tensor([2.0 ** -10, 1.0, 2.0 ** 3, 0.37])        # 0.37: scale * q is rounded to the operand type
    N, K, ldq, ld = 8, 256, 272, 264
    q = torch.stack([codes, codes.flip(0)] * 4)
    s = scales.repeat_interleave(2)
    qbuf = torch.full((N, ldq), 0x7F, dtype=torch.uint8)            # NaN codes behind every row
    qbuf[:, :K] = q
    qbuf = qbuf.cuda()
    out = Banded(N, ld, _opd(), SENTINEL16, guard=4)
    got = ops.fp8_dequant_rows(qbuf[:, :K].view(FP8), s.cuda(), out=out.view[:, :K])
    torch.cuda.synchronize()
    want = (q.view(FP8).float() * s[:, None]).to(_opd())
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))
    out.assert_intact("dequant rows")
    assert (out.view[:, K:].view(torch.int16) == SENTINEL16).all(), "elements behind column K were written"
    exact = (want[:6].double() == (q.view(FP8).double() * s[:, None].double())[:6])
    assert exact.all() or _opd() == torch.float16                   # power-of-two scales: no rounding (fp16: below its normal range it rounds)
    alloc = ops.fp8_dequant_rows(qbuf[:, :K].view(FP8), s.cuda())
    assert torch.equal(alloc, got)


# ------------------------------------------------------------------------------------------------ the GEMM
def weight(N, K, seed, mirror=None):
    """(q, scale, fp64 scale * q, e): codes of N(0, 16^2) values, scale[n] = 2^e[n] / (16 * 2^round(log2 sqrt K)), e uniform in -12 .. 2.
    mirror: the e of another matrix; this one takes -10 - e (the same range), so the elementwise product of the two outputs has columns of one magnitude."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = (torch.randn(N, K, device="cuda", generator=g) * 16).clamp(-448, 448).to(FP8)
    e = torch.randint(-12, 3, (N,), device="cuda", generator=g).float()
    if mirror is not None:
        e = -10 - mirror
    assert e.min() >= -12 and e.max() <= 2
    s = torch.exp2(e - 4 - round(0.5 * torch.log2(torch.tensor(float(K))).item()))
    return q, s, q.double() * s.double()[:, None], e


def expect_plan(ops, epi, a, q, s, **kw):
    M, N = a.shape[0], q.shape[0]
    nb = 2 if ((N + 127) // 128) * ((M + 63) // 64) >= CUS else 1
    p = ops.gemm_w8_plan(a, q, s, **kw).split()
    assert p[0] == f"gemm_w8_kernel<{nb},{epi}>" and "split=1" in p and f"m_tiles={(M + 63) // 64}" in p and f"n_tiles={(N + 64 * nb - 1) // (64 * nb)}" in p, p
    return nb


def twice(fn, out):
    """the launch again on the same inputs: bit-equal"""
    first = out.clone()
    fn()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16 if out.element_size() == 2 else torch.int32), first.view(torch.int16 if out.element_size() == 2 else torch.int32))


def run_store(ops, label, M, N, K):
    a = operand(M, K, 1)
    q, s, w64, _ = weight(N, K, 2)
    out = Banded(M, N, _opd(), SENTINEL16, col_bands=True)
    out.view.fill_(float("nan"))
    nb = expect_plan(ops, STORE, a, q, s, out=out.view)
    launch = lambda: ops.gemm_w8(a, q, s, out=out.view)              # noqa: E731
    assert launch().data_ptr() == out.view.data_ptr()
    torch.cuda.synchronize()
    out.assert_intact(label)
    check_16_blocks(label, out.view, a.double() @ w64.t())
    twice(launch, out.view)
    return nb


def run_chain(ops, label, M, N, K):
    """h0 = gelu(x W0^T) between NaN rows, then g = (x W1^T) * h0 with h0 as the aux operand.  W1's exponents mirror W0's: each launch sees scales over
    2^-12 .. 2^2, and g's columns have one magnitude - a row of g whose norm sat in the two or three columns where both scales are large would measure the
    rounding of those few elements (up to 2^-9 each, twice), not the kernel."""
    a = operand(M, K, 1)
    q0, s0, w0, e0 = weight(N, K, 2)
    q1, s1, w1, _ = weight(N, K, 3, mirror=e0)
    h0, g = Banded(M, N, _opd(), nan16()), Banded(M, N, _opd(), SENTINEL16, col_bands=True)
    h0.view.fill_(float("nan"))
    g.view.fill_(float("nan"))
    call0, call1 = dict(act=ops.ACT_GELU, out=h0.view), dict(act=ops.ACT_MUL_AUX, aux=h0.view, out=g.view)
    expect_plan(ops, GELU, a, q0, s0, **call0)
    expect_plan(ops, MUL_AUX, a, q1, s1, **call1)
    ops.gemm_w8(a, q0, s0, **call0)
    ops.gemm_w8(a, q1, s1, **call1)
    torch.cuda.synchronize()
    h0.assert_intact(f"{label} h0")
    g.assert_intact(f"{label} g")
    want = F.gelu(a.double() @ w0.t(), approximate="tanh")
    check_16_blocks(f"{label} h0 = gelu(x W0^T)", h0.view, want)
    x1 = a.double() @ w1.t()
    check_16_blocks(f"{label} g = (x W1^T) * h0", g.view, x1 * h0.view.double())          # the launch against ITS operands: the h0 it read, in fp64
    record_parity(f"{label} g vs gelu(x W0^T) * (x W1^T), whole tensor (h0's rounding and its own; not bounded)", rel_l2(g.view, want * x1))
    twice(lambda: ops.gemm_w8(a, q0, s0, **call0), h0.view)
    twice(lambda: ops.gemm_w8(a, q1, s1, **call1), g.view)


class _AsGemm:
    """accumulate_twice calls ops.gemm(a, b, layout, out_f32=, accumulate=True, split_k=): here b is (q, scale) and the call is gemm_w8"""

    def __init__(self, ops):
        self.ops = ops

    def gemm(self, a, b, layout, out_f32=None, accumulate=True, split_k=1):
        assert accumulate and split_k == 1
        return self.ops.gemm_w8(a, b[0], b[1], out_f32=out_f32)


def run_residual(ops, label, M, N, K, col_bands=False):
    a = operand(M, K, 1)
    q, s, w64, _ = weight(N, K, 2)
    x = Banded(M, N, torch.float32, MINUS_ZERO32, col_bands=col_bands)
    expect_plan(ops, ADD_F32, a, q, s, out_f32=x.view)
    accumulate_twice(_AsGemm(ops), label, a, (q, s), None, x, a.double() @ w64.t(), split_k=1, poison=False)
    y = Banded(M, N, torch.float32, MINUS_ZERO32, col_bands=col_bands)           # the same two calls from the same start: the same bits
    y.view.copy_(_gpu_rnd(M, N, seed=9))
    for _ in range(2):
        ops.gemm_w8(a, q, s, out_f32=y.view)
    torch.cuda.synchronize()
    assert torch.equal(x.view.view(torch.int32), y.view.view(torch.int32))


@pytest.mark.parametrize("N,K", [(128, 64), (136, 80)])
@pytest.mark.parametrize("M", ["1", "15", "16", "17", "64", "65", "77", "300", "max_m"])
def test_every_row_count_on_the_small_widths(ops, M, N, K):
    """all four epilogues at every row count: one k-step (K = 64 of a 128 chunk), and N = 136 = two waves and a half, K = 80"""
    M = ops.gemm_w8_max_m() if M == "max_m" else int(M)
    assert ops.gemm_w8_max_m() >= 512
    label = f"w8 {M}x{N} K={K}"
    assert run_store(ops, label + " store", M, N, K) == 1
    run_chain(ops, label, M, N, K)
    run_residual(ops, label + " residual", M, N, K, col_bands=(N == 136))


@pytest.mark.parametrize("N,K", [(384, 1040), (1280, 1024), (1024, 1280)])
@pytest.mark.parametrize("M", [77, 300])
def test_middle_widths(ops, M, N, K):
    label = f"w8 {M}x{N} K={K}"
    run_store(ops, label + " store", M, N, K)
    run_chain(ops, label, M, N, K)
    run_residual(ops, label + " residual", M, N, K)


def test_xxl_wqkv(ops):
    """(300, 12288, 4096): 96 x 5 = 480 workgroups of 128 columns"""
    assert run_store(ops, "w8 xxl wqkv 300x12288 K=4096", 300, 12288, 4096) == 2


def test_xxl_wo(ops):
    """(300, 4096, 4096) into the residual: 32 x 5 < 256, so 64 columns per workgroup, 320 workgroups"""
    a = torch.empty(300, 4096, dtype=_opd())
    run_residual(ops, "w8 xxl wo 300x4096 K=4096", 300, 4096, 4096)
    assert ops.gemm_w8_plan(a, torch.empty(4096, 4096, dtype=torch.uint8).view(FP8), torch.ones(4096), out_f32=torch.empty(300, 4096)).split()[0] == "gemm_w8_kernel<1,3>"


def test_xxl_gated_gelu_chain(ops):
    """(300, 10240, 4096) twice: 80 x 5 = 400 workgroups of 128 columns, GELU then multiply by h0"""
    run_chain(ops, "w8 xxl wi 300x10240 K=4096", 300, 10240, 4096)


def test_xxl_wff(ops):
    """(300, 4096, 10240) into the residual: 80 chunks into one accumulator"""
    run_residual(ops, "w8 xxl wff 300x4096 K=10240", 300, 4096, 10240)


def test_refusals_come_before_any_launch(ops):
    from pixart_sigma_amd import lib
    a, (q, s, _, _) = operand(16, 64, 1), weight(128, 64, 2)
    with pytest.raises(lib.PixartHipError, match="rc=-1.*M="):
        ops.gemm_w8(torch.empty(ops.gemm_w8_max_m() + 1, 64, dtype=_opd(), device="cuda"), q, s)
    with pytest.raises(lib.PixartHipError, match="rc=-1.*16-byte"):
        ops.gemm_w8(a, q, torch.ones(132, device="cuda")[1:129])
    with pytest.raises(lib.PixartHipError, match="rc=-1.*K=72"):
        ops.gemm_w8(torch.empty(16, 72, dtype=_opd(), device="cuda"), torch.empty(128, 72, dtype=torch.uint8, device="cuda").view(FP8), s)


# ------------------------------------------------------------------------------------------------ the fp16-operand build
def test_f16_build_runs_this_file():
    """This file again, in a fresh process under the fp16-operand library, with BF16_TOL of that build; started after this process's work is done."""
    torch.cuda.synchronize()
    env = dict(os.environ, PXA_OPERAND_DTYPE="f16")
    env.pop("PXA_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-s", "-p", "no:cacheprovider", "-k", "not f16_build"],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    tail = "\n".join(ln for ln in r.stdout.splitlines() if ("passed" in ln or "failed" in ln or "FAILED" in ln or "Error" in ln))
    print("\n[f16 build] " + tail.replace("\n", "\n[f16 build] "))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert "skipped" not in tail and "passed" in tail, tail
