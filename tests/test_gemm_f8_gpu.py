"""GPU checks of csrc/gemm_f8.hip in the process's operand build: the MX quantiser and dequantiser against the host rule (tests/mx_fp8_refs.py), and
pxa_gemm_f8 on exact-integer data (which settles the k order inside a lane and which row / k-block a lane's scale byte belongs to: per-block scales drawn
independently for both operands, asymmetric data) and on random data against the fp64 product of the dequantised operands.

Guard bands.  Every buffer a kernel writes is a view into a larger tensor: GUARD rows above and below and PAD columns behind every row start as a sentinel
byte pattern and are compared bit for bit afterwards (a whole stray 128-row tile on either side lands in a band).

Bounds.  Exact data: bit for bit.  Random data: one ulp of the operand type at |ref| plus K * 2^-23 * sum_k |a| |w| (an fp32 accumulation of exact
products in any order), times 1.13 under GELU (its largest slope).  Against ops.gemm on the dequantised operands (bf16 build): twice that, each side being
within it of the fp64 product.  Every case prints its worst error / bound before it asserts."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import mx_fp8_refs as R  # noqa: E402
from conftest import record_parity  # noqa: E402

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
GUARD, PAD = 136, 16
SENT = 0xA5
SHAPES = [(1, 128, 128), (16, 128, 256), (127, 384, 1152), (129, 128, 1152), (300, 256, 4608)]


@pytest.fixture(scope="module")
def ops():
    from pixart_sigma_amd import ops as o
    return o


def banded(rows, cols, dtype, pad=PAD):
    """(whole, view): whole is (GUARD + rows + GUARD, cols + pad) of sentinel bytes, view its middle rows and first cols."""
    whole = torch.full((2 * GUARD + rows, (cols + pad) * torch.empty(0, dtype=dtype).element_size()), SENT, dtype=torch.uint8, device="cuda").view(dtype)
    return whole, whole[GUARD:GUARD + rows, :cols]


def assert_bands(whole, rows, cols, what):
    b = whole.view(torch.uint8)
    es = whole.element_size()
    assert (b[:GUARD] == SENT).all() and (b[GUARD + rows:] == SENT).all(), f"{what}: a row outside the view was written"
    assert (b[GUARD:GUARD + rows, cols * es:] == SENT).all(), f"{what}: bytes behind column {cols} were written"


def operand_ulp(ops, ref):
    """One ulp of the operand type at |ref| (fp64 tensor)."""
    p, emin = (10, -14) if ops.BF16 == torch.float16 else (7, -126)
    ex = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin)))
    return torch.exp2(ex - p)


# ------------------------------------------------------------------------------------------------ quantiser / dequantiser
def quant_source(Rr, K, seed):
    g = torch.Generator().manual_seed(seed)
    nb = K // 32
    mag = torch.exp(torch.empty(Rr, nb, 1).uniform_(-13.8, 9.2, generator=g))          # 1e-6 .. 1e4 per block
    x = (torch.randn(Rr, nb, 32, generator=g) * mag)
    x[0, 0] = 0.0                                                                      # a zero block
    if Rr > 1:
        x[Rr // 2, nb // 2] = 0.0
    k = nb - 1
    x[Rr - 1, k] = x[Rr - 1, k].clamp(-1.0, 1.0)
    x[Rr - 1, k, 5] = -448.0 * 2.0 ** -3                                               # amax exactly 448 * 2^k
    return x.reshape(Rr, K).clamp(-6e4, 6e4)


@pytest.mark.parametrize("f32", [False, True], ids=["src16", "src32"])
@pytest.mark.parametrize("K", [32, 128, 1152])
@pytest.mark.parametrize("Rr", [1, 17, 300])
def test_quant_rows_against_host_rule(ops, Rr, K, f32):
    dtype = torch.float32 if f32 else ops.BF16
    x = quant_source(Rr, K, 100 * Rr + K).to(dtype)
    src = torch.zeros(Rr, K + 8, dtype=dtype, device="cuda")[:, :K]                    # padded pitch
    src.copy_(x)
    wq, q = banded(Rr, K, FP8)
    we, e = banded(Rr, K // 32, torch.uint8, pad=5)
    ops.mx_quant_rows(src, q=q, e=e)
    torch.cuda.synchronize()
    q_ref, e_ref = R.quant_rows(x)
    assert (e.cpu() == e_ref).all(), f"{(e.cpu() != e_ref).sum().item()} scale bytes differ"
    assert e_ref[Rr - 1, -1] == 127 - 3 and (Rr * K == 32 or e_ref[0, 0] == 127)        # the source holds what it says (one block: the 448 * 2^k one)
    assert (q.cpu().float() == q_ref.float()).all()
    assert not ((q.cpu().view(torch.uint8) & 0x7F) == 0x7F).any()
    assert_bands(wq, Rr, K, "q")
    assert_bands(we, Rr, K // 32, "e")
    # and back: the dequantiser is the exact inverse of the scaling
    wd, d = banded(Rr, K, ops.BF16, pad=8)
    ops.mx_dequant_rows(q, e, out=d)
    torch.cuda.synchronize()
    want = R.dequant(q_ref, e_ref).to(ops.BF16)
    if ops.BF16 == torch.bfloat16:
        assert (want.double() == R.dequant(q_ref, e_ref)).all(), "q * 2^(e - 127) is exact in bf16"
    assert (d.cpu().double() == want.double()).all()
    assert_bands(wd, Rr, K, "dequantised")


# ------------------------------------------------------------------------------------------------ GEMM
def upload(q, e):
    """Device copies with padded pitches (16 bytes for q, 4 for e)."""
    Rr, K = q.shape
    dq = torch.zeros(Rr, K + 16, dtype=torch.uint8, device="cuda").view(FP8)[:, :K]
    de = torch.zeros(Rr, K // 32 + 4, dtype=torch.uint8, device="cuda")[:, :K // 32]
    dq.view(torch.uint8).copy_(q.view(torch.uint8))
    de.copy_(e)
    return dq, de


def outputs(ops, M, N):
    w16, o16 = banded(M, N, ops.BF16, pad=8)
    wq, oq = banded(M, N, FP8)
    we, oe = banded(M, N // 32, torch.uint8, pad=4)
    return (w16, wq, we), (o16, oq, oe)


def assert_all_bands(wholes, M, N, what):
    assert_bands(wholes[0], M, N, what + " out16")
    assert_bands(wholes[1], M, N, what + " out_q")
    assert_bands(wholes[2], M, N // 32, what + " out_e")


def exact_operands(Rr, K, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-3, 4, (Rr, K), generator=g).float()
    e = torch.randint(126, 129, (Rr, K // 32), generator=g, dtype=torch.uint8)
    return v.to(FP8), e


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_exact_integers(ops, M, N, K):
    qa, ea = exact_operands(M, K, 7 * M + K)
    qw, ew = exact_operands(N, K, 11 * N + K + 1)
    ref = R.matmul64(qa, ea, qw, ew)
    assert (ref * 4 == torch.round(ref * 4)).all() and ref.abs().max() * 4 < 2 ** 24
    want = ref.to(ops.BF16)
    A, W = upload(qa, ea), upload(qw, ew)
    wholes, (o16, oq, oe) = outputs(ops, M, N)
    ops.gemm_f8(*A, *W, out=o16, out_q=oq, out_e=oe)
    torch.cuda.synchronize()
    got = o16.cpu()
    bad = (got.double() != want.double())
    assert not bad.any(), f"{bad.sum().item()} of {M * N} elements differ; first at {bad.nonzero()[0].tolist()}: {got[bad][0].item()} vs {want[bad][0].item()}"
    assert_all_bands(wholes, M, N, "exact")
    q2, e2 = ops.mx_quant_rows(o16)
    assert torch.equal(oe, e2) and torch.equal(oq.view(torch.uint8), q2.view(torch.uint8))
    # the same call again, into fresh buffers: the same bits
    _, (p16, pq, pe) = outputs(ops, M, N)
    ops.gemm_f8(*A, *W, out=p16, out_q=pq, out_e=pe)
    assert torch.equal(p16.view(torch.int16), o16.view(torch.int16))


def random_operands(Rr, K, seed, spread):
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp(torch.empty(Rr, K // 32, 1).uniform_(-spread, spread, generator=g))
    x = (torch.randn(Rr, K // 32, 32, generator=g) * mag).reshape(Rr, K)
    return R.quant_rows(x)


@pytest.mark.parametrize("act", [0, 1], ids=["none", "gelu"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_random(ops, M, N, K, act):
    qa, ea = random_operands(M, K, 3 * M + K + act, 1.5)
    qw, ew = random_operands(N, K, 5 * N + K + act, 1.5)
    w_scale = 1.0 / (K ** 0.5)                                                          # pre-activations of order one: GELU sees its curved part
    ew = (ew.int() + int(torch.log2(torch.tensor(w_scale)).round())).to(torch.uint8)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(N + K))
    a64, w64 = R.dequant(qa, ea), R.dequant(qw, ew)
    pre = a64 @ w64.t() + bias.double()
    ref = R.gelu_tanh64(pre) if act else pre
    bound = (operand_ulp(ops, ref) + K * 2.0 ** -23 * (a64.abs() @ w64.abs().t())) * (1.13 if act else 1.0)
    A, W = upload(qa, ea), upload(qw, ew)
    db = bias.cuda()
    wholes, (o16, oq, oe) = outputs(ops, M, N)
    ops.gemm_f8(*A, *W, bias=db, act=act, out=o16, out_q=oq, out_e=oe)
    torch.cuda.synchronize()
    got = o16.cpu().double()
    ratio = ((got - ref).abs() / bound).max().item()
    print(f"gemm_f8 random M={M} N={N} K={K} act={act}: worst |err| / bound = {ratio:.3f}, worst |err| = {(got - ref).abs().max().item():.3e}")
    record_parity(f"gemm_f8 {M}x{N}x{K} act{act} err/bound", ratio, 1.0)
    assert_all_bands(wholes, M, N, "random")
    assert ratio <= 1.0, ratio
    # the fused MX output is the quantiser's output on out16, bit for bit - also when it is the only output
    q2, e2 = ops.mx_quant_rows(o16)
    assert torch.equal(oe, e2) and torch.equal(oq.view(torch.uint8), q2.view(torch.uint8))
    wq, pq = banded(M, N, FP8)
    we, pe = banded(M, N // 32, torch.uint8, pad=4)
    ops.gemm_f8(*A, *W, bias=db, act=act, out_q=pq, out_e=pe, out16=False)
    torch.cuda.synchronize()
    assert torch.equal(pe, e2) and torch.equal(pq.view(torch.uint8), q2.view(torch.uint8))
    assert_bands(wq, M, N, "mx-only out_q")
    assert_bands(we, M, N // 32, "mx-only out_e")
    if ops.BF16 == torch.bfloat16:                                                      # oracle 2: the 16-bit GEMM on exactly dequantised operands
        g16 = ops.gemm(ops.mx_dequant_rows(*A), ops.mx_dequant_rows(*W), ops.NT, bias=db, act=act).cpu().double()
        r2 = ((got - g16).abs() / (2 * bound)).max().item()
        print(f"    against ops.gemm on the dequantised operands: worst |diff| / (2 bound) = {r2:.3f}")
        record_parity(f"gemm_f8 {M}x{N}x{K} act{act} vs gemm diff/(2 bound)", r2, 1.0)
        assert r2 <= 1.0, r2


def test_gemm_refusals_reach_python(ops):
    from pixart_sigma_amd import lib
    qa, ea = upload(*exact_operands(4, 128, 0))
    qw, ew = upload(*exact_operands(64, 128, 1))
    with pytest.raises(lib.PixartHipError, match="N=64 must be a positive multiple of 128"):
        ops.gemm_f8(qa, ea, qw, ew)
