"""csrc/gemm_f8.hip at the sizes the engine launches and at the edges of its value range, in the process's operand build.  tests/test_gemm_f8_gpu.py
settles the lane and scale maps and the quantiser rule at up to 3 row tiles and 21,600 pieces; this file runs what those sizes never reach:

A.  pxa_gemm_f8 past the first group of 8 row tiles (the workgroup map's `r8 / n_tiles` term), in the instances that write the 16-bit result alone
    (<0,1,0>, <1,1,0>: five of the engine's six linears) - into sentinel-filled buffers, compared whole, so a tile left out or written from a wrong
    (mt, nt) shows.
B.  Every finite e4m3fn byte (subnormals, -0, +-448) through the MFMA with an exact expected sum, and E8M0 scale bytes far from 127.
C.  The second grid-stride pass of the quantiser and the dequantiser (more than 16384 * 256 pieces).
D.  The quantiser on rounding ties, on block maxima at the edges of the exponent rule (448 * 2^k and its neighbours, subnormals, 3e38), and on non-finite
    inputs, for the standalone kernel and the GEMM's fused MX epilogue.

Bounds: bit for bit against the host rule (tests/mx_fp8_refs.py) or the fp64 product rounded once, except random data and GELU, which take the bound of
test_gemm_random unchanged (one ulp of the operand type at |ref| + K 2^-23 sum |a||w|, times 1.13 under GELU).  Every buffer a kernel writes is a banded
view (test_gemm_f8_gpu.banded) and the bands are compared afterwards.  Every case prints what it measured before it asserts."""
import os
import sys
import time

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import mx_fp8_refs as R  # noqa: E402
from conftest import record_parity  # noqa: E402
from test_gemm_f8_gpu import (FP8, assert_all_bands, assert_bands, banded, exact_operands, operand_ulp, outputs, random_operands,  # noqa: E402
                              upload)

pytestmark = pytest.mark.gpu

ROW_GROUP_SHAPES = [(1025, 384, 256),      # 9 row tiles: the second group holds one live tile (one live row) and seven that return; odd n_tiles
                    (2049, 128, 128),      # 17 row tiles, three groups
                    (1152, 256, 128)]      # 9 full row tiles, no row tail


@pytest.fixture(scope="module")
def ops():
    from pixart_sigma_amd import ops as o
    return o


def u8(t):
    return t.cpu().view(torch.uint8)


def assert_same_values(got, want, what):
    """Every element equal (as numbers: a sum of -0 products is -0 in the reference and +0 from an accumulator that starts at +0)."""
    got, want = got.cpu().double(), want.double()
    bad = got != want
    print(f"{what}: {bad.sum().item()} of {bad.numel()} elements differ (bound: 0)")
    assert not bad.any(), f"{what}: {bad.sum().item()} of {bad.numel()} differ; first at {bad.nonzero()[0].tolist()}: {got[bad][0].item()} vs {want[bad][0].item()}"


def assert_no_nan_codes(q, e, what):
    assert not ((u8(q) & 0x7F) == 0x7F).any(), f"{what}: an e4m3fn NaN code (0x7F / 0xFF) was written"
    assert not (e.cpu() == 0xFF).any(), f"{what}: the E8M0 NaN code was written"


def random_bound(ops, ref, a64, w64, K, act):
    """test_gemm_random's bound."""
    return (operand_ulp(ops, ref) + K * 2.0 ** -23 * (a64.abs() @ w64.abs().t())) * (1.13 if act else 1.0)


def check_ratio(label, got, ref, bound):
    err = (got.cpu().double() - ref).abs()
    ratio = (err / bound).max().item()
    print(f"{label}: worst |err| / bound = {ratio:.3f}, worst |err| = {err.max().item():.3e}")
    record_parity(label + " err/bound", ratio, 1.0)
    assert ratio <= 1.0, (label, ratio)


def alone16(ops, A, W, M, N, what, instance, **kw):
    """gemm_f8 writing the 16-bit result only, into a sentinel-filled banded view; returns the view."""
    whole, o16 = banded(M, N, ops.BF16, pad=8)
    assert ops.gemm_f8_plan(*A, *W, out=o16, **kw).startswith(f"gemm_f8_kernel<{instance}> ")
    r = ops.gemm_f8(*A, *W, out=o16, **kw)
    torch.cuda.synchronize()
    assert r is o16
    assert_bands(whole, M, N, what)
    return o16


def assert_fused_is_quantiser(ops, o16, oq, oe, what):
    q2, e2 = ops.mx_quant_rows(o16)
    assert torch.equal(oe, e2) and torch.equal(oq.view(torch.uint8), q2.view(torch.uint8)), f"{what}: the fused MX output is not mx_quant_rows(out16)"


# ------------------------------------------------------------------------------------------------ A. row groups, the 16-bit-only instances
@pytest.mark.parametrize("M,N,K", ROW_GROUP_SHAPES)
def test_row_groups_exact_integers(ops, M, N, K):
    qa, ea = exact_operands(M, K, 7 * M + K)
    qw, ew = exact_operands(N, K, 11 * N + K + 1)
    a64, w64 = R.dequant(qa, ea), R.dequant(qw, ew)
    ref = a64 @ w64.t()
    assert (ref * 4 == torch.round(ref * 4)).all() and ref.abs().max() * 4 < 2 ** 24
    want = ref.to(ops.BF16)
    A, W = upload(qa, ea), upload(qw, ew)
    tag = f"row groups exact {M}x{N}x{K}"
    o16 = alone16(ops, A, W, M, N, tag + " <0,1,0>", "0,1,0")
    assert_same_values(o16, want, tag + " <0,1,0>")
    g16 = alone16(ops, A, W, M, N, tag + " <1,1,0>", "1,1,0", act=ops.ACT_GELU)
    ref_g = R.gelu_tanh64(ref)
    check_ratio(f"gemm_f8 {M}x{N}x{K} <1,1,0> exact operands", g16, ref_g, random_bound(ops, ref_g, a64, w64, K, 1))
    wholes, (p16, pq, pe) = outputs(ops, M, N)
    ops.gemm_f8(*A, *W, out=p16, out_q=pq, out_e=pe)
    torch.cuda.synchronize()
    assert_all_bands(wholes, M, N, tag + " <0,1,1>")
    assert_same_values(p16, want, tag + " <0,1,1>")
    assert torch.equal(p16.view(torch.int16), o16.view(torch.int16)), "<0,1,0> and the three-output form differ in out16"
    assert_fused_is_quantiser(ops, p16, pq, pe, tag)


def test_row_groups_random_with_bias(ops):
    """The engine's two forms (_lin_f8 with mx_out False / True) on random data: <0,1,0> against the bound; GELU against the bound from <1,1,0>, and <1,0,1>
    is that result through the quantiser, bit for bit."""
    M, N, K = ROW_GROUP_SHAPES[0]
    qa, ea = random_operands(M, K, 3 * M + K, 1.5)
    qw, ew = random_operands(N, K, 5 * N + K, 1.5)
    ew = (ew.int() + int(torch.log2(torch.tensor(1.0 / K ** 0.5)).round())).to(torch.uint8)      # pre-activations of order one
    bias = torch.randn(N, generator=torch.Generator().manual_seed(N + K))
    a64, w64 = R.dequant(qa, ea), R.dequant(qw, ew)
    pre = a64 @ w64.t() + bias.double()
    A, W, db = upload(qa, ea), upload(qw, ew), bias.cuda()
    o16 = alone16(ops, A, W, M, N, "random <0,1,0>", "0,1,0", bias=db)
    check_ratio(f"gemm_f8 {M}x{N}x{K} <0,1,0> bias", o16, pre, random_bound(ops, pre, a64, w64, K, 0))
    ref_g = R.gelu_tanh64(pre)
    g16 = alone16(ops, A, W, M, N, "random <1,1,0>", "1,1,0", bias=db, act=ops.ACT_GELU)
    check_ratio(f"gemm_f8 {M}x{N}x{K} <1,1,0> bias", g16, ref_g, random_bound(ops, ref_g, a64, w64, K, 1))
    wq, pq = banded(M, N, FP8)
    we, pe = banded(M, N // 32, torch.uint8, pad=4)
    assert ops.gemm_f8_plan(*A, *W, bias=db, act=ops.ACT_GELU, out_q=pq, out_e=pe, out16=False).startswith("gemm_f8_kernel<1,0,1> ")
    ops.gemm_f8(*A, *W, bias=db, act=ops.ACT_GELU, out_q=pq, out_e=pe, out16=False)
    torch.cuda.synchronize()
    assert_bands(wq, M, N, "random <1,0,1> out_q")
    assert_bands(we, M, N // 32, "random <1,0,1> out_e")
    assert_fused_is_quantiser(ops, g16, pq, pe, "random <1,0,1>")
    assert_no_nan_codes(pq, pe, "random <1,0,1>")


def test_gelu_without_bias(ops):
    M, N, K = 129, 128, 128
    qa, ea = random_operands(M, K, 3 * M + K + 1, 1.5)
    qw, ew = random_operands(N, K, 5 * N + K + 1, 1.5)
    ew = (ew.int() + int(torch.log2(torch.tensor(1.0 / K ** 0.5)).round())).to(torch.uint8)
    a64, w64 = R.dequant(qa, ea), R.dequant(qw, ew)
    ref = R.gelu_tanh64(a64 @ w64.t())
    bound = random_bound(ops, ref, a64, w64, K, 1)
    A, W = upload(qa, ea), upload(qw, ew)
    g16 = alone16(ops, A, W, M, N, "bias-less GELU <1,1,0>", "1,1,0", bias=None, act=ops.ACT_GELU)
    check_ratio(f"gemm_f8 {M}x{N}x{K} <1,1,0> no bias", g16, ref, bound)
    wholes, (p16, pq, pe) = outputs(ops, M, N)
    ops.gemm_f8(*A, *W, bias=None, act=ops.ACT_GELU, out=p16, out_q=pq, out_e=pe)
    torch.cuda.synchronize()
    assert_all_bands(wholes, M, N, "bias-less GELU <1,1,1>")
    check_ratio(f"gemm_f8 {M}x{N}x{K} <1,1,1> no bias", p16, ref, bound)
    # the two instances are compiled apart and may contract GELU's multiply-adds differently: fp16 build, a last bit in a few elements (bf16: none seen)
    print(f"    <1,1,0> and <1,1,1> differ in {(p16.view(torch.int16) != g16.view(torch.int16)).sum().item()} of {M * N} elements")
    assert_fused_is_quantiser(ops, p16, pq, pe, "bias-less GELU")


# ------------------------------------------------------------------------------------------------ B. every code; scales across the E8M0 range
def all_codes_rows(rows, seed):
    """(rows, 256) uint8: every row holds each of the 254 finite bytes once and two zeros, in an order of its own."""
    codes = torch.cat([R.finite_codes(), torch.zeros(2, dtype=torch.uint8)])
    order = torch.rand(rows, 256, generator=torch.Generator().manual_seed(seed)).argsort(dim=1)
    return codes[order]


def sparse_unit_rows(rows, seed):
    """(rows, 256) uint8 of 0, +1 (0x38), -1 (0xB8): four non-zeros per row, 128 rows cover every k twice.  No two of a row share a group of 8
    consecutive k, the unit inside which the instruction aligns products to the largest and drops what lies more than 13 binary places below its leading
    bit (measured; csrc/gemm_f8.hip's header): they sit two to a 128-deep step, in different 32-blocks and on different lanes.  Non-zero j of row n is
    k = 128 (j & 1) + 64 h + 16 g + r with r = n % 16, h = (n / 16) % 2, g = (j + n / 32) % 4."""
    assert rows % 128 == 0
    g = torch.Generator().manual_seed(seed)
    q = torch.zeros(rows, 256, dtype=torch.uint8)
    for n in range(rows):
        r, h, rot = n % 16, (n // 16) % 2, (n // 32) % 4
        ks = [128 * (j & 1) + 64 * h + 16 * ((j + rot) % 4) + r for j in range(4)]
        assert len({k // 8 for k in ks}) == 4 and len({k // 32 for k in ks}) == 4
        q[n, ks] = torch.where(torch.rand(4, generator=g) < 0.5, 0x38, 0xB8).to(torch.uint8)
    assert ((q != 0).sum(dim=1) == 4).all() and ((q != 0).sum(dim=0) == rows // 64).all()
    return q


@pytest.mark.parametrize("dense", ["A", "W"])
def test_every_finite_code_exact(ops, dense):
    """Every finite byte - subnormals, -0, +-448 - as an MFMA operand, against an exact sum: four terms per output, each a code times +-1 times
    2^(-1 .. 2); in units of the smallest term (2^-9 times the smallest scale product) the sum of magnitudes stays below 2^24, so an fp32 sum in any order
    is exact - and the four terms lie in four different groups of 8 k (sparse_unit_rows), because inside one group the instruction is NOT an fp32 sum: with
    two of the four terms on neighbouring k, 9 / 19 (bf16 build, codes in A / W) and 52 / 90 (fp16 build) of these outputs came out one 16-bit ulp away
    from the rounded exact sum, each of them what aligning a group's products to its largest and dropping bits 14 and further below reproduces."""
    M, N, K = (64, 128, 256) if dense == "A" else (128, 128, 256)
    g = torch.Generator().manual_seed(41 + (dense == "W"))
    if dense == "A":
        qa, qw = all_codes_rows(M, 5), sparse_unit_rows(N, 6)
    else:
        qa, qw = sparse_unit_rows(M, 7), all_codes_rows(N, 8)
    qa, qw = qa.view(FP8), qw.view(FP8)
    ea = torch.randint(126, 129, (M, K // 32), generator=g, dtype=torch.uint8)
    ew = torch.randint(127, 129, (N, K // 32), generator=g, dtype=torch.uint8)
    a64, w64 = R.dequant(qa, ea), R.dequant(qw, ew)
    unit = 2.0 ** -9 * 2.0 ** (int(ea.min()) + int(ew.min()) - 254)
    span = ((a64.abs() @ w64.abs().t()) / unit).max().item()
    print(f"all codes in {dense}: sum |a||w| / smallest term = {span:.0f} = 2^{torch.log2(torch.tensor(span)).item():.2f} (must be below 2^24)")
    assert span < 2 ** 24
    dense_q = (qa if dense == "A" else qw).view(torch.uint8)
    assert (torch.bincount(dense_q.flatten().long(), minlength=256)[R.finite_codes().long()] > 0).all() and not ((dense_q & 0x7F) == 0x7F).any()
    assert (R.code_values(dense_q) == dense_q.view(FP8).double()).all()
    ref = a64 @ w64.t()
    assert (ref / unit == torch.round(ref / unit)).all()
    want = ref.to(ops.BF16)
    A, W = upload(qa, ea), upload(qw, ew)
    o16 = alone16(ops, A, W, M, N, f"all codes in {dense}", "0,1,0")
    assert_same_values(o16, want, f"all codes in {dense}")
    if ops.BF16 == torch.bfloat16:                                                      # the 16-bit GEMM on exactly dequantised operands: the same exact sums
        g16 = ops.gemm(ops.mx_dequant_rows(*A), ops.mx_dequant_rows(*W), ops.NT)
        assert torch.equal(g16, o16), f"{(g16 != o16).sum().item()} elements differ from ops.gemm on the dequantised operands"


SCALE_SHIFTS = (-100, -60, -17, 0, 23, 64, 100)


def far_scale_operands(M, N, K, shifts, seed):
    """Exact-integer operands whose block scales are 2^(s[b] + da) for A and 2^(-s[b] + dw) for W: the shift cancels in every product."""
    g = torch.Generator().manual_seed(seed)
    qa, _ = exact_operands(M, K, seed + 1)
    qw, _ = exact_operands(N, K, seed + 2)
    nb = K // 32
    s = torch.tensor([shifts[i % len(shifts)] for i in torch.randperm(nb, generator=g).tolist()])
    ea = 127 + s[None, :] + torch.randint(-1, 2, (M, nb), generator=g)
    ew = 127 - s[None, :] + torch.randint(-1, 2, (N, nb), generator=g)
    assert 0 <= min(ea.min(), ew.min()) and max(ea.max(), ew.max()) <= 254
    return qa, ea.to(torch.uint8), qw, ew.to(torch.uint8), s


def test_scales_far_from_the_middle(ops):
    """Block scales 2^(+-100) that cancel between the operands: every product is an integer times 2^(-2 .. 2), the fp64 sum is exact, and the instruction has
    to apply two far-apart scale bytes exactly to reproduce it."""
    M, N, K = 129, 128, 256
    qa, ea, qw, ew, s = far_scale_operands(M, N, K, SCALE_SHIFTS, 77)
    assert set(s.tolist()) == set(SCALE_SHIFTS), "every shift of the set is used by a k-block"
    ref = R.matmul64(qa, ea, qw, ew)
    assert (ref * 4 == torch.round(ref * 4)).all() and ref.abs().max() * 16 < 2 ** 24
    A, W = upload(qa, ea), upload(qw, ew)
    o16 = alone16(ops, A, W, M, N, "far scales", "0,1,0")
    assert_same_values(o16, ref.to(ops.BF16), f"scale bytes {int(min(ea.min(), ew.min()))} .. {int(max(ea.max(), ew.max()))}")


# ------------------------------------------------------------------------------------------------ C. the second grid pass
BIG_R, BIG_K = 58300, 1152


@pytest.fixture(scope="module")
def big_source():
    """fp32 (58300, 1152) in the style of test_gemm_f8_gpu.quant_source: per-block magnitudes 1e-6 .. 1e4, a zero block and a block whose maximum is
    exactly 448 * 2^-3 in the rows of the second pass, within fp16's range.  Built once for both source types and never changed."""
    g = torch.Generator().manual_seed(58300)
    nb = BIG_K // 32
    mag = torch.exp(torch.empty(BIG_R, nb, 1).uniform_(-13.8, 9.2, generator=g))
    x = torch.randn(BIG_R, nb, 32, generator=g) * mag
    x[0, 0] = 0.0
    x[BIG_R - 20, 9] = 0.0
    x[BIG_R - 1, nb - 1] = x[BIG_R - 1, nb - 1].clamp(-1.0, 1.0)
    x[BIG_R - 1, nb - 1, 21] = -448.0 * 2.0 ** -3
    return x.reshape(BIG_R, BIG_K).clamp(-6e4, 6e4)


@pytest.mark.parametrize("f32", [False, True], ids=["src16", "src32"])
def test_quant_dequant_second_grid_pass(ops, big_source, f32):
    """The only large case.  pxa_mx_quant_rows and pxa_mx_dequant_rows launch at most 16384 blocks of 256 threads and stride on; a second pass exists only
    past 16384 * 256 = 4,194,304 16-element pieces.  At the engine's K = 1152 (72 pieces per row) 58,300 rows are the first multiple of 100 past that cap
    (58,255 rows cross it): the seam lies inside row 58,254 at column 256 and the second pass covers the last 46 rows.  Depth-28 weights (96,768 rows) take
    this path on every refresh.  Everything is compared against the host rule on all rows."""
    t0 = time.perf_counter()
    per_row = BIG_K // 16
    assert 16384 * 256 // per_row == 58254 == BIG_R - 46 and 16384 * 256 % per_row * 16 == 256
    dtype = torch.float32 if f32 else ops.BF16
    x = big_source.to(dtype)
    src = torch.zeros(BIG_R, BIG_K + 8, dtype=dtype, device="cuda")[:, :BIG_K]            # padded pitch
    src.copy_(x)
    wq, q = banded(BIG_R, BIG_K, FP8)
    we, e = banded(BIG_R, BIG_K // 32, torch.uint8, pad=5)
    ops.mx_quant_rows(src, q=q, e=e)
    torch.cuda.synchronize()
    q_ref, e_ref = R.quant_rows(x)
    assert e_ref[BIG_R - 1, -1] == 127 - 3 and e_ref[BIG_R - 20, 9] == 127 and (q_ref[BIG_R - 20, 9 * 32:10 * 32].float() == 0).all()
    e_bad, q_bad = e.cpu() != e_ref, u8(q) != q_ref.view(torch.uint8)
    rows_bad = (e_bad.any(dim=1) | q_bad.any(dim=1)).nonzero().flatten()
    print(f"quantiser, {BIG_R} x {BIG_K} from {dtype}: {e_bad.sum().item()} scale bytes and {q_bad.sum().item()} codes differ (bound: 0)"
          + (f"; rows {rows_bad[0].item()} .. {rows_bad[-1].item()}" if rows_bad.numel() else ""))
    assert not e_bad.any() and not q_bad.any()
    assert_bands(wq, BIG_R, BIG_K, "q")
    assert_bands(we, BIG_R, BIG_K // 32, "e")
    wd, d = banded(BIG_R, BIG_K, ops.BF16, pad=8)
    ops.mx_dequant_rows(q, e, out=d)
    torch.cuda.synchronize()
    want = R.dequant(q_ref, e_ref).to(ops.BF16)
    d_bad = d.cpu().float() != want.float()
    print(f"dequantiser: {d_bad.sum().item()} elements differ (bound: 0); wall time of the case {time.perf_counter() - t0:.2f} s")
    assert not d_bad.any()
    assert_bands(wd, BIG_R, BIG_K, "dequantised")


# ------------------------------------------------------------------------------------------------ D. ties, exponent edges, non-finite inputs
def device_source(x, dtype):
    src = torch.zeros(x.shape[0], x.shape[1] + 8, dtype=dtype, device="cuda")[:, :x.shape[1]]
    src.copy_(x.to(dtype))
    return src


def quantise_banded(ops, src):
    Rr, K = src.shape
    wq, q = banded(Rr, K, FP8)
    we, e = banded(Rr, K // 32, torch.uint8, pad=5)
    ops.mx_quant_rows(src, q=q, e=e)
    torch.cuda.synchronize()
    assert_bands(wq, Rr, K, "q")
    assert_bands(we, Rr, K // 32, "e")
    return q, e


def assert_dequant_matches(ops, q, e, q_ref, e_ref, what):
    Rr, K = q.shape
    wd, d = banded(Rr, K, ops.BF16, pad=8)
    ops.mx_dequant_rows(q, e, out=d)
    torch.cuda.synchronize()
    assert_bands(wd, Rr, K, what + " dequantised")
    assert_same_values(d, R.dequant(q_ref, e_ref).to(ops.BF16), what + " dequantised")


@pytest.mark.parametrize("f32", [False, True], ids=["src16", "src32"])
def test_quantiser_rounds_ties_to_even(ops, f32):
    """All 252 signed midpoints between adjacent codes, unscaled (the block holds 448) and with the block times 2^-9 and 2^6: the even code."""
    dtype = torch.float32 if f32 else ops.BF16
    x, q_want, e_want = R.tie_rows()
    assert (x.to(dtype).double() == x.double()).all()
    q, e = quantise_banded(ops, device_source(x, dtype))
    bad = u8(q) != q_want
    print(f"ties from {dtype}: {bad.sum().item()} of {3 * 252} midpoints miss the even code (bound: 0), {(e.cpu() != e_want).sum().item()} scale bytes differ")
    assert (e.cpu() == e_want).all()
    assert not bad.any(), f"first: {x[bad][0].item()} -> {u8(q)[bad][0].item():#x}, even code {q_want[bad][0].item():#x}"
    q_ref, e_ref = R.quant_rows(x.to(dtype))
    assert torch.equal(q_ref.view(torch.uint8), q_want) and torch.equal(e_ref, e_want)


@pytest.mark.parametrize("f32", [False, True], ids=["src16", "src32"])
def test_quantiser_exponent_edges(ops, f32):
    """Block maxima at 448 * 2^k and one ulp (of fp32, fp16, bf16) either side, 2^-126, fp32 / bf16 / fp16 subnormals and 3e38.  From the operand type: the
    rows whose maximum that type holds exactly, a subnormal of its own among them."""
    dtype = torch.float32 if f32 else ops.BF16
    x, X = R.exponent_edge_rows()
    amax = x.abs().amax(dim=1)
    keep = amax.to(dtype).double() == amax.double()                                    # the smaller elements of a kept row round to the type; amax does not move
    x, X, amax = x[keep].to(dtype).float(), X[keep], amax[keep]
    assert (x.abs().amax(dim=1) == amax).all()
    tiny = torch.finfo(ops.BF16).tiny
    assert keep.sum() >= 8 and ((amax > 0) & (amax < tiny)).any(), "a subnormal of the operand type is among the cases"
    assert not f32 or (keep.all() and (amax < 2.0 ** -126).sum() >= 4 and (X == 120).any())
    q, e = quantise_banded(ops, device_source(x, dtype))
    q_ref, e_ref = R.quant_rows(x.to(dtype))
    assert (e_ref.long() == X[:, None] + 127).all()
    e_bad, q_bad = e.cpu() != e_ref, u8(q) != q_ref.view(torch.uint8)
    print(f"exponent edges from {dtype}, {int(keep.sum())} cases: {e_bad.sum().item()} scale bytes and {q_bad.sum().item()} codes differ (bound: 0)"
          + (f"; first case amax = {amax[e_bad.any(dim=1) | q_bad.any(dim=1)][0].item():.9e}" if e_bad.any() or q_bad.any() else ""))
    assert not e_bad.any(), (e.cpu()[e_bad].tolist(), e_ref[e_bad].tolist())
    assert not q_bad.any()
    assert_dequant_matches(ops, q, e, q_ref, e_ref, "exponent edges")


def nonfinite_rows():
    """fp32 (4, 256) of ordinary values with +inf, -inf and NaN as single elements of separate blocks, both in one block, and a block that is all NaN."""
    g = torch.Generator().manual_seed(9)
    x = torch.randn(4, 8, 32, generator=g) * torch.exp(torch.empty(4, 8, 1).uniform_(-6.0, 6.0, generator=g))
    inf, nan = float("inf"), float("nan")
    x[0, 1, 3], x[0, 4, 17], x[0, 6, 0] = inf, -inf, nan
    x[1, 2, :] = nan
    x[1, 5, 2], x[1, 5, 30] = inf, nan
    x[2, 0, 31], x[2, 7, 16] = nan, -inf
    return x.reshape(4, 256)


@pytest.mark.parametrize("f32", [False, True], ids=["src16", "src32"])
def test_quantiser_nonfinite_inputs(ops, f32):
    """What the kernel's header promises for inputs the host rule does not define: no NaN code in q, no 0xFF in e, and every block without a non-finite
    element is untouched by its neighbours."""
    dtype = torch.float32 if f32 else ops.BF16
    x = nonfinite_rows().to(dtype)
    finite = torch.isfinite(x).reshape(4, 8, 32).all(dim=2)
    assert (~finite).sum() == 7 and finite[3].all()
    q, e = quantise_banded(ops, device_source(x, dtype))
    assert_no_nan_codes(q, e, "non-finite inputs")
    q_ref, e_ref = R.quant_rows(torch.where(torch.isfinite(x), x, torch.zeros_like(x)))
    same_q = (u8(q) == q_ref.view(torch.uint8)).reshape(4, 8, 32).all(dim=2)
    same_e = e.cpu() == e_ref
    print(f"non-finite inputs from {dtype}: {(finite & ~(same_q & same_e)).sum().item()} of {finite.sum().item()} finite blocks differ from the host rule (bound: 0); "
          f"bytes written for the non-finite blocks: e {e.cpu()[~finite].tolist()}")
    assert (same_q & same_e)[finite].all()


def test_fused_epilogue_overflowing_outputs(ops):
    """Exact sums of which a few exceed 65504: finite in the bf16 build, +-inf in the fp16 build.  The fused MX output is the quantiser's on out16 either
    way, with no NaN code, and blocks without an overflow follow the host rule."""
    M, N, K = 16, 128, 128
    qa, ea = exact_operands(M, K, 501)
    qw, ew = exact_operands(N, K, 502)
    ea[:], ew[:] = 127, 127 + 8
    ea[3], ea[9] = 127 + 2, 127 + 2
    ref = R.matmul64(qa, ea, qw, ew)
    over = ref.abs() > 65504
    print(f"fused epilogue: {over.sum().item()} of {M * N} outputs exceed 65504 ({(ref > 65504).sum().item()} positive, {(ref < -65504).sum().item()} negative); "
          f"largest {ref.abs().max().item():.0f}")
    assert (ref > 65504).any() and (ref < -65504).any() and over.sum() < M * N // 32 and over.any(dim=1).nonzero().flatten().tolist() == [3, 9]
    assert (ref / 256 == torch.round(ref / 256)).all() and ref.abs().max() / 256 < 2 ** 24
    want = ref.to(ops.BF16)
    assert torch.isinf(want).any() == (ops.BF16 == torch.float16)
    A, W = upload(qa, ea), upload(qw, ew)
    wholes, (o16, oq, oe) = outputs(ops, M, N)
    ops.gemm_f8(*A, *W, out=o16, out_q=oq, out_e=oe)
    torch.cuda.synchronize()
    assert_all_bands(wholes, M, N, "overflowing outputs")
    assert_same_values(o16, want, "overflowing outputs, out16")
    assert_fused_is_quantiser(ops, o16, oq, oe, "overflowing outputs")
    assert_no_nan_codes(oq, oe, "overflowing outputs")
    finite = torch.isfinite(want).reshape(M, N // 32, 32).all(dim=2)
    q_ref, e_ref = R.quant_rows(torch.where(torch.isfinite(want), want, torch.zeros_like(want)))
    same = (u8(oq) == q_ref.view(torch.uint8)).reshape(M, N // 32, 32).all(dim=2) & (oe.cpu() == e_ref)
    assert same[finite].all()
