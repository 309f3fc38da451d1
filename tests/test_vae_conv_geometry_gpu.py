"""The VAE's implicit-convolution GEMM (csrc/gemm.hip: gemm_pers_kernel<0, EPI, RM, SEG = true>) at the tile counts where its scheduler changes behaviour,
with guard bands around everything a kernel writes.

Reference of every kernel-level case: F.conv2d in fp64 on the CPU from the operand-rounded input and weights, so what is left is the fp32 accumulation
order plus ONE rounding to the operand type.  Bound: 2^-9 with bf16 operands, 2^-11 with fp16 operands (chosen from ops.BF16 at run time), from the
formats, not from a measurement: a value m * 2^e (1 <= m < 2) is stored with an error uniform in +-2^-p * 2^e, p = 8 (bf16) / 11 (fp16) significand
bits, so the rms relative error is 2^-p / sqrt(3) * sqrt(E[m^-2]); mantissas spread over [1, 2) give E[m^-2] = 1/2, i.e. 1.6e-3 / 2.0e-4 expected.
The bf16 bound is therefore 1.2 x the expected value of a correct kernel (a second rounding, sqrt(2) x, fails it), the fp16 bound 2.4 x.
Statistics are compared with fp64 sums of the STORED (rounded) interior output at the project's bounds (partial sums 1e-5, mean / rstd of
pxa_vae_gn_finalize 2e-5; 1e-4 behind the phase convolution, as its existing test), conv2d(interpolate(x)) keeps BF16_TOL, the model level MODEL_TOL
(bf16 operands) / F16_VAE_TOL (fp16 operands).

Guard bands.  Every buffer a kernel writes is a view into a larger tensor of the same allocation and the bands on both sides are compared bit for bit:
  out      GUARD_ROWS rows on each side, filled with the bit pattern SENTINEL;
  gn_part  one whole slot (B * N/2 floats) on each side of the 16 slots, filled with -0.0.  A stray `atomicAdd(+0.0f)` - what a wave beyond M adds - turns
           -0.0 into +0.0 under IEEE round-to-nearest, where any other sentinel would survive it; test_masked_statistics_adds_clear_the_sign_of_minus_zero
           is the in-bounds positive control that shows the GPU's atomic unit does so.  Without it the band assertions of gn_part prove nothing.
The paired statistics flavours (RM = 1, EPI 5 / 6) with an odd m-tile count run the second half of their last pair beyond M; with mt % 8 == 7 its second wave
row uses slot 15 and image index gn_B: the N/2 floats behind the buffer, i.e. the first floats of the upper band here.

Tile arithmetic (mt = ceil(M / 256), M = B * ip; `r`: ip = _img_rows(H, W), the product's layout; `u`: ip = (H+2)(W+2), partial last tile).  Every case
recomputes and asserts its mt, so a change of the tile size cannot silently move a case off its edge.  N = 128: paired items only; 384: full + paired;
256 / 512: full tiles only.  EPI: 0 plain, 4 + residual, 5 + statistics, 6 + residual + statistics; K tap-interleaved (k_tap = Cin) as the VAE uses it.

  geometry (B, H, W)   ip r / u      mt r / u   why
  (7, 14, 14)          256 / 256     7          one tile per image, odd batch, mt % 8 == 7
  (15, 14, 14)         256           15         likewise, two groups of 8 m-tiles
  (23, 14, 14)         256           23         likewise, three groups
  (1, 40, 40)          1792 / 1764   7 / 7      seven tiles in one image; u: partial last tile
  (3, 32, 32)          1280 / 1156   15 / 14    several tiles per image, mt % 8 == 7; u: even
  (5, 20, 31)          768 / 726     15 / 15    likewise with odd sizes; u: odd and partial
  (3, 20, 31)          768 / 726     9 / 9      mt odd, mt % 8 == 1: the stray add of the unguarded kernel stays inside the buffer
  (9, 14, 14)          256           9          likewise, one tile per image
  (8, 14, 14)          256           8          mt % 8 == 0
  (2, 30, 30)          1024          8          mt % 8 == 0, several tiles per image
  (4, 14, 14)          256           4          M = 1024: the smallest M of the persistent kernel
  (3, 14, 14)          256           3          M = 768: the two-stage kernel (EPI 0 / 4; statistics are refused: own test)
  (1, 1, 510)          1536          6          rp = 512: an image row straddles tiles
  (1, 510, 1)          1536          6          rp = 3: 85.3 image rows per tile
CASES below is the pruned cross of these with N in {128, 384, 256, 512}, Cin in {64, 128, 256} and the four epilogues (49 cases).  The phase convolution
(pxa_gemm_args.up_*) runs on low-res grids (3, 32, 32) [mt = 15], (1, 40, 40) [7] and (5, 20, 31) [15] with 128 and 256 channels."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from conftest import record_parity, rel_l2  # noqa: E402
from test_f16_parity_gpu import F16_VAE_TOL  # noqa: E402
from test_vae_gpu import BF16_TOL, MODEL_TOL, _pair, from_grid, ops, rnd, to_grid  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 256                # rows of an output tile of the persistent kernel
GUARD_ROWS = 512          # >= 256: a whole stray tile on either side of `out` lands in a band
SENTINEL = 0x5A5A         # 16-bit pattern of the output bands (bf16 1.5e16, fp16 203.25: no convolution result here)
STAT_SUM_TOL, STAT_FIN_TOL = 1e-5, 2e-5      # test_vae_gpu.py::test_conv_epilogue_groupnorm_statistics
PHASE_FIN_TOL = 1e-4                         # test_vae_gpu.py::test_upsample_conv_as_four_phase_convolutions (zero-mean output: E[x^2] - E[x]^2 is benign, the mean is small)


def unit_roundoff(ops):
    """The bound of a result that carries one rounding to the operand type, against an fp64 reference (file header)."""
    return 2.0 ** -11 if ops.BF16 == torch.float16 else 2.0 ** -9


def model_tol(ops):
    return F16_VAE_TOL if ops.BF16 == torch.float16 else MODEL_TOL


def conv_instance(M, N, epi):
    """The kernel instance pxa_gemm gives an implicit convolution of M rows and N channels with epilogue `epi` (file header; csrc/gemm.hip, choose_gemm): the
    persistent kernel from 1024 rows on, its remainder column (N % 256 == 128) as PAIRED items (RM 1) or, under PXA_GEMM_SEG_HALF, HALF items (RM 2); below
    1024 rows the two-stage 128 x 128 kernel, staged epilogue without a residual, direct with one.  Assumes no other dispatch knob is set
    (PXA_GEMM_NO_PERSISTENT would send every case to the two-stage kernel and fail these asserts, not the numbers)."""
    if M < 1024:
        return f"gemm_glds_kernel<0,128,128,2,2,{int(epi == 0)},true>"
    rm = 0 if N % 256 == 0 else 2 if os.environ.get("PXA_GEMM_SEG_HALF") else 1
    return f"gemm_pers_kernel<0,{epi},{rm},true>"


def img_rows(H, W):
    from pixart_sigma_amd.vae.autoencoder_kl import _img_rows
    return _img_rows(H, W)


def banded_rows(ops, rows, C):
    """(whole tensor, the middle `rows` rows as the view a kernel gets): every row starts as the sentinel."""
    whole = torch.full((rows + 2 * GUARD_ROWS, C), SENTINEL, dtype=torch.int16, device="cuda").view(ops.BF16)
    return whole, whole[GUARD_ROWS:GUARD_ROWS + rows]


def assert_row_bands_untouched(whole, what):
    bits = whole.view(torch.int16)
    assert (bits[:GUARD_ROWS] == SENTINEL).all(), f"{what}: a store in front of the output"
    assert (bits[-GUARD_ROWS:] == SENTINEL).all(), f"{what}: a store behind the output"


def banded_part(ops, B, N):
    """(flat tensor of 16 + 2 slots, the middle 16 as the (16, B, N/4, 2) view a kernel gets): bands -0.0, the 16 slots +0.0."""
    slot = B * N // 2
    flat = torch.zeros((ops.COLSUM_SLOTS + 2) * slot, dtype=torch.float32, device="cuda")
    flat[:slot] = -0.0
    flat[-slot:] = -0.0
    part = flat[slot:-slot].view(ops.COLSUM_SLOTS, B, N // 4, 2)
    assert part.is_contiguous() and part.data_ptr() == flat.data_ptr() + 4 * slot
    return flat, part


def assert_part_bands_untouched(flat, B, N, what):
    slot, bits = B * N // 2, flat.view(torch.int32)
    minus_zero = -(1 << 31)
    lo, hi = bits[:slot] != minus_zero, bits[-slot:] != minus_zero
    assert not lo.any(), f"{what}: {int(lo.sum())} floats in front of gn_part were written"
    assert not hi.any(), f"{what}: {int(hi.sum())} floats behind gn_part were written (first at +{int(hi.nonzero()[0])})"


def padded_input(ops, g, B, C, H, W, ip):
    """The zero-bordered copy an implicit convolution reads: [W+3 guard | B x ip pixel slots | W+3 guard]; returns (buffer, the (B*ip, 9C) A view)."""
    rp = W + 2
    buf = torch.zeros((B * ip + 2 * (W + 3)) * C, dtype=ops.BF16, device="cuda")
    ops.vae_gn_apply(g, ops.Grid(buf, B, H, W, C, rp, ip, origin=(W + 3) + rp + 1))
    return buf, buf.as_strided((B * ip, 9 * C), (C, 1))


def conv_ref64(x, w, bias):
    """fp64 CPU conv2d of the operand-rounded input and weights."""
    return F.conv2d(x.double().cpu(), w.double().cpu(), bias.double().cpu(), padding=1)


def check_statistics(ops, part, y, B, Co, H, W, label, fin_tol=STAT_FIN_TOL):
    """part (16, B, Co/4, 2) against fp64 sums of the stored interior output y (B, Co, H, W), and pxa_vae_gn_finalize against GroupNorm's mean / rstd."""
    y = y.cpu()
    yq = y.double().view(B, Co // 4, 4, H, W)
    sums = part.double().sum(0).cpu()
    e0, e1 = rel_l2(sums[..., 0], yq.sum((2, 3, 4))), rel_l2(sums[..., 1], (yq * yq).sum((2, 3, 4)))
    groups = 32
    mean, rstd = (t.cpu() for t in ops.vae_gn_finalize(part, B, Co, groups, H * W, 1e-6))
    yg = y.double().view(B, groups, -1)
    em, er = rel_l2(mean, yg.mean(-1).flatten()), rel_l2(rstd, (yg.var(-1, unbiased=False) + 1e-6).rsqrt().flatten())
    print(f"  {label}: sum {e0:.2e} sumsq {e1:.2e} (bound {STAT_SUM_TOL:.0e}); mean {em:.2e} rstd {er:.2e} (bound {fin_tol:.0e})")
    record_parity(f"{label} partial sums", max(e0, e1), STAT_SUM_TOL)
    record_parity(f"{label} finalize", max(em, er), fin_tol)
    assert e0 < STAT_SUM_TOL and e1 < STAT_SUM_TOL, (label, e0, e1)
    assert em < fin_tol and er < fin_tol, (label, em, er)


# (B, H, W, Cin, N, EPI, rounded ip, expected mt)
CASES = [
    # paired statistics flavours, mt % 8 == 7 (the stray add of an unguarded kernel leaves the buffer)
    (7, 14, 14, 64, 128, 5, True, 7), (7, 14, 14, 64, 128, 6, True, 7),
    (15, 14, 14, 128, 128, 5, True, 15), (15, 14, 14, 128, 128, 6, True, 15),
    (23, 14, 14, 64, 128, 5, True, 23), (23, 14, 14, 64, 128, 6, True, 23),
    (1, 40, 40, 256, 128, 5, True, 7), (1, 40, 40, 256, 128, 6, True, 7),
    (3, 32, 32, 128, 128, 5, True, 15), (3, 32, 32, 128, 128, 6, True, 15),
    (5, 20, 31, 64, 128, 5, True, 15), (5, 20, 31, 64, 128, 6, True, 15),
    (7, 14, 14, 128, 384, 5, True, 7), (7, 14, 14, 128, 384, 6, True, 7),
    (1, 40, 40, 64, 384, 5, True, 7), (1, 40, 40, 64, 384, 6, True, 7),
    (5, 20, 31, 128, 384, 5, True, 15), (5, 20, 31, 128, 384, 6, True, 15),
    # full tiles only at the same tile counts
    (1, 40, 40, 64, 256, 5, True, 7), (3, 32, 32, 64, 512, 6, True, 15),
    # mt odd with mt % 8 == 1, and mt % 8 == 0
    (3, 20, 31, 128, 128, 5, True, 9), (3, 20, 31, 128, 128, 6, True, 9), (9, 14, 14, 64, 128, 5, True, 9),
    (8, 14, 14, 64, 128, 5, True, 8), (2, 30, 30, 128, 384, 6, True, 8),
    # M = 1024: the smallest persistent launch
    (4, 14, 14, 128, 128, 5, True, 4), (4, 14, 14, 64, 128, 6, True, 4),
    # thin images
    (1, 1, 510, 64, 128, 5, True, 6), (1, 510, 1, 64, 128, 5, True, 6), (1, 1, 510, 128, 384, 6, True, 6), (1, 510, 1, 128, 384, 6, True, 6),
    # plain / residual, the product's rounded layout
    (7, 14, 14, 128, 128, 0, True, 7), (1, 40, 40, 128, 384, 4, True, 7), (3, 32, 32, 64, 128, 4, True, 15), (5, 20, 31, 256, 256, 0, True, 15),
    (4, 14, 14, 64, 128, 0, True, 4), (1, 1, 510, 64, 128, 4, True, 6), (1, 510, 1, 64, 384, 0, True, 6),
    # plain / residual, unrounded ip: M % 256 != 0, partial last tile
    (1, 40, 40, 128, 128, 0, False, 7), (1, 40, 40, 128, 128, 4, False, 7), (5, 20, 31, 64, 128, 4, False, 15), (5, 20, 31, 64, 384, 0, False, 15),
    (3, 20, 31, 256, 384, 4, False, 9), (1, 40, 40, 64, 512, 0, False, 7), (3, 32, 32, 128, 128, 0, False, 14),
    # M = 768 < 1024: the two-stage 128 x 128 kernel behind the same entry point
    (3, 14, 14, 64, 128, 0, True, 3), (3, 14, 14, 128, 128, 4, True, 3), (3, 14, 14, 64, 384, 4, True, 3), (3, 14, 14, 128, 256, 0, True, 3),
]


def case_id(c):
    B, H, W, C, N, epi, rounded, mt = c
    return f"B{B}_{H}x{W}_C{C}_N{N}_epi{epi}_{'r' if rounded else 'u'}_mt{mt}"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_implicit_conv_guarded(ops, case):
    """One implicit 3 x 3 convolution per case: output (interior pixels) against fp64 conv2d within one rounding, statistics against fp64 sums of the stored
    output, and nothing written outside `out` and `gn_part`."""
    B, H, W, C, Co, epi, rounded, want_mt = case
    stats, residual = epi in (5, 6), epi in (4, 6)
    rp = W + 2
    ip = img_rows(H, W) if rounded else (H + 2) * rp
    M = B * ip
    mt = (M + TILE - 1) // TILE
    assert mt == want_mt, f"the tile arithmetic of this case moved: M = {M}, mt = {mt}, expected {want_mt}"
    assert (M % TILE == 0) == (rounded or (H + 2) * rp % TILE == 0)
    assert not stats or (rounded and ip % TILE == 0 and ip >= (H + 2) * rp)
    g, x = to_grid(ops, rnd(B, C, H, W, seed=1))
    w = rnd(Co, C, 3, 3, scale=(9 * C) ** -0.5, seed=2).to(ops.BF16)
    bias = rnd(Co, seed=3) + 0.5                                       # non-zero mean: the variance must survive E[x^2] - E[x]^2
    _, a = padded_input(ops, g, B, C, H, W, ip)
    wk = w.permute(0, 2, 3, 1).reshape(Co, 3, 3, C // 64, 64).permute(0, 3, 1, 2, 4).reshape(Co, 9 * C).contiguous()
    res = (rnd(M, Co, seed=4) * 3.0).to(ops.BF16) if residual else None
    whole, out = banded_rows(ops, M, Co)
    flat, part = banded_part(ops, B, Co) if stats else (None, None)
    call = dict(bias=bias, out=out, k_seg=3 * C, a_seg_stride=rp * C, k_tap=C, act=ops.ACT_ADD_AUX if residual else ops.ACT_NONE, aux=res,
                gn_part=part, gn_geom=(ip, rp, H, W) if stats else None)
    assert ops.gemm_plan(a, wk, ops.NT, **call).split()[0] == conv_instance(M, Co, epi)
    got = ops.gemm(a, wk, ops.NT, **call)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    label = case_id(case)
    assert_row_bands_untouched(whole, label)
    if stats:
        assert_part_bands_untouched(flat, B, Co, label)
    y = from_grid(ops.Grid(out, B, H, W, Co, rp, ip, origin=W + 3))
    ref = conv_ref64(x, w, bias)
    if residual:
        ref = ref + from_grid(ops.Grid(res, B, H, W, Co, rp, ip, origin=W + 3)).double().cpu()
    e, u = rel_l2(y.cpu(), ref), unit_roundoff(ops)
    print(f"\n{label}: rel-L2 vs fp64 conv2d {e:.2e} (bound u = {u:.2e})")
    record_parity(f"{label} output vs fp64", e, u)
    assert e < u, (label, e, u)
    if stats:
        check_statistics(ops, part, y.cpu(), B, Co, H, W, label)


def test_masked_statistics_adds_clear_the_sign_of_minus_zero(ops):
    """Positive control of the -0.0 bands, in bounds by construction: one 6 x 6 image in a 1792-row slot (mt = 7, N = 128).  Tiles 1 ... 6 hold tail rows only,
    so slots 2 ... 13 of gn_part receive nothing but the masked sums, which are exactly +0.0f.  Pre-filled with -0.0 they must read +0.0 afterwards:
    (-0) + (+0) = +0 in round-to-nearest.  If this fails, the atomic unit keeps the sign and the gn_part band checks of this file cannot fire."""
    B, C, Co, H, W, ip = 1, 64, 128, 6, 6, 1792
    rp = W + 2
    assert ip % TILE == 0 and ip // TILE == 7 and (H + 2) * rp <= TILE, "tiles 1 ... 6 must hold no image row"
    g, x = to_grid(ops, rnd(B, C, H, W, seed=1))
    w = rnd(Co, C, 3, 3, scale=(9 * C) ** -0.5, seed=2).to(ops.BF16)
    bias = rnd(Co, seed=3) + 0.5
    _, a = padded_input(ops, g, B, C, H, W, ip)
    wk = w.permute(0, 2, 3, 1).reshape(Co, 3, 3, C // 64, 64).permute(0, 3, 1, 2, 4).reshape(Co, 9 * C).contiguous()
    whole, out = banded_rows(ops, B * ip, Co)
    flat, part = banded_part(ops, B, Co)
    part[2:14] = -0.0
    assert (part[2:14].view(torch.int32) == -(1 << 31)).all()
    call = dict(bias=bias, out=out, k_seg=3 * C, a_seg_stride=rp * C, k_tap=C, gn_part=part, gn_geom=(ip, rp, H, W))
    assert ops.gemm_plan(a, wk, ops.NT, **call).split()[0] == conv_instance(B * ip, Co, 5)
    ops.gemm(a, wk, ops.NT, **call)
    torch.cuda.synchronize()
    bits = part.view(torch.int32)
    kept = int((bits[2:14] == -(1 << 31)).sum())
    print(f"\npositive control: {kept} of {bits[2:14].numel()} pre-filled -0.0 kept their sign after the masked +0.0 adds")
    assert (bits[2:14] == 0).all(), f"{kept} floats of slots 2 ... 13 are not +0.0: the -0.0 bands cannot detect a stray add of +0.0"
    assert (bits[14:] == 0).all()                                      # slots 14 / 15 belong to the half of the last pair beyond M: never touched
    assert_row_bands_untouched(whole, "control")
    assert_part_bands_untouched(flat, B, Co, "control")
    y = from_grid(ops.Grid(out, B, H, W, Co, rp, ip, origin=W + 3))
    e, u = rel_l2(y.cpu(), conv_ref64(x, w, bias)), unit_roundoff(ops)
    assert e < u, (e, u)
    check_statistics(ops, part, y.cpu(), B, Co, H, W, "control B1 6x6 in 1792 rows")


def test_statistics_below_1024_rows_are_refused(ops):
    """M = 768 takes the two-stage kernel, which has no statistics epilogue: pxa_gemm must refuse gn_part there (no silent fall-back), with the documented text."""
    from pixart_sigma_amd.lib import PixartHipError
    B, C, Co, H, W = 3, 64, 128, 14, 14
    rp, ip = W + 2, img_rows(H, W)
    assert B * ip == 768 < 1024 and (B + 1) * ip == 1024
    g, _ = to_grid(ops, rnd(B, C, H, W, seed=1))
    _, a = padded_input(ops, g, B, C, H, W, ip)
    wk = rnd(Co, 9 * C, scale=(9 * C) ** -0.5, seed=2).to(ops.BF16)
    whole, out = banded_rows(ops, B * ip, Co)
    flat, part = banded_part(ops, B, Co)
    with pytest.raises(PixartHipError, match="gn_part needs the persistent implicit-convolution path"):
        ops.gemm(a, wk, ops.NT, out=out, k_seg=3 * C, a_seg_stride=rp * C, k_tap=C, gn_part=part, gn_geom=(ip, rp, H, W))
    with pytest.raises(PixartHipError, match="gn_part needs the persistent implicit-convolution path"):      # the plan of the same call is refused alike
        ops.gemm_plan(a, wk, ops.NT, out=out, k_seg=3 * C, a_seg_stride=rp * C, k_tap=C, gn_part=part, gn_geom=(ip, rp, H, W))
    torch.cuda.synchronize()
    assert (whole.view(torch.int16) == SENTINEL).all() and (part == 0).all()
    assert_part_bands_untouched(flat, B, Co, "refused")


@pytest.mark.parametrize("B,H,W,Co,want_mt", [(3, 32, 32, 128, 15), (3, 32, 32, 256, 15), (1, 40, 40, 128, 7), (1, 40, 40, 256, 7), (5, 20, 31, 128, 15)])
def test_phase_convolution_scatter_guarded(ops, B, H, W, Co, want_mt):
    """Upsample2D as four phase launches (ops.gemm(..., up=...), called as AutoencoderKL._conv3_up2 does) into a sentinel-filled high-res buffer: every row that is
    not an interior pixel (border rows and columns, each image's tail, the bands) is still the sentinel afterwards and every interior row is not; interior
    against the fp64 2 x 2 convolutions of the PACKED phase weights within one rounding, against conv2d(interpolate(x)) of the module's weights within BF16_TOL
    (the packed taps carry their own rounding); the statistics summed over the four launches against the stored output."""
    from pixart_sigma_amd.vae import AutoencoderKL
    torch.manual_seed(3)
    vae = AutoencoderKL(block_out_channels=(128, Co), layers_per_block=1).cuda()
    vae._prepare()
    conv = vae.decoder.up_blocks[0].upsamplers[0].conv
    C = conv.in_channels
    assert (C, conv.out_channels) == (Co, Co)
    phases, bias = vae._packed[("up", id(conv))]
    ipL, rpL = img_rows(H, W), W + 2
    assert B * ipL // TILE == want_mt and want_mt % 2 == 1 and B * ipL >= 1024
    H2, W2 = 2 * H, 2 * W
    ipH, rpH = img_rows(H2, W2), W2 + 2
    g, x = to_grid(ops, rnd(B, C, H, W, seed=1))
    buf = torch.zeros((B * ipL + 2 * (W + 3)) * C, dtype=ops.BF16, device="cuda")
    ops.vae_gn_apply(g, ops.Grid(buf, B, H, W, C, rpL, ipL, origin=(W + 3) + rpL + 1))
    whole, out = banded_rows(ops, B * ipH, Co)
    flat, part = banded_part(ops, B, Co)
    for i, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        off = (W + 3) + (dy - 1) * rpL + dx - 1
        a = buf.as_strided((B * ipL, 4 * C), (C, 1), off * C)
        call = dict(bias=bias, out=out, k_seg=2 * C, a_seg_stride=rpL * C, gn_part=part, gn_geom=(ipL, rpL, H, W), up=(rpH, ipH, dy, dx))
        assert ops.gemm_plan(a, phases[i], ops.NT, **call).split()[0] == conv_instance(B * ipL, Co, 5)
        ops.gemm(a, phases[i], ops.NT, **call)
    torch.cuda.synchronize()
    label = f"phase conv B{B} {H}x{W} C{Co} mt{want_mt}"
    assert_row_bands_untouched(whole, label)
    assert_part_bands_untouched(flat, B, Co, label)
    # which rows of the high-res padded grid are interior pixels
    slot = torch.arange(ipH, device="cuda")
    py, px = slot // rpH, slot % rpH
    interior = ((py >= 1) & (py <= H2) & (px >= 1) & (px <= W2)).repeat(B)
    assert int(interior.sum()) == B * H2 * W2
    is_sentinel = (out.view(torch.int16) == SENTINEL).all(1)
    leaked = (~is_sentinel & ~interior).nonzero().flatten()
    assert leaked.numel() == 0, f"{label}: {leaked.numel()} non-interior rows were written, first: row {int(leaked[0]) % ipH} of image {int(leaked[0]) // ipH} (row pitch {rpH})"
    missing = (is_sentinel & interior).nonzero().flatten()
    assert missing.numel() == 0, f"{label}: {missing.numel()} interior rows were never written"
    y = from_grid(ops.Grid(out, B, H2, W2, Co, rpH, ipH, origin=W2 + 3)).cpu()
    # fp64 reference from the packed phase weights: phase (dy, dx) is a 2 x 2 convolution of the zero-bordered input
    xp = F.pad(x.double().cpu(), (1, 1, 1, 1))
    ref = torch.empty(B, Co, H2, W2, dtype=torch.float64)
    for i, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        wp = phases[i].double().cpu().view(Co, 2, 2, C).permute(0, 3, 1, 2)
        ref[:, :, dy::2, dx::2] = F.conv2d(xp, wp, bias.double().cpu())[:, :, dy:dy + H, dx:dx + W]
    e, u = rel_l2(y, ref), unit_roundoff(ops)
    ref3 = F.conv2d(F.interpolate(x.double().cpu(), scale_factor=2.0, mode="nearest"), conv.weight.double().cpu(), conv.bias.double().cpu(), padding=1)
    e3 = rel_l2(y, ref3)
    print(f"\n{label}: rel-L2 vs fp64 phase convolutions {e:.2e} (bound u = {u:.2e}); vs conv2d(interpolate(x)) {e3:.2e} (bound {BF16_TOL:.0e})")
    record_parity(f"{label} vs fp64 phases", e, u)
    record_parity(f"{label} vs conv2d(interpolate)", e3, BF16_TOL)
    assert e < u, (label, e, u)
    assert e3 < BF16_TOL, (label, e3)
    check_statistics(ops, part, y, B, Co, H2, W2, label, fin_tol=PHASE_FIN_TOL)


def assert_pad_cache_clean(vae):
    """The _padded contract: border, per-image tail and both W + 3 guards of every cached zero-bordered input are still all-zero bits."""
    assert vae._pad_cache, "the decode went through no implicit convolution"
    for (B, H, W, C, _), buf in vae._pad_cache.items():
        ip, rp, guard = img_rows(H, W), W + 2, W + 3
        pix = buf.view(torch.int16).view(-1, C)
        assert pix.shape[0] == B * ip + 2 * guard
        slot = torch.arange(ip, device=buf.device)
        py, px = slot // rp, slot % rp
        interior = ((py >= 1) & (py <= H) & (px >= 1) & (px <= W)).repeat(B)
        keep_zero = torch.cat([torch.ones(guard, dtype=torch.bool, device=buf.device), ~interior, torch.ones(guard, dtype=torch.bool, device=buf.device)])
        dirty = (pix != 0).any(1) & keep_zero
        assert not dirty.any(), f"_pad_cache[{(B, H, W, C)}]: {int(dirty.sum())} border / tail / guard pixels are not zero, first at pixel {int(dirty.nonzero()[0])}"


@pytest.mark.parametrize("B,H,W,want_mt", [(7, 16, 12, 7), (3, 32, 32, 15)])
def test_two_level_decode_odd_batch(ops, B, H, W, want_mt):
    """Decode of the two-level configuration at an odd batch whose 128-channel block (at the image's resolution) runs mt % 8 == 7 paired statistics launches,
    against oracle/vae_ref.py (fp32, CPU); afterwards every cached zero-bordered input still has its zero border, tail and guards.  One 256-row tile per image
    at B = 7 is a 16 x 12 image here (18 x 14 = 252 padded pixels), not 14 x 14: the mid-block attention needs a latent H * W that is a multiple of 8."""
    mt = B * img_rows(H, W) // TILE
    assert mt == want_mt and mt % 8 == 7 and B * img_rows(H // 2, W // 2) >= 1024 and (H // 2) * (W // 2) % 8 == 0
    cfg = dict(block_out_channels=(128, 256), layers_per_block=1)
    ref, vae = _pair(cfg, seed=5)
    z = rnd(B, 4, H // 2, W // 2, seed=6).cpu()
    with torch.no_grad():
        want = ref.decode(z)
    got = vae.decode(z.cuda()).sample
    torch.cuda.synchronize()
    assert got.shape == want.shape == (B, 3, H, W)
    e = rel_l2(got.cpu(), want)
    print(f"\ntwo-level decode B{B} {H}x{W} (mt = {mt}): rel-L2 vs the fp32 restatement {e:.2e} (bound {model_tol(ops):.1e})")
    record_parity(f"two-level decode B{B} {H}x{W}", e, model_tol(ops))
    assert e < model_tol(ops)
    assert_pad_cache_clean(vae)


def test_full_architecture_decode_256px_batch3(ops):
    """Full SD / SDXL decoder, latent (3, 4, 32, 32) -> (3, 3, 256, 256): the 128-channel level runs 3 x 261 = 783 m-tiles (783 % 8 == 7) through the paired
    statistics flavours.  fp32 restatement on the GPU, as test_vae_gpu.py::test_full_architecture_decode_512px_batch2."""
    mt = 3 * img_rows(256, 256) // TILE
    assert mt == 783 and mt % 8 == 7
    ref, vae = _pair(dict(), seed=5)
    z = rnd(3, 4, 32, 32, seed=6)
    with torch.no_grad():
        want = ref.cuda().decode(z)
    got = vae.decode(z).sample
    torch.cuda.synchronize()
    e = rel_l2(got, want)
    print(f"\n256px batch-3 decode rel-L2 vs fp32 restatement {e:.2e} (bound {model_tol(ops):.1e})")
    record_parity("full architecture decode 256px B3", e, model_tol(ops))
    assert got.shape == (3, 3, 256, 256) and e < model_tol(ops)
    assert_pad_cache_clean(vae)


def test_half_item_instances_statistics_subset():
    """PXA_GEMM_SEG_HALF=1 (read once per process) selects the round-5 HALF remainder items (gemm_pers_kernel<0, EPI, 2, true>), still compiled as the A/B partner
    of the paired ones: the statistics and residual cases of this file once more through them, in a fresh child."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    env = dict(os.environ, PXA_GEMM_SEG_HALF="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-s", "-p", "no:cacheprovider",
                        "-k", "test_implicit_conv_guarded and (epi4 or epi5 or epi6) or test_phase_convolution_scatter_guarded or test_masked_statistics"],
                       capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    tail = "\n".join(l for l in r.stdout.splitlines() if ("passed" in l or "failed" in l or "FAILED" in l or "Error" in l))
    print("\n[HALF items] " + tail.replace("\n", "\n[HALF items] "))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert " passed" in tail and "skipped" not in tail and "deselected" in tail, tail
