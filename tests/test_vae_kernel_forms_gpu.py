"""The VAE kernels outside the convolution GEMM (csrc/vae.hip: pxa_vae_gn_stats, _gn_finalize, _gn_apply, _im2col3x3, _conv3x3_small_out, _add,
_softmax_rows, _nchw_to_grid, _grid_to_nchw) in the forms vae/autoencoder_kl.py calls them, at the sizes where their launch arithmetic changes.

Harness.  A grid a kernel reads or writes is a view inside a larger allocation (Banded: max(4 (W + 2) + 3, 64) pixels of band on each side) in one of the layouts
  compact    rp = W, ip = H * W, origin 0
  padded     rp = W + 2, ip = _img_rows(H, W), origin W + 3: the output of an implicit convolution (border and tail rows hold what the GEMM left there)
  padded_g   the same pitches inside the W + 3 guard _padded allocates, origin (W + 3) + rp + 1: the INPUT of an implicit convolution, as _conv3 builds it
  padded_u   rp = W + 2, ip = (H + 2) * (W + 2) (not rounded to the GEMM tile), origin W + 3: the header's padded-grid view
An input grid holds NaN in every pixel slot that is not an interior pixel (border, image tails, bands): a kernel that reads one of them gives a NaN, and
every comparison below fails on a NaN.  An output grid holds the 16-bit SENTINEL of test_vae_conv_geometry_gpu.py there - or zeros inside the slots, as
_padded makes them, where the test stands for a cached convolution input - and is compared bit for bit afterwards.  fp32 outputs (img, mean, rstd, the
NCHW image, col as 16-bit rows) sit between sentinel bands of 64 floats.  Every comparison is taken per (sample, image row) - per matrix row for
softmax_rows and im2col, per (sample, group) for statistics - the worst row is asserted and recorded (record_parity, value = worst error / bound, bound 1).

Bounds (p = 8 significand bits with bf16 operands, 11 with fp16, chosen from ops.BF16 at run time).  References are fp64 formulas of the operand-rounded
inputs.  Derived from the formats, not measured; tests/test_vae_kernel_forms_host.py shows on the CPU that an fp32 emulation of a correct kernel passes
each of them and that the same emulation with a second rounding to the operand type fails.
  bit-equal   A copy, or ONE IEEE fp32 operation and one rounding: gn_apply without norm and SiLU (plain / upsampling), vae_add, nchw_to_grid (img * mul),
              grid_to_nchw, im2col without norm - equal to torch doing the same fp32 operation and .to(ops.BF16), zero padding of channels and taps included.
              (nchw_to_grid with mul != 1 found the fp16 build rounding the exact product once through v_fma_mixlo_f16; the kernel now keeps the fp32
              product apart from the conversion, so both builds follow this arithmetic.)
  element     Behind a GroupNorm, a SiLU or the softmax: |got - want| <= (2^-p + 2^-16) |want| + 2^-20 A + floor.  2^-p |want| is half an ulp of the
              stored value.  A is the size of the terms that cancel: |(x - m) r gamma| + |beta| for the norm - its fp32 evaluation makes at most four
              roundings of 2^-24 relative to a term of that size, and the SiLU (slope <= 1.1) passes them on - and 0 for the softmax and a SiLU alone.
              2^-16 |want| covers the roundings relative to the result: at most 8 fp32 operations, and __expf / rcp: __expf(a) = v_exp_f32(a * log2 e)
              carries the rounding of its argument, |a| 2^-24 relative, plus one ulp (2^-23) - below 2^-19 for the SiLU's |a| <= 16.  The softmax's
              argument (s - max) * scale is rounded twice more in front of that: 3 |a| 2^-24 + 2^-23 + the sum and the division (3 * 2^-24) is
              (3 |a| + 5) 2^-24 <= 245 * 2^-24 < 2^-16 for the |a| <= 80 used here.  floor = 2^-25 in the fp16 build only: half the smallest fp16
              subnormal, the rounding of a stored value below 2^-14 (softmax tails, SiLU of a very negative argument, a normalised value that cancels to
              nearly nothing); the issue names it for the softmax, the same rounding applies to every stored fp16 value.
              So that this bound applies to gn_apply, im2col and small_out alone, the tests hand them mean / rstd computed in fp64 by the test and rounded to
              fp32, and the reference uses exactly those fp32 values.
  small_out   fp32 image from packed 16-bit dot products of a staged operand that carries one rounding.  Reference: fp64 conv2d of the fp64 activation
              rounded to the operand type.  Per output row (b, y) rel-L2 over (Cout, W): 2e-5 without the norm (fp32 accumulation of 9 C products).  With
              norm + SiLU the kernel's fp32 activation can land on the other side of a rounding boundary than the fp64 one (one operand ulp on that
              tap): SMALL_OUT_NORM_TOL = 2 x the worst row of the host file's fp32 emulation over these very cases, 3.3e-5 (bf16) / 3.5e-5 (fp16) -
              it was 1e-3 over the whole tensor.
  statistics  2e-5 on mean and rstd as in test_vae_gpu.py, now relative per (sample, group).  The shifted case (mean = r sigma, r = 4) has the derived
              bound 0.5 (1 + r^2) D 2^-24 on rstd: var = E[x^2] - mean^2 with E[x^2] = (1 + r^2) var, every fp32 addition of a chain of D loses at most
              2^-24 of the running sum, rstd = var^-1/2 halves it.  D = loads per thread + the 2 additions that fold a quad + the LDS additions per
              group (gn_stats), computed from the launcher's arithmetic and asserted; block sums are combined in fp64.

Launch arithmetic (csrc/vae.hip) behind the shapes; each test recomputes and asserts the quantity that puts it on its edge.
  gn_stats    CV = C / 8 chunks per pixel, 256 threads, ppb = 256 / CV pixels per pass, per_row = ceil(W / ppb); nb = H blocks if per_row >= 8, else
              ceil(H * per_row / 8), clamped to [1, H]; a thread's two halves of a chunk go to groups (8 cv) / cpg and (8 cv + 4) / cpg.
  gn_finalize 64 threads per block over B * groups, cpg / 4 quads per group, PXA_COLSUM_SLOTS slots.
  gn_apply    a thread owns one 16-byte chunk column of GA_ROWS = 4 output rows: grid (ceil(Wo C / 8 / 256), ceil(Ho / 4), B); rows beyond Ho are
              loaded from the clamped row Ho - 1 and not stored.
  im2col3x3   grid (ceil(Wo * 9 * CV / 256), Ho, B).  Wo * 9 * CV is a multiple of 9, so 255 / 256 / 257 do not exist: 252 (one block, four idle threads),
              261 (a second block of five threads), 504 / 513 (a third block of one thread), 288 (C = 64).
  small_out   8 x 32 pixel tiles with a one-pixel halo, 64-channel chunks (SO_CC): grid (ceil(W / 32), ceil(H / 8), B).
  vae_add     grid (ceil(W C / 8 / 256), H, B).
  softmax     256 threads, one float4 per thread and pass: min(256, cols / 4) threads have work, ceil(cols / 1024) passes at the most.
  nchw / grid grid (ceil(W / 256), H, B), 8 channels per store.

Product call sites (vae/autoencoder_kl.py) each test stands for:
  test_gn_stats_forms                 _norm:314 on a convolution output (padded) below 1024 rows, on _conv1 / im2col outputs (compact)
  test_gn_stats_workspace_is_cleared  ops._GN_WS: one workspace per B * groups, shared by every layer of that key
  test_gn_stats_shifted_mean          the same call on activations with a large mean (post-residual levels)
  test_gn_finalize_forms              _norm:312 behind every statistics epilogue
  test_gn_apply_forms                 _conv3:328 compact -> padded_g (after attention / stem) and padded -> padded_g (resnets), with upsample = 2 the
                                      fallback of _conv3_up2:354; _conv3_up2:358 (plain copy); _attention:393 padded -> compact; the zero border of
                                      _padded:306 across consecutive calls
  test_im2col_forms                   _conv3:344 (stem: C = 8, stride 1, compact), _conv3_s2:375 (stride 2 from a padded grid)
  test_small_out_forms                decode:484 (padded grid, statistics from gn_finalize, norm + SiLU, Cout = 3)
  test_add_forms                      _conv3:342 vae_add(y, residual, y), y padded / residual compact; _attention:400 vae_add(o, x, o), o compact / x padded
  test_softmax_rows_forms             _attention_scores:422 (sbuf -> pbuf, cols = H * W of the latent)
  test_layout_conversion_forms        _to_grid:443 (encode:451 images 3 -> 8, decode:471 latents 4 -> 8 with mul); grid_to_nchw has no product caller left
  test_refusals                       the PXA_CHECK lines of every entry point
"""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from conftest import record_parity  # noqa: E402
from test_vae_conv_geometry_gpu import SENTINEL, img_rows  # noqa: E402
from test_vae_gpu import ops  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_SENTINEL = 0x5A5A5A5A            # 1.54e16 as a float
F32_BAND = 64
STAT_TOL = 2e-5                      # test_vae_gpu.py::test_groupnorm_stats_and_apply, ::test_conv_epilogue_groupnorm_statistics
SMALL_OUT_TOL = 2e-5                 # test_vae_gpu.py::test_conv3x3_small_out_is_groupnorm_silu_conv2d, without the norm
SMALL_OUT_NORM_TOL = {torch.bfloat16: 3.3e-5, torch.float16: 3.5e-5}      # file header; tests/test_vae_kernel_forms_host.py pins them to 2 x its emulation
GA_ROWS = 4
EPS = 1e-6


# ------------------------------------------------------------------------------------------------ bounds and references (CPU, shared with the host file)
def p_bits(dtype):
    return 11 if dtype == torch.float16 else 8


def elem_bound(want, A, dtype):
    """The element-wise bound of the file header; want, A fp64."""
    return (2.0 ** -p_bits(dtype) + 2.0 ** -16) * want.abs() + 2.0 ** -20 * A + (2.0 ** -25 if dtype == torch.float16 else 0.0)


def worst_row(got, want, bound=None):
    """(worst ratio, its row) of |got - want| / bound per row of the leading dimension; without a bound: the per-row rel-L2.  NaN counts as infinite."""
    got, want = got.double().flatten(1), want.double().flatten(1)
    if bound is None:
        ratio = (got - want).norm(dim=1) / want.norm(dim=1).clamp_min(1e-30)
    else:
        err = (got - want).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.flatten(1)).amax(1)
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    i = int(ratio.argmax())
    return float(ratio[i]), i


def cpu_rnd(*shape, scale=1.0, shift=0.0, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift


def norm_case(dtype, B, C, H, W, groups, seed):
    """Operand-rounded activation (B, C, H, W) with its GroupNorm statistics taken in fp64 and rounded to fp32, and an affine."""
    x = cpu_rnd(B, C, H, W, scale=1.5, shift=0.3, seed=seed).to(dtype)
    xg = x.double().view(B, groups, -1)
    mean, rstd = xg.mean(-1).flatten().float(), (xg.var(-1, unbiased=False) + EPS).rsqrt().flatten().float()
    return dict(x=x, mean=mean, rstd=rstd, gamma=cpu_rnd(C, scale=0.3, shift=1.0, seed=seed + 100), beta=cpu_rnd(C, scale=0.2, seed=seed + 200), groups=groups)


def _per_channel(c, B, C):
    G = c["groups"]
    m = c["mean"].view(B, G, 1).expand(B, G, C // G).reshape(B, C, 1, 1)
    r = c["rstd"].view(B, G, 1).expand(B, G, C // G).reshape(B, C, 1, 1)
    return m, r, c["gamma"].view(1, C, 1, 1), c["beta"].view(1, C, 1, 1)


def act_ref(c, norm, silu):
    """fp64 act(norm(x)) of the rounded x with the fp32 statistics: (want, A) as (B, C, H, W)."""
    x = c["x"].double()
    B, C = x.shape[:2]
    A = torch.zeros_like(x)
    if norm:
        m, r, ga, be = (t.double() for t in _per_channel(c, B, C))
        t = (x - m) * r * ga
        x, A = t + be, t.abs() + be.abs()
    return (x * torch.sigmoid(x) if silu else x), A


def act_emulate(c, norm, silu, dtype, second_rounding=False):
    """What a correct kernel stores: the kernel's fp32 formula - SiLU as v * (1 / (1 + exp2(-v * log2 e))), the product rounded to fp32 in front of the
    exponential as __expf does - and ONE rounding.  second_rounding: the intermediates go through the operand type too."""
    x = c["x"].float()
    B, C = x.shape[:2]
    if norm:
        m, r, ga, be = _per_channel(c, B, C)
        x = (x - m) * r
        if second_rounding and not silu:
            x = x.to(dtype).float()
        x = x * ga + be
    if silu:
        if second_rounding:
            x = x.to(dtype).float()
        sig = 1.0 / (1.0 + torch.exp2(-x * torch.tensor(math.log2(math.e), dtype=torch.float32)))
        if second_rounding:
            sig = sig.to(dtype).float()
        x = x * sig
    return x.to(dtype)


def softmax_scores(cols, scale, level, seed):
    """(8, cols) fp32 scores whose scaled values have spread `level` (1: unit normal; 80: the largest scaled gap of every row is 78); row 0 constant, row 1 one
    dominant entry, row 2 its maximum in the last four columns."""
    n = cpu_rnd(8, cols, seed=seed).double()
    if level > 1:
        n = (n - n.amax(1, keepdim=True)) / (n.amax(1, keepdim=True) - n.amin(1, keepdim=True)) * 78.0
    n[0] = 0.37
    n[1] = -n[1].abs().clamp(max=48.0) - 30.0
    n[1, cols // 3] = 0.0
    n[2, cols - 2] = n[2].max() + 1.0
    return (n / scale).float()


def softmax_ref(s, scale):
    z = (s.double() - s.double().amax(1, keepdim=True)) * float(torch.tensor(scale, dtype=torch.float32))
    e = z.exp()
    return e / e.sum(1, keepdim=True), z


def softmax_emulate(s, scale, dtype, second_rounding=False):
    sc = torch.tensor(scale, dtype=torch.float32)
    e = ((s - s.amax(1, keepdim=True)) * sc).exp()
    inv = 1.0 / e.sum(1, keepdim=True)
    if second_rounding:
        e = e.to(dtype).float()
    return (e * inv).to(dtype)


# (Cout, C, groups, H, W, layout, norm, bias): C = 192 -> three chunks of SO_CC and cpg = 12; W, H around the 8 x 32 tile
SMALL_OUT_CASES = [(3, 128, 32, 9, 33, "padded", True, True), (1, 64, 16, 7, 31, "compact", True, True), (2, 192, 16, 8, 32, "padded", True, True),
                   (4, 64, 16, 17, 65, "padded", True, False), (3, 192, 16, 9, 31, "compact", False, True), (4, 128, 32, 7, 65, "padded", False, False),
                   (2, 64, 16, 17, 33, "padded_u", True, True)]


def small_out_case(dtype, Co, C, groups, H, W, seed=1):
    B = 2
    c = norm_case(dtype, B, C, H, W, groups, seed)
    c["w"] = cpu_rnd(Co, C, 3, 3, scale=(9 * C) ** -0.5, seed=seed + 1).to(dtype)
    c["bias"] = cpu_rnd(Co, seed=seed + 2)
    return c


def small_out_ref(c, norm, bias, dtype):
    a, _ = act_ref(c, norm, norm)
    return F.conv2d(a.to(dtype).double(), c["w"].double(), c["bias"].double() if bias else None, padding=1)


def small_out_emulate(c, norm, bias, dtype, second_rounding=False):
    a = act_emulate(c, norm, norm, dtype, second_rounding)
    return F.conv2d(a.float(), c["w"].float(), c["bias"] if bias else None, padding=1)


def image_rows(t):
    """(B, Co, H, W) -> (B * H, Co * W): one row per (sample, image row)."""
    return t.permute(0, 2, 1, 3).reshape(t.shape[0] * t.shape[2], -1)


# shifted statistics: B, C, groups, H, W and the mean in units of the standard deviation
SHIFT_CASE = (2, 512, 32, 8, 16, 4.0)


def gn_stats_launch(H, W, C):
    """(CV, ppb, per_row, nb) of pxa_vae_gn_stats."""
    CV = C // 8
    ppb = 256 // CV
    per_row = (W + ppb - 1) // ppb
    nb = H if per_row >= 8 else (H * per_row + 7) // 8
    return CV, ppb, per_row, max(1, min(nb, H))


def gn_stats_chain(H, W, C, groups):
    """D: the longest fp32 addition chain of gn_stats_kernel at this geometry (file header)."""
    CV, ppb, per_row, nb = gn_stats_launch(H, W, C)
    loads = per_row * ((H + nb - 1) // nb)
    lds_adds = ppb * (C // groups) // 4          # thread halves of a block that add into one group's LDS pair
    return loads + 2 + lds_adds


def shifted_rstd_bound(r, D):
    return 0.5 * (1.0 + r * r) * D * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ GPU harness
def geometry(B, H, W, layout):
    """(row pitch, image pitch, origin, pixel slots of the view)."""
    if layout == "compact":
        return W, H * W, 0, B * H * W
    rp = W + 2
    if layout == "padded":
        return rp, img_rows(H, W), W + 3, B * img_rows(H, W)
    if layout == "padded_g":
        return rp, img_rows(H, W), (W + 3) + rp + 1, B * img_rows(H, W) + 2 * (W + 3)
    assert layout == "padded_u"
    return rp, (H + 2) * rp, W + 3, B * (H + 2) * rp


class Banded:
    """banded_grid: a Grid whose buffer is a view inside a larger allocation.  fill: "nan" (input), "sentinel" or "zero" (output; zero: the slots are zero as
    _padded makes them, the bands the sentinel)."""

    def __init__(self, ops, B, H, W, C, layout, fill):
        rp, ip, origin, slots = geometry(B, H, W, layout)
        band = max(GA_ROWS * (W + 2) + 3, 64)           # >= W + 3, and a whole row group of gn_apply: a kernel that walks past the last image row stays inside
        if fill == "nan":
            whole = torch.full((band + slots + band, C), float("nan"), dtype=ops.BF16, device="cuda")
        else:
            whole = torch.full((band + slots + band, C), SENTINEL, dtype=torch.int16, device="cuda").view(ops.BF16)
            if fill == "zero":
                whole[band:band + slots] = 0
        dev = whole.device
        self.idx = (torch.arange(B, device=dev)[:, None, None] * ip + torch.arange(H, device=dev)[None, :, None] * rp
                    + torch.arange(W, device=dev)[None, None, :] + origin + band)
        assert int(self.idx.min()) >= band and int(self.idx.max()) < band + slots
        self.outside = torch.ones(whole.shape[0], dtype=torch.bool, device=dev)
        self.outside[self.idx.flatten()] = False
        self.whole, self.init = whole, whole.view(torch.int16).clone()
        self.grid = ops.Grid(whole[band:band + slots], B, H, W, C, rp, ip, origin)
        assert self.grid.buf.data_ptr() == whole.data_ptr() + band * C * 2

    def put(self, nchw):
        self.whole[self.idx] = nchw.permute(0, 2, 3, 1).to(self.whole.dtype).cuda()
        return self

    def get(self):
        """(B, C, H, W) of the interior pixels, on the CPU, in the operand type."""
        return self.whole[self.idx].permute(0, 3, 1, 2).cpu()

    def assert_outside_untouched(self, what):
        bad = ((self.whole.view(torch.int16) != self.init).any(1) & self.outside).nonzero().flatten()
        assert bad.numel() == 0, f"{what}: {bad.numel()} pixel slots outside the interior were written, first at slot {int(bad[0])} of the allocation"


def banded_grid(ops, B, H, W, C, layout, fill="sentinel"):
    return Banded(ops, B, H, W, C, layout, fill)


def input_grid(ops, x, layout):
    B, C, H, W = x.shape
    return Banded(ops, B, H, W, C, layout, "nan").put(x)


class BandedF32:
    """n floats (or 16-bit rows: dtype) between two sentinel bands of F32_BAND floats."""

    def __init__(self, n, dtype=torch.float32, fill=F32_SENTINEL):
        per = 4 // torch.empty(0, dtype=dtype).element_size()
        self.whole = torch.full((2 * F32_BAND + (n + per - 1) // per,), fill, dtype=torch.int32, device="cuda")
        self.view = self.whole[F32_BAND:-F32_BAND].view(dtype)[:n]
        self.fill = fill

    def assert_bands_untouched(self, what):
        assert (self.whole[:F32_BAND] == self.fill).all(), f"{what}: a store in front of the output"
        assert (self.whole[-F32_BAND:] == self.fill).all(), f"{what}: a store behind the output"

    def assert_untouched(self, what):
        assert (self.whole == self.fill).all(), f"{what}: a refused call wrote its output"


def nan_banded_f32(t):
    """A copy of the fp32 tensor t inside an allocation that holds NaN everywhere else."""
    whole = torch.full((2 * F32_BAND + t.numel(),), float("nan"), dtype=torch.float32, device="cuda")
    view = whole[F32_BAND:F32_BAND + t.numel()].view(t.shape)
    view.copy_(t)
    return whole, view


def norm_args(c):
    return tuple(c[k].cuda() for k in ("mean", "rstd", "gamma", "beta")) + (c["groups"],)


def check(label, got, want, bound=None, tol=1.0):
    """Per-row comparison (rows = leading dimension): worst row asserted and recorded; with a bound the ratio error / bound against 1, else rel-L2 against tol."""
    assert torch.isfinite(got.float()).all(), f"{label}: the result is not finite (a slot outside the interior was read?)"
    worst, row = worst_row(got, want, bound)
    print(f"\n{label}: worst row {row}: {'error / bound' if bound is not None else 'rel-L2'} {worst:.3e} (bound {tol:.1e})")
    record_parity(label, worst, tol)
    assert worst <= tol, (label, row, worst, tol)


def assert_bit_equal(label, got, want):
    """got, want (rows, ...) of the operand type: equal bit for bit, reported per row."""
    assert got.dtype == want.dtype and got.shape == want.shape
    ne = (got.contiguous().view(torch.int16) != want.contiguous().view(torch.int16)).flatten(1).sum(1) if got.element_size() == 2 else \
        (got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).flatten(1).sum(1)
    assert int(ne.sum()) == 0, f"{label}: {int(ne.sum())} elements differ in {int((ne > 0).sum())} rows, first row {int((ne > 0).nonzero()[0])}"


def grid_rows(t):
    """(B, C, H, W) -> (B * H, W, C): one row per (sample, image row), in the grid's memory order."""
    return t.permute(0, 2, 3, 1).reshape(t.shape[0] * t.shape[2], t.shape[3], t.shape[1])


# ------------------------------------------------------------------------------------------------ 1. gn_stats
# (B, H, W, C, groups) -> expected (CV, ppb, per_row, nb)
GN_STATS_CASES = [
    ((3, 1, 7, 8, 2), (1, 256, 1, 1)),          # CV = 1: the two halves of a chunk are two groups; H = 1; W < ppb; B = 3
    ((2, 4, 300, 8, 2), (1, 256, 2, 1)),        # W no multiple of ppb, one block walks all four rows
    ((2, 12, 20, 64, 16), (8, 32, 1, 2)),       # cpg = 4; nb = 2 < H: a block walks six rows
    ((1, 5, 9, 512, 32), (64, 4, 3, 2)),        # W no multiple of ppb = 4
    ((1, 9, 7, 2048, 256), (256, 1, 7, 8)),     # CV = 256: one pixel per pass, the LDS array full; per_row = 7 -> nb = 8 < H = 9
    ((1, 3, 8, 2048, 256), (256, 1, 8, 3)),     # per_row = 8: the branch to one block per row
    ((1, 1, 1, 2048, 256), (256, 1, 1, 1)),     # one pixel
]


def call_gn_stats(ops, g, groups):
    from pixart_sigma_amd import lib
    n = g.B * groups
    ws = torch.full((2 * n,), float("nan"), dtype=torch.float64, device="cuda")       # the call zeroes it
    mean, rstd = BandedF32(n), BandedF32(n)
    lib.call("pxa_vae_gn_stats", g.arg(), groups, EPS, lib.ptr(ws), lib.ptr(mean.view), lib.ptr(rstd.view))
    torch.cuda.synchronize()
    return mean, rstd


def stats_ref(x, groups):
    xg = x.double().view(x.shape[0], groups, -1)
    return xg.mean(-1).flatten(), (xg.var(-1, unbiased=False) + EPS).rsqrt().flatten()


def check_stats(label, mean, rstd, want_mean, want_rstd, tol_mean=STAT_TOL, tol_rstd=STAT_TOL):
    """mean / rstd per (sample, group): relative error of each, the worst asserted and recorded."""
    for name, got, want, tol in (("mean", mean, want_mean, tol_mean), ("rstd", rstd, want_rstd, tol_rstd)):
        got = got.cpu()
        assert torch.isfinite(got).all(), f"{label}: {name} is not finite"
        rel = (got.double() - want).abs() / want.abs()
        i = int(rel.argmax())
        print(f"\n{label}: {name} worst (sample, group) {i}: rel {float(rel[i]):.3e} (bound {tol:.2e})")
        record_parity(f"{label} {name}", float(rel[i]), tol)
        assert float(rel[i]) <= tol, (label, name, i, float(rel[i]), tol)


@pytest.mark.parametrize("layout", ["compact", "padded"])
@pytest.mark.parametrize("case,want", GN_STATS_CASES, ids=lambda v: "x".join(map(str, v)) if len(v) == 5 else None)
def test_gn_stats_forms(ops, case, want, layout):
    B, H, W, C, groups = case
    assert gn_stats_launch(H, W, C) == want, f"the launch arithmetic of this case moved: {gn_stats_launch(H, W, C)}"
    x = cpu_rnd(B, C, H, W, shift=1.5, seed=1).to(ops.BF16)              # every group's mean is several of its own standard errors away from 0
    bg = input_grid(ops, x, layout)
    mean, rstd = call_gn_stats(ops, bg.grid, groups)
    label = f"gn_stats B{B} {H}x{W} C{C} G{groups} {layout}"
    mean.assert_bands_untouched(label), rstd.assert_bands_untouched(label)
    check_stats(label, mean.view, rstd.view, *stats_ref(x, groups))
    bg.assert_outside_untouched(label)


def test_gn_stats_workspace_is_cleared(ops):
    """ops._GN_WS keeps one workspace per B * groups: two calls of equal product (3 x 16, then 6 x 8), then the second key again on other data - every call
    must start from its own zeroed sums."""
    seen = set()
    for B, C, groups, seed in ((3, 64, 16, 1), (6, 32, 8, 2), (6, 32, 8, 3)):
        x = cpu_rnd(B, C, 5, 9, shift=1.5, seed=seed).to(ops.BF16)
        mean, rstd = ops.vae_gn_stats(input_grid(ops, x, "padded").grid, groups, EPS)
        ws = [v for k, v in ops._GN_WS.items() if k[1] == B * groups]
        assert B * groups == 48 and len(ws) == 1, "ops._GN_WS no longer shares one workspace per B * groups: this test pins nothing"
        seen.add(ws[0].data_ptr())
        check_stats(f"gn_stats workspace B{B} G{groups} seed {seed}", mean, rstd, *stats_ref(x, groups))
    assert len(seen) == 1


def test_gn_stats_shifted_mean(ops):
    B, C, groups, H, W, r = SHIFT_CASE
    D = gn_stats_chain(H, W, C, groups)
    assert gn_stats_launch(H, W, C) == (64, 4, 4, 4) and D == 8 + 2 + 16, (gn_stats_launch(H, W, C), D)
    bound = shifted_rstd_bound(r, D)
    assert bound <= STAT_TOL, bound
    x = cpu_rnd(B, C, H, W, shift=r, seed=5).to(ops.BF16)
    mean, rstd = call_gn_stats(ops, input_grid(ops, x, "padded").grid, groups)
    check_stats(f"gn_stats shifted r = {r:g} D = {D}", mean.view, rstd.view, *stats_ref(x, groups), tol_rstd=bound)


# ------------------------------------------------------------------------------------------------ 2. gn_finalize
@pytest.mark.parametrize("B,C,groups,n", [(3, 84, 21, 63), (4, 128, 16, 64), (5, 208, 13, 65), (3, 96, 8, 24), (3, 252, 21, 63)])
def test_gn_finalize_forms(ops, B, C, groups, n):
    """Partial sums laid down by the test in all PXA_COLSUM_SLOTS slots: random parts of both signs whose fp64 totals are the quad sums of known data.
    cpg 4 (84 / 21), 8 (128 / 16), 16 (208 / 13) and 12 (96 / 8, 252 / 21: not a power of two); B * groups 63, 64 and 65 around the 64-thread block
    (B = 3 at 63; 64 and 65 are no multiples of 3: B = 4 and 5 there)."""
    from pixart_sigma_amd import lib
    pixels = 40
    assert B * groups == n and C % groups == 0 and (C // groups) % 4 == 0
    x = cpu_rnd(B, C, pixels, shift=1.5, seed=C).double()
    q = x.view(B, C // 4, 4 * pixels)
    total = torch.stack([q.sum(-1), (q * q).sum(-1)], -1)                                         # (B, C/4, 2)
    parts = cpu_rnd(ops.COLSUM_SLOTS, B, C // 4, 2, seed=C + 1).double() * total.abs()
    parts[-1] = total - parts[:-1].sum(0)
    parts = parts.float()                                                                          # what the kernel reads; its fp64 sum is the known total
    tot = parts.double().sum(0)
    cnt = pixels * (C // groups)
    m = tot[..., 0].view(B, groups, -1).sum(-1) / cnt
    var = (tot[..., 1].view(B, groups, -1).sum(-1) / cnt - m * m).clamp_min(0)
    assert (var > 0.3).all()
    whole, part = nan_banded_f32(parts.cuda())
    mean, rstd = BandedF32(n), BandedF32(n)
    lib.call("pxa_vae_gn_finalize", lib.ptr(part), B, C, groups, pixels, EPS, lib.ptr(mean.view), lib.ptr(rstd.view))
    torch.cuda.synchronize()
    label = f"gn_finalize C{C} G{groups} cpg{C // groups}"
    mean.assert_bands_untouched(label), rstd.assert_bands_untouched(label)
    check_stats(label, mean.view, rstd.view, m.flatten(), (var + EPS).rsqrt().flatten())


# ------------------------------------------------------------------------------------------------ 3. gn_apply
# (H, W, C, groups, upsample, input layout, output layout, norm, silu) -> (chunks of an output row, blocks in x, row groups, rows of the last group)
GN_APPLY_CASES = [
    ((1, 255, 8, 2, 1, "compact", "compact", True, True), (255, 1, 1, 1)),        # cpg = 4: the halves of the only chunk are two groups
    ((3, 256, 8, 2, 1, "compact", "padded_g", True, False), (256, 1, 1, 3)),
    ((4, 257, 8, 2, 1, "padded", "padded_g", True, True), (257, 2, 1, 4)),
    ((5, 85, 24, 2, 1, "padded", "compact", True, False), (255, 1, 2, 1)),        # C = 24, cpg = 12: the division branch of Norm::apply
    ((9, 86, 24, 2, 1, "padded", "padded_g", True, True), (258, 2, 3, 1)),
    ((5, 11, 96, 8, 1, "padded", "padded_g", True, True), (132, 1, 2, 1)),        # C = 96, groups = 8: cpg = 12
    ((9, 22, 96, 8, 1, "padded", "compact", True, False), (264, 2, 3, 1)),
    ((3, 40, 64, 16, 1, "compact", "padded_g", True, True), (320, 2, 1, 3)),
    ((5, 257, 8, 2, 1, "padded_u", "padded_u", False, False), (257, 2, 2, 1)),    # plain copy between padded views
    ((9, 256, 8, 2, 1, "compact", "padded_g", False, True), (256, 1, 3, 1)),      # SiLU alone
    ((1, 127, 8, 2, 2, "compact", "padded_g", False, False), (254, 1, 1, 2)),     # upsampling copy (_conv3_up2's fallback): output heights 2, 6, 8, 10, 18
    ((3, 128, 8, 2, 2, "padded", "padded_g", False, False), (256, 1, 2, 2)),
    ((4, 43, 24, 2, 2, "padded", "padded_g", True, True), (258, 2, 2, 4)),
    ((5, 129, 8, 2, 2, "padded", "compact", True, False), (258, 2, 3, 2)),
    ((9, 6, 96, 8, 2, "compact", "padded_g", True, True), (144, 1, 5, 2)),
]


@pytest.mark.parametrize("case,want", GN_APPLY_CASES, ids=lambda v: "_".join(map(str, v)) if len(v) == 9 else None)
def test_gn_apply_forms(ops, case, want):
    """Two consecutive calls with different inputs into the same target (the _pad_cache promise: zero border, tail and guards of a padded target stay zero),
    the second result checked per (sample, image row)."""
    H, W, C, groups, up, lin, lout, norm, silu = case
    B, Ho, Wo = 2, H * up, W * up
    chunks = Wo * C // 8
    assert (chunks, (chunks + 255) // 256, (Ho + GA_ROWS - 1) // GA_ROWS, (Ho - 1) % GA_ROWS + 1) == want, "the launch arithmetic of this case moved"
    out = banded_grid(ops, B, Ho, Wo, C, lout, "zero" if lout != "compact" else "sentinel")
    label = "gn_apply " + "_".join(map(str, case))
    for seed in (1, 2):
        c = norm_case(ops.BF16, B, C, H, W, groups, seed)
        ops.vae_gn_apply(input_grid(ops, c["x"], lin).grid, out.grid, norm_args(c) if norm else None, silu, up)
        torch.cuda.synchronize()
        out.assert_outside_untouched(f"{label} call {seed}")
    got = out.get()
    want_v, A = (t.repeat_interleave(up, 2).repeat_interleave(up, 3) for t in act_ref(c, norm, silu))
    if norm or silu:
        check(label, grid_rows(got), grid_rows(want_v), grid_rows(elem_bound(want_v, A, ops.BF16)))
    else:
        assert_bit_equal(label, grid_rows(got), grid_rows(c["x"].repeat_interleave(up, 2).repeat_interleave(up, 3)))


# ------------------------------------------------------------------------------------------------ 4. im2col3x3
# (H, W, C, groups, stride, layout, norm) -> (chunks of an output row's patches, blocks in x, Ho)
IM2COL_CASES = [
    ((5, 28, 8, 2, 1, "compact", False), (252, 1, 5)),            # the stem: C = 8, stride 1, pad 1
    ((1, 29, 8, 2, 1, "compact", False), (261, 2, 1)),            # Ho = 1: every patch hangs over the top and the bottom
    ((4, 57, 8, 2, 1, "compact", False), (513, 3, 4)),            # a third block with one thread
    ((6, 56, 8, 2, 2, "padded", False), (252, 1, 3)),             # _conv3_s2: stride 2, pad 0 from a padded grid
    ((2, 58, 8, 2, 2, "padded", False), (261, 2, 1)),
    ((5, 9, 64, 16, 2, "padded", False), (288, 2, 2)),            # odd H and W: the last row / column of taps stays inside
    ((4, 4, 64, 16, 1, "compact", True), (288, 2, 4)),            # norm + SiLU
    ((3, 10, 24, 2, 1, "padded", True), (270, 2, 3)),             # cpg = 12
    ((2, 6, 96, 8, 2, "padded", True), (324, 2, 1)),              # cpg = 12, stride 2
]


@pytest.mark.parametrize("case,want", IM2COL_CASES, ids=lambda v: "_".join(map(str, v)) if len(v) == 7 else None)
def test_im2col_forms(ops, case, want):
    """The patch matrix itself against F.unfold of the fp64 activation: taps outside the image are exactly zero, not act(norm(0))."""
    from pixart_sigma_amd import lib
    H, W, C, groups, stride, layout, norm = case
    B = 2
    Ho, Wo, pad = (H, W, 1) if stride == 1 else (H // 2, W // 2, 0)
    chunks = Wo * 9 * (C // 8)
    assert (chunks, (chunks + 255) // 256, Ho) == want, "the launch arithmetic of this case moved"
    c = norm_case(ops.BF16, B, C, H, W, groups, seed=3)
    bg = input_grid(ops, c["x"], layout)
    rows = B * Ho * Wo
    col = BandedF32(rows * 9 * C, ops.BF16)
    mean, rstd, gamma, beta, g = norm_args(c) if norm else (None, None, None, None, 1)
    lib.call("pxa_vae_im2col3x3", bg.grid.arg(), lib.ptr(mean), lib.ptr(rstd), lib.ptr(gamma), lib.ptr(beta), g, int(norm), stride, pad, Ho, Wo, lib.ptr(col.view))
    torch.cuda.synchronize()
    label = "im2col " + "_".join(map(str, case))
    col.assert_bands_untouched(label)
    bg.assert_outside_untouched(label)

    def patches(t):                                     # (B, C, H, W) fp64 -> (B * Ho * Wo, 9 * C), k = tap * C + c
        u = F.unfold(t, 3, padding=1) if stride == 1 else F.unfold(F.pad(t, (0, 1, 0, 1)), 3, stride=2)
        assert u.shape[2] == Ho * Wo
        return u.view(B, C, 9, Ho * Wo).permute(0, 3, 2, 1).reshape(rows, 9 * C)
    got = col.view.view(rows, 9 * C).cpu()
    if norm:
        want_v, A = (patches(t) for t in act_ref(c, True, True))
        outside = patches(torch.ones_like(c["x"], dtype=torch.float64)) == 0
        assert (got[outside].view(torch.int16) == 0).all(), f"{label}: a tap outside the image is not +0"
        check(label, got, want_v, elem_bound(want_v, A, ops.BF16))
    else:
        assert_bit_equal(label, got, patches(c["x"].double()).to(ops.BF16))


# ------------------------------------------------------------------------------------------------ 5. conv3x3_small_out
@pytest.mark.parametrize("case", SMALL_OUT_CASES, ids=lambda v: "_".join(map(str, v)))
def test_small_out_forms(ops, case):
    from pixart_sigma_amd import lib
    Co, C, groups, H, W, layout, norm, bias = case
    B = 2
    assert C % 64 == 0 and (C // groups) % 4 == 0
    c = small_out_case(ops.BF16, Co, C, groups, H, W)
    bg = input_grid(ops, c["x"], layout)
    img = BandedF32(B * Co * H * W)
    taps = c["w"].permute(2, 3, 0, 1).reshape(9, Co, C).contiguous().cuda()
    mean, rstd, gamma, beta, g = norm_args(c) if norm else (None, None, None, None, 1)
    bias_t = c["bias"].cuda() if bias else None
    lib.call("pxa_vae_conv3x3_small_out", bg.grid.arg(), lib.ptr(mean), lib.ptr(rstd), lib.ptr(gamma), lib.ptr(beta), g, int(norm), lib.ptr(taps),
             lib.ptr(bias_t), Co, lib.ptr(img.view))
    torch.cuda.synchronize()
    label = "small_out " + "_".join(map(str, case))
    img.assert_bands_untouched(label)
    bg.assert_outside_untouched(label)
    check(label, image_rows(img.view.view(B, Co, H, W).cpu()), image_rows(small_out_ref(c, norm, bias, ops.BF16)),
          tol=SMALL_OUT_NORM_TOL[ops.BF16] if norm else SMALL_OUT_TOL)


# ------------------------------------------------------------------------------------------------ 6. vae_add
@pytest.mark.parametrize("form", ["y_res_y", "o_x_o", "three"])
@pytest.mark.parametrize("H,W,C", [(1, 255, 8), (3, 256, 8), (2, 257, 8), (3, 33, 64)], ids=lambda v: str(v))
def test_add_forms(ops, form, H, W, C):
    B = 2
    chunks = W * C // 8
    assert chunks in (255, 256, 257, 264)
    a, b = (cpu_rnd(B, C, H, W, seed=s).to(ops.BF16) for s in (1, 2))
    la, lb, lo = dict(y_res_y=("padded", "compact", None), o_x_o=("compact", "padded", None), three=("padded", "padded_u", "padded_g"))[form]
    ga, gb = input_grid(ops, a, la), input_grid(ops, b, lb)
    go = banded_grid(ops, B, H, W, C, lo) if lo else ga                 # in place: the NaN outside a's interior is the sentinel that must survive
    ops.vae_add(ga.grid, gb.grid, go.grid)
    torch.cuda.synchronize()
    label = f"vae_add {form} {H}x{W} C{C}"
    for g in (ga, gb, go):
        g.assert_outside_untouched(label)
    assert_bit_equal(label, grid_rows(go.get()), grid_rows((a.float() + b.float()).to(ops.BF16)))
    assert_bit_equal(label + " (b unchanged)", grid_rows(gb.get()), grid_rows(b))


# ------------------------------------------------------------------------------------------------ 7. softmax_rows
# cols -> (threads with work, passes of thread 0, threads that make that many passes)
SOFTMAX_COLS = {8: (2, 1, 2), 384: (96, 1, 96), 1024: (256, 1, 256), 1032: (256, 2, 2), 2052: (256, 3, 1)}


@pytest.mark.parametrize("level", [1, 80])
@pytest.mark.parametrize("cols", list(SOFTMAX_COLS))
def test_softmax_rows_forms(ops, cols, level):
    from pixart_sigma_amd import lib
    quads = cols // 4
    assert (min(256, quads), (quads + 255) // 256, (quads - 1) % 256 + 1) == SOFTMAX_COLS[cols], "the launch arithmetic of this case moved"
    C = 512 if level == 1 else 256
    scale = C ** -0.5
    s = softmax_scores(cols, scale, level, seed=cols)
    want, z = softmax_ref(s, scale)
    assert float(z.min()) >= -80.0 and (level == 1 or float(z[3:].amin(1).max()) <= -77.0)
    rows, ld, ldp = s.shape[0], cols + 12, cols + 20
    sw = torch.full((F32_BAND + rows * ld + F32_BAND,), float("nan"), dtype=torch.float32, device="cuda")
    sv = sw[F32_BAND:F32_BAND + rows * ld].view(rows, ld)
    sv[:, :cols] = s.cuda()
    out = BandedF32(rows * ldp, ops.BF16)
    lib.call("pxa_vae_softmax_rows", lib.ptr(sv), ld, lib.ptr(out.view), ldp, rows, cols, scale)
    torch.cuda.synchronize()
    label = f"softmax_rows cols {cols} spread {level} scale {C}^-1/2"
    out.assert_bands_untouched(label)
    p = out.view.view(rows, ldp).cpu()
    assert (p[:, cols:].contiguous().view(torch.int16) == SENTINEL).all(), f"{label}: a store between the rows of the output"
    p = p[:, :cols]
    check(label, p, want, elem_bound(want, torch.zeros_like(want), ops.BF16))
    dev = (p.double().sum(1) - 1.0).abs().max().item()
    assert dev <= cols * 2.0 ** -p_bits(ops.BF16), (label, dev)
    # the compact form of the product (sbuf -> pbuf)
    assert torch.equal(ops.vae_softmax_rows(s.cuda(), scale).cpu(), p)


# ------------------------------------------------------------------------------------------------ 8. nchw_to_grid / grid_to_nchw
@pytest.mark.parametrize("C,Cg,W,layout,mul", [(3, 8, 255, "compact", 1.0), (4, 8, 256, "compact", 1 / 0.13025), (8, 8, 257, "padded", 1 / 0.13025),
                                               (9, 16, 257, "padded_u", 1.0), (4, 8, 257, "padded_g", 1.0)])
def test_layout_conversion_forms(ops, C, Cg, W, layout, mul):
    from pixart_sigma_amd import lib
    B, H = 2, 3
    assert (W + 255) // 256 == (1 if W <= 256 else 2)
    img = cpu_rnd(B, C, H, W, seed=C + W)
    whole, view = nan_banded_f32(img.cuda())
    out = banded_grid(ops, B, H, W, Cg, layout)
    lib.call("pxa_vae_nchw_to_grid", lib.ptr(view), C, mul, out.grid.arg())
    torch.cuda.synchronize()
    label = f"nchw_to_grid C{C}->{Cg} W{W} {layout} mul {mul:.4g}"
    out.assert_outside_untouched(label)
    want = torch.zeros(B, Cg, H, W)
    want[:, :C] = img * torch.tensor(mul, dtype=torch.float32)
    got = out.get()
    assert_bit_equal(label, grid_rows(got), grid_rows(want.to(ops.BF16)))                  # padding channels: +0 exactly
    # and back, out of the same (possibly padded) grid whose other slots now hold NaN
    src = input_grid(ops, got, layout)
    back = BandedF32(B * C * H * W)
    lib.call("pxa_vae_grid_to_nchw", src.grid.arg(), C, lib.ptr(back.view))
    torch.cuda.synchronize()
    back.assert_bands_untouched(label + " back")
    assert_bit_equal(label + " back", back.view.view(B * C * H, W).cpu(), got[:, :C].float().reshape(B * C * H, W))


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals(ops):
    """The refused calls of every entry point (the PXA_CHECK lines of csrc/vae.hip): -1, the message in pxa_last_error, outputs untouched."""
    from pixart_sigma_amd import lib
    from pixart_sigma_amd.lib import PixartHipError
    P = lib.ptr
    B, H, W, C = 1, 2, 4, 64
    x = input_grid(ops, cpu_rnd(B, C, H, W, seed=1).to(ops.BF16), "padded")
    y = banded_grid(ops, B, H, W, C, "padded_g")
    y2 = banded_grid(ops, B, 2 * H, 2 * W, C, "compact")
    f = [BandedF32(4096) for _ in range(3)]
    o16 = BandedF32(B * H * W * 9 * C, ops.BF16)
    ws = torch.zeros(512, dtype=torch.float64, device="cuda")
    v = torch.ones(C, device="cuda")
    s = torch.zeros(4, 64, device="cuda")
    taps = torch.zeros(9, 4, C, dtype=ops.BF16, device="cuda")

    def grid(g, **kw):
        a = g.grid.arg()
        for k, val in kw.items():
            setattr(a, k, val)
        return a
    none = (None, None, None, None, 1)
    refused = [
        ("pxa_vae_gn_stats", (grid(x, C=60), 4, EPS, P(ws), P(f[0].view), P(f[1].view)), "bad grid"),
        ("pxa_vae_gn_stats", (grid(x, row_pitch=W - 1), 4, EPS, P(ws), P(f[0].view), P(f[1].view)), "bad pitches"),
        ("pxa_vae_gn_stats", (grid(x, img_pitch=H * (W + 2) - 3), 4, EPS, P(ws), P(f[0].view), P(f[1].view)), "bad pitches"),
        ("pxa_vae_gn_stats", (grid(x), 4, EPS, None, P(f[0].view), P(f[1].view)), "null output"),
        ("pxa_vae_gn_stats", (grid(x), 32, EPS, P(ws), P(f[0].view), P(f[1].view)), "must be a multiple of 4"),
        ("pxa_vae_gn_stats", (grid(x), 0, EPS, P(ws), P(f[0].view), P(f[1].view)), "must be a multiple of 4"),
        ("pxa_vae_gn_stats", (grid(x, C=24), 2, EPS, P(ws), P(f[0].view), P(f[1].view)), "must be 8 \\* a power of two"),
        ("pxa_vae_gn_finalize", (P(s), 0, C, 16, 8, EPS, P(f[0].view), P(f[1].view)), "bad arguments"),
        ("pxa_vae_gn_finalize", (P(s), 1, C, 16, 0, EPS, P(f[0].view), P(f[1].view)), "bad arguments"),
        ("pxa_vae_gn_finalize", (P(s), 1, C, 32, 8, EPS, P(f[0].view), P(f[1].view)), "must be a multiple of 4"),
        ("pxa_vae_gn_apply", (grid(x),) + none + (0, 3, grid(y)), "upsample must be 1 or 2"),
        ("pxa_vae_gn_apply", (grid(x),) + none + (0, 2, grid(y)), "output grid does not match"),
        ("pxa_vae_gn_apply", (grid(x),) + none + (0, 1, grid(y2)), "output grid does not match"),
        ("pxa_vae_gn_apply", (grid(x),) + none + (0, 1, grid(y, C=60)), "bad grid"),
        ("pxa_vae_gn_apply", (grid(x), P(v), None, P(v), P(v), 16, 0, 1, grid(y)), "GroupNorm needs mean, rstd, gamma and beta"),
        ("pxa_vae_gn_apply", (grid(x), P(v), P(v), P(v), P(v), 32, 0, 1, grid(y)), "must be a multiple of 4"),
        ("pxa_vae_im2col3x3", (grid(x),) + none + (0, 3, 1, H, W, P(o16.view)), "bad arguments"),
        ("pxa_vae_im2col3x3", (grid(x),) + none + (0, 1, 2, H, W, P(o16.view)), "bad arguments"),
        ("pxa_vae_im2col3x3", (grid(x),) + none + (0, 1, 1, 0, W, P(o16.view)), "bad arguments"),
        ("pxa_vae_im2col3x3", (grid(x), P(v), P(v), P(v), None, 16, 0, 1, 1, H, W, P(o16.view)), "GroupNorm needs"),
        ("pxa_vae_add", (grid(x), grid(x), grid(y2)), "grids differ"),
        ("pxa_vae_add", (grid(x), grid(y, row_pitch=1), grid(y)), "bad pitches"),
        ("pxa_vae_softmax_rows", (P(s), 64, P(o16.view), 64, 4, 62, 1.0), "multiples of 4"),
        ("pxa_vae_softmax_rows", (P(s), 66, P(o16.view), 64, 4, 60, 1.0), "multiples of 4"),
        ("pxa_vae_softmax_rows", (P(s), 64, P(o16.view), 64, 0, 64, 1.0), "bad arguments"),
        ("pxa_vae_softmax_rows", (P(s[0, 1:]), 64, P(o16.view), 64, 3, 60, 1.0), "16-byte"),
        ("pxa_vae_softmax_rows", (P(s), 64, P(o16.view[2:]), 64, 4, 60, 1.0), "8-byte aligned"),
        ("pxa_vae_nchw_to_grid", (P(s), 65, 1.0, grid(y)), "bad channel count"),
        ("pxa_vae_nchw_to_grid", (P(s), 0, 1.0, grid(y)), "bad channel count"),
        ("pxa_vae_grid_to_nchw", (grid(x), 65, P(f[2].view)), "bad channel count"),
        ("pxa_vae_grid_to_nchw", (grid(x), 3, None), "bad channel count"),
        ("pxa_vae_conv3x3_small_out", (grid(x),) + none + (0, P(taps), None, 5, P(f[2].view)), "must be 1..4"),
        ("pxa_vae_conv3x3_small_out", (grid(x),) + none + (0, P(taps), None, 0, P(f[2].view)), "must be 1..4"),
        ("pxa_vae_conv3x3_small_out", (grid(x, C=32),) + none + (0, P(taps), None, 3, P(f[2].view)), "must be a multiple of 64"),
        ("pxa_vae_conv3x3_small_out", (grid(x), P(v), P(v), P(v), P(v), 32, 1, P(taps), None, 3, P(f[2].view)), "must be a multiple of 4"),
    ]
    for name, args, msg in refused:
        with pytest.raises(PixartHipError, match=rf"{name} failed \(rc=-1\): .*{msg}"):
            lib.call(name, *args)
    torch.cuda.synchronize()
    for b in f + [o16]:
        b.assert_untouched("refused calls")
    for g in (y, y2):
        assert (g.whole.view(torch.int16) == g.init).all(), "a refused call wrote its output grid"
    assert {n for n, _, _ in refused} == {n for n in lib.SIGNATURES if n.startswith("pxa_vae_") and n != "pxa_vae_attn"}


# ------------------------------------------------------------------------------------------------ the fp16-operand build
def test_f16_build_runs_this_file():
    """This file again, in a fresh process under the fp16-operand library (one operand type per process), with the bounds of that type."""
    env = dict(os.environ, PXA_OPERAND_DTYPE="f16")
    env.pop("PXA_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-s", "-p", "no:cacheprovider", "-k", "not f16_build"],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    tail = "\n".join(ln for ln in r.stdout.splitlines() if ("passed" in ln or "failed" in ln or "FAILED" in ln or "Error" in ln))
    print("\n[f16 build] " + tail.replace("\n", "\n[f16 build] "))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert "skipped" not in tail and "passed" in tail, tail
