"""pxa_vae_posterior (csrc/vae.hip) and AutoencoderKL.encode_latents: the posterior sample at the end of the encoder in one launch,
    x0 = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * eps),
read from the fp32 moments of quant_conv where the GEMM leaves them (padded-grid layout: origin W + 3, row pitch W + 2, image pitch a multiple of 256 pixel
slots, _c8(2 * latent_channels) floats per slot) and written as fp32 NCHW.

Kernel against fp64.  The moment buffer is a view between guard bands of its own allocation; the bands, every border pixel slot, every slot of an image's tail
and every channel beyond 2 * latent_channels hold NaN, so a read outside the interior shows in the output.  The output is a view between sentinel bands that are
compared bit for bit.  logvar spans -40 .. 30: both clamps act.  Per element
    |x0 - ref| <= 8 * 2^-24 * |scale| * (|mean| + |std * eps|),
ref = the formula in fp64 on the same fp32 inputs and the fp32 value of scale.  The bound is the chain's five roundings (0.5 * logvar is exact; expf <= 1 ulp =
2 units of 2^-24 on std * eps; the product, the sum and the scaling half an ulp = 1 unit each on at most |mean| + |std * eps|): 5 units, with room for expf's
last place.  torch's own fp32 chain measures 4.2 of these units on the CPU over 200,000 draws.

The launch grid is min(ceil(pixels / 256), 2048) blocks of 256 threads, one pixel per thread and pass: 524,288 pixels per pass.  The case (2, 512, 520) has
532,480 pixels, so the last 8,192 are a second pass of the grid-stride loop.

encode_latents against encode: the same launches up to quant_conv, so with sample=False and scale=1 it must EQUAL encode(x).latent_dist.mode() for fp32 x, and
with noise= it must meet the bound above against the moments encode returns.  Both need two encodes of one picture to agree bit for bit.  The picture is
64 x 8, the narrowest the encoder takes (8 = its downsampling factor; 8 x 1 latent pixels, a multiple of 8 for the mid-block attention): one image, fewer than
1024 padded pixel slots, so no convolution epilogue accumulates GroupNorm statistics with atomics and every statistic comes from pxa_vae_gn_stats, whose
blocks fold their partial sums in a fixed order.  (They used to fold them with fp32 LDS atomics: two encodes of this picture then differed by about 1e-3
under the fp16 build - sums of fp16 squares round, in an order that varied - and these two tests failed there.)

Measured on an MI355X (largest |difference| of the latent mode over four encodes and four encode_latents of one picture, every pair):
    1 x 64 x 8, 2 x 64 x 8, 1 x 8 x 64, 2 x 8 x 64     0 in both builds
    1 x 96 x 64, 2 x 96 x 64                           bf16 0 or 2e-2, fp16 2.4e-3 .. 3.7e-3 (statistics from the convolution epilogues' atomics)
The kernel against fp64: worst 2.75 units of the 8, at 2 x 4 x 512 x 520; encode_latents(noise=) against encode's moments 1.23 units.

The file runs again under the fp16-operand build in a child process (one operand type per process)."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

UNIT = 2.0 ** -24
BOUND_UNITS = 8.0
GUARD = 1024                       # floats in front of and behind each buffer (a multiple of 4: the moments stay 16-byte aligned)
SENTINEL = -12345.6789
PASS_PIXELS = 2048 * 256           # pixels one pass of the launch grid covers
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 16, 24), (2, 512, 520)]


def _c8(n):
    return (n + 7) // 8 * 8


def _img_rows(H, W):
    return ((H + 2) * (W + 2) + 255) // 256 * 256


_CASES = {}


def _case(B, h, w, lc):
    """(moments fp32 (B, lc2, h, w) on the host, eps, the padded-grid buffer on the device as (allocation, view))."""
    key = (B, h, w, lc)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * lc + 31 * h + w)
        mean = torch.randn(B, lc, h, w, generator=g) * 3.0
        logvar = torch.rand(B, lc, h, w, generator=g) * 70.0 - 40.0
        if h * w >= 4:                                  # the clamps' own values and the ends of the range
            logvar.view(B, lc, -1)[:, :, :4] = torch.tensor([-40.0, -30.0, 20.0, 30.0])
        eps = torch.randn(B, lc, h, w, generator=g)
        cs, ip = _c8(2 * lc), _img_rows(h, w)
        grid = torch.full((B, ip, cs), float("nan"))
        inner = grid[:, :(h + 2) * (w + 2)].view(B, h + 2, w + 2, cs)
        inner[:, 1:-1, 1:-1, :2 * lc] = torch.cat([mean, logvar], 1).permute(0, 2, 3, 1)
        alloc = torch.full((2 * GUARD + B * ip * cs,), float("nan"))
        alloc[GUARD:GUARD + B * ip * cs] = grid.reshape(-1)
        _CASES[key] = (mean, logvar, eps, alloc.cuda())
    mean, logvar, eps, alloc = _CASES[key]
    cs, ip = _c8(2 * lc), _img_rows(h, w)
    return mean, logvar, eps, alloc, alloc[GUARD:GUARD + B * ip * cs].view(B * ip, cs)


def _banded_out(B, lc, h, w):
    n = B * lc * h * w
    alloc = torch.full((2 * GUARD + n,), SENTINEL, device="cuda")
    return alloc, alloc[GUARD:GUARD + n].view(B, lc, h, w)


def _bands_untouched(alloc, n):
    want = torch.full((GUARD,), SENTINEL).view(torch.int32)
    return torch.equal(alloc[:GUARD].cpu().view(torch.int32), want) and torch.equal(alloc[GUARD + n:].cpu().view(torch.int32), want)


def _ref_and_bound(mean, logvar, eps, scale):
    s = float(torch.tensor(scale, dtype=torch.float32))
    std_eps = torch.exp(0.5 * logvar.double().clamp(-30.0, 20.0)) * eps.double()
    ref = s * (mean.double() + std_eps)
    return ref, BOUND_UNITS * UNIT * abs(s) * (mean.double().abs() + std_eps.abs())


@pytest.mark.parametrize("lc,scale", [(4, 0.13025), (2, -0.18215)])
@pytest.mark.parametrize("B,h,w", SHAPES)
def test_kernel_against_fp64(B, h, w, lc, scale):
    from pixart_sigma_amd import ops
    mean, logvar, eps, alloc, mom = _case(B, h, w, lc)
    if (B, h, w) == SHAPES[-1]:
        assert B * h * w > PASS_PIXELS, "the large case must need a second pass of the launch grid"
    before = alloc.clone()
    oalloc, out = _banded_out(B, lc, h, w)
    got = ops.vae_posterior(mom, B, h, w, lc, eps=eps.cuda(), scale=scale, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(alloc.view(torch.int32), before.view(torch.int32)), "the kernel wrote its input"
    assert _bands_untouched(oalloc, out.numel()), "a write outside x0"
    x0 = out.cpu()
    assert torch.isfinite(x0).all(), "NaN or inf in x0: a border slot, a spare channel or a guard band was read"
    ref, bound = _ref_and_bound(mean, logvar, eps, scale)
    units = ((x0.double() - ref).abs() / (bound / BOUND_UNITS)).max().item()
    print(f"\nposterior {(B, lc, h, w)} scale {scale}: worst error {units:.2f} units of 2^-24 |scale| (|mean| + |std eps|) (bound {BOUND_UNITS:g})")
    assert ((x0.double() - ref).abs() <= bound).all(), units


@pytest.mark.parametrize("lc,scale", [(4, 0.13025), (2, -0.18215)])
@pytest.mark.parametrize("B,h,w", SHAPES)
def test_mode_is_mean_times_scale_exactly(B, h, w, lc, scale):
    from pixart_sigma_amd import ops
    mean, _, _, _, mom = _case(B, h, w, lc)
    oalloc, out = _banded_out(B, lc, h, w)
    ops.vae_posterior(mom, B, h, w, lc, eps=None, scale=scale, out=out)
    torch.cuda.synchronize()
    assert _bands_untouched(oalloc, out.numel())
    assert torch.equal(out.cpu(), mean * torch.tensor(scale, dtype=torch.float32))


def test_bad_arguments_are_refused():
    from pixart_sigma_amd import lib, ops
    from pixart_sigma_amd.lib import PixartHipError, ptr
    _, _, _, _, mom = _case(3, 5, 7, 4)
    oalloc, out = _banded_out(3, 4, 5, 7)
    ip = mom.shape[0] // 3
    for args, msg in (((None, 3, 5, 7, 4, 8, 9, ip, 10, None, 1.0, ptr(out)), "null moments or output"),
                      ((ptr(mom), 3, 5, 7, 4, 8, 9, ip, 10, None, 1.0, None), "null moments or output"),
                      ((ptr(mom), 3, 0, 7, 4, 8, 9, ip, 10, None, 1.0, ptr(out)), "bad shape"),
                      ((ptr(mom), 3, 5, 7, 5, 8, 9, ip, 10, None, 1.0, ptr(out)), "channel stride"),
                      ((ptr(mom.view(-1)[1:]), 3, 5, 7, 4, 8, 9, ip, 10, None, 1.0, ptr(out)), "16-byte aligned"),
                      ((ptr(mom), 3, 5, 7, 4, 8, 6, ip, 10, None, 1.0, ptr(out)), "bad pitches"),
                      ((ptr(mom), 3, 5, 7, 4, 8, 9, 30, 10, None, 1.0, ptr(out)), "bad pitches")):
        with pytest.raises(PixartHipError, match=rf"pxa_vae_posterior failed \(rc=-1\): .*{msg}"):
            lib.call("pxa_vae_posterior", *args)
    torch.cuda.synchronize()
    assert _bands_untouched(oalloc, out.numel()) and (out.cpu() == SENTINEL).all(), "a refused call wrote"
    with pytest.raises(AssertionError, match="eps must be fp32 NCHW"):
        ops.vae_posterior(mom, 3, 5, 7, 4, eps=torch.zeros(3, 4, 7, 5, device="cuda"))


# ------------------------------------------------------------------------------------------------ encode_latents against encode
@pytest.fixture(scope="module")
def vae_and_picture():
    from oracle.vae_ref import AutoencoderKLRef, randomize_
    from pixart_sigma_amd.vae import AutoencoderKL
    cfg = dict(block_out_channels=(128, 256, 512, 512), layers_per_block=2)
    vae = AutoencoderKL(**cfg)
    vae.load_state_dict(randomize_(AutoencoderKLRef(**cfg), seed=5).state_dict())
    x = torch.rand(1, 3, 64, 8, generator=torch.Generator().manual_seed(3)) * 2 - 1
    return vae.cuda(), x.cuda()


def test_encode_latents_mode_equals_encode_mode(vae_and_picture):
    vae, x = vae_and_picture
    want = vae.encode(x).latent_dist.mode()
    got = vae.encode_latents(x, scale=1, sample=False)
    assert got.dtype == torch.float32 and got.shape == (1, 4, 8, 1) and got.is_contiguous()
    assert torch.equal(got, want)
    assert torch.equal(vae.encode_latents(x, sample=False), want * torch.tensor(vae.config.scaling_factor, dtype=torch.float32))


def test_encode_latents_with_noise_against_encode_moments(vae_and_picture):
    vae, x = vae_and_picture
    mean, logvar = vae.encode(x).latent_dist.parameters.cpu().chunk(2, dim=1)
    eps = torch.randn(1, 4, 8, 1, generator=torch.Generator().manual_seed(4))
    got = vae.encode_latents(x, noise=eps.cuda()).cpu()
    ref, bound = _ref_and_bound(mean, logvar, eps, vae.config.scaling_factor)
    units = ((got.double() - ref).abs() / (bound / BOUND_UNITS)).max().item()
    print(f"\nencode_latents(noise=) against encode's moments: worst error {units:.2f} units (bound {BOUND_UNITS:g})")
    assert ((got.double() - ref).abs() <= bound).all(), units
    # the noise the method draws itself is torch.randn's on the device, from the generator given
    g = torch.Generator(device="cuda").manual_seed(11)
    a = vae.encode_latents(x, generator=g)
    drawn = torch.randn((1, 4, 8, 1), generator=torch.Generator(device="cuda").manual_seed(11), device="cuda", dtype=torch.float32)
    assert torch.equal(a, vae.encode_latents(x, noise=drawn))


# ------------------------------------------------------------------------------------------------ the fp16-operand build
def test_f16_build_runs_this_file():
    env = dict(os.environ, PXA_OPERAND_DTYPE="f16")
    env.pop("PXA_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-s", "-p", "no:cacheprovider", "-k", "not f16_build"],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    tail = "\n".join(ln for ln in r.stdout.splitlines() if ("passed" in ln or "failed" in ln or "FAILED" in ln or "Error" in ln))
    print("\n[f16 build] " + tail.replace("\n", "\n[f16 build] "))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
