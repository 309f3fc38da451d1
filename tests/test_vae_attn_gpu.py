"""GPU parity of the streaming VAE mid-block attention (csrc/vae_attn.hip, pxa_vae_attn) through the C ABI, in the operand type of the build under test.

Reference: fp64 softmax(scale * q k^T) v on the GPU from the same 16-bit-rounded inputs.  Bounds, for every case:
  * rel-L2(streaming, fp64) < BF16_TOL = 4e-3, the project's "one bf16 rounding" constant (tests/test_vae_gpu.py), for the bf16 AND the fp16 build;
  * where the scores path exists (H*W a multiple of 8): rel-L2(streaming, fp64) <= 1.25 x rel-L2(scores path, fp64) on the same inputs, the scores path being
    the chain AutoencoderKL._attention composes - ops.gemm NT (fp32 scores) -> ops.vae_softmax_rows -> ops.gemm NN.  The 25 % cover the different rounding
    point of P: the streaming kernel rounds exp(s - m), the scores path exp(s - m) / sum.
Sizes: the kernel's tiles are 64 query rows x 32 keys (neither above 128), so the list below crosses every tile edge: 1, one short tile, 31 / 32 / 33 keys,
63 / 64 / 65 query rows (second workgroup), 127 / 128 / 129, 257 and 1000 (many workgroups, tail in both directions)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import record_parity, rel_l2  # noqa: E402

BF16_TOL = 4e-3
MODEL_TOL = 2.5e-2
RATIO = 1.25


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pixart_sigma_amd import ops as o
    return o


def packed(ops, B, HW, C, seed, q_mul=1.0):
    """The (B*HW, 3C) qkv projection as the model holds it, N(0, 1) entries (q times q_mul), in the operand type; its three column slices."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(B * HW, 3 * C, generator=g)
    t[:, :C] *= q_mul
    t = t.cuda().to(ops.BF16)
    return t, t[:, :C], t[:, C:2 * C], t[:, 2 * C:]


def reference(q, k, v, B, HW, scale):
    """fp64 softmax(scale * q k^T) v per image, from the rounded inputs."""
    out = []
    for b in range(B):
        r = slice(b * HW, (b + 1) * HW)
        out.append(torch.softmax(scale * (q[r].double() @ k[r].double().t()), -1) @ v[r].double())
    return torch.cat(out)


def scores_path(ops, q, k, v, B, HW, scale):
    """The parent's path, as AutoencoderKL._attention composes it (one image at a time; H*W a multiple of 8)."""
    C = q.shape[1]
    o = torch.empty(B * HW, C, dtype=ops.BF16, device=q.device)
    s = torch.empty(HW, HW, dtype=torch.float32, device=q.device)
    p = torch.empty(HW, HW, dtype=ops.BF16, device=q.device)
    for b in range(B):
        r = slice(b * HW, (b + 1) * HW)
        ops.gemm(q[r], k[r], ops.NT, out_f32=s)
        ops.vae_softmax_rows(s, scale, out=p)
        ops.gemm(p, v[r], ops.NN, out=o[r])
    return o


def check(ops, label, got, q, k, v, B, HW, scale, want=None):
    """Both bounds of the module docstring; every measured value goes to the parity summary.  Returns the fp64 reference."""
    want = reference(q, k, v, B, HW, scale) if want is None else want
    assert got.shape == want.shape and got.dtype == ops.BF16
    assert torch.isfinite(got.float()).all()
    e = rel_l2(got.float(), want)
    record_parity(f"{label} streaming vs fp64", e, BF16_TOL)
    print(f"\n{label}: streaming rel-L2 {e:.3e} (bound {BF16_TOL:.1e})", end="")
    es = None
    if HW % 8 == 0:
        es = rel_l2(scores_path(ops, q, k, v, B, HW, scale).float(), want)
        record_parity(f"{label} scores path vs fp64", es)
        record_parity(f"{label} streaming / scores", e / es, RATIO)
        print(f", scores path {es:.3e}, ratio {e / es:.3f} (bound {RATIO})", end="")
    assert e < BF16_TOL
    if es is not None:
        assert e <= RATIO * es
    return want


@pytest.mark.parametrize("HW", [1, 7, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 1000])
@pytest.mark.parametrize("B", [1, 3])
def test_sizes_width_512(ops, B, HW):
    C = 512
    _, q, k, v = packed(ops, B, HW, C, seed=HW * 4 + B)
    got = ops.vae_attention(q, k, v, B, HW, C ** -0.5)
    check(ops, f"C{C} B{B} HW{HW}", got, q, k, v, B, HW, C ** -0.5)


@pytest.mark.parametrize("HW", [33, 96, 257])
def test_sizes_width_256(ops, HW):
    B, C = 2, 256
    _, q, k, v = packed(ops, B, HW, C, seed=HW)
    got = ops.vae_attention(q, k, v, B, HW, C ** -0.5)
    check(ops, f"C{C} B{B} HW{HW}", got, q, k, v, B, HW, C ** -0.5)


@pytest.mark.parametrize("spread", [1, 8, 24])
def test_logit_spread(ops, spread):
    """q, k ~ N(0, 1): q . k / sqrt(C) has standard deviation 1; q times `spread` gives the scaled logits that standard deviation (the spreads the
    self-attention tests use: from nearly uniform rows to rows owned by one or two keys)."""
    B, HW, C = 2, 257, 512
    _, q, k, v = packed(ops, B, HW, C, seed=100 + spread, q_mul=float(spread))
    sd = (C ** -0.5 * (q[:HW].double() @ k[:HW].double().t())).std().item()
    assert 0.9 * spread < sd < 1.1 * spread
    got = ops.vae_attention(q, k, v, B, HW, C ** -0.5)
    check(ops, f"spread {spread}", got, q, k, v, B, HW, C ** -0.5)


@pytest.mark.parametrize("at", [0, 256])
def test_one_key_dominates_every_row(ops, at):
    """Every query has mean 1 per channel and key `at` is 0.5 in every channel: its scaled logit is 11.3 +- 0.5 in every row, the others are N(0, 2).  At index 0 the
    running maximum is final after the first tile; at index 256 it moves in the last tile, which holds that one key and 31 masked ones."""
    B, HW, C = 1, 257, 512
    g = torch.Generator().manual_seed(7 + at)
    t = torch.randn(HW, 3 * C, generator=g)
    t[:, :C] += 1.0
    t[at, C:2 * C] = 0.5
    t = t.cuda().to(ops.BF16)
    q, k, v = t[:, :C], t[:, C:2 * C], t[:, 2 * C:]
    logits = C ** -0.5 * (q.double() @ k.double().t())
    assert (logits.argmax(-1) == at).all()
    got = ops.vae_attention(q, k, v, B, HW, C ** -0.5)
    check(ops, f"dominant key at {at}", got, q, k, v, B, HW, C ** -0.5)


def test_packed_inputs_and_strided_output_with_canaries(ops):
    """q, k, v: the column slices of one (B*HW, 3C) tensor (ld = 3C).  out: columns 32 .. 32 + C of a (rows, C + 64) buffer (ldo = C + 64) with 5 rows in front and
    behind: every element outside the slice keeps its canary value."""
    B, HW, C, PAD, CANARY = 3, 65, 512, 5, 7.0
    _, q, k, v = packed(ops, B, HW, C, seed=11)
    assert q.stride(0) == k.stride(0) == v.stride(0) == 3 * C
    buf = torch.full((PAD + B * HW + PAD, C + 64), CANARY, dtype=ops.BF16, device="cuda")
    out = buf[PAD:PAD + B * HW, 32:32 + C]
    assert out.stride(0) == C + 64
    got = ops.vae_attention(q, k, v, B, HW, C ** -0.5, out=out)
    assert got.data_ptr() == out.data_ptr()
    want = check(ops, "packed / strided", got, q, k, v, B, HW, C ** -0.5)
    assert (buf[:PAD] == CANARY).all() and (buf[PAD + B * HW:] == CANARY).all()
    assert (buf[:, :32] == CANARY).all() and (buf[:, 32 + C:] == CANARY).all()
    assert torch.equal(ops.vae_attention(q.contiguous(), k.contiguous(), v.contiguous(), B, HW, C ** -0.5), got)      # strides change nothing
    assert rel_l2(got.float(), want) < BF16_TOL


def test_tail_rows_do_not_leak(ops):
    """B = 1, HW = 33: the second key tile holds one key and 31 masked ones, the first workgroup 31 query rows that are not stored.  The inputs are views of a
    64-row buffer whose rows 33 .. 63 are NaN (inside the allocation: this is about masking, not addressing) - nothing of them reaches the result."""
    HW, C = 33, 512
    t, _, _, _ = packed(ops, 1, 64, C, seed=13)
    t[HW:] = float("nan")
    q, k, v = t[:HW, :C], t[:HW, C:2 * C], t[:HW, 2 * C:]
    got = ops.vae_attention(q, k, v, 1, HW, C ** -0.5)
    assert torch.isfinite(got.float()).all()
    check(ops, "NaN rows behind the image", got, q, k, v, 1, HW, C ** -0.5)


def test_real_shape_memory_and_graph_capture(ops):
    """The 512px mid-block (H*W = 4096, C = 512), two images.  The call allocates its 8 MiB output and nothing else (the scores path: 2 x (64 + 32) MiB here);
    the same launch captured in a graph - one kernel node - and replayed gives the same bits."""
    B, HW, C = 2, 4096, 512
    _, q, k, v = packed(ops, B, HW, C, seed=17)
    ops.vae_attention(q[:64], k[:64], v[:64], 1, 64, C ** -0.5)                 # the kernel's LDS opt-in happens outside the measurement and the capture
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = ops.vae_attention(q, k, v, B, HW, C ** -0.5)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    out_bytes = B * HW * C * 2
    record_parity("real shape: bytes allocated over the call / (output + 1 MiB)", rise / (out_bytes + (1 << 20)), 1.0)
    assert out_bytes == 8 << 20 and rise <= out_bytes + (1 << 20)
    check(ops, f"C{C} B{B} HW{HW}", got, q, k, v, B, HW, C ** -0.5)
    replayed = torch.zeros_like(got)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.vae_attention(q, k, v, B, HW, C ** -0.5, out=replayed)
    replayed.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(replayed, got)


def test_host_checks_launch_nothing(ops):
    from pixart_sigma_amd import lib
    L = lib.load()
    B, HW, C = 1, 32, 512
    _, q, k, v = packed(ops, B, HW, 512, seed=19)
    out = torch.full((B * HW, C), 7.0, dtype=ops.BF16, device="cuda")
    ld = q.stride(0)

    def call(qq=q, oo=out, ldq=ld, width=C):
        return L.pxa_vae_attn(lib.ptr(qq), lib.ptr(k), lib.ptr(v), ldq, ld, ld, lib.ptr(oo) if oo is not None else None, out.stride(0), B, HW, width,
                              width ** -0.5, lib.stream())
    assert call(width=384) == -1 and b"384" in L.pxa_last_error()
    assert call(ldq=C - 8) == -1 and b"stride" in L.pxa_last_error()
    assert call(oo=None) == -1 and b"null" in L.pxa_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    with pytest.raises(lib.PixartHipError):
        ops.vae_attention(q[:, :384], k[:, :384], v[:, :384], B, HW, 384 ** -0.5)
    assert call() == 0                                                          # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert not (out == 7.0).all()


def _pair(cfg, seed):
    from oracle.vae_ref import AutoencoderKLRef, randomize_
    from pixart_sigma_amd.vae import AutoencoderKL
    ref = randomize_(AutoencoderKLRef(**cfg), seed=seed)
    vae = AutoencoderKL(**cfg)
    vae.load_state_dict(ref.state_dict())
    return ref, vae.cuda()


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).cuda()


def test_small_model_streaming_matches_oracle_and_calls_the_kernel_once_per_mid_block(ops, monkeypatch):
    """(128, 256) / one layer per block, B = 2, 16 x 24 image (mid-blocks of 96 tokens, C = 256), as test_autoencoder_decode_and_encode_match_oracle: decode and
    encode in streaming mode against oracle/vae_ref.py; the default mode never reaches ops.vae_attention, streaming reaches it exactly once per mid-block."""
    monkeypatch.delenv("PXA_VAE_ATTN", raising=False)
    ref, vae = _pair(dict(block_out_channels=(128, 256), layers_per_block=1), seed=5)
    B, H, W = 2, 16, 24
    z, x = rnd(B, 4, H // 2, W // 2, seed=6), rnd(B, 3, H, W, seed=7)
    with torch.no_grad():
        want = ref.decode(z.cpu())
        mean, logvar = ref.encode_moments(x.cpu())
    calls, real = [], ops.vae_attention

    def counting(*a, **kw):
        calls.append(a[3:5])
        return real(*a, **kw)
    monkeypatch.setattr(ops, "vae_attention", counting)

    def errors():
        d = rel_l2(vae.decode(z).sample.cpu(), want)
        dist = vae.encode(x).latent_dist
        return d, rel_l2(dist.mean.cpu(), mean), rel_l2(dist.logvar.cpu(), logvar)
    assert vae.attention_mode() == "auto"
    scores = errors()
    assert calls == []
    vae.set_attention("streaming")
    streaming = errors()
    assert calls == [(B, 96), (B, 96)]                                          # one launch over both images per mid-block: the decoder's, the encoder's
    for name, a, b in zip(("decode", "encode mean", "encode logvar"), streaming, scores):
        record_parity(f"small model {name}: streaming", a, MODEL_TOL)
        record_parity(f"small model {name}: scores", b, MODEL_TOL)
        print(f"\nsmall model {name}: streaming {a:.3e}, scores {b:.3e} (bound {MODEL_TOL:.1e})", end="")
    assert max(streaming) < MODEL_TOL
    vae.set_attention("scores")
    errors()
    assert len(calls) == 2


def test_full_architecture_decode_512px_streaming(ops, monkeypatch):
    """Full SD / SDXL architecture, latent (1, 4, 64, 64) -> 512px with the mid-block (4096 tokens, C = 512) on the streaming kernel; fp32 restatement on the GPU."""
    monkeypatch.delenv("PXA_VAE_ATTN", raising=False)
    ref, vae = _pair(dict(), seed=5)
    z = rnd(1, 4, 64, 64, seed=6)
    with torch.no_grad():
        want = ref.cuda().decode(z)
    got = vae.set_attention("streaming").decode(z).sample
    e = rel_l2(got, want)
    record_parity("512px decode, streaming attention, vs fp32 restatement", e, MODEL_TOL)
    print(f"\n512px decode with streaming attention: rel-L2 vs fp32 restatement {e:.2e} (bound {MODEL_TOL:.1e})")
    assert got.shape == (1, 3, 512, 512) and e < MODEL_TOL
