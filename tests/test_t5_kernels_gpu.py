"""GPU parity of the T5 encoder's kernels (csrc/t5.hip: pxa_t5_embed, pxa_t5_rmsnorm, pxa_t5_attn) and of the GeGLU feed-forward through the GEMM epilogues, in
the operand type of the build under test.  Expected values are fp64 formulas on the operand-rounded inputs; 16-bit outputs are bounded by BF16_TOL = 4e-3
rel-L2, the project's one-rounding constant (tests/test_vae_attn_gpu.py), in both builds; fp32 outputs of the norm by 1e-6; the gather is bit-exact.

Attention sizes: the kernel's tiles are 64 query rows x 32 keys, so the cases cross one row, one short tile, a key length of 1 behind a full sample, 300 = 9 tiles
+ 12 keys with a second sample of 137, 64 heads, the largest L (512) and a key length one past a tile edge (33)."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import ROOT, record_parity, rel_l2  # noqa: E402

BF16_TOL = 4e-3
F32_TOL = 1e-6
ATTN_CASES = [(1, 1, 1, [1]), (2, 3, 77, [77, 1]), (2, 4, 300, [300, 137]), (1, 64, 120, [120]), (1, 2, 512, [512]), (2, 2, 64, [33, 64])]
CANARY = 7.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pixart_sigma_amd import ops as o
    return o


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def canaried(rows, cols, dtype, pad=3):
    """A (rows, cols) contiguous view inside a buffer with `pad` canary rows in front and behind."""
    buf = torch.full((rows + 2 * pad, cols), CANARY, dtype=dtype, device="cuda")
    return buf, buf[pad:pad + rows]


def canaries_intact(buf, rows, pad=3):
    return bool((buf[:pad] == CANARY).all() and (buf[pad + rows:] == CANARY).all())


# ------------------------------------------------------------------------------------------------ embedding gather
@pytest.mark.parametrize("D", [128, 4096])
@pytest.mark.parametrize("R", [1, 231, 600])
def test_embed_is_bit_equal_to_the_table_rows(ops, R, D):
    vocab = 97
    table = rnd(vocab, D, seed=R + D).to(ops.BF16)
    ids = torch.randint(0, vocab, (R,), generator=torch.Generator().manual_seed(R)).to(torch.int32)
    ids[0], ids[-1] = vocab - 1, 0
    buf, out = canaried(R, D, torch.float32)
    got = ops.t5_embed(ids.cuda(), table, out=out)
    assert got.data_ptr() == out.data_ptr() and got.dtype == torch.float32
    assert torch.equal(got, table[ids.cuda().long()].float())
    assert canaries_intact(buf, R)
    record_parity(f"embed R{R} D{D}: rows that differ", (got != table[ids.cuda().long()].float()).any(1).sum().item(), 0)


def test_embed_clamps_ids_outside_the_vocabulary(ops):
    """The Python side refuses such ids; the kernel still forms no address outside the table: -5 reads row 0, vocab + 9 row vocab - 1.  (The table is the middle
    of a larger allocation, so this test reads inside one whatever the kernel does.)"""
    vocab, D = 40, 128
    big = rnd(vocab + 32, D, seed=1).to(ops.BF16)
    table = big[16:16 + vocab]
    ids = torch.tensor([-5, 0, vocab - 1, vocab + 9, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32).cuda()
    got = ops.t5_embed(ids, table)
    assert torch.equal(got, table[[0, 0, vocab - 1, vocab - 1, vocab - 1, 0]].float())


# ------------------------------------------------------------------------------------------------ RMS norm
@pytest.mark.parametrize("D", [128, 256, 4096])
@pytest.mark.parametrize("R", [1, 77, 600])
def test_rmsnorm_rows(ops, R, D):
    x = rnd(R, D, seed=3 * R + D) * torch.tensor([1e-3, 1.0, 1e3], device="cuda")[torch.arange(R, device="cuda") % 3][:, None]
    w = 1 + 0.2 * rnd(D, seed=D)
    eps = 1e-6
    want = x.double() * torch.rsqrt(x.double().pow(2).mean(-1, keepdim=True) + eps) * w.double()
    b16, y16 = canaried(R, D, ops.BF16)
    b32, y32 = canaried(R, D, torch.float32)
    got16, got32 = ops.t5_rmsnorm(x, w, eps, out=y16, out_f32=y32)
    assert got16.data_ptr() == y16.data_ptr() and got32.data_ptr() == y32.data_ptr()
    e32, e16 = rel_l2(got32, want), rel_l2(got16.float(), want)
    worst_row = ((got32.double() - want).norm(dim=1) / want.norm(dim=1)).max().item()
    record_parity(f"rmsnorm R{R} D{D} fp32 out vs fp64", e32, F32_TOL)
    record_parity(f"rmsnorm R{R} D{D} fp32 out vs fp64, worst row", worst_row, F32_TOL)
    record_parity(f"rmsnorm R{R} D{D} 16-bit out vs fp64", e16, BF16_TOL)
    print(f"\nrmsnorm R{R} D{D}: fp32 {e32:.2e} (worst row {worst_row:.2e}; bound {F32_TOL:.0e}), 16-bit {e16:.2e} (bound {BF16_TOL:.0e})", end="")
    assert e32 <= F32_TOL and worst_row <= F32_TOL and e16 < BF16_TOL
    assert canaries_intact(b16, R) and canaries_intact(b32, R)
    assert torch.equal(got16, got32.to(ops.BF16))                                     # one rounding of the fp32 result
    only16, none32 = ops.t5_rmsnorm(x, w, eps)
    none16, only32 = ops.t5_rmsnorm(x, w, eps, want_bf16=False, want_f32=True)
    assert none32 is None and none16 is None and torch.equal(only16, got16) and torch.equal(only32, got32)


# ------------------------------------------------------------------------------------------------ attention
def attn_inputs(ops, B, H, L, spread, seed, bias_scale=1.0):
    """The packed (B*L, 3*H*64) projection with N(0, 1) entries, q times spread / 8 (q . k over 64 channels then has standard deviation `spread`: no softmax
    scale in T5), its three column slices, and an fp32 (H, 2L - 1) bias."""
    W = H * 64
    t = rnd(B * L, 3 * W, seed=seed)
    t[:, :W] *= spread / 8.0
    t = t.to(ops.BF16)
    bias = (bias_scale * rnd(H, 2 * L - 1, seed=seed + 1)).contiguous()
    return t, t[:, :W], t[:, W:2 * W], t[:, 2 * W:], bias


def attn_reference(q, k, v, bias, lens, B, H, L):
    """fp64 softmax(q k^T + bias[h][j - i]) v over the first lens[b] keys, for EVERY query row, from the rounded inputs."""
    out = torch.empty(B * L, H * 64, dtype=torch.float64, device=q.device)
    pos = torch.arange(L, device=q.device)
    idx = (pos[None, :] - pos[:, None]) + L - 1
    for b in range(B):
        n = lens[b]
        for h in range(H):
            r, c = slice(b * L, (b + 1) * L), slice(h * 64, (h + 1) * 64)
            s = q[r, c].double() @ k[r, c][:n].double().t() + bias[h].double()[idx][:, :n]
            out[r, c] = torch.softmax(s, -1) @ v[r, c][:n].double()
    return out


def run_attn(ops, q, k, v, bias, lens, B, H, L, **kw):
    return ops.t5_attention(q, k, v, bias, torch.tensor(lens, dtype=torch.int32).cuda(), B, H, L, **kw)


def check_attn(ops, label, got, want):
    assert got.shape == want.shape and got.dtype == ops.BF16
    assert torch.isfinite(got.float()).all()
    e = rel_l2(got.float(), want)
    record_parity(f"{label} vs fp64", e, BF16_TOL)
    print(f"\n{label}: rel-L2 {e:.3e} (bound {BF16_TOL:.1e})", end="")
    assert e < BF16_TOL
    return e


@pytest.mark.parametrize("spread", [1, 8, 24])
@pytest.mark.parametrize("B,H,L,lens", ATTN_CASES)
def test_attention_sizes_and_logit_spreads(ops, B, H, L, lens, spread):
    _, q, k, v, bias = attn_inputs(ops, B, H, L, spread, seed=1000 * L + 10 * H + spread)
    if B * L >= 64:
        sd = (q[:L, :64].double() @ k[:L, :64].double().t()).std().item()
        assert 0.8 * spread < sd < 1.2 * spread
    got = run_attn(ops, q, k, v, bias, lens, B, H, L)
    check_attn(ops, f"attn B{B} H{H} L{L} lens{lens} spread {spread}", got, attn_reference(q, k, v, bias, lens, B, H, L))


@pytest.mark.parametrize("B,H,L,lens", [(2, 3, 77, [77, 1]), (2, 4, 300, [300, 137])])
def test_attention_where_the_bias_alone_picks_every_argmax(ops, B, H, L, lens):
    """bias: the 2L - 1 values of a ramp from -30 to 30, shuffled per head, so neighbouring offsets differ by 60 / (2L - 2) >= 0.1 and no two are equal; q k^T has
    standard deviation 0.005.  Every query's largest logit is then the key whose OFFSET has the largest bias among its valid keys: an off-by-one in the (j - i)
    index or a flipped sign moves every row's weight to another key."""
    W = H * 64
    _, q, k, v, _ = attn_inputs(ops, B, H, L, 0.005, seed=50 + L)
    g = torch.Generator().manual_seed(60 + L)
    ramp = torch.linspace(-30, 30, 2 * L - 1)
    bias = torch.stack([ramp[torch.randperm(2 * L - 1, generator=g)] for _ in range(H)]).cuda().contiguous()
    pos = torch.arange(L, device="cuda")
    idx = (pos[None, :] - pos[:, None]) + L - 1
    for b in range(B):
        for h in range(H):
            r, c = slice(b * L, (b + 1) * L), slice(h * 64, (h + 1) * 64)
            only_bias = bias[h][idx][:, :lens[b]].double()
            full = q[r, c].double() @ k[r, c][:lens[b]].double().t() + only_bias
            assert torch.equal(full.argmax(-1), only_bias.argmax(-1))
    want = attn_reference(q, k, v, bias, lens, B, H, L)
    got = run_attn(ops, q, k, v, bias, lens, B, H, L)
    check_attn(ops, f"attn bias-dominated B{B} H{H} L{L}", got, want)
    shifted = attn_reference(q, k, v, torch.roll(bias, 1, dims=1), lens, B, H, L)     # what an off-by-one would compute: far outside the bound
    flipped = attn_reference(q, k, v, torch.flip(bias, dims=[1]), lens, B, H, L)      # and the other sign of the offset
    assert rel_l2(shifted, want) > 0.3 and rel_l2(flipped, want) > 0.3


def test_attention_packed_slices_and_strided_output_with_canaries(ops):
    """q, k, v: column slices of one packed tensor (ld = 3 H 64).  out: columns 32 .. 32 + H 64 of a wider buffer with canary rows in front and behind: every
    element outside the slice keeps its value, and the result is bit-equal to the call on contiguous copies."""
    B, H, L, lens, PAD = 2, 3, 77, [77, 40], 5
    W = H * 64
    _, q, k, v, bias = attn_inputs(ops, B, H, L, 8, seed=11)
    assert q.stride(0) == k.stride(0) == v.stride(0) == 3 * W
    buf = torch.full((PAD + B * L + PAD, W + 64), CANARY, dtype=ops.BF16, device="cuda")
    out = buf[PAD:PAD + B * L, 32:32 + W]
    got = run_attn(ops, q, k, v, bias, lens, B, H, L, out=out)
    assert got.data_ptr() == out.data_ptr()
    check_attn(ops, "attn packed / strided", got, attn_reference(q, k, v, bias, lens, B, H, L))
    assert (buf[:PAD] == CANARY).all() and (buf[PAD + B * L:] == CANARY).all()
    assert (buf[:, :32] == CANARY).all() and (buf[:, 32 + W:] == CANARY).all()
    assert torch.equal(run_attn(ops, q.contiguous(), k.contiguous(), v.contiguous(), bias, lens, B, H, L), got)


@pytest.mark.parametrize("B,H,L,lens", [(2, 3, 77, [77, 1]), (2, 4, 300, [300, 137]), (2, 2, 64, [33, 64])])
def test_attention_nan_behind_the_key_length_does_not_reach_the_output(ops, B, H, L, lens):
    W = H * 64
    t, q, k, v, bias = attn_inputs(ops, B, H, L, 8, seed=13 + L)
    clean = run_attn(ops, q, k, v, bias, lens, B, H, L)
    for b in range(B):
        t[b * L + lens[b]:(b + 1) * L, W:] = float("nan")                             # K and V rows of the padded positions; their query rows stay
    got = run_attn(ops, q, k, v, bias, lens, B, H, L)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, clean)
    check_attn(ops, f"attn NaN keys B{B} H{H} L{L}", got, attn_reference(q, k, v, bias, lens, B, H, L))


def test_attention_python_binding_refuses_what_the_library_refuses(ops):
    from pixart_sigma_amd import lib
    B, H, L = 1, 2, 16
    _, q, k, v, bias = attn_inputs(ops, B, H, L, 1, seed=3)
    out = torch.full((B * L, H * 64), CANARY, dtype=ops.BF16, device="cuda")
    a = lib.T5AttnArgs()
    a.q, a.k, a.v, a.o = lib.ptr(q), lib.ptr(k), lib.ptr(v), lib.ptr(out)
    a.ldq = a.ldk = a.ldv = q.stride(0)
    a.ldo = out.stride(0)
    a.bias, a.kv_len = lib.ptr(bias), lib.ptr(torch.tensor([L], dtype=torch.int32).cuda())
    a.B, a.H, a.L, a.head_dim = B, H, L, 72
    import ctypes
    assert lib.load().pxa_t5_attn(ctypes.byref(a), lib.stream()) == -1 and b"head_dim=72" in lib.load().pxa_last_error()
    torch.cuda.synchronize()
    assert (out == CANARY).all()
    a.head_dim = 64
    assert lib.load().pxa_t5_attn(ctypes.byref(a), lib.stream()) == 0
    torch.cuda.synchronize()
    assert not (out == CANARY).any()


# ------------------------------------------------------------------------------------------------ GeGLU through the GEMM epilogues
@pytest.mark.parametrize("N,K", [(320, 128), (384, 256)])
@pytest.mark.parametrize("M", [1, 231, 600])
def test_geglu_through_the_gemm_epilogues(ops, M, N, K):
    """The encoder's feed-forward input: h0 = gemm(x, W0, act GELU), g = gemm(x, W1, act MUL_AUX, aux = h0), against fp64 gelu_tanh(x W0^T) * (x W1^T)."""
    x = rnd(M, K, seed=M + N).to(ops.BF16)
    w0, w1 = (rnd(N, K, seed=N + K) * K ** -0.5).to(ops.BF16), (rnd(N, K, seed=N + K + 1) * K ** -0.5).to(ops.BF16)
    h0 = ops.gemm(x, w0, ops.NT, act=ops.ACT_GELU)
    g = ops.gemm(x, w1, ops.NT, act=ops.ACT_MUL_AUX, aux=h0)
    a = x.double() @ w0.double().t()
    want_h = torch.nn.functional.gelu(a, approximate="tanh")
    want = want_h * (x.double() @ w1.double().t())
    eh, eg = rel_l2(h0.float(), want_h), rel_l2(g.float(), want)
    record_parity(f"geglu M{M} N{N} K{K}: gelu(x W0^T) vs fp64", eh, BF16_TOL)
    record_parity(f"geglu M{M} N{N} K{K}: gelu(x W0^T) * (x W1^T) vs fp64", eg, BF16_TOL)
    print(f"\ngeglu M{M} N{N} K{K}: h0 {eh:.2e}, product {eg:.2e} (bound {BF16_TOL:.0e})", end="")
    assert eh < BF16_TOL and eg < BF16_TOL


def test_projection_adds_into_the_fp32_residual(ops):
    """The o / wo form: gemm(out_f32 = x, accumulate) leaves x + a W^T with the product never rounded (bound: fp32 accumulation over K = 320)."""
    M, N, K = 231, 128, 320
    a, w = rnd(M, K, seed=5).to(ops.BF16), (rnd(N, K, seed=6) * K ** -0.5).to(ops.BF16)
    x = rnd(M, N, seed=7)
    want = x.double() + a.double() @ w.double().t()
    ops.gemm(a, w, ops.NT, out_f32=x, accumulate=True)
    e = rel_l2(x, want)
    record_parity("residual accumulate M231 N128 K320 vs fp64", e, 1e-5)
    assert e < 1e-5


# ------------------------------------------------------------------------------------------------ the fp16-operand build
def test_f16_build_runs_this_file():
    """This file again, in a fresh process under the fp16-operand library (one operand type per process), with the same bounds."""
    env = dict(os.environ, PXA_OPERAND_DTYPE="f16")
    env.pop("PXA_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-s", "-p", "no:cacheprovider", "-k", "not f16_build"],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    tail = "\n".join(ln for ln in r.stdout.splitlines() if ("passed" in ln or "failed" in ln or "FAILED" in ln or "Error" in ln))
    print("\n[f16 build] " + tail.replace("\n", "\n[f16 build] "))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert "skipped" not in tail and "passed" in tail, tail
