"""The small hand-written kernels - KV compression (csrc/kvcompress.hip), the token boundary (csrc/embed.hip) and the flat-buffer optimizer kernels
(csrc/optim.hip) - at the sizes where their guards, second trips and cross-block flushes run; tests/test_kernels_gpu.py launches each of them at one shape
that divides every blocking evenly.  Helpers and band conventions: tests/test_gemm_grad_forms_gpu.py.

References: fp64 torch on the CPU from the same operand-rounded inputs the kernel reads - F.conv2d + F.layer_norm + autograd (compression), F.conv2d +
autograd (patch embedding), an explicit AdamW recurrence (optimizer), plain indexing for the copies.  None of them goes through the library.  The plain
functions `kv_compress_ref`, `patch_embed_ref`, `unpatchify_ref`, `gather_rows_ref` and `adamw_ref` run on any device; tests/test_host_logic.py holds them
against tests/fake_ops.py (shapes) and torch.optim.AdamW in fp64 (values) without a GPU.

Blocking, from the sources:
  kv_compress_fwd   one 32-lane half-wave per compressed token, 8 tokens per 256-thread block; `row >= total` retires half-waves of the last block
  kv_compress_bwd   KB_ROWS = 64 compressed tokens per block, parameter gradients summed in (3 + sr * sr) * C floats of dynamic LDS and flushed with one
                    global atomic per element and block; sr = 4 needs 87,552 bytes, more than a launch gets without the opt-in
  kv_pick           one block per compressed token
  patch_embed_fwd   PE_TOK = 32 tokens per block;  patch_embed_bwd  PB_TOK = 256 tokens per block, one global atomic per element and block
  unpatchify / patchify_bwd   256 elements per block, `idx >= total` guard
  gather_rows       one block per row, 256 threads x float4 = 1024 columns per trip
  optimizer         grid_for(n4) = min(4096, ceil(n4 / 256)) blocks of 256 threads, one float4 per thread and trip: a trip of the grid-stride loop covers
                    TRIP = 4096 * 256 * 4 = 4,194,304 floats, whatever n is.  scale_copy caps its grid at 2048 blocks per strided block: 2,097,152 floats.

Bounds (none new): 16-bit outputs BF16_TOL for the whole tensor and the worst row; compression parameter gradients 1e-4, patch embedding 1e-6 forward and
1e-5 on dw / db, sumsq 1e-5 (test_kernels_gpu.py).  Gradients that a call adds into are compared on the ADDED part (result minus what was there before).
AdamW has no fixed bound: torch.optim.AdamW in fp32 on the same inputs is measured against the same fp64 recurrence, and the kernel gets 4 x that, per
quantity and per region (both are fp32 evaluations of one recurrence in a different operation order).

Guard bands.  Every tensor a kernel writes is a Banded view in the middle of one flat allocation (a fixed bit pattern in front and behind: at least four
rows of the view, 256 elements for a flat one, so the view keeps its 16-byte alignment); tensors a kernel adds into have bands of -0.0.  Where a kernel writes only part of a buffer (the k / v slice of dqkv, the tokens the floor of H / sr, W / sr covers) the rest holds
SENTINEL16 and is compared bit for bit as well."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from conftest import record_parity, rel_l2  # noqa: E402
from test_gemm_grad_forms_gpu import MINUS_ZERO32, SENTINEL16, SENTINEL32, Banded, worst_row  # noqa: E402
from test_kernels_gpu import BF16_TOL, _opd, ops  # noqa: E402,F401

C = 1152
LN_EPS = 1e-5
FWD_ROWS_PER_BLOCK = 8          # kv_compress_fwd_kernel: one half-wave per compressed token
KB_ROWS = 64                    # kv_compress_bwd_kernel
PE_TOK, PB_TOK = 32, 256        # patch_embed_fwd_kernel / patch_embed_bwd_kernel
GRID_CAP, THREADS = 4096, 256   # csrc/optim.hip: grid_for
TRIP = GRID_CAP * THREADS * 4   # floats one trip of a grid-stride loop covers (one float4 per thread)
KV_GRAD_TOL, PE_FWD_TOL, PE_GRAD_TOL, SUMSQ_TOL = 1e-4, 1e-6, 1e-5, 1e-5


def crnd(*shape, scale=1.0, seed=0):
    """N(0, scale) fp32 on the CPU: the fp64 references are computed there, the kernels get .cuda() copies."""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def banded(shape, dtype, fill, init=None):
    """(Banded, view of `shape`) over one flat allocation: bands of at least four rows of the view (256 elements for a flat or very wide one)."""
    guard = max(256, 4 * shape[-1]) if len(shape) > 1 and shape[-1] <= 8192 else 256
    b = Banded(math.prod(shape), 1, dtype, fill, guard=guard)
    v = b.view.view(shape)
    assert v.data_ptr() % 16 == 0
    if torch.is_tensor(init):
        v.copy_(init.view(shape))
    elif init is not None:
        v.fill_(init)
    return b, v


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


# ------------------------------------------------------------------------------------------------ references (plain functions, any device)
def kv_compress_ref(x, cw, cb, lw, lb, B, H, W, sr, eps=LN_EPS):
    """x (B, H * W, C) -> (B, (H // sr) * (W // sr), C) in fp64: depthwise Conv2d(kernel = stride = sr) over the token grid, affine LayerNorm."""
    Cc = x.shape[-1]
    t = x.double().reshape(B, H, W, Cc).permute(0, 3, 1, 2)
    t = F.conv2d(t, cw.double(), cb.double(), stride=sr, groups=Cc).flatten(2).transpose(1, 2)
    return F.layer_norm(t, (Cc,), lw.double(), lb.double(), eps=eps)


def kv_pick_ref(x, B, H, W, sr):
    """x (B, H * W, C) -> the tokens (r * sr, c * sr), r < H // sr, c < W // sr."""
    nH, nW = H // sr, W // sr
    return x.reshape(B, H, W, -1)[:, :nH * sr:sr, :nW * sr:sr].reshape(B, nH * nW, -1)


def covered_tokens(H, W, sr):
    """bool (H * W,): the tokens inside the (H // sr * sr) x (W // sr * sr) corner that the compression reads."""
    m = torch.zeros(H, W, dtype=torch.bool)
    m[:H // sr * sr, :W // sr * sr] = True
    return m.flatten()


def patch_embed_ref(x, w, bias, pos):
    """x (B, 4, Hl, Wl), w (D, 4, 2, 2), pos (N, D) -> (B, N, D) in fp64."""
    return F.conv2d(x.double(), w.double(), bias.double(), stride=2).flatten(2).transpose(1, 2) + pos.double()


def unpatchify_ref(lin, B, h, w, Co):
    return torch.einsum("nhwpqc->nchpwq", lin.view(B, h, w, 2, 2, Co)).reshape(B, Co, 2 * h, 2 * w)


def gather_rows_ref(src, row_idx, L, alt=None, drop=None):
    """src (B * L, Cw), row_idx (rows,) -> (rows, Cw): row b * L + l of src, or row l of alt where drop[b]."""
    idx = row_idx.long()
    out = src[idx]
    if alt is not None and drop is not None:
        out = torch.where(drop.bool()[idx // L, None], alt[idx % L], out)
    return out


def adamw_ref(p0, grads, lr, b1, b2, eps, wd):
    """torch.optim.AdamW's recurrence written out, in fp64: (p - p0, m, v) after one step per gradient."""
    p = p0.double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for t, g in enumerate(grads, 1):
        g = g.double()
        p = p * (1.0 - lr * wd)
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        p = p - (lr / (1.0 - b1 ** t)) * m / (v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps)
    return p - p0.double(), m, v


# ------------------------------------------------------------------------------------------------ KV compression
# (B, H, W, sr, what it reaches)
KV_SHAPES = [(3, 10, 6, 2, "fwd_partial_block"), (2, 18, 10, 2, "bwd_two_blocks"), (1, 9, 7, 2, "floor"), (2, 12, 20, 4, "lds_optin"),
             (1, 9, 6, 3, "nine_taps"), (1, 3, 5, 1, "one_tap")]


def kv_id(s):
    return f"B{s[0]}_{s[1]}x{s[2]}_sr{s[3]}"


def assert_kv_shape(B, H, W, sr, why):
    """the property each shape is in the table for, from the blocking constants"""
    rows = B * (H // sr) * (W // sr)
    if why == "fwd_partial_block":
        assert rows % FWD_ROWS_PER_BLOCK != 0 and rows % 2 == 1      # the last row shares its wave with a half-wave that has none
    elif why == "bwd_two_blocks":
        assert KB_ROWS < rows <= 2 * KB_ROWS and rows % KB_ROWS != 0
    elif why == "floor":
        assert H % sr != 0 and W % sr != 0
    elif why == "lds_optin":
        assert (3 + sr * sr) * C * 4 > 65536
    return rows


def kv_params(sr, seed=20):
    cw, cb = 0.25 + crnd(C, 1, sr, sr, scale=0.05, seed=seed), crnd(C, scale=0.05, seed=seed + 1)
    lw, lb = 1 + crnd(C, scale=0.05, seed=seed + 2), crnd(C, scale=0.05, seed=seed + 3)
    return cw, cb, lw, lb


@pytest.mark.parametrize("shape", KV_SHAPES, ids=kv_id)
def test_kv_compress_fwd_edges(ops, shape):
    """pxa_kv_compress_fwd on the k and the v slice of a qkv buffer: whole output and worst compressed token against fp64, bands around the output."""
    B, H, W, sr, why = shape
    rows = assert_kv_shape(B, H, W, sr, why)
    N, Nk = H * W, rows // B
    qkv = crnd(B, N, 3 * C, seed=1).to(_opd())
    par = kv_params(sr)
    qkv_d, par_d = qkv.cuda(), [t.cuda() for t in par]
    for name, lo in (("k", C), ("v", 2 * C)):
        band, out = banded((B, Nk, C), _opd(), SENTINEL16)
        ops.call("pxa_kv_compress_fwd", ops.ptr(qkv_d[..., lo:lo + C]), N * 3 * C, 3 * C, *(ops.ptr(t) for t in par_d), ops.ptr(out), B, H, W, C, sr, LN_EPS)
        torch.cuda.synchronize()
        band.assert_intact(f"kv_compress_fwd {name}")
        ref = kv_compress_ref(qkv[..., lo:lo + C], *par, B, H, W, sr)
        got = out.cpu().float()
        assert torch.isfinite(got).all()
        e, er = rel_l2(got, ref), worst_row(got.reshape(rows, C), ref.reshape(rows, C))
        print(f"\n[kv_compress_fwd {kv_id(shape)} {name}] whole {e:.2e}  worst row {er:.2e}  (bound {BF16_TOL:.0e})")
        record_parity(f"kv_compress_fwd {name} whole", e, BF16_TOL)
        record_parity(f"kv_compress_fwd {name} worst row", er, BF16_TOL)
        assert e < BF16_TOL and er < BF16_TOL, (name, e, er)
    assert torch.equal(ops.kv_compress_fwd(qkv_d[..., 2 * C:], N * 3 * C, 3 * C, *par_d, B, H, W, C, sr), out)     # the wrapper makes the same call


@pytest.mark.parametrize("shape", KV_SHAPES, ids=kv_id)
def test_kv_compress_bwd_edges(ops, shape):
    """pxa_kv_compress_bwd as engine.py's block backward calls it: once for the k and once for the v slice of one dqkv buffer, both into the same four
    parameter gradients, which already hold other gradients.  The added part of each parameter gradient against the sum of the two fp64 references; the
    source-token gradients whole and by worst token; the q slice, every token the floor leaves uncovered, and all bands bit for bit."""
    B, H, W, sr, why = shape
    rows = assert_kv_shape(B, H, W, sr, why)
    N, Nk = H * W, rows // B
    qkv = crnd(B * N, 3 * C, seed=1).to(_opd())
    dyc = {C: crnd(B, Nk, C, seed=6).to(_opd()), 2 * C: crnd(B, Nk, C, seed=7).to(_opd())}
    par = kv_params(sr)
    before = [crnd(*t.shape, scale=0.5, seed=30 + i) for i, t in enumerate(par)]    # d_conv_w, d_conv_b, d_ln_w, d_ln_b
    grads = [banded(tuple(t.shape), torch.float32, MINUS_ZERO32, init=t) for t in before]
    dq_band, dqkv = banded((B * N, 3 * C), _opd(), SENTINEL16)
    qkv_d, par_d = qkv.cuda(), [t.cuda() for t in par]
    for lo, d in dyc.items():
        ops.kv_compress_bwd(d.cuda(), qkv_d[:, lo:lo + C], N * 3 * C, 3 * C, par_d[0], par_d[1], par_d[2], dqkv[:, lo:lo + C], N * 3 * C, 3 * C,
                            *(v for _, v in grads), B, H, W, C, sr)
    torch.cuda.synchronize()
    dq_band.assert_intact("kv_compress_bwd dqkv")
    for (band, _), nm in zip(grads, ("d_conv_w", "d_conv_b", "d_ln_w", "d_ln_b")):
        band.assert_intact(f"kv_compress_bwd {nm}")
    # fp64 reference: the parameters are shared leaves, so autograd sums the two calls' parameter gradients
    leaves = [t.double().requires_grad_(True) for t in par]
    x = {lo: qkv[:, lo:lo + C].double().reshape(B, N, C).requires_grad_(True) for lo in dyc}
    sum((kv_compress_ref(x[lo], *leaves, B, H, W, sr) * dyc[lo].double()).sum() for lo in dyc).backward()
    for (_, got), pre, leaf, nm in zip(grads, before, leaves, ("d_conv_w", "d_conv_b", "d_ln_w", "d_ln_b")):
        added = got.cpu().double().reshape(leaf.shape) - pre.double()
        e = rel_l2(added, leaf.grad)
        print(f"\n[kv_compress_bwd {kv_id(shape)}] {nm} added part {e:.2e}  (bound {KV_GRAD_TOL:.0e})")
        record_parity(f"kv_compress_bwd {nm} added part", e, KV_GRAD_TOL)
        assert e < KV_GRAD_TOL, (nm, e)
    cov = covered_tokens(H, W, sr)
    din = dqkv.cpu().view(B, N, 3 * C)
    for name, lo in (("k", C), ("v", 2 * C)):
        got, ref = din[:, cov, lo:lo + C].float().reshape(-1, C), x[lo].grad[:, cov].reshape(-1, C)
        assert torch.isfinite(got).all() and got.shape[0] == rows * sr * sr
        e, er = rel_l2(got, ref), worst_row(got, ref)
        print(f"\n[kv_compress_bwd {kv_id(shape)}] din {name} whole {e:.2e}  worst token {er:.2e}  (bound {BF16_TOL:.0e})")
        record_parity(f"kv_compress_bwd din {name} whole", e, BF16_TOL)
        record_parity(f"kv_compress_bwd din {name} worst token", er, BF16_TOL)
        assert e < BF16_TOL and er < BF16_TOL, (name, e, er)
        if (~cov).any():
            assert x[lo].grad[:, ~cov].abs().max().item() == 0
    untouched = bits(din)
    assert (untouched[:, :, :C] == SENTINEL16).all(), "the q slice of dqkv was written"
    assert (untouched[:, ~cov, C:] == SENTINEL16).all(), "tokens outside the floor(H / sr) x floor(W / sr) grid were written"


@pytest.mark.parametrize("shape", [KV_SHAPES[2], KV_SHAPES[3]], ids=kv_id)
def test_kv_pick_floor_and_sr4(ops, shape):
    """pxa_kv_pick forward (rows copied out of the k slice) and backward (scattered into the k slice of a buffer of sentinels): bit-exact, nothing else moves."""
    B, H, W, sr, _ = shape
    N, Nk = H * W, (H // sr) * (W // sr)
    qkv = crnd(B * N, 3 * C, seed=1).to(_opd()).cuda()
    k = qkv[:, C:2 * C]
    ref = kv_pick_ref(k, B, H, W, sr)
    band, kc = banded((B, Nk, C), _opd(), SENTINEL16)
    ops.kv_pick(k, kc, N * 3 * C, 3 * C, B, H, W, C, sr)
    torch.cuda.synchronize()
    band.assert_intact("kv_pick forward")
    assert torch.equal(kc, ref)
    band, back = banded((B * N, 3 * C), _opd(), SENTINEL16)
    dkc = crnd(B, Nk, C, seed=8).to(_opd()).cuda()
    ops.kv_pick(dkc, back[:, C:2 * C], N * 3 * C, 3 * C, B, H, W, C, sr, backward=True)
    torch.cuda.synchronize()
    band.assert_intact("kv_pick backward")
    want = torch.full((B, H, W, 3 * C), SENTINEL16, dtype=torch.int16, device="cuda").view(_opd())
    want[:, :H // sr * sr:sr, :W // sr * sr:sr, C:2 * C] = dkc.view(B, H // sr, W // sr, C)
    assert torch.equal(bits(back), bits(want.view(B * N, 3 * C)))


# ------------------------------------------------------------------------------------------------ token boundary
@pytest.mark.parametrize("B,Hl,Wl", [(3, 10, 14), (2, 24, 28)])
def test_patch_embed_tails_and_two_blocks(ops, B, Hl, Wl):
    """T = 105: a forward tail of 9 tokens, pos indexed by tok % N across three samples.  T = 336: two backward blocks (256 + 80), forward tail 16.
    dw / db already hold other gradients; the added part is compared."""
    D, N = 1152, (Hl // 2) * (Wl // 2)
    T = B * N
    assert T % PE_TOK != 0 and (T > PB_TOK) == (B == 2) and T % PB_TOK != 0
    x, w, b, pos = crnd(B, 4, Hl, Wl, seed=1), crnd(D, 4, 2, 2, scale=0.2, seed=2), crnd(D, seed=3), crnd(N, D, seed=4)
    xd = x.cuda()
    band, out = banded((T, D), torch.float32, SENTINEL32)
    ops.patch_embed_fwd(xd, w.cuda(), b.cuda(), pos.cuda(), out=out)
    torch.cuda.synchronize()
    band.assert_intact("patch_embed_fwd")
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = patch_embed_ref(x, wr, br, pos)
    e = rel_l2(out.cpu().view(B, N, D), ref.detach())
    record_parity("patch_embed_fwd", e, PE_FWD_TOL)
    assert e < PE_FWD_TOL, e
    dtok = crnd(T, D, seed=5)
    ref.backward(dtok.double().view(B, N, D))
    pre_w, pre_b = crnd(D, 16, scale=0.5, seed=6), crnd(D, scale=0.5, seed=7)
    (band_w, dw), (band_b, db) = banded((D, 16), torch.float32, MINUS_ZERO32, init=pre_w), banded((D,), torch.float32, MINUS_ZERO32, init=pre_b)
    ops.patch_embed_bwd(xd, dtok.cuda(), dw, db)
    torch.cuda.synchronize()
    band_w.assert_intact("patch_embed_bwd dw")
    band_b.assert_intact("patch_embed_bwd db")
    ew = rel_l2(dw.cpu().double() - pre_w.double(), wr.grad.view(D, 16))
    eb = rel_l2(db.cpu().double() - pre_b.double(), br.grad)
    print(f"\n[patch_embed T={T}] forward {e:.2e} (bound {PE_FWD_TOL:.0e})  dw added {ew:.2e}  db added {eb:.2e}  (bound {PE_GRAD_TOL:.0e})")
    record_parity("patch_embed_bwd dw added part", ew, PE_GRAD_TOL)
    record_parity("patch_embed_bwd db added part", eb, PE_GRAD_TOL)
    assert ew < PE_GRAD_TOL and eb < PE_GRAD_TOL, (ew, eb)


def test_unpatchify_patchify_partial_block(ops):
    """3360 elements = 13 blocks of 256 and one of 32: the `idx >= total` guard of both permutations.  Bit-exact, and the round trip too."""
    B, h, w, Co = 3, 5, 7, 8
    total = B * h * w * 4 * Co
    assert total % 256 != 0
    lin = crnd(B * h * w, 4 * Co, seed=1).cuda()
    ref = unpatchify_ref(lin, B, h, w, Co)
    band, img = banded((B, Co, 2 * h, 2 * w), torch.float32, SENTINEL32)
    ops.call("pxa_unpatchify_fwd", ops.ptr(lin), ops.ptr(img), B, h, w, Co)
    torch.cuda.synchronize()
    band.assert_intact("unpatchify_fwd")
    assert torch.equal(img, ref)
    band, back = banded((B * h * w, 4 * Co), _opd(), SENTINEL16)
    ops.call("pxa_patchify_bwd", ops.ptr(img), ops.ptr(back), B, h, w, Co)
    torch.cuda.synchronize()
    band.assert_intact("patchify_bwd")
    assert torch.equal(back, lin.to(_opd()))
    assert torch.equal(ops.unpatchify_fwd(lin, B, h, w, Co), ref) and torch.equal(ops.patchify_bwd(ref, h, w), lin.to(_opd()))     # the wrappers


@pytest.mark.parametrize("form,Cw", [("inference", 4096), ("drop_all_zero", 4096), ("second_trip", 1028)])
def test_gather_rows_forms(ops, form, Cw):
    """pxa_gather_rows_bf16 without alt / drop (the inference call), with a drop vector that drops nobody, and with a row length of 1024 + 4 (a second trip
    of the column loop with one float4).  Rows come from a non-contiguous index set.  Bit-exact."""
    B, L = 3, 20
    y, alt = crnd(B * L, Cw, seed=1).cuda(), crnd(L, Cw, seed=2).cuda()
    mask = torch.zeros(B, L, dtype=torch.bool)
    mask[0, ::3] = mask[1, 1:3] = mask[1, 17] = mask[2, 5:9] = True
    idx = mask.flatten().nonzero().flatten().to(torch.int32).cuda()
    rows = idx.numel()
    a, drop = {"inference": (None, None), "drop_all_zero": (alt, torch.zeros(B, dtype=torch.int32, device="cuda")),
               "second_trip": (alt, torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda"))}[form]
    assert (Cw > 1024 and Cw % 1024 == 4) == (form == "second_trip")
    band, out = banded((rows, Cw), _opd(), SENTINEL16)
    ops.call("pxa_gather_rows_bf16", ops.ptr(y), ops.ptr(a), ops.ptr(idx), ops.ptr(drop), ops.ptr(out), rows, L, Cw)
    torch.cuda.synchronize()
    band.assert_intact(f"gather_rows {form}")
    ref = gather_rows_ref(y, idx, L, alt=a, drop=drop).to(_opd())
    if form != "second_trip":
        assert torch.equal(ref, y[idx.long()].to(_opd()))
    assert torch.equal(out, ref)
    assert torch.equal(ops.gather_rows_bf16(y, idx, L, alt=a, drop=drop), ref)


# ------------------------------------------------------------------------------------------------ optimizer at grid-stride sizes
# grid_for (csrc/optim.hip) launches min(4096, ceil(n / 4 / 256)) blocks of 256 threads and every thread takes one float4 per trip of
# `for (i = blockIdx.x * 256 + threadIdx.x; i < n / 4; i += gridDim.x * 256)`: from n = TRIP = 4096 * 256 * 4 floats on, the grid is capped and the loop's
# second trip begins at element TRIP.
ADAMW_N = TRIP + 4 * 1000
ADAMW_REGIONS = {"first trip": slice(0, TRIP), "second trip": slice(TRIP, ADAMW_N), "last 4096": slice(ADAMW_N - 4096, ADAMW_N)}
LOSS_SCALE = 65536.0


def _f32(v):
    """the value a `float` argument of the C ABI carries"""
    return torch.tensor(v, dtype=torch.float32).item()


@pytest.fixture(scope="module")
def adamw_case():
    """Inputs of two AdamW steps over TRIP + 4000 floats with the project's hyper-parameters; the fp64 recurrence; and the error of torch.optim.AdamW in fp32
    against it, per quantity (update p - p0, m, v) and region.  All three evaluate the recurrence of the fp32-rounded hyper-parameters: that is what the
    library's `float` arguments carry, so the rounding of 0.9 or 2e-5 to fp32 is an input here and not an error of either implementation."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    n = ADAMW_N
    hp = dict(lr=_f32(2e-5), b1=_f32(0.9), b2=_f32(0.999), eps=_f32(1e-10), wd=_f32(3e-2))
    gs = _f32(0.37)                                                     # the clip coefficient the step multiplies the gradient by
    p0 = crnd(n, seed=1).cuda()
    grads = [crnd(n, scale=0.1, seed=2).cuda(), crnd(n, scale=0.1, seed=3).cuda()]
    ref = adamw_ref(p0, [g.double() * gs for g in grads], **hp)
    pr = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pr], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"])
    for g in grads:
        pr.grad = g * gs                                                # one fp32 rounding, as in the kernel
        opt.step()
    st = opt.state[pr]
    got = (pr.detach().double() - p0.double(), st["exp_avg"], st["exp_avg_sq"])
    torch_err = {(q, r): rel_l2(t[sl], f[sl]) for q, t, f in zip(("update", "m", "v"), got, ref) for r, sl in ADAMW_REGIONS.items()}
    return dict(n=n, hp=hp, gs=gs, p0=p0, grads=grads, ref=ref, torch_err=torch_err)


@pytest.mark.parametrize("entry", ["adamw_step", "adamw_step_scaled"])
def test_adamw_second_trip(ops, adamw_case, entry):
    """pxa_adamw_step with a gradient multiplier, and pxa_adamw_step_scaled with a clean scaler record ([0] loss scale, [1] growth tracker, [2] found_inf = 0,
    [3] applied steps = the step being taken, [4] skipped steps; gradients x 65536 and the multiplier / 65536, both exact), over a full trip of the capped
    grid plus a partial second one.  Update, m and v against the fp64 recurrence on [0, TRIP), [TRIP, n) and the last 4096 elements - a stretch the loop
    skipped has an update error of 1.0 in its region, where the whole-buffer figure would move by 1e-3 - each within 4 x what torch.optim.AdamW in fp32
    measures there.  The shadow weights are the rounded master weights bit for bit; nothing is written behind n."""
    c = adamw_case
    n, hp, opd = c["n"], c["hp"], _opd()
    (band_p, p), (band_m, m), (band_v, v) = (banded((n,), torch.float32, SENTINEL32, init=i) for i in (c["p0"], 0.0, 0.0))
    band_pb, pb = banded((n,), opd, SENTINEL16)
    scaled = entry == "adamw_step_scaled"
    gsc = torch.tensor([c["gs"] / LOSS_SCALE if scaled else c["gs"]], dtype=torch.float32, device="cuda")
    assert gsc.double().item() * (LOSS_SCALE if scaled else 1.0) == c["gs"]
    for t, g in enumerate(c["grads"], 1):
        if scaled:
            sc = torch.tensor([LOSS_SCALE, float(t), 0.0, float(t), 0.0], device="cuda")
            ops.adamw_step_scaled(p, g * LOSS_SCALE, m, v, pb, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], gsc, sc)
            assert sc.tolist() == [LOSS_SCALE, float(t), 0.0, float(t), 0.0]
        else:
            ops.adamw_step(p, g, m, v, pb, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], t, gscale=gsc)
    torch.cuda.synchronize()
    for band, nm in ((band_p, "p"), (band_m, "m"), (band_v, "v"), (band_pb, "p_bf16")):
        band.assert_intact(f"{entry} {nm}")
    got = (p.double() - c["p0"].double(), m, v)
    failed = []
    for q, t, f in zip(("update", "m", "v"), got, c["ref"]):
        assert torch.isfinite(t).all()
        for r, sl in ADAMW_REGIONS.items():
            e, te = rel_l2(t[sl], f[sl]), c["torch_err"][(q, r)]
            print(f"\n[{entry}] {q}, {r}: kernel {e:.3e}  torch fp32 {te:.3e}  (bound 4 x = {4 * te:.3e})")
            record_parity(f"{entry} {q} {r}", e, 4 * te)
            record_parity(f"{entry} {q} {r}: torch.optim.AdamW fp32", te)
            if not e <= 4 * te:
                failed.append((q, r, e, te))
    assert not failed, failed
    assert torch.equal(pb, p.to(opd))


def test_sumsq_second_trip_and_scalar_tail(ops):
    """n = TRIP + 4 * 123 + 3: a second trip of 123 float4 and three elements for the scalar tail.  The tail elements are +-1000 among N(0, 1) data, about
    0.42 of the sum; the second trip is 6.8e-5 of it: leaving either out is outside the bound."""
    n = TRIP + 4 * 123 + 3
    x = crnd(n, seed=1)
    x[-3:] = torch.tensor([1000.0, -1000.0, 1000.0])
    band_x, xd = banded((n,), torch.float32, SENTINEL32, init=x)        # anything read behind n would be 1.5e16
    band_s, s = banded((1,), torch.float32, MINUS_ZERO32, init=0.0)
    ops.sumsq(xd, s)
    torch.cuda.synchronize()
    band_x.assert_intact("sumsq input")
    band_s.assert_intact("sumsq output")
    ref = x.double().pow(2).sum().item()
    assert x[-3:].double().pow(2).sum().item() > 0.4 * ref and x[TRIP:-3].double().pow(2).sum().item() > 5 * SUMSQ_TOL * ref
    e = abs(s.item() - ref) / ref
    record_parity("sumsq second trip + scalar tail", e, SUMSQ_TOL)
    assert e < SUMSQ_TOL, (s.item(), ref, e)


def test_scale_copy_second_trip(ops):
    """The engine's qkv weight copy: two blocks of 3 * 1152 * 1152 floats, 3888 thread blocks' worth each against a grid capped at 2048, the first third
    scaled.  16-bit and fp32 outputs bit-exact."""
    D, nb = 1152, 2
    n_total, n_scaled = 3 * D * D, D * D
    stride = n_total + 256
    assert (n_total // 4 + 255) // 256 > 2048
    src = crnd(nb * stride, seed=9).cuda()
    band16, out = banded((nb, n_total), _opd(), SENTINEL16)
    band32, outf = banded((nb, n_total), torch.float32, SENTINEL32)
    ops.scale_copy(src, stride, nb, n_scaled, n_total, ops.Q_PRESCALE, out_bf16=out)
    ops.scale_copy(src, stride, nb, n_scaled, n_total, ops.Q_PRESCALE, out_f32=outf)
    torch.cuda.synchronize()
    band16.assert_intact("scale_copy 16-bit")
    band32.assert_intact("scale_copy fp32")
    ref = torch.stack([src[b * stride:b * stride + n_total] for b in range(nb)])
    ref[:, :n_scaled] *= torch.tensor(ops.Q_PRESCALE, dtype=torch.float32, device="cuda")
    assert torch.equal(outf, ref)
    assert torch.equal(out, ref.to(_opd()))
