"""ops.gemm in the forms the training step calls it with an fp32 output or at ragged row counts (pixart_sigma_amd/engine.py: _lin_bwd, the kv_linear input
gradient into ctx["dye"], the final layer, the caption branch), at the shapes where pxa_gemm's host-side dispatch changes (csrc/gemm.hip: the (tile, split)
cost model of split_k = 0, the re-derived split count, the four accumulate modes, the paired remainder column of the persistent TN kernel, the register-staged
fallback gemm_kernel whenever K % 64 != 0), with LOCALISED error metrics and guard bands.  The model goldens bound a whole-tensor rel-L2, which one wrong row of
65,536 or the last partial tile of a 2304 x 1152 gradient does not move; tests/test_local_metrics.py is the standing proof.

Reference everywhere: the fp64 matmul of the operand-rounded inputs, on the GPU (no product here is larger than 65,536 x 1152).
Bounds (none new): fp32 outputs 2e-5 (test_kernels_gpu.py, header) for the whole tensor AND the worst 128 x 128 block AND the worst row; 16-bit outputs BF16_TOL
for the whole tensor and the worst row.  Why the same bound holds locally (CPU experiment with the reference alone): one rounding of N(0,1) data gives a worst
row over 65,536 rows of 1.85e-3 (bf16) / 2.3e-4 (fp16) at 1152 columns and 2.8e-3 / 3.5e-4 at 32 columns, against 4e-3 / 5e-4; an fp32 matmul against fp64 at
K = 371 / 4800 / 16384 has whole-tensor 1.3 / 1.5 / 1.8e-7 and its worst 128 x 128 tile and worst row within 1.1 x of that.

Guard bands.  Every tensor a kernel writes is a view into a larger tensor of the same allocation (GUARD rows in front and behind, and GUARD columns on both
sides where ld > N); the bands are compared bit for bit afterwards.  Plainly stored outputs: bands of a fixed bit pattern (SENTINEL16 / SENTINEL32).  Outputs a
kernel adds into (accumulate=True: atomics, read-modify-write, or the split-K reduce): bands of -0.0, which a stray add of +0.0 - what a masked lane contributes -
turns into +0.0 where any other sentinel would survive it (positive control: test_vae_conv_geometry_gpu.py::test_masked_statistics_adds_clear_the_sign_of_minus_zero).
GUARD = 256 = the largest tile edge, so a stray tile lands inside the allocation.

Each case asserts, in Python, the shape condition of the launcher branch it is there for (BK, the 1024 / 256 thresholds), so that a change of those constants
cannot silently move it off its edge.

Census: engine.py call site -> test
  _lin_bwd  gemm(dy, x, TN, out_f32=grad, accumulate, split_k=0)      test_weight_gradient_accumulate (ragged text rows, cost model, M = 32, remainder column)
  pxa_gemm's split count, modes 1 / 2 / 3                              test_explicit_split_counts, test_atomic_accumulate_when_workspace_is_short
  plain fp32 store                                                     test_plain_store_f32
  a C-ABI caller's ld_f32 > N                                          test_f32_output_column_slice
  block_bwd kv_linear dx  gemm(dkvc, W, NN, out_f32=dye, accumulate)   test_kv_linear_input_gradient_f32
  forward   final layer   gemm(xn, W, NT, bias, out_dtype=F32)         test_final_layer_f32
  backward  final layer   _lin_bwd -> gemm(dlin, W, NN), K = 32        test_final_layer_input_gradient
  caption_fwd  fc1        gemm(yb, W, NT, bias, GELU_SAVE_GRAD, out2)  test_caption_fc1_forward_ragged_rows
  caption_bwd  fc2 dx     gemm(dye, W, NN, MUL_AUX, aux=hpre)          test_caption_fc2_input_gradient_ragged_rows"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from conftest import record_parity, rel_l2  # noqa: E402
from test_kernels_gpu import BF16_TOL, _gpu_rnd, _opd, bf, ops, rnd  # noqa: E402,F401

F32_TOL = 2e-5            # fp32 GEMM outputs (test_kernels_gpu.py, header)
BK = 64                   # csrc/gemm.hip: the k-tile; K % BK != 0 -> the register-staged fallback gemm_kernel
GUARD = 256               # rows / columns of a band: one 256 x 256 tile
SENTINEL16 = 0x5A5A       # bf16 1.5e16, fp16 203.25
SENTINEL32 = 0x5A5A5A5A   # fp32 1.5e16
MINUS_ZERO32 = -(1 << 31)


# ------------------------------------------------------------------------------------------------ shared helpers (test_row_kernel_forms_gpu.py imports them)
def _block_sums(t, rows, cols):
    M, N = t.shape
    t = F.pad(t, (0, -N % cols, 0, -M % rows))
    return t.view(t.shape[0] // rows, rows, t.shape[1] // cols, cols).sum((1, 3))


def worst_block(got, ref, rows, cols):
    """max over the rows x cols blocks of a 2-D pair (ragged last blocks included) of the block's rel-L2, in fp64."""
    assert got.dim() == 2 and got.shape == ref.shape, (got.shape, ref.shape)
    r = ref.double()
    d2, r2 = _block_sums((got.double() - r).square(), rows, cols), _block_sums(r.square(), rows, cols)
    return (d2 / r2.clamp_min(1e-60)).sqrt().max().item()


def worst_row(got, ref):
    return worst_block(got, ref, 1, ref.shape[1])


class Banded:
    """A (rows, cols) view in the middle of a larger tensor of one allocation: GUARD rows in front and behind, GUARD columns on both sides if col_bands.
    The bands hold the bit pattern `fill`; assert_intact compares them bit for bit."""

    def __init__(self, rows, cols, dtype, fill, col_bands=False, guard=GUARD):
        self.bits = {2: torch.int16, 4: torch.int32}[torch.empty(0, dtype=dtype).element_size()]
        self.fill, self.g, self.c0 = fill, guard, guard if col_bands else 0
        self.rows, self.cols = rows, cols
        self.whole = torch.full((rows + 2 * guard, cols + 2 * self.c0), fill, dtype=self.bits, device="cuda").view(dtype)
        self.view = self.whole[guard:guard + rows, self.c0:self.c0 + cols]

    def assert_intact(self, what):
        b, g, c0 = self.whole.view(self.bits), self.g, self.c0
        for name, band in (("in front of", b[:g]), ("behind", b[g + self.rows:]), ("left of", b[g:g + self.rows, :c0]), ("right of", b[g:g + self.rows, c0 + self.cols:])):
            bad = band != self.fill
            assert not bad.any(), f"{what}: {int(bad.sum())} elements {name} the output were written (first at {bad.nonzero()[0].tolist()} of that band)"


def check_f32(label, got, ref, bound=F32_TOL):
    """whole tensor, worst 128 x 128 block and worst row of an fp32 result against fp64, all at `bound`."""
    assert torch.isfinite(got).all(), f"{label}: the output holds {int((~torch.isfinite(got)).sum())} non-finite values"
    e, eb, er = rel_l2(got, ref), worst_block(got, ref, 128, 128), worst_row(got, ref)
    print(f"\n[{label}] whole {e:.2e}  worst 128x128 block {eb:.2e}  worst row {er:.2e}  (bound {bound:.0e})")
    record_parity(f"{label} whole", e, bound)
    record_parity(f"{label} worst 128x128 block", eb, bound)
    record_parity(f"{label} worst row", er, bound)
    assert e < bound and eb < bound and er < bound, (label, e, eb, er, bound)


def check_16(label, got, ref, bound=None):
    """whole tensor and worst row of a 16-bit result against fp64, at BF16_TOL."""
    bound = BF16_TOL if bound is None else bound
    assert torch.isfinite(got).all(), f"{label}: the output holds {int((~torch.isfinite(got)).sum())} non-finite values"
    e, er = rel_l2(got, ref), worst_row(got, ref)
    print(f"\n[{label}] whole {e:.2e}  worst row {er:.2e}  (bound {bound:.0e})")
    record_parity(f"{label} whole", e, bound)
    record_parity(f"{label} worst row", er, bound)
    assert e < bound and er < bound, (label, e, er, bound)


def poison_splitk_workspace(ops, a, M, N):
    """The cached split-K slab workspace of a's device, as ops.gemm would size it, filled with NaN: a slab cell that a slice does not write then reaches
    the output through splitk_reduce_kernel."""
    ws = ops._SPLITK_WS.get(a.device)
    if ws is None or ws.numel() < 16 * M * N:
        ws = ops._SPLITK_WS[a.device] = torch.empty(16 * M * N, dtype=torch.float32, device=a.device)
    ws.fill_(float("nan"))
    return ws


def surviving_slices(K, split_k):
    """pxa_gemm's re-derivation: slices of ceil(K / split_k) rounded up to BK; how many of them hold a k at all."""
    kps = ((K + split_k - 1) // split_k + BK - 1) // BK * BK
    return (K + kps - 1) // kps, kps


def plan_of(ops, a, b, layout, **kw):
    """ops.gemm_plan of a call as a dict: "kernel" = the instance as its template is written, the other fields as integers."""
    w = ops.gemm_plan(a, b, layout, **kw).split()
    return dict(kernel=w[0], **{k: int(v) for k, v in (kv.split("=") for kv in w[1:])})


def tn_operands(M, N, K):
    """dW[M][N] = sum_k A[k][M] B[k][N]: (a, b, fp64 reference)."""
    a, b = bf(_gpu_rnd(K, M, seed=1)), bf(_gpu_rnd(K, N, seed=2))
    return a, b, a.double().t() @ b.double()


def accumulate_twice(ops, label, a, b, layout, out, ref, split_k, poison):
    """out (a Banded of -0.0 bands) starts as a random fp32 g0 - a gradient buffer is never zero on the second micro-step; two accumulating calls, (out - g0)
    against the fp64 product after each."""
    M, N = ref.shape
    g0 = _gpu_rnd(M, N, seed=9)
    out.view.copy_(g0)
    for n in (1, 2):
        if poison:
            poison_splitk_workspace(ops, a, M, N)
        got = ops.gemm(a, b, layout, out_f32=out.view, accumulate=True, split_k=split_k)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.view.data_ptr()
        out.assert_intact(f"{label} call {n}")
        check_f32(f"{label} call {n}", out.view.double() - g0.double(), n * ref)


# ------------------------------------------------------------------------------------------------ 1. weight gradients: Engine._lin_bwd
# (M, N, K, class)
WGRAD_CASES = [
    (2304, 1152, 371, "ragged"), (1152, 4096, 371, "ragged"), (1152, 1152, 7, "ragged"), (2304, 1152, 4799, "ragged"),
    (2304, 1152, 4800, "model"), (1152, 4096, 4800, "model"), (1152, 1152, 64, "model"),
    (32, 1152, 4096, "m32"), (32, 1152, 65536, "m32"),
    (1152, 1152, 16384, "rem5"), (2304, 1152, 16384, "rem9"), (3456, 1152, 16384, "rem14"), (1152, 4608, 16384, "norem"),
]


@pytest.mark.parametrize("M,N,K,cls", WGRAD_CASES, ids=lambda v: str(v))
def test_weight_gradient_accumulate(ops, M, N, K, cls):
    """gemm(dy, x, TN, out_f32=grad, accumulate=True, split_k=0), the exact form of Engine._lin_bwd, called twice into a random gradient buffer, the split-K
    workspace poisoned with NaN before each call.
      ragged  K % 64 != 0 (K = the sum of the caption lengths of a ragged batch): the cost model is skipped, one slice, gemm_kernel<2> with the single-slice
              read-modify-write (accumulate mode 2); K = 7 is less than one k-tile.
      model   the same operands with K % 64 == 0: the (tile, split) cost model decides (engine.py, block_bwd: the kv_linear comment).
      m32     final layer, M = 32 < 256: only the 128-tile candidate is legal, 96 of 128 tile rows are beyond M.
      remX    N % 256 == 128: the paired remainder column of the persistent TN kernel, odd (9) and even (14) m-tile counts, at mid K; at 5 m-tiles the cost
              model picks the 128 x 128 kernel instead (asserted below through ops.gemm_plan, as is every kernel this docstring names).
      norem   N % 256 == 0."""
    assert M % 8 == 0 and N % 8 == 0
    if cls == "ragged":
        assert K % BK != 0
    else:
        assert K % BK == 0
    if cls == "m32":
        assert M < 256 and 128 - M == 96
    if cls.startswith("rem"):
        assert 0 < N % 256 <= 128 and M >= 256 and (M + 255) // 256 == int(cls[3:])
    if cls == "norem":
        assert N % 256 == 0 and M >= 256
    a, b, ref = tn_operands(M, N, K)
    out = Banded(M, N, torch.float32, MINUS_ZERO32)
    plan = plan_of(ops, a, b, ops.TN, out_f32=out.view, accumulate=True, split_k=0)
    if cls == "ragged":
        assert (plan["kernel"], plan["split"], plan["accumulate"], plan["splitk_reduce"]) == ("gemm_kernel<2>", 1, 2, 0), plan
    if cls == "m32":
        assert plan["kernel"] == "gemm_glds_kernel<2,128,128,2,2,0,false>", plan
    if cls.startswith("rem"):          # (rem5: the cost model prefers 128 x 128 tiles for 5 x 5 padded 256 tiles at this K; its remainder column is the 128 kernel's)
        assert plan["kernel"] == ("gemm_glds_kernel<2,128,128,2,2,0,false>" if cls == "rem5" else "gemm_pers_kernel<2,0,1,false>"), plan
    if cls == "norem":
        assert plan["kernel"] == "gemm_pers_kernel<2,0,0,false>", plan
    accumulate_twice(ops, f"TN dW {M}x{N} K={K} {cls}", a, b, ops.TN, out, ref, split_k=0, poison=True)


# ------------------------------------------------------------------------------------------------ 2. explicit splits, the re-derived split count
@pytest.mark.parametrize("K,split_k,slices,slice_k", [(4096, 16, 16, 256), (1000, 16, 16, 64), (130, 8, 3, 64), (64, 4, 1, 64)])
def test_explicit_split_counts(ops, K, split_k, slices, slice_k):
    """pxa_gemm re-derives the split count from slices of ceil(K / split_k) rounded up to 64: (1000, 16) keeps 16 slices with a ragged last one (and, K % 64 != 0,
    runs them in the fallback kernel), (130, 8) keeps 3, (64, 4) keeps 1 and so becomes the single-slice read-modify-write; slabs + splitk_reduce_kernel otherwise."""
    M = N = 1152
    assert surviving_slices(K, split_k) == (slices, slice_k) and (slices - 1) * slice_k < K <= slices * slice_k
    a, b, ref = tn_operands(M, N, K)
    out = Banded(M, N, torch.float32, MINUS_ZERO32)
    poison_splitk_workspace(ops, a, M, N)                   # (so that the plan sees the workspace the calls below get)
    plan = plan_of(ops, a, b, ops.TN, out_f32=out.view, accumulate=True, split_k=split_k)
    assert (plan["split"], plan["k_per_split"]) == (slices, slice_k), plan
    assert (plan["accumulate"], plan["splitk_reduce"]) == ((2, 0) if slices == 1 else (3, 1)), plan
    assert plan["kernel"] == ("gemm_kernel<2>" if K % BK else "gemm_pers_kernel<2,0,1,false>"), plan
    accumulate_twice(ops, f"TN {M}x{N} K={K} split_k={split_k} ({slices} slices)", a, b, ops.TN, out, ref, split_k=split_k, poison=True)
    assert ops._SPLITK_WS[a.device].numel() >= slices * M * N


def test_atomic_accumulate_when_workspace_is_short(ops):
    """accumulate mode 1 (atomicAdd straight into the gradient): more surviving slices than the workspace holds.  (K, split_k) = (1088, 17): 17 slices of 64 survive
    the re-derivation (at K = 4096, 17 would collapse to 16 slices of 256); ops.gemm allocates exactly 16 slabs after the cache entry is dropped."""
    M = N = 1152
    K, split_k = 1088, 17
    assert surviving_slices(K, split_k) == (17, 64) and surviving_slices(4096, 17)[0] == 16
    a, b, ref = tn_operands(M, N, K)
    out = Banded(M, N, torch.float32, MINUS_ZERO32)
    saved = ops._SPLITK_WS.pop(a.device, None)
    try:
        accumulate_twice(ops, f"TN {M}x{N} K={K} split_k={split_k} atomics", a, b, ops.TN, out, ref, split_k=split_k, poison=False)
        assert ops._SPLITK_WS[a.device].numel() < 17 * M * N, "the workspace held all 17 slabs: this case did not reach the atomic mode"
        plan = plan_of(ops, a, b, ops.TN, out_f32=out.view, accumulate=True, split_k=split_k)
        assert (plan["split"], plan["accumulate"], plan["splitk_reduce"]) == (17, 1, 0), plan
    finally:
        cur = ops._SPLITK_WS.get(a.device)
        if saved is not None and (cur is None or saved.numel() > cur.numel()):
            ops._SPLITK_WS[a.device] = saved


# ------------------------------------------------------------------------------------------------ 3. plain store
@pytest.mark.parametrize("M,N,K", [(1152, 1152, 512), (32, 1152, 448)])
def test_plain_store_f32(ops, M, N, K):
    """TN into fp32 with accumulate=False: the output, pre-filled with NaN, is overwritten (mode 0), whatever it held."""
    assert K % BK == 0
    a, b, ref = tn_operands(M, N, K)
    out = Banded(M, N, torch.float32, SENTINEL32)
    out.view.fill_(float("nan"))
    ops.gemm(a, b, ops.TN, out_f32=out.view, accumulate=False)
    torch.cuda.synchronize()
    out.assert_intact(f"TN store {M}x{N} K={K}")
    check_f32(f"TN store {M}x{N} K={K}", out.view, ref)


# ------------------------------------------------------------------------------------------------ 4. ld_f32 > N
@pytest.mark.parametrize("M,N,K", [(1152, 1152, 4800), (2304, 1152, 371)])
def test_f32_output_column_slice(ops, M, N, K):
    """The gradient is the column slice [:, 256:256+N] of a wider fp32 tensor (ld_f32 = N + 512, a multiple of 4): what a caller of the C ABI may pass.  Slabs + reduce
    (K % 64 == 0) and the fallback kernel's read-modify-write (K % 64 != 0) both address the output with ld_f32, the slabs with N."""
    out = Banded(M, N, torch.float32, MINUS_ZERO32, col_bands=True)
    assert out.view.stride(0) == N + 2 * GUARD and out.view.stride(0) % 4 == 0 and out.view.stride(0) > N
    a, b, ref = tn_operands(M, N, K)
    accumulate_twice(ops, f"TN dW {M}x{N} K={K} ld={out.view.stride(0)}", a, b, ops.TN, out, ref, split_k=0, poison=True)


# ------------------------------------------------------------------------------------------------ 5. kv_linear input gradient
@pytest.mark.parametrize("M,N,K", [(371, 1152, 2304), (4800, 1152, 2304), (8, 1152, 2304)])
def test_kv_linear_input_gradient_f32(ops, M, N, K):
    """gemm(dkvc, W, NN, out_f32=dye, accumulate=True, split_k=0) (engine.py block_bwd): d(y_emb) of the Ltot packed text rows, accumulated over the blocks
    in fp32.  M = 371 / 8: no 256-tile candidate (M < 256 for 8), a partial last row tile; rows beyond M are banded."""
    assert K % BK == 0 and K % 8 == 0
    dy, w = bf(_gpu_rnd(M, K, seed=1)), bf(_gpu_rnd(K, N, scale=K ** -0.5, seed=2))
    ref = dy.double() @ w.double()
    out = Banded(M, N, torch.float32, MINUS_ZERO32)
    accumulate_twice(ops, f"NN dye {M}x{N} K={K}", dy, w, ops.NN, out, ref, split_k=0, poison=True)


# ------------------------------------------------------------------------------------------------ 6. final layer
@pytest.mark.parametrize("M", [64, 4096, 65536])
def test_final_layer_f32(ops, M):
    """gemm(xn, W, NT, bias, out_dtype=F32) with N = 32 output features, K = 1152: K % 64 == 0 and N < 1024, so the 128 x 128 DMA kernel with 96 of its 128 B rows
    clamped (the existing (130, 32, 72) case takes the fallback kernel, 72 % 64 != 0)."""
    N, K = 32, 1152
    assert K % BK == 0 and N < 1024 and 128 - N == 96
    a, w, b = bf(_gpu_rnd(M, K, seed=1)), bf(_gpu_rnd(N, K, scale=K ** -0.5, seed=2)), _gpu_rnd(N, seed=3)
    ref = a.double() @ w.double().t() + b.double()
    out = Banded(M, N, torch.float32, SENTINEL32)
    out.view.fill_(float("nan"))
    assert plan_of(ops, a, w, ops.NT, bias=b, out_f32=out.view)["kernel"] == "gemm_glds_kernel<0,128,128,2,2,0,false>"
    ops.gemm(a, w, ops.NT, bias=b, out_f32=out.view)
    torch.cuda.synchronize()
    out.assert_intact(f"NT final {M}x{N} K={K}")
    check_f32(f"NT final {M}x{N} K={K}", out.view, ref)
    # the engine's spelling (out_dtype=F32, the wrapper allocates) is the same C call: bit-identical
    assert torch.equal(ops.gemm(a, w, ops.NT, bias=b, out_dtype=torch.float32), out.view)


@pytest.mark.parametrize("M", [4096, 65536])
def test_final_layer_input_gradient(ops, M):
    """_lin_bwd("final_layer.linear"): dxn = gemm(dlin, W, NN, descending=True) with K = 32 output features: K % 64 != 0, so the fallback kernel at
    M >= 1024 and N >= 1024, where every other NN call of the step is a persistent launch."""
    N, K = 1152, 32
    assert K % BK != 0 and K % 8 == 0 and M >= 1024 and N >= 1024
    dy, w = bf(_gpu_rnd(M, K, seed=1)), bf(_gpu_rnd(K, N, scale=K ** -0.5, seed=2))
    ref = dy.double() @ w.double()
    out = Banded(M, N, _opd(), SENTINEL16)
    out.view.fill_(float("nan"))
    assert plan_of(ops, dy, w, ops.NN, out=out.view, descending=True)["kernel"] == "gemm_kernel<1>"
    ops.gemm(dy, w, ops.NN, out=out.view, descending=True)
    torch.cuda.synchronize()
    out.assert_intact(f"NN final dx {M}x{N} K={K}")
    check_16(f"NN final dx {M}x{N} K={K}", out.view, ref)


# ------------------------------------------------------------------------------------------------ 7. caption branch at ragged row counts
def _gelu64(pre):
    x = pre.clone().requires_grad_(True)
    y = F.gelu(x, approximate="tanh")
    y.backward(torch.ones_like(y))
    return y.detach(), x.grad


@pytest.mark.parametrize("M", [371, 4800])
def test_caption_fc1_forward_ragged_rows(ops, M):
    """caption_fwd: gemm(yb, W, NT, bias, act=GELU_SAVE_GRAD, out2=hpre) with M = Ltot packed text rows (odd M is legal for NT / NN), N = 1152, K = 4096:
    the 128-tile kernel below 1024 rows, the persistent kernel's two-output flavour with a half-filled last tile column (N % 256 == 128) above."""
    N, K = 1152, 4096
    assert K % BK == 0 and (M < 1024) == (M == 371) and N % 256 == 128
    a, w, b = bf(_gpu_rnd(M, K, seed=1)), bf(_gpu_rnd(N, K, scale=K ** -0.5, seed=2)), _gpu_rnd(N, seed=3)
    y64, dy64 = _gelu64(a.double() @ w.double().t() + b.double())
    out, out2 = Banded(M, N, _opd(), SENTINEL16), Banded(M, N, _opd(), SENTINEL16)
    out.view.fill_(float("nan"))
    out2.view.fill_(float("nan"))
    call = dict(bias=b, act=ops.ACT_GELU_SAVE_GRAD, out=out.view, out2=out2.view, descending=False)
    assert plan_of(ops, a, w, ops.NT, **call)["kernel"] == ("gemm_glds_kernel<0,128,128,2,2,0,false>" if M < 1024 else "gemm_pers_kernel<0,1,0,false>")
    ops.gemm(a, w, ops.NT, **call)
    torch.cuda.synchronize()
    out.assert_intact(f"NT caption fc1 {M} rows: out")
    out2.assert_intact(f"NT caption fc1 {M} rows: out2")
    check_16(f"NT caption fc1 {M}x{N} K={K} gelu", out.view, y64)
    check_16(f"NT caption fc1 {M}x{N} K={K} gelu'", out2.view, dy64)


@pytest.mark.parametrize("M", [371, 4800])
def test_caption_fc2_input_gradient_ragged_rows(ops, M):
    """caption_bwd: dh = gemm(dye, W, NN, act=MUL_AUX, aux=hpre) without column sums, M = Ltot, N = K = 1152: the 128-tile staged epilogue below 1024 rows, the
    persistent kernel's run-time generic flavour above (MUL_AUX has a flavour of its own only together with colsum)."""
    N = K = 1152
    assert K % BK == 0 and (M < 1024) == (M == 371)
    dy, w, aux = bf(_gpu_rnd(M, K, seed=1)), bf(_gpu_rnd(K, N, scale=K ** -0.5, seed=2)), bf(_gpu_rnd(M, N, seed=5))
    ref = (dy.double() @ w.double()) * aux.double()
    out = Banded(M, N, _opd(), SENTINEL16)
    out.view.fill_(float("nan"))
    call = dict(act=ops.ACT_MUL_AUX, aux=aux, out=out.view, descending=False)
    assert plan_of(ops, dy, w, ops.NN, **call)["kernel"] == ("gemm_glds_kernel<1,128,128,2,2,1,false>" if M < 1024 else "gemm_pers_kernel<1,3,0,false>")
    ops.gemm(dy, w, ops.NN, **call)
    torch.cuda.synchronize()
    out.assert_intact(f"NN caption fc2 dx {M} rows")
    check_16(f"NN caption fc2 dx {M}x{N} K={K} x aux", out.view, ref)
