"""The call list that pins pxa_gemm's host-side dispatch (csrc/gemm.hip: fill_gemm, choose_gemm, launch_instance), and the script that issues it.

    python tools/gemm_dispatch.py                     every call of ALL_CASES once on cuda:0, seeded inputs: per call ops.gemm_plan's line, then " | " and the
                                                      errors of what the call wrote against reference(); also meant to run under
                                                      `rocprofv3 --kernel-trace --output-format csv -- python ...`
    python tools/gemm_dispatch.py --launches x.csv    the ordered (kernel, grid, workgroup, LDS bytes) list of a kernel-trace csv, GEMM-side kernels only
    python tools/gemm_dispatch.py --check x.csv out   --launches, checked against the plan lines: per call the instance named, then the column-sum pass and
                                                      the split-K reduce where the plan says so (needs no GPU)

CASES (the denoiser's and the VAE's calls, and the refused ones), T5_CASES (the text encoder's) and ALL_CASES (both: what is run) are shared with
tests/test_gemm_plan.py (the expected plan lines live there) and tests/test_gemm_call_list_gpu.py (the values: prepare_outputs, reference and errors below,
per setting in a child process each).  Each case is (name, dict): layout, M, N, K and what else the call carries.
Shapes are the smallest that reach a branch: M = 1024 rows, N = 1024 / 1152 (N % 256 == 128: the remainder column) / 1280, N = 128 / 256 / 384 for the
convolutions, K of one or two k-units, 4096 for the cost model and explicit splits, 72 for the register-staged kernel; the T5 encoder's forms at ragged row
counts (1120, 1200, 900).  SETTINGS are the environments the list runs under: every once-per-process knob needs a process of its own."""
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NT, NN, TN = 0, 1, 2
SETTINGS = {
    "default": {}, "no_persistent": {"PXA_GEMM_NO_PERSISTENT": "1"}, "no_half_items": {"PXA_GEMM_NO_HALF_ITEMS": "1"},
    "no_staged_epilogue": {"PXA_GEMM_NO_STAGED_EPILOGUE": "1"}, "seg_half": {"PXA_GEMM_SEG_HALF": "1"},
    "tile_128": {"PXA_GEMM_TILE": "128"}, "tile_256x128": {"PXA_GEMM_TILE": "256x128"}, "tile_256": {"PXA_GEMM_TILE": "256"},
    "no_glds": {"PXA_GEMM_NO_GLDS": "1"}, "nt4": {"PXA_GEMM_NT4": "1"},
}


def _conv(N, act=0, stats=False, B=4, **kw):
    """implicit 3 x 3 convolution of B 14 x 14 images (256 padded-pixel rows each), 64 input channels, tap-interleaved K"""
    return dict(layout=NT, M=B * 256, N=N, K=576, conv=(B, 14, 14, 64), act=act, stats=stats, bias=True, **kw)


CASES = [
    # token GEMMs, 16-bit output: the persistent kernel's flavours per layout
    ("nt_plain_1024", dict(layout=NT, M=1024, N=1024, K=64)),
    ("nt_plain_1152", dict(layout=NT, M=1024, N=1152, K=128, bias=True)),
    ("nt_plain_1280", dict(layout=NT, M=1024, N=1280, K=64, descending=True)),
    ("nt_plain_2048_rows", dict(layout=NT, M=2048, N=1024, K=256)),                # the one-wave-per-SIMD NT kernel takes it under PXA_GEMM_NT4=1
    ("nt_gelu_save_grad", dict(layout=NT, M=1024, N=1024, K=64, bias=True, act=3, out2=True)),
    ("nt_mul_aux_colsum_1024", dict(layout=NT, M=1024, N=1024, K=64, act=4, colsum=True)),
    ("nt_mul_aux_colsum_1152", dict(layout=NT, M=1024, N=1152, K=64, act=4, colsum=True)),
    ("nt_gelu_1024", dict(layout=NT, M=1024, N=1024, K=64, bias=True, act=1)),
    ("nt_gelu_1152", dict(layout=NT, M=1024, N=1152, K=64, bias=True, act=1)),
    ("nt_gelu_out2", dict(layout=NT, M=1024, N=1024, K=64, bias=True, act=1, out2=True)),
    ("nt_colsum", dict(layout=NT, M=1024, N=1024, K=64, colsum=True)),
    ("nn_plain_1024", dict(layout=NN, M=1024, N=1024, K=64)),
    ("nn_plain_1152", dict(layout=NN, M=1024, N=1152, K=128)),
    ("nn_gelu_save_grad", dict(layout=NN, M=1024, N=1024, K=64, act=3, out2=True)),
    ("nn_mul_aux_colsum_1024", dict(layout=NN, M=1024, N=1024, K=64, act=4, colsum=True)),
    ("nn_mul_aux_colsum_1152", dict(layout=NN, M=1024, N=1152, K=64, act=4, colsum=True)),
    ("nn_mul_aux", dict(layout=NN, M=1024, N=1024, K=64, act=4)),
    ("nn_gelu_1024", dict(layout=NN, M=1024, N=1024, K=64, act=1)),
    # below 1024 columns: the 128 x 128 two-stage kernel, staged and direct epilogues, fused and separate column sums
    ("nt_small", dict(layout=NT, M=1024, N=256, K=64)),
    ("nt_small_colsum", dict(layout=NT, M=1024, N=256, K=64, colsum=True)),
    ("nt_small_gelu_save_grad", dict(layout=NT, M=1024, N=256, K=64, act=3, out2=True)),
    ("nt_small_gelu_out2_colsum", dict(layout=NT, M=1024, N=256, K=64, act=1, out2=True, colsum=True)),
    ("nt_small_f32", dict(layout=NT, M=1024, N=32, K=128, bias=True, f32=True)),
    ("nn_small", dict(layout=NN, M=1024, N=256, K=64)),
    ("tn_small", dict(layout=TN, M=1024, N=256, K=64, f32=True)),
    # fp32 weight gradients (TN): the four accumulate modes, explicit splits, the cost model, the paired remainder column
    ("tn_store_1024", dict(layout=TN, M=1024, N=1024, K=64, f32=True)),
    ("tn_store_1152", dict(layout=TN, M=1024, N=1152, K=128, f32=True)),
    ("tn_accumulate_one_slice", dict(layout=TN, M=1024, N=1152, K=128, f32=True, accumulate=True)),
    ("tn_split_4", dict(layout=TN, M=1024, N=1152, K=4096, f32=True, accumulate=True, split_k=4)),
    ("tn_split_17_atomics", dict(layout=TN, M=1024, N=1024, K=1088, f32=True, accumulate=True, split_k=17, short_ws=True)),    # one slice more than ops.gemm's workspace holds
    ("tn_cost_model_1152", dict(layout=TN, M=1024, N=1152, K=4096, f32=True, accumulate=True, split_k=0)),
    ("tn_cost_model_1024", dict(layout=TN, M=1024, N=1024, K=4096, f32=True, accumulate=True, split_k=0)),
    ("tn_cost_model_32_rows", dict(layout=TN, M=32, N=1152, K=4096, f32=True, accumulate=True, split_k=0)),
    ("tn_cost_model_4608_rows", dict(layout=TN, M=4608, N=1152, K=4096, f32=True, accumulate=True, split_k=0)),   # the smallest here that the model gives 256 x 256 tiles
    ("tn_bias", dict(layout=TN, M=1024, N=1024, K=64, f32=True, bias=True)),
    ("nn_f32_accumulate", dict(layout=NN, M=1024, N=1152, K=4096, f32=True, accumulate=True, split_k=0)),
    # K % 64 != 0: the register-staged kernel, column sums in a pass of their own
    ("nt_k72", dict(layout=NT, M=1024, N=1024, K=72)),
    ("nt_k72_colsum", dict(layout=NT, M=1024, N=1024, K=72, colsum=True)),
    ("nn_k72", dict(layout=NN, M=1024, N=1152, K=72)),
    ("tn_k72_accumulate", dict(layout=TN, M=1024, N=1152, K=72, f32=True, accumulate=True, split_k=0)),
    ("tn_k1000_split_16", dict(layout=TN, M=1024, N=1024, K=1000, f32=True, accumulate=True, split_k=16)),
    # implicit convolutions: epilogue from (act, gn_part), remainder mode from N
    ("conv_128", _conv(128)), ("conv_256", _conv(256)), ("conv_384", _conv(384)),
    ("conv_res_128", _conv(128, act=5)), ("conv_res_256", _conv(256, act=5)), ("conv_res_384", _conv(384, act=5)),
    ("conv_stats_128", _conv(128, stats=True)), ("conv_stats_256", _conv(256, stats=True)), ("conv_stats_384", _conv(384, stats=True)),
    ("conv_res_stats_128", _conv(128, act=5, stats=True)), ("conv_res_stats_256", _conv(256, act=5, stats=True)), ("conv_res_stats_384", _conv(384, act=5, stats=True)),
    ("conv_phase_128", _conv(128, stats=True, up=(0, 1))),
    ("conv_768_rows", _conv(128, B=3)), ("conv_res_768_rows", _conv(128, act=5, B=3)),
    ("conv_f32", _conv(128, f32=True)),
    # refused calls (pxa_gemm_plan only: nothing to launch)
    ("refuse_stats_768_rows", _conv(128, stats=True, B=3, refused="gn_part needs the persistent implicit-convolution path")),
    ("refuse_phase_residual", _conv(128, act=5, stats=True, up=(1, 0), refused="up_row_pitch needs an implicit convolution with gn_part, act 0 and the plain segment order")),
    ("refuse_k_seg_nn", dict(layout=NN, M=1024, N=1024, K=128, k_seg=64, refused="k_seg needs layout NT, no split-K, no colsum")),
    ("refuse_k_seg_32", dict(layout=NT, M=1024, N=1024, K=128, k_seg=32, refused="k_seg=32 must be a multiple of 64 dividing K=128")),
    ("refuse_stats_without_k_seg", dict(layout=NT, M=1024, N=1024, K=128, stats_plain=True, refused="gn_part needs an implicit convolution (k_seg) with a bf16 output and act 0 or 5")),
]


# the T5 encoder's five calls per block (pixart_sigma_amd/t5/encoder.py), a list of their own beside the denoiser's and the VAE's: no bias anywhere, GELU with one
# output, x aux without column sums, the fp32 residual as a single-slice accumulate target; M = B L is never a multiple of 256: 1120 = 4 x 256 + 96 (the last
# tile's second 128-row wave row is wholly out of range), 1200 = 4 x 256 + 176 (partly in range), 900 rows: below the 1024-row threshold
T5_CASES = [
    ("t5_qkv_1120_rows", dict(layout=NT, M=1120, N=1536, K=128)),
    ("t5_gelu_no_bias", dict(layout=NT, M=1120, N=1280, K=128, act=1)),
    ("t5_mul_aux", dict(layout=NT, M=1120, N=1280, K=128, act=4)),
    ("t5_mul_aux_1152", dict(layout=NT, M=1200, N=1152, K=128, act=4)),
    ("t5_residual_1024", dict(layout=NT, M=1120, N=1024, K=128, f32=True, accumulate=True)),
    ("t5_residual_k320", dict(layout=NT, M=1200, N=1280, K=320, f32=True, accumulate=True)),
    ("t5_residual_900_rows", dict(layout=NT, M=900, N=1024, K=320, f32=True, accumulate=True)),
]
# what the scripts and the tests run: the launched calls, the T5 forms behind them (a case's seed is its place here), the refused calls last
ALL_CASES = [c for c in CASES if "refused" not in c[1]] + T5_CASES + [c for c in CASES if "refused" in c[1]]


def make_call(spec, device, seed=0, values=True):
    """(a, b, keyword arguments) of ops.gemm / ops.gemm_plan for one case: seeded operands, zeroed outputs and partial buffers (values=False: shapes only)."""
    import torch
    from pixart_sigma_amd import ops
    from pixart_sigma_amd.vae.autoencoder_kl import _img_rows
    g = torch.Generator().manual_seed(seed)
    M, N, K, layout = spec["M"], spec["N"], spec["K"], spec["layout"]

    def rnd(*shape, dtype=ops.BF16, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(dtype).to(device) if values else torch.empty(*shape, dtype=dtype, device=device)

    def zeros(*shape, dtype=ops.BF16):
        return torch.zeros(*shape, dtype=dtype, device=device) if values else torch.empty(*shape, dtype=dtype, device=device)
    kw = dict(layout=layout, act=spec.get("act", 0), accumulate=spec.get("accumulate", False), split_k=spec.get("split_k", 1), descending=spec.get("descending", False))
    b = rnd(N, K, scale=K ** -0.5) if layout == NT else rnd(K, N, scale=K ** -0.5)
    if "conv" in spec:
        B, H, W, C = spec["conv"]
        rp, ip = W + 2, _img_rows(H, W)
        assert B * ip == M and (K == 9 * C or "up" in spec)
        buf = rnd((M + 3 * rp + 8) * C)                                  # every row's 3 x 3 patch stays inside the buffer
        if "up" in spec:                                                 # one phase of the convolution over the 2x upsampled grid: K = 4 C, plain segment order
            dy, dx = spec["up"]
            a, b = buf.as_strided((M, 4 * C), (C, 1)), rnd(N, 4 * C, scale=0.06)
            rpH, ipH = 2 * W + 2, _img_rows(2 * H, 2 * W)
            kw.update(k_seg=2 * C, a_seg_stride=rp * C, up=(rpH, ipH, dy, dx), out=zeros(B * ipH, N))
        else:
            a = buf.as_strided((M, 9 * C), (C, 1))
            kw.update(k_seg=3 * C, a_seg_stride=rp * C, k_tap=C)
        if spec.get("stats"):
            kw.update(gn_part=zeros(ops.COLSUM_SLOTS, B, N // 4, 2, dtype=torch.float32), gn_geom=(ip, rp, H, W))
    else:
        a = rnd(K, M) if layout == TN else rnd(M, K)
        if spec.get("short_ws"):                                         # ops.gemm then allocates its 16 slabs of M x N anew
            ops._SPLITK_WS.pop(a.device, None)
        if "k_seg" in spec:
            kw.update(k_seg=spec["k_seg"], a_seg_stride=K)
        if spec.get("stats_plain"):
            kw.update(gn_part=zeros(ops.COLSUM_SLOTS, 4, N // 4, 2, dtype=torch.float32), gn_geom=(256, 16, 14, 14))
    if spec.get("bias"):
        kw["bias"] = rnd(N, dtype=torch.float32)
    if kw["act"] in (2, 4, 5):
        kw["aux"] = rnd(M, N)
    if spec.get("out2"):
        kw.update(out=zeros(M, N), out2=zeros(M, N))
    if spec.get("f32"):
        kw["out_f32"] = zeros(M, N, dtype=torch.float32)
    if spec.get("colsum"):
        kw["colsum"] = zeros(ops.COLSUM_SLOTS, N, dtype=torch.float32)
    return a, b, kw


# ------------------------------------------------------------------------------------------------ what a call writes, and what it should have written
BLOCK = 64                 # rows and columns of the block the errors are taken over: a wave's store tile


def written(spec):
    """the kinds of figures errors() returns for a case: one per output the call writes"""
    kinds = ["out_f32"] if spec.get("f32") else ["out"]
    kinds += ["out2"] * bool(spec.get("out2")) + ["colsum_to_stored", "colsum_to_reference"] * bool(spec.get("colsum")) + ["gn_sums", "gn_finalize"] * bool(spec.get("stats"))
    return kinds


def prepare_outputs(spec, a, kw, seed=0):
    """The outputs of make_call's keyword arguments as a values check wants them before the call: an accumulate target holds seeded N(0, 1) values, every other
    output is all NaN (the 16-bit `out` the call would allocate is given), so a tile the kernel never writes shows; colsum and gn_part stay zeroed."""
    import torch
    from pixart_sigma_amd import ops
    if spec.get("f32"):
        t = kw["out_f32"]
        if kw["accumulate"]:
            t.copy_(torch.randn(t.shape, generator=torch.Generator().manual_seed(1000 + seed)))
        else:
            t.fill_(float("nan"))
    else:
        if "out" not in kw:
            kw["out"] = torch.empty(spec["M"], spec["N"], dtype=ops.BF16, device=a.device)
        kw["out"].fill_(float("nan"))
    if "out2" in kw:
        kw["out2"].fill_(float("nan"))
    return kw


def _geometry():
    """tests/test_vae_conv_geometry_gpu.py: img_rows, conv_ref64 and check_statistics are stated there, once"""
    tests = os.path.join(ROOT, "tests")
    if tests not in sys.path:
        sys.path.insert(0, tests)
    import test_vae_conv_geometry_gpu as geo
    return geo


def _conv_rows(spec, device):
    """(B, H, W) row indices of the interior pixels: in the A operand's padded grid, and in `out` (the 2x grid for a phase of the upsampled convolution)"""
    import torch
    B, H, W, _ = spec["conv"]
    rp, ip = W + 2, _geometry().img_rows(H, W)
    b, py, px = (torch.arange(n, device=device).view(s) for n, s in ((B, (B, 1, 1)), (H, (1, H, 1)), (W, (1, 1, W))))
    low = b * ip + (py + 1) * rp + px + 1
    if "up" not in spec:
        return low, low
    dy, dx = spec["up"]
    return low, b * _geometry().img_rows(2 * H, 2 * W) + (2 * py + 1 + dy) * (2 * W + 2) + 2 * px + 1 + dx


def _gelu64(pre):
    """tanh-GELU and its derivative in fp64"""
    import torch
    import torch.nn.functional as F
    x = pre.clone().requires_grad_(True)
    y = F.gelu(x, approximate="tanh")
    y.sum().backward()
    return y.detach(), x.grad


def reference(spec, a, b, kw):
    """The fp64 expectation of everything the call of make_call(spec) writes, from the 16-bit-rounded operands as they are, on their device (include/pixart_hip.h;
    tests/test_kernels_gpu.py states the same per epilogue).  Call it before ops.gemm: an accumulate target is read for what it holds.  Returns a dict:
      "out" / "out2" / "out_f32"   the output's shape in fp64;
      "rows"                       implicit convolutions only: the rows of the output that are specified (interior pixels; for the phase of an upsampled
                                   convolution their places in the 2x grid), the others of the expectation are zero and mean nothing;
      "colsum"                     the column sums of "out" (the kernel's sums are taken over the stored 16-bit values: errors() has both comparisons).
    The implicit convolutions are F.conv2d in fp64 (conv_ref64 of tests/test_vae_conv_geometry_gpu.py) over the padded pixel grid the A operand is a view of."""
    import torch
    M, N, K, layout, act = spec["M"], spec["N"], spec["K"], spec["layout"], kw["act"]
    bias = kw["bias"].double() if "bias" in kw else torch.zeros(N, dtype=torch.float64, device=a.device)
    aux = kw["aux"].double() if "aux" in kw else None
    ref = {}
    if "conv" in spec:
        geo = _geometry()
        B, H, W, C = spec["conv"]
        rp, ip = W + 2, geo.img_rows(H, W)
        pix = a.as_strided((a.untyped_storage().nbytes() // a.element_size() // C, C), (C, 1), 0)           # the pixel rows A's patches are views of
        b_, i_, j_ = (torch.arange(n, device=a.device).view(s) for n, s in ((B, (B, 1, 1)), (H + 3, (1, H + 3, 1)), (rp, (1, 1, rp))))
        if "up" in spec:         # row m = sum over a 2 x 2 patch from pixel m on, K = [2 rows][2 taps][C]: conv2d (padding 1) of the grid whose (i, j) is pixel i rp + j
            grid, w, sl = pix[(b_ * ip + i_ * rp + j_)[:, :H + 2]], b.view(N, 2, 2, C).permute(0, 3, 1, 2), (slice(2, H + 2), slice(2, W + 2))
        else:                    # row m = sum over a 3 x 3 patch from pixel m on, K = [C / 64][3 rows][3 taps][64]: the grid whose (i, j) is pixel i rp + j + 1
            assert kw["k_tap"] == C and C % 64 == 0
            grid, w, sl = pix[b_ * ip + i_ * rp + j_ + 1], b.view(N, C // 64, 3, 3, 64).permute(0, 1, 4, 2, 3).reshape(N, C, 3, 3), (slice(2, H + 2), slice(1, W + 1))
        y = geo.conv_ref64(grid.permute(0, 3, 1, 2), w, bias)[:, :, sl[0], sl[1]].to(a.device)               # (B, N, H, W): the interior pixels
        low, high = _conv_rows(spec, a.device)
        y = y.permute(0, 2, 3, 1).reshape(-1, N)
        if act == 5:
            y = y + aux[low.flatten()]
        else:
            assert act == 0
        target = kw["out_f32"] if spec.get("f32") else kw["out"]
        full = torch.zeros(target.shape, dtype=torch.float64, device=a.device)
        full[high.flatten()] = y
        ref["out_f32" if spec.get("f32") else "out"] = full
        ref["rows"] = torch.zeros(target.shape[0], dtype=torch.bool, device=a.device)
        ref["rows"][high.flatten()] = True
        assert int(ref["rows"].sum()) == B * H * W
        return ref
    A, Bm = a.double(), b.double()
    pre = (A @ Bm.t() if layout == NT else A @ Bm if layout == NN else A.t() @ Bm) + bias
    if spec.get("f32"):
        assert act == 0
        ref["out_f32"] = pre + kw["out_f32"].double() if kw["accumulate"] else pre
        return ref
    if act in (1, 3):
        ref["out"], grad = _gelu64(pre)
        if "out2" in kw:
            ref["out2"] = pre if act == 1 else grad
    elif act == 2:
        ref["out"] = pre * _gelu64(aux)[1]
    else:
        ref["out"] = pre if act == 0 else pre * aux if act == 4 else pre + aux
    if "colsum" in kw:
        ref["colsum"] = ref["out"].sum(0)
    return ref


def block_rel_l2(got, want, rows=None):
    """(the largest rel-L2 over the BLOCK x BLOCK blocks of a 2-D output, the number of non-finite values): a global rel-L2 dilutes one bad tile of a large
    output to nothing.  rows: the specified rows (a block's figure is over those only; a block without any has none)."""
    import torch
    import torch.nn.functional as F
    got, want = got.double(), want.double()
    if got.dim() == 1:
        got, want = got[None], want[None]
    if rows is not None:                              # (the blocks stay where the kernel's tiles are)
        got, want = torch.where(rows[:, None], got, 0.0), torch.where(rows[:, None], want, 0.0)
    bad = int((~torch.isfinite(got)).sum())
    R, N = got.shape
    pad = (0, -N % BLOCK, 0, -R % BLOCK)
    num = F.pad((got - want) ** 2, pad).view((R + BLOCK - 1) // BLOCK, BLOCK, -1, BLOCK).sum((1, 3))
    den = F.pad(want ** 2, pad).view((R + BLOCK - 1) // BLOCK, BLOCK, -1, BLOCK).sum((1, 3))
    e = (num / den.clamp_min(1e-300)).sqrt()
    return (float("nan") if torch.isnan(e).any() else e.max().item()), bad


def errors(spec, kw, ref, statistics=True):
    """{kind: figure} for every kind of written(spec), after the call: the 2-D outputs as block_rel_l2 against reference(); the column sums (summed over the slots)
    against the column sums of the STORED 16-bit output and against the reference's; the GroupNorm partials through check_statistics of
    tests/test_vae_conv_geometry_gpu.py (its two figures; "gn_assert" holds its message where it failed).  "nan": non-finite values found where a value is
    specified, over all outputs.  statistics = False leaves the partials out (check_statistics finalizes on the GPU)."""
    out, nan = {}, 0
    for kind in ("out", "out2", "out_f32"):
        if kind in ref:
            out[kind], bad = block_rel_l2(kw[kind], ref[kind], ref.get("rows"))
            nan += bad
    if "colsum" in kw:
        sums = kw["colsum"].double().sum(0)
        out["colsum_to_stored"], bad = block_rel_l2(sums, kw["out"].double().sum(0))
        out["colsum_to_reference"], _ = block_rel_l2(sums, ref["colsum"])
        nan += bad
    if spec.get("stats") and statistics:
        import conftest
        from pixart_sigma_amd import ops
        geo = _geometry()
        B, H, W, _ = spec["conv"]
        y = kw["out"][_conv_rows(spec, kw["out"].device)[1]].permute(0, 3, 1, 2).contiguous()           # the stored interior pixels, (B, N, H, W)
        first = len(conftest.PARITY)
        try:
            geo.check_statistics(ops, kw["gn_part"], y, B, spec["N"], H, W, "call list", fin_tol=geo.PHASE_FIN_TOL if "up" in spec else geo.STAT_FIN_TOL)
        except AssertionError as e:
            out["gn_assert"] = str(e)
        figures = conftest.PARITY[first:]
        del conftest.PARITY[first:]
        out["gn_sums"], out["gn_finalize"] = figures[0]["value"], figures[1]["value"]
    out["nan"] = nan
    return out


# ------------------------------------------------------------------------------------------------ kernel-trace csv -> launches
GEMM_SIDE = r"gemm_\w*kernel|splitk_reduce_kernel|colsum_kernel"


def launches(path):
    """[(kernel name as its template is written, grid, workgroup, LDS bytes)] of a rocprofv3 kernel-trace csv, in start order, GEMM-side kernels only."""
    rows = []
    for r in csv.DictReader(open(path)):
        r = {k.lower(): v for k, v in r.items()}
        m = re.search(r"\b(%s)\b(<[^>]*>)?" % GEMM_SIDE, r["kernel_name"])
        if m:
            name = m.group(0).replace(" ", "")
            rows.append((int(r["start_timestamp"]), name, int(r["grid_size_x"]), int(r["workgroup_size_x"]), int(r["lds_block_size"])))
    return [r[1:] for r in sorted(rows)]


def check(got, plan_lines):
    """the launches of a trace against the plan lines of the calls that made them: per call the instance named (under PXA_GEMM_NT4=1 the launches of
    gemm_nt4_kernel instead, where it took the call), then the column-sum pass and the split-K reduce where the plan says so"""
    nt4_on, i, n = os.environ.get("PXA_GEMM_NT4", "0") not in ("", "0"), 0, 0
    for case, line in plan_lines:
        f = dict(kv.split("=") for kv in line.split()[1:])
        want = [line.split()[0]] + ["colsum_kernel"] * (f["colsum_pass_after"] == "1") + ["splitk_reduce_kernel"] * (f["splitk_reduce"] == "1")
        if nt4_on and f["try_nt4"] == "1" and i < len(got) and got[i][0].startswith("gemm_nt4_kernel"):
            while i < len(got) and got[i][0].startswith("gemm_nt4_kernel"):     # (full columns and the remainder column are launches of their own)
                i += 1
            want = want[1:]
        for k in want:
            assert i < len(got), f"{case}: the trace ends before {k}"
            assert got[i][0] == k, f"{case}: the plan names {k}, the trace shows {got[i][0]}"
            i, n = i + 1, n + 1
    assert i == len(got), f"{len(got) - i} launches more than the plans name, first {got[i]}"
    return n


def main():
    if len(sys.argv) > 2 and sys.argv[1] in ("--launches", "--check"):
        got = launches(sys.argv[2])
        for l in got:
            print(*l)
        if sys.argv[1] == "--check":                                     # argv[3]: the output of the run that was traced
            plan_lines = [l.split(" | ")[0].split(": ", 1) for l in open(sys.argv[3]).read().splitlines() if ": gemm_" in l]
            print(f"# {len(got)} launches of {len(plan_lines)} calls: every kernel is the one its plan names ({check(got, plan_lines)} matched by name)")
        return
    import torch
    from pixart_sigma_amd import ops
    from pixart_sigma_amd.lib import PixartHipError
    for i, (name, spec) in enumerate(ALL_CASES):
        if "refused" in spec:
            continue
        a, b, kw = make_call(spec, "cuda:0", seed=i)
        prepare_outputs(spec, a, kw, seed=i)
        try:
            line = ops.gemm_plan(a, b, **kw)
        except PixartHipError as e:                                      # (a setting can refuse a call of the list: the plan says so before anything is launched)
            print(f"{name}: refused: {e}", flush=True)
            continue
        ref = reference(spec, a, b, kw)
        ops.gemm(a, b, **kw)
        torch.cuda.synchronize()
        print(f"{name}: {line} | " + " ".join(f"{k} {v:.2e}" if isinstance(v, float) else f"{k} {v}" for k, v in errors(spec, kw, ref).items()), flush=True)
    print("# done")


if __name__ == "__main__":
    main()
