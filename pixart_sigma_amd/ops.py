"""Tensor-level wrappers over the C ABI (pixart_sigma_amd/lib.py).  Each function validates shapes/dtypes, allocates
outputs with torch (device memory + stream plumbing only) and launches exactly one libpixart_hip.so entry point.
No math happens in Python."""
import ctypes as C
import math

import torch

from . import lib
from .lib import AttnArgs, GemmArgs, GridArg, T5AttnArgs, call, ptr

# BF16 = the process's 16-bit operand dtype: torch.bfloat16, or torch.float16 under PXA_OPERAND_DTYPE=f16 (historical name)
from .lib import OPERAND_DTYPE as BF16  # noqa: E402
F32 = torch.float32
NT, NN, TN = 0, 1, 2
ACT_NONE, ACT_GELU, ACT_GELU_GRAD, ACT_GELU_SAVE_GRAD, ACT_MUL_AUX, ACT_ADD_AUX = 0, 1, 2, 3, 4, 5
_SPLITK_WS = {}


def _chk(t, dtype, name, cuda=True):
    assert (t.is_cuda or not cuda) and t.dtype == dtype and t.stride(-1) == 1, f"{name}: need contiguous-last-dim {dtype} CUDA tensor"


def gemm(a, b, layout=NT, bias=None, act=ACT_NONE, aux=None, out=None, out2=None, out_f32=None, accumulate=False,
         split_k=1, out_dtype=BF16, colsum=None, k_seg=0, a_seg_stride=0, k_tap=0, gn_part=None, gn_geom=None, descending=False, up=None):
    """C = op(A) op(B) (see include/pixart_hip.h).  a, b: 2-D bf16 (row stride arbitrary multiple of 8).
    Returns the bf16 output (or fp32 when out_dtype is float32 / out_f32 is given).
    k_seg / a_seg_stride / k_tap: segmented-K A operand (the implicit 3x3 convolution of the VAE kernel set).
    gn_part (PXA_COLSUM_SLOTS, B, N/4, 2) fp32 zeros + gn_geom = (img_rows, row_pitch, H, W): GroupNorm statistics of the output
    accumulated by the epilogue (see pxa_gemm_args.gn_part).
    descending: the persistent NT / NN kernels walk their output tiles from the last token rows to the first (pxa_gemm_args.items_descending) - for a launch
    whose A operand was just written by a kernel that swept the rows upwards; bit-identical results.
    up = (row_pitch, img_rows, dy, dx) of the HIGH-RES padded output grid: this launch is phase (dy, dx) of a 3x3 convolution over a 2x nearest-upsampled
    input, computed on the low-res grid (pxa_gemm_args.up_*); `out` must be given (its rows are high-res padded pixels)."""
    g, res = _gemm_args(False, **locals())         # (locals() = the arguments, nothing else yet)
    call("pxa_gemm", g)
    return res


def gemm_plan(a, b, layout=NT, bias=None, act=ACT_NONE, aux=None, out=None, out2=None, out_f32=None, accumulate=False,
              split_k=1, out_dtype=BF16, colsum=None, k_seg=0, a_seg_stride=0, k_tap=0, gn_part=None, gn_geom=None, descending=False, up=None):
    """What gemm would launch for the same arguments, as pxa_gemm_plan's one line of text (kernel instance, split, k_per_split, accumulate mode, ...); raises
    what gemm would raise for a call the library refuses.  Launches nothing, allocates nothing and needs no GPU: the tensors may live on any device (only
    their shapes, strides and the presence of each pointer matter)."""
    g, _ = _gemm_args(True, **locals())
    buf = C.create_string_buffer(256)
    lib.check(lib.load().pxa_gemm_plan(C.byref(g), buf, len(buf)), "pxa_gemm_plan")
    return buf.value.decode()


class _Unallocated:
    """gemm_plan's stand-in for a buffer gemm would allocate: rows x cols of a dtype at an address that is not NULL and never used."""
    _somewhere = C.c_double()

    def __init__(self, rows, cols, dtype):
        self.shape, self.dtype = (rows, cols), dtype

    def __getitem__(self, i):
        return self

    def stride(self, d):
        return (self.shape[1], 1)[d]

    def numel(self):
        return self.shape[0] * self.shape[1]


def _gemm_args(plan, a, b, layout, bias, act, aux, out, out2, out_f32, accumulate, split_k, out_dtype, colsum, k_seg, a_seg_stride, k_tap, gn_part, gn_geom,
               descending, up):
    """The pxa_gemm_args block of gemm / gemm_plan and the tensor gemm returns.  gemm allocates the outputs and the split-K workspace that are not given;
    plan = True (gemm_plan) only says where they would be, and the tensors need not be on the GPU."""
    def chk(t, dtype, name):
        if not isinstance(t, _Unallocated):
            _chk(t, dtype, name, cuda=not plan)

    def ptr(t):
        return C.c_void_p(C.addressof(t._somewhere)) if isinstance(t, _Unallocated) else lib.ptr(t, cuda=not plan)

    def new(rows, cols, dtype):
        return _Unallocated(rows, cols, dtype) if plan else torch.empty((rows, cols), dtype=dtype, device=a.device)
    chk(a, BF16, "A")
    chk(b, BF16, "B")
    if layout == NT:
        M, K = a.shape
        N, K2 = b.shape
    elif layout == NN:
        M, K = a.shape
        K2, N = b.shape
    else:
        K, M = a.shape
        K2, N = b.shape
    assert K == K2, f"gemm: K mismatch {K} vs {K2}"
    g = GemmArgs()
    g.A, g.B, g.lda, g.ldb = ptr(a), ptr(b), a.stride(0), b.stride(0)
    g.M, g.N, g.K, g.layout = M, N, K, layout
    if bias is not None:
        chk(bias, F32, "bias")
        assert bias.numel() == N
    g.bias, g.act = ptr(bias), act
    if act in (ACT_GELU_GRAD, ACT_MUL_AUX, ACT_ADD_AUX):
        chk(aux, BF16, "aux")
        g.aux, g.ldaux = ptr(aux), aux.stride(0)
    want_f32 = out_f32 is not None or out_dtype == F32
    if want_f32:
        if out_f32 is None:
            out_f32 = new(M, N, F32)
        chk(out_f32, F32, "out_f32")
        g.out_f32, g.ld_f32 = ptr(out_f32), out_f32.stride(0)
    else:
        if out is None:
            out = new(M, N, BF16)
    if out is not None:
        chk(out, BF16, "out")
        g.out_bf16, g.ld_out = ptr(out), out.stride(0)
    if out2 is not None:
        chk(out2, BF16, "out2")
        assert out is not None and out2.stride(0) == out.stride(0)
        g.out2_bf16 = ptr(out2)
    g.accumulate, g.split_k = int(accumulate), split_k
    g.items_descending = int(bool(descending))
    g.k_seg, g.a_seg_stride, g.k_tap = k_seg, a_seg_stride, k_tap
    if gn_part is not None:
        chk(gn_part, F32, "gn_part")
        assert gn_part.is_contiguous() and gn_part.numel() == COLSUM_SLOTS * (M // gn_geom[0]) * (N // 4) * 2
        g.gn_part = ptr(gn_part)
        g.gn_img_rows, g.gn_row_pitch, g.gn_h, g.gn_w = gn_geom
    if up is not None:
        assert out is not None and gn_part is not None
        g.up_row_pitch, g.up_img_rows, g.up_dy, g.up_dx = up
    if colsum is not None:               # (PXA_COLSUM_SLOTS, stride) partial buffer view: row 0 of the slice to accumulate
        g.colsum, g.colsum_stride = ptr(colsum), colsum.stride(0)
    if accumulate and split_k != 1:       # split-K partial slabs: caller-owned workspace, cached per device (max 16 slabs)
        need = 16 * M * N
        ws = _SPLITK_WS.get(a.device)
        if ws is None or ws.numel() < need:
            ws = new(1, need, F32)[0]
            if not plan:
                _SPLITK_WS[a.device] = ws
        g.splitk_ws, g.splitk_ws_elems = ptr(ws), ws.numel()
    return g, (out_f32 if want_f32 else out)


def ln_mod_fwd(x, shift=None, scale=None, mod_stride=0, u=None, gate=None, gate_stride=None, x_out=None, want_xn=True, want_xb=False,
               want_stats=False, rows_per_batch=None, eps=1e-6):
    """x' = x + gate*u; xn = LN(x')*(1+scale)+shift.  x: (R,D) fp32.  shift/scale/gate: fp32 views whose sample b
    starts at data_ptr + b*mod_stride floats.  Returns dict(x, xn, xb, mean, rstd)."""
    _chk(x, F32, "x")
    R, D = x.shape
    rpb = rows_per_batch or R
    xn = torch.empty((R, D), dtype=BF16, device=x.device) if want_xn else None
    xb = torch.empty((R, D), dtype=BF16, device=x.device) if want_xb else None
    mean = torch.empty(R, dtype=F32, device=x.device) if want_stats else None
    rstd = torch.empty(R, dtype=F32, device=x.device) if want_stats else None
    if u is not None and x_out is None:
        x_out = torch.empty_like(x)
    call("pxa_ln_mod_fwd", ptr(x), ptr(u), ptr(gate), mod_stride if gate_stride is None else gate_stride, ptr(shift), ptr(scale), mod_stride, ptr(x_out), ptr(xn), ptr(xb),
         ptr(mean), ptr(rstd), R, D, rpb, eps)
    return {"x": x_out if x_out is not None else x, "xn": xn, "xb": xb, "mean": mean, "rstd": rstd}


def ln_mod_bwd(dy, x, mean, rstd, scale, mod_stride, dx_in, dx_out, dshift, dscale, dmod_stride, rows_per_batch, dx_bf16=None, dbias=None):
    """dbias: optional (COLSUM_SLOTS, >= D) fp32 partials view receiving the column sums of dx_out (the bias gradient of the Linear behind dx_bf16)."""
    R, D = x.shape
    call("pxa_ln_mod_bwd", ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(scale), mod_stride, ptr(dx_in), ptr(dx_out), ptr(dx_bf16),
         ptr(dshift), ptr(dscale), dmod_stride, ptr(dbias), dbias.stride(0) if dbias is not None else 0, R, D, rows_per_batch)
    return dx_out


def ln_affine_fwd(x, w, b, eps=1e-5, save=True):
    """nn.LayerNorm(D) (affine) over bf16 rows, IN PLACE on the (possibly column-sliced) 2-D view x; returns (xsave, mean, rstd)."""
    _chk(x, BF16, "x"); _chk(w, F32, "w"); _chk(b, F32, "b")
    R, D = x.shape
    assert x.stride(1) == 1
    xsave = torch.empty((R, D), dtype=BF16, device=x.device) if save else None
    mean, rstd = torch.empty(R, dtype=F32, device=x.device), torch.empty(R, dtype=F32, device=x.device)
    call("pxa_ln_affine_fwd", ptr(x), x.stride(0), ptr(w), ptr(b), ptr(x), x.stride(0), ptr(xsave), ptr(mean), ptr(rstd), R, D, float(eps))
    return xsave, mean, rstd


def ln_affine_bwd(dy, xsave, mean, rstd, w, dw, db):
    """Backward of ln_affine_fwd, IN PLACE on the 2-D view dy (dy <- dx); dw / db (fp32 [D]) are accumulated into."""
    _chk(dy, BF16, "dy"); _chk(xsave, BF16, "xsave")
    R, D = dy.shape
    assert dy.stride(1) == 1 and xsave.is_contiguous()
    call("pxa_ln_affine_bwd", ptr(dy), dy.stride(0), ptr(xsave), ptr(mean), ptr(rstd), ptr(w), ptr(dy), dy.stride(0), ptr(dw), ptr(db), R, D)


def gate_bwd(dx, add=None, u=None, gate=None, mod_stride=0, dx_out=None, du=None, dgate=None, dmod_stride=0, rows_per_batch=None, dbias=None):
    R, D = dx.shape
    call("pxa_gate_bwd", ptr(dx), ptr(add), ptr(u), ptr(gate), mod_stride, ptr(dx_out), ptr(du), ptr(dgate), dmod_stride, ptr(dbias),
         dbias.stride(0) if dbias is not None else 0, R, D, rows_per_batch or R)


COLSUM_SLOTS = 16


def colsum_reduce(part, out):
    """out (n,) += part (COLSUM_SLOTS, >= n).sum(0)"""
    call("pxa_colsum_reduce", ptr(part), part.stride(0), ptr(out), out.numel())


def colsum(dy, out):
    """out[n] += sum_r dy[r][n]  (bf16 in, fp32 accumulate)."""
    R, N = dy.shape
    call("pxa_colsum_bf16", ptr(dy), dy.stride(0), ptr(out), R, N)
    return out


Q_PRESCALE = 72 ** -0.5 * 1.4426950408889634      # scale * log2 e of the denoiser's heads: what a prescaled q carries (pxa_attn_args.q_prescaled)


def _attn_args(q, k, v, o, B, H, Nq, Nk, strides, kv_start=None, kv_len=None, max_kv_len=0, scale=None, head_dim=72, q_prescaled=False, cuda=True):
    def ptr(t):     # cuda=False: attention_plan, where only the presence of a pointer matters
        return lib.ptr(t, cuda)
    a = AttnArgs()
    a.q, a.k, a.v, a.o = ptr(q), ptr(k), ptr(v), ptr(o)
    (a.q_bs, a.q_ts, a.q_hs), (a.k_bs, a.k_ts, a.k_hs), (a.v_bs, a.v_ts, a.v_hs), (a.o_bs, a.o_ts, a.o_hs) = strides
    a.B, a.H, a.Nq, a.Nk, a.head_dim = B, H, Nq, Nk, head_dim
    a.kv_start, a.kv_len, a.max_kv_len = ptr(kv_start), ptr(kv_len), max_kv_len
    a.scale = scale if scale is not None else head_dim ** -0.5
    a.q_prescaled = int(bool(q_prescaled))
    return a


def _check_max_kv_len(kw):
    """The keys-resident kernels size their LDS by max_kv_len and clamp to it: a sample longer than the caller's bound would be truncated silently where
    the streaming kernels honour kv_len.  The lengths are only known here when the caller keeps a host copy (`kv_len_host`)."""
    lens = kw.pop("kv_len_host", None)
    if lens is not None and kw.get("max_kv_len", 0) > 0:
        assert max(lens) <= kw["max_kv_len"], f"max_kv_len {kw['max_kv_len']} < longest sample {max(lens)}"


def attention_fwd(q, k, v, o, lse, B, H, Nq, Nk, strides, **kw):
    """q/k/v/o: bf16 tensors (any view); strides = ((q_bs,q_ts,q_hs),(k..),(v..),(o..)) in elements."""
    _check_max_kv_len(kw)
    a = _attn_args(q, k, v, o, B, H, Nq, Nk, strides, **kw)
    a.lse = ptr(lse)
    call("pxa_attn_fwd", a)
    return o


_bwd_stats = {}


def attn_bwd_stats(B, H, Nq, device):
    """The dK/dV kernel's lse / delta workspace (include/pixart_hip.h: pxa_attn_args.bwd_stats): written by the backward's own pre-pass and consumed
    by its last kernel on ONE stream, so the calls of a (device, stream) pair share the largest buffer asked for so far.  Keyed by the current stream
    (two streams would overwrite each other's rows) and bypassed while a graph is being captured (a buffer first allocated during capture lives in the
    graph's private pool and must not be handed to eager calls): there the caching allocator serves each call."""
    n = lib.load().pxa_attn_bwd_stats_bytes(B, H, Nq)
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(n, dtype=torch.uint8, device=device)
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    buf = _bwd_stats.get(key)
    if buf is None or buf.numel() < n:
        buf = _bwd_stats[key] = torch.empty(n, dtype=torch.uint8, device=device)
    return buf


def attention_bwd(q, k, v, o, d_o, lse, delta, dq, dk, dv, B, H, Nq, Nk, strides, dstrides, colsums=(None, None, None), **kw):
    """colsums: optional fp32 (H*72,) accumulators receiving the column sums of dq / dk / dv (bias gradients)."""
    _check_max_kv_len(kw)
    a = _attn_args(q, k, v, o, B, H, Nq, Nk, strides, **kw)
    stats = attn_bwd_stats(B, H, Nq, q.device) if dk is not None else None     # held until the launch below: under graph capture it is a fresh allocation
    a.bwd_stats = ptr(stats)
    a.dq_colsum, a.dk_colsum, a.dv_colsum = (ptr(t) for t in colsums)
    a.colsum_stride = next((t.stride(0) for t in colsums if t is not None), 0)
    a.lse, a.delta, a.d_o, a.dq, a.dk, a.dv = ptr(lse), ptr(delta), ptr(d_o), ptr(dq), ptr(dk), ptr(dv)
    (a.dq_bs, a.dq_ts, a.dq_hs), (a.dk_bs, a.dk_ts, a.dk_hs), (a.dv_bs, a.dv_ts, a.dv_hs) = dstrides
    call("pxa_attn_bwd", a)            # dq=None skips the dQ kernel, dk=dv=None the dK/dV kernel
    del stats


def attention_plan(q, k, v, o, *rest, colsums=(None, None, None), **kw):
    """What attention_fwd (called with its arguments: q, k, v, o, lse, B, H, Nq, Nk, strides, ...) or attention_bwd (with its own: q, k, v, o, d_o, lse,
    delta, dq, dk, dv, B, H, Nq, Nk, strides, dstrides, ...) would launch, as pxa_attn_plan's one line of text; raises what they would raise for a call
    the library refuses.  Launches nothing and allocates nothing: the tensors may live on any device, only their presence, the shapes and the strides
    matter (the statistics workspace attention_bwd would pass is stood in for by an address that is never used)."""
    _check_max_kv_len(kw)
    backward = len(rest) == 12
    assert len(rest) in (6, 12), "attention_plan takes the positional arguments of attention_fwd or of attention_bwd"
    p = lambda t: lib.ptr(t, cuda=False)   # noqa: E731
    if backward:
        d_o, lse, delta, dq, dk, dv, B, H, Nq, Nk, strides, dstrides = rest
        a = _attn_args(q, k, v, o, B, H, Nq, Nk, strides, cuda=False, **kw)
        a.bwd_stats = C.c_void_p(C.addressof(_Unallocated._somewhere)) if dk is not None else None
        a.dq_colsum, a.dk_colsum, a.dv_colsum = (p(t) for t in colsums)
        a.colsum_stride = next((t.stride(0) for t in colsums if t is not None), 0)
        a.lse, a.delta, a.d_o, a.dq, a.dk, a.dv = p(lse), p(delta), p(d_o), p(dq), p(dk), p(dv)
        (a.dq_bs, a.dq_ts, a.dq_hs), (a.dk_bs, a.dk_ts, a.dk_hs), (a.dv_bs, a.dv_ts, a.dv_hs) = dstrides
    else:
        lse, B, H, Nq, Nk, strides = rest
        a = _attn_args(q, k, v, o, B, H, Nq, Nk, strides, cuda=False, **kw)
        a.lse = p(lse)
    buf = C.create_string_buffer(256)
    lib.check(lib.load().pxa_attn_plan(C.byref(a), int(backward), buf, len(buf)), "pxa_attn_plan")
    return buf.value.decode()


def patch_embed_fwd(x, w, bias, pos, out=None):
    B, Cc, Hl, Wl = x.shape
    D = w.shape[0]
    if out is None:
        out = torch.empty((B * (Hl // 2) * (Wl // 2), D), dtype=F32, device=x.device)
    call("pxa_patch_embed_fwd", ptr(x), ptr(w), ptr(bias), ptr(pos), ptr(out), B, Cc, Hl, Wl, D)
    return out


def patch_embed_bwd(x, dtok, dw, dbias):
    B, Cc, Hl, Wl = x.shape
    call("pxa_patch_embed_bwd", ptr(x), ptr(dtok), ptr(dw), ptr(dbias), B, Cc, Hl, Wl, dw.shape[0])


def unpatchify_fwd(lin, B, h, w, Co):
    img = torch.empty((B, Co, 2 * h, 2 * w), dtype=F32, device=lin.device)
    call("pxa_unpatchify_fwd", ptr(lin), ptr(img), B, h, w, Co)
    return img


def patchify_bwd(dimg, h, w):
    B, Co = dimg.shape[0], dimg.shape[1]
    dlin = torch.empty((B * h * w, 4 * Co), dtype=BF16, device=dimg.device)
    call("pxa_patchify_bwd", ptr(dimg), ptr(dlin), B, h, w, Co)
    return dlin


def gather_rows_bf16(src, row_idx, L, alt=None, drop=None):
    """src: (B*L, Cw) fp32 rows; row_idx int32 (rows,) -> (rows, Cw) bf16."""
    Cw = src.shape[-1]
    rows = row_idx.numel()
    out = torch.empty((rows, Cw), dtype=BF16, device=src.device)
    call("pxa_gather_rows_bf16", ptr(src), ptr(alt), ptr(row_idx), ptr(drop), ptr(out), rows, L, Cw)
    return out


def kv_compress_fwd(inp, in_bs, in_ts, conv_w, conv_b, ln_w, ln_b, B, H, W, Cc, sr, eps=1e-5):
    out = torch.empty((B, (H // sr) * (W // sr), Cc), dtype=BF16, device=inp.device)
    call("pxa_kv_compress_fwd", ptr(inp), in_bs, in_ts, ptr(conv_w), ptr(conv_b), ptr(ln_w), ptr(ln_b), ptr(out), B, H, W, Cc, sr, eps)
    return out


def kv_compress_bwd(dyc, inp, in_bs, in_ts, conv_w, conv_b, ln_w, din, din_bs, din_ts, d_conv_w, d_conv_b, d_ln_w, d_ln_b, B, H, W, Cc, sr, eps=1e-5):
    call("pxa_kv_compress_bwd", ptr(dyc), ptr(inp), in_bs, in_ts, ptr(conv_w), ptr(conv_b), ptr(ln_w), ptr(din), din_bs, din_ts,
         ptr(d_conv_w), ptr(d_conv_b), ptr(d_ln_w), ptr(d_ln_b), B, H, W, Cc, sr, eps)


def kv_pick(src, dst, full_bs, full_ts, B, H, W, Cc, sr, backward=False):
    call("pxa_kv_pick", int(backward), ptr(src), ptr(dst), full_bs, full_ts, B, H, W, Cc, sr)


def iddpm_loss_fwd(model_out, x0, noise, coef8, tzero):
    B, C, H, W = x0.shape
    mse, vb = torch.empty(B, dtype=F32, device=x0.device), torch.empty(B, dtype=F32, device=x0.device)
    call("pxa_iddpm_loss_fwd", ptr(model_out), ptr(x0), ptr(noise), ptr(coef8), ptr(tzero), B, C, H * W, ptr(mse), ptr(vb))
    return mse, vb


def iddpm_loss_bwd(model_out, x0, noise, coef8, tzero, g_mse, g_vb):
    B, C, H, W = x0.shape
    d = torch.empty_like(model_out)
    call("pxa_iddpm_loss_bwd", ptr(model_out), ptr(x0), ptr(noise), ptr(coef8), ptr(tzero), B, C, H * W, ptr(g_mse), ptr(g_vb), ptr(d))
    return d


def sumsq(x, out):
    call("pxa_sumsq_f32", ptr(x), x.numel(), ptr(out))


def clip_coef(sumsq_t, out2, max_norm, inv_world=1.0):
    call("pxa_clip_coef", ptr(sumsq_t), ptr(out2), float(max_norm), float(inv_world))


def clip_coef_scaled(sumsq_t, out2, max_norm, inv_world, scaler_state, growth_factor, backoff_factor, growth_interval):
    call("pxa_clip_coef_scaled", ptr(sumsq_t), ptr(out2), float(max_norm), float(inv_world), ptr(scaler_state), float(growth_factor),
         float(backoff_factor), int(growth_interval))


def adamw_step_scaled(p, g, m, v, p_bf16, lr, beta1, beta2, eps, weight_decay, gscale, scaler_state):
    call("pxa_adamw_step_scaled", ptr(p), ptr(g), ptr(m), ptr(v), ptr(p_bf16), p.numel(), lr, beta1, beta2, eps, weight_decay, ptr(gscale), ptr(scaler_state))


def adamw_step(p, g, m, v, p_bf16, lr, beta1, beta2, eps, weight_decay, step, gscale=None):
    call("pxa_adamw_step", ptr(p), ptr(g), ptr(m), ptr(v), ptr(p_bf16), p.numel(), lr, beta1, beta2, eps, weight_decay, step, ptr(gscale))


def ema_update(ema, p, decay, scaler_state=None):
    """ema <- ema + (1 - decay) (p - ema) over two flat fp32 buffers; with the loss scaler's record, nothing is written on a skipped step (csrc/ema.hip)."""
    assert ema.dtype == F32 and p.dtype == F32 and ema.numel() == p.numel() and ema.is_contiguous() and p.is_contiguous()
    call("pxa_ema_update", ptr(ema), ptr(p), p.numel(), float(decay), ptr(scaler_state))


def swap_f32(a, b):
    """a <-> b, two disjoint flat fp32 buffers, in place."""
    assert a.dtype == F32 and b.dtype == F32 and a.numel() == b.numel() and a.is_contiguous() and b.is_contiguous()
    call("pxa_swap_f32", ptr(a), ptr(b), a.numel())


def scale_copy(src, src_stride, nblocks, n_scaled, n_total, scale, out_bf16=None, out_f32=None):
    """nblocks strided blocks of a flat fp32 buffer -> (nblocks, n_total) copies whose first n_scaled elements carry `scale` (one rounding)."""
    out = out_bf16 if out_bf16 is not None else out_f32
    assert out.is_contiguous() and out.shape[0] == nblocks and out[0].numel() == n_total
    call("pxa_scale_copy_f32", ptr(src), src_stride, ptr(out_bf16), ptr(out_f32), n_total, nblocks, n_scaled, n_total, float(scale))


def linear_f32_fwd(x, w, b=None):
    """y = x W^T + b, fp32 (conditioning linears: csrc/condlin.hip)."""
    _chk(x, F32, "x"); _chk(w, F32, "w")
    M, K = x.shape
    N = w.shape[0]
    assert x.is_contiguous() and w.is_contiguous() and w.shape[1] == K
    y = torch.empty((M, N), dtype=F32, device=x.device)
    call("pxa_linear_f32_fwd", ptr(x), ptr(w), ptr(b), ptr(y), M, N, K)
    return y


def linear_f32_bwd(dy, x, w, need_dx=True, need_dw=True, need_db=True):
    _chk(dy, F32, "dy"); _chk(x, F32, "x"); _chk(w, F32, "w")
    M, K = x.shape
    N = w.shape[0]
    assert dy.is_contiguous() and x.is_contiguous() and w.is_contiguous() and dy.shape == (M, N)
    dx = torch.zeros((M, K), dtype=F32, device=x.device) if need_dx else None
    dw = torch.empty((N, K), dtype=F32, device=x.device) if (need_dw or need_db) else None
    db = torch.empty((N,), dtype=F32, device=x.device) if need_db else None
    call("pxa_linear_f32_bwd", ptr(dy), ptr(x), ptr(w), ptr(dx), ptr(dw), ptr(db), M, N, K)
    return dx, (dw if need_dw else None), db


def cast_bf16(x, out=None):
    if out is None:
        out = torch.empty(x.shape, dtype=BF16, device=x.device)
    call("pxa_cast_f32_bf16", ptr(x), ptr(out), x.numel())
    return out


# ------------------------------------------------------------------------------------------------ LoRA adapters
LORA_MAX_RANK = 64
_LORA_WS = {}


def lora_merge(master, lo, hi, A, Bt, s, dst, dst2=None, mul_rows=(0, 0), mul=1.0, dst_f32=None):
    """Rows [lo, hi) of dst <- round16(master + s * Bt^T A) (pxa_lora_merge): master (rows, K) fp32, dst its 16-bit copy (same rows), A (r, K) and
    Bt (r, hi - lo) fp32.  dst2: optional second 16-bit copy whose rows in mul_rows carry `mul` (the q-prescaled qkv copy); dst_f32: optional fp32
    destination laid out as master (master itself: merge_and_unload)."""
    _chk(master, F32, "master"); _chk(A, F32, "A"); _chk(Bt, F32, "Bt"); _chk(dst, BF16, "dst")
    r, K = A.shape
    assert master.dim() == 2 and master.shape[1] == K and tuple(dst.shape) == tuple(master.shape) and 0 <= lo < hi <= master.shape[0]
    assert tuple(Bt.shape) == (r, hi - lo) and A.is_contiguous(), "lora_merge: A (r, K) contiguous, Bt (r, hi - lo)"
    if dst2 is not None:
        _chk(dst2, BF16, "dst2")
        assert tuple(dst2.shape) == tuple(master.shape)
    if dst_f32 is not None:
        _chk(dst_f32, F32, "dst_f32")
        assert tuple(dst_f32.shape) == tuple(master.shape) and dst_f32.stride(0) == master.stride(0)
    call("pxa_lora_merge", ptr(master), master.stride(0), lo, hi, K, ptr(A), ptr(Bt), Bt.stride(0), r, float(s), ptr(dst), dst.stride(0),
         ptr(dst2), dst2.stride(0) if dst2 is not None else 0, int(mul_rows[0]), int(mul_rows[1]), float(mul), ptr(dst_f32))


def lora_bwd(x, dy, A16, Bt16, s, dA, dBt):
    """dA += s u^T x, dBt += s t^T dy with t = x A16^T, u = dy Bt16^T rounded once to the operand type (pxa_lora_bwd).  x (M, K), dy (M, N) 16-bit with unit
    column stride (dy may be a column block of a wider matrix); A16 (r, K), Bt16 (r, N) the adapters' 16-bit copies; dA (r, K), dBt (r, N) fp32.  The workspace
    is cached per (device, stream): the call's kernels run on one stream and the last one has read it before the next call's first writes."""
    for name, t in (("x", x), ("dy", dy), ("A16", A16), ("Bt16", Bt16)):
        _chk(t, BF16, name)
    _chk(dA, F32, "dA"); _chk(dBt, F32, "dBt")
    M, K = x.shape
    N, r = dy.shape[1], A16.shape[0]
    assert dy.shape[0] == M and tuple(A16.shape) == (r, K) and tuple(Bt16.shape) == (r, N) and tuple(dA.shape) == (r, K) and tuple(dBt.shape) == (r, N)
    assert A16.is_contiguous() and Bt16.is_contiguous() and dA.is_contiguous() and dBt.is_contiguous()
    need = lib.load().pxa_lora_bwd_ws_bytes(M, K, N, r)
    if need < 0:
        raise lib.PixartHipError(f"pxa_lora_bwd: no workspace size for M={M}, K={K}, N={N}, r={r} (1 <= r <= {LORA_MAX_RANK})")
    if torch.cuda.is_current_stream_capturing():
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    else:
        key = (x.device, torch.cuda.current_stream(x.device).cuda_stream)
        ws = _LORA_WS.get(key)
        if ws is None or ws.numel() < need:
            ws = _LORA_WS[key] = torch.empty(need, dtype=torch.uint8, device=x.device)
    call("pxa_lora_bwd", ptr(x), x.stride(0), ptr(dy), dy.stride(0), ptr(A16), ptr(Bt16), M, K, N, r, float(s), ptr(dA), ptr(dBt), ptr(ws), ws.numel())


# ------------------------------------------------------------------------------------------------ images
U8, I32 = torch.uint8, torch.int32


def image_resample(src, resized, window, out, htab=None, vtab=None, rows=None, lut=None, ws=None):
    """The window (cy, cx, ch, cw) of `src` resized to resized = (Hr, Wr) by Pillow's 8-bit resampler (pxa_image_resample).  src: uint8 (h, w, 3), pixels
    contiguous, any row pitch >= 3 w.  htab = (coefficients int32 (ksize, Wr) tap-major, bounds int32 (Wr, 2)) or None when Wr == w; vtab = (coefficients int32
    (Hr, ksize), bounds int32 (Hr, 2)) or None when Hr == h; rows = (row0, count), the source rows the window's vertical taps reach (with vtab).  out: an fp32
    (3, ch, cw) contiguous slot of a batch (needs lut, the 256 fp32 values a byte maps to) or a uint8 (ch, cw, 3) view with any row pitch.  ws: uint8 workspace
    for the intermediate image, allocated here when both passes run and none is given.  Returns out."""
    assert src.is_cuda and src.dtype == U8 and src.dim() == 3 and src.shape[2] == 3 and src.stride(2) == 1 and src.stride(1) == 3, "src: uint8 (h, w, 3) on the GPU"
    h, w = src.shape[:2]
    Hr, Wr = (int(v) for v in resized)
    cy, cx, ch, cw = (int(v) for v in window)
    assert src.stride(0) >= 3 * w and 0 <= cy and 0 <= cx and ch >= 1 and cw >= 1 and cy + ch <= Hr and cx + cw <= Wr, "window outside the resized image"
    hk = hb = vk = vb = None
    hks = vks = 0
    if htab is not None:
        hk, hb = htab
        _chk(hk, I32, "htab coefficients"); _chk(hb, I32, "htab bounds")
        hks = hk.shape[0]
        assert hk.is_contiguous() and hb.is_contiguous() and tuple(hk.shape) == (hks, Wr) and tuple(hb.shape) == (Wr, 2), "htab: (ksize, Wr) and (Wr, 2)"
    else:
        assert Wr == w, "no horizontal tables: the width must not change"
    row0, nrows = cy, ch
    if vtab is not None:
        vk, vb = vtab
        _chk(vk, I32, "vtab coefficients"); _chk(vb, I32, "vtab bounds")
        vks = vk.shape[1]
        assert vk.is_contiguous() and vb.is_contiguous() and tuple(vk.shape) == (Hr, vks) and tuple(vb.shape) == (Hr, 2), "vtab: (Hr, ksize) and (Hr, 2)"
        assert rows is not None, "vtab needs rows = (first source row, count)"
        row0, nrows = (int(v) for v in rows)
        assert 0 <= row0 and nrows >= 1 and row0 + nrows <= h, "rows outside the source"
    else:
        assert Hr == h, "no vertical tables: the height must not change"
    need = 0
    if htab is not None and vtab is not None:
        need = lib.load().pxa_image_resample_ws_bytes(nrows, cw)
        if ws is None:
            ws = torch.empty(need, dtype=U8, device=src.device)
        assert ws.is_cuda and ws.dtype == U8 and ws.is_contiguous() and ws.numel() >= need, f"ws: {need} uint8 on the GPU"
    out_f32 = out_u8 = None
    pitch = 0
    if out.dtype == F32:
        assert out.is_cuda and tuple(out.shape) == (3, ch, cw) and out.is_contiguous(), "out: fp32 (3, ch, cw) contiguous"
        assert lut is not None and lut.is_cuda and lut.dtype == F32 and lut.numel() == 256 and lut.is_contiguous(), "fp32 output needs the 256-entry table"
        out_f32 = out
    else:
        assert out.is_cuda and out.dtype == U8 and tuple(out.shape) == (ch, cw, 3) and out.stride(2) == 1 and out.stride(1) == 3 and out.stride(0) >= 3 * cw, \
            "out: uint8 (ch, cw, 3), pixels contiguous"
        out_u8, pitch = out, out.stride(0)
    call("pxa_image_resample", ptr(src), src.stride(0), h, w, ptr(hk), ptr(hb), hks, Wr, ptr(vk), ptr(vb), vks, Hr, cy, cx, ch, cw, row0, nrows,
         ptr(ws) if need else None, ws.numel() if need else 0, ptr(out_f32), ptr(lut) if out_f32 is not None else None, ptr(out_u8), pitch)
    return out


def image_to_u8(x, out=None):
    """(B, 3, H, W) fp16 / fp32 in [-1, 1] -> uint8 (B, H, W, 3): torchvision.utils.save_image(normalize=True, value_range=(-1, 1))'s
    clamp, (x + 1) / 2, * 255 + 0.5, clamp, truncate (pxa_image_to_u8).  The arithmetic is fp32 whatever the input type; the reference does it in the tensor's own
    dtype, so an fp16 input can differ from it by one step where the fp16 product rounds across an integer."""
    assert x.is_cuda and x.dim() == 4 and x.shape[1] == 3 and x.dtype in (torch.float16, F32) and x.is_contiguous(), "x: (B, 3, H, W) fp16 / fp32 contiguous on the GPU"
    B, _, H, W = x.shape
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=U8, device=x.device)
    assert out.is_cuda and out.dtype == U8 and tuple(out.shape) == (B, H, W, 3) and out.is_contiguous()
    call("pxa_image_to_u8", ptr(x), int(x.dtype == torch.float16), B, H, W, ptr(out))
    return out


# ------------------------------------------------------------------------------------------------ VAE conv stack
class Grid:
    """A bf16 NHWC pixel grid (pxa_grid): pixel (b, y, x) is the C-vector at buf[(b*img_pitch + y*row_pitch + x + origin) * C]."""

    def __init__(self, buf, B, H, W, C, row_pitch=None, img_pitch=None, origin=0):
        _chk(buf, BF16, "grid buffer")
        self.buf, self.B, self.H, self.W, self.C = buf, B, H, W, C
        self.row_pitch = W if row_pitch is None else row_pitch
        self.img_pitch = H * W if img_pitch is None else img_pitch
        self.origin = origin

    @classmethod
    def compact(cls, B, H, W, C, device):
        return cls(torch.empty(B * H * W, C, dtype=BF16, device=device), B, H, W, C)

    @property
    def is_compact(self):
        return self.origin == 0 and self.row_pitch == self.W and self.img_pitch == self.H * self.W

    def rows(self):
        """(pixels, C) matrix over every pixel slot of the grid (border slots of a padded-grid view included)."""
        return self.buf.view(-1, self.C)[: self.B * self.img_pitch] if not self.is_compact else self.buf.view(-1, self.C)

    def like_rows(self, out, C):
        """The grid of a row-wise op's output: same pixel slots, C channels."""
        return Grid(out, self.B, self.H, self.W, C, self.row_pitch, self.img_pitch, self.origin)

    def arg(self):
        g = GridArg()
        g.ptr, g.B, g.H, g.W, g.C = ptr(self.buf), self.B, self.H, self.W, self.C
        g.row_pitch, g.img_pitch, g.origin = self.row_pitch, self.img_pitch, self.origin
        return g


_GN_WS = {}


def vae_gn_stats(x, groups, eps):
    """GroupNorm statistics of a grid: (mean, rstd), each (B*groups,) fp32."""
    dev = x.buf.device
    ws = _GN_WS.get((dev, x.B * groups))
    if ws is None:
        ws = _GN_WS[(dev, x.B * groups)] = torch.empty(x.B * groups * 2, dtype=torch.float64, device=dev)
    mean = torch.empty(x.B * groups, dtype=F32, device=dev)
    rstd = torch.empty_like(mean)
    call("pxa_vae_gn_stats", x.arg(), groups, eps, ptr(ws), ptr(mean), ptr(rstd))
    return mean, rstd


def vae_gn_finalize(part, B, C, groups, pixels, eps):
    """(mean, rstd) from the per-channel partial sums a convolution epilogue accumulated (gemm(..., gn_part=...))."""
    mean = torch.empty(B * groups, dtype=F32, device=part.device)
    rstd = torch.empty_like(mean)
    call("pxa_vae_gn_finalize", ptr(part), B, C, groups, pixels, eps, ptr(mean), ptr(rstd))
    return mean, rstd


def vae_gn_apply(x, y, norm=None, silu=False, upsample=1):
    """y = act(norm(x)) (optionally 2x nearest upsampled).  norm = (mean, rstd, gamma, beta, groups) or None."""
    mean, rstd, gamma, beta, groups = norm if norm is not None else (None, None, None, None, 1)
    call("pxa_vae_gn_apply", x.arg(), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), groups, int(silu), upsample, y.arg())
    return y


def vae_im2col3x3(x, stride, pad, Ho, Wo, norm=None, silu=False):
    mean, rstd, gamma, beta, groups = norm if norm is not None else (None, None, None, None, 1)
    col = torch.empty(x.B * Ho * Wo, 9 * x.C, dtype=BF16, device=x.buf.device)
    call("pxa_vae_im2col3x3", x.arg(), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), groups, int(silu), stride, pad, Ho, Wo, ptr(col))
    return col


def vae_add(a, b, out):
    call("pxa_vae_add", a.arg(), b.arg(), out.arg())
    return out


def vae_softmax_rows(s, scale, out=None):
    _chk(s, F32, "scores")
    rows, cols = s.shape
    if out is None:
        out = torch.empty(rows, cols, dtype=BF16, device=s.device)
    call("pxa_vae_softmax_rows", ptr(s), s.stride(0), ptr(out), out.stride(0), rows, cols, scale)
    return out


def vae_attention(q, k, v, B, HW, scale, out=None):
    """softmax(scale * q[b] k[b]^T) v[b] for B images of HW tokens in one streaming launch (pxa_vae_attn): (B*HW, C) of the operand type.  q, k, v: (B*HW, C)
    with unit column stride and any row stride (e.g. the column slices of the packed qkv projection); C = 512 or 256; no score buffers, no scratch."""
    rows, C = q.shape
    for name, x in (("q", q), ("k", k), ("v", v)):
        _chk(x, BF16, name)
        assert tuple(x.shape) == (B * HW, C) and x.stride(1) == 1, f"vae_attention: {name} must be (B*HW, C) with unit column stride"
    if out is None:
        out = torch.empty(rows, C, dtype=BF16, device=q.device)
    _chk(out, BF16, "out")
    assert tuple(out.shape) == (rows, C) and out.stride(1) == 1
    call("pxa_vae_attn", ptr(q), ptr(k), ptr(v), q.stride(0), k.stride(0), v.stride(0), ptr(out), out.stride(0), B, HW, C, scale)
    return out


# ------------------------------------------------------------------------------------------------ T5 text encoder
T5_MAX_L, T5_MAX_H, T5_HEAD_DIM = 512, 64, 64


def t5_embed(ids, table, out=None):
    """out[r] = float(table[ids[r]]) (pxa_t5_embed).  ids: int32 (R,), table: (vocab, D) of the operand type; returns fp32 (R, D)."""
    _chk(table, BF16, "table")
    assert ids.is_cuda and ids.dtype == torch.int32 and ids.dim() == 1 and ids.is_contiguous() and table.is_contiguous()
    R, (vocab, D) = ids.numel(), table.shape
    if out is None:
        out = torch.empty(R, D, dtype=F32, device=table.device)
    _chk(out, F32, "out")
    assert tuple(out.shape) == (R, D) and out.is_contiguous()
    call("pxa_t5_embed", ptr(ids), ptr(table), ptr(out), R, D, vocab)
    return out


def t5_rmsnorm(x, w, eps=1e-6, out=None, out_f32=None, want_bf16=True, want_f32=False):
    """T5LayerNorm rows (pxa_t5_rmsnorm): x (R, D) fp32, w (D,) fp32.  Returns (operand-type output or None, fp32 output or None)."""
    _chk(x, F32, "x")
    _chk(w, F32, "w")
    R, D = x.shape
    assert x.is_contiguous() and w.numel() == D
    if out is None and want_bf16:
        out = torch.empty(R, D, dtype=BF16, device=x.device)
    if out_f32 is None and want_f32:
        out_f32 = torch.empty(R, D, dtype=F32, device=x.device)
    if out is not None:
        _chk(out, BF16, "out")
        assert tuple(out.shape) == (R, D) and out.is_contiguous()
    if out_f32 is not None:
        _chk(out_f32, F32, "out_f32")
        assert tuple(out_f32.shape) == (R, D) and out_f32.is_contiguous()
    call("pxa_t5_rmsnorm", ptr(x), ptr(w), ptr(out), ptr(out_f32), R, D, eps)
    return out, out_f32


def t5_attention(q, k, v, bias, kv_len, B, H, L, out=None):
    """softmax(q k^T + bias[h][j - i] + key mask) v per (sample, head), head_dim 64, no scale (pxa_t5_attn).  q, k, v: (B*L, H*64) of the operand type with unit
    column stride and any row stride (the column slices of the packed projection); bias: fp32 (H, 2L - 1); kv_len: int32 (B,) on the device."""
    W = H * T5_HEAD_DIM
    for name, x in (("q", q), ("k", k), ("v", v)):
        _chk(x, BF16, name)
        assert tuple(x.shape) == (B * L, W), f"t5_attention: {name} must be (B*L, H*64)"
    _chk(bias, F32, "bias")
    assert tuple(bias.shape) == (H, 2 * L - 1) and bias.is_contiguous()
    assert kv_len.is_cuda and kv_len.dtype == torch.int32 and kv_len.numel() == B and kv_len.is_contiguous()
    if out is None:
        out = torch.empty(B * L, W, dtype=BF16, device=q.device)
    _chk(out, BF16, "out")
    assert tuple(out.shape) == (B * L, W)
    a = T5AttnArgs()
    a.q, a.k, a.v, a.o = ptr(q), ptr(k), ptr(v), ptr(out)
    a.ldq, a.ldk, a.ldv, a.ldo = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
    a.bias, a.kv_len = ptr(bias), ptr(kv_len)
    a.B, a.H, a.L, a.head_dim = B, H, L, T5_HEAD_DIM
    call("pxa_t5_attn", C.byref(a))
    return out


# ------------------------------------------------------------------------------------------------ FP8 (e4m3fn) weights of the T5 encoder
FP8 = torch.float8_e4m3fn


def _chk_fp8(q, scale, cuda=True):
    assert (q.is_cuda or not cuda) and q.dtype == FP8 and q.dim() == 2 and q.stride(1) == 1, "q: need a 2-D contiguous-last-dim float8_e4m3fn CUDA tensor"
    _chk(scale, F32, "scale", cuda=cuda)
    assert scale.dim() == 1 and scale.numel() == q.shape[0], f"scale: need ({q.shape[0]},) fp32, got {tuple(scale.shape)}"


def fp8_quant_rows(w, q=None, scale=None):
    """The project's FP8 quantiser (pxa_fp8_quant_rows): w (N, K) of the operand type or fp32 -> (q (N, K) float8_e4m3fn, scale (N,) fp32) with
    scale[n] = 2^ceil(log2(max_k |w[n][k]| / 448)) (1 for an all-zero row) and q = e4m3fn(w / scale), round to nearest even, saturating at +-448."""
    assert w.is_cuda and w.dim() == 2 and w.stride(1) == 1 and w.dtype in (BF16, F32), f"fp8_quant_rows: need a 2-D CUDA tensor of {BF16} or fp32, got {w.dtype}"
    N, K = w.shape
    if q is None:
        q = torch.empty(N, K, dtype=FP8, device=w.device)
    if scale is None:
        scale = torch.empty(N, dtype=F32, device=w.device)
    _chk_fp8(q, scale)
    assert tuple(q.shape) == (N, K)
    call("pxa_fp8_quant_rows", ptr(w), int(w.dtype == F32), w.stride(0), N, K, ptr(q), q.stride(0), ptr(scale))
    return q, scale


def fp8_dequant_rows(q, scale, out=None):
    """out[n][k] = scale[n] * q[n][k] rounded once to the operand type (pxa_fp8_dequant_rows): exact for a power-of-two scale.  out may be a (N, K) view of a
    larger buffer (the encoder's one scratch matrix)."""
    _chk_fp8(q, scale)
    N, K = q.shape
    if out is None:
        out = torch.empty(N, K, dtype=BF16, device=q.device)
    _chk(out, BF16, "out")
    assert tuple(out.shape) == (N, K)
    call("pxa_fp8_dequant_rows", ptr(q), q.stride(0), ptr(scale), N, K, ptr(out), out.stride(0))
    return out


def gemm_w8_max_m():
    return lib.load().pxa_gemm_w8_max_m()


_W8_SOMEWHERE = (C.c_char * 32)()


def _gemm_w8_args(plan, a, q, scale, act, aux, out, out_f32):
    def chk(t, dtype, name):
        if not isinstance(t, _Unallocated):
            _chk(t, dtype, name, cuda=not plan)

    def ptr(t):                    # the plan entry tests alignment: a 16-byte aligned address stands for a buffer gemm_w8 would allocate
        return C.c_void_p((C.addressof(_W8_SOMEWHERE) + 15) & ~15) if isinstance(t, _Unallocated) else lib.ptr(t, cuda=not plan)
    chk(a, BF16, "A")
    _chk_fp8(q, scale, cuda=not plan)
    M, K = a.shape
    N, K2 = q.shape
    assert K == K2, f"gemm_w8: K mismatch {K} vs {K2}"
    g = lib.GemmW8Args()
    g.A, g.lda, g.q, g.ldq, g.scale = ptr(a), a.stride(0), ptr(q), q.stride(0), ptr(scale)
    g.M, g.N, g.K, g.act = M, N, K, act
    if act == ACT_MUL_AUX:
        chk(aux, BF16, "aux")
        assert tuple(aux.shape) == (M, N)
        g.aux, g.ldaux = ptr(aux), aux.stride(0)
    if out_f32 is not None:
        assert out is None, "gemm_w8: out and out_f32 exclude each other"
        chk(out_f32, F32, "out_f32")
        assert tuple(out_f32.shape) == (M, N)
        g.out_f32, g.ld_f32 = ptr(out_f32), out_f32.stride(0)
        return g, out_f32
    if out is None:
        out = _Unallocated(M, N, BF16) if plan else torch.empty((M, N), dtype=BF16, device=a.device)
    chk(out, BF16, "out")
    assert tuple(out.shape) == (M, N)
    g.out16, g.ld_out = ptr(out), out.stride(0)
    return g, out


def gemm_w8(a, q, scale, act=ACT_NONE, aux=None, out=None, out_f32=None):
    """scale[n] * sum_k a[m][k] q[n][k] with FP8 weights streamed against 16-bit activations (pxa_gemm_w8).  a (M, K) operand type, q (N, K) float8_e4m3fn,
    scale (N,) fp32.  act: ACT_NONE, ACT_GELU or ACT_MUL_AUX (with aux (M, N)) into a 16-bit `out` (allocated if not given), or out_f32 (M, N) fp32 given:
    out_f32 += the product.  Returns the tensor written."""
    g, res = _gemm_w8_args(False, a, q, scale, act, aux, out, out_f32)
    call("pxa_gemm_w8", C.byref(g))
    return res


def gemm_w8_plan(a, q, scale, act=ACT_NONE, aux=None, out=None, out_f32=None):
    """pxa_gemm_w8_plan's line for the call gemm_w8 would make (kernel instance, split, tiles); raises what gemm_w8 would raise for a call the library
    refuses.  Needs no GPU: the tensors may live on any device."""
    g, _ = _gemm_w8_args(True, a, q, scale, act, aux, out, out_f32)
    buf = C.create_string_buffer(256)
    lib.check(lib.load().pxa_gemm_w8_plan(C.byref(g), buf, len(buf)), "pxa_gemm_w8_plan")
    return buf.value.decode()


# ------------------------------------------------------------------------------------------------ MXFP8 (e4m3fn + one E8M0 scale per 32 k) for denoiser inference
U8 = torch.uint8


def _chk_mx(q, e, name, cuda=True):
    assert (q.is_cuda or not cuda) and q.dtype == FP8 and q.dim() == 2 and q.stride(1) == 1, f"{name}: q needs a 2-D contiguous-last-dim float8_e4m3fn CUDA tensor"
    assert q.shape[1] % 32 == 0, f"{name}: K={q.shape[1]} must be a multiple of 32"
    _chk(e, U8, f"{name} scales", cuda=cuda)
    assert tuple(e.shape) == (q.shape[0], q.shape[1] // 32), f"{name}: e needs ({q.shape[0]}, {q.shape[1] // 32}) uint8, got {tuple(e.shape)}"


def mx_quant_rows(x, q=None, e=None):
    """The project's MXFP8 quantiser (pxa_mx_quant_rows): x (R, K) of the operand type or fp32, K % 32 == 0 -> (q (R, K) float8_e4m3fn, e (R, K / 32) uint8, E8M0)
    with, per block of 32 consecutive k, X = ceil(log2(amax / 448)) (0 for an all-zero block, clamped to [-127, 127]), e = X + 127, q = e4m3fn(x / 2^X)."""
    assert x.is_cuda and x.dim() == 2 and x.stride(1) == 1 and x.dtype in (BF16, F32), f"mx_quant_rows: need a 2-D CUDA tensor of {BF16} or fp32, got {x.dtype}"
    R, K = x.shape
    assert K % 32 == 0, f"mx_quant_rows: K={K} must be a multiple of 32"
    if q is None:
        q = torch.empty(R, K, dtype=FP8, device=x.device)
    if e is None:
        e = torch.empty(R, K // 32, dtype=U8, device=x.device)
    _chk_mx(q, e, "mx_quant_rows")
    assert tuple(q.shape) == (R, K)
    call("pxa_mx_quant_rows", ptr(x), int(x.dtype == F32), x.stride(0), R, K, ptr(q), q.stride(0), ptr(e), e.stride(0))
    return q, e


def mx_dequant_rows(q, e, out=None):
    """out[r][k] = q[r][k] * 2^(e[r][k / 32] - 127) in the operand type (pxa_mx_dequant_rows): the exact inverse of mx_quant_rows' scaling."""
    _chk_mx(q, e, "mx_dequant_rows")
    R, K = q.shape
    if out is None:
        out = torch.empty(R, K, dtype=BF16, device=q.device)
    _chk(out, BF16, "out")
    assert tuple(out.shape) == (R, K)
    call("pxa_mx_dequant_rows", ptr(q), q.stride(0), ptr(e), e.stride(0), R, K, ptr(out), out.stride(0))
    return out


def _gemm_f8_args(plan, qa, ea, qw, ew, bias, act, out, out_q, out_e, out16, mx):
    def ptr(t):                    # the plan entry tests alignment: a 16-byte aligned address stands for a buffer gemm_f8 would allocate
        return C.c_void_p((C.addressof(_W8_SOMEWHERE) + 15) & ~15) if isinstance(t, _Unallocated) else lib.ptr(t, cuda=not plan)
    _chk_mx(qa, ea, "gemm_f8: A", cuda=not plan)
    _chk_mx(qw, ew, "gemm_f8: W", cuda=not plan)
    M, K = qa.shape
    N, K2 = qw.shape
    assert K == K2, f"gemm_f8: K mismatch {K} vs {K2}"
    g = lib.GemmF8Args()
    g.qa, g.ldqa, g.ea, g.ldea = ptr(qa), qa.stride(0), ptr(ea), ea.stride(0)
    g.qw, g.ldqw, g.ew, g.ldew = ptr(qw), qw.stride(0), ptr(ew), ew.stride(0)
    g.M, g.N, g.K, g.act = M, N, K, act
    if bias is not None:
        _chk(bias, F32, "bias", cuda=not plan)
        assert bias.numel() == N
        g.bias = ptr(bias)
    assert (out_q is None) == (out_e is None), "gemm_f8: out_q and out_e go together"
    if out16 or out is not None:
        if out is None:
            out = _Unallocated(M, N, BF16) if plan else torch.empty((M, N), dtype=BF16, device=qa.device)
        if not isinstance(out, _Unallocated):
            _chk(out, BF16, "out", cuda=not plan)
        assert tuple(out.shape) == (M, N)
        g.out16, g.ld_out = ptr(out), out.stride(0)
    if mx or out_q is not None:
        if out_q is None:
            out_q = _Unallocated(M, N, FP8) if plan else torch.empty((M, N), dtype=FP8, device=qa.device)
            out_e = _Unallocated(M, N // 32, U8) if plan else torch.empty((M, N // 32), dtype=U8, device=qa.device)
        if not isinstance(out_q, _Unallocated):
            _chk_mx(out_q, out_e, "gemm_f8: out", cuda=not plan)
        assert tuple(out_q.shape) == (M, N)
        g.out_q, g.ld_outq, g.out_e, g.ld_oute = ptr(out_q), out_q.stride(0), ptr(out_e), out_e.stride(0)
    return g, out, out_q, out_e


def gemm_f8(qa, ea, qw, ew, bias=None, act=ACT_NONE, out=None, out_q=None, out_e=None, out16=True, mx=False):
    """act(sum_k A[m][k] W[n][k] + bias[n]) with both operands in MXFP8 on the block-scaled K = 128 MFMA (pxa_gemm_f8).  A = (qa (M, K), ea (M, K / 32)),
    W = (qw (N, K), ew (N, K / 32)); N and K multiples of 128; bias (N,) fp32 or None; act ACT_NONE or ACT_GELU.  out16: write the 16-bit result (`out`, allocated
    if not given); mx (or out_q / out_e given): also, or only, write that 16-bit-rounded result quantised along N by mx_quant_rows' rule.  Returns `out` where only
    the 16-bit result is asked for, (out_q, out_e) where only the quantised one is, (out, out_q, out_e) for both."""
    g, out, out_q, out_e = _gemm_f8_args(False, qa, ea, qw, ew, bias, act, out, out_q, out_e, out16, mx)
    call("pxa_gemm_f8", C.byref(g))
    if out_q is None:
        return out
    return (out_q, out_e) if out is None else (out, out_q, out_e)


def gemm_f8_plan(qa, ea, qw, ew, bias=None, act=ACT_NONE, out=None, out_q=None, out_e=None, out16=True, mx=False):
    """pxa_gemm_f8_plan's line for the call gemm_f8 would make (kernel instance, tile, grid); raises what gemm_f8 would raise for a call the library refuses.
    Needs no GPU: the tensors may live on any device."""
    g, *_ = _gemm_f8_args(True, qa, ea, qw, ew, bias, act, out, out_q, out_e, out16, mx)
    buf = C.create_string_buffer(256)
    lib.check(lib.load().pxa_gemm_f8_plan(C.byref(g), buf, len(buf)), "pxa_gemm_f8_plan")
    return buf.value.decode()


def vae_nchw_to_grid(img, y, mul=1.0):
    _chk(img, F32, "image")
    assert img.is_contiguous() and img.shape[0] == y.B and img.shape[2] == y.H and img.shape[3] == y.W
    call("pxa_vae_nchw_to_grid", ptr(img), img.shape[1], mul, y.arg())
    return y


def vae_conv3x3_small_out(x, w_taps, bias, Cout, norm=None, silu=False):
    """fp32 NCHW image (B, Cout, H, W) = conv3x3(act(norm(x))) for Cout <= 4 (decoder conv_out); w_taps (9, Cout, C) in the operand type."""
    mean, rstd, gamma, beta, groups = norm if norm is not None else (None, None, None, None, 1)
    _chk(w_taps, BF16, "w_taps")
    assert w_taps.is_contiguous() and tuple(w_taps.shape) == (9, Cout, x.C)
    img = torch.empty(x.B, Cout, x.H, x.W, dtype=F32, device=x.buf.device)
    call("pxa_vae_conv3x3_small_out", x.arg(), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), groups, int(silu), ptr(w_taps), ptr(bias), Cout, ptr(img))
    return img


def vae_grid_to_nchw(x, C):
    img = torch.empty(x.B, C, x.H, x.W, dtype=F32, device=x.buf.device)
    call("pxa_vae_grid_to_nchw", x.arg(), C, ptr(img))
    return img


def vae_posterior(moments, B, H, W, latent_channels, eps=None, scale=1.0, out=None):
    """x0 (B, latent_channels, H, W) fp32 = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * eps) from the fp32 moments of quant_conv in the padded-grid
    layout of its input (rows of _c8(2 * latent_channels) floats; origin W + 3, row pitch W + 2, image pitch = rows per image): pxa_vae_posterior, one launch.
    eps: fp32 NCHW noise the caller drew (None: the mode, scale * mean)."""
    _chk(moments, F32, "moments")
    assert moments.dim() == 2 and moments.is_contiguous() and moments.shape[0] % B == 0, "moments: (B * img_pitch, channel stride) fp32 rows"
    ip, cs = moments.shape[0] // B, moments.shape[1]
    assert ip >= (H + 2) * (W + 2) and cs >= 2 * latent_channels, f"moments of {tuple(moments.shape)} for {B} padded grids of {H} x {W} x {2 * latent_channels}"
    if eps is not None:
        _chk(eps, F32, "eps")
        assert eps.is_contiguous() and tuple(eps.shape) == (B, latent_channels, H, W), f"eps must be fp32 NCHW {(B, latent_channels, H, W)}"
    if out is None:
        out = torch.empty(B, latent_channels, H, W, dtype=F32, device=moments.device)
    _chk(out, F32, "x0")
    assert out.is_contiguous() and tuple(out.shape) == (B, latent_channels, H, W)
    call("pxa_vae_posterior", ptr(moments), B, H, W, latent_channels, cs, W + 2, ip, W + 3, ptr(eps), float(scale), ptr(out))
    return out
