"""Host-side orchestration of the PixArt-Sigma denoiser on the HIP kernels: which kernel runs when, which
activations are kept for backward, where weight gradients land.  Pure sequencing — all arithmetic is in
libpixart_hip.so (ops.py -> C ABI).  Mirrors the dataflow of PixArtMS.forward / PixArtMSBlock.forward
(reference diffusion/model/nets/PixArtMS.py:71-79,165-211) with these fusions:

  block l:  x_in  = x2[l-1] + gate_mlp[l-1]*u3[l-1] ; xn1 = LN(x_in)(1+scale_msa)+shift_msa      (ln_mod_fwd, 1 pass)
            qkv   = xn1 Wqkv^T + b                                                                (gemm NT)
            a     = softmax(q k^T/sqrt(hd)) v          [k,v optionally KV-compressed]             (attn_fwd)
            u1    = a Wproj^T + b                                                                 (gemm NT)
            x1    = x_in + gate_msa*u1 ; x1b = bf16(x1)                                           (ln_mod_fwd, no LN)
            qc    = x1b Wq^T + b ; kvc = y Wkv^T + b ; c = varlen-attn(qc, kvc) ; u2 = c Wcp^T+b  (gemm, attn_fwd, gemm)
            x2    = x1 + u2 ; xn2 = LN(x2)(1+scale_mlp)+shift_mlp                                 (ln_mod_fwd)
            h     = gelu(xn2 W1^T + b)  (pre-activation kept) ; u3 = h W2^T + b                   (gemm+GELU, gemm)
  final:    x3 = x2 + gate_mlp*u3 ; LN+modulate ; Linear(D,32) ; unpatchify

The residual stream, LayerNorm statistics, softmax and all accumulators are fp32; GEMM / attention operands and the
stored branch activations are bf16 (DESIGN.md "Numerics").  Backward is hand-sequenced (no autograd inside): weight
gradients are accumulated straight into the flat fp32 gradient buffer (ParamStore.grad).
"""
import collections
import dataclasses
import os
import typing
import weakref

import numpy as np
import torch

from . import ops
from .ops import BF16, F32, NN, NT, TN


def sincos_pos_embed(embed_dim, h, w, pe_interpolation, base_size):
    """Host float64 table, same arithmetic as the reference's get_2d_sincos_pos_embed (PixArt.py:258-307):
    float32 grid coordinates, float64 omega/sin/cos, w (column) coordinate in the first half.  Cached per geometry
    on the device instead of being rebuilt in numpy on every forward (PixArtMS.py:177-182)."""
    grid_h = np.arange(h, dtype=np.float32) / (h / base_size) / pe_interpolation
    grid_w = np.arange(w, dtype=np.float32) / (w / base_size) / pe_interpolation
    gw, gh = np.meshgrid(grid_w, grid_h)
    quarter = embed_dim // 4
    omega = np.arange(quarter, dtype=np.float64)
    omega /= embed_dim / 4.0
    omega = 1.0 / 10000 ** omega

    def enc(pos):
        out = np.einsum("m,d->md", pos.reshape(-1), omega)
        return np.concatenate([np.sin(out), np.cos(out)], axis=1)
    return np.concatenate([enc(gw), enc(gh)], axis=1)


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class ParamStore:
    """All model parameters in ONE flat fp32 buffer (master), ONE flat fp32 gradient buffer and ONE flat bf16 shadow
    (the GEMM operands), sharing offsets.  nn.Parameters are re-pointed to views of the master so optimizers, state
    dicts and the data-parallel all-reduce see ordinary tensors, while the fused AdamW / grad-norm / all-reduce kernels
    work on contiguous ranges.  Order = forward order (embedders, block 0..L-1, final layer) so a block's gradients are a
    contiguous bucket that completes at a known point of the hand-sequenced backward."""
    ALIGN = 64

    def __init__(self, named_params, device, group_of=None):
        """group_of: optional name -> group label; consecutive parameters with one label form a bucket (store.groups)."""
        self.names, self.offset, self.shape, self.numel = [], {}, {}, {}
        self.groups = {}
        off = 0
        for name, p in named_params:
            self.names.append(name)
            self.offset[name], self.shape[name], self.numel[name] = off, tuple(p.shape), p.numel()
            end = self._end(name)
            if group_of is not None:
                gname = group_of(name)
                if gname in self.groups:
                    assert self.groups[gname][1] == off, f"group {gname} is not contiguous at {name}"
                    self.groups[gname] = (self.groups[gname][0], end)
                else:
                    self.groups[gname] = (off, end)
            off = end
        self.total = off
        self.device = device
        self.master = torch.zeros(off, dtype=F32, device=device)
        self.grad = torch.zeros(off, dtype=F32, device=device)
        self.shadow = torch.zeros(off, dtype=BF16, device=device)
        self.params = dict(named_params)
        self._versions = None
        self.generation = 0        # bumped whenever the shadow weights change (re-cast here, fused optimizer steps): keys everything cached from them
        self._on_change = []       # callables run at every bump: buffers DERIVED from the weights are rewritten in place there (Engine._refresh_qs)
        for name, p in named_params:
            v = self.view(self.master, name)
            v.copy_(p.data)
            p.data = v
            p.grad = self.view(self.grad, name)

    def _end(self, name):
        """End of the parameter's aligned slot = offset of the one behind it."""
        return self.offset[name] + (self.numel[name] + self.ALIGN - 1) // self.ALIGN * self.ALIGN

    def view(self, flat, name):
        o = self.offset[name]
        return flat[o:o + self.numel[name]].view(self.shape[name])

    def w(self, name):   # bf16 shadow weight (2-D)
        return self.view(self.shadow, name)

    def f(self, name):   # fp32 master (bias / table)
        return self.view(self.master, name)

    def g(self, name):   # fp32 gradient accumulator
        return self.view(self.grad, name)

    def range_of(self, prefix):
        """[start, end) element range of all parameters whose name starts with prefix (contiguous by construction)."""
        idx = [i for i, n in enumerate(self.names) if n.startswith(prefix)]
        assert idx and idx == list(range(idx[0], idx[-1] + 1)), prefix
        return self.offset[self.names[idx[0]]], self._end(self.names[idx[-1]])

    def bias_range(self, prefix):
        """[start, end) of the contiguous run of '*.bias' parameters under `prefix` (the model orders a block's weights first,
        then its biases, so that fused bias-gradient partials can be folded into the gradient buffer with one launch)."""
        idx = [i for i, n in enumerate(self.names) if n.startswith(prefix) and n.endswith(".bias")]
        assert idx and idx == list(range(idx[0], idx[-1] + 1)), f"biases under {prefix} are not contiguous in the flat store"
        return self.offset[self.names[idx[0]]], self._end(self.names[idx[-1]])

    def owns(self, p, name):
        return p.data_ptr() == self.master.data_ptr() + 4 * self.offset[name] and p.device == self.master.device

    def owns_all(self, named_params):
        """True iff EVERY parameter still lives at its offset of this store's master buffer (a stand-alone block engine, .to(),
        or an assignment to p.data re-points parameters one by one; checking only the first one would keep reading stale copies)."""
        return all(n in self.offset and self.owns(p, n) for n, p in named_params)

    def bump(self):
        """The shadow weights changed (a re-cast, a fused optimizer step): new generation, and every buffer derived from the weights is rewritten IN PLACE now -
        so whatever holds its address (a captured HIP graph) keeps reading current values, exactly as it does for the shadow itself."""
        self.generation += 1
        for ref in list(self._on_change):            # weak references: a store must not keep a discarded engine (and its buffers) alive
            fn = ref()
            if fn is None:
                self._on_change.remove(ref)
            else:
                fn()

    def refresh_shadow(self, force=False):
        """Re-cast master -> bf16 shadow if any parameter was modified by torch ops since the last cast (the fused AdamW
        kernel refreshes the shadow itself and does not bump versions)."""
        try:
            vers = tuple(p._version for p in self.params.values())
        except RuntimeError:      # parameters created under torch.inference_mode() carry no version counter: re-cast every call
            vers, force = None, True
        if force or vers != self._versions:
            ops.cast_bf16(self.master, self.shadow)
            self._versions = vers
            self.bump()

    def attach_grads(self):
        """Make every p.grad the view of the flat buffer; returns True if the buffer had to be (re)zeroed."""
        missing = [n for n, p in self.params.items() if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + 4 * self.offset[n]]
        if not missing:
            return False
        if len(missing) == len(self.params):
            self.grad.zero_()
        for n in missing:
            p = self.params[n]
            v = self.view(self.grad, n)
            if len(missing) != len(self.params):
                v.zero_()
                if p.grad is not None:
                    v.copy_(p.grad)
            p.grad = v
        return True


@dataclasses.dataclass
class StepCtx:
    """What every block of one forward / backward reads: geometry, the modulation tensor (L, B, 6, D), the text-length index tensors of the varlen
    cross-attention and the packed caption rows `ye`.  Built by Engine.step_ctx.  kvc: inference only, the per-block cross-attention K / V list of
    Engine._text_cache.  dmod / dye: the backward's accumulators for d(mod) and d(ye)."""
    B: int
    N: int
    hw: tuple
    mod: torch.Tensor
    kv_len: torch.Tensor
    kv_start: torch.Tensor
    max_len: int
    lens_host: typing.Optional[tuple]
    need_grad_aux: bool = True         # False: no backward reads this forward's GELU' (inference, the discarded forward of a checkpointed step)
    ye: typing.Optional[torch.Tensor] = None
    kvc: typing.Optional[list] = None
    dmod: typing.Optional[torch.Tensor] = None
    dye: typing.Optional[torch.Tensor] = None


# Where a block's self-attention reads its keys / values and how their gradients get back into dqkv (Engine._self_kv).  k, v, Nk, sk: what attention is
# handed (sk = the key / value strides).  bwd: 'direct' - dK / dV are dqkv's own k, v column blocks; 'strided' - the same, on every sr-th token;
# 'compress' / 'pick' - k, v are compressed buffers whose gradients go through kv_compress_bwd / kv_pick into dqkv.  zero_dqkv: that path leaves rows
# of dqkv unwritten, so it must start zeroed.
SelfKV = collections.namedtuple("SelfKV", "k v Nk sk bwd zero_dqkv")

# What block_fwd keeps for block_bwd (skv: the block's SelfKV; qkn: the q_norm / k_norm outputs).  save='ckpt' keeps x_in alone and _recompute makes the rest again.
BlockSaved = collections.namedtuple("BlockSaved", "x_in mean1 rstd1 xn1 qkv a lse u1 x1b qc kvc cr lse_c x2 mean2 rstd2 xn2 hpre h u3 skv qkn", defaults=(None,) * 21)

# What Engine.forward keeps for Engine.backward.  blocks: one BlockSaved per block, released as the backward passes it.
Saved = collections.namedtuple("Saved", "ctx blocks cap x x3 meanf rstdf xnf fin_mod mode")


class Engine:
    """Forward/backward sequencing for one PixArtMS instance."""

    def __init__(self, store, cfg):
        self.S, self.cfg = store, cfg
        self._pos_cache = {}
        self._len_cache = {}
        # Inference-only cache of everything that depends on the text alone: the caption MLP output and every block's cross-attention K / V
        # (kv_linear of the packed caption rows).  A sampler calls the model 20+ times with the SAME caption tensor (scripts/inference.py,
        # DPM_Solver.sample): those 1 + depth GEMMs per call (28 of them on M <= 4,800 rows: the 512px inference tail) run once.
        # Key = identity + version of y / the drop mask / y_null and the lengths; any training forward (save != None) clears it - weights may change.
        self._text_cache = None
        self.grad_ready_hook = None   # callable(prefix) fired when a parameter group's gradients are complete
        # Round 5: the softmax scale rides in the qkv projection.  The forward multiplies by a COPY of every block's attn.qkv weight / bias whose q rows
        # carry scale * log2 e (cast from the fp32 master in one rounding; ops.scale_copy, one launch per run of equally spaced blocks after each optimizer
        # step), so q leaves the GEMM as the exponent's argument: the attention kernels take q k^T straight into exp2 (pxa_attn_args.q_prescaled) - one
        # multiply per score less in the dK/dV kernel, and the fp16 forward's folded first product loses its second rounding of q.  The backward is
        # untouched: dq comes out with respect to the unscaled queries and the dX / dW GEMMs read the true weights.  Off under qk_norm (the LayerNorm behind
        # the projection would normalise the factor away) and with PXA_Q_PRESCALE=0 (A/B).
        self.head_dim = cfg["hidden_size"] // cfg["num_heads"]
        self.prescale = (not cfg.get("qk_norm")) and os.environ.get("PXA_Q_PRESCALE", "1") != "0" and self.head_dim == 72
        # The copy lives in ONE pair of buffers per engine, allocated here and rewritten in place whenever the shadow weights change (ParamStore.bump):
        # a HIP graph captured over the forward (DPM_Solver.sample_graphed) bakes these addresses exactly as it bakes the shadow's, and replays after an
        # optimizer step / weight load read current values (the per-generation allocation it replaces left such a graph reading a freed block,
        # and cost the training step a 223 MB allocate / free).
        self._qs = None
        if self.prescale:
            D, depth = cfg["hidden_size"], cfg["depth"]
            self._qs = (torch.empty((depth, 3 * D, D), dtype=BF16, device=store.device), torch.empty((depth, 3 * D), dtype=F32, device=store.device))
            store._on_change.append(weakref.WeakMethod(self._refresh_qs))
        # LoRA adapters (lora.py, attach_lora): None = the plain engine, whose launches are exactly those of tests/golden/engine_schedule_*.txt.  Otherwise the
        # adapters are folded into the shadow weights (and the prescaled qkv copy) behind every re-cast / optimizer step, the forward and the dX GEMMs run
        # unchanged on the merged operands, and the backward computes adapter gradients only: the base model is frozen.
        self.lora = None
        self._lora_refs = ()
        # FP8 inference (enable_fp8): None = the 16-bit engine, whose launches are exactly those of tests/golden/engine_schedule_*.txt.
        self.fp8 = None
        self._f8 = None
        self._f8_ref = None

    # ------------------------------------------------------------------ helpers
    def pos_table(self, h, w):
        key = (h, w)
        if key not in self._pos_cache:
            c = self.cfg
            tab = sincos_pos_embed(c["hidden_size"], h, w, c["pe_interpolation"], c["base_size"])
            self._pos_cache[key] = torch.from_numpy(tab).to(F32).to(self.S.device).contiguous()
        return self._pos_cache[key]

    def step_ctx(self, B, N, hw, mod, lens):
        lk = tuple(int(v) for v in lens)
        if lk not in self._len_cache:                        # per-sample text lengths -> device index tensors, uploaded once per distinct set
            if len(self._len_cache) > 64:
                self._len_cache.clear()
            starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
            self._len_cache[lk] = (torch.tensor(lens, dtype=torch.int32, device=mod.device), torch.from_numpy(starts).to(mod.device))
        kv_len, kv_start = self._len_cache[lk]
        return StepCtx(B, N, hw, mod, kv_len, kv_start, int(max(lens)), lk)

    def _cross_strides(self, N):
        """(batch, token, head) element strides of q, k, v, o of the cross-attention; the first three are its backward's dstrides.  k / v: column halves of
        the packed text rows (found through kv_start)."""
        D, hd = self.cfg["hidden_size"], self.head_dim
        return ((N * D, D, hd), (0, 2 * D, hd), (0, 2 * D, hd), (N * D, D, hd))

    # Item order of the token GEMMs (round 5, pxa_gemm_args.items_descending).  Every row kernel and attention kernel sweeps the token rows upwards, so the rows it
    # wrote LAST are the ones still in the 256 MB Infinity Cache when the next GEMM starts: that GEMM walks its tiles downwards, and its own output then ends with the
    # first rows - fresh for the ascending consumer behind it.  The second GEMM of a GEMM -> GEMM pair (fc2 behind fc1; fc1's dX behind fc2's dX) follows its
    # producer by walking upwards.  Bit-identical results; -1.7 ... -2.1 ms per training step (profiles/r5_16 / r5_17_step_ab_reverse.txt).  PXA_GEMM_ASCENDING=1: off (A/B).
    @staticmethod
    def _desc(name):
        return not name.endswith(("mlp.fc2", "kv_linear", "y_proj.fc1", "y_proj.fc2"))

    def _lin(self, x, name, **kw):
        return ops.gemm(x, self.S.w(name + ".weight"), NT, bias=self.S.f(name + ".bias"), descending=self._desc(name), **kw)

    def _lin_bwd(self, dy, x, name, need_dx=True, dx_kw=None, bias_done=False):
        """dW += dy^T x ; db += colsum(dy) (unless the kernel that produced dy already accumulated it) ; returns dx = dy W (bf16).
        With adapters attached: the base weight and bias are frozen - no TN GEMM, no column sum - and every adapted row slice of the linear gets its
        dA / dBt from one ops.lora_bwd on x and the slice's column block of dy; dx = dy W_merged is the same GEMM on the merged shadow."""
        S = self.S
        if self.lora is not None:
            A = self.lora.store
            for lo, hi, ad in self.lora.slices.get(name, ()):
                ops.lora_bwd(x, dy[:, lo:hi], A.w(ad + ".lora_A"), A.w(ad + ".lora_Bt"), self.lora.scale, A.g(ad + ".lora_A"), A.g(ad + ".lora_Bt"))
        else:
            # (order measured: the weight gradient FIRST - its pass over dy leaves dy in the Infinity Cache for the dX GEMM; dX first is 1.6 ms per step slower,
            # profiles/r5_20_step_ab_dx_first.txt)
            ops.gemm(dy, x, TN, out_f32=S.g(name + ".weight"), accumulate=True, split_k=0)
            if not bias_done:
                ops.colsum(dy, S.g(name + ".bias"))
        if need_dx:                 # dX of fc1 follows fc2's dX GEMM (upwards); the text-row and caption-MLP GEMMs are too small to care
            desc = not name.endswith(("mlp.fc1", "kv_linear", "y_proj.fc1", "y_proj.fc2"))
            return ops.gemm(dy, S.w(name + ".weight"), NN, descending=desc, **(dx_kw or {}))
        return None

    def _refresh_qs(self):
        """Rewrite the prescaled qkv weight / bias copies from the fp32 master (one rounding), in place: one launch per run of equally spaced blocks."""
        S, D, depth = self.S, self.cfg["hidden_size"], self.cfg["depth"]
        w, b = self._qs
        offw = [S.offset[f"blocks.{i}.attn.qkv.weight"] for i in range(depth)]
        offb = [S.offset[f"blocks.{i}.attn.qkv.bias"] for i in range(depth)]
        i = 0
        while i < depth:                                  # runs of equally spaced blocks (KV-compressed blocks carry extra parameters)
            n, st = 1, 0
            if i + 1 < depth:
                st = offw[i + 1] - offw[i]
                while i + n < depth and offw[i + n] - offw[i + n - 1] == st and offb[i + n] - offb[i + n - 1] == st:
                    n += 1
            ops.scale_copy(S.master[offw[i]:], st if n > 1 else 0, n, D * D, 3 * D * D, ops.Q_PRESCALE, out_bf16=w[i:i + n])
            ops.scale_copy(S.master[offb[i]:], st if n > 1 else 0, n, D, 3 * D, ops.Q_PRESCALE, out_f32=b[i:i + n])
            i += n

    # ------------------------------------------------------------------ LoRA adapters
    def attach_lora(self, lora):
        """lora: lora.LoraAdapters with its ParamStore built on this engine's device.  From here on every bump of either store re-merges: the base store's
        re-cast (refresh_shadow) wipes the merge and is followed by it; an adapter update (optimizer step, re-cast of edited adapters) bumps the base store, so
        the generation that keys Engine._text_cache moves and the shadow / prescaled copy are rewritten in place under any captured graph."""
        if self.fp8 is not None:
            raise RuntimeError("FP8 inference is on: adapters cannot be attached to it (disable_fp8() first, or merge_and_unload() the adapters and enable FP8 "
                               "on the merged weights)")
        self.detach_lora(remerge=False)
        self.lora = lora
        self._lora_refs = (weakref.WeakMethod(self._lora_merge), weakref.WeakMethod(self._lora_changed))
        self.S._on_change.append(self._lora_refs[0])          # behind _refresh_qs: the prescaled copy is first rewritten from the master, then its adapted rows merged
        lora.store._on_change.append(self._lora_refs[1])
        self.S.bump()

    def detach_lora(self, remerge=True):
        if self.lora is None:
            return
        for lst, ref in ((self.S._on_change, self._lora_refs[0]), (self.lora.store._on_change, self._lora_refs[1])):
            if ref in lst:
                lst.remove(ref)
        self.lora, self._lora_refs = None, ()
        if remerge:
            self.S.refresh_shadow(force=True)

    def _lora_changed(self):
        self.S.bump()

    def _lora_merge(self, into_master=False):
        """shadow rows <- round16(master + s Bt^T A) for every adapted slice: one launch per slice, reading the fp32 masters of both stores (one rounding)."""
        S, lo_ = self.S, self.lora
        D = self.cfg["hidden_size"]
        for name, slices in lo_.slices.items():
            l = int(name.split(".")[1])
            qs = self._qs[0][l] if self._qs is not None and name.endswith("attn.qkv") else None
            for lo, hi, ad in slices:
                ops.lora_merge(S.f(name + ".weight"), lo, hi, lo_.store.f(ad + ".lora_A"), lo_.store.f(ad + ".lora_Bt"), lo_.scale, S.w(name + ".weight"),
                               dst2=qs, mul_rows=(0, D), mul=ops.Q_PRESCALE, dst_f32=S.f(name + ".weight") if into_master else None)

    def _pg(self, name):
        """Gradient accumulator of a base parameter - or, with adapters attached (the base is frozen), a throw-away buffer for kernels that must write one."""
        return self.S.g(name) if self.lora is None else torch.empty(self.S.shape[name], dtype=F32, device=self.S.device)

    # ------------------------------------------------------------------ caption branch
    def caption_fwd(self, y, row_idx, L, drop, y_null):
        """y (B*L, 4096) fp32 -> packed y_emb (Ltot, D) bf16  (CaptionEmbedder, PixArt_blocks.py:400-407 after masked_select).
        y_null: the y_embedding buffer substituted for dropped samples (token_drop)."""
        S = self.S
        yb = ops.gather_rows_bf16(y, row_idx, L, alt=y_null if drop is not None else None, drop=drop)
        hpre = torch.empty((yb.shape[0], S.shape["y_embedder.y_proj.fc1.weight"][0]), dtype=BF16, device=y.device)
        h = self._lin(yb, "y_embedder.y_proj.fc1", act=ops.ACT_GELU_SAVE_GRAD, out2=hpre)   # hpre holds GELU'(pre-activation)
        ye = self._lin(h, "y_embedder.y_proj.fc2")
        return ye, (yb, hpre, h)

    def caption_bwd(self, dye_f32, saved):
        yb, hpre, h = saved
        dye = torch.empty(dye_f32.shape, dtype=BF16, device=dye_f32.device)
        ops.gate_bwd(dye_f32, du=dye, rows_per_batch=dye_f32.shape[0])
        dh = self._lin_bwd(dye, h, "y_embedder.y_proj.fc2", dx_kw=dict(act=ops.ACT_MUL_AUX, aux=hpre))
        self._lin_bwd(dh, yb, "y_embedder.y_proj.fc1", need_dx=False)

    # ------------------------------------------------------------------ block
    def _self_kv(self, l, qkv, ctx):
        """The one place that knows where block l's self-attention reads its keys / values: qkv's own column blocks, or one of the KV-compression modes
        (PixArt_blocks.py:97-115), whose forward kernels are launched here."""
        S, c = self.S, self.cfg
        B, N, D = ctx.B, ctx.N, c["hidden_size"]
        p = f"blocks.{l}.attn."
        k, v, bs, ts = qkv[:, D:2 * D], qkv[:, 2 * D:], N * 3 * D, 3 * D
        sr = c["kv_scale_factor"] if l in c["kv_layers"] else 1
        if sr == 1:
            return SelfKV(k, v, N, (bs, ts, self.head_dim), "direct", False)
        hh, ww = ctx.hw
        if c["kv_sampling"] == "conv":
            cw, cb, lw, lb = S.f(p + "sr.weight"), S.f(p + "sr.bias"), S.f(p + "norm.weight"), S.f(p + "norm.bias")
            kc = ops.kv_compress_fwd(k, bs, ts, cw, cb, lw, lb, B, hh, ww, D, sr)
            vc = ops.kv_compress_fwd(v, bs, ts, cw, cb, lw, lb, B, hh, ww, D, sr)
            bwd, zero = "compress", not (hh % sr == 0 and ww % sr == 0)      # covered: every token lies in a window, kv_compress_bwd writes all of dqkv's k, v
        elif c["kv_sampling"] == "uniform_every":          # strided keys: gradients land on the picked tokens, the rest stay zero
            return SelfKV(k, v, (N + sr - 1) // sr, (bs, ts * sr, self.head_dim), "strided", True)
        elif c["kv_sampling"] in ("uniform", "ave"):      # 'ave' = nearest interpolation = the same strided pick (PixArt_blocks.py:110-115)
            kc = torch.empty((B, (hh // sr) * (ww // sr), D), dtype=BF16, device=qkv.device)
            vc = torch.empty_like(kc)
            ops.kv_pick(k, kc, bs, ts, B, hh, ww, D, sr)
            ops.kv_pick(v, vc, bs, ts, B, hh, ww, D, sr)
            bwd, zero = "pick", True
        else:
            raise ValueError(f"unknown kv sampling mode {c['kv_sampling']!r}")
        Nk = kc.shape[1]
        return SelfKV(kc, vc, Nk, (Nk * D, D, self.head_dim), bwd, zero)

    # ------------------------------------------------------------------ FP8 inference (MXFP8 token GEMMs, csrc/gemm_f8.hip)
    F8_LINEARS = ("attn.qkv", "attn.proj", "cross_attn.q_linear", "cross_attn.proj", "mlp.fc1", "mlp.fc2")

    def enable_fp8(self, gemm="mx"):
        """Opt-in W8A8 inference: the six token GEMMs of every block take MXFP8 operands (e4m3fn, one E8M0 scale per 32 k).  gemm="mx": ops.gemm_f8 on the
        block-scaled K = 128 MFMA; gemm="dequant": the same quantised operands, dequantised exactly and multiplied by ops.gemm - the reference / A/B mode.
        The MX copies of the weights are allocated once, quantised from the 16-bit operands (attn.qkv from the q-prescaled copy where prescaling is on) and
        rewritten in place behind _refresh_qs at every ParamStore.bump, so a captured sampling graph reads current FP8 weights after a weight load or an
        optimizer step.  The fp32 masters and the 16-bit shadow are untouched.  kv_linear, the caption MLP, the embedders and the final layer stay 16-bit."""
        if gemm not in ("mx", "dequant"):
            raise ValueError(f"enable_fp8: gemm={gemm!r} is not one of 'mx', 'dequant'")
        if self.lora is not None:
            raise RuntimeError("FP8 inference with LoRA adapters attached is not built: call merge_and_unload() first, then enable_fp8()")
        S, depth = self.S, self.cfg["depth"]
        if self._f8 is None:
            self._f8 = {}
            for name in self.F8_LINEARS:
                N, K = S.shape[f"blocks.0.{name}.weight"]
                self._f8[name] = (torch.empty((depth, N, K), dtype=torch.float8_e4m3fn, device=S.device), torch.empty((depth, N, K // 32), dtype=torch.uint8, device=S.device))
        if self._f8_ref is None:
            self._f8_ref = weakref.WeakMethod(self._refresh_f8)
            S._on_change.append(self._f8_ref)              # behind _refresh_qs: attn.qkv is quantised from the copy that one has just rewritten
        self.fp8 = gemm
        self._text_cache = None
        self._refresh_f8()

    def disable_fp8(self):
        """Back to the 16-bit launches.  The MX buffers stay allocated (a later enable_fp8 rewrites them at the same addresses) but are no longer refreshed."""
        if self._f8_ref is not None and self._f8_ref in self.S._on_change:
            self.S._on_change.remove(self._f8_ref)
        self._f8_ref = None
        self.fp8 = None

    def _refresh_f8(self):
        """Re-quantise the MX weight copies from the 16-bit operands, in place."""
        S, depth = self.S, self.cfg["depth"]
        for name in self.F8_LINEARS:
            q, e = self._f8[name]
            if name == "attn.qkv" and self._qs is not None:  # one launch: the prescaled copies of all blocks are one matrix
                ops.mx_quant_rows(self._qs[0].view(-1, q.shape[2]), q=q.view(-1, q.shape[2]), e=e.view(-1, e.shape[2]))
                continue
            for l in range(depth):
                ops.mx_quant_rows(S.w(f"blocks.{l}.{name}.weight"), q=q[l], e=e[l])

    def _lin_f8(self, x, l, name, act=ops.ACT_NONE, mx_out=False):
        """Linear `name` of block l on MXFP8 operands.  x: a 16-bit matrix (quantised here) or an (q, e) pair a previous GEMM left.  mx_out: return the result
        as an (q, e) pair - from the GEMM's own epilogue in 'mx' mode."""
        S = self.S
        wq, we = self._f8[name]
        bias = self._qs[1][l] if name == "attn.qkv" and self._qs is not None else S.f(f"blocks.{l}.{name}.bias")
        xq, xe = x if isinstance(x, tuple) else ops.mx_quant_rows(x)
        if self.fp8 == "mx":
            return ops.gemm_f8(xq, xe, wq[l], we[l], bias=bias, act=act, out16=not mx_out, mx=mx_out)
        y = ops.gemm(ops.mx_dequant_rows(xq, xe), ops.mx_dequant_rows(wq[l], we[l]), NT, bias=bias, act=act, descending=self._desc(name))
        return ops.mx_quant_rows(y) if mx_out else y

    def block_fwd(self, l, x_prev, u_prev, gate_prev, ctx):
        """Returns (x2, u3, gate_mlp, saved).  x_prev/u_prev/gate_prev: residual, pending gated branch of the previous block."""
        S, c = self.S, self.cfg
        B, N, D, H = ctx.B, ctx.N, c["hidden_size"], c["num_heads"]
        p = f"blocks.{l}."
        mod = ctx.mod[l]                                      # (B, 6, D) fp32 view
        sm, scm, gm, sl, scl, gl = (mod[:, i] for i in range(6))
        st = 6 * D
        r = ops.ln_mod_fwd(x_prev, sm, scm, st, u=u_prev, gate=gate_prev, gate_stride=st, rows_per_batch=N, want_stats=True)
        x_in, xn1, mean1, rstd1 = r["x"], r["xn"], r["mean"], r["rstd"]
        pre = dict(q_prescaled=True) if self.prescale else {}
        f8 = self.fp8 is not None   # FP8 inference (enable_fp8; Engine.forward refuses it with a backward to feed): the six token GEMMs go through _lin_f8
        if f8:
            qkv = self._lin_f8(xn1, l, "attn.qkv")
        elif self.prescale:         # block l's views of the engine's persistent copy: weight (3D, D), bias (3D,) with the q rows times scale * log2 e
            qkv = ops.gemm(xn1, self._qs[0][l], NT, bias=self._qs[1][l], descending=True)
        else:
            qkv = self._lin(xn1, p + "attn.qkv")
        qkn = None
        if c.get("qk_norm"):        # q_norm / k_norm on the full-resolution q, k column blocks, in place (PixArt_blocks.py:133-134)
            qkn = (ops.ln_affine_fwd(qkv[:, :D], S.f(p + "attn.q_norm.weight"), S.f(p + "attn.q_norm.bias")),
                   ops.ln_affine_fwd(qkv[:, D:2 * D], S.f(p + "attn.k_norm.weight"), S.f(p + "attn.k_norm.bias")))
        a = torch.empty((B * N, D), dtype=BF16, device=qkv.device)
        lse = torch.empty((B, H, N), dtype=F32, device=qkv.device)
        skv = self._self_kv(l, qkv, ctx)
        ops.attention_fwd(qkv[:, :D], skv.k, skv.v, a, lse, B, H, N, skv.Nk, ((N * 3 * D, 3 * D, self.head_dim), skv.sk, skv.sk, (N * D, D, self.head_dim)), **pre)
        u1 = self._lin_f8(a, l, "attn.proj") if f8 else self._lin(a, p + "attn.proj")
        r = ops.ln_mod_fwd(x_in, u=u1, gate=gm, gate_stride=st, want_xn=False, want_xb=True, rows_per_batch=N)
        x1, x1b = r["x"], r["xb"]
        qc = self._lin_f8(x1b, l, "cross_attn.q_linear") if f8 else self._lin(x1b, p + "cross_attn.q_linear")
        kvc = ctx.kvc[l] if ctx.kvc is not None else None      # inference: constant over the sampler's steps (Engine._text_cache)
        if kvc is None:
            kvc = self._lin(ctx.ye, p + "cross_attn.kv_linear")
            if ctx.kvc is not None:
                ctx.kvc[l] = kvc
        cr = torch.empty((B * N, D), dtype=BF16, device=qkv.device)
        lse_c = torch.empty((B, H, N), dtype=F32, device=qkv.device)
        ops.attention_fwd(qc, kvc[:, :D], kvc[:, D:], cr, lse_c, B, H, N, ctx.max_len, self._cross_strides(N),
                          kv_start=ctx.kv_start, kv_len=ctx.kv_len, max_kv_len=ctx.max_len, kv_len_host=ctx.lens_host)
        u2 = self._lin_f8(cr, l, "cross_attn.proj") if f8 else self._lin(cr, p + "cross_attn.proj")
        r = ops.ln_mod_fwd(x1, sl, scl, st, u=u2, x_out=x1, rows_per_batch=N, want_stats=True)
        x2, xn2, mean2, rstd2 = r["x"], r["xn"], r["mean"], r["rstd"]
        if f8:                                     # h leaves fc1 as MXFP8, an (q, e) pair from the GEMM's own epilogue: no pass between fc1 and fc2
            hpre = None
            h = self._lin_f8(xn2, l, "mlp.fc1", act=ops.ACT_GELU, mx_out=True)
        elif ctx.need_grad_aux:
            hpre = torch.empty((B * N, S.shape[p + "mlp.fc1.weight"][0]), dtype=BF16, device=qkv.device)
            h = self._lin(xn2, p + "mlp.fc1", act=ops.ACT_GELU_SAVE_GRAD, out2=hpre)   # hpre holds GELU'(pre-activation), bf16
        else:                                      # inference / the discarded forward of a checkpointed step: no backward reads GELU' - one output, half the
            hpre = None                            # epilogue's transcendentals and stores
            h = self._lin(xn2, p + "mlp.fc1", act=ops.ACT_GELU)
        u3 = self._lin_f8(h, l, "mlp.fc2") if f8 else self._lin(h, p + "mlp.fc2")
        saved = BlockSaved(x_in=x_in, mean1=mean1, rstd1=rstd1, xn1=xn1, qkv=qkv, a=a, lse=lse, u1=u1, x1b=x1b, qc=qc, kvc=kvc,
                           cr=cr, lse_c=lse_c, x2=x2, mean2=mean2, rstd2=rstd2, xn2=xn2, hpre=hpre, h=h, u3=u3, skv=skv, qkn=qkn)
        return x2, u3, gl, saved

    def block_bwd(self, l, G, sv, ctx):
        """G: fp32 (R, D) gradient w.r.t. this block's output residual x3 = x2 + gate_mlp*u3; overwritten with the
        gradient w.r.t. x_in.  Accumulates parameter gradients, d(mod) and d(y_emb)."""
        S, c = self.S, self.cfg
        B, N, D, H = ctx.B, ctx.N, c["hidden_size"], c["num_heads"]
        R = B * N
        p = f"blocks.{l}."
        mod, dmod = ctx.mod[l], ctx.dmod[l]
        st = 6 * D
        dev = G.device
        # bias gradients ride along with the kernels that produce the output gradients (no separate column-sum passes); they add
        # into PXA_COLSUM_SLOTS partial rows laid out like this block's bias range of the flat gradient buffer
        frozen = self.lora is not None                  # adapters attached: no base bias gradient is collected anywhere
        bs, be = S.bias_range(p)
        part = None if frozen else torch.zeros((ops.COLSUM_SLOTS, be - bs), dtype=F32, device=dev)

        def pb(name, lo=0, hi=None):
            if frozen:
                return None
            o = S.offset[p + name] - bs
            return part[:, o + lo:o + (S.numel[p + name] if hi is None else hi)]
        # ---- MLP branch: x3 = x2 + gate_mlp * u3
        du = torch.empty((R, D), dtype=BF16, device=dev)
        ops.gate_bwd(G, u=sv.u3, gate=mod[:, 5], mod_stride=st, du=du, dgate=dmod[:, 5], dmod_stride=st, rows_per_batch=N,
                     dbias=pb("mlp.fc2.bias"))
        dh = self._lin_bwd(du, sv.h, p + "mlp.fc2", dx_kw=dict(act=ops.ACT_MUL_AUX, aux=sv.hpre, colsum=pb("mlp.fc1.bias")), bias_done=True)
        dxn = self._lin_bwd(dh, sv.xn2, p + "mlp.fc1", bias_done=True)
        del dh
        # ---- cross attention: x2 = x1 + u2 (no gate, no norm): du2 = bf16(G2) comes out of the LN backward pass itself
        # (round 5: cross_attn.proj's bias gradient = column sums of G2 ride in this pass; PXA_FUSED_CPROJ_BIAS=0: the separate colsum pass, A/B)
        fused_cb = os.environ.get("PXA_FUSED_CPROJ_BIAS", "1") != "0"
        ops.ln_mod_bwd(dxn, sv.x2, sv.mean2, sv.rstd2, mod[:, 4], st, G, G, dmod[:, 3], dmod[:, 4], st, N, dx_bf16=du,
                       dbias=pb("cross_attn.proj.bias") if fused_cb else None)
        dc = self._lin_bwd(du, sv.cr, p + "cross_attn.proj", bias_done=fused_cb)
        dqc = torch.empty((R, D), dtype=BF16, device=dev)
        dkvc = torch.empty_like(sv.kvc)
        delta = torch.empty((B, H, N), dtype=F32, device=dev)
        sc_str = self._cross_strides(N)
        ops.attention_bwd(sv.qc, sv.kvc[:, :D], sv.kvc[:, D:], sv.cr, dc, sv.lse_c, delta, dqc, dkvc[:, :D], dkvc[:, D:],
                          B, H, N, ctx.max_len, sc_str, sc_str[:3],
                          kv_start=ctx.kv_start, kv_len=ctx.kv_len, max_kv_len=ctx.max_len, kv_len_host=ctx.lens_host)
        gq = self._lin_bwd(dqc, sv.x1b, p + "cross_attn.q_linear")
        # 4,800 text rows fill 95 of 256 CUs with 256 x 256 tiles: split_k = 0 lets the library's (tile, split) model choose (128 x 128 here: 72us -> 47us)
        self._lin_bwd(dkvc, ctx.ye, p + "cross_attn.kv_linear", need_dx=not frozen, dx_kw=dict(out_f32=ctx.dye, accumulate=True, split_k=0))   # frozen caption MLP: nobody reads d(ye)
        # ---- self attention: x1 = x_in + gate_msa * u1 ; G1 = G + gq
        ops.gate_bwd(G, add=gq, u=sv.u1, gate=mod[:, 2], mod_stride=st, dx_out=G, du=du, dgate=dmod[:, 2], dmod_stride=st, rows_per_batch=N,
                     dbias=pb("attn.proj.bias"))
        da = self._lin_bwd(du, sv.a, p + "attn.proj", bias_done=True)
        qkv, skv = sv.qkv, sv.skv
        s3 = (N * 3 * D, 3 * D, self.head_dim)
        pre = dict(q_prescaled=True) if self.prescale else {}
        dqkv = torch.zeros_like(qkv) if skv.zero_dqkv else torch.empty_like(qkv)
        if skv.bwd in ("direct", "strided"):
            dk, dv = dqkv[:, D:2 * D], dqkv[:, 2 * D:]
        else:                                               # compressed K/V buffers: attention backward, then the compression's backward
            dk, dv = torch.empty_like(skv.k), torch.empty_like(skv.v)
        ops.attention_bwd(qkv[:, :D], skv.k, skv.v, sv.a, da, sv.lse, delta, dqkv[:, :D], dk, dv,
                          B, H, N, skv.Nk, (s3, skv.sk, skv.sk, (N * D, D, self.head_dim)), (s3, skv.sk, skv.sk), **pre)
        if skv.bwd == "compress":
            (hh, ww), sr = ctx.hw, c["kv_scale_factor"]
            cw, cb, lw = S.f(p + "attn.sr.weight"), S.f(p + "attn.sr.bias"), S.f(p + "attn.norm.weight")
            gcw, gcb = self._pg(p + "attn.sr.weight"), self._pg(p + "attn.sr.bias")
            glw, glb = self._pg(p + "attn.norm.weight"), self._pg(p + "attn.norm.bias")
            for dyc, lo in ((dk, D), (dv, 2 * D)):     # the same sr / norm parameters process K and V (PixArt_blocks.py:138-139)
                ops.kv_compress_bwd(dyc, qkv[:, lo:lo + D], N * 3 * D, 3 * D, cw, cb, lw, dqkv[:, lo:lo + D], N * 3 * D, 3 * D,
                                    gcw, gcb, glw, glb, B, hh, ww, D, sr)
        elif skv.bwd == "pick":
            (hh, ww), sr = ctx.hw, c["kv_scale_factor"]
            ops.kv_pick(dk, dqkv[:, D:2 * D], N * 3 * D, 3 * D, B, hh, ww, D, sr, backward=True)
            ops.kv_pick(dv, dqkv[:, 2 * D:], N * 3 * D, 3 * D, B, hh, ww, D, sr, backward=True)
        if sv.qkn is not None:                               # back through q_norm / k_norm: dqkv's q, k blocks become d(raw q), d(raw k)
            (qs, qm, qr), (ks_, km, kr) = sv.qkn
            ops.ln_affine_bwd(dqkv[:, :D], qs, qm, qr, S.f(p + "attn.q_norm.weight"), self._pg(p + "attn.q_norm.weight"), self._pg(p + "attn.q_norm.bias"))
            ops.ln_affine_bwd(dqkv[:, D:2 * D], ks_, km, kr, S.f(p + "attn.k_norm.weight"), self._pg(p + "attn.k_norm.weight"), self._pg(p + "attn.k_norm.bias"))
        # the attention kernels can also emit the q/k/v bias-gradient sums (pxa_attn_args.d*_colsum), but the cross-lane row
        # reductions cost them more (~0.5 ms/block) than one streaming column-sum pass over dqkv (~0.2 ms/block): measured, not used
        dxn = self._lin_bwd(dqkv, sv.xn1, p + "attn.qkv")
        ops.ln_mod_bwd(dxn, sv.x_in, sv.mean1, sv.rstd1, mod[:, 1], st, G, G, dmod[:, 0], dmod[:, 1], st, N)
        if not frozen:
            ops.colsum_reduce(part, S.grad[bs:be])
        if self.grad_ready_hook:
            self.grad_ready_hook(f"blocks.{l}")
        return G

    def block_standalone_fwd(self, x, y, mod, lens, hw):
        """One block outside the model (PixArtMSBlock.forward): x (B*N, D) fp32, y the packed text rows (.., D), mod (1, B, 6, D) fp32.
        Returns (x2 + gate_mlp * u3 as (B*N, D) fp32, what block_standalone_bwd needs)."""
        B, D = mod.shape[1], mod.shape[3]
        N = x.shape[0] // B
        ctx = self.step_ctx(B, N, hw, mod, lens)
        ctx.lens_host = None                       # as before the one step_ctx: no host copy of the lengths goes to the attention wrappers from here
        ctx.ye = y.reshape(-1, D).to(BF16).contiguous()
        x2, u3, gl, sv = self.block_fwd(0, x, None, None, ctx)
        r = ops.ln_mod_fwd(x2, u=u3, gate=gl, gate_stride=6 * D, want_xn=False, rows_per_batch=N)    # the pending gated MLP branch: inside the model the next block's first pass
        return r["x"], (ctx, sv)

    def block_standalone_bwd(self, G, saved):
        """G (B*N, D) fp32, overwritten -> (d x, d mod (B, 6, D), d y (Ltot, D) fp32); parameter gradients go to the flat buffer."""
        ctx, sv = saved
        ctx.dmod = torch.zeros_like(ctx.mod)
        ctx.dye = torch.zeros(ctx.ye.shape, dtype=F32, device=G.device)
        return self.block_bwd(0, G, sv, ctx), ctx.dmod[0], ctx.dye

    # ------------------------------------------------------------------ whole core
    def forward(self, x, y, mod, fin_mod, row_idx, lens, drop, save, y_null=None):
        """x (B,4,Hl,Wl) fp32, y (B*L,4096) fp32, mod (L,B,6,D) fp32, fin_mod (B,2,D) fp32 -> (out (B,2C,Hl,Wl), saved)."""
        S, c = self.S, self.cfg
        B, _, Hl, Wl = x.shape
        h, w = Hl // 2, Wl // 2
        N, D, depth = h * w, c["hidden_size"], c["depth"]
        if self.fp8 is not None and (save or torch.is_grad_enabled()):
            raise RuntimeError("FP8 inference is on (enable_fp8): a forward that keeps activations for a backward is not built - run it under torch.no_grad(), "
                               "or disable_fp8() before training")
        ctx = self.step_ctx(B, N, (h, w), mod, lens)
        ctx.need_grad_aux = save == "all"
        L = y.shape[0] // B
        tkey = None
        if save or torch.is_grad_enabled():
            self._text_cache = None
        elif _capturing() or os.environ.get("PXA_TEXT_CACHE", "1") == "0":
            pass                                  # a captured graph must own every buffer it reads: no cache inside sample_graphed's capture
        else:
            tkey = (S.generation, y.data_ptr(), y._version, tuple(y.shape), ctx.lens_host, None if drop is None else (drop.data_ptr(), drop._version),
                    None if y_null is None else (y_null.data_ptr(), y_null._version), row_idx.data_ptr())
        if tkey is not None and self._text_cache is not None and self._text_cache["key"] == tkey:
            ctx.ye, cap_saved = self._text_cache["ye"], None
            ctx.kvc = self._text_cache["kvc"]
        else:
            ctx.ye, cap_saved = self.caption_fwd(y, row_idx, L, drop, y_null)
            if tkey is not None:
                ctx.kvc = [None] * depth
                self._text_cache = dict(key=tkey, ye=ctx.ye, kvc=ctx.kvc, y=y)      # holds y so that its address cannot be reused by another tensor
        xt = ops.patch_embed_fwd(x, S.f("x_embedder.proj.weight"), S.f("x_embedder.proj.bias"), self.pos_table(h, w))
        x_prev, u_prev, gate_prev = xt, None, None
        blocks = []
        for l in range(depth):
            x_prev, u_prev, gate_prev, sv = self.block_fwd(l, x_prev, u_prev, gate_prev, ctx)
            blocks.append(sv if save == "all" else (BlockSaved(x_in=sv.x_in) if save == "ckpt" else None))
        r = ops.ln_mod_fwd(x_prev, fin_mod[:, 0], fin_mod[:, 1], 2 * D, u=u_prev, gate=gate_prev, gate_stride=6 * D, rows_per_batch=N, want_stats=True)
        lin = ops.gemm(r["xn"], S.w("final_layer.linear.weight"), NT, bias=S.f("final_layer.linear.bias"), out_dtype=F32)
        out = ops.unpatchify_fwd(lin, B, h, w, c["out_channels"])
        saved = None
        if save:
            saved = Saved(ctx=ctx, blocks=blocks, cap=cap_saved, x=x, x3=r["x"], meanf=r["mean"], rstdf=r["rstd"], xnf=r["xn"], fin_mod=fin_mod, mode=save)
        return out, saved

    def backward(self, dout, saved):
        """dout (B,2C,Hl,Wl) fp32 -> (dmod (L,B,6,D), dfin (B,2,D)); parameter gradients go to the flat buffer."""
        S, c = self.S, self.cfg
        ctx = saved.ctx
        B, N, D, depth = ctx.B, ctx.N, c["hidden_size"], c["depth"]
        h, w = ctx.hw
        dev = dout.device
        ctx.dmod = torch.zeros_like(ctx.mod)
        dfin = torch.zeros_like(saved.fin_mod)
        frozen = self.lora is not None                  # adapters attached: the embedders and the final layer are frozen, the blocks' adapters alone get gradients
        ctx.dye = None if frozen else torch.zeros(ctx.ye.shape, dtype=F32, device=dev)
        dlin = ops.patchify_bwd(dout.contiguous(), h, w)
        dxn = self._lin_bwd(dlin, saved.xnf, "final_layer.linear")
        G = torch.empty((B * N, D), dtype=F32, device=dev)
        ops.ln_mod_bwd(dxn, saved.x3, saved.meanf, saved.rstdf, saved.fin_mod[:, 1], 2 * D, None, G, dfin[:, 0], dfin[:, 1], 2 * D, N)
        if self.grad_ready_hook:
            self.grad_ready_hook("final")
        ctx.need_grad_aux = True                         # the recomputed forwards of a checkpointed step feed block_bwd
        for l in reversed(range(depth)):
            sv = saved.blocks[l]
            if saved.mode == "ckpt":   # recompute this block's activations from its saved input (auto_grad_checkpoint semantics)
                sv = self._recompute(l, sv, ctx)
            G = self.block_bwd(l, G, sv, ctx)
            saved.blocks[l] = None
        if not frozen:
            ops.patch_embed_bwd(saved.x, G, S.g("x_embedder.proj.weight"), S.g("x_embedder.proj.bias"))
            self.caption_bwd(ctx.dye, saved.cap)
        return ctx.dmod, dfin

    def _recompute(self, l, sv, ctx):
        """Re-run block l forward from its saved input x_in (x_in already includes the previous block's gated MLP branch)."""
        return self.block_fwd(l, sv.x_in, None, None, ctx)[3]
