"""The T5 v1.1 encoder (forward only, frozen) on the HIP path: what the reference reaches as `T5EncoderModel.from_pretrained(..., torch_dtype=bfloat16)` and
`model(input_ids, attention_mask)['last_hidden_state']` (reference diffusion/model/t5.py:87,106-111).

Per block, on an fp32 residual stream x of (B*L, d_model) rows:
    xn  = rmsnorm(x) * ln0                      pxa_t5_rmsnorm  -> operand type
    qkv = xn Wqkv^T                             pxa_gemm NT, one packed (3 * H * 64, d_model) weight
    a   = softmax(q k^T + bias[h][j - i]) v     pxa_t5_attn (no scale, per-sample key lengths, every query row)
    x  += a Wo^T                                pxa_gemm NT, out_f32 = x, accumulate: the projection is never rounded
    xn  = rmsnorm(x) * ln1
    h0  = gelu_new(xn Wi0^T)                    pxa_gemm NT, act GELU (tanh)
    g   = (xn Wi1^T) * h0                       pxa_gemm NT, act MUL_AUX
    x  += g Wo_ff^T                             pxa_gemm NT, out_f32 = x, accumulate
and last_hidden_state = rmsnorm(x) * final_ln in fp32.  16-bit weights are held once, in the operand type of the process (no fp32 master: XXL has 4.7 B
parameters); norm weights and the 32-row relative-attention bias embedding stay fp32.  The bucket table is host math (the port of transformers'
_relative_position_bucket) and the (2L - 1, H) gather from the embedding is conditioning-sized torch work.

FP8 weight storage (opt-in: weight_dtype="fp8_e4m3"; csrc/gemm_w8.hip).  The seven weight matrices of a block (wqkv packed as above) are
held as OCP e4m3fn bytes b{i}_<name> plus one fp32 scale per output row b{i}_<name>_scale, W ~ scale[n] * q[n][k]: half the weight bytes.  The embedding, the norm
weights and the bias table stay as they are.  16-bit / fp32 tensors given to load_state_dict are cast to the operand type (as the 16-bit encoder holds them) and
quantised on the device by pxa_fp8_quant_rows, matrix by matrix: scale = 2^ceil(log2(amax / 448)), a power of two, so scale * q is exact in the operand type
and both GEMM paths multiply the same weights.  FP8 tensors (transformers' key X.weight as float8_e4m3fn, X.weight_scale fp32 of shape (N,), (N, 1) or scalar;
no scale = a plain cast, scale 1) are taken bit for bit; a NaN code (0x7F / 0xFF) is refused.  Scales that are not powers of two are accepted: the dequant
path then rounds scale * q once to the operand type, the stream path multiplies the fp32 sum by the scale, so the two paths differ by that rounding.
set_fp8_gemm chooses the path of the five GEMM calls per block: "stream" = pxa_gemm_w8 (FP8 bytes widened in registers, for the rows of one prompt or a few),
"dequant" = pxa_fp8_dequant_rows into ONE operand-type scratch matrix per encoder (the largest matrix: 100 MB at XXL), then the pxa_gemm call of the 16-bit
encoder, in stream order; "auto" = stream when B * L <= STREAM_MAX_M.  Without weight_dtype every call is what it was.

There is no CPU or eager fallback: without the library or a GPU, forward raises (and so does quantising 16-bit weights)."""
import json
import math
import os
import warnings
from dataclasses import dataclass, fields

import torch

from .. import lib

MAX_LENGTH = 512          # pxa_t5_attn: 1 <= L <= 512
MAX_HEADS = 64
FP8_E4M3 = "fp8_e4m3"
FP8 = torch.float8_e4m3fn
MATRICES = ("wqkv", "wo", "wi0", "wi1", "wff")
FP8_GEMM_PATHS = ("auto", "stream", "dequant")
# auto: the streaming kernel up to this many rows (B * L), dequantise + pxa_gemm above.  From tools/bench_t5.py --sweep_w8 on an MI355X,
# us for the five calls of an XXL block, stream / dequant + pxa_gemm:  M = 16: 192 / 426,  64: 190 / 433,  120: 203 / 438,  300: 262 / 445,  600: 451 / 488,
# 1200: 731 / 743 (738 / 734 in a second run: a tie),  2048: 1152 / 1028.  600 is the largest row count of the sweep at which stream wins beyond the spread.
STREAM_MAX_M = 600


def check_weight_dtype(weight_dtype):
    if weight_dtype not in (None, FP8_E4M3):
        raise ValueError(f"T5Encoder: weight_dtype={weight_dtype!r} is not supported: None (16-bit, as stored) or {FP8_E4M3!r}")
    return weight_dtype


@dataclass
class T5Config:
    vocab_size: int = 32128
    d_model: int = 4096
    d_kv: int = 64
    d_ff: int = 10240
    num_layers: int = 24
    num_heads: int = 64
    relative_attention_num_buckets: int = 32
    relative_attention_max_distance: int = 128
    layer_norm_epsilon: float = 1e-6
    feed_forward_proj: str = "gated-gelu"

    @classmethod
    def from_dict(cls, d):
        """From a transformers config.json dict (or a T5Config); keys this encoder does not use are ignored."""
        if isinstance(d, cls):
            return d
        names = {f.name for f in fields(cls)}
        return cls(**{k: v for k, v in dict(d).items() if k in names})

    def check(self):
        if self.feed_forward_proj not in ("gated-gelu", "gated-gelu_new"):
            raise ValueError(f"T5Encoder: feed_forward_proj={self.feed_forward_proj!r} is not supported: only the gated gelu_new feed-forward of T5 v1.1 "
                             "('gated-gelu') is built")
        if self.d_kv != 64:
            raise ValueError(f"T5Encoder: d_kv={self.d_kv} is not supported: the attention kernel is built for head width 64")
        if not 1 <= self.num_heads <= MAX_HEADS:
            raise ValueError(f"T5Encoder: num_heads={self.num_heads} is outside the attention kernel's range 1 .. {MAX_HEADS}")
        if self.d_model % 8 or self.d_ff % 8:
            raise ValueError(f"T5Encoder: d_model={self.d_model} and d_ff={self.d_ff} must be multiples of 8")
        return self


def relative_position_bucket(relative_position, num_buckets=32, max_distance=128):
    """transformers' T5Attention._relative_position_bucket for the bidirectional (encoder) case, operation for operation: integer tensor of offsets
    (key position - query position) -> bucket numbers in [0, num_buckets).  Host math; the logarithm is fp32, as there."""
    relative_position = torch.as_tensor(relative_position, dtype=torch.long, device="cpu")
    num_buckets //= 2
    buckets = (relative_position > 0).to(torch.long) * num_buckets
    relative_position = torch.abs(relative_position)
    max_exact = num_buckets // 2
    is_small = relative_position < max_exact
    if_large = max_exact + (torch.log(relative_position.float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)).to(torch.long)
    if_large = torch.min(if_large, torch.full_like(if_large, num_buckets - 1))
    return buckets + torch.where(is_small, relative_position, if_large)


def key_lengths(attention_mask):
    """(B, L) 0/1 mask -> int64 (B,) count of valid keys.  The kernel masks by length, so every row must be a run of ones followed by zeros (right padding, what
    the tokenizer call of the reference produces), with at least one valid token."""
    m = torch.as_tensor(attention_mask).cpu()
    if m.dim() != 2:
        raise ValueError(f"T5Encoder: attention_mask must be (B, L), got {tuple(m.shape)}")
    m = m != 0
    lens = m.sum(1)
    if (lens == 0).any():
        raise ValueError(f"T5Encoder: attention_mask row {int((lens == 0).nonzero()[0])} has no valid token (softmax over an empty key set)")
    if not torch.equal(m, torch.arange(m.shape[1])[None, :] < lens[:, None]):
        raise ValueError("T5Encoder: attention_mask must be right-padded (ones, then zeros, in every row): the attention kernel masks keys by length")
    return lens


_WARNED_F16 = False


class T5Encoder(torch.nn.Module):
    """T5EncoderModel's forward on the HIP kernels.  Weights come through load_state_dict (transformers' key names) or from_pretrained."""

    def __init__(self, config, weight_dtype=None):
        super().__init__()
        global _WARNED_F16
        self.config = T5Config.from_dict(config).check()
        self.weight_dtype = check_weight_dtype(weight_dtype)
        if weight_dtype and (self.config.d_model % 16 or self.config.d_ff % 16):
            raise ValueError(f"T5Encoder: weight_dtype={FP8_E4M3!r} needs d_model={self.config.d_model} and d_ff={self.config.d_ff} to be multiples of 16 "
                             "(the FP8 kernels move 16 weights at a time)")
        self.fp8_gemm = "auto"
        self.set_fp8_gemm(os.environ.get("PXA_T5_FP8_GEMM", "auto"))
        self._scratch = None
        if lib.OPERAND == "f16" and not _WARNED_F16:
            _WARNED_F16 = True
            warnings.warn("T5Encoder under the fp16-operand build: the reference runs T5 in bf16 and trained T5-XXL activations overflow fp16; "
                          "set PXA_OPERAND_DTYPE=bf16 for real checkpoints", stacklevel=2)
        c, op = self.config, lib.OPERAND_DTYPE
        inner = c.num_heads * c.d_kv

        def buf(name, shape, dtype):
            if weight_dtype and dtype == op and name != "embed":
                self.register_buffer(name, torch.zeros(shape, dtype=FP8), persistent=False)
                name, shape, dtype = name + "_scale", shape[:1], torch.float32
                self.register_buffer(name, torch.ones(shape, dtype=dtype), persistent=False)
                return
            self.register_buffer(name, torch.zeros(shape, dtype=dtype), persistent=False)
        buf("embed", (c.vocab_size, c.d_model), op)
        buf("rel_bias", (c.relative_attention_num_buckets, c.num_heads), torch.float32)
        buf("final_ln", (c.d_model,), torch.float32)
        for i in range(c.num_layers):
            buf(f"b{i}_ln0", (c.d_model,), torch.float32)
            buf(f"b{i}_wqkv", (3 * inner, c.d_model), op)
            buf(f"b{i}_wo", (c.d_model, inner), op)
            buf(f"b{i}_ln1", (c.d_model,), torch.float32)
            buf(f"b{i}_wi0", (c.d_ff, c.d_model), op)
            buf(f"b{i}_wi1", (c.d_ff, c.d_model), op)
            buf(f"b{i}_wff", (c.d_model, c.d_ff), op)
        self._bias_cache = {}
        self.requires_grad_(False)

    # ------------------------------------------------------------------------------------------------ weights
    def _hf_names(self):
        """transformers key -> (buffer name, row slice or None) for everything but the token embedding."""
        c = self.config
        inner = c.num_heads * c.d_kv
        names = {"encoder.final_layer_norm.weight": ("final_ln", None),
                 "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight": ("rel_bias", None)}
        for i in range(c.num_layers):
            p = f"encoder.block.{i}.layer."
            for j, n in enumerate("qkv"):
                names[f"{p}0.SelfAttention.{n}.weight"] = (f"b{i}_wqkv", slice(j * inner, (j + 1) * inner))
            names[f"{p}0.SelfAttention.o.weight"] = (f"b{i}_wo", None)
            names[f"{p}0.layer_norm.weight"] = (f"b{i}_ln0", None)
            names[f"{p}1.layer_norm.weight"] = (f"b{i}_ln1", None)
            names[f"{p}1.DenseReluDense.wi_0.weight"] = (f"b{i}_wi0", None)
            names[f"{p}1.DenseReluDense.wi_1.weight"] = (f"b{i}_wi1", None)
            names[f"{p}1.DenseReluDense.wo.weight"] = (f"b{i}_wff", None)
        return names

    EMBED_KEYS = ("shared.weight", "encoder.embed_tokens.weight")

    @classmethod
    def wanted_key(cls, k):
        """Keys of a checkpoint this encoder reads (a loader can drop the rest - the decoder and lm_head of a full model - shard by shard)."""
        return k in cls.EMBED_KEYS or k.startswith("encoder.")

    def set_fp8_gemm(self, path):
        """The GEMM path of an FP8 encoder: "auto", "stream" or "dequant" (module docstring).  A 16-bit encoder ignores it."""
        if path not in FP8_GEMM_PATHS:
            raise ValueError(f"T5Encoder.set_fp8_gemm: {path!r} is not one of {FP8_GEMM_PATHS}")
        self.fp8_gemm = path
        return self

    def _quant_device(self):
        """Where 16-bit weights are quantised: the module's device if it is a GPU, else the current one.  There is no host quantiser."""
        if self.embed.is_cuda:
            return self.embed.device
        if not torch.cuda.is_available():
            raise lib.PixartHipError("T5Encoder: quantising 16-bit weights to FP8 runs pxa_fp8_quant_rows and needs the MI355X (there is no CPU fallback); "
                                     "FP8 files load without one")
        return torch.device("cuda", torch.cuda.current_device())

    def _put_fp8(self, name, rows, src, scale, key):
        """One matrix (or the rows of wqkv it fills) into the FP8 buffers: FP8 bits as they are, anything else through the quantiser."""
        from .. import ops
        q_dst, s_dst = getattr(self, name), getattr(self, name + "_scale")
        if rows is not None:
            q_dst, s_dst = q_dst[rows], s_dst[rows]
        if tuple(src.shape) != tuple(q_dst.shape):
            raise ValueError(f"T5Encoder.load_state_dict: {key} has shape {tuple(src.shape)}, expected {tuple(q_dst.shape)}")
        N = q_dst.shape[0]
        if src.dtype == FP8:
            bits = src.contiguous().view(torch.uint8)
            if bool(((bits & 0x7F) == 0x7F).any()):
                raise ValueError(f"T5Encoder.load_state_dict: {key} holds an FP8 NaN code (0x7F / 0xFF): the file is refused")
            if scale is None:
                scale = torch.ones(N)
            scale = torch.as_tensor(scale, dtype=torch.float32)
            if scale.numel() not in (1, N) or scale.dim() > 2 or (scale.dim() == 2 and scale.shape[1] != 1):
                raise ValueError(f"T5Encoder.load_state_dict: {key}_scale has shape {tuple(scale.shape)}, expected ({N},), ({N}, 1) or a scalar")
            if not bool(torch.isfinite(scale).all()):
                raise ValueError(f"T5Encoder.load_state_dict: {key}_scale is not finite")
            q_dst.view(torch.uint8).copy_(bits)
            s_dst.copy_(scale.reshape(-1).expand(N))
            return
        if not src.dtype.is_floating_point:
            raise ValueError(f"T5Encoder.load_state_dict: {key} has dtype {src.dtype}")
        dev = self._quant_device()
        q, sc = ops.fp8_quant_rows(src.to(device=dev, dtype=lib.OPERAND_DTYPE).contiguous())       # the values a 16-bit encoder would hold
        q_dst.view(torch.uint8).copy_(q.view(torch.uint8))
        s_dst.copy_(sc)

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """transformers' key names.  A 16-bit encoder casts every tensor to the buffer's type.  An FP8 encoder takes float8_e4m3fn matrices (with X.weight_scale:
        (N,), (N, 1), a scalar, or none = 1) bit for bit and refuses a NaN code; 16-bit / fp32 matrices are cast to the operand type and quantised on the GPU
        with pxa_fp8_quant_rows, one matrix at a time.  An FP8 embedding is widened to the operand type."""
        names = self._hf_names()
        embed = [k for k in self.EMBED_KEYS if k in state_dict]
        missing = [k for k in names if k not in state_dict] + ([] if embed else ["shared.weight | encoder.embed_tokens.weight"])
        if missing:
            raise KeyError(f"T5Encoder.load_state_dict: {len(missing)} missing key(s), first: {missing[:4]}")
        scales = {k + "_scale" for k in names if k.endswith(".weight")} if self.weight_dtype else set()
        unexpected = [k for k in state_dict if k not in names and k not in scales and k not in self.EMBED_KEYS and not k.startswith(("decoder.", "lm_head."))]
        if unexpected and strict:
            raise KeyError(f"T5Encoder.load_state_dict: unexpected key(s): {unexpected[:4]}")

        def put(dst, rows, src, key):
            view = dst if rows is None else dst[rows]
            if tuple(src.shape) != tuple(view.shape):
                raise ValueError(f"T5Encoder.load_state_dict: {key} has shape {tuple(src.shape)}, expected {tuple(view.shape)}")
            if src.dtype == FP8 and key not in self.EMBED_KEYS:
                raise ValueError(f"T5Encoder.load_state_dict: {key} is float8_e4m3fn and this encoder holds 16-bit weights: build it with "
                                 f"weight_dtype={FP8_E4M3!r} (T5Encoder.from_pretrained does that for an FP8 file)")
            view.copy_(src)                      # casts to the buffer's type: 16-bit weights are held once, in the operand type
        with torch.no_grad():
            put(self.embed, None, state_dict[embed[0]], embed[0])
            for k, (name, rows) in names.items():
                if self.weight_dtype and name.split("_", 1)[1] in MATRICES:
                    self._put_fp8(name, rows, state_dict[k], state_dict.get(k + "_scale"), k)
                else:
                    put(getattr(self, name), rows, state_dict[k], k)
        self._bias_cache.clear()
        return torch.nn.modules.module._IncompatibleKeys([], unexpected)

    @classmethod
    def from_pretrained(cls, path, device=None, weight_dtype=None):
        """config.json + the weights of a transformers T5 directory: one model.safetensors, sharded safetensors with model.safetensors.index.json, or
        pytorch_model.bin / pytorch_model-*.bin shards with pytorch_model.bin.index.json.  Does not import transformers.
        weight_dtype None: as stored - a directory whose matrices are float8_e4m3fn (save_pretrained of an FP8 encoder, tools/quantize_t5.py, or a plain-cast
        file without scales) gives an FP8 encoder, a 16-bit one today's encoder.  "fp8_e4m3": a 16-bit checkpoint is quantised while loading, one matrix on the
        device at a time (the 16-bit model is never on the device as a whole); give `device`."""
        check_weight_dtype(weight_dtype)
        with open(os.path.join(path, "config.json")) as f:
            config = json.load(f)
        sd = {}
        for fname in _weight_files(path):
            full = os.path.join(path, fname)
            if fname.endswith(".safetensors"):
                from safetensors import safe_open
                with safe_open(full, framework="pt", device="cpu") as f:
                    for k in f.keys():
                        if cls.wanted_key(k):
                            sd[k] = f.get_tensor(k)
            else:
                part = torch.load(full, map_location="cpu", weights_only=True)
                sd.update({k: v for k, v in part.items() if cls.wanted_key(k)})
                del part
        if weight_dtype is None and any(v.dtype == FP8 for k, v in sd.items() if k not in cls.EMBED_KEYS):
            weight_dtype = FP8_E4M3
        model = cls(config, weight_dtype=weight_dtype)
        if weight_dtype and device is not None:
            model = model.to(device)             # empty FP8 buffers first: load_state_dict then quantises straight into them
        model.load_state_dict(sd)
        return model.to(device) if device is not None else model

    def quantize_fp8(self):
        """A loaded 16-bit encoder on the GPU becomes an FP8 one, in place: each matrix through pxa_fp8_quant_rows, the 16-bit copy dropped as it goes.
        The same bits as from_pretrained(..., weight_dtype="fp8_e4m3") of the checkpoint it was loaded from."""
        from .. import ops
        if self.weight_dtype:
            return self
        c = self.config
        if c.d_model % 16 or c.d_ff % 16:
            raise ValueError(f"T5Encoder.quantize_fp8: d_model={c.d_model} and d_ff={c.d_ff} must be multiples of 16")
        if not self.embed.is_cuda:
            raise lib.PixartHipError("T5Encoder.quantize_fp8 runs pxa_fp8_quant_rows and needs the module on the MI355X (there is no CPU fallback)")
        for i in range(c.num_layers):
            for n in MATRICES:
                name = f"b{i}_{n}"
                q, sc = ops.fp8_quant_rows(getattr(self, name))
                delattr(self, name)
                self.register_buffer(name, q, persistent=False)
                self.register_buffer(name + "_scale", sc, persistent=False)
        self.weight_dtype = FP8_E4M3
        return self

    def save_pretrained(self, path):
        """config.json + model.safetensors under transformers' key names, readable by from_pretrained bit for bit.  An FP8 encoder writes X.weight as
        float8_e4m3fn and X.weight_scale as fp32 (N,) for the matrices (q / k / v unpacked); the embedding (shared.weight) in the operand type, norm weights
        and the bias table fp32."""
        from safetensors.torch import save_file
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(dict({fl.name: getattr(self.config, fl.name) for fl in fields(self.config)}, model_type="t5", architectures=["T5EncoderModel"]), f, indent=1)
        out = {"shared.weight": self.embed.detach().cpu().contiguous()}
        for k, (name, rows) in self._hf_names().items():
            t = getattr(self, name)
            out[k] = (t if rows is None else t[rows]).detach().cpu().contiguous()
            if self.weight_dtype and name.split("_", 1)[1] in MATRICES:
                sc = getattr(self, name + "_scale")
                out[k + "_scale"] = (sc if rows is None else sc[rows]).detach().cpu().contiguous()
        save_file(out, os.path.join(path, "model.safetensors"))
        return path

    def weight_bytes(self):
        """Bytes of every buffer this encoder holds (the scratch matrix of the dequant path included once it exists)."""
        n = sum(b.numel() * b.element_size() for b in self.buffers())
        return n + (self._scratch.numel() * self._scratch.element_size() if self._scratch is not None else 0)

    # ------------------------------------------------------------------------------------------------ forward
    def position_bias(self, L):
        """fp32 (H, 2L - 1): entry [h][(j - i) + L - 1] is the bias of key j for query i."""
        c = self.config
        key = (L, self.rel_bias.device)
        if key not in self._bias_cache:
            buckets = relative_position_bucket(torch.arange(-(L - 1), L), c.relative_attention_num_buckets, c.relative_attention_max_distance)
            self._bias_cache[key] = self.rel_bias[buckets.to(self.rel_bias.device)].t().contiguous()
        return self._bias_cache[key]

    def fp8_gemm_path(self, rows):
        """The path a forward of `rows` = B * L rows takes: "stream" or "dequant"."""
        return self.fp8_gemm if self.fp8_gemm != "auto" else ("stream" if rows <= STREAM_MAX_M else "dequant")

    def _fp8_mm(self, rows):
        """The GEMM call of an FP8 forward: (a, q, scale, **kw) -> what ops.gemm(a, W, NT, **kw) returns on the 16-bit encoder."""
        from .. import ops
        if self.fp8_gemm_path(rows) == "stream":
            return ops.gemm_w8
        c = self.config
        need = max(3 * c.num_heads * c.d_kv, c.d_ff) * c.d_model
        if self._scratch is None or self._scratch.device != self.embed.device or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=lib.OPERAND_DTYPE, device=self.embed.device)      # one matrix, once per encoder: the stream orders its reuse

        def mm(a, q, scale, out_f32=None, **kw):
            w = ops.fp8_dequant_rows(q, scale, out=self._scratch[:q.numel()].view(q.shape))
            if out_f32 is not None:
                return ops.gemm(a, w, ops.NT, out_f32=out_f32, accumulate=True)
            return ops.gemm(a, w, ops.NT, **kw)
        return mm

    @torch.no_grad()
    def forward(self, input_ids, attention_mask=None, output_hidden_states=False):
        """input_ids (B, L) integer, attention_mask (B, L) 0/1 right-padded (None: all valid) -> last_hidden_state fp32 (B, L, d_model), every row computed.
        output_hidden_states: also the list [embedding, block 1 output, ..., block N-1 output, last_hidden_state] (transformers' hidden_states)."""
        from .. import ops
        c = self.config
        if not (torch.cuda.is_available() and self.embed.is_cuda):
            raise lib.PixartHipError("T5Encoder.forward needs the MI355X and the module on it (there is no CPU / eager fallback)")
        ids = torch.as_tensor(input_ids)
        if ids.dim() != 2 or ids.dtype.is_floating_point:
            raise ValueError(f"T5Encoder: input_ids must be an integer (B, L) tensor, got {ids.dtype} {tuple(ids.shape)}")
        B, L = ids.shape
        if not 1 <= L <= MAX_LENGTH:
            raise ValueError(f"T5Encoder: sequence length {L} is outside the attention kernel's range 1 .. {MAX_LENGTH}")
        lo, hi = int(ids.min()), int(ids.max())
        if lo < 0 or hi >= c.vocab_size:
            raise ValueError(f"T5Encoder: input_ids span [{lo}, {hi}], outside the vocabulary [0, {c.vocab_size})")
        if attention_mask is None:
            attention_mask = torch.ones(B, L, dtype=torch.long)
        if tuple(attention_mask.shape) != (B, L):
            raise ValueError(f"T5Encoder: attention_mask {tuple(attention_mask.shape)} does not match input_ids {(B, L)}")
        dev = self.embed.device
        kv_len = key_lengths(attention_mask).to(device=dev, dtype=torch.int32)
        bias = self.position_bias(L)
        H, inner = c.num_heads, c.num_heads * c.d_kv
        x = ops.t5_embed(ids.to(device=dev, dtype=torch.int32).reshape(-1).contiguous(), self.embed)
        hidden = [x.clone()] if output_hidden_states else None
        mm = self._fp8_mm(B * L) if self.weight_dtype else None
        for i in range(c.num_layers):
            w = lambda n: getattr(self, f"b{i}_{n}")                                    # noqa: E731
            xn, _ = ops.t5_rmsnorm(x, w("ln0"), c.layer_norm_epsilon)
            if mm is None:
                qkv = ops.gemm(xn, w("wqkv"), ops.NT)
                a = ops.t5_attention(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], bias, kv_len, B, H, L)
                ops.gemm(a, w("wo"), ops.NT, out_f32=x, accumulate=True)
                ops.t5_rmsnorm(x, w("ln1"), c.layer_norm_epsilon, out=xn)
                h0 = ops.gemm(xn, w("wi0"), ops.NT, act=ops.ACT_GELU)
                g = ops.gemm(xn, w("wi1"), ops.NT, act=ops.ACT_MUL_AUX, aux=h0)
                ops.gemm(g, w("wff"), ops.NT, out_f32=x, accumulate=True)
            else:                                                                       # the same five calls on the FP8 matrices
                qkv = mm(xn, w("wqkv"), w("wqkv_scale"))
                a = ops.t5_attention(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], bias, kv_len, B, H, L)
                mm(a, w("wo"), w("wo_scale"), out_f32=x)
                ops.t5_rmsnorm(x, w("ln1"), c.layer_norm_epsilon, out=xn)
                h0 = mm(xn, w("wi0"), w("wi0_scale"), act=ops.ACT_GELU)
                g = mm(xn, w("wi1"), w("wi1_scale"), act=ops.ACT_MUL_AUX, aux=h0)
                mm(g, w("wff"), w("wff_scale"), out_f32=x)
            if output_hidden_states and i + 1 < c.num_layers:
                hidden.append(x.clone())
        _, y = ops.t5_rmsnorm(x, self.final_ln, c.layer_norm_epsilon, want_bf16=False, want_f32=True)
        y = y.view(B, L, c.d_model)
        if output_hidden_states:
            return y, [h.view(B, L, c.d_model) for h in hidden] + [y]
        return y


def _weight_files(path):
    """The weight files of a transformers model directory, in the order of the list in the issue: safetensors before .bin, an index before a single file."""
    for index, single in (("model.safetensors.index.json", "model.safetensors"), ("pytorch_model.bin.index.json", "pytorch_model.bin")):
        if os.path.exists(os.path.join(path, index)):
            with open(os.path.join(path, index)) as f:
                return sorted(set(json.load(f)["weight_map"].values()))
        if os.path.exists(os.path.join(path, single)):
            return [single]
    raise FileNotFoundError(f"T5Encoder.from_pretrained: no model.safetensors / pytorch_model.bin (or their index json) in {path}")
