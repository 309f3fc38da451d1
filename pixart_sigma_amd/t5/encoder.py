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

There is no CPU or eager fallback: without the library or a GPU, forward raises."""
import json
import math
import os
import warnings
from dataclasses import dataclass, fields

import torch

from .. import lib

MAX_LENGTH = 512          # pxa_t5_attn: 1 <= L <= 512
MAX_HEADS = 64


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

    def __init__(self, config):
        super().__init__()
        global _WARNED_F16
        self.config = T5Config.from_dict(config).check()
        if lib.OPERAND == "f16" and not _WARNED_F16:
            _WARNED_F16 = True
            warnings.warn("T5Encoder under the fp16-operand build: the reference runs T5 in bf16 and trained T5-XXL activations overflow fp16; "
                          "set PXA_OPERAND_DTYPE=bf16 for real checkpoints", stacklevel=2)
        c, op = self.config, lib.OPERAND_DTYPE
        inner = c.num_heads * c.d_kv

        def buf(name, shape, dtype):
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

    def load_state_dict(self, state_dict, strict=True, assign=False):
        names = self._hf_names()
        embed = [k for k in self.EMBED_KEYS if k in state_dict]
        missing = [k for k in names if k not in state_dict] + ([] if embed else ["shared.weight | encoder.embed_tokens.weight"])
        if missing:
            raise KeyError(f"T5Encoder.load_state_dict: {len(missing)} missing key(s), first: {missing[:4]}")
        unexpected = [k for k in state_dict if k not in names and k not in self.EMBED_KEYS and not k.startswith(("decoder.", "lm_head."))]
        if unexpected and strict:
            raise KeyError(f"T5Encoder.load_state_dict: unexpected key(s): {unexpected[:4]}")

        def put(dst, rows, src, key):
            view = dst if rows is None else dst[rows]
            if tuple(src.shape) != tuple(view.shape):
                raise ValueError(f"T5Encoder.load_state_dict: {key} has shape {tuple(src.shape)}, expected {tuple(view.shape)}")
            view.copy_(src)                      # casts to the buffer's type: 16-bit weights are held once, in the operand type
        with torch.no_grad():
            put(self.embed, None, state_dict[embed[0]], embed[0])
            for k, (name, rows) in names.items():
                put(getattr(self, name), rows, state_dict[k], k)
        self._bias_cache.clear()
        return torch.nn.modules.module._IncompatibleKeys([], unexpected)

    @classmethod
    def from_pretrained(cls, path, device=None):
        """config.json + the weights of a transformers T5 directory: one model.safetensors, sharded safetensors with model.safetensors.index.json, or
        pytorch_model.bin / pytorch_model-*.bin shards with pytorch_model.bin.index.json.  Does not import transformers."""
        with open(os.path.join(path, "config.json")) as f:
            model = cls(json.load(f))
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
        model.load_state_dict(sd)
        return model.to(device) if device is not None else model

    # ------------------------------------------------------------------------------------------------ forward
    def position_bias(self, L):
        """fp32 (H, 2L - 1): entry [h][(j - i) + L - 1] is the bias of key j for query i."""
        c = self.config
        key = (L, self.rel_bias.device)
        if key not in self._bias_cache:
            buckets = relative_position_bucket(torch.arange(-(L - 1), L), c.relative_attention_num_buckets, c.relative_attention_max_distance)
            self._bias_cache[key] = self.rel_bias[buckets.to(self.rel_bias.device)].t().contiguous()
        return self._bias_cache[key]

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
        for i in range(c.num_layers):
            w = lambda n: getattr(self, f"b{i}_{n}")                                    # noqa: E731
            xn, _ = ops.t5_rmsnorm(x, w("ln0"), c.layer_norm_epsilon)
            qkv = ops.gemm(xn, w("wqkv"), ops.NT)
            a = ops.t5_attention(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], bias, kv_len, B, H, L)
            ops.gemm(a, w("wo"), ops.NT, out_f32=x, accumulate=True)
            ops.t5_rmsnorm(x, w("ln1"), c.layer_norm_epsilon, out=xn)
            h0 = ops.gemm(xn, w("wi0"), ops.NT, act=ops.ACT_GELU)
            g = ops.gemm(xn, w("wi1"), ops.NT, act=ops.ACT_MUL_AUX, aux=h0)
            ops.gemm(g, w("wff"), ops.NT, out_f32=x, accumulate=True)
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
