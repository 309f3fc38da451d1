"""The T5 v1.1 encoder once more, in plain torch and fp64, and a seeded recipe of weights and inputs for it: the reference of tests/test_t5_host.py (against
the stored transformers outputs) and of tests/test_t5_model_gpu.py::test_parity_at_production_dispatch; tools/make_t5_golden.py loads the same recipe into
transformers.T5EncoderModel for tests/golden/t5_wide.json.  No GPU needed, no `transformers`, nothing of pixart_sigma_amd.

encoder64 states the architecture in its own words: token embedding; per block RMS norm (no mean, no bias) -> q, k, v -> softmax(q k^T + bias[bucket(j - i)]
+ key mask) v WITHOUT a 1 / sqrt(d) scale -> o added to the residual -> RMS norm -> gelu_tanh(x W0^T) * (x W1^T) -> wo added to the residual; a final RMS
norm.  All rows are computed, the padded ones too (they attend to the valid keys of their sample, as in transformers).  With round_to = a 16-bit type it rounds
where pixart_sigma_amd.t5.T5Encoder rounds: the weights and the embedding to the operand type, every GEMM operand (the norm outputs, the attention output, g),
the 16-bit GEMM outputs (q, k, v, h0, g), the probabilities P; the residual stream is held in fp32.  That is an emulation of the module's rounding POINTS, not
of its kernels' summation orders."""
import hashlib
import math

import torch

DEFAULTS = dict(d_kv=64, relative_attention_num_buckets=32, relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu")
# the seeded fixture of tests/golden/t5_wide.json: B L = 1200 rows at widths >= 1024, so the encoder's five GEMM calls take the plans of a production batch
WIDE = dict(cfg=dict(d_model=1024, num_heads=16, d_ff=1280, num_layers=2, vocab_size=64), B=4, L=300, lens=[300, 137, 1, 77], seed=22)
WIDE_TAIL = slice(1024, 1200)          # the rows of the ragged last 256-row tile


def full_config(cfg):
    return dict(DEFAULTS, **cfg)


def state_dict(cfg, seed):
    """transformers' key names -> bf16 tensors, every value bf16-representable.  T5's init scales (factor 1): embedding 1, q (d_model d_kv)^-1/2, k / v / wi_0 /
    wi_1 d_model^-1/2, o (H d_kv)^-1/2, wo d_ff^-1/2; then, as tools/make_t5_golden.py describes, q x 8 (unscaled logits that spread as in a trained T5), norm
    weights 1 + 0.2 N(0, 1), the bias table 2 N(0, 1).  One generator, drawn in the order of the keys below."""
    c = full_config(cfg)
    D, H, dk, dff, V = c["d_model"], c["num_heads"], c["d_kv"], c["d_ff"], c["vocab_size"]
    g = torch.Generator().manual_seed(seed)

    def n(*shape, scale=1.0, shift=0.0):
        return (shift + scale * torch.randn(*shape, generator=g)).to(torch.bfloat16)
    sd = {"shared.weight": n(V, D)}
    sd["encoder.embed_tokens.weight"] = sd["shared.weight"]
    for i in range(c["num_layers"]):
        p = f"encoder.block.{i}.layer."
        sd[p + "0.SelfAttention.q.weight"] = n(H * dk, D, scale=8 * (D * dk) ** -0.5)
        sd[p + "0.SelfAttention.k.weight"] = n(H * dk, D, scale=D ** -0.5)
        sd[p + "0.SelfAttention.v.weight"] = n(H * dk, D, scale=D ** -0.5)
        sd[p + "0.SelfAttention.o.weight"] = n(D, H * dk, scale=(H * dk) ** -0.5)
        if i == 0:
            sd[p + "0.SelfAttention.relative_attention_bias.weight"] = n(c["relative_attention_num_buckets"], H, scale=2.0)
        sd[p + "0.layer_norm.weight"] = n(D, scale=0.2, shift=1.0)
        sd[p + "1.DenseReluDense.wi_0.weight"] = n(dff, D, scale=D ** -0.5)
        sd[p + "1.DenseReluDense.wi_1.weight"] = n(dff, D, scale=D ** -0.5)
        sd[p + "1.DenseReluDense.wo.weight"] = n(D, dff, scale=dff ** -0.5)
        sd[p + "1.layer_norm.weight"] = n(D, scale=0.2, shift=1.0)
    sd["encoder.final_layer_norm.weight"] = n(D, scale=0.2, shift=1.0)
    return sd


def inputs(cfg, B, L, lens, seed):
    """(input_ids, attention_mask): ids in [2, vocab), right-padded with id 0 behind each sample's length"""
    g = torch.Generator().manual_seed(seed + 2000)
    ids = torch.randint(2, full_config(cfg)["vocab_size"], (B, L), generator=g)
    mask = (torch.arange(L)[None, :] < torch.tensor(lens)[:, None]).long()
    return ids * mask, mask


def checksum(sd, ids):
    """sha256 over the ids (int64) and the bits of every weight, keys in sorted order"""
    h = hashlib.sha256(ids.to(torch.int64).contiguous().numpy().tobytes())
    for k in sorted(sd):
        assert sd[k].dtype == torch.bfloat16
        h.update(k.encode())
        h.update(sd[k].contiguous().view(torch.int16).numpy().tobytes())
    return h.hexdigest()


def buckets(offsets, num_buckets=32, max_distance=128):
    """bucket of the offset (key position - query position), bidirectional: half of the buckets per sign; per sign the first half one offset each, the second
    half logarithmic up to max_distance, everything farther in the last.  The logarithm is taken in fp32 (tests/golden/t5_buckets.pt pins this against
    transformers at every offset up to 1023)."""
    off = torch.as_tensor(offsets, dtype=torch.long)
    half, exact = num_buckets // 2, num_buckets // 4
    n = off.abs()
    far = exact + (torch.log(n.float() / exact) / math.log(max_distance / exact) * (half - exact)).long()
    return (off > 0).long() * half + torch.where(n < exact, n, far.clamp(max=half - 1))


def rms_norm(x, w, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def encoder64(cfg, sd, ids, mask, round_to=None, device="cpu"):
    """-> [embedding, output of block 1, ..., of block N - 1, last_hidden_state] as fp64 (B, L, d_model) tensors (transformers' hidden_states)."""
    c = full_config(cfg)
    assert c["feed_forward_proj"] in ("gated-gelu", "gated-gelu_new")
    H, dk, eps = c["num_heads"], c["d_kv"], c["layer_norm_epsilon"]
    B, L = ids.shape

    def rt(t):                                             # a 16-bit tensor of the module
        return t if round_to is None else t.to(round_to).double()

    def w(key, sixteen=True):
        t = sd[key].to(device)
        return rt(t.double()) if sixteen else t.double()
    ids, mask = ids.to(device), mask.to(device)
    x = w("shared.weight")[ids]                                                        # (B, L, D)
    pos = torch.arange(L)
    table = w("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", sixteen=False)
    bias = table[buckets(pos[None, :] - pos[:, None], c["relative_attention_num_buckets"], c["relative_attention_max_distance"]).to(device)]     # (L query, L key, H)
    bias = bias.permute(2, 0, 1)[None] + torch.where(mask.bool(), 0.0, float("-inf")).double()[:, None, None, :]           # (B, H, L, L)
    hidden = [x.clone()]

    def heads(t):
        return t.view(B, L, H, dk).transpose(1, 2)
    for i in range(c["num_layers"]):
        p = f"encoder.block.{i}.layer."
        xn = rt(rms_norm(x, w(p + "0.layer_norm.weight", sixteen=False), eps))
        q, k, v = (heads(rt(xn @ w(p + f"0.SelfAttention.{n}.weight").t())) for n in "qkv")
        P = rt(torch.softmax(q @ k.transpose(-1, -2) + bias, -1))
        a = rt((P @ v).transpose(1, 2).reshape(B, L, H * dk))
        x = x + a @ w(p + "0.SelfAttention.o.weight").t()
        if round_to is not None:
            x = x.float().double()
        xn = rt(rms_norm(x, w(p + "1.layer_norm.weight", sixteen=False), eps))
        h0 = rt(torch.nn.functional.gelu(xn @ w(p + "1.DenseReluDense.wi_0.weight").t(), approximate="tanh"))
        g = rt((xn @ w(p + "1.DenseReluDense.wi_1.weight").t()) * h0)
        x = x + g @ w(p + "1.DenseReluDense.wo.weight").t()
        if round_to is not None:
            x = x.float().double()
        if i + 1 < c["num_layers"]:
            hidden.append(x.clone())
    hidden.append(rms_norm(x, w("encoder.final_layer_norm.weight", sixteen=False), eps))
    return hidden


def rel_l2_rows(a, b):
    """rel-L2 of every row of a (rows, D) pair, fp64"""
    a, b = a.double(), b.double()
    return (a - b).norm(dim=-1) / b.norm(dim=-1).clamp_min(1e-300)
