"""The FP8 (e4m3fn) weight format of pixart_sigma_amd.t5.T5Encoder in plain torch: the quantiser rule the HIP kernel pxa_fp8_quant_rows is pinned against, and
state dicts whose weight matrices went through it.  No GPU, nothing of pixart_sigma_amd.

    amax  = max_k |W[n][k]|
    scale = 2^ceil(log2(amax / 448)), 1 for an all-zero row         (the logarithm in fp64: amax is an fp32 value, so amax / 448 is 2^-23 relative away from a
                                                                     power of two or on it, and fp64 resolves that)
    q     = (w.float() / scale[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)"""
import torch

FP8 = torch.float8_e4m3fn
MATRIX_SUFFIXES = tuple(f"SelfAttention.{n}.weight" for n in "qkvo") + tuple(f"DenseReluDense.{n}.weight" for n in ("wi_0", "wi_1", "wo"))


def is_matrix(key):
    return key.startswith("encoder.block.") and key.endswith(MATRIX_SUFFIXES)


def scales(w):
    amax = w.float().abs().amax(dim=1).double()
    s = torch.exp2(torch.ceil(torch.log2(amax / 448.0)))
    return torch.where(amax == 0, torch.ones_like(s), s).float()


def quant_rows(w):
    """(q float8_e4m3fn (N, K), scale fp32 (N,)) of a 2-D tensor, by the rule above."""
    s = scales(w)
    return (w.float() / s[:, None]).clamp(-448, 448).to(FP8), s


def dequant(q, s):
    return q.float() * s.reshape(-1, 1).float()


def dequant_state_dict(sd, through=None):
    """The state dict with every weight matrix replaced by scale * q (fp32, exact).  through: a 16-bit dtype the matrices are cast to first, as the encoder of
    that operand type holds them."""
    out = {}
    for k, v in sd.items():
        if is_matrix(k):
            w = v if through is None else v.to(through)
            out[k] = dequant(*quant_rows(w))
        else:
            out[k] = v
    return out


def fp8_state_dict(sd, scale_shape="vector"):
    """The state dict as an FP8 file holds it: X.weight float8_e4m3fn and X.weight_scale fp32 ((N,), or (N, 1) with scale_shape="column")."""
    out = {}
    for k, v in sd.items():
        if is_matrix(k):
            q, s = quant_rows(v)
            out[k], out[k + "_scale"] = q, (s[:, None].contiguous() if scale_shape == "column" else s)
        else:
            out[k] = v
    return out
