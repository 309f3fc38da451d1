"""The MXFP8 format of the denoiser's FP8 inference path in plain torch: the quantiser rule the HIP kernel pxa_mx_quant_rows is pinned against, its inverse, and
the fp64 product of two MX matrices.  No GPU, nothing of pixart_sigma_amd.

A matrix X (R, K), K % 32 == 0, is q (R, K) float8_e4m3fn and e (R, K / 32) uint8 (E8M0: the block scale is 2^(e - 127)).  Per block of 32 consecutive k:

    amax = max |x|
    X    = ceil(log2(amax / 448)), 0 for an all-zero block, clamped to [-127, 127]   (the logarithm in fp64: amax is an fp32 value, so amax / 448 is 2^-23
                                                                                      relative away from a power of two or on it, and fp64 resolves that)
    e    = X + 127                                                                   (0 .. 254: the E8M0 NaN code 0xFF is never written)
    q    = e4m3fn(x / 2^X), round to nearest even                                    (|x| / 2^X <= 448: nothing is clipped, 0x7F / 0xFF are never written)"""
import torch

FP8 = torch.float8_e4m3fn
BLOCK = 32


def exponents(x):
    """X (R, K / 32) int64 of a 2-D tensor."""
    R, K = x.shape
    assert K % BLOCK == 0
    amax = x.float().abs().reshape(R, K // BLOCK, BLOCK).amax(dim=2).double()
    X = torch.ceil(torch.log2(amax / 448.0))
    X = torch.where(amax == 0, torch.zeros_like(X), X).clamp(-127, 127)
    return X.long()


def quant_rows(x):
    """(q float8_e4m3fn (R, K), e uint8 (R, K / 32)) of a 2-D tensor, by the rule above.  No clamp is applied to the quotient: `never clips` is a property."""
    X = exponents(x)
    s = torch.exp2(X.double()).repeat_interleave(BLOCK, dim=1)
    y = (x.double() / s).float()                       # exact: a power-of-two quotient of an fp32 value (fp64 carries what fp32 would flush)
    return y.to(FP8), (X + 127).to(torch.uint8)


def dequant(q, e, dtype=torch.float64):
    s = torch.exp2(e.double() - 127.0).repeat_interleave(BLOCK, dim=1)
    return (q.double() * s).to(dtype)


def matmul64(qa, ea, qw, ew):
    """sum_k A[m][k] W[n][k] in fp64 of the dequantised operands (M, N)."""
    return dequant(qa, ea) @ dequant(qw, ew).t()


def gelu_tanh64(x):
    return torch.nn.functional.gelu(x.double(), approximate="tanh")
