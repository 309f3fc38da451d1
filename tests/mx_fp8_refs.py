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


# ------------------------------------------------------------------------------------------------ the code table: every finite byte, and the rounding ties
def finite_codes():
    """The 254 finite e4m3fn bytes, 0x00 .. 0x7E and 0x80 .. 0xFE (uint8), -0 included."""
    b = torch.arange(256, dtype=torch.uint8)
    return b[(b & 0x7F) != 0x7F]


def code_values(b):
    """fp64 value of every byte of a uint8 tensor of finite codes, from the bit fields (not through torch's float8 conversion): subnormal m 2^-9, normal
    (1 + m / 8) 2^(E - 7), sign bit 0x80."""
    b = b.long()
    E, m = (b >> 3) & 0xF, (b & 7).double()
    mag = torch.where(E == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * torch.exp2(E.double() - 7.0))
    return torch.where((b & 0x80) != 0, -mag, mag)


def tie_midpoints():
    """(x fp32 (252,), want uint8 (252,)): the midpoint of every pair of adjacent non-negative codes c, c + 1 (c = 0x00 .. 0x7D), in both signs, and the
    code round-to-nearest-even gives it: the one of c, c + 1 whose last mantissa bit - the byte's last bit - is 0, with the sign.  Every midpoint has at
    most five significant bits: exact in fp32, bf16 and fp16."""
    c = torch.arange(0x7E, dtype=torch.uint8)
    mid = (code_values(c) + code_values(c + 1)) / 2
    even = torch.where((c & 1) == 0, c, c + 1)
    x = torch.cat([mid, -mid]).float()
    assert (x.double() == torch.cat([mid, -mid])).all()
    return x, torch.cat([even, even | 0x80])


def exponent_edge_rows():
    """(x fp32 (cases, 64), X int64 (cases,)): one row per block maximum at which the exponent rule can go wrong, with X worked out by hand, not by the
    logarithm.  Block 0 holds +amax in its first 16-element half, block 1 holds -amax in its second; the other elements are amax times a factor of magnitude at most 3/4
    (rounded to fp32 where amax is a subnormal)."""
    u32, u16, ub = 2.0 ** -23, 2.0 ** -10, 2.0 ** -7            # one ulp of fp32 / fp16 / bf16 relative to a power of two; 448 = 1.75 * 2^8
    cases = []
    for k in (-20, 0, 10):
        s = 2.0 ** k
        cases += [(448.0 * s, k)]
        cases += [(256.0 * (1.75 + u) * s, k + 1) for u in (u32, u16, ub)]
        cases += [(256.0 * (1.75 - u) * s, k) for u in (u32, u16, ub)]
    cases += [(2.0 ** -126, -127), (1e-45, -127), (2.0 ** -130, -127), (2.0 ** -133, -127), (3 * 2.0 ** -133, -127),      # fp32 / bf16 subnormals: the lower clamp
              (2.0 ** -24, -32), (3 * 2.0 ** -24, -31), (1023 * 2.0 ** -24, -22),                                          # fp16 subnormals
              (3e38, 120)]
    amax = torch.tensor([c[0] for c in cases], dtype=torch.float64).float()
    fill = torch.tensor([0.5, -0.25, 0.0, -0.5, 0.25, 0.125, -0.75, 0.0]).repeat(4)
    x = (amax[:, None] * fill[None, :]).repeat(1, 2)
    x[:, 5], x[:, 32 + 20] = amax, -amax
    return x, torch.tensor([c[1] for c in cases])


TIE_SHIFTS = (0, -9, 6)


def tie_rows():
    """(x fp32 (3, 288), q uint8 (3, 288), e uint8 (3, 9)): the 252 signed midpoints, 28 to a block, each block also holding 448 (alternating sign, at a
    position that moves through both 16-element halves) so that X = 0 and the midpoint reaches the conversion unscaled; row i is row 0 times
    2^TIE_SHIFTS[i] (exact in fp32, bf16 and fp16: at least 2^-19 and at most 448 * 64), so X = TIE_SHIFTS[i] and the codes are the same.  q is the expected
    byte: the even neighbour."""
    mid, want = tie_midpoints()
    x = torch.zeros(9, 32)
    q = torch.zeros(9, 32, dtype=torch.uint8)
    for b in range(9):
        pos = (7 * b + 3) % 32
        slots = [i for i in range(32) if i != pos][:28]
        x[b, slots], q[b, slots] = mid[28 * b:28 * b + 28], want[28 * b:28 * b + 28]
        x[b, pos], q[b, pos] = (448.0, 0x7E) if b % 2 == 0 else (-448.0, 0xFE)
    x = torch.stack([x.reshape(288) * 2.0 ** s for s in TIE_SHIFTS])
    e = torch.tensor([[127 + s] * 9 for s in TIE_SHIFTS], dtype=torch.uint8)
    return x, q.reshape(1, 288).repeat(3, 1), e
