"""The two LoRA kernels (csrc/lora.hip) in the forms the engine calls them, against fp64 on the host.  Runs under either operand build (PXA_OPERAND_DTYPE;
tests/test_lora_f16_gpu.py re-runs the file under f16).

pxa_lora_merge: the reference is the fp64 evaluation of W + s B A rounded ONCE to the operand type.  The kernel evaluates in fp32 and rounds once, so an
element may differ only where the fp32 error moves the value across a rounding boundary - then by one representable value - and only rarely: the share of
differing elements is capped at 1e-3 (the host's own fp32 evaluation measures <= 2.7e-4 on the first two shapes, bf16 and fp16).

pxa_lora_bwd: the reference is fp64 from the same 16-bit inputs.  The one rounding the design permits is that of t = x A^T and u = dy B to the operand type in
front of the second product; its size is MEASURED per case by a host emulation (fp32 products, t and u rounded once, fp32 accumulation) and the kernel is
held to 2 x that figure.  Emulation figures, rel-L2 over the 32 cases, measured on the host: bf16 build dA 1.3e-3 ... 2.0e-3, dBt 4.9e-4 ... 2.2e-3; fp16 build
dA 3.5e-5 ... 3.8e-4, dBt 1.8e-4 ... 4.0e-4 (the small ends are the M = 1 cases, where one rounding of one number is the whole error)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import record_parity, rel_l2  # noqa: E402
from pixart_sigma_amd import lib as _lib  # noqa: E402

OPD = _lib.OPERAND_DTYPE
NAN16, NAN32 = torch.tensor(float("nan"), dtype=OPD).view(torch.int16).item(), 0x7FC00000
GUARD = 4096                       # elements of poison in front of and behind every tensor
MERGE_MISMATCH_CAP = 1e-3
BWD_FACTOR = 2.0                   # kernel error <= 2 x the host emulation's (see the header)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _banded(rows, cols, dtype, ld=None, col0=0, fill=None):
    """(view (rows, cols) with row pitch ld starting at column col0 of a wider matrix, the whole allocation): the allocation is NaN everywhere - guard bands,
    the other columns of the wider matrix - except the view, which holds `fill` (or stays NaN for the caller to fill)."""
    ld = ld or cols
    flat = torch.full((2 * GUARD + rows * ld,), float("nan"), dtype=dtype, device="cuda")
    view = flat[GUARD:GUARD + rows * ld].view(rows, ld)[:, col0:col0 + cols]
    if fill is not None:
        view.copy_(fill)
    return view, flat


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _untouched_outside(flat, before, view_mask_fn):
    """Every element of the allocation outside the view has the bits it had."""
    same = _bits(flat) == _bits(before)
    mask = torch.ones_like(same)
    view_mask_fn(mask)
    return bool(same[mask].all())


def _ulp_steps(a, b):
    """Per element: how many representable values apart two 16-bit tensors are (same sign assumed where they differ)."""
    ia, ib = _bits(a.contiguous()).int(), _bits(b.contiguous()).int()
    return (ia - ib).abs()


# ---------------------------------------------------------------------------------------------- merge
MERGE_CASES = {"320x192_r16": (320, 0, 320, 192, 16, 0.10), "1152x1152_r64": (1152, 0, 1152, 1152, 64, 0.25), "3456x1152_rows1152-3456_r4": (3456, 1152, 3456, 1152, 4, 0.06)}


@pytest.mark.parametrize("case", list(MERGE_CASES))
def test_merge_rounds_once_and_touches_only_its_rows(case):
    from pixart_sigma_amd import ops
    rows, lo, hi, K, r, frac = MERGE_CASES[case]
    g = torch.Generator().manual_seed(7)
    W = torch.randn(rows, K, generator=g) * 0.03
    A = torch.randn(r, K, generator=g)
    Bt = torch.randn(r, hi - lo, generator=g)
    delta = Bt.double().t() @ A.double()
    s = float(np.float32(frac * W[lo:hi].double().norm() / delta.norm()))              # ||s B A|| = frac ||W|| on the slice: 6 ... 25 %
    mul = float(np.float32(ops.Q_PRESCALE))
    mlo, mhi = lo, lo + (hi - lo) // 2                                                 # the multiplier covers the first half of the slice
    v64 = W.double().clone()
    v64[lo:hi] += s * delta
    want = v64.to(OPD)
    v2 = v64.clone()
    v2[mlo:mhi] *= mul
    want2 = v2.to(OPD)
    Wd, Ad, Btd = W.cuda(), A.cuda(), Bt.cuda()
    prev = (torch.randn(rows, K, generator=g) * 0.03).to(OPD)                          # what the destination held: must survive outside [lo, hi)
    dst, flat = _banded(rows, K, OPD, fill=prev)
    dst2, flat2 = _banded(rows, K, OPD, fill=prev)
    before, before2 = flat.clone(), flat2.clone()
    ops.lora_merge(Wd, lo, hi, Ad, Btd, s, dst, dst2=dst2, mul_rows=(mlo, mhi), mul=mul)
    torch.cuda.synchronize()
    first, first2 = dst.clone(), dst2.clone()
    for name, got, ref, fl, bef in (("dst", dst, want, flat, before), ("dst2 (prescaled)", dst2, want2, flat2, before2)):
        steps = _ulp_steps(got[lo:hi].cpu(), ref[lo:hi])
        share = (steps != 0).float().mean().item()
        print(f"\n[{case}] {name}: differing elements {share:.2e} (cap {MERGE_MISMATCH_CAP:.0e}), furthest {int(steps.max())} representable value(s)")
        record_parity(f"lora_merge {case} {name}: share of elements off the fp64 rounding", share, MERGE_MISMATCH_CAP)
        assert torch.isfinite(got[lo:hi].float()).all()
        assert int(steps.max()) <= 1, f"{name}: an element is {int(steps.max())} representable values from the once-rounded fp64 value: a second rounding"
        assert share <= MERGE_MISMATCH_CAP
        # rows outside [lo, hi) and the guard bands (NaN in front of and behind the destination) are untouched
        def inside(mask, lo=lo, hi=hi):
            mask[GUARD + lo * K:GUARD + hi * K] = False
        assert _untouched_outside(fl, bef, inside), f"{name}: written outside rows [{lo}, {hi})"
    # the delta is really there (a missing scale or slice would pass nothing above, but make the norm explicit)
    moved = rel_l2(dst[lo:hi].float().cpu(), W[lo:hi])
    assert 0.8 * frac < moved < 1.25 * frac + 5e-3, moved
    # two calls give the same bits
    ops.lora_merge(Wd, lo, hi, Ad, Btd, s, dst, dst2=dst2, mul_rows=(mlo, mhi), mul=mul)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dst), _bits(first)) and torch.equal(_bits(dst2), _bits(first2))


def test_merge_scale_zero_is_the_plain_cast_and_fp32_destination():
    """s = 0 gives the base model's bits (set_lora_scale(0)): the cast of the master, and for the prescaled copy what scale_copy makes of it.  dst_f32: the
    merged fp32 value itself (merge_and_unload), rounding to the 16-bit destination."""
    from pixart_sigma_amd import ops
    g = torch.Generator().manual_seed(3)
    rows, K, r = 384, 192, 8
    W = (torch.randn(rows, K, generator=g) * 0.03).cuda()
    A, Bt = torch.randn(r, K, generator=g).cuda(), torch.randn(r, rows, generator=g).cuda()
    dst, dst2 = torch.empty(rows, K, dtype=OPD, device="cuda"), torch.empty(rows, K, dtype=OPD, device="cuda")
    ops.lora_merge(W, 0, rows, A, Bt, 0.0, dst, dst2=dst2, mul_rows=(0, 128), mul=ops.Q_PRESCALE)
    assert torch.equal(_bits(dst), _bits(ops.cast_bf16(W)))
    sc = torch.empty(1, rows * K, dtype=OPD, device="cuda")
    ops.scale_copy(W.view(-1), 0, 1, 128 * K, rows * K, ops.Q_PRESCALE, out_bf16=sc)
    assert torch.equal(_bits(dst2), _bits(sc.view(rows, K)))
    Wm = W.clone()
    ops.lora_merge(Wm, 0, rows, A, Bt, 0.125, dst, dst_f32=Wm)
    ref = W.double() + 0.125 * (Bt.double().t() @ A.double())
    assert rel_l2(Wm.cpu(), ref.cpu()) < 1e-6
    assert torch.equal(_bits(dst), _bits(Wm.to(OPD)))


def test_merge_refuses_bad_arguments():
    L = _lib.load()
    W = torch.zeros(64, 64, device="cuda")
    A, Bt = torch.zeros(4, 64, device="cuda"), torch.zeros(4, 64, device="cuda")
    dst = torch.full((64, 64), 1.0, dtype=OPD, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                                             # noqa: E731

    def call(lo=0, hi=64, K=64, r=4, ld=64, ldbt=64, dstp=None):
        return L.pxa_lora_merge(p(W), ld, lo, hi, K, p(A), p(Bt), ldbt, r, 1.0, dstp if dstp is not None else p(dst), 64, None, 0, 0, 0, 1.0, None, None)
    assert call() == 0
    torch.cuda.synchronize()
    dst.fill_(1.0)
    for kw in (dict(r=0), dict(r=65), dict(lo=8, hi=8), dict(K=62), dict(ld=32), dict(ldbt=16), dict(dstp=C.c_void_p(0))):
        assert call(**kw) != 0, kw
        assert b"pxa_lora_merge" in L.pxa_last_error()
    torch.cuda.synchronize()
    assert bool((dst == 1.0).all())                                                    # nothing was launched


# ---------------------------------------------------------------------------------------------- backward
BWD_MS, BWD_RS = (1, 77, 300, 1024 + 64), (1, 4, 16, 64)
BWD_SHAPES = {"192x192": (192, 192, 192, 0), "1152x2304of3456": (1152, 2304, 3456, 1152)}       # K, N, lddy, first column of the block
_REF = {}


def _bwd_case(shape, M, r):
    """Inputs (16-bit, on the host), the fp64 reference and the host emulation's error, made once per case and shared."""
    key = (shape, M, r)
    if key not in _REF:
        K, N, lddy, col0 = BWD_SHAPES[shape]
        g = torch.Generator().manual_seed(1000 * M + 10 * r + len(shape))
        x = torch.randn(M, K, generator=g).to(OPD)
        dy = (torch.randn(M, N, generator=g) * 0.05).to(OPD)
        A16 = (torch.randn(r, K, generator=g) / r).to(OPD)
        Bt16 = (torch.randn(r, N, generator=g) * 0.05).to(OPD)
        s = 0.5
        xd, dyd, Ad, Bd = x.double(), dy.double(), A16.double(), Bt16.double()
        ref = (s * (dyd @ Bd.t()).t() @ xd, s * (xd @ Ad.t()).t() @ dyd)              # dA = s u^T x, dBt = s t^T dy, nothing rounded
        t16 = (x.float() @ A16.float().t()).to(OPD).float()                           # the emulation: fp32 products, t / u rounded once, fp32 accumulation
        u16 = (dy.float() @ Bt16.float().t()).to(OPD).float()
        emu = (s * u16.t() @ x.float(), s * t16.t() @ dy.float())
        _REF[key] = dict(x=x, dy=dy, A16=A16, Bt16=Bt16, s=s, ref=ref, emu_err=(rel_l2(emu[0], ref[0]), rel_l2(emu[1], ref[1])))
    return _REF[key]


@pytest.mark.parametrize("r", BWD_RS)
@pytest.mark.parametrize("M", BWD_MS)
@pytest.mark.parametrize("shape", list(BWD_SHAPES))
def test_bwd_matches_fp64_within_the_one_permitted_rounding(shape, M, r):
    from pixart_sigma_amd import ops
    K, N, lddy, col0 = BWD_SHAPES[shape]
    c = _bwd_case(shape, M, r)
    x, xflat = _banded(M, K, OPD, fill=c["x"])
    dy, dyflat = _banded(M, N, OPD, ld=lddy, col0=col0, fill=c["dy"])                   # the other columns of the wider matrix are NaN
    A16, _ = _banded(r, K, OPD, fill=c["A16"])
    Bt16, _ = _banded(r, N, OPD, fill=c["Bt16"])
    dA, dAflat = _banded(r, K, torch.float32, fill=torch.zeros(r, K))
    dBt, dBflat = _banded(r, N, torch.float32, fill=torch.zeros(r, N))
    before = dAflat.clone(), dBflat.clone()
    ops.lora_bwd(x, dy, A16, Bt16, c["s"], dA, dBt)
    torch.cuda.synchronize()
    once = dA.clone(), dBt.clone()
    for name, got, ref, emu in (("dA", dA, c["ref"][0], c["emu_err"][0]), ("dBt", dBt, c["ref"][1], c["emu_err"][1])):
        assert torch.isfinite(got).all(), f"{name}: poison was read"
        e = rel_l2(got.cpu(), ref)
        print(f"\n[{shape} M={M} r={r}] {name} rel-L2 {e:.2e}; host emulation (t, u rounded once) {emu:.2e}, bound {BWD_FACTOR:g}x = {BWD_FACTOR * emu:.2e}")
        record_parity(f"lora_bwd {shape} M={M} r={r}: {name} vs fp64", e, BWD_FACTOR * emu)
        assert e <= BWD_FACTOR * emu            # emulation figures: header of this file (bf16 4.9e-4 ... 2.2e-3, fp16 3.5e-5 ... 4.0e-4)
    for fl, bef, n in ((dAflat, before[0], r * K), (dBflat, before[1], r * N)):
        def inside(mask, n=n):
            mask[GUARD:GUARD + n] = False
        assert _untouched_outside(fl, bef, inside), "written outside the output"
    # += : a second call doubles the result (the partial sums are the same bits, so exactly; allowed: fp32 rounding)
    ops.lora_bwd(x, dy, A16, Bt16, c["s"], dA, dBt)
    torch.cuda.synchronize()
    for got, first in ((dA, once[0]), (dBt, once[1])):
        assert rel_l2(got, 2 * first) <= 1e-6


def test_bwd_refuses_bad_arguments_without_launching():
    L = _lib.load()
    M, K, N, r = 64, 64, 128, 4
    x, dy = torch.zeros(M, K, dtype=OPD, device="cuda"), torch.zeros(M, N, dtype=OPD, device="cuda")
    A16, Bt16 = torch.zeros(r, K, dtype=OPD, device="cuda"), torch.zeros(r, N, dtype=OPD, device="cuda")
    dA, dBt = torch.full((r, K), 3.0, device="cuda"), torch.full((r, N), 3.0, device="cuda")
    need = L.pxa_lora_bwd_ws_bytes(M, K, N, r)
    assert need > 0 and L.pxa_lora_bwd_ws_bytes(M, K, N, 65) < 0 and L.pxa_lora_bwd_ws_bytes(0, K, N, r) < 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)                                # noqa: E731

    def call(M=M, K=K, N=N, r=r, ldx=K, lddy=N, xp=None, wsb=need):
        return L.pxa_lora_bwd(xp if xp is not None else p(x), ldx, p(dy), lddy, p(A16), p(Bt16), M, K, N, r, 1.0, p(dA), p(dBt), p(ws), wsb, None)
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((dA == 3.0).all())                                                     # zeros in: += 0
    for kw in (dict(r=0), dict(r=65), dict(M=0), dict(K=96), dict(N=100), dict(ldx=32), dict(lddy=N + 4), dict(xp=p(x, 2)), dict(wsb=need - 1), dict(xp=C.c_void_p(0))):
        dA.fill_(3.0)
        assert call(**kw) != 0, kw
        assert b"pxa_lora_bwd" in L.pxa_last_error()
    torch.cuda.synchronize()
    assert bool((dA == 3.0).all()) and bool((dBt == 3.0).all())
    from pixart_sigma_amd import ops
    with pytest.raises(AssertionError):
        ops.lora_bwd(x, dy[:, :64], A16, Bt16, 1.0, dA, dBt)                           # Bt16 does not fit the column block
