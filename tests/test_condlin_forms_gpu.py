"""The fp32 conditioning linears (csrc/condlin.hip: pxa_linear_f32_fwd / _bwd) per element against fp64, at the sizes where their three kernels take another
path: N that is no multiple of the forward's four columns per block (1, 3, 5, 1153) or of the dX kernel's slices of 128 (1, 127, 129, 300), K of 4, just under /
at / over one lane stride of 256 (252, 256, 260) and one block of 1024 (1024, 1028: a second block with one active thread), M of 1, 15, 16, 17, 33 around the 16
rows per pass; with and without bias; every combination of requested gradients the model uses; the model's own forms.  Outputs sit in NaN-filled allocations
(caller-owned buffers through the library's entry points), which must come back bit-identical outside the output.

Bound per element (train_tail_refs.condlin_chain; U = 2^-24):  (roundings on the longest chain) . U . sum_k |a_k| |b_k|
    y    ceil(K / 256) additions in a lane + 3 inside a group of four products + 6 (wave_sum) + 1 (bias), on sum |x||w| + |b|
    dx   min(N, 128) serial additions + 1 (product) + ceil(N / 128) atomics (+ 1 on a pre-filled buffer, + |pre-fill| itself)
    dw   M additions + 1;   db   M additions, on sum |dy|

Measured (MI355X), worst value over bound over all cases: y 0.11, dx 0.96 (M 15, N 1, K 1028 into a pre-filled buffer: a chain of 4, where the pre-fill's own half ulp is most of the bound), dw 0.64, db 0.50."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import record_parity  # noqa: E402
import train_tail_refs as R  # noqa: E402

GUARD = 1024
NAN32 = 0x7FC00000


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _banded(shape, fill=None):
    """(view, allocation): the view sits between GUARD NaNs on either side; it holds `fill` or NaN."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((2 * GUARD + n,), float("nan"), device="cuda")
    view = flat[GUARD:GUARD + n].view(shape)
    if fill is not None:
        view.copy_(fill)
    return view, flat


def _guards_intact(flat):
    b = flat.view(torch.int32)
    return bool((b[:GUARD] == NAN32).all()) and bool((b[-GUARD:] == NAN32).all())


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _inputs(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.05, torch.randn(N, generator=g), torch.randn(M, N, generator=g)


def _check(label, got, ref, mag, chain, extra=None):
    bound = chain * R.U * mag + (0 if extra is None else extra)
    ok, w = R.within(got.cpu(), ref, bound)
    print(f"\n[{label}] worst value / bound {w:.3g} (chain {chain})")
    record_parity(f"condlin {label}: worst element / bound", w, 1.0)
    assert ok, (label, w)


# ---------------------------------------------------------------------------------------------- forward
FWD = [(1, 1, 4), (15, 3, 252), (16, 5, 256), (17, 384, 260), (33, 1153, 1024), (1, 1153, 1028), (16, 384, 1024), (33, 5, 1028), (17, 3, 256), (15, 1, 260),
       (33, 1, 4), (16, 1153, 252)]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("M,N,K", FWD)
def test_forward_per_element_inside_guard_bands(M, N, K, bias):
    from pixart_sigma_amd import lib, ops
    x, w, b, _ = _inputs(M, N, K, 1000 * M + N + K)
    b = b if bias else None
    ref, mag = R.linear_ref64(x, w, b)
    xd, wd, bd = x.cuda(), w.cuda(), (b.cuda() if bias else None)
    y, flat = _banded((M, N))
    assert lib.load().pxa_linear_f32_fwd(_p(xd), _p(wd), _p(bd), _p(y), M, N, K, lib.stream()) == 0
    torch.cuda.synchronize()
    assert _guards_intact(flat), "written outside y"
    _check(f"fwd M{M} N{N} K{K} bias={bias}", y, ref, mag, R.condlin_chain("fwd", M, N, K))
    assert torch.equal(ops.linear_f32_fwd(xd, wd, bd), y)                              # the wrapper makes the same call


# ---------------------------------------------------------------------------------------------- backward
BWD = [(1, 1, 4), (15, 127, 1024), (16, 128, 1028), (17, 129, 4), (33, 300, 1028), (16, 300, 1024), (33, 129, 1028), (1, 128, 4), (17, 127, 4), (15, 1, 1028)]
FLAGS = ["TTT", "FTT", "TFF", "FFT", "TFT", "TTF"]
_BREF = {}


def _bwd_ref(M, N, K):
    if (M, N, K) not in _BREF:
        x, w, _, dy = _inputs(M, N, K, 77 * M + N + 3 * K)
        _BREF[(M, N, K)] = (x, w, dy) + R.linear_bwd_ref64(dy, x, w)
    return _BREF[(M, N, K)]


def _check_bwd(tag, M, N, K, got, refs, mags, prefill=None):
    dx, dw, db = got
    if dx is not None:
        extra = None if prefill is None else R.U * prefill.double().abs()
        ref = refs[0] if prefill is None else refs[0] + prefill.double()
        _check(f"{tag} dx", dx, ref, mags[0], R.condlin_chain("dx", M, N, K, prefill is not None), extra)
    if dw is not None:
        _check(f"{tag} dw", dw, refs[1], mags[1], R.condlin_chain("dw", M, N, K))
    if db is not None:
        _check(f"{tag} db", db, refs[2], mags[2], R.condlin_chain("db", M, N, K))


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("M,N,K", BWD)
def test_backward_flag_combinations_per_element(M, N, K, flags):
    """ops.linear_f32_bwd: a gradient that was not asked for comes back None, one that was is right - whatever the others are."""
    from pixart_sigma_amd import ops
    x, w, dy, refs, mags = _bwd_ref(M, N, K)
    need = [f == "T" for f in flags]
    got = ops.linear_f32_bwd(dy.cuda(), x.cuda(), w.cuda(), need_dx=need[0], need_dw=need[1], need_db=need[2])
    torch.cuda.synchronize()
    for g, nd, name in zip(got, need, ("dx", "dw", "db")):
        assert (g is not None) == nd, f"{name}: requested {nd}, returned {type(g).__name__}"
    _check_bwd(f"bwd M{M} N{N} K{K} {flags}", M, N, K, got, refs, mags)


@pytest.mark.parametrize("M,N,K", BWD)
def test_backward_into_caller_buffers_prefilled_dx(M, N, K):
    """The header's contract, through the entry point: dx ACCUMULATES (pre-fill + dX comes back), dw and db are overwritten (NaN in, values out), db comes from
    the call that writes dw; nothing outside the three outputs is touched."""
    from pixart_sigma_amd import lib
    x, w, dy, refs, mags = _bwd_ref(M, N, K)
    g = torch.Generator().manual_seed(5)
    pre = torch.randn(M, K, generator=g)
    dx, fx = _banded((M, K), fill=pre)
    dw, fw = _banded((N, K))
    db, fb = _banded((N,))
    assert lib.load().pxa_linear_f32_bwd(_p(dy.cuda()), _p(x.cuda()), _p(w.cuda()), _p(dx), _p(dw), _p(db), M, N, K, lib.stream()) == 0
    torch.cuda.synchronize()
    assert _guards_intact(fx) and _guards_intact(fw) and _guards_intact(fb), "written outside an output"
    _check_bwd(f"bwd direct M{M} N{N} K{K}", M, N, K, (dx, dw, db), refs, mags, prefill=pre)
    # dx alone: dw and db stay as they were
    dx2, fx2 = _banded((M, K), fill=torch.zeros(M, K))
    before = fw.clone(), fb.clone()
    assert lib.load().pxa_linear_f32_bwd(_p(dy.cuda()), _p(x.cuda()), _p(w.cuda()), _p(dx2), None, None, M, N, K, lib.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(fw.view(torch.int32), before[0].view(torch.int32)) and torch.equal(fb.view(torch.int32), before[1].view(torch.int32))
    _check_bwd(f"bwd direct dx only M{M} N{N} K{K}", M, N, K, (dx2, None, None), refs, mags)


# ---------------------------------------------------------------------------------------------- the model's own forms
@pytest.mark.parametrize("B", [2, 16])
def test_model_forms(B):
    """t_embedder.mlp[0]: (B, 256 -> 1152) with no dX (its input is the sinusoid table); t_block: (B, 1152 -> 6912); the size embedders: (2B, 256 -> 384)."""
    from pixart_sigma_amd import ops
    for tag, M, K, N, need_dx in (("t_embedder.mlp.0", B, 256, 1152, False), ("t_block", B, 1152, 6912, True), ("csize_embedder.mlp.0", 2 * B, 256, 384, False)):
        x, w, b, dy = _inputs(M, N, K, B + N)
        ref, mag = R.linear_ref64(x, w, b)
        xd, wd, dyd = x.cuda(), w.cuda(), dy.cuda()
        _check(f"{tag} B{B} y", ops.linear_f32_fwd(xd, wd, b.cuda()), ref, mag, R.condlin_chain("fwd", M, N, K))
        got = ops.linear_f32_bwd(dyd, xd, wd, need_dx=need_dx)
        assert (got[0] is None) == (not need_dx)
        _check_bwd(f"{tag} B{B}", M, N, K, got, *R.linear_bwd_ref64(dy, x, w))


# ---------------------------------------------------------------------------------------------- refusals
def test_k_not_a_multiple_of_four_is_refused_and_nothing_is_written():
    from pixart_sigma_amd import lib, ops
    L = lib.load()
    M, N, K = 3, 5, 8
    x, w, b, dy = (t.cuda() for t in _inputs(M, N, K, 1))
    y, fy = _banded((M, N))
    dx, fx = _banded((M, K))
    dw, fw = _banded((N, K))
    db, fb = _banded((N,))
    before = [f.clone() for f in (fy, fx, fw, fb)]
    for k in (6, 7, 0):
        assert L.pxa_linear_f32_fwd(_p(x), _p(w), _p(b), _p(y), M, N, k, lib.stream()) != 0
        assert b"pxa_linear_f32_fwd" in L.pxa_last_error()
        assert L.pxa_linear_f32_bwd(_p(dy), _p(x), _p(w), _p(dx), _p(dw), _p(db), M, N, k, lib.stream()) != 0
        assert b"pxa_linear_f32_bwd" in L.pxa_last_error()
    assert L.pxa_linear_f32_fwd(None, _p(w), _p(b), _p(y), M, N, K, lib.stream()) != 0
    assert L.pxa_linear_f32_bwd(_p(dy), None, _p(w), _p(dx), _p(dw), _p(db), M, N, K, lib.stream()) != 0
    torch.cuda.synchronize()
    for f, bf in zip((fy, fx, fw, fb), before):
        assert torch.equal(f.view(torch.int32), bf.view(torch.int32)), "a refused call wrote"
    with pytest.raises(lib.PixartHipError):
        ops.linear_f32_fwd(torch.zeros(2, 6, device="cuda"), torch.zeros(3, 6, device="cuda"))
