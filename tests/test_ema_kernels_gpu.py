"""pxa_ema_update and pxa_swap_f32 (csrc/ema.hip) per element, between guard bands.

Sizes: 4 (one thread), 1028 (a part-filled block), 4 * 256 * 4096 + 1028 (more than one grid-stride sweep of the 4096-block cap, with a ragged end).
Reference of the update: e + (1 - d) (p - e) in fp64 with d the fp32 value passed.  Bound per element |got - ref| <= 2^-23 max(|e|, |p|), derived, not
measured: 1 - d is exact in fp32 for d in [0.5, 1) (Sterbenz); p - e is rounded once (<= 2^-24 |p - e| <= 2^-23 max), that error is scaled by
om = 1 - d <= 0.5 (<= 2^-24 max); the fma rounds once more (<= 2^-24 |result| <= 2^-24 max, the result lying between e and p).  p == e returns e bit
for bit (fma(om, 0, e) = e).  Both operand builds load the same fp32 kernels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [4, 1028, 4 * 256 * 4096 + 1028]
DECAYS = [0.5, 0.95, 0.9999]
G = 64                       # guard band, elements (keeps the 16-byte alignment of the view between the bands)
BAND = 0x7FC0BEEF            # a quiet NaN with a payload: arithmetic on it, or a store over it, shows


def banded(values):
    """A buffer [band | values | band] of its own allocation; returns (whole buffer, the view between the bands)."""
    n = values.numel()
    buf = torch.full((n + 2 * G,), BAND, dtype=torch.int32, device="cuda").view(torch.float32)
    buf[G:G + n] = values.cuda()
    return buf, buf[G:G + n]


def bands_intact(buf):
    b = buf.view(torch.int32)
    return bool((b[:G] == BAND).all() and (b[-G:] == BAND).all())


def bits(t):
    return t.detach().view(torch.int32).cpu()


def values(n, seed):
    """Normal fp32 values over 13 binades and both signs, exact zeros in both, and a run where p == e."""
    g = torch.Generator().manual_seed(seed)
    def draw():
        return (1 + torch.rand(n, generator=g)) * torch.exp2(torch.randint(-6, 7, (n,), generator=g).float()) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1.0)
    e, p = draw(), draw()
    e[0::7] = 0.0
    p[3::11] = 0.0
    run = slice(n // 2, n // 2 + max(1, n // 8))
    p[run] = e[run]
    return e.float(), p.float()


def reference(e, p, decay):
    d = np.float64(np.float32(decay))
    return e.double() + (1.0 - d) * (p.double() - e.double())


@pytest.fixture(scope="module")
def ops():
    from pixart_sigma_amd import ops
    return ops


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("decay", DECAYS)
def test_ema_update_against_fp64(ops, n, decay):
    e, p = values(n, seed=n % 1000 + int(decay * 1e4))
    ebuf, ev = banded(e)
    pbuf, pv = banded(p)
    ops.ema_update(ev, pv, decay)
    torch.cuda.synchronize()
    got = ev.cpu()
    ref = reference(e, p, decay)
    err = (got.double() - ref).abs()
    bound = 2.0 ** -23 * torch.maximum(e.abs(), p.abs()).double()
    worst = (err - bound).max().item()
    print(f"n={n} decay={decay}: max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert worst <= 0.0, f"{int((err > bound).sum())} elements beyond 2^-23 max(|e|, |p|)"
    same = p == e
    assert same.any() and torch.equal(bits(got)[same], bits(e)[same])            # p == e: e bit for bit
    assert bands_intact(ebuf) and bands_intact(pbuf)
    assert torch.equal(bits(pv), bits(p))                                        # p is only read


def test_ema_update_twice_gives_equal_bits(ops):
    n = SIZES[2]
    e, p = values(n, seed=5)
    outs = []
    for _ in range(2):
        _, ev = banded(e)
        _, pv = banded(p)
        ops.ema_update(ev, pv, 0.9999)
        outs.append(bits(ev))
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("n", SIZES[:2])
def test_scaler_record(ops, n):
    e, p = values(n, seed=11)
    _, ev0 = banded(e)
    _, pv = banded(p)
    ops.ema_update(ev0, pv, 0.95)                                                # null scaler
    for found_inf in (1.0, 0.0):
        ebuf, ev = banded(e)
        sc = torch.tensor([65536.0, 3.0, found_inf, 7.0, 1.0], device="cuda")
        ops.ema_update(ev, pv, 0.95, sc)
        torch.cuda.synchronize()
        assert torch.equal(bits(ev), bits(e) if found_inf else bits(ev0))
        assert bands_intact(ebuf) and torch.equal(sc.cpu(), torch.tensor([65536.0, 3.0, found_inf, 7.0, 1.0]))


@pytest.mark.parametrize("n", SIZES)
def test_swap(ops, n):
    a, b = values(n, seed=n % 1000 + 1)
    abuf, av = banded(a)
    bbuf, bv = banded(b)
    ops.swap_f32(av, bv)
    torch.cuda.synchronize()
    assert torch.equal(bits(av), bits(b)) and torch.equal(bits(bv), bits(a))
    assert bands_intact(abuf) and bands_intact(bbuf)
    ops.swap_f32(av, bv)
    torch.cuda.synchronize()
    assert torch.equal(bits(av), bits(a)) and torch.equal(bits(bv), bits(b))
    assert bands_intact(abuf) and bands_intact(bbuf)


def test_refusals(ops):
    from pixart_sigma_amd.lib import PixartHipError, call, ptr
    n = 1028
    e, p = values(n + 8, seed=3)
    ebuf, ev = banded(e)
    pbuf, pv = banded(p)
    before = bits(ebuf), bits(pbuf)
    cases = [
        ("multiple of 4", lambda: call("pxa_ema_update", ptr(ev), ptr(pv), n + 2, 0.5, None)),
        ("multiple of 4", lambda: call("pxa_swap_f32", ptr(ev), ptr(pv), n + 2)),
        ("multiple of 4", lambda: call("pxa_ema_update", ptr(ev), ptr(pv), 0, 0.5, None)),
        ("16-byte aligned", lambda: ops.ema_update(ev[1:n + 1], pv[:n], 0.5)),
        ("16-byte aligned", lambda: ops.ema_update(ev[:n], pv[1:n + 1], 0.5)),
        ("16-byte aligned", lambda: ops.swap_f32(ev[1:n + 1], pv[:n])),
        (r"decay must lie in \[0, 1\)", lambda: ops.ema_update(ev, pv, 1.0)),
        (r"decay must lie in \[0, 1\)", lambda: ops.ema_update(ev, pv, -0.1)),
        ("same buffer", lambda: ops.ema_update(ev, ev, 0.5)),
        ("null pointer", lambda: call("pxa_ema_update", None, ptr(pv), n, 0.5, None)),
        ("overlap", lambda: ops.swap_f32(ev[:n], ev[8:n + 8])),
        ("overlap", lambda: ops.swap_f32(ev, ev)),
    ]
    for msg, fn in cases:
        with pytest.raises(PixartHipError, match=msg):
            fn()
    torch.cuda.synchronize()
    assert torch.equal(bits(ebuf), before[0]) and torch.equal(bits(pbuf), before[1])      # nothing was launched
