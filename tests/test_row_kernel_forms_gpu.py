"""The row kernels of csrc/norm.hip in the aliased / strided forms the training step uses (pixart_sigma_amd/engine.py), at batches of more than COLSUM_SLOTS
samples and at token counts that do not fit the kernels' blocking, with per-row / per-sample error metrics and guard bands (helpers and band conventions:
tests/test_gemm_grad_forms_gpu.py).  References in fp64 from the same operand-rounded inputs: closed-form LayerNorm backward, plain sums.  D = 1152.

Blocking (csrc/norm.hip).  Backward kernels (ln_mod_bwd, gate_bwd): a 256-thread block = 8 half-waves x BWD_ROWS = 16 rows = ROWS_PER_BLOCK = 128 rows, walked
interleaved (half-wave h takes rows first + h + 8 i).  A block whose rows belong to one sample combines its column sums in LDS and adds once; any other block lets
every half-wave flush with atomics whenever its walk enters another sample.  The bias-gradient partials go to slot b % COLSUM_SLOTS.  Forward kernel: 8 rows
per block.  Each geometry asserts the property it is there for from these constants, so that the table is re-derived if the blocking changes:

  (B, N)      R      why
  (19, 128)   2432   one sample per block, b % 16 wraps for samples 16 - 18
  (21, 40)    840    blocks straddle up to 4 samples (per-half-wave flush path), slots wrap, partial last block
  (40, 5)     200    every row of a half-wave's walk is in a different sample: a flush per row
  (1, 200)    200    partial last block that IS one sample (LDS combine with short walks)
  (1, 131)    131    likewise with 3 rows in the last block: five half-waves have no row at all
  (3, 37)     111    R % 8 != 0: the forward kernel's last 8-row block is partial
  (2, 4096)   8192   the 1024 px token count

Bounds (none new): dx by worst row 1e-5 and dshift / dscale per sample 1e-5 (test_kernels_gpu.py::test_ln_mod_bwd), the bias gradient folded over its slots 1e-5,
gate_bwd's dx_out 1e-6, dgate per sample 1e-5, 16-bit outputs by worst row BF16_TOL, mean / rstd per row 1e-4 (absolute) / 1e-5 (relative)
(test_ln_mod_fwd_variants), colsum whole-vector 1e-5 (test_gate_bwd_and_colsum).

Census: engine.py call site -> test
  block_bwd  ln_mod_bwd(dxn, x, mean, rstd, mod[:, 1], 6D, G, G, dmod[:, 0], dmod[:, 1], 6D, N)                test_ln_mod_bwd_forms[aliased]
  block_bwd  ln_mod_bwd(..., mod[:, 4], 6D, G, G, dmod[:, 3], dmod[:, 4], 6D, N, dx_bf16=du, dbias=pb(...))    test_ln_mod_bwd_forms[aliased_dbias]
  backward   ln_mod_bwd(..., fin_mod[:, 1], 2D, None, G, dfin[:, 0], dfin[:, 1], 2D, N)                        test_ln_mod_bwd_forms[final]
  block_bwd  gate_bwd(G, u=u3, gate=mod[:, 5], du=du, dgate=dmod[:, 5], dbias=pb(...))                         test_gate_bwd_forms[mlp]
  block_bwd  gate_bwd(G, add=gq, u=u1, gate=mod[:, 2], dx_out=G, du=du, dgate=dmod[:, 2], dbias=pb(...))       test_gate_bwd_forms[attn_in_place]
  caption_bwd gate_bwd(dye_f32, du=dye, rows_per_batch=R)                                                      test_gate_bwd_forms[cast]
  block_fwd  ln_mod_fwd(x1, sl, scl, 6D, u=u2, x_out=x1, rows_per_batch=N, want_stats=True)                    test_ln_mod_fwd_forms[in_place]
  forward    ln_mod_fwd(x, fin_mod[:, 0], fin_mod[:, 1], 2D, u=u, gate=gate, gate_stride=6D, ...)              test_ln_mod_fwd_forms[final_strides]
  (every output of pxa_ln_mod_fwd banded behind row R)                                                         test_ln_mod_fwd_forms[banded]
  _lin_bwd   colsum(dy, grad_bias)                                                                             test_colsum_forms"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import record_parity, rel_l2  # noqa: E402
from test_gemm_grad_forms_gpu import GUARD, MINUS_ZERO32, SENTINEL16, SENTINEL32, Banded, worst_row  # noqa: E402
from test_kernels_gpu import BF16_TOL, _gpu_rnd, _opd, bf, ops, rnd  # noqa: E402,F401

D = 1152
ROWS_PER_BLOCK = 128      # backward kernels: 8 half-waves x BWD_ROWS = 16 rows
HALF_WAVES = 8            # ... and the stride of a half-wave's interleaved walk
FWD_ROWS_PER_BLOCK = 8    # ln_mod_fwd: one row per half-wave
EPS = 1e-6
DX_TOL, SUM_TOL, DXO_TOL, MEAN_TOL, RSTD_TOL = 1e-5, 1e-5, 1e-6, 1e-4, 1e-5

# (B, N, why)
GEOMETRIES = [(19, 128, "sample_per_block"), (21, 40, "straddle"), (40, 5, "flush_per_row"), (1, 200, "partial_one_sample"), (1, 131, "idle_half_waves"),
              (3, 37, "fwd_partial"), (2, 4096, "px1024")]


def geometry_id(g):
    return f"B{g[0]}xN{g[1]}"


def assert_geometry(ops, B, N, why):
    R = B * N
    if why == "sample_per_block":
        assert N == ROWS_PER_BLOCK and B > ops.COLSUM_SLOTS
    elif why == "straddle":
        assert N < ROWS_PER_BLOCK and ROWS_PER_BLOCK % N != 0 and (ROWS_PER_BLOCK - 1) // N + 1 == 4 and B > ops.COLSUM_SLOTS and R % ROWS_PER_BLOCK != 0
    elif why == "flush_per_row":
        assert N <= HALF_WAVES and B > ops.COLSUM_SLOTS and R % ROWS_PER_BLOCK != 0
    elif why == "partial_one_sample":
        assert B == 1 and R > ROWS_PER_BLOCK and R % ROWS_PER_BLOCK >= HALF_WAVES
    elif why == "idle_half_waves":
        assert B == 1 and R > ROWS_PER_BLOCK and 0 < R % ROWS_PER_BLOCK < HALF_WAVES
    elif why == "fwd_partial":
        assert R % FWD_ROWS_PER_BLOCK != 0 and R % ROWS_PER_BLOCK != 0
    else:
        assert N == 4096 and N % ROWS_PER_BLOCK == 0


# ------------------------------------------------------------------------------------------------ banded buffers of the per-sample / per-slot sums
def banded_mod(B, planes):
    """(whole (B + 2, planes, D), the middle B samples): one whole sample of -0.0 on each side, the B samples +0.0 as the engine's zeros_like."""
    whole = torch.zeros(B + 2, planes, D, device="cuda")
    whole[0] = -0.0
    whole[-1] = -0.0
    return whole, whole[1:B + 1]


def assert_mod_bands(whole, what):
    bits = whole.view(torch.int32)
    for name, band in (("in front of", bits[0]), ("behind", bits[-1])):
        bad = band != MINUS_ZERO32
        assert not bad.any(), f"{what}: {int(bad.sum())} floats {name} the modulation gradient were written"


def banded_part(ops):
    """(whole (16 + 2, GUARD + D + GUARD) of -0.0, the (16, D) partials view at column GUARD of rows 1 ... 16, zeroed): a slot of -0.0 on each side and
    GUARD columns of -0.0 left and right of every slot, as a bias's column range inside a block's wider partials buffer."""
    whole = torch.full((ops.COLSUM_SLOTS + 2, D + 2 * GUARD), MINUS_ZERO32, dtype=torch.int32, device="cuda").view(torch.float32)
    part = whole[1:-1, GUARD:GUARD + D]
    part.zero_()
    return whole, part


def assert_part_bands(whole, what):
    bits = whole.view(torch.int32).clone()
    bits[1:-1, GUARD:GUARD + D] = MINUS_ZERO32
    bad = bits != MINUS_ZERO32
    assert not bad.any(), f"{what}: {int(bad.sum())} floats around the bias-gradient partials were written (first at {bad.nonzero()[0].tolist()})"


def per_sample(label, got, ref, bound):
    """max over the samples b of the rel-L2 of got[b] (D,) against ref[b]."""
    e = worst_row(got.reshape(-1, D), ref.reshape(-1, D))
    print(f"  [{label}] worst sample {e:.2e} (bound {bound:.0e})")
    record_parity(f"{label} worst sample", e, bound)
    assert e < bound, (label, e, bound)


def per_row(label, got, ref, bound):
    e = worst_row(got, ref)
    print(f"  [{label}] worst row {e:.2e} (bound {bound:.0e})")
    record_parity(f"{label} worst row", e, bound)
    assert e < bound, (label, e, bound)


def whole_vector(label, got, ref, bound):
    e = rel_l2(got, ref)
    print(f"  [{label}] rel-L2 {e:.2e} (bound {bound:.0e})")
    record_parity(label, e, bound)
    assert e < bound, (label, e, bound)


def rows_of(t, N):
    """(B, D) per-sample values -> (B * N, D) per-row values"""
    return t.repeat_interleave(N, 0)


# ------------------------------------------------------------------------------------------------ 1. ln_mod_bwd
@pytest.mark.parametrize("form", ["aliased", "final", "aliased_dbias"])
@pytest.mark.parametrize("geom", GEOMETRIES, ids=geometry_id)
def test_ln_mod_bwd_forms(ops, geom, form):
    """aliased        dx_in is dx_out: one tensor G, planes 0 / 1 of a (B, 6, D) modulation (engine.py block_bwd, the norm1 call);
    final          dx_in = None, mod_stride = dmod_stride = 2 D into a (B, 2, D) buffer (engine.py backward, the final layer);
    aliased_dbias  aliased + dx_bf16 + the bias-gradient partials as a column range of a wider (16, W) buffer, planes 3 / 4 (block_bwd, the norm2 call).
    The aliased forms must equal the two-tensor call bit for bit in dx."""
    B, N, why = geom
    assert_geometry(ops, B, N, why)
    R = B * N
    label = f"ln_mod_bwd {form} {geometry_id(geom)}"
    planes, (p_shift, p_scale) = (2, (0, 1)) if form == "final" else (6, (3, 4) if form == "aliased_dbias" else (0, 1))
    st = planes * D
    x, dy, dxin = _gpu_rnd(R, D, seed=1), bf(_gpu_rnd(R, D, seed=3)), _gpu_rnd(R, D, seed=4)
    mod = _gpu_rnd(B, planes, D, scale=0.3, seed=2)
    scale = mod[:, p_scale]
    stats = ops.ln_mod_fwd(x, mod[:, p_shift], scale, st, rows_per_batch=N, want_stats=True)
    # fp64 closed form
    x64, dy64 = x.double(), dy.double()
    mu, rs = x64.mean(1, keepdim=True), (x64.var(1, unbiased=False, keepdim=True) + EPS).rsqrt()
    xh = (x64 - mu) * rs
    g = dy64 * (1 + rows_of(scale.double(), N))
    dx64 = rs * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    if form != "final":
        dx64 = dx64 + dxin.double()
    dshift64, dscale64 = dy64.view(B, N, D).sum(1), (dy64 * xh).view(B, N, D).sum(1)
    # the two-tensor call: plain buffers
    dmod0, dx0 = torch.zeros(B, planes, D, device="cuda"), torch.empty_like(x)
    ops.ln_mod_bwd(dy, x, stats["mean"], stats["rstd"], scale, st, None if form == "final" else dxin, dx0, dmod0[:, p_shift], dmod0[:, p_scale], st, N)
    # the engine's form: banded buffers
    G = Banded(R, D, torch.float32, SENTINEL32)
    mod_whole, dmod = banded_mod(B, planes)
    kw, dxb, part_whole = {}, None, None
    if form == "final":
        G.view.fill_(float("nan"))
        dx_in = None
    else:
        G.view.copy_(dxin)
        dx_in = G.view
    if form == "aliased_dbias":
        dxb = Banded(R, D, _opd(), SENTINEL16)
        dxb.view.fill_(float("nan"))
        part_whole, part = banded_part(ops)
        assert part.stride(0) == D + 2 * GUARD
        kw = dict(dx_bf16=dxb.view, dbias=part)
    ops.ln_mod_bwd(dy, x, stats["mean"], stats["rstd"], scale, st, dx_in, G.view, dmod[:, p_shift], dmod[:, p_scale], st, N, **kw)
    torch.cuda.synchronize()
    G.assert_intact(f"{label}: dx")
    assert_mod_bands(mod_whole, label)
    print(f"\n{label}")
    assert torch.equal(G.view, dx0), f"{label}: dx differs from the two-tensor call in {int((G.view != dx0).sum())} elements"
    per_row(f"{label} dx", G.view, dx64, DX_TOL)
    per_sample(f"{label} dshift", dmod[:, p_shift], dshift64, SUM_TOL)
    per_sample(f"{label} dscale", dmod[:, p_scale], dscale64, SUM_TOL)
    others = [p for p in range(planes) if p not in (p_shift, p_scale)]
    assert (dmod[:, others].contiguous().view(torch.int32) == 0).all(), f"{label}: a modulation plane the call does not own was written"
    if form == "aliased_dbias":
        dxb.assert_intact(f"{label}: dx_bf16")
        assert_part_bands(part_whole, label)
        per_row(f"{label} dx_bf16", dxb.view, dx64, BF16_TOL)
        whole_vector(f"{label} dbias folded", part.double().sum(0), dx64.sum(0), SUM_TOL)


# ------------------------------------------------------------------------------------------------ 2. gate_bwd
@pytest.mark.parametrize("form", ["mlp", "attn_in_place", "cast"])
@pytest.mark.parametrize("geom", GEOMETRIES, ids=geometry_id)
def test_gate_bwd_forms(ops, geom, form):
    """mlp            no `add`, no dx_out: du = gate * G, dgate, the bias-gradient partials (engine.py block_bwd, the MLP branch, plane 5);
    attn_in_place  G <- G + add with dx_out is dx, then the same (block_bwd, the self-attention branch, plane 2); bit-identical to the two-tensor call;
    cast           du = the 16-bit copy of dx, rows_per_batch = R, nothing else (caption_bwd)."""
    B, N, why = geom
    assert_geometry(ops, B, N, why)
    R = B * N
    label = f"gate_bwd {form} {geometry_id(geom)}"
    g0, add, u = _gpu_rnd(R, D, seed=1), bf(_gpu_rnd(R, D, seed=2)), bf(_gpu_rnd(R, D, seed=3))
    mod = _gpu_rnd(B, 6, D, scale=0.3, seed=4)
    du = Banded(R, D, _opd(), SENTINEL16)
    du.view.fill_(float("nan"))
    print(f"\n{label}")
    if form == "cast":
        ops.gate_bwd(g0, du=du.view, rows_per_batch=R)
        torch.cuda.synchronize()
        du.assert_intact(f"{label}: du")
        per_row(f"{label} du", du.view, g0.double(), BF16_TOL)
        return
    plane = 5 if form == "mlp" else 2
    gate = mod[:, plane]
    g64 = g0.double() + (add.double() if form == "attn_in_place" else 0)
    du64 = g64 * rows_of(gate.double(), N)
    dgate64 = (g64 * u.double()).view(B, N, D).sum(1)
    mod_whole, dmod = banded_mod(B, 6)
    part_whole, part = banded_part(ops)
    G = Banded(R, D, torch.float32, SENTINEL32)
    G.view.copy_(g0)
    if form == "mlp":
        ops.gate_bwd(G.view, u=u, gate=gate, mod_stride=6 * D, du=du.view, dgate=dmod[:, plane], dmod_stride=6 * D, rows_per_batch=N, dbias=part)
    else:
        dxo, du0, dmod0 = torch.empty_like(g0), torch.empty(R, D, dtype=_opd(), device="cuda"), torch.zeros(B, 6, D, device="cuda")
        ops.gate_bwd(g0, add=add, u=u, gate=gate, mod_stride=6 * D, dx_out=dxo, du=du0, dgate=dmod0[:, plane], dmod_stride=6 * D, rows_per_batch=N)
        ops.gate_bwd(G.view, add=add, u=u, gate=gate, mod_stride=6 * D, dx_out=G.view, du=du.view, dgate=dmod[:, plane], dmod_stride=6 * D, rows_per_batch=N, dbias=part)
    torch.cuda.synchronize()
    G.assert_intact(f"{label}: dx")
    du.assert_intact(f"{label}: du")
    assert_mod_bands(mod_whole, label)
    assert_part_bands(part_whole, label)
    if form == "mlp":
        assert torch.equal(G.view, g0), f"{label}: dx was written without a dx_out"
    else:
        assert torch.equal(G.view, dxo) and torch.equal(du.view, du0), f"{label}: the in-place call differs from the two-tensor call"
        per_row(f"{label} dx_out", G.view, g64, DXO_TOL)
    per_row(f"{label} du", du.view, du64, BF16_TOL)
    per_sample(f"{label} dgate", dmod[:, plane], dgate64, SUM_TOL)
    others = [p for p in range(6) if p != plane]
    assert (dmod[:, others].contiguous().view(torch.int32) == 0).all(), f"{label}: a modulation plane the call does not own was written"
    whole_vector(f"{label} dbias folded", part.double().sum(0), du64.sum(0), SUM_TOL)


# ------------------------------------------------------------------------------------------------ 3. ln_mod_fwd
def check_ln_fwd(label, N, x_out, xn, mean, rstd, xr64, shift, scale, xb=None):
    mu, var = xr64.mean(1), xr64.var(1, unbiased=False)
    rs = (var + EPS).rsqrt()
    xn64 = (xr64 - mu[:, None]) * rs[:, None] * (1 + rows_of(scale.double(), N)) + rows_of(shift.double(), N)
    per_row(f"{label} x", x_out, xr64, DXO_TOL)
    per_row(f"{label} xn", xn, xn64, BF16_TOL)
    if xb is not None:
        per_row(f"{label} xb", xb, xr64, BF16_TOL)
    e_mean, e_rstd = (mean.double() - mu).abs().max().item(), ((rstd.double() - rs).abs() / rs).max().item()
    print(f"  [{label}] mean: max abs error {e_mean:.2e} (bound {MEAN_TOL:.0e}); rstd: max rel error {e_rstd:.2e} (bound {RSTD_TOL:.0e})")
    record_parity(f"{label} mean max abs", e_mean, MEAN_TOL)
    record_parity(f"{label} rstd max rel", e_rstd, RSTD_TOL)
    assert e_mean < MEAN_TOL and e_rstd < RSTD_TOL, (label, e_mean, e_rstd)


@pytest.mark.parametrize("form", ["in_place", "final_strides", "banded"])
@pytest.mark.parametrize("geom", GEOMETRIES, ids=geometry_id)
def test_ln_mod_fwd_forms(ops, geom, form):
    """in_place       x_out is x with the ungated residual, LayerNorm and statistics (engine.py block_fwd, the norm2 call): bit-identical to the two-tensor call;
    final_strides  mod_stride = 2 D for shift / scale, gate_stride = 6 D for the previous block's gate (engine.py forward, the final layer);
    banded         pxa_ln_mod_fwd with every output on (x_out, xn, xb, mean, rstd), each a view with bands: nothing behind row R (R = 111: a partial last block)."""
    B, N, why = geom
    assert_geometry(ops, B, N, why)
    R = B * N
    label = f"ln_mod_fwd {form} {geometry_id(geom)}"
    x, u = _gpu_rnd(R, D, seed=1), bf(_gpu_rnd(R, D, seed=2))
    mod, fin = _gpu_rnd(B, 6, D, scale=0.3, seed=3), _gpu_rnd(B, 2, D, scale=0.3, seed=5)
    print(f"\n{label}")
    if form == "in_place":
        shift, scale = mod[:, 3], mod[:, 4]
        r0 = ops.ln_mod_fwd(x, shift, scale, 6 * D, u=u, rows_per_batch=N, want_stats=True)
        x1 = Banded(R, D, torch.float32, SENTINEL32)
        x1.view.copy_(x)
        r = ops.ln_mod_fwd(x1.view, shift, scale, 6 * D, u=u, x_out=x1.view, rows_per_batch=N, want_stats=True)
        torch.cuda.synchronize()
        x1.assert_intact(f"{label}: x")
        assert r["x"].data_ptr() == x1.view.data_ptr()
        for k in ("x", "xn", "mean", "rstd"):
            assert torch.equal(r[k], r0[k]), f"{label}: {k} differs from the two-tensor call"
        check_ln_fwd(label, N, x1.view, r["xn"], r["mean"], r["rstd"], x.double() + u.double(), shift, scale)
        return
    shift, scale, gate = fin[:, 0], fin[:, 1], mod[:, 5]
    xr64 = x.double() + rows_of(gate.double(), N) * u.double()
    r = ops.ln_mod_fwd(x, shift, scale, 2 * D, u=u, gate=gate, gate_stride=6 * D, rows_per_batch=N, want_stats=True, want_xb=form == "banded")
    if form == "final_strides":
        check_ln_fwd(label, N, r["x"], r["xn"], r["mean"], r["rstd"], xr64, shift, scale)
        return
    from pixart_sigma_amd.lib import call, ptr
    xo, xn, xb = Banded(R, D, torch.float32, SENTINEL32), Banded(R, D, _opd(), SENTINEL16), Banded(R, D, _opd(), SENTINEL16)
    mean, rstd = Banded(R, 1, torch.float32, SENTINEL32), Banded(R, 1, torch.float32, SENTINEL32)
    for t in (xo, xn, xb, mean, rstd):
        t.view.fill_(float("nan"))
    assert mean.view.stride(0) == 1 and rstd.view.stride(0) == 1
    call("pxa_ln_mod_fwd", ptr(x), ptr(u), ptr(gate), 6 * D, ptr(shift), ptr(scale), 2 * D, ptr(xo.view), ptr(xn.view), ptr(xb.view), ptr(mean.view), ptr(rstd.view),
         R, D, N, EPS)
    torch.cuda.synchronize()
    for name, t in (("x_out", xo), ("xn", xn), ("xb", xb), ("mean", mean), ("rstd", rstd)):
        t.assert_intact(f"{label}: {name}")
    assert torch.equal(xo.view, r["x"]) and torch.equal(xn.view, r["xn"]) and torch.equal(xb.view, r["xb"])
    assert torch.equal(mean.view[:, 0], r["mean"]) and torch.equal(rstd.view[:, 0], r["rstd"])
    check_ln_fwd(label, N, xo.view, xn.view, mean.view[:, 0], rstd.view[:, 0], xr64, shift, scale, xb=xb.view)


# ------------------------------------------------------------------------------------------------ 4. colsum
@pytest.mark.parametrize("R,N,ld", [(65536, 32, 32), (371, 2304, 2304), (1, 1152, 1152), (4801, 1152, 1152), (777, 1096, 1096), (4800, 1152, 2304)])
def test_colsum_forms(ops, R, N, ld):
    """pxa_colsum_bf16 as _lin_bwd calls it, accumulating into a random bias gradient: (65536, 32) the final layer's bias (one column group, 44 of its 48 column
    threads idle), ragged row counts down to one row, N % 384 != 0, and a column slice of a wider tensor (ld > N: the k / v halves of dkvc).  The output is the
    middle of a longer vector whose -0.0 bands must keep their sign bit."""
    assert N % 8 == 0 and ld % 8 == 0
    if (R, N) == (65536, 32):
        assert N // 8 == 4 and 48 - N // 8 == 44
    if N == 1096:
        assert N % 384 != 0
    wide = bf(_gpu_rnd(R, ld, seed=5))
    dy = wide[:, ld - N:]
    assert dy.stride(0) == ld
    whole = torch.full((N + 2 * GUARD,), MINUS_ZERO32, dtype=torch.int32, device="cuda").view(torch.float32)
    out = whole[GUARD:GUARD + N]
    out0 = _gpu_rnd(N, seed=6)
    out.copy_(out0)
    ops.colsum(dy, out)
    torch.cuda.synchronize()
    bits = whole.view(torch.int32)
    assert (bits[:GUARD] == MINUS_ZERO32).all() and (bits[GUARD + N:] == MINUS_ZERO32).all(), f"colsum {R}x{N}: an add outside out[:N]"
    print(f"\ncolsum {R}x{N} ld {ld}")
    whole_vector(f"colsum {R}x{N} ld {ld}", out, out0.double() + dy.double().sum(0), SUM_TOL)
