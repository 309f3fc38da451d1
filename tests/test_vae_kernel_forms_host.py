"""The bounds of tests/test_vae_kernel_forms_gpu.py, checked without a GPU: for every bounded case an emulation of a CORRECT kernel in torch (the fp32
formula and one .to(dtype), both operand types) passes the very bound the GPU test asserts, and the same emulation with a SECOND rounding (fp32 -> operand
type -> arithmetic -> operand type) fails it - the bounds are neither unreachable nor vacuous.  The references, the bounds and the inputs are the GPU file's
own functions, called here with the dtype the GPU test takes from ops.BF16.  SMALL_OUT_NORM_TOL is taken from here: 2 x the emulation's worst row."""
import pytest
import torch

import test_vae_kernel_forms_gpu as forms

DTYPES = [torch.bfloat16, torch.float16]
ACT_CASES = [(c, w) for c, w in forms.GN_APPLY_CASES if c[7] or c[8]]          # (H, W, C, groups, upsample, layouts, norm, silu)


def _ids(v):
    return str(v).replace("torch.", "") if isinstance(v, torch.dtype) else None


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_element_bound_passes_one_rounding_and_fails_two(dtype):
    """gn_apply / im2col / the staged operand of small_out: act(norm(x)) of every gn_apply case (upsampling and the patch gather copy stored values)."""
    margins = []
    for (H, W, C, groups, up, _, _, norm, silu), _ in ACT_CASES:
        c = forms.norm_case(dtype, 2, C, H, W, groups, seed=2)
        want, A = forms.act_ref(c, norm, silu)
        bound = forms.elem_bound(want, A, dtype)
        one, _ = forms.worst_row(forms.grid_rows(forms.act_emulate(c, norm, silu, dtype)), forms.grid_rows(want), forms.grid_rows(bound))
        two, _ = forms.worst_row(forms.grid_rows(forms.act_emulate(c, norm, silu, dtype, second_rounding=True)), forms.grid_rows(want), forms.grid_rows(bound))
        margins.append((one, two))
        assert one <= 1.0, ((H, W, C, norm, silu), one)
        assert two > 1.0, ((H, W, C, norm, silu), two)
    print(f"\n{dtype}: one rounding worst {max(m[0] for m in margins):.3f} of the bound, two roundings {min(m[1] for m in margins):.3f} ... {max(m[1] for m in margins):.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("level", [1, 80])
def test_softmax_bound_passes_one_rounding_and_fails_two(dtype, level):
    for cols in forms.SOFTMAX_COLS:
        scale = (512 if level == 1 else 256) ** -0.5
        s = forms.softmax_scores(cols, scale, level, seed=cols)
        want, z = forms.softmax_ref(s, scale)
        assert float(z.min()) >= -80.0
        bound = forms.elem_bound(want, torch.zeros_like(want), dtype)
        one, _ = forms.worst_row(forms.softmax_emulate(s, scale, dtype), want, bound)
        two, _ = forms.worst_row(forms.softmax_emulate(s, scale, dtype, second_rounding=True), want, bound)
        assert one <= 1.0, (cols, one)
        assert two > 1.0 or cols == 8, (cols, two)            # 8 columns: too few elements for a double rounding to be certain
        p = forms.softmax_emulate(s, scale, dtype).double()
        assert (p.sum(1) - 1.0).abs().max() <= cols * 2.0 ** -forms.p_bits(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_small_out_bounds(dtype):
    """Without the norm the emulation passes 2e-5 per row; with it, SMALL_OUT_NORM_TOL is 2 x the emulation's worst row (rounded up to two digits, so the
    emulation sits between 0.47 and 0.5 of it) and a second rounding of the staged operand fails it."""
    worst = 0.0
    for Co, C, groups, H, W, _, norm, bias in forms.SMALL_OUT_CASES:
        c = forms.small_out_case(dtype, Co, C, groups, H, W)
        want = forms.image_rows(forms.small_out_ref(c, norm, bias, dtype))
        one, _ = forms.worst_row(forms.image_rows(forms.small_out_emulate(c, norm, bias, dtype)), want)
        if not norm:
            assert one <= forms.SMALL_OUT_TOL, ((Co, C, H, W), one)
            continue
        worst = max(worst, one)
        two, _ = forms.worst_row(forms.image_rows(forms.small_out_emulate(c, norm, bias, dtype, second_rounding=True)), want)
        assert two > forms.SMALL_OUT_NORM_TOL[dtype], ((Co, C, H, W), two)
    tol = forms.SMALL_OUT_NORM_TOL[dtype]
    print(f"\n{dtype}: small_out with the norm: emulation worst row {worst:.3e}, bound {tol:.1e}")
    assert 0.47 * tol <= worst <= 0.5 * tol, (worst, tol)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_shifted_statistics_bound_is_consistent(dtype):
    """The shifted case: the rounded data has the mean / sigma ratio the bound is derived for, the bound stays inside the project's 2e-5 and above the floor of
    a single fp32 rounding of each sum, and an fp32 emulation of the kernel's summation order (per-thread chains, the quad fold, LDS additions, fp64 across
    blocks) stays inside it."""
    B, C, groups, H, W, r = forms.SHIFT_CASE
    CV, ppb, per_row, nb = forms.gn_stats_launch(H, W, C)
    D = forms.gn_stats_chain(H, W, C, groups)
    bound = forms.shifted_rstd_bound(r, D)
    assert 0.5 * (1 + r * r) * 2.0 ** -24 < bound <= forms.STAT_TOL
    x = forms.cpu_rnd(B, C, H, W, shift=r, seed=5).to(dtype)
    xg = x.double().view(B, groups, -1)
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    ratio = mean / var.sqrt()
    assert (ratio - r).abs().max() < 0.15 * r, ratio
    # the kernel's order: block j owns rows j, j + nb, ...; thread (pixel lane pl, chunk cv) chains its loads; halves fold to quads first
    xf = x.float().permute(0, 2, 3, 1)                                               # (B, H, W, C)
    cpg = C // groups
    s64, q64 = torch.zeros(B, groups, dtype=torch.float64), torch.zeros(B, groups, dtype=torch.float64)
    for blk in range(nb):
        s = torch.zeros(B, ppb, C // 4)
        q = torch.zeros(B, ppb, C // 4)
        for y in range(blk, H, nb):
            for x0 in range(0, W, ppb):
                px = xf[:, y, x0:x0 + ppb].reshape(B, -1, C // 4, 4)                   # (B, pixels of this pass, quads, 4)
                n = px.shape[1]
                s[:, :n] += (px[..., 0] + px[..., 1]) + (px[..., 2] + px[..., 3])
                q[:, :n] += (px[..., 0] * px[..., 0] + px[..., 1] * px[..., 1]) + (px[..., 2] * px[..., 2] + px[..., 3] * px[..., 3])
        red_s, red_q = torch.zeros(B, groups), torch.zeros(B, groups)
        for pl in range(ppb):                                                          # LDS additions, one after the other (any order is a chain this long)
            for k in range(cpg // 4):
                red_s += s[:, pl].view(B, groups, cpg // 4)[..., k]
                red_q += q[:, pl].view(B, groups, cpg // 4)[..., k]
        s64 += red_s.double()
        q64 += red_q.double()
    cnt = H * W * cpg
    m = s64 / cnt
    rstd = ((q64 / cnt - m * m).clamp_min(0) + forms.EPS).rsqrt()
    rel = ((rstd - (var + forms.EPS).rsqrt()).abs() / (var + forms.EPS).rsqrt()).max().item()
    print(f"\n{dtype}: shifted statistics r = {r:g}, D = {D}: emulated rstd error {rel:.2e}, bound {bound:.2e}")
    assert rel <= bound
