"""CPU tier: the fp64 references and bound functions of tests/train_tail_refs.py, which the GPU files test_loss_forms_gpu.py, test_came_forms_gpu.py and
test_condlin_forms_gpu.py rely on.  Each reference is tied to the statement it restates; each bound passes a result that carries one rounding of the right size,
and fails a planted error and a dropped addend at the smallest shape.

What a planted 2^-18 relative error can and cannot show: a bound of k 2^-24 relative sees it where k < 64 - the MSE half and the per-sample mse of the loss, the
second-moment statistics and the parameters of CAME, every output of the linears at the smallest shapes.  Where the formula itself cancels (the KL / NLL
derivatives: true_mean - mean, cdf_plus - cdf_min, the two lv products; CAME's residual (u - m)^2 and exp_avg behind two rsqrt of long sums) the running error
bound is 1e-5 ... 1e-3 relative by construction, and the test plants an error of 4 x the bound there instead, beside the dropped addend."""
import pytest
import torch

import train_tail_refs as R
from pixart_sigma_amd import IDDPM

PLANT = 2.0 ** -18


@pytest.fixture(scope="module")
def diff():
    return IDDPM("1000", learn_sigma=True, pred_sigma=True, snr=False)


def _edge_lv(diff):
    tab = diff._tab(torch.device("cpu"))
    return float(tab["post_logvar"][0].float()), float(tab["log_betas"][0].float())


def _case64(diff, name):
    c = R.loss_case(name, _edge_lv(diff))
    k8 = R.loss_coef8(diff, c["t"])
    return c, k8, {k: c[k].double() for k in ("out", "x0", "noise", "g_mse", "g_vb")}


def _statement(diff, c, dtype):
    """iddpm.py's torch statement (training_losses) in `dtype` on the host: (mse, vb, d (g_mse mse + g_vb vb) / d out)."""
    out = c["out"].to(dtype).requires_grad_(True)
    terms = diff.training_losses(lambda x, timestep, **kw: out, c["x0"].to(dtype), c["t"], noise=c["noise"].to(dtype))
    (terms["mse"] * c["g_mse"].to(dtype) + terms["vb"] * c["g_vb"].to(dtype)).sum().backward()
    return terms["mse"].detach(), terms["vb"].detach(), out.grad


# ================================================================================================ loss
@pytest.mark.parametrize("name", list(R.LOSS_CASES))
def test_loss_reference_is_the_torch_statement_in_fp64(diff, name):
    """Values and autograd, every regime.  Run in fp64 the statement compares x0 with the DOUBLE 0.999, so the reference is given that constant here; with the fp32
    constant it differs from it at exactly the two planted elements equal to float32(+-0.999) - and there it takes the branch the fp32 statement takes."""
    c, k8, d = _case64(diff, name)
    got = R.loss_ref64_grad(d["out"], d["x0"], d["noise"], k8.double(), c["tzero"], d["g_mse"], d["g_vb"], thr=0.999)
    want = _statement(diff, c, torch.float64)
    for g, w, n in zip(got, want, ("mse", "vb", "d")):
        assert float((g - w).abs().max()) <= 1e-12 * max(1.0, float(w.abs().max())), n
    # the analytic derivative inside the bound form is the same function
    T = R.loss_terms(d["out"], d["x0"], d["noise"], k8.double(), c["tzero"], d["g_mse"], d["g_vb"], thr=0.999)
    assert float((T["d"].v - want[2]).abs().max()) <= 1e-12 * max(1.0, float(want[2].abs().max()))
    assert float((T["mse"].v - want[0]).abs().max()) <= 1e-12 * float(want[0].abs().max()) and float((T["vb"].v - want[1]).abs().max()) <= 1e-12 * float(want[1].abs().max())
    a = T["arg"]
    assert not bool(((a > R.BAND[0]) & (a < R.BAND[1])).any())
    for b, reg in enumerate(c["regimes"]):                                           # the regimes are what the GPU file says they are
        z = T["z"][b]
        if reg == "near":
            assert float(a[b].min()) >= 2.5e-3 and float(z.max()) <= 3.9
        elif reg in ("deep", "clamp"):
            assert float(z.min()) >= 32 and bool(((a[b] <= R.LOG_CLAMP) | (a[b] == 1.0)).all())
        elif reg == "edge":
            assert bool((a[b] <= R.LOG_CLAMP).all()) and bool((a[b] > 0).all()) and 4.7 < float(z.min()) and float(z.max()) < 4.95


def test_loss_threshold_elements_follow_the_fp32_comparison(diff):
    c, k8, d = _case64(diff, "n1020_B4_t0_first")
    Cc = c["x0"].shape[1]
    assert torch.equal(c["x0"][0].flatten()[5:11], R.loss_thresholds())
    _, _, g32 = R.loss_ref64_grad(d["out"], d["x0"], d["noise"], k8.double(), c["tzero"], d["g_mse"], d["g_vb"])            # fp32 constant
    _, _, g64 = R.loss_ref64_grad(d["out"], d["x0"], d["noise"], k8.double(), c["tzero"], d["g_mse"], d["g_vb"], thr=0.999)
    differ = torch.nonzero((g32 != g64).flatten()).flatten().tolist()
    base = c["x0"][0].numel()                                                        # the v half of sample 0 starts behind its C H W eps values
    assert differ == [base + 5, base + 8]                                            # float32(0.999) and float32(-0.999) only
    st = _statement(diff, c, torch.float32)[2]
    sel = slice(base + 5, base + 11)
    assert float(((st.flatten()[sel].double() - g32.flatten()[sel]) / g32.flatten()[sel]).abs().max()) < 1e-3
    assert float(((g64.flatten()[sel] - g32.flatten()[sel]) / g32.flatten()[sel]).abs().max()) > 0.05


def test_loss_bounds_pass_one_rounding_and_hold_the_fp32_statement(diff):
    worst = 0.0
    for name in R.LOSS_CASES:
        c, k8, d = _case64(diff, name)
        mse, vb, grad = R.loss_ref64_grad(d["out"], d["x0"], d["noise"], k8.double(), c["tzero"], d["g_mse"], d["g_vb"])
        T = R.loss_terms(d["out"], d["x0"], d["noise"], k8.double(), c["tzero"], d["g_mse"], d["g_vb"])
        for ref, e in ((grad, T["d"].e), (mse, T["mse"].e), (vb, T["vb"].e)):
            assert R.ratio(ref.float(), ref, e) <= 1.0                              # the fp64 result rounded once
        st = _statement(diff, c, torch.float32)
        for got, ref, e in ((st[2], grad, T["d"].e), (st[0], mse, T["mse"].e), (st[1], vb, T["vb"].e)):
            worst = max(worst, R.ratio(got, ref, e))
    assert 0.05 < worst < 1.0, worst            # the fp32 statement on the host: inside the running error bound, and not by orders of magnitude (0.58: the MSE half)


def test_loss_bounds_fail_planted_errors_and_dropped_addends(diff):
    c, k8, d = _case64(diff, "n16_B1_t0")
    Cc, n = c["x0"].shape[1], 16
    mse, vb, grad = R.loss_ref64_grad(d["out"], d["x0"], d["noise"], k8.double(), c["tzero"], d["g_mse"], d["g_vb"])
    T = R.loss_terms(d["out"], d["x0"], d["noise"], k8.double(), c["tzero"], d["g_mse"], d["g_vb"])
    c_stmt = 4 * R.ratio(_statement(diff, c, torch.float32)[2][:, :Cc], grad[:, :Cc], T["d"].e[:, :Cc])                      # what the GPU file would grant the MSE half
    bad = grad.clone()
    bad[0, 1, 0, 1] *= 1 + PLANT                                                      # MSE half: 2^-18 relative, one element
    assert R.ratio(bad, grad, T["d"].e) > max(c_stmt, 4.0)
    assert R.ratio(mse * (1 + PLANT), mse, T["mse"].e) > 1.0
    for idx in ((0, Cc, 0, 0), (0, Cc + 2, 1, 1)):                                    # NLL derivative: 4 x its own bound
        bad = grad.clone()
        bad[idx] += 4 * R.U * T["d"].e[idx] * (1 if grad[idx] >= 0 else -1)
        assert 3.9 < R.ratio(bad, grad, T["d"].e) < 4.1
        assert float(R.U * T["d"].e[idx] / grad[idx].abs()) < 2e-2                   # ... which is itself a small fraction of the element
    # dropped addends: one element of a sample's sum; the 1 of (1 + 3 a z^2) in the cdf's derivative is worth more than that
    e_mse = ((d["noise"] - d["out"][:, :Cc]) ** 2)[0].flatten()
    assert R.ratio((mse * n - e_mse[3]) / n, mse, T["mse"].e) > 100
    o2 = d["out"].clone()
    o2[0, 0, 0, 0] += 0.05                                                            # one wrong element of 16 (its eps moved by 0.05): the sample's sum sees it
    _, vb3, _ = R.loss_ref64_grad(o2, d["x0"], d["noise"], k8.double(), c["tzero"], d["g_mse"], d["g_vb"])
    assert R.ratio(vb3, vb, T["vb"].e) > 4.0


# ================================================================================================ CAME
SMALL = {"a.weight": (7, 4), "b.bias": (7,), "c.weight": (2, 3, 5), "d.weight": (33, 7), "e.weight": (6, 1284)}


def _came_run(wd, steps=3, keep64=True):
    from oracle.came_ref import CAMERef
    g = torch.Generator().manual_seed(1)
    host = {n: torch.randn(s, generator=g) * 0.05 for n, s in SMALL.items()}
    p64, p32 = [v.double().clone() for v in host.values()], [v.clone() for v in host.values()]
    o64, o32 = R.came_ref64(p64, lr=1e-3, weight_decay=wd), CAMERef(p32, lr=1e-3, weight_decay=wd)
    bounds = [R.CameBound(s, 262144, 1e-3, o64.betas, o64.eps, o64.clip, wd) for s in SMALL.values()]
    E = [None] * len(SMALL)
    for step in range(steps):
        grads = [torch.randn(s, generator=g) * 10.0 ** (i % 3 - 1) for i, s in enumerate(SMALL.values())]
        before, pb = [{k: v.clone() for k, v in st.items()} for st in o64.state], [p.clone() for p in p64]
        o64.step([x.double() for x in grads])
        o32.step(grads)
        for i in range(len(SMALL)):
            E[i] = bounds[i].update(grads[i].double(), before[i], o64.state[i], pb[i], p64[i])
    return o64, o32, p64, p32, E


@pytest.mark.parametrize("wd", [0.0, 0.03])
def test_came_fp64_wrapper_is_the_oracle_and_the_bounds_hold_it(wd):
    o64, o32, p64, p32, E = _came_run(wd)
    for i, n in enumerate(SMALL):
        assert all(v.dtype == torch.float64 for v in o64.state[i].values()) and p64[i].dtype == torch.float64
        assert set(o64.state[i]) == set(o32.state[i])
        for k, v in o64.state[i].items():
            if k != "exp_avg":                                                        # within fp32 noise: the issue's CPU run measured 1e-6 on the statistics
                assert float(((o32.state[i][k].double() - v) / v).abs().max()) < 1e-5, (n, k)
            ok, w = R.within(o32.state[i][k], v, E[i][k])                             # the fp32 oracle is inside the derived bounds ...
            assert ok, (n, k, w)
            ok, w = R.within(v.float(), v, E[i][k])                                   # ... and so is the fp64 result rounded once
            assert ok, (n, k, w)
        assert R.within(p32[i], p64[i], E[i]["p"])[0] and R.within(p64[i].float(), p64[i], E[i]["p"])[0]
    with pytest.raises(AssertionError):
        o64.step([torch.zeros(s) for s in SMALL.values()])                            # fp32 gradients are refused: the wrapper would silently fall back to fp32


def test_came_bounds_fail_planted_errors_and_dropped_addends():
    o64, _, p64, _, E = _came_run(0.0, steps=1)
    st, e = o64.state[0], E[0]                                                        # (7, 4): the smallest vector-path tensor
    for k in ("exp_avg_sq_row", "exp_avg_sq_col"):
        bad = st[k].clone()
        bad.flatten()[1] *= 1 + PLANT
        assert not R.within(bad, st[k], e[k])[0], k
    nf = o64.state[1]["exp_avg_sq"].clone()
    nf[2] *= 1 + PLANT
    assert not R.within(nf, o64.state[1]["exp_avg_sq"], E[1]["exp_avg_sq"])[0]
    bad = p64[0].clone()
    bad.flatten()[p64[0].abs().argmax()] *= 1 + PLANT
    assert not R.within(bad, p64[0], e["p"])[0]
    # a dropped addend: one column missing from a row mean (1 / C of it), one row from a column mean
    for k, cnt in (("exp_avg_sq_row", 4), ("exp_avg_res_row", 4), ("exp_avg_sq_col", 7), ("exp_avg_res_col", 7)):
        bad = st[k].clone()
        bad.flatten()[0] *= 1 - 0.02 / cnt                                            # the smallest addend a mean of cnt terms can lose is not this small
        assert not R.within(bad, st[k], e[k])[0], k
    bad = st["exp_avg"].clone()
    bad[0, 0] += 4 * e["exp_avg"][0, 0]
    assert not R.within(bad, st["exp_avg"], e["exp_avg"])[0]
    assert float((e["exp_avg"] / st["exp_avg"].abs()).median()) < 1e-5               # exp_avg after one step: a few 1e-6 relative
    assert all(R.came_chains(s, 262144)["path"] == p for s, p in (((9, 1280), "vec5"), ((6, 1284), "vec18"), ((5, 4608), "vec18"), ((3, 4612), "scalar"),
                                                                  ((33, 7), "scalar"), ((2, 3, 1280), "scalar"), ((7,), "1d")))
    ch = R.came_chains((2100, 64), 262144)
    assert ch["col"] == 525 + 4 + 1 and ch["row"] == 4 + 6 and R.came_chains((300, 1152), 262144)["col"] == 56 + 4 + 2


# ================================================================================================ conditioning linears
def test_condlin_bounds_pass_one_rounding_fail_planted_and_dropped():
    g = torch.Generator().manual_seed(2)
    # the smallest shapes, positive data (no cancellation: sum |a||b| is the value)
    x, w, b = torch.rand(1, 4, generator=g) + 0.5, torch.rand(1, 4, generator=g) + 0.5, torch.rand(1, generator=g) + 0.5
    y, mag = R.linear_ref64(x, w, b)
    bound = R.condlin_chain("fwd", 1, 1, 4) * R.U * mag
    assert R.within(y.float(), y, bound)[0]
    assert not R.within(y * (1 + PLANT), y, bound)[0]
    assert not R.within(y - x[0, 3].double() * w[0, 3].double(), y, bound)[0]         # a dropped product
    assert not R.within(y - b.double(), y, bound)[0]                                  # the dropped bias
    dy = torch.rand(1, 1, generator=g) + 0.5
    refs, mags = R.linear_bwd_ref64(dy, x, w)
    for kind, ref, mg in zip(("dx", "dw", "db"), refs, mags):
        bound = R.condlin_chain(kind, 1, 1, 4) * R.U * mg
        assert R.within(ref.float(), ref, bound)[0], kind
        bad = ref.clone()
        bad.flatten()[0] *= 1 + PLANT
        assert not R.within(bad, ref, bound)[0], kind
    # a dropped addend where there is more than one: a slice of dX that stops 1 short, a row of dW
    x, w, dy = torch.rand(3, 8, generator=g) + 0.5, torch.rand(129, 8, generator=g) + 0.5, torch.rand(3, 129, generator=g) + 0.5
    refs, mags = R.linear_bwd_ref64(dy, x, w)
    short = dy[:, :128].double() @ w[:128].double()
    assert not R.within(short, refs[0], R.condlin_chain("dx", 3, 129, 8) * R.U * mags[0])[0]
    assert R.within(refs[0].float(), refs[0], R.condlin_chain("dx", 3, 129, 8) * R.U * mags[0])[0]
    assert not R.within(dy[:2].double().t() @ x[:2].double(), refs[1], R.condlin_chain("dw", 3, 129, 8) * R.U * mags[1])[0]
    assert not R.within(dy[:2].double().sum(0), refs[2], R.condlin_chain("db", 3, 129, 8) * R.U * mags[2])[0]
    assert [R.condlin_chain("fwd", 1, 1, k) for k in (4, 256, 260, 1028)] == [11, 11, 12, 15]
    assert [R.condlin_chain("dx", 1, n, 4) for n in (1, 128, 129, 300)] == [3, 130, 131, 132]
