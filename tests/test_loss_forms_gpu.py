"""The fused IDDPM objective (csrc/loss.hip: pxa_iddpm_loss_fwd / _bwd) called directly, per element and per branch, against the fp64 evaluation of the formula
of pixart_sigma_amd/diffusion/iddpm.py:125-137 (tests/train_tail_refs.py: loss_ref64, derivatives by fp64 autograd, the fp32 coefficient rows cast to double).

Cases (train_tail_refs.LOSS_CASES): n = C H W of 16, 1020, 1024, 1028, 2560 and 4608 (5 blocks), B of 1, 4 and 5, t = 0 at the first sample, at the last, twice in
a batch, t of 1, 2, 500, 998, 999, weights g_mse / g_vb that differ per sample and include a zero.  The t = 0 samples are built in four regimes:
  near   eps = noise + 0.7 randn, x0 uniform in [-1.2, 1.2] with float32(+-0.999) and both fp32 neighbours planted: every log argument >= 2.5e-3, |z| <= 3.9
  deep   eps = noise +- 40, both signs in each x0 range: |z| >= 33, every cdf exactly 0 or 1 in fp32 and fp64 - the 1e-12 clamp or log 1
  clamp  deep, x0 between the thresholds: every element sits on the clamp (n a power of two: the sample's vb is then predictable to the bit)
  edge   cdf_plus - cdf_min = 2e-13 ... 5e-13 in fp64 (under the clamp) while 1 - |tanh| is 4 ... 6 fp32 spacings and z+ and z- differ by fp32 spacings: the fp32
         difference is exactly 0, the two halves of the derivative's numerator are not equal - only the `> 1e-12` guard makes the derivative 0
and the test asserts that no log argument of its inputs lies in the band (1e-12, 1e-3) in between, where fp32 cancellation in cdf_plus - cdf_min decides.
Elements of the deep / clamp / edge samples are asserted exactly: derivative 0, and - for a sample wholly on the clamp - vb = fl(-logf(1e-12f) / ln 2) to the bit.

Everything else is held to an element-wise bound of the form  c . 2^-24 . (running sum of |terms| as the formula adds them, + |argument| per exp)
(train_tail_refs.loss_terms: every operation of the formula carries its operands' error bounds and adds one rounding of its result; a sample's sum adds its depth).
c is not fixed in advance: the fp32 torch statement (the PXA_FUSED_LOSS=0 path of training_losses, on the GPU) is measured against the same fp64 reference in the
same form, per class of output - MSE half of d_model_out, KL, the three NLL branches, and the per-sample mse and vb - and the kernel gets 4 x the statement's worst
ratio of its class (it uses __expf, and the compiler may contract multiply-adds torch performs apart).  The last step of the form follows autograd:
d lv / d v is formed as two products with max_lv and true_lv that cancel (the kernel subtracts first, which is exact), so at t >= 500 the form is loose by
(|max_lv| + |true_lv|) / (max_lv - true_lv) - the statement itself is no sharper there.

Measured (MI355X, worst over the cases; ratio = error / (2^-24 . form)):   statement   kernel    c = 4 x statement
  d_model_out, MSE half                                                     0.576       0.576     2.30
  d_model_out, KL samples                                                   0.0168      0.0187    0.0674
  d_model_out, NLL x0 < -0.999                                              0.0146      0.0087    0.0582
  d_model_out, NLL x0 > 0.999                                               0.0126      0.0081    0.0505
  d_model_out, NLL between                                                  0.0057      0.0030    0.0230
  mse per sample                                                            0.0727      0.0754    0.291
  vb per sample                                                             0.0624      0.0673    0.250
(the statement on the host measures the same 0.576 / 0.0168 / 0.0146 / 0.0126 / 0.0057: tests/test_train_tail_host.py).  The kernel sits at or below the
statement's own error in every class, i.e. at a quarter of what it is granted.
"""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import record_parity  # noqa: E402
import train_tail_refs as R  # noqa: E402

FACTOR = 4.0
CLASSES = ("d mse half", "d kl", "d nll x0<-0.999", "d nll x0>0.999", "d nll between", "mse", "vb")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _diff():
    from pixart_sigma_amd import IDDPM
    return IDDPM("1000", learn_sigma=True, pred_sigma=True, snr=False)


def _class_masks(T, regimes, C_):
    """class -> boolean mask over d (B, 2C, H, W), leaving out the samples asserted exactly."""
    br = T["branch"]
    exact = torch.zeros_like(br, dtype=torch.bool)
    for b, reg in enumerate(regimes):
        if reg in ("deep", "clamp", "edge"):
            exact[b] = True
    none = torch.zeros_like(exact)
    half = lambda m: torch.cat([none, m & ~exact], 1)                                   # noqa: E731
    return {"d mse half": torch.cat([torch.ones_like(exact), none], 1), "d kl": half(br == 0), "d nll x0<-0.999": half(br == 1),
            "d nll x0>0.999": half(br == 2), "d nll between": half(br == 3)}, exact


@pytest.fixture(scope="module")
def world():
    """Per case: inputs, fp64 reference, bound form; and over all cases the torch statement's worst ratio per class (made once, shared, left unchanged)."""
    diff = _diff()
    tab = diff._tab(torch.device("cpu"))
    edge_lv = (float(tab["post_logvar"][0].float()), float(tab["log_betas"][0].float()))
    cases, ref_ratio = {}, {k: 0.0 for k in CLASSES}
    old = os.environ.get("PXA_FUSED_LOSS")
    os.environ["PXA_FUSED_LOSS"] = "0"
    try:
        for name in R.LOSS_CASES:
            c = R.loss_case(name, edge_lv)
            k8 = R.loss_coef8(diff, c["t"])
            d64 = {k: c[k].double() for k in ("out", "x0", "noise", "g_mse", "g_vb")}
            mse, vb, grad = R.loss_ref64_grad(d64["out"], d64["x0"], d64["noise"], k8.double(), c["tzero"], d64["g_mse"], d64["g_vb"])
            T = R.loss_terms(d64["out"], d64["x0"], d64["noise"], k8.double(), c["tzero"], d64["g_mse"], d64["g_vb"])
            assert float((T["d"].v - grad).abs().max()) <= 1e-12 * float(grad.abs().max()), "the analytic derivative of the bound form is not autograd's"
            a = T["arg"]
            assert not bool(((a > R.BAND[0]) & (a < R.BAND[1])).any()), f"{name}: a log argument lies in the band the test leaves out"
            masks, exact = _class_masks(T, c["regimes"], c["x0"].shape[1])
            # the fp32 torch statement on the GPU
            out = c["out"].cuda().requires_grad_(True)
            terms = diff.training_losses(lambda x, timestep, **kw: out, c["x0"].cuda(), c["t"].cuda(), noise=c["noise"].cuda())
            (terms["mse"] * c["g_mse"].cuda() + terms["vb"] * c["g_vb"].cuda()).sum().backward()
            sg = out.grad.cpu()
            for k, m in masks.items():
                if bool(m.any()):
                    ref_ratio[k] = max(ref_ratio[k], R.ratio(sg[m], grad[m], T["d"].e[m]))
            ref_ratio["mse"] = max(ref_ratio["mse"], R.ratio(terms["mse"].detach().cpu(), mse, T["mse"].e))
            ref_ratio["vb"] = max(ref_ratio["vb"], R.ratio(terms["vb"].detach().cpu(), vb, T["vb"].e))
            cases[name] = dict(c=c, k8=k8, mse=mse, vb=vb, grad=grad, T=T, masks=masks, exact=exact, stmt=(terms["mse"].detach().cpu(), terms["vb"].detach().cpu(), sg))
    finally:
        if old is None:
            del os.environ["PXA_FUSED_LOSS"]
        else:
            os.environ["PXA_FUSED_LOSS"] = old
    for k, v in ref_ratio.items():
        assert 0 < v < 1.0, f"the fp32 statement is at {v} of the running error bound in class {k}: the bound form is wrong"
    print("\n[loss] fp32 torch statement, worst error / (2^-24 x form) per class: " + ", ".join(f"{k} {v:.3g}" for k, v in ref_ratio.items()))
    return dict(cases=cases, ref_ratio=ref_ratio, kernel_ratio={k: 0.0 for k in CLASSES})


def _run_kernel(w, name):
    from pixart_sigma_amd import ops
    cs = w["cases"][name]
    c = cs["c"]
    dev = {k: c[k].cuda().contiguous() for k in ("out", "x0", "noise", "g_mse", "g_vb")}
    k8, tz = cs["k8"].cuda(), c["tzero"].to(torch.int32).cuda()
    mse, vb = ops.iddpm_loss_fwd(dev["out"], dev["x0"], dev["noise"], k8, tz)
    d = ops.iddpm_loss_bwd(dev["out"], dev["x0"], dev["noise"], k8, tz, dev["g_mse"], dev["g_vb"])
    torch.cuda.synchronize()
    return mse.cpu(), vb.cpu(), d.cpu()


@pytest.mark.parametrize("name", list(R.LOSS_CASES))
def test_every_element_per_branch_against_fp64(world, name):
    cs = world["cases"][name]
    c, T, grad = cs["c"], cs["T"], cs["grad"]
    mse, vb, d = _run_kernel(world, name)
    assert torch.isfinite(d).all() and torch.isfinite(mse).all() and torch.isfinite(vb).all()
    fails = []
    for k, m in cs["masks"].items():
        if not bool(m.any()):
            continue
        cc = FACTOR * world["ref_ratio"][k]
        r = R.ratio(d[m], grad[m], T["d"].e[m])
        world["kernel_ratio"][k] = max(world["kernel_ratio"][k], r)
        print(f"\n[{name}] {k}: kernel {r:.3g}, statement {world['ref_ratio'][k]:.3g}, c = {cc:.3g} (units of 2^-24 x form)")
        record_parity(f"iddpm loss {name}: {k}, error / (2^-24 x form)", r, cc)
        zero = (T["d"].e[m] == 0)
        if bool(zero.any()) and bool((d[m][zero] != 0).any()):
            fails.append((k, "an element with a zero weight is not zero"))
        if r > cc:
            fails.append((k, r, cc))
    for k, got, ref, e in (("mse", mse, cs["mse"], T["mse"].e), ("vb", vb, cs["vb"], T["vb"].e)):
        cc = FACTOR * world["ref_ratio"][k]
        for b in range(len(got)):                                                     # per sample: the KL samples do not carry the NLL ones
            r = R.ratio(got[b:b + 1], ref[b:b + 1], e[b:b + 1])
            world["kernel_ratio"][k] = max(world["kernel_ratio"][k], r)
            if r > cc:
                fails.append((k, b, c["regimes"][b], r, cc))
        r = R.ratio(got, ref, e)
        print(f"[{name}] {k} per sample: kernel {r:.3g}, statement {world['ref_ratio'][k]:.3g}, c = {cc:.3g}")
        record_parity(f"iddpm loss {name}: {k} per sample, error / (2^-24 x form)", r, cc)
    assert not fails, fails


@pytest.mark.parametrize("name", [n for n, v in R.LOSS_CASES.items() if set(v[4]) & {"deep", "clamp", "edge"}])
def test_clamp_and_log_one_elements_bit_for_bit(world, name):
    """deep / clamp / edge samples: the derivative with respect to v is exactly 0 at every element (the clamp's derivative is 0; log 1 has value and derivative 0),
    the fp64 reference agrees, and a sample wholly on the clamp has vb = fl(-logf(1e-12f) . fl(1 / ln 2)) to the bit."""
    cs = world["cases"][name]
    c = cs["c"]
    Cc = c["x0"].shape[1]
    mse, vb, d = _run_kernel(world, name)
    L = -torch.log(torch.tensor(1e-12, dtype=torch.float32, device="cuda"))
    want_vb = (L * torch.tensor(1.4426950408889634, dtype=torch.float32, device="cuda")).cpu()
    for b, reg in enumerate(c["regimes"]):
        if reg not in ("deep", "clamp", "edge"):
            continue
        arg = cs["T"]["arg"][b]
        assert bool(((arg <= R.LOG_CLAMP) | (arg == 1.0)).all())
        assert bool((cs["grad"][b, Cc:] == 0).all())
        dv = d[b, Cc:]
        assert bool((dv == 0).all()), f"sample {b} ({reg}): {int((dv != 0).sum())} derivative(s) not 0, largest {float(dv.abs().max()):.3e}"
        assert bool((cs["stmt"][2][b, Cc:] == 0).all())                                # the torch statement says the same
        if reg == "deep":
            assert bool((arg <= R.LOG_CLAMP).any()) and bool((arg == 1.0).any())       # both kinds are there
        else:
            n = arg.numel()
            assert n & (n - 1) == 0 and bool((arg <= R.LOG_CLAMP).all())
            assert vb[b].view(torch.int32).item() == want_vb.view(torch.int32).item(), (float(vb[b]), float(want_vb))
            assert abs(float(cs["vb"][b]) - 12 * 2.302585092994046 / 0.6931471805599453) < 1e-9


def test_threshold_elements_take_the_fp32_comparisons_branch(world):
    """x0 = float32(+-0.999) and its fp32 neighbours: the branch of `x0 < -0.999f` / `x0 > 0.999f`; a neighbouring branch's derivative is far outside the bound."""
    cs = world["cases"]["n1020_B4_t0_first"]
    c, T = cs["c"], cs["T"]
    Cc = c["x0"].shape[1]
    thr = R.loss_thresholds()
    x = c["x0"][0].flatten()
    assert torch.equal(x[5:11], thr)
    br = T["branch"][0].flatten()[5:11].tolist()
    assert br == [3, 2, 3, 3, 1, 3]                                                      # 0.999f itself is NOT above 0.999f; its upper neighbour is
    _, _, d = _run_kernel(world, "n1020_B4_t0_first")
    got, ref, e = d[0, Cc:].flatten()[5:11], cs["grad"][0, Cc:].flatten()[5:11], T["d"].e[0, Cc:].flatten()[5:11]
    for i in range(6):
        k = CLASSES[1 + br[i]]
        cc = FACTOR * world["ref_ratio"][k]
        r = R.ratio(got[i:i + 1], ref[i:i + 1], e[i:i + 1])
        record_parity(f"iddpm loss threshold element {i} ({k})", r, cc)
        assert r <= cc, (i, float(x[5 + i]), k, r, cc)
    # the other reading of the comparison (a double 0.999, or <= for <) gives another value by far more than the bound: the check above can tell them apart
    d64 = {k: c[k].double() for k in ("out", "x0", "noise", "g_mse", "g_vb")}
    _, _, other = R.loss_ref64_grad(d64["out"], d64["x0"], d64["noise"], cs["k8"].double(), c["tzero"], d64["g_mse"], d64["g_vb"], thr=0.999)
    o = other[0, Cc:].flatten()[5:11]
    for i in (0, 3):                                                                   # float32(0.999) and float32(-0.999)
        assert float((o[i] - ref[i]).abs()) > 100 * FACTOR * world["ref_ratio"]["d nll between"] * R.U * float(e[i])


def test_kernel_ratios_are_recorded(world):
    """(runs last in the file) the worst ratios of the run, per class, next to the statement's."""
    for k in CLASSES:
        print(f"\n[loss] {k}: statement {world['ref_ratio'][k]:.3g}  kernel {world['kernel_ratio'][k]:.3g}  c {FACTOR * world['ref_ratio'][k]:.3g}")
        record_parity(f"iddpm loss, all cases: {k}, kernel ratio over c", world["kernel_ratio"][k], FACTOR * world["ref_ratio"][k])
        record_parity(f"iddpm loss, all cases: {k}, fp32 torch statement's ratio (of the running error bound)", world["ref_ratio"][k], 1.0)
        assert world["kernel_ratio"][k] <= FACTOR * world["ref_ratio"][k]


# ---------------------------------------------------------------------------------------------- refusals, repeat calls
def _direct(fwd, case, mse=None, vb=None, dout=None, hw=None, null=None):
    from pixart_sigma_amd import lib
    L = lib.load()
    c = case["c"]
    B, Cc, H, W = c["x0"].shape
    t = dict(out=c["out"].cuda().contiguous(), x0=c["x0"].cuda().contiguous(), noise=c["noise"].cuda().contiguous(), k8=case["k8"].cuda(),
             tz=c["tzero"].to(torch.int32).cuda(), g_mse=c["g_mse"].cuda(), g_vb=c["g_vb"].cuda())
    p = lambda n, x=None: None if null == n else C.c_void_p((t[n] if x is None else x).data_ptr())    # noqa: E731
    hw = H * W if hw is None else hw
    if fwd:
        return L.pxa_iddpm_loss_fwd(p("out"), p("x0"), p("noise"), p("k8"), p("tz"), B, Cc, hw, p("mse", mse), p("vb", vb), lib.stream())
    return L.pxa_iddpm_loss_bwd(p("out"), p("x0"), p("noise"), p("k8"), p("tz"), B, Cc, hw, p("g_mse"), p("g_vb"), p("d", dout), lib.stream())


def test_refusals_launch_nothing(world):
    from pixart_sigma_amd import lib, ops
    cs = world["cases"]["n1028_B4_deep_last"]
    B = 4
    mse, vb = torch.full((B,), 7.0, device="cuda"), torch.full((B,), 7.0, device="cuda")
    dout = torch.full_like(cs["c"]["out"], 7.0).cuda()
    for fwd in (True, False):
        assert _direct(fwd, cs, mse, vb, dout, hw=1027) != 0                           # H W not a multiple of 4 (and C H W would then pass the end of the buffers)
        assert b"pxa_iddpm_loss" in lib.load().pxa_last_error()
        assert _direct(fwd, cs, mse, vb, dout, hw=0) != 0
        for null in ("out", "x0", "noise", "k8", "tz") + (("mse", "vb") if fwd else ("g_mse", "g_vb", "d")):
            assert _direct(fwd, cs, mse, vb, dout, null=null) != 0, null
    torch.cuda.synchronize()
    assert bool((mse == 7.0).all()) and bool((vb == 7.0).all()) and bool((dout == 7.0).all())      # nothing was launched, not even the memsets
    x = torch.zeros(1, 4, 1, 2, device="cuda")
    with pytest.raises(lib.PixartHipError):
        ops.iddpm_loss_fwd(torch.zeros(1, 8, 1, 2, device="cuda"), x, x, torch.zeros(1, 8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))
    with pytest.raises(lib.PixartHipError):
        ops.iddpm_loss_bwd(torch.zeros(1, 8, 1, 2, device="cuda"), x, x, torch.zeros(1, 8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
                           torch.ones(1, device="cuda"), torch.ones(1, device="cuda"))


@pytest.mark.parametrize("name", ["n1020_B4_t0_first", "n4608_B5_five_blocks"])
def test_two_forward_calls_into_the_same_buffers(world, name):
    """The per-sample sums are atomics into mse / vb: the memset in front of them belongs to the call.  One block per sample: the same bits; five blocks: the
    atomics may arrive in another order - the same values within the sum's bound, and never twice the value."""
    cs = world["cases"][name]
    B = len(cs["c"]["t"])
    mse, vb = torch.full((B,), 1e6, device="cuda"), torch.full((B,), -1e6, device="cuda")
    assert _direct(True, cs, mse, vb) == 0
    torch.cuda.synchronize()
    first = mse.clone(), vb.clone()
    assert _direct(True, cs, mse, vb) == 0
    torch.cuda.synchronize()
    for got, one, ref, e, k in ((mse, first[0], cs["mse"], cs["T"]["mse"].e, "mse"), (vb, first[1], cs["vb"], cs["T"]["vb"].e, "vb")):
        if cs["c"]["x0"][0].numel() <= 1024:
            assert torch.equal(got.view(torch.int32), one.view(torch.int32))
        assert R.ratio(got.cpu(), ref, e) <= FACTOR * world["ref_ratio"][k] and R.ratio(one.cpu(), ref, e) <= FACTOR * world["ref_ratio"][k]
