"""The fused CAME step (csrc/came.hip through dp.FusedCAME) against oracle/came_ref.py run in fp64 (train_tail_refs.came_ref64), every state of every tensor per
element after every one of 4 steps: exp_avg, the four factored statistics through opt.layout, the 1-D second moment, the parameters; the 16-bit shadow is the
parameters cast to the operand type, bit for bit; column-state padding and the gaps between tensors stay 0.  Runs under either operand build (the shadow's
type differs; tests/test_f16_parity_gpu.py re-runs the file under f16).

Tensors: the first and last width of each of the kernel's three paths - C = 1280 | 1284 (MAXJ = 5 | 18) and C = 4608 | 4612 (MAXJ = 18 | scalar) - each between
small neighbours in the flat store, C = 4, R = 1, C % 4 != 0, batched tensors (narrow, wide, one whose batch . C is no multiple of 4: column-state padding),
2100 rows of 64 in one tile (525 rows per wave), two tiles of one matrix, 1-D tensors of 7, 1030 and TILE_ELEMS + 5 elements, a matrix and a vector that never
receive a gradient, and a matrix whose every 5th row and 7th column receive none (eps0 = 1e-30 alone keeps those rsqrt finite).

Bounds (train_tail_refs.CameBound, propagated per element next to the oracle; U = 2^-24).  The statistics are sums of non-negative terms, so whatever the order
of the atomics their error is (additions on the longest chain) U relative; the chains, from the kernel (train_tail_refs.came_chains):
    row mean     vector paths 4 ceil(C / 256) serial additions in a lane + 6 (wave_sum);  scalar path ceil(C / 64) + 6
    column mean  vector paths ceil(rows of the tile / 4) serial in a lane + 4 (LDS atomics) + tiles;  scalar path R (one global atomic per row)
    mean_r(row)  ceil(rows of the tile / 4) + 8 (block_sum) + tiles;  batched R
    sum u^2      (rows per wave) x (addends per lane and row) + 8 + tiles;  1-D ceil(tile / 256) + 8 + tiles
plus 4 roundings in an addend g^2 + eps0 (g = grad x clip coefficient), 1 for the division and 3 for the exponential average, whose previous error decays with
beta.  exp_avg: the relative errors of the two rsqrt factors (half the statistics' + 2 for the rsqrt), of the clip factor (half of sum u^2's + 3) and 4 products on
|u|, averaged with beta1, + 3 roundings.  The residual statistics are sums of (u - m)^2 + eps1: each addend carries 2 |u - m| (err u + err m).  Parameters: lr x (the
update's error) + half an ulp of p per step (three halves with weight decay: p (1 - lr wd) rounds, and 1 - lr wd is itself held in fp32).
The fp32 oracle is measured against the fp64 one in the same form: it must stay inside the derived bounds as well (it is printed next to the kernel), and no
relative bound on a statistic or on an update exceeds the 1e-4 tests/test_came_gpu.py grants: where a chain is long (2100 rows of 64: sum u^2 has 2100 serial
additions in a lane; the derived figures there reach 3.7e-4 on the residual statistics after 4 steps) the bound is capped at 1e-4.

Measured (MI355X), worst value over bound across tensors, the 4 steps, both parametrisations and both operand builds:
                      kernel   resumed optimizer   fp32 oracle (host)
    exp_avg           0.095    0.102               0.139
    exp_avg_sq_row    0.28     0.26                0.28
    exp_avg_sq_col    0.49     0.46                0.45
    exp_avg_res_row   0.041    0.037               0.059
    exp_avg_res_col   0.051    0.040               0.059
    exp_avg_sq (1-D)  0.74     0.72                0.65
    p                 0.976    0.78                0.976
The first form of the parameter bound (one ulp with weight decay) was too small for the kernel - 1.15 on a 1-D tensor: the kernel multiplies by fl32(1 - lr wd),
the oracle adds p (-lr wd); the third half-ulp above is that constant's rounding, derived, not fitted."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import record_parity  # noqa: E402
import train_tail_refs as R  # noqa: E402

LR = 1e-3
STEPS = 4
STATES = ("exp_avg", "exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_res_row", "exp_avg_res_col", "exp_avg_sq", "p")
ZERO_GRAD = ("zero.weight", "tail.bias")


def _shapes(tile_elems):
    return {"s0.bias": (7,), "w1280.weight": (9, 1280), "s1.weight": (7, 4), "w1284.weight": (6, 1284), "s2.weight": (1, 8), "w4608.weight": (5, 4608),
            "s3.weight": (33, 7), "w4612.weight": (3, 4612), "b4.weight": (3, 5, 8, 12), "bw.weight": (2, 3, 1280), "b5.weight": (5, 3, 7, 9),
            "tall.weight": (2100, 64), "v1030.bias": (1030,), "two.weight": (300, 1152), "zero.weight": (12, 20), "long.bias": (tile_elems + 5,),
            "holes.weight": (35, 28), "s4.weight": (1, 8), "tail.bias": (7,)}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _make(shapes, seed=0):
    from pixart_sigma_amd.dp import FusedCAME  # noqa: F401
    from pixart_sigma_amd.engine import ParamStore
    g = torch.Generator().manual_seed(seed)
    host = {n: torch.randn(s, generator=g) * 0.05 for n, s in shapes.items()}
    params = [(n, torch.nn.Parameter(v.clone().cuda())) for n, v in host.items()]
    store = ParamStore(params, torch.device("cuda"))
    return host, params, store


def _opt(store, wd, max_norm):
    from pixart_sigma_amd.dp import FusedCAME
    model = SimpleNamespace(_store=store, _engine=SimpleNamespace(grad_ready_hook=None))
    return FusedCAME(model, lr=LR, weight_decay=wd, max_grad_norm=max_norm)


def _grads(shapes, step):
    g = torch.Generator().manual_seed(100 + step)
    out = {}
    for i, (n, s) in enumerate(shapes.items()):
        gr = torch.randn(s, generator=g) * (10.0 ** (i % 3 - 1))
        if n in ZERO_GRAD:
            gr.zero_()
        if n == "holes.weight":
            gr[::5, :] = 0
            gr[:, ::7] = 0
        out[n] = gr
    return out


def _kernel_states(opt, store, name, shape):
    """The kernel's states of one tensor in the oracle's names and shapes (host copies)."""
    lay = opt.layout[name]
    st = {"exp_avg": store.view(opt.m, name).cpu()}
    if lay["factored"]:
        (ro, rn), (co, cn) = lay["row"], lay["col"]
        st["exp_avg_sq_row"], st["exp_avg_res_row"] = opt.sq_row[ro:ro + rn].view(shape[:-1]).cpu(), opt.res_row[ro:ro + rn].view(shape[:-1]).cpu()
        st["exp_avg_sq_col"] = opt.sq_col[co:co + cn].view(shape[:-2] + shape[-1:]).cpu()
        st["exp_avg_res_col"] = opt.res_col[co:co + cn].view(shape[:-2] + shape[-1:]).cpu()
    else:
        o, n = lay["nf"]
        st["exp_avg_sq"] = opt.nf_sq[o:o + n].view(shape).cpu()
    return st


def _outside_is_zero(opt, store, shapes):
    """Column-state padding, and the alignment gaps of the flat store, hold exactly 0."""
    cmask = torch.ones(opt.sq_col.numel(), dtype=torch.bool)
    fmask = torch.ones(store.total, dtype=torch.bool)
    for n in shapes:
        lay = opt.layout[n]
        if lay["factored"]:
            cmask[lay["col"][0]:lay["col"][0] + lay["col"][1]] = False
        fmask[store.offset[n]:store.offset[n] + store.numel[n]] = False
    assert int(cmask.sum()) > 0 and int(fmask.sum()) > 0                               # there IS padding to watch
    for t in (opt.sq_col, opt.res_col):
        assert bool((t.cpu()[cmask] == 0).all()), "column-state padding was written"
    for t in (opt.m, store.master, store.shadow.float()):
        assert bool((t.cpu()[fmask] == 0).all()), "written between two tensors of the flat store"


class _Oracles:
    """The fp64 oracle, the fp32 oracle and the bound propagation, stepped together."""

    def __init__(self, host, tile_elems, wd):
        self.names = list(host)
        self.p64 = [host[n].double().clone() for n in self.names]
        self.p32 = [host[n].clone() for n in self.names]
        self.o64 = R.came_ref64(self.p64, lr=LR, weight_decay=wd)
        from oracle.came_ref import CAMERef
        self.o32 = CAMERef(self.p32, lr=LR, weight_decay=wd)
        self.bounds = [R.CameBound(host[n].shape, tile_elems, LR, self.o64.betas, self.o64.eps, self.o64.clip, wd) for n in self.names]
        self.E = [None] * len(self.names)

    def step(self, grads, coef):
        """grads: name -> fp32 host gradient; coef: the kernel's own fp32 clip coefficient (so that its rounding is not counted against the states)."""
        before = [{k: v.clone() for k, v in st.items()} for st in self.o64.state]
        p_before = [p.clone() for p in self.p64]
        g64 = [grads[n].double() * float(coef) for n in self.names]
        self.o64.step(g64)
        self.o32.step([grads[n] * coef for n in self.names])
        for i in range(len(self.names)):
            self.E[i] = self.bounds[i].update(g64[i], before[i], self.o64.state[i], p_before[i], self.p64[i])


def _compare(tag, worst, name, got, got_p, orc, i, coef_slack=0.0):
    """One tensor against the fp64 oracle within its bounds; returns the failures.  coef_slack: relative difference between this optimizer's clip coefficient and
    the one the oracle was given (the resumed optimizer's own sum of squares: float atomics) - the second moments scale with its square, the updates not at all."""
    fails = []
    E, ref = orc.E[i], orc.o64.state[i]
    for k in list(ref) + ["p"]:
        r = orc.p64[i] if k == "p" else ref[k]
        g = got_p if k == "p" else got[k]
        bound = E[k] + (2.5 * coef_slack * r.abs() if k.startswith("exp_avg_sq") else 0)
        ok, w = R.within(g, r, bound)
        worst[(tag, k)] = max(worst.get((tag, k), 0.0), w)
        if not ok:
            fails.append((tag, name, k, w))
    return fails


@pytest.mark.parametrize("wd,max_norm", [(0.0, 0.01), (0.03, 0.0)])
def test_every_state_per_element_and_resume(wd, max_norm):
    from pixart_sigma_amd import lib
    from pixart_sigma_amd.dp import FusedCAME
    OPD = lib.OPERAND_DTYPE
    tile = FusedCAME.TILE_ELEMS
    shapes = _shapes(tile)
    assert [R.came_path(shapes[n]) for n in ("w1280.weight", "w1284.weight", "w4608.weight", "w4612.weight", "bw.weight", "s3.weight")] == \
        ["vec5", "vec18", "vec18", "scalar", "scalar", "scalar"]
    host, params, store = _make(shapes)
    opt = _opt(store, wd, max_norm)
    assert sum(1 for t in opt.layout.values() if t["factored"] and t["col"][1] % 4) >= 2          # (33, 7) and (5, 3, 7, 9) leave padding behind them
    orc = _Oracles(host, tile, wd)
    names = list(shapes)
    worst, fails = {}, []
    opt2 = store2 = params2 = None
    for step in range(STEPS):
        grads = _grads(shapes, step)
        for o, ps in ((opt, params),) + (((opt2, params2),) if opt2 is not None else ()):
            o.zero_grad()
            for n, p in ps:
                p.grad.copy_(grads[n].cuda())
        before = {n: p.detach().clone() for n, p in params}
        opt.step()
        if opt2 is not None:
            opt2.step()
        torch.cuda.synchronize()
        total = torch.sqrt(sum((x.double() ** 2).sum() for x in grads.values()))
        coef = opt.coef[0].cpu()
        want = min(1.0, max_norm / (float(total) + 1e-6)) if max_norm else 1.0
        assert abs(float(opt.last_norm) / float(total) - 1) < 1e-5 and abs(float(coef) / want - 1) < 1e-5
        orc.step(grads, coef)
        for i, (n, p) in enumerate(params):
            fails += _compare("kernel", worst, n, _kernel_states(opt, store, n, shapes[n]), p.detach().cpu(), orc, i)
            fails += _compare("fp32 oracle", worst, n, orc.o32.state[i], orc.p32[i], orc, i)
            if opt2 is not None:
                slack = abs(float(opt2.coef[0]) / float(coef) - 1)
                assert slack <= 1e-6
                fails += _compare("resumed", worst, n, _kernel_states(opt2, store2, n, shapes[n]), dict(params2)[n].detach().cpu(), orc, i, slack)
            rel = orc.bounds[i].worst_relative({k: v for k, v in orc.o64.state[i].items()})
            assert rel <= 1e-4 * (1 + 1e-9), (n, rel)
            if n in ZERO_GRAD:                                                         # no gradient: only the decay moves p, exactly; m stays 0
                decay = torch.tensor(1.0 - LR * wd, dtype=torch.float64).float().cuda()
                assert torch.equal(p.detach(), before[n] * decay), n
                assert bool((store.view(opt.m, n) == 0).all()), n
        for o, s in ((opt, store),) + (((opt2, store2),) if opt2 is not None else ()):
            for t in (o.m, o.sq_row, o.sq_col, o.res_row, o.res_col, o.nf_sq, s.master):
                assert bool(torch.isfinite(t).all())
            assert torch.equal(s.shadow.view(torch.int16), s.master.to(OPD).view(torch.int16)), "the 16-bit shadow is not the parameters cast once"
            _outside_is_zero(o, s, shapes)
        if step == 1:                                                                  # resume: a second optimizer over a cloned store takes the state and goes on
            sd = opt.state_dict()
            _, params2, store2 = _make(shapes)
            store2.master.copy_(store.master)
            store2.shadow.copy_(store.shadow)
            opt2 = _opt(store2, wd, max_norm)
            opt2.load_state_dict({k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()})
            assert opt2.t == 2
            for k in ("m", "sq_row", "sq_col", "res_row", "res_col", "nf_sq"):
                assert torch.equal(getattr(opt2, k), getattr(opt, k)) and getattr(opt2, k).data_ptr() != getattr(opt, k).data_ptr()
    for (tag, k), w in sorted(worst.items()):
        print(f"\n[came wd={wd} clip={max_norm}] {tag}: {k} worst value / bound {w:.3g}")
        record_parity(f"came {tag} wd={wd} max_grad_norm={max_norm}: {k}, worst element / bound over {STEPS} steps", w, 1.0)
    assert not fails, fails[:20]
    assert all(("kernel", k) in worst and ("resumed", k) in worst for k in STATES)      # every state was compared


def test_load_state_dict_refuses_another_layout():
    shapes = {"a.weight": (8, 12), "a.bias": (12,)}
    _, _, s1 = _make(shapes)
    o1 = _opt(s1, 0.0, 0.0)
    other = {"a.bias": (12,), "a.weight": (8, 12)}                                      # same tensors, another order: other offsets
    _, _, s2 = _make(other)
    o2 = _opt(s2, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="layout"):
        o2.load_state_dict(o1.state_dict())
    _, _, s3 = _make({"a.weight": (8, 16), "a.bias": (12,)})
    with pytest.raises(RuntimeError, match="layout"):
        _opt(s3, 0.0, 0.0).load_state_dict(o1.state_dict())
    o1.load_state_dict(_opt(_make(shapes)[2], 0.0, 0.0).state_dict())                 # the same layout loads
