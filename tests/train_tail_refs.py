"""fp64 references and element-wise error bounds of the training step's tail: the fused IDDPM objective (csrc/loss.hip), the CAME step (csrc/came.hip) and
the fp32 conditioning linears (csrc/condlin.hip).  Shared by tests/test_loss_forms_gpu.py, tests/test_came_forms_gpu.py, tests/test_condlin_forms_gpu.py;
tests/test_train_tail_host.py checks this module itself on the CPU.  Nothing here touches a GPU.

All bounds are first-order running error bounds in units of U = 2^-24 (half an fp32 ulp, relative): a rounded operation adds |result| U, an input error is
carried through the operation's derivative, a sum of n non-negative terms added in ANY order costs (additions on the longest chain) U relative."""
import math

import numpy as np
import torch

U = 2.0 ** -24
F64 = torch.float64


# ================================================================================================ IDDPM loss
THR32 = float(np.float32(0.999))          # the comparison constant as an fp32 statement sees it (`x < -0.999` on a float tensor, `-0.999f` in the kernel)
LOG_CLAMP = 1e-12
BAND = (1e-12, 1e-3)                      # fp64 log arguments in here are left out: fp32 cancellation in cdf_plus - cdf_min decides the value


def _cdf64(z):
    return 0.5 * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))


def loss_ref64(out, x0, noise, coef8, tzero, thr=THR32):
    """The objective of pixart_sigma_amd/diffusion/iddpm.py:125-137 with _discretized_gaussian_log_likelihood, in fp64, written once.  out (B, 2C, H, W),
    x0 / noise (B, C, H, W), coef8 (B, 8) = the fp32 table rows cast to double (sqrt_ac, sqrt_1mac, post_c1, post_c2, post_logvar, log_betas, sqrt_recip_ac,
    sqrt_recipm1_ac), tzero (B,) bool.  Returns (mse (B,), vb (B,)) - differentiable in `out`."""
    B, C = x0.shape[:2]
    k = [coef8[:, i].reshape(B, 1, 1, 1) for i in range(8)]
    eps, v = torch.split(out, C, dim=1)
    e = eps.detach()
    xt = k[0] * x0 + k[1] * noise
    true_mean = k[2] * x0 + k[3] * xt
    frac = (v + 1) / 2
    lv = frac * k[5] + (1 - frac) * k[4]
    pred_x0 = k[6] * xt - k[7] * e
    mean = k[2] * pred_x0 + k[3] * xt
    kl = 0.5 * (-1.0 + lv - k[4] + torch.exp(k[4] - lv) + (true_mean - mean) ** 2 * torch.exp(-lv))
    cx = x0 - mean
    inv = torch.exp(-0.5 * lv)
    cp, cm = _cdf64(inv * (cx + 1.0 / 255.0)), _cdf64(inv * (cx - 1.0 / 255.0))
    ll = torch.where(x0 < -thr, torch.log(cp.clamp(min=LOG_CLAMP)),
                     torch.where(x0 > thr, torch.log((1.0 - cm).clamp(min=LOG_CLAMP)), torch.log((cp - cm).clamp(min=LOG_CLAMP))))
    vb = torch.where(tzero.reshape(B, 1, 1, 1), -ll, kl).flatten(1).mean(1) / math.log(2.0)
    mse = ((noise - eps) ** 2).flatten(1).mean(1)
    return mse, vb


def loss_ref64_grad(out, x0, noise, coef8, tzero, g_mse, g_vb, thr=THR32):
    """(mse, vb, d (g_mse . mse + g_vb . vb) / d out) by fp64 autograd."""
    o = out.detach().clone().requires_grad_(True)
    mse, vb = loss_ref64(o, x0, noise, coef8, tzero, thr)
    (mse * g_mse + vb * g_vb).sum().backward()
    return mse.detach(), vb.detach(), o.grad


class Tr:
    """A value with a running bound on its absolute error, in units of U.  Inputs are exact (e = 0); a constant that fp32 rounds carries e = |c|."""

    def __init__(self, v, e=None):
        self.v = v if torch.is_tensor(v) else torch.tensor(float(v), dtype=F64)
        self.e = torch.zeros_like(self.v) if e is None else e

    @staticmethod
    def const(c):                       # a literal that is not an fp32 number (1/255, sqrt(2/pi), 0.044715, 1/ln 2, 1/n)
        t = torch.tensor(float(c), dtype=F64)
        return Tr(t, t.abs())

    @staticmethod
    def _of(x):
        return x if isinstance(x, Tr) else Tr(x)

    def __add__(self, o):
        o = Tr._of(o)
        v = self.v + o.v
        return Tr(v, self.e + o.e + v.abs())

    __radd__ = __add__

    def __neg__(self):
        return Tr(-self.v, self.e)

    def __sub__(self, o):
        return self + (-Tr._of(o))

    def __rsub__(self, o):
        return Tr._of(o) + (-self)

    def __mul__(self, o):
        o = Tr._of(o)
        v = self.v * o.v
        return Tr(v, self.v.abs() * o.e + o.v.abs() * self.e + v.abs())

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Tr._of(o)
        v = self.v / o.v
        return Tr(v, self.e / o.v.abs() + v.abs() * o.e / o.v.abs() + v.abs())

    def exp(self):                      # __expf = exp2(a log2 e): the rounded product moves the result by |a| U relative, the instruction by one more
        v = torch.exp(self.v)
        return Tr(v, v * self.e + v * (1.0 + self.v.abs()))

    def tanh(self):
        v = torch.tanh(self.v)
        return Tr(v, (1 - v * v) * self.e + 2.0 * v.abs())

    def log(self):
        v = torch.log(self.v)
        return Tr(v, self.e / self.v.abs() + 2.0 * v.abs() + 2.0 ** -20)          # (the last term: fp32 numbers next to 1 have a log of their own spacing)

    def where(self, cond, o):
        o = Tr._of(o)
        return Tr(torch.where(cond, self.v, o.v), torch.where(cond, self.e, o.e))


SUM_DEPTH = 16      # a sample's sum: 3 serial adds in a thread, 6 + 2 tree levels in the block, the / n and / ln 2, and room for torch's own order; + the blocks' atomics


def loss_terms(out, x0, noise, coef8, tzero, g_mse, g_vb, thr=THR32):
    """The same objective with its analytic derivative, every operation in the order csrc/loss.hip and the torch statement perform it, as Tr values.  Returns
    dict(mse, vb: (B,) Tr;  d: (B, 2C, H, W) Tr;  arg: the fp64 log argument of the branch an element takes (t = 0 samples; 1 elsewhere);
    branch: (B, C, H, W) int, 0 = KL, 1 = x0 < -thr, 2 = x0 > thr, 3 = between)."""
    B, C = x0.shape[:2]
    n = x0[0].numel()
    k = [Tr(coef8[:, i].reshape(B, 1, 1, 1)) for i in range(8)]
    sqrt_ac, sqrt_1mac, c1, c2, true_lv, max_lv, r1, r2 = k
    eps, v = (Tr(t) for t in torch.split(out, C, dim=1))
    x0t, nz = Tr(x0), Tr(noise)
    t0 = tzero.reshape(B, 1, 1, 1).expand_as(x0)
    xt = sqrt_ac * x0t + sqrt_1mac * nz
    d = nz - eps
    mse_e = d * d
    dmse = Tr(-2.0) * d
    true_mean = c1 * x0t + c2 * xt
    frac = (v + 1.0) * 0.5
    lv = frac * max_lv + (1.0 - frac) * true_lv
    pred_x0 = r1 * xt - r2 * eps
    mean = c1 * pred_x0 + c2 * xt
    # KL
    e1, dm = (true_lv - lv).exp(), true_mean - mean
    e2 = dm * dm * (-lv).exp()
    kl = Tr(0.5) * (Tr(-1.0) + lv - true_lv + e1 + e2)
    dkl = Tr(0.5) * (Tr(1.0) - e1 - e2)
    # NLL
    cx, inv = x0t - mean, (Tr(-0.5) * lv).exp()
    c255, kk, a3 = Tr.const(1.0 / 255.0), Tr.const(math.sqrt(2.0 / math.pi)), Tr.const(0.044715)

    def cdf(z):
        th = (kk * (z + a3 * z * z * z)).tanh()
        return Tr(0.5) * (Tr(1.0) + th), Tr(0.5) * (Tr(1.0) - th * th) * kk * (Tr(1.0) + Tr(3.0) * a3 * z * z)

    zp, zm = inv * (cx + c255), inv * (cx - c255)
    (cp, dp), (cm, dmn) = cdf(zp), cdf(zm)
    om, dl = Tr(1.0) - cm, cp - cm
    lo, hi = x0 < -thr, x0 > thr
    arg = cp.where(lo, om.where(hi, dl))
    num = (dp * (Tr(-0.5) * zp)).where(lo, (-(dmn * (Tr(-0.5) * zm))).where(hi, dp * (Tr(-0.5) * zp) - dmn * (Tr(-0.5) * zm)))
    live = arg.v > LOG_CLAMP
    safe = Tr(torch.where(live, arg.v, torch.ones_like(arg.v)), torch.where(live, arg.e, torch.zeros_like(arg.e)))
    ll = safe.log().where(live, Tr(torch.full_like(arg.v, math.log(LOG_CLAMP)), torch.full_like(arg.v, 2.0 * abs(math.log(LOG_CLAMP)))))
    dll = (num / safe).where(live, Tr(torch.zeros_like(arg.v)))
    vb_e = (-ll).where(t0, kl)
    dterm = (-dll).where(t0, dkl)
    # d lv / d v as autograd forms it from lv = frac max_lv + (1 - frac) true_lv: two products that cancel (the kernel forms max_lv - true_lv first, which is
    # exact; the torch statement does not, and the bound has to hold for the order either of them uses)
    half = dterm * 0.5
    dvb = half * max_lv - half * true_lv
    inv_n, inv_ln2 = Tr.const(1.0 / n), Tr.const(1.0 / math.log(2.0))
    gm = Tr(g_mse.reshape(B, 1, 1, 1)) * inv_n
    gv = Tr(g_vb.reshape(B, 1, 1, 1)) * inv_n * inv_ln2
    de, dv = gm * dmse, gv * dvb
    depth = SUM_DEPTH + (n + 1023) // 1024

    def total(t, scale):
        s = t.v.flatten(1).sum(1)
        e = t.e.flatten(1).sum(1) + depth * t.v.abs().flatten(1).sum(1)
        r = Tr(s, e)
        for c in scale:
            r = r * c
        return r

    branch = torch.where(t0, torch.where(lo, 1, torch.where(hi, 2, 3)), torch.zeros_like(x0, dtype=torch.long))
    return dict(mse=total(mse_e, (inv_n,)), vb=total(vb_e, (inv_n, inv_ln2)), d=Tr(torch.cat([de.v, dv.v], 1), torch.cat([de.e, dv.e], 1)),
                arg=torch.where(t0, arg.v, torch.ones_like(arg.v)), branch=branch, z=torch.maximum(zp.v.abs(), zm.v.abs()))


def ratio(got, ref, bound_units, floor=1e-300):
    """max over elements of |got - ref| / (bound in units of U x U)."""
    return float(((got.double() - ref).abs() / (bound_units * U).clamp_min(floor)).max())


# ================================================================================================ CAME
class _Keep64(torch.Tensor):
    """A gradient whose .float() keeps it in fp64: CAMERef.step() casts every gradient with .float(); with this wrapper the oracle's own statements run in double."""

    def float(self):                    # noqa: A003
        return self.as_subclass(torch.Tensor)


def came_ref64(params, **kw):
    """oracle.came_ref.CAMERef over double parameters; step(grads) takes double gradients and keeps every state in fp64."""
    from oracle.came_ref import CAMERef

    class CAMERef64(CAMERef):
        def step(self, grads=None):
            assert grads is not None and all(g.dtype == F64 for g in grads)
            return super().step([g.as_subclass(_Keep64) for g in grads])

    assert all(p.dtype == F64 for p in params)
    return CAMERef64(params, **kw)


TERM = 4            # roundings in one addend g^2 + eps0 with g = grad * gscale: 1, 2 + 1, + 1
RSQ = 2             # a reciprocal square root (v_rsq_f32: 1 ulp; torch on the host: sqrt and division)
MAXJ5, MAXJ18 = 256 * 5, 256 * 18


def came_path(shape):
    if len(shape) < 2:
        return "1d"
    R, C = shape[-2], shape[-1]
    batch = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
    if batch == 1 and C % 4 == 0 and C <= MAXJ5:
        return "vec5"
    if batch == 1 and C % 4 == 0 and C <= MAXJ18:
        return "vec18"
    return "scalar"


def came_chains(shape, tile_elems):
    """Additions on the longest chain of each of the kernel's sums for one tensor (csrc/came.hip), from its path and its tiles (dp.came_tables):
      row   a lane adds its 4 * ceil(C / 256) (vector paths) or ceil(C / 64) (scalar path) addends one after the other, then 6 levels of wave_sum
      col   vector paths: a lane adds one addend per row its wave walks in the tile (ceil(rows per tile / 4)), 4 LDS atomics, one global atomic per tile;
            scalar path: one global atomic per row of the matrix (R), whatever their order
      rm    one matrix: lane 0 of a wave adds nv / R over the wave's rows (ceil(rows per tile / 4)), block_sum (6 + 2), one atomic per tile; batched: R atomics
      usq   a lane adds (rows of its wave) x (its addends per row), block_sum (6 + 2), one atomic per tile;  1-D: ceil(tile / 256) + 8 + tiles"""
    n = int(np.prod(shape))
    path = came_path(shape)
    if path == "1d":
        tiles = -(-n // tile_elems)
        return dict(path=path, usq=-(-min(n, tile_elems) // 256) + 8 + tiles)
    R, C = shape[-2], shape[-1]
    rows = n // C
    per = max(4, tile_elems // C // 4 * 4)
    if path == "scalar":
        per = min(per, 64)
    per = min(per, rows)
    tiles = -(-rows // per)
    wave_rows = -(-per // 4)
    if path == "scalar":
        lane = -(-C // 64)
        return dict(path=path, row=lane + 6, col=R, rm=R, usq=wave_rows * lane + 8 + tiles)
    lane = 4 * -(-C // 256)
    return dict(path=path, row=lane + 6, col=wave_rows + 4 + tiles, rm=wave_rows + 8 + tiles, usq=wave_rows * lane + 8 + tiles)


CAME_CAP = 1e-4     # no relative bound on a statistic or on an update is looser than what tests/test_came_gpu.py grants on updates, however long the chain


def _ema_err(E_prev, beta, omb, mean_err, mean_term, chain, value):
    """Absolute error of state = beta state + omb mean(terms): the previous error decays with beta, the mean carries its addends' errors, (chain + 1) U of its
    value for the sum and the division, and the update rounds three times.  Capped at CAME_CAP of the value."""
    return torch.minimum(beta * E_prev + omb * (mean_err + (chain + 1) * U * mean_term) + 3 * U * value, CAME_CAP * value)


class CameBound:
    """Element-wise absolute error bounds of every CAME state of ONE tensor after each step, propagated next to the fp64 oracle from the chain lengths above.
    update(...) takes the oracle's values before / after a step and returns dict(name -> bound tensor)."""

    def __init__(self, shape, tile_elems, lr, betas, eps, clip, wd):
        self.shape, self.ch = tuple(shape), came_chains(shape, tile_elems)
        self.lr, self.betas, self.eps, self.clip, self.wd = lr, betas, eps, clip, wd
        self.E = None

    def _factor_err(self, row, E_row, col, E_col):
        """Relative error (elementwise, broadcast to the tensor) of rsqrt(row / mean_r row) * rsqrt(col)."""
        ch = self.ch
        rm = row.mean(-1, keepdim=True)
        E_rm = E_row.mean(-1, keepdim=True) + (ch["rm"] + 1) * U * rm
        rel_rf = 0.5 * (E_row / row + E_rm / rm + U) + RSQ * U
        rel_cf = 0.5 * (E_col / col) + RSQ * U
        return rel_rf.unsqueeze(-1) + rel_cf.unsqueeze(-2)

    def update(self, g, st_before, st_after, p_before, p_after):
        """g: the scaled fp64 gradient the oracle was given; st_*: the oracle's state dict (clones) before / after; p_*: parameter before / after."""
        b1, b2, b3 = self.betas
        ch, factored = self.ch, len(self.shape) >= 2
        z = lambda t: torch.zeros_like(t)                       # noqa: E731
        if self.E is None:
            self.E = {k: z(v) for k, v in st_after.items()} | {"p": z(p_after)}
        E = self.E
        term = g * g + self.eps[0]
        if factored:
            E["exp_avg_sq_row"] = _ema_err(E["exp_avg_sq_row"], b2, 1 - b2, TERM * U * term.mean(-1), term.mean(-1), ch["row"], st_after["exp_avg_sq_row"])
            E["exp_avg_sq_col"] = _ema_err(E["exp_avg_sq_col"], b2, 1 - b2, TERM * U * term.mean(-2), term.mean(-2), ch["col"], st_after["exp_avg_sq_col"])
            rel_f = self._factor_err(st_after["exp_avg_sq_row"], E["exp_avg_sq_row"], st_after["exp_avg_sq_col"], E["exp_avg_sq_col"])
            rel_pre = U + rel_f + 2 * U                         # g, the two factors, two products
        else:
            nf = st_after["exp_avg_sq"]
            E["exp_avg_sq"] = b2 * E["exp_avg_sq"] + (1 - b2) * TERM * U * term + 3 * U * nf
            rel_pre = U + 0.5 * E["exp_avg_sq"] / nf + RSQ * U + U
        m_old = st_before["exp_avg"] if st_before else z(g)
        m_new = st_after["exp_avg"]
        u = (m_new - b1 * m_old) / (1 - b1)                     # the clipped update the oracle used
        # clip factor 1 / max(1, rms / clip): rms from sum(u_pre^2) over the whole tensor - a non-negative sum; 1-Lipschitz in rms / clip
        rel_sc = 0.5 * (2 * float(rel_pre.max()) + (ch["usq"] + 2) * U) + 3 * U
        rel_u = torch.clamp(rel_pre + U + rel_sc, max=CAME_CAP)
        E_u = u.abs() * rel_u
        E["exp_avg"] = b1 * E["exp_avg"] + (1 - b1) * E_u + (b1 * m_old.abs() + (1 - b1) * u.abs() + m_new.abs()) * U
        if factored:
            res = (u - m_new) ** 2 + self.eps[1]
            E_res = 2 * (u - m_new).abs() * (E_u + E["exp_avg"]) + TERM * U * res
            E["exp_avg_res_row"] = _ema_err(E["exp_avg_res_row"], b3, 1 - b3, E_res.mean(-1), res.mean(-1), ch["row"], st_after["exp_avg_res_row"])
            E["exp_avg_res_col"] = _ema_err(E["exp_avg_res_col"], b3, 1 - b3, E_res.mean(-2), res.mean(-2), ch["col"], st_after["exp_avg_res_col"])
            rel_f2 = self._factor_err(st_after["exp_avg_res_row"], E["exp_avg_res_row"], st_after["exp_avg_res_col"], E["exp_avg_res_col"])
            decay = 1 - self.lr * self.wd
            upd = (p_before * decay - p_after) / self.lr        # m * factors, as the oracle applied it
            scale = torch.where(m_new != 0, upd / torch.where(m_new != 0, m_new, torch.ones_like(m_new)), z(m_new)).abs()
            E_upd = E["exp_avg"] * scale + upd.abs() * (rel_f2 + 3 * U)
        else:
            E_upd = E["exp_avg"] + m_new.abs() * U
        ulp = 2.0 ** (torch.floor(torch.log2(p_after.abs().clamp_min(2.0 ** -126))) - 23)
        # half an ulp of p for the subtraction; with weight decay two more halves: p (1 - lr wd) rounds, and the kernel holds 1 - lr wd itself as an fp32 number
        # (|fl(d) - d| <= 2^-25 below 1, i.e. at most |p| 2^-25 <= ulp(p) / 2 per step; the oracle's p += p (-lr wd) does not have this one)
        E["p"] = E["p"] * (1 - self.lr * self.wd) + self.lr * E_upd + (0.5 if self.wd == 0 else 1.5) * ulp
        return dict(E)

    def worst_relative(self, st_after):
        """The largest bound relative to its state, over the non-negative statistics (for the `no bound looser than 1e-4` check)."""
        return max(float((self.E[k] / st_after[k]).max()) for k in st_after if k != "exp_avg")


# ================================================================================================ conditioning linears
def linear_ref64(x, w, b=None):
    """(y, sum_k |x||w| + |b|) in fp64."""
    xd, wd = x.double(), w.double()
    y, mag = xd @ wd.t(), xd.abs() @ wd.abs().t()
    if b is not None:
        y, mag = y + b.double(), mag + b.double().abs()
    return y, mag


def linear_bwd_ref64(dy, x, w):
    """(dx, dw, db) and their magnitude sums in fp64."""
    g, xd, wd = dy.double(), x.double(), w.double()
    return (g @ wd, g.t() @ xd, g.sum(0)), (g.abs() @ wd.abs(), g.abs().t() @ xd.abs(), g.abs().sum(0))


def condlin_chain(kind, M, N, K, prefilled=False):
    """Roundings on the longest chain of an output element of csrc/condlin.hip:
      fwd  a lane adds one group per 256 k (ceil(K / 256) additions; inside a group a product and two levels of a pair tree), 6 levels of wave_sum, the bias
      dx   a thread adds the products of its slice of at most 128 n one after the other (the product, the addition), then one atomic per slice (+ the pre-fill)
      dw   a thread adds a product per row m: M additions and the product;  db: M additions"""
    if kind == "fwd":
        return -(-K // 256) + 3 + 6 + 1
    if kind == "dx":
        return min(N, 128) + 1 + -(-N // 128) + (1 if prefilled else 0)
    if kind == "dw":
        return M + 1
    if kind == "db":
        return M
    raise KeyError(kind)


def within(got, ref, bound):
    """Every element of got within the (absolute, elementwise) bound of ref; returns (ok, worst value over bound)."""
    err = (got.double() - ref).abs()
    ok = bool((err <= bound).all()) and bool(torch.isfinite(got).all())
    nz = bound > 0
    worst = float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0
    if bool((err[~nz] > 0).any()):
        worst = float("inf")
    return ok, worst


# ================================================================================================ loss test cases (inputs only; shared by the CPU and GPU files)
# name -> (C, H, W, t per sample, regime per sample: "kl", "near", "deep" (both signs, three x0 ranges), "clamp" (deep, every element on the 1e-12 clamp))
LOSS_CASES = {
    "n16_B1_t0": (4, 2, 2, [0], ["near"]),
    "n16_B4_clamp_first": (4, 2, 2, [0, 0, 999, 1], ["clamp", "near", "kl", "kl"]),
    "n1020_B4_t0_first": (3, 4, 85, [0, 1, 500, 999], ["near", "kl", "kl", "kl"]),
    "n1024_B5_t0_last_two": (4, 16, 16, [2, 998, 0, 500, 0], ["kl", "kl", "clamp", "kl", "near"]),
    "n1028_B4_deep_last": (1, 4, 257, [1, 2, 998, 0], ["kl", "kl", "kl", "deep"]),
    "n2560_B1_t500": (4, 16, 40, [500], ["kl"]),
    "n4608_B5_five_blocks": (4, 32, 36, [0, 999, 0, 1, 2], ["near", "kl", "deep", "kl", "kl"]),
    "n16_B2_edge": (4, 2, 2, [0, 500], ["edge", "kl"]),
}
_G_MSE, _G_VB = [0.3, 1.0, 0.0, 2.0, 0.5], [1.5, 0.0, 0.25, 1.0, 0.7]


def loss_thresholds():
    """float32(+-0.999) and its two fp32 neighbours, both signs: 6 values."""
    t = np.float32(0.999)
    up, dn = np.nextafter(t, np.float32(2)), np.nextafter(t, np.float32(0))
    return torch.tensor([t, up, dn, -t, -up, -dn], dtype=torch.float32)


def loss_case(name, edge_lv=(-9.8, -9.2)):
    """fp32 inputs of a case (on the host): dict(out, x0, noise, t, tzero, g_mse, g_vb, regimes).  edge_lv: (post_logvar[0], log_betas[0]) of the schedule, for
    the "edge" regime (cdf_plus - cdf_min under the clamp, derivative numerator not zero)."""
    C, H, W, ts, regimes = LOSS_CASES[name]
    B, n = len(ts), C * H * W
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x0 = torch.randn(B, C, H, W, generator=g)
    noise = torch.randn(B, C, H, W, generator=g)
    out = torch.randn(B, 2 * C, H, W, generator=g) * 0.7
    for b, reg in enumerate(regimes):
        if reg == "kl":
            continue
        x = torch.rand(n, generator=g) * 2.4 - 1.2
        if reg == "clamp":
            x = torch.rand(n, generator=g) * 1.8 - 0.9                       # between the thresholds: cdf_plus - cdf_min = 0 on either side
        elif reg == "near" and n >= 16:
            x[5:11] = loss_thresholds()
        x0[b] = x.view(C, H, W)
        if reg == "edge":
            # cdf_plus - cdf_min below 1e-12 in fp64 while neither tanh is +-1 in fp32 (|z| = 4.75 ... 4.9: 1 - |tanh| = 4 ... 6 fp32 spacings): x0 - mean near
            # 1.25e5, where +-1/255 moves it by one fp32 spacing each way, and a log-variance that brings z back to 4.8.  The clamp is what makes the derivative 0 here:
            # the two halves of its numerator differ in fp32.
            x = torch.rand(n, generator=g) * 1.8 - 0.9
            x0[b] = x.view(C, H, W)
            sign = torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0).view(C, H, W)
            cx = sign * (1.2e5 + 500.0 * torch.arange(n).view(C, H, W))
            out[b, :C] = noise[b] + cx / 0.01                                 # mean = x0 + sqrt_recipm1_ac[0] (noise - eps), sqrt_recipm1_ac[0] = 0.01
            z = 4.75 + 0.15 * torch.arange(n).view(C, H, W) / n
            lv = -2.0 * torch.log(z / cx.abs())
            out[b, C:] = 2.0 * (lv - edge_lv[0]) / (edge_lv[1] - edge_lv[0]) - 1.0
            continue
        if reg == "near":
            out[b, :C] = noise[b] + 0.7 * torch.randn(C, H, W, generator=g)
        else:
            lo, hi = torch.nonzero(x < -0.9995).flatten(), torch.nonzero(x > 0.9995).flatten()
            sign = torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0)          # both signs in every range: alternate by position within each range
            for idx in (lo, hi, torch.nonzero((x >= -0.9995) & (x <= 0.9995)).flatten()):
                sign[idx] = torch.where(torch.arange(idx.numel()) % 2 == 0, 1.0, -1.0)
            out[b, :C] = noise[b] + 40.0 * sign.view(C, H, W)
    t = torch.tensor(ts)
    return dict(out=out, x0=x0, noise=noise, t=t, tzero=t == 0, g_mse=torch.tensor(_G_MSE[:B]), g_vb=torch.tensor(_G_VB[:B]), regimes=regimes)


def loss_coef8(diff, t, device="cpu"):
    """The (B, 8) fp32 coefficient rows the engine hands the kernel (iddpm.py:121-123)."""
    T = diff._tab(torch.device(device))
    return torch.stack([T[k].float() for k in ("sqrt_ac", "sqrt_1mac", "post_c1", "post_c2", "post_logvar", "log_betas", "sqrt_recip_ac", "sqrt_recipm1_ac")],
                       dim=1)[t.to(device)].contiguous()
