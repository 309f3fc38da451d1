"""train_scripts/train.py's step loop (train_loop) and batch sources (batches, data_source) on the CPU, with fakes for the optimizer, the diffusion
object, the loss scaler and the VAE, and the real LRSchedule.  The expected call sequence is the one of the loop as it stood inline in main():
zero_grad, opt.lr = sched.lr, `accum` micro-batches (next(it), t, training_losses, backward; all but the last inside reducer.no_sync()), opt.step,
sched.step, then - at a log step or in front of a save - the loss scaler's skipped steps taken back from the schedule, the log line, save.  No GPU."""
import contextlib
import importlib.util
import os
import types

import pytest
import torch

from conftest import ROOT
from pixart_sigma_amd.lr_schedule import LRSchedule

B = 2


@pytest.fixture(scope="module")
def train():
    spec = importlib.util.spec_from_file_location("train_loop_host_train", os.path.join(ROOT, "train_scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Opt:
    def __init__(self, trace):
        self.trace, self.steps, self.last_norm = trace, 0, torch.tensor(0.5)
        self.reducer = types.SimpleNamespace(no_sync=self.no_sync)

    lr = property(lambda self: self._lr)

    @lr.setter
    def lr(self, v):
        self._lr = v
        self.trace.append(("lr", v))

    def zero_grad(self):
        self.trace.append("zero_grad")

    def step(self):
        self.steps += 1
        self.trace.append("opt.step")

    @contextlib.contextmanager
    def no_sync(self):
        self.trace.append("no_sync enter")
        yield
        self.trace.append("no_sync exit")


class Diff:
    """Call k returns the per-sample losses [0.3 k, 0.3 k] * leaf, leaf = 1: the gradient that reaches the leaf is d(what was backpropagated) / d leaf =
    what was backpropagated."""
    def __init__(self, trace):
        self.trace, self.calls, self.ts = trace, 0, []

    def training_losses(self, model, x0, t, model_kwargs):
        assert set(model_kwargs) == {"y", "mask", "data_info"}
        self.calls += 1
        self.ts.append(t)
        self.trace.append("training_losses")
        leaf = torch.ones((), requires_grad=True)
        leaf.register_hook(lambda g: self.trace.append(("backward", float(g))))
        return {"loss": leaf * torch.full((x0.shape[0],), 0.3 * self.calls)}


class Sched(LRSchedule):
    def __init__(self, trace, **kw):
        super().__init__(1.0, "constant", num_warmup_steps=4, **kw)
        self.trace = trace

    def step(self, applied=True):
        self.trace.append("sched.step")
        return super().step(applied)


class Scaler:
    """One skipped step, reported from optimizer step 2 on."""
    value = 4.0

    def __init__(self, opt):
        self.opt = opt

    steps_skipped = property(lambda self: 1 if self.opt.steps >= 2 else 0)

    def scale(self, loss):
        return loss * self.value


def source(trace):
    info = {"img_hw": torch.tensor([[256.0, 256.0]] * B), "aspect_ratio": torch.tensor([[1.0]] * B)}
    while True:
        trace.append("next")
        yield torch.rand(B, 4, 2, 2), torch.zeros(B, 1, 3, 8), torch.ones(B, 3, dtype=torch.int64), info      # draws, as the VAE's sample() does


def cfg_of(train, **kw):
    return dict(train.DEFAULTS, **kw)


def run(train, cfg, world=1, rank=0, start_step=0, max_steps=2, scaler=False):
    trace, saves = [], []
    opt, diff = Opt(trace), Diff(trace)
    sched = Sched(trace, steps_per_call=world)
    sc = Scaler(opt) if scaler else None
    out = train.train_loop(cfg, object(), diff, opt, sched, sc, source(trace), "cpu", rank, world, start_step, max_steps,
                           lambda step: saves.append((step, sched.last_step)))
    return types.SimpleNamespace(trace=trace, saves=saves, opt=opt, diff=diff, sched=sched, out=out)


def test_call_order_and_loss_scaling(train, capsys):
    cfg = cfg_of(train, gradient_accumulation_steps=3, log_interval=1, save_model_steps=1000)
    torch.manual_seed(7)
    r = run(train, cfg)
    backward = lambda k: [("backward", pytest.approx(0.3 * k / 3, rel=1e-6))]                             # noqa: E731  loss / accum reaches backward
    local = lambda k: ["next", "training_losses", "no_sync enter"] + backward(k) + ["no_sync exit"]      # noqa: E731  no all-reduce for this one
    step = lambda first, lr: (["zero_grad", ("lr", lr)] + local(first) + local(first + 1) + ["next", "training_losses"] + backward(first + 2)      # noqa: E731
                              + ["opt.step", "sched.step"])
    assert r.trace == step(1, 0.0) + step(4, 0.25)                       # lr = sched.lr before the step: warm-up factor k / 4
    # next(it) draws before t does
    torch.manual_seed(7)
    for t in r.diff.ts:
        torch.rand(B, 4, 2, 2)
        assert torch.equal(t, torch.randint(0, 1000, (B,))) and t.dtype == torch.int64
    step_no, loss = r.out
    assert step_no == 2 and loss.item() == pytest.approx(0.3 * 6, rel=1e-6)
    lines = capsys.readouterr().out.splitlines()                         # the logged loss is the last micro-batch's, not divided
    assert len(lines) == 2 and lines[0].startswith("step 1 loss 0.9000 grad_norm 0.5000 lr 0.000e+00 ") and lines[0].endswith(" s/step")
    assert lines[1].startswith("step 2 loss 1.8000 grad_norm 0.5000 lr 2.500e-01 ") and "loss_scale" not in lines[1]


def test_scaled_loss_reaches_backward_and_the_log_line(train, capsys):
    cfg = cfg_of(train, gradient_accumulation_steps=2, log_interval=1, save_model_steps=1000)
    r = run(train, cfg, max_steps=1, scaler=True)
    assert [e for e in r.trace if isinstance(e, tuple) and e[0] == "backward"] == [("backward", pytest.approx(4.0 * 0.3 / 2)), ("backward", pytest.approx(4.0 * 0.6 / 2))]
    assert capsys.readouterr().out.startswith("step 1 loss 0.6000 grad_norm 0.5000 lr 0.000e+00 loss_scale 4 skipped 0 ")


def test_steps_and_saves(train, capsys):
    cfg = cfg_of(train, log_interval=1000, save_model_steps=3)
    r = run(train, cfg, start_step=5, max_steps=4)
    assert r.out[0] == 9 and r.opt.steps == 4 and [s for s, _ in r.saves] == [6, 9]
    r = run(train, cfg, rank=1, start_step=5, max_steps=4)
    assert r.out[0] == 9 and r.opt.steps == 4 and r.saves == []
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("rank", [0, 1])
def test_skipped_steps_leave_the_schedule_in_front_of_a_save(train, capsys, rank):
    cfg = cfg_of(train, log_interval=5, save_model_steps=3)
    r = run(train, cfg, world=2, rank=rank, max_steps=5, scaler=True)
    assert r.sched.last_step == 2 * (5 - 1)                              # every rank reconciles
    assert r.saves == ([(3, 2 * (3 - 1))] if rank == 0 else [])          # and has done so when save(3) runs
    out = capsys.readouterr().out
    assert (out.startswith("step 5 ") and " skipped 1 " in out and out.count("\n") == 1) if rank == 0 else out == ""
    r = run(train, cfg, world=2, rank=rank, max_steps=5)                 # no scaler: nothing subtracted
    assert r.sched.last_step == 2 * 5 and r.saves == ([(3, 2 * 3)] if rank == 0 else [])


@pytest.mark.parametrize("load_vae_feat", [True, False])
def test_batches_yield_their_default_data_info(train, load_vae_feat):
    cfg = cfg_of(train, load_vae_feat=load_vae_feat)
    batch = next(train.batches(cfg, B, 32, 4, "cpu", 0, 1, synthetic=True))
    assert len(batch) == 4
    z, y, mask, info = batch
    assert tuple(z.shape) == ((B, 4, 32, 32) if load_vae_feat else (B, 3, 256, 256)) and tuple(y.shape) == (B, 1, 4, 4096) and tuple(mask.shape) == (B, 4)
    assert info["img_hw"].tolist() == [[256.0, 256.0]] * B and info["aspect_ratio"].tolist() == [[1.0]] * B


def test_data_source_encodes_and_scales_one_batch_per_next(train, monkeypatch):
    zs = [torch.full((B, 3, 8, 8), float(i)) for i in (1, 2)]
    monkeypatch.setattr(train, "batches", lambda *a: iter([(z, "y", "mask", "info") for z in zs]))
    seen = []

    def encode(z):
        seen.append(z)
        return types.SimpleNamespace(latent_dist=types.SimpleNamespace(sample=lambda: (z[:, :1] + 0.5).double()))
    cfg = cfg_of(train, load_vae_feat=False, scale_factor=0.25)
    it, captions = train.data_source(cfg, True, B, 1, 4, "cpu", 0, 1, types.SimpleNamespace(encode=encode))
    assert captions is None and seen == []                               # nothing is encoded ahead of the next() that needs it
    for i, z in enumerate(zs):
        x0, y, mask, info = next(it)
        assert len(seen) == i + 1 and seen[i] is z and (y, mask, info) == ("y", "mask", "info")
        assert x0.dtype == torch.float32 and torch.equal(x0, torch.full((B, 1, 8, 8), 0.25 * (i + 1.5)))
    # without a VAE the latents are only scaled
    it, _ = train.data_source(cfg_of(train, scale_factor=0.25), True, B, 1, 4, "cpu", 0, 1, None)
    assert torch.equal(next(it)[0], zs[0] * 0.25)
