"""TEST INFRASTRUCTURE: CPU stand-ins for what train_scripts/train.py's train_loop drives - optimizer, diffusion object, schedule, batch source (the ones of
tests/test_train_loop_host.py, which stays as it is) - plus the two that the EMA / validation keyword arguments add: an EMA that records its update() and a
validate callback that records the step it was called for.  Everything appends to one trace list."""
import contextlib
import types

import torch

from pixart_sigma_amd.lr_schedule import LRSchedule

B = 2


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
    def __init__(self, trace):
        self.trace, self.calls = trace, 0

    def training_losses(self, model, x0, t, model_kwargs):
        self.calls += 1
        self.trace.append("training_losses")
        leaf = torch.ones((), requires_grad=True)
        leaf.register_hook(lambda g: self.trace.append("backward"))
        return {"loss": leaf * torch.full((x0.shape[0],), 0.3 * self.calls)}


class Sched(LRSchedule):
    def __init__(self, trace, **kw):
        super().__init__(1.0, "constant", num_warmup_steps=0, **kw)
        self.trace = trace

    def step(self, applied=True):
        self.trace.append("sched.step")
        return super().step(applied)


class Ema:
    def __init__(self, trace):
        self.trace = trace

    def update(self):
        self.trace.append("ema.update")


def source(trace):
    info = {"img_hw": torch.tensor([[256.0, 256.0]] * B), "aspect_ratio": torch.tensor([[1.0]] * B)}
    while True:
        trace.append("next")
        yield torch.rand(B, 4, 2, 2), torch.zeros(B, 1, 3, 8), torch.ones(B, 3, dtype=torch.int64), info


def run(train, cfg, max_steps, start_step=0, rank=0, ema=False, validate=False, keywords=True):
    """train_loop over the fakes; keywords=False calls it with the positional arguments alone, as every caller did before the keyword arguments existed."""
    trace = []
    opt, diff, sched = Opt(trace), Diff(trace), Sched(trace)
    args = (cfg, object(), diff, opt, sched, None, source(trace), "cpu", rank, 1, start_step, max_steps, lambda step: trace.append(("save", step)))
    if keywords:
        kw = dict(ema=Ema(trace) if ema else None, validate=(lambda step: trace.append(("validate", step))) if validate else None)
        train.train_loop(*args, **kw)
    else:
        train.train_loop(*args)
    return trace
