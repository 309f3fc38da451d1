"""Exponential moving average of the trained weights, on the flat parameter store.

Replaces the reference's `model_ema` (a deep copy of the model updated parameter by parameter by ema_update, written as `state_dict_ema`:
diffusion/utils/checkpoint.py:11-20,45,62-63; `ema_rate = 0.9999`, configs/PixArt_xl2_internal.py) with ONE flat fp32 buffer beside ParamStore.master:

  * update(): one pxa_ema_update launch over the whole buffer behind the optimizer step (csrc/ema.hip).  With a LossScaler the kernel reads the scaler's
    device record and writes nothing on a step that was skipped on overflow - no host synchronisation, the EMA counts applied steps;
  * swapped(): the one way to RUN the model on the averaged weights.  There is no second model: master and EMA exchange their contents in place
    (pxa_swap_f32), the store's ordinary "weights changed" path runs (refresh_shadow(force=True) -> bump(): 16-bit shadow, q-prescaled qkv copy, LoRA
    merge and the generation that keys the text cache all follow, in place, under any captured graph), and the same happens again on the way out.
    Afterwards master, EMA and shadow have their earlier bits, every nn.Parameter still points where it pointed, and no full-size temporary exists.

With trainable LoRA adapters the EMA is over the adapters' store (what FusedAdamW updates); the frozen base is not copied.

More than one rank: nothing is communicated.  The EMA is a deterministic function of the sequence of master weights, which dp.check_replicas already
holds equal on every rank, so every rank computes the same average.  This has NOT been run on more than one GPU.
"""
import contextlib

import torch

from .dp import FusedAdamW


class WeightEMA:
    def __init__(self, model, decay=0.9999, scaler=None):
        assert model._store is not None, "call model.prepare(device) (or run one forward) before building the EMA"
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError(f"EMA decay must lie in [0, 1), got {decay!r}")
        self.model, self.store = model, FusedAdamW._live_store(model)
        self.decay, self.scaler = float(decay), scaler
        self.ema = self.store.master.clone()
        self._swapped = False

    @property
    def on_adapters(self):
        return self.store is not self.model._store

    def _check_store(self):
        if FusedAdamW._live_store(self.model) is not self.store:
            raise RuntimeError("the model rebuilt its flat parameter store after this EMA was created (model moved to another device, or a "
                               "parameter's storage was replaced): the EMA would follow orphaned buffers - build it after the move")

    def update(self):
        """ema <- decay * ema + (1 - decay) * master, behind optimizer.step().  One launch, no host synchronisation."""
        from . import ops
        self._check_store()
        if self._swapped:
            raise RuntimeError("WeightEMA.update() inside swapped(): the master buffer holds the EMA there")
        ops.ema_update(self.ema, self.store.master, self.decay, self.scaler.state if self.scaler is not None else None)

    def reset(self):
        """Start the average again from the current master weights (after weights were loaded)."""
        self._check_store()
        self.ema.copy_(self.store.master)

    # ---- state
    def state_dict(self):
        """name -> tensor, views of the flat EMA buffer.  Base store: the keys and order of model.state_dict(), the model's buffers carried as they are
        (the reference's state_dict_ema layout).  Adapter store: the adapters' internal names."""
        st = self.store
        if self.on_adapters:
            return {n: st.view(self.ema, n) for n in st.names}
        return {k: (st.view(self.ema, k) if k in st.offset else v) for k, v in self.model.state_dict().items()}

    def load_state_dict(self, sd):
        st = self.store
        buffers = set() if self.on_adapters else {k for k, _ in self.model.named_buffers()}
        missing = [n for n in st.names if n not in sd]
        unexpected = [k for k in sd if k not in st.offset and k not in buffers]
        if missing or unexpected:
            raise KeyError(f"WeightEMA.load_state_dict: missing {missing}, unexpected {unexpected}")
        for n in st.names:
            v = sd[n]
            if tuple(v.shape) != tuple(st.shape[n]):
                raise ValueError(f"WeightEMA.load_state_dict: {n} has shape {tuple(v.shape)}, the parameter {tuple(st.shape[n])}")
            st.view(self.ema, n).copy_(v)

    # ---- running the model on the average
    def _exchange(self):
        from . import ops
        ops.swap_f32(self.store.master, self.ema)
        self.store.refresh_shadow(force=True)      # re-cast + bump(): derived buffers rewritten in place; on the adapter store the bump re-merges

    @contextlib.contextmanager
    def swapped(self):
        """Inside, the model computes with the EMA weights (and `self.ema` holds the live ones).  Exit restores both, on exceptions too.  Not re-entrant."""
        if self._swapped:
            raise RuntimeError("WeightEMA.swapped() is already active: it does not nest")
        self._check_store()
        self._swapped = True
        try:
            self._exchange()
            yield self
        finally:
            try:
                self._exchange()
            finally:
                self._swapped = False
