"""TEST INFRASTRUCTURE: CPU stand-ins for the two LoRA ops (pixart_sigma_amd.ops.lora_merge / lora_bwd) beside tests/fake_ops.py, and a recorder that adds them
to the launch-schedule trace of tests/ops_trace.py - so the engine's sequencing WITH adapters (which slices are merged, which x / dy column blocks each
adapter-gradient call reads, when gradient groups are reported complete) can be checked without a GPU."""
import contextlib
import types

import torch

import fake_ops
import ops_trace
from pixart_sigma_amd import engine


def lora_merge(master, lo, hi, A, Bt, s, dst, dst2=None, mul_rows=(0, 0), mul=1.0, dst_f32=None):
    fake_ops.CALLS.append(("lora_merge", lo, hi))


def lora_bwd(x, dy, A16, Bt16, s, dA, dBt):
    fake_ops.CALLS.append(("lora_bwd", tuple(x.shape), tuple(dy.shape)))
    dA.add_(fake_ops.pattern(dA, 31))
    dBt.add_(fake_ops.pattern(dBt, 32))


@contextlib.contextmanager
def recording():
    """ops_trace.recording() with the two LoRA ops recorded like every other op (arguments by the real wrappers' parameter names)."""
    fake_ops.lora_merge, fake_ops.lora_bwd = lora_merge, lora_bwd
    try:
        with ops_trace.recording() as tr:
            for n in ("lora_merge", "lora_bwd"):
                setattr(engine.ops, n, tr.wrap(n))
            yield tr
    finally:
        del fake_ops.lora_merge, fake_ops.lora_bwd


def store_names(store):
    """What Trace.lines needs to print an adapter store's buffers by parameter name."""
    return types.SimpleNamespace(S=store, _qs=None)


def lora_case(save="all", sampling=None, qk_norm=False, targets=None, r=4):
    """The depth-2 engine case of tests/ops_trace.py (_engine_case) with adapters on `targets` (default: all ten block linears); returns (lines, model)."""
    from pixart_sigma_amd.lora import BLOCK_MODULES, LoraConfig
    from pixart_sigma_amd.model.nets.PixArtMS import PixArtMS
    B, L, LENS, D = ops_trace.B, ops_trace.L, ops_trace.LENS, ops_trace.D
    with ops_trace._env(), recording() as tr:
        torch.manual_seed(0)
        kv = {"sampling": sampling, "scale_factor": 2, "kv_compress_layer": [1]} if sampling else None
        m = PixArtMS(depth=2, input_size=8, model_max_length=L, class_dropout_prob=0.0, qk_norm=qk_norm, kv_compress_config=kv)
        m.add_lora(LoraConfig(r=r, target_modules=list(targets or BLOCK_MODULES)))
        m._prepare(torch.device("cpu"))
        eng = m._engine
        eng.grad_ready_hook = tr.hook
        x, y2d = torch.zeros(B, 4, 8, 8), torch.zeros(B * L, 4096)
        mod, fin = torch.zeros(2, B, 6, D), torch.zeros(B, 2, D)
        row_idx = torch.tensor([b * L + i for b, n in enumerate(LENS) for i in range(n)], dtype=torch.int32)
        tr.mark("forward")
        out, saved = eng.forward(x, y2d, mod, fin, row_idx, LENS, None, save)
        tr.mark("backward")
        eng.backward(torch.zeros_like(out), saved)
        return tr.lines(eng, store_names(m._lora.store)), m
