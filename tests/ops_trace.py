"""TEST INFRASTRUCTURE: the launch schedule of engine.Engine as text.  A recorder wraps every kernel stand-in of tests/fake_ops.py and writes one line per
call - the op, then every argument that was passed, by parameter name (names from the real pixart_sigma_amd.ops signatures) - and one line per
grad_ready_hook firing.  tests/test_engine_schedule.py holds the lines against tests/golden/engine_schedule_<case>.txt:

    python tests/ops_trace.py --write      # records every case from the tree it runs in; the first line of each file names that commit

A tensor is `buffer+element_offset:(shape)/(strides):dtype`.  `buffer` is `master`, `grad` or `shadow` of the ParamStore, with the parameter's name when
offset and size match one (`grad[blocks.1.mlp.fc1.weight]`); `qs_w` / `qs_b` are the engine's prescaled qkv copies; any other storage is `t<k>`, numbered in
order of first sighting (arguments of a call first, then what it returned) - `z<k>` when the sequencing code itself allocated it zero-filled (torch.zeros /
zeros_like in engine.py or PixArtMS.py), so "this gradient buffer may be torch.empty" and "it must be zeroed" are different texts.  That marking sees only
`torch.zeros` / `torch.zeros_like` spelled through the two modules' `torch` global (replaced by a proxy while a trace runs): a buffer zeroed another way
(`x.new_zeros`, `torch.empty(...).zero_()`) would read `t<k>`.  The recorder keeps
every storage it has seen alive until the trace is rendered, so a freed block's address cannot come back under another number: a changed lifetime cannot
alias two buffers in the text."""
import contextlib
import inspect
import os
import subprocess
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fake_ops  # noqa: E402
from pixart_sigma_amd import engine, ops as real_ops  # noqa: E402
import pixart_sigma_amd.model.nets.PixArtMS  # noqa: E402,F401

nets = sys.modules["pixart_sigma_amd.model.nets.PixArtMS"]      # the module (the package re-exports the class under the same name)

GOLDEN = os.path.join(HERE, "golden")
DTYPES = {real_ops.F32: "f32", real_ops.BF16: "bf16", torch.int32: "i32"}     # BF16 = the process's 16-bit operand type (its historical name)
OPS = [n for n, f in vars(fake_ops).items() if inspect.isfunction(f) and not n.startswith("_") and hasattr(real_ops, n)]


class _T:
    """What the text says about a tensor, taken when the call is made."""

    def __init__(self, t):
        self.ptr, self.off, self.shape, self.strides, self.dtype = t.untyped_storage().data_ptr(), t.storage_offset(), tuple(t.shape), t.stride(), t.dtype


class _Torch:
    """`torch` as the sequencing modules see it while a trace runs: zeros / zeros_like report their storage to the trace, everything else is torch's."""

    def __init__(self, tr):
        self._tr = tr

    def __getattr__(self, name):
        return getattr(torch, name)

    def zeros(self, *a, **kw):
        return self._tr.zeroed(torch.zeros(*a, **kw))

    def zeros_like(self, *a, **kw):
        return self._tr.zeroed(torch.zeros_like(*a, **kw))


class Trace:
    def __init__(self):
        self.calls, self._keep, self._zeroed = [], [], set()

    def zeroed(self, t):
        self._keep.append(t.untyped_storage())
        self._zeroed.add(t.untyped_storage().data_ptr())
        return t

    def _snap(self, v):
        if isinstance(v, torch.Tensor):
            self._keep.append(v.untyped_storage())
            return _T(v)
        if isinstance(v, (tuple, list)):
            return tuple(self._snap(e) for e in v)
        if isinstance(v, dict):
            return {k: self._snap(e) for k, e in v.items()}
        return v

    def wrap(self, name):
        fn, sig = getattr(fake_ops, name), inspect.signature(getattr(real_ops, name))

        def traced(*a, **kw):
            bound = sig.bind(*a, **kw)
            args = []
            for k, v in bound.arguments.items():
                kind = sig.parameters[k].kind
                if kind == inspect.Parameter.VAR_KEYWORD:
                    args += list(v.items())
                elif kind == inspect.Parameter.VAR_POSITIONAL:
                    args += [(f"{k}{i}", e) for i, e in enumerate(v)]
                else:
                    args.append((k, v))
            call = [name, [(k, self._snap(v)) for k, v in args], None]
            self.calls.append(call)
            ret = fn(*a, **kw)
            call[2] = self._snap(ret)
            return ret
        return traced

    def hook(self, prefix):
        """For Engine.grad_ready_hook."""
        self.calls.append(["grad_ready_hook", [("prefix", prefix)], None])

    def mark(self, text):
        self.calls.append(["#", text, None])

    def lines(self, *engines):
        """The text.  engines: whose ParamStore buffers and _qs pair get their names."""
        named, params = {}, {}
        for e in engines:
            S = e.S
            for buf in ("master", "grad", "shadow"):
                p = getattr(S, buf).untyped_storage().data_ptr()
                named[p] = buf
                params[p] = {(S.offset[n], S.numel[n]): n for n in S.names}
            if e._qs is not None:
                named[e._qs[0].untyped_storage().data_ptr()], named[e._qs[1].untyped_storage().data_ptr()] = "qs_w", "qs_b"
        count = [0]

        def fmt(v):
            if isinstance(v, _T):
                if v.ptr not in named:
                    named[v.ptr] = f"{'z' if v.ptr in self._zeroed else 't'}{count[0]}"
                    count[0] += 1
                buf = named[v.ptr]
                n = 1
                for s in v.shape:
                    n *= s
                pname = params.get(v.ptr, {}).get((v.off, n))
                if pname is not None:
                    buf += f"[{pname}]"
                tup = lambda t: "(" + ",".join(str(i) for i in t) + ")"     # noqa: E731
                return f"{buf}+{v.off}:{tup(v.shape)}/{tup(v.strides)}:{DTYPES.get(v.dtype, v.dtype)}"
            if isinstance(v, tuple):
                return "(" + ", ".join(fmt(e) for e in v) + ")"
            if isinstance(v, dict):
                return "{" + ", ".join(f"{k}={fmt(e)}" for k, e in v.items()) + "}"
            return repr(v)
        out = []
        for name, args, ret in self.calls:
            if name == "#":
                out.append(f"# {args}")
                continue
            line = " ".join([name] + [f"{k}={fmt(v)}" for k, v in args])
            out.append(line if name == "grad_ready_hook" else f"{line} -> {fmt(ret)}")
        return out


@contextlib.contextmanager
def recording():
    """engine.ops is the recorder's wrapped fake_ops inside the block (as tests/test_dp_gloo.py installs the plain one), and pixart_sigma_amd.ops.ln_mod_fwd its
    wrapper: only a _BlockFn that calls that kernel through the real module needs it (the one the fixtures were recorded from did; the recorder has to run on
    both).  `torch` of engine.py and PixArtMS.py is _Torch.  All are put back on exit."""
    tr = Trace()
    ns = types.SimpleNamespace(**{k: v for k, v in vars(fake_ops).items() if not k.startswith("__")})
    for n in OPS:
        setattr(ns, n, tr.wrap(n))
    keep = engine.ops, real_ops.ln_mod_fwd, engine.torch, nets.torch
    engine.ops, real_ops.ln_mod_fwd, engine.torch, nets.torch = ns, ns.ln_mod_fwd, _Torch(tr), _Torch(tr)
    try:
        yield tr
    finally:
        engine.ops, real_ops.ln_mod_fwd, engine.torch, nets.torch = keep


@contextlib.contextmanager
def _env(**kv):
    """The A/B knobs of the cases; PXA_TEXT_CACHE is taken out so that an outer setting cannot change the inference case."""
    kv = dict({"PXA_TEXT_CACHE": None, "PXA_Q_PRESCALE": None, "PXA_FUSED_CPROJ_BIAS": None}, **kv)
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


B, L, LENS, D = 2, 8, [8, 5], 1152


def _engine_case(sampling=None, qk_norm=False, latent=(8, 8), save="all", drop=False, calls=1, env=None):
    """depth-2 PixArtMS at the default width, compression (if any) on layer 1 only, B = 2 with ragged text lengths; Engine.forward / backward driven directly."""
    from pixart_sigma_amd.model.nets.PixArtMS import PixArtMS
    with _env(**(env or {})), recording() as tr:
        torch.manual_seed(0)
        kv = {"sampling": sampling, "scale_factor": 2, "kv_compress_layer": [1]} if sampling else None
        m = PixArtMS(depth=2, input_size=8, model_max_length=L, class_dropout_prob=0.0, qk_norm=qk_norm, kv_compress_config=kv)
        m._prepare(torch.device("cpu"))
        eng = m._engine
        eng.grad_ready_hook = tr.hook
        x, y2d = torch.zeros(B, 4, *latent), torch.zeros(B * L, 4096)
        mod, fin = torch.zeros(2, B, 6, D), torch.zeros(B, 2, D)
        row_idx = torch.tensor([b * L + i for b, n in enumerate(LENS) for i in range(n)], dtype=torch.int32)
        dmask = torch.tensor([0, 1], dtype=torch.int32) if drop else None
        y_null = torch.zeros(L, 4096) if drop else None
        for i in range(calls):
            if calls > 1:
                tr.mark(f"call {i + 1}")
            if save:
                out, saved = eng.forward(x, y2d, mod, fin, row_idx, LENS, dmask, save, y_null=y_null)
                tr.mark("backward")
                eng.backward(torch.zeros_like(out), saved)
            else:
                with torch.no_grad():
                    eng.forward(x, y2d, mod, fin, row_idx, LENS, dmask, None, y_null=y_null)
        return tr.lines(eng)


def _block_case(sampling=None, sr=1):
    """A stand-alone PixArtMSBlock through autograd (_BlockFn) on the 4 x 4 token grid."""
    from pixart_sigma_amd.model.nets.PixArtMS import PixArtMSBlock
    with _env(), recording() as tr:
        torch.manual_seed(0)
        blk = PixArtMSBlock(D, 16, sampling=sampling, sr_ratio=sr)
        x = torch.zeros(B, 16, D, requires_grad=True)
        y = torch.zeros(1, sum(LENS), D, requires_grad=True)
        t = torch.zeros(B, 6 * D, requires_grad=True)
        out = blk(x, y, t, mask=LENS, HW=(4, 4))
        blk._standalone.grad_ready_hook = tr.hook
        tr.mark("backward")
        out.sum().backward()
        return tr.lines(blk._standalone)


CASES = {
    "plain_all": lambda: _engine_case(),
    "plain_ckpt": lambda: _engine_case(save="ckpt"),
    "conv_covered": lambda: _engine_case("conv"),
    "conv_not_covered": lambda: _engine_case("conv", latent=(12, 10)),
    "kv_uniform": lambda: _engine_case("uniform"),
    "kv_ave": lambda: _engine_case("ave"),
    "kv_uniform_every": lambda: _engine_case("uniform_every"),
    "qk_norm": lambda: _engine_case(qk_norm=True),
    "no_q_prescale": lambda: _engine_case(env={"PXA_Q_PRESCALE": "0"}),
    "no_fused_cproj_bias": lambda: _engine_case(env={"PXA_FUSED_CPROJ_BIAS": "0"}),
    "drop_y_null": lambda: _engine_case(drop=True),
    "inference_twice": lambda: _engine_case(save=None, calls=2),
    "block_plain": lambda: _block_case(),
    "block_conv": lambda: _block_case("conv", 2),
}


def fixture(case):
    return os.path.join(GOLDEN, f"engine_schedule_{case}.txt")


if __name__ == "__main__":
    assert sys.argv[1:] == ["--write"], __doc__
    head = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    dirty = subprocess.run(["git", "status", "--porcelain", "--", "pixart_sigma_amd"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    for case, run in CASES.items():
        text = "\n".join([f"# engine schedule '{case}', recorded from commit {head}{' (package modified)' if dirty else ''} by tests/ops_trace.py --write"] + run()) + "\n"
        assert len(text) < 100_000, (case, len(text))
        with open(fixture(case), "w") as f:
            f.write(text)
        print(case, len(text))
