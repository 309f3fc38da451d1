"""Optimizer step time on the full XL/2 parameter set (610.9 M parameters, flat store): fused AdamW vs fused CAME (clip included).
Usage (GPU box): python tools/bench_opt.py
                 python tools/bench_opt.py --ema [--out FILE]    the EMA kernels (pxa_ema_update, pxa_swap_f32) alone at XL/2's store.total, and each
                                                                 optimizer's step with and without WeightEMA.update() behind it; one JSON line"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pixart_sigma_amd import PixArtMS_XL_2  # noqa: E402
from pixart_sigma_amd.dp import FusedAdamW, FusedCAME  # noqa: E402


def timed(fn, iters=10, warm=2):
    """Milliseconds per call, events around `iters` back-to-back calls."""
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def bench_ema(m, out):
    from pixart_sigma_amd import ops
    from pixart_sigma_amd.ema import WeightEMA
    st = m._store
    ema = WeightEMA(m, 0.9999)
    n = st.total
    ms_u = timed(lambda: ops.ema_update(ema.ema, st.master, 0.9999), iters=20)
    ms_s = timed(lambda: ops.swap_f32(st.master, ema.ema), iters=20)             # an even number of swaps: both buffers end where they began
    ms_c = timed(lambda: ema.ema.copy_(st.master), iters=20)                     # the runtime's own device copy of the same buffer, 8 bytes per element
    out["ema"] = {"elements": n,
                  "ema_update": {"ms": ms_u, "bytes": 12 * n, "TB_per_s": 12 * n / ms_u / 1e9},
                  "swap_f32": {"ms": ms_s, "bytes": 16 * n, "TB_per_s": 16 * n / ms_s / 1e9},
                  "copy": {"ms": ms_c, "bytes": 8 * n, "TB_per_s": 8 * n / ms_c / 1e9}}
    for name, cls in (("adamw", FusedAdamW), ("came", FusedCAME)):
        opt = cls(m)
        opt.zero_grad()
        st.grad.normal_(std=1e-3)

        def both():
            opt.step()
            ema.update()
        out["ema"][name] = {"ms_per_step": timed(opt.step), "ms_per_step_with_ema": timed(both)}
        out["ema"][name]["finite"] = bool(torch.isfinite(st.master).all() and torch.isfinite(ema.ema).all())
        del opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ema", action="store_true", help="time the EMA kernels and the optimizer step with / without the update behind it")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    torch.manual_seed(0)
    m = PixArtMS_XL_2(input_size=32, pe_interpolation=0.5, model_max_length=300).cuda().train()
    m.prepare(torch.device("cuda"))
    n = sum(p.numel() for p in m.parameters())
    out = {"parameters": n}
    if a.ema:
        bench_ema(m, out)
    else:
        for name, cls in (("adamw", FusedAdamW), ("came", FusedCAME)):
            opt = cls(m)
            opt.zero_grad()
            m._store.grad.normal_(std=1e-3)
            for _ in range(2):
                opt.step()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                opt.step()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / 10
            state = sum(v.numel() * v.element_size() for v in opt.state_dict().values() if torch.is_tensor(v))
            out[name] = {"ms_per_step": ms, "state_GB": state / 1e9, "finite": bool(torch.isfinite(m._store.master).all())}
            del opt
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
