"""Inference workloads of BASELINE.json on one MI355X (parity-tested elsewhere; this measures them):
  config 2: PixArt-Sigma-XL/2 512px, batch 8, 20-step DPM-Solver++ with CFG 4.5 (model batch 16)
  config 4: PixArt-Sigma-XL/2 2K multi-scale, KV compression (conv, x2) on layers 14-27, batch 2 (model batch 4), 20 steps
Usage: python tools/bench_infer.py [512|2k|both] [--steps 20] [--graph] [--fp8 [mx|dequant]]
       python tools/bench_infer.py --sweep_f8      # ops.gemm_f8 against ops.gemm at the six (N, K) of a block, and the quantise passes alone
--fp8 runs the same workloads with PixArtMS.enable_fp8 (MXFP8 token GEMMs) and adds the relative L2 of the sample against the 16-bit one of the same weights
(random weights: no statement about pictures)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench import MFMA_PEAK, fwd_flops_per_sample  # noqa: E402
from pixart_sigma_amd import DPMS, PixArtMS_XL_2  # noqa: E402


def run(name, image_size, bs, steps, kv, graph=False, fp8=None):
    lat = image_size // 8
    N = (lat // 2) ** 2
    kvc = {"sampling": "conv", "scale_factor": 2, "kv_compress_layer": list(range(14, 28))} if kv else None
    torch.manual_seed(0)
    m = PixArtMS_XL_2(input_size=lat, pe_interpolation=image_size / 512, model_max_length=300, kv_compress_config=kvc)
    with torch.no_grad():
        for blk in m.blocks:
            blk.cross_attn.proj.weight.normal_(std=0.02)
        m.final_layer.linear.weight.normal_(std=0.02)
    m = m.cuda().eval()
    g = torch.Generator().manual_seed(1)
    z = torch.randn(bs, 4, lat, lat, generator=g).cuda()
    y = torch.randn(bs, 1, 300, 4096, generator=g).cuda()
    null_y = torch.randn(1, 1, 300, 4096, generator=g).repeat(bs, 1, 1, 1).cuda()
    mask = torch.ones(bs, 300, dtype=torch.int64)      # host mask: no per-step sync

    solver = DPMS(m.forward_with_dpmsolver, condition=y, uncondition=null_y, cfg_scale=4.5, model_kwargs=dict(data_info=None, mask=mask))

    def sample():
        fn = solver.sample_graphed if graph else solver.sample
        return fn(z, steps=steps, order=2, skip_type="time_uniform", method="multistep")
    extra = {}
    if fp8:
        with torch.no_grad():           # what FP8 does to one evaluation and to the whole chain, against the 16-bit path of the same (random) weights
            t1 = torch.full((bs,), 500, device="cuda")
            e16, s16 = m.forward_with_dpmsolver(z, t1, y, data_info=None, mask=mask), solver.sample(z, steps=steps, order=2, skip_type="time_uniform", method="multistep")
            m.enable_fp8(fp8)
            e8, s8 = m.forward_with_dpmsolver(z, t1, y, data_info=None, mask=mask), solver.sample(z, steps=steps, order=2, skip_type="time_uniform", method="multistep")
        rel = lambda a, b: ((a.double() - b.double()).norm() / b.double().norm()).item()      # noqa: E731
        extra = {"fp8": fp8, "rel_l2_one_nfe_vs_16bit": rel(e8, e16), f"rel_l2_{steps}_step_sample_vs_16bit": rel(s8, s16)}
        name += f" [fp8 {fp8}]"
    with torch.no_grad():
        ref = sample() if not graph else solver.sample(z, steps=steps, order=2, skip_type="time_uniform", method="multistep")
        first = sample()
        assert not graph or torch.equal(first, ref), "graph replay must reproduce the eager sample bit for bit"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = sample()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    n_kv = None
    flops = 0.0
    for l in range(28):
        nk = N // 4 if (kv and l >= 14) else N
        flops += fwd_flops_per_sample(N, n_kv=nk) / 28      # per-layer share with that layer's key count
    flops_nfe = flops * 2 * bs
    res = {"workload": name + (" [HIP graph]" if graph else ""), "image_size": image_size, "batch": bs, "model_batch": 2 * bs, "tokens": N, "steps": steps,
           "seconds": dt, "denoising_steps_per_s": steps / dt, "images_per_s": bs / dt, "ms_per_nfe": dt / steps * 1e3,
           "TFLOP/s": flops_nfe * steps / dt / 1e12, "mfma_frac": flops_nfe * steps / dt / MFMA_PEAK, "finite": bool(torch.isfinite(out).all()), **extra}
    print(json.dumps(res))
    del m
    torch.cuda.empty_cache()


def sweep_f8(iters=20):
    """One JSON line per (M, N, K): ops.gemm_f8 (16-bit output; for fc1 also the fused GELU + MX output) against ops.gemm on 16-bit operands of the same shape,
    and the activation quantise pass that FP8 adds in front of it.  N(0, 1) data (zero-filled operands read high)."""
    from pixart_sigma_amd import ops
    D = 1152
    names = [("attn.qkv", 3 * D, D), ("attn.proj", D, D), ("cross_attn.q_linear", D, D), ("cross_attn.proj", D, D), ("mlp.fc1", 4 * D, D), ("mlp.fc2", D, 4 * D)]

    def timed(fn):
        for _ in range(3):
            fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(iters):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / iters * 1e3           # microseconds
    for M in (16384, 65536):
        for name, N, K in names:
            g = torch.Generator(device="cuda").manual_seed(N + K)
            a = torch.randn(M, K, device="cuda", generator=g).to(ops.BF16)
            w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(ops.BF16)
            bias = torch.zeros(N, device="cuda")
            act = ops.ACT_GELU if name == "mlp.fc1" else ops.ACT_NONE
            out = torch.empty(M, N, dtype=ops.BF16, device="cuda")
            qa, ea = ops.mx_quant_rows(a)
            qw, ew = ops.mx_quant_rows(w)
            oq, oe = torch.empty(M, N, dtype=ops.FP8, device="cuda"), torch.empty(M, N // 32, dtype=torch.uint8, device="cuda")
            t16 = timed(lambda: ops.gemm(a, w, ops.NT, bias=bias, act=act, out=out))
            t8 = timed(lambda: ops.gemm_f8(qa, ea, qw, ew, bias=bias, act=act, out=out))
            tq = timed(lambda: ops.mx_quant_rows(a, q=qa, e=ea))
            res = {"sweep_f8": name, "M": M, "N": N, "K": K, "gemm_us": t16, "gemm_f8_us": t8, "quant_rows_us": tq, "gemm_TFLOPs": 2e-6 * M * N * K / t16,
                   "gemm_f8_TFLOPs": 2e-6 * M * N * K / t8, "speedup_gemm_only": t16 / t8, "speedup_with_quant_pass": t16 / (t8 + tq),
                   "quant_rows_GBs": M * K * (2 + 1 + 1 / 32) / tq * 1e-3}
            if name == "mlp.fc1":
                res["gemm_f8_mx_out_us"] = timed(lambda: ops.gemm_f8(qa, ea, qw, ew, bias=bias, act=act, out_q=oq, out_e=oe, out16=False))
            print(json.dumps(res), flush=True)
            del a, w, out, qa, ea, qw, ew, oq, oe


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="both")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--graph", action="store_true", help="replay the sampling loop as one HIP graph (DPM_Solver.sample_graphed)")
    ap.add_argument("--fp8", nargs="?", const="mx", default=None, choices=["mx", "dequant"], help="MXFP8 token GEMMs (PixArtMS.enable_fp8)")
    ap.add_argument("--sweep_f8", action="store_true", help="time ops.gemm_f8 against ops.gemm at a block's six GEMM shapes, and the quantise passes; nothing else runs")
    a = ap.parse_args()
    if a.sweep_f8:
        sweep_f8()
        sys.exit(0)
    if a.what in ("256",):
        run("config1-like: XL/2 256px bs1 20-step DPM-Solver++ CFG", 256, 1, a.steps, kv=False, graph=a.graph, fp8=a.fp8)
    if a.what in ("512", "both"):
        run("config2: XL/2 512px bs8 20-step DPM-Solver++ CFG", 512, 8, a.steps, kv=False, graph=a.graph, fp8=a.fp8)
    if a.what in ("2k", "both"):
        run("config4: XL/2 2K bs2 KV-compress(14-27) 20-step DPM-Solver++ CFG", 2048, 2, a.steps, kv=True, graph=a.graph, fp8=a.fp8)
