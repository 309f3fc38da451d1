"""LoRA fine-tuning step against the full fine-tuning step of the same build, in one process on one GPU: PixArt-Sigma-XL/2 at 1024px, batch 16, L = 300
(bench.py's flagship workload and its warm-up / step counts), adapters of rank 16 on all ten block linears.  Also: pxa_lora_bwd alone at the two large
shapes of that step, and one full re-merge of all adapters (what every optimizer step pays).  Prints one JSON line.

    python tools/bench_lora.py [--steps 5] [--warmup 2] [--dtype fp16|bf16] [--rank 16] [--no-step] [--no-kernels]

bytes of x + dy over time is reported as a fraction of the 6.29 TB/s device copy rate (MI355X_MICROARCH.md); the gradient kernel reads x and dy a second
time by design (csrc/lora.hip), from the Infinity Cache when the row chunking works - a counter run of its own (tools/pmc_*.sh style) says how often."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LTXT, COPY_RATE = 300, 6.29e12


def _events(fn, iters, warm=3):
    import torch
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def bench_kernels(rank):
    import torch
    from pixart_sigma_amd import ops
    out = {}
    g = torch.Generator().manual_seed(0)
    for M, K, N in ((65536, 1152, 3456), (65536, 4608, 1152)):
        x = torch.randn(M, K, generator=g).to("cuda", ops.BF16)
        dy = (torch.randn(M, N, generator=g) * 0.05).to("cuda", ops.BF16)
        A16 = (torch.randn(rank, K, generator=g) / rank).to("cuda", ops.BF16)
        Bt16 = (torch.randn(rank, N, generator=g) * 0.05).to("cuda", ops.BF16)
        dA, dBt = torch.zeros(rank, K, device="cuda"), torch.zeros(rank, N, device="cuda")
        ms = _events(lambda: ops.lora_bwd(x, dy, A16, Bt16, 0.5, dA, dBt), 20)
        nbytes = 2 * M * (K + N)
        # the weight-gradient GEMM + bias column sum this call replaces
        dw, db = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda")
        ms_dw = _events(lambda: (ops.gemm(dy, x, ops.TN, out_f32=dw, accumulate=True, split_k=0), ops.colsum(dy, db)), 10)
        out[f"lora_bwd_M{M}_K{K}_N{N}_r{rank}"] = {"ms": ms, "x_dy_bytes": nbytes, "x_dy_TBps": nbytes / ms / 1e9, "fraction_of_copy_rate": nbytes / (ms * 1e-3) / COPY_RATE,
                                                   "dW_gemm_plus_colsum_ms": ms_dw, "finite": bool(torch.isfinite(dA).all() and torch.isfinite(dBt).all())}
        del x, dy, dw
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--image-size", type=int, default=1024)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="fp16")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    a = ap.parse_args()
    if a.dtype == "fp16":
        os.environ["PXA_OPERAND_DTYPE"] = "f16"
    import torch
    from pixart_sigma_amd import IDDPM, PixArtMS_XL_2
    from pixart_sigma_amd.dp import FusedAdamW, LossScaler
    from pixart_sigma_amd.lora import BLOCK_MODULES, LoraConfig
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"workload": f"PixArt-Sigma-XL/2 {a.image_size}px bs{a.batch} L{LTXT}", "dtype": a.dtype, "rank": a.rank, "steps": a.steps, "warmup": a.warmup}
    if not a.no_kernels:
        out["kernels"] = bench_kernels(a.rank)
    if not a.no_step:
        lat, B = a.image_size // 8, a.batch
        torch.manual_seed(0)
        model = PixArtMS_XL_2(input_size=lat, pe_interpolation=a.image_size / 512, model_max_length=LTXT, class_dropout_prob=0.0)
        with torch.no_grad():                                 # as bench.py: no numerically dead branch
            for blk in model.blocks:
                blk.cross_attn.proj.weight.normal_(std=0.02)
            model.final_layer.linear.weight.normal_(std=0.02)
        model = model.to(dev).train()
        model.prepare(dev)
        diff = IDDPM(str(1000), learn_sigma=True, pred_sigma=True, snr=False)
        g = torch.Generator(device="cpu").manual_seed(1234)
        x0, noise = torch.randn(B, 4, lat, lat, generator=g).to(dev), torch.randn(B, 4, lat, lat, generator=g).to(dev)
        y = torch.randn(B, 1, LTXT, 4096, generator=g).to(dev)
        t = torch.randint(0, 1000, (B,), generator=g).to(dev)
        mask = torch.ones(B, LTXT, dtype=torch.int64)

        def run(label):
            scaler = LossScaler(dev) if a.dtype == "fp16" else None
            opt = FusedAdamW(model, lr=2e-5, weight_decay=3e-2, eps=1e-10, max_grad_norm=0.01, scaler=scaler)

            def step():
                opt.zero_grad()
                loss = diff.training_losses(model, x0, t, model_kwargs=dict(y=y, mask=mask, data_info=None), noise=noise)["loss"].mean()
                (scaler.scale(loss) if scaler is not None else loss).backward()
                opt.step()
                return loss
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            for _ in range(a.warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = step()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / a.steps
            out[label] = {"ms_per_step": dt * 1e3, "steps_per_s": 1 / dt, "peak_memory_GB": torch.cuda.max_memory_allocated() / 1e9, "final_loss": float(loss.item()),
                          "optimizer_state_GB": (opt.m.numel() + opt.v.numel()) * 4 / 1e9, "trainable_parameters": opt.store.total}
            opt.reducer.close()

        run("full_finetune")
        lo = model.add_lora(LoraConfig(r=a.rank, target_modules=list(BLOCK_MODULES)))
        with torch.no_grad():                                 # B != 0: the adapters' own gradients are all live
            for n, p in lo.params.items():
                if n.endswith("lora_Bt"):
                    p.normal_(std=0.01)
        model.prepare(dev)
        run("lora")
        out["lora_step_over_full_step"] = out["lora"]["ms_per_step"] / out["full_finetune"]["ms_per_step"]
        out["remerge_all_adapters_ms"] = _events(model._engine._lora_merge, 10)
        out["adapted_slices"] = sum(len(v) for v in lo.slices.values())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
