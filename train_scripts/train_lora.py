#!/usr/bin/env python
"""LoRA fine-tuning entry point: the reference's train_scripts/train_pixart_lora_hf.py workflow (freeze the transformer, peft LoRA adapters on its linears,
AdamW on the adapters, `save_pretrained` of the adapters) on the MI355X denoiser, with the conventions of train_scripts/train.py - config file, `--synthetic`,
`--max-steps`, `--mixed-precision`, `--load-from`, the same data paths:

    python train_scripts/train_lora.py <config.py> --load-from base.pth --work-dir output/lora --rank 16 [--lora-alpha 8] [--use-rslora]

The base weights stay frozen (no weight-gradient GEMMs, no optimizer state for them); the adapters (pixart_sigma_amd.lora) are trained with the fused AdamW
and written to `<work-dir>/lora` (and `<work-dir>/checkpoints/lora_step_<n>`) in peft's layout: adapter_config.json + adapter_model.safetensors, loadable by
`scripts/inference.py --lora_path`.  Adapters cover the transformer blocks' linears; the reference's targets outside the blocks, DoRA, dropout, CAME on
adapters and the DreamBooth prior-preservation data path are not implemented (the script says so instead of dropping them).  One GPU per process group has
been run; with more ranks the optimizer checks at construction that every rank holds the same adapters (seed or load them alike).

`--ema [--ema-rate X]` keeps an exponential moving average of the ADAPTERS (pixart_sigma_amd.ema.WeightEMA on the adapters' store) and writes it beside every
adapter directory: `<work-dir>/lora_ema` and `<work-dir>/checkpoints/lora_ema_step_<n>`, the same peft layout; `--resume-lora DIR` then starts the average from
`DIR_ema` when that exists.  `--visualize [--validation-feats DIR]` writes validation pictures as train.py does."""
import argparse
import os
import sys

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from config_file import early_mixed_precision  # noqa: E402

MIXED_PRECISION = early_mixed_precision(sys.argv[1:]) if __name__ == "__main__" else "bf16"   # before train.py imports the library: see config_file.py
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import train as T  # noqa: E402
from pixart_sigma_amd import IDDPM  # noqa: E402
from pixart_sigma_amd.dp import FusedAdamW, LossScaler  # noqa: E402
from pixart_sigma_amd.lora import DEFAULT_TARGETS, LoraConfig  # noqa: E402


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("config", nargs="?", default=None)
    p.add_argument("--work-dir", "--work_dir", default="output/lora")
    p.add_argument("--load-from", default=None, help="base model checkpoint (PixArt .pth); random init without it (smoke runs)")
    p.add_argument("--resume-lora", default=None, help="adapter directory to continue from (its rank / targets win)")
    p.add_argument("--debug", action="store_true")
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--max-steps", type=int, default=None)
    p.add_argument("--mixed-precision", choices=["fp16", "bf16"], default=None, help="overrides the config's mixed_precision")
    p.add_argument("--rank", type=int, default=16, help="LoRA rank, 1..64 (train_pixart_lora_hf.py --rank)")
    p.add_argument("--lora-alpha", type=float, default=8, help="peft's default; the reference passes only the rank")
    p.add_argument("--use-rslora", action="store_true", help="s = alpha / sqrt(r)")
    p.add_argument("--target-modules", nargs="+", default=list(DEFAULT_TARGETS), help="diffusers module names or suffixes inside the transformer blocks")
    p.add_argument("--lr", type=float, default=None, help="overrides the config's optimizer lr (the reference LoRA script defaults to 1e-6 ... 1e-4)")
    T.add_ema_visualize_args(p)
    return p.parse_args()


def read_adapters(path):
    """An adapter directory's tensors under the adapters' internal names and orientation (lora_B transposed), for WeightEMA.load_state_dict."""
    from safetensors.torch import load_file
    from pixart_sigma_amd.lora import internal_name
    out = {}
    for k, v in load_file(os.path.join(path, "adapter_model.safetensors")).items():
        n = internal_name(k)
        out[n] = v.t() if n.endswith("lora_Bt") else v
    return out


def main():
    a = parse_args()
    cfg = T.load_config(a.config, a.debug)
    cfg["mixed_precision"] = MIXED_PRECISION
    decay = T.ema_decay(a, cfg)
    prompts = T.check_visualize(a, cfg, T.pictures_mode(cfg, a.synthetic) and not cfg["load_t5_feat"])
    world, rank, dev = T.init_process()
    torch.manual_seed(cfg["seed"])                                                 # the same adapters on every rank
    lat, L, B, accum = cfg["image_size"] // 8, cfg["model_max_length"], cfg["train_batch_size"], int(cfg["gradient_accumulation_steps"])
    o = dict(cfg["optimizer"])
    if o.get("type", "AdamW") in ("CAMEWrapper", "CAME"):
        raise SystemExit("CAME on LoRA adapters is not implemented: set optimizer = dict(type='AdamW', ...) (the reference's LoRA scripts train with AdamW)")
    model = T.build_denoiser(cfg)
    if a.load_from:
        sd = torch.load(a.load_from, map_location="cpu", weights_only=False)
        model.load_state_dict(sd.get("state_dict", sd), strict=False)
    elif rank == 0:
        print("no --load-from: adapters on a randomly initialised base model", flush=True)
    if a.resume_lora:
        model.load_lora(a.resume_lora)
    else:
        model.add_lora(LoraConfig(r=a.rank, lora_alpha=a.lora_alpha, use_rslora=a.use_rslora, target_modules=a.target_modules))
    model = model.to(dev).train()
    model.prepare(dev)
    n_ad, n_base = sum(p.numel() for p in model.lora_parameters()), sum(p.numel() for p in model.parameters())
    if a.lr is not None:
        o["lr"] = a.lr
    sched, _ = T.make_schedule(cfg, o, B, world, accum)
    scaler = LossScaler(dev) if cfg["mixed_precision"] == "fp16" else None
    opt = FusedAdamW(model, lr=o["lr"], weight_decay=o.get("weight_decay", 1e-2), eps=o.get("eps", 1e-8), betas=o.get("betas", (0.9, 0.999)),
                     max_grad_norm=cfg["gradient_clip"], scaler=scaler)
    c = model._lora.config
    if rank == 0:
        print(f"LoRA r={c.r} alpha={c.lora_alpha} rslora={c.use_rslora} s={c.scaling:g} targets {c.target_modules}: {n_ad:,} trainable of {n_ad + n_base:,} "
              f"parameters ({100 * n_ad / (n_ad + n_base):.3f} %); lr {o['lr']:.3e}, operands {cfg['mixed_precision']}", flush=True)
    ema = None
    if decay is not None:
        from pixart_sigma_amd.ema import WeightEMA
        ema = WeightEMA(model, decay, scaler=scaler)            # over the adapters; starts as a copy of them
        ema_dir = a.resume_lora.rstrip("/") + "_ema" if a.resume_lora else None
        if ema_dir and os.path.isdir(ema_dir):
            ema.load_state_dict(read_adapters(ema_dir))
        elif a.resume_lora and rank == 0:
            print(f"resume: no {ema_dir}; the EMA starts from the loaded adapters", flush=True)
        if rank == 0:
            print(f"EMA of the adapters at rate {decay:g}", flush=True)
    diff = IDDPM(str(cfg["train_sampling_steps"]), learn_sigma=cfg["learn_sigma"], pred_sigma=cfg["pred_sigma"], snr=cfg["snr_loss"])
    vae = T.load_vae(cfg, dev)
    os.makedirs(os.path.join(a.work_dir, "checkpoints"), exist_ok=True)
    it, captions = T.data_source(cfg, a.synthetic, B, lat, L, dev, rank, world, vae)   # pictures (and text) or feature files, as in train.py
    validate = T.make_validate(a, cfg, model, vae, captions, dev, prompts, ema) if prompts and rank == 0 else None

    def save(path, path_ema):
        model.save_lora(path)
        if ema is not None:
            with ema.swapped():                                 # the adapters' parameters hold the average here: the same writer, the same layout
                model.save_lora(path_ema)
    ck = os.path.join(a.work_dir, "checkpoints")
    step, loss = T.train_loop(cfg, model, diff, opt, sched, scaler, it, dev, rank, world, 0, a.max_steps,
                              lambda step: save(os.path.join(ck, f"lora_step_{step}"), os.path.join(ck, f"lora_ema_step_{step}")), ema=ema, validate=validate)
    if rank == 0:
        save(os.path.join(a.work_dir, "lora"), os.path.join(a.work_dir, "lora_ema"))
        print(f"finished at step {step}: loss {loss.item():.4f} grad_norm {opt.last_norm.item():.4f}; adapters in {os.path.join(a.work_dir, 'lora')}", flush=True)
    if captions is not None:
        captions.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
