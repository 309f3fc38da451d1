#!/usr/bin/env python
"""LoRA fine-tuning entry point: the reference's train_scripts/train_pixart_lora_hf.py workflow (freeze the transformer, peft LoRA adapters on its linears,
AdamW on the adapters, `save_pretrained` of the adapters) on the MI355X denoiser, with the conventions of train_scripts/train.py - config file, `--synthetic`,
`--max-steps`, `--mixed-precision`, `--load-from`, the same data paths:

    python train_scripts/train_lora.py <config.py> --load-from base.pth --work-dir output/lora --rank 16 [--lora-alpha 8] [--use-rslora]

The base weights stay frozen (no weight-gradient GEMMs, no optimizer state for them); the adapters (pixart_sigma_amd.lora) are trained with the fused AdamW
and written to `<work-dir>/lora` (and `<work-dir>/checkpoints/lora_step_<n>`) in peft's layout: adapter_config.json + adapter_model.safetensors, loadable by
`scripts/inference.py --lora_path`.  Adapters cover the transformer blocks' linears; the reference's targets outside the blocks, DoRA, dropout, CAME on
adapters and the DreamBooth prior-preservation data path are not implemented (the script says so instead of dropping them).  One GPU per process group has
been run; with more ranks the optimizer checks at construction that every rank holds the same adapters (seed or load them alike)."""
import argparse
import os
import runpy
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def _config_value(path, key, default=None, _seen=()):
    """`key` of a config file, `_base_` parents first (the lookup train.py's _run_config does; needed before train.py - and with it the library - is imported)."""
    path = os.path.abspath(path)
    if path in _seen:
        raise SystemExit(f"{path}: circular _base_")
    ns = runpy.run_path(path)
    val = default
    bases = ns.get("_base_", [])
    for b in ([bases] if isinstance(bases, str) else bases):
        val = _config_value(os.path.join(os.path.dirname(path), b), key, val, _seen + (path,))
    return ns.get(key, val)


def _early_dtype():
    """The operand type is a per-process choice that must be made before pixart_sigma_amd is imported (see train.py)."""
    early = argparse.ArgumentParser(add_help=False)
    early.add_argument("--mixed-precision", default=None)
    mp = early.parse_known_args(sys.argv[1:])[0].mixed_precision
    if mp is None:
        cfgs = [a for a in sys.argv[1:] if a.endswith(".py") and os.path.exists(a)]
        mp = _config_value(cfgs[0], "mixed_precision", "bf16") if cfgs else "bf16"
    if mp not in ("fp16", "bf16"):
        raise SystemExit(f"mixed_precision={mp!r}: this path computes with bf16 or fp16 MFMA operands only")
    if mp == "fp16":
        os.environ["PXA_OPERAND_DTYPE"] = "f16"
    return mp


MIXED_PRECISION = _early_dtype() if __name__ == "__main__" else "bf16"
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import train as T  # noqa: E402
from pixart_sigma_amd import IDDPM, build_model  # noqa: E402
from pixart_sigma_amd.dp import FusedAdamW, LossScaler  # noqa: E402
from pixart_sigma_amd.lora import DEFAULT_TARGETS, LoraConfig  # noqa: E402
from pixart_sigma_amd.lr_schedule import LRSchedule, auto_scale_lr  # noqa: E402


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
    return p.parse_args()


def main():
    a = parse_args()
    cfg = T.load_config(a.config, a.debug)
    cfg["mixed_precision"] = MIXED_PRECISION
    world, rank, local = int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)
    torch.manual_seed(cfg["seed"])                                                 # the same adapters on every rank
    lat, L, B, accum = cfg["image_size"] // 8, cfg["model_max_length"], cfg["train_batch_size"], int(cfg["gradient_accumulation_steps"])
    o = dict(cfg["optimizer"])
    if o.get("type", "AdamW") in ("CAMEWrapper", "CAME"):
        raise SystemExit("CAME on LoRA adapters is not implemented: set optimizer = dict(type='AdamW', ...) (the reference's LoRA scripts train with AdamW)")
    model = build_model(cfg["model"], cfg["grad_checkpointing"], cfg["fp32_attention"], gc_step=cfg["gc_step"], input_size=lat,
                        pe_interpolation=cfg["image_size"] / 512, model_max_length=L, micro_condition=cfg["micro_condition"],
                        kv_compress_config=cfg["kv_compress_config"] if cfg["kv_compress"] else None,
                        pred_sigma=cfg["pred_sigma"], learn_sigma=cfg["learn_sigma"], class_dropout_prob=cfg["class_dropout_prob"])
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
    ratio = 1.0
    if cfg["auto_lr"]:
        o["lr"], ratio = auto_scale_lr(B * world * accum, o["lr"], **cfg["auto_lr"])
    sched = LRSchedule(o["lr"], cfg["lr_schedule"], lr_scale_ratio=ratio, steps_per_call=world,
                       num_training_steps=(cfg["num_steps_per_epoch"] or 0) * cfg["num_epochs"] or None, **(cfg["lr_schedule_args"] or {}))
    scaler = LossScaler(dev) if cfg["mixed_precision"] == "fp16" else None
    opt = FusedAdamW(model, lr=o["lr"], weight_decay=o.get("weight_decay", 1e-2), eps=o.get("eps", 1e-8), betas=o.get("betas", (0.9, 0.999)),
                     max_grad_norm=cfg["gradient_clip"], scaler=scaler)
    c = model._lora.config
    if rank == 0:
        print(f"LoRA r={c.r} alpha={c.lora_alpha} rslora={c.use_rslora} s={c.scaling:g} targets {c.target_modules}: {n_ad:,} trainable of {n_ad + n_base:,} "
              f"parameters ({100 * n_ad / (n_ad + n_base):.3f} %); lr {o['lr']:.3e}, operands {cfg['mixed_precision']}", flush=True)
    diff = IDDPM(str(cfg["train_sampling_steps"]), learn_sigma=cfg["learn_sigma"], pred_sigma=cfg["pred_sigma"], snr=cfg["snr_loss"])
    vae = None
    if not cfg["load_vae_feat"]:
        from pixart_sigma_amd.vae import AutoencoderKL
        have = os.path.isdir(str(cfg["vae_pretrained"]))
        vae = (AutoencoderKL.from_pretrained(cfg["vae_pretrained"], torch_dtype=torch.float16) if have else AutoencoderKL(scaling_factor=cfg["scale_factor"])).to(dev)
        cfg["scale_factor"] = vae.config.scaling_factor
    os.makedirs(os.path.join(a.work_dir, "checkpoints"), exist_ok=True)
    use_ds = bool(cfg["data_root"]) and not a.synthetic and os.path.exists(os.path.join(cfg["data_root"], "data_info.json"))
    pictures, captions = T.pictures_mode(cfg, a.synthetic), None                   # pictures (and text) instead of feature files, as in train.py
    if pictures:
        it, captions = T.picture_batches(cfg, B, L, dev, rank, world, vae)
    else:
        it = T.feature_batches(cfg, B, L, dev, rank, world) if use_ds else T.batches(cfg, B, lat, L, dev, rank, world, a.synthetic)
    t0, step = time.time(), 0
    while a.max_steps is None or step < a.max_steps:
        opt.zero_grad()
        opt.lr = sched.lr
        for micro in range(accum):
            batch = next(it)
            z, y, mask = batch[:3]
            info = batch[3] if len(batch) > 3 else {"img_hw": torch.tensor([[z.shape[-2] * 8.0, z.shape[-1] * 8.0]] * z.shape[0]),
                                                    "aspect_ratio": torch.tensor([[z.shape[-2] / z.shape[-1]]] * z.shape[0])}
            if pictures:                                                           # x0 comes out of the iterator, scale factor included
                x0 = z
            else:
                if vae is not None:
                    z = vae.encode(z).latent_dist.sample().float()
                x0 = z * cfg["scale_factor"]
            t = torch.randint(0, cfg["train_sampling_steps"], (z.shape[0],), device=dev).long()
            loss = diff.training_losses(model, x0, t, model_kwargs=dict(y=y, mask=mask, data_info=info))["loss"].mean() / accum
            if micro + 1 < accum:
                with opt.reducer.no_sync():
                    (scaler.scale(loss) if scaler else loss).backward()
            else:
                (scaler.scale(loss) if scaler else loss).backward()
        opt.step()
        sched.step()
        step += 1
        if step % cfg["log_interval"] == 0 and rank == 0:
            extra = f" loss_scale {scaler.value:g} skipped {scaler.steps_skipped}" if scaler else ""
            print(f"step {step} loss {loss.item() * accum:.4f} grad_norm {opt.last_norm.item():.4f} lr {opt.lr:.3e}{extra} "
                  f"{(time.time() - t0) / cfg['log_interval']:.3f} s/step", flush=True)
            t0 = time.time()
        if step % cfg["save_model_steps"] == 0 and rank == 0:
            model.save_lora(os.path.join(a.work_dir, "checkpoints", f"lora_step_{step}"))
    if rank == 0:
        model.save_lora(os.path.join(a.work_dir, "lora"))
        print(f"finished at step {step}: loss {loss.item() * accum:.4f} grad_norm {opt.last_norm.item():.4f}; adapters in {os.path.join(a.work_dir, 'lora')}", flush=True)
    if captions is not None:
        captions.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
