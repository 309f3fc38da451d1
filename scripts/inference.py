#!/usr/bin/env python
"""Text-to-image sampling entry point with the reference's CLI (reference scripts/inference.py:24-44), on the MI355X
denoiser.  The frozen side nets are outside this repo's scope: captions are read as
precomputed T5 features (tools/extract_features.py format: .npz with `caption_feature` (1,L,4096) and `attention_mask`
(1,L)) from `--caption_feats`, made from the prompts by the in-repo T5 encoder with `--t5_path DIR` (tools/extract_t5_features.py in a child process of its
own: T5 runs under the bf16 operand build and its 9.5 GB of weights are gone before the denoiser loads), or drawn at random with `--synthetic`; latents are decoded by the HIP VAE
(pixart_sigma_amd.vae.AutoencoderKL, reference inference.py:136,191-196) when the diffusers-format `vae/` directory exists, else
saved as latents (`--random_vae` decodes with a random-init VAE: plumbing / timing runs without weights).

Fixes relative to the reference script: `--kv_compress*` reaches the model constructor, and
batch size 1 no longer indexes an empty prompt list.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# The reference samples with fp16 weights for both the denoiser and the VAE (scripts/inference.py:191-196 `weight_dtype = torch.float16`),
# so this entry point defaults to the fp16-operand build of the kernels (forward parity <= 1e-3 incl. the VAE at 1.5e-3..2.0e-3; the bf16
# build sits at 3e-3 / 1.4e-2).  The operand type is a per-process choice made before the package is imported: --dtype bf16 overrides.
_early = argparse.ArgumentParser(add_help=False)               # both `--dtype bf16` and `--dtype=bf16`
_early.add_argument("--dtype", default="fp16")
_dt = _early.parse_known_args(sys.argv[1:])[0].dtype
if _dt not in ("fp16", "bf16"):
    raise SystemExit(f"--dtype must be fp16 or bf16, got {_dt!r}")
os.environ["PXA_OPERAND_DTYPE"] = "f16" if _dt == "fp16" else "bf16"
from pixart_sigma_amd import DPMS, IDDPM, PixArtMS_XL_2, SASolverSampler  # noqa: E402


def get_args():
    p = argparse.ArgumentParser()
    p.add_argument("--image_size", default=1024, type=int)
    p.add_argument("--version", default="sigma", type=str)
    p.add_argument("--pipeline_load_from", default="output/pretrained_models/pixart_sigma_sdxlvae_T5_diffusers", type=str)
    p.add_argument("--txt_file", default="asset/samples.txt", type=str)
    p.add_argument("--caption_feats", default=None, type=str, help="dir of <idx>.npz T5 features (one per prompt line)")
    p.add_argument("--model_path", default=None, type=str, help=".pth checkpoint in the reference's format (random init if omitted)")
    p.add_argument("--sdvae", action="store_true")
    p.add_argument("--random_vae", action="store_true")
    p.add_argument("--bs", default=1, type=int)
    p.add_argument("--cfg_scale", default=4.5, type=float)
    p.add_argument("--sampling_algo", default="dpm-solver", type=str, choices=["iddpm", "dpm-solver", "sa-solver"])
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--dataset", default="custom", type=str)
    p.add_argument("--step", default=-1, type=int)
    p.add_argument("--save_name", default="test_sample", type=str)
    p.add_argument("--kv_compress", action="store_true")
    p.add_argument("--kv_compress_sampling", default="conv")
    p.add_argument("--kv_compress_scale", default=2, type=int)
    p.add_argument("--kv_compress_layers", default="14-27")
    p.add_argument("--synthetic", action="store_true", help="random caption features (plumbing check without T5 weights)")
    p.add_argument("--t5_path", default=None, type=str, help="transformers T5 directory (weights + tokenizer): encode the prompts with the in-repo T5 encoder first")
    p.add_argument("--t5_weight_dtype", default=None, choices=["fp8_e4m3"], help="with --t5_path: hold the T5 encoder's matrices as FP8 e4m3 (default: as stored)")
    p.add_argument("--t5_timeout", default=1800, type=int, help="seconds the T5 child process may take")
    p.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"], help="MFMA operand type of the whole process (reference: fp16)")
    p.add_argument("--lora_path", default=None, type=str, help="peft-format adapter directory (adapter_config.json + adapter_model.safetensors) for the transformer blocks")
    p.add_argument("--lora_scale", default=1.0, type=float, help="multiplies the adapters' lora_alpha / r (0 = the base model)")
    p.add_argument("--dit_fp8", nargs="?", const="mx", default=None, choices=["mx", "dequant"],
                   help="run the six token GEMMs of every denoiser block on MXFP8 operands (PixArtMS.enable_fp8): mx = the block-scaled FP8 MFMA GEMM, "
                        "dequant = the same quantised operands through the 16-bit GEMM (A/B reference).  Adapters of --lora_path are merged first")
    p.add_argument("--load_ema", action="store_true", help="with --model_path: sample from the checkpoint's state_dict_ema (written by train.py --ema)")
    p.add_argument("--save_images", default=None, choices=["png", "jpg"], help="also write one picture per sample (as the reference's save_image: output/<save_name>/<index>.<ext>)")
    return p.parse_args()


def load_captions(args, n, L, dev, first=0):
    """Features and masks of prompts first .. first + n - 1 (files <idx>.npz of --caption_feats) and the null caption's features."""
    if args.synthetic:
        g = torch.Generator().manual_seed(args.seed)
        return torch.randn(n, 1, L, 4096, generator=g).to(dev), torch.ones(n, L, dtype=torch.int64), torch.randn(1, 1, L, 4096, generator=g).to(dev)
    import numpy as np
    feats, masks = [], []
    for i in range(n):
        z = np.load(os.path.join(args.caption_feats, f"{first + i}.npz"))
        feats.append(torch.from_numpy(z["caption_feature"]).float().reshape(1, 1, -1, z["caption_feature"].shape[-1])[:, :, :L])
        masks.append(torch.from_numpy(z["attention_mask"]).reshape(1, -1)[:, :L])
    null = np.load(os.path.join(args.caption_feats, "null.npz"))
    return torch.cat(feats).to(dev), torch.cat(masks), torch.from_numpy(null["caption_feature"]).float().reshape(1, 1, -1, null["caption_feature"].shape[-1])[:, :, :L].to(dev)


def t5_child_command(args, prompts_file, out_dir, L):
    """The command line of the T5 child process of --t5_path (tools/extract_t5_features.py)."""
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "extract_t5_features.py")
    cmd = [sys.executable, tool, "--t5_path", args.t5_path, "--prompts", prompts_file, "--out", out_dir, "--max_length", str(L)]
    return cmd + (["--weight_dtype", args.t5_weight_dtype] if getattr(args, "t5_weight_dtype", None) else [])


def encode_prompts(args, prompts, L):
    """--t5_path: caption features of `prompts` into output/<save_name>/caption_feats by a fresh child process, BEFORE this process touches the GPU (one operand
    build per process: the child pins bf16, this one defaults to fp16; and the T5 weights do not stay resident beside the denoiser).  Returns the directory."""
    import subprocess
    out_dir = os.path.join("output", args.save_name, "caption_feats")
    os.makedirs(out_dir, exist_ok=True)
    prompts_file = os.path.join(out_dir, "prompts.txt")
    with open(prompts_file, "w") as f:
        f.write("\n".join(prompts) + "\n")
    env = dict(os.environ, PXA_OPERAND_DTYPE="bf16")
    env.pop("PXA_LIB_PATH", None)
    r = subprocess.run(t5_child_command(args, prompts_file, out_dir, L), env=env, timeout=args.t5_timeout)
    if r.returncode != 0:
        raise SystemExit(f"--t5_path: the T5 encoder process failed (exit {r.returncode})")
    return out_dir


def checkpoint_weights(sd, path, load_ema):
    """The weights to sample from: state_dict (or the file itself), or with --load_ema the averaged ones."""
    if not load_ema:
        return sd.get("state_dict", sd)
    if not isinstance(sd, dict) or "state_dict_ema" not in sd:
        raise SystemExit(f"{path}: the checkpoint has no state_dict_ema (it was written without --ema): --load_ema cannot take its weights from it")
    return sd["state_dict_ema"]


@torch.no_grad()
def main():
    args = get_args()
    L = {"alpha": 120, "sigma": 300}[args.version]
    prompts = [ln.strip() for ln in open(args.txt_file)] if os.path.exists(args.txt_file) else [f"prompt {i}" for i in range(args.bs)]
    if args.t5_path and not args.synthetic:
        args.caption_feats = encode_prompts(args, prompts, L)
    dev = torch.device("cuda")
    torch.manual_seed(args.seed)
    latent = args.image_size // 8
    steps = args.step if args.step > 0 else {"iddpm": 100, "dpm-solver": 20, "sa-solver": 25}[args.sampling_algo]           # reference inference.py:159-160
    kvc = None
    if args.kv_compress:
        lo, hi = (int(v) for v in args.kv_compress_layers.split("-"))
        kvc = {"sampling": args.kv_compress_sampling, "scale_factor": args.kv_compress_scale, "kv_compress_layer": list(range(lo, hi + 1))}
    model = PixArtMS_XL_2(input_size=latent, pe_interpolation=args.image_size / 512, model_max_length=L, kv_compress_config=kvc,
                          micro_condition=(args.version == "alpha" and args.image_size == 1024))
    if args.model_path:
        sd = torch.load(args.model_path, map_location="cpu")
        model.load_state_dict(checkpoint_weights(sd, args.model_path, args.load_ema), strict=False)
    elif args.load_ema:
        raise SystemExit("--load_ema needs --model_path")
    if args.lora_path:                  # folded into the 16-bit operand weights when the model is prepared: the sampler runs the unchanged kernels
        lo = model.load_lora(args.lora_path, scale=args.lora_scale)
        print(f"LoRA adapters from {args.lora_path}: r={lo.config.r}, s={lo.scale:g}, {len(lo.params) // 2} adapted linears")
    model = model.to(dev).eval()
    if args.dit_fp8:
        if args.lora_path:              # FP8 quantises the merged weights: there is no adapter path beside an FP8 GEMM
            model.merge_and_unload()
        model.enable_fp8(args.dit_fp8)
        print(f"denoiser token GEMMs on MXFP8 operands ({args.dit_fp8})")
    from pixart_sigma_amd.vae import AutoencoderKL
    vae_dir = "output/pretrained_models/sd-vae-ft-ema" if args.sdvae else f"{args.pipeline_load_from}/vae"    # reference inference.py:191-196
    vae = None
    if os.path.isdir(vae_dir):
        vae = AutoencoderKL.from_pretrained(vae_dir).to(dev).to(torch.float16)
    elif args.random_vae:
        vae = AutoencoderKL(scaling_factor=0.18215 if args.sdvae else 0.13025).to(dev).to(torch.float16)
    os.makedirs(os.path.join("output", args.save_name), exist_ok=True)
    for start in range(0, len(prompts), args.bs):
        chunk = prompts[start:start + args.bs]                      # bs == 1 works (reference indexes prompts[0] before appending)
        n = len(chunk)
        y, mask, null_y = load_captions(args, n, L, dev, first=start if args.t5_path else 0)      # --t5_path wrote one file per prompt line
        hw = torch.tensor([[args.image_size, args.image_size]] * n, dtype=torch.float, device=dev)
        ar = torch.ones(n, 1, device=dev)
        z = torch.randn(n, 4, latent, latent, device=dev)
        if args.sampling_algo == "iddpm":                            # reference inference.py:89-101: ancestral sampling, batch = [cond ; null]
            z2 = z.repeat(2, 1, 1, 1)
            kw = dict(y=torch.cat([y, null_y.repeat(n, 1, 1, 1)]), cfg_scale=args.cfg_scale, data_info={"img_hw": hw, "aspect_ratio": ar}, mask=mask)
            samples = IDDPM(str(steps)).p_sample_loop(model.forward_with_cfg, z2.shape, z2, clip_denoised=False, model_kwargs=kw, device=dev)
            samples, _ = samples.chunk(2, dim=0)
        elif args.sampling_algo == "sa-solver":                      # reference inference.py:119-133: 25 steps, eta = 1
            sa = SASolverSampler(model.forward_with_dpmsolver, device=dev)
            samples = sa.sample(S=steps, batch_size=n, shape=(4, latent, latent), eta=1, conditioning=y, unconditional_conditioning=null_y.repeat(n, 1, 1, 1),
                                unconditional_guidance_scale=args.cfg_scale, model_kwargs=dict(data_info={"img_hw": hw, "aspect_ratio": ar}, mask=mask), x_T=z)[0]
        else:
            dpms = DPMS(model.forward_with_dpmsolver, condition=y, uncondition=null_y.repeat(n, 1, 1, 1), cfg_scale=args.cfg_scale,
                        model_kwargs=dict(data_info={"img_hw": hw, "aspect_ratio": ar}, mask=mask))
            samples = dpms.sample(z, steps=steps, order=2, skip_type="time_uniform", method="multistep")
        if vae is not None:
            imgs = vae.decode(samples.half() / vae.config.scaling_factor).sample
            torch.save(imgs.cpu(), os.path.join("output", args.save_name, f"images_{start}.pt"))
            if args.save_images:                                     # reference inference.py:137: save_image(normalize=True, value_range=(-1, 1))
                from pixart_sigma_amd.data.images import save_png
                for i in range(n):
                    save_png(imgs[i], os.path.join("output", args.save_name, f"{start + i}.{args.save_images}"))
        else:
            torch.save(samples.cpu(), os.path.join("output", args.save_name, f"latents_{start}.pt"))
        print(f"[{start}:{start + n}] sampled {tuple(samples.shape)} in {steps} steps")


if __name__ == "__main__":
    main()
