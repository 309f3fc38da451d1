#!/usr/bin/env python
"""Training entry point with the reference's launch shape (reference train_scripts/train.py:244-296:
`python -m torch.distributed.run --nproc_per_node=N train_scripts/train.py <config.py> --work-dir ... [--load-from ...]
[--resume-from ...] [--debug]`), driving the MI355X denoiser + fused AdamW + overlapped RCCL all-reduce.

Data, chosen by the config (top-level `load_vae_feat` / `load_t5_feat`, else those of its `data` dict, as in the reference's configs):
  * feature files (load_vae_feat = True, the default): precomputed features in the reference's layout (tools/extract_features.py: `<name>.npy` =
    cat[mean, std] latent, `<name>.npz` = caption_feature + attention_mask) listed in `config.data_root`, or `--synthetic`;
  * pictures and text (load_vae_feat = False, load_t5_feat = False: every PixArt-Sigma config): pictures and caption strings of `data_info.json`, the latents
    from the HIP VAE and the caption features from the HIP T5 encoder inside every step, as in reference train.py:144-168 - pixart_sigma_amd.data.pipeline
    (PictureBatches) keeps one batch ahead of the step; `t5_path` names the T5 directory, `real_prompt_ratio` mixes in the sharegpt4v captions.  Under
    mixed_precision = 'fp16' the T5 encoder, which needs bf16 operands, runs in a worker process per rank (pixart_sigma_amd.t5.captions);
  * pictures and caption feature files (load_vae_feat = False, load_t5_feat = True).
With `load_vae_feat = False` and `--synthetic` (or no data_root) the batches are noise images and the latents come from the HIP VAE on the fly
(`vae_pretrained` = a diffusers AutoencoderKL directory; a random-init VAE when it is absent).  tensorboard/wandb trackers are outside this repo's scope
(SURVEY.md section 2): the config is a plain Python file (with mmcv's `_base_` inheritance) whose module-level names are the keys of section 5 of the survey.

Opt-in, off by default (a run without these flags makes the launches and files it made before they existed):
  * `--ema [--ema-rate X]`: an exponential moving average of the weights (pixart_sigma_amd.ema.WeightEMA) at the config's `ema_rate`, updated behind every
    optimizer step and written as `state_dict_ema` beside `state_dict` (the reference's checkpoint layout); `--load-ema` starts from a checkpoint's
    `state_dict_ema`;
  * `--visualize`: validation pictures of the config's `validation_prompts` after step 1 and every `eval_sampling_steps` steps (reference train.py:45-103,
    225-228) into `<work-dir>/validation/step_<n>[_ema]/<i>.png`; caption features from `--validation-feats DIR` or, with text captions, from the T5 encoder.
"""
import argparse
import glob
import os
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # RCCL across processes needs dmabuf IPC on this driver; set before the HIP runtime starts

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from config_file import early_mixed_precision, run_config  # noqa: E402

MIXED_PRECISION = early_mixed_precision(sys.argv[1:]) if __name__ == "__main__" else "bf16"   # before the library is imported: see config_file.py
from pixart_sigma_amd import IDDPM, build_model  # noqa: E402
from pixart_sigma_amd.dp import FusedAdamW, FusedCAME, LossScaler  # noqa: E402
from pixart_sigma_amd.lr_schedule import LRSchedule, auto_scale_lr  # noqa: E402

DEFAULTS = dict(model="PixArtMS_XL_2", image_size=1024, train_batch_size=16, num_epochs=1, model_max_length=300, pred_sigma=True,
                learn_sigma=True, class_dropout_prob=0.1, kv_compress=False, kv_compress_config=None, micro_condition=False,
                grad_checkpointing=False, fp32_attention=False, gc_step=1, scale_factor=0.13025, gradient_clip=0.01,
                optimizer=dict(type="AdamW", lr=2e-5, weight_decay=3e-2, eps=1e-10), train_sampling_steps=1000, snr_loss=False,
                log_interval=20, save_model_steps=1000, seed=43, data_root=None, load_vae_feat=True,
                # pictures instead of feature files (reference train.py:144-168): see load_config for the `data` dict of the reference's configs
                load_t5_feat=True, sample_posterior=True, t5_path="output/pretrained_models/pixart_sigma_sdxlvae_T5_diffusers/text_encoder", num_workers=4,
                t5_weight_dtype=None,                  # "fp8_e4m3": the T5 encoder of text captions holds its matrices as FP8 (quantised while loading)
                real_prompt_ratio=1.0, image_list_json="data_info.json", data_type=None, data_subdir=None,
                vae_pretrained="output/pretrained_models/pixart_sigma_sdxlvae_T5_diffusers/vae",
                # schedule / scaling keys of the reference configs (configs/PixArt_xl2_internal.py:34-57)
                gradient_accumulation_steps=1, auto_lr=None, lr_schedule="constant", lr_schedule_args=dict(num_warmup_steps=0),
                mixed_precision="bf16", aspect_ratio_type=None, valid_num=0, num_steps_per_epoch=None,
                # read only under --ema / --visualize (the config keys alone switch nothing on, as in the reference's Sigma train.py, which keeps no EMA
                # whatever ema_rate says): the EMA decay (0.9999 when None), the prompts of the validation pictures and the interval between them
                ema_rate=None, validation_prompts=None, eval_sampling_steps=250)
# keys of reference configs that name subsystems outside this path and cannot change what is trained: accepted and ignored.
# Anything else that is not in DEFAULTS raises: a recognised-but-unsupported option must not silently change what is trained.
# `visualize`: every Sigma config sets it, so the key alone stays without effect - validation pictures are switched on by --visualize.
IGNORED_KEYS = {"work_dir", "visualize", "resume_from", "load_from",
                "save_model_epochs", "window_block_indexes", "window_size", "use_rel_pos", "lewei_scale", "pe_interpolation", "roots",
                "tracker_project_name", "name", "num_ddim_timesteps", "w_max", "w_min", "cfg_scale", "eval_metric", "max_length",
                # the rest of configs/PixArt_xl2_internal.py, which every PixArt-Sigma config inherits: validation, logging and storage settings, and two
                # names (lora_rank, num_group_tokens) the reference's train.py never reads
                "eval_batch_size", "deterministic_validation", "save_image_epochs", "tensorboard_mox_interval", "s3_work_dir", "lora_rank", "num_group_tokens"}
# keys that DO change what is trained and that this path implements for one value only: that value (or absence) is accepted, anything else refused
# (real_prompt_ratio is checked in load_config: any value in [0, 1] when captions are text, 1.0 only with caption feature files).
SEMANTIC_KEYS = {"qk_norm": (False,), "mask_loss_coef": (0.0, 0), "mask_type": ("null", None), "load_mask_index": (False,),
                 "loss_type": (None, "mse", "l2", "huber"), "huber_c": None, "ema_decay": None, "skip_step": (0,), "conditional_dropout": (False, None),
                 "multi_scale": None, "use_fsdp": (False,)}      # None = any value: the EMA's decay is `ema_rate` (under --ema), huber_c only matters under loss_type 'huber', multi_scale is the
                                                                  # dataset class choice (the bucketed FeatureDatasetMS handles both); loss_type = 'huber' comes with
                                                                  # configs/PixArt_xl2_internal.py, the base of every Sigma config, and only train_pixart_lcm.py reads it:
                                                                  # the reference's train.py trains those configs with the IDDPM loss, as this one does


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("config", nargs="?", default=None)
    p.add_argument("--work-dir", "--work_dir", default="output/debug")
    p.add_argument("--resume-from", default=None)
    p.add_argument("--load-from", default=None)
    p.add_argument("--debug", action="store_true")
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--max-steps", type=int, default=None)
    p.add_argument("--mixed-precision", choices=["fp16", "bf16"], default=None, help="overrides the config's mixed_precision")
    add_ema_visualize_args(p)
    p.add_argument("--load-ema", action="store_true", help="with --load-from / --resume-from: start from the checkpoint's state_dict_ema")
    return p.parse_args()


def add_ema_visualize_args(p):
    """The opt-in arguments train.py and train_lora.py share."""
    p.add_argument("--ema", action="store_true", help="keep an EMA of the trained weights at the config's ema_rate (0.9999 without one)")
    p.add_argument("--ema-rate", type=float, default=None, help="with --ema: overrides the config's ema_rate")
    p.add_argument("--visualize", action="store_true", help="sample the config's validation_prompts after step 1 and every eval_sampling_steps steps")
    p.add_argument("--validation-feats", default=None, help="with --visualize: directory of <idx>.npz + null.npz caption features, index = position in validation_prompts")


def ema_decay(a, cfg):
    """The EMA's decay, or None when no EMA is kept: --ema switches it on, then --ema-rate wins over the config's ema_rate, which wins over 0.9999."""
    if not a.ema:
        if a.ema_rate is not None:
            raise SystemExit("--ema-rate needs --ema")
        return None
    d = a.ema_rate if a.ema_rate is not None else cfg.get("ema_rate")
    d = 0.9999 if d is None else d
    if not isinstance(d, (int, float)) or not 0 <= d < 1:
        raise SystemExit(f"EMA rate {d!r} must lie in [0, 1)")
    return float(d)


def ema_weights_of(sd, path):
    """--load-ema / --load_ema: the checkpoint's averaged weights."""
    if not isinstance(sd, dict) or "state_dict_ema" not in sd:
        raise SystemExit(f"{path}: the checkpoint has no state_dict_ema (it was written without --ema): --load-ema cannot take its weights from it")
    return sd["state_dict_ema"]


def check_visualize(a, cfg, text_captions):
    """Start-up check of --visualize: the prompts, the interval and a source of caption features.  Returns the prompts ([] without --visualize)."""
    if not a.visualize:
        return []
    prompts = cfg.get("validation_prompts")
    if not prompts or not all(isinstance(s, str) for s in prompts):
        raise SystemExit("--visualize: the config has no validation_prompts (a list of strings)")
    k = cfg.get("eval_sampling_steps")
    if not isinstance(k, int) or k < 1:
        raise SystemExit(f"--visualize: eval_sampling_steps={k!r} must be a positive integer")
    if not a.validation_feats and not text_captions:
        raise SystemExit("--visualize needs the caption features of validation_prompts: give --validation-feats DIR (<idx>.npz + null.npz, as "
                         "tools/extract_t5_features.py writes them), or train from text captions (load_t5_feat = False with a picture list and t5_path), "
                         "where the T5 encoder makes them before the first step")
    if a.validation_feats and not os.path.isdir(a.validation_feats):
        raise SystemExit(f"--validation-feats {a.validation_feats}: not a directory")
    return list(prompts)


def validation_due(step, every):
    """After step 1 and after every step divisible by eval_sampling_steps (reference train.py:225-228)."""
    return step == 1 or step % every == 0


def build_validation(a, cfg, model, vae, captions, dev, prompts):
    """The ValidationSampler of --visualize; the VAE is loaded here when the data mode did not need one (reference train.py:84-85)."""
    from pixart_sigma_amd.validation import ValidationSampler, load_validation_feats
    L = cfg["model_max_length"]
    if a.validation_feats:
        feats, masks, null = load_validation_feats(a.validation_feats, len(prompts), L, dev)
    else:
        if captions.outstanding:
            raise RuntimeError("validation prompts must be encoded before the first batch is requested")
        y, m = [], []
        for text in prompts + [""]:                                               # one at a time: the encoder's batch limit is the training batch's
            f, k = captions.encode([text])
            y.append(f.float().clone())
            m.append(torch.as_tensor(k).reshape(1, -1).long().cpu())
        feats, masks, null = torch.cat(y[:-1]), torch.cat(m[:-1]), y[-1]
    if vae is None:
        from pixart_sigma_amd.vae import AutoencoderKL
        have = os.path.isdir(str(cfg["vae_pretrained"]))
        vae = (AutoencoderKL.from_pretrained(cfg["vae_pretrained"], torch_dtype=torch.float16) if have else AutoencoderKL(scaling_factor=cfg["scale_factor"])).to(dev)
    return ValidationSampler(model, vae, feats, masks, null, cfg["image_size"], os.path.join(a.work_dir, "validation"), seed=cfg["seed"])


def batches(cfg, B, lat, L, dev, rank, world, synthetic):
    """Flat feature files or synthetic data; yields (z, y, mask, data_info), z unscaled (noise images of 8 * lat pixels with load_vae_feat = False)."""
    # micro-conditioning inputs (reference train.py:156): these sources have one square size, that of the picture
    info = {"img_hw": torch.tensor([[lat * 8.0, lat * 8.0]] * B), "aspect_ratio": torch.tensor([[1.0]] * B)}
    if synthetic or not cfg["data_root"]:
        g = torch.Generator().manual_seed(cfg["seed"] + rank)
        while not cfg["load_vae_feat"]:                                            # images in, latents from the VAE inside the step
            yield torch.randn(B, 3, lat * 8, lat * 8, generator=g).clamp(-1, 1).to(dev), torch.randn(B, 1, L, 4096, generator=g).to(dev), torch.ones(B, L, dtype=torch.int64), info
        while True:
            yield torch.randn(B, 4, lat, lat, generator=g).to(dev), torch.randn(B, 1, L, 4096, generator=g).to(dev), torch.ones(B, L, dtype=torch.int64), info
    names = sorted(glob.glob(os.path.join(cfg["data_root"], "*.npz")))[rank::world]
    while True:
        for i in range(0, len(names) - B + 1, B):
            zs, ys, ms = [], [], []
            for n in names[i:i + B]:
                f = np.load(n)
                lat_stats = np.load(n[:-4] + ".npy")                               # cat[mean, std] (InternalData.py:296-301)
                mean, std = np.split(lat_stats.reshape(8, lat, lat), 2)
                zs.append(torch.from_numpy(mean + std * np.random.randn(*mean.shape)).float())
                ys.append(torch.from_numpy(f["caption_feature"]).float().reshape(1, -1, 4096)[:, :L])
                ms.append(torch.from_numpy(f["attention_mask"]).reshape(-1)[:L])
            yield torch.stack(zs).to(dev), torch.stack(ys).to(dev), torch.stack(ms), info


def load_config(path, debug=False):
    cfg = dict(DEFAULTS)
    if path:
        user = run_config(path)
        unknown = sorted(k for k in user if k not in DEFAULTS and k not in IGNORED_KEYS and k not in SEMANTIC_KEYS and k != "data")
        if unknown:
            raise SystemExit(f"{path}: config keys this training path does not implement: {unknown} (supported: {sorted(DEFAULTS)})")
        bad = {k: user[k] for k, ok in SEMANTIC_KEYS.items() if k in user and ok is not None and user[k] not in ok}
        if bad:
            raise SystemExit(f"{path}: these settings change what is trained and only one value is implemented here: "
                             + ", ".join(f"{k}={v!r} (implemented: {SEMANTIC_KEYS[k][0]!r})" for k, v in bad.items()))
        cfg.update({k: v for k, v in user.items() if k in DEFAULTS})
        # the dataset dict of the reference's configs (data = dict(type=..., root=..., load_vae_feat=..., load_t5_feat=...)): a top-level key wins where
        # a config sets both, as it did when `data` was not read at all
        data = user.get("data") or {}
        if not isinstance(data, dict):
            raise SystemExit(f"{path}: data must be a dict, got {type(data).__name__}")
        for k in ("load_vae_feat", "load_t5_feat", "image_list_json"):
            if k in data and k not in user:
                cfg[k] = data[k]
        cfg["data_type"], cfg["data_subdir"] = data.get("type"), data.get("root")
    if isinstance(cfg["image_list_json"], (list, tuple)) and len(cfg["image_list_json"]) == 1:
        cfg["image_list_json"] = cfg["image_list_json"][0]
    r = cfg["real_prompt_ratio"]
    if not isinstance(r, (int, float)) or not 0 <= r <= 1:
        raise SystemExit(f"{path}: real_prompt_ratio={r!r} must lie in [0, 1]")
    if cfg["load_t5_feat"] and r != 1.0:             # FeatureDatasetMS and the caption-file mode of the picture datasets always take the real prompt
        raise SystemExit(f"{path}: these settings change what is trained and only one value is implemented here: real_prompt_ratio={r!r} (implemented: 1.0) "
                         "with caption feature files (load_t5_feat=True); any value in [0, 1] needs text captions (load_t5_feat=False)")
    if cfg["t5_weight_dtype"] not in (None, "fp8_e4m3"):
        raise SystemExit(f"{path}: t5_weight_dtype={cfg['t5_weight_dtype']!r} is not implemented (None or 'fp8_e4m3')")
    if cfg["load_vae_feat"] and not cfg["load_t5_feat"]:
        raise SystemExit(f"{path}: load_vae_feat=True with load_t5_feat=False (latent files with text captions) is not implemented")
    if debug:
        cfg.update(train_batch_size=2, log_interval=1)
    if cfg["lr_schedule"] not in ("constant", "cosine", "cosine_decay_to_constant"):
        raise SystemExit(f"Unrecognized lr schedule {cfg['lr_schedule']}.")
    return cfg


def feature_batches(cfg, B, L, dev, rank, world):
    """Feature files in the reference's layout (InternalDataMSSigma + AspectRatioBatchSampler, reference train.py:404-421): every batch has
    one latent shape; yields (z, y, mask, data_info)."""
    from pixart_sigma_amd.data import AspectRatioBatchSampler, FeatureDatasetMS
    ratios = cfg["aspect_ratio_type"]
    if not isinstance(ratios, dict):
        raise SystemExit("aspect_ratio_type must be the bucket table itself: {ratio string: [H, W]} (the reference's ASPECT_RATIO_* dicts)")
    ds = FeatureDatasetMS(cfg["data_root"], ratios, resolution=cfg["image_size"], max_length=L)
    g = torch.Generator().manual_seed(cfg["seed"] + rank)
    while True:
        order = torch.randperm(len(ds), generator=g).tolist()[rank::world]
        for idx in AspectRatioBatchSampler(order, ds, B, ratios, drop_last=True, valid_num=cfg["valid_num"], ratio_nums={str(k): v for k, v in ds.ratio_nums.items()}):
            items = [ds.__getitem__(i, g) for i in idx]
            z = torch.stack([it[0] for it in items]).float().to(dev)
            y = torch.stack([it[1].float() for it in items]).to(dev)                    # (B, 1, L, 4096)
            mask = torch.cat([it[2].reshape(1, -1) for it in items]).long()             # host mask: no device sync for y_lens
            info = {"img_hw": torch.stack([it[3]["img_hw"] for it in items]), "aspect_ratio": torch.tensor([[it[3]["aspect_ratio"]] for it in items])}
            yield z, y, mask, info


def picture_root(cfg):
    """The dataset root of the picture modes: data_root joined with the `root` of the config's data dict, as the reference's get_data_path joins them,
    where that directory exists; data_root itself otherwise."""
    sub = os.path.join(cfg["data_root"], cfg["data_subdir"]) if cfg.get("data_subdir") else None
    return sub if sub and os.path.isdir(sub) else cfg["data_root"]


def pictures_mode(cfg, synthetic):
    """True when the batches come from pictures (load_vae_feat = False with a real image list): reference train.py:144-168."""
    if cfg["load_vae_feat"] or synthetic or not cfg["data_root"]:
        return False
    lists = cfg["image_list_json"] if isinstance(cfg["image_list_json"], (list, tuple)) else [cfg["image_list_json"]]
    return all(os.path.exists(os.path.join(picture_root(cfg), j)) for j in lists)


def picture_batches(cfg, B, L, dev, rank, world, vae):
    """Pictures (and caption strings, with load_t5_feat = False) in, (x0, y, mask, data_info) out - x0 already times the scale factor: the dataset class of
    the config's data['type'], PictureBatches one batch ahead of the step, CaptionEncoder for text.  Returns (iterator, the CaptionEncoder or None)."""
    from pixart_sigma_amd.data import PictureBatches, PictureCaptionDataset, PictureCaptionDatasetMS, load_ratio_table
    root, kind = picture_root(cfg), cfg.get("data_type")
    common = dict(image_list_json=cfg["image_list_json"], resolution=cfg["image_size"], real_prompt_ratio=cfg["real_prompt_ratio"], max_length=L,
                  load_t5_feat=cfg["load_t5_feat"])
    if kind == "InternalDataMSSigma" or (kind is None and cfg["aspect_ratio_type"] is not None):
        try:
            ratios = load_ratio_table(cfg["aspect_ratio_type"])
        except ValueError as e:
            raise SystemExit(str(e))
        ds = PictureCaptionDatasetMS(root, ratios, **common)
    elif kind in (None, "InternalDataSigma"):
        ratios, ds = None, PictureCaptionDataset(root, **common)
    else:
        raise SystemExit(f"data type {kind!r} is not implemented for pictures (implemented: InternalDataMSSigma, InternalDataSigma)")
    captions = None
    if not cfg["load_t5_feat"]:
        from pixart_sigma_amd.t5.captions import CaptionEncoder
        tok_dir = os.path.join(os.path.dirname(str(cfg["t5_path"]).rstrip("/")), "tokenizer")
        if not os.path.isdir(str(cfg["t5_path"])):
            raise SystemExit(f"t5_path={cfg['t5_path']!r} is not a directory: text captions (load_t5_feat=False) need the T5 encoder's weights")
        from transformers import AutoTokenizer
        tokenizer = AutoTokenizer.from_pretrained(tok_dir if os.path.isdir(tok_dir) else cfg["t5_path"])
        captions = CaptionEncoder(cfg["t5_path"], tokenizer, model_max_length=L, device=dev, max_batch=B, weight_dtype=cfg["t5_weight_dtype"])
    it = PictureBatches(ds, B, ratios, vae, captions, cfg["seed"], rank, world, device=dev, num_workers=cfg["num_workers"], valid_num=cfg["valid_num"],
                        scale=cfg["scale_factor"], sample_posterior=cfg["sample_posterior"])
    return iter(it), captions


def load_optimizer_state(opt, sd, rank):
    """Our own flat-buffer state (validated against the parameter layout) or a reference checkpoint's torch / CAME state_dict
    ('state' / 'param_groups': per-parameter tensors in the reference's parameter order) - the latter is skipped with a warning."""
    o = sd.get("optimizer")
    if o is None:
        return False
    if "param_groups" in o or "state" in o:
        if rank == 0:
            print("resume: the checkpoint carries a torch-format optimizer state (reference checkpoint); moments are re-initialised", flush=True)
        return False
    opt.load_state_dict(o)
    return True


def init_process():
    """(world, rank, device) from the launcher's environment; the nccl process group when there is more than one rank."""
    world, rank, local = int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)
    return world, rank, dev


def build_denoiser(cfg):
    return build_model(cfg["model"], cfg["grad_checkpointing"], cfg["fp32_attention"], gc_step=cfg["gc_step"], input_size=cfg["image_size"] // 8,
                       pe_interpolation=cfg["image_size"] / 512, model_max_length=cfg["model_max_length"], micro_condition=cfg["micro_condition"],
                       kv_compress_config=cfg["kv_compress_config"] if cfg["kv_compress"] else None,
                       pred_sigma=cfg["pred_sigma"], learn_sigma=cfg["learn_sigma"], class_dropout_prob=cfg["class_dropout_prob"])


def make_schedule(cfg, o, B, world, accum):
    """Learning rate: batch-size scaling (reference train.py:448-452), which rewrites o["lr"], + warm-up schedule (lr_scheduler.py:10-40).
    Returns (schedule, auto_lr ratio)."""
    ratio = 1.0
    if cfg["auto_lr"]:
        o["lr"], ratio = auto_scale_lr(B * world * accum, o["lr"], **cfg["auto_lr"])
    # accelerate steps the prepared scheduler `world` times per optimizer step (split_batches=False, the reference's setting): steps_per_call
    sched = LRSchedule(o["lr"], cfg["lr_schedule"], lr_scale_ratio=ratio, steps_per_call=world,
                       num_training_steps=(cfg["num_steps_per_epoch"] or 0) * cfg["num_epochs"] or None, **(cfg["lr_schedule_args"] or {}))
    return sched, ratio


def load_vae(cfg, dev):
    """The VAE of the modes that train from pictures (reference train.py:351-354), whose scaling factor becomes cfg["scale_factor"]; None with feature files."""
    if cfg["load_vae_feat"]:
        return None
    from pixart_sigma_amd.vae import AutoencoderKL
    have = os.path.isdir(str(cfg["vae_pretrained"]))
    vae = (AutoencoderKL.from_pretrained(cfg["vae_pretrained"], torch_dtype=torch.float16) if have else AutoencoderKL(scaling_factor=cfg["scale_factor"])).to(dev)
    cfg["scale_factor"] = vae.config.scaling_factor
    return vae


def _scaled_latents(it, cfg, vae):
    for z, y, mask, info in it:
        if vae is not None:                                                        # reference train.py:147-153
            z = vae.encode(z).latent_dist.sample().float()
        yield z * cfg["scale_factor"], y, mask, info


def data_source(cfg, synthetic, B, lat, L, dev, rank, world, vae):
    """The batches of the config's data mode, every one (x0, y, mask, data_info) with x0 already times the scale factor.  Returns (iterator, the
    CaptionEncoder to close or None)."""
    if pictures_mode(cfg, synthetic):                                              # VAE, posterior kernel and scale factor inside the iterator
        return picture_batches(cfg, B, L, dev, rank, world, vae)
    use_ds = bool(cfg["data_root"]) and not synthetic and os.path.exists(os.path.join(cfg["data_root"], "data_info.json"))
    it = feature_batches(cfg, B, L, dev, rank, world) if use_ds else batches(cfg, B, lat, L, dev, rank, world, synthetic)
    return _scaled_latents(it, cfg, vae), None


def make_validate(a, cfg, model, vae, captions, dev, prompts, ema):
    """validate(step) of train_loop: pictures from the raw weights, and from the EMA when one is kept."""
    sampler = build_validation(a, cfg, model, vae, captions, dev, prompts)

    def validate(step):
        sampler.run(step)
        if ema is not None:
            sampler.run(step, ema=ema)
        print(f"step {step}: validation pictures of {len(prompts)} prompts in {os.path.join(sampler.out_dir, f'step_{step}')}" + (" and ..._ema" if ema is not None else ""), flush=True)
    return validate


def train_loop(cfg, model, diff, opt, sched, scaler, it, dev, rank, world, start_step, max_steps, save, ema=None, validate=None):
    """Optimizer steps start_step + 1 ... start_step + max_steps (without end when max_steps is None), `save(step)` on rank 0 every save_model_steps.
    ema: its update() runs directly behind every opt.step() (once per optimizer step, not per micro-batch).  validate: `validate(step)` on rank 0 after
    step 1 and every eval_sampling_steps steps, behind the log line.  Returns (last step, its loss as the log line prints it, still a tensor)."""
    accum = int(cfg["gradient_accumulation_steps"])
    t0, step = time.time(), start_step
    sched_skips_seen = scaler.steps_skipped if scaler else 0
    while max_steps is None or step < start_step + max_steps:
        opt.zero_grad()
        opt.lr = sched.lr
        for micro in range(accum):                                                 # accelerator.accumulate (reference train.py:175)
            x0, y, mask, info = next(it)
            t = torch.randint(0, cfg["train_sampling_steps"], (x0.shape[0],), device=dev).long()
            loss = diff.training_losses(model, x0, t, model_kwargs=dict(y=y, mask=mask, data_info=info))["loss"].mean() / accum
            if micro + 1 < accum:
                with opt.reducer.no_sync():                                        # local accumulation, no all-reduce yet
                    (scaler.scale(loss) if scaler else loss).backward()
            else:
                (scaler.scale(loss) if scaler else loss).backward()
        opt.step()
        if ema is not None:
            ema.update()
        sched.step()
        step += 1
        saving = step % cfg["save_model_steps"] == 0
        if scaler and (step % cfg["log_interval"] == 0 or saving):   # accelerate does not advance the schedule on a step the GradScaler skipped; the skip count
            skipped = scaler.steps_skipped                     # lives on the device, so the schedule is reconciled where the host syncs anyway (skips are rare) -
            sched.last_step -= world * (skipped - sched_skips_seen)   # and ALWAYS in front of a checkpoint: a resumed run starts its own count from the loaded
            sched_skips_seen = skipped                         # scaler's total, so skips not yet subtracted at save time would never be
        if step % cfg["log_interval"] == 0 and rank == 0:      # host sync only here (the reference syncs every step, train.py:187)
            extra = f" loss_scale {scaler.value:g} skipped {scaler.steps_skipped}" if scaler else ""
            print(f"step {step} loss {loss.item() * accum:.4f} grad_norm {opt.last_norm.item():.4f} lr {opt.lr:.3e}{extra} "
                  f"{(time.time() - t0) / cfg['log_interval']:.3f} s/step", flush=True)
            t0 = time.time()
        if validate is not None and rank == 0 and validation_due(step, cfg["eval_sampling_steps"]):
            validate(step)
            t0 = time.time()                                    # the pictures' time is not a training step's
        if saving and rank == 0:
            save(step)
    return step, loss.detach().double() * accum


def main():
    a = parse_args()
    cfg = load_config(a.config, a.debug)
    cfg["mixed_precision"] = MIXED_PRECISION
    decay = ema_decay(a, cfg)
    text_captions = pictures_mode(cfg, a.synthetic) and not cfg["load_t5_feat"]
    prompts = check_visualize(a, cfg, text_captions)
    if a.load_ema and not (a.resume_from or a.load_from):
        raise SystemExit("--load-ema needs --load-from or --resume-from")
    world, rank, dev = init_process()
    torch.manual_seed(cfg["seed"])
    lat, L, B, accum = cfg["image_size"] // 8, cfg["model_max_length"], cfg["train_batch_size"], int(cfg["gradient_accumulation_steps"])
    model = build_denoiser(cfg)
    start_step, sd = 0, None
    ck = a.resume_from or a.load_from
    if ck:
        sd = torch.load(ck, map_location="cpu", weights_only=False)
        model.load_state_dict(ema_weights_of(sd, ck) if a.load_ema else sd.get("state_dict", sd), strict=False)
    model = model.to(dev).train()
    model.prepare(dev)
    o = dict(cfg["optimizer"])
    sched, ratio = make_schedule(cfg, o, B, world, accum)
    scaler = LossScaler(dev) if cfg["mixed_precision"] == "fp16" else None      # GradScaler protocol of accelerate's fp16 mode, on the device
    if o.get("type", "AdamW") in ("CAMEWrapper", "CAME"):      # the optimizer of the PixArt-Sigma configs (reference optimizer.py:242-246)
        opt = FusedCAME(model, lr=o["lr"], weight_decay=o.get("weight_decay", 0.0), eps=o.get("eps", (1e-30, 1e-16)),
                        betas=o.get("betas", (0.9, 0.999, 0.9999)), max_grad_norm=cfg["gradient_clip"], scaler=scaler)
    else:
        opt = FusedAdamW(model, lr=o["lr"], weight_decay=o["weight_decay"], eps=o.get("eps", 1e-8), betas=o.get("betas", (0.9, 0.999)),
                         max_grad_norm=cfg["gradient_clip"], scaler=scaler)
    if a.resume_from and sd is not None:
        if load_optimizer_state(opt, sd, rank):
            start_step = int(sd.get("step", 0))
        if "lr_scheduler" in sd:
            sched.load_state_dict(sd["lr_scheduler"], optimizer_step=sd.get("step"))
        elif "scheduler" in sd:                                 # reference checkpoint: torch LambdaLR state (save_checkpoint)
            sched.load_state_dict(sd["scheduler"])
        if scaler is not None and "loss_scaler" in sd:
            scaler.load_state_dict(sd["loss_scaler"])
        if "_step_" in a.resume_from and not start_step:
            start_step = int(os.path.basename(a.resume_from).split("_step_")[-1].split(".")[0])
    if rank == 0:
        print(f"lr {o['lr']:.3e} (auto_lr x{ratio:.3f}), schedule {cfg['lr_schedule']} {cfg['lr_schedule_args']}, accumulation {accum}, "
              f"operands {cfg['mixed_precision']}" + (f", loss scale {scaler.value:g}" if scaler else ""), flush=True)
    ema = None
    if decay is not None:
        from pixart_sigma_amd.ema import WeightEMA
        ema = WeightEMA(model, decay, scaler=scaler)            # starts as a copy of the loaded weights
        if a.resume_from and sd is not None and not a.load_ema:
            if "state_dict_ema" in sd:
                ema.load_state_dict(sd["state_dict_ema"])
            elif rank == 0:
                print(f"resume: {a.resume_from} has no state_dict_ema; the EMA starts from the loaded weights", flush=True)
        if rank == 0:
            print(f"EMA of the weights at rate {decay:g}", flush=True)
    diff = IDDPM(str(cfg["train_sampling_steps"]), learn_sigma=cfg["learn_sigma"], pred_sigma=cfg["pred_sigma"], snr=cfg["snr_loss"])
    vae = load_vae(cfg, dev)
    os.makedirs(os.path.join(a.work_dir, "checkpoints"), exist_ok=True)
    it, captions = data_source(cfg, a.synthetic, B, lat, L, dev, rank, world, vae)
    if rank == 0 and pictures_mode(cfg, a.synthetic):
        print(f"data: pictures of {picture_root(cfg)} with {'caption feature files' if cfg['load_t5_feat'] else 'text captions'}", flush=True)
    validate = make_validate(a, cfg, model, vae, captions, dev, prompts, ema) if prompts and rank == 0 else None

    def save(step):
        torch.save({"state_dict": model.state_dict(), "optimizer": opt.state_dict(), "lr_scheduler": sched.state_dict(), "step": step,
                    **({"state_dict_ema": ema.state_dict()} if ema is not None else {}),
                    **({"loss_scaler": scaler.state_dict()} if scaler else {})},
                   os.path.join(a.work_dir, "checkpoints", f"epoch_1_step_{step}.pth"))
    step, loss = train_loop(cfg, model, diff, opt, sched, scaler, it, dev, rank, world, start_step, a.max_steps, save, ema=ema, validate=validate)
    if rank == 0:
        print(f"finished at step {step}: loss {loss.item():.4f} grad_norm {opt.last_norm.item():.4f} lr {opt.lr:.3e}", flush=True)
    if captions is not None:
        captions.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
