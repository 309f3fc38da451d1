"""Validation pictures during training: the reference's log_validation (train_scripts/train.py:45-103, called at :225-228 every `eval_sampling_steps`)
on the HIP denoiser and VAE - without trackers; the pictures are PNG files.

Per prompt, batch 1: DPMS(model.forward_with_dpmsolver, condition, uncondition=null, cfg_scale=4.5).sample(z, steps=14, order=2, skip_type="time_uniform",
method="multistep"), eager; vae.decode(latent / scaling_factor); clamp(127.5 x + 128, 0, 255) truncated to uint8, HWC; `<out_dir>/step_<step>/<i>.png`.
The noise z is the same for every prompt (the reference's validation_noise) and comes from the sampler's own generator, re-seeded at every call (its
deterministic_validation), so pictures of different steps differ by the weights alone.

run() is safe between two training steps.  After it returns these have the bits / values they had before: store.master, store.shadow, store.grad, the
optimizer's moments, the EMA buffer, the loss scaler's record, torch.get_rng_state(), torch.cuda.get_rng_state() and model.training.  Only
store.generation, and the caches keyed on it, may have moved.  With `ema` it samples inside ema.swapped() and writes into `step_<step>_ema/`.
"""
import contextlib
import os

import torch

from .diffusion import DPMS


def to_uint8_hwc(samples):
    """(1, 3, H, W) decoder output in [-1, 1] -> (H, W, 3) uint8 numpy array, reference train.py:89."""
    return torch.clamp(127.5 * samples.float() + 128.0, 0, 255).permute(0, 2, 3, 1).to("cpu", dtype=torch.uint8).numpy()[0]


class ValidationSampler:
    def __init__(self, model, vae, feats, masks, null_feat, image_size, out_dir, steps=14, cfg_scale=4.5, seed=0):
        """feats (n, 1, L, C) caption features of the n validation prompts, masks (n, L) on the host, null_feat (1, 1, L, C) the empty prompt's features."""
        assert feats.dim() == 4 and feats.shape[1] == 1 and null_feat.dim() == 4 and null_feat.shape[0] == 1 and masks.shape[0] == feats.shape[0]
        self.model, self.vae = model, vae
        self.feats, self.masks, self.null_feat = feats, masks.cpu(), null_feat
        self.image_size, self.out_dir = int(image_size), out_dir
        self.steps, self.cfg_scale, self.seed = int(steps), float(cfg_scale), int(seed)
        self._gen = None

    def noise(self, device):
        """The validation noise: the sampler's own generator, re-seeded, so the global generators are not advanced."""
        if self._gen is None or self._gen.device != torch.device(device):
            self._gen = torch.Generator(device=device)
        self._gen.manual_seed(self.seed)
        lat = self.image_size // 8
        return torch.randn(1, 4, lat, lat, generator=self._gen, device=device)

    def sample(self, model, z):
        """The latents of every prompt from `model` and the noise z (one eager DPM-Solver run per prompt)."""
        dev = z.device
        hw = torch.tensor([[self.image_size, self.image_size]], dtype=torch.float, device=dev)
        ar = torch.tensor([[1.0]], device=dev)
        null = self.null_feat.to(dev)
        out = []
        for i in range(self.feats.shape[0]):
            dpms = DPMS(model.forward_with_dpmsolver, condition=self.feats[i:i + 1].to(dev), uncondition=null, cfg_scale=self.cfg_scale,
                        model_kwargs=dict(data_info={"img_hw": hw, "aspect_ratio": ar}, mask=self.masks[i:i + 1]))
            out.append(dpms.sample(z.clone(), steps=self.steps, order=2, skip_type="time_uniform", method="multistep"))
        return out

    def decode(self, latent):
        """One latent -> (H, W, 3) uint8."""
        return to_uint8_hwc(self.vae.decode(latent.to(self.vae.dtype) / self.vae.config.scaling_factor).sample)

    def run(self, step, ema=None):
        from PIL import Image
        model = self.model
        dev = next(model.parameters()).device
        was_training = model.training
        z = self.noise(dev)
        with torch.no_grad(), (ema.swapped() if ema is not None else contextlib.nullcontext()):
            model.eval()
            try:
                latents = self.sample(model, z)
            finally:
                model.train(was_training)
        d = os.path.join(self.out_dir, f"step_{step}" + ("_ema" if ema is not None else ""))
        os.makedirs(d, exist_ok=True)
        with torch.no_grad():
            for i, latent in enumerate(latents):
                Image.fromarray(self.decode(latent)).save(os.path.join(d, f"{i}.png"))
        return latents


def load_validation_feats(path, n, L, device):
    """(feats (n, 1, L, C), masks (n, L), null (1, 1, L, C)) from `<idx>.npz` + `null.npz` (tools/extract_t5_features.py's layout), index = position of the prompt."""
    import numpy as np
    need = [f"{i}.npz" for i in range(n)] + ["null.npz"]
    lack = [f for f in need if not os.path.exists(os.path.join(path, f))]
    if lack:
        raise SystemExit(f"--validation-feats {path}: missing {lack} (one <idx>.npz per validation prompt and null.npz, as tools/extract_t5_features.py writes them)")

    def feat(name):
        z = np.load(os.path.join(path, name))
        f = torch.from_numpy(z["caption_feature"]).float()
        return f.reshape(1, 1, -1, f.shape[-1])[:, :, :L], torch.from_numpy(z["attention_mask"]).reshape(1, -1)[:, :L]
    pairs = [feat(f"{i}.npz") for i in range(n)]
    return torch.cat([f for f, _ in pairs]).to(device), torch.cat([m for _, m in pairs]).long(), feat("null.npz")[0].to(device)
