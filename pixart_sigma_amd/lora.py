"""LoRA adapters on the block linears of PixArtMS: fine-tuning and inference with peft-format files.

Replaces what the reference's fine-tuning scripts get from peft (train_scripts/train_pixart_lora_hf.py:505-524: LoraConfig + get_peft_model; :552 / :990:
get_peft_model_state_dict + save_pretrained): `y = x (W + s B A)^T + b`, A (r, in), B (out, r), s = lora_alpha / r (lora_alpha / sqrt(r) under rsLoRA).

How it runs here (DESIGN.md "LoRA"):
  * the adapter is folded into the 16-bit operand copy of W (ParamStore.shadow), never into the fp32 master: shadow = round16(W + s B A), one fp32 evaluation
    and one rounding (ops.lora_merge), redone behind every re-cast of the base and every change of the adapters.  Forward GEMMs, fused epilogues, the text
    cache and the dX GEMMs run unchanged on the merged operand;
  * the backward never forms dW: t = x A^T, u = dy B, dA = s u^T x, dB^T = s t^T dy (ops.lora_bwd), one call per adapted row slice; the base is frozen;
  * adapters are ordinary fp32 nn.Parameters - A as `lora_A` (r, in), B TRANSPOSED as `lora_Bt` (r, out) - in a small ParamStore of their own with the base
    store's `blocks.{i}` group labels, so Engine.grad_ready_hook, GradReducer and FusedAdamW work on it as they do on the base store.

Adapters are named by the diffusers module they belong to (model/checkpoint_compat.py holds the same PixArt <-> diffusers map for the weights); a fused
linear (attn.qkv, cross_attn.kv_linear) carries one adapter per row slice.  peft and diffusers are not dependencies: the on-disk layout below is a from-spec
restatement of peft's (adapter_config.json + adapter_model.safetensors, keys `base_model.model.transformer_blocks.{i}.<module>.lora_A.weight` (r, in) /
`.lora_B.weight` (out, r))."""
import dataclasses
import json
import math
import os
import typing

import torch
import torch.nn as nn

MAX_RANK = 64
# diffusers module of a transformer block -> (PixArt linear, row slice index, number of slices of that linear)
BLOCK_MODULES = {
    "attn1.to_q": ("attn.qkv", 0, 3), "attn1.to_k": ("attn.qkv", 1, 3), "attn1.to_v": ("attn.qkv", 2, 3), "attn1.to_out.0": ("attn.proj", 0, 1),
    "attn2.to_q": ("cross_attn.q_linear", 0, 1), "attn2.to_k": ("cross_attn.kv_linear", 0, 2), "attn2.to_v": ("cross_attn.kv_linear", 1, 2),
    "attn2.to_out.0": ("cross_attn.proj", 0, 1), "ff.net.0.proj": ("mlp.fc1", 0, 1), "ff.net.2": ("mlp.fc2", 0, 1),
}
# the rest of the reference's target list (train_pixart_lora_hf.py:508-521): modules outside the transformer blocks
OUTSIDE_BLOCKS = ("proj", "linear", "linear_1", "linear_2", "proj_in", "proj_out")
DEFAULT_TARGETS = ("to_k", "to_q", "to_v", "to_out.0", "ff.net.0.proj", "ff.net.2")
PEFT_PREFIX = "base_model.model.transformer_blocks."


@dataclasses.dataclass
class LoraConfig:
    """peft.LoraConfig's fields as the reference uses them.  lora_alpha = 8 is peft's default (the reference passes only r); init_lora_weights = "gaussian":
    A ~ N(0, (1/r)^2) as peft draws it (std 1 / r), B = 0."""
    r: int = 16
    lora_alpha: float = 8
    target_modules: typing.Sequence[str] = DEFAULT_TARGETS
    use_rslora: bool = False
    init_lora_weights: typing.Union[str, bool] = "gaussian"
    use_dora: bool = False
    lora_dropout: float = 0.0

    def __post_init__(self):
        if isinstance(self.target_modules, str):
            self.target_modules = [self.target_modules]
        self.target_modules = list(self.target_modules)
        if self.use_dora:
            raise NotImplementedError("use_dora=True: DoRA is not implemented on the HIP path")
        if self.lora_dropout:
            raise NotImplementedError("lora_dropout != 0 is not implemented on the HIP path")
        if not (isinstance(self.r, int) and 1 <= self.r <= MAX_RANK):
            raise ValueError(f"LoRA rank must be an integer in 1..{MAX_RANK} (the gradient kernel's tile), got {self.r!r}")
        if self.init_lora_weights not in ("gaussian", True, False):
            raise ValueError(f"init_lora_weights={self.init_lora_weights!r}: 'gaussian', True (kaiming-uniform A) or False (random B too)")
        resolve_targets(self.target_modules)

    @property
    def scaling(self):
        return self.lora_alpha / (math.sqrt(self.r) if self.use_rslora else self.r)


def resolve_targets(target_modules):
    """peft's matching rule (a module is adapted if its name equals a target or ends with '.' + target) over the ten linears of a block.  Targets that
    name modules outside the blocks raise - they are never dropped silently - and so does a target that matches nothing."""
    out = []
    for t in target_modules:
        if t in OUTSIDE_BLOCKS:
            raise NotImplementedError(f"target module {t!r}: LoRA is not implemented for modules outside the transformer blocks "
                                      f"(supported: {', '.join(BLOCK_MODULES)} and their suffixes)")
        hit = [m for m in BLOCK_MODULES if m == t or m.endswith("." + t)]
        if not hit:
            raise ValueError(f"target module {t!r} matches no linear of a transformer block ({', '.join(BLOCK_MODULES)})")
        out += [m for m in hit if m not in out]
    return [m for m in BLOCK_MODULES if m in out]


def peft_key(name):
    """'blocks.3.attn1.to_q.lora_A' -> 'base_model.model.transformer_blocks.3.attn1.to_q.lora_A.weight' ('lora_Bt' -> 'lora_B': stored transposed)."""
    assert name.startswith("blocks.")
    stem, leaf = name[len("blocks."):].rsplit(".", 1)
    return f"{PEFT_PREFIX}{stem}.{ {'lora_A': 'lora_A', 'lora_Bt': 'lora_B'}[leaf]}.weight"


def internal_name(key):
    """Inverse of peft_key; also takes keys that carry peft's adapter name ('...lora_A.default.weight')."""
    if not (key.startswith(PEFT_PREFIX) and key.endswith(".weight")):
        raise KeyError(f"not a transformer-block LoRA key: {key!r}")
    stem = key[len(PEFT_PREFIX):-len(".weight")]
    if stem.endswith(".default"):
        stem = stem[:-len(".default")]
    stem, leaf = stem.rsplit(".", 1)
    i, module = stem.split(".", 1)
    if module not in BLOCK_MODULES or leaf not in ("lora_A", "lora_B") or not i.isdigit():
        raise KeyError(f"not a transformer-block LoRA key: {key!r}")
    return f"blocks.{i}.{module}.{'lora_A' if leaf == 'lora_A' else 'lora_Bt'}"


class LoraAdapters:
    """The adapters of one model: parameters, their flat store, and for every adapted PixArt linear its row slices [(lo, hi, adapter name)].  Deliberately not
    an nn.Module of the model: the base model's parameter list, state dict and flat store stay exactly what they are without adapters."""

    def __init__(self, model, config):
        self.config, self.multiplier = config, 1.0
        self.params, self.slices = {}, {}
        self.store = None
        mods = resolve_targets(config.target_modules)
        dev = next(model.parameters()).device
        for i, blk in enumerate(model.blocks):
            for m in mods:
                lin, j, n = BLOCK_MODULES[m]
                w = blk.get_submodule(lin).weight
                rows, fin = w.shape[0] // n, w.shape[1]
                ad = f"blocks.{i}.{m}"
                a = torch.empty(config.r, fin, device=dev)
                bt = torch.zeros(config.r, rows, device=dev)
                if config.init_lora_weights == "gaussian":
                    nn.init.normal_(a, std=1.0 / config.r)
                else:
                    nn.init.kaiming_uniform_(a, a=math.sqrt(5))
                    if config.init_lora_weights is False:
                        nn.init.normal_(bt, std=0.02)
                self.params[ad + ".lora_A"], self.params[ad + ".lora_Bt"] = nn.Parameter(a), nn.Parameter(bt)
                self.slices.setdefault(f"blocks.{i}.{lin}", []).append((j * rows, (j + 1) * rows, ad))
        self._frozen = [(p, p.requires_grad) for p in model.parameters()]
        for p, _ in self._frozen:                                  # everything but the adapters is frozen (train_pixart_lora_hf.py:498-503)
            p.requires_grad_(False)

    @property
    def scale(self):
        return self.config.scaling * self.multiplier

    @property
    def trainable(self):
        return any(p.requires_grad for p in self.params.values())

    def named_parameters(self):
        return list(self.params.items())

    def prepare(self, model, device):
        """(Re)build the adapter store on the base store's device and attach it to the model's engine; re-cast the 16-bit copies of edited adapters."""
        from .engine import ParamStore
        named = self.named_parameters()
        if self.store is None or self.store.device != device or not self.store.owns_all(named):
            self.store = ParamStore(named, device, group_of=lambda n: ".".join(n.split(".")[:2]))
        if model._engine.lora is not self or model._engine._lora_refs[1] not in self.store._on_change:
            model._engine.attach_lora(self)
        self.store.refresh_shadow()

    def state_dict(self):
        """peft layout: key -> contiguous fp32 CPU tensor, lora_B as (out, r)."""
        return {peft_key(n): (p.detach().t() if n.endswith("lora_Bt") else p.detach()).to("cpu", torch.float32).contiguous().clone() for n, p in self.params.items()}

    def load_state_dict(self, sd):
        seen = set()
        for k, v in sd.items():
            n = internal_name(k)
            if n not in self.params:
                raise KeyError(f"{k}: the model has no adapter {n!r} (target_modules {self.config.target_modules})")
            p = self.params[n]
            v = v.t() if n.endswith("lora_Bt") else v
            if tuple(v.shape) != tuple(p.shape):
                raise ValueError(f"{k}: shape {tuple(v.shape)} does not fit the adapter's {tuple(p.shape)}")
            with torch.no_grad():
                p.copy_(v)
            seen.add(n)
        missing = sorted(set(self.params) - seen)
        if missing:
            raise KeyError(f"adapter file lacks {len(missing)} tensors, e.g. {peft_key(missing[0])}")

    def adapter_config(self):
        c = self.config
        return {"peft_type": "LORA", "task_type": None, "base_model_name_or_path": None, "r": c.r, "lora_alpha": c.lora_alpha,
                "target_modules": list(c.target_modules), "use_rslora": bool(c.use_rslora), "use_dora": False, "lora_dropout": 0.0, "bias": "none",
                "init_lora_weights": c.init_lora_weights, "fan_in_fan_out": False, "inference_mode": not self.trainable, "modules_to_save": None}


def add_lora(model, config=None, **kw):
    """Attach fresh adapters to the block linears of `model` (PixArtMS) and freeze everything else; returns the LoraAdapters.  add_lora(model, r=16, ...)
    builds the LoraConfig."""
    if config is None:
        config = LoraConfig(**kw)
    elif kw:
        raise TypeError("add_lora takes a LoraConfig or its fields, not both")
    if getattr(model, "fp8", None) is not None:
        raise RuntimeError("FP8 inference is on: adapters cannot be attached to it (disable_fp8() first, or merge_and_unload() the adapters and enable FP8 on "
                           "the merged weights)")
    if getattr(model, "_lora", None) is not None:
        raise RuntimeError("the model already carries LoRA adapters: merge_and_unload() first")
    model._lora = LoraAdapters(model, config)
    if model._store is not None:
        model._prepare(model._store.device)
    return model._lora


def save_lora(model, path):
    """peft's on-disk layout: adapter_config.json + adapter_model.safetensors under `path`."""
    from safetensors.torch import save_file
    lo = _adapters(model)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump(lo.adapter_config(), f, indent=2, sort_keys=True)
    save_file(lo.state_dict(), os.path.join(path, "adapter_model.safetensors"), metadata={"format": "pt"})


def read_adapter_config(path):
    with open(os.path.join(path, "adapter_config.json")) as f:
        c = json.load(f)
    if c.get("peft_type", "LORA") != "LORA":
        raise ValueError(f"{path}: peft_type {c.get('peft_type')!r}, only LORA adapters are supported")
    if c.get("bias", "none") != "none":
        raise NotImplementedError(f"{path}: bias={c['bias']!r} adapters are not implemented")
    tm = c["target_modules"]
    return LoraConfig(r=int(c["r"]), lora_alpha=c.get("lora_alpha", 8), target_modules=[tm] if isinstance(tm, str) else list(tm),
                      use_rslora=bool(c.get("use_rslora", False)), init_lora_weights=c.get("init_lora_weights", "gaussian"),
                      use_dora=bool(c.get("use_dora", False)), lora_dropout=float(c.get("lora_dropout", 0.0)))


def load_lora(model, path, scale=1.0):
    """Adapters from a peft directory onto `model` (attached first if the model carries none); `scale` multiplies s (scripts/inference.py --lora_scale)."""
    from safetensors.torch import load_file
    config = read_adapter_config(path)
    lo = getattr(model, "_lora", None)
    if lo is None:
        lo = add_lora(model, config)
    elif (lo.config.r, resolve_targets(lo.config.target_modules)) != (config.r, resolve_targets(config.target_modules)):
        raise ValueError(f"{path}: rank / targets differ from the adapters the model carries")
    else:
        lo.config = config
    lo.load_state_dict(load_file(os.path.join(path, "adapter_model.safetensors")))
    set_lora_scale(model, scale)
    return lo


def set_lora_scale(model, x):
    """s <- (lora_alpha / r) * x and re-merge; 0 gives the base model's bits."""
    lo = _adapters(model)
    lo.multiplier = float(x)
    if model._store is not None and model._engine.lora is lo:
        model._store.bump()


def merge_and_unload(model):
    """W <- W + s B A in the fp32 master of every adapted slice, then drop the adapters (peft's merge_and_unload); the parameters' requires_grad flags are
    put back to what add_lora found."""
    lo = _adapters(model)
    if model._store is not None and model._engine.lora is lo and model._store.device.type == "cuda":
        model._engine._lora_merge(into_master=True)         # the merge kernel, with its fp32 value also written over the master
        model._engine.detach_lora(remerge=False)
        model._store.bump()
    else:
        with torch.no_grad():
            named = dict(model.named_parameters())
            for name, slices in lo.slices.items():
                w = named[name + ".weight"]
                for a, b, ad in slices:
                    w[a:b] += lo.scale * (lo.params[ad + ".lora_Bt"].t().to(w.device) @ lo.params[ad + ".lora_A"].to(w.device))
        if model._engine is not None:
            model._engine.detach_lora(remerge=False)
    for p, flag in lo._frozen:
        p.requires_grad_(flag)
    model._lora = None
    return model


def _adapters(model):
    lo = getattr(model, "_lora", None)
    if lo is None:
        raise RuntimeError("the model carries no LoRA adapters (add_lora / load_lora first)")
    return lo
