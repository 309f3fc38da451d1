"""train_scripts/train_lora.py end to end on the GPU, one subprocess under `timeout`: PixArtMS_XL_2 at 256px (the only registered denoiser), batch 2, fp16
operands with the loss scaler, gradient accumulation 2, rank-4 adapters on a randomly initialised base, 2 steps with an adapter checkpoint at step 2.
Nothing is asserted about the adapters' values moving: with a randomly initialised base the final layer is zero, and so are the blocks' gradients."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_train_lora_entry_point_fp16_accumulation(tmp_path):
    cfg = tmp_path / "cfg.py"
    cfg.write_text("image_size = 256\ntrain_batch_size = 2\nmodel_max_length = 16\nmixed_precision = 'fp16'\ngradient_accumulation_steps = 2\n"
                   "log_interval = 1\nsave_model_steps = 2\n")
    env = {k: v for k, v in os.environ.items() if k not in ("PXA_OPERAND_DTYPE", "PXA_LIB_PATH")}
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "train_scripts", "train_lora.py"), str(cfg), "--synthetic",
                        "--max-steps", "2", "--rank", "4", "--work-dir", str(tmp_path / "w")], capture_output=True, text=True, cwd=ROOT, env=env)
    print("\n" + r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("step ")]
    assert len(lines) == 2 and "operands fp16" in r.stdout and "LoRA r=4" in r.stdout
    for ln in lines:
        assert "loss_scale" in ln and math.isfinite(float(ln.split("loss ")[1].split()[0])), ln
    from safetensors.torch import load_file
    for d in (tmp_path / "w" / "lora", tmp_path / "w" / "checkpoints" / "lora_step_2"):
        assert json.loads((d / "adapter_config.json").read_text())["r"] == 4
        tensors = load_file(str(d / "adapter_model.safetensors"))
        assert tensors and all(torch.isfinite(v).all() for v in tensors.values())
