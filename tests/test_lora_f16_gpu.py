"""The LoRA kernel and model tests re-run against the fp16-operand build (libpixart_hip_f16.so, PXA_OPERAND_DTYPE=f16), the way tests/test_f16_parity_gpu.py
re-runs the other GPU files: the operand type is a per-process choice, so the files run in a subprocess.  Their bounds are per build (one fp16 rounding of
t / u in the adapter gradients; forward <= 1e-3, loss <= 1e-3, gradients <= 1.2e-3 at model level)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("file", ["test_lora_kernels_gpu.py", "test_lora_model_gpu.py"])
def test_f16_operand_build_lora_suite(file):
    env = dict(os.environ, PXA_OPERAND_DTYPE="f16")
    env.pop("PXA_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", file), "-q", "-m", "gpu", "-s", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=env, timeout=1200, cwd=ROOT)
    tail = "\n".join(l for l in r.stdout.splitlines() if ("rel-L2" in l or "passed" in l or "failed" in l or "FAILED" in l or "Error" in l))
    print("\n[f16 build] " + tail.replace("\n", "\n[f16 build] "))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert "skipped" not in tail, tail
