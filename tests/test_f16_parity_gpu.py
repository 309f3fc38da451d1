"""The fp16-operand build (libpixart_hip_f16.so, PXA_OPERAND_DTYPE=f16) meets the north-star forward tolerance: rel-L2 <= 1e-3 against
the fp32 reference goldens, including the full-depth XL/2 of BASELINE config 1.  The operand type is a per-process choice, so the
check runs tools/f16_parity.py in a subprocess."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16_FWD_TOL = 1e-3        # BASELINE.json north_star tolerance
F16_SAMPLE_TOL = 2e-3     # 2-step CFG-4.5 sampler amplifies the forward error (bf16 build: 8.5e-3)


@pytest.mark.gpu
def test_f16_operand_build_meets_1e3_forward_parity():
    env = dict(os.environ, PXA_OPERAND_DTYPE="f16")
    env.pop("PXA_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "f16_parity.py")], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print("\n", res)
    assert res["operand"] == "f16"
    for name, e in res["cases"].items():
        assert e < (F16_SAMPLE_TOL if name.endswith(":sample") else F16_FWD_TOL), (name, e)


@pytest.mark.gpu
def test_f16_operand_build_model_suite():
    """tests/test_model_gpu.py re-run under the fp16-operand build: there its bounds are the north-star ones (forward <= 1e-3 at every
    BASELINE token geometry, loss <= 1e-3, loss-scaled gradients <= 1.2e-3 per tensor; see that file's header)."""
    env = dict(os.environ, PXA_OPERAND_DTYPE="f16")
    env.pop("PXA_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_model_gpu.py"), "-q", "-m", "gpu", "-s", "-x",
                        "-p", "no:cacheprovider"], capture_output=True, text=True, env=env, timeout=2400, cwd=ROOT)
    tail = "\n".join(l for l in r.stdout.splitlines() if ("rel-L2" in l or "grad err" in l or "passed" in l or "failed" in l or "Error" in l))
    print("\n[f16 build] " + tail.replace("\n", "\n[f16 build] "))
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_f16_operand_build_kernel_suite():
    """tests/test_kernels_gpu.py re-run against libpixart_hip_f16.so - the library bench.py times: every GEMM epilogue, the row kernels, the dK/dV /
    dQ kernel mode matrix and the full-grid B = 16 attention test, with the fp16 bounds of that file (one fp16 rounding: 5e-4; gradients 1e-3)."""
    env = dict(os.environ, PXA_OPERAND_DTYPE="f16")
    env.pop("PXA_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_kernels_gpu.py"), "-q", "-m", "gpu", "-s",
                        "-p", "no:cacheprovider"], capture_output=True, text=True, env=env, timeout=2400, cwd=ROOT)
    tail = "\n".join(l for l in r.stdout.splitlines() if ("rel-L2" in l or "passed" in l or "failed" in l or "FAILED" in l or "Error" in l))
    print("\n[f16 build] " + tail.replace("\n", "\n[f16 build] "))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_f16_operand_build_vae_kernel_suite():
    """tests/test_vae_gpu.py and tests/test_vae_conv_geometry_gpu.py re-run against libpixart_hip_f16.so - the library bench.py times: the VAE's kernel set op by
    op.  test_vae_gpu.py keeps its bf16-sized bound there; the geometry file bounds every convolution by one fp16 rounding (2^-11) against fp64."""
    env = dict(os.environ, PXA_OPERAND_DTYPE="f16")
    env.pop("PXA_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_vae_gpu.py"), os.path.join(ROOT, "tests", "test_vae_conv_geometry_gpu.py"),
                        "-q", "-m", "gpu", "-s", "-p", "no:cacheprovider"], capture_output=True, text=True, env=env, timeout=2400, cwd=ROOT)
    tail = "\n".join(l for l in r.stdout.splitlines() if ("passed" in l or "failed" in l or "FAILED" in l or "Error" in l or "positive control" in l))
    print("\n[f16 build] " + tail.replace("\n", "\n[f16 build] "))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert "skipped" not in tail, tail


@pytest.mark.gpu
def test_f16_operand_build_gradient_gemm_and_row_kernel_forms():
    """tests/test_gemm_grad_forms_gpu.py and tests/test_row_kernel_forms_gpu.py re-run against libpixart_hip_f16.so - the library bench.py times: the fp32-output
    and ragged-row GEMM forms and the row kernels' aliased / strided forms of the training step, 16-bit outputs at one fp16 rounding (5e-4) per row."""
    env = dict(os.environ, PXA_OPERAND_DTYPE="f16")
    env.pop("PXA_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gemm_grad_forms_gpu.py"), os.path.join(ROOT, "tests", "test_row_kernel_forms_gpu.py"),
                        "-q", "-m", "gpu", "-s", "-p", "no:cacheprovider"], capture_output=True, text=True, env=env, timeout=2400, cwd=ROOT)
    tail = "\n".join(l for l in r.stdout.splitlines() if ("passed" in l or "failed" in l or "FAILED" in l or "Error" in l))
    print("\n[f16 build] " + tail.replace("\n", "\n[f16 build] "))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert "skipped" not in tail, tail


@pytest.mark.gpu
def test_f16_operand_build_came_forms():
    """tests/test_came_forms_gpu.py re-run against libpixart_hip_f16.so: the optimizer's fp32 states per element as under bf16, and the 16-bit shadow - fp16 there -
    bit-equal to the parameters cast once."""
    env = dict(os.environ, PXA_OPERAND_DTYPE="f16")
    env.pop("PXA_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_came_forms_gpu.py"), "-q", "-m", "gpu", "-s", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    tail = "\n".join(l for l in r.stdout.splitlines() if ("passed" in l or "failed" in l or "FAILED" in l or "Error" in l))
    print("\n[f16 build] " + tail.replace("\n", "\n[f16 build] "))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert "skipped" not in tail, tail


F16_VAE_TOL = 4e-3        # measured 1.5e-3 ... 2.0e-3 (bf16 build: 1.2e-2 ... 1.7e-2); the reference runs this network in fp16


@pytest.mark.gpu
def test_f16_operand_build_vae_parity():
    """The VAE under the fp16-operand build - the like-for-like comparison with the reference's `.to(torch.float16)` VAE."""
    env = dict(os.environ, PXA_OPERAND_DTYPE="f16")
    env.pop("PXA_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "vae_parity.py")], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print("\n", res)
    assert res["operand"] == "f16"
    for px in ("64px", "128px", "512px_b2"):
        for name, e in res[px].items():
            assert e < F16_VAE_TOL, (px, name, e)
