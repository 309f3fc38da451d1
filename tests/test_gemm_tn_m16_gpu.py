"""The TN (weight-gradient) GEMM into fp32 at the smallest shapes where the main loop of gemm_pers_kernel<2, ...> changes path: k-unit counts around the ring
depth and the two-unit pairs of the 16-row build (csrc/gemm.hip: run_units / run_units_tn), the paired remainder column with a padded last pair, every
accumulate mode, more items than CUs (two hand-overs in a row per workgroup), and the -DGEMM_WAIT_ALL=1 build bit for bit.  The file runs against whatever
library the process loads: the product build, or an A/B build through PXA_LIB_PATH (tools/build_variant.py ... -DGEMM_M16=7, the 16-row TN main loop).

Reference: the fp64 product of the same 16-bit operands.  Bound, guard bands, NaN poison: those of tests/test_gemm_grad_forms_gpu.py, imported.

What reaches which kernel (asserted per case through ops.gemm_plan, printed for the others):
  * the persistent kernel takes k ranges that are multiples of 64 only, i.e. an EVEN number of 32-deep units >= 2; K % 64 != 0 runs gemm_kernel<2>.  The sweep
    K = 32 ... 288 at 256 x 256 with split_k = 1 is kept as the issue states it - it runs the 128 x 128 kernels there (M, N < 1024 without a cost-model hint) -
    and is repeated at 1024 x 1024, where split_k = 1 maps to the persistent kernel for K = 64, 128, 192, 256, 320, 384, 448, 512 (2, 4, ... 16 units:
    nk == 2, the 4-unit and 6-unit tails, and 1 - 5 steady-state pairs in front of them).
  * TH == 1 (half items) exists only in the 16-bit NT / NN instances (RM == 2); no TN plan has it.  The one half-item case here is therefore an NT call."""
import functools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gemm_grad_forms_gpu import (BK, MINUS_ZERO32, SENTINEL16, SENTINEL32, Banded, accumulate_twice, check_16, check_f32, plan_of,  # noqa: E402
                                      poison_splitk_workspace, surviving_slices, tn_operands)
from test_kernels_gpu import _gpu_rnd, _opd, bf, ops  # noqa: E402,F401

PERS_TN = "gemm_pers_kernel<2,0,"


@functools.lru_cache(maxsize=None)
def operands(M, N, K):
    return tn_operands(M, N, K)


def store_case(ops, M, N, K, split_k, want_kernel=None):
    """plain store into a NaN-filled, banded output"""
    a, b, ref = operands(M, N, K)
    out = Banded(M, N, torch.float32, SENTINEL32)
    out.view.fill_(float("nan"))
    plan = plan_of(ops, a, b, ops.TN, out_f32=out.view, accumulate=False, split_k=split_k)
    print(f"\nTN {M}x{N} K={K} split_k={split_k}: {plan}")
    if want_kernel is not None:
        assert plan["kernel"].startswith(want_kernel), plan
    ops.gemm(a, b, ops.TN, out_f32=out.view, accumulate=False, split_k=split_k)
    torch.cuda.synchronize()
    out.assert_intact(f"TN store {M}x{N} K={K}")
    check_f32(f"TN store {M}x{N} K={K} split_k={split_k}", out.view, ref)


@pytest.mark.parametrize("K", [32, 64, 96, 128, 160, 192, 224, 288])
def test_k_units_small_tile(ops, K):
    """1 - 7 and 9 units of 32 at 256 x 256, split_k = 1."""
    store_case(ops, 256, 256, K, 1)


@pytest.mark.parametrize("K", [64, 128, 192, 256, 320, 384, 448, 512])
def test_k_units_persistent(ops, K):
    """2, 4, ... 16 units per item in the persistent kernel: every tail of run_units / run_units_tn and up to five steady-state pairs."""
    assert K % BK == 0
    store_case(ops, 1024, 1024, K, 1, PERS_TN + "0,")


@pytest.mark.parametrize("M", [256, 1152])
def test_remainder_column(ops, M):
    """N = 384 (N % 256 == 128) at 1 and 5 m-tiles (the last one padded), K = 320."""
    assert 384 % 256 == 128 and 320 % BK == 0
    store_case(ops, M, 384, 320, 1)


def test_paired_remainder_column_persistent(ops):
    """2304 x 1152: 9 m-tiles, so the last paired item's second half lies beyond M; 10 units per item."""
    assert (2304 + 255) // 256 == 9 and 1152 % 256 == 128
    store_case(ops, 2304, 1152, 320, 1, PERS_TN + "1,")


def test_half_items_nt(ops):
    """the TH == 1 path: NT with a 16-bit output at N % 256 == 128 (see the header)."""
    M, N, K = 1024, 1152, 128
    a, w = bf(_gpu_rnd(M, K, seed=1)), bf(_gpu_rnd(N, K, scale=K ** -0.5, seed=2))
    ref = a.double() @ w.double().t()
    out = Banded(M, N, _opd(), SENTINEL16)
    out.view.fill_(float("nan"))
    assert plan_of(ops, a, w, ops.NT, out=out.view)["kernel"] == "gemm_pers_kernel<0,0,2,false>"
    ops.gemm(a, w, ops.NT, out=out.view)
    torch.cuda.synchronize()
    out.assert_intact("NT half items")
    check_16(f"NT half items {M}x{N} K={K}", out.view, ref)


@pytest.mark.parametrize("K,split_k", [(960, 0), (1000, 0), (1000, 4), (960, 4)])
def test_accumulate_modes(ops, K, split_k):
    """accumulate twice into a random buffer: the cost model's split (split_k = 0) and an explicit split of 4 with a ragged last slice, at K = 1000 (K % 64 != 0:
    the fallback kernel) and at K = 960 (slices of 256, 256, 256, 192 in the persistent kernel, slabs + reduce)."""
    M = N = 1152
    a, b, ref = operands(M, N, K)
    out = Banded(M, N, torch.float32, MINUS_ZERO32)
    poison_splitk_workspace(ops, a, M, N)
    plan = plan_of(ops, a, b, ops.TN, out_f32=out.view, accumulate=True, split_k=split_k)
    print(f"\nTN {M}x{N} K={K} split_k={split_k}: {plan}")
    if split_k == 4:
        assert surviving_slices(K, 4) == (4, 256) and plan["split"] == 4
        assert plan["kernel"] == ("gemm_pers_kernel<2,0,1,false>" if K % BK == 0 else "gemm_kernel<2>"), plan
    accumulate_twice(ops, f"TN {M}x{N} K={K} split_k={split_k}", a, b, ops.TN, out, ref, split_k=split_k, poison=True)


def test_atomic_mode_short_workspace(ops):
    """accumulate mode 1: 17 surviving slices, 16 slabs of workspace (as tests/test_gemm_grad_forms_gpu.py::test_atomic_accumulate_when_workspace_is_short)."""
    M = N = 1152
    K, split_k = 1088, 17
    a, b, ref = operands(M, N, K)
    out = Banded(M, N, torch.float32, MINUS_ZERO32)
    saved = ops._SPLITK_WS.pop(a.device, None)
    try:
        accumulate_twice(ops, f"TN {M}x{N} K={K} atomics", a, b, ops.TN, out, ref, split_k=split_k, poison=False)
        plan = plan_of(ops, a, b, ops.TN, out_f32=out.view, accumulate=True, split_k=split_k)
        assert (plan["split"], plan["accumulate"]) == (17, 1), plan
    finally:
        cur = ops._SPLITK_WS.get(a.device)
        if saved is not None and (cur is None or saved.numel() > cur.numel()):
            ops._SPLITK_WS[a.device] = saved


def test_more_items_than_cus(ops):
    """4608 x 4608 at K = 128: 324 items of 4 units on at most 304 workgroups - the hand-over with its prefetch and counted waits runs twice in a row."""
    assert (4608 // 256) ** 2 > 304
    store_case(ops, 4608, 4608, 128, 1, PERS_TN + "0,")


def test_wait_all_build_gives_the_same_bits(tmp_path):
    """-DGEMM_WAIT_ALL=1 (every counted vmcnt wait becomes vmcnt(0)) against the library of this process, on three persistent TN shapes (tools/gemm_tn_dump.py),
    both in child processes, built the way test_kernels_gpu.py::test_gemm_counted_waits_match_full_waits builds it (reused when newer than the sources)."""
    import shutil
    from conftest import ROOT
    from pixart_sigma_amd import lib as L_
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc on this box: the debug variant cannot be built")
    env = dict(os.environ, VARIANT_OPERAND=L_.OPERAND, PXA_OPERAND_DTYPE=L_.OPERAND)
    env.pop("PXA_LIB_PATH", None)                               # (the product library and its debug twin, whatever A/B build the parent process runs)
    name = "waitall_" + L_.OPERAND
    flags = ["-DGEMM_WAIT_ALL=1"]
    variant = os.path.join(ROOT, "pixart_sigma_amd", "variants", f"lib_{name}.so")
    csrc = os.path.join(ROOT, "pixart_sigma_amd", "csrc")
    newest = max(os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc))
    if not os.path.exists(variant) or os.path.getmtime(variant) < newest:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "build_variant.py"), name, "csrc/gemm.hip", *flags], capture_output=True, text=True,
                           env=env, cwd=ROOT, timeout=1200)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    outs = {}
    for tag, e in (("product", env), ("waitall", dict(env, PXA_LIB_PATH=variant))):
        out = str(tmp_path / f"{tag}.pt")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gemm_tn_dump.py"), out], capture_output=True, text=True, env=e, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        outs[tag] = torch.load(out, weights_only=False)
    assert set(outs["product"]) == set(outs["waitall"]) and len(outs["product"]) == 3
    for k, a in outs["product"].items():
        assert torch.isfinite(a).all(), k
        assert torch.equal(a, outs["waitall"][k]), k
