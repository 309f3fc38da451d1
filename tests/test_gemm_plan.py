"""pxa_gemm's host-side dispatch, pinned without a GPU: ops.gemm_plan (pxa_gemm_plan: the argument checks, the split choice and choose_gemm of
csrc/gemm.hip, shared with pxa_gemm) for the call list of tools/gemm_dispatch.py, in the default environment and under each dispatch knob.  The knobs that
are read once per process run in a child process each; PXA_GEMM_NO_GLDS is flipped inside one process, which pins that it is read per call.

The expected lines are meant to be the parent commit's behaviour.  So far they rest on reading the parent's dispatch: the kernel-trace
comparison that is to establish them on a GPU (tools/gemm_dispatch.py under rocprofv3 --kernel-trace at both commits, --check against these plan lines) has not
been run yet.  They additionally rest on values: tests/test_gemm_call_list_gpu.py runs every launched call on the GPU under each setting (default, no_persistent,
no_half_items, no_staged_epilogue, seg_half, tile_128, tile_256x128, tile_256, no_glds, nt4, and ascending / static_items / dynamic_items with the default
plans), asserts expected() on the plan line of the very call and compares what the kernel wrote with an fp64 reference.

The seven t5_* cases (the T5 encoder's forms, added after the dispatch was pinned) were taken from ops.gemm_plan of the unchanged library and confirmed against
choose_gemm by reading: bf16-only NT at M, N >= 1024 is the persistent kernel (PLAIN; GELU for act 1 with one output and no remainder column; GENERIC for act
4 without column sums, which carries no remainder mode of its own, so PXA_GEMM_NO_HALF_ITEMS changes nothing at N = 1152); an fp32 output is never the
persistent kernel for NT, so the residual takes the two-stage kernel's direct epilogue at the tile the row count or PXA_GEMM_TILE gives, and split 1 makes the
accumulate mode 2."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gemm_dispatch as gd  # noqa: E402

# case -> (kernel instance, split, k_per_split, accumulate mode, flags: n = try_nt4, c = colsum_pass_after, r = splitk_reduce), default environment
DEFAULT = {
    "nt_plain_1024":            ("gemm_pers_kernel<0,0,0,false>", 1, 64, 0, "n"),
    "nt_plain_1152":            ("gemm_pers_kernel<0,0,2,false>", 1, 128, 0, "n"),
    "nt_plain_1280":            ("gemm_pers_kernel<0,0,0,false>", 1, 64, 0, "n"),
    "nt_plain_2048_rows":       ("gemm_pers_kernel<0,0,0,false>", 1, 256, 0, "n"),
    "nt_gelu_save_grad":        ("gemm_pers_kernel<0,1,0,false>", 1, 64, 0, ""),
    "nt_mul_aux_colsum_1024":   ("gemm_pers_kernel<0,2,0,false>", 1, 64, 0, ""),
    "nt_mul_aux_colsum_1152":   ("gemm_pers_kernel<0,2,2,false>", 1, 64, 0, ""),
    "nt_gelu_1024":             ("gemm_pers_kernel<0,7,0,false>", 1, 64, 0, ""),
    "nt_gelu_1152":             ("gemm_pers_kernel<0,3,0,false>", 1, 64, 0, ""),
    "nt_gelu_out2":             ("gemm_pers_kernel<0,3,0,false>", 1, 64, 0, ""),
    "nt_colsum":                ("gemm_pers_kernel<0,3,0,false>", 1, 64, 0, ""),
    "nn_plain_1024":            ("gemm_pers_kernel<1,0,0,false>", 1, 64, 0, ""),
    "nn_plain_1152":            ("gemm_pers_kernel<1,0,2,false>", 1, 128, 0, ""),
    "nn_gelu_save_grad":        ("gemm_pers_kernel<1,1,0,false>", 1, 64, 0, ""),
    "nn_mul_aux_colsum_1024":   ("gemm_pers_kernel<1,2,0,false>", 1, 64, 0, ""),
    "nn_mul_aux_colsum_1152":   ("gemm_pers_kernel<1,2,2,false>", 1, 64, 0, ""),
    "nn_mul_aux":               ("gemm_pers_kernel<1,3,0,false>", 1, 64, 0, ""),
    "nn_gelu_1024":             ("gemm_pers_kernel<1,3,0,false>", 1, 64, 0, ""),
    "nt_small":                 ("gemm_glds_kernel<0,128,128,2,2,1,false>", 1, 64, 0, ""),
    "nt_small_colsum":          ("gemm_glds_kernel<0,128,128,2,2,1,false>", 1, 64, 0, ""),
    "nt_small_gelu_save_grad":  ("gemm_glds_kernel<0,128,128,2,2,0,false>", 1, 64, 0, ""),
    "nt_small_gelu_out2_colsum":("gemm_glds_kernel<0,128,128,2,2,0,false>", 1, 64, 0, "c"),
    "nt_small_f32":             ("gemm_glds_kernel<0,128,128,2,2,0,false>", 1, 128, 0, ""),
    "nn_small":                 ("gemm_glds_kernel<1,128,128,2,2,1,false>", 1, 64, 0, ""),
    "tn_small":                 ("gemm_glds_kernel<2,128,128,2,2,0,false>", 1, 64, 0, ""),
    "tn_store_1024":            ("gemm_pers_kernel<2,0,0,false>", 1, 64, 0, ""),
    "tn_store_1152":            ("gemm_pers_kernel<2,0,1,false>", 1, 128, 0, ""),
    "tn_accumulate_one_slice":  ("gemm_pers_kernel<2,0,1,false>", 1, 128, 2, ""),
    "tn_split_4":               ("gemm_pers_kernel<2,0,1,false>", 4, 1024, 3, "r"),
    "tn_split_17_atomics":      ("gemm_glds_kernel<2,256,256,2,4,0,false>", 17, 64, 1, ""),
    "tn_cost_model_1152":       ("gemm_glds_kernel<2,128,128,2,2,0,false>", 6, 704, 3, "r"),
    "tn_cost_model_1024":       ("gemm_glds_kernel<2,128,128,2,2,0,false>", 6, 704, 3, "r"),
    "tn_cost_model_32_rows":    ("gemm_glds_kernel<2,128,128,2,2,0,false>", 16, 256, 3, "r"),
    "tn_cost_model_4608_rows":  ("gemm_pers_kernel<2,0,1,false>", 3, 1408, 3, "r"),
    "tn_bias":                  ("gemm_glds_kernel<2,256,256,2,4,0,false>", 1, 64, 0, ""),
    "nn_f32_accumulate":        ("gemm_glds_kernel<1,128,128,2,2,0,false>", 6, 704, 3, "r"),
    "nt_k72":                   ("gemm_kernel<0>", 1, 128, 0, ""),
    "nt_k72_colsum":            ("gemm_kernel<0>", 1, 128, 0, "c"),
    "nn_k72":                   ("gemm_kernel<1>", 1, 128, 0, ""),
    "tn_k72_accumulate":        ("gemm_kernel<2>", 1, 128, 2, ""),
    "tn_k1000_split_16":        ("gemm_kernel<2>", 16, 64, 3, "r"),
    "conv_128":                 ("gemm_pers_kernel<0,0,1,true>", 1, 576, 0, ""),
    "conv_256":                 ("gemm_pers_kernel<0,0,0,true>", 1, 576, 0, ""),
    "conv_384":                 ("gemm_pers_kernel<0,0,1,true>", 1, 576, 0, ""),
    "conv_res_128":             ("gemm_pers_kernel<0,4,1,true>", 1, 576, 0, ""),
    "conv_res_256":             ("gemm_pers_kernel<0,4,0,true>", 1, 576, 0, ""),
    "conv_res_384":             ("gemm_pers_kernel<0,4,1,true>", 1, 576, 0, ""),
    "conv_stats_128":           ("gemm_pers_kernel<0,5,1,true>", 1, 576, 0, ""),
    "conv_stats_256":           ("gemm_pers_kernel<0,5,0,true>", 1, 576, 0, ""),
    "conv_stats_384":           ("gemm_pers_kernel<0,5,1,true>", 1, 576, 0, ""),
    "conv_res_stats_128":       ("gemm_pers_kernel<0,6,1,true>", 1, 576, 0, ""),
    "conv_res_stats_256":       ("gemm_pers_kernel<0,6,0,true>", 1, 576, 0, ""),
    "conv_res_stats_384":       ("gemm_pers_kernel<0,6,1,true>", 1, 576, 0, ""),
    "conv_phase_128":           ("gemm_pers_kernel<0,5,1,true>", 1, 256, 0, ""),
    "conv_768_rows":            ("gemm_glds_kernel<0,128,128,2,2,1,true>", 1, 576, 0, ""),
    "conv_res_768_rows":        ("gemm_glds_kernel<0,128,128,2,2,0,true>", 1, 576, 0, ""),
    "conv_f32":                 ("gemm_glds_kernel<0,128,128,2,2,0,true>", 1, 576, 0, ""),
    "t5_qkv_1120_rows":         ("gemm_pers_kernel<0,0,0,false>", 1, 128, 0, "n"),
    "t5_gelu_no_bias":          ("gemm_pers_kernel<0,7,0,false>", 1, 128, 0, ""),
    "t5_mul_aux":               ("gemm_pers_kernel<0,3,0,false>", 1, 128, 0, ""),
    "t5_mul_aux_1152":          ("gemm_pers_kernel<0,3,0,false>", 1, 128, 0, ""),
    "t5_residual_1024":         ("gemm_glds_kernel<0,256,256,2,4,0,false>", 1, 128, 2, ""),
    "t5_residual_k320":         ("gemm_glds_kernel<0,256,256,2,4,0,false>", 1, 320, 2, ""),
    "t5_residual_900_rows":     ("gemm_glds_kernel<0,128,128,2,2,0,false>", 1, 320, 2, ""),
}
# setting -> the cases whose plan differs from DEFAULT: (kernel instance, flags), or ("refused", message); split, k_per_split and the accumulate mode never
# depend on a knob
CHANGED = {
    "no_persistent": {
        "nt_plain_1024":            ("gemm_glds_kernel<0,256,256,2,4,1,false>", ""),
        "nt_plain_1152":            ("gemm_glds_kernel<0,256,256,2,4,1,false>", ""),
        "nt_plain_1280":            ("gemm_glds_kernel<0,256,256,2,4,1,false>", ""),
        "nt_plain_2048_rows":       ("gemm_glds_kernel<0,256,256,2,4,1,false>", ""),
        "nt_gelu_save_grad":        ("gemm_glds_kernel<0,256,256,2,4,0,false>", ""),
        "nt_mul_aux_colsum_1024":   ("gemm_glds_kernel<0,256,256,2,4,1,false>", ""),
        "nt_mul_aux_colsum_1152":   ("gemm_glds_kernel<0,256,256,2,4,1,false>", ""),
        "nt_gelu_1024":             ("gemm_glds_kernel<0,256,256,2,4,1,false>", ""),
        "nt_gelu_1152":             ("gemm_glds_kernel<0,256,256,2,4,1,false>", ""),
        "nt_gelu_out2":             ("gemm_glds_kernel<0,256,256,2,4,0,false>", ""),
        "nt_colsum":                ("gemm_glds_kernel<0,256,256,2,4,1,false>", ""),
        "nn_plain_1024":            ("gemm_glds_kernel<1,256,256,2,4,1,false>", ""),
        "nn_plain_1152":            ("gemm_glds_kernel<1,256,256,2,4,1,false>", ""),
        "nn_gelu_save_grad":        ("gemm_glds_kernel<1,256,256,2,4,0,false>", ""),
        "nn_mul_aux_colsum_1024":   ("gemm_glds_kernel<1,256,256,2,4,1,false>", ""),
        "nn_mul_aux_colsum_1152":   ("gemm_glds_kernel<1,256,256,2,4,1,false>", ""),
        "nn_mul_aux":               ("gemm_glds_kernel<1,256,256,2,4,1,false>", ""),
        "nn_gelu_1024":             ("gemm_glds_kernel<1,256,256,2,4,1,false>", ""),
        "tn_store_1024":            ("gemm_glds_kernel<2,256,256,2,4,0,false>", ""),
        "tn_store_1152":            ("gemm_glds_kernel<2,256,256,2,4,0,false>", ""),
        "tn_accumulate_one_slice":  ("gemm_glds_kernel<2,256,256,2,4,0,false>", ""),
        "tn_split_4":               ("gemm_glds_kernel<2,256,256,2,4,0,false>", "r"),
        "tn_cost_model_4608_rows":  ("gemm_glds_kernel<2,256,256,2,4,0,false>", "r"),
        "conv_128":                 ("gemm_glds_kernel<0,128,128,2,2,1,true>", ""),
        "conv_256":                 ("gemm_glds_kernel<0,128,128,2,2,1,true>", ""),
        "conv_384":                 ("gemm_glds_kernel<0,128,128,2,2,1,true>", ""),
        "conv_res_128":             ("gemm_glds_kernel<0,128,128,2,2,0,true>", ""),
        "conv_res_256":             ("gemm_glds_kernel<0,128,128,2,2,0,true>", ""),
        "conv_res_384":             ("gemm_glds_kernel<0,128,128,2,2,0,true>", ""),
        "conv_stats_128":           ("refused", "gn_part needs the persistent implicit-convolution path"),
        "conv_stats_256":           ("refused", "gn_part needs the persistent implicit-convolution path"),
        "conv_stats_384":           ("refused", "gn_part needs the persistent implicit-convolution path"),
        "conv_res_stats_128":       ("refused", "gn_part needs the persistent implicit-convolution path"),
        "conv_res_stats_256":       ("refused", "gn_part needs the persistent implicit-convolution path"),
        "conv_res_stats_384":       ("refused", "gn_part needs the persistent implicit-convolution path"),
        "conv_phase_128":           ("refused", "gn_part needs the persistent implicit-convolution path"),
        "t5_qkv_1120_rows":         ("gemm_glds_kernel<0,256,256,2,4,1,false>", ""),
        "t5_gelu_no_bias":          ("gemm_glds_kernel<0,256,256,2,4,1,false>", ""),
        "t5_mul_aux":               ("gemm_glds_kernel<0,256,256,2,4,1,false>", ""),
        "t5_mul_aux_1152":          ("gemm_glds_kernel<0,256,256,2,4,1,false>", ""),
    },
    "no_half_items": {
        "nt_plain_1152":            ("gemm_pers_kernel<0,0,0,false>", "n"),
        "nt_mul_aux_colsum_1152":   ("gemm_pers_kernel<0,2,0,false>", ""),
        "nt_gelu_1152":             ("gemm_pers_kernel<0,7,0,false>", ""),
        "nn_plain_1152":            ("gemm_pers_kernel<1,0,0,false>", ""),
        "nn_mul_aux_colsum_1152":   ("gemm_pers_kernel<1,2,0,false>", ""),
    },
    "no_staged_epilogue": {
        "nt_small":                 ("gemm_glds_kernel<0,128,128,2,2,0,false>", ""),
        "nt_small_colsum":          ("gemm_glds_kernel<0,128,128,2,2,0,false>", "c"),
        "nn_small":                 ("gemm_glds_kernel<1,128,128,2,2,0,false>", ""),
    },
    "seg_half": {
        "conv_128":                 ("gemm_pers_kernel<0,0,2,true>", ""),
        "conv_384":                 ("gemm_pers_kernel<0,0,2,true>", ""),
        "conv_res_128":             ("gemm_pers_kernel<0,4,2,true>", ""),
        "conv_res_384":             ("gemm_pers_kernel<0,4,2,true>", ""),
        "conv_stats_128":           ("gemm_pers_kernel<0,5,2,true>", ""),
        "conv_stats_384":           ("gemm_pers_kernel<0,5,2,true>", ""),
        "conv_res_stats_128":       ("gemm_pers_kernel<0,6,2,true>", ""),
        "conv_res_stats_384":       ("gemm_pers_kernel<0,6,2,true>", ""),
        "conv_phase_128":           ("gemm_pers_kernel<0,5,2,true>", ""),
    },
    "tile_128": {
        "nt_plain_1024":            ("gemm_glds_kernel<0,128,128,2,2,1,false>", ""),
        "nt_plain_1152":            ("gemm_glds_kernel<0,128,128,2,2,1,false>", ""),
        "nt_plain_1280":            ("gemm_glds_kernel<0,128,128,2,2,1,false>", ""),
        "nt_plain_2048_rows":       ("gemm_glds_kernel<0,128,128,2,2,1,false>", ""),
        "nt_gelu_save_grad":        ("gemm_glds_kernel<0,128,128,2,2,0,false>", ""),
        "nt_mul_aux_colsum_1024":   ("gemm_glds_kernel<0,128,128,2,2,1,false>", ""),
        "nt_mul_aux_colsum_1152":   ("gemm_glds_kernel<0,128,128,2,2,1,false>", ""),
        "nt_gelu_1024":             ("gemm_glds_kernel<0,128,128,2,2,1,false>", ""),
        "nt_gelu_1152":             ("gemm_glds_kernel<0,128,128,2,2,1,false>", ""),
        "nt_gelu_out2":             ("gemm_glds_kernel<0,128,128,2,2,0,false>", ""),
        "nt_colsum":                ("gemm_glds_kernel<0,128,128,2,2,1,false>", ""),
        "nn_plain_1024":            ("gemm_glds_kernel<1,128,128,2,2,1,false>", ""),
        "nn_plain_1152":            ("gemm_glds_kernel<1,128,128,2,2,1,false>", ""),
        "nn_gelu_save_grad":        ("gemm_glds_kernel<1,128,128,2,2,0,false>", ""),
        "nn_mul_aux_colsum_1024":   ("gemm_glds_kernel<1,128,128,2,2,1,false>", ""),
        "nn_mul_aux_colsum_1152":   ("gemm_glds_kernel<1,128,128,2,2,1,false>", ""),
        "nn_mul_aux":               ("gemm_glds_kernel<1,128,128,2,2,1,false>", ""),
        "nn_gelu_1024":             ("gemm_glds_kernel<1,128,128,2,2,1,false>", ""),
        "tn_store_1024":            ("gemm_glds_kernel<2,128,128,2,2,0,false>", ""),
        "tn_store_1152":            ("gemm_glds_kernel<2,128,128,2,2,0,false>", ""),
        "tn_accumulate_one_slice":  ("gemm_glds_kernel<2,128,128,2,2,0,false>", ""),
        "tn_split_4":               ("gemm_glds_kernel<2,128,128,2,2,0,false>", "r"),
        "tn_split_17_atomics":      ("gemm_glds_kernel<2,128,128,2,2,0,false>", ""),
        "tn_cost_model_4608_rows":  ("gemm_glds_kernel<2,128,128,2,2,0,false>", "r"),
        "tn_bias":                  ("gemm_glds_kernel<2,128,128,2,2,0,false>", ""),
        "t5_qkv_1120_rows":         ("gemm_glds_kernel<0,128,128,2,2,1,false>", ""),
        "t5_gelu_no_bias":          ("gemm_glds_kernel<0,128,128,2,2,1,false>", ""),
        "t5_mul_aux":               ("gemm_glds_kernel<0,128,128,2,2,1,false>", ""),
        "t5_mul_aux_1152":          ("gemm_glds_kernel<0,128,128,2,2,1,false>", ""),
        "t5_residual_1024":         ("gemm_glds_kernel<0,128,128,2,2,0,false>", ""),
        "t5_residual_k320":         ("gemm_glds_kernel<0,128,128,2,2,0,false>", ""),
    },
    "tile_256x128": {
        "nt_plain_1024":            ("gemm_glds_kernel<0,256,128,4,2,1,false>", ""),
        "nt_plain_1152":            ("gemm_glds_kernel<0,256,128,4,2,1,false>", ""),
        "nt_plain_1280":            ("gemm_glds_kernel<0,256,128,4,2,1,false>", ""),
        "nt_plain_2048_rows":       ("gemm_glds_kernel<0,256,128,4,2,1,false>", ""),
        "nt_gelu_save_grad":        ("gemm_glds_kernel<0,256,128,4,2,0,false>", ""),
        "nt_mul_aux_colsum_1024":   ("gemm_glds_kernel<0,256,128,4,2,1,false>", ""),
        "nt_mul_aux_colsum_1152":   ("gemm_glds_kernel<0,256,128,4,2,1,false>", ""),
        "nt_gelu_1024":             ("gemm_glds_kernel<0,256,128,4,2,1,false>", ""),
        "nt_gelu_1152":             ("gemm_glds_kernel<0,256,128,4,2,1,false>", ""),
        "nt_gelu_out2":             ("gemm_glds_kernel<0,256,128,4,2,0,false>", ""),
        "nt_colsum":                ("gemm_glds_kernel<0,256,128,4,2,1,false>", ""),
        "nn_plain_1024":            ("gemm_glds_kernel<1,256,128,4,2,1,false>", ""),
        "nn_plain_1152":            ("gemm_glds_kernel<1,256,128,4,2,1,false>", ""),
        "nn_gelu_save_grad":        ("gemm_glds_kernel<1,256,128,4,2,0,false>", ""),
        "nn_mul_aux_colsum_1024":   ("gemm_glds_kernel<1,256,128,4,2,1,false>", ""),
        "nn_mul_aux_colsum_1152":   ("gemm_glds_kernel<1,256,128,4,2,1,false>", ""),
        "nn_mul_aux":               ("gemm_glds_kernel<1,256,128,4,2,1,false>", ""),
        "nn_gelu_1024":             ("gemm_glds_kernel<1,256,128,4,2,1,false>", ""),
        "nt_small":                 ("gemm_glds_kernel<0,256,128,4,2,1,false>", ""),
        "nt_small_colsum":          ("gemm_glds_kernel<0,256,128,4,2,1,false>", ""),
        "nt_small_gelu_save_grad":  ("gemm_glds_kernel<0,256,128,4,2,0,false>", ""),
        "nt_small_gelu_out2_colsum":("gemm_glds_kernel<0,256,128,4,2,0,false>", "c"),
        "nt_small_f32":             ("gemm_glds_kernel<0,256,128,4,2,0,false>", ""),
        "nn_small":                 ("gemm_glds_kernel<1,256,128,4,2,1,false>", ""),
        "tn_small":                 ("gemm_glds_kernel<2,256,128,4,2,0,false>", ""),
        "tn_store_1024":            ("gemm_glds_kernel<2,256,128,4,2,0,false>", ""),
        "tn_store_1152":            ("gemm_glds_kernel<2,256,128,4,2,0,false>", ""),
        "tn_accumulate_one_slice":  ("gemm_glds_kernel<2,256,128,4,2,0,false>", ""),
        "tn_split_4":               ("gemm_glds_kernel<2,256,128,4,2,0,false>", "r"),
        "tn_split_17_atomics":      ("gemm_glds_kernel<2,256,128,4,2,0,false>", ""),
        "tn_cost_model_1152":       ("gemm_glds_kernel<2,256,128,4,2,0,false>", "r"),
        "tn_cost_model_1024":       ("gemm_glds_kernel<2,256,128,4,2,0,false>", "r"),
        "tn_cost_model_32_rows":    ("gemm_glds_kernel<2,256,128,4,2,0,false>", "r"),
        "tn_cost_model_4608_rows":  ("gemm_glds_kernel<2,256,128,4,2,0,false>", "r"),
        "tn_bias":                  ("gemm_glds_kernel<2,256,128,4,2,0,false>", ""),
        "nn_f32_accumulate":        ("gemm_glds_kernel<1,256,128,4,2,0,false>", "r"),
        "t5_qkv_1120_rows":         ("gemm_glds_kernel<0,256,128,4,2,1,false>", ""),
        "t5_gelu_no_bias":          ("gemm_glds_kernel<0,256,128,4,2,1,false>", ""),
        "t5_mul_aux":               ("gemm_glds_kernel<0,256,128,4,2,1,false>", ""),
        "t5_mul_aux_1152":          ("gemm_glds_kernel<0,256,128,4,2,1,false>", ""),
        "t5_residual_1024":         ("gemm_glds_kernel<0,256,128,4,2,0,false>", ""),
        "t5_residual_k320":         ("gemm_glds_kernel<0,256,128,4,2,0,false>", ""),
        "t5_residual_900_rows":     ("gemm_glds_kernel<0,256,128,4,2,0,false>", ""),
    },
    "tile_256": {
        "nt_small":                 ("gemm_pers_kernel<0,0,0,false>", "n"),
        "nt_small_colsum":          ("gemm_pers_kernel<0,3,0,false>", ""),
        "nt_small_gelu_save_grad":  ("gemm_pers_kernel<0,1,0,false>", ""),
        "nt_small_gelu_out2_colsum":("gemm_pers_kernel<0,3,0,false>", ""),
        "nt_small_f32":             ("gemm_glds_kernel<0,256,256,2,4,0,false>", ""),
        "nn_small":                 ("gemm_pers_kernel<1,0,0,false>", ""),
        "tn_small":                 ("gemm_pers_kernel<2,0,0,false>", ""),
        "tn_cost_model_1152":       ("gemm_pers_kernel<2,0,1,false>", "r"),
        "tn_cost_model_1024":       ("gemm_pers_kernel<2,0,0,false>", "r"),
        "tn_cost_model_32_rows":    ("gemm_pers_kernel<2,0,1,false>", "r"),
        "nn_f32_accumulate":        ("gemm_glds_kernel<1,256,256,2,4,0,false>", "r"),
        "t5_residual_900_rows":     ("gemm_glds_kernel<0,256,256,2,4,0,false>", ""),
    },
    "no_glds": {
        "nt_plain_1024":            ("gemm_kernel<0>", ""),
        "nt_plain_1152":            ("gemm_kernel<0>", ""),
        "nt_plain_1280":            ("gemm_kernel<0>", ""),
        "nt_plain_2048_rows":       ("gemm_kernel<0>", ""),
        "nt_gelu_save_grad":        ("gemm_kernel<0>", ""),
        "nt_mul_aux_colsum_1024":   ("gemm_kernel<0>", "c"),
        "nt_mul_aux_colsum_1152":   ("gemm_kernel<0>", "c"),
        "nt_gelu_1024":             ("gemm_kernel<0>", ""),
        "nt_gelu_1152":             ("gemm_kernel<0>", ""),
        "nt_gelu_out2":             ("gemm_kernel<0>", ""),
        "nt_colsum":                ("gemm_kernel<0>", "c"),
        "nn_plain_1024":            ("gemm_kernel<1>", ""),
        "nn_plain_1152":            ("gemm_kernel<1>", ""),
        "nn_gelu_save_grad":        ("gemm_kernel<1>", ""),
        "nn_mul_aux_colsum_1024":   ("gemm_kernel<1>", "c"),
        "nn_mul_aux_colsum_1152":   ("gemm_kernel<1>", "c"),
        "nn_mul_aux":               ("gemm_kernel<1>", ""),
        "nn_gelu_1024":             ("gemm_kernel<1>", ""),
        "nt_small":                 ("gemm_kernel<0>", ""),
        "nt_small_colsum":          ("gemm_kernel<0>", "c"),
        "nt_small_gelu_save_grad":  ("gemm_kernel<0>", ""),
        "nt_small_gelu_out2_colsum":("gemm_kernel<0>", "c"),
        "nt_small_f32":             ("gemm_kernel<0>", ""),
        "nn_small":                 ("gemm_kernel<1>", ""),
        "tn_small":                 ("gemm_kernel<2>", ""),
        "tn_store_1024":            ("gemm_kernel<2>", ""),
        "tn_store_1152":            ("gemm_kernel<2>", ""),
        "tn_accumulate_one_slice":  ("gemm_kernel<2>", ""),
        "tn_split_4":               ("gemm_kernel<2>", "r"),
        "tn_split_17_atomics":      ("gemm_kernel<2>", ""),
        "tn_cost_model_1152":       ("gemm_kernel<2>", "r"),
        "tn_cost_model_1024":       ("gemm_kernel<2>", "r"),
        "tn_cost_model_32_rows":    ("gemm_kernel<2>", "r"),
        "tn_cost_model_4608_rows":  ("gemm_kernel<2>", "r"),
        "tn_bias":                  ("gemm_kernel<2>", ""),
        "nn_f32_accumulate":        ("gemm_kernel<1>", "r"),
        "t5_qkv_1120_rows":         ("gemm_kernel<0>", ""),
        "t5_gelu_no_bias":          ("gemm_kernel<0>", ""),
        "t5_mul_aux":               ("gemm_kernel<0>", ""),
        "t5_mul_aux_1152":          ("gemm_kernel<0>", ""),
        "t5_residual_1024":         ("gemm_kernel<0>", ""),
        "t5_residual_k320":         ("gemm_kernel<0>", ""),
        "t5_residual_900_rows":     ("gemm_kernel<0>", ""),
    },
}


def plan_fields(line):
    w = line.split()
    f = dict(kv.split("=") for kv in w[1:])
    assert list(f) == ["split", "k_per_split", "accumulate", "try_nt4", "colsum_pass_after", "splitk_reduce"], line
    flags = "n" * int(f["try_nt4"]) + "c" * int(f["colsum_pass_after"]) + "r" * int(f["splitk_reduce"])
    return (w[0], int(f["split"]), int(f["k_per_split"]), int(f["accumulate"]), flags)


def plans_of_this_process():
    """{case: plan fields, or ("refused", text)} of every case of the list in this process's environment, on CPU tensors"""
    from pixart_sigma_amd import ops
    from pixart_sigma_amd.lib import PixartHipError
    out = {}
    for i, (name, spec) in enumerate(gd.ALL_CASES):
        a, b, kw = gd.make_call(spec, "cpu", values=False)
        try:
            out[name] = plan_fields(ops.gemm_plan(a, b, **kw))
        except PixartHipError as e:
            out[name] = ("refused", str(e))
    return out


def expected(setting):
    want = dict(DEFAULT)
    for name, v in CHANGED.get(setting, {}).items():
        want[name] = v if v[0] == "refused" else (v[0], *DEFAULT[name][1:4], v[1])
    for name, spec in gd.ALL_CASES:
        if "refused" in spec:
            want[name] = ("refused", spec["refused"])
    return want


def assert_plans(got, setting):
    want = expected(setting)
    assert list(got) == [n for n, _ in gd.ALL_CASES] and set(want) == set(got)
    for name, w in want.items():
        if w[0] == "refused":
            assert got[name][0] == "refused" and "pxa_gemm_plan failed (rc=-1): pxa_gemm: " + w[1] in got[name][1], (setting, name, got[name])
        else:
            assert got[name] == w, (setting, name, got[name], w)


def test_tables_cover_the_call_list():
    launched = [n for n, s in gd.ALL_CASES if "refused" not in s]
    assert list(DEFAULT) == launched and len(set(launched)) == len(launched)
    assert set(CHANGED) | {"default", "nt4"} == set(gd.SETTINGS)
    for setting, rows in CHANGED.items():
        assert rows and set(rows) <= set(DEFAULT), setting
    named = {v[0] for v in DEFAULT.values()} | {v[0] for rows in CHANGED.values() for v in rows.values() if v[0] != "refused"}
    # every reachable instance family and flavour is named somewhere: 3 simple, 12 convolution + 15 token persistent, 14 of the 20 two-stage instances
    assert sum(n.startswith("gemm_kernel<") for n in named) == 3
    assert sum(n.startswith("gemm_pers_kernel<") for n in named) == 27
    assert sum(n.startswith("gemm_glds_kernel<") for n in named) == 17


def plans_in_a_child(env_add, *argv):
    """the last line a fresh process prints when it runs this file: no PXA_GEMM_* variable but env_add, no static of the library frozen yet"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("PXA_GEMM_")}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *argv], capture_output=True, text=True, cwd=ROOT, env={**env, **env_add})
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.splitlines()[-1])


def test_default_environment_and_per_call_no_glds():
    """one child, four rounds: default; PXA_GEMM_NO_GLDS set (read on every call: the same process now plans the register-staged kernel); unset again;
    PXA_GEMM_NO_PERSISTENT set (read once per process, and that was before: no effect any more)"""
    rounds = plans_in_a_child({}, "flip")
    assert len(rounds) == 4
    for got, setting in zip(rounds, ("default", "no_glds", "default", "default")):
        assert_plans({k: tuple(v) for k, v in got.items()}, setting)


@pytest.mark.parametrize("setting", [s for s in gd.SETTINGS if s not in ("default", "no_glds")])
def test_once_per_process_knob_in_a_child(setting):
    got = {k: tuple(v) for k, v in plans_in_a_child(gd.SETTINGS[setting]).items()}
    assert_plans(got, "default" if setting == "nt4" else setting)      # PXA_GEMM_NT4 is gemm_nt4.hip's own switch: the plan only says try_nt4


def test_refused_plan_sets_the_error_of_pxa_gemm():
    """the C entry itself: same return code and pxa_last_error() as pxa_gemm for a refused block; a short text buffer is an error, not a truncation"""
    import ctypes as C
    from pixart_sigma_amd import lib
    L = lib.load()
    g = lib.GemmArgs()
    buf = C.create_string_buffer(256)
    assert L.pxa_gemm_plan(C.byref(g), buf, len(buf)) == -1 and L.pxa_last_error() == b"pxa_gemm: null operand"
    g.A = g.B = g.out_bf16 = 64                                        # never dereferenced
    g.M = g.N = g.K = g.lda = g.ldb = g.ld_out = 1024
    assert L.pxa_gemm_plan(C.byref(g), buf, len(buf)) == 0 and buf.value.decode().split()[0] == "gemm_pers_kernel<0,0,0,false>"
    assert L.pxa_gemm_plan(C.byref(g), buf, 16) == -1 and b"too small" in L.pxa_last_error()
    g.N = 1028
    assert L.pxa_gemm_plan(C.byref(g), buf, len(buf)) == -1 and L.pxa_last_error() == b"pxa_gemm: N=1028 must be a multiple of 8"


if __name__ == "__main__":                                             # the children of the tests above
    if sys.argv[1:] == ["flip"]:
        rounds = [plans_of_this_process()]
        for name, value in (("PXA_GEMM_NO_GLDS", "1"), ("PXA_GEMM_NO_GLDS", None), ("PXA_GEMM_NO_PERSISTENT", "1")):
            os.environ.pop(name) if value is None else os.environ.__setitem__(name, value)
            rounds.append(plans_of_this_process())
        print(json.dumps(rounds))
    else:
        print(json.dumps(plans_of_this_process()))
