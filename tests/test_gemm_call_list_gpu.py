"""The VALUES of every launched call of tools/gemm_dispatch.py:ALL_CASES, under every dispatch knob: what the kernel that launch_instance's switch launches
(csrc/gemm.hip, gemm_nt4.hip) wrote, against gd.reference() - plain torch in fp64 from the 16-bit-rounded operands.  tests/test_gemm_plan.py pins which
instance the plan NAMES, on CPU tensors; here the same plan line is asserted beside the numbers, so a value belongs to the instance named.

One test and one fresh child process per setting (the knobs are read once per process; this file's __main__ is the child): every entry of gd.SETTINGS and
three that live here only and must not change a plan - ascending (PXA_GEMM_ASCENDING=1), static_items (PXA_GEMM_STATIC=1), dynamic_items
(PXA_GEMM_DYNAMIC=1).  The child builds each call with make_call(spec, "cuda:0", seed=i), fills accumulate targets with seeded N(0, 1) values and every
other output with NaN (gd.prepare_outputs), records ops.gemm_plan's line, calls ops.gemm, synchronises and compares (gd.errors); it prints one JSON object
and stops at the first HIP error.  After a child that timed out, died on a signal, exited 134 / 139 or reported a HIP error, the remaining settings skip:
nothing more is started on a card that has just faulted.

Figures.  rel-L2 per 64-row x 64-column block of each output (a wave's store tile), the maximum over blocks: a global rel-L2 dilutes one bad tile of a
1024 x 1152 output to nothing.  Any non-finite value where one is specified fails.  Of an implicit convolution only the interior padded-pixel rows are
specified.  Bounds, from the project and not from the kernels under test:
  16-bit outputs        BF16_TOL of tests/test_kernels_gpu.py (4e-3 with bf16 operands, 5e-4 under PXA_OPERAND_DTYPE=f16);
  fp32 outputs          2e-5 (test_gemm_tn_splitk_accumulate: K = 4096, split 8);
  column sums           1e-4 against the sums of the stored 16-bit values, 5e-3 against the reference's (test_gemm_persistent_kernel_epilogues);
  gn_part               what check_statistics of tests/test_vae_conv_geometry_gpu.py asserts.
The reference alone, rounded once to the type of the output and held against itself with the same figures on the CPU, over all 64 cases, the seven T5 forms
included (worst block): 16-bit outputs 1.84e-3 (out, t5_gelu_no_bias) and 2.06e-3 (out2 = GELU', nt_gelu_save_grad) of the 4e-3 with bf16 operands, 2.26e-4
and 2.44e-4 of the 5e-4 with fp16 operands; fp32 outputs 2.8e-8 (t5_residual_900_rows) of the 2e-5; column sums of the rounded values against the reference's
2.48e-3 (bf16) / 2.7e-4 (fp16) of the 5e-3, against the stored values 3e-8 of the 1e-4.  No case's reference alone uses more than 52 % of its bound (the T5
cases: 46 %), so no bound is widened.  The T5 forms on an MI355X, worst block over the 13 settings (bf16 operands): t5_qkv_1120_rows 1.73e-3, t5_gelu_no_bias
1.84e-3, t5_mul_aux 1.83e-3, t5_mul_aux_1152 1.79e-3 - the reference's own rounding - and the fp32 residuals t5_residual_1024 5.3e-8, t5_residual_k320 7.9e-8,
t5_residual_900_rows 7.8e-8.
What reading the kernels for this list found: the LDS-staged epilogue of gemm_glds_kernel summed the column sums from the fp32 values BEFORE they were rounded
(about 1e-3 from the sums of the stored bf16 values, ten times the 1e-4), where the persistent kernel and the separate pass sum what is stored, as
include/pixart_hip.h says; it now sums the packed values (cases nt_small_colsum and, under the tile / no_persistent knobs, every colsum case).
test_the_checker_has_teeth (CPU) feeds the comparison a correct rounded result and eight defective ones, three of them in the T5 encoder's forms (the fp32
residual overwritten, its last 32 rows added twice, x aux of the ragged tile one row off)."""
import json
import os
import subprocess
import sys
import time

import pytest
import torch

from conftest import ROOT, record_parity
from test_kernels_gpu import BF16_TOL, F16_BUILD  # noqa: E402
import test_gemm_plan as tgp  # noqa: E402  (puts tools/ on the path)
import gemm_dispatch as gd  # noqa: E402

OWN_SETTINGS = {"ascending": {"PXA_GEMM_ASCENDING": "1"}, "static_items": {"PXA_GEMM_STATIC": "1"}, "dynamic_items": {"PXA_GEMM_DYNAMIC": "1"}}
ALL_SETTINGS = {**gd.SETTINGS, **OWN_SETTINGS}
F32_TOL, COLSUM_STORED_TOL, COLSUM_REFERENCE_TOL = 2e-5, 1e-4, 5e-3
CHILD_TIMEOUT = 12         # seconds: three times the measured wall time of the slowest setting's child (process start and library load dominate and vary).  On an
#                            MI355X the 13 children of the 64-case list took 3.1 - 3.8 s (the first one started, `default`, 3.8 s), the children of the 57-case list
#                            before the T5 forms 2.8 - 3.5 s; each test records its child's wall time with record_parity
LAUNCHED = [n for n, s in gd.ALL_CASES if "refused" not in s]
_STOP = []                 # why no further child is started


def bound(spec, kind):
    geo = gd._geometry()
    return {"out": BF16_TOL, "out2": BF16_TOL, "out_f32": F32_TOL, "colsum_to_stored": COLSUM_STORED_TOL, "colsum_to_reference": COLSUM_REFERENCE_TOL,
            "gn_sums": geo.STAT_SUM_TOL, "gn_finalize": geo.PHASE_FIN_TOL if "up" in spec else geo.STAT_FIN_TOL}[kind]


def misses(name, spec, errs, kinds=None):
    """the bounds a case's figures miss, as text; every kind the case writes must have a figure"""
    kinds = gd.written(spec) if kinds is None else kinds
    bad = [f"{name}: figures {sorted(errs)} for outputs {kinds}"] if set(errs) - {"nan", "gn_assert"} != set(kinds) else []
    bad += [f"{name}: {errs['nan']} non-finite values where one is specified"] if errs["nan"] else []
    bad += [f"{name}: check_statistics: {errs['gn_assert']}"] if "gn_assert" in errs else []
    return bad + [f"{name}: {k} {errs[k]:.3e} >= {bound(spec, k):.0e}" for k in kinds if k in errs and not errs[k] < bound(spec, k)]


def run_child(setting):
    """(the JSON object the child printed, its wall time); marks _STOP when the card may have faulted"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("PXA_GEMM_")}
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, env={**env, **ALL_SETTINGS[setting]}, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _STOP.append(f"the child of setting {setting} ran into its time limit of {CHILD_TIMEOUT} s")
        pytest.fail(_STOP[-1])
    wall = time.perf_counter() - t0
    lines = r.stdout.splitlines()
    got = json.loads(lines[-1]) if lines and lines[-1].startswith("{") else {}
    if r.returncode < 0 or r.returncode in (134, 139):
        _STOP.append(f"the child of setting {setting} ended with status {r.returncode}")
    elif "hip_error" in got:
        _STOP.append(f"the child of setting {setting} reported a HIP error: {got['hip_error']}")
    assert r.returncode == 0 and "hip_error" not in got, (_STOP[-1:] or [r.returncode], r.stdout[-2000:], r.stderr[-3000:])
    return got, wall


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(ALL_SETTINGS))
def test_call_list_values(setting):
    if _STOP:
        pytest.skip(_STOP[0] + ": nothing more is started on this card")
    got, wall = run_child(setting)
    cases = got["cases"]
    assert list(cases) == LAUNCHED, set(LAUNCHED) ^ set(cases)                                   # a silently skipped case fails
    want = tgp.expected(setting if setting in tgp.CHANGED else "default")                        # nt4 and the three of this file: the default plans
    specs, bad, worst = dict(gd.ALL_CASES), [], {}
    print(f"\n[{setting}] child wall time {wall:.1f} s")
    for name, c in cases.items():
        if want[name][0] == "refused":
            assert c["plan"] is None and "pxa_gemm_plan failed (rc=-1): pxa_gemm: " + want[name][1] in c["refused"], (setting, name, c)
            continue
        assert c["plan"] is not None and tgp.plan_fields(c["plan"]) == want[name], (setting, name, c["plan"], want[name])
        errs = c["errors"]
        print(f"  {name}: {c['plan'].split()[0]} " + " ".join(f"{k} {v:.2e}" if isinstance(v, float) else f"{k} {v}" for k, v in errs.items()))
        bad += misses(name, specs[name], errs)
        for k in gd.written(specs[name]):
            if k in errs and not errs[k] <= worst.get((k, bound(specs[name], k)), 0.0):          # (a NaN is the worst)
                worst[(k, bound(specs[name], k))] = errs[k]
    for (k, b), v in worst.items():
        record_parity(f"gemm call list [{setting}] worst {k}", v, b)
    record_parity(f"gemm call list [{setting}] child wall time (s)", wall, CHILD_TIMEOUT)
    assert not bad, "\n".join([setting] + bad)


def test_the_checker_has_teeth():
    """gd.errors and the bounds above on the CPU: the fp64 expectation rounded once to the operand type passes (token GEMM with bias, two outputs, column sums,
    accumulate; the convolutions against a second statement of them - the segmented A operand gathered, times B, row by row, scattered for the phase case - which also
    pins reference()'s conv2d geometry), and each of five defects fails at the figure it should."""
    from pixart_sigma_amd import ops
    specs = dict(gd.ALL_CASES)

    def call(name):
        spec = specs[name]
        a, b, kw = gd.make_call(spec, "cpu", seed=LAUNCHED.index(name))
        gd.prepare_outputs(spec, a, kw, seed=LAUNCHED.index(name))
        return spec, a, b, kw, gd.reference(spec, a, b, kw)

    def store(kw, ref, edit=lambda r: r):
        r = edit({k: v.clone() for k, v in ref.items()})
        for k in ("out", "out2", "out_f32"):
            if k in r:
                kw[k].copy_(r[k].to(kw[k].dtype))
        if "colsum" in kw:
            kw["colsum"].zero_()
            kw["colsum"][3] = r["colsum"].float() if "colsum_given" in r else kw["out"].double().sum(0).float()

    def verdict(name, spec, kw, ref):
        return misses(name, spec, gd.errors(spec, kw, ref, statistics=False), [k for k in gd.written(spec) if not k.startswith("gn_")])

    # clean results pass
    for name in ("nt_plain_1152", "nt_gelu_save_grad", "nt_gelu_out2", "nn_mul_aux_colsum_1152", "nt_small_colsum", "tn_accumulate_one_slice", "tn_bias", "nt_small_f32",
                 "t5_residual_1024", "t5_mul_aux"):
        spec, a, b, kw, ref = call(name)
        store(kw, ref)
        assert verdict(name, spec, kw, ref) == [], name
    # the convolutions: A's segments gathered as pxa_gemm_args.k_seg describes them, times B, for every row
    for name in ("conv_res_128", "conv_384", "conv_f32", "conv_phase_128"):
        spec, a, b, kw, ref = call(name)
        C, K = spec["conv"][3], b.shape[1]                                                      # (C = 64: the tap-interleaved K order is the plain one)
        patches = a.as_strided((spec["M"], K // kw["k_seg"], kw["k_seg"]), (C, kw["a_seg_stride"], 1)).reshape(spec["M"], K)
        rows = patches.double() @ b.double().t() + kw["bias"].double() + (kw["aux"].double() if "aux" in kw else 0.0)
        low, high = gd._conv_rows(spec, "cpu")
        target = kw["out_f32" if spec.get("f32") else "out"]
        if "up" in spec:
            target[high.flatten()] = rows[low.flatten()].to(target.dtype)
        else:
            target.copy_(rows.to(target.dtype))
        assert verdict(name, spec, kw, ref) == [], name
        target[high[1, 2, 3]] = float("nan")                                                    # one interior pixel never written
        assert any("non-finite" in m for m in verdict(name, spec, kw, ref)), name

    def fails(name, edit, kind):
        spec, a, b, kw, ref = call(name)
        store(kw, ref, edit)
        got = verdict(name, spec, kw, ref)
        assert got and all(f": {kind} " in m for m in got), (name, kind, got)

    def scaled_block(r):
        r["out"][320:384, 448:512] *= 1.01
        return r
    fails("nt_plain_1152", scaled_block, "out")                         # one 64 x 64 block scaled by 1.01 (global rel-L2: 1.01 / sqrt(288) = 6e-4, under the bound)
    spec, a, b, kw, ref = call("nt_plain_1152")

    def no_bias_in_the_remainder_column(r, bias=kw["bias"].double()):
        r["out"][:, 1024:] -= bias[1024:]
        return r
    fails("nt_plain_1152", no_bias_in_the_remainder_column, "out")

    def swapped_row(r):
        r["out"][700], r["out2"][700] = r["out2"][700].clone(), r["out"][700].clone()
        return r
    for name in ("nt_gelu_out2", "nt_gelu_save_grad"):
        spec, a, b, kw, ref = call(name)
        store(kw, ref, swapped_row)
        got = verdict(name, spec, kw, ref)
        assert any(": out " in m for m in got) and any(": out2 " in m for m in got), got

    def unrounded_sums_one_column_off(r):
        r["colsum"][77] *= 1.001
        r["colsum_given"] = True
        return r
    fails("nn_mul_aux_colsum_1152", unrounded_sums_one_column_off, "colsum_to_stored")
    fails("nn_mul_aux_colsum_1152", lambda r: dict(r, colsum_given=True), "colsum_to_stored")   # the sums of the unrounded values alone
    spec, a, b, kw, ref = call("nt_small_colsum")                                               # the sums of the stored values, the largest of a block 1e-3 off
    store(kw, ref)
    col = 64 + int(kw["colsum"][3, 64:128].abs().argmax())
    kw["colsum"][3, col] *= 1.001
    got = verdict("nt_small_colsum", spec, kw, ref)
    assert got and all(": colsum_to_stored " in m for m in got), got

    def overwritten(name):
        def edit(r):
            spec, a, b, kw, _ = call(name)
            r["out_f32"] -= kw["out_f32"].double()
            return r
        return edit
    fails("tn_accumulate_one_slice", overwritten("tn_accumulate_one_slice"), "out_f32")
    fails("t5_residual_1024", overwritten("t5_residual_1024"), "out_f32")                       # the encoder's residual stream, stored where it is added into

    def last_wave_row_adds_twice(r):
        spec, a, b, kw, _ = call("t5_residual_1024")
        r["out_f32"][1088:] += r["out_f32"][1088:] - kw["out_f32"].double()[1088:]               # the 32 rows of the ragged tile's last wave tile
        return r
    fails("t5_residual_1024", last_wave_row_adds_twice, "out_f32")

    def aux_of_the_row_before(r):
        spec, a, b, kw, _ = call("t5_mul_aux")
        r["out"][1024:] = (a.double() @ b.double().t())[1024:] * kw["aux"].double()[1023:-1]    # the ragged last tile reads its aux rows one row off
        return r
    fails("t5_mul_aux", aux_of_the_row_before, "out")


if __name__ == "__main__":                                             # the child of test_call_list_values: the list once, in this process's environment
    from pixart_sigma_amd import ops
    from pixart_sigma_amd.lib import PixartHipError
    cases = {}
    for i, (name, spec) in enumerate(gd.ALL_CASES):
        if "refused" in spec:
            continue
        try:
            a, b, kw = gd.make_call(spec, "cuda:0", seed=i)
            gd.prepare_outputs(spec, a, kw, seed=i)
            try:
                line = ops.gemm_plan(a, b, **kw)
            except PixartHipError as e:                                # a setting refuses the call: nothing is launched
                cases[name] = {"plan": None, "refused": str(e)}
                continue
            ref = gd.reference(spec, a, b, kw)
            ops.gemm(a, b, **kw)
            torch.cuda.synchronize()
            cases[name] = {"plan": line, "errors": gd.errors(spec, kw, ref)}
        except (PixartHipError, RuntimeError) as e:                    # the first HIP error ends the child: no further launch, no teardown on the device
            print(json.dumps({"cases": cases, "hip_error": f"{name}: {e}"}), flush=True)
            os._exit(3)
    print(json.dumps({"cases": cases}), flush=True)
