"""The host-side dispatch of pxa_attn_fwd / pxa_attn_bwd, pinned without a GPU: ops.attention_plan (pxa_attn_plan: fill, read_knobs and the choose_* functions
of csrc/attn.hip, shared with the two entry points, and the grid helpers their launchers use) for shapes that never reach the large-LDS opt-in query - more
than 320 keys per sample or fewer than 512 queries, where keys_fit_lds answers before the runtime is asked.  The keys-resident lines (fwd=kvres, dq=kvres,
pre=none) need the device's answer and are asserted in tests/test_attn_forms_gpu.py, on the very calls that run.

The expected lines rest on reading the parent commit's dispatch (the end of csrc/attn.hip: choose_fwd, choose_dq_kvres, choose_prepass, choose_dq, choose_dkv,
launch_* for nx), not on a kernel trace; tests/test_attn_forms_gpu.py ties each line it asserts to the values the launched kernels write.

  forward    two-sub-tile kernel from 256 queries on, the one-sub-tile kernel below; the one-wave-per-SIMD kernel for dense keys in whole 64-key tiles - by
             default only in the fp16 build (FWD4_FOLD) from 8 key tiles on, PXA_ATTN_FWD4=1 wherever it applies, =0 never
  pre-pass   rows for token-contiguous O with H <= 16, else strided; none under PXA_ATTN_BWD_NO_PREPASS
  dQ         dq4 for dense keys in whole tiles, Nk >= 128, Nq >= 256, else dq2; PXA_ATTN_DQ = 0 the round-2 kernel, 1 dq2, 4 dq4 where it applies
  dK/dV      dkv4 for dense keys in whole tiles, Nk >= 256, whole 64-query tiles, Nq >= 128, else dkv2; PXA_ATTN_DKV = 0 round-2, 1 dkv2_plain, 2 dkv2,
             3 dkv3, 4 / 5 dkv4 / dkv5 where they apply, else dkv2; no bwd_stats workspace or no dk: the round-2 kernel / skip
PXA_ATTN_FWD1 and PXA_ATTN_NO_KVRES are read once per process: a child process each (as tests/test_gemm_plan.py does for its knobs)."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

KNOBS = ("PXA_ATTN_FWD1", "PXA_ATTN_NO_KVRES", "PXA_ATTN_FWD4", "PXA_ATTN_DKV", "PXA_ATTN_DQ", "PXA_ATTN_BWD_NO_PREPASS")
FWD_KERNEL = {"fwd4": "attn_fwd4_kernel", "fwd2": "attn_fwd2_kernel", "fwd1": "attn_fwd_kernel"}
PRE_KERNEL = {"none": "-", "rows": "attn_delta_rows_kernel", "strided": "attn_delta_kernel"}
DQ_KERNEL = {"dq4": "attn_bwd_dq4_kernel<false>", "dq2": "attn_bwd_dq2_kernel", "r2": "attn_bwd_dq_kernel", "skip": "-"}
DKV_KERNEL = {"dkv4": "attn_bwd_dkv4_kernel<false>", "dkv2": "attn_bwd_dkv2_kernel<1>", "dkv2_plain": "attn_bwd_dkv2_kernel<0>", "dkv5": "attn_bwd_dkv5_kernel<false>",
              "dkv3": "attn_bwd_dkv3_kernel<2>", "r2": "attn_bwd_dkv_kernel", "skip": "-"}


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _f16():
    from pixart_sigma_amd import lib
    return lib.OPERAND == "f16"


def plan(B, H, Nq, Nk, backward, varlen=False, max_kv_len=0, dq=True, dkv=True, o_ts=None, **kw):
    """ops.attention_plan of a dense (or, varlen, packed) call on CPU tensors that are never dereferenced, as a dict of its fields"""
    from pixart_sigma_amd import ops
    D = H * 72
    t, f, i = torch.empty(16, dtype=ops.BF16), torch.empty(16), torch.empty(4, dtype=torch.int32)
    sq, sk = (Nq * D, D, 72), (Nk * D, D, 72)
    so = (Nq * o_ts, o_ts, 72) if o_ts else sq
    if varlen:
        kw.update(kv_start=i, kv_len=i, max_kv_len=max_kv_len)
    if not backward:
        line = ops.attention_plan(t, t, t, t, f, B, H, Nq, Nk, (sq, sk, sk, so), **kw)
        keys = ["fwd", "fwd_kernel", "fwd_nx"]
    else:
        line = ops.attention_plan(t, t, t, t, t, f, f, t if dq else None, t if dkv else None, t if dkv else None, B, H, Nq, Nk, (sq, sk, sk, so), (sq, sk, sk), **kw)
        keys = ["pre", "dq", "dkv", "pre_kernel", "dq_kernel", "dq_nx", "dkv_kernel", "dkv_nx"]
    fields = dict(w.split("=") for w in line.split())
    assert list(fields) == keys, line
    return fields


def fwd(B, H, Nq, Nk, **kw):
    p = plan(B, H, Nq, Nk, False, **kw)
    assert p["fwd_kernel"] == FWD_KERNEL[p["fwd"]], p
    return p["fwd"], int(p["fwd_nx"])


def bwd(B, H, Nq, Nk, **kw):
    p = plan(B, H, Nq, Nk, True, **kw)
    pre = "<true>" if kw.get("q_prescaled") else "<false>"
    assert p["pre_kernel"] == PRE_KERNEL[p["pre"]] and p["dq_kernel"] == DQ_KERNEL[p["dq"]].replace("<false>", pre), p
    assert p["dkv_kernel"] == DKV_KERNEL[p["dkv"]].replace("<false>", pre), p
    return p["pre"], p["dq"], int(p["dq_nx"]), p["dkv"], int(p["dkv_nx"])


# (Nq, Nk) -> (kernel, nx); "f4" = fwd4 in the fp16 build (its default from 8 whole key tiles on), fwd2 in the bf16 build
FWD_DEFAULT = [
    ((255, 256), ("fwd1", 2)), ((256, 256), ("fwd2", 1)), ((256, 64), ("fwd2", 1)), ((256, 128), ("fwd2", 1)), ((256, 192), ("fwd2", 1)),
    ((256, 448), ("fwd2", 1)), ((256, 512), ("f4", 1)), ((256, 520), ("fwd2", 1)), ((300, 512), ("f4", 2)), ((200, 512), ("fwd1", 2)),
    ((1024, 1024), ("f4", 4)), ((600, 4096), ("f4", 3)), ((64, 1024), ("fwd1", 1)), ((130, 77), ("fwd1", 2)),
]


def _f4(want, on):
    return (("fwd4" if on else "fwd2") if want[0] == "f4" else want[0], want[1])


def test_forward_default_and_fwd4_knob(monkeypatch):
    for (Nq, Nk), want in FWD_DEFAULT:
        assert fwd(2, 3, Nq, Nk) == _f4(want, _f16()), (Nq, Nk)
    assert fwd(2, 3, 300, 512, varlen=True) == ("fwd2", 2)                        # kv_start given: never the one-wave kernel (max_k = Nk = 512 > 320)
    assert fwd(2, 3, 1024, 512, varlen=True, max_kv_len=400) == ("fwd2", 4)
    monkeypatch.setenv("PXA_ATTN_FWD4", "0")
    for (Nq, Nk), want in FWD_DEFAULT:
        assert fwd(2, 3, Nq, Nk) == _f4(want, False), (Nq, Nk)
    monkeypatch.setenv("PXA_ATTN_FWD4", "1")                                      # wherever it applies: >= 256 queries, dense keys in whole tiles
    for (Nq, Nk), want in FWD_DEFAULT:
        applies = Nq >= 256 and Nk % 64 == 0
        assert fwd(2, 3, Nq, Nk) == (("fwd4", want[1]) if applies else _f4(want, False)), (Nq, Nk)
    assert fwd(2, 3, 300, 512, varlen=True) == ("fwd2", 2)


# (Nq, Nk) -> (dq, dq_nx, dkv, dkv_nx) in the default environment, dense keys, bwd_stats given
BWD_DEFAULT = [
    ((255, 256), ("dq2", 2, "dkv2", 2)), ((256, 256), ("dq4", 1, "dkv4", 1)), ((256, 64), ("dq2", 2, "dkv2", 1)), ((256, 128), ("dq4", 1, "dkv2", 1)),
    ((256, 192), ("dq4", 1, "dkv2", 2)), ((256, 320), ("dq4", 1, "dkv4", 2)), ((256, 512), ("dq4", 1, "dkv4", 2)), ((256, 520), ("dq2", 2, "dkv2", 5)),
    ((320, 512), ("dq4", 2, "dkv4", 2)), ((300, 512), ("dq4", 2, "dkv2", 4)), ((128, 256), ("dq2", 1, "dkv4", 1)), ((64, 256), ("dq2", 1, "dkv2", 2)),
    ((130, 77), ("dq2", 2, "dkv2", 1)), ((1024, 1024), ("dq4", 4, "dkv4", 4)),
]


def test_backward_default():
    for (Nq, Nk), want in BWD_DEFAULT:
        assert bwd(2, 3, Nq, Nk) == ("rows", *want), (Nq, Nk)
        assert bwd(2, 3, Nq, Nk, q_prescaled=True) == ("rows", *want), (Nq, Nk)     # the same kernels, their <true> instances (checked in bwd())
    # kv_start given: the two-wave kernels, the dK/dV grid from max_kv_len
    assert bwd(2, 3, 300, 512, varlen=True, max_kv_len=400) == ("rows", "dq2", 3, "dkv2", 4)
    assert bwd(2, 3, 256, 512, varlen=True) == ("rows", "dq2", 2, "dkv2", 4)
    # a NULL gradient skips its kernel; ops.attention_bwd passes no bwd_stats when dk is None
    for (Nq, Nk), want in BWD_DEFAULT:
        assert bwd(2, 3, Nq, Nk, dq=False) == ("rows", "skip", 0, *want[2:]), (Nq, Nk)
        assert bwd(2, 3, Nq, Nk, dkv=False) == ("rows", *want[:2], "skip", 0), (Nq, Nk)


def test_prepass_form():
    assert bwd(1, 16, 130, 77)[0] == "rows" and bwd(1, 17, 130, 77)[0] == "strided"          # attn_delta_rows_kernel: a thread per (token, head) of 16
    assert bwd(1, 2, 130, 77, o_ts=2 * 2 * 72)[0] == "strided"                                # O rows that are not token-contiguous
    assert bwd(1, 2, 130, 77, o_ts=2 * 72)[0] == "rows"


@pytest.mark.parametrize("mode", ["0", "1", "4"])
def test_dq_knob(monkeypatch, mode):
    monkeypatch.setenv("PXA_ATTN_DQ", mode)
    for (Nq, Nk), want in BWD_DEFAULT:
        dq = {"0": ("r2", (Nq + 127) // 128), "1": ("dq2", (Nq + 127) // 128), "4": want[:2]}[mode]
        assert bwd(2, 3, Nq, Nk) == ("rows", *dq, *want[2:]), (Nq, Nk)
    assert bwd(2, 3, 300, 512, varlen=True, max_kv_len=400)[1] == ("r2" if mode == "0" else "dq2")


@pytest.mark.parametrize("mode", ["0", "1", "2", "3", "4", "5"])
def test_dkv_knob(monkeypatch, mode):
    monkeypatch.setenv("PXA_ATTN_DKV", mode)
    for (Nq, Nk), want in BWD_DEFAULT:
        n128, n256 = (Nk + 127) // 128, (Nk + 255) // 256
        one_wave = want[2] == "dkv4"                                                           # where the one-wave kernels apply
        dkv = {"0": ("r2", n128), "1": ("dkv2_plain", n128), "2": ("dkv2", n128), "3": ("dkv3", n256),
               "4": ("dkv4", n256) if one_wave else ("dkv2", n128), "5": ("dkv5", n256) if one_wave else ("dkv2", n128)}[mode]
        assert bwd(2, 3, Nq, Nk) == ("rows", *want[:2], *dkv), (Nq, Nk)
        assert bwd(2, 3, Nq, Nk, dkv=False)[3:] == ("skip", 0)
    assert bwd(2, 3, 256, 512, varlen=True)[3] == {"0": "r2", "1": "dkv2_plain", "3": "dkv3"}.get(mode, "dkv2")


def test_no_prepass_knob(monkeypatch):
    monkeypatch.setenv("PXA_ATTN_BWD_NO_PREPASS", "1")
    assert bwd(2, 3, 256, 256) == ("none", "dq4", 1, "dkv4", 1)


def _raw(**f):
    """a pxa_attn_args block by hand (addresses that are never used): what ops.attention_bwd cannot express, such as dk without a bwd_stats workspace"""
    from pixart_sigma_amd import lib
    a = lib.AttnArgs()
    B, H, Nq, Nk = f.pop("B", 2), f.pop("H", 3), f.pop("Nq", 256), f.pop("Nk", 256)
    D = H * 72
    for n in ("q", "k", "v", "o", "d_o", "dq", "dk", "dv", "lse", "delta", "bwd_stats"):
        setattr(a, n, 64)
    a.B, a.H, a.Nq, a.Nk, a.head_dim, a.scale = B, H, Nq, Nk, 72, 72 ** -0.5
    for n, rows in (("q", Nq), ("k", Nk), ("v", Nk), ("o", Nq), ("dq", Nq), ("dk", Nk), ("dv", Nk)):
        setattr(a, n + "_bs", rows * D), setattr(a, n + "_ts", D), setattr(a, n + "_hs", 72)
    for n, v in f.items():
        setattr(a, n, v)
    return a


def _raw_plan(a, backward, size=256):
    import ctypes as C
    from pixart_sigma_amd import lib
    L, buf = lib.load(), C.create_string_buffer(256)
    rc = L.pxa_attn_plan(C.byref(a), backward, buf, size)
    return rc, (buf.value.decode() if rc == 0 else L.pxa_last_error().decode())


def test_no_stats_workspace_runs_the_round_2_dkv_kernel():
    rc, line = _raw_plan(_raw(), 1)
    assert rc == 0 and line.startswith("pre=rows dq=dq4 dkv=dkv4 "), line
    rc, line = _raw_plan(_raw(bwd_stats=None), 1)
    assert rc == 0 and line == "pre=rows dq=dq4 dkv=r2 pre_kernel=attn_delta_rows_kernel dq_kernel=attn_bwd_dq4_kernel<false> dq_nx=1 dkv_kernel=attn_bwd_dkv_kernel dkv_nx=2", line
    rc, line = _raw_plan(_raw(o=72), 1)                     # an O address that is no multiple of 16 bytes: the strided pre-pass
    assert rc == 0 and line.startswith("pre=strided "), line
    rc, line = _raw_plan(_raw(), 0)
    assert rc == 0 and line == "fwd=fwd2 fwd_kernel=attn_fwd2_kernel fwd_nx=1", line


def test_refused_calls_and_short_buffer():
    """the same return code and pxa_last_error() as pxa_attn_fwd / pxa_attn_bwd; a short text buffer is an error, not a truncation"""
    for backward, a, msg in [
        (0, _raw(head_dim=64), "attn: head_dim 64 unsupported (PixArt XL/2 uses 72)"),
        (1, _raw(B=0), "attn: bad shape"),
        (0, _raw(kv_start=64), "attn: kv_start/kv_len must both be given"),
        (0, _raw(k_ts=3 * 72 + 4), "attn: strides must be multiples of 8 elements (16-byte rows)"),
        (0, _raw(o=None), "pxa_attn_fwd: null tensor"),
        (1, _raw(d_o=None), "pxa_attn_bwd: null tensor"),
        (1, _raw(delta=None), "pxa_attn_bwd: null tensor"),
        (1, _raw(dq=None, dk=None, dv=None), "pxa_attn_bwd: need dq and/or both of dk, dv (a NULL gradient skips the kernel that produces it)"),
        (1, _raw(dv=None), "pxa_attn_bwd: need dq and/or both of dk, dv (a NULL gradient skips the kernel that produces it)"),
        (1, _raw(dk_ts=3 * 72 + 2), "pxa_attn_bwd: gradient strides must be multiples of 4 elements"),
        (1, _raw(B=1 << 20, H=1 << 10, Nq=256, Nk=512), "pxa_attn_bwd: grid too large"),
        (0, _raw(B=1 << 20, H=1 << 10, Nq=512, Nk=512), "pxa_attn_fwd: grid too large"),
    ]:
        assert _raw_plan(a, backward) == (-1, msg), msg
    import ctypes as C
    from pixart_sigma_amd import lib
    assert lib.load().pxa_attn_plan(None, 0, C.create_string_buffer(8), 8) == -1 and lib.load().pxa_last_error() == b"attn: null args"
    rc, msg = _raw_plan(_raw(), 1, size=32)
    assert rc == -1 and "too small" in msg
    rc, msg = _raw_plan(_raw(), 0, size=0)
    assert rc == -1 and msg == "pxa_attn_plan: no text buffer"
    from pixart_sigma_amd import ops
    t, f = torch.empty(16, dtype=ops.BF16), torch.empty(16)
    with pytest.raises(lib.PixartHipError, match="pxa_attn_plan failed .rc=-1.: attn: head_dim 64 unsupported"):
        ops.attention_plan(t, t, t, t, f, 1, 2, 256, 256, ((256 * 128, 128, 64),) * 4, head_dim=64)


def _child_rows():
    """[forward, backward] plans of a few shapes, two of them with keys that would stay resident (1024 queries, 77 / 320 keys): the two once-per-process
    knobs answer before the device is asked"""
    return [[list(fwd(2, 3, Nq, Nk)), list(bwd(2, 3, Nq, Nk))] for Nq, Nk in ((1024, 77), (1024, 320), (256, 256), (255, 256), (1024, 1024))]


def _in_a_child(env_add):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, env={**env, **env_add})
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.splitlines()[-1])


def test_no_kvres_in_a_child():
    """PXA_ATTN_NO_KVRES: text-sized keys on the streaming kernels - no keys-resident forward, no dQ kernel that replaces the pre-pass"""
    f4 = "fwd4" if _f16() else "fwd2"
    assert _in_a_child({"PXA_ATTN_NO_KVRES": "1"}) == [
        [["fwd2", 4], ["rows", "dq2", 8, "dkv2", 1]], [["fwd2", 4], ["rows", "dq4", 4, "dkv4", 2]], [["fwd2", 1], ["rows", "dq4", 1, "dkv4", 1]],
        [["fwd1", 2], ["rows", "dq2", 2, "dkv2", 2]], [[f4, 4], ["rows", "dq4", 4, "dkv4", 4]]]


def test_fwd1_in_a_child():
    """PXA_ATTN_FWD1: the one-sub-tile forward everywhere, 128 queries per workgroup; with PXA_ATTN_NO_KVRES beside it the backward stays on the streaming kernels"""
    got = _in_a_child({"PXA_ATTN_FWD1": "1", "PXA_ATTN_NO_KVRES": "1"})
    assert [g[0] for g in got] == [["fwd1", 8], ["fwd1", 8], ["fwd1", 2], ["fwd1", 2], ["fwd1", 8]]
    assert got[2][1] == ["rows", "dq4", 1, "dkv4", 1]


if __name__ == "__main__":                                             # the children of the tests above
    print(json.dumps(_child_rows()))
