"""T5Encoder with FP8 (e4m3fn) weights on the GPU, on both GEMM paths ("stream" = pxa_gemm_w8, "dequant" = pxa_fp8_dequant_rows + pxa_gemm).

Parity.  The weights go through the quantiser kernel; the reference is t5_refs.encoder64 in fp64 ON THE DEQUANTISED WEIGHTS (scale * q), so the bound isolates the
kernels from the quantisation: rel-L2 of last_hidden_state over all rows <= 1.1 x the stored yardstick of the fixture and build (transformers' own 16-bit loss,
tests/golden/t5_ref_noise.json, t5_wide.json), for t5_wide over rows 1024 .. 1199 as well.  tests/test_t5_fp8_host.py holds the condition under which that
yardstick is usable on dequantised weights (the rounding-point emulation stays inside the same margin).  t5_wide has 1200 rows, below pxa_gemm_w8_max_m() =
2048: its stream case runs the whole batch, as the dequant case does.
The effect of the quantisation itself - encoder64 on dequantised against encoder64 on the original weights - is recorded (record_parity), not bounded: the
fixtures are random weights, and no trained T5 checkpoint is available to measure it on.

Measured on an MI355X, error / yardstick (bound 1.1), stream path (dequant equal to three digits in bf16): bf16 build t5_tiny 0.507, t5_l300 0.913, t5_wide 0.618
(tail rows 0.347); fp16 build 0.667 / 0.712 / 0.863 (tail 0.874; dequant 0.672 / 0.713 / 0.846, tail 0.795).  Quantisation effect: 0.133 / 0.145 / 0.139.

Equalities, bit for bit: auto = the path it names; from_pretrained(16-bit directory, weight_dtype="fp8_e4m3") = quantize_fp8() on the loaded 16-bit encoder =
from_pretrained(directory written by save_pretrained); a batch = each sample alone; ids at padded positions change no valid row.  A 16-bit encoder built after
all this gives what it gave (the stored goldens).  tools/quantize_t5.py -> tools/extract_t5_features.py in child processes equal the in-process FP8 forward."""
import json
import os
import subprocess
import sys
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

import t5_fixtures  # noqa: E402
import t5_fp8_refs as R  # noqa: E402
import t5_refs  # noqa: E402
from conftest import ROOT, record_parity, rel_l2  # noqa: E402
from test_t5_model_gpu import MARGIN, write_model_dir  # noqa: E402

PATHS = ("stream", "dequant")


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pixart_sigma_amd import lib as l_
    return l_


def fp8_encoder(cfg, sd):
    from pixart_sigma_amd.t5 import T5Encoder
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # the fp16-build notice
        m = T5Encoder(cfg, weight_dtype="fp8_e4m3").cuda()
    m.load_state_dict(sd)                                  # 16-bit tensors: through pxa_fp8_quant_rows
    return m


def recipe(name):
    """(cfg, state dict, ids, mask, yardstick of this build: dict rows -> figure, rows: dict name -> slice)"""
    from pixart_sigma_amd import lib as l_
    if name == "t5_wide":
        W = t5_refs.WIDE
        with open(os.path.join(t5_fixtures.GOLDEN_DIR, "t5_wide.json")) as f:
            rec = json.load(f)
        ids, mask = t5_refs.inputs(W["cfg"], W["B"], W["L"], W["lens"], W["seed"])
        return t5_refs.full_config(W["cfg"]), t5_refs.state_dict(W["cfg"], W["seed"]), ids, mask, rec["yardstick"][l_.OPERAND], \
            {"all_rows": slice(None), "tail_rows": t5_refs.WIDE_TAIL}
    fx = t5_fixtures.load(name)
    return fx["config"], fx["state_dict"], fx["input_ids"], fx["attention_mask"], {"all_rows": t5_fixtures.ref_noise()[name][l_.OPERAND]}, {"all_rows": slice(None)}


_REFS = {}


def reference(name):
    """encoder64 on the dequantised weights (and the quantisation effect against the original ones), once per fixture"""
    if name not in _REFS:
        from pixart_sigma_amd import lib as l_
        cfg, sd, ids, mask, _, _ = recipe(name)
        dq = R.dequant_state_dict(sd, through=l_.OPERAND_DTYPE)
        want = t5_refs.encoder64(cfg, dq, ids, mask, device="cuda")[-1]
        orig = t5_refs.encoder64(cfg, sd, ids, mask, device="cuda")[-1]
        record_parity(f"{name} effect of FP8 quantisation: encoder64 on dequantised vs original weights (random weights; not bounded)", rel_l2(want, orig))
        _REFS[name] = want
    return _REFS[name]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["t5_tiny", "t5_l300", "t5_wide"])
def test_parity_against_encoder64_on_dequantised_weights(lib, name, path):
    from pixart_sigma_amd import ops
    cfg, sd, ids, mask, yard, rows = recipe(name)
    m = fp8_encoder(cfg, sd).set_fp8_gemm(path)
    assert ids.numel() <= ops.gemm_w8_max_m()                # the stream case runs every row of the fixture
    k = "encoder.block.0.layer.1.DenseReluDense.wi_1.weight"
    q, s = R.quant_rows(sd[k].to(lib.OPERAND_DTYPE))
    assert torch.equal(m.b0_wi1.cpu().view(torch.uint8), q.view(torch.uint8)) and torch.equal(m.b0_wi1_scale.cpu(), s)      # the weights the reference dequantises
    with torch.no_grad():
        y = m(ids, mask)
    assert m.fp8_gemm_path(ids.numel()) == path and (m._scratch is not None) == (path == "dequant")
    want = reference(name)
    D = y.shape[-1]
    assert y.dtype == torch.float32 and tuple(y.shape) == tuple(want.shape) and torch.isfinite(y).all()
    for rname, sl in rows.items():
        e = rel_l2(y.reshape(-1, D)[sl], want.reshape(-1, D)[sl])
        record_parity(f"{name} FP8 {path} last_hidden_state vs encoder64 on dequantised weights, {rname} (bound = {MARGIN} x yardstick)", e, MARGIN * yard[rname])
        print(f"\n{name} [{lib.OPERAND}] {path} {rname}: {e:.3e} = {e / yard[rname]:.3f} x yardstick {yard[rname]:.3e} (bound {MARGIN})", end="")
        assert e <= MARGIN * yard[rname], (name, path, rname, e, yard[rname])


@pytest.fixture(scope="module")
def tiny(lib):
    fx = t5_fixtures.load("t5_tiny")
    m = fp8_encoder(fx["config"], fx["state_dict"])
    out = {}
    for path in PATHS:
        with torch.no_grad():
            out[path] = m.set_fp8_gemm(path)(fx["input_ids"], fx["attention_mask"])
    return fx, m, out


def test_auto_is_the_path_it_names(tiny, monkeypatch):
    from pixart_sigma_amd.t5 import encoder
    fx, m, out = tiny
    rows = fx["input_ids"].numel()
    m.set_fp8_gemm("auto")
    monkeypatch.setattr(encoder, "STREAM_MAX_M", rows)
    assert m.fp8_gemm_path(rows) == "stream"
    with torch.no_grad():
        assert torch.equal(m(fx["input_ids"], fx["attention_mask"]), out["stream"])
    monkeypatch.setattr(encoder, "STREAM_MAX_M", rows - 1)
    assert m.fp8_gemm_path(rows) == "dequant"
    with torch.no_grad():
        assert torch.equal(m(fx["input_ids"], fx["attention_mask"]), out["dequant"])


def test_three_ways_to_an_fp8_encoder_give_the_same_bits(tiny, tmp_path):
    from pixart_sigma_amd.t5 import T5Encoder
    fx, m, out = tiny
    write_model_dir(str(tmp_path / "t5"), fx)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = T5Encoder.from_pretrained(str(tmp_path / "t5"), device="cuda", weight_dtype="fp8_e4m3")
        b = T5Encoder.from_pretrained(str(tmp_path / "t5"), device="cuda").quantize_fp8()
        a.save_pretrained(str(tmp_path / "fp8"))
        c = T5Encoder.from_pretrained(str(tmp_path / "fp8"), device="cuda")
    assert a.weight_dtype == b.weight_dtype == c.weight_dtype == "fp8_e4m3"
    for x in (a, b, c):
        assert x.b0_wqkv.dtype == torch.float8_e4m3fn and x.b0_wqkv.is_cuda
        assert torch.equal(x.b1_wff.view(torch.uint8), m.b1_wff.view(torch.uint8)) and torch.equal(x.b1_wff_scale, m.b1_wff_scale)
        for path in PATHS:
            with torch.no_grad():
                assert torch.equal(x.set_fp8_gemm(path)(fx["input_ids"], fx["attention_mask"]), out[path]), path
    held16 = sum(bf.numel() * bf.element_size() for n, bf in T5Encoder(fx["config"]).named_buffers() if n[0] == "b" and bf.dim() == 2)
    held8 = sum(bf.numel() * bf.element_size() for n, bf in a.named_buffers() if n[0] == "b" and bf.dim() == 2)
    assert held8 * 2 == held16


@pytest.mark.parametrize("path", PATHS)
def test_batch_equals_each_sample_alone(tiny, path):
    fx, m, out = tiny
    m.set_fp8_gemm(path)
    for b in range(fx["input_ids"].shape[0]):
        with torch.no_grad():
            one = m(fx["input_ids"][b:b + 1], fx["attention_mask"][b:b + 1])
        assert torch.equal(one[0], out[path][b]), (path, b)


@pytest.mark.parametrize("path", PATHS)
def test_ids_at_padded_positions_change_no_valid_row(tiny, path):
    fx, m, out = tiny
    ids, mask = fx["input_ids"].clone(), fx["attention_mask"]
    other = torch.randint(2, fx["config"]["vocab_size"], ids.shape, generator=torch.Generator().manual_seed(5))
    ids = torch.where(mask.bool(), ids, other)
    assert not torch.equal(ids, fx["input_ids"])
    with torch.no_grad():
        y2 = m.set_fp8_gemm(path)(ids, mask)
    valid = mask.bool().cuda()
    assert torch.equal(y2[valid], out[path][valid]) and not torch.equal(y2[~valid], out[path][~valid])


def test_sixteen_bit_encoder_is_unchanged(tiny, lib, tmp_path):
    """built and run after the FP8 encoders of this module: the stored golden within the yardstick, and from_pretrained without weight_dtype the same bits"""
    from pixart_sigma_amd.t5 import T5Encoder
    fx = tiny[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = T5Encoder(fx["config"])
    m.load_state_dict(fx["state_dict"])
    m = m.cuda()
    assert m.weight_dtype is None and m.b0_wqkv.dtype == lib.OPERAND_DTYPE
    with torch.no_grad():
        y = m(fx["input_ids"], fx["attention_mask"])
    assert m._scratch is None
    assert rel_l2(y.cpu(), fx["last_hidden_state"]) <= MARGIN * t5_fixtures.ref_noise()["t5_tiny"][lib.OPERAND]
    write_model_dir(str(tmp_path / "t5"), fx)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m2 = T5Encoder.from_pretrained(str(tmp_path / "t5"), device="cuda")
    with torch.no_grad():
        assert m2.weight_dtype is None and torch.equal(m2(fx["input_ids"], fx["attention_mask"]), y)


def test_quantize_tool_then_feature_tool_end_to_end(tiny, lib, tmp_path):
    """tools/quantize_t5.py, then tools/extract_t5_features.py on its output, each in a child process (both pin the bf16 build): the feature files equal the
    in-process FP8 forward on the path auto takes - bit for bit when this process is the bf16 build too."""
    import numpy as np
    fx, m, out = tiny
    write_model_dir(str(tmp_path / "t5"), fx)
    torch.save({"input_ids": fx["input_ids"], "attention_mask": fx["attention_mask"]}, tmp_path / "ids.pt")
    B, L = fx["input_ids"].shape
    env = {k: v for k, v in os.environ.items() if k != "PXA_T5_FP8_GEMM"}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "quantize_t5.py"), "--t5_path", str(tmp_path / "t5"), "--out", str(tmp_path / "fp8")],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    from safetensors import safe_open
    with safe_open(str(tmp_path / "fp8" / "model.safetensors"), framework="pt") as f:
        assert f.get_tensor("encoder.block.0.layer.0.SelfAttention.q.weight").dtype == torch.float8_e4m3fn
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_t5_features.py"), "--t5_path", str(tmp_path / "fp8"), "--ids", str(tmp_path / "ids.pt"),
                        "--out", str(tmp_path / "feats"), "--max_length", str(L)], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "feats")) == [f"{i}.npz" for i in range(B)] + ["null.npz"]
    got = torch.cat([torch.from_numpy(np.load(tmp_path / "feats" / f"{i}.npz")["caption_feature"]) for i in range(B)])
    want = out[m.set_fp8_gemm("auto").fp8_gemm_path(B * L)]
    if lib.OPERAND == "bf16":
        assert torch.equal(got, want.cpu())
    else:                                                  # the tools ran bf16, this process fp16: one yardstick apart
        assert rel_l2(got, want.cpu()) <= 2 * MARGIN * t5_fixtures.ref_noise()["t5_tiny"]["bf16"]
