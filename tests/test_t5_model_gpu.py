"""GPU parity of pixart_sigma_amd.t5.T5Encoder against transformers.T5EncoderModel's fp32 output (tests/golden/t5_tiny, t5_l300: made by
tools/make_t5_golden.py from the class the reference calls).

Bound: rel-L2 of last_hidden_state over ALL rows (padded ones included) <= 1.1 x the yardstick of the same fixture and operand type in
tests/golden/t5_ref_noise.json - what transformers' own bf16 / fp16 model loses against its fp32 run on the same input; the margin is the one the project
asserts against ref_fp16_noise.json.  A CPU emulation of this module's rounding points (operands and GEMM outputs rounded, fp32 residual and statistics, P
rounded) lands at 0.66 - 0.87 of the yardstick; a wrong bias index or mask moves the output by tens of percent at these logit spreads."""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

import t5_fixtures  # noqa: E402
from conftest import ROOT, record_parity, rel_l2  # noqa: E402

MARGIN = 1.1


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pixart_sigma_amd import lib as l_
    return l_


def encoder(name):
    from pixart_sigma_amd.t5 import T5Encoder
    fx = t5_fixtures.load(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # the fp16-build notice
        m = T5Encoder(fx["config"])
    m.load_state_dict(fx["state_dict"])
    return fx, m.cuda()


@pytest.fixture(scope="module")
def tiny(lib):
    fx, m = encoder("t5_tiny")
    with torch.no_grad():
        y = m(fx["input_ids"], fx["attention_mask"])
    return fx, m, y


def write_model_dir(path, fx):
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dict(fx["config"], model_type="t5"), f)
    save_file({k: v.clone() for k, v in fx["state_dict"].items() if k != "encoder.embed_tokens.weight"}, os.path.join(path, "model.safetensors"))


@pytest.mark.parametrize("name", ["t5_tiny", "t5_l300"])
def test_parity_with_transformers_fp32(lib, name):
    fx, m = encoder(name)
    with torch.no_grad():
        y, hidden = m(fx["input_ids"], fx["attention_mask"], output_hidden_states=True)
    assert y.dtype == torch.float32 and tuple(y.shape) == tuple(fx["last_hidden_state"].shape)
    assert torch.isfinite(y).all()
    assert len(hidden) == len(fx["hidden_states"])
    for i, (h, g) in enumerate(zip(hidden, fx["hidden_states"])):
        record_parity(f"{name} hidden state {i} (0 = embedding, last = final norm) vs transformers fp32", rel_l2(h.cpu(), g))
    yard = t5_fixtures.ref_noise()[name][lib.OPERAND]
    e = rel_l2(y.cpu(), fx["last_hidden_state"])
    valid = fx["attention_mask"].bool()
    e_valid, e_pad = rel_l2(y.cpu()[valid], fx["last_hidden_state"][valid]), None
    if (~valid).any():
        e_pad = rel_l2(y.cpu()[~valid], fx["last_hidden_state"][~valid])
        record_parity(f"{name} last_hidden_state, padded rows only", e_pad)
    record_parity(f"{name} last_hidden_state, valid rows only", e_valid)
    record_parity(f"{name} last_hidden_state vs transformers fp32 (bound = {MARGIN} x transformers' own {lib.OPERAND} error)", e, MARGIN * yard)
    record_parity(f"{name} error / yardstick", e / yard, MARGIN)
    print(f"\n{name} [{lib.OPERAND}]: rel-L2 {e:.3e} = {e / yard:.3f} x transformers' own {lib.OPERAND} error {yard:.3e} (bound {MARGIN}); valid rows {e_valid:.3e}, "
          f"padded rows {e_pad}", end="")
    assert e <= MARGIN * yard


def test_ids_at_padded_positions_change_no_valid_row(tiny):
    fx, m, y = tiny
    ids, mask = fx["input_ids"].clone(), fx["attention_mask"]
    g = torch.Generator().manual_seed(5)
    other = torch.randint(2, fx["config"]["vocab_size"], ids.shape, generator=g)
    ids = torch.where(mask.bool(), ids, other)
    assert not torch.equal(ids, fx["input_ids"])
    with torch.no_grad():
        y2 = m(ids, mask)
    valid = mask.bool().cuda()
    assert torch.equal(y2[valid], y[valid])
    assert not torch.equal(y2[~valid], y[~valid])          # the padded rows are computed from their own ids, as T5EncoderModel computes them


def test_batch_equals_each_sample_alone(tiny):
    fx, m, y = tiny
    for b in range(fx["input_ids"].shape[0]):
        with torch.no_grad():
            one = m(fx["input_ids"][b:b + 1], fx["attention_mask"][b:b + 1])
        assert torch.equal(one[0], y[b]), b


def test_usable_under_no_grad_and_without_a_mask(tiny):
    fx, m, y = tiny
    full = (fx["attention_mask"].sum(1) == fx["attention_mask"].shape[1]).nonzero()[0].item()
    with torch.no_grad():
        a = m(fx["input_ids"][full:full + 1])
    b = m(fx["input_ids"][full:full + 1].cuda(), fx["attention_mask"][full:full + 1].cuda())         # device tensors, grad mode on: still no graph
    assert not a.requires_grad and not b.requires_grad
    assert torch.equal(a[0], y[full]) and torch.equal(b[0], y[full])


def test_from_pretrained_gives_the_same_output(tiny, tmp_path):
    from pixart_sigma_amd.t5 import T5Encoder
    fx, m, y = tiny
    write_model_dir(str(tmp_path / "t5"), fx)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m2 = T5Encoder.from_pretrained(str(tmp_path / "t5"), device="cuda")
    with torch.no_grad():
        assert torch.equal(m2(fx["input_ids"], fx["attention_mask"]), y)


def test_feature_tool_end_to_end(lib, tmp_path, monkeypatch):
    """tools/extract_t5_features.py on t5_tiny's ids in a child process (it pins the bf16 build), then scripts/inference.py's load_captions: the features equal
    the in-process forward - bit for bit when this process is the bf16 build too."""
    fx = t5_fixtures.load("t5_tiny")
    write_model_dir(str(tmp_path / "t5"), fx)
    torch.save({"input_ids": fx["input_ids"], "attention_mask": fx["attention_mask"]}, tmp_path / "ids.pt")
    out = tmp_path / "feats"
    B, L = fx["input_ids"].shape
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_t5_features.py"), "--t5_path", str(tmp_path / "t5"), "--ids", str(tmp_path / "ids.pt"),
                        "--out", str(out), "--max_length", str(L)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["0.npz", "1.npz", "2.npz", "null.npz"]
    monkeypatch.setenv("PXA_OPERAND_DTYPE", os.environ.get("PXA_OPERAND_DTYPE", "bf16"))           # the script pins its own process's build at import: restored
    monkeypatch.setattr("sys.argv", ["x"])
    spec = importlib.util.spec_from_file_location("t5test_inference", os.path.join(ROOT, "scripts", "inference.py"))
    inf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(inf)
    y, mask, null_y = inf.load_captions(argparse.Namespace(synthetic=False, caption_feats=str(out), seed=0), B, L, "cuda")
    D = fx["config"]["d_model"]
    assert tuple(y.shape) == (B, 1, L, D) and tuple(null_y.shape) == (1, 1, L, D) and torch.equal(mask, fx["attention_mask"])
    _, m = encoder("t5_tiny")
    null_ids, null_mask = torch.zeros(1, L, dtype=torch.long), torch.zeros(1, L, dtype=torch.long)
    null_ids[0, 0], null_mask[0, 0] = 1, 1
    with torch.no_grad():
        want, want_null = m(fx["input_ids"], fx["attention_mask"]), m(null_ids, null_mask)
    if lib.OPERAND == "bf16":
        assert torch.equal(y[:, 0], want) and torch.equal(null_y[0], want_null)
    else:                                                                                          # the tool ran bf16, this process fp16: one yardstick apart
        yard = t5_fixtures.ref_noise()["t5_tiny"]["bf16"]
        assert rel_l2(y[:, 0], want) <= 2 * MARGIN * yard
