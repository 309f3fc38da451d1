"""GPU parity of pixart_sigma_amd.t5.T5Encoder against transformers.T5EncoderModel's fp32 output (tests/golden/t5_tiny, t5_l300: made by
tools/make_t5_golden.py from the class the reference calls).

Bound: rel-L2 of last_hidden_state over ALL rows (padded ones included) <= 1.1 x the yardstick of the same fixture and operand type in
tests/golden/t5_ref_noise.json - what transformers' own bf16 / fp16 model loses against its fp32 run on the same input; the margin is the one the project
asserts against ref_fp16_noise.json.  A CPU emulation of this module's rounding points (operands and GEMM outputs rounded, fp32 residual and statistics, P
rounded) lands at 0.66 - 0.87 of the yardstick; a wrong bias index or mask moves the output by tens of percent at these logit spreads.  That emulation is
tests/t5_refs.py: encoder64(round_to=...).

Both fixtures keep every GEMM below pxa_gemm's M >= 1024 and N >= 1024 threshold (the 128 x 128 kernel).  test_parity_at_production_dispatch runs a third,
seeded one (t5_refs.WIDE; figures in tests/golden/t5_wide.json, no tensors) whose five calls per block take the instances of a production batch, against
encoder64 in fp64."""
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


def test_parity_at_production_dispatch(lib):
    """The encoder at a width where its five GEMM calls per block take the kernels a production batch takes (tests/test_t5_gemm_forms_gpu.py has them one by
    one): the seeded fixture t5_wide of tests/t5_refs.py, d_model 1024, 16 heads, d_ff 1280, 2 blocks, 4 x 300 tokens with lengths 300 / 137 / 1 / 77, so
    M = 1200 = 4 x 256 + 176 rows.  Weights and ids are regenerated from the recipe and must hash to what tests/golden/t5_wide.json records; the reference is
    t5_refs.encoder64 in fp64 on the GPU (3.5e-7 from transformers' fp64 model, whose norm takes its variance in fp32; transformers' fp32 run is 2.0e-6 from it).
    Asserted on last_hidden_state: rel-L2 over all rows, and over rows 1024 .. 1199 alone (the ragged last 256-row tile: padded positions of the last sample,
    computed like every row), each <= 1.1 x transformers' own loss in the operand type on the same rows (the json's yardstick; the margin is this file's).
    The CPU emulation of the module's rounding points (encoder64(round_to=...), in the json) lands at 0.65 (all rows) / 0.45 (tail rows) of the bf16
    yardstick and 0.78 / 0.70 of the fp16 one.  Measured on an MI355X: bf16 build 1.277e-2 = 0.651 x the yardstick over all rows, 1.227e-2 = 0.472 x over the
    tail rows (worst single row 3.6e-2); fp16 build 1.618e-3 = 0.769 x and 1.553e-3 = 0.667 x (worst row 4.3e-3)."""
    import t5_refs
    from pixart_sigma_amd import ops
    from pixart_sigma_amd.t5 import T5Encoder
    with open(os.path.join(t5_fixtures.GOLDEN_DIR, "t5_wide.json")) as f:
        rec = json.load(f)
    W = t5_refs.WIDE
    cfg = t5_refs.full_config(W["cfg"])
    sd = t5_refs.state_dict(W["cfg"], W["seed"])
    ids, mask = t5_refs.inputs(W["cfg"], W["B"], W["L"], W["lens"], W["seed"])
    assert rec["cfg"] == cfg and t5_refs.checksum(sd, ids) == rec["checksum"], "the regenerated weights / ids are not the ones t5_wide.json's figures were taken on"
    for key in ("bf16", "f16"):                            # the condition the yardstick is usable under: the emulation itself stays inside the margin
        for rows in ("all_rows", "tail_rows"):
            assert rec["emulation_vs_encoder64"][key][rows] <= MARGIN * rec["yardstick"][key][rows], (key, rows)
    # the five calls of this config name the instances of a production batch
    M, D, inner, dff, op = W["B"] * W["L"], cfg["d_model"], cfg["num_heads"] * cfg["d_kv"], cfg["d_ff"], lib.OPERAND_DTYPE
    assert M == 1200 and t5_refs.WIDE_TAIL == slice(1024, M)

    def plan(K, N, **kw):
        kw = {k: torch.empty(M, N, dtype=torch.float32 if k == "out_f32" else op) if k in ("aux", "out_f32") else v for k, v in kw.items()}
        return ops.gemm_plan(torch.empty(M, K, dtype=op), torch.empty(N, K, dtype=op), ops.NT, **kw).split()
    assert plan(D, 3 * inner)[0] == "gemm_pers_kernel<0,0,0,false>"
    assert plan(D, dff, act=ops.ACT_GELU)[0] == "gemm_pers_kernel<0,7,0,false>"
    assert plan(D, dff, act=ops.ACT_MUL_AUX, aux=True)[0] == "gemm_pers_kernel<0,3,0,false>"
    for K in (inner, dff):
        p = plan(K, D, out_f32=True, accumulate=True)
        assert p[0] == "gemm_glds_kernel<0,256,256,2,4,0,false>" and "accumulate=2" in p and "split=1" in p, p
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # the fp16-build notice
        m = T5Encoder(cfg)
    m.load_state_dict(sd)
    with torch.no_grad():
        y, hidden = m.cuda()(ids, mask, output_hidden_states=True)
    want = t5_refs.encoder64(cfg, sd, ids, mask, device="cuda")
    assert y.dtype == torch.float32 and tuple(y.shape) == (W["B"], W["L"], D) and torch.isfinite(y).all() and len(hidden) == len(want)
    for i, (h, g) in enumerate(zip(hidden, want)):
        record_parity(f"t5_wide hidden state {i} (0 = embedding, last = final norm) vs encoder64", rel_l2(h, g))
    yard = rec["yardstick"][lib.OPERAND]
    got2, want2 = y.reshape(M, D), want[-1].reshape(M, D)
    e_all, e_tail = rel_l2(got2, want2), rel_l2(got2[t5_refs.WIDE_TAIL], want2[t5_refs.WIDE_TAIL])
    worst_row = t5_refs.rel_l2_rows(got2, want2).max().item()
    record_parity(f"t5_wide last_hidden_state vs encoder64, all rows (bound = {MARGIN} x transformers' own {lib.OPERAND} error)", e_all, MARGIN * yard["all_rows"])
    record_parity(f"t5_wide last_hidden_state vs encoder64, rows 1024 .. 1199 (bound = {MARGIN} x transformers' own {lib.OPERAND} error there)", e_tail, MARGIN * yard["tail_rows"])
    record_parity("t5_wide error / yardstick, all rows", e_all / yard["all_rows"], MARGIN)
    record_parity("t5_wide error / yardstick, rows 1024 .. 1199", e_tail / yard["tail_rows"], MARGIN)
    record_parity("t5_wide last_hidden_state, worst row", worst_row)
    print(f"\nt5_wide [{lib.OPERAND}]: all rows {e_all:.3e} = {e_all / yard['all_rows']:.3f} x yardstick {yard['all_rows']:.3e}; rows 1024 .. 1199 {e_tail:.3e} = "
          f"{e_tail / yard['tail_rows']:.3f} x yardstick {yard['tail_rows']:.3e} (bound {MARGIN}); worst row {worst_row:.3e}", end="")
    assert e_all <= MARGIN * yard["all_rows"] and e_tail <= MARGIN * yard["tail_rows"]


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
