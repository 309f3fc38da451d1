"""Host-side checks of the FP8 (e4m3fn) weight storage of the T5 encoder: the quantiser rule in torch (tests/t5_fp8_refs.py - what the GPU tests pin the HIP
quantiser against), the file format and its round trip on the CPU, the refusals, the condition under which the model tests may use the stored yardsticks, the
plan entry of the streaming GEMM, and the weight_dtype option on its way through CaptionEncoder, tools/extract_t5_features.py, scripts/inference.py and
train_scripts/train.py.  No GPU."""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import warnings

import pytest
import torch

import t5_fixtures
import t5_fp8_refs as R
import t5_refs
from conftest import ROOT, rel_l2

MARGIN = 1.1
FP8 = torch.float8_e4m3fn


def _encoder(cfg, **kw):
    from pixart_sigma_amd.t5 import T5Encoder
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return T5Encoder(cfg, **kw)


def _load_script(monkeypatch, rel):
    monkeypatch.setenv("PXA_OPERAND_DTYPE", os.environ.get("PXA_OPERAND_DTYPE", "bf16"))
    monkeypatch.setattr("sys.argv", ["x"])
    spec = importlib.util.spec_from_file_location("t5fp8_" + os.path.basename(rel)[:-3], os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ops():
    from pixart_sigma_amd import build, ops as o
    build.build()
    return o


# ------------------------------------------------------------------------------------------------ the quantiser rule
def wide_matrices():
    W = t5_refs.WIDE
    return {k: v for k, v in t5_refs.state_dict(W["cfg"], W["seed"]).items() if R.is_matrix(k)}


def test_quantiser_rule_properties():
    worst_rel, worst_fro = 0.0, 0.0
    for k, w in wide_matrices().items():
        w = w.clone()
        w[3] = 0                                                   # an all-zero row
        q, s = R.quant_rows(w)
        assert torch.equal(torch.exp2(torch.log2(s).round()), s) and (s > 0).all(), k          # powers of two
        assert s[3] == 1.0 and (q[3].view(torch.uint8) == 0).all()
        bits = q.view(torch.uint8)
        assert not ((bits & 0x7F) == 0x7F).any(), k                                            # no NaN code
        amax = w.float().abs().amax(1)
        nz = amax > 0
        assert ((amax / s)[nz] <= 448).all() and ((amax / s)[nz] > 224).all(), k                # the smallest power of two that fits
        d = R.dequant(q, s)
        assert torch.equal(d.to(torch.bfloat16).float(), d), k                                 # scale * q is a bf16 number
        wf, sc = w.float(), s[:, None]
        err, big = (wf - d).abs(), wf.abs() >= sc * 2.0 ** -6
        assert (err[big] <= wf.abs()[big] / 17 * (1 + 1e-6)).all(), k                          # three mantissa bits: half a step of 1/8 at 1 + 1/16
        assert (err[~big] <= (sc * 2.0 ** -10).expand_as(err)[~big]).all(), k                  # half the subnormal step 2^-9
        worst_rel = max(worst_rel, (err[big] / wf.abs()[big]).max().item())
        worst_fro = max(worst_fro, rel_l2(d, wf))
    print(f"\nt5_wide matrices through the rule: worst element {worst_rel:.4f} (1/17 = {1 / 17:.4f}), worst relative Frobenius error {worst_fro:.3e}")
    assert worst_rel <= 1 / 17 + 1e-6


def test_quantiser_rule_edge_rows():
    w = torch.zeros(6, 16)
    w[0, 0] = 448 * 2.0 ** -5                                      # a maximum of exactly 448 * 2^e: scale 2^e, code 0x7E
    w[1, 0] = 448 * 2.0 ** -5 * (1 + 2.0 ** -23)                    # one ulp above: the next power of two
    w[3, :3] = torch.tensor([448.0, 1.0625, -1.1875])              # scale 1: 1.0625 ties to 1.0 (even), -1.1875 ties to -1.25 (even)
    w[4, :3] = torch.tensor([448.0, 2.0 ** -11, 2.0 ** -10])       # below half the subnormal step -> 0; exactly half -> 0 (even)
    w[5, :2] = torch.tensor([448.0, -0.0])
    q, s = R.quant_rows(w)
    b = q.view(torch.uint8)
    assert s[0] == 2.0 ** -5 and b[0, 0] == 0x7E
    assert s[1] == 2.0 ** -4
    assert s[3] == 1 and q[3, 1].float() == 1.0 and q[3, 2].float() == -1.25
    assert b[4, 1] == 0 and b[4, 2] == 0
    assert b[5, 1] == 0x80


# ------------------------------------------------------------------------------------------------ files
def tiny_fp8_encoder(scale_shape="vector"):
    fx = t5_fixtures.load("t5_tiny")
    m = _encoder(fx["config"], weight_dtype="fp8_e4m3")
    m.load_state_dict(R.fp8_state_dict(fx["state_dict"], scale_shape))           # FP8 tensors: taken as they are, no GPU
    return fx, m


def _same_bytes(a, b):
    na, nb = dict(a.named_buffers()), dict(b.named_buffers())
    assert na.keys() == nb.keys()
    for k in na:
        assert na[k].dtype == nb[k].dtype and na[k].shape == nb[k].shape, k
        x, y = na[k].contiguous(), nb[k].contiguous()
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), k


def test_fp8_encoder_holds_half_the_weight_bytes_and_the_quantised_bits():
    fx, m = tiny_fp8_encoder()
    m16 = _encoder(fx["config"])
    c = m.config
    inner = c.num_heads * c.d_kv
    for i in range(c.num_layers):
        for n in ("wqkv", "wo", "wi0", "wi1", "wff"):
            q, w16 = getattr(m, f"b{i}_{n}"), getattr(m16, f"b{i}_{n}")
            assert q.dtype == FP8 and q.shape == w16.shape and q.numel() * q.element_size() * 2 == w16.numel() * w16.element_size()
            assert getattr(m, f"b{i}_{n}_scale").dtype == torch.float32 and getattr(m, f"b{i}_{n}_scale").shape == (q.shape[0],)
    assert m.embed.dtype == m16.embed.dtype and m.b0_ln0.dtype == torch.float32 and m.rel_bias.dtype == torch.float32
    want_q, want_s = R.quant_rows(fx["state_dict"]["encoder.block.0.layer.0.SelfAttention.k.weight"])
    assert torch.equal(m.b0_wqkv[inner:2 * inner].view(torch.uint8), want_q.view(torch.uint8)) and torch.equal(m.b0_wqkv_scale[inner:2 * inner], want_s)


def test_save_pretrained_from_pretrained_round_trip_on_bytes(tmp_path):
    from pixart_sigma_amd.t5 import T5Encoder
    from safetensors import safe_open
    fx, m = tiny_fp8_encoder()
    m.save_pretrained(str(tmp_path / "fp8"))
    with safe_open(str(tmp_path / "fp8" / "model.safetensors"), framework="pt") as f:
        keys = set(f.keys())
        k = "encoder.block.1.layer.1.DenseReluDense.wo.weight"
        assert f.get_tensor(k).dtype == FP8 and f.get_tensor(k + "_scale").dtype == torch.float32
        assert tuple(f.get_tensor(k + "_scale").shape) == (fx["config"]["d_model"],)
        assert "encoder.block.0.layer.0.SelfAttention.q.weight_scale" in keys and "shared.weight" in keys
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m2 = T5Encoder.from_pretrained(str(tmp_path / "fp8"))                        # weight_dtype None: as stored
    assert m2.weight_dtype == "fp8_e4m3"
    _same_bytes(m, m2)
    m2.save_pretrained(str(tmp_path / "again"))
    assert open(tmp_path / "fp8" / "model.safetensors", "rb").read() == open(tmp_path / "again" / "model.safetensors", "rb").read()


@pytest.mark.parametrize("shape", ["vector", "column", "scalar", "missing"])
def test_scale_shapes_on_reading(shape):
    fx = t5_fixtures.load("t5_tiny")
    sd = R.fp8_state_dict(fx["state_dict"], "column" if shape == "column" else "vector")
    key = "encoder.block.0.layer.1.DenseReluDense.wi_0.weight"
    if shape == "scalar":
        sd = {k: (torch.tensor(0.25) if k.endswith("_scale") else v) for k, v in sd.items()}
    if shape == "missing":
        sd = {k: v for k, v in sd.items() if not k.endswith("_scale")}
    m = _encoder(fx["config"], weight_dtype="fp8_e4m3")
    m.load_state_dict(sd)
    want = {"vector": sd.get(key + "_scale"), "column": None, "scalar": torch.full((m.config.d_ff,), 0.25), "missing": torch.ones(m.config.d_ff)}[shape]
    if shape == "column":
        want = sd[key + "_scale"][:, 0]
    assert torch.equal(m.b0_wi0_scale, want)
    assert torch.equal(m.b0_wi0.view(torch.uint8), sd[key].view(torch.uint8))
    bad = dict(sd)
    bad[key + "_scale"] = torch.ones(3)
    with pytest.raises(ValueError, match="weight_scale"):
        _encoder(fx["config"], weight_dtype="fp8_e4m3").load_state_dict(bad)


def test_refusals():
    fx = t5_fixtures.load("t5_tiny")
    sd = R.fp8_state_dict(fx["state_dict"])
    key = "encoder.block.1.layer.0.SelfAttention.o.weight"
    for code in (0x7F, 0xFF):
        bad = dict(sd)
        b = sd[key].clone().view(torch.uint8)
        b[2, 5] = code
        bad[key] = b.view(FP8)
        with pytest.raises(ValueError, match="SelfAttention.o.weight.*NaN"):
            _encoder(fx["config"], weight_dtype="fp8_e4m3").load_state_dict(bad)
    with pytest.raises(ValueError, match="multiples of 16"):
        _encoder(dict(fx["config"], d_ff=fx["config"]["d_ff"] + 8), weight_dtype="fp8_e4m3")
    with pytest.raises(ValueError, match="weight_dtype"):
        _encoder(fx["config"], weight_dtype="int8")
    with pytest.raises(ValueError, match="fp8_e4m3"):                               # FP8 matrices into a 16-bit encoder: said, not cast without their scales
        _encoder(fx["config"]).load_state_dict({k: v for k, v in sd.items() if not k.endswith("_scale")})
    with pytest.raises(KeyError, match="unexpected"):
        _encoder(fx["config"]).load_state_dict({**fx["state_dict"], key + "_scale": torch.ones(1)})
    with pytest.raises(ValueError, match="set_fp8_gemm"):
        _encoder(fx["config"], weight_dtype="fp8_e4m3").set_fp8_gemm("fast")
    m = _encoder(fx["config"], weight_dtype="fp8_e4m3")
    assert m.fp8_gemm_path(1) == "stream" and m.fp8_gemm_path(10 ** 6) == "dequant" and m.set_fp8_gemm("dequant").fp8_gemm_path(1) == "dequant"
    if not torch.cuda.is_available():                                                # 16-bit weights into an FP8 encoder need the quantiser kernel
        from pixart_sigma_amd import lib
        with pytest.raises(lib.PixartHipError, match="pxa_fp8_quant_rows"):
            _encoder(fx["config"], weight_dtype="fp8_e4m3").load_state_dict(fx["state_dict"])


def test_sixteen_bit_directories_load_as_before(tmp_path):
    from pixart_sigma_amd.t5 import T5Encoder
    from safetensors.torch import save_file
    fx = t5_fixtures.load("t5_tiny")
    d = tmp_path / "t5"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(dict(fx["config"], model_type="t5")))
    save_file({k: v.clone() for k, v in fx["state_dict"].items() if k != "encoder.embed_tokens.weight"}, str(d / "model.safetensors"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = T5Encoder.from_pretrained(str(d))
    ref = _encoder(fx["config"])
    ref.load_state_dict(fx["state_dict"])
    assert m.weight_dtype is None and all(b.dtype != FP8 for b in m.buffers()) and not any(n.endswith("_scale") for n, _ in m.named_buffers())
    _same_bytes(m, ref)
    m.save_pretrained(str(tmp_path / "again"))                                       # a 16-bit encoder writes a 16-bit directory
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _same_bytes(T5Encoder.from_pretrained(str(tmp_path / "again")), ref)


# ------------------------------------------------------------------------------------------------ the condition the model bound rests on
def _emulation_over_yardstick(cfg, sd, ids, mask, yard, rows=None):
    """encoder64 with the module's rounding points on the DEQUANTISED weights against encoder64 on the same weights, over the yardstick, per operand type"""
    out = {}
    for key, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        dq = R.dequant_state_dict(sd, through=dt)
        want = t5_refs.encoder64(cfg, dq, ids, mask)[-1]
        got = t5_refs.encoder64(cfg, dq, ids, mask, round_to=dt)[-1]
        D = want.shape[-1]
        out[key] = {name: rel_l2(got.reshape(-1, D)[sl], want.reshape(-1, D)[sl]) / yard(key, name) for name, sl in (rows or {"all_rows": slice(None)}).items()}
    return out


@pytest.mark.parametrize("name", ["t5_tiny", "t5_l300"])
def test_yardstick_is_usable_on_dequantised_weights(name):
    fx = t5_fixtures.load(name)
    noise = t5_fixtures.ref_noise()[name]
    r = _emulation_over_yardstick(fx["config"], fx["state_dict"], fx["input_ids"], fx["attention_mask"], lambda key, _: noise[key])
    print(f"\n{name}: emulation on dequantised weights / yardstick: {r}")
    for key in r:
        assert r[key]["all_rows"] <= MARGIN, (name, key, r)


def test_yardstick_is_usable_on_dequantised_weights_wide():
    W = t5_refs.WIDE
    with open(os.path.join(t5_fixtures.GOLDEN_DIR, "t5_wide.json")) as f:
        rec = json.load(f)
    sd = t5_refs.state_dict(W["cfg"], W["seed"])
    ids, mask = t5_refs.inputs(W["cfg"], W["B"], W["L"], W["lens"], W["seed"])
    r = _emulation_over_yardstick(t5_refs.full_config(W["cfg"]), sd, ids, mask, lambda key, rows: rec["yardstick"][key][rows],
                                  rows={"all_rows": slice(None), "tail_rows": t5_refs.WIDE_TAIL})
    print(f"\nt5_wide: emulation on dequantised weights / yardstick: {r}")
    for key in r:
        assert r[key]["all_rows"] <= MARGIN and r[key]["tail_rows"] <= MARGIN, (key, r)


# ------------------------------------------------------------------------------------------------ the plan entry
def _w8(M, N, K, lda=None, ldq=None, **kw):
    a = torch.zeros(M, lda or K, dtype=torch.bfloat16)[:, :K] if M else torch.zeros(0, K, dtype=torch.bfloat16)
    q = torch.zeros(N, ldq or K, dtype=torch.uint8).view(FP8)[:, :K]
    return a, q, torch.ones(N)


def test_gemm_w8_plan_names_the_instance_and_refuses_like_the_launch(ops):
    from pixart_sigma_amd import lib
    if ops.BF16 != torch.bfloat16:
        pytest.skip("operand type of this process is fp16: the host tensors below are bf16")
    max_m = ops.gemm_w8_max_m()
    assert max_m >= 512
    p = ops.gemm_w8_plan(*_w8(300, 4096, 4096)).split()
    assert p[0] == "gemm_w8_kernel<1,0>" and "split=1" in p and "m_tiles=5" in p and "n_tiles=64" in p, p
    p = ops.gemm_w8_plan(*_w8(300, 12288, 4096), act=ops.ACT_GELU).split()
    assert p[0] == "gemm_w8_kernel<2,1>" and "n_tiles=96" in p, p
    a, q, s = _w8(77, 10240, 4096)
    assert ops.gemm_w8_plan(a, q, s, act=ops.ACT_MUL_AUX, aux=torch.zeros(77, 10240, dtype=torch.bfloat16)).split()[0] == "gemm_w8_kernel<1,2>"
    a, q, s = _w8(300, 4096, 10240)
    assert ops.gemm_w8_plan(a, q, s, out_f32=torch.zeros(300, 4096)).split()[0] == "gemm_w8_kernel<1,3>"
    assert ops.gemm_w8_plan(*_w8(max_m, 128, 64)).split()[0] == "gemm_w8_kernel<1,0>"
    for args, word in ((_w8(0, 128, 64), "M=0"), (_w8(max_m + 1, 128, 64), f"M={max_m + 1}"), (_w8(16, 128, 72), "K=72"), (_w8(16, 132, 64), "N=132"),
                       (_w8(16, 128, 64, lda=68), "lda=68"), (_w8(16, 128, 64, ldq=72), "ldq=72")):
        with pytest.raises(lib.PixartHipError, match=r"rc=-1.*" + word):
            ops.gemm_w8_plan(*args)
    a, q, s = _w8(16, 128, 64)
    with pytest.raises(lib.PixartHipError, match="rc=-1.*16-byte"):
        ops.gemm_w8_plan(a, q, torch.ones(132)[1:129])
    with pytest.raises(lib.PixartHipError, match="rc=-1.*ld_f32"):
        ops.gemm_w8_plan(a, q, s, out_f32=torch.zeros(16, 132)[:, :128])


# ------------------------------------------------------------------------------------------------ the option on its way down
class _FakeProc:
    def __init__(self, cmd, **kw):
        _FakeProc.seen = dict(cmd=list(cmd), env=kw.get("env"))
        self.stdin = self.stdout = open(os.devnull, "rb")

    def poll(self):
        return 0


@pytest.mark.parametrize("weight_dtype", [None, "fp8_e4m3"])
def test_caption_encoder_hands_weight_dtype_to_its_worker_and_to_the_in_process_encoder(monkeypatch, tmp_path, weight_dtype):
    from pixart_sigma_amd.t5 import captions, encoder
    (tmp_path / "config.json").write_text(json.dumps(dict(d_model=64)))
    monkeypatch.setattr(captions.subprocess, "Popen", _FakeProc)
    monkeypatch.setattr(captions._Worker, "_await", lambda self, word, limit: [])
    ce = captions.CaptionEncoder(str(tmp_path), tokenizer=lambda *a, **k: None, model_max_length=8, device="cpu", max_batch=2, worker=True, weight_dtype=weight_dtype)
    cmd = _FakeProc.seen["cmd"]
    ce.close()
    assert cmd[1:4] == ["-m", "pixart_sigma_amd.t5.captions", "--worker"] and _FakeProc.seen["env"]["PXA_OPERAND_DTYPE"] == "bf16"
    assert (cmd[-2:] == ["--weight-dtype", "fp8_e4m3"]) if weight_dtype else ("--weight-dtype" not in cmd)
    seen = {}
    monkeypatch.setattr(captions.lib, "OPERAND", "bf16")
    monkeypatch.setattr(encoder.T5Encoder, "from_pretrained", classmethod(lambda cls, path, **kw: seen.update(path=path, **kw) or "enc"))
    ce = captions.CaptionEncoder(str(tmp_path), tokenizer=lambda *a, **k: None, model_max_length=8, device="cpu", worker=False, weight_dtype=weight_dtype)
    assert ce.encoder == "enc" and seen["weight_dtype"] == weight_dtype and ce.worker is None
    with pytest.raises(ValueError, match="weight_dtype"):
        captions.CaptionEncoder(str(tmp_path), tokenizer=lambda *a, **k: None, device="cpu", worker=False, weight_dtype="fp4")


def test_worker_program_parses_weight_dtype():
    src = open(os.path.join(ROOT, "pixart_sigma_amd", "t5", "captions.py")).read()
    assert 'add_argument("--weight-dtype", default=None)' in src and "weight_dtype=a.weight_dtype" in src


@pytest.mark.parametrize("flag", [[], ["--weight_dtype", "fp8_e4m3"]])
def test_extract_t5_features_passes_weight_dtype(monkeypatch, tmp_path, flag):
    tool = _load_script(monkeypatch, "tools/extract_t5_features.py")
    from pixart_sigma_amd.t5 import encoder
    seen = {}

    def fake(cls, path, **kw):
        seen.update(path=path, **kw)
        return lambda ids, mask: torch.zeros(ids.shape[0], ids.shape[1], 8)
    monkeypatch.setattr(encoder.T5Encoder, "from_pretrained", classmethod(fake))
    torch.save({"input_ids": torch.ones(2, 4, dtype=torch.long), "attention_mask": torch.ones(2, 4, dtype=torch.long)}, tmp_path / "ids.pt")
    monkeypatch.setattr("sys.argv", ["x", "--t5_path", "/models/t5", "--ids", str(tmp_path / "ids.pt"), "--out", str(tmp_path / "o"), "--max_length", "4"] + flag)
    tool.main()
    assert seen == dict(path="/models/t5", device="cuda", weight_dtype="fp8_e4m3" if flag else None)
    assert sorted(os.listdir(tmp_path / "o")) == ["0.npz", "1.npz", "null.npz"]
    monkeypatch.setattr("sys.argv", ["x", "--t5_path", "p", "--ids", "i", "--out", "o", "--weight_dtype", "int4"])
    with pytest.raises(SystemExit):
        tool.main()


def test_inference_child_command_carries_t5_weight_dtype(monkeypatch):
    inf = _load_script(monkeypatch, "scripts/inference.py")
    base = inf.t5_child_command(argparse.Namespace(t5_path="/m", t5_weight_dtype=None), "p.txt", "o", 300)
    assert "--weight_dtype" not in base
    assert inf.t5_child_command(argparse.Namespace(t5_path="/m", t5_weight_dtype="fp8_e4m3"), "p.txt", "o", 300) == base + ["--weight_dtype", "fp8_e4m3"]
    monkeypatch.setattr("sys.argv", ["x", "--t5_path", "/m", "--t5_weight_dtype", "fp8_e4m3"])
    assert inf.get_args().t5_weight_dtype == "fp8_e4m3"
    monkeypatch.setattr("sys.argv", ["x"])
    assert inf.get_args().t5_weight_dtype is None


def test_train_config_key_t5_weight_dtype(tmp_path):
    spec = importlib.util.spec_from_file_location("t5fp8_train", os.path.join(ROOT, "train_scripts", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    assert train.DEFAULTS["t5_weight_dtype"] is None and train.load_config(None)["t5_weight_dtype"] is None
    cfg = tmp_path / "c.py"
    cfg.write_text("t5_weight_dtype = 'fp8_e4m3'\n")
    assert train.load_config(str(cfg))["t5_weight_dtype"] == "fp8_e4m3"
    cfg.write_text("t5_weight_dtype = 'int8'\n")
    with pytest.raises(SystemExit, match="t5_weight_dtype"):
        train.load_config(str(cfg))
    src = open(os.path.join(ROOT, "train_scripts", "train.py")).read()
    assert 'weight_dtype=cfg["t5_weight_dtype"]' in src


def test_quantize_tool_and_bench_options_parse():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "quantize_t5.py"), "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and "--t5_path" in r.stdout and "--out" in r.stdout and "--device" in r.stdout
    src = open(os.path.join(ROOT, "tools", "bench_t5.py")).read()
    assert '"--weight_dtype"' in src and '"--fp8_gemm"' in src
