"""Host side of the T5 text encoder (pixart_sigma_amd/t5, csrc/t5.hip): the relative-position bucket port, the argument checks of the three entries (they
return -1 before any HIP call, so no GPU is needed), the ctypes mirror of pxa_t5_attn_args, the state-dict and directory loaders, T5Embedder with a stub
tokenizer, and the feature files of tools/extract_t5_features.py against scripts/inference.py's reader.  No GPU."""
import ctypes
import importlib.util
import json
import os
import re
import warnings

import pytest
import torch

import t5_fixtures
from conftest import ROOT


def _load_script(monkeypatch, rel):
    """Import a script by path.  Both scripts pin PXA_OPERAND_DTYPE for THEIR process at import: the variable is restored when the test ends."""
    monkeypatch.setenv("PXA_OPERAND_DTYPE", os.environ.get("PXA_OPERAND_DTYPE", "bf16"))
    monkeypatch.setattr("sys.argv", ["x"])
    spec = importlib.util.spec_from_file_location("t5test_" + os.path.basename(rel)[:-3], os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def L():
    from pixart_sigma_amd import build, lib
    build.build()
    return lib.load()


# ------------------------------------------------------------------------------------------------ buckets
@pytest.mark.parametrize("key,max_distance", [("32_128", 128), ("32_64", 64)])
def test_bucket_port_equals_transformers(key, max_distance):
    from pixart_sigma_amd.t5 import relative_position_bucket
    g = torch.load(os.path.join(t5_fixtures.GOLDEN_DIR, "t5_buckets.pt"), weights_only=False)
    assert g["offsets"][0] == -1023 and g["offsets"][-1] == 1023
    got = relative_position_bucket(g["offsets"], 32, max_distance)
    assert got.dtype == torch.long and torch.equal(got, g[key].long())
    assert int(got.min()) == 0 and int(got.max()) == 31


# ------------------------------------------------------------------------------------------------ the fp64 reference encoder of tests/t5_refs.py
def test_reference_buckets_equal_transformers():
    import t5_refs
    g = torch.load(os.path.join(t5_fixtures.GOLDEN_DIR, "t5_buckets.pt"), weights_only=False)
    assert torch.equal(t5_refs.buckets(g["offsets"], 32, 128), g["32_128"].long()) and torch.equal(t5_refs.buckets(g["offsets"], 32, 64), g["32_64"].long())


@pytest.mark.parametrize("name", ["t5_tiny", "t5_l300"])
def test_reference_encoder_equals_transformers_fp32(name):
    """t5_refs.encoder64 on the committed fixtures against their stored transformers-fp32 hidden states, per hidden state and per row.  Bound 1e-5: the stored
    outputs are fp32 (transformers' fp32 run of this architecture is 2.5e-6 rel-L2 from its own fp64 run); a wrong bucket, mask or GELU variant is off by
    percent.  Measured on last_hidden_state: t5_tiny 1.4e-6 whole, 7.6e-6 worst row; t5_l300 2.2e-6 whole, 6.0e-6 worst row (the block outputs: 0.5 - 1.1e-6 whole,
1.8 - 2.8e-6 worst row; the embedding is exact)."""
    import t5_refs
    fx = t5_fixtures.load(name)
    got = t5_refs.encoder64(fx["config"], fx["state_dict"], fx["input_ids"], fx["attention_mask"])
    assert len(got) == len(fx["hidden_states"]) == fx["config"]["num_layers"] + 1
    assert torch.equal(fx["hidden_states"][-1], fx["last_hidden_state"])
    D = fx["config"]["d_model"]
    for i, (h, want) in enumerate(zip(got, fx["hidden_states"])):
        assert h.dtype == torch.float64 and tuple(h.shape) == tuple(want.shape)
        whole = ((h - want.double()).norm() / want.double().norm()).item()
        rows = t5_refs.rel_l2_rows(h.reshape(-1, D), want.reshape(-1, D)).max().item()
        print(f"\n{name} hidden state {i}: whole {whole:.2e}, worst row {rows:.2e}", end="")
        assert whole <= 1e-5 and rows <= 1e-5, (name, i, whole, rows)


def test_wide_recipe_is_the_one_recorded():
    """the seeded weights and ids of t5_refs.WIDE hash to what tests/golden/t5_wide.json holds: its yardsticks are statements about exactly these tensors"""
    import t5_refs
    with open(os.path.join(t5_fixtures.GOLDEN_DIR, "t5_wide.json")) as f:
        rec = json.load(f)
    W = t5_refs.WIDE
    assert rec["cfg"] == t5_refs.full_config(W["cfg"]) and (rec["B"], rec["L"], rec["lens"], rec["seed"]) == (W["B"], W["L"], W["lens"], W["seed"])
    sd = t5_refs.state_dict(W["cfg"], W["seed"])
    ids, mask = t5_refs.inputs(W["cfg"], W["B"], W["L"], W["lens"], W["seed"])
    assert mask.sum(1).tolist() == W["lens"] and ids.shape == (W["B"], W["L"])
    assert all(torch.equal(v.float().to(torch.bfloat16), v) and torch.isfinite(v.float()).all() for v in sd.values())
    assert t5_refs.checksum(sd, ids) == rec["checksum"]


# ------------------------------------------------------------------------------------------------ argument checks
def _attn_args(lib, **over):
    buf = (ctypes.c_char * 4096)()                         # host memory, 16-byte aligned below; a refused call reads none of it
    base = (ctypes.addressof(buf) + 15) & ~15
    a = lib.T5AttnArgs()
    a.q = a.k = a.v = a.o = base
    a.bias = a.kv_len = base
    a.ldq = a.ldk = a.ldv = a.ldo = 192
    a.B, a.H, a.L, a.head_dim = 1, 3, 77, 64
    for k, v in over.items():
        setattr(a, k, v)
    return a, buf


@pytest.mark.parametrize("over,word", [
    (dict(q=None), "null"), (dict(o=None), "null"), (dict(bias=None), "null"), (dict(kv_len=None), "null"),
    (dict(head_dim=72), "head_dim=72"), (dict(head_dim=32), "head_dim=32"),
    (dict(ldq=196), "multiples of 8"), (dict(ldo=204), "multiples of 8"), (dict(ldk=184), ">= H*64"), (dict(ldv=128), ">= H*64"),
    (dict(L=0), "L=0"), (dict(L=513), "L=513"), (dict(H=0), "H=0"), (dict(H=65, ldq=4160, ldk=4160, ldv=4160, ldo=4160), "H=65"),
    (dict(B=0), "B=0"),
])
def test_attn_refuses_bad_arguments_without_a_gpu(L, over, word):
    from pixart_sigma_amd import lib
    a, keep = _attn_args(lib, **over)
    assert L.pxa_t5_attn(ctypes.byref(a), None) == -1
    msg = L.pxa_last_error().decode()
    assert msg.startswith("pxa_t5_attn") and word in msg, msg


def test_attn_refuses_a_misaligned_pointer_and_null_args(L):
    from pixart_sigma_amd import lib
    a, keep = _attn_args(lib)
    a.k = a.k + 8
    assert L.pxa_t5_attn(ctypes.byref(a), None) == -1 and "16-byte" in L.pxa_last_error().decode()
    assert L.pxa_t5_attn(None, None) == -1 and "null" in L.pxa_last_error().decode()


def test_rmsnorm_and_embed_refuse_bad_arguments_without_a_gpu(L):
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)

    def err():
        return L.pxa_last_error().decode()
    assert L.pxa_t5_rmsnorm(None, p, p, p, 4, 128, 1e-6, None) == -1 and "null" in err()
    assert L.pxa_t5_rmsnorm(p, None, p, p, 4, 128, 1e-6, None) == -1 and "null" in err()
    assert L.pxa_t5_rmsnorm(p, p, None, None, 4, 128, 1e-6, None) == -1 and "null" in err()
    assert L.pxa_t5_rmsnorm(p, p, p, None, 4, 132, 1e-6, None) == -1 and "D=132" in err()
    assert L.pxa_t5_rmsnorm(p, p, p, None, 4, 0, 1e-6, None) == -1 and "D=0" in err()
    assert L.pxa_t5_rmsnorm(p, p, p, None, 0, 128, 1e-6, None) == -1 and "R=0" in err()
    assert L.pxa_t5_embed(None, p, p, 4, 128, 64, None) == -1 and "null" in err()
    assert L.pxa_t5_embed(p, None, p, 4, 128, 64, None) == -1 and "null" in err()
    assert L.pxa_t5_embed(p, p, None, 4, 128, 64, None) == -1 and "null" in err()
    assert L.pxa_t5_embed(p, p, p, 4, 100, 64, None) == -1 and "D=100" in err()
    assert L.pxa_t5_embed(p, p, p, 0, 128, 64, None) == -1 and "R=0" in err()
    assert L.pxa_t5_embed(p, p, p, 4, 128, 0, None) == -1 and "vocab=0" in err()


def test_attn_args_struct_has_the_c_field_order():
    from pixart_sigma_amd import lib
    src = open(os.path.join(ROOT, "include", "pixart_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} pxa_t5_attn_args", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, kinds = [], []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        kind = lib.c_void_p if "*" in decl else lib.c_long if decl.startswith("long") else lib.c_int
        for part in decl.split(","):
            fields.append(re.findall(r"[A-Za-z_0-9]+", part)[-1])
            kinds.append(kind)
    assert fields == [f[0] for f in lib.T5AttnArgs._fields_]
    assert kinds == [f[1] for f in lib.T5AttnArgs._fields_]
    for name in ("pxa_t5_attn", "pxa_t5_rmsnorm", "pxa_t5_embed"):
        assert name in lib.SIGNATURES and re.search(r"int\s+" + name + r"\s*\(", src)


# ------------------------------------------------------------------------------------------------ state dict
def _encoder(cfg=None, **over):
    from pixart_sigma_amd.t5 import T5Encoder
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # the fp16-build notice, when the suite runs under PXA_OPERAND_DTYPE=f16
        return T5Encoder(dict(cfg or t5_fixtures.load("t5_tiny")["config"], **over))


def _same_weights(a, b):
    return all(torch.equal(x, y) for (_, x), (_, y) in zip(sorted(a.named_buffers()), sorted(b.named_buffers())))


def test_state_dict_of_the_fixture_loads_and_is_held_once_in_the_operand_type():
    from pixart_sigma_amd import lib
    fx = t5_fixtures.load("t5_tiny")
    sd = fx["state_dict"]
    m = _encoder()
    m.load_state_dict(sd)
    inner = 3 * 64
    assert m.b0_wqkv.dtype == lib.OPERAND_DTYPE and tuple(m.b0_wqkv.shape) == (3 * inner, 128)
    for j, n in enumerate("qkv"):
        assert torch.equal(m.b1_wqkv[j * inner:(j + 1) * inner].float(), sd[f"encoder.block.1.layer.0.SelfAttention.{n}.weight"].to(lib.OPERAND_DTYPE).float())
    assert m.b0_ln0.dtype == torch.float32 and torch.equal(m.b0_ln0, sd["encoder.block.0.layer.0.layer_norm.weight"].float())
    assert m.rel_bias.dtype == torch.float32 and tuple(m.rel_bias.shape) == (32, 3)
    assert torch.equal(m.embed.float(), sd["shared.weight"].to(lib.OPERAND_DTYPE).float())
    n_16bit = sum(b.numel() for _, b in m.named_buffers() if b.dtype == lib.OPERAND_DTYPE)
    n_all = sum(b.numel() for _, b in m.named_buffers())
    n_src = sum(v.numel() for k, v in sd.items() if k != "encoder.embed_tokens.weight")
    assert n_all == n_src and n_16bit > 0.99 * n_all       # every weight once; nothing but the norm weights and the bias embedding in fp32
    assert not any(p.requires_grad for p in m.parameters())


@pytest.mark.parametrize("keep", ["shared.weight", "encoder.embed_tokens.weight"])
def test_either_embedding_key_alone_loads(keep):
    sd = dict(t5_fixtures.load("t5_tiny")["state_dict"])
    full = _encoder()
    full.load_state_dict(sd)
    drop = "encoder.embed_tokens.weight" if keep == "shared.weight" else "shared.weight"
    assert drop in sd and keep in sd
    del sd[drop]
    m = _encoder()
    m.load_state_dict(sd)
    assert _same_weights(m, full)
    del sd[keep]
    with pytest.raises(KeyError, match="missing"):
        _encoder().load_state_dict(sd)


def test_full_model_dict_with_decoder_keys_loads_and_other_keys_do_not():
    sd = dict(t5_fixtures.load("t5_tiny")["state_dict"])
    full = _encoder()
    full.load_state_dict(sd)
    sd["decoder.block.0.layer.0.SelfAttention.q.weight"] = torch.zeros(192, 128)
    sd["decoder.final_layer_norm.weight"] = torch.zeros(128)
    sd["lm_head.weight"] = torch.zeros(64, 128)
    m = _encoder()
    m.load_state_dict(sd)
    assert _same_weights(m, full)
    sd["encoder.block.7.layer.0.layer_norm.weight"] = torch.zeros(128)
    with pytest.raises(KeyError, match="unexpected"):
        _encoder().load_state_dict(sd)


def test_wrong_shape_and_unsupported_configs_are_refused():
    from pixart_sigma_amd.t5 import T5Encoder
    sd = dict(t5_fixtures.load("t5_tiny")["state_dict"])
    sd["encoder.block.0.layer.1.DenseReluDense.wi_1.weight"] = torch.zeros(320, 64)
    with pytest.raises(ValueError, match="wi_1.*shape"):
        _encoder().load_state_dict(sd)
    cfg = t5_fixtures.load("t5_tiny")["config"]
    with pytest.raises(ValueError, match="feed_forward_proj"):
        T5Encoder(dict(cfg, feed_forward_proj="relu"))
    with pytest.raises(ValueError, match="feed_forward_proj"):
        T5Encoder(dict(cfg, feed_forward_proj="gated-silu"))
    with pytest.raises(ValueError, match="d_kv=32"):
        T5Encoder(dict(cfg, d_kv=32))
    with pytest.raises(ValueError, match="num_heads=65"):
        T5Encoder(dict(cfg, num_heads=65))


def test_masks_and_lengths_are_checked_on_the_host():
    from pixart_sigma_amd.t5 import key_lengths
    assert key_lengths(torch.tensor([[1, 1, 1, 0], [1, 0, 0, 0], [1, 1, 1, 1]])).tolist() == [3, 1, 4]
    with pytest.raises(ValueError, match="row 1 has no valid token"):
        key_lengths(torch.tensor([[1, 1, 0], [0, 0, 0]]))
    with pytest.raises(ValueError, match="right-padded"):
        key_lengths(torch.tensor([[1, 0, 1]]))


def test_forward_raises_without_a_gpu_and_refuses_bad_inputs():
    from pixart_sigma_amd import lib
    m = _encoder()
    m.load_state_dict(t5_fixtures.load("t5_tiny")["state_dict"])
    ids = torch.zeros(1, 8, dtype=torch.long)
    if not torch.cuda.is_available():
        with pytest.raises(lib.PixartHipError, match="no CPU"):
            m(ids, torch.ones(1, 8, dtype=torch.long))
        return
    m = m.cuda()
    with pytest.raises(ValueError, match="1 .. 512"):
        m(torch.zeros(1, 513, dtype=torch.long))
    with pytest.raises(ValueError, match="vocabulary"):
        m(ids + 64)
    with pytest.raises(ValueError, match="no valid token"):
        m(ids, torch.zeros(1, 8, dtype=torch.long))


# ------------------------------------------------------------------------------------------------ directories
def _write_dir(path, fx, kind):
    from safetensors.torch import save_file
    os.makedirs(path)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dict(fx["config"], architectures=["T5EncoderModel"], model_type="t5", dropout_rate=0.1), f)
    sd = {k: v.clone() for k, v in fx["state_dict"].items() if k != "encoder.embed_tokens.weight"}       # safetensors refuses shared storage; HF drops the tied copy too
    sd["decoder.final_layer_norm.weight"] = torch.ones(128, dtype=torch.bfloat16)
    keys = sorted(sd)
    if kind == "single":
        save_file(sd, os.path.join(path, "model.safetensors"))
        return
    halves = [keys[:len(keys) // 2], keys[len(keys) // 2:]]
    ext, stem = ("safetensors", "model") if kind == "st_shards" else ("bin", "pytorch_model")
    weight_map = {}
    for i, ks in enumerate(halves):
        name = f"{stem}-{i + 1:05d}-of-00002.{ext}"
        part = {k: sd[k] for k in ks}
        save_file(part, os.path.join(path, name)) if ext == "safetensors" else torch.save(part, os.path.join(path, name))
        weight_map.update({k: name for k in ks})
    with open(os.path.join(path, f"{stem}.{ext}.index.json"), "w") as f:
        json.dump({"metadata": {}, "weight_map": weight_map}, f)


@pytest.mark.parametrize("kind", ["single", "st_shards", "bin_shards"])
def test_from_pretrained_reads_the_three_directory_layouts(tmp_path, kind):
    from pixart_sigma_amd.t5 import T5Encoder
    fx = t5_fixtures.load("t5_tiny")
    _write_dir(str(tmp_path / kind), fx, kind)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = T5Encoder.from_pretrained(str(tmp_path / kind))
    full = _encoder()
    full.load_state_dict(fx["state_dict"])
    assert m.config == full.config and _same_weights(m, full)


def test_from_pretrained_without_weights_says_so(tmp_path):
    from pixart_sigma_amd.t5 import T5Encoder
    with open(tmp_path / "config.json", "w") as f:
        json.dump(t5_fixtures.load("t5_tiny")["config"], f)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(FileNotFoundError, match="model.safetensors"):
            T5Encoder.from_pretrained(str(tmp_path))


def test_product_path_does_not_import_transformers():
    import subprocess
    import sys
    code = "import sys; import pixart_sigma_amd.t5; assert 'transformers' not in sys.modules; print('ok')"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ embedder
def test_embedder_passes_ids_and_mask_through_and_applies_model_max_length():
    from pixart_sigma_amd.t5 import T5Embedder
    seen = {}

    def tokenizer(texts, **kw):
        seen["texts"], seen["kw"] = list(texts), kw
        n, Lmax = len(texts), kw["max_length"]
        ids = torch.zeros(n, Lmax + 3, dtype=torch.long)       # a tokenizer that ignores truncation: the embedder still cuts at model_max_length
        mask = torch.zeros(n, Lmax + 3, dtype=torch.long)
        for i, t in enumerate(texts):
            k = min(len(t.split()) + 1, Lmax + 3)
            ids[i, :k] = torch.arange(2, 2 + k)
            mask[i, :k] = 1
        return {"input_ids": ids, "attention_mask": mask}

    calls = []

    def recorder(ids, mask):
        calls.append((ids.clone(), mask.clone()))
        return torch.zeros(ids.shape[0], ids.shape[1], 16)
    emb = T5Embedder(recorder, tokenizer, model_max_length=5)
    texts = ["a cat", "a very long caption of nine words in total here"]
    embs, mask = emb.get_text_embeddings(texts)
    assert seen["texts"] == texts
    assert seen["kw"] == dict(max_length=5, padding="max_length", truncation=True, return_attention_mask=True, add_special_tokens=True, return_tensors="pt")
    assert len(calls) == 1
    ids_seen, mask_seen = calls[0]
    assert tuple(ids_seen.shape) == (2, 5) and tuple(mask_seen.shape) == (2, 5)
    assert ids_seen[0].tolist() == [2, 3, 4, 0, 0] and mask_seen[0].tolist() == [1, 1, 1, 0, 0]
    assert ids_seen[1].tolist() == [2, 3, 4, 5, 6] and mask_seen[1].tolist() == [1, 1, 1, 1, 1]
    assert tuple(embs.shape) == (2, 5, 16) and torch.equal(mask, mask_seen)
    assert T5Embedder(recorder, tokenizer).model_max_length == 120
    assert "out of scope" in T5Embedder.__doc__.lower()


# ------------------------------------------------------------------------------------------------ feature files
def test_feature_writer_matches_the_inference_reader(tmp_path, monkeypatch):
    tool = _load_script(monkeypatch, "tools/extract_t5_features.py")
    inf = _load_script(monkeypatch, "scripts/inference.py")
    import argparse
    import numpy as np
    g = torch.Generator().manual_seed(3)
    n, Lq, D = 3, 300, 4096
    feats = torch.randn(n, Lq, D, generator=g)
    masks = (torch.arange(Lq)[None, :] < torch.tensor([300, 1, 40])[:, None]).to(torch.int32)
    null, null_mask = torch.randn(1, Lq, D, generator=g), (torch.arange(Lq)[None, :] < 1).long()
    names = tool.write_features(str(tmp_path), feats, masks, null, null_mask)
    assert names == ["0.npz", "1.npz", "2.npz", "null.npz"] and sorted(os.listdir(tmp_path)) == sorted(names)
    z = np.load(tmp_path / "1.npz")
    assert sorted(z.files) == ["attention_mask", "caption_feature"]
    assert z["caption_feature"].shape == (1, Lq, D) and z["caption_feature"].dtype == np.float32
    assert z["attention_mask"].shape == (1, Lq) and z["attention_mask"].dtype == np.int64
    zn = np.load(tmp_path / "null.npz")
    assert zn["caption_feature"].shape == (1, Lq, D) and zn["attention_mask"].shape == (1, Lq) and zn["attention_mask"].sum() == 1
    args = argparse.Namespace(synthetic=False, caption_feats=str(tmp_path), seed=0)
    y, m, null_y = inf.load_captions(args, n, Lq, "cpu")
    assert tuple(y.shape) == (n, 1, Lq, D) and torch.equal(y[:, 0], feats)
    assert tuple(m.shape) == (n, Lq) and torch.equal(m, masks.long())
    assert tuple(null_y.shape) == (1, 1, Lq, D) and torch.equal(null_y[0], null)
    y2, m2, _ = inf.load_captions(args, 2, 120, "cpu", first=1)                 # the sigma reader cuts at its own L; --t5_path indexes by prompt
    assert torch.equal(y2[:, 0], feats[1:3, :120]) and torch.equal(m2, masks[1:3, :120].long())


def test_inference_t5_child_runs_the_tool_under_bf16(monkeypatch, tmp_path):
    inf = _load_script(monkeypatch, "scripts/inference.py")
    import argparse
    import subprocess
    monkeypatch.chdir(tmp_path)
    seen = {}

    def fake_run(cmd, env=None, timeout=None, **kw):
        seen.update(cmd=cmd, env=env, timeout=timeout)
        return subprocess.CompletedProcess(cmd, 0)
    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setenv("PXA_OPERAND_DTYPE", "f16")
    args = argparse.Namespace(t5_path="/models/t5", save_name="s", t5_timeout=77)
    out = inf.encode_prompts(args, ["a cat", "a dog"], 300)
    assert out == os.path.join("output", "s", "caption_feats")
    assert open(os.path.join(out, "prompts.txt")).read() == "a cat\na dog\n"
    assert seen["env"]["PXA_OPERAND_DTYPE"] == "bf16" and seen["timeout"] == 77
    assert seen["cmd"][1].endswith(os.path.join("tools", "extract_t5_features.py"))
    assert seen["cmd"][2:] == ["--t5_path", "/models/t5", "--prompts", os.path.join(out, "prompts.txt"), "--out", out, "--max_length", "300"]


def test_fp16_build_warns_once_and_bf16_does_not():
    import subprocess
    import sys
    code = ("import warnings, sys; sys.path.insert(0, 'tests'); import t5_fixtures\n"
            "from pixart_sigma_amd.t5 import T5Encoder\n"
            "cfg = t5_fixtures.load('t5_tiny')['config']\n"
            "with warnings.catch_warnings(record=True) as w:\n"
            "    warnings.simplefilter('always'); T5Encoder(cfg); T5Encoder(cfg)\n"
            "print(len([x for x in w if 'fp16' in str(x.message)]))")
    for operand, want in (("f16", "1"), ("bf16", "0")):
        env = dict(os.environ, PXA_OPERAND_DTYPE=operand)
        env.pop("PXA_LIB_PATH", None)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env)
        assert r.returncode == 0 and r.stdout.split()[-1] == want, (operand, r.stdout, r.stderr[-1000:])
