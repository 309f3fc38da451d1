"""LoRA adapters, host side (no GPU): the internal <-> peft key map and file layout, the refusals, and the launch schedule of a backward with adapters
attached, driven on the CPU stand-ins (tests/fake_ops.py, tests/ops_trace.py, tests/lora_fakes.py)."""
import json
import os
import re

import pytest
import torch

import lora_fakes
import ops_trace
from pixart_sigma_amd import lora
from pixart_sigma_amd.lora import BLOCK_MODULES, LoraConfig

D = ops_trace.D


def _model(**kw):
    from pixart_sigma_amd.model.nets.PixArtMS import PixArtMS
    torch.manual_seed(0)
    return PixArtMS(depth=2, input_size=8, model_max_length=8, class_dropout_prob=0.0, **kw)


# ---------------------------------------------------------------------------------------------- key map and files
def test_key_round_trip_covers_all_ten_modules_per_block():
    assert len(BLOCK_MODULES) == 10
    seen = set()
    for i in (0, 27):
        for mod in BLOCK_MODULES:
            for leaf, peft_leaf in (("lora_A", "lora_A"), ("lora_Bt", "lora_B")):
                name = f"blocks.{i}.{mod}.{leaf}"
                key = lora.peft_key(name)
                assert key == f"base_model.model.transformer_blocks.{i}.{mod}.{peft_leaf}.weight"
                assert lora.internal_name(key) == name
                assert lora.internal_name(key.replace(".weight", ".default.weight")) == name          # peft's in-memory keys carry the adapter name
                seen.add(key)
    assert len(seen) == 2 * 10 * 2
    for bad in ("base_model.model.proj_out.lora_A.weight", "base_model.model.transformer_blocks.0.attn1.to_q.weight",
                "base_model.model.transformer_blocks.0.attn3.to_q.lora_A.weight"):
        with pytest.raises(KeyError):
            lora.internal_name(bad)


def test_slices_of_fused_linears_and_shapes():
    m = _model()
    lo = m.add_lora(LoraConfig(r=4, target_modules=list(BLOCK_MODULES)))
    assert lo.slices["blocks.1.attn.qkv"] == [(0, D, "blocks.1.attn1.to_q"), (D, 2 * D, "blocks.1.attn1.to_k"), (2 * D, 3 * D, "blocks.1.attn1.to_v")]
    assert lo.slices["blocks.0.cross_attn.kv_linear"] == [(0, D, "blocks.0.attn2.to_k"), (D, 2 * D, "blocks.0.attn2.to_v")]
    assert lo.slices["blocks.0.mlp.fc1"] == [(0, 4 * D, "blocks.0.ff.net.0.proj")]
    sd = lo.state_dict()
    assert len(sd) == 2 * 10 * 2
    assert tuple(sd["base_model.model.transformer_blocks.0.ff.net.0.proj.lora_A.weight"].shape) == (4, D)
    assert tuple(sd["base_model.model.transformer_blocks.0.ff.net.0.proj.lora_B.weight"].shape) == (4 * D, 4)
    assert tuple(sd["base_model.model.transformer_blocks.1.ff.net.2.lora_A.weight"].shape) == (4, 4 * D)
    assert tuple(sd["base_model.model.transformer_blocks.1.attn2.to_v.lora_B.weight"].shape) == (D, 4)
    # gaussian init: B = 0, A drawn; everything but the adapters is frozen; the base parameter list is what it was
    assert all(not p.requires_grad for p in m.parameters()) and all(p.requires_grad for p in m.lora_parameters())
    assert all(k.endswith("lora_A.weight") or not v.any() for k, v in sd.items())
    assert not any("lora" in n for n, _ in m.named_parameters()) and not any("lora" in k for k in m.state_dict())
    a = sd["base_model.model.transformer_blocks.0.attn1.to_q.lora_A.weight"]
    assert abs(a.std().item() - 0.25) < 0.02                 # peft draws A with std 1 / r
    # suffix targets, the reference's way of naming them: to_q adapts attn1.to_q and attn2.to_q
    assert lora.resolve_targets(["to_q", "ff.net.2"]) == ["attn1.to_q", "attn2.to_q", "ff.net.2"]
    assert lora.resolve_targets(list(lora.DEFAULT_TARGETS)) == list(BLOCK_MODULES)
    assert LoraConfig(r=16).scaling == 0.5 and LoraConfig(r=16, use_rslora=True).scaling == 2.0 and LoraConfig(r=4, lora_alpha=32).scaling == 8.0


def test_save_load_round_trip_is_bit_exact(tmp_path):
    m = _model()
    lo = m.add_lora(LoraConfig(r=8, lora_alpha=16, use_rslora=True, target_modules=["to_q", "to_k", "to_v", "to_out.0", "ff.net.0.proj", "ff.net.2"]))
    with torch.no_grad():
        for p in m.lora_parameters():
            p.normal_()
    m.save_lora(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["adapter_config.json", "adapter_model.safetensors"]
    cfg = json.load(open(tmp_path / "adapter_config.json"))
    want = dict(peft_type="LORA", r=8, lora_alpha=16, use_rslora=True, use_dora=False, lora_dropout=0.0, bias="none",
                target_modules=["to_q", "to_k", "to_v", "to_out.0", "ff.net.0.proj", "ff.net.2"])
    assert {k: cfg[k] for k in want} == want
    from safetensors.torch import load_file
    sd = load_file(str(tmp_path / "adapter_model.safetensors"))
    assert set(sd) == set(lo.state_dict()) and all(v.dtype == torch.float32 for v in sd.values())
    m2 = _model()
    lo2 = m2.load_lora(str(tmp_path))
    assert lo2.config.r == 8 and lo2.config.use_rslora and lo2.scale == lo.scale == 16 / 8 ** 0.5
    assert list(lo2.params) == list(lo.params)
    for n in lo.params:
        assert torch.equal(lo.params[n], lo2.params[n]), n
    # a file that lacks a tensor, or carries a foreign one, is an error
    bad = dict(sd)
    bad.pop("base_model.model.transformer_blocks.1.ff.net.2.lora_B.weight")
    with pytest.raises(KeyError):
        lo2.load_state_dict(bad)
    with pytest.raises(KeyError):
        lo2.load_state_dict(dict(sd, **{"base_model.model.proj_out.lora_A.weight": torch.zeros(8, D)}))


def test_merge_and_unload_on_the_host_folds_into_the_master():
    m = _model()
    w0 = m.blocks[1].attn.qkv.weight.detach().clone()
    lo = m.add_lora(LoraConfig(r=2, target_modules=["attn1.to_k"]))
    with torch.no_grad():
        for p in m.lora_parameters():
            p.normal_()
    a, bt, s = lo.params["blocks.1.attn1.to_k.lora_A"].detach(), lo.params["blocks.1.attn1.to_k.lora_Bt"].detach(), lo.scale
    m.merge_and_unload()
    assert m._lora is None and m.lora_parameters() == [] and all(p.requires_grad for p in m.parameters())
    w1 = m.blocks[1].attn.qkv.weight.detach()
    assert torch.equal(w1[:D], w0[:D]) and torch.equal(w1[2 * D:], w0[2 * D:])
    assert torch.allclose(w1[D:2 * D], w0[D:2 * D] + s * bt.t() @ a, rtol=0, atol=1e-5)
    with pytest.raises(RuntimeError):
        m.set_lora_scale(1.0)


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("target", ["proj", "linear", "linear_1", "linear_2", "proj_in", "proj_out"])
def test_targets_outside_the_blocks_raise(target):
    with pytest.raises(NotImplementedError, match="not implemented for modules outside the transformer blocks"):
        LoraConfig(r=4, target_modules=["to_q", target])
    with pytest.raises(NotImplementedError, match="outside the transformer blocks"):
        _model().add_lora(r=4, target_modules=[target])


def test_dora_dropout_rank_and_unknown_targets_raise(tmp_path):
    with pytest.raises(NotImplementedError, match="DoRA"):
        LoraConfig(r=4, use_dora=True)
    with pytest.raises(NotImplementedError, match="dropout"):
        LoraConfig(r=4, lora_dropout=0.1)
    for r in (0, 65, 128, 2.5):
        with pytest.raises(ValueError, match="rank"):
            LoraConfig(r=r)
    LoraConfig(r=64), LoraConfig(r=1)
    with pytest.raises(ValueError, match="matches no linear"):
        LoraConfig(r=4, target_modules=["to_qq"])
    m = _model()
    m.add_lora(r=4)
    with pytest.raises(RuntimeError, match="already carries"):
        m.add_lora(r=4)
    # a DoRA file is refused when it is read
    m.save_lora(str(tmp_path))
    cfg = json.load(open(tmp_path / "adapter_config.json"))
    json.dump(dict(cfg, use_dora=True), open(tmp_path / "adapter_config.json", "w"))
    with pytest.raises(NotImplementedError):
        _model().load_lora(str(tmp_path))


def test_came_on_adapters_is_refused():
    from pixart_sigma_amd.dp import FusedCAME
    with ops_trace._env(), lora_fakes.recording():
        m = _model()
        m.add_lora(LoraConfig(r=4))
        m._prepare(torch.device("cpu"))
        with pytest.raises(NotImplementedError, match="CAME"):
            FusedCAME(m)


# ---------------------------------------------------------------------------------------------- launch schedule
def _parse(line):
    return dict(re.findall(r"(\w+)=((?:\w+(?:\[[^\]]*\])?\+\d+:\([\d,]*\)/\([\d,]*\):\w+)|[^ ]+)", line))


def _buf(arg):
    """'t75+1152:(32,1152)/(3456,1):bf16' -> (buffer, element offset, shape, strides)"""
    mo = re.fullmatch(r"([^+]+)\+(\d+):\(([\d,]*)\)/\(([\d,]*)\):\w+", arg)
    tup = lambda s: tuple(int(v) for v in s.split(",") if v)     # noqa: E731
    return mo.group(1), int(mo.group(2)), tup(mo.group(3)), tup(mo.group(4))


@pytest.mark.parametrize("save", ["all", "ckpt"])
def test_backward_schedule_with_adapters_on_every_target(save):
    lines, m = lora_fakes.lora_case(save=save)
    base = [l for l in open(ops_trace.fixture("plain_all" if save == "all" else "plain_ckpt")).read().splitlines() if not l.startswith("#")]
    bwd = lines[lines.index("# backward") + 1:]
    # no weight-gradient (TN) GEMM, no bias column sum, no bias partials, nothing into the base gradient buffer
    assert not [l for l in bwd if l.startswith("gemm ") and "layout=2" in l]
    assert not [l for l in bwd if l.split(" ")[0] in ("colsum", "colsum_reduce", "patch_embed_bwd")]
    assert not [l for l in bwd if re.search(r"=grad\[(?!blocks\.\d+\.[\w.]+\.lora_)", l)]
    assert all("dbias=None" in l for l in bwd if l.startswith("gate_bwd ")) and all("colsum=None" in l for l in bwd if "act=4" in l)
    # the same grad_ready_hook prefixes, in the same order, as the schedule without adapters
    hooks = lambda ls: [l for l in ls if l.startswith("grad_ready_hook")]     # noqa: E731
    assert hooks(lines) == hooks(base) == ["grad_ready_hook prefix='final'", "grad_ready_hook prefix='blocks.1'", "grad_ready_hook prefix='blocks.0'"]
    # exactly one lora_bwd per adapted slice, on its own adapter tensors
    calls = [_parse(l) for l in bwd if l.startswith("lora_bwd ")]
    assert len(calls) == 2 * 10
    by_ad = {}
    for c in calls:
        ad = re.fullmatch(r"shadow\[(.+)\.lora_A\]", _buf(c["A16"])[0]).group(1)
        assert ad not in by_ad
        by_ad[ad] = c
        assert _buf(c["Bt16"])[0] == f"shadow[{ad}.lora_Bt]" and _buf(c["dA"])[0] == f"grad[{ad}.lora_A]" and _buf(c["dBt"])[0] == f"grad[{ad}.lora_Bt]"
        assert float(c["s"]) == m._lora.scale == 2.0
    assert sorted(by_ad) == sorted(f"blocks.{i}.{mod}" for i in range(2) for mod in BLOCK_MODULES)
    # ... before the block's group is reported complete
    for i in range(2):
        done = bwd.index(f"grad_ready_hook prefix='blocks.{i}'")
        idx = [k for k, l in enumerate(bwd) if l.startswith("lora_bwd ") and f"[blocks.{i}." in l]
        assert len(idx) == 10 and max(idx) < done and (i == 1 or min(idx) > bwd.index("grad_ready_hook prefix='blocks.1'"))
    # x / dy: the buffers and column blocks of the dX GEMM that follows (dy) and of the forward GEMM that produced dy's primal (x)
    R, Lt = ops_trace.B * 16, sum(ops_trace.LENS)
    for i in range(2):
        q, k, v = (by_ad[f"blocks.{i}.attn1.to_{n}"] for n in "qkv")
        assert _buf(q["x"]) == _buf(k["x"]) == _buf(v["x"]) and _buf(q["x"])[2] == (R, D)
        dq, dk, dv = _buf(q["dy"]), _buf(k["dy"]), _buf(v["dy"])
        assert dq[0] == dk[0] == dv[0] and (dq[1], dk[1], dv[1]) == (0, D, 2 * D) and dq[2:] == dk[2:] == dv[2:] == ((R, D), (3 * D, 1))
        ck, cv = by_ad[f"blocks.{i}.attn2.to_k"], by_ad[f"blocks.{i}.attn2.to_v"]
        assert _buf(ck["x"]) == _buf(cv["x"]) and _buf(ck["x"])[2] == (Lt, D)                       # the packed caption rows: sum(lens) of them
        assert _buf(ck["dy"])[0] == _buf(cv["dy"])[0] and (_buf(ck["dy"])[1], _buf(cv["dy"])[1]) == (0, D) and _buf(ck["dy"])[2:] == ((Lt, D), (2 * D, 1))
        assert _buf(by_ad[f"blocks.{i}.ff.net.0.proj"]["x"])[2] == (R, D) and _buf(by_ad[f"blocks.{i}.ff.net.0.proj"]["dy"])[2] == (R, 4 * D)
        assert _buf(by_ad[f"blocks.{i}.ff.net.2"]["x"])[2] == (R, 4 * D) and _buf(by_ad[f"blocks.{i}.ff.net.2"]["dy"])[2] == (R, D)
        # the dX GEMM behind each call reads the same dy (whole matrix for the fused linears) against the merged shadow weight
        for mod, (lin, j, n) in BLOCK_MODULES.items():
            if lin == "cross_attn.kv_linear":
                continue                                                                                   # frozen caption MLP: no dX for the text rows
            at = next(k for k, l in enumerate(bwd) if l.startswith("lora_bwd ") and f"[blocks.{i}.{mod}.lora_A]" in l)
            nxt = next(_parse(l) for l in bwd[at:] if l.startswith("gemm "))
            assert _buf(nxt["b"])[0] == f"shadow[blocks.{i}.{lin}.weight]" and nxt["layout"] == "1"
            assert _buf(nxt["a"])[0] == _buf(by_ad[f"blocks.{i}.{mod}"]["dy"])[0]
    # x of every adapted linear is the A operand its forward GEMM read (saved, or recomputed under checkpointing)
    fwd_a = {}
    for l in lines:
        if l.startswith("gemm ") and "layout=0" in l:
            p = _parse(l)
            wname = re.fullmatch(r"(?:shadow\[(.+)\.weight\]|qs_w)", _buf(p["b"])[0])
            if wname:
                fwd_a.setdefault(wname.group(1) or "qs", []).append(_buf(p["a"]))
    for i in range(2):
        for mod, (lin, j, n) in BLOCK_MODULES.items():
            pool = fwd_a["qs"] if lin == "attn.qkv" else fwd_a[f"blocks.{i}.{lin}"]
            assert _buf(by_ad[f"blocks.{i}.{mod}"]["x"]) in pool, (i, mod)


def test_merge_follows_every_recast_and_adapter_update():
    """Every bump of the base store (a re-cast wipes the merge) and every bump of the adapter store (an optimizer step) re-merges all slices behind the
    prescaled-qkv rewrite, in place, and moves the generation that keys the text cache."""
    import fake_ops
    with ops_trace._env(), lora_fakes.recording():
        m = _model()
        m.add_lora(LoraConfig(r=4, target_modules=["to_q", "to_v"]))
        m._prepare(torch.device("cpu"))
        S, A = m._store, m._lora.store
        nsl = 2 * 4                                        # attn1.to_q / to_v, attn2.to_q / to_v, two blocks

        def merges(fn):
            del fake_ops.CALLS[:]
            g = S.generation
            fn()
            ops_ = [c[0] for c in fake_ops.CALLS if c[0] in ("scale_copy", "lora_merge")]
            return ops_, S.generation - g
        ops_, dg = merges(lambda: S.refresh_shadow(force=True))
        assert ops_ == ["scale_copy"] * 2 + ["lora_merge"] * nsl and dg == 1
        ops_, dg = merges(A.bump)                           # what FusedAdamW.step does to the adapter store
        assert ops_ == ["scale_copy"] * 2 + ["lora_merge"] * nsl and dg == 1
        with torch.no_grad():
            m._lora.params["blocks.0.attn1.to_q.lora_Bt"].add_(1.0)
        ops_, dg = merges(lambda: m._prepare(torch.device("cpu")))      # an edit of an adapter by torch ops: re-cast of the adapters, then the merge
        assert ops_[-nsl:] == ["lora_merge"] * nsl and dg == 1
        ops_, dg = merges(lambda: m._prepare(torch.device("cpu")))      # nothing changed: nothing runs
        assert ops_ == [] and dg == 0
        ops_, dg = merges(lambda: m.set_lora_scale(0.0))
        assert ops_[-nsl:] == ["lora_merge"] * nsl and dg == 1 and m._lora.scale == 0.0
        # the q slice of attn.qkv carries the prescaled copy as its second destination; the others do not
        del fake_ops.CALLS[:]
        assert m._engine._qs is not None


def test_fused_adamw_takes_the_adapter_store():
    from pixart_sigma_amd.dp import FusedAdamW
    with ops_trace._env(), lora_fakes.recording():
        m = _model()
        m.add_lora(LoraConfig(r=4))
        m._prepare(torch.device("cpu"))
        opt = FusedAdamW(m, lr=1e-3)
        assert opt.store is m._lora.store and opt.m.numel() == m._lora.store.total < m._store.total // 100
        assert sorted(opt.store.groups) == ["blocks.0", "blocks.1"]
        opt._check_store()
        m._lora.store = None                                   # the adapters' store was rebuilt / dropped after the optimizer was made
        m._lora.store = type(opt.store).__new__(type(opt.store))
        with pytest.raises(RuntimeError, match="rebuilt its flat parameter store"):
            opt._check_store()
