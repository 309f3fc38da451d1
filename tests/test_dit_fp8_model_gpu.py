"""FP8 inference of the denoiser (PixArtMS.enable_fp8) on the GPU, in the process's operand build: depth-2 models at the default width with seeded random
weights (oracle.weights), ragged captions.

What is compared, as relative L2 of the model output:
* `mx` (ops.gemm_f8 on the block-scaled MFMA) against `dequant` (the same quantised operands, dequantised exactly, through the 16-bit ops.gemm): the two
  differ by the summation order inside a GEMM and by the 16-bit roundings that order flips, propagated through two blocks;
* `mx` against the 16-bit forward of the same weights: what quantising the six token GEMMs of a block to MXFP8 costs.  RANDOM-WEIGHT EVIDENCE ONLY: it says
  nothing about pictures from a trained checkpoint.
Both are printed, kept with record_parity and asserted at twice the worst value measured on an MI355X over the cases below (the table in CASE_NOTES).

And the plumbing: a captured sampling graph follows a weight load (the MX weight copies are rewritten in place), disable_fp8() restores the 16-bit output bit
for bit, training forwards and adapters are refused."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from conftest import record_parity, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (latent (Hl, Wl), model options).  B = 2: 16 x 24 latents are M = 192 token rows (a row tail of the 128-row GEMM tile), 32 x 32 are M = 512.
CASES = {
    "plain_16x24": ((16, 24), {}),
    "plain_32x32": ((32, 32), {}),
    "kvconv_16x24": ((16, 24), dict(kv_sampling="conv", kv_scale_factor=2, kv_layers=(1,))),
    "qknorm_16x24": ((16, 24), dict(qk_norm=True)),
}
# Worst measured over CASES on an MI355X (bf16 build / fp16 build), see CASE_NOTES; asserted at twice that.
MEASURED_MX_VS_DEQUANT = {"bf16": 4.58e-3, "f16": 2.55e-3}
MEASURED_MX_VS_16BIT = {"bf16": 2.10e-2, "f16": 2.16e-2}
CASE_NOTES = """measured rel-L2 (bf16 build / fp16 build):
    case            mx vs dequant          mx vs 16-bit
    plain_16x24     3.52e-3 / 1.90e-3      1.56e-2 / 1.56e-2
    plain_32x32     3.35e-3 / 1.86e-3      1.54e-2 / 1.57e-2
    kvconv_16x24    4.02e-3 / 2.30e-3      1.79e-2 / 1.73e-2
    qknorm_16x24    4.58e-3 / 2.55e-3      2.10e-2 / 2.16e-2
mx vs dequant is well above one 16-bit rounding because a flipped rounding of an activation can flip its FP8 code at the next quantiser (a 2^-4 relative step),
and, in the fp16 build, because the dequantised operands of `dequant` lose what falls below fp16's normal range."""
L_TEXT, LENS = 20, [20, 9]


def build(latent, opts, seed=0):
    from oracle import pixart_oracle as po
    from oracle.weights import make_inputs, make_state_dict
    from pixart_sigma_amd import build_model
    cfg = po.OracleCfg(depth=2, input_size=16, model_max_length=L_TEXT, **opts)
    kv = {"sampling": cfg.kv_sampling, "scale_factor": cfg.kv_scale_factor, "kv_compress_layer": list(cfg.kv_layers)} if cfg.kv_sampling else None
    m = build_model("PixArtMS", depth=2, hidden_size=1152, num_heads=16, input_size=16, model_max_length=L_TEXT, class_dropout_prob=0.0,
                    qk_norm=cfg.qk_norm, kv_compress_config=kv)
    m.load_state_dict(make_state_dict(cfg, seed=seed))
    m = m.to("cuda:0").eval()
    inp = make_inputs(B=2, Hl=latent[0], Wl=latent[1], L=L_TEXT, seed=1, lens=LENS)
    return m, inp


def fwd(m, inp):
    with torch.no_grad():
        y = m(inp["x"].cuda(), inp["t"].cuda(), inp["y"].cuda(), mask=inp["mask"], data_info=None)
    torch.cuda.synchronize()
    return y.float().cpu()


@pytest.fixture(scope="module")
def outputs():
    """case -> (16-bit output, mx output, dequant output, 16-bit output after disable_fp8), computed once."""
    out = {}
    for name, (latent, opts) in CASES.items():
        m, inp = build(latent, opts)
        y16 = fwd(m, inp)
        assert m.fp8 is None
        m.enable_fp8("mx")
        assert m.fp8 == "mx"
        ymx = fwd(m, inp)
        m.enable_fp8("dequant")
        assert m.fp8 == "dequant"
        ydq = fwd(m, inp)
        m.disable_fp8()
        assert m.fp8 is None
        out[name] = (y16, ymx, ydq, fwd(m, inp))
        del m
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_mx_against_dequant_and_16bit(outputs, case):
    from pixart_sigma_amd import lib
    y16, ymx, ydq, _ = outputs[case]
    assert torch.isfinite(ymx).all() and torch.isfinite(ydq).all()
    e_dq, e_16 = rel_l2(ymx, ydq), rel_l2(ymx, y16)
    b_dq, b_16 = 2 * MEASURED_MX_VS_DEQUANT[lib.OPERAND], 2 * MEASURED_MX_VS_16BIT[lib.OPERAND]
    print(f"\nFP8 denoiser {case} [{lib.OPERAND}]: mx vs dequant rel-L2 {e_dq:.2e} (bound {b_dq:.1e}); mx vs the 16-bit forward {e_16:.2e} (bound {b_16:.1e}; "
          "random weights)")
    record_parity(f"dit fp8 {case}: mx vs dequant", e_dq, b_dq)
    record_parity(f"dit fp8 {case}: mx vs 16-bit (random weights)", e_16, b_16)
    assert e_dq > 0 or torch.equal(ymx, ydq)
    assert e_16 > 1e-4, "the FP8 forward equals the 16-bit one: it did not run on quantised operands"
    assert e_dq <= b_dq, (e_dq, b_dq)
    assert e_16 <= b_16, (e_16, b_16)


@pytest.mark.parametrize("case", list(CASES))
def test_disable_restores_the_16bit_output(outputs, case):
    y16, _, _, y16_again = outputs[case]
    assert torch.equal(y16, y16_again)


def test_graphed_sampler_follows_weight_updates_in_fp8():
    """The MX weight copies are buffers derived from the weights: they keep their addresses and are rewritten in place behind the prescaled qkv copy, so a
    replay of a captured sampling graph after load_state_dict equals a fresh eager FP8 sample bit for bit."""
    from pixart_sigma_amd import DPMS
    m, inp = build((16, 24), {})
    m.enable_fp8("mx")
    null_y = torch.randn(1, 1, L_TEXT, 4096, generator=torch.Generator().manual_seed(5)).repeat(2, 1, 1, 1).cuda()
    solver = DPMS(m.forward_with_dpmsolver, condition=inp["y"].cuda(), uncondition=null_y, cfg_scale=4.5, model_kwargs=dict(data_info=None, mask=inp["mask"]))
    kw = dict(steps=3, order=2, skip_type="time_uniform", method="multistep")
    x = inp["x"].cuda()
    g1 = solver.sample_graphed(x, **kw)
    assert torch.equal(g1, solver.sample(x, **kw))
    graph = solver._graph
    ptrs = {n: (q.data_ptr(), e.data_ptr()) for n, (q, e) in m._engine._f8.items()}
    w_before = m._engine._f8["mlp.fc1"][0].view(torch.uint8).clone()
    m.load_state_dict({k: (v * 1.3 if (".attn.qkv." in k or ".mlp.fc1.weight" in k) else v) for k, v in m.state_dict().items()})
    g2 = solver.sample_graphed(x, **kw)
    assert solver._graph is graph
    assert ptrs == {n: (q.data_ptr(), e.data_ptr()) for n, (q, e) in m._engine._f8.items()}, "a derived FP8 buffer moved"
    assert not torch.equal(w_before, m._engine._f8["mlp.fc1"][0].view(torch.uint8)), "the MX copy of mlp.fc1 was not re-quantised"
    assert not torch.equal(g2, g1), "new weights did not change the FP8 output"
    assert torch.equal(g2, solver.sample(x, **kw)), "the replay read stale FP8 weights"


def test_refusals():
    m, inp = build((16, 24), {})
    m.enable_fp8("mx")
    with pytest.raises(RuntimeError, match="torch.no_grad"):
        m(inp["x"].cuda(), inp["t"].cuda(), inp["y"].cuda(), mask=inp["mask"], data_info=None)        # gradients enabled
    with pytest.raises(RuntimeError, match="merge_and_unload"):
        m.add_lora(r=4)
    assert m._lora is None
    m.disable_fp8()
    m.add_lora(r=4)
    with pytest.raises(RuntimeError, match=r"merge_and_unload\(\) first"):
        m.enable_fp8("mx")
    assert m.fp8 is None
    m.merge_and_unload()
    m.enable_fp8("mx")
    assert torch.isfinite(fwd(m, inp)).all()
