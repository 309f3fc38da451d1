#!/usr/bin/env python
"""Recipe of the T5 encoder fixtures under tests/golden/ (CPU, needs `transformers`): the oracle is transformers.T5EncoderModel itself, the class the
reference calls (reference diffusion/model/t5.py:87,106-111), in fp32 and eval().

    python tools/make_t5_golden.py [--out tests/golden]

Writes
  t5_tiny.pt, t5_l300.pt   config, input_ids, attention_mask, last_hidden_state and the list of part files
  t5_<name>.partK.pt       the state dict (bf16, every value bf16-representable) and every hidden state (output_hidden_states, all rows), cut into files
                           below the repository's 1 MiB limit; tests/t5_fixtures.py puts them together again
  t5_buckets.pt            T5Attention._relative_position_bucket for offsets -1023 .. 1023 at (32, 128) and (32, 64)
  t5_ref_noise.json        the yardstick: rel-L2 of transformers' own bf16 model, and of its fp16 model, against its fp32 output on the same input
  t5_wide.json             a third, seeded fixture at widths >= 1024 and 1200 rows, as figures only (make_wide below; --only-wide writes it alone)
Weights: transformers' random init, then norm weights 1 + 0.2 N(0,1), the bias embedding 2 N(0,1), q weights x 8 (unscaled logits that spread as in a trained
T5), everything rounded to bf16."""
import argparse
import json
import os

import torch

FIXTURES = {
    "t5_tiny": dict(cfg=dict(d_model=128, num_heads=3, d_ff=320, num_layers=2, vocab_size=64), B=3, L=77, lens=[77, 1, 40], seed=20),
    "t5_l300": dict(cfg=dict(d_model=256, num_heads=4, d_ff=384, num_layers=2, vocab_size=64), B=2, L=300, lens=[300, 137], seed=21),
}
PART_BYTES = 900 * 1024


def make_model(cfg, seed):
    from transformers import T5Config, T5EncoderModel
    torch.manual_seed(seed)
    config = T5Config(feed_forward_proj="gated-gelu", d_kv=64, relative_attention_num_buckets=32, relative_attention_max_distance=128, dropout_rate=0.0,
                      is_encoder_decoder=False, use_cache=False, **cfg)
    model = T5EncoderModel(config).float().eval()
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("layer_norm.weight"):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith("relative_attention_bias.weight"):
                p.copy_(2 * torch.randn(p.shape, generator=g))
            elif name.endswith("SelfAttention.q.weight"):
                p.mul_(8)
        for p in model.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    return config, model


def make_inputs(B, L, lens, vocab, seed):
    g = torch.Generator().manual_seed(seed + 2000)
    ids = torch.randint(2, vocab, (B, L), generator=g)
    mask = (torch.arange(L)[None, :] < torch.tensor(lens)[:, None]).long()
    return ids * mask, mask                      # pad id 0 behind each caption


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def make_fixture(name, spec, out):
    config, model = make_model(spec["cfg"], spec["seed"])
    ids, mask = make_inputs(spec["B"], spec["L"], spec["lens"], spec["cfg"]["vocab_size"], spec["seed"])
    with torch.no_grad():
        ref = model(input_ids=ids, attention_mask=mask, output_hidden_states=True)
        noise = {}
        for key, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
            low = model.to(dt)(input_ids=ids, attention_mask=mask)["last_hidden_state"].float()
            noise[key] = rel_l2(low, ref["last_hidden_state"])
            model.float()
    assert torch.isfinite(ref["last_hidden_state"]).all()
    items = [("state_dict." + k, v.to(torch.bfloat16).clone()) for k, v in model.state_dict().items()]
    items += [(f"hidden_states.{i}", h.clone()) for i, h in enumerate(ref["hidden_states"])]
    parts, cur, size = [], {}, 0
    for k, v in items:
        n = v.numel() * v.element_size()
        if cur and size + n > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += n
    parts.append(cur)
    names = []
    for i, p in enumerate(parts):
        names.append(f"{name}.part{i}.pt")
        torch.save(p, os.path.join(out, names[-1]))
    cfg_keys = ("vocab_size", "d_model", "d_kv", "d_ff", "num_layers", "num_heads", "relative_attention_num_buckets", "relative_attention_max_distance",
                "layer_norm_epsilon", "feed_forward_proj")
    torch.save(dict(config={k: getattr(config, k) for k in cfg_keys}, input_ids=ids, attention_mask=mask, last_hidden_state=ref["last_hidden_state"].clone(),
                    parts=names, lens=spec["lens"]), os.path.join(out, name + ".pt"))
    n_par = sum(p.numel() for p in model.parameters())
    print(f"{name}: {n_par / 1e6:.2f} M parameters, {len(names)} part files, transformers bf16 {noise['bf16']:.3e}, fp16 {noise['f16']:.3e}")
    return noise


def make_wide(out):
    """t5_wide.json: the seeded recipe of tests/t5_refs.py (no tensor is stored: the tests regenerate weights and ids and compare the checksum) loaded into
    transformers.T5EncoderModel; what transformers' own bf16 / fp16 model loses against its fp32 output, over all rows and over the rows of the ragged last
    256-row tile; how far t5_refs.encoder64 is from transformers' fp64 output, and its rounding-point emulations from its fp64 output, on the same row sets."""
    import sys
    from transformers import T5Config, T5EncoderModel
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import t5_refs
    W = t5_refs.WIDE
    cfg = t5_refs.full_config(W["cfg"])
    sd = t5_refs.state_dict(W["cfg"], W["seed"])
    ids, mask = t5_refs.inputs(W["cfg"], W["B"], W["L"], W["lens"], W["seed"])
    config = T5Config(dropout_rate=0.0, is_encoder_decoder=False, use_cache=False, **cfg)
    model = T5EncoderModel(config).eval()
    model.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    D, tail = cfg["d_model"], t5_refs.WIDE_TAIL

    def both(got, want):
        got, want = got.reshape(-1, D), want.reshape(-1, D)
        return dict(all_rows=rel_l2(got, want), tail_rows=rel_l2(got[tail], want[tail]))
    with torch.no_grad():
        hf64 = model.double()(input_ids=ids, attention_mask=mask)["last_hidden_state"]
        hf32 = model.float()(input_ids=ids, attention_mask=mask)["last_hidden_state"]
        yard = {}
        for key, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
            low = model.to(dt)(input_ids=ids, attention_mask=mask)["last_hidden_state"].float()
            assert torch.isfinite(low).all(), key
            yard[key] = both(low, hf32)
            model.float()
    ref64 = t5_refs.encoder64(cfg, sd, ids, mask)[-1]
    emu = {key: both(t5_refs.encoder64(cfg, sd, ids, mask, round_to=dt)[-1], ref64) for key, dt in (("bf16", torch.bfloat16), ("f16", torch.float16))}
    rec = dict(what="the seeded fixture t5_wide of tests/t5_refs.py: rel-L2 figures of last_hidden_state, over all B L rows and over rows "
                    f"{tail.start} .. {tail.stop - 1} (tail_rows)",
               cfg=cfg, B=W["B"], L=W["L"], lens=W["lens"], seed=W["seed"], checksum=t5_refs.checksum(sd, ids),
               encoder64_vs_transformers_fp64=both(ref64, hf64), transformers_fp32_vs_fp64=both(hf32, hf64),
               yardstick=yard, emulation_vs_encoder64=emu)
    with open(os.path.join(out, "t5_wide.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print("t5_wide:", json.dumps({k: rec[k] for k in ("encoder64_vs_transformers_fp64", "transformers_fp32_vs_fp64", "yardstick", "emulation_vs_encoder64")}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    ap.add_argument("--only-wide", action="store_true", help="write t5_wide.json alone and leave the stored fixtures as they are")
    a = ap.parse_args()
    make_wide(a.out)
    if a.only_wide:
        return
    from transformers.models.t5.modeling_t5 import T5Attention
    noise = {name: make_fixture(name, spec, a.out) for name, spec in FIXTURES.items()}
    with open(os.path.join(a.out, "t5_ref_noise.json"), "w") as f:
        json.dump(dict(what="rel-L2 of transformers.T5EncoderModel in bf16 / fp16 against its own fp32 output, last_hidden_state over all rows", **noise), f, indent=1)
    off = torch.arange(-1023, 1024)
    torch.save({"offsets": off,
                "32_128": T5Attention._relative_position_bucket(off, True, 32, 128).to(torch.int16),
                "32_64": T5Attention._relative_position_bucket(off, True, 32, 64).to(torch.int16)}, os.path.join(a.out, "t5_buckets.pt"))


if __name__ == "__main__":
    main()
