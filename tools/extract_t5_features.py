#!/usr/bin/env python
"""Caption features from the in-repo T5 encoder (pixart_sigma_amd.t5), in the format scripts/inference.py --caption_feats reads: <idx>.npz per prompt with
`caption_feature` (1, L, d_model) fp32 and `attention_mask` (1, L) int64, plus null.npz for the empty prompt (the reference's tools/extract_features.py and
the null caption of its scripts/inference.py).

    python tools/extract_t5_features.py --t5_path DIR --out DIR (--prompts FILE | --ids FILE) [--max_length 300] [--weight_dtype fp8_e4m3]

--prompts: one caption per line, tokenised with the tokenizer in --t5_path (needs `transformers` and the directory's spiece.model).
--ids:     a torch file with `input_ids` and `attention_mask` (N, L), optionally `null_input_ids` / `null_attention_mask` (1, L) - no tokenizer needed.
           Without the null entries the empty prompt is T5's: the end-of-sequence token (id 1) alone, padded with id 0.
--weight_dtype fp8_e4m3: quantise a 16-bit checkpoint to FP8 weights while loading (an FP8 directory, e.g. from tools/quantize_t5.py, is FP8 without it).
The process runs under the bf16 operand build whatever the caller's environment says: the reference runs T5 in bf16 and real XXL weights overflow fp16."""
import argparse
import os
import sys

os.environ["PXA_OPERAND_DTYPE"] = "bf16"
os.environ.pop("PXA_LIB_PATH", None)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def write_features(out_dir, feats, masks, null_feat, null_mask):
    """feats (N, L, D) fp32, masks (N, L); null_feat (1, L, D), null_mask (1, L) -> <idx>.npz and null.npz under out_dir.  Returns the file names."""
    os.makedirs(out_dir, exist_ok=True)
    feats, masks = torch.as_tensor(feats).detach().float().cpu(), torch.as_tensor(masks).detach().cpu().to(torch.int64)
    assert feats.dim() == 3 and tuple(masks.shape) == tuple(feats.shape[:2])
    names = []
    for i in range(feats.shape[0]):
        names.append(f"{i}.npz")
        np.savez(os.path.join(out_dir, names[-1]), caption_feature=feats[i:i + 1].numpy(), attention_mask=masks[i:i + 1].numpy())
    names.append("null.npz")
    np.savez(os.path.join(out_dir, "null.npz"), caption_feature=torch.as_tensor(null_feat).detach().float().cpu().reshape(1, *feats.shape[1:]).numpy(),
             attention_mask=torch.as_tensor(null_mask).detach().cpu().to(torch.int64).reshape(1, -1).numpy())
    return names


def tokenise(args):
    """(ids, mask, null_ids, null_mask) from --prompts or --ids."""
    L = args.max_length
    if args.ids:
        d = torch.load(args.ids, map_location="cpu", weights_only=True)
        ids, mask = d["input_ids"][:, :L], d["attention_mask"][:, :L]
        if "null_input_ids" in d:
            return ids, mask, d["null_input_ids"][:, :L], d["null_attention_mask"][:, :L]
        null_ids, null_mask = torch.zeros(1, ids.shape[1], dtype=torch.long), torch.zeros(1, ids.shape[1], dtype=torch.long)
        null_ids[0, 0], null_mask[0, 0] = 1, 1
        return ids, mask, null_ids, null_mask
    from transformers import AutoTokenizer
    tok = AutoTokenizer.from_pretrained(args.tokenizer_path or args.t5_path)
    texts = [ln.strip() for ln in open(args.prompts)]
    kw = dict(max_length=L, padding="max_length", truncation=True, return_attention_mask=True, add_special_tokens=True, return_tensors="pt")
    t, n = tok(texts, **kw), tok([""], **kw)
    return t["input_ids"], t["attention_mask"], n["input_ids"], n["attention_mask"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--t5_path", required=True, help="transformers T5 directory: config.json + safetensors / .bin weights (+ the tokenizer files for --prompts)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--prompts", default=None)
    ap.add_argument("--ids", default=None)
    ap.add_argument("--tokenizer_path", default=None)
    ap.add_argument("--max_length", default=300, type=int)
    ap.add_argument("--batch", default=8, type=int)
    ap.add_argument("--weight_dtype", default=None, choices=["fp8_e4m3"], help="hold the encoder's matrices as FP8 e4m3 (default: as stored in --t5_path)")
    args = ap.parse_args()
    if bool(args.prompts) == bool(args.ids):
        ap.error("give exactly one of --prompts and --ids")
    from pixart_sigma_amd.t5 import T5Encoder
    ids, mask, null_ids, null_mask = tokenise(args)
    enc = T5Encoder.from_pretrained(args.t5_path, device="cuda", weight_dtype=args.weight_dtype)
    feats = torch.cat([enc(ids[i:i + args.batch], mask[i:i + args.batch]).cpu() for i in range(0, ids.shape[0], args.batch)])
    names = write_features(args.out, feats, mask, enc(null_ids, null_mask).cpu(), null_mask)
    print(f"wrote {len(names)} files to {args.out}: caption_feature {tuple(feats.shape[1:])} per prompt")


if __name__ == "__main__":
    main()
