#!/usr/bin/env python
"""A 16-bit (or fp32) transformers T5 directory in, an FP8 one out: the encoder's weight matrices as OCP e4m3fn bytes with one power-of-two fp32 scale per
output row (pixart_sigma_amd.t5.T5Encoder, csrc/gemm_w8.hip), half the bytes.

    python tools/quantize_t5.py --t5_path DIR --out DIR [--device cuda]

Writes config.json and model.safetensors (X.weight float8_e4m3fn, X.weight_scale fp32 (N,); embedding, norm weights and the bias table as they are); tokenizer
files of the source directory are copied beside them.  T5Encoder.from_pretrained(OUT) and every tool that takes --t5_path read the result as an FP8 encoder.
The quantiser is the HIP kernel pxa_fp8_quant_rows, matrix by matrix: the 16-bit model is never on the device as a whole.  The process runs under the bf16
operand build whatever the caller's environment says, as tools/extract_t5_features.py does."""
import argparse
import os
import shutil
import sys

os.environ["PXA_OPERAND_DTYPE"] = "bf16"
os.environ.pop("PXA_LIB_PATH", None)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TOKENIZER_FILES = ("spiece.model", "tokenizer.json", "tokenizer_config.json", "special_tokens_map.json", "added_tokens.json")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--t5_path", required=True, help="transformers T5 directory: config.json + safetensors / .bin weights")
    ap.add_argument("--out", required=True)
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    from pixart_sigma_amd.t5 import T5Encoder
    enc = T5Encoder.from_pretrained(args.t5_path, device=args.device, weight_dtype="fp8_e4m3")
    enc.save_pretrained(args.out)
    for f in TOKENIZER_FILES:
        if os.path.exists(os.path.join(args.t5_path, f)):
            shutil.copy(os.path.join(args.t5_path, f), os.path.join(args.out, f))
    print(f"wrote {args.out}: {enc.weight_bytes() / 1e9:.3f} GB of encoder buffers (matrices FP8 e4m3 + fp32 row scales)")


if __name__ == "__main__":
    main()
