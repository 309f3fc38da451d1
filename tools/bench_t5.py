#!/usr/bin/env python
"""Times the in-repo T5 encoder (pixart_sigma_amd.t5.T5Encoder) at the T5-v1.1-XXL geometry - 24 blocks, d_model 4096, 64 heads, d_ff 10240, vocab 32128 -
with random weights, under the bf16 operand build (the reference's T5 dtype).

    python tools/bench_t5.py [--shapes 1x300,16x120,64x120] [--iters 10] [--warmup 3] [--layers 24] [--weight_dtype fp8_e4m3 [--fp8_gemm auto|stream|dequant]]
    python tools/bench_t5.py --sweep_w8 [--sweep_m 16,64,120,300,600,1200,2048]

One JSON line per shape: ms per forward (events on the launch stream, after warm-up), the same pass's attention / norm / GEMM launches timed family by family
(each family alone, same arguments), algorithmic TFLOP/s and its fraction of the box's own pxa_mfma_rate_probe, weight bytes over time as a fraction of the
HBM3E sheet bandwidth (8 TB/s; at B = 1 the pass is weight-bound), and beside them transformers' own bf16 T5EncoderModel on torch when it is importable
("absent" otherwise).  All keys are valid (full-length captions): the attention time is its upper end.
--weight_dtype fp8_e4m3: the same encoder quantised to FP8 weights (T5Encoder.quantize_fp8) on the GEMM path --fp8_gemm; the line then also carries weight_dtype,
fp8_gemm, the path taken and the bytes of device memory the encoder holds.  Without the flag the line is what it was.
--sweep_w8: no forward; the five GEMM calls of a block at XXL widths, per row count M: pxa_gemm_w8 alone against pxa_fp8_dequant_rows + pxa_gemm and against
pxa_gemm on 16-bit weights, each over enough distinct weight copies that no call finds its weights in the 256 MB last-level cache.  One JSON line per (M, call)
and one per M with the sums: STREAM_MAX_M of t5/encoder.py is the largest M at which the stream sum wins."""
import argparse
import ctypes
import json
import os
import sys

os.environ["PXA_OPERAND_DTYPE"] = "bf16"
os.environ.pop("PXA_LIB_PATH", None)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def timed(fn, iters, warm):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def mfma_rate(seconds=1.0):
    """pxa_mfma_rate_probe (32 x 32 x 16, N(0,1) operands), rate over the second half of a back-to-back run."""
    from pixart_sigma_amd import lib as L_, ops
    lib = L_.load()
    buf = torch.randn(lib.pxa_mfma_rate_probe_bytes() // 2, device="cuda").to(ops.BF16)
    sink = torch.zeros(1, device="cuda")
    fl = ctypes.c_double(0.0)
    launch = lambda: L_.check(lib.pxa_mfma_rate_probe(L_.ptr(buf), 32, 4096, L_.ptr(sink), ctypes.byref(fl), L_.stream()), "pxa_mfma_rate_probe")  # noqa: E731
    k = max(4, int(seconds / 2 / timed(launch, 3, 1)))
    timed(launch, k, 0)
    return fl.value / timed(launch, k, 0)


def build_encoder(cfg):
    from pixart_sigma_amd.t5 import T5Encoder
    with torch.device("cuda"):
        m = T5Encoder(cfg)
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, b in m.named_buffers():
        if b.dim() == 2 and name != "rel_bias":
            for r in range(0, b.shape[0], 4096):                       # in slabs: no fp32 copy of a whole matrix
                blk = b[r:r + 4096]
                blk.copy_(torch.randn(blk.shape, device="cuda", generator=g) * (b.shape[1] ** -0.5 if name != "embed" else 1.0))
        else:
            b.copy_(1 + 0.2 * torch.randn(b.shape, device="cuda", generator=g) if b.dim() == 1 else 2 * torch.randn(b.shape, device="cuda", generator=g))
    return m


def families(m, B, L, iters, warm):
    """The launches of one forward, family by family, with the forward's own shapes."""
    from pixart_sigma_amd import ops
    c = m.config
    R, H, inner, n = B * L, c.num_heads, c.num_heads * c.d_kv, c.num_layers
    x = torch.randn(R, c.d_model, device="cuda")
    xn = torch.randn(R, c.d_model, device="cuda").to(ops.BF16)
    qkv = torch.randn(R, 3 * inner, device="cuda").to(ops.BF16)
    a = torch.randn(R, inner, device="cuda").to(ops.BF16)
    h0 = torch.randn(R, c.d_ff, device="cuda").to(ops.BF16)
    g = torch.empty_like(h0)
    bias, kv_len = m.position_bias(L), torch.full((B,), L, dtype=torch.int32, device="cuda")
    out16, res = torch.empty_like(xn), torch.zeros(R, c.d_model, device="cuda")

    def attn():
        for _ in range(n):
            ops.t5_attention(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], bias, kv_len, B, H, L, out=a)

    def norm():
        for _ in range(2 * n):
            ops.t5_rmsnorm(x, m.final_ln, out=out16)

    def gemm_fp8():
        mm = m._fp8_mm(R)
        for i in range(n):
            w = lambda k: getattr(m, f"b{i}_{k}")                                       # noqa: E731
            mm(xn, w("wqkv"), w("wqkv_scale"), out=qkv)
            mm(a, w("wo"), w("wo_scale"), out_f32=res)
            mm(xn, w("wi0"), w("wi0_scale"), act=ops.ACT_GELU, out=h0)
            mm(xn, w("wi1"), w("wi1_scale"), act=ops.ACT_MUL_AUX, aux=h0, out=g)
            mm(g, w("wff"), w("wff_scale"), out_f32=res)

    def gemm():
        if m.weight_dtype:
            return gemm_fp8()
        for i in range(n):
            w = lambda k: getattr(m, f"b{i}_{k}")                                       # noqa: E731
            ops.gemm(xn, w("wqkv"), ops.NT, out=qkv)
            ops.gemm(a, w("wo"), ops.NT, out_f32=res, accumulate=True)
            ops.gemm(xn, w("wi0"), ops.NT, act=ops.ACT_GELU, out=h0)
            ops.gemm(xn, w("wi1"), ops.NT, act=ops.ACT_MUL_AUX, aux=h0, out=g)
            ops.gemm(g, w("wff"), ops.NT, out_f32=res, accumulate=True)
    return {k: timed(f, iters, warm) * 1e3 for k, f in (("attention_ms", attn), ("norm_ms", norm), ("gemm_ms", gemm))}


_HF = {}


def transformers_ms(cfg, ids, iters, warm):
    try:
        from transformers import T5Config, T5EncoderModel
    except Exception:      # noqa: BLE001
        return "absent"
    if "model" in _HF:
        return _hf_time(_HF["model"], ids, iters, warm)
    hf = T5Config(feed_forward_proj="gated-gelu", dropout_rate=0.0, is_encoder_decoder=False, use_cache=False,
                  **{k: cfg[k] for k in ("vocab_size", "d_model", "d_kv", "d_ff", "num_layers", "num_heads")})
    with torch.device("cuda"):
        torch.set_default_dtype(torch.bfloat16)
        try:
            model = T5EncoderModel(hf).eval()
        finally:
            torch.set_default_dtype(torch.float32)
    _HF["model"] = model
    return _hf_time(model, ids, iters, warm)


def _hf_time(model, ids, iters, warm):
    dev_ids = ids.cuda()
    with torch.no_grad():
        return timed(lambda: model(input_ids=dev_ids)["last_hidden_state"], iters, warm) * 1e3


def hf_ms(cfg, ids, iters, warm):
    try:
        return transformers_ms(cfg, ids, iters, warm)
    except Exception as e:      # noqa: BLE001
        return f"failed: {type(e).__name__}: {str(e)[:120]}"


def sweep_w8(ms, iters, warm):
    """The five calls of an XXL block, stream against dequant + pxa_gemm against 16-bit pxa_gemm, per M."""
    from pixart_sigma_amd import ops
    D, inner, dff = 4096, 4096, 10240
    calls = [("wqkv", 3 * inner, D, {}), ("wo", D, inner, {"f32": True}), ("wi0", dff, D, {"act": ops.ACT_GELU}), ("wi1", dff, D, {"act": ops.ACT_MUL_AUX}),
             ("wff", D, dff, {"f32": True})]
    g = torch.Generator(device="cuda").manual_seed(0)
    scratch = torch.empty(3 * inner * D, dtype=ops.BF16, device="cuda")
    for name, N, K, kind in calls:
        copies = max(2, -(-600_000_000 // (N * K)))
        w16 = [(torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(ops.BF16) for _ in range(copies)]
        wq = [ops.fp8_quant_rows(w) for w in w16]
        for M in ms:
            a = torch.randn(M, K, device="cuda", generator=g).to(ops.BF16)
            aux = torch.randn(M, N, device="cuda", generator=g).to(ops.BF16) if kind.get("act") == ops.ACT_MUL_AUX else None
            res = torch.zeros(M, N, device="cuda") if kind.get("f32") else None
            out = None if kind.get("f32") else torch.empty(M, N, dtype=ops.BF16, device="cuda")
            kw8 = dict(out_f32=res) if res is not None else dict(act=kind.get("act", ops.ACT_NONE), aux=aux, out=out)
            kw16 = dict(out_f32=res, accumulate=True) if res is not None else dict(act=kind.get("act", ops.ACT_NONE), aux=aux, out=out)
            state = {"i": 0}

            def nxt():
                state["i"] = (state["i"] + 1) % copies
                return state["i"]

            def stream():
                q, sc = wq[nxt()]
                ops.gemm_w8(a, q, sc, **kw8)

            def dequant():
                q, sc = wq[nxt()]
                ops.gemm(a, ops.fp8_dequant_rows(q, sc, out=scratch[:N * K].view(N, K)), ops.NT, **kw16)

            def plain():
                ops.gemm(a, w16[nxt()], ops.NT, **kw16)
            t = {k: timed(f, iters, warm) * 1e6 for k, f in (("stream_us", stream), ("dequant_gemm_us", dequant), ("gemm16_us", plain))}
            yield dict(tool="bench_t5", sweep="w8", call=name, M=M, N=N, K=K, **t, stream_tbytes_per_s=N * K / t["stream_us"] / 1e6,
                       stream_tflops=2.0 * M * N * K / t["stream_us"] / 1e6, plan=ops.gemm_w8_plan(a, *wq[0], **kw8).split()[0])
        del w16, wq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x300,16x120,64x120")
    ap.add_argument("--iters", default=10, type=int)
    ap.add_argument("--warmup", default=3, type=int)
    ap.add_argument("--layers", default=24, type=int)
    ap.add_argument("--no_transformers", action="store_true")
    ap.add_argument("--weight_dtype", default=None, choices=["fp8_e4m3"])
    ap.add_argument("--fp8_gemm", default="auto", choices=["auto", "stream", "dequant"])
    ap.add_argument("--sweep_w8", action="store_true")
    ap.add_argument("--sweep_m", default="16,64,120,300,600,1200,2048")
    args = ap.parse_args()
    from pixart_sigma_amd import lib
    if args.sweep_w8:
        sums = {}
        for r in sweep_w8([int(v) for v in args.sweep_m.split(",")], args.iters, args.warmup):
            print(json.dumps(r), flush=True)
            s_ = sums.setdefault(r["M"], dict(stream_us=0.0, dequant_gemm_us=0.0, gemm16_us=0.0))
            for k in s_:
                s_[k] += r[k]
        for M, s_ in sorted(sums.items()):
            print(json.dumps(dict(tool="bench_t5", sweep="w8", call="block_sum", M=M, **s_, stream_wins=s_["stream_us"] < s_["dequant_gemm_us"])), flush=True)
        return
    cfg = dict(vocab_size=32128, d_model=4096, d_kv=64, d_ff=10240, num_layers=args.layers, num_heads=64)
    m = build_encoder(cfg)
    if args.weight_dtype:
        m.quantize_fp8().set_fp8_gemm(args.fp8_gemm)
        torch.cuda.empty_cache()
    weight_bytes = sum(b.numel() * b.element_size() for n, b in m.named_buffers() if n != "embed")
    probe = mfma_rate()
    inner = cfg["num_heads"] * cfg["d_kv"]
    for shape in args.shapes.split(","):
        B, L = (int(v) for v in shape.split("x"))
        ids = torch.randint(2, cfg["vocab_size"], (B, L), generator=torch.Generator().manual_seed(1))
        mask = torch.ones(B, L, dtype=torch.long)
        with torch.no_grad():
            t = timed(lambda: m(ids, mask), args.iters, args.warmup)
        flops = cfg["num_layers"] * (2.0 * B * L * cfg["d_model"] * (4 * inner + 3 * cfg["d_ff"]) + 4.0 * B * cfg["num_heads"] * L * L * cfg["d_kv"])
        res = dict(tool="bench_t5", operand=lib.OPERAND, B=B, L=L, layers=cfg["num_layers"], ms_per_forward=t * 1e3, **families(m, B, L, args.iters, args.warmup),
                   algorithmic_tflops=flops / t / 1e12, mfma_probe_tflops=probe / 1e12, fraction_of_mfma_probe=flops / t / probe,
                   weight_gbytes=weight_bytes / 1e9, weight_bytes_per_s_over_hbm=weight_bytes / t / HBM_BYTES_PER_S,
                   transformers_bf16_ms="not run" if args.no_transformers else hf_ms(cfg, ids, args.iters, args.warmup))
        if args.weight_dtype:
            res.update(weight_dtype=args.weight_dtype, fp8_gemm=args.fp8_gemm, fp8_gemm_path=m.fp8_gemm_path(B * L), encoder_device_gbytes=m.weight_bytes() / 1e9)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
