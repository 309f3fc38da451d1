"""Training from pictures against training from feature files, in one process on one GPU: PixArt-Sigma-XL/2 at 1024px, batch 16, L = 300, random weights
everywhere (denoiser, SDXL-VAE geometry, T5), generated pictures.  Prints one JSON line:

    step time from feature files (FeatureDatasetMS through train.py's feature_batches) - the comparison base of the run;
    step time from pictures with caption feature files, and from pictures with text captions (PictureBatches one batch ahead of the step);
    the split of one picture batch, each phase synchronised: decode wait, transform, VAE encode, the posterior kernel alone, T5 (caption round trip), and
    the denoiser step; under --dtype fp16 the caption worker's round trip alone (submit + collect of one batch with nothing else on the GPU).

    python tools/bench_train_pictures.py [--steps 5] [--warmup 2] [--dtype fp16|bf16] [--pictures 32] [--t5-layers 24] [--no-text]

The data set is written to a temporary directory first: --pictures PNGs of about 1024 x 1024 (two buckets), their data_info.json, caption feature files, VAE
feature files and a T5 directory of --t5-layers random blocks at T5-XXL's widths (24 blocks are 9.4 GB of weights; fewer shorten the text rows only) with
a sentencepiece tokenizer trained on the generated captions.  Nothing is asserted about the numbers."""
import argparse
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "train_scripts"))
LTXT = 300
RATIOS = {"0.88": [960, 1088], "1.0": [1024, 1024]}
WORDS = "a red blue green small large cube sphere house tree dog cat on under over beside table field river sky with many bright dark old new".split()


def make_data(top, n, t5_layers, text):
    import numpy as np
    import torch
    from PIL import Image
    root, imgs = os.path.join(top, "InternData"), os.path.join(top, "InternImgs", "pics")
    for d in (imgs, os.path.join(root, "caption_features_new"), os.path.join(root, "img_sdxl_vae_features_1024resolution_ms_new")):
        os.makedirs(d)
    rng, meta = np.random.default_rng(0), []
    g = torch.Generator().manual_seed(0)
    for i in range(n):
        h, w = ((1100, 1100), (1000, 1150))[i % 2]
        low = rng.integers(0, 256, size=(h // 8, w // 8, 3), dtype=np.uint8)                       # blocks of 8 x 8: a PNG that decodes at a photograph's cost
        Image.fromarray(np.kron(low, np.ones((8, 8, 1), dtype=np.uint8))).save(os.path.join(imgs, f"p{i:03d}.png"), compress_level=1)
        cap = lambda k: " ".join(WORDS[j] for j in rng.integers(0, len(WORDS), size=k))            # noqa: E731
        meta.append({"path": f"pics/p{i:03d}.png", "height": h, "width": w, "ratio": h / w, "prompt": cap(12), "sharegpt4v": cap(60)})
        H, W = RATIOS["1.0" if i % 2 == 0 else "0.88"]
        np.savez(os.path.join(root, "caption_features_new", f"pics_p{i:03d}.npz"), caption_feature=torch.randn(1, 120, 4096, generator=g).to(torch.float16).numpy(),
                 attention_mask=np.ones((1, 120), dtype=np.int64))
        np.save(os.path.join(root, "img_sdxl_vae_features_1024resolution_ms_new", f"pics_p{i:03d}.npy"),
                torch.cat([torch.randn(4, H // 8, W // 8, generator=g), torch.rand(4, H // 8, W // 8, generator=g) * 0.1]).to(torch.float16).numpy())
    with open(os.path.join(root, "data_info.json"), "w") as f:
        json.dump(meta, f)
    t5 = None
    if text:
        import sentencepiece as spm
        from safetensors.torch import save_file
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import t5_refs
        t5 = os.path.join(top, "t5")
        os.makedirs(t5)
        model = io.BytesIO()
        spm.SentencePieceTrainer.train(sentence_iterator=iter([m["prompt"] for m in meta] + [m["sharegpt4v"] for m in meta]), model_writer=model, vocab_size=48,
                                       model_type="unigram", pad_id=0, eos_id=1, unk_id=2, bos_id=-1, hard_vocab_limit=False)
        with open(os.path.join(t5, "spiece.model"), "wb") as f:
            f.write(model.getvalue())
        with open(os.path.join(t5, "tokenizer_config.json"), "w") as f:
            json.dump({"tokenizer_class": "T5Tokenizer", "extra_ids": 0, "model_max_length": LTXT}, f)
        cfg = dict(d_model=4096, num_heads=64, d_ff=10240, num_layers=t5_layers, vocab_size=64)
        with open(os.path.join(t5, "config.json"), "w") as f:
            json.dump(dict(t5_refs.full_config(cfg), model_type="t5"), f)
        save_file({k: v.clone() for k, v in t5_refs.state_dict(cfg, 1).items() if k != "encoder.embed_tokens.weight"}, os.path.join(t5, "model.safetensors"))
    return root, t5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--pictures", type=int, default=32)
    ap.add_argument("--t5-layers", type=int, default=24)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="fp16")
    ap.add_argument("--no-text", action="store_true")
    a = ap.parse_args()
    if a.dtype == "fp16":
        os.environ["PXA_OPERAND_DTYPE"] = "f16"
    import torch
    import train as T
    from pixart_sigma_amd import IDDPM, PixArtMS_XL_2, ops
    from pixart_sigma_amd.data import PictureBatches, PictureCaptionDatasetMS
    from pixart_sigma_amd.dp import FusedAdamW, LossScaler
    from pixart_sigma_amd.vae import AutoencoderKL
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, out = a.batch, {"workload": f"PixArt-Sigma-XL/2 1024px bs{a.batch} L{LTXT}", "dtype": a.dtype, "steps": a.steps, "warmup": a.warmup, "pictures": a.pictures,
                       "decode_threads": min(a.workers, 8), "t5_layers": None if a.no_text else a.t5_layers}
    with tempfile.TemporaryDirectory() as top:
        root, t5 = make_data(top, a.pictures, a.t5_layers, not a.no_text)
        torch.manual_seed(0)
        model = PixArtMS_XL_2(input_size=128, pe_interpolation=2.0, model_max_length=LTXT, class_dropout_prob=0.1)
        with torch.no_grad():                                 # as bench.py: no numerically dead branch
            for blk in model.blocks:
                blk.cross_attn.proj.weight.normal_(std=0.02)
            model.final_layer.linear.weight.normal_(std=0.02)
        model = model.to(dev).train()
        model.prepare(dev)
        diff = IDDPM(str(1000), learn_sigma=True, pred_sigma=True, snr=False)
        scaler = LossScaler(dev) if a.dtype == "fp16" else None
        opt = FusedAdamW(model, lr=2e-5, weight_decay=3e-2, eps=1e-10, max_grad_norm=0.01, scaler=scaler)
        vae = AutoencoderKL(scaling_factor=0.13025).to(dev)

        def step(batch):
            x0, y, mask, info = batch
            opt.zero_grad()
            t = torch.randint(0, 1000, (x0.shape[0],), device=dev).long()
            loss = diff.training_losses(model, x0, t, model_kwargs=dict(y=y, mask=mask, data_info=info))["loss"].mean()
            (scaler.scale(loss) if scaler is not None else loss).backward()
            opt.step()
            return loss

        def timed(it, label):
            for _ in range(a.warmup):
                step(next(it))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = step(next(it))
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / a.steps
            out[label] = {"ms_per_step": dt * 1e3, "steps_per_s": 1 / dt, "final_loss": float(loss.item())}

        cfg = dict(T.DEFAULTS, data_root=root, aspect_ratio_type=RATIOS, image_size=1024, seed=0)
        feats = ((z * 0.13025, y, m, i) for z, y, m, i in T.feature_batches(cfg, B, LTXT, dev, 0, 1))
        timed(feats, "from_feature_files")
        base = out["from_feature_files"]["ms_per_step"]

        def pictures(captions, profile=False):
            ds = PictureCaptionDatasetMS(root, RATIOS, resolution=1024, real_prompt_ratio=1.0 if captions is None else 0.5, max_length=LTXT, load_t5_feat=captions is None)
            return PictureBatches(ds, B, RATIOS, vae, captions, seed=0, device=dev, num_workers=a.workers, scale=0.13025, profile=profile)
        timed(iter(pictures(None)), "from_pictures_and_caption_files")
        out["from_pictures_and_caption_files"]["over_feature_files"] = out["from_pictures_and_caption_files"]["ms_per_step"] / base
        # the split of one picture batch, every phase synchronised (so the phases add up to more than a pipelined step)
        pb = pictures(None, profile=True)
        it = iter(pb)
        split = {}
        for _ in range(3):
            batch = next(it)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(batch)
            torch.cuda.synchronize()
            split = dict(pb.timing, denoiser_step=time.perf_counter() - t0)
        it.close()
        h = vae._conv1                                          # the posterior kernel alone, on moments of the batch's shape
        H, W = pb.pictures.shape[2] // 8, pb.pictures.shape[3] // 8
        ip = ((H + 2) * (W + 2) + 255) // 256 * 256
        mom, eps = torch.randn(B * ip, 8, device=dev), torch.randn(B, 4, H, W, device=dev)
        for _ in range(3):
            ops.vae_posterior(mom, B, H, W, 4, eps=eps, scale=0.13025)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            ops.vae_posterior(mom, B, H, W, 4, eps=eps, scale=0.13025)
        e1.record()
        e1.synchronize()
        split["posterior_kernel"] = e0.elapsed_time(e1) / 20 * 1e-3
        del h
        out["split_ms"] = {k: v * 1e3 for k, v in split.items()}
        if not a.no_text:
            from transformers import AutoTokenizer
            from pixart_sigma_amd.t5.captions import CaptionEncoder
            with CaptionEncoder(t5, AutoTokenizer.from_pretrained(t5), model_max_length=LTXT, device=dev, max_batch=B) as ce:
                texts = [m["prompt"] for m in json.load(open(os.path.join(root, "data_info.json")))][:B]
                rt = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ce.encode(texts)
                    torch.cuda.synchronize()
                    rt.append(time.perf_counter() - t0)
                out["caption_encode_alone_ms"] = {"path": "in process" if ce.in_process else "worker round trip", "ms": min(rt) * 1e3}
                out["split_ms"]["t5"] = min(rt) * 1e3
                timed(iter(pictures(ce)), "from_pictures_and_text")
                out["from_pictures_and_text"]["over_feature_files"] = out["from_pictures_and_text"]["ms_per_step"] / base
        opt.reducer.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
