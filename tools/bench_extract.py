#!/usr/bin/env python
"""What bounds tools/extract_features.py?  Prints one JSON line.

JPEGs are generated in memory by Pillow at run time (2048 x 1536 and 4000 x 3000, half each), the transform is the 1024-pixel multi-scale `stretch` form
(bicubic, bucket 896 x 1152), decoding runs on 8 threads, the VAE is the full architecture with random weights.  Images per second of
    pillow_transform   decode + Pillow resize + ToTensor + Normalize on the threads, fp32 upload         (the reference's DataLoader work)
    hip_transform      decode on the threads, uint8 upload + pxa_image_resample                           (this repository's path)
    vae_encode         vae.encode alone at the tool's batch
    tool_hip / tool_pillow   the whole tool on files, --transform hip / pillow
and the two resampling kernels' device times alone (events around repeated launches on device-resident sources) as bytes moved over time, beside the device
copy rate DESIGN.md quotes for the row passes (6.29 TB/s)."""
import argparse
import importlib.util
import io
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

COPY_RATE_GBS = 6290.0
TARGET = (896, 1152)


def make_jpegs(n):
    from PIL import Image
    rng = np.random.default_rng(0)
    out = []
    for i in range(n):
        w, h = ((2048, 1536), (4000, 3000))[i % 2]
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        img = np.stack([127 + 120 * np.sin(xx / (37 + i)) * np.cos(yy / 53), 127 + 120 * np.sin((xx + yy) / (71 + i)), 255 * xx / w], axis=-1)
        img = np.clip(img + rng.normal(0, 6, size=img.shape), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="JPEG", quality=90)
        out.append((buf.getvalue(), h, w))
    return out


def decode(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return im.convert("RGB")


def device_time_ms(fn, iters=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def kernel_times(ops, images, h, w):
    """The horizontal and the vertical kernel alone on an (h, w) source -> TARGET, bicubic: ms and bytes moved / time."""
    H, W = TARGET
    src = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda")
    hk, hb = images.resample_tables(w, W, "bicubic")
    vk, vb = images.resample_tables(h, H, "bicubic")
    htab = (torch.from_numpy(np.ascontiguousarray(hk.T)).cuda(), torch.from_numpy(hb).cuda())
    vtab = (torch.from_numpy(vk).cuda(), torch.from_numpy(vb).cuda())
    mid = torch.empty((h, W, 3), dtype=torch.uint8, device="cuda")
    out = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
    lut = images.normalize_lut().cuda()
    t_h = device_time_ms(lambda: ops.image_resample(src, (h, W), (0, 0, h, W), mid, htab=htab))
    t_v = device_time_ms(lambda: ops.image_resample(mid, (H, W), (0, 0, H, W), out, vtab=vtab, rows=(0, h), lut=lut))
    b_h, b_v = 3 * h * w + 3 * h * W, 3 * h * W + 12 * H * W
    return {"source": f"{h}x{w}", "hpass_ms": round(t_h, 4), "hpass_gbs": round(b_h / t_h / 1e6, 1), "vpass_ms": round(t_v, 4), "vpass_gbs": round(b_v / t_v / 1e6, 1),
            "hpass_of_copy_rate": round(b_h / t_h / 1e6 / COPY_RATE_GBS, 3), "vpass_of_copy_rate": round(b_v / t_v / 1e6 / COPY_RATE_GBS, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", default=16, type=int)
    ap.add_argument("--threads", default=8, type=int)
    ap.add_argument("--batch", default=4, type=int)
    ap.add_argument("--repeats", default=2, type=int)
    a = ap.parse_args()
    from pixart_sigma_amd import ops
    from pixart_sigma_amd.data import images
    from pixart_sigma_amd.vae import AutoencoderKL
    spec = importlib.util.spec_from_file_location("extract_features_tool", os.path.join(ROOT, "tools", "extract_features.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    jpegs = make_jpegs(a.images)
    res = {"images": a.images, "threads": a.threads, "batch": a.batch, "target": list(TARGET), "filter": "bicubic", "copy_rate_gbs": COPY_RATE_GBS}

    def best(fn):
        ts = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return a.images / min(ts)

    with ThreadPoolExecutor(max_workers=a.threads) as pool:
        def decode_only():
            list(pool.map(lambda j: decode(j[0]), jpegs))

        def pillow_path():
            for t in pool.map(lambda j: images.pillow_transform(decode(j[0]), "stretch", "bicubic", TARGET), jpegs):
                t.cuda()
        pre = images.ImagePreprocessor("stretch", "bicubic", "cuda")
        side = torch.cuda.Stream("cuda")
        batch = torch.empty((1, 3, *TARGET), dtype=torch.float32, device="cuda")

        def hip_path():
            for im in pool.map(lambda j: images.to_device_u8(decode(j[0]), "cuda", stream=side), jpegs):      # as the tool: RGB + uint8 upload on the decoding thread
                pre(im, TARGET, out=batch)
        hip_path()                                                        # tables, workspace, first launches
        res["decode_only_img_s"] = round(best(decode_only), 2)
        res["pillow_transform_img_s"] = round(best(pillow_path), 2)
        res["hip_transform_img_s"] = round(best(hip_path), 2)
    torch.manual_seed(0)
    vae = AutoencoderKL().cuda()
    x = torch.randn(a.batch, 3, *TARGET, device="cuda").clamp(-1, 1)
    vae.encode(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        vae.encode(x)
    torch.cuda.synchronize()
    res["vae_encode_img_s"] = round(3 * a.batch / (time.perf_counter() - t0), 2)

    def encode(t):
        d = vae.encode(t).latent_dist
        return d.mean, d.std
    with tempfile.TemporaryDirectory() as root:
        meta = []
        for i, (data, h, w) in enumerate(jpegs):
            with open(os.path.join(root, f"{i}.jpg"), "wb") as f:
                f.write(data)
            meta.append({"path": f"{i}.jpg", "height": h, "width": w, "ratio": h / w, "prompt": ""})
        json.dump(meta, open(os.path.join(root, "data_info.json"), "w"))
        json.dump({"0.78": list(TARGET)}, open(os.path.join(root, "ratios.json"), "w"))
        for mode in ("warm_hip", "warm_pillow", "hip", "pillow", "hip2", "pillow2"):      # a warm-up run each (tables, the encoder's buffers at this shape), then twice each
            args = tool.get_args(["--run_vae_feature_extract", "--multi_scale", "--img_size", "1024", "--aspect_ratios", os.path.join(root, "ratios.json"), "--dataset_root", root,
                                  "--vae_save_root", os.path.join(root, mode), "--batch", str(a.batch), "--workers", str(a.threads), "--transform", "hip" if "hip" in mode else "pillow"] +
                                 (["--end_index", str(a.batch)] if mode.startswith("warm") else []))
            t0 = time.perf_counter()
            n = len(tool.extract_vae(args, encode=encode))
            torch.cuda.synchronize()
            if not mode.startswith("warm"):
                key = f"tool_{mode.rstrip('2')}_img_s"
                res[key] = max(res.get(key, 0.0), round(n / (time.perf_counter() - t0), 2))
    res["kernels"] = [kernel_times(ops, images, 1536, 2048), kernel_times(ops, images, 3000, 4000)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
