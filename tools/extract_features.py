#!/usr/bin/env python
"""Image files to the features the trainers read (pixart_sigma_amd.data.FeatureDatasetMS), with the reference's flags (tools/extract_features.py):

    python tools/extract_features.py --make_json DIR
    python tools/extract_features.py --run_vae_feature_extract --multi_scale --img_size 1024 --aspect_ratios RATIOS.json \\
        --dataset_root DIR --vae_json_file data_info.json --vae_models_dir VAE_DIR --vae_save_root DIR
    python tools/extract_features.py --run_t5_feature_extract --t5_json_path DIR/data_info.json --t5_models_dir T5_DIR --t5_save_root DIR

--make_json DIR            writes DIR/data_info.json ({path, height, width, ratio, prompt} per image) from the pictures under DIR that have a `<name>.txt` caption.
--run_vae_feature_extract  decodes the pictures on a small thread pool (--workers, default 8, at most 16), applies the reference's resize / crop / normalise, sends
                           batches grouped by bucket through the HIP VAE's encode and np.saves cat[mean, std] (8, h / 8, w / 8) float16 as
                           <vae_save_root>/img_sdxl_vae_features_<res>resolution_ms_new/<dir>_<name>.npy (single scale: ..._<res>resolution_new/).  Files that
                           exist are skipped.  --multi_scale: T.Resize([H, W]) to the closest bucket of --aspect_ratios (a JSON file {ratio: [H, W]}: the bucket
                           table is an input, as in train_scripts/train.py), BICUBIC; single scale: T.Resize(n) + CenterCrop(n), BILINEAR; LANCZOS for both at
                           2048 / 2880.  --transform hip: the threads only decode and upload uint8, the transform runs on the GPU (pixart_sigma_amd.data.images:
                           Pillow's bytes, bit for bit, a quarter of the upload); --transform pillow (default): Pillow on the threads, fp32 upload.  Same files
                           either way; which is faster end to end is measured by tools/bench_extract.py.
--run_t5_feature_extract   glue: the prompts of the JSON go to the in-repo T5 encoder (tools/extract_t5_features.py in a child process under the bf16 build), and its
                           <idx>.npz become <t5_save_root>/caption_features_new/<dir>_<name>.npz."""
import argparse
import collections
import json
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMG_EXT = (".png", ".jpg", ".jpeg", ".webp", ".JPEG", ".JPG")
MAX_WORKERS = 16


def feature_name(path):
    """`<dir>_<name>` of an image path, exactly as FeatureDatasetMS builds its file names."""
    from pixart_sigma_amd.data.features import replace_img_ext
    return replace_img_ext("_".join(path.rsplit("/", 1)), "")


def filter_for(img_size, multi_scale):
    """The reference's interpolation table: tools/extract_features.py:57-62 (multi-scale) and 216-218 (single scale)."""
    if img_size in (2048, 2880):
        return "lanczos"
    return "bicubic" if multi_scale else "bilinear"


def vae_save_dir(args):
    d = os.path.join(args.vae_save_root, f"img_sdxl_vae_features_{args.img_size}resolution_{'ms_new' if args.multi_scale else 'new'}")
    return d if args.save_path_suffix is None else f"{d}_{args.save_path_suffix}"


def make_json(root):
    """data_info.json of the pictures under `root` that come with a `<name>.txt` caption; paths relative to `root`."""
    from PIL import Image
    items = []
    for d, _, files in sorted(os.walk(root)):
        for f in sorted(files):
            stem, ext = os.path.splitext(f)
            txt = os.path.join(d, stem + ".txt")
            if ext not in IMG_EXT or not os.path.exists(txt):
                continue
            with Image.open(os.path.join(d, f)) as im:
                w, h = im.size
            with open(txt) as t:
                prompt = " ".join(t.read().split())
            items.append({"path": os.path.relpath(os.path.join(d, f), root).replace(os.sep, "/"), "height": h, "width": w, "ratio": h / w, "prompt": prompt})
    out = os.path.join(root, "data_info.json")
    with open(out, "w") as f:
        json.dump(items, f, indent=1)
    return out, len(items)


def _load_image(path):
    from PIL import Image
    with Image.open(path) as im:
        return im.convert("RGB")


def plan_vae(args, meta, ratios):
    """[(target, [(image path, output path), ...]), ...]: the images still to do, grouped by what they are resized to.  target = (H, W) of the closest bucket
    (--multi_scale) or n.  Items with ratio > 4.5 are dropped, as in the reference (and in FeatureDatasetMS)."""
    from pixart_sigma_amd.data.sampler import closest_ratio
    save = vae_save_dir(args)
    groups = collections.OrderedDict()
    keep = [it for it in meta if it["ratio"] <= 4.5][args.start_index:args.end_index]
    for it in keep:
        out = os.path.join(save, feature_name(it["path"]) + ".npy")
        if os.path.exists(out):
            continue
        target = tuple(int(v) for v in closest_ratio(it["height"], it["width"], ratios)[1]) if args.multi_scale else int(args.img_size)
        groups.setdefault(target, []).append((os.path.join(args.dataset_root, it["path"]), out))
    return list(groups.items())


def extract_vae(args, encode=None, load=_load_image, transform=None, device="cuda"):
    """--run_vae_feature_extract.  encode: fp32 (B, 3, H, W) batch -> (mean, std); load: path -> image; transform: (image, target, batch, slot) fills batch[slot].
    The defaults are the HIP VAE, Pillow's decoder and the GPU transform; the parameters exist for --transform pillow and for tests without a GPU.
    Returns the files written."""
    import numpy as np
    import torch
    from pixart_sigma_amd.data import images
    with open(os.path.join(args.dataset_root, args.vae_json_file)) as f:
        meta = json.load(f)
    ratios = None
    if args.multi_scale:
        if not args.aspect_ratios:
            raise SystemExit("--multi_scale needs --aspect_ratios FILE.json: the bucket table {ratio: [H, W]}")
        with open(args.aspect_ratios) as f:
            ratios = json.load(f)
    form, filt = ("stretch" if args.multi_scale else "short_side"), filter_for(args.img_size, args.multi_scale)
    prepare = load                                                                # what a pool thread does with a path
    if transform is None:
        if args.transform == "hip":
            pre = images.ImagePreprocessor(form, filt, device)

            side = torch.cuda.Stream(device)                                     # uploads do not queue behind the encoder's kernels

            def prepare(path, target):                                            # decode, RGB and the uint8 upload on the pool thread: the main thread only launches
                return images.to_device_u8(load(path), device, stream=side)

            def transform(img, target, batch, slot):
                pre(img, target, out=batch, slot=slot)
        else:                                                                     # Pillow's transform on the pool threads, as the reference's DataLoader workers do it
            def prepare(path, target):
                return images.pillow_transform(load(path), form, filt, target)

            def transform(img, target, batch, slot):
                batch[slot].copy_(img, non_blocking=True)
    if encode is None:
        from pixart_sigma_amd.vae import AutoencoderKL
        vae = AutoencoderKL.from_pretrained(args.vae_models_dir).to(device)

        def encode(x):
            d = vae.encode(x).latent_dist
            return d.mean, d.std
    os.makedirs(vae_save_dir(args), exist_ok=True)
    workers = max(1, min(int(args.workers), MAX_WORKERS))
    written = []
    with ThreadPoolExecutor(max_workers=workers) as pool:
        for target, items in plan_vae(args, meta, ratios):
            H, W = (target, target) if isinstance(target, int) else target
            pending = collections.deque()                                         # in flight ahead of the GPU: two per thread (a 12-megapixel JPEG takes a thread
            ahead = max(2 * args.batch, 2 * workers)                              # ~0.1 s, its Pillow transform 0.4 s: fewer in flight leaves threads idle)
            it = iter(items)

            def refill():
                while len(pending) < ahead:
                    nxt = next(it, None)
                    if nxt is None:
                        return
                    pending.append((pool.submit(prepare, nxt[0], *((target,) if prepare is not load else ())), nxt[1]))
            refill()
            while pending:
                n = min(args.batch, len(pending))
                batch = torch.empty((n, 3, H, W), dtype=torch.float32, device=device)
                outs = []
                for slot in range(n):
                    fut, out = pending.popleft()
                    transform(fut.result(), target, batch, slot)
                    outs.append(out)
                    refill()
                mean, std = encode(batch)
                res = torch.cat([mean, std], dim=1).detach().to(torch.float16).cpu().numpy()
                for r, out in zip(res, outs):
                    np.save(out, r)
                    written.append(out)
    return written


def t5_child_command(args, prompts_file, out_dir):
    tool = os.path.join(ROOT, "tools", "extract_t5_features.py")
    return [sys.executable, tool, "--t5_path", args.t5_models_dir, "--prompts", prompts_file, "--out", out_dir, "--max_length", str(args.max_length)]


def extract_t5(args, command=t5_child_command):
    """--run_t5_feature_extract: prompts file -> child process -> <idx>.npz renamed to caption_features_new/<dir>_<name>.npz.  Returns the files in place."""
    with open(args.t5_json_path) as f:
        meta = json.load(f)[args.start_index:args.end_index]
    save = os.path.join(args.t5_save_root, "caption_features_new")
    save = save if args.save_path_suffix is None else f"{save}_{args.save_path_suffix}"
    os.makedirs(save, exist_ok=True)
    todo = [(it, os.path.join(save, feature_name(it["path"]) + ".npz")) for it in meta]
    todo = [(it, out) for it, out in todo if not os.path.exists(out)]
    if not todo:
        return []
    tmp = os.path.join(save, "_t5_child")
    os.makedirs(tmp, exist_ok=True)
    prompts_file = os.path.join(tmp, "prompts.txt")
    with open(prompts_file, "w") as f:
        f.write("\n".join(" ".join(str(it[args.caption_label]).split()) for it, _ in todo) + "\n")
    env = dict(os.environ, PXA_OPERAND_DTYPE="bf16")                              # the reference runs T5 in bf16; real XXL weights overflow fp16
    env.pop("PXA_LIB_PATH", None)
    r = subprocess.run(command(args, prompts_file, tmp), env=env, timeout=args.t5_timeout)
    if r.returncode != 0:
        raise SystemExit(f"--run_t5_feature_extract: the T5 encoder process failed (exit {r.returncode})")
    done = []
    for i, (_, out) in enumerate(todo):
        os.replace(os.path.join(tmp, f"{i}.npz"), out)
        done.append(out)
    shutil.rmtree(tmp)
    return done


def get_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--run_t5_feature_extract", action="store_true")
    p.add_argument("--run_vae_feature_extract", action="store_true")
    p.add_argument("--make_json", default=None, metavar="DIR")
    p.add_argument("--start_index", default=0, type=int)
    p.add_argument("--end_index", default=50000000, type=int)
    p.add_argument("--save_path_suffix", default=None, type=str)
    p.add_argument("--multi_scale", action="store_true")
    p.add_argument("--img_size", default=512, type=int)
    p.add_argument("--aspect_ratios", default=None, help="JSON file {ratio string: [H, W]}: the bucket table of --multi_scale")
    p.add_argument("--dataset_root", default="pixart-sigma-toy-dataset", type=str)
    p.add_argument("--vae_json_file", default="data_info.json", type=str, help="relative to --dataset_root")
    p.add_argument("--vae_models_dir", default="output/pretrained_models/pixart_sigma_sdxlvae_T5_diffusers/vae", type=str)
    p.add_argument("--vae_save_root", default="pixart-sigma-toy-dataset/InternData", type=str)
    p.add_argument("--batch", default=4, type=int, help="images of one bucket per vae.encode call")
    p.add_argument("--workers", default=8, type=int, help=f"image-decoding threads (at most {MAX_WORKERS})")
    p.add_argument("--transform", default="pillow", choices=["hip", "pillow"],
                   help="where resize / crop / normalise run: Pillow on the decoding threads, or the GPU kernels (the same bits; measured end to end in DESIGN.md section 4g)")
    p.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"], help="MFMA operand type of the VAE (reference: fp16)")
    p.add_argument("--max_length", default=300, type=int)
    p.add_argument("--t5_json_path", default="pixart-sigma-toy-dataset/InternData/data_info.json", type=str)
    p.add_argument("--t5_models_dir", default=None, type=str)
    p.add_argument("--caption_label", default="prompt", type=str)
    p.add_argument("--t5_save_root", default="pixart-sigma-toy-dataset/InternData", type=str)
    p.add_argument("--t5_timeout", default=7200, type=int)
    return p.parse_args(argv)


def main(argv=None):
    args = get_args(argv)
    os.environ["PXA_OPERAND_DTYPE"] = "f16" if args.dtype == "fp16" else "bf16"   # a per-process choice, made before the package is imported
    if args.make_json:
        out, n = make_json(args.make_json)
        print(f"wrote {out}: {n} images")
    if args.run_t5_feature_extract:
        if not args.t5_models_dir:
            raise SystemExit("--run_t5_feature_extract needs --t5_models_dir")
        print(f"T5: {len(extract_t5(args))} caption feature files")
    if args.run_vae_feature_extract:
        print(f"VAE: {len(extract_vae(args))} feature files in {vae_save_dir(args)}")
    print("Done")


if __name__ == "__main__":
    main()
