"""tools/extract_features.py end to end on the GPU: PNG files -> ImagePreprocessor (the reference's multi-scale `stretch` transform, bit for bit Pillow's) -> the
HIP VAE's encode -> .npy files under the names, shape and dtype FeatureDatasetMS loads.  The VAE is the small random-init one of tests/test_vae_gpu.py (its
four-level configuration: the files are (8, h / 8, w / 8)).

The file contents are compared with vae.encode on the same tensor, computed here.  Two encodes of one tensor are compared first: where they are bitwise equal
the files must EQUAL cat[mean, std] rounded to float16; otherwise the bound is the one tests/test_vae_gpu.py applies to encode (MODEL_TOL = 2.5e-2 rel-L2).
Which case held is recorded in the session's parity summary (conftest.record_parity: label `encode_bitwise_repeatable`, 1 = equal).  Measured on an MI355X
(bf16 operands): two encodes are NOT bitwise equal (the GroupNorm statistics are accumulated with atomics), so the tolerance branch holds; file against a
second encode 5.1e-3 (tall) and 4.0e-3 (wide) rel-L2."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import image_refs as R
from conftest import ROOT, record_parity, rel_l2

pytestmark = pytest.mark.gpu

MODEL_TOL = 2.5e-2                                    # tests/test_vae_gpu.py
RATIOS = {"0.67": [64, 96], "1.5": [96, 64]}


def _tool():
    spec = importlib.util.spec_from_file_location("imgtest_extract_features_gpu", os.path.join(ROOT, "tools", "extract_features.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_png_files_to_feature_files(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    Image = pytest.importorskip("PIL.Image", reason="Pillow is needed to write and decode the PNG files")
    from oracle.vae_ref import AutoencoderKLRef, randomize_
    from pixart_sigma_amd.data import FeatureDatasetMS
    from pixart_sigma_amd.data.images import ImagePreprocessor, pillow_transform
    from pixart_sigma_amd.vae import AutoencoderKL
    tool = _tool()
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "pics"))
    meta, arrays = [], {}
    for name, (h, w) in (("tall", (70, 45)), ("wide", (45, 70))):
        arrays[name] = R.make_image(h, w, seed=h)
        Image.fromarray(arrays[name]).save(os.path.join(root, "pics", name + ".png"))
        meta.append({"path": f"pics/{name}.png", "height": h, "width": w, "ratio": h / w, "prompt": name})
    with open(os.path.join(root, "data_info.json"), "w") as f:
        json.dump(meta, f)
    with open(os.path.join(root, "ratios.json"), "w") as f:
        json.dump(RATIOS, f)

    cfg = dict(block_out_channels=(128, 256, 512, 512), layers_per_block=2)
    vae = AutoencoderKL(**cfg)
    vae.load_state_dict(randomize_(AutoencoderKLRef(**cfg), seed=5).state_dict())
    vae = vae.cuda()

    def encode(x):
        d = vae.encode(x).latent_dist
        return d.mean, d.std

    # the transform: GPU tensor == the Pillow path's tensor == the restatement's
    pre = ImagePreprocessor("stretch", "bicubic", "cuda")
    tensors = {}
    for name, target in (("tall", (96, 64)), ("wide", (64, 96))):
        with Image.open(os.path.join(root, "pics", name + ".png")) as im:
            got = pre(im, target)
            want = pillow_transform(im, "stretch", "bicubic", target)
        assert got.shape == (1, 3, *target) and torch.equal(got[0].cpu(), want)
        assert torch.equal(want, R.to_float(R.transform_u8(arrays[name], "stretch", "bicubic", target)))
        tensors[name] = got

    args = tool.get_args(["--run_vae_feature_extract", "--multi_scale", "--img_size", "512", "--aspect_ratios", os.path.join(root, "ratios.json"),
                          "--dataset_root", root, "--vae_json_file", "data_info.json", "--vae_save_root", root, "--workers", "2", "--transform", "hip"])
    written = tool.extract_vae(args, encode=encode)
    ds = FeatureDatasetMS(root, RATIOS, resolution=512)
    assert sorted(written) == sorted(ds.vae_feat) and [os.path.basename(p) for p in ds.vae_feat] == ["pics_tall.npy", "pics_wide.npy"]

    a, b = encode(tensors["tall"]), encode(tensors["tall"])
    repeatable = torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    record_parity("encode_bitwise_repeatable", 1.0 if repeatable else 0.0)
    for path, name, (h, w) in zip(ds.vae_feat, ("tall", "wide"), ((96, 64), (64, 96))):
        arr = np.load(path)
        assert arr.dtype == np.float16 and arr.shape == (8, h // 8, w // 8)
        mean, std = encode(tensors[name])
        want = torch.cat([mean, std], dim=1)[0].to(torch.float16).cpu()
        got = torch.from_numpy(arr)
        err = rel_l2(got.float(), want.float())
        print(f"\n{name}: encode repeatable bitwise = {repeatable}; file vs vae.encode rel-L2 {err:.2e}")
        record_parity(f"extract_file_vs_encode_{name}", err, None if repeatable else MODEL_TOL)
        if repeatable:
            assert torch.equal(got, want)
        else:
            assert err < MODEL_TOL
    assert tool.extract_vae(args, encode=encode) == []                                # everything exists: nothing is decoded or written again
    from pixart_sigma_amd.data.features import vae_feat_loader
    sample = vae_feat_loader(ds.vae_feat[0])
    assert sample.shape == (4, 12, 8) and sample.dtype == torch.float16
