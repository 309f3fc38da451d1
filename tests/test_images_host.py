"""Host side of the image pipeline, no GPU: the numpy restatement of Pillow's resampler against Pillow, the product's coefficient tables and geometry against
the restatement and hand-computed cases, the extraction tool's file naming through FeatureDatasetMS (fake encoder), the T5 glue's rename (fake child), and the
three new symbols of the C ABI."""
import ctypes
import importlib.util
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import image_refs as R
from conftest import ROOT


def _tool():
    spec = importlib.util.spec_from_file_location("imgtest_extract_features", os.path.join(ROOT, "tools", "extract_features.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", R.FILTER_NAMES)
def test_restatement_is_pillow_byte_for_byte(name):
    Image = pytest.importorskip("PIL.Image")
    res = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[name]
    for hw, HW in R.RESIZE_CASES + [((200, 131), (32, 40))]:
        img = R.make_image(*hw, seed=hw[0] + hw[1])
        want = np.asarray(Image.fromarray(img).resize((HW[1], HW[0]), res))
        assert int((R.resize(img, HW, name) != want).sum()) == 0, (hw, HW)
    for value in (0, 255):
        img = np.full((37, 53, 3), value, dtype=np.uint8)
        assert int((R.resize(img, (16, 24), name) != np.asarray(Image.fromarray(img).resize((24, 16), res))).sum()) == 0


@pytest.mark.parametrize("name", R.FILTER_NAMES)
def test_resample_tables_equal_the_restatement(name):
    from pixart_sigma_amd.data.images import resample_tables
    sizes = sorted({(i, o) for hw, HW in R.RESIZE_CASES for i, o in zip(hw, HW)} | {(1, 5), (5, 1), (4000, 1024), (1024, 1024)})
    for i, o in sizes:
        k, b = resample_tables(i, o, name)
        kr, br = R.tables(i, o, name)
        assert k.dtype == np.int32 and b.dtype == np.int32 and k.shape == kr.shape == (o, int(np.ceil(R.SUPPORT[name] * max(i / o, 1.0))) * 2 + 1)
        assert np.array_equal(k, kr) and np.array_equal(b, br), (i, o)
    assert resample_tables(200, 8, "lanczos")[0].shape[1] == 151


def test_transform_geometry_hand_computed():
    from pixart_sigma_amd.data.images import center_crop_offset, transform_geometry
    assert [center_crop_offset(32 + r, 32) for r in (0, 1, 2, 3, 4, 5)] == [0, 0, 1, 2, 2, 2]          # halves go to the even neighbour
    assert transform_geometry("stretch", (70, 45), (32, 48)) == ((32, 48), (0, 0, 32, 48))
    # cover, 32/70 = 0.457 < 32/45 = 0.711: the width fits, the height overhangs: int(70 * 32 / 45) = 49, top = round(8.5) = 8
    assert transform_geometry("cover", (70, 45), (32, 32)) == ((49, 32), (8, 0, 32, 32))
    # cover, 32/45 = 0.711 > 40/70 = 0.571: the height fits: int(70 * 32 / 45) = 49, left = round(4.5) = 4
    assert transform_geometry("cover", (45, 70), (32, 40)) == ((32, 49), (0, 4, 32, 40))
    assert transform_geometry("cover", (100, 100), (32, 35)) == ((35, 35), (2, 0, 32, 35))            # remainder 3 -> 2 (1.5 rounds to even)
    assert transform_geometry("cover", (100, 100), (32, 33)) == ((33, 33), (0, 0, 32, 33))            # remainder 1 -> 0
    assert transform_geometry("cover", (64, 64), (32, 32)) == ((32, 32), (0, 0, 32, 32))              # equality takes the else branch
    # short_side: 45 -> 24, the long side int(24 * 70 / 45) = 37, left = round(6.5) = 6
    assert transform_geometry("short_side", (45, 70), 24) == ((24, 37), (0, 6, 24, 24))
    assert transform_geometry("short_side", (70, 45), 24) == ((37, 24), (6, 0, 24, 24))
    assert transform_geometry("short_side", (50, 50), 24) == ((24, 24), (0, 0, 24, 24))
    for form, hw, target in (("cover", (70, 45), (32, 32)), ("cover", (45, 70), (32, 40)), ("short_side", (45, 70), 24), ("stretch", (9, 9), (3, 5))):
        assert transform_geometry(form, hw, target) == R.geometry(form, hw, target)
    from pixart_sigma_amd.data.images import crop_window
    assert crop_window((40, 35), (32, 32)) == (4, 2, 32, 32)
    for resized in ((31, 40), (40, 31)):                                                                 # a crop larger than the image: the reference would pad
        with pytest.raises(ValueError):
            crop_window(resized, (32, 32))


def test_transform_against_torch_normalisation():
    from pixart_sigma_amd.data.images import normalize_lut
    lut = normalize_lut()
    u = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(lut, (u.float() / 255 - 0.5) / 0.5) and lut[0] == -1 and lut[255] == 1
    img = R.make_image(9, 7, seed=1)
    assert torch.equal(R.to_float(img), lut[torch.from_numpy(img).long()].permute(2, 0, 1))


def _dataset(tmp_path, n=5):
    root = tmp_path / "data"
    meta = []
    for i in range(n):
        h, w = ((70, 45), (45, 70))[i % 2]
        meta.append({"path": f"shard{i // 2}/img{i}.png", "height": h, "width": w, "ratio": h / w, "prompt": f"picture {i}\nsecond line"})
    meta.append({"path": "shard9/panorama.jpg", "height": 10, "width": 1, "ratio": 10.0, "prompt": "dropped: ratio > 4.5"})
    os.makedirs(root)
    with open(root / "data_info.json", "w") as f:
        json.dump(meta, f)
    ratios = {"0.5": [32, 64], "2.0": [64, 32]}
    with open(root / "ratios.json", "w") as f:
        json.dump(ratios, f)
    return str(root), meta, ratios


def test_extraction_file_names_round_trip_through_feature_dataset(tmp_path):
    """The tool's loop with a fake loader, transform and encoder: what it writes is what FeatureDatasetMS opens, grouped by bucket, existing files skipped."""
    from pixart_sigma_amd.data import FeatureDatasetMS
    tool = _tool()
    root, meta, ratios = _dataset(tmp_path)
    args = tool.get_args(["--run_vae_feature_extract", "--multi_scale", "--img_size", "512", "--aspect_ratios", os.path.join(root, "ratios.json"),
                          "--dataset_root", root, "--vae_json_file", "data_info.json", "--vae_save_root", root, "--batch", "2", "--workers", "64"])
    seen = {"batches": [], "loaded": []}

    def load(path):
        seen["loaded"].append(path)
        return os.path.basename(path)

    def transform(img, target, batch, slot):
        batch[slot].fill_(float(img[3:-4]))                       # the image's number

    def encode(x):
        seen["batches"].append(tuple(x.shape))
        m = x[:, :1, ::8, ::8].repeat(1, 4, 1, 1)
        return m, m + 0.5

    written = tool.extract_vae(args, encode=encode, load=load, transform=transform, device="cpu")
    assert len(written) == 5 and sorted(seen["batches"]) == sorted([(2, 3, 64, 32), (1, 3, 64, 32), (2, 3, 32, 64)])      # by bucket, no panorama
    ds = FeatureDatasetMS(root, ratios, resolution=512)
    assert sorted(ds.vae_feat) == sorted(written)
    for i, p in enumerate(ds.vae_feat):
        a = np.load(p)
        h, w = ((64, 32), (32, 64))[i % 2]
        assert a.dtype == np.float16 and a.shape == (8, h // 8, w // 8) and (a[:4] == i).all() and (a[4:] == i + 0.5).all()
        assert os.path.basename(p) == f"shard{i // 2}_img{i}.npy" and os.path.basename(os.path.dirname(p)) == "img_sdxl_vae_features_512resolution_ms_new"
    seen["loaded"].clear()
    os.remove(ds.vae_feat[3])
    assert tool.extract_vae(args, encode=encode, load=load, transform=transform, device="cpu") == [ds.vae_feat[3]] and len(seen["loaded"]) == 1
    single = tool.get_args(["--img_size", "256", "--vae_save_root", root, "--save_path_suffix", "x"])
    assert tool.vae_save_dir(single) == os.path.join(root, "img_sdxl_vae_features_256resolution_new_x")
    assert [tool.filter_for(s, ms) for s, ms in ((512, True), (1024, True), (2048, True), (2880, True), (256, False), (512, False), (2048, False))] == \
        ["bicubic", "bicubic", "lanczos", "lanczos", "bilinear", "bilinear", "lanczos"]
    assert tool.MAX_WORKERS == 16 and tool.get_args([]).workers == 8 and tool.get_args([]).transform in ("hip", "pillow")


def test_t5_glue_renames_the_child_files(tmp_path):
    from pixart_sigma_amd.data import FeatureDatasetMS
    tool = _tool()
    root, meta, ratios = _dataset(tmp_path, n=3)
    child = tmp_path / "fake_child.py"
    child.write_text("import sys, numpy as np\nprompts = [l.rstrip('\\n') for l in open(sys.argv[1])]\n"
                     "for i, p in enumerate(prompts):\n    np.savez(f'{sys.argv[2]}/{i}.npz', caption_feature=np.full((1, 4, 8), float(p.split()[1]), dtype=np.float32), "
                     "attention_mask=np.ones((1, 4), dtype=np.int64))\nnp.savez(f'{sys.argv[2]}/null.npz', caption_feature=np.zeros((1, 4, 8), dtype=np.float32))\n")
    args = tool.get_args(["--run_t5_feature_extract", "--t5_json_path", os.path.join(root, "data_info.json"), "--t5_models_dir", "/models/t5", "--t5_save_root", root,
                          "--end_index", "3"])
    done = tool.extract_t5(args, command=lambda a, prompts_file, out_dir: [sys.executable, str(child), prompts_file, out_dir])
    ds = FeatureDatasetMS(root, ratios, resolution=512)
    assert done == ds.txt_feat[:3] and [os.path.basename(p) for p in done] == ["shard0_img0.npz", "shard0_img1.npz", "shard1_img2.npz"]
    for i, p in enumerate(done):
        assert float(np.load(p)["caption_feature"][0, 0, 0]) == i                  # prompt i ("picture i second line": one line per prompt) landed on image i
    assert not os.path.exists(os.path.join(root, "caption_features_new", "_t5_child"))
    assert tool.extract_t5(args, command=lambda *a: [sys.executable, "-c", "raise SystemExit(3)"]) == []      # everything exists: no child
    cmd = tool.t5_child_command(args, "P", "O")
    assert cmd[1].endswith(os.path.join("tools", "extract_t5_features.py")) and cmd[2:] == ["--t5_path", "/models/t5", "--prompts", "P", "--out", "O", "--max_length", "300"]


def test_make_json_reads_sidecar_captions(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    tool = _tool()
    os.makedirs(tmp_path / "a")
    Image.fromarray(R.make_image(20, 30)).save(tmp_path / "a" / "one.png")
    Image.fromarray(R.make_image(30, 20)).save(tmp_path / "two.jpg")
    Image.fromarray(R.make_image(8, 8)).save(tmp_path / "no_caption.png")
    (tmp_path / "a" / "one.txt").write_text("a wide picture\n")
    (tmp_path / "two.txt").write_text("a tall\npicture")
    out, n = tool.make_json(str(tmp_path))
    items = json.load(open(out))
    assert n == 2 and items == [{"path": "two.jpg", "height": 30, "width": 20, "ratio": 1.5, "prompt": "a tall picture"},
                                {"path": "a/one.png", "height": 20, "width": 30, "ratio": 20 / 30, "prompt": "a wide picture"}]
    assert tool.feature_name("a/one.png") == "a_one" and tool.feature_name("two.jpg") == "two"


def test_pillow_transform_equals_the_restatement():
    Image = pytest.importorskip("PIL.Image")
    from pixart_sigma_amd.data.images import pillow_transform
    img = R.make_image(70, 45, seed=5)
    for form, name, target in (("stretch", "bicubic", (32, 48)), ("cover", "bicubic", (32, 32)), ("short_side", "bilinear", 24), ("short_side", "lanczos", 45)):
        assert torch.equal(pillow_transform(Image.fromarray(img), form, name, target), R.to_float(R.transform_u8(img, form, name, target))), (form, name)


def test_image_symbols_declared_exported_and_bound():
    from pixart_sigma_amd import build, lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pixart_hip.h")).read(), flags=re.S)
    dll = ctypes.CDLL(build.build())
    for name in ("pxa_image_resample", "pxa_image_to_u8", "pxa_image_resample_ws_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared"
        assert hasattr(dll, name), f"{name} not exported"
        assert name in lib.SIGNATURES or name in lib.OTHER_SYMBOLS, f"{name} not bound"
    L = lib.load()
    assert L.pxa_abi_version() == 11 == lib.ABI_VERSION
    assert L.pxa_image_resample_ws_bytes(7, 5) == 105 and L.pxa_image_resample_ws_bytes(0, 5) < 0
    assert L.pxa_image_resample_ws_bytes(65535, 65535) == 65535 * 65535 * 3                               # past 2^31: a long
    n_args = len(re.search(r"int pxa_image_resample\(([^)]*)\)", src).group(1).split(","))
    assert n_args == len(lib.SIGNATURES["pxa_image_resample"]) == 25
