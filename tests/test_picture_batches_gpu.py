"""PictureBatches (pixart_sigma_amd/data/pipeline.py) on the GPU: generated pictures in two buckets, a random-weight VAE (the four-level configuration of
tests/test_vae_gpu.py) and caption feature files.  16 PNGs of assorted sizes (8 tall, about 4 : 1 -> bucket "4.0" = 64 x 8; 8 wide -> "0.25" = 8 x 64), one
of them a file that holds no picture, batches of 2.

The buckets are the narrowest pictures the encoder takes, because at 2 x 64 x 8 and 2 x 8 x 64 two encodes of one tensor agree bit for bit in both operand
builds (measured: tests/test_vae_posterior_gpu.py; larger pictures vary in the last bits through the atomics of the convolution epilogues' GroupNorm
statistics) - so that "two iterators with one seed agree exactly" can be asserted on x0 as on everything else.

What must hold: every picture tensor that enters the VAE equals pillow_transform of the file the batch names, bit for bit (the `cover` form, bicubic); two
iterators with one seed, one decoding on 1 thread and one on 8, agree exactly - pictures, noise, caption features, masks, data_info and x0; the ranks' index
sets are disjoint; x0 has the bucket's latent shape and data_info is the json's."""
import json

import numpy as np
import pytest
import torch

import image_refs as R

pytestmark = pytest.mark.gpu

RATIOS = {"0.25": [8, 64], "4.0": [64, 8]}
TALL = [(120, 30), (100, 26), (90, 21), (130, 33), (88, 22), (110, 25), (96, 24), (140, 36)]          # ratios 3.8 .. 4.4: under the datasets' 4.5 filter
L, BROKEN = 8, 9


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    Image = pytest.importorskip("PIL.Image")
    from oracle.vae_ref import AutoencoderKLRef, randomize_
    from pixart_sigma_amd.data import PictureCaptionDatasetMS
    from pixart_sigma_amd.vae import AutoencoderKL
    top = tmp_path_factory.mktemp("batches")
    root, imgs = top / "InternData", top / "InternImgs" / "pics"
    (root / "caption_features_new").mkdir(parents=True)
    imgs.mkdir(parents=True)
    meta = []
    g = torch.Generator().manual_seed(0)
    for i in range(16):
        h, w = TALL[i // 2] if i % 2 == 0 else TALL[i // 2][::-1]
        name = f"p{i:02d}"
        if i == BROKEN:
            (imgs / f"{name}.png").write_bytes(b"no picture in here")
        else:
            Image.fromarray(R.make_image(h, w, seed=100 + i)).save(imgs / f"{name}.png")
        meta.append({"path": f"pics/{name}.png", "height": h, "width": w, "ratio": h / w, "prompt": name})
        n = 5 + i % 4                                                                                  # 5 .. 8 caption tokens: padded to L by the dataset
        np.savez(root / "caption_features_new" / f"pics_{name}.npz", caption_feature=torch.randn(1, n, 4096, generator=g).to(torch.float16).numpy(),
                 attention_mask=np.ones((1, n), dtype=np.int64))
    (root / "data_info.json").write_text(json.dumps(meta))
    ds = PictureCaptionDatasetMS(str(root), RATIOS, resolution=64, max_length=L, load_t5_feat=True)
    cfg = dict(block_out_channels=(128, 256, 512, 512), layers_per_block=2)
    vae = AutoencoderKL(**cfg)
    vae.load_state_dict(randomize_(AutoencoderKLRef(**cfg), seed=5).state_dict())
    return ds, vae.cuda(), meta


def _take(ds, vae, n, seed=3, rank=0, world=1, workers=3):
    from pixart_sigma_amd.data import PictureBatches
    pb = PictureBatches(ds, 2, RATIOS, vae, None, seed=seed, rank=rank, world=world, num_workers=workers, scale=0.13025)
    out, it = [], iter(pb)
    for _ in range(n):
        x0, y, mask, info = next(it)
        out.append(dict(x0=x0, y=y, mask=mask, info=info, pictures=pb.pictures, noise=pb.noise, indices=list(pb.indices)))
    it.close()
    return out


def test_batches_hold_pillows_pictures_and_the_jsons_data_info(setup):
    from PIL import Image
    from pixart_sigma_amd.data.images import pillow_transform
    ds, vae, meta = setup
    assert ds.filter == "bicubic" and ds.form == "cover"
    seen = set()
    for b in _take(ds, vae, 4):
        key, (H, W) = ds.bucket(b["indices"][0])
        assert BROKEN not in b["indices"]
        assert b["pictures"].dtype == torch.float32 and tuple(b["pictures"].shape) == (2, 3, H, W)
        for slot, i in enumerate(b["indices"]):
            assert ds.bucket(i)[0] == key                                                             # one bucket per batch
            with Image.open(ds.img_samples[i]) as im:
                want = pillow_transform(im, "cover", "bicubic", (H, W))
            assert torch.equal(b["pictures"][slot].cpu(), want), (i, ds.img_samples[i])
            assert b["info"]["img_hw"][slot].tolist() == [float(meta[i]["height"]), float(meta[i]["width"])]
            assert torch.equal(b["info"]["aspect_ratio"][slot], torch.tensor([float(key)]))
            feat, m = ds.caption_features(ds.txt_feat_samples[i])
            assert torch.equal(b["y"][slot].cpu(), feat.float()) and torch.equal(b["mask"][slot], m.reshape(-1).long())
        assert b["x0"].dtype == torch.float32 and tuple(b["x0"].shape) == (2, 4, H // 8, W // 8) and torch.isfinite(b["x0"]).all()
        assert tuple(b["y"].shape) == (2, 1, L, 4096) and b["y"].is_cuda and b["y"].dtype == torch.float32
        assert tuple(b["mask"].shape) == (2, L) and b["mask"].dtype == torch.int64 and not b["mask"].is_cuda
        assert tuple(b["info"]["img_hw"].shape) == (2, 2) and tuple(b["info"]["aspect_ratio"].shape) == (2, 1)
        assert tuple(b["noise"].shape) == tuple(b["x0"].shape)
        seen.add(key)
    assert seen == {"0.25", "4.0"}


def test_two_iterators_with_one_seed_agree(setup):
    ds, vae, _ = setup
    a, b = _take(ds, vae, 4, workers=1), _take(ds, vae, 4, workers=8)
    for u, v in zip(a, b):
        assert u["indices"] == v["indices"]
        for k in ("pictures", "noise", "y", "mask", "x0"):
            assert torch.equal(u[k], v[k]), k
        assert torch.equal(u["info"]["img_hw"], v["info"]["img_hw"]) and torch.equal(u["info"]["aspect_ratio"], v["info"]["aspect_ratio"])
    other = _take(ds, vae, 1, seed=4)
    assert other[0]["indices"] != a[0]["indices"] or not torch.equal(other[0]["noise"], a[0]["noise"])


def test_rank_split_is_disjoint(setup):
    from pixart_sigma_amd.data import PictureBatches
    ds, vae, _ = setup
    # 16 items, 2 ranks: 8 per rank and epoch in two buckets, so at least 3 full batches of 2 - the first 3 batches of a rank lie in its first epoch.
    # The index order is what is split (a picture that replaces an undecodable one may belong to the other rank's slice, as in the reference).
    order = torch.randperm(16, generator=torch.Generator().manual_seed(3)).tolist()
    first = []
    for r in (0, 1):
        gen = PictureBatches(ds, 2, RATIOS, vae, None, seed=3, rank=r, world=2).index_batches()
        first.append([next(gen) for _ in range(3)])
        assert {i for b in first[r] for i in b} <= set(order[r::2])
    s0, s1 = ({i for b in f for i in b} for f in first)
    assert len(s0) == 6 and len(s1) == 6 and not (s0 & s1)
    assert any(BROKEN in b for b in first[1])                                                         # seed 3: rank 1 meets the broken file at once
    got = _take(ds, vae, 3, rank=1, world=2)
    assert [b["indices"] for b in got] == [[1 if i == BROKEN else i for i in b] for b in first[1]]   # replaced by item 1, its bucket's entry of ratio_index
