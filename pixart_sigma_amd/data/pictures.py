"""Pictures and caption strings, the data of the PixArt-Sigma training configs (`data = dict(..., load_vae_feat=False, load_t5_feat=False)`): the reference's
`InternalDataMSSigma` (diffusion/data/datasets/InternalData_ms.py:170-351) and the fixed-resolution `InternalDataSigma` (InternalData.py:162-290) with
load_vae_feat = False, restated without torchvision / mmcv.

    <root>/<image_list_json>                         [{"path", "height", "width", "ratio", "prompt", ["sharegpt4v"]}, ...]
    <root with InternData -> InternImgs>/<path>      the picture (InternalData_ms.py:236)
    <root>/caption_features_new/...npz               only with load_t5_feat = True (caption feature files next to pictures, which the reference also allows)

What differs from the reference is where the transform runs.  There `__getitem__` resizes and crops with Pillow in a DataLoader worker; here the dataset hands
out the picture's PATH (or, with decode=True, its decoded RGB bytes) together with the geometry - `form` ("cover" for the bucketed class, "short_side" for
the fixed one), `filter` and `target(idx)` - and ImagePreprocessor(form, filter) runs the same arithmetic on the GPU (data/images.py; data/pipeline.py joins
the two).  A transformed tensor never leaves this module.

Random choices - the caption kind, `random.random() < real_prompt_ratio` there, and the index that replaces an undecodable picture - come from a
torch.Generator the caller passes, so that a run is a function of its seed.

The bucket table is an input, as everywhere in this repository: the dict {ratio string: [H, W]} or the path of a JSON file that holds one.  The reference's
table names ('ASPECT_RATIO_1024') are refused: its tables are not copied into this tree."""
import json
import os
import re

import numpy as np
import torch

from .features import replace_img_ext
from .sampler import closest_ratio

MAX_RATIO = 4.5                 # items with ratio > 4.5 are dropped (InternalData_ms.py:233, InternalData.py:210)
LANCZOS_BASE_SIZES = (2048, 2880)
RETRIES = 20


def load_ratio_table(aspect_ratio_type):
    """The bucket table {ratio string: [H, W]} from the dict itself or from the path of a JSON file holding it."""
    if isinstance(aspect_ratio_type, dict):
        table = aspect_ratio_type
    elif isinstance(aspect_ratio_type, (str, os.PathLike)) and os.path.isfile(aspect_ratio_type):
        with open(aspect_ratio_type) as f:
            table = json.load(f)
    elif isinstance(aspect_ratio_type, str) and re.fullmatch(r"ASPECT_RATIO_\d+(_TEST)?", aspect_ratio_type):
        raise ValueError(f"aspect_ratio_type={aspect_ratio_type!r} is the name of one of the reference's bucket tables, and its tables are not part of this "
                         "repository: pass the table itself, {ratio string: [H, W]}, or the path of a JSON file that holds it")
    else:
        raise ValueError(f"aspect_ratio_type must be the bucket table {{ratio string: [H, W]}} or the path of a JSON file holding it, got {aspect_ratio_type!r}")
    if not isinstance(table, dict) or not table or not all(len(v) == 2 for v in table.values()):
        raise ValueError("the bucket table must map ratio strings to [H, W]")
    for k in table:
        float(k)
    return table


def table_base_size(table):
    """The base size of a bucket table: the side of its square bucket (the number in the reference's table names, InternalData_ms.py:203)."""
    return int(table[min(table, key=lambda k: abs(float(k) - 1.0))][0])


def decode_rgb(path):
    """The picture as uint8 (h, w, 3): torchvision's default_loader (Image.open(...).convert('RGB')) and the transform's T.Lambda, on the host."""
    from PIL import Image
    with open(path, "rb") as f, Image.open(f) as im:
        return np.array(im.convert("RGB"))


class PictureCaptionDataset(torch.utils.data.Dataset):
    """InternalDataSigma with load_vae_feat = False and the `default_train` transform (diffusion/data/transforms.py:21-30): T.Resize(n) then CenterCrop(n), the
    `short_side` form of ImagePreprocessor with target n = resolution.  T.Resize(n) carries torchvision's default interpolation, which is bilinear (the comment
    beside it says bicubic; tools/extract_features.py reads it the same way), so `filter` is "bilinear" here.  data_info is the reference's: img_hw =
    (resolution, resolution), aspect_ratio = 1.  An undecodable picture is replaced by a uniformly drawn index (InternalData.py:289), up to 20 times."""
    form = "short_side"

    def __init__(self, root, image_list_json="data_info.json", resolution=256, real_prompt_ratio=1.0, max_length=300, load_t5_feat=False, mask_type="null"):
        self.root, self.resolution, self.max_length, self.mask_type = root, int(resolution), int(max_length), mask_type
        self.real_prompt_ratio, self.load_t5_feat = float(real_prompt_ratio), bool(load_t5_feat)
        if not 0.0 <= self.real_prompt_ratio <= 1.0:
            raise ValueError(f"real_prompt_ratio={real_prompt_ratio!r} must lie in [0, 1]")
        self.filter = self._filter()
        self.meta, self.img_samples, self.txt_samples, self.sharegpt4v_txt_samples = [], [], [], []
        self.txt_feat_samples, self.gpt4v_txt_feat_samples = [], []
        self.ori_imgs_nums = 0
        img_root = root.replace("InternData", "InternImgs")
        for jf in (image_list_json if isinstance(image_list_json, (list, tuple)) else [image_list_json]):
            with open(os.path.join(root, jf)) as f:
                meta = json.load(f)
            self.ori_imgs_nums += len(meta)
            keep = [it for it in meta if it["ratio"] <= MAX_RATIO]
            self.meta += keep
            self.img_samples += [os.path.join(img_root, it["path"]) for it in keep]
            self.txt_samples += [it["prompt"] for it in keep]
            self.sharegpt4v_txt_samples += [it["sharegpt4v"] if "sharegpt4v" in it else "" for it in keep]
            names = [self._feat_name(it["path"]) for it in keep]
            self.txt_feat_samples += [os.path.join(root, "caption_features_new", n) for n in names]
            self.gpt4v_txt_feat_samples += [os.path.join(root, "sharegpt4v_caption_features_new", n) for n in names]
        if self.real_prompt_ratio < 1:                                             # InternalData_ms.py:263-264
            assert len(self.sharegpt4v_txt_samples[0]) != 0, "real_prompt_ratio < 1 needs the 'sharegpt4v' captions in the image list"

    def _filter(self):
        return "bilinear"

    @staticmethod
    def _feat_name(path):
        return path.rsplit("/", 1)[-1].replace(".png", ".npz")                     # InternalData.py:221

    def __len__(self):
        return len(self.meta)

    def get_data_info(self, idx):
        return {"height": self.meta[idx]["height"], "width": self.meta[idx]["width"]}

    # ---- geometry and bookkeeping of one item
    def target(self, idx):
        """What ImagePreprocessor(self.form, self.filter) takes as `target` for this item."""
        return self.resolution

    def output_hw(self, idx):
        return (self.resolution, self.resolution)

    def data_info(self, idx):
        return {"img_hw": torch.tensor([self.resolution, self.resolution], dtype=torch.float32), "aspect_ratio": 1.0, "mask_type": self.mask_type}

    def replacement(self, idx, generator=None):
        """The index the reference's __getitem__ tries after item idx failed to decode."""
        return int(torch.randint(len(self), (), generator=generator))

    def decode(self, idx):
        return decode_rgb(self.img_samples[idx])

    def caption(self, idx, generator=None):
        """(real_prompt, text, feature file): the user prompt with probability real_prompt_ratio, else the sharegpt4v caption (getdata's first lines)."""
        real = float(torch.rand((), generator=generator)) < self.real_prompt_ratio
        return (real, self.txt_samples[idx] if real else self.sharegpt4v_txt_samples[idx],
                self.txt_feat_samples[idx] if real else self.gpt4v_txt_feat_samples[idx])

    def caption_features(self, npz_path):
        """(caption feature (1, max_length, 4096) padded by repeating the last token, mask (1, 1, max_length) int16): getdata with load_t5_feat."""
        z = np.load(npz_path)
        txt = torch.from_numpy(z["caption_feature"])
        mask = torch.from_numpy(z["attention_mask"])[None] if "attention_mask" in z.files else torch.ones(1, 1, self.max_length)
        if txt.shape[1] != self.max_length:
            txt = torch.cat([txt, txt[:, -1:].repeat(1, self.max_length - txt.shape[1], 1)], dim=1)
            mask = torch.cat([mask, torch.zeros(1, 1, self.max_length - mask.shape[-1])], dim=-1)
        return txt, mask.to(torch.int16)

    def __getitem__(self, idx, generator=None, decode=False):
        """(picture, caption, attention mask (1, 1, max_length) int16, data_info, index used).  picture: the path, or with decode=True the RGB bytes uint8
        (h, w, 3) - then an undecodable file is replaced as the reference replaces it, and `index used` tells by which item.  caption: the string, or with
        load_t5_feat the features of the caption file."""
        for _ in range(RETRIES):
            try:
                real, txt, npz = self.caption(idx, generator)
                pic = self.decode(idx) if decode else self.img_samples[idx]
                mask = torch.ones(1, 1, self.max_length).to(torch.int16)
                if self.load_t5_feat:
                    txt, mask = self.caption_features(npz)
                return pic, txt, mask, self.data_info(idx), idx
            except Exception as e:      # noqa: BLE001  (the reference catches everything, prints and goes on)
                print(f"Error details {self.img_samples[idx]}: {e}")
                idx = self.replacement(idx, generator)
        raise RuntimeError("Too many bad data.")


class PictureCaptionDatasetMS(PictureCaptionDataset):
    """InternalDataMSSigma with load_vae_feat = False.  The bucket of an item is the closest ratio of the height / width RECORDED in the json; the picture is
    resized so that the bucket is covered and centre-cropped to it (the `cover` form); the filter is bicubic, Lanczos for a table of base size 2048 or 2880
    (InternalData_ms.py:216-218).  `ratio_nums` counts the first third of the list, as FeatureDatasetMS does.  data_info = {img_hw: the recorded (h, w) fp32,
    aspect_ratio: the closest ratio}.  An undecodable picture is replaced by an entry of ratio_index[its bucket] - which, without feature files, holds the
    first item of that bucket among the first third of the list and nothing else (InternalData_ms.py:277-283, 300-301 fill it only under load_vae_feat)."""
    form = "cover"

    def __init__(self, root, aspect_ratio_type, image_list_json="data_info.json", resolution=1024, real_prompt_ratio=1.0, max_length=300, load_t5_feat=False,
                 mask_type="null"):
        self.aspect_ratio = load_ratio_table(aspect_ratio_type)
        self.base_size = table_base_size(self.aspect_ratio)
        super().__init__(root, image_list_json, resolution, real_prompt_ratio, max_length, load_t5_feat, mask_type)
        self.ratio_index = {float(k): [] for k in self.aspect_ratio}
        self.ratio_nums = {float(k): 0 for k in self.aspect_ratio}
        for i, it in enumerate(self.meta[: len(self.meta) // 3]):
            r = float(closest_ratio(it["height"], it["width"], self.aspect_ratio)[0])
            self.ratio_nums[r] += 1
            if len(self.ratio_index[r]) == 0:
                self.ratio_index[r].append(i)

    def _filter(self):
        return "lanczos" if self.base_size in LANCZOS_BASE_SIZES else "bicubic"

    @staticmethod
    def _feat_name(path):
        return replace_img_ext("_".join(path.rsplit("/", 1)), ".npz")               # InternalData_ms.py:244

    def bucket(self, idx):
        """(ratio key, (H, W) ints) of the item's bucket."""
        it = self.meta[idx]
        key, size = closest_ratio(it["height"], it["width"], self.aspect_ratio)
        return key, (int(size[0]), int(size[1]))

    def target(self, idx):
        return self.bucket(idx)[1]

    def output_hw(self, idx):
        return self.bucket(idx)[1]

    def data_info(self, idx):
        it = self.meta[idx]
        return {"img_hw": torch.tensor([it["height"], it["width"]], dtype=torch.float32), "aspect_ratio": float(self.bucket(idx)[0]), "mask_type": self.mask_type}

    def replacement(self, idx, generator=None):
        pool = self.ratio_index[float(self.bucket(idx)[0])]
        if not pool:
            raise RuntimeError(f"{self.img_samples[idx]} cannot be decoded and its bucket has no item among the first third of the list to replace it")
        return pool[int(torch.randint(len(pool), (), generator=generator))]
