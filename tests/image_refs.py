"""numpy restatement of Pillow's 8-bit resampler (Image.resize for RGB images) and of the reference's three image transforms, written from the description
of the algorithm, scalar and slow on purpose: the reference of the image tests wherever Pillow is absent, and checked against Pillow where it imports
(tests/test_images_host.py).  Not shared with pixart_sigma_amd/data/images.py: the two are compared with each other."""
import math

import numpy as np
import torch

SUPPORT = {"bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}


def _filter(name, x):
    if name == "bilinear":
        x = abs(x)
        return 1.0 - x if x < 1.0 else 0.0
    if name == "bicubic":
        a = -0.5
        x = abs(x)
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    if -3.0 <= x < 3.0:
        def sinc(v):
            return 1.0 if v == 0.0 else math.sin(v * math.pi) / (v * math.pi)
        return sinc(x) * sinc(x / 3)
    return 0.0


def tables(in_size, out_size, name):
    """(coefficients int32 (out, ksize), bounds int32 (out, 2) = (xmin, n)) of one axis."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = SUPPORT[name] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / fs
    k = np.zeros((out_size, ksize), dtype=np.int32)
    b = np.zeros((out_size, 2), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [_filter(name, (x + xmin - center + 0.5) * inv) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            k[xx, x] = int(0.5 + v * (1 << 22)) if v >= 0 else int(-0.5 + v * (1 << 22))
        b[xx] = (xmin, n)
    return k, b


def _pass(img, k, b):
    """One pass along axis 0 of a uint8 (in, m, 3) array."""
    out = np.empty((k.shape[0],) + img.shape[1:], dtype=np.uint8)
    src = img.astype(np.int64)
    for i in range(k.shape[0]):
        xmin, n = int(b[i, 0]), int(b[i, 1])
        acc = (1 << 21) + (src[xmin:xmin + n] * k[i, :n].astype(np.int64)[:, None, None]).sum(0)
        assert np.abs(acc).max() < 2 ** 31                  # the int32 accumulator of the real thing does not wrap
        out[i] = np.clip(acc >> 22, 0, 255)
    return out


def resize(img, size, name):
    """uint8 (h, w, 3) -> uint8 (H, W, 3): horizontal pass first, a pass whose size does not change skipped."""
    h, w = img.shape[:2]
    H, W = size
    if W != w:
        img = _pass(img.transpose(1, 0, 2), *tables(w, W, name)).transpose(1, 0, 2)
    if H != h:
        img = _pass(img, *tables(h, H, name))
    return np.ascontiguousarray(img)


def crop_offset(size, crop):
    return int(round((size - crop) / 2.0))                  # Python's round: half to even


def geometry(form, hw, target):
    h, w = hw
    if form == "stretch":
        H, W = target
        return (H, W), (0, 0, H, W)
    if form == "cover":
        H, W = target
        Hr, Wr = (H, int(w * H / h)) if H / h > W / w else (int(h * W / w), W)
        return (Hr, Wr), (crop_offset(Hr, H), crop_offset(Wr, W), H, W)
    n = target
    Hr, Wr = (int(n * h / w), n) if w <= h else (n, int(n * w / h))
    return (Hr, Wr), (crop_offset(Hr, n), crop_offset(Wr, n), n, n)


def transform_u8(img, form, name, target):
    resized, (cy, cx, ch, cw) = geometry(form, img.shape[:2], target)
    return np.ascontiguousarray(resize(img, resized, name)[cy:cy + ch, cx:cx + cw])


def to_float(u8):
    """uint8 (H, W, 3) array -> fp32 (3, H, W) tensor: ToTensor + Normalize([.5], [.5]) as torch computes them on the CPU."""
    u = torch.from_numpy(np.array(u8, dtype=np.uint8, order="C"))
    return ((u.float() / 255 - 0.5) / 0.5).permute(2, 0, 1).contiguous()


def make_image(h, w, seed=0):
    """Random bytes with 0 / 255 checker patches (the negative lobes overshoot both clip limits)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for (y0, x0, s) in ((0, 0, 1), (h // 3, w // 4, 2), (h // 2, w // 2, 3)):
        y1, x1 = min(h, y0 + max(4, h // 3)), min(w, x0 + max(4, w // 3))
        patch = ((((yy // s) + (xx // s)) % 2) * 255).astype(np.uint8)
        img[y0:y1, x0:x1] = patch[y0:y1, x0:x1, None]
    return img


FILTER_NAMES = ("bilinear", "bicubic", "lanczos")
# (h, w) -> (H, W): down, up, each pass skipped once, tiny source, ksize up to 151, more than one 256-pixel block per row
RESIZE_CASES = [((37, 53), (16, 24)), ((16, 24), (37, 53)), ((64, 48), (64, 20)), ((41, 29), (13, 29)), ((7, 5), (33, 31)), ((200, 131), (8, 8)),
                ((33, 700), (20, 300))]
