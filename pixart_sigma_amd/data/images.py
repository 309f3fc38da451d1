"""Images in, images out: the reference's resize / crop / normalise transforms on the GPU, bit-identical to what it computes with Pillow and torchvision, and
the PNG side of torchvision.utils.save_image.

The three call sites of the reference all end in ToTensor + Normalize([.5], [.5]) after img.convert('RGB'); they differ in geometry (`transform_geometry`):

    stretch      tools/extract_features.py:103-111      T.Resize([H, W]) to the bucket size; the centre crop is a no-op
    cover        InternalData_ms.py:145-152, 326-333    resize so that the bucket is covered, aspect ratio kept, then CenterCrop([H, W])
    short_side   tools/extract_features.py:216-225      T.Resize(n): short side n, long side int(n * long / short); CenterCrop(n)

T.Resize on a PIL image is Image.resize: for 8-bit images Pillow's separable resampler with 22-bit fixed-point coefficients.  `resample_tables` computes those
coefficients as Pillow does (float64, weights summed in order, truncation toward zero) and pxa_image_resample (csrc/image.hip) applies them with Pillow's
integer arithmetic, horizontal pass first through a uint8 intermediate - so the bytes are Pillow's bytes and the floats torch's floats, not close to them.
Pillow itself is imported lazily and only to decode and encode files."""
import math

import numpy as np
import torch

FILTERS = {"bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}          # filter -> support
FORMS = ("stretch", "cover", "short_side")
PRECISION_BITS = 22


def _bilinear(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    # math.sin, element by element: the C library's sine, which is what Pillow calls (a vectorised sine may differ in the last bit)
    return np.array([_sinc(v) * _sinc(v / 3) if -3.0 <= v < 3.0 else 0.0 for v in x.ravel()], dtype=np.float64).reshape(x.shape)


_FILTER_FN = {"bilinear": _bilinear, "bicubic": _bicubic, "lanczos": _lanczos}


def resample_tables(in_size, out_size, filter):
    """Pillow's coefficient tables of one axis (Resample.c precompute_coeffs + normalize_coeffs_8bpc): (coefficients int32 (out_size, ksize), bounds int32
    (out_size, 2) = (first source index, tap count)).  Coefficients past the tap count are zero."""
    assert in_size >= 1 and out_size >= 1 and filter in FILTERS, (in_size, out_size, filter)
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = FILTERS[filter] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)                  # a C cast: toward zero, like astype
    n = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.float64)[None, :]
    w = _FILTER_FN[filter]((x + xmin[:, None] - center[:, None] + 0.5) * ss)
    w = np.where(np.arange(ksize)[None, :] < n[:, None], w, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for t in range(ksize):                                                            # the in-order sum: fp64 addition is not associative
        ww = ww + w[:, t]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int64).astype(np.int32)
    return k, np.stack([xmin, n], axis=1).astype(np.int32)


def center_crop_offset(size, crop):
    """torchvision CenterCrop's offset: int(round((size - crop) / 2.0)) with Python's round (half to even): remainder 1 -> 0, remainder 3 -> 2."""
    return int(round((size - crop) / 2.0))


def crop_window(resized, crop):
    """(cy, cx, ch, cw) of CenterCrop(crop) on an image of `resized`.  A crop larger than the image is refused: torchvision would pad it with black, and no
    geometry of the reference's transforms asks for that."""
    (Hr, Wr), (H, W) = resized, crop
    if Hr < H or Wr < W:
        raise ValueError(f"centre crop {H} x {W} of an image resized to {Hr} x {Wr}: the reference would pad it")
    return (center_crop_offset(Hr, H), center_crop_offset(Wr, W), H, W)


def transform_geometry(form, hw, target):
    """((Hr, Wr), (cy, cx, ch, cw)): the size the reference resizes an (h, w) image to and the window its centre crop keeps.  target: (H, W) for `stretch` and
    `cover`, n for `short_side`.  Raises where the reference's CenterCrop would pad (a crop larger than the resized image)."""
    h, w = int(hw[0]), int(hw[1])
    assert form in FORMS and h >= 1 and w >= 1, (form, hw)
    if form == "short_side":
        n = int(target)
        short, long = (w, h) if w <= h else (h, w)
        new_long = int(n * long / short)
        Hr, Wr = (new_long, n) if w <= h else (n, new_long)
        H = W = n
    else:
        H, W = int(target[0]), int(target[1])
        if form == "stretch":
            Hr, Wr = H, W
        elif H / h > W / w:
            Hr, Wr = H, int(w * H / h)
        else:
            Hr, Wr = int(h * W / w), W
    return (Hr, Wr), crop_window((Hr, Wr), (H, W))


def normalize_lut():
    """The 256 floats ToTensor + Normalize([.5], [.5]) make of a byte, computed by torch on the CPU as the reference computes them."""
    return (torch.arange(256, dtype=torch.uint8).float() / 255 - 0.5) / 0.5


def _rgb_array(img):
    """PIL image or uint8 HWC array -> uint8 (h, w, 3) array (img.convert('RGB') on the host, as the reference)."""
    if isinstance(img, np.ndarray):
        assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3, "array input: uint8 (h, w, 3)"
        return img
    if isinstance(img, torch.Tensor):
        assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3, "tensor input: uint8 (h, w, 3)"
        return img
    return np.array(img.convert("RGB"))                     # a writable copy: torch.from_numpy wants one


class Uploaded:
    """A uint8 (h, w, 3) device tensor whose copy was issued on a side stream, and the event that marks the copy done."""

    def __init__(self, tensor, event):
        self.tensor, self.event = tensor, event


def to_device_u8(img, device="cuda", stream=None):
    """PIL image or uint8 HWC array -> uint8 (h, w, 3) tensor on `device`: the RGB conversion and the upload, the part of the transform that is host work.  Meant
    for the decoding threads, which keeps both off the thread that launches kernels.  With `stream` (a torch.cuda.Stream) the copy is issued there and an
    `Uploaded` comes back: on the launching thread's own stream the copy would queue behind whatever that stream is running - a whole vae.encode - and the
    decoding thread would wait for it; ImagePreprocessor waits for the event on its stream before the kernels read the tensor."""
    a = _rgb_array(img)
    a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if stream is None:
        return a.to(device)
    with torch.cuda.stream(stream):
        t = a.to(device)
        ev = torch.cuda.Event()
        ev.record(stream)
    return Uploaded(t, ev)


class ImagePreprocessor:
    """form / filter of one of the reference's transforms, on `device`.  __call__(img, target, out=None, slot=0) resamples one image (PIL, or uint8 HWC array /
    tensor, on the host or already uploaded by `to_device_u8`) into out[slot] of an fp32 (B, 3, H, W) batch (allocated as (1, 3, H, W) when not given) and returns the batch; `to_u8` gives the bytes instead.
    Tables are cached per (in, out, filter) on the device; the intermediate image's workspace grows to the largest need and is reused (calls on one stream)."""

    def __init__(self, form="stretch", filter="bicubic", device="cuda"):
        assert form in FORMS and filter in FILTERS, (form, filter)
        self.form, self.filter, self.device = form, filter, torch.device(device)
        self._tables, self._ws, self._lut = {}, None, None

    def _axis(self, in_size, out_size, tap_major):
        if in_size == out_size:
            return None, None
        key = (in_size, out_size, self.filter, tap_major)
        if key not in self._tables:
            k, b = resample_tables(in_size, out_size, self.filter)
            kd = torch.from_numpy(np.ascontiguousarray(k.T if tap_major else k)).to(self.device)
            self._tables[key] = ((kd, torch.from_numpy(b).to(self.device)), b)
        return self._tables[key]

    def _run(self, img, target, out):
        from .. import ops
        if isinstance(img, Uploaded):                                     # copied on a side stream: order this stream behind the copy, and keep the allocator
            cur = torch.cuda.current_stream(self.device)                  # from handing the memory out again before this stream's kernels have read it
            cur.wait_event(img.event)
            img.tensor.record_stream(cur)
            src = img.tensor
        else:
            src = to_device_u8(img, self.device)
        h, w = src.shape[:2]
        resized, win = transform_geometry(self.form, (h, w), target)
        cy, cx, ch, cw = win
        htab, _ = self._axis(w, resized[1], True)
        vtab, vb = self._axis(h, resized[0], False)
        rows = None
        if vtab is not None:
            row0 = int(vb[cy, 0])
            rows = (row0, int(vb[cy + ch - 1, 0] + vb[cy + ch - 1, 1]) - row0)
            if htab is not None:
                need = rows[1] * cw * 3
                if self._ws is None or self._ws.numel() < need:
                    self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        if self._lut is None:
            self._lut = normalize_lut().to(self.device)
        o = out(ch, cw)
        ops.image_resample(src, resized, win, o, htab=htab, vtab=vtab, rows=rows, lut=self._lut, ws=self._ws)

    def __call__(self, img, target, out=None, slot=0):
        box = {}

        def pick(ch, cw):
            box["out"] = torch.empty((1, 3, ch, cw), dtype=torch.float32, device=self.device) if out is None else out
            assert tuple(box["out"].shape[1:]) == (3, ch, cw), f"batch of {tuple(box['out'].shape)} for a {ch} x {cw} window"
            return box["out"][slot]
        self._run(img, target, pick)
        return box["out"]

    def to_u8(self, img, target):
        """The transform's bytes, uint8 (H, W, 3): what the reference has before ToTensor."""
        box = {}

        def pick(ch, cw):
            box["out"] = torch.empty((ch, cw, 3), dtype=torch.uint8, device=self.device)
            return box["out"]
        self._run(img, target, pick)
        return box["out"]


def pillow_transform(img, form, filter, target):
    """The reference's transform on the CPU, with Pillow: (3, H, W) fp32.  The comparison path of the extraction tool (--transform pillow) and of the tests."""
    from PIL import Image
    res = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[filter]
    img = img.convert("RGB")
    (Hr, Wr), (cy, cx, ch, cw) = transform_geometry(form, (img.size[1], img.size[0]), target)
    if (Hr, Wr) != (img.size[1], img.size[0]):
        img = img.resize((Wr, Hr), res)
    u = torch.from_numpy(np.asarray(img.crop((cx, cy, cx + cw, cy + ch))).copy())
    return ((u.float() / 255 - 0.5) / 0.5).permute(2, 0, 1).contiguous()


def save_png(tensor, path, format=None, **kw):
    """One (3, H, W) or (1, 3, H, W) image in [-1, 1] (fp16 / fp32, on the GPU) -> a picture file, as torchvision.utils.save_image(normalize=True,
    value_range=(-1, 1)) writes it: bytes from ops.image_to_u8, the file from Pillow (format by the path's extension unless given)."""
    from PIL import Image
    from .. import ops
    t = tensor if tensor.dim() == 4 else tensor[None]
    assert t.shape[0] == 1 and t.shape[1] == 3, "save_png writes one RGB image"
    u = ops.image_to_u8(t.contiguous())[0].cpu().numpy()
    Image.fromarray(u).save(path, format=format, **kw)
    return path
