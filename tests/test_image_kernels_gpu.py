"""pxa_image_resample / pxa_image_to_u8 (csrc/image.hip) against tests/image_refs.py (the numpy restatement of Pillow's resampler; test_images_host.py pins it
to Pillow) and, where Pillow imports, against Pillow itself.  Parity is exact: zero differing bytes for the uint8 output, torch.equal for the float one - the
resampler is integer arithmetic on tables the host computed, and the float is a table look-up of what torch computes on the CPU.

Every run poisons what the kernels must not touch: the fp32 slot sits in the middle of a (3, 3, H, W) batch, the uint8 output inside a larger buffer, the
intermediate-image workspace between two guard bands."""
import numpy as np
import pytest
import torch

import image_refs as R

pytestmark = pytest.mark.gpu

POISON_F, POISON_B, GUARD = 7.5, 0xA5, 64
_REF = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pixart_sigma_amd import ops as o
    return o


def ref_resized(key, img, resized, name):
    """The whole resized image by the restatement, computed once per (image key, size, filter)."""
    k = (key, tuple(resized), name)
    if k not in _REF:
        _REF[k] = R.resize(img, resized, name).copy()             # resize returns its input when nothing changes
        _REF[k].setflags(write=False)
    return _REF[k]


def device_tables(in_size, out_size, name, tap_major):
    from pixart_sigma_amd.data.images import resample_tables
    if in_size == out_size:
        return None, None
    k, b = resample_tables(in_size, out_size, name)
    return (torch.from_numpy(np.ascontiguousarray(k.T if tap_major else k)).cuda(), torch.from_numpy(b).cuda()), b


def run_both_outputs(ops, img, resized, window, name, pitch_pad=0):
    """uint8 and fp32 results of one call each, with every neighbour of the outputs and of the workspace checked untouched."""
    from pixart_sigma_amd.data.images import normalize_lut
    h, w = img.shape[:2]
    cy, cx, ch, cw = window
    if pitch_pad:
        buf = torch.full((h, 3 * w + pitch_pad), POISON_B, dtype=torch.uint8)
        buf[:, :3 * w] = torch.from_numpy(img.copy()).reshape(h, 3 * w)
        src = buf.cuda().as_strided((h, w, 3), (3 * w + pitch_pad, 3, 1))
    else:
        src = torch.from_numpy(img.copy()).cuda()
    htab, _ = device_tables(w, resized[1], name, True)
    vtab, vb = device_tables(h, resized[0], name, False)
    rows = None
    if vtab is not None:
        rows = (int(vb[cy, 0]), int(vb[cy + ch - 1, 0] + vb[cy + ch - 1, 1] - vb[cy, 0]))
    need = rows[1] * cw * 3 if (htab is not None and vtab is not None) else 0
    lut = normalize_lut().cuda()
    outs = []
    for want_float in (False, True):
        wsbuf = torch.full((need + 2 * GUARD,), POISON_B, dtype=torch.uint8, device="cuda")
        ws = wsbuf[GUARD:GUARD + need] if need else None
        if want_float:
            batch = torch.full((3, 3, ch, cw), POISON_F, device="cuda")
            ops.image_resample(src, resized, window, batch[1], htab=htab, vtab=vtab, rows=rows, lut=lut, ws=ws)
            torch.cuda.synchronize()
            assert (batch[0] == POISON_F).all() and (batch[2] == POISON_F).all(), "a neighbouring batch slot was written"
            outs.append(batch[1].cpu())
        else:
            big = torch.full((ch + 2, 3 * cw + 32), POISON_B, dtype=torch.uint8, device="cuda")
            view = big.as_strided((ch, cw, 3), (3 * cw + 32, 3, 1), (3 * cw + 32) + 16)
            ops.image_resample(src, resized, window, view, htab=htab, vtab=vtab, rows=rows, ws=ws)
            torch.cuda.synchronize()
            got = big.cpu()
            inner = got[1:ch + 1, 16:16 + 3 * cw].clone()
            got[1:ch + 1, 16:16 + 3 * cw] = POISON_B
            assert (got == POISON_B).all(), "bytes around the uint8 output were written"
            outs.append(inner.reshape(ch, cw, 3))
        assert (wsbuf[:GUARD] == POISON_B).all() and (wsbuf[GUARD + need:] == POISON_B).all(), "bytes around the workspace were written"
    return outs


def check(ops, key, img, resized, window, name, pitch_pad=0, pillow=True):
    cy, cx, ch, cw = window
    want = np.ascontiguousarray(ref_resized(key, img, resized, name)[cy:cy + ch, cx:cx + cw])
    got_u8, got_f = run_both_outputs(ops, img, resized, window, name, pitch_pad)
    diff = int((got_u8.numpy() != want).sum())
    assert diff == 0, f"{diff} differing bytes of {want.size}"
    assert torch.equal(got_f, R.to_float(want))
    if pillow:
        try:
            from PIL import Image
        except ImportError:
            return
        res = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[name]
        pil = np.asarray(Image.fromarray(img).resize((resized[1], resized[0]), res))[cy:cy + ch, cx:cx + cw]
        assert int((got_u8.numpy() != pil).sum()) == 0, "differs from Pillow"


@pytest.mark.parametrize("name", R.FILTER_NAMES)
@pytest.mark.parametrize("hw,HW", R.RESIZE_CASES, ids=[f"{a[0]}x{a[1]}to{b[0]}x{b[1]}" for a, b in R.RESIZE_CASES])
def test_resize_is_pillow_byte_for_byte(ops, hw, HW, name):
    img = R.make_image(*hw, seed=hw[0] + hw[1])
    check(ops, ("rand", hw), img, HW, (0, 0, HW[0], HW[1]), name)


@pytest.mark.parametrize("name", R.FILTER_NAMES)
@pytest.mark.parametrize("resized,window", [((40, 33), (4, 0, 32, 32)), ((40, 35), (4, 2, 32, 32))], ids=["left0", "left2"])
def test_crop_window_equals_resize_then_crop(ops, resized, window, name):
    """Only the window is computed (and only the source rows its vertical taps reach); the bytes are those of resizing everything, then cropping."""
    from pixart_sigma_amd.data.images import center_crop_offset
    assert (center_crop_offset(resized[0], 32), center_crop_offset(resized[1], 32)) == window[:2]          # half to even: 0.5 -> 0, 1.5 -> 2
    img = R.make_image(57, 49, seed=3)
    check(ops, ("rand", (57, 49)), img, resized, window, name)


@pytest.mark.parametrize("name", R.FILTER_NAMES)
@pytest.mark.parametrize("form,hw,target", [("cover", (70, 45), (32, 32)), ("cover", (45, 70), (32, 40)), ("short_side", (45, 70), 24)], ids=["cover_tall", "cover_wide", "short_side"])
def test_transforms_end_to_end_from_transform_geometry(ops, form, hw, target, name):
    from pixart_sigma_amd.data.images import transform_geometry
    resized, window = transform_geometry(form, hw, target)
    assert (resized, window) == R.geometry(form, hw, target)
    img = R.make_image(*hw, seed=11)
    check(ops, ("rand11", hw), img, resized, window, name)


@pytest.mark.parametrize("name", R.FILTER_NAMES)
@pytest.mark.parametrize("value", [0, 255])
def test_constant_images_stay_constant(ops, value, name):
    img = np.full((37, 53, 3), value, dtype=np.uint8)
    check(ops, ("const", value), img, (16, 24), (0, 0, 16, 24), name)
    check(ops, ("const", value), img, (50, 70), (3, 5, 40, 60), name)


@pytest.mark.parametrize("name", R.FILTER_NAMES)
def test_source_row_pitch_larger_than_the_row(ops, name):
    img = R.make_image(37, 53, seed=90)
    check(ops, ("rand", (37, 53)), img, (16, 24), (0, 0, 16, 24), name, pitch_pad=13)
    check(ops, ("rand", (37, 53)), img, (37, 24), (2, 1, 30, 20), name, pitch_pad=13)      # horizontal pass only, straight to the output
    check(ops, ("rand", (37, 53)), img, (16, 53), (1, 7, 12, 40), name, pitch_pad=13)      # vertical pass only, straight from the source
    check(ops, ("rand", (37, 53)), img, (37, 53), (5, 6, 20, 33), name, pitch_pad=13)      # neither: the window copied


def test_image_preprocessor_batch_slots(ops):
    """ImagePreprocessor: numpy in, slot of a caller's batch out, tables cached; equal to the restatement's transform."""
    from pixart_sigma_amd.data.images import ImagePreprocessor
    pre = ImagePreprocessor("cover", "bicubic", "cuda")
    a, b = R.make_image(70, 45, seed=1), R.make_image(45, 70, seed=2)
    batch = torch.full((3, 3, 32, 32), POISON_F, device="cuda")
    pre(a, (32, 32), out=batch, slot=0)
    pre(b, (32, 32), out=batch, slot=2)
    n_tables = len(pre._tables)
    pre(a, (32, 32), out=batch, slot=0)
    assert len(pre._tables) == n_tables
    assert (batch[1] == POISON_F).all()
    assert torch.equal(batch[0].cpu(), R.to_float(R.transform_u8(a, "cover", "bicubic", (32, 32))))
    assert torch.equal(batch[2].cpu(), R.to_float(R.transform_u8(b, "cover", "bicubic", (32, 32))))
    assert np.array_equal(pre.to_u8(b, (32, 32)).cpu().numpy(), R.transform_u8(b, "cover", "bicubic", (32, 32)))


def _u8_inputs(shape, dtype):
    halfway = (2.0 * (torch.arange(256, dtype=torch.float64) + 0.5) / 255.0 - 1.0)           # (x + 1) / 2 * 255 = k + 0.5
    special = torch.cat([torch.tensor([-1.0, 1.0, -2.0, 2.0, -1.0000001, 1.0000001, 0.0], dtype=torch.float64), halfway])
    n = int(np.prod(shape))
    if n < special.numel():
        special = torch.cat([special[:7], halfway[::3]])
    g = torch.Generator().manual_seed(n)
    x = (torch.rand(n, generator=g, dtype=torch.float64) * 2.6 - 1.3)
    x[:special.numel()] = special
    return x[torch.randperm(n, generator=g)].reshape(shape).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (2, 3, 33, 130)], ids=["1x3x5x7", "2x3x33x130"])
def test_image_to_u8_is_save_image_arithmetic_in_fp32(ops, shape, dtype):
    x = _u8_inputs(shape, dtype)
    want = x.float().clamp(-1, 1).add(1).div(2).mul(255).add(0.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    B, _, H, W = shape
    buf = torch.full((B * H * W * 3 + 2 * GUARD,), POISON_B, dtype=torch.uint8, device="cuda")
    out = buf[GUARD:-GUARD].view(B, H, W, 3)
    ops.image_to_u8(x.cuda(), out=out)
    torch.cuda.synchronize()
    assert (buf[:GUARD] == POISON_B).all() and (buf[-GUARD:] == POISON_B).all()
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("ext", ["png", "jpg"])
def test_save_png_writes_the_bytes_of_image_to_u8(ops, tmp_path, ext):
    Image = pytest.importorskip("PIL.Image", reason="Pillow encodes the file")
    from pixart_sigma_amd.data.images import save_png
    x = _u8_inputs((1, 3, 33, 130), torch.float16).cuda()
    path = save_png(x[0], str(tmp_path / f"sample.{ext}"))
    with Image.open(path) as im:
        assert im.mode == "RGB" and im.size == (130, 33)
        if ext == "png":                                       # lossless: the file holds the kernel's bytes
            assert np.array_equal(np.asarray(im), ops.image_to_u8(x)[0].cpu().numpy())
