"""GPU checks of the device PNG encoder (csrc/png.hip, postprocess.encode_png / save_prediction).  PNG is lossless, so every check is
exact: PIL decodes the file to the pixels that went in, zlib inflates the IDAT payload (which verifies the Adler-32 combined from the
band partial sums) to a filtered stream of the right length whose filter bytes are None / Sub / Up / Paeth.  Sizes are checked on the
real-size fixture so that an encoder of stored blocks cannot pass."""
import io
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from tests import png_ref as R

pytestmark = pytest.mark.gpu

BAND = 8                                     # PF_PNG_BAND_ROWS
SHAPES = [(1, 1), (1, 300), (300, 1), (37, 53), (64, 64), (129, 1031), (BAND * 3 + 1, 70)]
FORMATS = ["u8c1", "u8c3", "u8c4", "u8c3_bgr", "u16"]
CONTENTS = ["constant", "hramp", "vramp", "noise", "constant_with_noise_rows"]

# IDAT size over zlib Z_HUFFMAN_ONLY (level 6, memLevel 9) on the same filtered stream, measured on the MI355X on the real-size fixture
# (DESIGN 9b); the encoder has one table per image and repeats its header in every band, zlib re-tunes its table per block.
MEASURED_RATIO = {"u16": 1.0055, "bgr": 1.0042}
_REAL = {}


def _mods():
    from patchfusion_amd import postprocess as post
    from patchfusion_amd.hip_ops import ops
    return post, ops


def _array(fmt, content, H, W):
    ch = {"u8c1": 1, "u8c3": 3, "u8c4": 4, "u8c3_bgr": 3, "u16": 1}[fmt]
    dtype, top = (np.uint16, 65536) if fmt == "u16" else (np.uint8, 256)
    rng = np.random.default_rng(H * 100003 + W * 17 + ch)
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(ch), indexing="ij")
    step = 259 if fmt == "u16" else 3                       # the 16-bit ramps move both bytes of a sample
    if content == "constant":
        a = np.full((H, W, ch), 7 if fmt != "u16" else 0x1207)
    elif content == "hramp":
        a = x * step + c * 11
    elif content == "vramp":
        a = y * step + c * 5
    elif content == "noise":
        a = rng.integers(0, top, (H, W, ch))
    else:
        # Slot-bound case.  Almost every byte of the filtered stream is 0 and takes the 1-bit code, so the image-wide table gives the noise
        # bytes of the first band its longest codes (8 to 10 bits at 129 x 1031): that band grows beyond its raw size.  This exercises the
        # slot bound of 15 bits per stream byte + header + flush; a slot sized for the raw band would be overrun.
        a = np.zeros((H, W, ch), dtype=np.int64)
        a[:BAND] = rng.integers(0, top, a[:BAND].shape)
    a = (a % top).astype(dtype)
    return np.ascontiguousarray(a if ch > 1 else a[..., 0])


def _check_file(png, x, bgr=False):
    """PIL round trip + IDAT checks; -> (filtered stream, IDAT bytes)"""
    H, W = x.shape[:2]
    bpp = x.dtype.itemsize * (x.shape[2] if x.ndim == 3 else 1)
    im = Image.open(io.BytesIO(png))
    im.load()
    got = np.asarray(im)
    want = x[..., ::-1] if bgr else x
    if x.dtype == np.uint16:
        got = got.astype(np.uint16)
        assert im.mode.startswith("I;16"), im.mode
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, im.mode)
    assert np.array_equal(got, want)
    idat = R.idat_payload(png)
    stream = zlib.decompress(idat)                          # checks the Adler-32
    assert len(stream) == H * (1 + W * bpp)
    filters = set(stream[::1 + W * bpp])
    assert filters <= {0, 1, 2, 4}, filters
    return stream, idat


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_round_trip(shape, fmt):
    post, _ = _mods()
    H, W = shape
    for content in CONTENTS:
        x = _array(fmt, content, H, W)
        png = post.encode_png(torch.from_numpy(x).cuda(), bgr=fmt.endswith("bgr"))
        _check_file(png, x, bgr=fmt.endswith("bgr"))


def test_bgr_with_alpha_and_argument_errors():
    post, ops = _mods()
    x = _array("u8c4", "noise", 19, 23)
    png = post.encode_png(torch.from_numpy(x).cuda(), bgr=True)
    got = np.asarray(Image.open(io.BytesIO(png)))
    assert np.array_equal(got, x[..., [2, 1, 0, 3]])
    with pytest.raises(ValueError):
        post.encode_png(torch.zeros(4, 4, dtype=torch.uint8).cuda(), bgr=True)
    with pytest.raises(ValueError):
        post.encode_png(torch.zeros(4, 4, 2, dtype=torch.uint8).cuda())
    with pytest.raises(ValueError):
        post.encode_png(torch.zeros(4, 4).cuda())


def test_band_of_rare_bytes_grows_beyond_its_raw_size_inside_its_slot():
    """the slot bound at work (see _array): band 0 holds the noise rows, coded with a table tuned to zeros"""
    _, ops = _mods()
    H, W = 129, 1031
    x = torch.from_numpy(_array("u8c4", "constant_with_noise_rows", H, W)).cuda()
    ws_bytes, out_bytes, nbands = ops.png_workspace(x)
    assert nbands == (H + BAND - 1) // BAND
    slot = out_bytes // nbands
    raw_band = BAND * (1 + W * 4)
    assert slot >= 256 + (raw_band + 1) * 15 // 8 + 6          # header + 15 bits per byte and end-of-block + flush
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    hist = torch.empty(257, dtype=torch.int32, device="cuda")
    ops.png_filter_histogram(x, ws, hist)
    h = hist.cpu().numpy()
    assert int(h[:256].sum()) == H * (1 + W * 4) and int(h[256]) == nbands
    table = ops.png_build_table(h)
    out = torch.empty(out_bytes, dtype=torch.uint8, device="cuda")
    meta = torch.empty(2 + 3 * nbands, dtype=torch.int32, device="cuda")
    ops.png_encode(x, torch.from_numpy(table.view(np.int32)).cuda(), ws, out, meta)
    m = meta.cpu().numpy().view(np.uint32)
    sizes = m[2::3]
    lens = R.code_lengths(table)
    assert lens[0] == 1 and max(lens) > 8                       # zeros are cheap, noise bytes cost more than their 8 bits
    assert raw_band < sizes[0] <= slot, (raw_band, int(sizes[0]), slot)
    assert int(sizes.sum()) == int(m[0]) and max(sizes[1:]) < raw_band // 4


def _real():
    """the m1-sized fixture (seeded numpy), both device images and their files: made once, left unchanged"""
    if not _REAL:
        post, _ = _mods()
        H, W = 1568, 2072
        y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        d = 5 + 3 * np.sin(x / 300) * np.cos(y / 200) + 0.002 * np.random.default_rng(0).standard_normal((H, W))
        dev = torch.from_numpy(d.astype(np.float32)).cuda()
        for key, img, bgr in (("u16", post.depth_to_uint16(dev), False), ("bgr", post.colorize(dev, cmap="magma_r", layout="bgr"), True)):
            png = post.encode_png(img, bgr=bgr)
            _REAL[key] = (img.cpu().numpy(), png, bgr)
    return _REAL


@pytest.mark.parametrize("key", ["u16", "bgr"])
def test_real_size_round_trip_and_size(key):
    x, png, bgr = _real()[key]
    assert x.shape[:2] == (1568, 2072) and x.dtype == (np.uint16 if key == "u16" else np.uint8)
    stream, idat = _check_file(png, x, bgr=bgr)
    raw = len(stream)
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_HUFFMAN_ONLY)
    ref = len(c.compress(stream) + c.flush())
    stride = raw // x.shape[0]
    filters = np.bincount(np.frombuffer(stream, dtype=np.uint8)[::stride], minlength=5)
    print(f"\npng {key}: raw {raw} IDAT {len(idat)} ({len(idat) / raw:.4f} of raw) zlib huffman-only {ref} ratio {len(idat) / ref:.4f} "
          f"rows per filter None/Sub/Up/Paeth {filters[0]}/{filters[1]}/{filters[2]}/{filters[4]}")
    assert len(idat) < 0.5 * raw
    assert filters[1] + filters[2] + filters[4] >= 1               # the smooth fixture does not leave every row unfiltered
    assert len(idat) <= MEASURED_RATIO[key] * 1.05 * ref, (len(idat), ref)


@pytest.mark.parametrize("gray_scale", [False, True])
def test_save_prediction_files_decode_to_the_device_images(tmp_path, gray_scale):
    post, _ = _mods()
    rng = np.random.default_rng(11)
    yy, xx = np.meshgrid(np.arange(97.0), np.arange(131.0), indexing="ij")
    d = torch.from_numpy((2 + np.sin(xx / 17) * np.cos(yy / 13) + 0.05 * rng.standard_normal((97, 131))).astype(np.float32)).cuda()
    result = d[None, None]                                         # the model's [1,1,H,W]
    colour_path, u16_path = post.save_prediction(result, str(tmp_path), "img_007", gray_scale=gray_scale)
    assert colour_path == str(tmp_path / "img_007.png") and u16_path == str(tmp_path / "img_007_uint16.png")
    want_rgb = post.colorize(result, cmap="gray_r" if gray_scale else "magma_r")[..., :3].cpu().numpy()
    want_u16 = post.depth_to_uint16(result).cpu().numpy()
    got_rgb = np.asarray(Image.open(colour_path))
    got_u16 = np.asarray(Image.open(u16_path)).astype(np.uint16)
    assert got_rgb.shape == want_rgb.shape and np.array_equal(got_rgb, want_rgb)
    assert got_u16.shape == want_u16.shape and np.array_equal(got_u16, want_u16)
    assert len(np.unique(want_rgb.reshape(-1, 3), axis=0)) > 16 and want_u16.max() > want_u16.min()
