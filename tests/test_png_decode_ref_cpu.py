"""tests/png_decode_ref.py against PIL and against zlib: the reference decoder equals PIL on every file PIL can write (live and from the
committed fixture), the writer round-trips all 15 colour-type / depth pairs, and the model of the device algorithm reproduces
zlib.decompress on every case the device tests run, inside the default caps."""
import io
import zlib

import numpy as np
import pytest

from tests import png_decode_ref as R

FIXTURE = R.load_cases()
DEVICE = R.device_cases()


def _pil(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    if im.mode == "P":
        im = im.convert("RGB")
    a = np.asarray(im)
    if a.dtype == bool:
        a = a.astype(np.uint8) * 255
    return a.astype(np.uint16) if a.dtype.itemsize > 1 else a


@pytest.mark.parametrize("name", sorted(FIXTURE))
def test_decoder_equals_the_fixture(name):
    png, exp = FIXTURE[name]
    got = R.decode(png)
    assert got.dtype == exp.dtype and np.array_equal(got, exp)


def test_decoder_equals_pil_live():
    pytest.importorskip("PIL")
    n = 0
    for name, (png, exp) in FIXTURE.items():
        if name.startswith("pil_"):
            assert np.array_equal(_pil(png), exp), name
            n += 1
    for name, png in DEVICE.items():
        h = R.parse(png)
        if h["depth"] == 8 or (h["color_type"], h["depth"]) in ((0, 1), (0, 16), (3, 1), (3, 2), (3, 4)):     # what PIL decodes losslessly
            assert np.array_equal(_pil(png), R.decode(png)), name
            n += 1
    assert n >= 30


@pytest.mark.parametrize("ct,depth", R.PAIRS)
def test_writer_decoder_round_trip(ct, depth):
    rng = np.random.default_rng(ct * 17 + depth)
    H, W, ch = 11, 19, R.CHANNELS[ct]
    pal = R.palette_of(1 << depth) if ct == 3 else None
    s = rng.integers(0, 1 << depth, (H, W, ch))
    got = R.decode(R.write_png(s, ct, depth, filters=(4, 3, 2, 1, 0), palette=pal, idat_split=[7, 40]))
    if ct == 3:
        exp = pal[s[..., 0]]
    elif depth < 8:
        exp = (s[..., 0] * (255 // ((1 << depth) - 1))).astype(np.uint8)
    else:
        exp = s.astype(np.uint16 if depth == 16 else np.uint8)
        exp = exp[..., 0] if ch == 1 else exp
    assert got.dtype == exp.dtype and np.array_equal(got, exp)


MODEL_FILES = {**DEVICE, **{k: v[0] for k, v in FIXTURE.items() if "150x200" in k or k.startswith("encode_png")}}


@pytest.mark.parametrize("name", sorted(MODEL_FILES))
def test_model_equals_zlib_inside_the_default_caps(name):
    z = R.parse(MODEL_FILES[name])["idat"]
    raw = zlib.decompress(z)
    m = R.model(z[2:], len(raw))
    assert m["fallback"] is None and m["out"] == raw
    assert set(b[0] for b in m["blocks"] if b[1] == 2) <= set(m["candidates"])         # candidates hold every true dynamic start
    assert m["jump_rounds_used"] <= m["jump_rounds"] - 1                               # ceil(log2(blocks)) rounds suffice; one more is run
    assert 1 <= m["chain_rounds"] <= 8


def test_the_cases_are_what_their_names_say():
    kinds = lambda name: [b[1] for b in R.model(R.parse(DEVICE[name])["idat"][2:], len(zlib.decompress(R.parse(DEVICE[name])["idat"])))["blocks"]]  # noqa: E731
    many = kinds("many_blocks_48x64")
    assert many.count(2) >= 24
    comp = [k for k in kinds("composite_150x200")]
    first_fixed, stored = comp.index(1), [i for i, k in enumerate(comp) if k == 0]
    assert comp[0] == 2 and comp[-1] == 2 and comp[first_fixed - 1] == 0 and any(i > first_fixed for i in stored)
    z = R.parse(DEVICE["composite_150x200"])["idat"]
    m = R.model(z[2:], len(zlib.decompress(z)))
    assert m["chain_rounds"] >= 2
    assert any(n > 0 for s, k, o, n in m["blocks"] if k == 0) and any(n == 0 for s, k, o, n in m["blocks"] if k == 0)
    assert R.model(z[2:], len(zlib.decompress(z)), max_chain_rounds=0)["fallback"] == "rounds"
    assert kinds("far_match") == [1] and kinds("constant_64x64") == [2] and kinds("ramp_96x1024") == [2]
    png, _ = FIXTURE["pil_rgb_150x200_l6"]
    z = R.parse(png)["idat"]
    assert R.model(z[2:], len(zlib.decompress(z)), max_block_bits=1024)["fallback"] == "bits"


def test_cross_block_references_need_jumps():
    z = R.parse(DEVICE["many_blocks_48x64"])["idat"]
    m = R.model(z[2:], len(zlib.decompress(z)))
    assert m["jump_rounds_used"] >= 2 and m["jump_rounds"] == (len(m["blocks"]) - 1).bit_length() + 1
