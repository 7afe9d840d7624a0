"""GPU checks of the run-match coding of the device PNG encoder (csrc/png_rle.hip, postprocess.encode_png(strategy='rle' | 'auto')).
Everything is exact: PIL decodes each file to the pixels that went in, zlib inflates the IDAT payload (which verifies the Adler-32) to
the filtered stream of the literal-only encoder, the device token histogram equals that of the numpy tokenizer in tests/png_rle_ref.py,
and on the real-size fixture the sizes are held against the literal-only file and against zlib's Z_RLE over the same stream."""
import zlib

import numpy as np
import pytest
import torch

from tests import png_ref as R
from tests import png_rle_ref as M
from tests import test_png_gpu as G

pytestmark = pytest.mark.gpu

RUN_CASES = M.run_length_cases()
_FILES = {}


def _rle_hist(ops, x, bgr=False):
    """device histograms of pass A' -> (literal counts 257, token counts 286, extra bits)"""
    ws = torch.empty(ops.png_rle_workspace(x, bgr)[0], dtype=torch.uint8, device="cuda")
    hist = torch.empty(ops.PNG_RLE_HIST_WORDS, dtype=torch.int32, device="cuda")
    ops.png_rle_filter_histogram(x, ws, hist, bgr)
    h = hist.cpu().numpy().view(np.uint32).astype(np.int64)
    assert h[543] == 0
    return h[:257], h[257:543], int(h[544]) | (int(h[545]) << 32)


def _check_histograms(ops, x_dev, stream, stride, bgr=False):
    rows = np.frombuffer(stream, dtype=np.uint8).reshape(-1, stride)
    nbands = (rows.shape[0] + G.BAND - 1) // G.BAND
    lit, tok, extra = _rle_hist(ops, x_dev, bgr)
    want_lit = np.bincount(rows.reshape(-1), minlength=257)
    want_lit[256] = nbands
    want_tok, want_extra = M.token_histogram(rows, nbands)
    assert np.array_equal(lit, want_lit)
    assert np.array_equal(tok, want_tok), np.flatnonzero(tok != want_tok)[:10]
    assert extra == want_extra


@pytest.mark.parametrize("fmt", G.FORMATS)
@pytest.mark.parametrize("shape", G.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_round_trip_rle_and_auto(shape, fmt):
    post, _ = G._mods()
    H, W = shape
    bgr = fmt.endswith("bgr")
    for content in G.CONTENTS + ["zero"]:
        x = G._array(fmt, "constant", H, W) * 0 if content == "zero" else G._array(fmt, content, H, W)
        dev = torch.from_numpy(x).cuda()
        want, _ = G._check_file(post.encode_png(dev, bgr=bgr, strategy="huffman"), x, bgr=bgr)
        for strategy in ("rle", "auto"):
            stream, _ = G._check_file(post.encode_png(dev, bgr=bgr, strategy=strategy), x, bgr=bgr)
            assert stream == want, (content, strategy)


@pytest.mark.parametrize("name", sorted(RUN_CASES))
def test_run_lengths_round_trip_and_token_histogram(name):
    post, ops = G._mods()
    x, want_runs = RUN_CASES[name]
    dev = torch.from_numpy(x).cuda()
    stride = x.shape[1] + 1
    for strategy in ("rle", "auto"):
        stream, idat = G._check_file(post.encode_png(dev, strategy=strategy), x)
        got_runs = M.stream_run_lengths(stream, stride)
        assert stream[0] == 1 and all(n in got_runs for n in want_runs), (want_runs, got_runs[:40])
    if max(want_runs) >= 258:                                                # a long run is a few matches against hundreds of literals
        assert len(idat) < len(R.idat_payload(post.encode_png(dev)))
    _check_histograms(ops, dev, stream, stride)


def test_token_histogram_of_noise_rows_in_four_channels():
    post, ops = G._mods()
    x = G._array("u8c4", "constant_with_noise_rows", 129, 1031)
    dev = torch.from_numpy(x).cuda()
    stream, _ = G._check_file(post.encode_png(dev, strategy="rle"), x)
    _check_histograms(ops, dev, stream, 1 + 1031 * 4)
    xb = G._array("u8c3_bgr", "hramp", 37, 53)
    stream, _ = G._check_file(post.encode_png(torch.from_numpy(xb).cuda(), bgr=True, strategy="rle"), xb, bgr=True)
    _check_histograms(ops, torch.from_numpy(xb).cuda(), stream, 1 + 53 * 3, bgr=True)


def test_default_strategy_gives_the_literal_only_file_and_unknown_strategies_raise():
    post, _ = G._mods()
    x = torch.from_numpy(G._array("u8c3", "hramp", 37, 53)).cuda()
    assert post.encode_png(x) == post.encode_png(x, strategy="huffman")
    with pytest.raises(ValueError):
        post.encode_png(x, strategy="lz77")


def _files(key):
    """the three files of one image of the real-size fixture of tests/test_png_gpu.py: made once, left unchanged"""
    if key not in _FILES:
        post, _ = G._mods()
        x, png, bgr = G._real()[key]
        dev = torch.from_numpy(x).cuda()
        _FILES[key] = {"huffman": png, "rle": post.encode_png(dev, bgr=bgr, strategy="rle"), "auto": post.encode_png(dev, bgr=bgr, strategy="auto")}
    return _FILES[key]


@pytest.mark.parametrize("key", ["u16", "bgr"])
def test_real_size_sizes_and_the_choice_of_auto(key):
    """The bounds are those of the CPU model with one table per image (0.69 of the literal-only IDAT, 1.02 of zlib Z_RLE) with room for
    the per-band headers and the 14-bit limit.  Measured on the MI355X, IDAT bytes: colour 'rle' 1 065 268 against 'huffman' 1 549 032
    (0.6877) and Z_RLE 1 043 074 (1.0213); uint16 'rle' 1 465 476 against 'huffman' 1 371 509 (1.0685), so 'auto' keeps the literals."""
    post, _ = G._mods()
    x, png, bgr = G._real()[key]
    files = _files(key)
    assert files["huffman"] == png == post.encode_png(torch.from_numpy(x).cuda(), bgr=bgr)
    want, _ = G._check_file(png, x, bgr=bgr)
    idat = {}
    for s in ("rle", "auto"):
        stream, idat[s] = G._check_file(files[s], x, bgr=bgr)
        assert stream == want
    idat["huffman"] = R.idat_payload(png)
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
    ref = len(c.compress(want) + c.flush())
    nbands = (x.shape[0] + G.BAND - 1) // G.BAND
    print(f"\npng rle {key}: IDAT huffman {len(idat['huffman'])} rle {len(idat['rle'])} auto {len(idat['auto'])} zlib Z_RLE {ref} "
          f"rle/huffman {len(idat['rle']) / len(idat['huffman']):.4f} rle/Z_RLE {len(idat['rle']) / ref:.4f} "
          f"files {len(files['huffman'])} {len(files['rle'])} {len(files['auto'])}")
    assert len(files["auto"]) <= min(len(files["rle"]), len(files["huffman"])) + nbands
    if key == "bgr":
        assert len(idat["rle"]) <= 0.75 * len(idat["huffman"]), (len(idat["rle"]), len(idat["huffman"]))
        assert len(idat["rle"]) <= 1.05 * ref, (len(idat["rle"]), ref)
        assert files["auto"] == files["rle"]
    else:
        assert files["auto"] == files["huffman"]


def test_save_prediction_passes_the_strategy_through(tmp_path):
    post, _ = G._mods()
    d = torch.zeros(1, 1, 40, 64, device="cuda") + 3.0
    d[..., :, 32:] = 5.0
    sizes = {}
    for s in ("huffman", "rle", "auto"):
        colour_path, u16_path = post.save_prediction(d, str(tmp_path), f"img_{s}", png_strategy=s)
        files = [open(p, "rb").read() for p in (colour_path, u16_path)]
        assert files[0] == post.encode_png(post.colorize(d, cmap="magma_r", layout="bgr"), bgr=True, strategy=s)
        assert files[1] == post.encode_png(post.depth_to_uint16(d), strategy=s)
        sizes[s] = [len(f) for f in files]
    assert sizes["rle"][0] < sizes["huffman"][0] and sizes["auto"] == [min(a, b) for a, b in zip(sizes["rle"], sizes["huffman"])]
