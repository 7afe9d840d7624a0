"""CPU checks of the run-match coding of the PNG encoder: the host table builder (csrc/png_huff.h, exported as pf_png_rle_build_table)
gives a complete prefix code of at most 14 bits over 286 symbols and a header zlib accepts, with matches of every length base; the
numpy tokenizer of tests/png_rle_ref.py, the model the kernels are held to on the GPU, inflates to the stream it was given; and the
host side of postprocess.encode_png(strategy=...) -- table hand-over, cost comparison of 'auto', Adler-32, container -- gives files
PIL decodes, with numpy standing in for the kernels.  The builder also runs stand-alone under the host sanitizers."""
import io
import os
import shutil
import subprocess
import zlib
from fractions import Fraction

import numpy as np
import pytest
import torch
from PIL import Image

import patchfusion_amd._lib as L
from patchfusion_amd import postprocess as post
from tests import png_ref as R
from tests import png_rle_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HISTS = M.histograms()
CASES = M.run_length_cases()


@pytest.mark.parametrize("name", sorted(HISTS))
def test_rle_table_is_a_complete_limited_prefix_code_and_zlib_inflates_matches_of_every_base(name):
    hist = HISTS[name]
    table = M.build_table(L.load(), hist)
    lens = M.code_lengths(table)
    used = [s for s in range(M.NSYM) if hist[s]]
    assert all(1 <= lens[s] <= M.MAX_BITS for s in used), [(s, lens[s]) for s in used if not 1 <= lens[s] <= M.MAX_BITS]
    assert lens[M.EOB] >= 1 and all(0 <= n <= M.MAX_BITS for n in lens)
    if len(used) >= 2:
        assert sum(Fraction(1, 2 ** n) for n in lens if n) == 1
    assert 0 < int(table[M.HDR_BITS_WORD]) <= M.HDR_BITS_BOUND <= M.HDR_BYTES * 8
    assert int(table[M.DIST_WORD]) == 1 << 16
    assert [int(t) & 0xffff for t in table[M.LEN_WORD0:M.LEN_WORD0 + 29]] == M.LENGTH_BASE
    assert [int(t) >> 16 for t in table[M.LEN_WORD0:M.LEN_WORD0 + 29]] == M.LENGTH_EXTRA
    order = sorted(used, key=lambda s: int(hist[s]))
    assert all(lens[a] >= lens[b] for a, b in zip(order, order[1:]) if hist[a] < hist[b])
    # every used literal, each followed by a match; the match lengths go through every length base and the length before the next
    lits = [s for s in used if s < 256]
    matches = [m for m in M.EVERY_BASE if lens[M.length_symbol(m)[0]]]
    assert matches == M.EVERY_BASE or name.endswith("no_matches") or name == "geometric_short_lengths"
    toks, want = [], bytearray()
    for i, v in enumerate(lits * 3):
        toks.append(v)
        want.append(v)
        if matches:
            m = matches[i % len(matches)]
            toks.append((m,))
            want += bytes([v]) * m
    assert M.expand(toks) == bytes(want)
    assert zlib.decompress(M.deflate_with_table(table, toks), wbits=-15) == bytes(want)
    assert zlib.decompress(M.deflate_with_table(table, []), wbits=-15) == b""


def test_fibonacci_histogram_needs_the_14_bit_limit_and_the_literal_table_is_unchanged():
    lens = M.code_lengths(M.build_table(L.load(), HISTS["fibonacci"]))
    assert max(lens) == 14 and sum(1 for n in lens if n == 14) > 2
    assert max(R.code_lengths(R.build_table(L.load(), R.histograms()["fibonacci"]))) == 15


def test_rle_builder_null_pointers_are_an_argument_error():
    assert L.load().pf_png_rle_build_table(None, None) == 1


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_rle_table_builder_stand_alone_under_host_sanitizers(tmp_path):
    exe = tmp_path / "png_rle_huff_main"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                        "-I", os.path.join(ROOT, "patchfusion_amd", "csrc"), os.path.join(ROOT, "tests", "host", "png_rle_huff_main.cpp"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "7 histograms ok" in r.stdout, r.stdout


def _stream_rows(x):
    """the filtered stream rows of a u8 image under the stand-in's filter choice (the heuristic of the kernels)"""
    ops = M.FakeRleOps()
    ops.png_filter_histogram(torch.from_numpy(x), torch.zeros(x.shape[0], dtype=torch.uint8), torch.zeros(257, dtype=torch.int32))
    return ops.streams


@pytest.mark.parametrize("name", sorted(CASES))
def test_tokenizer_inflates_to_the_stream_and_the_cases_hold_the_runs_they_are_named_for(name):
    x, want_runs = CASES[name]
    rows = _stream_rows(x)
    stream = b"".join(r.tobytes() for r in rows)
    got_runs = M.stream_run_lengths(stream, x.shape[1] + 1)
    assert all(n in got_runs for n in want_runs), (want_runs, got_runs[:40])
    assert rows[0][0] == 1                                            # Sub: the stream is the residuals the case was built from
    if name == "run_from_the_filter_byte":
        assert got_runs[0] == 8
    if name == "run_to_the_last_byte":
        assert got_runs[-1] == 40
    toks = M.tokens(rows)
    assert M.expand(toks) == stream
    nbands = (x.shape[0] + 7) // 8
    hist, extra = M.token_histogram(rows, nbands)
    count = np.zeros(M.NSYM, dtype=np.int64)
    for t in toks:
        count[M.length_symbol(t[0])[0] if isinstance(t, tuple) else t] += 1
    count[M.EOB] = nbands
    assert np.array_equal(hist, count)
    assert extra == sum(M.length_symbol(t[0])[1] for t in toks if isinstance(t, tuple))
    assert all(3 <= t[0] <= 258 for t in toks if isinstance(t, tuple))
    table = M.build_table(L.load(), hist)
    assert zlib.decompress(M.deflate_with_table(table, toks), wbits=-15) == stream


def test_tokens_of_the_lengths_around_the_chunk_of_258():
    """a run of L bytes: one literal, then L - 1 bytes in chunks of 258; 1 or 2 trailing bytes are literals"""
    def t(n):
        return M.row_tokens(np.full(n, 7, dtype=np.uint8))
    assert t(1) == [7] and t(2) == [7, 7] and t(3) == [7, 7, 7] and t(4) == [7, (3,)]
    assert t(259) == [7, (258,)] and t(260) == [7, (258,), 7] and t(261) == [7, (258,), 7, 7] and t(262) == [7, (258,), (3,)]
    assert t(517) == [7, (258,), (258,)] and t(519) == [7, (258,), (258,), 7, 7] and t(520) == [7, (258,), (258,), (3,)]
    two_rows = M.tokens([np.zeros(5, dtype=np.uint8), np.zeros(5, dtype=np.uint8)])
    assert two_rows == [0, (4,), 0, (4,)]                              # a run never crosses a row


IMAGES = [("u8c1_runs", (9, 40)), ("u8c3_bgr_smooth", (10, 12)), ("u8c4_zero", (3, 7)), ("u16_noise", (11, 9)), ("u8c1_noise", (17, 5)), ("u16_one_pixel", (1, 1))]


def _image(kind, H, W):
    rng = np.random.default_rng(H * 31 + W)
    if kind == "u8c1_runs":
        return np.repeat(rng.integers(0, 256, (H, W // 8), dtype=np.uint8), 8, axis=1)
    if kind == "u8c3_bgr_smooth":
        y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(3), indexing="ij")
        return ((x // 4) * 40 + (y // 5) * 3 + c).astype(np.uint8)
    if kind == "u8c4_zero":
        return np.zeros((H, W, 4), dtype=np.uint8)
    if kind == "u16_noise":
        return rng.integers(0, 65536, (H, W), dtype=np.uint16)
    if kind == "u8c1_noise":
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    return np.zeros((H, W), dtype=np.uint16)


@pytest.mark.parametrize("kind,shape", IMAGES, ids=[k for k, _ in IMAGES])
def test_encode_png_strategies_with_stand_in_kernels(kind, shape):
    a = _image(kind, *shape)
    bgr = "bgr" in kind
    files = {s: post.encode_png(torch.from_numpy(a), bgr=bgr, strategy=s, ops=M.FakeRleOps()) for s in ("huffman", "rle", "auto")}
    assert files["huffman"] == post.encode_png(torch.from_numpy(a), bgr=bgr, ops=M.FakeRleOps())        # the default
    want = a[..., ::-1] if bgr else a
    streams = set()
    for s, png in files.items():
        got = np.asarray(Image.open(io.BytesIO(png)))
        assert got.shape == want.shape and np.array_equal(got.astype(want.dtype), want), s
        streams.add(zlib.decompress(R.idat_payload(png)))                                              # checks the Adler-32
    assert len(streams) == 1 and len(streams.pop()) == a.shape[0] * (1 + a[0].size * a.dtype.itemsize)
    nbands = (a.shape[0] + 7) // 8
    sizes = {s: len(f) for s, f in files.items()}
    assert files["auto"] in (files["rle"], files["huffman"])
    assert sizes["auto"] <= min(sizes["rle"], sizes["huffman"]) + nbands, sizes
    if "zero" in kind or "runs" in kind:
        assert files["auto"] == files["rle"] and sizes["rle"] < sizes["huffman"], sizes
    if "noise" in kind:
        assert files["auto"] == files["huffman"], sizes


def test_unknown_strategy_is_a_value_error():
    with pytest.raises(ValueError):
        post.encode_png(torch.zeros(4, 4, dtype=torch.uint8), strategy="lz77", ops=M.FakeRleOps())
    with pytest.raises(ValueError):
        post.encode_png(torch.zeros(4, 4, dtype=torch.uint8), strategy=None, ops=M.FakeRleOps())


def test_cost_of_auto_is_the_size_of_the_blocks():
    """png_cost_bits against the slow bit writer: one band, so the only slack is the padding to a byte"""
    x = _image("u8c1_runs", 8, 64)
    rows = _stream_rows(x)
    hist, extra = M.token_histogram(rows, 1)
    table = M.build_table(L.load(), hist)
    w = R.BitWriter()
    M.put_block(w, table, M.tokens(rows))
    bits = post.png_cost_bits(hist, table, 286, table[M.HDR_BITS_WORD], 1, extra)
    assert bits == len(w.bits) + 3 + 32
    lit = np.bincount(np.concatenate(rows), minlength=257)
    lit[256] = 1
    ltable = R.build_table(L.load(), lit)
    lbits = post.png_cost_bits(lit, ltable, 257, ltable[R.NSYM], 1)
    assert (lbits - 32 + 7) // 8 + 4 == len(R.deflate_with_table(ltable, np.concatenate(rows)))        # block + 3 bits, padded, + LEN / NLEN
