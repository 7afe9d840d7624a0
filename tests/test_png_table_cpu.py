"""CPU checks of the host step of the PNG encoder (csrc/png_huff.h, exported as pf_png_build_table): the code it builds is a complete
prefix code of at most 15 bits, and a deflate block assembled from its header and codes by the slow bit writer of tests/png_ref.py is
accepted by zlib and inflates to the bytes that went in.  The second test runs the same header stand-alone under the host sanitizers."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import zlib

import patchfusion_amd._lib as L
from tests import png_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HISTS = R.histograms()


@pytest.mark.parametrize("name", sorted(HISTS))
def test_table_is_a_complete_limited_prefix_code_and_zlib_inflates_it(name):
    lib = L.load()
    hist = HISTS[name]
    table = R.build_table(lib, hist)
    lens = R.code_lengths(table)
    used = [s for s in range(R.NSYM) if hist[s]]
    assert all(1 <= lens[s] <= 15 for s in used), [(s, lens[s]) for s in used if not 1 <= lens[s] <= 15]
    assert lens[R.EOB] >= 1
    assert all(0 <= n <= 15 for n in lens)
    if len(used) >= 2:
        assert sum(Fraction(1, 2 ** n) for n in lens if n) == 1
    assert 0 < int(table[R.NSYM]) <= 2048
    # more frequent symbols never get longer codes
    order = sorted(used, key=lambda s: int(hist[s]))
    assert all(lens[a] >= lens[b] for a, b in zip(order, order[1:]) if hist[a] < hist[b])
    # a short byte string over the used literals, every one of them at least once
    lits = [s for s in used if s != R.EOB]
    rng = np.random.default_rng(7)
    data = bytes(lits + [lits[i] for i in rng.integers(0, len(lits), 200)])
    assert zlib.decompress(R.deflate_with_table(table, data), wbits=-15) == data
    assert zlib.decompress(R.deflate_with_table(table, b""), wbits=-15) == b""


def test_fibonacci_histogram_needs_the_limit():
    """the unlimited Huffman code of the Fibonacci histogram is deeper than 15: the limiter is what this case is for"""
    lens = R.code_lengths(R.build_table(L.load(), HISTS["fibonacci"]))
    assert max(lens) == 15 and sum(1 for n in lens if n == 15) > 2


def test_missing_end_of_block_count_still_gets_a_code():
    hist = HISTS["geometric"].copy()
    hist[R.EOB] = 0
    assert R.code_lengths(R.build_table(L.load(), hist))[R.EOB] >= 1


def test_null_pointers_are_an_argument_error():
    assert L.load().pf_png_build_table(None, None) == 1


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_png_huff_header_stand_alone_under_host_sanitizers(tmp_path):
    exe = tmp_path / "png_huff_main"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                        "-I", os.path.join(ROOT, "patchfusion_amd", "csrc"), os.path.join(ROOT, "tests", "host", "png_huff_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "5 histograms ok" in r.stdout, r.stdout
