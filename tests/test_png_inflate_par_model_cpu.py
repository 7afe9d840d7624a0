"""The C host models of the subsequence decode (pf_pngd_scan_par_host, pf_pngd_inflate_par_host: csrc/png_host.h over the lane decoder of
csrc/png_inflate.h, the code the kernels of csrc/png_inflate_par.hip compile) against the sequential host model, zlib and the Python
model of tests/png_inflate_par_ref.py, for every file of the device tests at lanes of 64, 256 and 1024 bits.  No GPU call."""
import zlib

import numpy as np
import pytest
import torch

from patchfusion_amd import _lib
from patchfusion_amd import preprocess as P
from tests import png_decode_ref as R
from tests import png_inflate_par_ref as M
from tests.png_inflate_par_fake_ops import host_words

FILES = {**R.device_cases(), **{k: v[0] for k, v in R.load_cases().items()}}
LANE_BITS = (64, 256, 1024)
# photo-like content through zlib's own block splitting: the files on which the decode has to be parallel, not merely right
PHOTO_LIKE = ("pil_rgb_150x200_l6", "pil_rgb_150x200_l1", "pil_i16_37x53", "pil_rgba_37x53", "many_blocks_48x64", "composite_150x200", "paeth_130x200",
              "run_broken_by_filter0")


def _ptr(t):
    return t.data_ptr()


def _block_table(blocks):
    return torch.from_numpy(np.asarray(blocks, dtype=np.int64).astype(np.uint32).view(np.int32).reshape(-1, 4).copy())


def test_window_constant_is_the_library_s():
    assert _lib.load().pf_pngd_par_window() == P.PNG_PAR_WINDOW and P.PNG_PAR_WINDOW % 64 == 0


@pytest.mark.parametrize("name", sorted(FILES))
def test_host_model_equals_sequential_model_zlib_and_python_model(name):
    lib = _lib.load()
    T = lib.pf_pngd_par_window()
    idat = R.parse(FILES[name])["idat"]
    deflate, raw = idat[2:-4], zlib.decompress(idat)
    n = len(raw)
    words, nbits = host_words(deflate)
    cand = R.find_candidates(deflate) + [3, 5, max(nbits - 9, 0)]                   # and three places that are no block starts
    starts = torch.tensor(cand, dtype=torch.int64).to(torch.int32)
    seq = torch.zeros((len(cand), 4), dtype=torch.int32)
    assert lib.pf_pngd_scan_host(_ptr(words), words.numel(), nbits, _ptr(starts), len(cand), 1 << 21, n, _ptr(seq)) == 0
    fine = (seq[:, 3] & 255) == R.S_OK
    blocks = R.model(deflate, n)["blocks"]
    coded = torch.tensor([k[0] for k in blocks if k[1] != 0], dtype=torch.int64).to(torch.int32)
    table = _block_table(blocks)
    for bits in LANE_BITS:
        par, rounds = torch.zeros((len(cand), 4), dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
        assert lib.pf_pngd_scan_par_host(_ptr(words), words.numel(), nbits, _ptr(starts), len(cand), 1 << 21, n, bits, _ptr(par), _ptr(rounds)) == 0
        assert torch.equal(par[fine], seq[fine]), bits
        assert torch.equal(par[~fine][:, 0], seq[~fine][:, 0]) and bool(((par[~fine][:, 3] & 255) != R.S_OK).all()), bits
        # the rounds of the true blocks: scan and inflate passes agree with each other and with the Python model
        model_recs, model_rounds = M.rounds_of_true_blocks(deflate, n, bits, T)
        recs, scan_rounds = torch.zeros((max(len(coded), 1), 4), dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
        if len(coded):                                  # a file of stored blocks only has nothing to scan
            assert lib.pf_pngd_scan_par_host(_ptr(words), words.numel(), nbits, _ptr(coded), len(coded), 1 << 21, n, bits, _ptr(recs),
                                             _ptr(scan_rounds)) == 0
        for got, want in zip(recs.numpy().view(np.uint32).tolist(), model_recs):
            assert got == [want[0], want[1], want[2], want[3] | want[4] << 8] and want[3] == R.S_OK, (bits, got, want)
        lit, ref = torch.zeros(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.int32)
        status, inflate_rounds = torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
        assert lib.pf_pngd_inflate_par_host(_ptr(words), words.numel(), nbits, _ptr(table), len(blocks), n, bits, _ptr(lit), _ptr(ref), _ptr(status),
                                            _ptr(inflate_rounds)) == 0
        assert int(status[0]) == 0
        assert int(scan_rounds[0]) == int(inflate_rounds[0]) == model_rounds, (bits, int(scan_rounds[0]), int(inflate_rounds[0]), model_rounds)
        r = ref.numpy().astype(np.int64)
        assert (r <= np.arange(n)).all()
        for _ in range(max(n - 1, 0).bit_length() + 1):
            r = r[r]
        assert lit.numpy()[r].tobytes() == raw, bits
        if bits == 256 and name in PHOTO_LIKE:
            # deflate self-synchronises within a few hundred bits on such files, so a window settles in a handful of rounds (1-5 were
            # counted); 16 leaves room and still shows that the decode is parallel: the window's lanes number up to the library's window
            assert model_rounds <= 16, model_rounds


@pytest.mark.parametrize("name", ["far_match", "composite_150x200", "many_blocks_48x64", "pil_rgb_150x200_l1"])
def test_references_point_to_literals_or_strictly_earlier_lanes(name):
    """what pf_pngd_resolve's round count rests on: after the inflate pass ref[i] is a literal's place or a place in front of the lane
    range that holds i, so a chain of references visits a lane range at most once"""
    lib = _lib.load()
    T = lib.pf_pngd_par_window()
    idat = R.parse(FILES[name])["idat"]
    deflate, n = idat[2:-4], len(zlib.decompress(idat))
    words, nbits = host_words(deflate)
    blocks = R.model(deflate, n)["blocks"]
    b = R.Bits(deflate)
    for bits in (64, 256):
        lit, ref = torch.zeros(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.int32)
        status, rounds = torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
        table = _block_table(blocks)
        assert lib.pf_pngd_inflate_par_host(_ptr(words), words.numel(), nbits, _ptr(table), len(blocks), n, bits, _ptr(lit), _ptr(ref), _ptr(status),
                                            _ptr(rounds)) == 0 and int(status[0]) == 0
        range_start = np.zeros(n, dtype=np.int64)                                    # first output byte of the unit that holds each byte
        for start, kind, off, size in blocks:
            if kind == 0:
                range_start[off:off + size] = off
                continue
            lit_t, dist_t, p = R.read_codes(b, start)
            first, o, done = p // bits, off, False
            while not done:
                entry, lanes, _ = M.window_rounds(b, first, p, b.nbits, bits, T, lit_t, dist_t)
                for ex, count, eob, invalid in lanes:
                    assert not invalid
                    range_start[o:o + count] = o
                    o += count
                    if eob is not None:
                        done = True
                        break
                p, first = lanes[-1][0], first + T
            assert o == off + size
        r = ref.numpy().astype(np.int64)
        i = np.arange(n)
        assert ((r == i) | (r[r] == r) | (r < range_start)).all(), bits              # a literal's place (its own or another's), or earlier
