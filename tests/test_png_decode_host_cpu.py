"""The host code of the PNG decoder through the C ABI (csrc/png_host.h, csrc/png_inflate.h; no GPU call) against tests/png_decode_ref.py:
the chunk parser against the Python one, the finder's register-only header test against the full header reader, the scan records, and the
sequential restatement of the whole device algorithm against zlib."""
import ctypes as C
import zlib

import numpy as np
import pytest

from patchfusion_amd import _lib
from patchfusion_amd import preprocess as P
from tests import png_decode_ref as R

FILES = {**R.device_cases(), **{k: v[0] for k, v in R.load_cases().items()}}


@pytest.mark.parametrize("name", sorted(FILES))
def test_c_parser_equals_the_python_parser(name):
    png = FILES[name]
    host, ref = P.PngHost(png, check_idat_crc=True), R.parse(png)
    h = host.header
    for k in ("width", "height", "depth", "color_type", "channels", "bpp", "rowbytes"):
        assert getattr(h, k) == ref[k], k
    assert bool(h.has_trns) == ref["has_trns"] and h.inflated_bytes == ref["height"] * (1 + ref["rowbytes"])
    assert host.deflate.tobytes() == ref["idat"][2:] and h.compressed_bytes == len(ref["idat"])
    if ref["palette"] is not None:
        assert h.plte_entries == len(ref["palette"]) and bytes(h.palette)[:3 * h.plte_entries] == ref["palette"].tobytes()
    raw, adler = host.inflate()
    assert raw.tobytes() == zlib.decompress(ref["idat"]) and adler == zlib.adler32(raw.tobytes())


@pytest.mark.parametrize("name", ["many_blocks_48x64", "composite_150x200", "far_match", "pil_rgb_150x200_l6", "pil_rgb_150x200_l1", "pil_i16_37x53",
                                  "encode_png_rgb_24x40", "fmt_ct2_d8_w13", "one_pixel"])
def test_finder_scan_and_model_equal_the_reference(name):
    lib = _lib.load()
    host = P.PngHost(FILES[name])
    words, nbits, expected = host.words(), 8 * host.deflate.size, host.header.inflated_bytes
    want = R.find_candidates(host.deflate.tobytes())
    got, count = np.zeros(len(want) + 8, dtype=np.uint32), C.c_long()
    assert lib.pf_pngd_find_host(words.ctypes.data, words.size, nbits, got.ctypes.data, got.size, C.byref(count)) == 0
    assert count.value == len(want) and got[:count.value].tolist() == want
    small, count = np.zeros(1, dtype=np.uint32), C.c_long()
    assert lib.pf_pngd_find_host(words.ctypes.data, words.size, nbits, small.ctypes.data, 0, C.byref(count)) == 0 and count.value == len(want)   # counts past the capacity
    b = R.Bits(host.deflate.tobytes())
    starts = np.array(want + [3, 5, max(nbits - 9, 0)], dtype=np.uint32)              # three places that are no block starts, too
    for bits in (1 << 21, 1024):
        rec = np.zeros((starts.size, 4), dtype=np.uint32)
        assert lib.pf_pngd_scan_host(words.ctypes.data, words.size, nbits, starts.ctypes.data, starts.size, bits, expected, rec.ctypes.data) == 0
        for r, s in zip(rec.tolist(), starts.tolist()):
            start, end, out, st, final = R.scan(b, s, bits, expected)
            assert r[0] == start and r[3] == (st | final << 8), (s, r, st)
            if st == R.S_OK:
                assert r[1:3] == [end, out]
    out, stats = np.zeros(expected, dtype=np.uint8), (C.c_long * 6)()
    assert lib.pf_pngd_inflate_model_host(host.deflate.ctypes.data, host.deflate.size, expected, 1 << 21, out.ctypes.data, stats) == 0
    m = R.model(host.deflate.tobytes(), expected)
    assert out.tobytes() == m["out"] == zlib.decompress(R.parse(FILES[name])["idat"])
    kinds = [k[1] for k in m["blocks"]]
    assert list(stats)[:4] == [kinds.count(2), kinds.count(1), kinds.count(0), len(want)]
    assert stats[4] <= m["jump_rounds_used"]                     # the C loop jumps in place, which only converges sooner


def test_every_parser_refusal_has_its_code():
    img = R.photo(6, 7, seed=1)
    good = R.write_png(img, 2, 8, filters=(1,))
    cases = {
        "PngSignature": b"\x89PNX" + good[4:],
        "PngChunk": good[:-20],
        "PngOrder": good[:8] + good[33:],
        "PngCrc": good[:20] + bytes([good[20] ^ 1]) + good[21:],
        "PngIhdr": R.write_png(img, 2, 8).replace(b"\x08\x02\x00\x00\x00", b"\x04\x02\x00\x00\x00", 1),
        "PngInterlaced": R.write_png(img, 2, 8, interlace=1),
        "PngPalette": R.write_png(img[..., :1] % 4, 3, 2),
    }
    ihdr = bytearray(cases["PngIhdr"])
    ihdr[29:33] = zlib.crc32(bytes(ihdr[12:29])).to_bytes(4, "big")
    cases["PngIhdr"] = bytes(ihdr)
    for head, what in ((b"\x79\x9c", "method"), (b"\x88\x1c", "window"), (b"\x78\xbb", "fdict"), (b"\x78\x9d", "fcheck")):
        cases["PngZlibHeader " + what] = R.write_png(img, 2, 8, zlib_header=head)
    for name, data in cases.items():
        with pytest.raises(P.PngError) as e:
            P.PngHost(data)
        assert type(e.value).__name__ == name.split()[0], (name, e.value)
    bad_idat = bytearray(good)
    at = good.index(b"IDAT") + 8
    bad_idat[at + 5] ^= 4
    P.PngHost(bytes(bad_idat))                                   # the IDAT CRC is only looked at for verify='full'
    with pytest.raises(P.PNG_ERRORS[93]):
        P.PngHost(bytes(bad_idat), check_idat_crc=True)
    P.PngHost(R.write_png(img, 2, 8, extra_chunks=[(b"gAMA", b"\0\0\xb1\x8f"), (b"tEXt", b"k\0v")]))        # ancillary chunks are skipped
