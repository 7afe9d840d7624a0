"""CPU checks of the host side of the progressive decoder (csrc/jpeg_host.h through the C ABI) against the model of tests/jpeg_prog_ref.py:
scan lists, coefficients, the stand-alone AC-refinement decoder, one error class per refusal, damaged files, and the reference's own
example files against PIL."""
import os

import numpy as np
import pytest

from patchfusion_amd import preprocess as P
from tests import jpeg_prog_ref as G
from tests import jpeg_ref as R

CASES = G.load_cases()
SUPPORTED = [n for n in CASES if CASES[n][1] is not None]


def test_parser_scan_lists_equal_the_model_s():
    for n in SUPPORTED:
        data = CASES[n][0]
        host = P.JpegProgHost(data)
        h, scans = G.parse(data)
        hh = host.header
        assert not host.baseline and hh.sof == 2 and (hh.width, hh.height, hh.ncomp, hh.nblocks, hh.orientation) == \
            (h.width, h.height, h.ncomp, h.nblocks, h.orientation), n
        assert len(host.scans) == len(scans), n
        for a, b in zip(host.scans, scans):
            assert (a.kind, list(a.comp[:a.ncomp]), a.ss, a.se, a.ah, a.al, a.restart_interval, a.begin, a.end, a.nblocks, a.blocks_per_unit) == \
                (b.kind, b.comps, b.ss, b.se, b.ah, b.al, b.dri, b.begin, b.end, b.nblocks, b.bpu), (n, b)
            for (tc, th), (bits, vals) in b.huff.items():          # the tables as they stand at that SOS
                assert list(a.huff_bits[4 * tc + th][1:17]) == bits and list(a.huff_vals[4 * tc + th][:len(vals)]) == vals, (n, b)
            if a.ncomp == 1:
                assert host.block_map(a).tolist() == G.block_map(h, b), (n, b)
            data_a, segs_a = host.prepare(a)
            data_b, segs_b = G.prepare_scan(data, b)
            assert segs_a.tolist() == [list(s) for s in segs_b] and data_a[:len(data_b)].tobytes() == data_b and not data_a[len(data_b):].any()
            assert data_a.size >= len(data_b) + 64 and data_a.size % 4 == 0
    redefined = P.JpegProgHost(CASES["w_example2_script"][0]).scans                # the writer defines a table per scan
    assert bytes(redefined[1].huff_vals[4]) != bytes(redefined[2].huff_vals[4])


def test_host_coefficients_equal_the_model_s_after_every_scan():
    for n in SUPPORTED:
        data, exp = CASES[n]
        host = P.JpegProgHost(data)
        parsed = G.parse(data)
        coef = np.zeros((host.header.nblocks, 64), dtype=np.int16)
        model = np.zeros((host.header.nblocks, 64), dtype=np.int64)
        for a, b in zip(host.scans, parsed[1]):
            host.decode_scan(a, coef)
            G.decode_scan(parsed[0], b, data, model)
            assert np.array_equal(coef, model), (n, b)
        assert np.array_equal(R.reconstruct(parsed[0], coef, parsed[0].orientation), exp), n


def test_stand_alone_ac_refinement_reproduces_the_host_decode():
    refined = 0
    for n in SUPPORTED:
        data = CASES[n][0]
        host = P.JpegProgHost(data)
        h, scans = G.parse(data)
        coef = np.zeros((h.nblocks, 64), dtype=np.int16)
        for a, b in zip(host.scans, scans):
            if b.kind != G.AC_REFINE:
                host.decode_scan(a, coef)
                continue
            masks = G.nonzero_masks(h, b, coef)                      # the model's masks
            rec = host.refine_ac(a, masks)
            assert not (rec[:, 0] & rec[:, 1]).any() and not (rec[:, 2] & ~rec[:, 1]).any()
            G.apply_records(h, b, coef, rec)
            assert np.array_equal(masks, G.nonzero_masks(h, b, coef)), (n, b)      # the updated masks are the new non-zero map
            refined += 1
        assert np.array_equal(coef, host.decode_entropy()), n
    assert refined >= 30                             # four such scans in each PIL-made file


def test_baseline_file_is_reported_as_such():
    host = P.JpegProgHost(R.load_cases()["17x19_smooth_422_opt"][0])
    assert host.baseline and host.scans == []


def _patched_sos(data, index, **kw):
    """the file with fields of its index-th SOS header overwritten: ss, se, ahal"""
    d, p = bytearray(data), -1
    for _ in range(index + 1):
        p = d.index(b"\xff\xda", p + 1)
    ns = d[p + 4]
    for k, off in (("ss", 5 + 2 * ns), ("se", 6 + 2 * ns), ("ahal", 7 + 2 * ns)):
        if k in kw:
            d[p + off] = kw[k]
    return bytes(d)


def test_each_new_refusal_has_its_own_error():
    data = CASES["100x75_smooth_420_q75"][0]
    h, scans = G.parse(data)
    coef = G.decode_entropy(data, (h, scans))
    E = P.JPEG_ERRORS
    dc, y, cb, cr = ((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 63, 0, 0), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0)
    sof = data.index(b"\xff\xc2")
    cases = [
        (50, CASES["refuse_no_first"][0]),
        (50, G.write(h, coef, [((0, 1, 2), 0, 0, 1, 0), y, cb, cr])),                               # DC refinement first
        (51, G.write(h, coef, [((0, 1, 2), 0, 0, 0, 2), ((0, 1, 2), 0, 0, 1, 0), y, cb, cr])),      # sent at Al = 2, refined from 1
        (51, G.write(h, coef, [dc, y, y, cb, cr])),                                                  # a first scan twice
        (52, G.write(h, coef, [((0, 1, 2), 0, 0, 0, 2), ((0, 1, 2), 0, 0, 2, 0), y, cb, cr])),      # Al != Ah - 1
        (53, CASES["refuse_two_component_ac"][0]),
        (54, G.write(h, coef, [y, dc, cb, cr])),
        (55, _patched_sos(data, 1, ss=6, se=5)),
        (55, _patched_sos(data, 1, se=64)),
        (55, _patched_sos(data, 0, se=1)),                                                           # a DC scan that reaches into the AC band
        (56, CASES["refuse_incomplete"][0]),
        (56, G.write(h, coef, [dc, y, cb])),                                                         # Cr's AC never sent
        (56, G.write(h, coef, [dc, ((0,), 1, 5, 0, 0), cb, cr])),                                    # luma 6-63 never sent
        (35, data[:sof + 1] + b"\xca" + data[sof + 2:]),                                             # SOF10 stays what it was
    ]
    for code, bad in cases:
        with pytest.raises(E[code]) as e:
            P.JpegProgHost(bad)
        assert type(e.value) is E[code] and isinstance(e.value, ValueError) and e.value.code == code, code
    assert len({E[c] for c, _ in cases}) == len({c for c, _ in cases}) == 8
    assert "smooth" in str(E[56](56, E[56].__doc__))


def _marker_boundaries(data):
    """every offset at which a marker segment or a scan's data begins or ends"""
    cuts, p = [2], 2
    while data[p + 1] != 0xd9:
        n = (data[p + 2] << 8) | data[p + 3]
        sos = data[p + 1] == 0xda
        p += 2 + n
        cuts.append(p)
        if sos:
            while not (data[p] == 0xff and data[p + 1] != 0 and not 0xd0 <= data[p + 1] <= 0xd7):
                p += 1
            cuts.append(p)
    return cuts + [p + 1]


def test_truncated_and_bit_flipped_files_return_an_error_or_decode():
    rng = np.random.default_rng(17)
    for name in ("100x75_smooth_420_rst", "37x53_noise_444_q95", "17x19_grey", "w_example3_script", "w_long_eob_run"):
        data = CASES[name][0]
        cuts = _marker_boundaries(data)
        assert len(cuts) > 2 * len(G.parse(data)[1])
        for cut in sorted({c + o for c in cuts for o in (-1, 0, 1)} - {1, len(data)}):        # every boundary, and a byte either side
            with pytest.raises(ValueError):
                P.JpegProgHost(data[:cut]).decode_entropy()
        ranges = [(s.begin, s.end) for s in G.parse(data)[1] if s.end > s.begin]
        for _ in range(150):
            d = bytearray(data)
            a, e = ranges[int(rng.integers(0, len(ranges)))]
            d[int(rng.integers(a, e))] ^= 1 << int(rng.integers(0, 8))                  # one bit of scan data
            try:
                host = P.JpegProgHost(bytes(d))
                host.decode_entropy()
                for s in host.scans:
                    prepared = host.prepare(s)
                    if s.kind in (0, 2):
                        host.plan(s, prepared[1], 32)
                        host.tables(s)
                    if s.kind == 3:
                        host.refine_ac(s, np.full(s.nblocks, 0x0123456789abcdef, dtype=np.uint64), prepared)
            except ValueError:
                pass


@pytest.mark.reference
@pytest.mark.parametrize("name", ["example_1.jpeg", "example_4.jpeg"])
def test_reference_examples_decode_to_pil_on_the_host_path(name):
    from PIL import Image
    from oracle import ref_shim
    path = os.path.join(ref_shim.REF_ROOT, "examples", name)
    if not os.path.exists(path):
        pytest.skip("reference tree not present")
    data = open(path, "rb").read()
    coef = P.JpegProgHost(data).decode_entropy()
    h, _ = G.parse(data)
    assert np.array_equal(R.reconstruct(h, coef, 1), np.asarray(Image.open(path).convert("RGB")))
