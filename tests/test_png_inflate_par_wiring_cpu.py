"""The host side of decode_png(inflate='device', block_decode='subsequences') without a GPU: the fake ops of
tests/png_inflate_par_fake_ops.py run the two new entry points through the C host models, everything else through the numpy stand-ins of
tests/png_decode_fake_ops.py.  Keyword routing and validation, the new PngInfo fields, the round count of pf_pngd_resolve, the
fallbacks, and that the defaults did not move."""
import numpy as np
import pytest

from patchfusion_amd import preprocess as P
from tests import png_decode_ref as R
from tests.png_decode_fake_ops import FakePngDecodeOps
from tests.png_inflate_par_fake_ops import FakePngInflateParOps

DEVICE = R.device_cases()
FIXTURE = R.load_cases()
PAR = dict(inflate="device", block_decode="subsequences")


def names_of(ops):
    return [c[0] for c in ops.calls]


@pytest.mark.parametrize("bits", [64, 256, 1024])
@pytest.mark.parametrize("name", sorted(DEVICE))
def test_subsequence_mode_decodes_every_case(name, bits):
    ops = FakePngInflateParOps()
    img, info = P.decode_png(DEVICE[name], device="cpu", subsequence_bits=bits, ops=ops, **PAR)
    exp = R.decode(DEVICE[name])
    assert info.inflate == "device" and info.fallback_reason is None
    assert (info.block_decode, info.subsequence_bits) == ("subsequences", bits) and isinstance(info.sync_rounds, int) and 0 <= info.sync_rounds < P.PNG_PAR_WINDOW
    assert img.numpy().dtype == exp.dtype and np.array_equal(img.numpy(), exp)
    called = names_of(ops)
    assert "scan" not in called and "inflate" not in called and "inflate_par" in called
    assert all(c[-1] == bits for c in ops.calls if c[0] in ("scan_par", "inflate_par"))
    assert info.bytes_downloaded == 4 + 16 * info.candidates + 16 * (info.chain_rounds - 1) + 12       # the round count rides with the status


@pytest.mark.parametrize("name", sorted(FIXTURE))
def test_subsequence_mode_decodes_the_fixture(name):
    png, exp = FIXTURE[name]
    img, info = P.decode_png(png, device="cpu", ops=FakePngInflateParOps(), **PAR)
    assert info.inflate == "device" and info.block_decode == "subsequences" and info.subsequence_bits == P.PNG_SUBSEQUENCE_BITS
    assert img.numpy().dtype == exp.dtype and np.array_equal(img.numpy(), exp)


def test_resolve_rounds_cover_the_lane_ranges():
    ops = FakePngInflateParOps()
    _, info = P.decode_png(DEVICE["far_match"], device="cpu", subsequence_bits=64, ops=ops, **PAR)
    nbits = 8 * P.PngHost(DEVICE["far_match"]).deflate.size
    lanes = nbits // 64                                     # one fixed block over the whole stream (less the Adler-32 behind it)
    assert lanes - 2 <= 2 ** (info.resolve_rounds - 1) and info.resolve_rounds == [c[1] for c in ops.calls if c[0] == "resolve"][0]
    assert info.resolve_rounds <= (lanes + 2).bit_length() + 1
    assert info.sync_rounds >= 2


def test_defaults_are_unchanged():
    assert (P.PNG_INFLATE, P.PNG_BLOCK_DECODE) == ("host", "sequential")
    ops = FakePngDecodeOps()                                 # has no subsequence entry point: the sequential arm must not ask for one
    img, info = P.decode_png(DEVICE["composite_150x200"], device="cpu", inflate="device", ops=ops)
    assert info.inflate == "device" and info.block_decode == "sequential" and info.sync_rounds == 0 and info.subsequence_bits == P.PNG_SUBSEQUENCE_BITS
    assert "scan" in names_of(ops) and "inflate" in names_of(ops)
    assert info.resolve_rounds == (sum(info.blocks.values()) - 1).bit_length() + 1
    img, info = P.decode_png(DEVICE["composite_150x200"], device="cpu", ops=FakePngDecodeOps())
    assert info.inflate == "host" and info.block_decode == "sequential" and info.sync_rounds == 0


def test_bad_keywords_raise_value_error():
    png = DEVICE["one_pixel"]
    for bad in (0, 32, 63, 65, 96 + 1, 100, (1 << 16) + 32, 1 << 17, -64, 256.0, "256", True):
        with pytest.raises(ValueError, match="subsequence_bits"):
            P.decode_png(png, device="cpu", subsequence_bits=bad, ops=FakePngInflateParOps(), **PAR)
    for good in (64, 96, 1 << 16):
        P.decode_png(png, device="cpu", subsequence_bits=good, ops=FakePngInflateParOps(), **PAR)
    with pytest.raises(ValueError, match="block_decode"):
        P.decode_png(png, device="cpu", inflate="device", block_decode="parallel", ops=FakePngInflateParOps())
    for arm in ("host", None):                               # None is the default arm, 'host'
        with pytest.raises(ValueError, match="inflate='device'"):
            P.decode_png(png, device="cpu", inflate=arm, block_decode="subsequences", ops=FakePngInflateParOps())


def test_fallbacks_keep_their_meaning_and_texts():
    png, exp = FIXTURE["pil_rgb_150x200_l6"]
    seq = P.decode_png(png, device="cpu", inflate="device", max_block_bits=1024, ops=FakePngDecodeOps())[1]
    img, info = P.decode_png(png, device="cpu", max_block_bits=1024, ops=FakePngInflateParOps(), **PAR)
    assert info.inflate == "host" and info.fallback_reason == seq.fallback_reason and "max_block_bits" in info.fallback_reason
    assert info.block_decode == "sequential" and info.sync_rounds == 0 and np.array_equal(img.numpy(), exp)
    seq = P.decode_png(DEVICE["composite_150x200"], device="cpu", inflate="device", max_chain_rounds=1, ops=FakePngDecodeOps())[1]
    img, info = P.decode_png(DEVICE["composite_150x200"], device="cpu", max_chain_rounds=1, ops=FakePngInflateParOps(), **PAR)
    assert info.inflate == "host" and info.fallback_reason == seq.fallback_reason and "max_chain_rounds" in info.fallback_reason
    seq = P.decode_png(DEVICE["many_blocks_48x64"], device="cpu", inflate="device", ops=FakePngDecodeOps(candidate_capacity=3))[1]
    img, info = P.decode_png(DEVICE["many_blocks_48x64"], device="cpu", ops=FakePngInflateParOps(candidate_capacity=3), **PAR)
    assert info.inflate == "host" and info.fallback_reason == seq.fallback_reason and "overflow" in info.fallback_reason


@pytest.mark.parametrize("name", sorted(R.refusal_cases()))
def test_refusals_are_those_of_the_sequential_decode(name):
    png, cls = R.refusal_cases()[name]
    with pytest.raises(P.PngError) as e:
        P.decode_png(png, device="cpu", ops=FakePngInflateParOps(), **PAR)
    assert type(e.value).__name__ == cls


def test_timing_keeps_its_keys_and_read_passes_the_options_through():
    timing = {}
    P.decode_png(DEVICE["composite_150x200"], device="cpu", ops=FakePngInflateParOps(), timing=timing, **PAR)
    assert {"finder", "scan", "chain_walk", "inflate", "resolve"} <= set(timing)
    ops = FakePngInflateParOps()
    pre = P.ImagePreprocessor(image_resolution=(20, 26), process_shape=(14, 14), device="cpu", ops=ops)
    pre.read(DEVICE["fmt_ct0_d16_w13"], png_options=dict(PAR, subsequence_bits=128))
    info = pre.last_png_info
    assert (info.inflate, info.block_decode, info.subsequence_bits) == ("device", "subsequences", 128)
    assert "inflate_par" in names_of(ops) and "to_rgb8" in names_of(ops)
