"""preprocess.decode_png and ImagePreprocessor.read over the numpy fake ops of tests/png_decode_fake_ops.py: every output layout, the
chain rounds, every way the device arm hands a file to the host arm, every refusal class on both arms, argument validation and the
keyword routing of read."""
import os
import re

import numpy as np
import pytest

from patchfusion_amd import preprocess as P
from tests import jpeg_ref as J
from tests import png_decode_ref as R
from tests.jpeg_fake_ops import FakeJpegOps
from tests.png_decode_fake_ops import FakePngDecodeOps

DEVICE = R.device_cases()
FIXTURE = R.load_cases()


@pytest.mark.parametrize("name", sorted(DEVICE))
def test_device_arm_decodes_every_case(name):
    png = DEVICE[name]
    exp = R.decode(png)
    img, info = P.decode_png(png, device="cpu", inflate="device", ops=FakePngDecodeOps())
    assert info.inflate == "device" and info.fallback_reason is None
    assert img.numpy().dtype == exp.dtype and np.array_equal(img.numpy(), exp)
    h = R.parse(png)
    assert (info.width, info.height, info.bit_depth, info.color_type, info.has_trns) == (h["width"], h["height"], h["depth"], h["color_type"], h["has_trns"])
    assert sum(info.blocks.values()) >= 1 and info.resolve_rounds == (sum(info.blocks.values()) - 1).bit_length() + 1
    assert info.compressed_bytes == len(h["idat"]) and info.bytes_uploaded >= len(h["idat"]) - 6 and info.bytes_downloaded == 4 + 16 * info.candidates + \
        16 * (info.chain_rounds - 1) + 8


@pytest.mark.parametrize("name", sorted(FIXTURE))
def test_both_arms_decode_the_fixture(name):
    png, exp = FIXTURE[name]
    for arm in ("device", "host"):
        ops = FakePngDecodeOps()
        img, info = P.decode_png(png, device="cpu", inflate=arm, ops=ops)
        assert info.inflate == arm and img.numpy().dtype == exp.dtype and np.array_equal(img.numpy(), exp)
        assert any(c[0] == "find" for c in ops.calls) == (arm == "device") and any(c[0] == "adler" for c in ops.calls)
    assert info.blocks is None and info.candidates == 0 and info.bytes_uploaded >= exp.shape[0]


def test_chain_rounds_and_the_round_cap():
    png = DEVICE["composite_150x200"]
    exp = R.decode(png)
    img, info = P.decode_png(png, device="cpu", inflate="device", ops=FakePngDecodeOps())
    assert info.inflate == "device" and info.chain_rounds >= 2 and info.blocks["fixed"] >= 1 and info.blocks["stored"] >= 2
    for cap in (0, info.chain_rounds - 1):
        img, low = P.decode_png(png, device="cpu", inflate="device", max_chain_rounds=cap, ops=FakePngDecodeOps())
        assert low.inflate == "host" and "max_chain_rounds" in low.fallback_reason and np.array_equal(img.numpy(), exp)
    img, same = P.decode_png(png, device="cpu", inflate="device", max_chain_rounds=info.chain_rounds, ops=FakePngDecodeOps())
    assert same.inflate == "device" and np.array_equal(img.numpy(), exp)


def test_block_bit_cap_and_list_overflow_fall_back_to_the_host_arm():
    png, exp = FIXTURE["pil_rgb_150x200_l6"]
    img, info = P.decode_png(png, device="cpu", inflate="device", max_block_bits=1024, ops=FakePngDecodeOps())
    assert info.inflate == "host" and "max_block_bits" in info.fallback_reason and np.array_equal(img.numpy(), exp)
    ops = FakePngDecodeOps(candidate_capacity=2)
    img, info = P.decode_png(png, device="cpu", inflate="device", ops=ops)
    assert info.inflate == "host" and "overflow" in info.fallback_reason and np.array_equal(img.numpy(), exp)
    assert not any(c[0] in ("scan", "inflate") for c in ops.calls)


@pytest.mark.parametrize("name", sorted(R.refusal_cases()))
def test_refusals_on_both_arms(name):
    png, cls = R.refusal_cases()[name]
    for arm in ("device", "host"):
        with pytest.raises(P.PngError) as e:
            P.decode_png(png, device="cpu", inflate=arm, ops=FakePngDecodeOps())
        assert type(e.value).__name__ == cls and isinstance(e.value, ValueError) and e.value.code in P.PNG_ERRORS
    if cls == "PngAdler":
        img, _ = P.decode_png(png, device="cpu", verify=False, ops=FakePngDecodeOps())
        assert np.array_equal(img.numpy(), R.photo(20, 24, seed=13))       # the image refusal_cases wrote


def test_verify_full_checks_the_idat_crc():
    png = bytearray(DEVICE["fmt_ct2_d8_w13"])
    at = bytes(png).index(b"IDAT") + 4
    n = int.from_bytes(png[at - 8:at - 4], "big")
    png[at + n] ^= 1                                             # the chunk's CRC itself
    P.decode_png(bytes(png), device="cpu", ops=FakePngDecodeOps())
    with pytest.raises(P.PNG_ERRORS[93]):
        P.decode_png(bytes(png), device="cpu", verify="full", ops=FakePngDecodeOps())


def test_the_default_arm_is_the_measured_one():
    png = DEVICE["one_pixel"]
    assert P.decode_png(png, device="cpu", ops=FakePngDecodeOps())[1].inflate == P.PNG_INFLATE == "host"
    assert P.decode_png(png, device="cpu", inflate="device", ops=FakePngDecodeOps())[1].inflate == "device"


def test_argument_validation(tmp_path):
    png = DEVICE["one_pixel"]
    for kw in (dict(inflate="gpu"), dict(verify="crc"), dict(max_chain_rounds=-1), dict(max_block_bits=8)):
        with pytest.raises(ValueError):
            P.decode_png(png, device="cpu", ops=FakePngDecodeOps(), **kw)
    with pytest.raises(ValueError):
        P.decode_png(np.zeros(4, dtype=np.uint8), device="cpu", ops=FakePngDecodeOps())
    with pytest.raises(P.PngError):
        P.decode_png(b"not a png", device="cpu", ops=FakePngDecodeOps())
    path = tmp_path / "a.png"
    path.write_bytes(png)
    img, _ = P.decode_png(str(path), device="cpu", ops=FakePngDecodeOps())
    assert img.numpy().tolist() == [[[9, 200, 31]]]


class BothOps(FakePngDecodeOps, FakeJpegOps):
    def __init__(self, jpeg=b""):
        FakePngDecodeOps.__init__(self)
        self.data = jpeg


@pytest.mark.parametrize("name", ["fmt_ct2_d8_w13", "fmt_ct0_d16_w13", "fmt_ct6_d8_w13", "fmt_ct4_d16_w13", "fmt_ct3_d2_w16", "fmt_ct0_d1_w13"])
def test_read_routes_a_png_to_decode_png(name, tmp_path):
    png = DEVICE[name]
    ops = BothOps()
    pre = P.ImagePreprocessor(image_resolution=(8, 8), process_shape=(4, 4), dataset_name="general", device="cpu", ops=ops)
    out = pre.read(png, png_options=dict(inflate="host"), apply_orientation=False, subsequence_bits=64, progressive=True)   # JPEG keywords: ignored
    assert set(out) == {"image_hr", "image_lr"} and pre.last_png_info.inflate == "host" and not hasattr(pre, "last_jpeg_info")
    fed = [c for c in ops.calls if c[0] == "bicubic"][0]
    assert np.array_equal(fed[2], R.to_rgb8(R.decode(png)))
    assert any(c[0] == "to_rgb8" for c in ops.calls) == (name not in ("fmt_ct2_d8_w13", "fmt_ct3_d2_w16"))   # those are uint8 [H,W,3] already
    path = tmp_path / "a.png"
    path.write_bytes(png)
    pre.read(str(path))
    assert pre.last_png_info.inflate == P.PNG_INFLATE


def test_read_leaves_jpeg_alone_and_u4k_refuses():
    data, exp = J.load_cases()["orient6_17x19"]
    ops = BothOps(data)
    pre = P.ImagePreprocessor(image_resolution=(8, 8), process_shape=(4, 4), dataset_name="general", device="cpu", ops=ops)
    pre.read(DEVICE["one_pixel"])
    info = pre.last_png_info
    pre.read(data)
    assert pre.last_jpeg_info.orientation == 6 and pre.last_png_info is info and ("reconstruct", 6) in ops.calls
    assert [c for c in ops.calls if c[0] == "bicubic"][-1][1] == exp.shape
    with pytest.raises(ValueError):
        P.ImagePreprocessor(dataset_name="u4k", device="cpu", ops=BothOps()).read(DEVICE["one_pixel"])


def test_python_constants_are_the_header_s():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pf_hip.h")).read()
    d = {k: int(v) for k, v in re.findall(r"#define (PF_PNGD_\w+) (\d+)", text)}
    assert sorted(P.PNG_ERRORS) == sorted(v for k, v in d.items() if k.startswith("PF_PNGD_E_"))
    assert [P.PNG_S_OK, P.PNG_S_INVALID, P.PNG_S_LIMIT, P.PNG_S_EOS, P.PNG_S_SIZE, P.PNG_S_DIST] == \
        [d["PF_PNGD_S_" + k] for k in ("OK", "INVALID", "LIMIT", "EOS", "SIZE", "DIST")]
    assert [P.PNG_F_STREAM, P.PNG_F_DISTANCE, P.PNG_F_FILTER, P.PNG_F_PLTE] == [d["PF_PNGD_F_" + k] for k in ("STREAM", "DISTANCE", "FILTER", "PLTE")]
    assert P.PNG_PAD_WORDS == d["PF_PNGD_PAD_WORDS"]
    assert [R.S_OK, R.S_INVALID, R.S_LIMIT, R.S_EOS, R.S_SIZE, R.S_DIST] == list(range(6))
