"""decode_png and ImagePreprocessor.read on the GPU (csrc/png_decode.hip).  The expected pixels come from tests/png_decode_ref.py at run
time and, for the PIL-written files, from the committed fixture; equality is exact.  Every case that is not about a fallback asserts that
the device arm decoded it (tests/test_png_decode_ref_cpu.py shows with the model that all of them stay inside the default caps)."""
import functools

import numpy as np
import pytest
import torch

from tests import png_decode_ref as R

pytestmark = pytest.mark.gpu

DEVICE = R.device_cases()
FIXTURE = R.load_cases()
REFUSALS = R.refusal_cases()


@functools.lru_cache(maxsize=None)
def expected(name):
    return R.decode(DEVICE[name])


def decode(png, **kw):
    from patchfusion_amd import preprocess as P
    img, info = P.decode_png(png, device="cuda", **kw)
    return img.cpu().numpy(), info


def same(got, exp):
    return got.dtype == exp.dtype and got.shape == exp.shape and np.array_equal(got, exp)


@pytest.mark.parametrize("name", sorted(DEVICE))
def test_device_arm_is_exact(name):
    got, info = decode(DEVICE[name], inflate="device")
    assert info.inflate == "device" and info.fallback_reason is None
    assert same(got, expected(name))
    if name == "many_blocks_48x64":
        assert info.blocks["dynamic"] >= 24 and info.candidates >= info.blocks["dynamic"]
    if name == "composite_150x200":
        assert info.chain_rounds >= 2 and info.blocks["fixed"] >= 1 and info.blocks["stored"] >= 2
    if name == "far_match":
        assert info.blocks == {"dynamic": 0, "fixed": 1, "stored": 0}


@pytest.mark.parametrize("name", sorted(FIXTURE))
def test_fixture_files_are_exact_on_the_device_arm(name):
    png, exp = FIXTURE[name]
    got, info = decode(png, inflate="device")
    assert info.inflate == "device" and same(got, exp)
    if name == "pil_p8_trns_37x53":
        assert info.has_trns


@pytest.mark.parametrize("name", ["many_blocks_48x64", "composite_150x200", "fmt_ct0_d16_w13"])
def test_host_arm_equals_device_arm(name):
    a, ia = decode(DEVICE[name], inflate="host")
    b, ib = decode(DEVICE[name], inflate="device")
    assert (ia.inflate, ib.inflate) == ("host", "device") and same(a, b) and same(a, expected(name))


def test_round_cap_completes_on_the_host_arm():
    got, info = decode(DEVICE["composite_150x200"], inflate="device", max_chain_rounds=0)
    assert info.inflate == "host" and info.fallback_reason and same(got, expected("composite_150x200"))


def test_block_bit_cap_completes_on_the_host_arm():
    png, exp = FIXTURE["pil_rgb_150x200_l6"]
    got, info = decode(png, inflate="device", max_block_bits=1024)
    assert info.inflate == "host" and "max_block_bits" in info.fallback_reason and same(got, exp)


@pytest.mark.parametrize("name", sorted(REFUSALS))
@pytest.mark.parametrize("arm", ["device", "host"])
def test_refusals(name, arm):
    from patchfusion_amd import preprocess as P
    png, cls = REFUSALS[name]
    with pytest.raises(P.PngError) as e:
        P.decode_png(png, device="cuda", inflate=arm)
    assert type(e.value).__name__ == cls


@pytest.mark.parametrize("strategy", ["huffman", "rle"])
def test_decode_of_encode_png_is_the_identity(strategy):
    from patchfusion_amd import postprocess
    depth = torch.from_numpy(R.photo(64, 80, 1, seed=31, maximum=65535)[..., 0].copy()).cuda()
    colour = torch.from_numpy(R.photo(64, 80, 3, seed=32).copy()).cuda()
    for x in (depth, colour):
        got, info = decode(postprocess.encode_png(x, strategy=strategy), inflate="device")
        assert info.inflate == "device" and same(got, x.cpu().numpy())


@pytest.mark.parametrize("name", ["fmt_ct2_d8_w13", "fmt_ct0_d16_w13", "fmt_ct6_d8_w13"])
def test_read_equals_call_on_the_reference_array(name):
    from patchfusion_amd.preprocess import ImagePreprocessor
    pre = ImagePreprocessor(image_resolution=(20, 26), process_shape=(14, 14), device="cuda")
    a = pre.read(DEVICE[name], png_options=dict(inflate="device"))
    b = pre(R.to_rgb8(expected(name)))
    assert pre.last_png_info.inflate == "device"
    for k in ("image_hr", "image_lr"):
        assert torch.equal(a[k], b[k])
