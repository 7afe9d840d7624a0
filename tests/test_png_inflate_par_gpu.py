"""decode_png(inflate='device', block_decode='subsequences') on the GPU (csrc/png_inflate_par.hip): exact pixels at lanes of 64, 256 and
1024 bits on every file the sequential device arm is tested on, the scan records against the sequential kernel's, the round count
against the C host model's, the refusals, the encoder round trip and ImagePreprocessor.read.  No case may fall back:
tests/test_png_decode_ref_cpu.py shows with the model that all of these files stay inside the default caps.

What the files are there for: one_pixel and constant_64x64 are blocks shorter than one lane; at 64 bits a 48-bit token overruns or skips
a lane; far_match is one fixed block of 276 kbit (1081 lanes at 256 bits, so it crosses a window), with matches at distance 32 768
into other lanes and speculative starts that read a false end-of-block code; composite_150x200 has dynamic, fixed and stored blocks and
the chain re-scan; ramp_96x1024 is periodic and never synchronises; many_blocks_48x64 has 64 short blocks; the level-1 photo has five
blocks of 81-198 kbit whose windows need several rounds."""
import functools
import zlib

import numpy as np
import pytest
import torch

from tests import png_decode_ref as R

pytestmark = pytest.mark.gpu

DEVICE = R.device_cases()
FIXTURE = R.load_cases()
REFUSALS = R.refusal_cases()
LANE_BITS = (64, 256, 1024)
PAR = dict(inflate="device", block_decode="subsequences")


@functools.lru_cache(maxsize=None)
def expected(name):
    return R.decode(DEVICE[name])


@functools.lru_cache(maxsize=None)
def level1_photo():
    """photo(192, 256, seed=41), Paeth rows, zlib level 1 -> (PNG bytes, the image from zlib.decompress + unfilter)"""
    png = R.write_png(R.photo(192, 256, seed=41), 2, 8, filters=(4,), level=1)
    h = R.parse(png)
    rows = R.unfilter(zlib.decompress(h["idat"]), h["height"], h["rowbytes"], h["bpp"])
    return png, rows.reshape(192, 256, 3)


def decode(png, **kw):
    from patchfusion_amd import preprocess as P
    img, info = P.decode_png(png, device="cuda", **kw)
    return img.cpu().numpy(), info


def same(got, exp):
    return got.dtype == exp.dtype and got.shape == exp.shape and np.array_equal(got, exp)


def decoded_in_subsequences(info, bits):
    return info.inflate == "device" and info.block_decode == "subsequences" and info.fallback_reason is None and info.subsequence_bits == bits


@pytest.mark.parametrize("bits", LANE_BITS)
@pytest.mark.parametrize("name", sorted(DEVICE))
def test_subsequence_decode_is_exact(name, bits):
    got, info = decode(DEVICE[name], subsequence_bits=bits, **PAR)
    assert decoded_in_subsequences(info, bits)
    assert same(got, expected(name))
    if name == "composite_150x200":
        assert info.chain_rounds >= 2 and info.blocks["fixed"] >= 1 and info.blocks["stored"] >= 2
    if name == "far_match":
        assert info.blocks == {"dynamic": 0, "fixed": 1, "stored": 0}
    if name == "one_pixel":
        assert info.sync_rounds == 0


@pytest.mark.parametrize("bits", LANE_BITS)
@pytest.mark.parametrize("name", sorted(FIXTURE))
def test_fixture_files_are_exact(name, bits):
    png, exp = FIXTURE[name]
    got, info = decode(png, subsequence_bits=bits, **PAR)
    assert decoded_in_subsequences(info, bits) and same(got, exp)


@pytest.mark.parametrize("bits", LANE_BITS)
def test_level_1_photo_is_exact(bits):
    png, exp = level1_photo()
    got, info = decode(png, subsequence_bits=bits, **PAR)
    assert decoded_in_subsequences(info, bits) and same(got, exp)
    assert info.blocks["dynamic"] + info.blocks["fixed"] >= 3 and info.sync_rounds >= 1


def test_default_lane_length_is_the_module_constant():
    from patchfusion_amd import preprocess as P
    got, info = decode(DEVICE["composite_150x200"], **PAR)
    assert decoded_in_subsequences(info, P.PNG_SUBSEQUENCE_BITS) and same(got, expected("composite_150x200"))


@pytest.mark.parametrize("bits", LANE_BITS)
@pytest.mark.parametrize("name", ["many_blocks_48x64", "composite_150x200", "far_match"])
def test_scan_records_and_round_count_equal_the_sequential_kernel_and_the_host_model(name, bits):
    """every candidate: the record of pngd_scan wherever that one's status is OK, the same start and BFINAL and some non-OK status elsewhere
    (which is all the scheme promises there); info.sync_rounds is the host model's number for the same calls"""
    from patchfusion_amd import preprocess as P
    from patchfusion_amd.hip_ops import ops
    from tests.png_inflate_par_fake_ops import FakePngInflateParOps
    host = P.PngHost(DEVICE[name])
    nbits, n = 8 * host.deflate.size, host.header.inflated_bytes
    words = torch.from_numpy(host.words()).cuda()
    cand = R.find_candidates(host.deflate.tobytes()) + [3, 5]                       # and two places that are no block starts
    starts = torch.tensor(cand, dtype=torch.int64).to(torch.int32).cuda()
    seq = ops.pngd_scan(words, nbits, starts, len(cand), 1 << 21, n, torch.empty((len(cand), 4), dtype=torch.int32, device="cuda")).cpu()
    rounds = torch.zeros(1, dtype=torch.int32, device="cuda")
    par = ops.pngd_scan_par(words, nbits, starts, len(cand), 1 << 21, n, bits, torch.empty((len(cand), 4), dtype=torch.int32, device="cuda"), rounds).cpu()
    fine = (seq[:, 3] & 255) == R.S_OK
    assert int(fine.sum()) >= 1 and torch.equal(par[fine], seq[fine])
    assert torch.equal(par[~fine][:, 0], seq[~fine][:, 0]) and torch.equal(par[~fine][:, 3] >> 8, seq[~fine][:, 3] >> 8)
    assert bool(((par[~fine][:, 3] & 255) != R.S_OK).all())
    model = torch.zeros(1, dtype=torch.int32)
    FakePngInflateParOps().pngd_scan_par(words.cpu(), nbits, starts.cpu(), len(cand), 1 << 21, n, bits, torch.empty((len(cand), 4), dtype=torch.int32), model)
    assert int(rounds.cpu()[0]) == int(model[0])
    _, on_gpu = decode(DEVICE[name], subsequence_bits=bits, **PAR)
    _, on_host = P.decode_png(DEVICE[name], device="cpu", subsequence_bits=bits, ops=FakePngInflateParOps(), **PAR)
    assert decoded_in_subsequences(on_gpu, bits) and on_gpu.sync_rounds == on_host.sync_rounds
    if name == "far_match" and bits <= 256:
        assert on_gpu.sync_rounds >= 2


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_are_those_of_the_sequential_decode(name):
    from patchfusion_amd import preprocess as P
    png, cls = REFUSALS[name]
    raised = []
    for mode in ("sequential", "subsequences"):
        with pytest.raises(P.PngError) as e:
            P.decode_png(png, device="cuda", inflate="device", block_decode=mode)
        raised.append(type(e.value))
    assert raised[0] is raised[1] and raised[1].__name__ == cls


@pytest.mark.parametrize("strategy", ["huffman", "rle"])
def test_decode_of_encode_png_is_the_identity(strategy):
    from patchfusion_amd import postprocess
    depth = torch.from_numpy(R.photo(64, 80, 1, seed=31, maximum=65535)[..., 0].copy()).cuda()
    colour = torch.from_numpy(R.photo(64, 80, 3, seed=32).copy()).cuda()
    for x in (depth, colour):
        got, info = decode(postprocess.encode_png(x, strategy=strategy), **PAR)
        assert info.inflate == "device" and info.block_decode == "subsequences" and info.fallback_reason is None
        assert same(got, x.cpu().numpy())


@pytest.mark.parametrize("name", ["fmt_ct2_d8_w13", "fmt_ct0_d16_w13", "fmt_ct6_d8_w13"])
def test_read_equals_call_on_the_reference_array(name):
    from patchfusion_amd.preprocess import ImagePreprocessor
    pre = ImagePreprocessor(image_resolution=(20, 26), process_shape=(14, 14), device="cuda")
    a = pre.read(DEVICE[name], png_options=dict(PAR))
    b = pre(R.to_rgb8(expected(name)))
    info = pre.last_png_info
    assert info.inflate == "device" and info.block_decode == "subsequences" and info.fallback_reason is None
    for k in ("image_hr", "image_lr"):
        assert torch.equal(a[k], b[k])
