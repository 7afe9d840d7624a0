"""GPU checks of the device JPEG decoder (csrc/jpeg.hip through preprocess.decode_jpeg): every supported file of tests/golden/jpeg_cases.npz
decodes to exactly the array PIL (libjpeg-turbo) gave when the fixture was written, on both entropy paths; the device entropy decoder's
coefficients equal the host decoder's for several subsequence lengths; the round loop is exercised; orientation; the round cap; read()."""
import numpy as np
import pytest
import torch

from tests import jpeg_ref as R

pytestmark = pytest.mark.gpu
CASES = R.load_cases()
SUPPORTED = [n for n in CASES if CASES[n][1] is not None]
BIG = ["256x256_noise_q100", "256x256_smooth_q30"]
NO_CAP = 1 << 20       # the q100 noise file never self-synchronises: its states only arrive along the chain, thousands of rounds at S = 32


@pytest.mark.parametrize("entropy", ["device", "host"])
def test_every_fixture_file_decodes_exactly(entropy):
    from patchfusion_amd.preprocess import decode_jpeg
    bad = []
    for n in SUPPORTED:
        data, exp = CASES[n]
        rgb, info = decode_jpeg(data, entropy=entropy, max_sync_rounds=NO_CAP)
        assert info.entropy == entropy
        got = rgb.cpu().numpy()
        if got.shape != exp.shape or not np.array_equal(got, exp):
            bad.append(n)
    assert not bad, bad


@pytest.mark.parametrize("S", [32, 64, 128, None])
def test_device_coefficients_equal_host_coefficients(S):
    from patchfusion_amd import preprocess as P
    from patchfusion_amd.hip_ops import ops
    names = BIG + ["64x48_smooth_rstrow", "37x53_noise_420_rst", "37x53_noise_444_q100", "17x19_smooth_422_opt", "17x19_noise_grey_q30",
                   "1x1_noise_444_q30"]
    for n in names:
        host = P.JpegHost(CASES[n][0])
        rc, rounds, coef, _ = P.jpeg_entropy_device(host, ops, torch.device("cuda"), S or P.JPEG_SUBSEQUENCE_BITS, NO_CAP)
        assert rc == 0 and np.array_equal(coef.cpu().numpy(), host.decode_entropy()), (n, S)


def test_noise_file_takes_the_model_s_round_count():
    """121 rounds at S = 1024 is what the Python model of the rounds gives (tests/test_jpeg_ref_cpu.py): double-buffered states make the
    count a property of the file"""
    from patchfusion_amd.preprocess import decode_jpeg
    _, info = decode_jpeg(CASES["256x256_noise_q100"][0], entropy="device", subsequence_bits=1024, max_sync_rounds=NO_CAP)
    assert info.entropy == "device" and info.sync_rounds == 121


@pytest.mark.parametrize("name", BIG)
def test_round_loop_is_exercised(name):
    from patchfusion_amd.preprocess import decode_jpeg
    data, exp = CASES[name]
    rgb, info = decode_jpeg(data, entropy="device", subsequence_bits=32, max_sync_rounds=NO_CAP)
    print(name, "sync rounds at S = 32:", info.sync_rounds)
    assert info.entropy == "device" and info.sync_rounds >= 3
    assert np.array_equal(rgb.cpu().numpy(), exp)


def test_one_pixel_file_is_one_mcu_one_subsequence():
    from patchfusion_amd.preprocess import JpegHost, decode_jpeg
    name = next(n for n in SUPPORTED if n.startswith("1x1_"))
    data, exp = CASES[name]
    host = JpegHost(data)
    lanes, segx, longest = host.plan(1024)
    assert host.header.nblocks == host.header.blocks_per_mcu and lanes.shape[0] == 1 and longest == 1
    rgb, info = decode_jpeg(data, entropy="device")
    assert info.entropy == "device" and info.sync_rounds == 0 and np.array_equal(rgb.cpu().numpy(), exp)


@pytest.mark.parametrize("o", range(1, 9))
def test_orientation(o):
    from patchfusion_amd.preprocess import decode_jpeg
    data, exp = CASES[f"orient{o}_17x19"]
    rgb, info = decode_jpeg(data)
    assert info.orientation == o and np.array_equal(rgb.cpu().numpy(), exp)
    raw, _ = decode_jpeg(data, apply_orientation=False)
    assert np.array_equal(R.orient(raw.cpu().numpy(), o), exp)


def test_round_cap_completes_on_the_host_path():
    from patchfusion_amd.preprocess import decode_jpeg
    data, exp = CASES["256x256_noise_q100"]
    rgb, info = decode_jpeg(data, entropy="device", subsequence_bits=32, max_sync_rounds=1)
    assert info.entropy == "host" and np.array_equal(rgb.cpu().numpy(), exp)


def test_refused_files_raise():
    from patchfusion_amd import preprocess as P
    with pytest.raises(P.JPEG_ERRORS[34]):
        P.decode_jpeg(CASES["refuse_progressive"][0])
    with pytest.raises(P.JPEG_ERRORS[39]):
        P.decode_jpeg(CASES["refuse_cmyk"][0])


def test_read_equals_call_on_the_expected_array():
    from patchfusion_amd.preprocess import ImagePreprocessor
    data, exp = CASES["256x256_smooth_q30"]
    pre = ImagePreprocessor(image_resolution=(96, 128), process_shape=(28, 42))
    a, b = pre.read(data), pre(exp)
    for k in ("image_hr", "image_lr"):
        assert torch.equal(a[k], b[k]), k
    with pytest.raises(ValueError):
        ImagePreprocessor(dataset_name="u4k").read(data)
