"""GPU checks of the progressive JPEG decoder (csrc/jpeg_prog.hip through preprocess.decode_jpeg(..., progressive=True)): every supported
file of tests/golden/jpeg_prog_cases.npz decodes to exactly the array PIL (libjpeg-turbo) gave when the fixture was written, on both
entropy paths; the device coefficients equal the host decoder's for several subsequence lengths; the round loop and the round cap; a
baseline file through the same keyword; read(); the refusals."""
import numpy as np
import pytest
import torch

from tests import jpeg_prog_ref as G
from tests import jpeg_ref as R

pytestmark = pytest.mark.gpu
CASES = G.load_cases()
SUPPORTED = [n for n in CASES if CASES[n][1] is not None]
BIG = ["256x256_noise_q100", "256x256_smooth_q30"]
NO_CAP = 1 << 20


@pytest.mark.parametrize("entropy", ["device", "host"])
def test_every_fixture_file_decodes_exactly(entropy):
    from patchfusion_amd.preprocess import decode_jpeg
    bad = []
    for n in SUPPORTED:
        data, exp = CASES[n]
        rgb, info = decode_jpeg(data, entropy=entropy, max_sync_rounds=NO_CAP, progressive=True)
        assert info.entropy == entropy and info.progressive and len(info.scans) == len(G.parse(data)[1])
        for e in info.scans:
            assert e["decoded"] == ("device" if entropy == "device" and e["kind"] != "ac_refine" else "host"), (n, e)
        got = rgb.cpu().numpy()
        if got.shape != exp.shape or not np.array_equal(got, exp):
            bad.append(n)
    assert not bad, bad


@pytest.mark.parametrize("S", [32, 64, 128, None])
def test_device_coefficients_equal_host_coefficients(S):
    from patchfusion_amd import preprocess as P
    from patchfusion_amd.hip_ops import ops
    names = BIG + ["100x75_smooth_420_q75", "100x75_smooth_420_rst", "1x1", "64x64_constant", "17x19_grey"] + [n for n in SUPPORTED if n.startswith("w_")]
    for n in names:
        host = P.JpegProgHost(CASES[n][0])
        rc, scans, coef, _, _ = P.jpeg_prog_entropy_device(host, ops, torch.device("cuda"), S or P.JPEG_SUBSEQUENCE_BITS, NO_CAP)
        assert rc == 0 and len(scans) == len(host.scans) and np.array_equal(coef.cpu().numpy(), host.decode_entropy()), (n, S)


@pytest.mark.parametrize("name", BIG)
def test_round_loop_is_exercised_and_counts_equal_the_model_s(name):
    from patchfusion_amd.preprocess import decode_jpeg
    data, exp = CASES[name]
    rgb, info = decode_jpeg(data, entropy="device", subsequence_bits=32, max_sync_rounds=NO_CAP, progressive=True)
    rounds = {k: max(e["sync_rounds"] for e in info.scans if e["kind"] == k) for k in ("dc_first", "ac_first")}
    print(name, "sync rounds at S = 32:", rounds)
    assert info.entropy == "device" and rounds["dc_first"] >= 3 and rounds["ac_first"] >= 3
    assert np.array_equal(rgb.cpu().numpy(), exp)
    _, info = decode_jpeg(data, entropy="device", subsequence_bits=1024, max_sync_rounds=NO_CAP, progressive=True)
    h, scans = G.parse(data)
    model = [G.sync_model(h, s, data, 1024) if s.kind in (G.DC_FIRST, G.AC_FIRST) else 0 for s in scans]
    assert [e["sync_rounds"] for e in info.scans] == model and info.sync_rounds == max(model)


def test_round_cap_completes_on_the_host_path():
    from patchfusion_amd.preprocess import decode_jpeg
    data, exp = CASES["256x256_noise_q100"]
    rgb, info = decode_jpeg(data, entropy="device", subsequence_bits=32, max_sync_rounds=1, progressive=True)
    assert info.entropy == "host" and all(e["decoded"] == "host" for e in info.scans) and np.array_equal(rgb.cpu().numpy(), exp)


def test_baseline_file_is_unchanged_by_the_keyword():
    from patchfusion_amd.preprocess import decode_jpeg
    data, exp = R.load_cases()["256x256_smooth_q30"]
    a, ia = decode_jpeg(data)
    b, ib = decode_jpeg(data, progressive=True)
    assert torch.equal(a, b) and np.array_equal(b.cpu().numpy(), exp)
    assert ib.entropy == ia.entropy == "device" and ib.sync_rounds == ia.sync_rounds and not ib.progressive and ib.scans == []


def test_read_equals_call_on_the_expected_array_and_orientation():
    from patchfusion_amd.preprocess import ImagePreprocessor, decode_jpeg
    data, exp = CASES["256x256_smooth_q30"]
    pre = ImagePreprocessor(image_resolution=(96, 128), process_shape=(28, 42))
    a, b = pre.read(data, progressive=True), pre(exp)
    for k in ("image_hr", "image_lr"):
        assert torch.equal(a[k], b[k]), k
    assert pre.last_jpeg_info.progressive
    data, exp = CASES["orient6_17x19"]
    rgb, info = decode_jpeg(data, progressive=True)
    assert info.orientation == 6 and np.array_equal(rgb.cpu().numpy(), exp)
    raw, _ = decode_jpeg(data, progressive=True, apply_orientation=False)
    assert np.array_equal(R.orient(raw.cpu().numpy(), 6), exp)


def test_refused_files_raise():
    from patchfusion_amd import preprocess as P
    for name, code in (("refuse_incomplete", 56), ("refuse_no_first", 50), ("refuse_two_component_ac", 53)):
        with pytest.raises(P.JPEG_ERRORS[code]):
            P.decode_jpeg(CASES[name][0], progressive=True)
    with pytest.raises(P.JPEG_ERRORS[34]):
        P.decode_jpeg(CASES["1x1"][0])
