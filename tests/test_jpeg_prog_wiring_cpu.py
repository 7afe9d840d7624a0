"""preprocess.decode_jpeg(..., progressive=True) over the numpy fake ops of tests/jpeg_prog_fake_ops.py: the default still refuses, a
baseline file takes the baseline ops, every scan goes where its kind says, and the round cap completes the file on the host path."""
import numpy as np
import pytest

from patchfusion_amd import preprocess as P
from tests import jpeg_prog_ref as G
from tests import jpeg_ref as R
from tests.jpeg_prog_fake_ops import FakeJpegProgOps

CASES = G.load_cases()


def test_default_still_refuses_a_progressive_file():
    data = CASES["100x75_smooth_420_q75"][0]
    for kw in (dict(), dict(progressive=False)):
        with pytest.raises(P.JPEG_ERRORS[34]):
            P.decode_jpeg(data, device="cpu", ops=FakeJpegProgOps(data), **kw)


def test_baseline_file_calls_exactly_the_baseline_ops():
    data, exp = R.load_cases()["37x53_noise_420_rst"]
    calls, infos = [], []
    for kw in (dict(), dict(progressive=True)):
        ops = FakeJpegProgOps(data)
        rgb, info = P.decode_jpeg(data, device="cpu", subsequence_bits=64, max_sync_rounds=1000, ops=ops, **kw)
        assert np.array_equal(rgb.numpy(), exp)
        calls.append(ops.calls)
        infos.append(info)
    assert calls[0] == calls[1] and not any(c[0].startswith("prog") for c in calls[1])
    assert infos[0].__dict__ == infos[1].__dict__ and infos[1].progressive is False and infos[1].scans == []


@pytest.mark.parametrize("name", ["100x75_smooth_420_q75", "w_example2_script", "w_noninterleaved_dc", "17x19_grey"])
def test_scans_are_routed_by_kind(name):
    data, exp = CASES[name]
    ops = FakeJpegProgOps(data)
    rgb, info = P.decode_jpeg(data, device="cpu", subsequence_bits=64, max_sync_rounds=1000, ops=ops, progressive=True)
    assert np.array_equal(rgb.numpy(), exp) and info.progressive and info.entropy == "device"
    scans = G.parse(data)[1]
    assert [(e["kind"], e["components"], e["band"], e["ah"], e["al"], e["bytes"]) for e in info.scans] == \
        [(G.KINDS[s.kind], tuple(s.comps), (s.ss, s.se), s.ah, s.al, s.end - s.begin) for s in scans]
    assert all(e["decoded"] == ("host" if e["kind"] == "ac_refine" else "device") for e in info.scans)
    assert info.sync_rounds == max(e["sync_rounds"] for e in info.scans)
    n = lambda k: sum(s.kind == k for s in scans)                  # noqa: E731
    assert sum(c[0] == "prog_scan" for c in ops.calls) == n(G.DC_FIRST) + n(G.AC_FIRST)
    assert sum(c[0] == "prog_dc_refine" for c in ops.calls) == n(G.DC_REFINE)
    assert sum(c[0] == "prog_apply" for c in ops.calls) == n(G.AC_REFINE)
    refined = {s.comps[0] for s in scans if s.kind == G.AC_REFINE}
    assert sorted(c[1] for c in ops.calls if c[0] == "prog_mask") == sorted(refined)       # one mask download per refined component
    for c in ops.calls:                                             # a one-component scan carries its block map, an interleaved one none
        if c[0] == "prog_scan":
            assert c[4] == (c[1] == "ac_first" or len(scans[0].comps) == 1 or name == "w_noninterleaved_dc")


def test_mask_is_downloaded_again_after_a_later_first_scan():
    """luma 1-5 sent and refined, then 6-63 sent and refined: the second refinement needs the non-zero map with the second band in it"""
    data = CASES["100x75_smooth_420_q75"][0]
    h, scans = G.parse(data)
    script = [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 5, 0, 1), ((0,), 1, 5, 1, 0), ((0,), 6, 63, 0, 1), ((0,), 6, 63, 1, 0), ((1,), 1, 63, 0, 0),
              ((2,), 1, 63, 0, 0)]
    made = G.write(h, G.decode_entropy(data, (h, scans)), script)
    ops = FakeJpegProgOps(made)
    rgb, info = P.decode_jpeg(made, device="cpu", ops=ops, progressive=True)
    assert np.array_equal(rgb.numpy(), R.pil_decode(made)) and sum(c[0] == "prog_mask" for c in ops.calls) == 2


def test_host_entropy_and_the_round_cap():
    data, exp = CASES["256x256_smooth_q30"]
    h, scans = G.parse(data)
    need = max(G.sync_model(h, s, data, 32) for s in scans if s.kind in (G.DC_FIRST, G.AC_FIRST))
    assert need >= 2
    ops = FakeJpegProgOps(data)
    rgb, info = P.decode_jpeg(data, device="cpu", entropy="host", ops=ops, progressive=True)
    assert info.entropy == "host" and np.array_equal(rgb.numpy(), exp) and [c[0] for c in ops.calls] == ["reconstruct"]
    assert all(e["decoded"] == "host" for e in info.scans) and info.bytes_uploaded == 128 * h.nblocks
    rgb, info = P.decode_jpeg(data, device="cpu", subsequence_bits=32, max_sync_rounds=need - 1, ops=FakeJpegProgOps(data), progressive=True)
    assert info.entropy == "host" and all(e["decoded"] == "host" for e in info.scans) and np.array_equal(rgb.numpy(), exp)
    rgb, info = P.decode_jpeg(data, device="cpu", subsequence_bits=32, max_sync_rounds=need, ops=FakeJpegProgOps(data), progressive=True)
    assert info.entropy == "device" and info.sync_rounds == need and np.array_equal(rgb.numpy(), exp)


def test_read_passes_the_keyword_through():
    data, exp = CASES["orient6_17x19"]
    ops = FakeJpegProgOps(data)
    pre = P.ImagePreprocessor(image_resolution=(8, 8), process_shape=(4, 4), device="cpu", ops=ops)
    with pytest.raises(P.JPEG_ERRORS[34]):
        pre.read(data)
    out = pre.read(data, progressive=True)
    assert set(out) == {"image_hr", "image_lr"} and pre.last_jpeg_info.progressive and pre.last_jpeg_info.orientation == 6
    assert ("reconstruct", 6) in ops.calls and ("bicubic", exp.shape) in ops.calls


def test_refused_files_raise_through_decode_jpeg():
    for name, code in (("refuse_incomplete", 56), ("refuse_no_first", 50), ("refuse_two_component_ac", 53)):
        with pytest.raises(P.JPEG_ERRORS[code]):
            P.decode_jpeg(CASES[name][0], device="cpu", ops=FakeJpegProgOps(b"\xff\xda"), progressive=True)
