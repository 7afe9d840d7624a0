"""The numpy restatement of the ground-truth loaders (tests/gt_ref.py) pinned to the reference's own DepthMap, readPFM and
UnrealStereo4kDataset arithmetic: live under the `reference` marker where the reference tree is present, and against the committed
fixture tests/golden/gt_readers.npz (tools/make_golden_gt.py) everywhere.  No GPU, no library.

On the parent commit this module fails at import: tests/gt_ref.py and the fixture do not exist there."""
import io
import os

import numpy as np
import pytest

from tests import gt_ref as R

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "gt_readers.npz"))
CASES = {c["name"]: c for c in R.golden_cases()}


same_bits = R.same_bits


def restated(case):
    if case["dataset"] == "pfm":
        a, scale = R.read_pfm(case["data"])
        return dict(pfm=a.astype(np.float32), scale=np.float64(scale))
    depth, _, edge = R.depth_map(case["dataset"], case["data"], **case["kwargs"])
    return dict(depth=depth, edge=edge)


def test_fixture_holds_the_cases_as_file_bytes():
    assert {k.split(".")[0] for k in G.files} == set(CASES)
    for name, case in CASES.items():
        assert G[name + ".file"].dtype == np.uint8 and G[name + ".file"].tobytes() == case["data"], name
        for k in G.files:
            assert G[k].ndim < 2 or (G[k].shape[0] <= 37 and G[k].shape[1] <= 53), k


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_reference_fixture(name):
    mine = restated(CASES[name])
    for k, v in mine.items():
        want = G[f"{name}.{k}"]
        assert same_bits(v, want) if v.ndim else float(v) == float(want), (name, k)


def test_the_cases_carry_what_they_promise():
    d = G["u4k_f4_be.depth"]                                     # df = 1e-38: denormal quotients
    assert ((d != 0) & (np.abs(d) < np.finfo(np.float32).tiny)).any()
    x = np.load(io.BytesIO(CASES["u4k_f8_le"]["data"]))
    with np.errstate(over="ignore"):
        assert (x.astype(np.float32).astype(np.float64) != x)[np.isfinite(x)].any()     # doubles that do round
    for name in ("u4k_f4_le", "mid_le", "mid_be", "eth3d", "gta_16", "cityscapes_16"):
        e = G[name + ".edge"]
        assert 0 < e.sum() < e.size, name                          # edges, and not everywhere
    m = G["mid_le.depth"]
    assert np.isnan(m).any() and (m == 0).any() and np.signbit(m[m == 0]).any()         # NaN kept, +inf masked, -inf -> -0.0
    assert np.isnan(G["u4k_f4_le.depth"]).any() and np.isinf(G["u4k_f4_le.depth"]).any()
    assert np.isfinite(G["eth3d.depth"]).all() and np.isfinite(G["cityscapes_16.depth"]).all()


@pytest.mark.reference
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_reference_live(name, tmp_path):
    from oracle import ref_shim
    if not ref_shim.reference_available():
        pytest.skip("reference tree not present")
    ref = R.run_reference(CASES[name], tmp_path)
    mine = restated(CASES[name])
    assert set(ref) == set(mine)
    for k, v in mine.items():
        assert same_bits(v, ref[k]) if v.ndim else float(v) == float(ref[k]), (name, k)


@pytest.mark.reference
def test_u4k_dataset_arithmetic_live(tmp_path):
    """UnrealStereo4kDataset.__getitem__ (u4k_dataset.py:110-178) in its evaluation mode: depth_factor / disp and get_boundaries"""
    from oracle import ref_shim
    if not ref_shim.reference_available():
        pytest.skip("reference tree not present")
    ref_shim.import_reference()
    import torch
    from estimator.datasets.u4k_dataset import UnrealStereo4kDataset
    case = CASES["u4k_f8_le"]
    npy, img = tmp_path / "disp.npy", tmp_path / "img.raw"
    npy.write_bytes(case["data"])
    img.write_bytes(bytes(2160 * 3840 * 3))
    ds = object.__new__(UnrealStereo4kDataset)
    ds.mode, ds.normalize, ds.resize = "infer", None, lambda t: t[..., :2, :2]
    ds.data_infos = [dict(img_path=str(img), depth_map_path=str(npy), depth_factor=case["kwargs"]["depth_factor"], filename="/a/b.raw")]
    with np.errstate(all="ignore"):
        item = ds[0]
    depth, _, edge = R.depth_map("u4k", case["data"], **case["kwargs"])
    got_d, got_e = item["depth_gt"], item["boundary"]
    assert isinstance(got_d, torch.Tensor) and tuple(got_d.shape) == (1,) + depth.shape
    assert same_bits(got_d[0].numpy(), depth) and same_bits(got_e[0].numpy(), edge)
