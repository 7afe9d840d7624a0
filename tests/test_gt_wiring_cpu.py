"""Host side of the ground-truth reader without a GPU: groundtruth.read_depth_gt / read_pfm / read_npy and datasets.ImageDataset driven
through the numpy stand-in ops of tests/gt_fake_ops.py must equal the restatement of tests/gt_ref.py bit for bit; the header parsers,
the path rules of the side files and every refusal are checked here.

On the parent commit this module fails at import: patchfusion_amd.groundtruth and patchfusion_amd.datasets do not exist there."""
import io

import numpy as np
import pytest
import torch

from patchfusion_amd import datasets, groundtruth as gt
from tests import gt_ref as R
from tests import png_decode_ref as P
from tests.gt_fake_ops import FakeGtOps

HOST_PNG = dict(inflate="host")
same_bits = R.same_bits


def read(data, dataset, **kw):
    kw.setdefault("ops", FakeGtOps())
    return gt.read_depth_gt(data, dataset, device="cpu", **kw)


def check(got, want, where):
    depth, edge_source, edge = want
    assert same_bits(got.depth.numpy(), depth), where
    assert same_bits(got.edge_source.numpy(), edge_source), where
    assert same_bits(got.edge.numpy(), edge), where
    assert got.info.shape == depth.shape


# ---------------------------------------------------------------- NPY
@pytest.mark.parametrize("version", [(1, 0), (2, 0), (3, 0)])
@pytest.mark.parametrize("descr", ["<f2", "<f4", "<f8", ">f2", ">f4", ">f8"])
def test_npy_versions_and_dtypes(version, descr):
    a = R.float_plane(5, 7, descr[1:], seed=3).astype(descr)
    data = R.npy_bytes(a, version)
    assert np.array_equal(np.load(io.BytesIO(data)), a, equal_nan=True)          # numpy reads the hand-written file
    ops = FakeGtOps()
    assert same_bits(gt.read_npy(data, device="cpu", ops=ops).numpy(), R.read_npy(data))
    got = read(data, "u4k", depth_factor=1234.5678, ops=ops)
    check(got, R.depth_map("u4k", data, depth_factor=1234.5678), (version, descr))
    assert (got.info.format, got.info.dtype, got.info.endianness, got.info.npy_version) == ("npy", descr[1:], descr[0], version)
    assert got.info.bytes_uploaded == a.nbytes
    assert ("gt_convert", descr[1:], "u4k", (5, 7), descr[0] == ">", False) in ops.calls


def test_npy_native_marks_and_unit_axes():
    a = R.float_plane(4, 6, "f4", seed=4)
    for descr in ("=f4", "|f4"):
        assert same_bits(gt.read_npy(R.npy_bytes(a, descr=descr), device="cpu", ops=FakeGtOps()).numpy(), a)
    for shape in ((1, 4, 6), (4, 6, 1), (1, 1, 4, 6, 1)):
        data = R.npy_bytes(a, shape=shape)
        check(read(data, "u4k", depth_factor=R.DENORMAL_DF), R.depth_map("u4k", data, depth_factor=R.DENORMAL_DF), shape)
    data = R.npy_bytes(a) + b"trailing bytes"                      # np.load reads what the header promises and no more
    assert same_bits(gt.read_npy(data, device="cpu", ops=FakeGtOps()).numpy(), a)
    assert same_bits(gt.read_npy(memoryview(bytearray(R.npy_bytes(a))), device="cpu", ops=FakeGtOps()).numpy(), a)


def test_npy_refusals():
    a = R.float_plane(4, 6, "f4", seed=5)
    good = R.npy_bytes(a)
    ints = np.arange(24).reshape(4, 6)
    cases = [
        (gt.GtNpyFortran, R.npy_bytes(a, fortran=True)),
        (gt.GtNpyDtype, R.npy_bytes(a, descr="|O")),
        (gt.GtNpyDtype, R.npy_bytes(a, descr=[("x", "<f4")])),
        (gt.GtNpyDtype, R.npy_bytes(ints.astype("<i4"))),
        (gt.GtNpyDtype, R.npy_bytes(ints.astype("<u2"))),
        (gt.GtNpyDtype, R.npy_bytes(a, descr="<c8")),
        (gt.GtPayloadSize, good[:-1]),
        (gt.GtNpyShape, R.npy_bytes(a, shape=(2, 2, 6))),
        (gt.GtNpyShape, R.npy_bytes(a, shape=(24,))),
        (gt.GtNpyShape, R.npy_bytes(a, shape=())),
        (gt.GtNpyHeader, b"\x93NUMPX" + good[6:]),
        (gt.GtNpyHeader, good[:6] + bytes((4, 0)) + good[8:]),
        (gt.GtNpyHeader, good[:8]),
        (gt.GtNpyHeader, good[:10] + b"{not a dict" + good[21:]),
        (gt.GtNpyHeader, good[:40]),
    ]
    for cls, data in cases:
        ops = FakeGtOps()
        with pytest.raises(cls) as e:
            read(data, "u4k", depth_factor=1.0, ops=ops)
        assert isinstance(e.value, gt.GtError) and isinstance(e.value, ValueError) and "ground truth" in str(e.value)
        assert not ops.calls                                       # refused before anything is uploaded
        with pytest.raises(cls):
            gt.read_npy(data, device="cpu", ops=FakeGtOps())


# ---------------------------------------------------------------- PFM
@pytest.mark.parametrize("little", [True, False])
@pytest.mark.parametrize("colour", [False, True])
def test_pfm_both_byte_orders_and_magics(little, colour):
    a = R.float_plane(5, 21 if colour else 7, "f4", seed=6)
    a = a.reshape(5, 7, 3) if colour else a
    data = R.pfm_bytes(a, little, scale=0.25, colour=colour)
    ops = FakeGtOps()
    got, scale = gt.read_pfm(data, device="cpu", ops=ops)
    want, want_scale = R.read_pfm(data)
    assert scale == want_scale == 0.25 and tuple(got.shape) == a.shape
    assert same_bits(got.numpy(), want.astype(np.float32)) and same_bits(got.numpy(), a)
    assert ops.calls == [("gt_convert", "f4", "raw", (5, 21 if colour else 7), not little, True)]
    if colour:
        with pytest.raises(gt.GtPfmColour):
            read(data, "mid", calib=R.CALIB)
    else:
        got = read(data, "mid", calib=R.CALIB)
        check(got, R.depth_map("mid", data, calib=R.CALIB), little)
        check(read(data, "mid", calib=R.calib_text()), R.depth_map("mid", data, calib=R.calib_text()), little)
        assert (got.info.format, got.info.endianness, got.info.scale, got.info.bytes_uploaded) == ("pfm", "<" if little else ">", 0.25, a.nbytes)


def test_pfm_refusals():
    a = R.float_plane(3, 4, "f4", seed=7)
    good = R.pfm_bytes(a)
    cases = [
        (gt.GtPfmHeader, b"P5" + good[2:]),
        (gt.GtPfmHeader, good.replace(b"4 3\n", b"4  3\n", 1)),          # the reference's pattern takes ONE blank between the numbers
        (gt.GtPfmHeader, good.replace(b"4 3\n", b"4 3", 1)),
        (gt.GtPfmHeader, good.replace(b"-1.0\n", b"abc\n", 1)),
        (gt.GtPfmHeader, good.replace(b"4 3\n", b"0 3\n", 1)),
        (gt.GtPayloadSize, good[:-4]),
        (gt.GtPayloadSize, good + bytes(4)),
    ]
    for cls, data in cases:
        with pytest.raises(cls):
            gt.read_pfm(data, device="cpu", ops=FakeGtOps())
        with pytest.raises(cls):
            read(data, "mid", calib=R.CALIB)
    for bad in ("cam0=3997 0 0\n\ndoffs=1\nbaseline=2\n", "cam0=[3997 0 0]\n", "cam0=[x 0 0]\n\ndoffs=1\nbaseline=2\n", (1.0, 2.0), object()):
        with pytest.raises(gt.GtCalib):
            read(good, "mid", calib=bad)


# ---------------------------------------------------------------- eth3d, PNG datasets
def test_eth3d_shape_and_size():
    a = R.float_plane(6, 9, "f4", seed=8)
    data = a.astype("<f4").tobytes()
    got = read(data, "eth3d", shape=(6, 9))
    check(got, R.depth_map("eth3d", data, shape=(6, 9)), "eth3d")
    assert got.edge_source is got.depth and got.info.format == "raw"
    for bad in (data[:-4], data + bytes(4)):
        with pytest.raises(gt.GtPayloadSize):
            read(bad, "eth3d", shape=(6, 9))
    with pytest.raises(gt.GtPayloadSize) as e:                       # the default shape is the dataset's 4032 x 6048
        read(data, "eth3d")
    assert "4032 x 6048" in str(e.value)


@pytest.mark.parametrize("dataset", ["gta", "cityscapes"])
@pytest.mark.parametrize("depth", [16, 8])
def test_png_datasets(dataset, depth):
    data = R.png_bytes(R.sample_plane(6, 11, depth, 9, dataset), depth)
    got = read(data, dataset, png_options=HOST_PNG)
    check(got, R.depth_map(dataset, data), (dataset, depth))
    assert (got.info.format, got.info.dtype) == ("png", "u2" if depth == 16 else "u1") and got.info.png.inflate == "host"
    check(read(data, dataset, png_options=HOST_PNG, th=0.5, dilation=3), R.depth_map(dataset, data, th=0.5, dilation=3), "dilated")
    assert read(data, dataset, png_options=HOST_PNG, edges=False).edge is None


def test_png_layout_refusals():
    rs = np.random.RandomState(10)
    files = [P.write_png(rs.randint(0, 256, (4, 5, 3)), 2, 8), P.write_png(rs.randint(0, 65536, (4, 5, 2)), 4, 16),
             P.write_png(rs.randint(0, 4, (4, 5, 1)), 3, 8, palette=rs.randint(0, 256, (4, 3))), P.write_png(rs.randint(0, 16, (4, 5, 1)), 0, 4)]
    for data in files:
        for dataset in ("gta", "cityscapes"):
            with pytest.raises(gt.GtPngLayout):
                read(data, dataset, png_options=HOST_PNG)
    from patchfusion_amd.preprocess import PngError
    with pytest.raises(PngError):                                    # a broken file keeps the PNG decoder's own refusal
        read(b"\x89PNG\r\n\x1a\n" + bytes(40), "gta", png_options=HOST_PNG)


# ---------------------------------------------------------------- side files, inputs, datasets
def test_side_files_follow_the_reference_path_rules(tmp_path):
    a = R.float_plane(5, 7, "f4", seed=11)
    npy = R.npy_bytes(a)
    (tmp_path / "val_gt" / "s1").mkdir(parents=True)
    (tmp_path / "val_factor" / "s1").mkdir(parents=True)
    (tmp_path / "val_gt" / "s1" / "00007.npy").write_bytes(npy)
    (tmp_path / "val_factor" / "s1" / "00007.txt").write_text("1832.25\nsecond line\n")
    got = read(str(tmp_path / "val_gt" / "s1" / "00007.npy"), "u4k")
    check(got, R.depth_map("u4k", npy, depth_factor=1832.25), "u4k path")
    assert got.info.depth_factor == 1832.25 and got.info.path.endswith("00007.npy")
    check(read(tmp_path / "val_gt" / "s1" / "00007.npy", "u4k", depth_factor=2.5), R.depth_map("u4k", npy, depth_factor=2.5), "given factor wins")
    pfm = R.pfm_bytes(a, little=False)
    (tmp_path / "gts").mkdir()
    (tmp_path / "calibs").mkdir()
    (tmp_path / "gts" / "Adirondack.pfm").write_bytes(pfm)
    (tmp_path / "calibs" / "Adirondack.txt").write_text(R.calib_text())
    got = read(str(tmp_path / "gts" / "Adirondack.pfm"), "mid")
    check(got, R.depth_map("mid", pfm, calib=R.CALIB), "mid path")
    assert got.info.calib == R.CALIB
    assert gt.u4k_factor_path("/d/val_gt/a.npy") == "/d/val_factor/a.txt" and gt.mid_calib_path("/d/gts/a.pfm") == "/d/calibs/a.txt"
    with pytest.raises(gt.GtSideFile):
        read(npy, "u4k")
    with pytest.raises(gt.GtSideFile):
        read(pfm, "mid")
    with pytest.raises(gt.GtCalib):
        read(npy, "u4k", depth_factor="not a number")
    with pytest.raises(FileNotFoundError):
        (tmp_path / "val_gt" / "lonely.npy").write_bytes(npy)
        read(str(tmp_path / "val_gt" / "lonely.npy"), "u4k")


def test_unknown_dataset_and_input_types():
    for name in ("nyu", "kitti", "", "U4K", None):
        with pytest.raises(NotImplementedError):
            read(b"", name)
    with pytest.raises(gt.GtInput):
        read(12, "u4k")
    import patchfusion_amd
    assert patchfusion_amd.read_depth_gt is gt.read_depth_gt and patchfusion_amd.GtError is gt.GtError
    assert patchfusion_amd.ImageDataset is datasets.ImageDataset


def test_depth_factor_meets_the_array_as_float32():
    """a factor above float32's range is inf before the division, as numpy makes it"""
    a = np.array([[1.0, 2.0, np.inf]], np.float32)
    data = R.npy_bytes(a)
    got = read(data, "u4k", depth_factor=1e39)
    check(got, R.depth_map("u4k", data, depth_factor=1e39), "overflow")
    assert np.isinf(got.depth[0, 0].item()) and np.isnan(got.depth[0, 2].item())


def test_image_dataset_keys_and_basenames(tmp_path):
    rs = np.random.RandomState(12)
    img_dir, gt_dir = tmp_path / "images", tmp_path / "depth"
    img_dir.mkdir()
    gt_dir.mkdir()
    names = ["b_scene.png", "a_scene.jpeg.png", "c.png"]
    gts = {}
    for i, n in enumerate(names):
        (img_dir / n).write_bytes(P.write_png(rs.randint(0, 256, (6, 8, 3)), 2, 8))
        gts[n] = R.png_bytes(R.sample_plane(6, 8, 16, 20 + i, "gta"))
        (gt_dir / n).write_bytes(gts[n])
    ops = FakeGtOps()
    ds = datasets.ImageDataset(str(img_dir), gt_dir=str(gt_dir), image_resolution=[12, 16], dataset_name="gta", network_process_size=(40, 50),
                               device="cpu", ops=ops)
    assert len(ds) == 3 and ds.files == sorted(names)
    for i, n in enumerate(sorted(names)):
        item = ds[i]
        assert list(item) == ["image_lr", "image_hr", "depth_gt", "boundary", "img_file_basename"]
        assert item["img_file_basename"] == n.replace(".jpg", "").replace(".png", "").replace(".jpeg", "")
        assert tuple(item["image_hr"].shape) == (3, 12, 16) and tuple(item["image_lr"].shape) == (3, 32, 64)   # multiples of 32, as midas.Resize
        depth, _, edge = R.depth_map("gta", gts[n])
        assert same_bits(item["depth_gt"].numpy(), depth) and tuple(item["boundary"].shape) == (1, 6, 8)
        assert same_bits(item["boundary"][0].numpy(), edge)
    assert [ds[i]["img_file_basename"] for i in range(3)] == ["a_scene", "b_scene", "c"]
    plain = datasets.ImageDataset(str(img_dir), image_resolution=[12, 16], dataset_name="gta", resize_mode="depth-anything",
                                  network_process_size=(392, 518), device="cpu", ops=ops)
    assert list(plain[0]) == ["image_lr", "image_hr", "img_file_basename"] and tuple(plain[0]["image_lr"].shape) == (3, 392, 518)
    with pytest.raises(NotImplementedError):
        datasets.ImageDataset(str(img_dir), resize_mode="other", device="cpu", ops=ops)
    # get_metrics / evaluator carry the reference's arguments (general_dataset.py:221-230)
    ops.calls.clear()
    item = ds[0]
    ds.get_metrics(item["depth_gt"], torch.ones(3, 4), item["boundary"])
    ev = ds.evaluator()
    ev.add(item["depth_gt"], torch.ones(3, 4), disp_gt_edges=item["boundary"])
    calls = [c for c in ops.calls if c[0] == "depth_metrics"]
    assert calls == [("depth_metrics", 1e-3, 80.0, (0, 6, 0, 8), True)] * 2
    assert (ev.garg_crop, ev.eigen_crop, ev.dataset) == (False, False, "gta")


def test_image_dataset_reads_u4k_raw_images(tmp_path):
    img_dir, gt_dir = tmp_path / "images", tmp_path / "val_gt"
    img_dir.mkdir()
    gt_dir.mkdir()
    (tmp_path / "val_factor").mkdir()
    raw = np.random.RandomState(13).randint(0, 256, datasets.U4K_IMAGE_SHAPE, dtype=np.uint8)
    raw.tofile(str(img_dir / "00001.raw"))
    npy = R.npy_bytes(R.float_plane(5, 7, "f4", seed=14))
    (gt_dir / "00001.npy").write_bytes(npy)
    (tmp_path / "val_factor" / "00001.txt").write_text("1000.5\n")
    ops = FakeGtOps()
    ds = datasets.ImageDataset(str(img_dir), gt_dir=str(gt_dir), dataset_name="u4k", device="cpu", ops=ops)
    item = ds[0]
    shape, sent = next((c[1], c[2]) for c in ops.calls if c[0] == "bicubic")
    assert shape == datasets.U4K_IMAGE_SHAPE and np.array_equal(sent, raw)        # the file's bytes, B G R order: the kernel reverses them
    assert tuple(item["image_hr"].shape) == (3, 2160, 3840) and item["img_file_basename"] == "00001.raw"
    depth, _, edge = R.depth_map("u4k", npy, depth_factor=1000.5)
    assert same_bits(item["depth_gt"].numpy(), depth) and same_bits(item["boundary"][0].numpy(), edge)
    (img_dir / "00002.raw").write_bytes(bytes(10))
    with pytest.raises(ValueError):
        ds = datasets.ImageDataset(str(img_dir), dataset_name="u4k", device="cpu", ops=ops)
        ds[1]
    with pytest.raises(ValueError):                                  # ImagePreprocessor.read keeps its refusal
        ds.preprocess.read(str(img_dir / "00001.raw"))


def test_registry_builds_the_dataset(tmp_path):
    from patchfusion_amd import registry
    (tmp_path / "x.png").write_bytes(P.write_png(np.zeros((2, 2, 3), np.uint8), 2, 8))
    ds = registry.build_dataset(dict(type="ImageDataset", rgb_image_dir=str(tmp_path), dataset_name="gta", device="cpu", ops=FakeGtOps()))
    assert isinstance(ds, datasets.ImageDataset) and len(ds) == 1
    assert registry.DATASETS.get("ImageDataset") is datasets.ImageDataset
