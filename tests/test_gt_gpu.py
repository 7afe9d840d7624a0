"""Ground-truth files read on the device (csrc/gtread.hip through groundtruth.read_depth_gt) against the numpy restatement of
tests/gt_ref.py: EQUALITY OF BIT PATTERNS for depth, edge source and edges.  NaNs match NaNs whatever their sign or payload (x86 and the
GPU make different default NaNs), -0.0 must come out as -0.0; there is no tolerance, every operation being one correctly rounded
float32 operation with denormals kept.

Shapes: one-pixel planes, widths below the vector width, rows that are not 16-byte aligned, exact and ragged tile edges, a flip with an
odd H.  Values: seeded, with the planted specials of tests/gt_ref.py at the start and the end of every plane.

On the parent commit this module fails at import: patchfusion_amd.groundtruth does not exist there."""
import ctypes as C
import functools
import io

import numpy as np
import pytest
import torch

from tests import eval_side_ref as E
from tests import gt_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
DF = 1234.5678


def _mods():
    from patchfusion_amd import _lib, groundtruth, hip_ops, postprocess
    return _lib, groundtruth, hip_ops, postprocess


# ---------------------------------------------------------------- files, made once per (dataset, shape)
@functools.lru_cache(maxsize=None)
def variants(dataset, H, W):
    """[(label, file bytes, keywords of read_depth_gt)]"""
    seed = 1000 * H + W
    out = []
    if dataset == "u4k":
        for kind in ("f2", "f4", "f8"):
            for order in "<>":
                a = R.float_plane(H, W, kind, seed).astype(order + kind)
                for df in (DF, R.DENORMAL_DF):
                    out.append((f"{order}{kind} df={df}", R.npy_bytes(a, (2, 0) if order == ">" else (1, 0)), dict(depth_factor=df)))
    elif dataset == "mid":
        for little in (True, False):
            out.append((f"little={little}", R.pfm_bytes(R.float_plane(H, W, "f4", seed + 1), little), dict(calib=R.CALIB)))
    elif dataset == "eth3d":
        out.append(("raw", R.float_plane(H, W, "f4", seed + 2).astype("<f4").tobytes(), dict(shape=(H, W))))
    else:
        for depth in (16, 8):
            out.append((f"{depth} bits", R.png_bytes(R.sample_plane(H, W, depth, seed + 3, dataset), depth), dict(png_options=dict(inflate="host"))))
    return out


@functools.lru_cache(maxsize=None)
def expected(dataset, H, W, index, dilation=0):
    _, data, kw = variants(dataset, H, W)[index]
    kw = {k: v for k, v in kw.items() if k != "png_options"}
    return R.depth_map(dataset, data, th=1.0, dilation=dilation, **kw)


def check(got, want, where):
    for name, g, w in zip(("depth", "edge source", "edge"), (got.depth, got.edge_source, got.edge), want):
        g = g.cpu().numpy()
        if not R.same_bits(g, w):
            bad = np.nonzero(~((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))))
            y, x = int(bad[0][0]), int(bad[1][0])
            raise AssertionError(f"{where}: {name} differs at {len(bad[0])} pixels, first ({y}, {x}): got {g[y, x]!r} "
                                 f"(0x{g.view(np.uint32)[y, x]:08x}), want {w[y, x]!r} (0x{w.view(np.uint32)[y, x]:08x})")


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dataset", R.DATASETS)
def test_reader_equals_the_restatement_bit_for_bit(dataset, shape):
    _, gt, _, _ = _mods()
    H, W = shape
    for i, (label, data, kw) in enumerate(variants(dataset, H, W)):
        got = gt.read_depth_gt(data, dataset, **kw)
        assert got.depth.is_cuda and got.depth.dtype == torch.float32 and tuple(got.depth.shape) == shape
        check(got, expected(dataset, H, W, i), (dataset, shape, label))
        if i == 0:
            check(gt.read_depth_gt(data, dataset, dilation=3, **kw), expected(dataset, H, W, 0, 3), (dataset, shape, label, "dilation 3"))


def test_the_planted_values_do_their_work():
    """the cases reach what they are meant to reach: denormal quotients, -0.0, NaN, ties that round to even"""
    d = expected("u4k", 37, 53, [v[0] for v in variants("u4k", 37, 53)].index(f"<f4 df={R.DENORMAL_DF}"))[0]
    assert ((d != 0) & (np.abs(d) < np.finfo(F32).tiny)).any() and np.isnan(d).any()
    assert d.reshape(-1)[11] == F32(R.DENORMAL_DF) / F32(3) and 0 < d.reshape(-1)[11] < np.finfo(F32).tiny
    m = expected("mid", 37, 53, 0)[0]
    assert np.signbit(m[m == 0]).any() and np.isnan(m).any() and np.isinf(m).any()
    x8 = np.load(io.BytesIO(variants("u4k", 37, 53)[8][1]))                                   # <f8
    ties = x8.reshape(-1)[15:25]
    assert all(float(F32(t)) != t for t in ties)                                              # none is a float32: each one rounds
    for ds in ("gta", "cityscapes"):
        s = R.P.decode(variants(ds, 37, 53)[0][1]).reshape(-1)
        assert s[:6].tolist() == [0, 1, 2, 255, 256, 65535]


@pytest.mark.parametrize("dataset", ["gta", "cityscapes"])
def test_png_inflated_on_the_device(dataset):
    _, gt, _, _ = _mods()
    _, data, _ = variants(dataset, 37, 53)[0]
    got = gt.read_depth_gt(data, dataset, png_options=dict(inflate="device"))
    assert got.info.png.inflate == "device" and got.info.dtype == "u2"
    check(got, expected(dataset, 37, 53, 0), (dataset, "inflate on the device"))


def test_read_pfm_and_read_npy():
    _, gt, _, _ = _mods()
    for little in (True, False):
        for colour in (False, True):
            a = R.float_plane(37, 159 if colour else 53, "f4", 77)
            a = a.reshape(37, 53, 3) if colour else a
            got, scale = gt.read_pfm(R.pfm_bytes(a, little, 3.5, colour))
            assert scale == 3.5 and R.same_bits(got.cpu().numpy(), a), (little, colour)
    for _, data, _ in variants("u4k", 37, 130)[::2]:
        assert R.same_bits(gt.read_npy(data).cpu().numpy(), R.read_npy(data))


# ---------------------------------------------------------------- the evaluator on the device planes
def metric_file(dataset, H, W):
    """a file whose depth stays inside [3, 8] -- with a prediction inside [8.4, 32] every sum of pf_depth_metrics is then exact in
    float64 whatever the order of the kernel's atomics (tests/eval_side_ref.py metric_case), so two runs can be compared bit for bit"""
    depth = R.metric_plane(H, W, 3.2, 7.8, seed=5)
    if dataset == "u4k":
        return R.npy_bytes((DF / depth).astype("<f4")), dict(depth_factor=DF)
    if dataset == "mid":
        f, doffs, base = R.CALIB
        return R.pfm_bytes((base * f / (1000.0 * depth) - doffs).astype(F32), True), dict(calib=R.CALIB)
    if dataset == "eth3d":
        return depth.astype("<f4").tobytes(), dict(shape=(H, W))
    if dataset == "gta":
        return R.png_bytes(np.round(depth * 256).astype(np.uint16)), dict(png_options=dict(inflate="host"))
    return R.png_bytes(np.round(0.209313 * 2262.52 / depth * 256 + 1).astype(np.uint16)), dict(png_options=dict(inflate="host"))


@pytest.mark.parametrize("dataset", R.DATASETS)
def test_evaluator_sums_equal_those_of_the_restatement(dataset):
    _, gt, _, post = _mods()
    H, W = 37, 130
    data, kw = metric_file(dataset, H, W)
    depth, _, edge = R.depth_map(dataset, data, **{k: v for k, v in kw.items() if k != "png_options"})
    assert depth.min() >= 3 and depth.max() <= 8 and edge.sum() > 0
    pred = torch.from_numpy(E.metric_case(1, 2 * (H // 2), 2 * (W // 2))[1]).cuda()           # [H/2, W/2] in [8.4, 32]
    got = gt.read_depth_gt(data, dataset, **kw)
    mine, ref = post.DepthEvaluator(1e-3, 80), post.DepthEvaluator(1e-3, 80)
    mine.add(got.depth, pred, disp_gt_edges=got.edge)
    ref.add(torch.from_numpy(depth).cuda(), pred, disp_gt_edges=torch.from_numpy(edge).cuda())
    a, b = mine._buf[0].cpu().numpy(), ref._buf[0].cpu().numpy()
    assert a.shape == (13,) and a[0] == H * W and a[12] > 0
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (a, b)
    assert mine.results() == ref.results()


# ---------------------------------------------------------------- the entry point itself
def test_grid_stride_loop_and_both_load_paths():
    """more groups of four than the capped grid has threads (8192 x 256): every thread loops; W odd and a flip take the per-sample
    loads, the second call the 16-byte loads"""
    _, _, hip_ops, _ = _mods()
    H, W = 2051, 4099
    rs = np.random.RandomState(3)
    x = (rs.rand(H, W).astype(F32) * F32(300) + F32(0.5))
    src = torch.from_numpy(x).cuda()
    depth, edge = torch.empty_like(src), torch.empty_like(src)
    assert (H * W + 3) // 4 > 8192 * 256
    want = F32(DF) / x
    hip_ops.ops.gt_convert(src.view(torch.uint8).view(-1), "f4", "u4k", H, W, DF, 0.0, depth, edge, flip=True)
    assert R.same_bits(depth.cpu().numpy(), want[::-1]) and R.same_bits(edge.cpu().numpy(), x[::-1])
    hip_ops.ops.gt_convert(src.view(torch.uint8).view(-1), "f4", "u4k", H, W, DF, 0.0, depth, edge)
    assert R.same_bits(depth.cpu().numpy(), want) and R.same_bits(edge.cpu().numpy(), x)


def test_a_payload_off_the_16_byte_grid_takes_the_per_sample_loads():
    _, _, hip_ops, _ = _mods()
    H, W = 37, 52
    for kind in ("f2", "f4", "f8"):
        a = R.float_plane(H, W, kind, 9)
        size = a.dtype.itemsize
        buf = torch.zeros(size + a.nbytes, dtype=torch.uint8, device="cuda")
        buf[size:] = torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()
        for flip in (False, True):
            depth = torch.empty(H, W, dtype=torch.float32, device="cuda")
            hip_ops.ops.gt_convert(buf[size:], kind, "raw", H, W, 0.0, 0.0, depth, flip=flip)
            with np.errstate(over="ignore"):
                want = a.astype(F32)
            assert R.same_bits(depth.cpu().numpy(), want[::-1] if flip else want), (kind, flip)


def test_bad_arguments_return_pf_err_arg():
    _lib, _, hip_ops, _ = _mods()
    lib = _lib.load()
    H, W = 8, 12
    src = torch.zeros(H * W * 8 + 16, dtype=torch.uint8, device="cuda")
    depth = torch.zeros(H * W + 4, dtype=torch.float32, device="cuda")
    edge = torch.zeros(H * W + 4, dtype=torch.float32, device="cuda")
    s, d, e = src.data_ptr(), depth.data_ptr(), edge.data_ptr()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    K, M = hip_ops.HipOps.GT_KINDS, hip_ops.HipOps.GT_MODES

    def call(src=s, kind=K["f4"], flags=0, mode=M["u4k"], H=H, W=W, depth=d, edge=e):
        return lib.pf_gt_convert(C.c_void_p(src), kind, flags, mode, H, W, 1.0, 0.0, C.c_void_p(depth), C.c_void_p(edge), stream)

    assert call() == 0 and call(edge=None) == 0
    bad = dict(null_src=dict(src=None), null_depth=dict(depth=None), zero_h=dict(H=0), negative_w=dict(W=-1), zero_w=dict(W=0),
               plane_of_2_31=dict(H=65536, W=32768), kind_5=dict(kind=5), kind_negative=dict(kind=-1), mode_6=dict(mode=6),
               mode_negative=dict(mode=-1), flag_4=dict(flags=4), u16_u4k=dict(kind=K["u2"]), u8_raw=dict(kind=K["u1"], mode=M["raw"]),
               f16_mid=dict(kind=K["f2"], mode=M["mid"]), f64_eth3d=dict(kind=K["f8"], mode=M["eth3d"]),
               f32_gta=dict(mode=M["gta"]), f32_cityscapes=dict(mode=M["cityscapes"]), swapped_eth3d=dict(mode=M["eth3d"], flags=1),
               swapped_gta=dict(kind=K["u2"], mode=M["gta"], flags=1), src_off_its_sample=dict(src=s + 2), depth_off_16=dict(depth=d + 4),
               edge_off_16=dict(edge=e + 8))
    for name, kw in bad.items():
        assert call(**kw) == 1, name
    torch.cuda.synchronize()
    assert call(kind=K["u2"], mode=M["gta"]) == 0 and call(mode=M["eth3d"]) == 0 and call(mode=M["mid"], flags=3) == 0
    torch.cuda.synchronize()


def test_the_op_refuses_cpu_tensors():
    _lib, _, hip_ops, _ = _mods()
    src = torch.zeros(4 * 6 * 4, dtype=torch.uint8)
    depth = torch.zeros(4, 6, dtype=torch.float32)
    with pytest.raises(_lib.PfError):
        hip_ops.ops.gt_convert(src, "f4", "u4k", 4, 6, 1.0, 0.0, depth)
    with pytest.raises(_lib.PfError):
        hip_ops.ops.gt_convert(src.cuda(), "f4", "u4k", 4, 6, 1.0, 0.0, depth)
    with pytest.raises(ValueError):
        hip_ops.ops.gt_convert(src.cuda(), "i4", "u4k", 4, 6, 1.0, 0.0, depth.cuda())
