"""pytest -m gpu: the 256-column three-step Winograd layers on the 128-tile fp16x2 product (csrc/wino_f16x2_n256.hip, pf_gemm_f16x2_points128).

Shapes that take the new kernel at DEFAULT switches, and smaller ones through PF_WINO_F16X2_N256=3 (the route is asserted: `wino3h` from the plan, PF_S3_ROUTE_PERSIST128 from
pf_gemm_f16x2_points_route on the whole layer's product).  Per case, from cold caches and NaN-filled outputs: element-wise and normwise error against
float64 samples (tests/f64_ref.py), held to the bars of every split Winograd route -- within 2x of the f32 three-step route on the same operands,
normwise <= NORM_CAP_WINO (3.2e-5), element-wise <= ELEM_CAP_WINO.  Several windows give the bits of one window, two launches give the same bits,
PF_WINO_F16X2_N256=0 puts the layer back on the bf16x3 planes, and a non-finite input pixel comes out non-finite."""
import ctypes as C
import os

import pytest
import torch

from patchfusion_amd import packing as pk
from tests import f64_ref as R
from tests import op_checks
from tests.test_float32_grade_gpu import _input, _operands

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("PF_WINOGRAD", "PF_WINOGRAD_MIN_PIXELS", "PF_WINO_FUSED", "PF_WS_CAP_GB", "PF_WINO_F16X2", "PF_WINO_F16X2_N256", "PF_WINO_SPLIT3", "PF_S3_PERSIST",
        "PF_S3_T192", "PF_S3_TILE_NOW")
P128 = 2


@pytest.fixture
def env():
    old = {k: os.environ.get(k) for k in KEYS}

    def set_env(**kw):
        for k in KEYS:
            os.environ.pop(k, None)
        os.environ.update(kw)
        op_checks._switches_changed()
    yield set_env
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    op_checks._switches_changed()


def _points_route(B, H, W, cin, cout, rows):
    from patchfusion_amd import _lib
    L = _lib.load()
    T = B * -(-H // 4) * -(-W // 4)
    q = _lib.ConvParams()
    q.B, q.OH, q.OW, q.H, q.W, q.Cin, q.Cout, q.batch, q.w_rows = 1, 1, T, 1, T, cin, cout, 36, rows
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return L.pf_gemm_f16x2_points_route(C.byref(q), cus)


def _plan_route(x, pw, y, o, r1):
    from patchfusion_amd.hip_ops import HipOps
    return HipOps._conv_plan(x, pw, y, 1, 1, o.get("act"), o.get("relu_in", False), r1, None, None)[0]


def _run(x, pw, y, o, r1):
    from patchfusion_amd.hip_ops import ops
    y.fill_(float("nan"))
    op_checks._flush_caches()
    ops.conv(x, pw, y, pad=1, act=o.get("act"), relu_in=o.get("relu_in", False), res=r1)
    torch.cuda.synchronize()
    assert not torch.isnan(y).any(), "an output element was not written"


# name, (B, H, W, cin, cout), options, kind, switches
# (switches {}: the layer takes the kernel by the default rule -- K >= 512 and at least 4096 tiles; PF_WINO_F16X2_N256=3: every PERSIST128 layer)
CASES = [
    ("512_256_random", (4, 112, 148, 512, 256), dict(act="relu"), "random", {}),
    ("512_256_pow40", (4, 112, 148, 512, 256), {}, "pow40", {}),
    ("512_256_cols", (4, 112, 148, 512, 256), dict(res=True), "cols", {}),
    ("768_256_ragged_wide", (5, 99, 133, 768, 256), dict(act="relu", relu_in=True, res=True), "wide", {}),
    ("768_256_ragged_spike", (5, 99, 133, 768, 256), {}, "spike", {}),
    ("768_256_ragged_dead", (5, 99, 133, 768, 256), dict(act="relu"), "dead", {}),
    ("512_256_small_random", (8, 56, 74, 512, 256), dict(act="relu"), "random", dict(PF_WINO_F16X2_N256="3")),
    ("256_256_wide", (2, 112, 148, 256, 256), dict(act="relu", relu_in=True, res=True), "wide", dict(PF_WINO_F16X2_N256="3")),
    ("320_256_ragged_wide", (3, 75, 101, 320, 256), dict(relu_in=True), "wide", dict(PF_WINO_F16X2_N256="3")),
]


@pytest.mark.parametrize("name,shape,opts,kind,sw", CASES, ids=[c[0] for c in CASES])
def test_n256_layer_is_float32_grade_and_window_free(env, name, shape, opts, kind, sw):
    from patchfusion_amd import hip_ops
    B, H, W, cin, cout = shape
    env(**sw)
    seed = sum(map(ord, name))
    w, b, s = _operands(kind, cout, cin, 3, seed)
    pw = pk.pack_conv(w, b, dtype=torch.float32).to(DEV)
    x = _input((B, H, W, cin), s, kind, seed + 3).to(DEV)
    r1 = torch.randn(B, H, W, cout, generator=torch.Generator().manual_seed(seed + 4)).to(DEV) if opts.get("res") else None
    y = torch.empty(B, H, W, cout, device=DEV)
    assert _plan_route(x, pw, y, opts, r1) == "wino3h", name
    assert _points_route(B, H, W, cin, cout, pw.wino_u.shape[1]) == P128, name
    window = hip_ops.wino3_window(B, H, W, pw)[0]
    pix = R.sample_pixels(B, H, W, n_random=192, seed=seed, window=window)
    ref, mag = R.conv_ref(x, w, pix, b, 1, 1, opts.get("act"), opts.get("relu_in", False), None, r1, None)

    _run(x, pw, y, opts, r1)
    y_one = y.clone()
    e = R.errors(R.gather_pixels(y, pix, cout), ref, mag)
    _run(x, pw, y, opts, r1)
    assert torch.equal(y, y_one), "two launches differ"

    env(PF_WS_CAP_GB="0.005", **sw)
    assert _plan_route(x, pw, y, opts, r1) == "wino3h" and hip_ops.wino3_window(B, H, W, pw)[1] >= 2
    _run(x, pw, y, opts, r1)
    assert torch.equal(y, y_one), "windows changed the numbers"

    env(PF_WINO_F16X2_N256="0")
    assert _plan_route(x, pw, y, opts, r1) == "wino3", "the switch must put the layer back on three bf16 planes"
    _run(x, pw, y, opts, r1)
    e3 = R.errors(R.gather_pixels(y, pix, cout), ref, mag)

    env(PF_WINO_SPLIT3="0", PF_WINO_FUSED="0")
    assert _plan_route(x, pw, y, opts, r1) == "wino"
    _run(x, pw, y, opts, r1)
    base = R.errors(R.gather_pixels(y, pix, cout), ref, mag)
    print(f"{name:24s} {kind:6s} fp16x2 elem {e[0]:.2e} norm {e[1]:.2e} | bf16x3 elem {e3[0]:.2e} norm {e3[1]:.2e} | f32 elem {base[0]:.2e} norm {base[1]:.2e}")
    assert base[1] <= R.NORM_CAP_WINO and base[0] <= R.ELEM_CAP_WINO, ("f32 three-step route", base)
    assert R.float32_grade(e, base, R.NORM_CAP_WINO, R.ELEM_CAP_WINO), (name, e, base)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_n256_non_finite_input_gives_non_finite_output(env, bad):
    env()
    B, H, W, cin, cout = 4, 112, 148, 512, 256
    w, b, s = _operands("random", cout, cin, 3, 11)
    xc = _input((B, H, W, cin), s, "random", 12)
    xc[1, 57, 93, 100] = bad
    pw = pk.pack_conv(w, b, dtype=torch.float32).to(DEV)
    x = xc.to(DEV)
    y = torch.empty(B, H, W, cout, device=DEV)
    assert _plan_route(x, pw, y, {}, None) == "wino3h" and _points_route(B, H, W, cin, cout, pw.wino_u.shape[1]) == P128
    from patchfusion_amd.hip_ops import ops
    op_checks._flush_caches()
    ops.conv(x, pw, y, pad=1)
    torch.cuda.synchronize()
    assert not torch.isfinite(y[1, 56:59, 92:95]).all(), "a non-finite input pixel must not come out finite"


def test_points128_gives_the_bits_of_the_192_tile_product(env):
    """the two fp16x2 products run the same chunk order and the same three terms per accumulator: identical M on the same planes"""
    from patchfusion_amd import _lib, hip_ops
    env()
    L = _lib.load()
    T, K, N, rows = 1000, 256, 200, 208
    g = torch.Generator().manual_seed(3)
    V2 = torch.randn(2, 36, K // 32, T, 32, generator=g).half().to(DEV)
    U2 = torch.randn(2, 36, K // 32, rows, 32, generator=g).half().to(DEV)
    fe = torch.randint(-6, 7, (36, rows), generator=g, dtype=torch.int32).to(DEV)
    q = _lib.ConvParams()
    q.x_ld, q.B, q.H, q.W, q.Cin, q.w_rows, q.Kpad = K, 1, 1, T, K, rows, K
    q.y_ld, q.OH, q.OW, q.Cout, q.KH, q.KW, q.stride, q.pad = N, 1, T, N, 1, 1, 1, 0
    q.act, q.shuffle, q.dtype, q.out_f32, q.korder, q.batch = 0, 1, 1, 1, 6, 36
    q.x, q.w, q.x_bstride, q.w_bstride = V2.data_ptr(), U2.data_ptr(), 36 * T * K, 36 * rows * K
    out = []
    for fn, nm in ((L.pf_gemm_f16x2_points, "pf_gemm_f16x2_points"), (L.pf_gemm_f16x2_points128, "pf_gemm_f16x2_points128")):
        M = torch.full((36, T, N), float("nan"), device=DEV)
        q.y = M.data_ptr()
        op_checks._flush_caches()
        hip_ops.check(fn(C.byref(q), C.c_void_p(fe.data_ptr()), 0, None), nm)
        torch.cuda.synchronize()
        out.append(M)
    assert not torch.isnan(out[1]).any()
    assert torch.equal(out[0], out[1])
    Vd, Ud = V2.double(), U2[:, :, :, :N].double()           # (h + l)(h + l) - l l = the three terms the kernel sums
    ref = torch.ldexp(torch.einsum("pktc,pknc->ptn", Vd[0] + Vd[1], Ud[0] + Ud[1]) - torch.einsum("pktc,pknc->ptn", Vd[1], Ud[1]), fe.double()[:, None, :N])
    assert float((out[1].double() - ref).abs().max() / ref.abs().max()) < 1e-5


def _tiny_product(L, T, K, N, rows, grid_cap, seed):
    from patchfusion_amd import _lib, hip_ops
    g = torch.Generator().manual_seed(seed)
    V2 = torch.randn(2, 36, K // 32, T, 32, generator=g).half().to(DEV)
    U2 = torch.randn(2, 36, K // 32, rows, 32, generator=g).half().to(DEV)
    fe = torch.randint(-6, 7, (36, rows), generator=g, dtype=torch.int32).to(DEV)
    q = _lib.ConvParams()
    q.x_ld, q.B, q.H, q.W, q.Cin, q.w_rows, q.Kpad = K, 1, 1, T, K, rows, K
    q.y_ld, q.OH, q.OW, q.Cout, q.KH, q.KW, q.stride, q.pad = N, 1, T, N, 1, 1, 1, 0
    q.act, q.shuffle, q.dtype, q.out_f32, q.korder, q.batch = 0, 1, 1, 1, 6, 36
    q.x, q.w, q.x_bstride, q.w_bstride = V2.data_ptr(), U2.data_ptr(), 36 * T * K, 36 * rows * K
    M = torch.full((36, T, N), float("nan"), device=DEV)
    q.y = M.data_ptr()
    hip_ops.check(L.pf_gemm_f16x2_points128(C.byref(q), C.c_void_p(fe.data_ptr()), grid_cap, None), "pf_gemm_f16x2_points128")
    torch.cuda.synchronize()
    Vd, Ud = V2.double(), U2[:, :, :, :N].double()
    ref = torch.ldexp(torch.einsum("pktc,pknc->ptn", Vd[0] + Vd[1], Ud[0] + Ud[1]) - torch.einsum("pktc,pknc->ptn", Vd[1], Ud[1]), fe.double()[:, None, :N])
    assert not torch.isnan(M).any()
    return float((M.double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("T,K,N,rows,cap", [(100, 32, 64, 64, 0), (300, 64, 128, 128, 0), (700, 96, 256, 256, 16), (2000, 160, 72, 80, 8)],
                         ids=["k32_one_tile", "k64", "k96_cap16", "k160_cap8"])
def test_points128_short_k_few_tiles_and_grid_cap(env, T, K, N, rows, cap):
    """the ring's fill and tails (one, two and three chunks per tile; tiles of several chunks walked by few blocks) against float64 of the same planes:
    three exact fp16 products per term summed in float32 -- 1e-5 is a loose float32 bound"""
    from patchfusion_amd import _lib
    env()
    assert _tiny_product(_lib.load(), T, K, N, rows, cap, K + T) < 1e-5


def _absmax_ref(L, t, relu):
    from patchfusion_amd import hip_ops
    Cc = t.shape[-1]
    cm = torch.zeros(Cc, dtype=torch.int32, device=DEV)
    hip_ops.check(L.pf_wino_absmax(C.c_void_p(t.data_ptr()), t.stride(-2), t.numel() // Cc, Cc, int(relu), C.c_void_p(cm.data_ptr()), None), "pf_wino_absmax")
    torch.cuda.synchronize()
    return cm


@pytest.mark.parametrize("producer", ["wino3", "wino3h"])
@pytest.mark.parametrize("relu", [False, True], ids=["abs", "relu"])
@pytest.mark.parametrize("windows", [False, True], ids=["one_window", "windows"])
def test_producer_maxima_equal_the_range_pass_and_output_bits_are_unchanged(env, producer, relu, windows):
    """the maxima-merging output transform: y has the bits of wino_output_kernel<4> on the same layer, and the maxima it hands over are the bits
    wino_absmax_kernel computes on that y -- with a residual in the producer's epilogue, with and without the consumer's relu_in, over several windows"""
    from patchfusion_amd import _lib, hip_ops
    from patchfusion_amd.hip_ops import HipOps
    L = _lib.load()
    sw = dict(PF_WINO_F16X2_N256="3" if producer == "wino3h" else "0")
    if windows:
        sw["PF_WS_CAP_GB"] = "0.005"
    env(**sw)
    B, H, W, cin, cout = 3, 75, 101, 320, 256
    w, b, s = _operands("wide", cout, cin, 3, 21)
    pw = pk.pack_conv(w, b, dtype=torch.float32).to(DEV)
    x = _input((B, H, W, cin), s, "wide", 22).to(DEV)
    r1 = torch.randn(B, H, W, cout, generator=torch.Generator().manual_seed(23)).to(DEV)
    y0 = torch.full((B, H, W, cout), float("nan"), device=DEV)
    y1 = torch.full((B, H, W, cout), float("nan"), device=DEV)
    route, p, extra = HipOps._conv_plan(x, pw, y0, 1, 1, None, False, r1, None, None)
    assert route == producer
    if windows:
        assert hip_ops.wino3_window(B, H, W, pw)[1] >= 2
    HipOps._conv_exec(route, p, extra, x.device)
    cm = torch.full((cout,), 0x7fffffff, dtype=torch.int32, device=DEV)          # (garbage: the call zeroes it)
    p.y = y1.data_ptr()
    HipOps._conv_exec(route, p, extra, x.device, cmax_out=cm, cmax_out_relu=relu)
    torch.cuda.synchronize()
    assert torch.equal(y0, y1), "the maxima-merging output transform changed y"
    assert torch.equal(cm, _absmax_ref(L, y1, relu))
    expect = (y1.clamp_min(0) if relu else y1.abs()).amax(dim=(0, 1, 2))
    assert torch.equal(cm.view(torch.float32), expect)


@pytest.mark.parametrize("relu_in", [False, True], ids=["plain", "relu_in"])
def test_two_layer_chain_gives_the_same_bits_with_the_hand_over_as_with_the_range_pass(env, relu_in):
    from patchfusion_amd import hip_ops
    from patchfusion_amd.hip_ops import HipOps, ops
    B, H, W, Cc = 4, 112, 148, 512
    w1, b1, s = _operands("wide", Cc, Cc, 3, 31)
    w2, b2, _ = _operands("random", 256, Cc, 3, 32)
    x = _input((B, H, W, Cc), s, "wide", 33).to(DEV)
    outs = {}
    for mode in ("1", "2"):
        env(PF_WINO_F16X2_N256=mode, PF_WS_CAP_GB="0.02")
        pw1 = pk.pack_conv(w1, b1, dtype=torch.float32).to(DEV)
        pw2 = pk.pack_conv(w2, b2, dtype=torch.float32).to(DEV)
        t = torch.full((B, H, W, Cc), float("nan"), device=DEV)
        y = torch.full((B, H, W, 256), float("nan"), device=DEV)
        kw1, kw2 = dict(pad=1, act=None if relu_in else "relu", relu_in=True), dict(pad=1, relu_in=relu_in, res=None)
        assert HipOps._conv_plan(x, pw1, t, 1, 1, kw1["act"], True, None, None, None)[0] in ("wino3", "wino3h")
        assert HipOps._conv_plan(t, pw2, y, 1, 1, None, relu_in, None, None, None)[0] == "wino3h"
        assert hip_ops._cmax_handover_enabled() == (mode == "1")
        op_checks._flush_caches()
        ops.conv_chain(x, pw1, t, pw2, y, kw1, kw2)
        torch.cuda.synchronize()
        assert not torch.isnan(y).any()
        outs[mode] = (t, y)
    assert torch.equal(outs["1"][0], outs["2"][0]) and torch.equal(outs["1"][1], outs["2"][1])
