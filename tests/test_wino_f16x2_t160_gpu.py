"""pytest -m gpu: the batched fp16x2 transform-domain product of the three-step Winograd layers on the 160 x 256 tile (csrc/wino_f16x2_t160.hip,
pf_gemm_f16x2_points160) against the forms it may replace, bit for bit.

Product level: M from the new launch equals M from pf_gemm_f16x2_points (192 x 192 tiles), or from pf_gemm_f16x2_points128 where the 192-tile entry
refuses the shape (fewer than 8 tiles), on random chunk-major planes and random column exponents; outputs NaN-filled, NaN guard floats on both sides
of M untouched; a second launch gives the same bits.  Shapes: the smallest that reach each path (tests/test_wino_f16x2_t160_model_cpu.py replays the
same list on the host and must pass before this file runs on a device).

Layer level: pf_conv_winograd_f16x2_windowed_ex with PF_WINO_F16_TILE=0 and =1, one window and three windows with a ragged last one: the same y bits,
and at =1 the float64 grade tests/test_float32_grade_gpu.py holds the wino3h route to."""
import ctypes as C
import os

import pytest
import torch

from patchfusion_amd import packing as pk
from tests import f64_ref as R
from tests import op_checks
from tests.test_float32_grade_gpu import WINO, _input, _operands
from tests.test_wino_f16x2_t160_model_cpu import IDS, PRODUCT_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("PF_WINOGRAD", "PF_WINOGRAD_MIN_PIXELS", "PF_WINO_FUSED", "PF_WS_CAP_GB", "PF_WINO_F16X2", "PF_WINO_F16X2_N256", "PF_WINO_SPLIT3", "PF_S3_PERSIST",
        "PF_S3_T192", "PF_S3_TILE_NOW", "PF_WINO_F16_TILE", "PF_S3_GRID")
GUARD = 64                                                 # floats on each side of M (keeps M 16-byte aligned)


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


def _launch(fn, name, q, fe, cap, n):
    from patchfusion_amd import hip_ops
    buf = torch.full((2 * GUARD + n,), float("nan"), device=DEV)
    q.y = buf.data_ptr() + 4 * GUARD
    op_checks._flush_caches()
    hip_ops.check(fn(C.byref(q), C.c_void_p(fe.data_ptr()), cap, None), name)
    torch.cuda.synchronize()
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all(), f"{name} wrote outside M"
    return buf[GUARD:GUARD + n]


@pytest.mark.parametrize("case", PRODUCT_CASES, ids=IDS)
def test_points160_gives_the_bits_of_the_existing_forms(env, case):
    from patchfusion_amd import _lib
    env()
    L = _lib.load()
    T, K, N, rows, batch, cap = case
    g = torch.Generator().manual_seed(T * 1000 + K + N + rows + batch)
    V2 = torch.randn(2, batch, K // 32, T, 32, generator=g).half().to(DEV)
    U2 = torch.randn(2, batch, K // 32, rows, 32, generator=g).half().to(DEV)
    fe = torch.randint(-6, 7, (batch, rows), generator=g, dtype=torch.int32).to(DEV)
    q = _lib.ConvParams()
    q.x_ld, q.B, q.H, q.W, q.Cin, q.w_rows, q.Kpad = K, 1, 1, T, K, rows, K
    q.y_ld, q.OH, q.OW, q.Cout, q.KH, q.KW, q.stride, q.pad = N, 1, T, N, 1, 1, 1, 0
    q.act, q.shuffle, q.dtype, q.out_f32, q.korder, q.batch = 0, 1, 1, 1, 6, batch
    q.x, q.w, q.x_bstride, q.w_bstride = V2.data_ptr(), U2.data_ptr(), batch * T * K, batch * rows * K
    n = batch * T * N
    t192 = -(-T // 192) * -(-N // 192) * batch
    ref_fn, ref_nm = (L.pf_gemm_f16x2_points, "pf_gemm_f16x2_points") if t192 >= 8 else (L.pf_gemm_f16x2_points128, "pf_gemm_f16x2_points128")
    want = _launch(ref_fn, ref_nm, q, fe, 0, n)
    assert not torch.isnan(want).any()
    got = _launch(L.pf_gemm_f16x2_points160, "pf_gemm_f16x2_points160", q, fe, cap, n)
    assert not torch.isnan(got).any(), "an element of M was not written"
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"differs from {ref_nm}"
    again = _launch(L.pf_gemm_f16x2_points160, "pf_gemm_f16x2_points160", q, fe, cap, n)
    assert torch.equal(again.view(torch.int32), got.view(torch.int32)), "two launches differ"


# name, (B, H, W, cin, cout), switches of the fp16x2 arms, Winograd tiles, window of the three-window run
LAYERS = [
    ("768_768", (2, 48, 52, 768, 768), {}, 312, 128),
    ("512_256", (2, 84, 88, 512, 256), dict(PF_WINO_F16X2_N256="3"), 924, 312),
]
_BASE = {}


def _layer(name, shape, win3):
    """operands, float64 samples and the f32 three-step baseline of a layer: computed once, shared by its cases, never changed"""
    if name not in _BASE:
        B, H, W, cin, cout = shape
        seed = sum(map(ord, name))
        w, b, s = _operands("wide", cout, cin, 3, seed)
        x = _input((B, H, W, cin), s, "wide", seed + 3).to(DEV)
        r1 = torch.randn(B, H, W, cout, generator=torch.Generator().manual_seed(seed + 4)).to(DEV)
        pw = pk.pack_conv(w, b, dtype=torch.float32).to(DEV)
        pix = R.sample_pixels(B, H, W, n_random=192, seed=seed, window=win3)
        ref, mag = R.conv_ref(x, w, pix, b, 1, 1, "relu", False, None, r1, None)
        _BASE[name] = dict(x=x, r1=r1, pw=pw, pix=pix, ref=ref, mag=mag, base=None)
    return _BASE[name]


def _tile_decision(shape):
    """what the library decides, under the switches of the moment, for the whole layer's product on this device"""
    from patchfusion_amd import _lib
    B, H, W, cin, cout = shape
    T = B * -(-H // 4) * -(-W // 4)
    q = _lib.ConvParams()
    q.B, q.OH, q.OW, q.H, q.W, q.Cin, q.Cout, q.batch, q.w_rows = 1, 1, T, 1, T, cin, cout, 36, cout
    return _lib.load().pf_wino_f16x2_tile_route(C.byref(q), torch.cuda.get_device_properties(0).multi_processor_count)


def _direct_call(d, shape, window):
    """pf_conv_winograd_f16x2_windowed_ex on buffers of this test's own (NaN-filled y); the switches are read by the library per call"""
    from patchfusion_amd import _lib, hip_ops
    from patchfusion_amd.hip_ops import HipOps
    L = _lib.load()
    B, H, W, cin, cout = shape
    pw, x, r1 = d["pw"], d["x"], d["r1"]
    y = torch.full((B, H, W, cout), float("nan"), device=DEV)
    p = HipOps._conv_plan(x, pw, y, 1, 1, "relu", False, r1, None, None)[1]
    T = B * -(-H // 4) * -(-W // 4)
    win = window or -(-T // 8) * 8
    rows, kpad = pw.wino_u.shape[1], pw.wino_u.shape[2]
    V2 = torch.empty(2 * 36 * win * cin, dtype=torch.float16, device=DEV)
    M = torch.empty(36 * win * cout, device=DEV)
    S = torch.empty(L.pf_wino_f16x2_scratch_bytes(cin, rows), dtype=torch.uint8, device=DEV)
    op_checks._flush_caches()
    hip_ops.check(L.pf_conv_winograd_f16x2_windowed_ex(C.byref(p), C.c_void_p(pw.wino_u.data_ptr()), rows, kpad, C.c_void_p(V2.data_ptr()),
                                                       C.c_void_p(M.data_ptr()), C.c_void_p(S.data_ptr()), window, None, None, 0, None),
                  "pf_conv_winograd_f16x2_windowed_ex")
    torch.cuda.synchronize()
    assert not torch.isnan(y).any(), "an output element was not written"
    return y


@pytest.mark.parametrize("windows", [1, 3], ids=["one_window", "three_windows"])
@pytest.mark.parametrize("name,shape,sw,tiles,win3", LAYERS, ids=[c[0] for c in LAYERS])
def test_layer_on_the_new_tile_has_the_bits_of_the_old_forms_and_the_float64_grade(env, name, shape, sw, tiles, win3, windows):
    from patchfusion_amd.hip_ops import HipOps, ops
    B, H, W, cin, cout = shape
    assert B * -(-H // 4) * -(-W // 4) == tiles
    window = 0 if windows == 1 else win3
    if windows == 3:
        assert -(-tiles // win3) == 3 and tiles % win3, "three windows, the last one ragged"
    d = _layer(name, shape, win3)
    env(PF_WINO_F16_TILE="0", **sw)
    assert _tile_decision(shape) == 0
    y0 = _direct_call(d, shape, window)
    env(PF_WINO_F16_TILE="1", **sw)
    assert _tile_decision(shape) == 1, "the switch must put the layer on the 160 x 256 tile"
    y1 = _direct_call(d, shape, window)
    assert torch.equal(y1.view(torch.int32), y0.view(torch.int32)), "the 160 x 256 tile changed the layer's bits"
    if windows == 3:                                       # the decision is per layer: three windows give the bits of one
        assert torch.equal(_direct_call(d, shape, 0).view(torch.int32), y1.view(torch.int32)), "windows changed the bits on the 160 x 256 tile"
    e = R.errors(R.gather_pixels(y1, d["pix"], cout), d["ref"], d["mag"])
    if d["base"] is None:                                  # the f32 three-step route on the same operands, as tests/test_float32_grade_gpu.py takes it
        env(PF_WINO_SPLIT3="0", **WINO)
        x, pw, r1 = d["x"], d["pw"], d["r1"]
        yb = torch.full((B, H, W, cout), float("nan"), device=DEV)
        assert HipOps._conv_plan(x, pw, yb, 1, 1, "relu", False, r1, None, None)[0] == "wino"
        ops.conv(x, pw, yb, pad=1, act="relu", res=r1)
        torch.cuda.synchronize()
        d["base"] = R.errors(R.gather_pixels(yb, d["pix"], cout), d["ref"], d["mag"])
    base = d["base"]
    print(f"{name:10s} windows {windows} fp16x2 on 160x256 elem {e[0]:.2e} norm {e[1]:.2e} | f32 three-step elem {base[0]:.2e} norm {base[1]:.2e}")
    assert base[1] <= R.NORM_CAP_WINO and base[0] <= R.ELEM_CAP_WINO, ("f32 three-step route", base)
    assert R.float32_grade(e, base, R.NORM_CAP_WINO, R.ELEM_CAP_WINO), (name, e, base)
