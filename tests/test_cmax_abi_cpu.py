"""CPU-side checks of the channel-maxima entry points (no launch, no GPU): the argument rules of the producers' _ex calls (csrc/imageops.hip) and the
route rule for layers whose maxima are given (csrc/gemm_split3.hip f16x2_points_route through pf_gemm_f16x2_points_route_ex)."""
import ctypes as C
import os

import pytest

P128, P192, NONE = 2, 3, -1
ERR_ARG = 1
BF16, F32 = 1, 0


@pytest.fixture
def L(monkeypatch):
    from patchfusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpf_hip.so not built")
    for v in ("PF_S3_TILE_NOW", "PF_S3_PERSIST", "PF_S3_T192", "PF_S3_GRID", "PF_WINO_F16X2_N256"):
        monkeypatch.delenv(v, raising=False)
    return _lib.load()


def _params(T, K, N=256):
    from patchfusion_amd import _lib
    p = _lib.ConvParams()
    p.B, p.OH, p.OW, p.H, p.W, p.Cin, p.Cout, p.batch = 1, 1, T, 1, T, K, N, 36
    return p


def test_producers_refuse_maxima_outside_float32_and_null_tensors(L):
    """(fake non-null pointers: every call returns before a launch)"""
    x, y, cm = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)
    assert L.pf_copy_channels_ex(None, 8, y, 8, 4, 8, 1, 1, F32, cm, None) == ERR_ARG
    assert L.pf_copy_channels_ex(x, 8, y, 8, 4, 8, 0, 0, BF16, cm, None) == ERR_ARG          # maxima: float32 calls only
    assert L.pf_copy_channels_ex(x, 8, y, 8, 4, 12, 1, 1, F32, cm, None) == ERR_ARG          # C % 8
    assert L.pf_roi_align_ex(x, 8, 1, 4, 4, 8, None, 1, y, 8, 4, 4, 1.0, 1, 1, F32, cm, None) == ERR_ARG
    assert L.pf_roi_align_ex(x, 8, 1, 4, 4, 8, x, 1, y, 8, 4, 4, 1.0, 0, 0, BF16, cm, None) == ERR_ARG
    assert L.pf_roi_align_ex(x, 1, 1, 4, 4, 1, x, 1, y, 1, 4, 4, 1.0, 1, 1, F32, cm, None) == ERR_ARG      # the planar depth map has no maxima
    assert L.pf_resize_bilinear_ex(x, 8, 1, 4, 4, 8, y, 8, 8, 8, None, 0, 0, 0, BF16, cm, None) == ERR_ARG
    assert L.pf_resize_bilinear_ex(None, 8, 1, 4, 4, 8, y, 8, 8, 8, None, 0, 1, 1, F32, cm, None) == ERR_ARG
    n = 2
    ptrs = (C.c_void_p * n)(0x1000, 0x1100)
    arr = lambda *v: (C.c_int * n)(*v)
    assert L.pf_resize_concat_ex(ptrs, arr(8, 8), arr(4, 4), arr(4, 4), arr(8, 8), n, 1, y, 16, 8, 8, BF16, cm, None) == ERR_ARG
    assert L.pf_resize_concat_ex(ptrs, arr(8, 8), arr(4, 4), arr(4, 4), arr(8, 12), n, 1, y, 16, 8, 8, F32, cm, None) == ERR_ARG
    assert L.pf_zero_u32(None, 4, None) == ERR_ARG and L.pf_zero_u32(cm, 0, None) == ERR_ARG


# the 256-column layers of the DA-ViT-L 4K pass, 8 tiles per batch: (H, W, K, fp16x2 by the default rule, fp16x2 under PF_WINO_F16X2_N256=5 with maxima given)
LAYERS = [(224, 296, 768, True, True), (224, 296, 256, False, True), (112, 148, 512, True, True), (112, 148, 256, False, True),
          (98, 129, 256, False, True), (56, 74, 512, False, True), (56, 74, 256, False, True)]


@pytest.mark.parametrize("H,W,K,dflt,wide", LAYERS)
def test_given_maxima_change_the_route_only_under_the_opt_in_switch(L, monkeypatch, H, W, K, dflt, wide):
    p = _params(8 * -(-H // 4) * -(-W // 4), K)
    for mode in (None, "1", "2", "0", "3"):
        if mode is None:
            monkeypatch.delenv("PF_WINO_F16X2_N256", raising=False)
        else:
            monkeypatch.setenv("PF_WINO_F16X2_N256", mode)
        plain = L.pf_gemm_f16x2_points_route(C.byref(p), 256)
        assert L.pf_gemm_f16x2_points_route_ex(C.byref(p), 256, 0) == plain
        assert L.pf_gemm_f16x2_points_route_ex(C.byref(p), 256, 1) == plain, "given maxima must not change the product at this switch"
        if mode in (None, "1", "2"):
            assert plain == (P128 if dflt else NONE)
    monkeypatch.setenv("PF_WINO_F16X2_N256", "5")
    assert L.pf_gemm_f16x2_points_route_ex(C.byref(p), 256, 0) == (P128 if dflt else NONE)
    assert L.pf_gemm_f16x2_points_route_ex(C.byref(p), 256, 1) == (P128 if wide else NONE)


def test_the_wider_rule_has_its_edges_at_k_256_and_2128_tiles(L, monkeypatch):
    monkeypatch.setenv("PF_WINO_F16X2_N256", "5")
    assert L.pf_gemm_f16x2_points_route_ex(C.byref(_params(2128, 256)), 256, 1) == P128
    assert L.pf_gemm_f16x2_points_route_ex(C.byref(_params(2127, 256)), 256, 1) == NONE
    assert L.pf_gemm_f16x2_points_route_ex(C.byref(_params(2128, 224)), 256, 1) == NONE
    assert L.pf_gemm_f16x2_points_route_ex(C.byref(_params(8 * 56 * 74, 544, 544)), 256, 1) == P192      # the 192-tile layers do not depend on it
    assert L.pf_gemm_f16x2_points_route_ex(None, 256, 1) == -1 and L.pf_gemm_f16x2_points_route_ex(C.byref(_params(2128, 256)), 0, 1) == -1
