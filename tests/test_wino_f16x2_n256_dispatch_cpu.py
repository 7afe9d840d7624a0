"""The dispatch rule of the fp16x2 Winograd product (csrc/gemm_split3.hip f16x2_points_route through pf_gemm_f16x2_points_route; no launch, no GPU):
which layers of the 4K pass take the 128-tile fp16x2 kernel of csrc/wino_f16x2_n256.hip on a 256-CU chip, and which shapes the GPU tests pin elsewhere."""
import ctypes as C
import os

import pytest

P128, P192, NONE = 2, 3, -1


@pytest.fixture
def route(monkeypatch):
    from patchfusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpf_hip.so not built")
    L = _lib.load()
    for v in ("PF_S3_TILE_NOW", "PF_S3_PERSIST", "PF_S3_T192", "PF_S3_GRID", "PF_WINO_F16X2_N256"):
        monkeypatch.delenv(v, raising=False)

    def f(B, H, W, K, N, cus=256):
        T = B * -(-H // 4) * -(-W // 4)
        p = _lib.ConvParams()
        p.B, p.OH, p.OW, p.H, p.W, p.Cin, p.Cout, p.batch = 1, 1, T, 1, T, K, N, 36
        return L.pf_gemm_f16x2_points_route(C.byref(p), cus)
    f.L = L
    return f


# the 256-column layers of the DA-ViT-L 4K pass, 8 tiles per batch (DESIGN.md 4e'): (H, W, K, fp16x2 at default switches).  The rule keeps the layers
# that measured faster as a whole (profiles/r11_n256_sweep.md): K >= 512 and at least 4096 Winograd tiles.
LAYERS = [(224, 296, 768, True), (224, 296, 512, True), (224, 296, 256, False), (196, 259, 256, False), (112, 148, 768, True), (112, 148, 512, True),
          (112, 148, 256, False), (98, 129, 256, False), (56, 74, 512, False)]


@pytest.mark.parametrize("H,W,K,f16", LAYERS)
def test_256_column_layers_of_the_pass(route, monkeypatch, H, W, K, f16):
    assert route.L is not None
    from patchfusion_amd import _lib
    T = 8 * -(-H // 4) * -(-W // 4)
    p = _lib.ConvParams()
    p.B, p.OH, p.OW, p.H, p.W, p.Cin, p.Cout, p.batch = 1, 1, T, 1, T, K, 256, 36
    assert route.L.pf_gemm_split3_route(C.byref(p), 256) == P128
    assert route.L.pf_gemm_f16x2_points_route(C.byref(p), 256) == (P128 if f16 else NONE)
    monkeypatch.setenv("PF_WINO_F16X2_N256", "3")
    assert route.L.pf_gemm_f16x2_points_route(C.byref(p), 256) == P128
    monkeypatch.setenv("PF_WINO_F16X2_N256", "2")                 # the rule, with the range pass kept (hip_ops)
    assert route.L.pf_gemm_f16x2_points_route(C.byref(p), 256) == (P128 if f16 else NONE)
    monkeypatch.setenv("PF_WINO_F16X2_N256", "0")
    assert route.L.pf_gemm_f16x2_points_route(C.byref(p), 256) == NONE


def test_layers_below_two_rounds_of_tiles_stay_on_bf16x3(route, monkeypatch):
    """1024->256 @ 8x28x37: 560 tiles = 10 tiles of 128 x 128 per point, 360 in the launch, under two rounds of a 256-CU chip -- split3_route gives the
    one-tile kernel, which has no fp16x2 form (a persistent fp16x2 walk measured 0.36-0.93x at so few tiles, round 8)"""
    monkeypatch.setenv("PF_WINO_F16X2_N256", "3")
    assert route(8, 28, 37, 1024, 256) == NONE


def test_pinned_shapes_keep_their_routes(route, monkeypatch):
    monkeypatch.setenv("PF_WINO_F16X2_N256", "3")
    assert route(2, 36, 44, 256, 256) == NONE and route(1, 36, 44, 256, 256) == NONE       # 144 / 72 tiles over the 36 points: TILE64, bf16x3
    monkeypatch.setenv("PF_S3_PERSIST", "2")
    assert route(2, 36, 44, 256, 256) == NONE and route(1, 36, 44, 256, 256) == NONE
    monkeypatch.delenv("PF_WINO_F16X2_N256")
    assert route(2, 36, 44, 256, 256) == NONE
    assert route(8, 392, 518, 544, 544) == P192 and route(8, 224, 296, 768, 768) == P192     # the round-7 layers
    monkeypatch.setenv("PF_S3_T192", "2")
    monkeypatch.setenv("PF_S3_TILE_NOW", "192")
    assert route(1, 40, 52, 1024, 256) == P192 and route(1, 64, 80, 544, 544) == P192      # the forced 192-tile cases of the GPU tests
    assert route.L.pf_gemm_f16x2_points_route(None, 256) == -1
