"""CPU-side checks of the head-backward entry points (csrc/head_bwd.hip): the symbols exist and every call refuses null or misaligned
pointers and mismatched sizes with PF_ERR_ARG before any launch (fake non-null pointers: no call below reaches a kernel)."""
import ctypes as C
import os

import pytest

ERR_ARG, OK = 1, 0
RELU, GELU, SOFTPLUS = 1, 2, 3


@pytest.fixture
def L():
    from patchfusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpf_hip.so not built")
    return _lib.load()


a, b, c, d, e = (C.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000))
odd = C.c_void_p(0x1002)                                   # not aligned to a float


def test_symbols_are_bound(L):
    for n in ("pf_conv1x1_wgrad_workspace_bytes", "pf_conv1x1_wgrad", "pf_resize_bilinear_bwd", "pf_attractor_bwd", "pf_logbinom_depth_bwd",
              "pf_act_bwd", "pf_silog_loss_bwd"):
        assert hasattr(L, n)


def test_wgrad_workspace_size_and_refusals(L):
    n = C.c_long(-1)
    assert L.pf_conv1x1_wgrad_workspace_bytes(850, 80, 160, 288, C.byref(n)) == OK and n.value == 3 * (80 * 160 + 80) * 4
    assert L.pf_conv1x1_wgrad_workspace_bytes(850, 80, 160, 0, C.byref(n)) == OK and n.value == 2 * (80 * 160 + 80) * 4     # default: 512 pixels
    assert L.pf_conv1x1_wgrad_workspace_bytes(8 * 392 * 518, 80, 160, 0, C.byref(n)) == OK and 400 * 12880 * 4 < n.value <= 512 * 12880 * 4
    for bad in ((0, 80, 160, 0), (850, 0, 160, 0), (850, 80, 0, 0), (850, 80, 160, -1), (850, 5000, 160, 0), (1 << 20, 8, 8, 1)):
        assert L.pf_conv1x1_wgrad_workspace_bytes(*bad, C.byref(n)) == ERR_ARG
    assert L.pf_conv1x1_wgrad_workspace_bytes(850, 80, 160, 0, None) == ERR_ARG
    big = 1 << 30
    good = (a, 80, b, 160, 850, 80, 160, c, d, e, big, 0, None)
    for i in (0, 2, 7, 9):                                 # dy, x, dw, workspace: null and misaligned
        for p in (None, odd):
            args = list(good)
            args[i] = p
            assert L.pf_conv1x1_wgrad(*args) == ERR_ARG
    assert L.pf_conv1x1_wgrad(a, 80, b, 160, 850, 80, 160, c, odd, e, big, 0, None) == ERR_ARG       # a misaligned bias gradient
    assert L.pf_conv1x1_wgrad(a, 79, b, 160, 850, 80, 160, c, d, e, big, 0, None) == ERR_ARG         # pixel stride below the channels
    assert L.pf_conv1x1_wgrad(a, 80, b, 159, 850, 80, 160, c, d, e, big, 0, None) == ERR_ARG
    assert L.pf_conv1x1_wgrad(a, 80, b, 160, 850, 80, 160, c, d, e, 2 * 12880 * 4 - 1, 0, None) == ERR_ARG   # a workspace one byte short
    assert L.pf_conv1x1_wgrad(a, 80, b, 160, 0, 80, 160, c, d, e, big, 0, None) == ERR_ARG


def test_resize_attractor_logbinom_refusals(L):
    assert L.pf_resize_bilinear_bwd(None, 8, 1, 4, 4, 8, b, 8, 2, 2, 0, None) == ERR_ARG
    assert L.pf_resize_bilinear_bwd(a, 8, 1, 4, 4, 8, odd, 8, 2, 2, 0, None) == ERR_ARG
    assert L.pf_resize_bilinear_bwd(a, 7, 1, 4, 4, 8, b, 8, 2, 2, 0, None) == ERR_ARG
    assert L.pf_resize_bilinear_bwd(a, 8, 1, 4, 4, 8, b, 8, 0, 2, 0, None) == ERR_ARG
    good = [a, 16, 16, 0, 0, b, 3, 5, c, d, 16, e, 2, 5, 7, 64, None]
    for i in (0, 5, 8, 9, 11):
        for p in (None, odd):
            args = list(good)
            args[i] = p
            assert L.pf_attractor_bwd(*args) == ERR_ARG
    for i, v in ((1, 15), (2, 0), (10, 15), (15, 260), (15, 0), (6, 0)):
        args = list(good)
        args[i] = v
        assert L.pf_attractor_bwd(*args) == ERR_ARG
    good = [a, 4, b, 5, 7, c, d, 4, e, 2, 9, 13, 64, 0.02, 50.0, None, None]         # (..., logc or null, stream)
    assert L.pf_logbinom_depth_bwd(*(good[:15] + [odd, None])) == ERR_ARG              # a misaligned table of constants
    for i in (0, 2, 5, 6, 8):
        for p in (None, odd):
            args = list(good)
            args[i] = p
            assert L.pf_logbinom_depth_bwd(*args) == ERR_ARG
    for i, v in ((1, 3), (7, 3), (12, 1), (12, 257), (3, 0)):
        args = list(good)
        args[i] = v
        assert L.pf_logbinom_depth_bwd(*args) == ERR_ARG


def test_act_and_silog_refusals(L):
    assert L.pf_act_bwd(None, 8, b, 8, 4, 8, RELU, None) == ERR_ARG and L.pf_act_bwd(a, 8, odd, 8, 4, 8, RELU, None) == ERR_ARG
    assert L.pf_act_bwd(a, 7, b, 8, 4, 8, GELU, None) == ERR_ARG and L.pf_act_bwd(a, 8, b, 7, 4, 8, SOFTPLUS, None) == ERR_ARG
    assert L.pf_act_bwd(a, 8, b, 8, 4, 8, 0, None) == ERR_ARG and L.pf_act_bwd(a, 8, b, 8, 0, 8, RELU, None) == ERR_ARG
    half = C.c_void_p(0x3004)                              # aligned to a float, not to a double
    assert L.pf_silog_loss_bwd(a, b, 16, 1e-3, 80.0, 0.15, half, 1.0, d, None) == ERR_ARG
    assert L.pf_silog_loss_bwd(a, b, 0, 1e-3, 80.0, 0.15, c, 1.0, d, None) == ERR_ARG
    for i in (0, 1, 6, 8):
        args = [a, b, 16, 1e-3, 80.0, 0.15, c, 1.0, d, None]
        args[i] = None
        assert L.pf_silog_loss_bwd(*args) == ERR_ARG
