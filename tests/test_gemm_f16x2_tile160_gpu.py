"""pytest -m gpu: the 160 x 256 tile form of the fp16x2 linear (csrc/gemm_f16x2_t160.hip) against the 192 x 192 form (csrc/gemm_split3.hip) on the
same operands, BIT FOR BIT: both sum the same three products per accumulator over the K chunks in the same order and run the same epilogue, so
PF_F16_TILE=1 must reproduce PF_F16_TILE=0 exactly.  The 192-tile route itself is graded against float64 in tests/test_float32_grade_gpu.py and
tests/test_vit_f16x2_gpu.py.

Shapes: M in {1, 159, 160, 161, 333, 1037} (one row, either side of a tile edge, several tiles, the pass's 1037), N in {256, 260, 512, 1024}
(260: a ragged last column tile with Cout % 32 != 0), K in {32, 64, 96, 128, 1024} (one, two and three chunks = the ring's lead-in and drain, four,
and a full stream), every combination under each epilogue form.  Outputs are pre-filled with NaN, have 16 guard rows either side and four guard
columns, every launch starts from cold caches (op_checks._flush_caches), and every result must repeat bit for bit."""
import ctypes as C
import itertools

import pytest
import torch

from patchfusion_amd import _lib
from patchfusion_amd import packing as pk
from patchfusion_amd.hip_ops import HipOps, ops
from tests import op_checks

pytestmark = pytest.mark.gpu
DEV = "cuda"
P192, T160 = 3, 4
MS, NS, KS = (1, 159, 160, 161, 333, 1037), (256, 260, 512, 1024), (32, 64, 96, 128, 1024)
GUARD = 16
FORMS = {
    "plain": dict(bias=False, ls=False, res=False, res2=False, act=None),
    "bias_ls_res": dict(bias=True, ls=True, res=True, res2=False, act=None),
    "res2": dict(bias=True, ls=True, res=True, res2=True, act=None),
    "relu": dict(bias=True, ls=False, res=False, res2=False, act="relu"),
    "gelu": dict(bias=True, ls=False, res=False, res2=False, act="gelu"),
}
_X, _W = {}, {}


def _x_planes(M, K):
    """float32 [M, K] with |x| <= 4 and its two chunk-major fp16 planes (exponents of a bound of 4 per channel); built once per shape"""
    if (M, K) not in _X:
        g = torch.Generator().manual_seed(1000 * M + K)
        x = torch.randn(M, K, generator=g).clamp_(-4, 4).float()
        e = pk.bound_exponents(torch.full((K,), 4.0, dtype=torch.float64))
        x2 = pk.rows_to_kmajor(torch.stack(pk.split_f16x2(torch.ldexp(x.double(), -e.double()[None, :]).float()))).to(DEV)
        _X[(M, K)] = (x, x2)
    return _X[(M, K)]


def _weights(N, K, bias, ls):
    key = (N, K, bias, ls)
    if key not in _W:
        g = torch.Generator().manual_seed(7 * N + K)
        w = (torch.randn(N, K, generator=g) / K ** 0.5).float()
        b = torch.randn(N, generator=g).float() if bias else None
        s = (0.5 + torch.rand(N, generator=g)).float() if ls else None
        _W[key] = (w, b, s, pk.pack_conv_f16x2(w, b, s, torch.full((K,), 4.0, dtype=torch.float64)).to(DEV))
    return _W[key]


def _route(x2, pw, y, act, res, res2, out_exp=None):
    p = HipOps._conv_f16x2_plan(x2, pw, y, act, res, res2, out_exp)
    return _lib.load().pf_gemm_f16x2_route(C.byref(p), 256)


def _run(monkeypatch, tile, x2, pw, M, N, act, res, res2):
    """one cold launch into a NaN-filled buffer with guard rows and columns -> the whole buffer"""
    monkeypatch.setenv("PF_F16_TILE", tile)
    buf = torch.full((M + 2 * GUARD, N + 4), float("nan"), device=DEV)
    y = buf[GUARD:GUARD + M, :N]
    assert _route(x2, pw, y, act, res, res2) == (T160 if tile == "1" else P192)
    op_checks._flush_caches()
    ops.conv_f16x2(x2, pw, y, act=act, res=res, res2=res2)
    return buf


def _check_case(monkeypatch, M, N, K, form):
    f = FORMS[form]
    x, x2 = _x_planes(M, K)
    w, b, s, pw = _weights(N, K, f["bias"], f["ls"])
    g = torch.Generator().manual_seed(M + N + K)
    res = torch.randn(M, N, generator=g).to(DEV) if f["res"] else None
    res2 = torch.randn(M, N, generator=g).to(DEV) if f["res2"] else None
    ref = _run(monkeypatch, "0", x2, pw, M, N, f["act"], res, res2)
    a = _run(monkeypatch, "1", x2, pw, M, N, f["act"], res, res2)
    a2 = _run(monkeypatch, "1", x2, pw, M, N, f["act"], res, res2)
    tag = (M, N, K, form)
    assert not torch.isnan(ref[GUARD:GUARD + M, :N]).any(), tag
    assert torch.isnan(ref[:GUARD]).all() and torch.isnan(ref[GUARD + M:]).all() and torch.isnan(ref[:, N:]).all(), tag
    assert torch.equal(a.view(torch.int32), ref.view(torch.int32)), tag        # valid region bit for bit; guards still the NaN fill
    assert torch.equal(a2.view(torch.int32), a.view(torch.int32)), tag
    return x, w, b, s, res, res2, a


@pytest.mark.parametrize("form", list(FORMS))
def test_tile160_matches_tile192_bit_for_bit(monkeypatch, form):
    monkeypatch.delenv("PF_S3_GRID", raising=False)
    for M, N, K in itertools.product(MS, NS, KS):
        _check_case(monkeypatch, M, N, K, form)


def test_one_block_walks_several_tiles(monkeypatch):
    """M = 1037, N = 1024, K = 128 with PF_S3_GRID=8: 7 x 4 = 28 tiles on 8 blocks, three or four tiles per block -- the tile switch, the epilogue
    beside the partner group's MFMAs and the ring wrapping across tiles.  The float64 check only guards against both forms being wrong together."""
    monkeypatch.setenv("PF_S3_GRID", "8")
    M, N, K = 1037, 1024, 128
    for form in ("bias_ls_res", "res2", "gelu"):
        x, w, b, s, res, res2, a = _check_case(monkeypatch, M, N, K, form)
    z = x.double() @ w.double().t() + b.double()
    ref = torch.nn.functional.gelu(z)
    y = a[GUARD:GUARD + M, :N].cpu().double()
    assert float((y - ref).abs().max() / ref.abs().max()) < 4e-6


def test_plane_outputs_stay_on_the_192_tile(monkeypatch):
    """the plane outputs (korder bits 16 / 32, three bf16 planes) exist on the 192-tile form only: the route must say so even when the new tile is forced"""
    M, N, K = 333, 512, 64
    _, x2 = _x_planes(M, K)
    pw = _weights(N, K, True, False)[3]
    oe = torch.zeros(N, dtype=torch.int32, device=DEV)
    outs = [(torch.empty(2, N // 32, M, 32, dtype=torch.float16, device=DEV), oe), (torch.empty(2, M, N, dtype=torch.float16, device=DEV), oe),
            (torch.empty(3, M, N, dtype=torch.bfloat16, device=DEV), None)]
    for tile in ("1", "0", None):
        if tile is None:
            monkeypatch.delenv("PF_F16_TILE", raising=False)
        else:
            monkeypatch.setenv("PF_F16_TILE", tile)
        for y, e in outs:
            assert _route(x2, pw, y, None, None, None, e) == P192
    monkeypatch.setenv("PF_F16_TILE", "1")
    y, e = outs[1]
    y.fill_(float("nan"))
    ops.conv_f16x2(x2, pw, y, out_exp=e)
    assert not torch.isnan(y).any()
