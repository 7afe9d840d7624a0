"""pytest -m gpu: the fp16x2 three-step Winograd layer (csrc/wino_f16x2.hip, pf_conv_winograd_f16x2_windowed) against a float64 convolution of the
same float32 operands, next to the bf16x3 route (PF_WINO_F16X2=0) and the f32-MFMA route (PF_WINO_SPLIT3=0) on the same data.

Cases: 544->544, 768->768 and 1024->256 (the 192 x 192 product), 256->256 (no fp16x2 form: stays on the bf16x3 route); random inputs and inputs
whose channels span 1e-3 ... 1e3 with weights that compensate (what tests/dynamic_range.py does to the RCU / double-conv pairs); one window and
several (PF_WS_CAP_GB small).  Small layers reach the 192 x 192 kernel through PF_S3_PERSIST=2 PF_S3_T192=2 PF_S3_TILE_NOW=192 (the dispatch
knobs of csrc/gemm_split3.hip).  Every checked launch starts from cold caches (op_checks._flush_caches)."""
import os

import pytest
import torch

from patchfusion_amd import packing as pk
from tests import op_checks

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("PF_WINOGRAD", "PF_WINOGRAD_MIN_PIXELS", "PF_WINO_FUSED", "PF_WS_CAP_GB", "PF_WINO_F16X2", "PF_WINO_SPLIT3", "PF_S3_PERSIST", "PF_S3_T192", "PF_S3_TILE_NOW")
BASE = dict(PF_WINOGRAD="4", PF_WINOGRAD_MIN_PIXELS="0", PF_WINO_FUSED="0", PF_S3_PERSIST="2")
T192 = dict(PF_S3_T192="2", PF_S3_TILE_NOW="192")


@pytest.fixture
def env():
    old = {k: os.environ.get(k) for k in KEYS}

    def set_env(**kw):
        for k in KEYS:
            os.environ.pop(k, None)
        os.environ.update(BASE)
        os.environ.update(kw)
        op_checks._switches_changed()
    yield set_env
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    op_checks._switches_changed()


def _layer(cin, cout, seed, wide):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) / (9 * cin) ** 0.5
    s = torch.ones(cin, dtype=torch.float64)
    if wide:                                            # input channel c carries s_c in [1e-3, 1e3], its weights 1 / s_c
        s = 10.0 ** (torch.rand(cin, generator=g, dtype=torch.float64) * 6 - 3)
        w = w / s[None, :, None, None]
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    return w.float(), b.float(), s


def _input(B, H, W, cin, s, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, H, W, cin, generator=g, dtype=torch.float64) * s).float()


def _ref(x, w, b, relu):
    y = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    return y.clamp_min(0) if relu else y


def _run(x, pw, relu):
    from patchfusion_amd.hip_ops import HipOps, ops
    y = torch.full((*x.shape[:3], pw.cout), -7.0, dtype=torch.float32, device=DEV)
    route = HipOps._conv_plan(x, pw, y, 1, 1, "relu" if relu else None, False, None, None, None)[0]
    op_checks._flush_caches()
    ops.conv(x, pw, y, pad=1, act="relu" if relu else None)
    torch.cuda.synchronize()
    return y, route


def _err(y, ref):
    return float((y.double().cpu() - ref).abs().max() / ref.abs().max())


CASES = [  # B, H, W, cin, cout, relu, fp16x2 form expected (the 256->256 case keeps the round-5 tile rule: 128 x 128, no fp16x2 form)
    (1, 64, 80, 544, 544, True, True),
    (1, 32, 40, 768, 768, False, True),
    (1, 40, 52, 1024, 256, True, True),
    (2, 36, 44, 256, 256, True, False),
]


@pytest.mark.parametrize("wide", [False, True], ids=["random", "wide"])
@pytest.mark.parametrize("B,H,W,cin,cout,relu,f16", CASES)
def test_f16x2_layer_error_against_float64_and_the_other_routes(env, B, H, W, cin, cout, relu, f16, wide):
    w, b, s = _layer(cin, cout, 100 + cin + cout, wide)
    xc = _input(B, H, W, cin, s, 200 + cin)
    ref = _ref(xc, w, b, relu)
    t192 = T192 if f16 else {}
    env(**t192)
    pw = pk.pack_conv(w, b, dtype=torch.float32).to(DEV)
    assert pw.wino_u3 is not None
    x = xc.to(DEV)
    errs, outs = {}, {}
    for name, kw in (("f16x2", {}), ("f16x2_win", dict(PF_WS_CAP_GB="0.005")), ("bf16x3", dict(PF_WINO_F16X2="0")), ("f32", dict(PF_WINO_SPLIT3="0"))):
        env(**t192, **kw)
        y, route = _run(x, pw, relu)
        assert route == {"f16x2": "wino3h" if f16 else "wino3", "f16x2_win": "wino3h" if f16 else "wino3", "bf16x3": "wino3", "f32": "wino"}[name], (name, route)
        assert torch.isfinite(y).all(), name
        errs[name], outs[name] = _err(y, ref), y
    if f16 and B * -(-H // 4) * -(-W // 4) > 192:
        from patchfusion_amd import hip_ops
        env(PF_WS_CAP_GB="0.005")
        assert hip_ops.wino3_window(B, H, W, pw)[1] >= 2           # several windows really ran
    assert torch.equal(outs["f16x2"], outs["f16x2_win"]), "windows changed the numbers"
    print(f"{cin}->{cout} {'wide' if wide else 'random'}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["f16x2"] <= 2 * errs["bf16x3"] and errs["f16x2"] <= 2 * errs["f32"], errs


def test_f16x2_two_launches_are_bit_identical(env):
    w, b, s = _layer(544, 544, 7, True)
    x = _input(1, 40, 52, 544, s, 8).to(DEV)
    env(**T192)
    pw = pk.pack_conv(w, b, dtype=torch.float32).to(DEV)
    y0, route = _run(x, pw, True)
    y1, _ = _run(x, pw, True)
    assert route == "wino3h"
    assert torch.equal(y0, y1)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_f16x2_non_finite_input_gives_non_finite_output(env, bad):
    w, b, s = _layer(544, 544, 9, False)
    x = _input(1, 40, 52, 544, s, 10)
    x[0, 17, 23, 100] = bad
    env(**T192)
    pw = pk.pack_conv(w, b, dtype=torch.float32).to(DEV)
    y, route = _run(x.to(DEV), pw, False)
    assert route == "wino3h"
    assert not torch.isfinite(y[0, 16:19, 22:25]).all(), "a non-finite input pixel must not come out finite"
