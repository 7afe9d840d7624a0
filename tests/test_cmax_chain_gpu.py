"""pytest -m gpu: an fp16x2 Winograd layer that takes its channel maxima from the kernels that wrote its input (hip_ops.cmax_begin, conv(cmax_in=),
conv_chain(cmax_in=, cmax_out=)) against the same layer running its own range pass.

Where both arms run the fp16x2 product the outputs are compared with torch.equal: the handed vector is bit-identical to the range pass, so nothing
downstream may move.  PF_WINO_F16X2_N256=2 is the arm in which every fp16x2 layer runs its own range pass.  At default switches a layer's product does
not depend on whether its maxima are given; under PF_WINO_F16X2_N256=5 (the wider rule of pf_gemm_f16x2_points_route_ex, measured but not adopted) a
K = 256 layer is fp16x2 ONLY when its maxima are given and runs three bf16 planes otherwise, so there the hand-over arm is held to float64 samples with
the caps of tests/f64_ref.py, like every split Winograd route."""
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
# the persistent 128-tile walk on a layer too small to earn it, and fp16x2 on every such layer: the hand-over at test size
FORCE = dict(PF_S3_TILE_NOW="128", PF_S3_PERSIST="2", PF_WINO_F16X2_N256="3")


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


def _route(x, pw, y, act, given):
    from patchfusion_amd.hip_ops import HipOps
    return HipOps._conv_plan(x, pw, y, 1, 1, act, False, None, None, None, given)[0]


def _resize_concat_conv(srcs, pw, handover):
    """u = resize_concat(srcs); y = relu(conv(u)) -- with the maxima from the resize kernel when `handover` (and the layer takes them)"""
    from patchfusion_amd.hip_ops import ops
    B, OH, OW = 2, 24, 40
    u = torch.full((B, OH, OW, pw.cin), float("nan"), device=DEV)
    y = torch.full((B, OH, OW, pw.cout), float("nan"), device=DEV)
    cm = ops.cmax_begin(u, pw, y, "u", pad=1, act="relu") if handover else None
    op_checks._flush_caches()
    if cm is None:
        ops.resize_concat(srcs, u)
        ops.conv(u, pw, y, pad=1, act="relu")
    else:
        ops.resize_concat(srcs, u, cmax=cm)
        ops.conv(u, pw, y, pad=1, act="relu", cmax_in=cm)
    torch.cuda.synchronize()
    assert not torch.isnan(y).any()
    return u, y, cm is not None


@pytest.mark.parametrize("chans", [(32, 32, 32), (32, 64, 64)], ids=["96_256", "160_256"])
def test_conv_fed_by_resize_concat_takes_the_resize_kernels_maxima(env, chans):
    """C -> 256 3x3 at 2 x 24 x 40, its input written by ONE resize_concat launch of three sources.  C = 96: below the 128 channels the three-step
    Winograd layers start at (packing.winograd_eligible), so no arm runs fp16x2, cmax_begin declines and all arms are one computation.  C = 160: the
    forced arms run fp16x2 and the conv takes the resize kernel's maxima."""
    g = torch.Generator().manual_seed(7)
    # channel magnitudes over six decades, as the decoder's concat buffers have (tests/dynamic_range.py)
    srcs = [(torch.randn(2, h, w, c, generator=g) * s).to(DEV) for (h, w, s), c in zip(((24, 40, 1e-3), (12, 20, 1.0), (13, 19, 1e3)), chans)]
    cin = sum(chans)
    w, b, _ = _operands("random", 256, cin, 3, 41)
    outs = {}
    for name, sw, handover in (("handover", FORCE, True), ("range_pass", FORCE, False), ("n256_2", dict(FORCE, PF_WINO_F16X2_N256="2"), True)):
        env(**sw)
        pw = pk.pack_conv(w, b, dtype=torch.float32).to(DEV)
        u, y, took = _resize_concat_conv(srcs, pw, handover)
        route = _route(u, pw, y, "relu", took)
        outs[name] = (u, y, took, route)
    print(f"resize_concat -> {cin}->256 routes:", {k: (v[3], "maxima handed" if v[2] else "own range pass / none") for k, v in outs.items()})
    assert not outs["range_pass"][2] and not outs["n256_2"][2], "PF_WINO_F16X2_N256=2 and a plain call: every layer runs its own range pass"
    assert torch.equal(outs["handover"][0], outs["range_pass"][0]) and torch.equal(outs["handover"][0], outs["n256_2"][0])
    if cin < 128:
        assert not outs["handover"][2] and "wino3h" not in [v[3] for v in outs.values()]
        assert torch.equal(outs["handover"][1], outs["range_pass"][1]) and torch.equal(outs["handover"][1], outs["n256_2"][1])
        return
    assert outs["handover"][2] and outs["handover"][3] == "wino3h", "the hand-over arm must run fp16x2 on the handed maxima"
    assert outs["range_pass"][3] == "wino3h"
    assert torch.equal(outs["handover"][1], outs["range_pass"][1]), "the handed maxima moved the output"
    if outs["n256_2"][3] == "wino3h":
        assert torch.equal(outs["handover"][1], outs["n256_2"][1])
    else:                                                    # (three bf16 planes there: another product of the same float32 grade)
        pix = R.sample_pixels(2, 24, 40, n_random=64, seed=3)
        ref, mag = R.conv_ref(outs["handover"][0], w, pix, b, 1, 1, "relu")
        for k in ("handover", "n256_2"):
            e = R.errors(R.gather_pixels(outs[k][1], pix, 256), ref, mag)
            print(f"resize_concat -> {cin}->256 {k:10s} elem {e[0]:.2e} norm {e[1]:.2e}")
            assert e[1] <= R.NORM_CAP_WINO and e[0] <= R.ELEM_CAP_WINO, (k, e)


def _chain(x, pws, handover):
    from patchfusion_amd.hip_ops import ops
    B, H, W, _ = x.shape
    t = torch.full((B, H, W, 256), float("nan"), device=DEV)
    y = torch.full((B, H, W, 256), float("nan"), device=DEV)
    op_checks._flush_caches()
    if handover:
        ops.conv_chain(x, pws[0], t, pws[1], y, dict(pad=1, act="relu"), dict(pad=1, act="relu"))
    else:
        ops.conv(x, pws[0], t, pad=1, act="relu")
        ops.conv(t, pws[1], y, pad=1, act="relu")
    torch.cuda.synchronize()
    assert not torch.isnan(y).any()
    return t, y


def test_256_256_256_chain_hands_the_maxima_to_a_layer_that_is_fp16x2_only_with_them(env):
    """2 x 116 x 148 = 2146 Winograd tiles: under PF_WINO_F16X2_N256=5 conv 2 (K = 256) runs fp16x2 exactly when conv 1's output transform hands over
    the maxima; at default switches the chain computes the bits of PF_WINO_F16X2_N256=2"""
    B, H, W = 2, 116, 148
    w1, b1, s = _operands("wide", 256, 256, 3, 51)
    w2, b2, _ = _operands("random", 256, 256, 3, 52)
    x = _input((B, H, W, 256), s, "wide", 53).to(DEV)
    pix = R.sample_pixels(B, H, W, n_random=128, seed=5)

    def packed():
        return [pk.pack_conv(w, b, dtype=torch.float32).to(DEV) for w, b in ((w1, b1), (w2, b2))]

    # every 128-tile layer on fp16x2: the chain against two plain calls, bit for bit
    env(PF_WINO_F16X2_N256="3")
    pws = packed()
    ta, ya = _chain(x, pws, True)
    tb, yb = _chain(x, pws, False)
    assert _route(tb, pws[1], yb, "relu", False) == "wino3h"
    assert torch.equal(ta, tb) and torch.equal(ya, yb), "the handed maxima moved the output"

    # default rule: given maxima do not change a layer's product -- the chain computes what PF_WINO_F16X2_N256=2 computes
    env()
    pws = packed()
    assert _route(ta, pws[1], ya, "relu", True) == "wino3" and _route(ta, pws[1], ya, "relu", False) == "wino3"
    td, yd = _chain(x, pws, True)

    # the wider rule: conv 2 takes fp16x2 because its maxima are given; called alone it stays on three bf16 planes, as under PF_WINO_F16X2_N256=2
    env(PF_WINO_F16X2_N256="5")
    pws = packed()
    assert _route(x, pws[0], ta, "relu", False) == "wino3"
    assert _route(ta, pws[1], ya, "relu", True) == "wino3h" and _route(ta, pws[1], ya, "relu", False) == "wino3"
    t1, y1 = _chain(x, pws, True)
    assert torch.equal(y1, _chain(x, pws, True)[1]), "two launches differ"
    env(PF_WINO_F16X2_N256="2")
    pws = packed()
    assert _route(t1, pws[1], y1, "relu", True) == "wino3"
    t2, y2 = _chain(x, pws, True)
    assert torch.equal(t1, t2), "conv 1 runs the same product in both arms"
    assert torch.equal(td, t2) and torch.equal(yd, y2), "default switches: the bits of the range-pass arm"
    ref, mag = R.conv_ref(t1, w2, pix, b2, 1, 1, "relu")
    e1 = R.errors(R.gather_pixels(y1, pix, 256), ref, mag)
    e2 = R.errors(R.gather_pixels(y2, pix, 256), ref, mag)
    env(PF_WINO_SPLIT3="0", PF_WINO_FUSED="0")
    pws = packed()
    assert _route(t1, pws[1], y1, "relu", False) == "wino"
    from patchfusion_amd.hip_ops import ops
    y3 = torch.full_like(y1, float("nan"))
    ops.conv(t1, pws[1], y3, pad=1, act="relu")
    torch.cuda.synchronize()
    base = R.errors(R.gather_pixels(y3, pix, 256), ref, mag)
    print(f"256->256->256 conv 2: PF_WINO_F16X2_N256=5 hand-over fp16x2 elem {e1[0]:.2e} norm {e1[1]:.2e} | PF_WINO_F16X2_N256=2 bf16x3 elem {e2[0]:.2e} norm {e2[1]:.2e} | "
          f"f32 elem {base[0]:.2e} norm {base[1]:.2e}")
    assert base[1] <= R.NORM_CAP_WINO and base[0] <= R.ELEM_CAP_WINO, ("f32 three-step route", base)
    assert R.float32_grade(e1, base, R.NORM_CAP_WINO, R.ELEM_CAP_WINO), (e1, base)
    assert R.float32_grade(e2, base, R.NORM_CAP_WINO, R.ELEM_CAP_WINO), (e2, base)
