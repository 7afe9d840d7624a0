"""pytest -m gpu: the channel-maxima hand-over as FusionNet.forward and the branches wire it (engine.py: cmax_begin slots "cat", "u", "v", absmax on
u5[..., :32], conv_chain, the slice arithmetic of cm_kw), through the model.

tests/test_cmax_producers_gpu.py and tests/test_cmax_chain_gpu.py hold the hand-over per op and per two-layer chain.  At the sizes of
tests/test_e2e_gpu.py no layer qualifies for the fp16x2 Winograd form, so through the engine ``cmax_begin`` returns None everywhere, and at the
headline size a too-large or stale maximum only costs precision inside the tolerance.  Here the form is forced at the tiny geometry (vits, 112 x
154, two crops: the concat buffers have 128, 192 and 160 channels, so all three slots, the level-5 absmax and the up convs' chain qualify) and the
arm that takes the maxima from the producers is compared with an arm in which every fp16x2 layer runs its own range pass.  include/pf_hip.h
promises the handed vector equals the range pass bit for bit, so the depth and every tap must be ``torch.equal``.

The arms.  PF_WINO_F16X2_N256=2 is the switch for "every fp16x2 layer runs its own range pass", but it is also a ROUTING value: under the forced
128-tile walk (tests/test_cmax_chain_gpu.py FORCE) value 3 puts every 128-tile layer on fp16x2 and value 2 only those with K >= 512 and 4096 tiles
(csrc/gemm_split3.hip f16x2_points_route), i.e. none at this size -- those layers then run three bf16 planes, another product of the same grade, and
no bit-for-bit comparison is possible.  So:
  * under FORCE the range-pass arm keeps the switches and turns the hand-over off where hip_ops decides it (``_cmax_handover_enabled``): same routes,
    asserted; the literal PF_WINO_F16X2_N256=2 arm is run too, must hand over nothing, and is held to twice the float32 end-to-end tolerance;
  * with the 192-tile walk forced as well (PF_S3_T192=2, PF_S3_TILE_NOW=192: tests/test_float32_grade_gpu.py T192) every layer is fp16x2 at either
    value, so there the arms are exactly the issue's: those switches against PF_WINO_F16X2_N256=2, same routes asserted, ``torch.equal``.
Each arm is also run under the "max" poison (tests/poison_alloc.py) with the two integer sites of the hand-over on the allow-list -- the cmax
vectors and the fp16x2 scratch start as 0x7F7F7F7F, larger than the bits of any finite float maximum -- and must reproduce its unpoisoned run bit for bit: a
vector that is not fully zeroed or fully merged shows here."""
import collections

import pytest
import torch

from tests import poison_alloc as pa
from tests.test_cmax_chain_gpu import FORCE
from tests.test_e2e_gpu import F32_TOL
from tests.test_float32_grade_gpu import T192, WINO
from tests.test_uninit_independence_gpu import _case, _model_run, switches  # noqa: F401  (switches: fixture)

pytestmark = pytest.mark.gpu


class Spies:
    def __init__(self, monkeypatch):
        from patchfusion_amd import hip_ops
        from patchfusion_amd.hip_ops import HipOps
        self.reset()
        real_begin, real_conv, real_chain, real_absmax, real_exec, real_buf = (HipOps.cmax_begin, HipOps.conv, HipOps.conv_chain, HipOps.absmax,
                                                                               HipOps._conv_exec, hip_ops._cmax_buffer)

        def begin(x, pw, y, slot, **k):
            cm = real_begin(x, pw, y, slot, **k)
            if cm is not None:
                self.begun[slot] += 1
                self.live[cm.data_ptr()] = slot
            return cm

        def consumed(cm):
            if cm is not None:
                self.consumed[self.live.get(cm.data_ptr(), "?")] += 1

        def conv(x, pw, y, *a, **k):
            consumed(k.get("cmax_in"))
            return real_conv(x, pw, y, *a, **k)

        def chain(x, pw1, t, pw2, y, kw1, kw2, cmax_in=None, cmax_out=None):
            consumed(cmax_in)
            if cmax_out is not None:
                self.chain_out += 1
            return real_chain(x, pw1, t, pw2, y, kw1, kw2, cmax_in=cmax_in, cmax_out=cmax_out)

        def absmax(x, cmax):
            self.absmax.append((x.shape[-1], x.stride(-2)))
            return real_absmax(x, cmax)

        def cmax_buffer(device, n, slot="t"):
            if slot == "t":                                         # conv_chain alone asks for this slot: conv 1 hands its maxima to conv 2
                self.chain_handed += 1
            return real_buf(device, n, slot)

        def conv_exec(route, p, extra, device, **k):
            self.routes.append(route)
            if k.get("cmax_in") is not None:
                self.given += 1
            return real_exec(route, p, extra, device, **k)

        for name, fn in (("cmax_begin", begin), ("conv", conv), ("conv_chain", chain), ("absmax", absmax), ("_conv_exec", conv_exec)):
            monkeypatch.setattr(HipOps, name, staticmethod(fn))
        monkeypatch.setattr(hip_ops, "_cmax_buffer", cmax_buffer)

    def reset(self):
        self.begun, self.consumed, self.live = collections.Counter(), collections.Counter(), {}
        self.absmax, self.routes, self.chain_handed, self.chain_out, self.given = [], [], 0, 0, 0

    def assert_handed(self, label):
        for slot in ("cat", "u", "v"):
            assert self.begun[slot] and self.consumed[slot] == self.begun[slot], (label, slot, dict(self.begun), dict(self.consumed))
        assert self.chain_handed, f"{label}: no conv_chain handed conv 1's maxima to conv 2"
        assert self.chain_out, f"{label}: no conv_chain wrote its output's maxima into the next consumer's vector"
        assert (32, 160) in self.absmax, f"{label}: the absmax branch of level 5 (u5[..., :32]) did not run: {self.absmax}"
        assert self.given and "wino3h" in self.routes

    def assert_none(self, label):
        assert not self.begun and not self.consumed and not self.chain_handed and not self.chain_out and not self.absmax and not self.given, \
            (label, dict(self.begun), dict(self.consumed), self.chain_handed, self.chain_out, self.absmax, self.given)


def _plain(run):
    out = pa.snapshot(run())
    assert not pa.non_finite(out), pa.non_finite(out)
    return out


def _poisoned(run, plain, label):
    with pa.poisoned("max", int_sites=tuple(pa.INT_ALLOW)) as rec:
        out = pa.snapshot(run())
    assert not pa.is_patched()
    names = {pa.site_name(s) for s in rec}
    assert {"hip_ops.empty", "hip_ops._workspace", "hip_ops._f16x2_scratch"} <= names, sorted(names)
    mm = pa.first_mismatch(plain, out)
    assert mm is None, f"{label}: under the 'max' poison the first differing tap is {mm[0]} ({mm[1]} of {mm[2]} elements)"
    return "hip_ops._cmax_buffer" in names


def _equal(a, b, label):
    mm = pa.first_mismatch(a, b)
    assert mm is None, f"{label}: the handed maxima moved the output: first differing tap {mm[0]} ({mm[1]} of {mm[2]} elements)"
    assert torch.equal(a["fusion.depth"], b["fusion.depth"]) and all(torch.equal(a[f"fusion.gf_out{i}"], b[f"fusion.gf_out{i}"]) for i in range(6))


def test_handover_through_the_engine_on_the_128_tile_walk(switches, monkeypatch):  # noqa: F811
    from patchfusion_amd import hip_ops
    sp = Spies(monkeypatch)
    run = _model_run(_case(), "fp32")
    forced = {**WINO, **FORCE}
    switches(**forced)
    a = _plain(run)
    sp.assert_handed("hand-over arm")
    routes_a = list(sp.routes)
    assert _poisoned(run, a, "hand-over arm"), "the poisoned hand-over arm never allocated a cmax vector"
    # the range-pass arm: the same switches, the hand-over off
    with monkeypatch.context() as mp:
        mp.setattr(hip_ops, "_cmax_handover_enabled", lambda: False)
        sp.reset()
        b = _plain(run)
        sp.assert_none("range-pass arm")
        assert sp.routes == routes_a, "the range-pass arm runs other kernels: not a comparison of the maxima alone"
        _poisoned(run, b, "range-pass arm")
    _equal(a, b, "128-tile walk")
    # PF_WINO_F16X2_N256=2 itself: nothing handed; at this size the 128-tile layers leave fp16x2 (module docstring), so float32 grade, not bits
    switches(**dict(forced, PF_WINO_F16X2_N256="2"))
    sp.reset()
    c = _plain(run)
    sp.assert_none("PF_WINO_F16X2_N256=2")
    err = float((a["fusion.depth"] - c["fusion.depth"]).abs().max())
    print(f"\nCMAX 128-tile walk: {routes_a.count('wino3h')} fp16x2 launches in the forced arms, {sp.routes.count('wino3h')} under PF_WINO_F16X2_N256=2; "
          f"max |depth difference| {err:.3e}")
    if sp.routes == routes_a:
        _equal(a, c, "PF_WINO_F16X2_N256=2")
    else:                                                            # both arms are within F32_TOL of the reference (tests/test_e2e_gpu.py)
        assert err <= 2 * F32_TOL, err


def test_handover_through_the_engine_on_the_192_tile_walk(switches, monkeypatch):  # noqa: F811
    """every three-step layer on the 192-tile fp16x2 product at either value of PF_WINO_F16X2_N256: the arms as stated, bit for bit"""
    sp = Spies(monkeypatch)
    run = _model_run(_case(), "fp32")
    forced = {**WINO, **FORCE, **T192}
    switches(**forced)
    a = _plain(run)
    sp.assert_handed("hand-over arm")
    routes_a = list(sp.routes)
    assert _poisoned(run, a, "hand-over arm")
    switches(**dict(forced, PF_WINO_F16X2_N256="2"))
    sp.reset()
    b = _plain(run)
    sp.assert_none("PF_WINO_F16X2_N256=2")
    assert sp.routes == routes_a and "wino3h" in routes_a, "PF_WINO_F16X2_N256=2 runs other kernels here too"
    _poisoned(run, b, "PF_WINO_F16X2_N256=2")
    _equal(a, b, "192-tile walk")
    print(f"\nCMAX 192-tile walk: {routes_a.count('wino3h')} fp16x2 launches in both arms, equal bits on {len(a)} taps")
