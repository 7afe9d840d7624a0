"""The instrument of tests/poison_alloc.py checked without a GPU (devices=("cpu",)): the patch goes in and comes out, the fills have the stated
bits, integer tensors are left alone off the allow-list, the site record names the allocating frame of the package -- and the comparison of
tests/test_uninit_independence_gpu.py (poison_alloc.check_independent) FAILS for planted defects in the engine driven by tests/fake_ops.py.

Why two poisons: the fourth planted defect reads a region nobody wrote only through a maximum with zero, the way the HIP kernels apply ReLU on
load, pool, and take channel maxima: ``fmaxf(NaN, 0) = 0``.  (``torch.fmax`` is that function; ``torch.maximum`` and ``F.relu`` propagate a NaN,
which the device's ``fmaxf`` does not.)  Under the "nan" fill that run is bit for bit the zero-filled run: the NaN arm alone passes.  The "max"
fill -- finfo.max, finite -- goes through the maximum and moves the output."""
import collections

import pytest
import torch

from patchfusion_amd.config import make_config
from patchfusion_amd.model import PatchFusion
from patchfusion_amd.spec import patchfusion_spec, synthetic_state_dict
from tests import poison_alloc as pa
from tests.fake_ops import FakeOps

CPU = ("cpu",)
TINY = ("vits", (112, 154), (448, 616), (2, 2))
FLOATS = (torch.float32, torch.bfloat16, torch.float16)


# ------------------------------------------------------------------------------------------------------------ the patch itself
def test_the_four_entry_points_are_patched_and_restored():
    before = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    own = "new_empty" in torch.Tensor.__dict__
    with pa.poisoned("nan", devices=CPU) as rec:
        assert pa.is_patched()
        assert all(a is not b for a, b in zip(before, (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)))
        a = torch.empty(3, 5)
        b = torch.empty_like(a)
        c = torch.empty_strided((4, 2), (1, 4))
        d = a.new_empty((7,))
        e = torch.empty((2, 2), dtype=torch.float64, device="cpu")
        for t in (a, b, c, d, e):
            assert bool(torch.isnan(t).all())
        assert c.stride() == (1, 4) and d.dtype == a.dtype
        assert len(rec) == 5 and [s.nbytes for s in rec] == [60, 60, 32, 28, 32]
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == before
    assert ("new_empty" in torch.Tensor.__dict__) == own and not pa.is_patched()


def test_restored_after_an_exception_inside_the_block():
    before = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    with pytest.raises(KeyError):
        with pa.poisoned("max", devices=CPU):
            torch.empty(2)
            raise KeyError("inside")
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == before and not pa.is_patched()
    with pa.poisoned("zero", devices=CPU):                       # and it can be entered again
        assert float(torch.empty(1)) == 0.0
    assert not pa.is_patched()


def test_bad_arguments_leave_torch_alone():
    before = torch.empty
    with pytest.raises(ValueError):
        with pa.poisoned("ones", devices=CPU):
            pass
    with pytest.raises(ValueError, match="allow-list"):
        with pa.poisoned("nan", devices=CPU, int_sites=("engine.forward",)):
            pass
    with pa.poisoned("nan", devices=CPU):
        with pytest.raises(RuntimeError, match="nest"):
            with pa.poisoned("nan", devices=CPU):
                pass
        assert pa.is_patched()
    assert torch.empty is before


@pytest.mark.parametrize("dtype,bits_max,int_view", [(torch.float32, 0x7F7FFFFF, torch.int32), (torch.bfloat16, 0x7F7F, torch.int16),
                                                     (torch.float16, 0x7BFF, torch.int16)], ids=["f32", "bf16", "f16"])
def test_the_three_fills_have_the_stated_bits(dtype, bits_max, int_view):
    got = {}
    for fill in pa.MODES:
        with pa.poisoned(fill, devices=CPU):
            got[fill] = torch.empty((5, 3), dtype=dtype)
    assert bool((got["zero"].view(int_view) == 0).all())                       # +0.0: all bits zero
    assert bool(torch.isnan(got["nan"]).all())
    assert bool((got["max"].view(int_view) == bits_max).all())
    assert bool(torch.isfinite(got["max"]).all()) and float(got["max"].float().max()) == torch.finfo(dtype).max
    # what the poison is for: finite, not swallowed by a maximum, and it overflows as soon as it is summed or multiplied
    mx = got["max"].float()
    assert bool((torch.fmax(mx, torch.zeros(())) == mx).all()) and bool(torch.isinf((got["max"] + got["max"])).all())
    assert bool((torch.fmax(got["nan"].float(), torch.zeros(())) == 0).all())  # fmaxf swallows the NaN


def test_integer_tensors_are_untouched_off_the_allow_list():
    probe = torch.empty(64, dtype=torch.int32).fill_(1234567)                  # (what an untouched allocation looks like cannot be known: count instead)
    del probe
    for fill in pa.MODES:
        with pa.poisoned(fill, devices=CPU) as rec:
            for dt in (torch.int32, torch.uint8, torch.int64, torch.bool, torch.int16):
                torch.empty(16, dtype=dt)
                torch.empty(16, dtype=torch.float32).new_empty(8, dtype=dt)
            n_int = len([s for s in rec if not s.dtype.is_floating_point])
        assert n_int == 0 and len(rec) == 5                                    # the five float32 parents alone
    with pa.poisoned("max", devices=("cuda",)) as rec:                         # another device is not this one's business
        t = torch.empty(4)
    assert rec == []


def test_allow_listed_integer_sites_get_the_byte_patterns():
    """hip_ops._cmax_buffer and hip_ops._f16x2_scratch are what the allow-list names; here a stand-in function of that name in a stand-in module
    file name is not possible without the device, so the rule is checked on the record: a site is poisoned iff its name is in int_sites"""
    assert set(pa.INT_ALLOW) == {"hip_ops._cmax_buffer", "hip_ops._f16x2_scratch"} and all(len(v) > 20 for v in pa.INT_ALLOW.values())
    assert pa._int_fill_value(torch.int32, "zero") == 0 and pa._int_fill_value(torch.int32, "nan") == -1
    assert pa._int_fill_value(torch.int32, "max") == 0x7F7F7F7F and pa._int_fill_value(torch.uint8, "nan") == 0xFF
    assert pa._int_fill_value(torch.uint8, "max") == 0x7F
    with pa.poisoned("max", devices=CPU, int_sites=("hip_ops._cmax_buffer",)) as rec:
        torch.empty(8, dtype=torch.int32)                                      # allocated HERE, not in hip_ops._cmax_buffer
    assert rec == []


class _Ops(FakeOps):
    """the torch op set with the product's `empty` (tests/fake_ops.py NaN-fills its own: here the instrument does the filling)"""
    @staticmethod
    def empty(shape, dtype, device):
        return torch.empty(shape, dtype=dtype, device=device)


def test_the_site_record_names_the_package_frame():
    from patchfusion_amd.engine import BinsHead
    head = object.__new__(BinsHead)
    head.clb_channels, head.dtype, head.device = 168, torch.float32, torch.device("cpu")
    with pa.poisoned("nan", devices=CPU) as rec:
        buf = head.new_clb_buffer(_Ops, 1, 4, 6)
    assert bool(torch.isnan(buf).all()) and len(rec) == 1
    s = rec[0]
    assert s.file == "patchfusion_amd/engine.py" and s.func == "new_clb_buffer" and pa.site_name(s) == "engine.new_clb_buffer"
    assert s.dtype == torch.float32 and s.nbytes == 4 * 6 * 168 * 4 and s.line > 0
    with pa.poisoned("nan", devices=CPU, sites=lambda r: r.func == "nowhere") as rec:          # the bisecting predicate: poison only these
        head.new_clb_buffer(_Ops, 1, 4, 6)
    assert rec == []


def test_the_comparison_is_on_bits_and_names_the_first_entry_in_order():
    a = collections.OrderedDict(x=torch.zeros(4), y=torch.tensor([1.0, float("nan")]), z=torch.arange(3), s=torch.tensor([1.0, 1e6], dtype=torch.float64))
    b = pa.snapshot(a)
    assert pa.first_mismatch(a, b) is None                                     # a NaN equals itself as an integer ...
    assert pa.non_finite(a) == ["y"]                                           # ... and is refused by the finite check instead
    b["z"][2] = 7
    b["y"][0] = 2.0
    assert pa.first_mismatch(a, b) == ("y", 1, 2)                              # y comes before z
    b = pa.snapshot(a)
    b["x"][1] = -0.0
    assert pa.first_mismatch(a, b) == ("x", 1, 4)                              # bits, not values
    b = pa.snapshot(a)
    del b["z"]
    assert pa.first_mismatch(a, b) == ("z", 3, 3)
    # sums accumulated in no fixed order: held to a relative bound, everything else still to bits; a NaN is a difference
    b = pa.snapshot(a)
    b["s"] *= 1 + 2.0 ** -50
    assert pa.first_mismatch(a, b) == ("s", 2, 2) and pa.first_mismatch(a, b, reorder={"s": 2.0 ** -49}) is None
    assert pa.first_mismatch(a, b, reorder={"s": 2.0 ** -52}) == ("s", 2, 2)
    b["s"][0] = float("nan")
    assert pa.first_mismatch(a, b, reorder={"s": 1.0}) == ("s", 1, 2)


# ------------------------------------------------------------------------------------------------------------ planted defects
@pytest.fixture(scope="module")
def tiny():
    cfg = make_config(*TINY)
    sd = synthetic_state_dict(patchfusion_spec(cfg), 0)
    g = torch.Generator().manual_seed(1234)
    lr = torch.rand(1, 3, *TINY[1], generator=g)
    crops = torch.rand(1, 3, *TINY[1], generator=g)
    rois = torch.tensor([[0.0, 77.0, 56.0, 154.0, 112.0]])
    return cfg, sd, lr, crops, rois


def _run(tiny, ops):
    """coarse branch + G2L, then fine branch + fusion for one crop: every tap in forward order, the final depth last.  The model is built inside
    the arm (this function is called under the poison)"""
    cfg, sd, lr, crops, rois = tiny

    def run():
        m = PatchFusion(cfg, compute_dtype="fp32", ops=ops).eval()
        m.load_state_dict(sd, strict=True)
        out, ct, ft = collections.OrderedDict(), {}, {}
        st = m._coarse(lr, ct)
        for k, v in ct.items():
            out["coarse." + k] = v
        for i, f in enumerate(st["feats"]):
            out[f"coarse.feat{i}"] = f
        for i, f in enumerate(st["g2l"]):
            out[f"g2l{i}"] = f
        out["coarse.depth"] = st["depth"]
        d = m.infer_forward(crops, rois, taps=ft)
        for k, v in ft.items():
            out["fusion." + k] = v
        out["depth"] = d
        return out
    return run


def test_the_engine_on_the_torch_ops_is_independent(tiny):
    stats = pa.check_independent(_run(tiny, _Ops()), devices=CPU, must_reach=("engine.forward", "engine.new_clb_buffer", "engine.run"), label="fake ops")
    assert stats["nan"] == stats["max"] == stats["zero"] and stats["max"][0] > 100


class _DropLastChannel(_Ops):
    @staticmethod
    def copy_channels(x, y):
        FakeOps.copy_channels(x[..., :-1], y)


class _DropLastSource(_Ops):
    @staticmethod
    def resize_concat(xs, y):
        FakeOps.resize_concat(xs[:-1], y)


class _LeaveLastRow(_Ops):
    @staticmethod
    def conv(x, pw, y, *a, **k):
        if y.dim() != 4 or y.shape[1] < 2:
            return FakeOps.conv(x, pw, y, *a, **k)
        keep = y[:, -1].clone()
        FakeOps.conv(x, pw, y, *a, **k)
        y[:, -1] = keep
        return y


class _PoolReadsPastTheEdge(_Ops):
    """max-pool over a scratch copy two columns wider than what it wrote, ReLU on load (exact for its inputs, which are outputs of a ReLU): the
    stray column reaches the output through maxima alone"""
    @staticmethod
    def maxpool2(x, y):
        B, H, W, C = x.shape
        s = torch.empty((B, H, W + 2, C), dtype=torch.float32, device=x.device)
        s[:, :, :W] = x.float()
        s = torch.fmax(s, torch.zeros((), dtype=s.dtype))                              # relu_in with fmaxf
        stray = s[:, :, W:].amax(dim=(1, 2), keepdim=True)                              # [B,1,1,C] (no NaN is left after the fmax)
        h, w = H // 2, W // 2
        pooled = torch.fmax(torch.fmax(s[:, 0::2, 0:W:2][:, :h, :w], s[:, 0::2, 1:W:2][:, :h, :w]),
                            torch.fmax(s[:, 1::2, 0:W:2][:, :h, :w], s[:, 1::2, 1:W:2][:, :h, :w]))
        y[..., :C] = torch.fmax(pooled, stray).to(y.dtype)


@pytest.mark.parametrize("ops,first", [(_DropLastChannel, "g2l0"),               # its first caller is G2LNet.forward_level
                                       (_DropLastSource, "fusion.gf_out1"),       # the Upv1 concat buffer of decoder level 1
                                       (_LeaveLastRow, "coarse.dpt_layer1_rn")],  # the first tap below the DPT projections
                         ids=["copy_channels", "resize_concat", "conv"])
def test_a_skipped_write_fails_the_comparison_under_both_poisons(tiny, ops, first):
    run = _run(tiny, ops())
    outs = {}
    for fill in pa.MODES:
        with pa.poisoned(fill, devices=CPU):
            outs[fill] = pa.snapshot(run())
    assert not pa.non_finite(outs["zero"])
    for fill in ("nan", "max"):
        mm = pa.first_mismatch(outs["zero"], outs[fill])
        assert mm is not None, f"the {fill} arm missed the planted defect"
        print(f"{ops.__name__} under {fill}: first differing tap {mm[0]}, {mm[1]} of {mm[2]} elements")
        assert mm[0] == first, (fill, mm)                         # the first tap in forward order downstream of the first skipped write
    with pytest.raises(AssertionError, match=f"depends on uninitialised memory.*first differing tap is {first} "):
        pa.check_independent(run, devices=CPU, label=ops.__name__)
    assert not pa.is_patched()


def test_a_read_through_a_maximum_passes_the_nan_arm_and_fails_the_max_arm(tiny):
    """the reason both arms exist"""
    run = _run(tiny, _PoolReadsPastTheEdge())
    outs = {}
    for fill in pa.MODES:
        with pa.poisoned(fill, devices=CPU):
            outs[fill] = pa.snapshot(run())
    assert pa.first_mismatch(outs["zero"], outs["nan"]) is None and not pa.non_finite(outs["nan"]), "fmaxf swallows the NaN: this arm sees nothing"
    mm = pa.first_mismatch(outs["zero"], outs["max"])
    assert mm is not None and mm[0].startswith("fusion."), mm
    with pytest.raises(AssertionError, match="under the 'max' fill"):
        pa.check_independent(run, devices=CPU, label="pool")
    # ... and the planted pool is the right pool wherever the stray column holds nothing: the zero run is the clean engine's
    with pa.poisoned("zero", devices=CPU):
        clean = pa.snapshot(_run(tiny, _Ops())())
    assert pa.first_mismatch(clean, outs["zero"]) is None
