"""pytest -m gpu: no output of the engine depends on the initial contents of an allocation it makes itself.

The per-kernel tests pre-fill the outputs they hand to a kernel; what engine.py, midas_core.py and the wrappers of hip_ops.py allocate with
``torch.empty`` -- concat buffers written slice by slice, the CLB buffer's padded tail, u5, the plane buffers of the split and fp16x2 linears, the
contexts of the head's backward, q / k / vt padded to Sp, the Winograd V / M arenas reused window after window with a ragged last window, the
workspaces of wgrad and SILog -- they cannot see.  Here every such allocation is poisoned (tests/poison_alloc.py) and whole runs are compared bit
for bit: under the "zero" fill twice (the runs must be deterministic, else the comparison means nothing), then under "nan" and under "max"
(finfo.max: finite, so it goes through the ``fmaxf`` of ReLU-on-load, max-pool, the range pass and the channel maxima, which swallow a NaN).  The
final depth and every tap the interface exposes (``taps=`` of ``_coarse`` / ``infer_forward``, ``_coarse_state``, the head's 44 gradients) must be
equal as integers and finite; a failure names the first differing tap in forward order and the number of differing elements.  The model is built
inside each arm (packing and the engine build run under the poison); inputs and state dicts are built outside.

Geometry: tests/test_e2e_gpu.py TINY (Depth-Anything vits, process shape 112 x 154, image 448 x 616, 2 x 2 tiles) unless a configuration says
otherwise: vitl at the same geometry for the 160 x 256 fp16x2 tile (N = 1024); vitb at process shape 224 x 308 with eight crops for the bf16
ping-pong GEMM (``pp`` needs 2048 token rows and 512 channels: 8 x 353 rows, D = 768); the native BEiT-L core at its 384 x 512 (24 x 32 grid).
Three-step Winograd layers run in several windows with a ragged last one under PF_WS_CAP_GB=0.02 (192 tiles per window: 704 tiles = 3 x 192 + 128
at 2 x 64 x 88, 2184 = 11 x 192 + 72 at 2 x 112 x 154).

Every run asserts that its record holds ``HipOps.empty`` and the sites its configuration must reach (an engine.py / model.py / midas_core.py
caller, ``hip_ops._workspace``, the q / k / vt lines of ``hip_ops.vit_attention`` ...): the guard that the patch is in effect.  packing.py allocates
nothing with ``empty`` (its planes come from ``zeros`` and arithmetic), so there is no packing site to assert.
Every configuration asserts the routes of HipOps._conv_exec it is there for; test_route_coverage asserts the union when the whole module ran.
No dependence was found: see DESIGN.md (test strategy) and profiles/r14_uninit_independence.log for sites, bytes and seconds per configuration.
"""
import collections
import functools
import os
import random
import time

import pytest
import torch

from patchfusion_amd.config import make_config
from patchfusion_amd.model import PatchFusion
from patchfusion_amd.spec import patchfusion_spec, synthetic_state_dict
from tests import poison_alloc as pa
from tests.test_cmax_chain_gpu import FORCE
from tests.test_e2e_gpu import TINY
from tests.test_float32_grade_gpu import WINO
from tests.test_midas_core_gpu import full_core  # noqa: F401  (module-scoped fixture: the seeded float64 restatement and a core loaded from it)

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("PF_WINOGRAD", "PF_WINOGRAD_MIN_PIXELS", "PF_WINO_FUSED", "PF_WS_CAP_GB", "PF_WINO_F16X2", "PF_WINO_F16X2_N256", "PF_WINO_SPLIT3",
        "PF_S3_PERSIST", "PF_S3_T192", "PF_S3_TILE_NOW", "PF_VIT_F16X2", "PF_VIT_ATTN_F16X2", "PF_LINEAR_SPLIT3", "PF_CONV1X1_SPLIT3", "PF_ATTN_QKV",
        "PF_F16_TILE", "PF_BF16_PP", "PF_BINS_TAIL")
WINDOWS = dict(PF_WS_CAP_GB="0.02")
ALL_ROUTES = ("direct", "s3_1x1", "fused", "wino3", "wino3h", "wino", "pp")
ROUTES = collections.Counter()          # route -> launches, over the module
MULTI = collections.Counter()           # route -> three-step launches that ran in more than one window
RAN = []                                # configurations that ran: test_route_coverage asserts the union only after all of them
N_CONFIGS = 19


def _engine_site(s):
    return s.caller is not None and s.caller.startswith("patchfusion_amd/engine.py")


def _midas_site(s):
    return s.caller is not None and s.caller.startswith("patchfusion_amd/midas_core.py")


def _model_site(s):
    return s.caller is not None and s.caller.startswith("patchfusion_amd/model.py")


@pytest.fixture
def switches():
    from patchfusion_amd import hip_ops
    old = {k: os.environ.get(k) for k in KEYS}

    def set_env(**kw):
        assert set(kw) <= set(KEYS), sorted(set(kw) - set(KEYS))
        for k in KEYS:
            os.environ.pop(k, None)
        os.environ.update(kw)
        hip_ops.refresh_env()
    yield set_env
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    hip_ops.refresh_env()


@pytest.fixture
def spy(monkeypatch):
    """routes of HipOps._conv_exec and calls of the ViT block ops, for this test (and added to the module's counters)"""
    from patchfusion_amd.hip_ops import HipOps
    seen = collections.Counter()
    real_exec = HipOps._conv_exec

    def conv_exec(route, p, extra, device, **kw):
        seen[route] += 1
        ROUTES[route] += 1
        if route in ("wino3", "wino3h"):
            T = p.B * -(-p.H // 4) * -(-p.W // 4)
            if 0 < extra[5] < T:
                seen["windows:" + route] += 1
                MULTI[route] += 1
                if T % extra[5]:
                    seen["ragged:" + route] += 1
        return real_exec(route, p, extra, device, **kw)
    monkeypatch.setattr(HipOps, "_conv_exec", staticmethod(conv_exec))
    for name in ("conv_f16x2", "conv_split3", "vit_attention", "vit_attention_f16x2", "layernorm", "layernorm_split3", "layernorm_f16x2", "bins_tail"):
        def wrap(*a, _real=getattr(HipOps, name), _name=name, **k):
            seen[_name] += 1
            return _real(*a, **k)
        monkeypatch.setattr(HipOps, name, staticmethod(wrap))
    return seen


@functools.lru_cache(maxsize=None)
def _case(enc=TINY[0], ps=TINY[1], raw=TINY[2], split=TINY[3], crops=2):
    """config, seeded state dict and inputs (all built outside the arms)"""
    cfg = make_config(enc, ps, raw, split)
    sd = synthetic_state_dict(patchfusion_spec(cfg), 0)
    g = torch.Generator().manual_seed(1234)
    img = torch.rand(1, 3, *raw, generator=g).to(DEV)
    cr = torch.rand(crops, 3, *ps, generator=g).to(DEV)
    # boxes in process coordinates: the four quadrants, then shifted boxes (fractional bin centres in roi_align)
    H, W = ps
    boxes = [[0, 0, W / 2, H / 2], [W / 2, H / 2, W, H], [W / 2, 0, W, H / 2], [0, H / 2, W / 2, H], [W / 4, H / 4, 3 * W / 4, 3 * H / 4],
             [W / 8, 0, 5 * W / 8, H / 2], [0, H / 8, W / 2, 5 * H / 8], [3 * W / 8, 3 * H / 8, 7 * W / 8, 7 * H / 8]][:crops]
    rois = torch.tensor([[0.0] + b for b in boxes], dtype=torch.float32).to(DEV)
    return cfg, sd, img, cr, rois


def _model_run(case, dtype, mode=None, process_num=2):
    """-> run(): build the model, coarse branch + G2L with taps, fine branch + fusion of the crops with taps, and (mode) the whole tiled inference"""
    cfg, sd, img, crops, rois = case

    def run():
        m = PatchFusion(cfg, compute_dtype=dtype).eval()
        m.load_state_dict(sd, strict=True)
        m = m.to(DEV)
        lr = m.resizer(img)
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
        out["fusion.depth"] = d
        if mode is not None:
            random.seed(5621)                                     # as tests/test_e2e_gpu.py seeds the random tiles of r4
            d, _ = m(mode="infer", image_lr=lr, image_hr=img, cai_mode=mode, process_num=process_num)
            for i, f in enumerate(m._coarse_state["feats"]):
                out[f"infer.coarse_feat{i}"] = f
            for i, f in enumerate(m._coarse_state["g2l"]):
                out[f"infer.g2l{i}"] = f
            out["infer.coarse_depth"] = m._coarse_state["depth"]
            out["depth"] = d
        torch.cuda.synchronize()
        return out
    return run


def _check(name, run, must_reach=("hip_ops.empty",), int_sites=(), reorder=None):
    t0 = time.time()
    stats = pa.check_independent(run, must_reach=must_reach, int_sites=int_sites, label=name, reorder=reorder)
    torch.cuda.synchronize()
    dt = time.time() - t0
    assert stats["nan"] == stats["max"], (name, stats)            # the same allocations in every poisoned arm
    print(f"\nUNINIT {name}: {stats['max'][0]} poisoned sites, {stats['max'][1] / 2 ** 20:.1f} MiB poisoned per run, four runs (each with its model build) "
          f"in {dt:.1f} s")
    RAN.append(name)
    return stats


ENGINE = ("hip_ops.empty", _engine_site)


# ------------------------------------------------------------------------------------------------ 1, 2: fp32, the three tile schedules
@pytest.mark.parametrize("mode", ["m1", "m2", "r4"])
def test_vits_fp32_infer(switches, spy, mode):
    """default switches.  m1: the plain grid; m2 / r4: the shifted and the random tiles -- the stitch and running-average buffers.  The fine branch
    runs the default ViT block: fp16x2 linears, fp16x2 attention and projection (PF_VIT_ATTN_F16X2=2)"""
    switches()
    _check(f"vits fp32 infer {mode}", _model_run(_case(), "fp32", mode, 2), ENGINE + (_model_site,))
    assert spy["conv_f16x2"] and spy["vit_attention_f16x2"] and spy["layernorm_f16x2"] and spy["conv_split3"] and spy["bins_tail"], dict(spy)
    assert spy["direct"], dict(spy)


# ------------------------------------------------------------------------------------------------ 3: bf16
def test_vits_bf16_infer(switches, spy):
    """bf16 mode: the attention goes through pf_qkv_split with the wrapper's own q / k / vt (vt padded to Sp = 128 columns for S = 89)"""
    switches()
    _check("vits bf16 infer m1", _model_run(_case(), "bf16", "m1", 2), ENGINE + ("hip_ops.vit_attention",))
    assert spy["vit_attention"] and not spy["conv_f16x2"] and not spy["conv_split3"], dict(spy)


# ------------------------------------------------------------------------------------------------ 4: the Winograd routes, windowed
def test_vits_fp32_winograd_f16x2_windows(switches, spy):
    """three-step Winograd forced at this size on the persistent 128-tile walk, fp16x2 on every such layer, several windows with a ragged last one"""
    switches(**{**WINO, **FORCE, **WINDOWS})
    _check("vits fp32 wino3h windows", _model_run(_case(), "fp32"), ENGINE + ("hip_ops._workspace", "hip_ops._f16x2_scratch", "hip_ops._cmax_buffer"),
           int_sites=tuple(pa.INT_ALLOW))
    assert spy["wino3h"] and spy["windows:wino3h"] and spy["ragged:wino3h"] and not spy["fused"], dict(spy)


def test_vits_fp32_winograd_bf16x3_windows(switches, spy):
    """the same with PF_WINO_F16X2=0: the bf16x3 form of every three-step layer"""
    switches(**{**WINO, **FORCE, **WINDOWS, "PF_WINO_F16X2": "0"})
    _check("vits fp32 wino3 windows", _model_run(_case(), "fp32"), ENGINE + ("hip_ops._workspace",))
    assert spy["wino3"] and spy["windows:wino3"] and spy["ragged:wino3"] and not spy["wino3h"], dict(spy)


def test_vits_fp32_winograd_f32_three_step(switches, spy):
    """PF_WINO_SPLIT3=0: the float32 three-step form (whole-layer V / M arenas)"""
    switches(**dict(WINO, PF_WINO_SPLIT3="0"))
    _check("vits fp32 wino f32", _model_run(_case(), "fp32"), ENGINE + ("hip_ops._workspace",))
    assert spy["wino"] and not spy["wino3"] and not spy["wino3h"], dict(spy)


def test_vits_fp32_fused_winograd_and_split_1x1(switches, spy):
    """PF_WINO_FUSED=2 and PF_CONV1X1_SPLIT3=2: the fused Winograd kernel and the split-precision 1x1 kernel wherever they are supported"""
    switches(PF_WINO_FUSED="2", PF_CONV1X1_SPLIT3="2")
    _check("vits fp32 fused + s3_1x1", _model_run(_case(), "fp32"), ENGINE)
    assert spy["fused"] and spy["s3_1x1"], dict(spy)


# ------------------------------------------------------------------------------------------------ 5: ViT block routes
def test_vit_block_bf16x3_planes(switches, spy):
    switches(PF_VIT_F16X2="0")
    _check("vits fp32 PF_VIT_F16X2=0", _model_run(_case(), "fp32"), ENGINE)
    assert spy["conv_split3"] and spy["layernorm_split3"] and not spy["conv_f16x2"] and not spy["vit_attention_f16x2"], dict(spy)


def test_vit_block_f32_mfma(switches, spy):
    switches(PF_LINEAR_SPLIT3="0", PF_CONV1X1_SPLIT3="0")
    _check("vits fp32 f32 MFMA linears", _model_run(_case(), "fp32"), ENGINE)
    assert spy["vit_attention"] and not spy["conv_split3"] and not spy["conv_f16x2"] and not spy["s3_1x1"], dict(spy)


def test_vit_block_qkv_split_fp32(switches, spy):
    """PF_ATTN_QKV=0 on float32 q / k / v rows (they exist with the f32 linears): pf_qkv_split + pf_vit_attention on the wrapper's own temporaries"""
    switches(PF_ATTN_QKV="0", PF_LINEAR_SPLIT3="0")
    _check("vits fp32 PF_ATTN_QKV=0", _model_run(_case(), "fp32"), ENGINE + ("hip_ops.vit_attention",))


def test_vit_block_qkv_split_bf16(switches, spy):
    switches(PF_ATTN_QKV="0")
    _check("vits bf16 PF_ATTN_QKV=0", _model_run(_case(), "bf16"), ENGINE + ("hip_ops.vit_attention",))


def test_vitl_fp32_tile160(switches, spy):
    """vitl (D = 1024) at the tiny geometry with PF_F16_TILE=1: proj and fc2 (N = 1024) on the 160 x 256 fp16x2 tile, 178 rows = one ragged tile"""
    switches(PF_F16_TILE="1")
    _check("vitl fp32 PF_F16_TILE=1", _model_run(_case(enc="vitl"), "fp32"), ENGINE)
    assert spy["conv_f16x2"] and spy["vit_attention_f16x2"], dict(spy)


def test_vitb_bf16_pingpong_gemm(switches, spy):
    """PF_BF16_PP=1, vitb (D = 768) at process shape 224 x 308 with eight crops: 8 x 353 = 2824 token rows through the 256 x 128 ping-pong GEMM"""
    switches(PF_BF16_PP="1")
    _check("vitb bf16 PF_BF16_PP=1", _model_run(_case(enc="vitb", ps=(224, 308), crops=8), "bf16"), ENGINE)
    assert spy["pp"], dict(spy)


# ------------------------------------------------------------------------------------------------ 6: the native MiDaS BEiT-L core
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_native_midas_core(switches, spy, full_core, dtype):  # noqa: F811
    """DPT_BEiT_L_384 at 384 x 512, one image; the weights are repacked inside each arm"""
    switches()
    core = full_core[1]
    img = torch.rand(1, 3, 384, 512, device=DEV, generator=torch.Generator(device=DEV).manual_seed(21))
    names = ["l4_rn", "r4", "r3", "r2", "r1", "out_conv"]

    def run():
        core.forget_packed()
        rel, feats = core(img)
        out = collections.OrderedDict(zip(names, feats))
        out["rel_depth"] = rel
        torch.cuda.synchronize()
        return out
    old = core.call_dtype
    core.call_dtype = dtype
    try:
        _check(f"midas BEiT-L core {str(dtype).split('.')[1]}", run, ("hip_ops.empty", _midas_site) + (("hip_ops.vit_attention_rpb_bf16",) if dtype == torch.bfloat16 else ()))
        assert core._packed["dtype"] == dtype
    finally:
        core.call_dtype = old
        core.forget_packed()


# ------------------------------------------------------------------------------------------------ 7: training
def test_train_forward_and_head_backward(switches, spy):
    """the configuration of tests/test_head_bwd_gpu.py test_public_interface_on_the_device: loss, depth, the 44 head gradients and the gradients
    that reach the head's inputs.  (The three SILog sums are double atomicAdds over 135 blocks, like the metric sums below, but they reach the
    outputs only through a rounding to float32 -- the loss, and d_pred = (float)(double expression) per pixel: a few ulps of a double move one of
    34 496 float32 roundings with probability ~1e-15 / 6e-8 each, ~1e-3 per test run.  Should the two zero-filled runs ever differ here, that is
    the cause, and the message says so.)"""
    from patchfusion_amd.engine import BinsHead
    from tests.test_train_forward_cpu import TINY as TRAIN_TINY, train_batch
    switches()
    cfg = make_config(*TRAIN_TINY)
    sd = synthetic_state_dict(patchfusion_spec(cfg), 0)
    image_lr, crops, bboxs, gt = (t.to(DEV) for t in train_batch())
    names = BinsHead.param_names()
    assert len(names) == 44

    def run():
        m = PatchFusion(cfg, compute_dtype="fp32").eval()
        m.load_state_dict(sd, strict=True)
        m = m.to(DEV)
        loss, aux = m.train_forward(image_lr, crops, gt, bboxs, head_grad=True)
        inputs = m.head_backward()
        out = collections.OrderedDict(depth=aux["depth_pred"], loss=loss["total_loss"])
        # backward order: the tail first, the seed layers last (BinsHead.backward)
        out["d_last"] = inputs["last"]
        for i in reversed(range(4)):
            out[f"d_x_block{i}"] = inputs["x_blocks"][i]
        out["d_x0"] = inputs["x0"]
        for n in reversed(names):
            out["grad." + n] = m.get_parameter(n).grad
        torch.cuda.synchronize()
        return out
    _check("vits fp32 train_forward + head_backward", run, ENGINE + ("hip_ops.conv1x1_wgrad", "hip_ops.silog_loss_saved", _model_site))


# ------------------------------------------------------------------------------------------------ 8: pre- and post-processing
def test_image_preprocessor(switches):
    from patchfusion_amd.preprocess import ImagePreprocessor
    switches()
    img = torch.randint(0, 256, (61, 83, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))

    def run():
        r = ImagePreprocessor(image_resolution=(96, 128), process_shape=(42, 56), device=DEV)(img)
        torch.cuda.synchronize()
        return collections.OrderedDict(image_hr=r["image_hr"], image_lr=r["image_lr"])
    _check("ImagePreprocessor 61x83 -> 96x128", run, ("preprocess.__call__",))


def test_colorize_and_metrics(switches, monkeypatch):
    """colorize with its own percentiles: bit for bit.  compute_metrics: depth_metrics_kernel (csrc/io.hip) adds the partial sums of its 24 blocks
    into the 13 float64 results with atomicAdd, in no fixed order, so two runs of it do not agree to the last bit whatever the memory held (measured:
    silog differed between the two zero-filled runs).  The metrics are host arithmetic on those sums, so the sums are what is compared: the five
    counts exactly (sums of ones: exact in any order), the six sums of non-negative float32 terms within 2 n u of each other (n <= 6144 terms, u =
    2^-53: each order is within (n - 1) u of the exact sum, Higham 4.4), and the signed sum of e = log p - log g after division by
    sqrt(count * sum e^2) >= sum |e| (Cauchy-Schwarz), which makes the same bound an absolute one.  A read of the poisoned result buffer would
    move them by 1.8e308 or a NaN."""
    from patchfusion_amd import postprocess
    from patchfusion_amd.hip_ops import HipOps
    switches()
    g = torch.Generator().manual_seed(9)
    pred = (0.5 + 4 * torch.rand(64, 96, generator=g)).to(DEV)
    gt = (0.5 + 4 * torch.rand(64, 96, generator=g)).to(DEV)
    gt[:3] = 0.0                                                   # invalid rows
    sums = []
    real = HipOps.depth_metrics
    monkeypatch.setattr(HipOps, "depth_metrics", staticmethod(lambda *a, **k: (real(*a, **k), sums.append(a[6]))[0]))
    bound = 2 * 64 * 96 * 2.0 ** -53

    def run():
        out = collections.OrderedDict()
        out["colorize"] = postprocess.colorize(pred)               # its own 2nd / 95th percentiles
        r = postprocess.compute_metrics(gt, pred, eigen_crop=False)
        assert all(v == v for v in r.values()), r
        s = sums.pop()
        out["metric_sums.counts"] = s[[0, 1, 2, 3, 12]]
        out["metric_sums.nonneg"] = s[[4, 5, 6, 7, 9, 10, 11]]
        out["metric_sums.signed"] = 1.5 + 0.5 * s[8] / torch.sqrt(s[0] * s[9])         # in [1, 2]: the relative bound is an absolute one
        torch.cuda.synchronize()
        return out
    _check("colorize + compute_metrics 64x96", run, ("hip_ops.percentiles", "postprocess.compute_metrics"),
           reorder={"metric_sums.nonneg": bound, "metric_sums.signed": 2 * bound})


# ------------------------------------------------------------------------------------------------ the instrument on the device
def test_a_planted_skipped_write_is_caught_on_the_device(switches, monkeypatch):
    """the comparison above fails on the device for a write that skips part of a buffer (the CPU planted defects of tests/test_poison_alloc_cpu.py
    prove the comparison, this one that the fills are in effect where the HIP kernels read): copy_channels leaves the last eight channels.  Its
    first caller is G2LNet.forward_level, so g2l0 is the first tap to move, under either poison."""
    from patchfusion_amd.hip_ops import HipOps
    switches()
    real = HipOps.copy_channels
    monkeypatch.setattr(HipOps, "copy_channels", staticmethod(lambda x, y, cmax=None: real(x[..., :-8], y, cmax=None if cmax is None else cmax[:-8])))
    run = _model_run(_case(), "fp32")
    outs = {}
    for fill in pa.MODES:
        with pa.poisoned(fill) as rec:
            outs[fill] = pa.snapshot(run())
        assert rec
    for fill in ("nan", "max"):
        mm = pa.first_mismatch(outs["zero"], outs[fill])
        assert mm is not None and mm[0] == "g2l0", (fill, mm)
    with pytest.raises(AssertionError, match="depends on uninitialised memory.*first differing tap is g2l0 "):
        pa.check_independent(run, label="planted")
    assert not pa.is_patched()


# ------------------------------------------------------------------------------------------------ the union
def test_route_coverage():
    """over the configurations above every route of HipOps._conv_exec ran (each configuration asserts its own), three-step layers ran in more than
    one window, and nothing left torch patched"""
    assert not pa.is_patched()
    print("\nUNINIT routes:", dict(ROUTES), "three-step launches in several windows:", dict(MULTI))
    if len(RAN) >= N_CONFIGS:                                      # the whole module ran
        missing = [r for r in ALL_ROUTES if not ROUTES[r]]
        assert not missing, missing
        assert MULTI["wino3"] and MULTI["wino3h"], dict(MULTI)
