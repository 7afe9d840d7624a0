"""pytest -m gpu: every float32 conv / linear route held to float64, element by element (tests/f64_ref.py).

Each case pins the PF_* switches it needs, asserts its route (HipOps._conv_plan), fills its output with NaN (channels outside a view must stay
NaN), starts from cold caches (op_checks._flush_caches), and runs the same operands through the float32 baseline: the f32-MFMA kernel
(`_direct=True`) for 1x1, linear and direct cases, the f32 three-step route (PF_WINO_SPLIT3=0) for the Winograd routes -- that route itself
checked against the direct kernel.  The bar (f64_ref.float32_grade): element-wise and normwise error each at most twice the baseline's, normwise
<= 2e-6 (1x1 / linear routes) or 3.2e-5 (Winograd routes), element-wise <= f64_ref.ELEM_CAP_GEMM / ELEM_CAP_WINO.  The direct and f32 three-step
routes and the fused-only layers are float32 routes themselves: they are held to the caps.  Measured errors: profiles/r9_float32_grade.log.

Input kinds (each for every route, not every shape x kind): random; per-input-channel scales 1e-3 .. 1e3 with compensating weights (wide);
spike pixels / rows at 1e3x; per-output-column magnitudes 1e-3 .. 1e3 through the weight rows and the bias (cols); all-zero input channels
(dead; zero-gamma channels for the LayerNorm producers); channel scales of 2^+-40 (pow40, wino3h: the route with per-channel runtime scales)."""
import os

import pytest
import torch

from patchfusion_amd import packing as pk
from patchfusion_amd._lib import PfError
from tests import f64_ref as R
from tests import op_checks

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("PF_WINOGRAD", "PF_WINOGRAD_MIN_PIXELS", "PF_WINO_FUSED", "PF_WS_CAP_GB", "PF_WINO_F16X2", "PF_WINO_SPLIT3", "PF_S3_PERSIST", "PF_S3_T192",
        "PF_S3_TILE_NOW", "PF_CONV1X1_SPLIT3", "PF_HALO_FORCE")
WINO = dict(PF_WINOGRAD="4", PF_WINOGRAD_MIN_PIXELS="0", PF_WINO_FUSED="0", PF_S3_PERSIST="2")
T192 = dict(PF_S3_T192="2", PF_S3_TILE_NOW="192")
RAN = []                       # (case, route) of every case that ran: test_route_coverage
LOG = []


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


def _log(line):
    """one line of the per-case error table (printed: run with -s)"""
    print(line)
    LOG.append(line)


def _operands(kind, cout, cin, k, seed, cin_real=None):
    """float32 weight [cout, cin, k, k], bias, and the per-channel input factor s (float64 [cin]) of an input kind"""
    g = torch.Generator().manual_seed(seed)
    cin_real = cin_real or cin
    w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) / (cin_real * k * k) ** 0.5
    w[:, cin_real:] = 0
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    s = torch.ones(cin, dtype=torch.float64)
    if kind == "wide":
        s = R.decade_spread(cin, 1e-3, 1e3, seed)
    elif kind == "pow40":
        s = torch.ldexp(torch.ones(cin, dtype=torch.float64), torch.where(torch.arange(cin) % 2 == 0, 40.0, -40.0).double())
    elif kind == "dead":
        s[torch.arange(cin) % 7 == 3] = 0
    if kind in ("wide", "pow40"):
        w = w / s[None, :, None, None]
    if kind == "cols":
        c = R.decade_spread(cout, 1e-3, 1e3, seed + 1)
        w, b = w * c[:, None, None, None], b * c
    return w.float(), b.float(), s


def _input(shape, s, kind, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g, dtype=torch.float64) * s
    if kind == "spike":
        flat = x.view(-1, shape[-1])
        idx = torch.randint(0, flat.shape[0], (5,), generator=g)
        flat[idx] *= 1e3
    return x.float()


# ---------------- conv routes ----------------
# name, expected route, switches, (B, H, W, cin, cout, k, stride, pad), options, kind
CONV = [
    ("direct_halo_res", "direct", dict(PF_WINOGRAD="0", PF_HALO_FORCE="1"), (2, 33, 67, 160, 64, 3, 1, 1), dict(relu_in=True, res=True), "random"),
    ("direct_small_cin", "direct", dict(PF_WINOGRAD="0"), (2, 40, 52, 8, 32, 3, 1, 1), dict(act="relu", cin_real=5), "dead"),
    ("direct_stride2", "direct", dict(PF_WINOGRAD="0"), (1, 96, 100, 96, 192, 3, 2, 1), {}, "cols"),
    ("direct_rcu_views", "direct", dict(PF_WINOGRAD="0"), (2, 28, 37, 64, 64, 3, 1, 1), dict(relu_in=True, res=True, res2=True, xe=32, ye=16), "spike"),
    ("direct_n272_scale_inplace", "direct", dict(PF_WINOGRAD="0"), (2, 20, 27, 64, 272, 3, 1, 1), dict(scale=True, res=True, inplace=True, ye=32), "wide"),
    ("direct_1x1_cout1", "direct", dict(PF_CONV1X1_SPLIT3="0"), (2, 17, 23, 128, 1, 1, 1, 0), dict(act="softplus"), "spike"),
    ("direct_1x1_cout16", "direct", dict(PF_CONV1X1_SPLIT3="0"), (1, 33, 47, 128, 16, 1, 1, 0), dict(act="softplus"), "wide"),
    ("direct_1x1_cout80", "direct", dict(PF_CONV1X1_SPLIT3="0"), (1, 33, 47, 168, 80, 1, 1, 0), dict(act="gelu"), "cols"),
    ("direct_1x1_dead", "direct", dict(PF_CONV1X1_SPLIT3="0"), (1, 33, 47, 128, 64, 1, 1, 0), dict(res=True), "dead"),
    # the whole epilogue at once (bias, act, scale, res, res2) on a ragged last row fragment (1037 rows) and column group (84 = 5 x 16 + 4 channels)
    ("direct_1x1_whole_epi", "direct", dict(PF_CONV1X1_SPLIT3="0"), (1, 17, 61, 64, 84, 1, 1, 0), dict(act="gelu", res=True, res2=True, scale=True), "random"),
    ("s3_1x1_whole_epi", "s3_1x1", dict(PF_CONV1X1_SPLIT3="2"), (1, 17, 61, 64, 84, 1, 1, 0), dict(act="softplus", res=True, res2=True, scale=True), "random"),
    ("s3_1x1_ragged_epi", "s3_1x1", dict(PF_CONV1X1_SPLIT3="2"), (1, 17, 61, 256, 64, 1, 1, 0), dict(relu_in=True, res=True, res2=True, scale=True), "random"),
    ("s3_1x1_n80_views", "s3_1x1", dict(PF_CONV1X1_SPLIT3="2"), (2, 40, 52, 64, 80, 1, 1, 0), dict(act="gelu", xe=16, ye=8), "cols"),
    ("s3_1x1_n272_inplace", "s3_1x1", dict(PF_CONV1X1_SPLIT3="2"), (1, 37, 50, 96, 272, 1, 1, 0), dict(scale=True, res=True, inplace=True), "wide"),
    ("s3_1x1_n544", "s3_1x1", dict(PF_CONV1X1_SPLIT3="2"), (1, 56, 74, 1024, 544, 1, 1, 0), dict(act="relu"), "spike"),
    ("s3_1x1_n544_dead", "s3_1x1", dict(PF_CONV1X1_SPLIT3="2"), (1, 33, 47, 128, 544, 1, 1, 0), dict(res=True), "dead"),
    ("fused_64", "fused", dict(PF_WINOGRAD="4", PF_WINO_FUSED="2"), (2, 40, 52, 64, 64, 3, 1, 1), dict(act="relu", relu_in=True, res=True, res2=True), "random"),
    ("fused_128_wide", "fused", dict(PF_WINOGRAD="4", PF_WINO_FUSED="2"), (1, 48, 60, 128, 128, 3, 1, 1), dict(act="relu"), "wide"),
    ("fused_160_views", "fused", dict(PF_WINOGRAD="4", PF_WINO_FUSED="2"), (1, 30, 41, 160, 160, 3, 1, 1), dict(xe=32, ye=32), "cols"),
    ("fused_256_128", "fused", dict(PF_WINOGRAD="4", PF_WINO_FUSED="2"), (1, 40, 52, 256, 128, 3, 1, 1), dict(act="relu"), "spike"),
    ("fused_64_dead", "fused", dict(PF_WINOGRAD="4", PF_WINO_FUSED="2"), (2, 33, 45, 64, 96, 3, 1, 1), {}, "dead"),
    ("wino3_256", "wino3", dict(WINO), (2, 36, 44, 256, 256, 3, 1, 1), dict(act="relu"), "wide"),
    ("wino3_544", "wino3", dict(WINO, PF_WINO_F16X2="0", **T192), (1, 64, 80, 544, 544, 3, 1, 1), dict(act="relu", res=True), "cols"),
    ("wino3_256_spike", "wino3", dict(WINO), (2, 36, 44, 256, 256, 3, 1, 1), {}, "spike"),
    ("wino3_256_dead", "wino3", dict(WINO), (1, 36, 44, 256, 256, 3, 1, 1), {}, "dead"),
    ("wino3_256_random_windows", "wino3", dict(WINO, PF_WS_CAP_GB="0.005"), (2, 36, 44, 256, 256, 3, 1, 1), dict(act="relu"), "random"),
    ("wino3h_544", "wino3h", dict(WINO, **T192), (1, 64, 80, 544, 544, 3, 1, 1), dict(act="relu"), "random"),
    ("wino3h_544_windows", "wino3h", dict(WINO, PF_WS_CAP_GB="0.005", **T192), (1, 64, 80, 544, 544, 3, 1, 1), dict(res=True), "spike"),
    ("wino3h_1024_256", "wino3h", dict(WINO, **T192), (1, 40, 52, 1024, 256, 3, 1, 1), dict(act="relu"), "pow40"),
    ("wino3h_1024_256_windows", "wino3h", dict(WINO, PF_WS_CAP_GB="0.005", **T192), (1, 64, 80, 1024, 256, 3, 1, 1), {}, "wide"),
    ("wino3h_544_cols", "wino3h", dict(WINO, **T192), (1, 40, 52, 544, 544, 3, 1, 1), {}, "cols"),
    ("wino3h_544_dead", "wino3h", dict(WINO, **T192), (1, 40, 52, 544, 544, 3, 1, 1), dict(act="relu"), "dead"),
    ("wino_f32_544", "wino", dict(WINO, PF_WINO_SPLIT3="0"), (1, 40, 52, 544, 544, 3, 1, 1), dict(act="relu"), "random"),
    ("wino_f32_256_wide", "wino", dict(WINO, PF_WINO_SPLIT3="0"), (1, 36, 44, 256, 256, 3, 1, 1), {}, "wide"),
]


def _run_conv(x, pw, y, r1, r2, o, direct, fill_from_res):
    from patchfusion_amd.hip_ops import ops
    y.fill_(float("nan")) if not fill_from_res else y.copy_(r1)
    op_checks._flush_caches()
    ops.conv(x, pw, y, stride=o["stride"], pad=o["pad"], act=o.get("act"), relu_in=o.get("relu_in", False), res=y if fill_from_res else r1, res2=r2,
             _direct=direct)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,route,sw,shape,opts,kind", CONV, ids=[c[0] for c in CONV])
def test_conv_route_is_float32_grade(env, name, route, sw, shape, opts, kind):
    from patchfusion_amd import hip_ops
    from patchfusion_amd.hip_ops import HipOps
    B, H, W, cin, cout, k, stride, pad = shape
    env(**sw)
    seed = sum(map(ord, name))
    w, b, s = _operands(kind, cout, cin, k, seed, opts.get("cin_real"))
    sc = (0.5 + torch.rand(cout, generator=torch.Generator().manual_seed(seed + 2))) if opts.get("scale") else None
    pw = pk.pack_conv(w, b, dtype=torch.float32, scale=sc).to(DEV)
    xe, ye = opts.get("xe", 0), opts.get("ye", 0)
    xb = torch.full((B, H, W, cin + xe), float("nan"))
    xb[..., xe // 2: xe // 2 + cin] = _input((B, H, W, cin), s, kind, seed + 3)
    xb = xb.to(DEV)
    x = xb[..., xe // 2: xe // 2 + cin]
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    n = pw.cout
    g = torch.Generator().manual_seed(seed + 4)
    r1 = torch.randn(B, OH, OW, n, generator=g).to(DEV) if opts.get("res") else None
    r2 = torch.randn(B, OH, OW, n, generator=g).to(DEV) if opts.get("res2") else None
    yb = torch.empty((B, OH, OW, n + ye), device=DEV)
    y = yb[..., ye // 2: ye // 2 + n]
    o = dict(opts, stride=stride, pad=pad)
    inplace = bool(opts.get("inplace"))
    got = HipOps._conv_plan(x, pw, y, stride, pad, o.get("act"), o.get("relu_in", False), y if inplace else r1, r2, None)[0]
    assert got == route, (name, got)
    window = hip_ops.wino3_window(B, H, W, pw)[0] if route in ("wino3", "wino3h") else None
    if "PF_WS_CAP_GB" in sw:
        assert hip_ops.wino3_window(B, H, W, pw)[1] >= 2                   # several windows really ran
    pix = R.sample_pixels(B, OH, OW, n_random=192, seed=seed, window=window)
    ref, mag = R.conv_ref(x, w, pix, b, stride, pad, o.get("act"), o.get("relu_in", False), sc, r1, r2)
    ref, mag = ref[:, :cout], mag[:, :cout]

    def measure(direct):
        yb.fill_(float("nan"))
        _run_conv(x, pw, y, r1, r2, o, direct, inplace)
        if ye:
            assert torch.isnan(yb[..., :ye // 2]).all() and torch.isnan(yb[..., ye // 2 + n:]).all(), "channels outside the view were written"
        assert not torch.isnan(y).any(), "an output element was not written"
        return R.errors(R.gather_pixels(y, pix, cout), ref, mag)

    e = measure(None)
    wino = route in ("fused", "wino3", "wino3h", "wino")
    norm_cap, elem_cap = (R.NORM_CAP_WINO, R.ELEM_CAP_WINO) if wino else (R.NORM_CAP_GEMM, R.ELEM_CAP_GEMM)
    if route in ("wino3", "wino3h") or (route == "fused" and pw.wino_u is not None):
        # baseline: the f32 three-step route on the same operands, itself checked against the direct kernel
        os.environ.update(PF_WINO_SPLIT3="0", PF_WINO_FUSED="0")
        op_checks._switches_changed()
        assert HipOps._conv_plan(x, pw, y, stride, pad, o.get("act"), o.get("relu_in", False), r1, r2, None)[0] == "wino"
        base = measure(None)
        direct = measure(True)
        assert base[1] <= norm_cap and base[0] <= elem_cap, ("f32 three-step route", base, direct)
        extra = f" | direct elem {direct[0]:.2e} norm {direct[1]:.2e}"
    elif route == "s3_1x1":
        base, extra = measure(True), ""
    else:
        # direct, wino and the fused-only layers ARE float32 routes (no three-step form to compare with): the caps, next to the direct kernel
        base = None
        direct = measure(True) if route != "direct" else e
        extra = f" | direct elem {direct[0]:.2e} norm {direct[1]:.2e}"
    b = "" if base is None else f" | baseline elem {base[0]:.2e} norm {base[1]:.2e}"
    _log(f"{name:28s} {route:7s} {kind:6s} elem {e[0]:.2e} norm {e[1]:.2e}{b}{extra}")
    RAN.append((name, route))
    if base is None:
        assert e[0] <= elem_cap and (route == "direct" or e[1] <= norm_cap), (name, e)
    else:
        assert R.float32_grade(e, base, norm_cap, elem_cap), (name, e, base)


@pytest.mark.parametrize("s", [2, 4])
def test_transposed_conv_is_float32_grade(s):
    from patchfusion_amd.hip_ops import HipOps, ops
    cin = 96 if s == 2 else 48
    g = torch.Generator().manual_seed(s)
    w = (torch.randn(cin, cin, s, s, generator=g) / cin ** 0.5)
    b = torch.randn(cin, generator=g)
    pw = pk.pack_conv_transpose(w, b, dtype=torch.float32).to(DEV)
    x = torch.randn(2, 40 if s == 2 else 8, 52 if s == 2 else 11, cin, generator=g).to(DEV)
    B, H, W, _ = x.shape
    yb = torch.full((B, H * s, W * s, cin + 8), float("nan"), device=DEV)
    y = yb[..., 4:4 + cin]
    assert HipOps._conv_plan(x, pw, y, 1, 0, None, False, None, None, None)[0] == "direct"
    pix = R.sample_pixels(B, H * s, W * s, n_random=192, seed=s)
    ref, mag = R.conv_transpose_ref(x, w, pix, b)
    op_checks._flush_caches()
    ops.conv(x, pw, y)
    torch.cuda.synchronize()
    assert torch.isnan(yb[..., :4]).all() and torch.isnan(yb[..., 4 + cin:]).all() and not torch.isnan(y).any()
    e = R.errors(R.gather_pixels(y, pix, cin), ref, mag)
    _log(f"convT_s{s:<23d} direct  random elem {e[0]:.2e} norm {e[1]:.2e}")
    RAN.append((f"convT_s{s}", "direct"))
    assert e[1] <= R.NORM_CAP_GEMM and e[0] <= R.ELEM_CAP_GEMM, e


# ---------------- the two dispatch bugs ----------------

@pytest.mark.parametrize("route", ["wino3h", "wino3"])
def test_windows_on_disjoint_channel_slices_of_one_buffer(env, route):
    """x = buf[..., :C], y = buf[..., C:C + Cout] in several windows (the engine's concat buffers): used to be refused (PF_ERR_ARG) because the
    alias rule compared byte spans; a y that really overlaps x must still be refused before any launch"""
    from patchfusion_amd import hip_ops
    from patchfusion_amd.hip_ops import HipOps, ops
    sw = dict(WINO, PF_WS_CAP_GB="0.005", **T192)
    if route == "wino3":
        sw["PF_WINO_F16X2"] = "0"
    env(**sw)
    B, H, W, C = 1, 64, 80, 544
    w, b, s = _operands("random", C, C, 3, 5)
    pw = pk.pack_conv(w, b, dtype=torch.float32).to(DEV)
    buf = torch.full((B, H, W, 2 * C + 32), float("nan"))
    buf[..., :C] = _input((B, H, W, C), s, "random", 6)
    buf = buf.to(DEV)
    x, y = buf[..., :C], buf[..., C:2 * C]
    assert HipOps._conv_plan(x, pw, y, 1, 1, "relu", False, None, None, None)[0] == route
    assert hip_ops.wino3_window(B, H, W, pw)[1] >= 2
    pix = R.sample_pixels(B, H, W, n_random=128, seed=7, window=hip_ops.wino3_window(B, H, W, pw)[0])
    ref, mag = R.conv_ref(x, w, pix, b, 1, 1, "relu")
    op_checks._flush_caches()
    ops.conv(x, pw, y, pad=1, act="relu")
    torch.cuda.synchronize()
    assert torch.isnan(buf[..., 2 * C:]).all()
    assert torch.equal(buf[..., :C].cpu(), _input((B, H, W, C), s, "random", 6)), "x was overwritten"
    e = R.errors(R.gather_pixels(y, pix, C), ref, mag)
    _log(f"{'alias_disjoint_' + route:28s} {route:7s} random elem {e[0]:.2e} norm {e[1]:.2e}")
    assert e[1] <= R.NORM_CAP_WINO and e[0] <= R.ELEM_CAP_WINO, e
    before = buf.cpu()
    with pytest.raises(PfError):
        ops.conv(x, pw, buf[..., 32:32 + C], pad=1, act="relu")            # y overlaps x: refused before any launch
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu().nan_to_num(7.0), before.nan_to_num(7.0)), "a refused call wrote"


def test_unaligned_residual_does_not_take_s3_1x1(env):
    """a res view one float off a 16-byte boundary must not reach the split 1x1 kernel (float4 epilogue loads); the route it falls to computes it"""
    from patchfusion_amd.hip_ops import HipOps, ops
    env(PF_CONV1X1_SPLIT3="2")
    B, H, W, K, N = 1, 37, 50, 96, 128
    w, b, s = _operands("random", N, K, 1, 11)
    pw = pk.pack_conv(w, b, dtype=torch.float32).to(DEV)
    x = _input((B, H, W, K), s, "random", 12).to(DEV)
    rbuf = torch.randn(B, H, W, N + 4, generator=torch.Generator().manual_seed(13)).to(DEV)
    r_ok, r_off = rbuf[..., :N], rbuf[..., 1:1 + N]
    y = torch.full((B, H, W, N), float("nan"), device=DEV)
    assert HipOps._conv_plan(x, pw, y, 1, 0, None, False, r_ok, None, None)[0] == "s3_1x1"
    assert HipOps._conv_plan(x, pw, y, 1, 0, None, False, r_off, None, None)[0] == "direct"
    pix = R.sample_pixels(B, H, W, n_random=128, seed=14, tile=64)
    for res in (r_ok, r_off, r_ok):               # (the cached plan of the aligned call must not decide the route of the unaligned one)
        ref, mag = R.conv_ref(x, w, pix, b, res=res)
        y.fill_(float("nan"))
        op_checks._flush_caches()
        ops.conv(x, pw, y, res=res)
        torch.cuda.synchronize()
        e = R.errors(R.gather_pixels(y, pix, N), ref, mag)
        assert e[1] <= R.NORM_CAP_GEMM and e[0] <= R.ELEM_CAP_GEMM, e


# ---------------- linears: conv_split3 / conv_f16x2 ----------------
def _linear_layer(D, layer, kind, seed):
    K, N = {"qkv": (D, 3 * D), "proj": (D, D), "fc1": (D, 4 * D), "fc2": (4 * D, D)}[layer]
    w, b, s = _operands(kind, N, K, 1, seed)
    act = "gelu" if layer == "fc1" else None
    sc = (0.5 + torch.rand(N, generator=torch.Generator().manual_seed(seed))) if layer == "fc2" else None
    return w[:, :, 0, 0], b, s, act, sc


# D, layer, M, input layout (split3) | None (f16x2), output form, kind
LIN = [
    (384, "qkv", 1037, "rows", "f32", "random"), (768, "fc1", 77, "kmaj", "kmaj3", "cols"), (1024, "proj", 1037, "kmaj", "rows3", "spike"),
    (384, "fc2", 8 * 1037, "kmaj", "f32", "wide"), (768, "qkv", 1037, "rows", "rows3", "dead"),
    (384, "qkv", 1037, None, "rows3", "random"), (768, "fc1", 8 * 1037, None, "f16", "cols"), (1024, "fc2", 77, None, "f32", "wide"),
    (384, "fc1", 1037, None, "f16", "spike"), (768, "proj", 1037, None, "f32", "dead"), (1024, "qkv", 8 * 1037, None, "rows3", "random"),
]


def _decode(y, form, N, out_exp=None):
    if form == "f32":
        return y[:, :N].double().cpu()
    if form == "rows3":
        return y.double().sum(0)[:, :N].cpu()
    v = pk.kmajor_to_rows(y.cpu()).double().sum(0)[:, :N]
    return torch.ldexp(v, out_exp.cpu().double()[None, :N]) if form == "f16" else v


def _linear_case(D, layer, M, layout, form, kind, stress=None):
    from patchfusion_amd.hip_ops import ops
    seed = D + M + len(layer) * 7 + len(kind)
    w, b, s, act, sc = _linear_layer(D, layer, kind, seed)
    N, K = w.shape
    x = _input((M, K), s, kind, seed + 1)
    bound = x.double().abs().amax(0)
    if stress is not None:                        # channels peak 2^-12 .. 2^-17 below their static bound
        bound = torch.ldexp(bound, torch.randint(stress[0], stress[1] + 1, (K,), generator=torch.Generator().manual_seed(seed)).double())
    res = torch.randn(M, N, generator=torch.Generator().manual_seed(seed + 2)).to(DEV) if layer == "fc2" else None
    rows = R.sample_rows(M, n_random=192, seed=seed)
    ref, mag = R.linear_ref(x, w, b, act, sc, res, None, rows)
    xd = x.to(DEV)
    out_exp = None
    if form == "f32":
        y = torch.full((M, N + 4), float("nan"), device=DEV)
    elif form == "rows3":
        y = torch.full((3, M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    elif form == "kmaj3":
        y = torch.full((3, N // 32, M, 32), float("nan"), dtype=torch.bfloat16, device=DEV)
    else:
        y = torch.full((2, N // 32, M, 32), float("nan"), dtype=torch.float16, device=DEV)
        out_exp = pk.bound_exponents(pk.gelu_linear_bound(w, b, bound)).to(DEV)          # (fc1 only: the static bound of the engine)
    yv = y[:, :N] if form == "f32" else y
    if layout is None:
        pw = pk.pack_conv_f16x2(w, b, sc, bound).to(DEV)
        x2 = pk.rows_to_kmajor(torch.stack(pk.split_f16x2(torch.ldexp(x.double(), -pw.in_exp.cpu().double()[None, :]).float()))).contiguous().to(DEV)
        op_checks._flush_caches()
        ops.conv_f16x2(x2, pw, yv, act=act, res=res, out_exp=out_exp)
        what = "conv_f16x2"
    else:
        pw = pk.pack_conv_split3(w, b, scale=sc, kmajor=True).to(DEV)
        x3 = torch.stack(pk.split3(x))
        x3 = (pk.rows_to_kmajor(x3).contiguous() if layout == "kmaj" else x3).to(DEV)
        op_checks._flush_caches()
        ops.conv_split3(x3, pw, yv, act=act, res=res)
        what = "conv_split3"
    torch.cuda.synchronize()
    if form == "f32":
        assert torch.isnan(y[:, N:]).all(), "columns beyond N were written"
    got = _decode(y, form, N, out_exp)
    assert not torch.isnan(got).any(), "an output element was not written"
    e = R.errors(got[rows], ref, mag)
    # baseline: the f32-MFMA kernel on the same float32 operands
    pw32 = pk.pack_conv(w.view(N, K, 1, 1), b, dtype=torch.float32, scale=sc).to(DEV)
    y32 = torch.full((M, N), float("nan"), device=DEV)
    op_checks._flush_caches()
    ops.conv(xd, pw32, y32, act=act, res=res, _direct=True)
    torch.cuda.synchronize()
    base = R.errors(y32.cpu()[rows], ref, mag)
    return what, e, base


@pytest.mark.parametrize("D,layer,M,layout,form,kind", LIN, ids=[f"{'s3' if c[3] else 'f16'}_{c[1]}_D{c[0]}_M{c[2]}_{c[4]}_{c[5]}" for c in LIN])
def test_linear_route_is_float32_grade(D, layer, M, layout, form, kind):
    what, e, base = _linear_case(D, layer, M, layout, form, kind)
    tag = f"{what[5:]}_{layer}_D{D}_M{M}"
    _log(f"{tag:28s} {(layout or '') + '>' + form:12s} {kind:6s} elem {e[0]:.2e} norm {e[1]:.2e} | baseline elem {base[0]:.2e} norm {base[1]:.2e}")
    RAN.append((tag, f"{what}:{layout}:{form}"))
    assert R.float32_grade(e, base, R.NORM_CAP_GEMM, R.ELEM_CAP_GEMM), (tag, e, base)


@pytest.mark.parametrize("lo,hi", [(12, 14), (15, 17)])
def test_fc2_static_bound_slack(lo, hi):
    """fc2 inputs whose channels peak 2^-lo .. 2^-hi below the static bound of their exponents (packing.gelu_linear_bound; the slack
    profiles/r8_vit_f16x2_slack.md measured): the fp16x2 planes lose bits to fp16's subnormal range only below 2^-17"""
    what, e, base = _linear_case(384, "fc2", 1037, None, "f32", "random", stress=(lo, hi))
    _log(f"{f'f16x2_fc2_slack_{lo}_{hi}':28s} {'>f32':12s} random elem {e[0]:.2e} norm {e[1]:.2e} | baseline elem {base[0]:.2e} norm {base[1]:.2e}")
    assert R.float32_grade(e, base, R.NORM_CAP_GEMM, R.ELEM_CAP_GEMM), (e, base)


@pytest.mark.parametrize("tile", ["0", "1"], ids=["t192", "t160"])
def test_f16x2_whole_epilogue_is_float32_grade(monkeypatch, tile):
    """bias, softplus, scale, res and res2 at once through each fp16x2 linear tile (PF_F16_TILE forces it; the route is asserted), on the smallest
    shape with a ragged last row fragment (1037 rows) and column group (260 = 16 x 16 + 4 channels).  The two tiles share csrc/pf_epilogue.h, so each
    is judged against float64 here, not against the other."""
    import ctypes as C
    from patchfusion_amd import _lib
    from patchfusion_amd.hip_ops import HipOps, ops
    monkeypatch.setenv("PF_F16_TILE", tile)
    M, K, N, seed = 1037, 64, 260, 160 + int(tile)
    w, b, s = _operands("random", N, K, 1, seed)
    w = w[:, :, 0, 0]
    g = torch.Generator().manual_seed(seed + 2)
    sc = 0.5 + torch.rand(N, generator=g)
    x = _input((M, K), s, "random", seed + 1)
    res, res2 = torch.randn(M, N, generator=g).to(DEV), torch.randn(M, N, generator=g).to(DEV)
    rows = R.sample_rows(M, n_random=192, seed=seed)
    ref, mag = R.linear_ref(x, w, b, "softplus", sc, res, res2, rows)
    pw = pk.pack_conv_f16x2(w, b, sc, x.double().abs().amax(0)).to(DEV)
    x2 = pk.rows_to_kmajor(torch.stack(pk.split_f16x2(torch.ldexp(x.double(), -pw.in_exp.cpu().double()[None, :]).float()))).contiguous().to(DEV)
    y = torch.full((M, N + 4), float("nan"), device=DEV)
    p = HipOps._conv_f16x2_plan(x2, pw, y[:, :N], "softplus", res, res2, None)
    assert _lib.load().pf_gemm_f16x2_route(C.byref(p), 256) == (4 if tile == "1" else 3)          # PF_S3_ROUTE_TILE160 / PERSIST192
    op_checks._flush_caches()
    ops.conv_f16x2(x2, pw, y[:, :N], act="softplus", res=res, res2=res2)
    torch.cuda.synchronize()
    assert torch.isnan(y[:, N:]).all(), "columns beyond N were written"
    assert not torch.isnan(y[:, :N]).any(), "an output element was not written"
    e = R.errors(y[:, :N].double().cpu()[rows], ref, mag)
    # baseline: the f32-MFMA kernel on the same float32 operands
    pw32 = pk.pack_conv(w.reshape(N, K, 1, 1), b, dtype=torch.float32, scale=sc).to(DEV)
    y32 = torch.full((M, N), float("nan"), device=DEV)
    op_checks._flush_caches()
    ops.conv(x.to(DEV), pw32, y32, act="softplus", res=res, res2=res2, _direct=True)
    torch.cuda.synchronize()
    base = R.errors(y32.cpu()[rows], ref, mag)
    name = f"f16x2_whole_epi_{'t160' if tile == '1' else 't192'}"
    _log(f"{name:28s} {'>f32':12s} random elem {e[0]:.2e} norm {e[1]:.2e} | baseline elem {base[0]:.2e} norm {base[1]:.2e}")
    assert R.float32_grade(e, base, R.NORM_CAP_GEMM, R.ELEM_CAP_GEMM), (name, e, base)


# ---------------- producers ----------------
@pytest.mark.parametrize("tile,M,N", [(128, 1024, 128), (192, 1536, 192)])
def test_persistent_split3_below_eight_blocks_runs_the_one_tile_kernel(monkeypatch, tile, M, N):
    """the fallback of the persistent split-GEMM launchers (csrc/pf_launch.h, PF_GRID_FALLBACK): 8 tiles route to the persistent walk under
    PF_S3_PERSIST=2, PF_S3_GRID=4 leaves no grid of 8 blocks, and the launcher hands the call to the one 128 x 128 tile per block kernel -- the kernel
    PF_S3_PERSIST=0 runs, so the two outputs are the same bits, and float32-grade.  (PF_S3_TILE_NOW=128 in both calls: without it 8 tiles are below
    one round of tiles and both calls take the 64 x 128 kernel, never reaching the persistent launcher.)"""
    import ctypes as C
    from patchfusion_amd import _lib
    from patchfusion_amd.hip_ops import HipOps, ops
    K, seed = 96, 1000 + tile
    w, b, s = _operands("random", N, K, 1, seed)
    w = w[:, :, 0, 0]
    x = _input((M, K), s, "random", seed + 1)
    rows = R.sample_rows(M, n_random=192, seed=seed)
    ref, mag = R.linear_ref(x, w, b, None, None, None, None, rows)
    pw = pk.pack_conv_split3(w, b, scale=None, kmajor=True).to(DEV)
    x3 = torch.stack(pk.split3(x)).to(DEV)
    for k in ("PF_S3_PP", "PF_S3_ORDER"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PF_S3_TILE_NOW", "128")
    monkeypatch.setenv("PF_S3_T192", "2" if tile == 192 else "0")
    out = {}
    for persist, grid, route in (("2", "4", 3 if tile == 192 else 2), ("0", None, 1)):
        monkeypatch.setenv("PF_S3_PERSIST", persist)
        monkeypatch.setenv("PF_S3_GRID", grid) if grid else monkeypatch.delenv("PF_S3_GRID", raising=False)
        y = torch.full((M, N), float("nan"), device=DEV)
        assert _lib.load().pf_gemm_split3_route(C.byref(HipOps._conv_split3_plan(x3, pw, y, None, None, None)), 256) == route
        if grid:                                                   # the launcher's grid rule answers "fall back" for this call
            assert _lib.load().pf_persist_grid(256, 0, (M // tile) * (N // tile), 1 | 2 | 8) == 0
        op_checks._flush_caches()
        ops.conv_split3(x3, pw, y)
        torch.cuda.synchronize()
        out[persist] = y.cpu()
    assert not torch.isnan(out["2"]).any(), "an output element was not written"
    assert torch.equal(out["2"], out["0"])
    e = R.errors(out["2"].double()[rows], ref, mag)
    pw32 = pk.pack_conv(w.view(N, K, 1, 1), b, dtype=torch.float32).to(DEV)
    y32 = torch.full((M, N), float("nan"), device=DEV)
    op_checks._flush_caches()
    ops.conv(x.to(DEV), pw32, y32, _direct=True)
    torch.cuda.synchronize()
    base = R.errors(y32.cpu()[rows], ref, mag)
    _log(f"{f'split3_fallback_t{tile}':28s} {'rows>f32':12s} random elem {e[0]:.2e} norm {e[1]:.2e} | baseline elem {base[0]:.2e} norm {base[1]:.2e}")
    assert R.float32_grade(e, base, R.NORM_CAP_GEMM, R.ELEM_CAP_GEMM), (e, base)


@pytest.mark.parametrize("D", [384, 1024])
def test_layernorm_planes_against_float64(D):
    from patchfusion_amd.hip_ops import ops
    M = 1037
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(M, D, generator=g) * (0.5 + torch.rand(D, generator=g)) + torch.randn(D, generator=g)).float()
    gamma = (torch.randn(D, generator=g) * 0.5).float()
    beta = (torch.randn(D, generator=g) * 0.2).float()
    gamma[::17], beta[::34] = 0, 0                                         # zero-gamma channels, some with zero beta too
    xd64 = x.double()
    mu, var = xd64.mean(1, keepdim=True), xd64.var(1, unbiased=False, keepdim=True)
    xh = (xd64 - mu) / (var + 1e-6).sqrt()
    ref = xh * gamma.double() + beta.double()
    mag = ((xd64 - mu).abs() + mu.abs()) / (var + 1e-6).sqrt() * gamma.double().abs() + beta.double().abs()
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    y32 = torch.full((M, D), float("nan"), device=DEV)
    ops.layernorm(xd, y32, gd, bd, 1e-6)
    base = R.errors(y32, ref, mag)
    outs = {}
    for lay in ("rows", "kmaj"):
        y3 = torch.full((3, M, D) if lay == "rows" else (3, D // 32, M, 32), float("nan"), dtype=torch.bfloat16, device=DEV)
        op_checks._flush_caches()
        ops.layernorm_split3(xd, y3, gd, bd, 1e-6)
        torch.cuda.synchronize()
        outs[f"split3_{lay}"] = (y3.double().sum(0) if lay == "rows" else pk.kmajor_to_rows(y3.cpu()).double().sum(0)).cpu()
    in_exp = pk.bound_exponents(pk.layernorm_bound(gamma, beta)).to(DEV)
    y2 = torch.full((2, D // 32, M, 32), float("nan"), dtype=torch.float16, device=DEV)
    op_checks._flush_caches()
    ops.layernorm_f16x2(xd, y2, gd, bd, 1e-6, in_exp)
    torch.cuda.synchronize()
    outs["f16x2"] = torch.ldexp(pk.kmajor_to_rows(y2.cpu()).double().sum(0), in_exp.cpu().double()[None, :])
    for k, v in outs.items():
        assert not torch.isnan(v).any(), k
        assert bool((v[:, ::17][:, (beta[::17] == 0).tolist()] == 0).all()), f"{k}: a zero-gamma, zero-beta channel is not exactly zero"
        e = R.errors(v, ref, mag)
        _log(f"{'layernorm_' + k + f'_D{D}':28s} {'producer':7s} zgamma elem {e[0]:.2e} norm {e[1]:.2e} | baseline elem {base[0]:.2e} norm {base[1]:.2e}")
        RAN.append((f"layernorm_{k}", "producer"))
        assert R.float32_grade(e, base, R.NORM_CAP_GEMM, R.ELEM_CAP_GEMM), (k, e, base)


# ---------------- coverage ----------------
REQUIRED = {"s3_1x1", "fused", "wino3h", "wino3", "wino", "direct", "conv_split3:rows", "conv_split3:kmaj"} | \
    {f"conv_split3:{f}" for f in ("f32", "rows3", "kmaj3")} | {f"conv_f16x2:{f}" for f in ("f32", "rows3", "f16")}


def _covered(routes):
    out = set()
    for r in routes:
        parts = r.split(":")
        out.add(parts[0])
        if len(parts) == 3:
            out.update({f"{parts[0]}:{parts[1]}", f"{parts[0]}:{parts[2]}"} if parts[1] != "None" else {f"{parts[0]}:{parts[2]}"})
    return out


def test_route_coverage():
    """the matrix covers every float32 route of HipOps._conv_plan, both conv_split3 input layouts and every output form of conv_split3 / conv_f16x2
    -- as declared, and as run (each case asserts its own route)"""
    declared = {c[1] for c in CONV} | {f"{'conv_split3' if c[3] else 'conv_f16x2'}:{c[3]}:{c[4]}" for c in LIN}
    assert REQUIRED <= _covered(declared), sorted(REQUIRED - _covered(declared))
    if len(RAN) >= len(CONV) + len(LIN):          # the whole module ran
        assert REQUIRED <= _covered(r for _, r in RAN), sorted(REQUIRED - _covered(r for _, r in RAN))
