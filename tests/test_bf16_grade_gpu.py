"""pytest -m gpu: every bf16 conv / linear kernel of csrc/igemm.hip, the ping-pong linear and the small bf16 producers held to float64, element by
element (tests/f64_ref.py; the bar proved on the CPU in tests/test_bf16_grade_ref_cpu.py).

bf16 operands are exact, their products exact in float32, the accumulator is float32 and every epilogue works in float32 through bias, act, scale,
res and res2 and rounds ONCE, to nearest even, on the store.  So a bf16 output must be a float32-grade value rounded once and an out_f32 output
float32-grade:

    excess = max(0, |y - ref| - half_ulp_bf16(y)) / mag      (bf16 y; the plain |y - ref| / mag for an out_f32 y)

at most f64_ref.ELEM_CAP_GEMM (2.3e-6) and at most twice the element-wise error of the float32-MFMA kernel (pack_conv(dtype=float32),
_direct=True) on the same bf16-valued operands, that baseline floored at 4 * 2^-24 (f64_ref.bf16_grade).  All operands are built in float32 and
rounded to bf16 before the reference is taken (bias and scale stay float32, as the kernels read them): the bar measures the kernel, not the cast.

Each case pins its switches (restored by the fixture), fills y with NaN -- through a wider buffer where it is a view, whose outer channels must
stay NaN --, starts from cold caches, asserts the kernel variant that ran (hip_ops.last_conv_variant(): family, tile, shuffle, RELU_IN; the 'pp'
route through HipOps._conv_plan) and samples the borders, either side of every tile seam of the kernel under test and 192 random pixels / rows.
Shapes are the smallest at which each kernel's edges exist; every persistent shape also runs with more tiles than resident blocks.

Input kinds, rotated so that every family sees each: random; cols (output-column magnitudes 1e-3 .. 1e3 through weight rows and bias); spike
(pixels / rows at 1e3x); dead (all-zero input channels); wide (input-channel scales 1e-3 .. 1e3 with compensating weights, both rounded to bf16).

Measured on the MI355X (profiles/r13_bf16_grade.log; 242 cases in 5.4 s), worst excess per family, bf16 outputs / out_f32 outputs, against the 2.3e-6 cap
(the float32-MFMA baseline's element-wise error on the same operands: 3.7e-8 .. 7.3e-7):
  halo 4.9e-8 / 2.2e-7   persistent 3.2e-8 / 9.0e-8   big 3.7e-8 / 2.2e-7   generic 1.7e-8 / 2.3e-7   'pp' 1.7e-8 / 9.6e-8   shuffle 7.2e-9 / 8.5e-8
  (the same outputs with the storage rounding left in: 5.6e-4 .. 3.9e-3, the half ulp of bf16).  No kernel failed the bar; none was changed.
  bf16 LayerNorm: excess <= 1.9e-8 (float32 restatement 1.6e-7 .. 2.0e-7); im2col / tokens: within their counted bounds, met with equality at ties;
  unbiased bf16 attention: normwise 1.5e-3 .. 2.2e-3 against torch.bfloat16's 2.6e-3 .. 1.1e-2, largest element 0.09x .. 0.63x the comparator's."""
import os

import pytest
import torch

from patchfusion_amd import packing as pk
from tests import f64_image_ref as RI
from tests import f64_ref as R
from tests import op_checks
from tests.test_float32_grade_gpu import _input, _operands

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
KEYS = ("PF_WINOGRAD", "PF_HALO_FORCE", "PF_GEMM_PERSIST", "PF_IGEMM_CFG", "PF_IGEMM_NOSPLIT", "PF_BF16_PP", "PF_ATTN_QKV")
KINDS = ("random", "cols", "spike", "dead", "wide")
RAN = []                       # (case, variant name) of every case that ran: test_variant_coverage
LOG = []


@pytest.fixture
def env():
    old = {k: os.environ.get(k) for k in KEYS}

    def set_env(**kw):
        for k in KEYS:
            os.environ.pop(k, None)
        os.environ.update(PF_WINOGRAD="0", **kw)       # (read when a layer is packed: the float32 baseline needs no Winograd filters)
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


def _bf(t):
    """float32 values that bf16 holds exactly"""
    return t.to(BF).float()


# ---------------- variant codes (include/pf_hip.h pf_conv_last_variant) ----------------
def _code(family, shape, shuffle=0, relu=False):
    return family * 10 ** 8 + shape * 100 + shuffle * 10 + int(relu)


def _variant_name(v):
    family, shape, shuffle, relu = v // 10 ** 8, v // 100 % 10 ** 6, v // 10 % 10, v % 10
    r = "_relu" if relu else ""
    if shuffle:
        return f"shuffle{shuffle}"
    return {1: f"halo{shape}{r}", 2: f"persist{shape}", 3: f"big{r}", 4: f"generic{shape}"}.get(family, f"f32_{shape}")


PERSIST = {128128: (128, 128, 2, 2), 12896: (128, 96, 2, 2), 12864: (128, 64, 2, 2), 144128: (144, 128, 3, 2), 14464: (144, 64, 3, 2),
           256128: (256, 128, 4, 2)}           # PF_GEMM_PERSIST code -> BM, BN, WM, WN (csrc/igemm.hip dispatch)
GENERIC = {1: (128, 128), 2: (128, 96), 3: (128, 64), 4: (256, 32), 5: (256, 16)}       # PF_IGEMM_CFG -> BM, BN (launch_generic)


def _persist_slots(code):
    """resident blocks of a persistent shape: PersistCfg of csrc/igemm.hip restated (LDS bytes of the double-buffered A and B tiles, rows padded to
    the 8 WM WN rows one load pass covers; blocks per CU from the 160 KiB of LDS; 256 CUs)"""
    bm, bn, wm, wn = PERSIST[code]
    rp = 8 * wm * wn
    smem = 2 * (-(-bm // rp) * rp + -(-bn // rp) * rp) * 128
    return 256 * ((160 * 1024) // smem)


def _persist_multi_cout(code, M):
    """the smallest whole number of channel tiles with more tiles than resident blocks and a ragged last round (launch_persist: grid = min(tiles, slots),
    block b walks tiles b, b + grid, ...)"""
    bm, bn, _, _ = PERSIST[code]
    mt, slots = -(-M // bm), _persist_slots(code)
    nt = 1
    while mt * nt <= slots or (mt * nt) % slots == 0:
        nt += 1
    return nt * bn, mt * nt, slots


# ---------------- samplers ----------------
def _flat_to_pix(rows, OH, OW):
    return torch.stack([rows // (OH * OW), rows // OW % OH, rows % OW], 1)


def _gemm_pixels(B, OH, OW, bm, seed):
    """output pixels of a kernel that tiles the FLAT pixel index by bm rows: f64_ref.sample_rows (0, 1, multiples of 64 .. 256 and their neighbours, the
    ragged tail, 192 random rows), either side of every bm seam, and the image borders / corners (zero padding of the 3x3 cases)"""
    M = B * OH * OW
    rows = set(R.sample_rows(M, n_random=192, seed=seed).tolist())
    for m in range(bm, M, bm):
        rows.update((m - 1, m))
    pix = set(map(tuple, _flat_to_pix(torch.tensor(sorted(rows)), OH, OW).tolist()))
    pix.update(map(tuple, R.sample_pixels(B, OH, OW, n_random=0, tile=4).tolist()))
    return torch.tensor(sorted(pix), dtype=torch.long)


def _halo_pixels(B, H, W, seed):
    """the halo kernel's tiles are 16 rows x 32 columns of one image: the borders, either side of every 16-row and every 32-column seam (a wrong halo
    tap shows there), and 192 random pixels"""
    ys = sorted({0, 1, H - 2, H - 1} | {y for s in range(16, H, 16) for y in (s - 1, s)})
    xs = sorted({0, 1, W - 2, W - 1} | {x for s in range(32, W, 32) for x in (s - 1, s)})
    pix = {(b, y, x) for b in {0, B - 1} for y in ys for x in xs}
    pix.update(map(tuple, R.sample_pixels(B, H, W, n_random=192, seed=seed, tile=16).tolist()))
    return torch.tensor(sorted(pix), dtype=torch.long)


# ---------------- one conv / linear case ----------------
def _conv_case(env, name, family, sw, shape, opts, kind, expect, pixels):
    """runs the bf16 kernel and the float32-MFMA baseline on the same bf16-valued operands; expect = variant code, or 'pp' (the route)"""
    from patchfusion_amd import hip_ops
    from patchfusion_amd.hip_ops import HipOps, ops
    B, H, W, cin, cout, k, stride, pad = shape
    env(**sw)
    seed = sum(map(ord, name))
    w, b, s = _operands(kind, cout, cin, k, seed, opts.get("cin_real"))
    w = _bf(w)
    sc = (0.5 + torch.rand(cout, generator=torch.Generator().manual_seed(seed + 2))) if opts.get("scale") else None
    pw = pk.pack_conv(w, b, dtype=BF, scale=sc).to(DEV)
    pw32 = pk.pack_conv(w, b, dtype=torch.float32, scale=sc).to(DEV)
    n = pw.cout
    assert n == cout and torch.equal(pw.w[:cout, :k * k * cin].float().cpu().view(cout, k, k, cin).permute(0, 3, 1, 2), w), "the packed weights are not the operands"
    act, relu_in, out_f32, inplace = opts.get("act"), bool(opts.get("relu_in")), bool(opts.get("out_f32")), bool(opts.get("inplace"))
    xe, ye = opts.get("xe", 0), opts.get("ye", 0)
    xv = _bf(_input((B, H, W, cin), s, kind, seed + 3))
    xb = torch.full((B, H, W, cin + xe), float("nan"), dtype=BF)
    xb[..., xe // 2: xe // 2 + cin] = xv.to(BF)
    xb = xb.to(DEV)
    x = xb[..., xe // 2: xe // 2 + cin]
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    g = torch.Generator().manual_seed(seed + 4)
    r1 = torch.randn(B, OH, OW, n, generator=g).to(BF).to(DEV) if opts.get("res") else None
    r2 = torch.randn(B, OH, OW, n, generator=g).to(BF).to(DEV) if opts.get("res2") else None
    assert not (inplace and out_f32)
    yb = torch.empty((B, OH, OW, n + ye), dtype=torch.float32 if out_f32 else BF, device=DEV)
    y = yb[..., ye // 2: ye // 2 + n]
    route = HipOps._conv_plan(x, pw, y, stride, pad, act, relu_in, y if inplace else r1, r2, None)[0]
    assert route == ("pp" if expect == "pp" else "direct"), (name, route)
    pix = pixels(B, OH, OW, seed)
    ref, mag = R.conv_ref(x, w, pix, b, stride, pad, act, relu_in, sc, r1, r2)

    def run(xx, pww, ybuf, yv, ra, rb, direct):
        ybuf.fill_(float("nan"))
        if inplace:
            yv.copy_(ra)
        op_checks._flush_caches()
        ops.conv(xx, pww, yv, stride=stride, pad=pad, act=act, relu_in=relu_in, res=yv if inplace else ra, res2=rb, _direct=direct)
        torch.cuda.synchronize()
        if ybuf.shape[-1] > n:
            assert torch.isnan(ybuf[..., :ye // 2]).all() and torch.isnan(ybuf[..., ye // 2 + n:]).all(), "channels outside the view were written"
        assert not torch.isnan(yv).any(), "an output element was not written"
        return R.gather_pixels(yv, pix, cout)

    got = run(x, pw, yb, y, r1, r2, None)
    if expect == "pp":
        vname = "pp"
    else:
        v = hip_ops.last_conv_variant()
        assert v == expect, (name, v, expect)
        vname = _variant_name(v)
    e = R.bf16_excess(got, ref, mag)
    raw = R.errors(got, ref, mag)
    # baseline: the float32-MFMA kernel on the same values (no tile forced)
    env()
    y32 = torch.empty((B, OH, OW, n), dtype=torch.float32, device=DEV)
    f = lambda t: None if t is None else t.float()
    base = R.errors(run(x.float().contiguous(), pw32, y32, y32, f(r1), f(r2), True), ref, mag)
    assert hip_ops.last_conv_variant() // 10 ** 8 == 5
    M = B * OH * OW
    _log(f"{name:34s} {vname:18s} {kind:6s} M {M:5d} K {k * k * cin:4d} N {cout:4d} {'f32' if out_f32 else 'bf16'} excess {e[0]:.2e} (raw elem {raw[0]:.2e}) | "
         f"baseline elem {base[0]:.2e}")
    RAN.append((name, vname, family, e[0]))
    assert R.bf16_grade(e, base), (name, e, base)


def _epi(i):
    """the epilogues, spread over the cases of a family"""
    return [dict(scale=True, res=True, inplace=True), dict(act="gelu"), dict(relu_in=True, res=True, res2=True), dict(ye=16), dict(out_f32=True, act="relu"),
            dict(res=True, xe=16), dict(act="relu", scale=True)][i % 7]


# the whole epilogue at once -- bias, softplus, scale, res, res2 -- on the smallest shape of a kernel with a ragged last row fragment (rows not a multiple
# of 16) and a ragged last column group (Cout a multiple of 4, not of 16): one case per kernel instantiation that shares csrc/pf_epilogue.h
WHOLE_EPI = dict(act="softplus", scale=True, res=True, res2=True)


# ---------------- halo kernels ----------------
def _halo_cases():
    """every variant and channel count x RELU_IN x both maps (each overhangs the 16 x 32 tile both ways) x Cin 32 / 96 / 160 (one chunk, a whole number
    of chunks, an odd chunk tail per tap); epilogues and input kinds rotate"""
    out, i = [], 0
    for shape, couts in ((121, (32, 20)), (122, (64, 48)), (242, (224,)), (243, (160, 544))):
        for cout in couts:
            for relu in (False, True):
                for B, H, W in ((2, 21, 45), (1, 33, 67)):
                    for cin in (32, 96, 160):
                        o = dict(_epi(i), relu_in=relu)
                        out.append((f"halo{shape}_n{cout}_c{cin}_{H}x{W}{'_relu' if relu else ''}", (B, H, W, cin, cout, 3, 1, 1), o, KINDS[i % 5],
                                    _code(1, shape, 0, relu)))
                        i += 1
    return out


HALO = _halo_cases() + [(f"halo{shape}_n{cout}_c32_21x45_whole_epi", (2, 21, 45, 32, cout, 3, 1, 1), WHOLE_EPI, "random", _code(1, shape, 0, False))
                        for shape, cout in ((121, 20), (122, 36), (242, 228), (243, 164))]


@pytest.mark.parametrize("name,shape,opts,kind,expect", HALO, ids=[c[0] for c in HALO])
def test_halo_kernel_is_bf16_grade(env, name, shape, opts, kind, expect):
    _conv_case(env, name, "halo", dict(PF_HALO_FORCE="1"), shape, opts, kind, expect, lambda B, OH, OW, seed: _halo_pixels(B, OH, OW, seed))


# ---------------- persistent GEMM ----------------
def _persist_cases():
    """per shape: one tile per block at M = 1037 (ragged against 128, 144 and 256) x Cin 128 / 192 (an even and an odd number of 64-wide chunks) x
    Cout 80 / 160 (a channel tail inside a tile), and several tiles per block at M = 8 x 1037, Cin 128"""
    out, i = [], 0
    for code in PERSIST:
        for cin in (128, 192):
            for cout in (80, 160):
                out.append((f"persist{code}_k{cin}_n{cout}", code, 1037, cin, cout, _epi(i), KINDS[i % 5], False))
                i += 1
        M = 8 * 1037
        cout, tiles, slots = _persist_multi_cout(code, M)
        out.append((f"persist{code}_multi_n{cout}", code, M, 128, cout, _epi(i), KINDS[i % 5], True))
        i += 1
    return out


PERSIST_CASES = _persist_cases() + [(f"persist{code}_k128_n84_whole_epi", code, 1037, 128, 84, WHOLE_EPI, "random", False) for code in PERSIST]


def test_persist_arithmetic_restated():
    """PersistCfg restated in Python gives the resident-block counts the kernel comments state: 128 x 64 runs three blocks per CU, 256 x 128 one"""
    assert [_persist_slots(c) for c in PERSIST] == [512, 512, 768, 512, 512, 256]
    assert _persist_multi_cout(12864, 8 * 1037) == (768, 780, 768)


@pytest.mark.parametrize("name,code,M,cin,cout,opts,kind,multi", PERSIST_CASES, ids=[c[0] for c in PERSIST_CASES])
def test_persistent_gemm_is_bf16_grade(env, name, code, M, cin, cout, opts, kind, multi):
    bm, bn, _, _ = PERSIST[code]
    if multi:
        tiles, slots = -(-M // bm) * -(-cout // bn), _persist_slots(code)
        assert tiles > slots and tiles % slots != 0, (tiles, slots)          # some blocks walk two tiles, some one
    relu = bool(opts.get("relu_in"))
    _conv_case(env, name, "persist", dict(PF_GEMM_PERSIST=str(code)), (1, 1, M, cin, cout, 1, 1, 0), opts, kind, _code(2, bm * 1000 + bn, 0, relu),
               lambda B, OH, OW, seed: _gemm_pixels(B, OH, OW, bm, seed))


# ---------------- the eight-wave big kernel and the generic four-wave kernel ----------------
def _map(M, stride):
    """(B, H, W) of the input whose output has M = 270 (2 x 9 x 15: one full 256-pixel tile + 14) or 1037 (17 x 61) pixels"""
    B, OH, OW = (2, 9, 15) if M == 270 else (1, 17, 61)
    return (B, OH, OW) if stride == 1 else (B, 2 * OH, 2 * OW)


def _big_cases():
    """K chunks of 64 through the ring of three: 1x1 Cin 64 .. 256 = 1 .. 4 chunks, 3x3 Cin 32 = 288 = 5 chunks (prologue, wrap, drain), the 3x3 at stride
    1 and 2; x M 270 / 1037 x Cout 96 / 144 / 272; RELU_IN, the epilogues (bf16 and out_f32 outputs among them) and the input kinds rotate"""
    out, i = [], 0
    for k, cin, stride in ((1, 64, 1), (1, 128, 1), (1, 192, 1), (1, 256, 1), (3, 32, 1), (3, 32, 2)):
        for M in (270, 1037):
            for cout in (96, 144, 272):
                o = dict(_epi(i), relu_in=bool(i % 2))
                out.append((f"big_{k}x{k}{'_s2' if stride == 2 else ''}_c{cin}_m{M}_n{cout}{'_relu' if i % 2 else ''}",
                            _map(M, stride) + (cin, cout, k, stride, k // 2), o, KINDS[i % 5]))
                i += 1
    return out


BIG = _big_cases() + [("big_1x1_c64_m1037_n100_whole_epi", _map(1037, 1) + (64, 100, 1, 1, 0), WHOLE_EPI, "random")]


@pytest.mark.parametrize("name,shape,opts,kind", BIG, ids=[c[0] for c in BIG])
def test_big_kernel_is_bf16_grade(env, name, shape, opts, kind):
    _conv_case(env, name, "big", dict(PF_IGEMM_CFG="0", PF_GEMM_PERSIST="0"), shape, opts, kind, _code(3, 256128, 0, bool(opts.get("relu_in"))),
               lambda B, OH, OW, seed: _gemm_pixels(B, OH, OW, 256, seed))


def _generic_cases():
    """PF_IGEMM_CFG 1 .. 5 (name, cfg, shape, options, kind), each tile with a channel count that leaves a tail: x M 270 / 1037 x 3x3 with Cin 8 (5 real
    channels), 32, 160 and 1x1 with Cin 64, 192; plus one stride-2 and one softplus out_f32 case"""
    out, i = [], 0
    for cfg, couts in ((1, (144,)), (2, (112,)), (3, (80,)), (4, (36,)), (5, (20, 4))):
        for cout in couts:
            for M in (270, 1037):
                for k, cin, real in ((3, 8, 5), (3, 32, None), (3, 160, None), (1, 64, None), (1, 192, None)):
                    o = dict(_epi(i), relu_in=bool(i % 2), cin_real=real)
                    out.append((f"gen{cfg}_{k}x{k}_c{cin}_m{M}_n{cout}", cfg, _map(M, 1) + (cin, cout, k, 1, k // 2), o, KINDS[i % 5]))
                    i += 1
    out.append(("gen3_3x3_s2_c32_m1037_n80", 3, _map(1037, 2) + (32, 80, 3, 2, 1), dict(ye=16), "random"))
    out.append(("gen4_1x1_c192_m270_n36_softplus_f32", 4, _map(270, 1) + (192, 36, 1, 1, 0), dict(act="softplus", out_f32=True), "spike"))
    return out


GEN = _generic_cases() + [(f"gen{cfg}_1x1_c64_m270_n{cout}_whole_epi", cfg, _map(270, 1) + (64, cout, 1, 1, 0), WHOLE_EPI, "random")
                          for cfg, cout in ((1, 148), (2, 116), (3, 84), (4, 36), (5, 20))]


@pytest.mark.parametrize("name,cfg,shape,opts,kind", GEN, ids=[c[0] for c in GEN])
def test_generic_kernel_is_bf16_grade(env, name, cfg, shape, opts, kind):
    bm, bn = GENERIC[cfg]
    _conv_case(env, name, "generic", dict(PF_IGEMM_CFG=str(cfg), PF_GEMM_PERSIST="0"), shape, opts, kind, _code(4, bm * 1000 + bn, 0, bool(opts.get("relu_in"))),
               lambda B, OH, OW, seed: _gemm_pixels(B, OH, OW, bm, seed))


# ---------------- the ping-pong linear (route 'pp') ----------------
PP = [
    ("pp_m2049_k512_n512_inplace", (1, 1, 2049, 512, 512, 1, 1, 0), dict(scale=True, res=True, inplace=True), "random"),
    ("pp_m2500_k576_n516_res2", (1, 1, 2500, 576, 516, 1, 1, 0), dict(act="relu", res=True, res2=True), "cols"),
    ("pp_m2049_k576_n516_gelu", (1, 1, 2049, 576, 516, 1, 1, 0), dict(act="gelu"), "spike"),
    ("pp_m2500_k512_n512_f32_views", (1, 50, 50, 512, 512, 1, 1, 0), dict(out_f32=True, xe=16, ye=24), "dead"),
    ("pp_m2049_k512_n516_wide", (1, 1, 2049, 512, 516, 1, 1, 0), dict(res=True), "wide"),
    ("pp_m2049_k512_n516_whole_epi", (1, 1, 2049, 512, 516, 1, 1, 0), WHOLE_EPI, "random"),
]


@pytest.mark.parametrize("name,shape,opts,kind", PP, ids=[c[0] for c in PP])
def test_pingpong_linear_is_bf16_grade(env, name, shape, opts, kind):
    _conv_case(env, name, "pp", dict(PF_BF16_PP="1"), shape, opts, kind, "pp", lambda B, OH, OW, seed: _gemm_pixels(B, OH, OW, 256, seed))


# ---------------- transposed conv: the shuffle epilogue ----------------
@pytest.mark.parametrize("out_f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("s", [2, 4])
def test_transposed_conv_is_bf16_grade(env, s, out_f32):
    from patchfusion_amd import hip_ops
    from patchfusion_amd.hip_ops import HipOps, ops
    env()
    cin = 96 if s == 2 else 48
    g = torch.Generator().manual_seed(s)
    w = _bf(torch.randn(cin, cin, s, s, generator=g) / cin ** 0.5)
    b = torch.randn(cin, generator=g)
    xv = _bf(torch.randn(2, 40 if s == 2 else 8, 52 if s == 2 else 11, cin, generator=g))
    B, H, W, _ = xv.shape
    pix = R.sample_pixels(B, H * s, W * s, n_random=192, seed=s, tile=s)
    ref, mag = R.conv_transpose_ref(xv, w, pix, b)
    res = {}
    for dt in (BF, torch.float32):
        pw = pk.pack_conv_transpose(w, b, dtype=dt).to(DEV)
        x = xv.to(dt).to(DEV)
        yb = torch.full((B, H * s, W * s, cin + 8), float("nan"), dtype=torch.float32 if (out_f32 or dt != BF) else BF, device=DEV)
        y = yb[..., 4:4 + cin]
        assert HipOps._conv_plan(x, pw, y, 1, 0, None, False, None, None, None)[0] == "direct"
        op_checks._flush_caches()
        ops.conv(x, pw, y, _direct=True if dt != BF else None)
        torch.cuda.synchronize()
        v = hip_ops.last_conv_variant()
        assert v // 10 % 10 == s and (v // 10 ** 8 in (3, 4) if dt == BF else v // 10 ** 8 == 5), v
        assert torch.isnan(yb[..., :4]).all() and torch.isnan(yb[..., 4 + cin:]).all() and not torch.isnan(y).any()
        res[dt] = R.gather_pixels(y, pix, cin), v
    e, base = R.bf16_excess(res[BF][0], ref, mag), R.errors(res[torch.float32][0], ref, mag)
    name = f"convT_s{s}_{'f32' if out_f32 else 'bf16'}"
    _log(f"{name:34s} {_variant_name(res[BF][1]):18s} random M {B * H * W:5d} K {cin:4d} N {s * s * cin:4d} {'f32' if out_f32 else 'bf16'} excess {e[0]:.2e} "
         f"(raw elem {R.errors(res[BF][0], ref, mag)[0]:.2e}) | baseline elem {base[0]:.2e}   [tile family {res[BF][1] // 10 ** 8}]")
    RAN.append((name, _variant_name(res[BF][1]), "shuffle", e[0]))
    assert R.bf16_grade(e, base), (name, e, base)


# ---------------- coverage ----------------
REQUIRED = {f"halo{s}{r}" for s in (121, 122, 242, 243) for r in ("", "_relu")} | {f"persist{bm * 1000 + bn}" for bm, bn, _, _ in PERSIST.values()} | \
    {"big", "big_relu"} | {f"generic{bm * 1000 + bn}" for bm, bn in GENERIC.values()} | {"pp", "shuffle2", "shuffle4"}
N_CASES = len(HALO) + len(PERSIST_CASES) + len(BIG) + len(GEN) + len(PP) + 4


def test_variant_coverage():
    """the matrix launches every bf16 variant of csrc/igemm.hip and the 'pp' route -- as declared (the variant code every case asserts), and, when the whole
    module ran, as observed from hip_ops.last_conv_variant(); every persistent shape ran with more tiles than resident blocks"""
    declared = {_variant_name(c[4]) for c in HALO} | {_variant_name(_code(2, PERSIST[c[1]][0] * 1000 + PERSIST[c[1]][1])) for c in PERSIST_CASES} | \
        {_variant_name(_code(3, 256128, 0, bool(c[2].get("relu_in")))) for c in BIG} | {_variant_name(_code(4, GENERIC[c[1]][0] * 1000 + GENERIC[c[1]][1])) for c in GEN} | \
        {"pp", "shuffle2", "shuffle4"}
    assert len(REQUIRED) == 8 + 6 + 2 + 5 + 3
    assert REQUIRED <= declared, sorted(REQUIRED - declared)
    assert {c[1] for c in PERSIST_CASES if c[7]} == set(PERSIST)
    if len(RAN) >= N_CASES:                       # the whole module ran
        seen = {v for _, v, _, _ in RAN}
        assert REQUIRED <= seen, sorted(REQUIRED - seen)
        assert {f"persist{PERSIST[c[1]][0] * 1000 + PERSIST[c[1]][1]}" for c in PERSIST_CASES if c[7]} <= {v for n, v, _, _ in RAN if "_multi_" in n}
        for fam in ("halo", "persist", "big", "generic", "pp", "shuffle"):
            _log(f"worst excess {fam:8s} {max(e for _, _, f, e in RAN if f == fam):.2e}")


# ---------------- the small bf16 producers ----------------
@pytest.mark.parametrize("remap", [False, True], ids=["plain", "remap"])
@pytest.mark.parametrize("D", [32, 64, 384, 1024])
def test_layernorm_bf16_against_float64(D, remap):
    """layernorm_kernel<bf16_t>: 2 x 89 rows, plain and with the row remap (rows 1 .. 88 of each batch -> 88 rows out); the excess over the one storage
    rounding at most twice the element-wise error of the float32 restatement (tests/fake_ops.py) on the same bf16 rows, that floored at 4 * 2^-24;
    a zero-gamma channel is bf16(beta) exactly"""
    from patchfusion_amd.hip_ops import ops
    from tests.fake_ops import ops as ref_ops
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(2 * 89, D, generator=g) * (0.5 + torch.rand(D, generator=g)) + torch.randn(D, generator=g)).to(BF)
    gamma, beta = torch.randn(D, generator=g) * 0.5, torch.randn(D, generator=g) * 0.2
    gamma[::7] = 0
    kw = dict(batches=2, in_rows_per_batch=89, in_row_offset=1, out_rows_per_batch=88) if remap else {}
    xs = x.double().view(2, 89, D)[:, 1:].reshape(-1, D) if remap else x.double()
    mu, var = xs.mean(1, keepdim=True), xs.var(1, unbiased=False, keepdim=True)
    rstd = 1.0 / (var + float(torch.tensor(1e-6, dtype=torch.float32))).sqrt()
    ref = (xs - mu) * rstd * gamma.double() + beta.double()
    mag = ((xs - mu).abs() + mu.abs()) * rstd * gamma.double().abs() + beta.double().abs()
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    rows = xs.shape[0]
    yb = torch.full((rows + 2, D), float("nan"), dtype=BF, device=DEV)
    y = yb[1:-1]
    op_checks._flush_caches()
    ops.layernorm(xd, y, gd, bd, 1e-6, **kw)
    y32 = torch.full((rows, D), float("nan"), device=DEV)
    ref_ops.layernorm(xd, y32, gd, bd, 1e-6, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(yb[0]).all() and torch.isnan(yb[-1]).all() and not torch.isnan(y).any()
    assert torch.equal(y[:, ::7].cpu(), beta[::7].to(BF).expand(rows, -1)), "a zero-gamma channel is not bf16(beta)"
    e, base = R.bf16_excess(y, ref, mag), R.errors(y32, ref, mag)
    _log(f"{f'layernorm_bf16_D{D}' + ('_remap' if remap else ''):34s} {'producer':18s} zgamma rows {rows} excess {e[0]:.2e} (raw elem {R.errors(y, ref, mag)[0]:.2e}) | "
         f"restatement elem {base[0]:.2e}")
    assert e[0] <= 2 * max(base[0], R.BASE_FLOOR), (e, base)


def test_patch_im2col_and_assemble_tokens_bf16_counted():
    """Each output is one rounding to bf16 of a float32 value with a countable path (f64_image_ref.counted_bar, bf16_out):
    pf_patch_im2col: v = (px - mean[c]) / std[c] on float32 constants -- one subtraction, one division: k = 2, mag = (|px| + |mean|) / std; the columns
    588 .. ld - 1 are exactly zero.  pf_assemble_tokens: cls[d] + pos[0, d] or emb + pos[1 + t, d] -- one addition: k = 1, mag = |a| + |pos|."""
    from patchfusion_amd.hip_ops import ops
    g = torch.Generator().manual_seed(1)
    img = torch.rand(2, 3, 112, 154, generator=g)
    img[0, :, :14, :14] = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1) + 1e-3 * torch.randn(3, 14, 14, generator=g)      # cancellation in px - mean
    col = torch.full((2 * 88, 592), float("nan"), dtype=BF, device=DEV)
    ops.patch_im2col(img.to(DEV), col)
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32).double().view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32).double().view(1, 3, 1, 1)
    im = lambda t: t.view(2, 3, 8, 14, 11, 14).permute(0, 2, 4, 3, 5, 1).reshape(2 * 88, 588)
    ref, mag = im((img.double() - mean) / std), im((img.double().abs() + mean) / std)
    torch.cuda.synchronize()
    assert bool((col[:, 588:] == 0).all())
    ok, worst = RI.counted_bar(col[:, :588], ref, mag, 2, bf16_out=True)
    _log(f"{'patch_im2col_bf16':34s} {'producer':18s} counted k 2: worst |y - ref| / bound {worst:.3f}")
    assert ok, worst
    S, D = 89, 384
    cls, pos = torch.randn(D, generator=g), torch.randn(S, D, generator=g)
    emb = (torch.randn(2 * (S - 1), D, generator=g) * 3).to(BF)
    tok = torch.full((2, S, D), float("nan"), dtype=BF, device=DEV)
    ops.assemble_tokens(emb.to(DEV), tok, cls.to(DEV), pos.to(DEV))
    torch.cuda.synchronize()
    a = torch.cat([cls.double().expand(2, 1, D), emb.double().view(2, S - 1, D)], 1)
    ok, worst = RI.counted_bar(tok, a + pos.double(), a.abs() + pos.double().abs(), 1, bf16_out=True)
    _log(f"{'assemble_tokens_bf16':34s} {'producer':18s} counted k 1: worst |y - ref| / bound {worst:.3f}")
    assert ok, worst


# ---------------- the unbiased bf16 attention ----------------
def _stats(got, ref64):
    """(max, p99.9, normwise) error against the float64 reference (tests/test_midas_core_bf16_gpu.py)"""
    d = (got.double() - ref64).abs().flatten()
    return float(d.max()), float(d.kthvalue(max(1, int(0.999 * d.numel()))).values), float(d.norm() / ref64.norm())


ATTN = [(1, 13, 2, 1.0, False), (3, 64, 4, 1.0, False), (2, 129, 3, 3.0, False), (1, 300, 6, 1.0, True), (1, 1037, 2, 1.0, False)]


@pytest.mark.parametrize("qkv_switch", [None, "0"], ids=["default", "PF_ATTN_QKV0"])
@pytest.mark.parametrize("B,S,heads,scale,hot_key", ATTN, ids=[f"B{c[0]}_S{c[1]}_h{c[2]}" + ("_hotkey" if c[4] else "") for c in ATTN])
def test_unbiased_bf16_attention_against_float64(env, B, S, heads, scale, hot_key, qkv_switch):
    """ops.vit_attention on bf16 qkv (pf_qkv_split + pf_vit_attention; PF_ATTN_QKV only moves the float32 mode, both settings run) against float64 on
    the same bf16 operands, by the bar of the biased kernel (tests/test_midas_core_bf16_gpu.py): torch.bfloat16 on the same operands is the comparator,
    normwise and 99.9th-percentile error at most 2x its, the single largest at most 4x.  hot_key: one key 8x above the rest late in the sequence."""
    from patchfusion_amd.hip_ops import ops
    env(**({} if qkv_switch is None else dict(PF_ATTN_QKV=qkv_switch)))
    D = heads * 64
    g = torch.Generator().manual_seed(100 * B + S)
    qkv = torch.randn(B * S, 3 * D, generator=g) * scale
    if hot_key:
        qkv.view(B, S, 3, D)[:, S - 7, 1] *= 8
    qkv = qkv.to(BF).to(DEV)
    out = torch.full((B * S + 2, D), float("nan"), dtype=BF, device=DEV)
    op_checks._flush_caches()
    ops.vit_attention(qkv, out[1:-1], B, S, heads)
    torch.cuda.synchronize()
    assert torch.isnan(out[0]).all() and torch.isnan(out[-1]).all() and torch.isfinite(out[1:-1].float()).all()

    def attn(xx):
        q, k, v = xx.view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)
        return (((q * 0.125) @ k.transpose(-2, -1)).softmax(-1) @ v).transpose(1, 2).reshape(B * S, D)
    ref = attn(qkv.double())
    e, c = _stats(out[1:-1], ref), _stats(attn(qkv), ref)
    _log(f"{f'attention_bf16_B{B}_S{S}_h{heads}' + ('_hot' if hot_key else ''):34s} {'PF_ATTN_QKV=' + str(qkv_switch):18s} hip max {e[0]:.2e} p99.9 {e[1]:.2e} norm {e[2]:.2e} | "
         f"torch.bfloat16 max {c[0]:.2e} p99.9 {c[1]:.2e} norm {c[2]:.2e}")
    assert e[2] <= 2 * c[2] and e[1] <= 2 * c[1] and e[0] <= 4 * c[0], (e, c)
