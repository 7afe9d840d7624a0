"""pytest -m gpu: the accepted CORNERS of the argument envelope (tests/envelope.py) -- the smallest shapes at which an edge of a kernel exists: one row,
one token, one pixel, the smallest channel count and leading dimension a launcher takes, the largest D, sizes one below / at / one above a tile.

Every case calls the library through the C ABI (hip_ops' thin wrappers or the ctypes functions themselves) on NaN-filled outputs with guard rows and
columns that must stay NaN, repeats the call and demands the same bits, and is held to the float64 references of tests/f64_image_ref.py,
tests/f64_attn_ref.py and tests/f64_ref.py with exactly the bar the grade module of that kernel applies (named in the printed line): counted_bar
where the roundings can be counted, baseline_bar (at most twice the float32 restatement of tests/fake_ops.py on the same operands -- also the bar for
the corners that degenerate the magnitude, D = 8 for LayerNorm), the caps of f64_ref for the float32 direct convolution, bit equality for copies and
selections.  One line per case (run with -s); profiles/envelope_corners.log is that table.

Before a corner came here its kernel was read at that shape: every load and store is bounded by the sizes the launcher now checks (the notes at
the cases say where the bound sits).  Nothing here passes an argument the launcher refuses: those rows run on the CPU-only machine
(tests/test_envelope_refusals_cpu.py)."""

import pytest
import torch

from tests import f64_attn_ref as A
from tests import f64_image_ref as I
from tests import f64_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])

# corner id of tests/envelope.py -> the tests of this module that run it
CORNER_TESTS = {
    "layernorm": ("test_layernorm_corners",), "patch_im2col": ("test_patch_im2col_corners",), "assemble_tokens": ("test_assemble_tokens_corners",),
    "readout_concat": ("test_readout_concat_corners",), "patch_im2col_norm": ("test_patch_im2col_norm_corners",), "vit_attention_qkv": ("test_attention_corners",), "vit_attention_heads": ("test_attention_corners",),
    "vit_attention_split3": ("test_attention_corners",), "vit_attention_split3_v2": ("test_attention_corners",),
    "vit_attention_qkv_split3": ("test_attention_corners",), "swin": ("test_swin_corners",), "add_rowwise": ("test_add_rowwise_one_token",),
    "resize": ("test_resize_corners",), "planar_resize": ("test_planar_resize_corners",), "roi_align": ("test_roi_align_corners",),
    "maxpool2": ("test_maxpool2_corners",), "copy_channels": ("test_one_pixel_copies",), "pack_fusion_input": ("test_one_pixel_copies",),
    "nhwc_to_nchw": ("test_one_pixel_copies",), "stitch_update": ("test_stitch_update_at_the_map_edge",), "bins": ("test_bins_corners",),
    "conv": ("test_conv_f32_corners", "test_conv_bf16_corners", "test_conv_shuffle2_cout16", "test_conv_batch2_planes", "test_conv_f32_cin4_one_pixel",
             "test_korder1_is_what_the_cin32_corner_runs"),
    "layernorm_planes": ("test_layernorm_plane_corners",), "linears": ("test_linear_corners",), "conv1x1_split3": ("test_conv1x1_split3_corners",),
    "gemm_bf16_pp": ("test_gemm_bf16_pp_corners",), "winograd": ("test_winograd_corners",), "vit_attention_f16x2": ("test_attention_f16x2_corners",),
    "vit_attention_split3_rpb": ("test_attention_rpb_corner",), "vit_attention_rpb_bf16": ("test_attention_rpb_bf16_corner",),
    "winograd_abi": ("test_winograd_32_to_8_through_the_abi",),
}


def _hip():
    from patchfusion_amd.hip_ops import ops
    return ops


def _fake():
    from tests.fake_ops import ops
    return ops


def _abi():
    from patchfusion_amd.hip_ops import _L, _p, _stream, check
    return _L, _p, _stream, check


def _nan(shape, dt=F32):
    return torch.full(shape, NAN, dtype=dt, device=DEV)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _line(text):
    print("\ncorner " + text)            # (a line of its own: under -s the first line of a test would follow pytest's progress dot)


def _graded(case, y, ref, mag, ybase, same):
    e, b = I.errors(y, ref, mag), I.errors(ybase, ref, mag)
    _line(f"{case:54s} elem {e[0]:.2e} norm {e[1]:.2e} | bar baseline_bar: restatement elem {b[0]:.2e} norm {b[1]:.2e} | repeat {same}")
    assert same and I.baseline_bar(e, b), (case, same, e, b)


def _counted(case, y, ref, mag, k, bf, same):
    ok, worst = I.counted_bar(y, ref, mag, k, bf)
    e = I.errors(y, ref, mag)
    _line(f"{case:54s} elem {e[0]:.2e} norm {e[1]:.2e} | bar counted_bar k={k}: worst |d| / bound {worst:.2f} | repeat {same}")
    assert same and ok, (case, same, worst)


def _equal(case, y, want, same):
    eq = torch.equal(_bits(y), _bits(want))
    _line(f"{case:54s} bar bit equality: {eq} | repeat {same}")
    assert same and eq, case


def _tag(dt):
    return "bf16" if dt == BF16 else "f32"


# ---------------- LayerNorm: one wave per row, four rows per block, 8 channels per lane ----------------
@DTYPES
@pytest.mark.parametrize("D", [8, 2048])
def test_layernorm_corners(D, dt):
    """rows 1, 3, 5 (a block holds 4: less than one block, one short, one over), x_ld = D with y_ld = D + 8, and the remap with one output row per
    batch.  The kernel bounds rows by batches * out_rows and channel vectors by D / 8; row addresses are row * ld."""
    g = torch.Generator().manual_seed(D)
    gamma, beta = (torch.randn(D, generator=g) * 0.5), (torch.randn(D, generator=g) * 0.2)
    for rows, remap in ((1, False), (3, False), (5, False), (3, True)):
        nin = rows * 4 if remap else rows
        x = (torch.randn(nin, D, generator=g) * (0.5 + torch.rand(D, generator=g)) + torch.randn(D, generator=g)).to(dt)
        kw = dict(batches=rows, in_rows_per_batch=4, in_row_offset=2, out_rows_per_batch=1) if remap else {}
        xs = (x.double().view(rows, 4, D)[:, 2] if remap else x.double())
        mu, var = xs.mean(1, keepdim=True), xs.var(1, unbiased=False, keepdim=True)
        rstd = 1.0 / (var + float(torch.tensor(1e-6, dtype=torch.float32))).sqrt()
        ref = (xs - mu) * rstd * gamma.double() + beta.double()
        mag = ((xs - mu).abs() + mu.abs()) * rstd * gamma.double().abs() + beta.double().abs()
        xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
        yb = _nan((rows, D), dt)
        _fake().layernorm(xd, yb, gd, bd, 1e-6, **kw)
        outs = []
        for _ in range(2):
            yw = _nan((rows + 2, D + 8), dt)
            yv = yw[1:-1, :D]
            assert xd.stride(0) == D and yv.stride(0) == D + 8
            _hip().layernorm(xd, yv, gd, bd, 1e-6, **kw)
            torch.cuda.synchronize()
            assert torch.isfinite(yv).all() and torch.isnan(yw[0]).all() and torch.isnan(yw[-1]).all() and torch.isnan(yw[:, D:]).all(), "guards"
            outs.append(yv.clone())
        _graded(f"layernorm_{_tag(dt)}_D{D}_rows{rows}{'_remap1' if remap else ''}", outs[0], ref, mag, yb, torch.equal(_bits(outs[0]), _bits(outs[1])))


# ---------------- patch im2col ----------------
@DTYPES
def test_patch_im2col_corners(dt):
    """one patch (14 x 14) and two (14 x 28); ld = 588 (no padding column) and 589, the next one the launcher takes (scalar stores)"""
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32).double().view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32).double().view(1, 3, 1, 1)
    for W in (14, 28):
        for ld in (588, 589):
            img = torch.rand(1, 3, 14, W, generator=torch.Generator().manual_seed(W + ld))
            n = W // 14
            im = lambda t: t.view(1, 3, 1, 14, n, 14).permute(0, 2, 4, 3, 5, 1).reshape(n, 588)
            ref, mag = im((img.double() - mean) / std), im((img.double().abs() + mean) / std)
            outs = []
            for _ in range(2):
                col = _nan((n + 2, ld), dt)
                _hip().patch_im2col(img.to(DEV), col[1:-1])
                torch.cuda.synchronize()
                assert torch.isnan(col[0]).all() and torch.isnan(col[-1]).all() and bool((col[1:-1, 588:] == 0).all()), "guards / padding column"
                outs.append(col[1:-1, :588].clone())
            _counted(f"patch_im2col_{_tag(dt)}_14x{W}_ld{ld}", outs[0], ref, mag, 2, dt == BF16, torch.equal(_bits(outs[0]), _bits(outs[1])))


@DTYPES
def test_patch_im2col_norm_corners(dt):
    """the P x P form with per-channel statistics: one patch of 16 x 16 and two (16 x 32); ld = 768 = 3 P^2 (no padding column) and 769.  The same
    expression as pf_patch_im2col -- one subtraction, one division: counted_bar k = 2 (+ the bf16 rounding)."""
    P = 16
    m3, s3 = (0.5, 0.4, 0.6), (0.5, 0.25, 0.3)
    mean = torch.tensor(m3, dtype=torch.float32).double().view(1, 3, 1, 1)
    std = torch.tensor(s3, dtype=torch.float32).double().view(1, 3, 1, 1)
    for W in (16, 32):
        for ld in (768, 769):
            img = torch.rand(1, 3, P, W, generator=torch.Generator().manual_seed(W + ld))
            n = W // P
            im = lambda t: t.view(1, 3, 1, P, n, P).permute(0, 2, 4, 3, 5, 1).reshape(n, 3 * P * P)
            ref, mag = im((img.double() - mean) / std), im((img.double().abs() + mean.abs()) / std)
            outs = []
            for _ in range(2):
                col = _nan((n + 2, ld), dt)
                _hip().patch_im2col_norm(img.to(DEV), col[1:-1], P, m3, s3)
                torch.cuda.synchronize()
                assert torch.isnan(col[0]).all() and torch.isnan(col[-1]).all() and bool((col[1:-1, 768:] == 0).all()), "guards / padding column"
                outs.append(col[1:-1, :768].clone())
            _counted(f"patch_im2col_norm_{_tag(dt)}_16x{W}_ld{ld}", outs[0], ref, mag, 2, dt == BF16, torch.equal(_bits(outs[0]), _bits(outs[1])))


# ---------------- token assembly, readout rows ----------------
@pytest.mark.parametrize("D", [8, 2048])
@pytest.mark.parametrize("S", [1, 2])
def test_assemble_tokens_corners(S, D):
    """S = 1: the cls token alone (the embedding is never read: s == 0 for every element); D = 8 is the smallest the launcher takes"""
    g = torch.Generator().manual_seed(S * D)
    cls, pos, emb = torch.randn(D, generator=g), torch.randn(S, D, generator=g), torch.randn(max(S - 1, 1), D, generator=g) * 3
    want = (torch.cat([cls.view(1, 1, D), emb.view(1, -1, D)[:, :S - 1]], 1) + pos)
    outs = []
    for _ in range(2):
        buf = _nan((S * D + 32,))
        tok = buf[16:-16].view(1, S, D)
        _hip().assemble_tokens(emb.to(DEV), tok, cls.to(DEV), pos.to(DEV))
        torch.cuda.synchronize()
        assert torch.isnan(buf[:16]).all() and torch.isnan(buf[-16:]).all(), "guards"
        outs.append(tok.clone())
    _equal(f"assemble_tokens_f32_S{S}_D{D}", outs[0], want, torch.equal(_bits(outs[0]), _bits(outs[1])))


@DTYPES
def test_readout_concat_corners(dt):
    """S = 2 (one token row + cls), D = 4 (f32) / 8 (bf16): one 16-byte granule per half, y_ld = 2 D exactly"""
    D = 4 if dt == F32 else 8
    x = torch.randn(2, D, generator=torch.Generator().manual_seed(D)).to(dt)
    outs = []
    for _ in range(2):
        buf = _nan((3, 2 * D), dt)
        _hip().readout_concat(x.to(DEV), buf[1:2], 1, 2)
        torch.cuda.synchronize()
        assert torch.isnan(buf[0]).all() and torch.isnan(buf[2]).all(), "guards"
        outs.append(buf[1:2].clone())
    _equal(f"readout_concat_{_tag(dt)}_S2_D{D}", outs[0], torch.cat([x[1], x[0]])[None], torch.equal(_bits(outs[0]), _bits(outs[1])))


# ---------------- ViT attention: S one below / at / one above a 64-key tile, and one token ----------------
@pytest.mark.parametrize("S", [1, 63, 64, 65])
def test_attention_corners(S):
    """B = Hh = 1.  Every kernel clamps its query row to S - 1 and zero-fills keys >= S (vit.hip: min(key, S - 1) / kg < S; attn_split3.hip: the
    same guards on its last tile), V^T is read from the Sp-padded buffer (Sp = 64 for S <= 64, 128 for S = 65)."""
    _L, _p, _stream, check = _abi()
    B, heads = 1, 1
    qkv = A.random(B, S, heads, 1.0, A.seed_of("corner", S)).to(DEV)
    ref, mag = A.attention_ref(qkv, B, S, heads)
    yb = A.restatement_f32(qkv, B, S, heads)
    M, D = B * S, heads * 64

    def twice(launch, make):
        a, b = make(), make()
        launch(a)
        launch(b)
        torch.cuda.synchronize()
        return a, torch.equal(_bits(a), _bits(b))

    rows = lambda: _nan((M + 2, D))
    y, same = twice(lambda o: check(_L.pf_vit_attention_qkv(_p(qkv), _p(o[1:-1]), B, S, heads, 0, _stream()), "qkv"), rows)
    assert torch.isnan(y[0]).all() and torch.isnan(y[-1]).all(), "guards"
    yf = y[1:-1]
    _graded(f"vit_attention_qkv_f32_S{S}", yf, ref, mag, yb, same)
    Sp = (S + 63) // 64 * 64
    q, k, vt = _nan((B, heads, S, 64)), _nan((B, heads, S, 64)), _nan((B, heads, 64, Sp))
    check(_L.pf_qkv_split(_p(qkv), B, S, heads, _p(q), _p(k), _p(vt), Sp, 0.125, 0, _stream()), "pf_qkv_split")
    torch.cuda.synchronize()
    qh, kh, vh = A._heads(qkv, B, S, heads)
    _equal(f"qkv_split_f32_S{S}_Sp{Sp}", torch.cat([q.flatten(), k.flatten(), vt[..., :S].flatten(), vt[..., S:].flatten()]),
           torch.cat([(qh * 0.125).flatten(), kh.flatten(), vh.transpose(-2, -1).flatten(), torch.zeros(64 * (Sp - S), device=DEV)]), True)
    y, same = twice(lambda o: check(_L.pf_vit_attention(_p(q), _p(k), _p(vt), _p(o[1:-1]), B, S, Sp, heads, 0, _stream()), "attention"), rows)
    assert torch.isnan(y[0]).all() and torch.isnan(y[-1]).all(), "guards"
    _graded(f"vit_attention_f32_S{S}_Sp{Sp}", y[1:-1], ref, mag, yb, same)
    # the split-precision kernels: the baseline is the larger of the restatement's and the f32-MFMA kernel's errors (tests/test_attention_grade_gpu.py)
    base_y = yf if max(I.errors(yf, ref, mag)) > max(I.errors(yb, ref, mag)) else yb
    q3 = torch.empty(3, M, 3 * D, dtype=BF16, device=DEV)
    _hip().split3(qkv, q3)
    assert torch.equal(q3.double().sum(0), qkv.double())
    planes = lambda: _nan((3, M, D), BF16)
    runs = [("split3_v1", lambda o: check(_L.pf_vit_attention_split3(_p(q3), q3.stride(0), _p(o), o.stride(0), 0, B, S, heads, _stream()), "v1"))]
    runs += [(f"split3_v2_qw{qw}_sched{sc}", lambda o, qw=qw, sc=sc: check(_L.pf_vit_attention_split3_v2(_p(q3), q3.stride(0), _p(o), o.stride(0), 0, B, S, heads, qw,
                                                                                                  sc, _stream()), "v2")) for qw, sc in ((16, 1), (32, 1), (0, 2))]
    runs += [("qkv_split3", lambda o: check(_L.pf_vit_attention_qkv_split3(_p(qkv), _p(o), o.stride(0), 0, B, S, heads, _stream()), "qkv_split3"))]
    for name, launch in runs:
        o, same = twice(launch, planes)
        _graded(f"vit_attention_{name}_S{S}", o.cpu().double().sum(0), ref, mag, base_y, same)


# ---------------- Swin ----------------
@DTYPES
@pytest.mark.parametrize("shift", [0, 6])
@pytest.mark.parametrize("case", [(1, 1, 1, 8, 1), (1, 13, 11, 32, 16)], ids=["1x1_C8_h1", "13x11_C32_h16"])
def test_swin_corners(case, shift, dt):
    """1 x 1 (padded to 12 x 12: 143 of 144 tokens are padding) and 13 x 11 (padded to 24 x 12); C = 8 with one head (head_dim 8, one lane per token in
    the partition kernel) and C = 32 with 16 heads (head_dim 2, the matrix-pipe kernel for float32)"""
    from tests import test_f64_image_ref_cpu as Cc
    B, H, W, Ch, heads = case
    x, gam, bet, qkv, bt, proj, Hp, Wp, nt = Cc.swin_operands(*case, dt)
    name = f"{'x'.join(map(str, case))}_s{shift}_{_tag(dt)}"
    xd, gd, bd = x.to(DEV), gam.to(DEV), bet.to(DEV)
    ref, mag = I.swin_ln_partition_ref(x, gam, bet, 1e-5, shift)
    yb = _nan((nt, Ch), dt)
    _fake().swin_ln_partition(xd, yb, gd, bd, 1e-5, shift)
    outs = []
    for _ in range(2):
        buf = _nan((nt + 2, Ch), dt)
        _hip().swin_ln_partition(xd, buf[1:-1], gd, bd, 1e-5, shift)
        torch.cuda.synchronize()
        assert torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all() and torch.isfinite(buf[1:-1]).all(), "guards"
        outs.append(buf[1:-1].clone())
    assert bool((outs[0].cpu()[mag == 0] == 0).all()), "a padded token is not exactly zero"
    _graded("swin_ln_partition_" + name, outs[0], ref, mag, yb, torch.equal(_bits(outs[0]), _bits(outs[1])))
    ref, mag = I.swin_window_attention_ref(qkv, bt, B, Hp, Wp, Ch, heads, shift)
    qd, btd = qkv.to(DEV), bt.to(DEV)
    yb = _nan(tuple(ref.shape), dt)
    _fake().swin_window_attention(qd, yb, btd, B, Hp, Wp, Ch, heads, shift)
    outs = []
    for _ in range(2):
        buf = _nan((nt + 2, Ch), dt)
        _hip().swin_window_attention(qd, buf[1:-1], btd, B, Hp, Wp, Ch, heads, shift)
        torch.cuda.synchronize()
        assert torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all() and torch.isfinite(buf[1:-1]).all(), "guards"
        outs.append(buf[1:-1].clone())
    _graded("swin_window_attention_" + name, outs[0], ref, mag, yb, torch.equal(_bits(outs[0]), _bits(outs[1])))
    ref, mag = I.swin_unpartition_add_ref(proj, x, shift)
    outs = []
    for _ in range(2):
        buf = _nan((B, H, W, Ch + 16), dt)
        _hip().swin_unpartition_add(proj.to(DEV), xd, buf[..., 8:8 + Ch], shift)
        torch.cuda.synchronize()
        assert torch.isnan(buf[..., :8]).all() and torch.isnan(buf[..., 8 + Ch:]).all(), "guards"
        outs.append(buf[..., 8:8 + Ch].clone())
    _counted("swin_unpartition_add_" + name, outs[0], ref, mag, I.K_ADD, dt == BF16, torch.equal(_bits(outs[0]), _bits(outs[1])))


@DTYPES
def test_add_rowwise_one_token(dt):
    """B = T = 1, C = 8: one 8-channel vector; x_ld = 16 so that the other half of the row must stay untouched"""
    g = torch.Generator().manual_seed(3)
    x, pos = torch.randn(1, 1, 8, generator=g).to(dt), torch.randn(1, 8, generator=g)
    ref, mag = x.double() + pos.double(), x.double().abs() + pos.double().abs()
    outs = []
    for _ in range(2):
        buf = _nan((1, 1, 16), dt)
        buf[..., :8] = x.to(DEV)
        _hip().add_rowwise(buf[..., :8], pos.to(DEV))
        torch.cuda.synchronize()
        assert torch.isnan(buf[..., 8:]).all(), "guards"
        outs.append(buf[..., :8].clone())
    _counted(f"add_rowwise_{_tag(dt)}_T1_C8", outs[0], ref, mag, I.K_ADD, dt == BF16, torch.equal(_bits(outs[0]), _bits(outs[1])))


# ---------------- resizes: the align_corners 0 / 0 case ----------------
RESIZE_CORNERS = [(1, 1, 1, 1), (1, 1, 3, 5), (3, 5, 1, 1)]


@pytest.mark.parametrize("v2", ["1", "0"], ids=["v2", "v1"])
@DTYPES
@pytest.mark.parametrize("h,w,oh,ow", RESIZE_CORNERS, ids=lambda v: str(v))
def test_resize_corners(monkeypatch, h, w, oh, ow, dt, v2):
    """an output (or input) of one row / column: the scale is (in - 1) / (out - 1) -> 0 for out = 1 by definition (ac_scale), every tap is element 0.
    Both kernel versions; resize, resize + add, the two-source concat and the bf16 -> float32 mixed form."""
    monkeypatch.setenv("PF_RESIZE_V2", v2)
    Ch = 8
    x, add = I.features((1, h, w, Ch), h + w, dt), I.features((1, oh, ow, Ch), oh + ow + 1, dt)
    xd, ad = x.to(DEV), add.to(DEV)
    bf = dt == BF16
    name = f"{h}x{w}_to_{oh}x{ow}_{_tag(dt)}_v{2 if v2 == '1' else 1}"

    def run(call, width, odt=dt):
        outs = []
        for _ in range(2):
            buf = _nan((1, oh, ow, width + 16), odt)
            call(buf[..., 8:8 + width])
            torch.cuda.synchronize()
            assert torch.isnan(buf[..., :8]).all() and torch.isnan(buf[..., 8 + width:]).all() and torch.isfinite(buf[..., 8:8 + width]).all(), "guards"
            outs.append(buf[..., 8:8 + width].clone())
        return outs[0], torch.equal(_bits(outs[0]), _bits(outs[1]))

    y, same = run(lambda o: _hip().resize(xd, o), Ch)
    _counted("resize_" + name, y, *I.bilinear_ref(x, oh, ow), I.K_BILERP, bf, same)
    y, same = run(lambda o: _hip().resize(xd, o, add=ad), Ch)
    _counted("resize_add_" + name, y, *I.bilinear_ref(x, oh, ow, add), I.K_BILERP_ADD, bf, same)
    y, same = run(lambda o: _hip().resize_concat([xd, xd], o), 2 * Ch)
    _counted("resize_concat2_" + name, y, *I.resize_concat_ref([x, x], oh, ow), I.K_BILERP, bf, same)
    if bf:
        y, same = run(lambda o: _hip().resize(xd, o), Ch, F32)
        _counted("resize_bf16_to_f32_" + name, y, *I.bilinear_ref(x, oh, ow), I.K_BILERP, False, same)


@pytest.mark.parametrize("h,w,oh,ow", RESIZE_CORNERS, ids=lambda v: str(v))
def test_planar_resize_corners(h, w, oh, ow):
    x = I.features((h, w, 1), h * w + 2)[..., 0].contiguous()
    xd = x.to(DEV)
    ref, mag = I.bilinear_plane_ref(x, oh, ow)
    for op, kind in ((_hip().resize_bilinear_f32, "bilinear"), (_hip().resize_nearest_f32, "nearest")):
        outs = []
        for _ in range(2):
            buf = _nan((oh + 2, ow))
            op(xd, buf[1:-1])
            torch.cuda.synchronize()
            assert torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all(), "guards"
            outs.append(buf[1:-1].clone())
        same = torch.equal(_bits(outs[0]), _bits(outs[1]))
        if kind == "bilinear":
            _counted(f"resize_bilinear_f32_{h}x{w}_to_{oh}x{ow}", outs[0], ref, mag, I.K_BILERP, False, same)
        else:
            _equal(f"resize_nearest_f32_{h}x{w}_to_{oh}x{ow}", outs[0], I.nearest_ref(x, oh, ow), same)


# ---------------- roi_align ----------------
@pytest.mark.parametrize("Ch", [1, 8])
def test_roi_align_corners(Ch):
    """an RoI of zero area (one sample per bin, all at one point) and one wholly outside the map (no sample: exactly 0); the planar C = 1 form and
    the NHWC C = 8 form.  Sample coordinates outside [-1, size] are skipped, inside they are clamped to [0, size - 1]: no tap leaves the map."""
    f = torch.randn(2, 6, 7, Ch, generator=torch.Generator().manual_seed(Ch))      # two maps: the RoIs name both (the batch index is clamped in the kernel)
    rois = torch.tensor([[1, 2.5, 3.0, 2.5, 3.0], [0, 40.0, 40.0, 50.0, 50.0], [1, 0.0, 0.0, 7.0, 6.0], [0, 0.0, 0.0, 7.0, 6.0]])
    ref, mag = I.roi_align_ref(f, rois, 2, 3, 1.0)
    fd, rd = f.to(DEV), rois.to(DEV)
    outs = []
    if Ch == 1:
        yb = _nan((4, 1, 2, 3))
        _fake().roi_align_depth(fd.permute(0, 3, 1, 2).contiguous(), rd, yb, 1.0)
        for _ in range(2):
            buf = _nan((6, 1, 2, 3))
            _hip().roi_align_depth(fd.permute(0, 3, 1, 2).contiguous(), rd, buf[1:-1], 1.0)
            torch.cuda.synchronize()
            assert torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all(), "guards"
            outs.append(buf[1:-1].clone())
        ref, mag = ref.permute(0, 3, 1, 2), mag.permute(0, 3, 1, 2)
    else:
        yb = _nan((4, 2, 3, Ch))
        _fake().roi_align(fd, rd, yb, 1.0)
        for _ in range(2):
            buf = _nan((4, 2, 3, Ch + 16))
            _hip().roi_align(fd, rd, buf[..., 8:8 + Ch], 1.0)
            torch.cuda.synchronize()
            assert torch.isnan(buf[..., :8]).all() and torch.isnan(buf[..., 8 + Ch:]).all(), "guards"
            outs.append(buf[..., 8:8 + Ch].clone())
    assert bool((outs[0][1] == 0).all()), "the RoI outside the map is not zero"
    assert not torch.equal(outs[0][2], outs[0][3]), "the same RoI on map 1 and on map 0 gave the same output: the batch index is not used"
    _graded(f"roi_align_C{Ch}_zero_area_outside_whole", outs[0], ref, mag, yb, torch.equal(_bits(outs[0]), _bits(outs[1])))


# ---------------- max-pool, copies ----------------
@DTYPES
@pytest.mark.parametrize("h,w", [(2, 2), (3, 5)])
def test_maxpool2_corners(h, w, dt):
    """2 x 2 -> one pixel; 3 x 5 -> 1 x 2: the odd last row and column are dropped (the kernel walks H / 2 x W / 2 outputs and reads 2 oy + 1 <= H - 1)"""
    x = torch.randn(1, h, w, 8, generator=torch.Generator().manual_seed(h * w)).to(dt)
    outs = []
    for _ in range(2):
        buf = _nan((1, h // 2, w // 2, 24), dt)
        _hip().maxpool2(x.to(DEV), buf[..., 8:16])
        torch.cuda.synchronize()
        assert torch.isnan(buf[..., :8]).all() and torch.isnan(buf[..., 16:]).all(), "guards"
        outs.append(buf[..., 8:16].clone())
    _equal(f"maxpool2_{_tag(dt)}_{h}x{w}", outs[0], I.maxpool2_ref(x), torch.equal(_bits(outs[0]), _bits(outs[1])))


@DTYPES
def test_one_pixel_copies(dt):
    """one pixel, C = 8: copy_channels (same dtype), pack_fusion_input and nhwc_to_nchw"""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, 1, 1, 8, generator=g).to(dt)
    buf = _nan((1, 1, 1, 24), dt)
    _hip().copy_channels(x.to(DEV), buf[..., 8:16])
    torch.cuda.synchronize()
    assert torch.isnan(buf[..., :8]).all() and torch.isnan(buf[..., 16:]).all(), "guards"
    _equal(f"copy_channels_{_tag(dt)}_1px_C8", buf[..., 8:16], x, True)
    cd, fd, crop = torch.rand(1, 1, 1, 1, generator=g), torch.rand(1, 1, 1, 1, generator=g), torch.rand(1, 3, 1, 1, generator=g)
    y = _nan((3, 1, 1, 8), dt)
    _hip().pack_fusion_input(cd.to(DEV), fd.to(DEV), crop.to(DEV), y[1:2])
    torch.cuda.synchronize()
    assert torch.isnan(y[0]).all() and torch.isnan(y[2]).all(), "guards"
    want = torch.cat([cd.flatten(), fd.flatten(), crop.flatten(), torch.zeros(3)]).to(dt).view(1, 1, 1, 8)
    _equal(f"pack_fusion_input_{_tag(dt)}_1px", y[1:2], want, True)
    out = _hip().nhwc_to_nchw(x.to(DEV))
    torch.cuda.synchronize()
    _equal(f"nhwc_to_nchw_{_tag(dt)}_1px_C8", out, x.float().permute(0, 3, 1, 2), True)


# ---------------- stitch ----------------
@pytest.mark.parametrize("y0,x0", [(4, 5), (5, 7)], ids=["ends_at_the_edge", "clipped_by_the_edge"])
def test_stitch_update_at_the_map_edge(y0, x0):
    """a 4 x 5 tile on an 8 x 10 map: ending exactly at the last row / column, and starting one row / two columns later so that the edge clips it
    (the kernel skips Y >= MH, X >= MW; the launcher refuses a window that starts in front of the map)"""
    g = torch.Generator().manual_seed(y0)
    avg, cnt = torch.rand(8, 10, generator=g) + 0.5, torch.ones(8, 10)
    d, m = torch.rand(4, 5, generator=g) + 0.5, torch.rand(4, 5, generator=g)
    vh, vw = min(4, 8 - y0), min(5, 10 - x0)
    (ra, ma), (rc, mc) = I.stitch_update_ref(avg, cnt, d[:vh, :vw], m[:vh, :vw], y0, x0)
    outs = []
    for _ in range(2):
        buf_a, buf_c = _nan((10, 10)), _nan((10, 10))
        buf_a[1:-1], buf_c[1:-1] = avg.to(DEV), cnt.to(DEV)
        _hip().stitch_update(buf_a[1:-1], buf_c[1:-1], d.to(DEV), m.to(DEV), y0, x0)
        torch.cuda.synchronize()
        assert torch.isnan(buf_a[0]).all() and torch.isnan(buf_a[-1]).all() and torch.isnan(buf_c[0]).all() and torch.isnan(buf_c[-1]).all(), "guards"
        outs.append((buf_a[1:-1].clone(), buf_c[1:-1].clone()))
    same = torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
    _counted(f"stitch_update_avg_y{y0}_x{x0}", outs[0][0], ra, ma, I.K_STITCH_AVG, False, same)
    _counted(f"stitch_update_count_y{y0}_x{x0}", outs[0][1], rc, mc, I.K_ADD, False, same)


# ---------------- metric-bins kernels at one pixel, four bins, one attractor ----------------
def test_bins_corners():
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(4)
    A_, bp = F.softplus(torch.randn(1, 1, 1, 4, generator=g)), F.softplus(torch.randn(1, 1, 1, 4, generator=g))
    ref, mag = I.attractor_ref(A_, 1, bp, 1, 1)
    y, yb = _nan((3, 1, 1, 4)), _nan((1, 1, 1, 4))
    _hip().attractor(A_.to(DEV), 1, bp.to(DEV), y[1:2])
    _fake().attractor(A_.to(DEV), 1, bp.to(DEV), yb)
    torch.cuda.synchronize()
    assert torch.isnan(y[0]).all() and torch.isnan(y[2]).all(), "guards"
    _graded("attractor_n1_1x1_bins4", y[1:2], ref, mag, yb, True)
    pt = F.softplus(torch.randn(1, 1, 1, 4, generator=g))
    cen = F.softplus(torch.randn(1, 1, 1, 4, generator=g))
    ref, mag = I.logbinom_depth_ref(pt, cen, 1, 1, 0.0212, 50.0)
    y, yb = _nan((3, 1, 1)), _nan((1, 1, 1))
    _hip().logbinom_depth(pt.to(DEV), cen.to(DEV), y[1:2], 0.0212, 50.0)
    _fake().logbinom_depth(pt.to(DEV), cen.to(DEV), yb, 0.0212, 50.0)
    torch.cuda.synchronize()
    assert torch.isnan(y[0]).all() and torch.isnan(y[2]).all(), "guards"
    _graded("logbinom_depth_1x1_bins4", y[1:2], ref, mag, yb, True)


# ---------------- pf_conv, float32: the direct kernels at their smallest shapes ----------------
CONV_CORNERS = [  # cin, cout, k, stride, pad, B, H, W
    (8, 4, 1, 1, 0, 1, 1, 1), (8, 4, 3, 1, 1, 1, 1, 1), (8, 4, 3, 2, 1, 1, 5, 7), (8, 4, 4, 4, 0, 1, 8, 8), (32, 8, 3, 1, 1, 2, 3, 5),
]


@pytest.mark.parametrize("c", CONV_CORNERS, ids=lambda c: f"{c[0]}to{c[1]}_k{c[2]}s{c[3]}p{c[4]}_{c[5]}x{c[6]}x{c[7]}")
def test_conv_f32_corners(c):
    """Cin = 8 (the packer pads input channels to 8: packing.pack_conv), Cout = 4 on one pixel with 1 x 1 and with 3 x 3 pad 1 (every tap but the centre is padding: the loaders bound-check against H x W);
    3 x 3 stride 2 on 5 x 7; 4 x 4 taps (the limit of 16) stride 4 on 8 x 8; two images of 3 x 5.  The direct route (pf_conv), its caps."""
    from patchfusion_amd import packing as pk
    cin, cout, k, stride, pad, B, H, W = c
    g = torch.Generator().manual_seed(sum(c))
    w, b = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5, torch.randn(cout, generator=g)
    x = torch.randn(B, H, W, cin, generator=g)
    pw = pk.pack_conv(w, b, dtype=F32).to(DEV)
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    pix = R.sample_pixels(B, OH, OW, n_random=8, seed=1)
    ref, mag = R.conv_ref(x, w, pix, b, stride=stride, pad=pad)
    outs = []
    for _ in range(2):
        buf = _nan((B, OH, OW, cout + 8))
        _hip().conv(x.to(DEV), pw, buf[..., 4:4 + cout], stride=stride, pad=pad, _direct=True)
        torch.cuda.synchronize()
        assert torch.isnan(buf[..., :4]).all() and torch.isnan(buf[..., 4 + cout:]).all() and torch.isfinite(buf[..., 4:4 + cout]).all(), "guards"
        outs.append(buf[..., 4:4 + cout].clone())
    same = torch.equal(_bits(outs[0]), _bits(outs[1]))
    e = R.errors(R.gather_pixels(outs[0], pix, cout), ref, mag)
    _line(f"{'conv_f32_direct_' + '_'.join(map(str, c)):54s} elem {e[0]:.2e} norm {e[1]:.2e} | bar f64_ref caps: elem {R.ELEM_CAP_GEMM:.1e} norm {R.NORM_CAP_GEMM:.1e} | repeat {same}")
    assert same and e[0] <= R.ELEM_CAP_GEMM and e[1] <= R.NORM_CAP_GEMM, (c, same, e)


def _conv_case(c, dt, seed_off=0):
    from patchfusion_amd import packing as pk
    cin, cout, k, stride, pad, B, H, W = c
    g = torch.Generator().manual_seed(sum(c) + seed_off)
    w, b = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5, torch.randn(cout, generator=g)
    x = torch.randn(B, H, W, cin, generator=g)
    if dt == BF16:
        w, x = w.to(BF16).float(), x.to(BF16).float()
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    pix = R.sample_pixels(B, OH, OW, n_random=8, seed=1)
    ref, mag = R.conv_ref(x, w, pix, b, stride=stride, pad=pad)
    return w, b, x, OH, OW, pix, ref, mag, pk


def _conv_run(x, pw, B, OH, OW, cout, dt, stride, pad, pix, direct):
    outs = []
    for _ in range(2):
        buf = _nan((B, OH, OW, cout + 16), dt)
        _hip().conv(x, pw, buf[..., 8:8 + cout], stride=stride, pad=pad, _direct=direct)
        torch.cuda.synchronize()
        assert torch.isnan(buf[..., :8]).all() and torch.isnan(buf[..., 8 + cout:]).all() and torch.isfinite(buf[..., 8:8 + cout]).all(), "guards"
        outs.append(buf[..., 8:8 + cout].clone())
    return R.gather_pixels(outs[0], pix, cout), torch.equal(_bits(outs[0]), _bits(outs[1]))


def test_korder1_is_what_the_cin32_corner_runs():
    """korder = 1 with Cin = 32: the packer gives every float32 k x k layer with Cin % 32 == 0 the chunk-major K order, so the 32 -> 8 3 x 3 case of
    test_conv_f32_corners IS that corner"""
    from patchfusion_amd import packing as pk
    assert pk.pack_conv(torch.zeros(8, 32, 3, 3), None, dtype=F32).korder == 1


@pytest.mark.parametrize("c", CONV_CORNERS, ids=lambda c: f"{c[0]}to{c[1]}_k{c[2]}s{c[3]}p{c[4]}_{c[5]}x{c[6]}x{c[7]}")
def test_conv_bf16_corners(c):
    """the same shapes in bf16 (Cin = 8 is the smallest: one 16-byte vector): bf16_grade against the float32-MFMA kernel on the same bf16-valued
    operands, the bar of tests/test_bf16_grade_gpu.py"""
    cin, cout, k, stride, pad, B, H, W = c
    w, b, x, OH, OW, pix, ref, mag, pk = _conv_case(c, BF16)
    got, same = _conv_run(x.to(BF16).to(DEV), pk.pack_conv(w, b, dtype=BF16).to(DEV), B, OH, OW, cout, BF16, stride, pad, pix, None)
    got32, _ = _conv_run(x.to(DEV), pk.pack_conv(w, b, dtype=F32).to(DEV), B, OH, OW, cout, F32, stride, pad, pix, True)
    e, base = R.bf16_excess(got, ref, mag), R.errors(got32, ref, mag)
    _line(f"{'conv_bf16_direct_' + '_'.join(map(str, c)):54s} excess elem {e[0]:.2e} norm {e[1]:.2e} | bar bf16_grade: f32 kernel elem {base[0]:.2e} norm {base[1]:.2e} | repeat {same}")
    assert same and R.bf16_grade(e, base), (c, same, e, base)


@DTYPES
def test_conv_shuffle2_cout16(dt):
    """shuffle = 2 with Cout = 16 (four output channels per sub-pixel, the smallest the launcher takes), one input pixel -> a 2 x 2 output"""
    from patchfusion_amd import packing as pk
    g = torch.Generator().manual_seed(16)
    w, b, xv = torch.randn(8, 4, 2, 2, generator=g) / 8 ** 0.5, torch.randn(4, generator=g), torch.randn(1, 1, 1, 8, generator=g)
    if dt == BF16:
        w, xv = w.to(BF16).float(), xv.to(BF16).float()
    pix = R.sample_pixels(1, 2, 2, n_random=4, seed=2, tile=2)
    ref, mag = R.conv_transpose_ref(xv, w, pix, b)
    res = {}
    for d in ((BF16, F32) if dt == BF16 else (F32,)):
        pw = pk.pack_conv_transpose(w, b, dtype=d).to(DEV)
        assert pw.shuffle == 2 and pw.cout == 16
        outs = []
        for _ in range(2):
            buf = _nan((1, 2, 2, 4 + 8), d)
            _hip().conv(xv.to(d).to(DEV), pw, buf[..., 4:8], _direct=True if d == F32 else None)
            torch.cuda.synchronize()
            assert torch.isnan(buf[..., :4]).all() and torch.isnan(buf[..., 8:]).all() and torch.isfinite(buf[..., 4:8]).all(), "guards"
            outs.append(buf[..., 4:8].clone())
        res[d] = (R.gather_pixels(outs[0], pix, 4), torch.equal(_bits(outs[0]), _bits(outs[1])))
    if dt == BF16:
        e, base = R.bf16_excess(res[BF16][0], ref, mag), R.errors(res[F32][0], ref, mag)
        _line(f"{'conv_bf16_shuffle2_cout16_1x1':54s} excess elem {e[0]:.2e} norm {e[1]:.2e} | bar bf16_grade: f32 kernel elem {base[0]:.2e} norm {base[1]:.2e} | repeat {res[BF16][1]}")
        assert res[BF16][1] and R.bf16_grade(e, base), (e, base)
    else:
        e = R.errors(res[F32][0], ref, mag)
        _line(f"{'conv_f32_shuffle2_cout16_1x1':54s} elem {e[0]:.2e} norm {e[1]:.2e} | bar f64_ref caps: elem {R.ELEM_CAP_GEMM:.1e} norm {R.NORM_CAP_GEMM:.1e} | repeat {res[F32][1]}")
        assert res[F32][1] and e[0] <= R.ELEM_CAP_GEMM and e[1] <= R.NORM_CAP_GEMM, e


def test_conv_batch2_planes():
    """batch = 2: two independent float32 GEMM planes in one launch (M = 3 rows, K = 32, N = 4), as csrc/winograd.hip issues its transform points;
    through the C ABI with the packed weights of two layers behind each other"""
    from patchfusion_amd import _lib
    from patchfusion_amd import packing as pk
    _L, _p, _stream, check = _abi()
    g = torch.Generator().manual_seed(22)
    M, K, N = 3, 32, 4
    ws = [torch.randn(N, K, 1, 1, generator=g) / K ** 0.5 for _ in range(2)]
    xs = torch.randn(2, M, K, generator=g)
    pws = [pk.pack_conv(w, None, dtype=F32) for w in ws]
    wp = torch.stack([pw.w for pw in pws]).contiguous().to(DEV)
    xd = xs.to(DEV)
    outs = []
    for _ in range(2):
        y = _nan((2, M + 1, N))                     # (one guard row behind each plane)
        p = _lib.ConvParams()
        p.x, p.x_ld, p.B, p.H, p.W, p.Cin = xd.data_ptr(), K, 1, 1, M, K
        p.w, p.w_rows, p.Kpad = wp.data_ptr(), wp.shape[1], wp.shape[2]
        p.y, p.y_ld, p.OH, p.OW, p.Cout = y.data_ptr(), N, 1, M, N
        p.KH = p.KW = p.stride = p.shuffle = 1
        p.batch, p.x_bstride, p.w_bstride, p.y_bstride = 2, M * K, wp.shape[1] * wp.shape[2], (M + 1) * N
        check(_L.pf_conv(C_byref(p), _stream()), "pf_conv")
        torch.cuda.synchronize()
        assert torch.isnan(y[:, M]).all() and torch.isfinite(y[:, :M]).all(), "guards"
        outs.append(y[:, :M].clone())
    same = torch.equal(_bits(outs[0]), _bits(outs[1]))
    for z in range(2):
        ref, mag = R.linear_ref(xs[z], ws[z][:, :, 0, 0])
        e = R.errors(outs[0][z], ref, mag)
        _line(f"{f'conv_f32_batch2_plane{z}_M3_K32_N4':54s} elem {e[0]:.2e} norm {e[1]:.2e} | bar f64_ref caps: elem {R.ELEM_CAP_GEMM:.1e} norm {R.NORM_CAP_GEMM:.1e} | repeat {same}")
        assert same and e[0] <= R.ELEM_CAP_GEMM and e[1] <= R.NORM_CAP_GEMM, (z, e)


@pytest.mark.parametrize("k", [1, 3])
def test_conv_f32_cin4_one_pixel(k):
    """Cin = Cout = 4, the smallest the launcher takes in float32 (one 16-byte vector; the engine's packer pads input channels to 8, so the weights
    are laid out here: [4 rows][Kpad], K order (ky, kx, c)), on one pixel with 1 x 1 and with 3 x 3 pad 1.  A K chunk holds eight taps then: the
    loader's tap mask has bits for the taps of the filter only, every other slot reads the zero page."""
    from patchfusion_amd import _lib
    _L, _p, _stream, check = _abi()
    g = torch.Generator().manual_seed(40 + k)
    w, b, x = torch.randn(4, 4, k, k, generator=g) / (4 * k * k) ** 0.5, torch.randn(4, generator=g), torch.randn(1, 1, 1, 4, generator=g)
    kpad = 32 if k == 1 else 64
    wp = torch.zeros(4, kpad)
    wp[:, :4 * k * k] = w.permute(0, 2, 3, 1).reshape(4, -1)
    wd, bd, xd = wp.to(DEV), b.to(DEV), x.to(DEV)
    pix = R.sample_pixels(1, 1, 1, n_random=1, seed=1)
    ref, mag = R.conv_ref(x, w, pix, b, stride=1, pad=k // 2)
    outs = []
    for _ in range(2):
        buf = _nan((1, 1, 1, 12))
        y = buf[..., 4:8]
        p = _lib.ConvParams()
        p.x, p.x_ld, p.B, p.H, p.W, p.Cin = xd.data_ptr(), 4, 1, 1, 1, 4
        p.w, p.w_rows, p.Kpad, p.bias = wd.data_ptr(), 4, kpad, bd.data_ptr()
        p.y, p.y_ld, p.OH, p.OW, p.Cout = y.data_ptr(), 12, 1, 1, 4
        p.KH = p.KW = k
        p.stride, p.pad, p.shuffle = 1, k // 2, 1
        check(_L.pf_conv(C_byref(p), _stream()), "pf_conv")
        torch.cuda.synchronize()
        assert torch.isnan(buf[..., :4]).all() and torch.isnan(buf[..., 8:]).all() and torch.isfinite(y).all(), "guards"
        outs.append(y.clone())
    same = torch.equal(_bits(outs[0]), _bits(outs[1]))
    e = R.errors(R.gather_pixels(outs[0], pix, 4), ref, mag)
    _line(f"{f'conv_f32_cin4_cout4_k{k}_1x1x1':54s} elem {e[0]:.2e} norm {e[1]:.2e} | bar f64_ref caps: elem {R.ELEM_CAP_GEMM:.1e} norm {R.NORM_CAP_GEMM:.1e} | repeat {same}")
    assert same and e[0] <= R.ELEM_CAP_GEMM and e[1] <= R.NORM_CAP_GEMM, e


def C_byref(p):
    import ctypes
    return ctypes.byref(p)


# ---------------- LayerNorm as plane producer ----------------
@pytest.mark.parametrize("D", [8, 32, 2048])
def test_layernorm_plane_corners(D):
    """pf_layernorm_split3 row-major (D = 8 and 2048) and chunk-major (D = 32 and 2048), pf_layernorm_f16x2 (D = 32 and 2048); rows 1, 3, 5.  The
    kernels are pf_layernorm's with other stores (split3_at bounds a chunk-major row by the row count).  D = 2048: the bar of
    tests/test_float32_grade_gpu.py, float32_grade against pf_layernorm on the same operands with the caps of f64_ref.  D = 8 and 32 degenerate the
    magnitude (a row of 8 / 32 values: pf_layernorm itself sits at one rounding, 6.5e-8 element-wise at D = 32, rows 3, where the fp16x2 planes --
    22 bits -- measured 1.42e-7, 2.2 times that): there the bar is the one the token and image modules use for that situation, baseline_bar against
    the float32 restatement of tests/fake_ops.py (twice the restatement, floored at 4 * 2^-24), and the line prints pf_layernorm's error beside it."""
    from patchfusion_amd import packing as pk
    g = torch.Generator().manual_seed(D + 1)
    gamma, beta = (torch.randn(D, generator=g) * 0.5), (torch.randn(D, generator=g) * 0.2)
    for rows in (1, 3, 5):
        x = torch.randn(rows, D, generator=g) * (0.5 + torch.rand(D, generator=g)) + torch.randn(D, generator=g)
        xd64 = x.double()
        mu, var = xd64.mean(1, keepdim=True), xd64.var(1, unbiased=False, keepdim=True)
        den = (var + float(torch.tensor(1e-6, dtype=torch.float32))).sqrt()
        ref = (xd64 - mu) / den * gamma.double() + beta.double()
        mag = ((xd64 - mu).abs() + mu.abs()) / den * gamma.double().abs() + beta.double().abs()
        xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
        y32, yres = _nan((rows, D)), _nan((rows, D))
        _hip().layernorm(xd, y32, gd, bd, 1e-6)
        _fake().layernorm(xd, yres, gd, bd, 1e-6)
        base, restated = R.errors(y32, ref, mag), R.errors(yres, ref, mag)
        forms = (["rows"] if D != 32 else []) + (["kmaj", "f16x2"] if D % 32 == 0 else [])
        for form in forms:
            outs = []
            for _ in range(2):
                if form == "rows":
                    buf = _nan((3, rows + 2, D), BF16)
                    y3 = buf[:, 1:-1]
                    _hip().layernorm_split3(xd, y3, gd, bd, 1e-6)
                    torch.cuda.synchronize()
                    assert torch.isnan(buf[:, 0]).all() and torch.isnan(buf[:, -1]).all(), "guards"
                    outs.append((y3.clone(), y3.double().sum(0).cpu()))
                elif form == "kmaj":
                    y3 = _nan((3, D // 32, rows, 32), BF16)
                    _hip().layernorm_split3(xd, y3, gd, bd, 1e-6)
                    torch.cuda.synchronize()
                    outs.append((y3.clone(), pk.kmajor_to_rows(y3.cpu()).double().sum(0)))
                else:
                    in_exp = pk.bound_exponents(pk.layernorm_bound(gamma, beta)).to(DEV)
                    y2 = _nan((2, D // 32, rows, 32), torch.float16)
                    _hip().layernorm_f16x2(xd, y2, gd, bd, 1e-6, in_exp)
                    torch.cuda.synchronize()
                    outs.append((y2.clone(), torch.ldexp(pk.kmajor_to_rows(y2.cpu()).double().sum(0), in_exp.cpu().double()[None, :])))
            same = torch.equal(_bits(outs[0][0]), _bits(outs[1][0]))
            v = outs[0][1]
            assert not torch.isnan(v).any(), "an element was not written"
            e = R.errors(v, ref, mag)
            name = f"layernorm_{'split3_' if form != 'f16x2' else ''}{form}_D{D}_rows{rows}"
            if D == 2048:
                _line(f"{name:54s} elem {e[0]:.2e} norm {e[1]:.2e} | bar float32_grade: pf_layernorm elem {base[0]:.2e} norm {base[1]:.2e}, caps {R.ELEM_CAP_GEMM:.1e} {R.NORM_CAP_GEMM:.1e} | repeat {same}")
                assert same and R.float32_grade(e, base, R.NORM_CAP_GEMM, R.ELEM_CAP_GEMM), (name, e, base)
            else:
                _line(f"{name:54s} elem {e[0]:.2e} norm {e[1]:.2e} | bar baseline_bar: restatement elem {restated[0]:.2e} norm {restated[1]:.2e} (pf_layernorm elem {base[0]:.2e} norm {base[1]:.2e}) | repeat {same}")
                assert same and I.baseline_bar(e, restated), (name, e, restated, base)


# ---------------- the linears: M = 1 and 17, K = one chunk, N = the smallest and the next ----------------
def _linear_operands(M, K, N, seed):
    g = torch.Generator().manual_seed(seed)
    w, b, x = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g), torch.randn(M, K, generator=g)
    return w, b, x


def _f32_linear(x, w, b, M, N):
    from patchfusion_amd import packing as pk
    y32 = _nan((M, N))
    _hip().conv(x.to(DEV), pk.pack_conv(w.view(N, -1, 1, 1), b, dtype=F32).to(DEV), y32, _direct=True)
    torch.cuda.synchronize()
    return y32


@pytest.mark.parametrize("N", [4, 8])
@pytest.mark.parametrize("M", [1, 17])
def test_linear_corners(monkeypatch, M, N):
    """pf_gemm_split3 (row-major and chunk-major planes in) and pf_gemm_f16x2 in both tile forms (PF_F16_TILE = 0: 192 x 192, 1: 160 x 256) at K = 32:
    rows past M come from a zero page (the tile kernels) or are clamped to row M - 1 (the persistent kernels), columns past N are never stored.
    Bar of tests/test_float32_grade_gpu.py: float32_grade against the f32-MFMA kernel."""
    from patchfusion_amd import packing as pk
    from tests import op_checks
    K = 32
    w, b, x = _linear_operands(M, K, N, M * 100 + N)
    ref, mag = R.linear_ref(x, w, b)
    base = R.errors(_f32_linear(x, w, b, M, N), ref, mag)
    runs = []
    pw3 = pk.pack_conv_split3(w, b, kmajor=True).to(DEV)
    x3 = torch.stack(pk.split3(x))
    for lay in ("rows", "kmaj"):
        xin = (pk.rows_to_kmajor(x3).contiguous() if lay == "kmaj" else x3).to(DEV)
        runs.append((f"gemm_split3_{lay}_in", None, lambda y, xin=xin: _hip().conv_split3(xin, pw3, y)))
    pwh = pk.pack_conv_f16x2(w, b, None, x.double().abs().amax(0)).to(DEV)
    x2 = pk.rows_to_kmajor(torch.stack(pk.split_f16x2(torch.ldexp(x.double(), -pwh.in_exp.cpu().double()[None, :]).float()))).contiguous().to(DEV)
    for tile in ("0", "1"):
        runs.append((f"gemm_f16x2_tile{'192' if tile == '0' else '160'}", tile, lambda y: _hip().conv_f16x2(x2, pwh, y)))
    for name, tile, launch in runs:
        if tile is not None:
            monkeypatch.setenv("PF_F16_TILE", tile)
        outs = []
        for _ in range(2):
            buf = _nan((M + 2, N + 4))
            op_checks._flush_caches()
            launch(buf[1:-1, :N])
            torch.cuda.synchronize()
            assert torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all() and torch.isnan(buf[:, N:]).all() and torch.isfinite(buf[1:-1, :N]).all(), "guards"
            outs.append(buf[1:-1, :N].clone())
        same = torch.equal(_bits(outs[0]), _bits(outs[1]))
        e = R.errors(outs[0], ref, mag)
        _line(f"{f'{name}_M{M}_K32_N{N}':54s} elem {e[0]:.2e} norm {e[1]:.2e} | bar float32_grade: f32 kernel elem {base[0]:.2e} norm {base[1]:.2e}, caps {R.ELEM_CAP_GEMM:.1e} {R.NORM_CAP_GEMM:.1e} | repeat {same}")
        assert same and R.float32_grade(e, base, R.NORM_CAP_GEMM, R.ELEM_CAP_GEMM), (name, e, base)


@pytest.mark.parametrize("N", [4, 8])
@pytest.mark.parametrize("M", [1, 17])
def test_conv1x1_split3_corners(monkeypatch, M, N):
    """the 1 x 1 split kernel on a 1 x M map: token rows past M are read from a zero page, weight rows past w3_rows likewise"""
    from patchfusion_amd import hip_ops
    from patchfusion_amd import packing as pk
    monkeypatch.setenv("PF_CONV1X1_SPLIT3", "2")
    hip_ops.refresh_env()
    try:
        w, b, x = _linear_operands(M, 32, N, M * 10 + N)
        ref, mag = R.linear_ref(x, w, b)
        base = R.errors(_f32_linear(x, w, b, M, N), ref, mag)
        pw = pk.pack_conv(w.view(N, 32, 1, 1), b, dtype=F32).to(DEV)
        xd = x.view(1, 1, M, 32).to(DEV)
        outs = []
        for _ in range(2):
            buf = _nan((1, 1, M, N + 8))
            y = buf[..., 4:4 + N]
            assert hip_ops.HipOps._conv_plan(xd, pw, y, 1, 0, None, False, None, None, None)[0] == "s3_1x1"
            _hip().conv(xd, pw, y)
            torch.cuda.synchronize()
            assert torch.isnan(buf[..., :4]).all() and torch.isnan(buf[..., 4 + N:]).all() and torch.isfinite(y).all(), "guards"
            outs.append(y.clone())
    finally:
        monkeypatch.undo()
        hip_ops.refresh_env()
    same = torch.equal(_bits(outs[0]), _bits(outs[1]))
    e = R.errors(outs[0].view(M, N), ref, mag)
    _line(f"{f'conv1x1_split3_M{M}_K32_N{N}':54s} elem {e[0]:.2e} norm {e[1]:.2e} | bar float32_grade: f32 kernel elem {base[0]:.2e} norm {base[1]:.2e}, caps {R.ELEM_CAP_GEMM:.1e} {R.NORM_CAP_GEMM:.1e} | repeat {same}")
    assert same and R.float32_grade(e, base, R.NORM_CAP_GEMM, R.ELEM_CAP_GEMM), (e, base)


@pytest.mark.parametrize("N", [4, 8])
@pytest.mark.parametrize("M", [1, 17])
def test_gemm_bf16_pp_corners(M, N):
    """the bf16 ping-pong linear (256 x 128 tiles) at K = 64, its one chunk: the engine sends it large token counts only, the entry point takes any;
    the plan of the direct route supplies the parameters"""
    from patchfusion_amd import hip_ops
    from patchfusion_amd import packing as pk
    _L, _p, _stream, check = _abi()
    w, b, x = _linear_operands(M, 64, N, M + N)
    w, x = w.to(BF16).float(), x.to(BF16).float()
    ref, mag = R.linear_ref(x, w, b)
    base = R.errors(_f32_linear(x, w, b, M, N), ref, mag)
    pw = pk.pack_conv(w.view(N, 64, 1, 1), b, dtype=BF16).to(DEV)
    xd = x.to(BF16).view(1, 1, M, 64).to(DEV)
    outs = []
    for _ in range(2):
        buf = _nan((1, 1, M, N + 16), BF16)
        y = buf[..., 8:8 + N]
        route, p, _ = hip_ops.HipOps._conv_plan(xd, pw, y, 1, 0, None, False, None, None, None)
        check(_L.pf_gemm_bf16_pp(C_byref(p), _stream()), "pf_gemm_bf16_pp")
        torch.cuda.synchronize()
        assert torch.isnan(buf[..., :8]).all() and torch.isnan(buf[..., 8 + N:]).all() and torch.isfinite(y).all(), "guards"
        outs.append(y.clone())
    same = torch.equal(_bits(outs[0]), _bits(outs[1]))
    e = R.bf16_excess(outs[0].view(M, N), ref, mag)
    _line(f"{f'gemm_bf16_pp_M{M}_K64_N{N}':54s} excess elem {e[0]:.2e} norm {e[1]:.2e} | bar bf16_grade: f32 kernel elem {base[0]:.2e} norm {base[1]:.2e} | repeat {same}")
    assert same and R.bf16_grade(e, base), (e, base)


# ---------------- Winograd: less than one tile, exactly one, one and a ragged one ----------------
WINO_ROUTES = [("fused", dict(PF_WINOGRAD="4", PF_WINOGRAD_MIN_PIXELS="0", PF_WINO_FUSED="2"), 32, 4),
               ("wino3", dict(PF_WINOGRAD="4", PF_WINOGRAD_MIN_PIXELS="0", PF_WINO_FUSED="0"), 128, 32),
               ("wino", dict(PF_WINOGRAD="4", PF_WINOGRAD_MIN_PIXELS="0", PF_WINO_FUSED="0", PF_WINO_SPLIT3="0"), 128, 32)]


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (4, 4), (5, 4)])
@pytest.mark.parametrize("route,sw,cin,cout", WINO_ROUTES, ids=[r[0] for r in WINO_ROUTES])
def test_winograd_corners(monkeypatch, route, sw, cin, cout, H, W):
    """the smallest channels each form is packed for (packing.pack_conv: fused from 32 -> 4, the three-step forms from 128 -> 32; the launchers
    themselves take Cin % 32 == 0, Cout % 8 == 0); the split three-step form runs in one window of 8 tiles.  The transforms
    skip tiles past T and pixels outside H x W, the batched product reads rows past T from a zero page.  The fp16x2 form does not qualify at these
    sizes (pf_conv_winograd_f16x2_supported: its product needs two rounds of tiles).  Bars of tests/test_float32_grade_gpu.py."""
    from patchfusion_amd import hip_ops
    from patchfusion_amd import packing as pk
    for k, v in sw.items():
        monkeypatch.setenv(k, v)
    hip_ops.refresh_env()
    try:
        c = (cin, cout, 3, 1, 1, 1, H, W)
        w, b, x, OH, OW, pix, ref, mag, _ = _conv_case(c, F32, 7)
        pw = pk.pack_conv(w, b, dtype=F32).to(DEV)
        xd = x.to(DEV)
        probe = _nan((1, H, W, cout + 16))[..., 8:8 + cout]
        assert hip_ops.HipOps._conv_plan(xd, pw, probe, 1, 1, None, False, None, None, None)[0] == route
        if route == "wino3":
            assert hip_ops.wino3_window(1, H, W, pw)[0] == 8
        got, same = _conv_run(xd, pw, 1, OH, OW, cout, F32, 1, 1, pix, None)
        e = R.errors(got, ref, mag)
        direct = R.errors(_conv_run(xd, pw, 1, OH, OW, cout, F32, 1, 1, pix, True)[0], ref, mag)
    finally:
        monkeypatch.undo()
        hip_ops.refresh_env()
    _line(f"{f'winograd_{route}_{cin}to{cout}_{H}x{W}':54s} elem {e[0]:.2e} norm {e[1]:.2e} | bar f64_ref caps: elem {R.ELEM_CAP_WINO:.1e} norm {R.NORM_CAP_WINO:.1e} | direct elem {direct[0]:.2e} norm {direct[1]:.2e} | repeat {same}")
    assert same and e[0] <= R.ELEM_CAP_WINO and e[1] <= R.NORM_CAP_WINO, (route, H, W, e)


# ---------------- the fp16x2 and the relative-position attention ----------------
@pytest.mark.parametrize("S", [1, 63, 64, 65])
def test_attention_f16x2_corners(S):
    """B = Hh = 1, planes of exactly B S Hh 192 / 64 elements; both output forms.  Bar of tests/test_attention_grade_gpu.py: at most twice the
    pipelined bf16x3 kernel on the same operands."""
    from patchfusion_amd import packing as pk
    from tests.test_attention_grade_gpu import _f16x2_exponents
    _L, _p, _stream, check = _abi()
    B, heads = 1, 1
    M, D = B * S, 64
    drawn = A.random(B, S, heads, 1.0, A.seed_of("corner16", S))
    exp, qk_exp = _f16x2_exponents(drawn, heads)
    q2 = torch.stack(pk.split_f16x2(torch.ldexp(drawn.double(), -exp.double()[None, :]).float())).contiguous()
    qkv = torch.ldexp(q2.double().sum(0), exp.double()[None, :]).float().to(DEV)
    q2, qk, ev = q2.to(DEV), qk_exp.to(DEV), exp[2 * D:].contiguous().to(DEV)
    assert q2.stride(0) == M * 192
    ref, mag = A.attention_ref(qkv, B, S, heads)
    q3 = torch.empty(3, M, 3 * D, dtype=BF16, device=DEV)
    _hip().split3(qkv, q3)
    o3 = _nan((3, M, D), BF16)
    check(_L.pf_vit_attention_split3_v2(_p(q3), q3.stride(0), _p(o3), o3.stride(0), 0, B, S, heads, 0, 0, _stream()), "v2")
    torch.cuda.synchronize()
    ybase = o3.cpu().double().sum(0)
    for form in ("fp16x2_out", "bf16x3_out"):
        planes3 = form == "bf16x3_out"
        outs = []
        for _ in range(2):
            o = _nan((3, D // 32, M, 32), BF16) if planes3 else _nan((2, D // 32, M, 32), torch.float16)
            check(_L.pf_vit_attention_f16x2(_p(q2), q2.stride(0), _p(qk), _p(o), o.stride(0), _p(ev) if planes3 else None, B, S, heads, _stream()), "f16x2")
            torch.cuda.synchronize()
            outs.append(o)
        y = pk.kmajor_to_rows(outs[0].cpu()).double().sum(0)
        if not planes3:
            y = torch.ldexp(y, exp[2 * D:].double()[None, :])
        _graded(f"vit_attention_f16x2_{form}_S{S}", y, ref, mag, ybase, torch.equal(_bits(outs[0]), _bits(outs[1])))


def test_attention_rpb_corner():
    """tw = 4, th = 1, S = 5 (cls + one row of four patches): the smallest grid the bf16 form takes too; 16 and 32 queries per wave, planes of exactly
    B S Hh 192 / 64 elements"""
    _L, _p, _stream, check = _abi()
    B, heads, th, tw = 1, 1, 1, 4
    S = 5
    M, D = B * S, 64
    qkv = A.random(B, S, heads, 1.0, A.seed_of("corner_rpb", S)).to(DEV)
    tab2 = A.rpb_table(th, tw, heads).to(DEV)
    bias = A.rpb_bias(tab2, th, tw)
    ref, mag = A.attention_ref(qkv, B, S, heads, bias)
    yb = A.restatement_f32(qkv, B, S, heads, bias)
    q3 = torch.empty(3, M, 3 * D, dtype=BF16, device=DEV)
    _hip().split3(qkv, q3)
    for qw in (16, 32):
        outs = []
        for _ in range(2):
            o = _nan((3, M, D), BF16)
            check(_L.pf_vit_attention_split3_rpb(_p(q3), q3.stride(0), _p(o), o.stride(0), 0, B, S, heads, _p(tab2), th, tw, qw, _stream()), "rpb")
            torch.cuda.synchronize()
            outs.append(o)
        _graded(f"vit_attention_split3_rpb_qw{qw}_th1_tw4_S5", outs[0].cpu().double().sum(0), ref, mag, yb, torch.equal(_bits(outs[0]), _bits(outs[1])))


def test_attention_rpb_bf16_corner():
    """pf_vit_attention_rpb_bf16 at tw = 4 (its lower limit), th = 1, S = 5, B = Hh = 1: one partial 128-query block (queries are clamped to row
    S - 1, stores guarded by qo < S), Sp = 64, a table slice of (0 + 1) * 7 + 3 entries (ntab = 10: the slice is the whole table); keys past S
    are masked and their bias gather is clamped into the slice.  Bar of tests/test_midas_core_bf16_gpu.py: PyTorch in bfloat16 on the same
    operands -- normwise and p99.9 at most twice, maximum at most four times its error against float64."""
    from tests.test_midas_core_bf16_gpu import _stats, _within
    B, heads, th, tw, S = 1, 1, 1, 4, 5
    D = 64
    g = torch.Generator().manual_seed(545)
    qkv = (torch.randn(B * S, 3 * D, generator=g) * 1.5).to(BF16).to(DEV)
    tab2 = A.rpb_table(th, tw, heads).to(DEV)
    bias = A.rpb_bias(tab2, th, tw).to(DEV)                                     # float64 [heads, S, S]

    def attn(xx, bb):
        q, k, v = xx.view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)
        a = (q * 0.125) @ k.transpose(-2, -1) + bb
        return (a.softmax(-1) @ v).transpose(1, 2).reshape(B * S, D)
    ref = attn(qkv.double(), bias)
    cmp = attn(qkv, bias.to(BF16))
    outs = []
    for _ in range(2):
        buf = _nan((S + 2, D), BF16)
        _hip().vit_attention_rpb_bf16(qkv, buf[1:-1], B, S, heads, tab2, th, tw)
        torch.cuda.synchronize()
        assert torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all() and torch.isfinite(buf[1:-1].float()).all(), "guards"
        outs.append(buf[1:-1].clone())
    same = torch.equal(_bits(outs[0]), _bits(outs[1]))
    e, c = _stats(outs[0], ref), _stats(cmp, ref)
    free = _stats(outs[0], attn(qkv.double(), torch.zeros_like(bias)))
    _line(f"{'vit_attention_rpb_bf16_th1_tw4_S5':54s} max {e[0]:.2e} p99.9 {e[1]:.2e} norm {e[2]:.2e} | bar within(2, 2, 4) x torch.bfloat16: max {c[0]:.2e} p99.9 {c[1]:.2e} "
          f"norm {c[2]:.2e} | from the bias-free reference norm {free[2]:.2e} | repeat {same}")
    assert same and _within(e, c), (same, e, c)


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (4, 4), (5, 4)])
def test_winograd_32_to_8_through_the_abi(H, W):
    """Cin = 32, Cout = 8: the smallest channels the three-step launchers take (the packer builds their filters from 128 -> 32 on, so the filters
    are transformed here with packing.winograd_filters): pf_conv_winograd (m = 4 and 2), pf_conv_winograd_split3, pf_conv_winograd_split3_windowed
    with window = 8 and its _ex form, whose maxima must be max |y| per channel bit for bit.  Bars of tests/test_float32_grade_gpu.py."""
    from patchfusion_amd import _lib
    from patchfusion_amd import packing as pk
    _L, _p, _stream, check = _abi()
    cin, cout, rows = 32, 8, 16
    c = (cin, cout, 3, 1, 1, 1, H, W)
    w, b, x, OH, OW, pix, ref, mag, _ = _conv_case(c, F32, 11)
    wk = torch.zeros(rows, 3, 3, cin)
    wk[:cout] = w.permute(0, 2, 3, 1)
    bp = torch.zeros(rows)
    bp[:cout] = b
    xd, bd = x.to(DEV), bp.to(DEV)
    U = {m: pk.winograd_filters(wk, m).to(DEV) for m in (2, 4)}
    U3 = torch.stack(pk.split3(U[4].cpu())).view(3, 36, rows, cin // 32, 32).permute(0, 1, 3, 2, 4).contiguous().to(DEV)

    def params(y):
        p = _lib.ConvParams()
        p.x, p.x_ld, p.B, p.H, p.W, p.Cin = xd.data_ptr(), cin, 1, H, W, cin
        p.bias = bd.data_ptr()
        p.y, p.y_ld, p.OH, p.OW, p.Cout = y.data_ptr(), cout + 16, H, W, cout
        p.KH = p.KW = 3
        p.stride = p.pad = p.shuffle = 1
        return p

    def run(name, launch):
        outs = []
        for _ in range(2):
            buf = _nan((1, H, W, cout + 16))
            y = buf[..., 8:8 + cout]
            extra = launch(params(y))
            torch.cuda.synchronize()
            assert torch.isnan(buf[..., :8]).all() and torch.isnan(buf[..., 8 + cout:]).all() and torch.isfinite(y).all(), "guards"
            outs.append((y.clone(), extra))
        same = torch.equal(_bits(outs[0][0]), _bits(outs[1][0]))
        e = R.errors(R.gather_pixels(outs[0][0], pix, cout), ref, mag)
        _line(f"{f'{name}_32to8_{H}x{W}':54s} elem {e[0]:.2e} norm {e[1]:.2e} | bar f64_ref caps: elem {R.ELEM_CAP_WINO:.1e} norm {R.NORM_CAP_WINO:.1e} | repeat {same}")
        assert same and e[0] <= R.ELEM_CAP_WINO and e[1] <= R.NORM_CAP_WINO, (name, e)
        return outs[0]

    for m in (4, 2):
        T = -(-H // m) * -(-W // m)
        a2 = (m + 2) ** 2
        V, M = _nan((a2 * T * cin,)), _nan((a2 * T * cout,))
        run(f"winograd_f32_m{m}", lambda p, m=m, V=V, M=M: check(_L.pf_conv_winograd(C_byref(p), m, _p(U[m]), rows, cin, _p(V), _p(M), _stream()), "wino"))
    V3, M3 = torch.zeros(3 * 36 * 8 * cin, dtype=BF16, device=DEV), _nan((36 * 8 * cout,))      # arenas of one window of 8 tiles (T <= 2 here)
    run("winograd_split3", lambda p: check(_L.pf_conv_winograd_split3(C_byref(p), _p(U3), rows, cin, _p(V3), _p(M3), _stream()), "split3"))
    run("winograd_split3_window8", lambda p: check(_L.pf_conv_winograd_split3_windowed(C_byref(p), _p(U3), rows, cin, _p(V3), _p(M3), 8, _stream()), "windowed"))

    def with_maxima(p):
        cm = torch.full((cout,), 0x7fffffff, dtype=torch.int32, device=DEV)                     # (the call zeroes it)
        check(_L.pf_conv_winograd_split3_windowed_ex(C_byref(p), _p(U3), rows, cin, _p(V3), _p(M3), 8, _p(cm), 0, _stream()), "windowed_ex")
        return cm
    y, cm = run("winograd_split3_window8_maxima", with_maxima)
    want = y.abs().amax(dim=(0, 1, 2)).contiguous().view(torch.int32)
    assert torch.equal(cm.cpu(), want.cpu()), "the merged maxima are not max |y| per channel"
