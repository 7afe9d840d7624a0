"""pytest -m gpu: the float32 instances of the small ViT producers (csrc/vit.hip) held to float64, element by element -- the float32 twins of
test_layernorm_bf16_against_float64 and test_patch_im2col_and_assemble_tokens_bf16_counted (tests/test_bf16_grade_gpu.py), which tests/op_checks.py
holds only to 1e-5 of max |y|.  Bars and metric of tests/f64_image_ref.py; every output is NaN-filled and every case prints one line (run with -s).

  * layernorm_kernel<float>: D = 32, 64, 384, 1024, 2048 (the kernel's limit), 2 x 89 rows plain and with the row remap (rows 1 .. 88 of each batch
    -> 88 rows out), x and y contiguous and as column slices of wider NaN buffers (x_ld = D + 16, y_ld = D + 24; the rest stays NaN); a zero-gamma
    channel is beta exactly; baseline_bar against the float32 restatement (tests/fake_ops.py) on the same operands.
    mag = (|x - mu| + |mu|) / sqrt(var + eps) |gamma| + |beta|.
  * patch_im2col_kernel<float>: v = (px - mean[c]) / std[c] -- one subtraction, one division: counted_bar k = 2, mag = (|px| + |mean|) / std, no
    storage rounding; columns 588 .. ld - 1 exactly 0; ld = 592 and ld = 588.
  * assemble_tokens_kernel<float>: one correctly rounded addition -- bit-equal to torch's float32 sum; S = 2 and S = 89.
  * qkv_split_kernel<float>: a copy (q times 2^-3, exact) -- bit-equal to the permuted view, V^T zero-padded to Sp; S = 13 and S = 1037 with the head
    counts of op_checks.vit_attention.  hip_ops reaches the kernel from ops.vit_attention on float32 rows only under PF_ATTN_QKV=0 (the default reads
    the QKV rows directly), on temporaries of its own: the test calls the library entry on NaN-filled buffers and shows that the route under the
    switch gives the bits of pf_qkv_split + pf_vit_attention."""
import os

import pytest
import torch

from tests import f64_image_ref as I
from tests.fake_ops import ops as fake

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
LOG = []
RAN = set()
WORST = {}
DONE = []

LN_D = (32, 64, 384, 1024, 2048)
QKV_SHAPES = ((2, 1037, 6), (1, 13, 16), (3, 13, 2))          # B, S, heads
REQUIRED = ({("layernorm", (D, remap, view)) for D in LN_D for remap in (False, True) for view in (False, True)}
            | {("patch_im2col", ld) for ld in (592, 588)} | {("assemble_tokens", S) for S in (2, 89)} | {("qkv_split", s) for s in QKV_SHAPES})


def _hip():
    from patchfusion_amd.hip_ops import ops
    return ops


def _log(line):
    print(line)
    LOG.append(line)


def _nan(shape):
    return torch.full(shape, NAN, device=DEV)


def _worst(op, ratio, case):
    if ratio > WORST.get(op, (-1.0, None))[0]:
        WORST[op] = (ratio, case)


@pytest.mark.parametrize("remap", [False, True], ids=["plain", "remap"])
@pytest.mark.parametrize("D", LN_D)
def test_layernorm_f32_against_float64(D, remap):
    DONE.append(1)
    g = torch.Generator().manual_seed(D)
    x = torch.randn(2 * 89, D, generator=g) * (0.5 + torch.rand(D, generator=g)) + torch.randn(D, generator=g)
    gamma, beta = torch.randn(D, generator=g) * 0.5, torch.randn(D, generator=g) * 0.2
    gamma[::7] = 0
    kw = dict(batches=2, in_rows_per_batch=89, in_row_offset=1, out_rows_per_batch=88) if remap else {}
    xs = x.double().view(2, 89, D)[:, 1:].reshape(-1, D) if remap else x.double()
    mu, var = xs.mean(1, keepdim=True), xs.var(1, unbiased=False, keepdim=True)
    rstd = 1.0 / (var + float(torch.tensor(1e-6, dtype=torch.float32))).sqrt()
    ref = (xs - mu) * rstd * gamma.double() + beta.double()
    mag = ((xs - mu).abs() + mu.abs()) * rstd * gamma.double().abs() + beta.double().abs()
    rows = xs.shape[0]
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    y32 = _nan((rows, D))
    fake.layernorm(xd, y32, gd, bd, 1e-6, **kw)
    base = I.errors(y32, ref, mag)
    for view in (False, True):
        xo, yo, x_ld, y_ld = (8, 16, D + 16, D + 24) if view else (0, 0, D, D)
        xw, yw = _nan((2 * 89, x_ld)), _nan((rows + 2, y_ld))
        xw[:, xo:xo + D] = xd
        xv, yv = xw[:, xo:xo + D], yw[1:-1, yo:yo + D]
        assert xv.stride(0) == x_ld and yv.stride(0) == y_ld
        _hip().layernorm(xv, yv, gd, bd, 1e-6, **kw)
        torch.cuda.synchronize()
        assert torch.isfinite(yv).all(), "an element of the output was not written"
        assert torch.isnan(yw[0]).all() and torch.isnan(yw[-1]).all() and torch.isnan(yw[:, :yo]).all() and torch.isnan(yw[:, yo + D:]).all(), \
            "written outside the output view"
        assert torch.isnan(xw[:, :xo]).all() and torch.isnan(xw[:, xo + D:]).all()
        assert torch.equal(yv[:, ::7].cpu(), beta[::7].expand(rows, -1)), "a zero-gamma channel is not beta"
        e = I.errors(yv, ref, mag)
        name = f"layernorm_f32_D{D}_{'remap' if remap else 'plain'}_{'slices' if view else 'contiguous'}"
        r = max(e[0] / max(base[0], I.FLOOR), e[1] / max(base[1], I.FLOOR))
        _log(f"{name:44s} rows {rows} elem {e[0]:.2e} norm {e[1]:.2e} | restatement elem {base[0]:.2e} norm {base[1]:.2e} | kernel / baseline {r:.2f}")
        assert I.baseline_bar(e, base), (name, e, base)
        _worst("layernorm", r, name)
        RAN.add(("layernorm", (D, remap, view)))


@pytest.mark.parametrize("ld", [592, 588])
def test_patch_im2col_f32_counted(ld):
    DONE.append(1)
    g = torch.Generator().manual_seed(1)
    img = torch.rand(2, 3, 112, 154, generator=g)
    img[0, :, :14, :14] = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1) + 1e-3 * torch.randn(3, 14, 14, generator=g)      # cancellation in px - mean
    col = _nan((2 * 88 + 2, ld))
    out = col[1:-1]
    _hip().patch_im2col(img.to(DEV), out)
    torch.cuda.synchronize()
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32).double().view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32).double().view(1, 3, 1, 1)
    im = lambda t: t.view(2, 3, 8, 14, 11, 14).permute(0, 2, 4, 3, 5, 1).reshape(2 * 88, 588)
    ref, mag = im((img.double() - mean) / std), im((img.double().abs() + mean) / std)
    assert torch.isnan(col[0]).all() and torch.isnan(col[-1]).all(), "written outside the output rows"
    assert bool((out[:, 588:] == 0).all()), "a padding column is not zero"
    ok, worst = I.counted_bar(out[:, :588], ref, mag, 2)
    yb = _nan((2 * 88, ld))
    fake.patch_im2col(img.to(DEV), yb)
    e, b = I.errors(out[:, :588], ref, mag), I.errors(yb[:, :588], ref, mag)
    _log(f"{f'patch_im2col_f32_ld{ld}':44s} elem {e[0]:.2e} norm {e[1]:.2e} | restatement elem {b[0]:.2e} norm {b[1]:.2e} | counted k=2: worst |d| / bound {worst:.3f}")
    assert ok, worst
    _worst("patch_im2col", worst, f"ld{ld}")
    RAN.add(("patch_im2col", ld))


@pytest.mark.parametrize("S", [2, 89])
def test_assemble_tokens_f32_bit_equal(S):
    DONE.append(1)
    D = 384
    g = torch.Generator().manual_seed(S)
    cls, pos = torch.randn(D, generator=g), torch.randn(S, D, generator=g)
    emb = torch.randn(2 * (S - 1), D, generator=g) * 3
    buf = _nan((2 * S * D + 32,))
    tok = buf[16:-16].view(2, S, D)
    _hip().assemble_tokens(emb.to(DEV), tok, cls.to(DEV), pos.to(DEV))
    torch.cuda.synchronize()
    assert torch.isnan(buf[:16]).all() and torch.isnan(buf[-16:]).all(), "written outside the tokens"
    want = torch.cat([cls.expand(2, 1, D), emb.view(2, S - 1, D)], 1) + pos
    same = torch.equal(tok.cpu(), want)
    _log(f"{f'assemble_tokens_f32_S{S}':44s} bit-equal {same}")
    assert same
    RAN.add(("assemble_tokens", S))


@pytest.mark.parametrize("B,S,heads", QKV_SHAPES, ids=[f"B{b}_S{s}_h{h}" for b, s, h in QKV_SHAPES])
def test_qkv_split_f32_bit_equal(B, S, heads):
    DONE.append(1)
    from patchfusion_amd import hip_ops
    from patchfusion_amd.hip_ops import _L, _p, _stream, check
    D = heads * 64
    qkv = torch.randn(B * S, 3 * D, generator=torch.Generator().manual_seed(S + heads))
    qkv.view(-1)[:6] = torch.tensor([-0.0, 0.0, 50.0, -50.0, 1e-30, -1e-30])
    qkv.view(-1)[-3:] = torch.tensor([2.0 ** -120, -7.0, 1.0])
    qd = qkv.to(DEV)
    Sp = (S + 63) // 64 * 64
    q, k, vt = _nan((B, heads, S, 64)), _nan((B, heads, S, 64)), _nan((B, heads, 64, Sp))
    check(_L.pf_qkv_split(_p(qd), B, S, heads, _p(q), _p(k), _p(vt), Sp, 0.125, 0, _stream()), "pf_qkv_split")
    torch.cuda.synchronize()
    qh, kh, vh = qkv.view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
    bits = lambda t: t.cpu().contiguous().view(torch.int32)
    same = (torch.equal(bits(q), bits(qh * 0.125)) and torch.equal(bits(k), bits(kh)) and torch.equal(bits(vt[..., :S]), bits(vh.transpose(-2, -1)))
            and torch.equal(bits(vt[..., S:]), torch.zeros(B, heads, 64, Sp - S, dtype=torch.int32)))
    # the route: ops.vit_attention on float32 rows takes this kernel only under PF_ATTN_QKV=0
    old = os.environ.get("PF_ATTN_QKV")
    os.environ["PF_ATTN_QKV"] = "0"
    hip_ops.refresh_env()
    try:
        routed = _nan((B * S, D))
        _hip().vit_attention(qd, routed, B, S, heads)
    finally:
        if old is None:
            os.environ.pop("PF_ATTN_QKV", None)
        else:
            os.environ["PF_ATTN_QKV"] = old
        hip_ops.refresh_env()
    direct = _nan((B * S, D))
    check(_L.pf_vit_attention(_p(q), _p(k), _p(vt), _p(direct), B, S, Sp, heads, 0, _stream()), "pf_vit_attention")
    torch.cuda.synchronize()
    route_same = torch.equal(bits(routed), bits(direct))
    _log(f"{f'qkv_split_f32_B{B}_S{S}_h{heads}':44s} bit-equal {same} | ops.vit_attention under PF_ATTN_QKV=0 gives the bits of the pair: {route_same}")
    assert same and route_same
    RAN.add(("qkv_split", (B, S, heads)))


def test_coverage():
    """every op and case of the list above was graded -- checked when the whole module ran; prints the worst ratios of the run"""
    assert len(REQUIRED) == 20 + 2 + 2 + 3
    for op, (ratio, case) in sorted(WORST.items()):
        _log(f"worst {op}: {ratio:.3f} at {case}")
    if len(DONE) >= 10 + 2 + 2 + 3:
        assert REQUIRED <= RAN, sorted(map(str, REQUIRED - RAN))
        assert RAN <= REQUIRED, sorted(map(str, RAN - REQUIRED))
