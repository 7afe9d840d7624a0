"""CPU model of the fp16x2 attention arithmetic (csrc/attn_split3.hip vit_attention_f16x2_pipe_kernel) against float64, and the static scale rules of
packing.vit_attn_f16x2_scales.  No GPU.

The model does what the kernel does, in torch: q / k / v as two fp16 planes of x / 2^e (h = fp16(x), l = fp16(x - h)), every product as hl + lh + hh in
float32, the base-2 online softmax over 32-key blocks with the deferred exponent reference (PSHIFT = 12 below the maximum it was taken from, moved when
a block's maximum exceeds it by more than 15), the probabilities split in registers the same way, O / l at the end."""
import math

import torch

from patchfusion_amd import packing as pk

PSHIFT, RESCALE = 12.0, 15.0
F16_MAX = 65504.0


def _split(v):
    h, l = pk.split_f16x2(v)
    return h.float(), l.float()


def _mm3(ah, al, bh, bl):
    """the three products, smallest first, float32 accumulation"""
    return (ah @ bl + al @ bh) + ah @ bh


def model_attention(q, k, v, eq, ek, ev):
    """q, k, v float32 [S, 64]; eq, ek int exponents per channel with eq + ek = E constant; ev per channel -> (out float64 [S, 64], max P-hat)"""
    S = q.shape[0]
    E = int((eq + ek)[0])
    assert bool(((eq + ek) == E).all())
    qh, ql = _split(torch.ldexp(q, -eq.float()))
    kh, kl = _split(torch.ldexp(k, -ek.float()))
    vh, vl = _split(torch.ldexp(v, -ev.float()))
    qscale = torch.tensor(0.125 * 1.4426950408889634, dtype=torch.float32) * 2.0 ** E
    m = torch.full((S,), -math.inf)
    l = torch.zeros(S)
    o = torch.zeros(S, 64)
    pmax = 0.0
    for j0 in range(0, S, 32):
        s = _mm3(qh, ql, kh[j0:j0 + 32].t(), kl[j0:j0 + 32].t())                # [S, <= 32] raw q-hat . k-hat
        mb = s.max(dim=1).values * qscale
        need = mb > m + RESCALE
        m_new = torch.where(need, mb - PSHIFT, m)
        a = torch.where(need, torch.exp2(m - m_new), torch.ones(S))
        p = torch.exp2(s * qscale - m_new[:, None])
        pmax = max(pmax, float(p.max()))
        ph, pl = _split(p)
        l = l * a + p.sum(1)
        o = o * a[:, None] + _mm3(ph, pl, vh[j0:j0 + 32], vl[j0:j0 + 32])
        m = m_new
    oh, ol = _split(o / l[:, None])                                             # the planes written: out / 2^ev
    return torch.ldexp((oh.double() + ol.double()), ev.double()), pmax


def _ref(q, k, v):
    q, k, v = q.double(), k.double(), v.double()
    return ((q * 0.125) @ k.t()).softmax(-1) @ v


def _exps(q, k, v):
    """per-channel exponents from the observed maxima, through the rule of vit_attn_f16x2_scales (paired q / k exponents)"""
    rq, rk, rv = (pk.bound_exponents(t.abs().amax(0).double()).long() for t in (q, k, v))
    E = int((rq + rk).max())
    eq = rq + (E - rq - rk) // 2
    return eq, E - eq, rv


def test_model_matches_float64_plain_and_large_logits():
    g = torch.Generator().manual_seed(0)
    for S, scale in ((1037, 1.0), (129, 6.0), (70, 3.0)):
        q, k, v = (torch.randn(S, 64, generator=g) * scale for _ in range(3))
        if S == 129:
            k[S - 29] *= 8.0                                 # one key far above the rest, late: the reference moves (rescale path)
        out, pmax = model_attention(q, k, v, *_exps(q, k, v))
        ref = _ref(q, k, v)
        den = max(1.0, float(ref.abs().max()))
        err = float((out - ref).abs().max()) / den
        f32 = ((q * 0.125) @ k.t()).softmax(-1) @ v          # plain float32 attention on the same operands: large logits cost float32 itself
        ef = float((f32.double() - ref).abs().max()) / den
        print(f"S={S} x{scale}: fp16x2 model {err:.2e}, float32 {ef:.2e}")
        assert err <= 1.25 * max(3e-6, ef), (S, scale, err, ef)     # the bar of op_checks.vit_attention_split3_v2
        assert pmax <= 2.0 ** RESCALE * (1 + 1e-5) < F16_MAX


def test_model_keeps_precision_over_six_decades_of_channel_scales():
    """tests/dynamic_range.py's transformation: q channel c x s_c, k channel c / s_c, v channel c x t_c -- paired exponents keep every product exact"""
    g = torch.Generator().manual_seed(1)
    S = 300
    q, k, v = (torch.randn(S, 64, generator=g) for _ in range(3))
    s = 10.0 ** (torch.rand(64, generator=g) * 6 - 3)
    t = 10.0 ** (torch.rand(64, generator=g) * 6 - 3)
    q2, k2, v2 = q * s, k / s, v * t
    out, _ = model_attention(q2, k2, v2, *_exps(q2, k2, v2))
    ref = _ref(q2, k2, v2)
    mag = ((q2.double() * 0.125) @ k2.double().t()).softmax(-1) @ v2.double().abs()
    assert float(((out - ref).abs() / mag).max()) < 3e-6


def test_dropped_low_plane_bound():
    """below P-hat = 2^-3 the low plane is subnormal: what the split drops is at most 2^-25 per key, S 2^-25 in all, against a row sum >= 2^PSHIFT"""
    p = torch.exp2(torch.linspace(-30, 15, 4001))
    h, l = _split(p)
    drop = (p.double() - h.double() - l.double()).abs()
    small = p < 2.0 ** -3
    assert float(drop[small].max()) <= 2.0 ** -25
    assert float((drop[~small] / p[~small].double()).max()) <= 2.0 ** -22
    assert 1037 * 2.0 ** -25 / 2.0 ** PSHIFT < 2.0 ** -24 / 4


def _weights(D, heads, seed, wide):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(3 * D, D, generator=g) / D ** 0.5
    b = torch.randn(3 * D, generator=g)
    if wide:
        s = 10.0 ** (torch.rand(D, generator=g) * 6 - 3)
        W[:D] *= s[:, None]; b[:D] *= s
        W[D:2 * D] /= s[:, None]; b[D:2 * D] /= s
        W[2 * D:] *= 10.0 ** (torch.rand(D, generator=g)[:, None] * 6 - 3)
    return W, b, pk.layernorm_bound(*_ln_params(D, seed))


def _ln_params(D, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(D, generator=g), torch.randn(D, generator=g) * 0.2


def test_scale_rules():
    D, heads = 256, 4
    for wide in (False, True):
        W, b, lnb = _weights(D, heads, 3, wide)
        sc = pk.vit_attn_f16x2_scales(W, b, lnb, heads)
        bound = pk.linear_bound(W, b, lnb)
        e = sc.out_exp.long()
        # every exponent covers its column bound: bound / 2^e <= 2^14
        assert bool((torch.ldexp(bound, -e.double()) <= 2.0 ** 14).all())
        # the product's exponent is constant along the contraction axis of QK^T, and it is what the kernel receives
        eq, ek = e[:D].reshape(heads, 64), e[D:2 * D].reshape(heads, 64)
        assert bool(((eq + ek) == sc.qk_exp.long()[:, None]).all())
        # ... and not larger than needed: some channel of every head has no surplus
        r = pk.bound_exponents(bound).long()
        assert bool(((r[:D] + r[D:2 * D]).reshape(heads, 64).max(1).values == sc.qk_exp.long()).all())
        # v: its own exponent per column, the smallest that covers the bound
        assert torch.equal(e[2 * D:], r[2 * D:])
        # the projection's in_exp is v's exponent, and v's bound holds for v rows made from ACTUAL LayerNorm outputs through W_v, hence for any convex
        # combination of them (softmax weights): |sum_j p_j v_jd| <= max_j |v_jd| <= v_bound_d <= 2^(in_exp_d + 14)
        pw = pk.pack_conv_f16x2(torch.randn(D, D), None, None, sc.v_bound)
        assert torch.equal(pw.in_exp.long(), e[2 * D:])
        assert torch.equal(sc.v_bound, bound[2 * D:])
        g = torch.Generator().manual_seed(9)
        gamma, beta = _ln_params(D, 3)
        x = torch.randn(50, D, generator=g, dtype=torch.float64) * 10.0 ** (torch.rand(50, 1, generator=g, dtype=torch.float64) * 4 - 2)
        x[0, 5] = 1e6                                        # a spike: one normalised entry close to sqrt(D - 1)
        hln = torch.nn.functional.layer_norm(x, (D,), gamma.double(), beta.double(), 1e-6)
        assert bool((hln.abs() <= lnb[None, :] * (1 + 1e-12)).all())
        vrows = hln @ W[2 * D:].double().t() + b[2 * D:].double()
        p = torch.rand(7, 50, generator=g, dtype=torch.float64) ** 8
        p = p / p.sum(1, keepdim=True)
        assert bool(((p @ vrows).abs() <= sc.v_bound[None, :] * (1 + 1e-12)).all())
        assert bool((torch.ldexp(sc.v_bound, -pw.in_exp.double()) <= 2.0 ** 14).all())
