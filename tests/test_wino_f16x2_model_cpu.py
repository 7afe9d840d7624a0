"""CPU model of the fp16x2 operands of the three-step Winograd GEMM (csrc/wino_f16x2.hip): the channel exponent e_c, the column exponent f_pn, the
h / l split and the three-product sum, bit for bit as the kernels define them (fp16 round-to-nearest-even, products exact in float32, float32
accumulation), against float64 and against a float32 GEMM of the same float32 operands.  Error measure: |y - exact| / sum_k |a||b|, per element."""
import numpy as np
import pytest

BT = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]],
              dtype=np.float64)


def clog2(a):
    """ceil(log2 a) for finite a > 0 (frexp: a = f 2^e, f in [0.5, 1))"""
    f, e = np.frexp(a)
    return np.where(f == 0.5, e - 1, e).astype(np.int64)


def chan_exp(m):
    """e_c = ceil(log2 m_c) + 7 - 15; 0 for an all-zero (or non-finite) channel"""
    ok = (m > 0) & np.isfinite(m)
    return np.where(ok, clog2(np.where(ok, m, 1.0)) - 8, 0)


def split(v):
    h = v.astype(np.float16)
    l = (v - h.astype(np.float32)).astype(np.float16)
    return h, l


def winograd_v(x):
    """x [T, 6, 6, C] float32 input tiles -> V [T, 36, C] = B^T d B (float64, rounded once to float32)"""
    v = np.einsum("ia,tabc,jb->tijc", BT, x.astype(np.float64), BT)
    return v.reshape(x.shape[0], 36, x.shape[3]).astype(np.float32)


def f16x2_gemm(V, U, m):
    """V [T, C] float32 (one transform point), U [C, N] float32, m [C] = channel maxima of the layer input -> y [T, N], plus the scaled planes"""
    e = chan_exp(m)
    vs = np.ldexp(V, -e[None, :]).astype(np.float32)
    us_full = U.astype(np.float64)
    nz = (U != 0) & np.isfinite(U)
    lg = np.where(nz, clog2(np.where(nz, np.abs(U), 1.0)) + e[:, None], np.iinfo(np.int64).min)
    mx = lg.max(axis=0)
    f = np.where(mx == np.iinfo(np.int64).min, 0, mx - 15)
    us = np.ldexp(us_full, e[:, None] - f[None, :]).astype(np.float32)
    vh, vl = split(vs)
    uh, ul = split(us)
    f32 = np.float32
    acc = vh.astype(f32) @ ul.astype(f32)
    acc += vl.astype(f32) @ uh.astype(f32)
    acc += vh.astype(f32) @ uh.astype(f32)
    return np.ldexp(acc, f[None, :]).astype(np.float32), (vs, vh, vl, us, uh, ul)


def rel_err(y, V, U):
    exact = V.astype(np.float64) @ U.astype(np.float64)
    den = np.abs(V).astype(np.float64) @ np.abs(U).astype(np.float64)
    return float(np.max(np.abs(y.astype(np.float64) - exact) / np.maximum(den, 1e-300)))


def case(kind, seed=0, T=384, C=288, N=160):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, 6, 6, C)).astype(np.float32)
    U = (rng.standard_normal((C, N)) / np.sqrt(9 * C)).astype(np.float32)
    if kind in ("wide", "zero"):
        s = 10.0 ** rng.uniform(-3, 3, C)                             # channels over six decades, weights compensating
        rows = 2.0 ** rng.uniform(0, 10, T)                           # and ten binades of spread over the tiles
        x = (x * s[None, None, None, :] * rows[:, None, None, None]).astype(np.float32)
        U = (U / s[:, None]).astype(np.float32)
    if kind == "zero":
        x[..., ::7] = 0.0
    if kind == "boundary":
        # channel 0 at the bound |V| = 100 m_c (B^T d B with d = m sign(B^T_0) sign(B^T_0)^T), m_c a power of two and just below one
        sg = np.sign(BT[0])
        x[0, :, :, 0] = np.outer(sg, sg)
        x[1, :, :, 1] = np.outer(sg, sg) * np.float32(1 - 2 ** -23)
        x[:, :, :, :2] = np.clip(x[:, :, :, :2], -1, 1)
        U[:, 0] = 2.0 ** -20                                           # a filter column whose scaled max lands exactly on 2^15
        U[:, 1] = np.float32(2.0 ** -20 * (1 - 2 ** -23))             # and just below it
    m = np.abs(x).reshape(-1, C).max(axis=0)
    return winograd_v(x), U, m


@pytest.mark.parametrize("kind", ["random", "wide", "zero", "boundary"])
def test_split_error_is_float32_class(kind):
    V, U, m = case(kind)
    worst16 = worst32 = 0.0
    for p in range(0, 36, 5):
        y16, _ = f16x2_gemm(V[:, p], U, m)
        y32 = (V[:, p] @ U).astype(np.float32)                          # float32 GEMM of the same operands
        worst16 = max(worst16, rel_err(y16, V[:, p], U))
        worst32 = max(worst32, rel_err(y32, V[:, p], U))
    assert np.isfinite(worst16) and worst16 <= 2 * worst32, (kind, worst16, worst32)


@pytest.mark.parametrize("kind", ["random", "wide", "zero", "boundary"])
def test_scaled_operands_stay_in_fp16_range_and_keep_22_bits_near_the_channel_max(kind):
    V, U, m = case(kind)
    e = chan_exp(m)
    assert np.all(np.abs(V) <= 100 * m[None, None, :] * (1 + 2 ** -20))           # the B^T row-sum bound the exponent relies on
    for p in range(36):
        _, (vs, vh, vl, us, uh, ul) = f16x2_gemm(V[:, p], U, m)
        assert np.all(np.abs(vs) < 2 ** 15) and np.all(np.abs(us) <= 2 ** 15)
        assert np.isfinite(vh).all() and np.isfinite(uh).all()
        for a, h, l in ((vs, vh, vl), (us, uh, ul)):
            cmax = np.abs(a).max(axis=0, keepdims=True)            # per channel of V, per column of U'
            near = np.abs(a) >= cmax * 2.0 ** -10
            resid = np.abs(a.astype(np.float64) - h.astype(np.float64) - l.astype(np.float64))
            assert np.all(resid[near] <= 2.0 ** -22 * np.abs(a[near])), (kind, p)
    if kind == "zero":
        assert np.all(e[::7] == 0)
    if kind == "boundary":
        assert e[0] == -8 and e[1] == -8                                  # m = 1 and m = 1 - 2^-23: ceil(log2 m) = 0
        _, (_, _, _, us, uh, _) = f16x2_gemm(V[:, 0], U, m)
        assert float(np.abs(us[:, 0]).max()) == 2.0 ** 15 and float(np.abs(uh[:, 0]).max()) == 2.0 ** 15
        assert 2.0 ** 14 < float(np.abs(us[:, 1]).max()) < 2.0 ** 15


def test_channel_exponent_rules():
    m = np.array([0.0, 1.0, 1.5, 2.0 ** -140, 3e38, np.inf, np.nan], dtype=np.float32)
    assert chan_exp(m).tolist() == [0, -8, -7, -148, 120, 0, 0]
