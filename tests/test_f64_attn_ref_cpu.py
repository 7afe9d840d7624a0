"""CPU checks of the float64 attention reference (tests/f64_attn_ref.py) and of the power of the bar of tests/test_attention_grade_gpu.py to fail a
kernel -- the instrument is proved before it is pointed at one, as tests/test_f64_ref_cpu.py does for the GEMM reference.

Agreement.  rpb_index equals tests/midas_beit_ref.py gen_relative_position_index; the one-hot inputs lead by more than 26 and their reference is
v[pi(i)] to 1e-11; the uniform inputs give the mean of V.

The bar accepts honest float32.  At every (shape, kind) pair of the GPU test with S <= 300, relative-position cases included, the float32
restatement passes f64_image_ref.baseline_bar against itself, and so do a float32 attention that walks the keys in blocks of 32 with an online
softmax (another summation order, the pipelined kernel's) and a float64 model of the split kernels (three bf16 planes per operand, the six leading
partial products, P as three planes of the float32 exp).

Planted faults.  Each is rejected by the element-wise bar on the kind named in FAULTS; `old` there records whether the bar of tests/op_checks.py,
max |y - ref| / max(1, max |ref|) <= 1.25 max(3e-6, the float32 attention's), accepts it (True = it would have gone unnoticed)."""
import pytest
import torch

from patchfusion_amd import packing as pk
from tests import f64_attn_ref as A
from tests import midas_beit_ref as mb

SMALL = [(s, k) for (s, k) in A.CASES if s[1] <= 300]
_CACHE = {}


def _case(shape, kind, grid=None):
    """qkv, bias (float64 or None), (ref, mag), the restatement and its errors -- computed once per case"""
    key = (shape, kind, grid)
    if key not in _CACHE:
        B, S, heads = shape
        qkv = A.build(kind, B, S, heads)
        bias = A.rpb_bias(A.rpb_table(*grid, heads), *grid) if grid else None
        ref, mag = A.attention_ref(qkv, B, S, heads, bias)
        y = A.restatement_f32(qkv, B, S, heads, bias)
        _CACHE[key] = (qkv, bias, ref, mag, y, A.errors(y, ref, mag))
    return _CACHE[key]


def _rpb_shape(B, grid):
    return (B, grid[0] * grid[1] + 1, A.RPB_HEADS)


# ---------------- float32 attention with planted faults ----------------
def attn32(qkv, B, S, heads, bias=None, keyw=None, block=None):
    """float32 torch attention.  keyw [S, S] (query, key): the weight a key's exponential is counted with (0 = ignored, 2 = counted twice).
    block = 32: the keys in blocks of 32 with an online softmax (running maximum, rescaled sum and output), the order of the pipelined kernel"""
    q, k, v = A._heads(qkv.float(), B, S, heads)
    a = (q * 0.125) @ k.transpose(-2, -1)
    if bias is not None:
        a = a + bias.float()[None]
    w = torch.ones(S, S) if keyw is None else keyw.float()
    if block is None:
        e = (a - a.amax(-1, keepdim=True)).exp() * w
        return A._rows((e @ v) / e.sum(-1, keepdim=True), B, S, heads)
    m = torch.full(a.shape[:-1] + (1,), -float("inf"))
    l, o = torch.zeros_like(m), torch.zeros_like(q)
    for j in range(0, S, block):
        aj = a[..., j:j + block]
        m2 = torch.maximum(m, aj.amax(-1, keepdim=True))
        e = (aj - m2).exp() * w[:, j:j + block]
        f = (m - m2).exp()
        l, o, m = l * f + e.sum(-1, keepdim=True), o * f + e @ v[..., j:j + block, :], m2
    return A._rows(o / l, B, S, heads)


def _planes(t):
    return [p.double() for p in pk.split3(t.float())]


KEPT = ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1))          # the six leading partial products of two three-plane operands


def split_model(qkv, B, S, heads, bias=None, drop=()):
    """float64 model of the split-precision kernels: q, k, v as three bf16 planes (exact), logits and P V as the six leading plane products
    summed in float64, P = the float32 exp(logit - row maximum) as three planes, normalised by the float64 sum of that float32 P.
    drop: 'qm_km' (the mid x mid logit product), 'p_low' / 'v_low' (every P V product with that plane)"""
    q, k, v = (_planes(t) for t in A._heads(qkv.float(), B, S, heads))
    a = sum(q[i] @ k[j].transpose(-2, -1) for i, j in KEPT if not ("qm_km" in drop and (i, j) == (1, 1))) * 0.125
    if bias is not None:
        a = a + bias[None]
    e = (a - a.amax(-1, keepdim=True)).exp().float()
    p = _planes(e)
    o = sum(p[i] @ v[j] for i, j in KEPT if not ("p_low" in drop and i == 2) and not ("v_low" in drop and j == 2))
    return A._rows(o / e.double().sum(-1, keepdim=True), B, S, heads)


def old_metric(y, ref):
    return float((y.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def old_bar_accepts(y, ref, y32):
    """tests/op_checks.py vit_attention_split3_v2, a torch float32 attention standing in for the f32-MFMA kernel"""
    return old_metric(y, ref) <= 1.25 * max(3e-6, old_metric(y32, ref))


# ---------------- agreement ----------------
@pytest.mark.parametrize("th,tw", A.RPB_GRIDS + [(24, 32), (1, 1), (1, 7), (7, 1)])
def test_rpb_index_is_generate_relative_position_index(th, tw):
    assert torch.equal(A.rpb_index(th, tw), mb.gen_relative_position_index(th, tw))


@pytest.mark.parametrize("th,tw", A.RPB_GRIDS)
def test_rpb_bias_is_the_table_gathered_and_divided_by_log2e(th, tw):
    tab = torch.randn(47 * 47 + 3, A.RPB_HEADS, generator=torch.Generator().manual_seed(1))
    want = mb.rel_pos_bias(tab, 24, th, tw).double()                       # [heads, S, S], float32 interpolation as packing does it
    got = A.rpb_bias(pk.beit_rel_pos_table(tab, 24, th, tw), th, tw)
    assert got.shape == want.shape and float((got - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max())   # two float32 roundings (x log2 e, stored)


@pytest.mark.parametrize("shape", [s for s in A.SHAPES if s[1] <= 300], ids=str)
def test_one_hot_selects_one_key_and_uniform_is_the_mean(shape):
    B, S, heads = shape
    qkv, pi = A.one_hot(B, S, heads, A.seed_of("one_hot", B, S, heads))
    assert torch.equal(qkv, A.build("one_hot", B, S, heads))
    assert A.one_hot_margin(qkv, B, S, heads) > 26.0
    ref, mag = A.attention_ref(qkv, B, S, heads)
    v = A._heads(qkv.double(), B, S, heads)[2]
    want = A._rows(torch.gather(v, 2, pi[..., None].expand(-1, -1, -1, 64)), B, S, heads)
    assert float((ref - want).abs().max()) <= 1e-11 and float((mag - want.abs()).abs().max()) <= 1e-11
    assert A.errors(A.restatement_f32(qkv, B, S, heads), ref, mag)[0] <= 1e-10
    qkv = A.build("uniform", B, S, heads)
    ref, mag = A.attention_ref(qkv, B, S, heads)
    v = A._heads(qkv.double(), B, S, heads)[2]
    assert float((ref - A._rows(v.mean(2, keepdim=True).expand_as(v), B, S, heads)).abs().max()) <= 1e-14


def test_wide_keeps_the_logits_and_spreads_the_columns():
    B, S, heads = 1, 257, 3
    qa, qb = A.build("wide", B, S, heads), A.random(B, S, heads, 1.0, A.seed_of("wide", B, S, heads))
    la, lb = ((q.double() @ k.double().transpose(-2, -1)) for q, k, _ in (A._heads(qa, B, S, heads), A._heads(qb, B, S, heads)))
    assert float((la - lb).abs().max()) <= 1e-4                            # (float32 rounding of the scaled channels)
    col = A.attention_ref(qa, B, S, heads)[1].amax(0)
    assert float(col.max() / col.min()) > 1e5


# ---------------- the bar accepts honest float32, at every small case of the GPU test ----------------
@pytest.mark.parametrize("shape,kind", SMALL, ids=lambda v: str(v))
def test_restatement_and_reorderings_pass_the_bar(shape, kind):
    B, S, heads = shape
    qkv, _, ref, mag, y, base = _case(shape, kind)
    assert A.baseline_bar(base, base)
    e = A.errors(attn32(qkv, B, S, heads, block=32), ref, mag)
    assert A.baseline_bar(e, base), (e, base)
    e = A.errors(split_model(qkv, B, S, heads), ref, mag)
    assert A.baseline_bar(e, base), (e, base)
    assert A.errors(attn32(qkv, B, S, heads), ref, mag) == pytest.approx(base, rel=0.5, abs=A.FLOOR)   # attn32 without a fault is the restatement


@pytest.mark.parametrize("B,grid,kind", A.RPB_CASES, ids=lambda v: str(v))
def test_restatement_and_reorderings_pass_the_bar_with_a_bias(B, grid, kind):
    shape = _rpb_shape(B, grid)
    S, heads = shape[1:]
    qkv, bias, ref, mag, y, base = _case(shape, kind, grid)
    assert A.baseline_bar(base, base)
    e = A.errors(attn32(qkv, B, S, heads, bias, block=32), ref, mag)
    assert A.baseline_bar(e, base), (e, base)
    e = A.errors(split_model(qkv, B, S, heads, bias), ref, mag)
    assert A.baseline_bar(e, base), (e, base)


# ---------------- planted faults ----------------
def _tail_queries(S):
    return slice((S - 1) // 128 * 128, S)


def _fault(name, shape, kind, grid):
    B, S, heads = shape
    qkv, bias, ref, mag, y32, base = _case(shape, kind, grid)
    if name in ("v_low", "p_low", "qm_km"):
        return split_model(qkv, B, S, heads, bias, drop=(name,))
    if name == "column":                                   # one column of one head scaled by 1 + 1e-4: the column with the smallest values
        y = y32.clone()
        y[:, int(mag.amax(0).argmin())] *= 1 + 1e-4
        return y
    w = torch.ones(S, S)
    if name == "last_key":                                 # the last key ignored for the queries of the last 128-query block
        w[_tail_queries(S), S - 1] = 0
    elif name == "last_row_twice":                         # row S - 1 counted twice: an unmasked clamped re-read
        w[:, S - 1] = 2
    elif name == "wave_share":                             # the key blocks 1 (mod 4) of the key-split tail block missing: one wave lost in the merge
        w[_tail_queries(S), (torch.arange(S) // 32) % 4 == 1] = 0
    elif name == "table_off_by_one":                       # one head reads its table one entry off
        tab = A.rpb_table(*grid, heads).clone()
        tab[1] = torch.roll(tab[1], 1)
        bias = A.rpb_bias(tab, *grid)
    elif name == "bias_base2":                             # the table's log2(e) not taken back out: the bias enters a base-e softmax as it is packed
        bias = bias * A.LOG2E
    else:
        raise ValueError(name)
    return attn32(qkv, B, S, heads, bias, keyw=w)


# name, shape, kind (the kind that rejects it), grid, old: does the bar of op_checks accept it?
FAULTS = [("v_low", (1, 257, 3), "random1", None, True), ("v_low", (1, 257, 3), "one_hot", None, False),
          ("p_low", (1, 257, 3), "random1", None, True),
          ("qm_km", (1, 257, 3), "random1", None, True), ("qm_km", (1, 257, 3), "random4hot", None, False),
          ("column", (1, 257, 3), "wide", None, True),
          ("last_key", (1, 257, 3), "uniform", None, False), ("last_key", (1, 288, 8), "one_hot", None, False),
          ("last_row_twice", (1, 257, 3), "uniform", None, False), ("last_row_twice", (1, 33, 1), "random1", None, False),
          ("wave_share", (1, 288, 8), "one_hot", None, False),
          ("table_off_by_one", (1, 141, 2), "random1.5", (10, 14), False),
          ("bias_base2", (1, 141, 2), "random1.5", (10, 14), False)]
OLD = {}


@pytest.mark.parametrize("name,shape,kind,grid,old", FAULTS, ids=lambda v: str(v))
def test_planted_fault_is_rejected(name, shape, kind, grid, old):
    _, _, ref, mag, y32, base = _case(shape, kind, grid)
    y = _fault(name, shape, kind, grid)
    e = A.errors(y, ref, mag)
    accepts = old_bar_accepts(y, ref, y32)
    OLD[(name, kind)] = accepts
    print(f"{name:17s} {str(shape):13s} {kind:10s} elem {e[0]:.2e} = {e[0] / max(base[0], A.FLOOR):8.1f} x baseline ({base[0]:.2e}) | old metric "
          f"{old_metric(y, ref):.2e}: {'accepted' if accepts else 'rejected'}")
    assert e[0] > 2 * max(base[0], A.FLOOR), "the element-wise bar accepts the fault"
    assert not A.baseline_bar(e, base)
    assert accepts == old, "what the old bar makes of this fault has changed"


def test_every_fault_of_the_list_is_planted():
    assert {f[0] for f in FAULTS} == {"v_low", "p_low", "qm_km", "column", "last_key", "last_row_twice", "wave_share", "table_off_by_one", "bias_base2"}
