"""pytest -m gpu: every float32 ViT attention kernel held to float64, element by element (tests/f64_attn_ref.py; the instrument itself is checked on
the CPU by tests/test_f64_attn_ref_cpu.py).

Kernels, through the C ABI (no environment switch decides what runs):
  pf_vit_attention_qkv, pf_qkv_split + pf_vit_attention          float32 MFMA                     baseline: the torch float32 restatement
  pf_vit_attention_split3 (v1), pf_vit_attention_split3_v2 with (queries per wave, schedule) = (16, 1), (32, 1), (0, 1), (32, 2), (0, 0),
  pf_vit_attention_qkv_split3, each row- and chunk-major           three bf16 planes                baseline: the larger of the restatement's and
                                                                                                    the f32-MFMA kernel's error on the same case
  pf_vit_attention_f16x2, both output forms                        two scaled fp16 planes           baseline: the pipelined bf16x3 kernel on the same
                                                                                                    operands (that kernel's "twice bf16x3" rule)
  pf_vit_attention_split3_rpb, 16 / 32 queries per wave, both
  layouts, grids 2x3, 10x14, 5x40, 40x5, 16x17, B = 1 and 3        three bf16 planes + bias table   baseline: the restatement with the float32 bias

Every output is filled with NaN first and must come back finite; two launches must agree bit for bit; schedule 1 of version 2 must equal version 1
bit for bit (the assertion of tests/op_checks.py, which stays).  Each kernel is graded with errors(y, ref, mag) against attention_ref on the
operand values it receives (the planes of ops.split3 sum to qkv exactly; the fp16x2 planes times their exponents are float32 values, and those are
the qkv of the case).  The bar is f64_image_ref.baseline_bar: element-wise and normwise error each at most twice the baseline's, the baseline
floored at 4 * 2^-24.  No constant of this file enters a bar.

Shapes and input kinds: f64_attn_ref.SHAPES / kinds_of (S below a key block, one key past a block, multiples of 64, one query past a 128-query
block, the key-split tail blocks of the pipelined kernel with 1 and with exactly 32 queries under both block orders, a 44-query tail, S = 1037).
The relative-position cases take the bias-free reference too: on the random inputs the output must be more than 100 baseline errors away from it
(on the one-hot inputs the winner leads by more than 26, so no bias of a std-1 table moves the output: there the case checks indices and masks).

One line per case is printed (-s); the table measured on an MI355X is profiles/attention_grade.log.  Worst element-wise error per kernel there,
all on the large-logit kind (scale 4, one key x 8: logits of several hundred) unless noted, next to its baseline's on the same case:
  pf_vit_attention_qkv 1.98e-5 (2.82e-5), pf_qkv_split + pf_vit_attention 3.09e-5 (2.82e-5), pf_vit_attention_qkv_split3 1.98e-5 (2.82e-5),
  version 1 and the two-phase schedule 6.76e-6 (4.13e-5), the pipelined schedule 1.99e-5 (2.82e-5),
  pf_vit_attention_f16x2 4.83e-7 (bf16x3 4.74e-7; B 3, S 64, N(0, 1)), pf_vit_attention_split3_rpb 1.00e-6 (2.64e-6; 16 x 17, B 3, N(0, 1.5^2)).
On the N(0, 1) kinds every kernel stays below 1e-6.  The case nearest its bar is pf_vit_attention_qkv at (3, 64, 4), N(0, 1): 0.83 of it.  No
kernel missed the bar, so no bound had to be derived from a count of roundings, and no kernel was changed."""
import pytest
import torch

from patchfusion_amd import packing as pk
from tests import f64_attn_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
V2 = ((16, 1), (32, 1), (0, 1), (32, 2), (0, 0))                 # (queries per wave, schedule) of pf_vit_attention_split3_v2
LAYOUTS = ("rows", "kmajor")
REQUIRED = ({("qkv_f32", None, "rows"), ("qkv_split+attention_f32", None, "rows")}
            | {("split3_v1", None, l) for l in LAYOUTS} | {("split3_v2", s, l) for s in V2 for l in LAYOUTS}
            | {("qkv_split3", None, l) for l in LAYOUTS} | {("f16x2", o, "kmajor") for o in ("fp16x2_out", "bf16x3_out")}
            | {("split3_rpb", qw, l) for qw in (16, 32) for l in LAYOUTS})
RAN = set()                    # (kernel, schedule, layout) of every launch that was graded: test_kernel_coverage
DONE = []                      # the cases that ran
_CACHE = {}


def _abi():
    from patchfusion_amd.hip_ops import _L, _p, _stream, check
    return _L, _p, _stream, check


def _log(name, e, base, extra=""):
    print(f"{name:58s} elem {e[0]:.2e} norm {e[1]:.2e} | baseline elem {base[0]:.2e} norm {base[1]:.2e}{extra}")


def _ident(shape, kind):
    return f"B{shape[0]}_S{shape[1]}_h{shape[2]}_{kind}"


def _both(a, b):
    """the larger of two baselines, component by component"""
    return max(a[0], b[0]), max(a[1], b[1])


def _out3(M, D, layout, planes=3, dtype=torch.bfloat16):
    return torch.full((planes, D // 32, M, 32) if layout == "kmajor" else (planes, M, D), NAN, dtype=dtype, device=DEV)


def _rows(o, layout):
    """output planes -> float64 [M, D] on the CPU (NaN stays NaN)"""
    o = o.cpu()
    return (pk.kmajor_to_rows(o) if layout == "kmajor" else o).double().sum(0)


def _same(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16)) if a.element_size() == 2 else torch.equal(a.view(torch.int32), b.view(torch.int32))


def _twice(launch, make):
    """two launches into NaN-filled outputs: bit-identical, and the first one's output"""
    a, b = make(), make()
    launch(a)
    launch(b)
    torch.cuda.synchronize()
    return a, _same(a, b)


def _f32_kernel(qkv, B, S, heads):
    _L, _p, _stream, check = _abi()
    return _twice(lambda o: check(_L.pf_vit_attention_qkv(_p(qkv), _p(o), B, S, heads, 0, _stream()), "pf_vit_attention_qkv"),
                  lambda: torch.full((B * S, heads * 64), NAN, device=DEV))


def _case(shape, kind):
    """qkv on the device, (ref, mag), the restatement's errors, the f32-MFMA kernel's output and errors -- once per case, never modified"""
    key = (shape, kind)
    if key not in _CACHE:
        B, S, heads = shape
        qkv = A.build(kind, B, S, heads).to(DEV)
        ref, mag = A.attention_ref(qkv, B, S, heads)
        base = A.errors(A.restatement_f32(qkv, B, S, heads), ref, mag)
        yf, same = _f32_kernel(qkv, B, S, heads)
        _CACHE[key] = (qkv, ref, mag, base, yf, same, A.errors(yf, ref, mag))
    return _CACHE[key]


# ---------------- the float32 MFMA kernels ----------------
@pytest.mark.parametrize("shape,kind", A.CASES, ids=lambda v: str(v).replace(" ", ""))
def test_f32_kernels_against_float64(shape, kind):
    _L, _p, _stream, check = _abi()
    B, S, heads = shape
    qkv, ref, mag, base, yf, same, ef = _case(shape, kind)
    name, bad = _ident(shape, kind), []
    _log(f"{name} qkv_f32", ef, base)
    RAN.add(("qkv_f32", None, "rows"))
    if not (same and A.baseline_bar(ef, base)):
        bad.append(("qkv_f32", same, ef, base))
    Sp = (S + 63) // 64 * 64
    q, k = (torch.full((B, heads, S, 64), NAN, device=DEV) for _ in range(2))
    vt = torch.full((B, heads, 64, Sp), NAN, device=DEV)
    check(_L.pf_qkv_split(_p(qkv), B, S, heads, _p(q), _p(k), _p(vt), Sp, 0.125, 0, _stream()), "pf_qkv_split")
    y, same2 = _twice(lambda o: check(_L.pf_vit_attention(_p(q), _p(k), _p(vt), _p(o), B, S, Sp, heads, 0, _stream()), "pf_vit_attention"),
                      lambda: torch.full((B * S, heads * 64), NAN, device=DEV))
    # the split itself is exact: q / 8, k, and v transposed with zero padding
    qh, kh, vh = A._heads(qkv, B, S, heads)
    assert torch.equal(q, qh * 0.125) and torch.equal(k, kh) and torch.equal(vt[..., :S], vh.transpose(-2, -1)) and not vt[..., S:].any()
    e = A.errors(y, ref, mag)
    _log(f"{name} qkv_split+attention_f32", e, base)
    RAN.add(("qkv_split+attention_f32", None, "rows"))
    if not (same2 and A.baseline_bar(e, base)):
        bad.append(("qkv_split+attention_f32", same2, e, base))
    DONE.append(("f32", shape, kind))
    assert not bad, bad


# ---------------- the split-precision kernels ----------------
@pytest.mark.parametrize("shape,kind", A.CASES, ids=lambda v: str(v).replace(" ", ""))
def test_split_kernels_against_float64(shape, kind):
    _L, _p, _stream, check = _abi()
    from patchfusion_amd.hip_ops import ops
    B, S, heads = shape
    M, D = B * S, heads * 64
    qkv, ref, mag, base, yf, _, ef = _case(shape, kind)
    base = _both(base, ef)
    name, bad = _ident(shape, kind), []
    q3 = torch.empty(3, M, 3 * D, dtype=torch.bfloat16, device=DEV)
    ops.split3(qkv, q3)
    assert torch.equal(q3.double().sum(0), qkv.double())             # the operands the split kernels receive are the qkv of the reference
    for layout in LAYOUTS:
        kmaj = int(layout == "kmajor")
        make = lambda: _out3(M, D, layout)
        runs = [("split3_v1", None, lambda o: check(_L.pf_vit_attention_split3(_p(q3), q3.stride(0), _p(o), o.stride(0), kmaj, B, S, heads, _stream()), "v1"))]
        runs += [("split3_v2", (qw, sc), lambda o, qw=qw, sc=sc: check(_L.pf_vit_attention_split3_v2(_p(q3), q3.stride(0), _p(o), o.stride(0), kmaj, B, S, heads,
                                                                                                 qw, sc, _stream()), "v2")) for qw, sc in V2]
        runs += [("qkv_split3", None, lambda o: check(_L.pf_vit_attention_qkv_split3(_p(qkv), _p(o), o.stride(0), kmaj, B, S, heads, _stream()), "qkv_split3"))]
        v1 = None
        for kernel, sched, launch in runs:
            o, same = _twice(launch, make)
            e = A.errors(_rows(o, layout), ref, mag)
            tag = kernel + ("" if sched is None else f"_qw{sched[0]}_sched{sched[1]}")
            extra = ""
            if kernel == "split3_v1":
                v1 = o
            if kernel == "split3_v2" and sched[1] == 1:                 # the two-phase schedule evaluates exactly version 1's operations
                eq = torch.equal(o.view(torch.int16), v1.view(torch.int16))
                extra = f" | identical to v1: {eq}"
                same = same and eq
            if kernel == "qkv_split3":                                  # the planes are the host split of the f32 kernel's output on this case
                eq = torch.equal(o.cpu(), _host_planes(yf, layout))
                extra = f" | planes of the f32 kernel's output: {eq}"
                same = same and eq
            _log(f"{name} {tag} {layout}", e, base, extra)
            RAN.add((kernel, sched, layout))
            if not (same and A.baseline_bar(e, base)):
                bad.append((tag, layout, same, e, base))
    DONE.append(("split", shape, kind))
    assert not bad, bad


def _host_planes(y, layout):
    p = torch.stack(pk.split3(y.cpu()))
    return pk.rows_to_kmajor(p) if layout == "kmajor" else p


# ---------------- the fp16x2 kernel ----------------
def _f16x2_exponents(qkv, heads):
    """the smallest per-column exponents that keep every value of the case inside fp16 with the 2^14 headroom of packing.bound_exponents
    (r_c = ceil(log2 max |column c|) - 14; an all-zero column counts as 1), q and k then sharing a head's surplus as packing.vit_attn_f16x2_scales
    does, so that eq[c] + ek[c] = E_h along the contraction -> out_exp int32 [3 D], qk_exp int32 [heads] (their per-head sum)"""
    D = heads * 64
    mx = qkv.abs().amax(0).double().cpu()
    mx = torch.where(mx > 0, mx, torch.ones_like(mx))
    m, e = torch.frexp(mx)
    r = (torch.where(m == 0.5, e - 1, e) - 14).long()
    assert bool((torch.ldexp(mx, -r) <= 2.0 ** 14).all()) and bool((torch.ldexp(mx, -r) > 2.0 ** 13).all())
    rq, rk = r[:D].reshape(heads, 64), r[D:2 * D].reshape(heads, 64)
    E = (rq + rk).max(dim=1).values
    eq = rq + (E[:, None] - rq - rk) // 2
    ek = E[:, None] - eq
    return torch.cat([eq.reshape(-1), ek.reshape(-1), r[2 * D:]]).to(torch.int32).contiguous(), E.to(torch.int32).contiguous()


@pytest.mark.parametrize("shape,kind", A.F16_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_f16x2_kernel_against_float64_within_twice_bf16x3(shape, kind):
    _L, _p, _stream, check = _abi()
    from patchfusion_amd.hip_ops import ops
    B, S, heads = shape
    M, D = B * S, heads * 64
    drawn = A.build(kind, B, S, heads)
    exp, qk_exp = _f16x2_exponents(drawn, heads)
    q2 = torch.stack(pk.split_f16x2(torch.ldexp(drawn.double(), -exp.double()[None, :]).float())).contiguous()
    assert float(q2[0].float().abs().max()) <= 2.0 ** 14
    hat = torch.ldexp(q2.double().sum(0), exp.double()[None, :])      # what the two planes hold: float32 values -- the qkv of this case
    qkv = hat.float().to(DEV)
    assert torch.equal(qkv.double().cpu(), hat)
    q2, qk, ev = q2.to(DEV), qk_exp.to(DEV), exp[2 * D:].contiguous().to(DEV)
    ref, mag = A.attention_ref(qkv, B, S, heads)
    q3 = torch.empty(3, M, 3 * D, dtype=torch.bfloat16, device=DEV)
    ops.split3(qkv, q3)
    o3 = _out3(M, D, "rows")
    check(_L.pf_vit_attention_split3_v2(_p(q3), q3.stride(0), _p(o3), o3.stride(0), 0, B, S, heads, 0, 0, _stream()), "v2")
    base = A.errors(_rows(o3, "rows"), ref, mag)
    name, bad = _ident(shape, kind), []
    for form in ("fp16x2_out", "bf16x3_out"):
        planes3 = form == "bf16x3_out"
        make = lambda: _out3(M, D, "kmajor", 3, torch.bfloat16) if planes3 else _out3(M, D, "kmajor", 2, torch.float16)
        o, same = _twice(lambda o: check(_L.pf_vit_attention_f16x2(_p(q2), q2.stride(0), _p(qk), _p(o), o.stride(0), _p(ev) if planes3 else None, B, S, heads,
                                                                  _stream()), "f16x2"), make)
        y = _rows(o, "kmajor")
        if not planes3:
            y = torch.ldexp(y, exp[2 * D:].double()[None, :])
        e = A.errors(y, ref, mag)
        _log(f"{name} f16x2 {form}", e, base, " (baseline: bf16x3 pipelined)")
        RAN.add(("f16x2", form, "kmajor"))
        if not (same and A.baseline_bar(e, base)):
            bad.append((form, same, e, base))
    DONE.append(("f16x2", shape, kind))
    assert not bad, bad


# ---------------- the relative-position kernel ----------------
@pytest.mark.parametrize("B,grid,kind", A.RPB_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_rpb_kernel_against_float64(B, grid, kind):
    _L, _p, _stream, check = _abi()
    from patchfusion_amd.hip_ops import ops
    th, tw = grid
    S, heads = th * tw + 1, A.RPB_HEADS
    M, D = B * S, heads * 64
    qkv = A.build(kind, B, S, heads).to(DEV)
    tab2 = A.rpb_table(th, tw).to(DEV)
    bias = A.rpb_bias(tab2, th, tw)
    ref, mag = A.attention_ref(qkv, B, S, heads, bias)
    free = A.attention_ref(qkv, B, S, heads)[0]
    base = A.errors(A.restatement_f32(qkv, B, S, heads, bias), ref, mag)
    q3 = torch.empty(3, M, 3 * D, dtype=torch.bfloat16, device=DEV)
    ops.split3(qkv, q3)
    assert torch.equal(q3.double().sum(0), qkv.double())
    name, bad = f"B{B}_grid{th}x{tw}_h{heads}_{kind}", []
    for qw in (16, 32):
        for layout in LAYOUTS:
            kmaj = int(layout == "kmajor")
            o, same = _twice(lambda o: check(_L.pf_vit_attention_split3_rpb(_p(q3), q3.stride(0), _p(o), o.stride(0), kmaj, B, S, heads, _p(tab2), th, tw, qw,
                                                                           _stream()), "rpb"), lambda: _out3(M, D, layout))
            y = _rows(o, layout)
            e, far = A.errors(y, ref, mag), A.errors(y, free, mag)[0]
            _log(f"{name} split3_rpb_qw{qw} {layout}", e, base, f" | from the bias-free reference {far:.2e}")
            RAN.add(("split3_rpb", qw, layout))
            applied = kind == "one_hot" or far > 100 * base[0]
            if not (same and A.baseline_bar(e, base) and applied):
                bad.append((qw, layout, same, e, base, far))
    DONE.append(("rpb", B, grid, kind))
    assert not bad, bad


def test_kernel_coverage():
    """every (kernel, schedule, layout) of the list above ran at least once -- checked when the whole module ran"""
    assert len(REQUIRED) == 2 + 2 + 10 + 2 + 2 + 4
    if len(DONE) >= 2 * len(A.CASES) + len(A.F16_CASES) + len(A.RPB_CASES):
        assert REQUIRED <= RAN, sorted(map(str, REQUIRED - RAN))
        assert RAN <= REQUIRED, sorted(map(str, RAN - REQUIRED))
