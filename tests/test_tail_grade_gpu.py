"""pytest -m gpu: the fused metric-bins tail (pf_bins_tail), the bin-centre kernels, the copy kernels and the mixed-dtype resize / RoI held to
float64, element by element (tests/f64_image_ref.py; references, bars, operands and planted defects are checked on the CPU in
tests/test_f64_image_ref_cpu.py).  Style of tests/test_image_grade_gpu.py: every output is NaN-filled, every element of the view must come out
finite and everything outside it must stay NaN, and every case prints one line with the kernel's and the baseline's errors (run with -s).

  * bins_tail: baseline_bar against fake_ops.bins_tail on the same operands on the GPU -- the path ends in exp / log at temperatures down to 0.02,
    so the roundings cannot be counted (the rule of logbinom_depth).  Finite everywhere, two launches bit-identical, `depth` inside a flat buffer
    with 16 NaN guard floats on each side, the embedding slice of the CLB buffer NaN (it must not be read).  The four HIP launches the kernel
    replaces are printed as a second baseline (information; tests/op_checks.py asserts them).
  * seed_bin_centers: the bounded combinations on baseline_bar, the baseline the larger of fake_ops' error and that of the float32 evaluation in
    the kernel's order on the CPU (torch sums the bins in vector lanes and is closer than ANY in-order walk: test_f64_image_ref_cpu.py);
    unbounded + normalize counted, k = 2 (difference, quotient); unbounded alone a copy, bit-equal.
  * bounded_bin_centers: non-decreasing, inside [lo, hi], counted k = 2 (product, sum) with the per-pixel mag.  The counted cases use ranges
    hi - lo that are float32 numbers (f64_image_ref.EXACT_RANGES): the rounding of the head's own 79.999 would be a third.
  * copy_channels, pack_fusion_input, nhwc_to_nchw, add_rowwise: bit-equal to torch (float32 -> bf16 round-to-nearest-even, bf16 -> float32
    exact, one float32 addition correctly rounded).
  * resize float32 -> bf16 and bf16 -> float32 (plain and add=) on the counted bar of the resize kernels, k = 6 / 7; roi_align in the same two
    modes on baseline_bar."""
import functools

import pytest
import torch

from tests import f64_image_ref as I
from tests import test_f64_image_ref_cpu as C
from tests.fake_ops import ops as fake

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
F32, BF16 = torch.float32, torch.bfloat16
LOG = []
RAN = set()                      # (op, case family) of everything that was graded: test_coverage
WORST = {}                       # op -> (ratio, case): the worst kernel / baseline (bins_tail) and |d| / bound (mixed resizes) of the run
DONE = []                        # the tests that ran
GUARD = 16

TAIL_VIEW_CASE = ("random_c168_2x37x50_ld176", "random", 168, (2, 37, 50), I.TAIL_EMB_GRID, I.TAIL_CEN_GRID)
TAIL_CASES = I.TAIL_CASES + [TAIL_VIEW_CASE]
SEED_COMBOS = ((True, True), (True, False), (False, True), (False, False))
BOUNDED_NPIX = (1, 5, 32773)                     # 32 773 = 8192 blocks x 4 waves + 5
BOUNDED_GRID_CAP = 16384 * 4 + 5                 # one more pass than the 16 384 blocks of csrc/imageops.hip grid_for cover, n_bins 64 only
REQUIRED = ({("bins_tail", f"shape_{'x'.join(map(str, s))}_c{c}") for s in I.TAIL_SHAPES for c in (168, 160)}
            | {("bins_tail", f"kind_{k}_c{c}") for k in I.TAIL_KINDS for c in (168, 160)}
            | {("bins_tail", f"grid_{g}_c{c}") for g in I.TAIL_GRIDS for c in (168, 160)} | {("bins_tail", "clb_view_ld176")}
            | {("seed_bin_centers", (nb, ld > nb, shape == (1, 1, 1), b, n)) for shape, nb, ld in C.SEED_SHAPES for b, n in SEED_COMBOS}
            | {("bounded_bin_centers", (nb, npix)) for nb in (64, 16, 63, 1) for npix in BOUNDED_NPIX} | {("bounded_bin_centers", (64, BOUNDED_GRID_CAP))}
            | {("copy_channels", (i, o, c)) for i in ("f32", "bf16") for o in ("f32", "bf16") for c in (8, 24)}
            | {(op, dt) for op in ("pack_fusion_input", "nhwc_to_nchw") for dt in ("f32", "bf16")}
            | {("add_rowwise", (dt, c)) for dt in ("f32", "bf16") for c in (8, 24)}
            | {("resize_mixed", (m, d, v)) for m in ("f32_to_bf16", "bf16_to_f32") for d in ("up", "down") for v in ("v2", "v1")}
            | {("roi_align_mixed", m) for m in ("f32_to_bf16", "bf16_to_f32")})


def _hip():
    from patchfusion_amd.hip_ops import ops
    return ops


def _log(line):
    print(line)
    LOG.append(line)


def _nan(shape, dt=F32):
    return torch.full(shape, NAN, dtype=dt, device=DEV)


def _tag(dt):
    return "bf16" if dt == BF16 else "f32"


def _written(buf, lo=0, hi=None):
    hi = buf.shape[-1] if hi is None else hi
    assert torch.isfinite(buf[..., lo:hi]).all(), "an element inside the view is not finite"
    assert torch.isnan(buf[..., :lo]).all() and torch.isnan(buf[..., hi:]).all(), "channels outside the view were written"


def _ratio(e, b):
    return max(e[0] / max(b[0], I.FLOOR), e[1] / max(b[1], I.FLOOR))


def _worst(op, ratio, case):
    if ratio > WORST.get(op, (-1.0, None))[0]:
        WORST[op] = (ratio, case)


def _line(case, e, b):
    return f"{case:44s} elem {e[0]:.2e} norm {e[1]:.2e} | baseline elem {b[0]:.2e} norm {b[1]:.2e}"


def _guarded(shape):
    """a float32 output of `shape` inside a flat NaN buffer with GUARD floats on each side -> (flat, view)"""
    n = 1
    for s in shape:
        n *= s
    flat = _nan((n + 2 * GUARD,))
    return flat, flat[GUARD:GUARD + n].view(shape)


def _guards_intact(flat):
    assert torch.isnan(flat[:GUARD]).all() and torch.isnan(flat[-GUARD:]).all(), "the kernel wrote outside its output"
    assert torch.isfinite(flat[GUARD:-GUARD]).all(), "an output element is not finite"


# ---------------- bins_tail ----------------
def _tail_family(case):
    name, kind, ctot, shp, eg, cg = case
    if case is TAIL_VIEW_CASE:
        return ["clb_view_ld176"]
    fam = []
    if (eg, cg) == (I.TAIL_EMB_GRID, I.TAIL_CEN_GRID):
        if kind == "random":
            fam.append(f"shape_{'x'.join(map(str, shp))}_c{ctot}")
        if shp == (2, 37, 50):
            fam.append(f"kind_{kind}_c{ctot}")
    for g, grids in I.TAIL_GRIDS.items():
        if (eg, cg) == grids and kind == "random":
            fam.append(f"grid_{g}_c{ctot}")
    return fam


@pytest.mark.parametrize("case", TAIL_CASES, ids=[c[0] for c in TAIL_CASES])
def test_bins_tail(case):
    DONE.append(1)
    name, kind, ctot, (B, H, W), eg, cg = case
    o = I.tail_operands(kind, ctot, B, H, W, eg, cg)
    ref, mag = I.tail_ref(o, H, W)
    tw = I.tail_pack(o).to(DEV)
    view = case is TAIL_VIEW_CASE
    clb = I.tail_clb(o, 176, 4, DEV) if view else I.tail_clb(o, device=DEV)
    assert torch.isnan(clb[..., 32:160]).all() and clb.stride(2) == (176 if view else ctot)
    emb, cen = o["emb"].to(DEV), o["centers"].to(DEV)
    hip = _hip()
    flat, depth = _guarded((B, H, W))
    hip.bins_tail(clb, emb, tw, cen, depth, I.MIN_TEMP, I.MAX_TEMP)
    torch.cuda.synchronize()
    _guards_intact(flat)
    flat2, again = _guarded((B, H, W))
    hip.bins_tail(clb, emb, tw, cen, again, I.MIN_TEMP, I.MAX_TEMP)
    yb = _nan((B, H, W))
    fake.bins_tail(clb, emb, tw, cen, yb, I.MIN_TEMP, I.MAX_TEMP)
    # the four launches the kernel replaces (PF_BINS_TAIL=0), as tests/op_checks.py bins_tail runs them
    packed = I.tail_pack(o)
    mlp0, mlp2 = packed.mlp0.to(DEV), packed.mlp2.to(DEV)
    buf = clb.clone()
    hip.resize(emb, buf[..., 32:160])
    t, pt, y4 = torch.zeros(B, H, W, 80, device=DEV), torch.zeros(B, H, W, 4, device=DEV), _nan((B, H, W))
    hip.conv(buf, mlp0, t, act="gelu")
    hip.conv(t, mlp2, pt, act="softplus")
    hip.logbinom_depth(pt, cen, y4, I.MIN_TEMP, I.MAX_TEMP)
    torch.cuda.synchronize()
    _guards_intact(flat2)
    e, b, f = I.errors(depth, ref, mag), I.errors(yb, ref, mag), I.errors(y4, ref, mag)
    r = _ratio(e, b)
    _log(f"{_line('bins_tail_' + name, e, b)} | four launches elem {f[0]:.2e} norm {f[1]:.2e} | kernel / baseline {r:.2f}")
    assert torch.equal(depth, again), "two launches differ"
    assert I.baseline_bar(e, b), (name, e, b)
    _worst("bins_tail", r, name)
    RAN.update(("bins_tail", fam) for fam in _tail_family(case))


# ---------------- seed_bin_centers ----------------
@pytest.mark.parametrize("shape,nb,ld", C.SEED_SHAPES, ids=[f"{'x'.join(map(str, s))}_nb{nb}_ld{ld}" for s, nb, ld in C.SEED_SHAPES])
def test_seed_bin_centers(shape, nb, ld):
    DONE.append(1)
    x = I.seed_operands(shape, nb, ld)
    xw = _nan((*shape, ld))
    xw[..., :nb] = x.to(DEV)
    xd = xw[..., :nb]                                      # x_ld = ld, NaN in the channels after the bins
    assert xd.stride(2) == ld
    hip = _hip()
    for bounded, normalize in SEED_COMBOS:
        name = f"seed_bin_centers_{'x'.join(map(str, shape))}_nb{nb}_ld{ld}_{'b' if bounded else 'u'}{'n' if normalize else '-'}"
        for lo, hi in ([C.HEAD_RANGE] if bounded or not normalize else I.EXACT_RANGES):
            ref, mag = I.seed_bin_centers_ref(x, nb, lo, hi, bounded, normalize)
            flat, y = _guarded((*shape, nb))
            hip.seed_bin_centers(xd, y, lo, hi, bounded, normalize)
            yb = fake.seed_bin_centers(xd, _nan((*shape, nb)), lo, hi, bounded, normalize)
            torch.cuda.synchronize()
            _guards_intact(flat)
            e = I.errors(y, ref, mag)
            if bounded:
                b = C.seed_baseline(x, nb, lo, hi, bounded, normalize, ref, mag, yb)
                _log(f"{_line(name, e, b)} (the larger of fake_ops and the in-order float32 walk)")
                assert I.baseline_bar(e, b), (name, e, b)
                assert bool((y[..., 1:] >= y[..., :-1]).all()), "bounded seed centres do not ascend"
            elif normalize:
                ok, worst = I.counted_bar(y, ref, mag, I.K_SEED_NORM)
                _log(f"{_line(f'{name}_{lo:g}_{hi:g}', e, I.errors(yb, ref, mag))} | counted k={I.K_SEED_NORM}: worst |d| / bound {worst:.2f}")
                assert ok, (name, lo, hi, worst)
            else:
                same = torch.equal(y.cpu(), x[..., :nb])
                _log(f"{name:44s} bit-equal {same}")
                assert same
        RAN.add(("seed_bin_centers", (nb, ld > nb, shape == (1, 1, 1), bounded, normalize)))


# ---------------- bounded_bin_centers ----------------
@pytest.mark.parametrize("npix,nb", [(p, nb) for nb in (64, 16, 63, 1) for p in BOUNDED_NPIX] + [(BOUNDED_GRID_CAP, 64)])
def test_bounded_bin_centers(npix, nb):
    DONE.append(1)
    b = I.bounded_operands(npix, nb)
    bd = b.to(DEV)
    hip = _hip()
    for lo, hi in I.EXACT_RANGES:
        ref, mag = I.bounded_bin_centers_ref(b, lo, hi)
        flat, y = _guarded(tuple(b.shape))
        hip.bounded_bin_centers(bd, y, lo, hi)
        yb = fake.bounded_bin_centers(bd, _nan(tuple(b.shape)), lo, hi)
        torch.cuda.synchronize()
        _guards_intact(flat)
        ok, worst = I.counted_bar(y, ref, mag, I.K_BOUNDED)
        name = f"bounded_bin_centers_npix{npix}_nb{nb}_{lo:g}_{hi:g}"
        _log(f"{_line(name, I.errors(y, ref, mag), I.errors(yb, ref, mag))} | counted k={I.K_BOUNDED}: worst |d| / bound {worst:.2f}")
        assert bool((y[..., 1:] >= y[..., :-1]).all()), "not sorted"
        lo32, hi32 = torch.tensor(lo, dtype=F32), torch.tensor(hi, dtype=F32)
        assert float(y.min()) >= float(lo32) and float(y.max()) <= float(hi32), "outside [lo, hi]"
        assert ok, (name, worst)
    RAN.add(("bounded_bin_centers", (nb, npix)))


# ---------------- copies ----------------
def _bit_equal(name, got, want):
    same = got.dtype == want.dtype and torch.equal(got.cpu(), want.cpu())
    _log(f"{name:44s} bit-equal {same}")
    assert same, name


@pytest.mark.parametrize("Cc", [8, 24])
@pytest.mark.parametrize("dout", [F32, BF16], ids=["to_f32", "to_bf16"])
@pytest.mark.parametrize("din", [F32, BF16], ids=["f32", "bf16"])
def test_copy_channels(din, dout, Cc):
    """3 x 5 x 7 = 105 pixels; x and y channel slices of wider buffers (x_ld = C + 16, y_ld = C + 24); a float32 x carries exact bf16 ties
    and values that round up into the next binade"""
    DONE.append(1)
    x = I.copy_operands((3, 5, 7, Cc), din)
    xw, yw = _nan((3, 5, 7, Cc + 16), din), _nan((3, 5, 7, Cc + 24), dout)
    xw[..., 8:8 + Cc] = x.to(DEV)
    _hip().copy_channels(xw[..., 8:8 + Cc], yw[..., 16:16 + Cc])
    torch.cuda.synchronize()
    _written(yw, 16, 16 + Cc)
    _bit_equal(f"copy_channels_{_tag(din)}_to_{_tag(dout)}_C{Cc}", yw[..., 16:16 + Cc], x.to(dout))
    RAN.add(("copy_channels", (_tag(din), _tag(dout), Cc)))


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_pack_fusion_input(dt):
    DONE.append(1)
    g = torch.Generator().manual_seed(41)
    cd, fd, crops = torch.rand(2, 1, 7, 9, generator=g), torch.rand(2, 7, 9, generator=g), torch.rand(2, 3, 7, 9, generator=g)
    e = I.bf16_edge_values()
    cd.view(-1)[:8], fd.view(-1)[-8:], crops.view(-1)[5:13] = e, e, e
    y = _nan((2, 7, 9, 8), dt)
    _hip().pack_fusion_input(cd.to(DEV), fd.to(DEV), crops.to(DEV), y)
    torch.cuda.synchronize()
    want = torch.cat([cd.view(2, 7, 9, 1), fd.view(2, 7, 9, 1), crops.permute(0, 2, 3, 1), torch.zeros(2, 7, 9, 3)], -1).to(dt)
    _bit_equal(f"pack_fusion_input_2x7x9_{_tag(dt)}", y, want)
    assert bool((y[..., 5:] == 0).all())
    RAN.add(("pack_fusion_input", _tag(dt)))


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_nhwc_to_nchw(dt):
    DONE.append(1)
    x = I.copy_operands((2, 5, 7, 24), dt)
    got = _hip().nhwc_to_nchw(x.to(DEV), Cc=13)
    torch.cuda.synchronize()
    _bit_equal(f"nhwc_to_nchw_2x5x7x24_Cc13_{_tag(dt)}", got, x[..., :13].float().permute(0, 3, 1, 2).contiguous())
    RAN.add(("nhwc_to_nchw", _tag(dt)))


@pytest.mark.parametrize("Cc", [8, 24])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_add_rowwise(dt, Cc):
    """x [3, 5, C] the channels [8, 8 + C) of a NaN-filled [3, 5, C + 16] (row stride C + 16), pos [5, C] float32, in place"""
    DONE.append(1)
    x, pos = I.copy_operands((3, 5, Cc), dt), I.copy_operands((5, Cc), F32, seed=32)
    wide = _nan((3, 5, Cc + 16), dt)
    wide[..., 8:8 + Cc] = x.to(DEV)
    _hip().add_rowwise(wide[..., 8:8 + Cc], pos.to(DEV))
    torch.cuda.synchronize()
    _written(wide, 8, 8 + Cc)
    _bit_equal(f"add_rowwise_3x5x{Cc}_{_tag(dt)}", wide[..., 8:8 + Cc], (x.float() + pos).to(dt))
    RAN.add(("add_rowwise", (_tag(dt), Cc)))


# ---------------- mixed-dtype resize and RoI ----------------
@functools.lru_cache(maxsize=None)
def _mixed_operands(case, din, dout):
    h, w, oh, ow, Cc = case
    x, add = I.features((2, h, w, Cc), h, din), I.features((2, oh, ow, Cc), w + 1, dout)
    refs = (I.bilinear_ref(x, oh, ow), I.bilinear_ref(x, oh, ow, add))
    x, add = x.to(DEV), add.to(DEV)
    b0, b1 = _nan((2, oh, ow, Cc), dout), _nan((2, oh, ow, Cc), dout)
    fake.resize(x, b0)
    fake.resize(x, b1, add=add)
    return x, add, refs, (b0.cpu(), b1.cpu())


@pytest.mark.parametrize("v2", ["1", "0"], ids=["v2", "v1"])
@pytest.mark.parametrize("din,dout", C.MIXED_MODES, ids=["f32_to_bf16", "bf16_to_f32"])
@pytest.mark.parametrize("case", C.MIXED_RESIZE_CASES, ids=["up", "down"])
def test_mixed_resize_counted(monkeypatch, case, din, dout, v2):
    DONE.append(1)
    monkeypatch.setenv("PF_RESIZE_V2", v2)
    h, w, oh, ow, Cc = case
    x, add, refs, base = _mixed_operands(case, din, dout)
    bf = dout == BF16
    mode = f"{_tag(din)}_to_{_tag(dout)}"
    name = f"resize_{'x'.join(map(str, case))}_{mode}_v{2 if v2 == '1' else 1}"
    buf = _nan((2, oh, ow, Cc + 16), dout)
    _hip().resize(x, buf[..., 8:8 + Cc])
    y = _nan((2, oh, ow, Cc), dout)
    _hip().resize(x, y, add=add)
    torch.cuda.synchronize()
    _written(buf, 8, 8 + Cc)
    _written(y)
    for nm, out, (ref, mag), k, yb in ((name, buf[..., 8:8 + Cc], refs[0], I.K_BILERP, base[0]), (name + "_add", y, refs[1], I.K_BILERP_ADD, base[1])):
        ok, worst = I.counted_bar(out, ref, mag, k, bf)
        _log(f"{_line(nm, I.errors(out, ref, mag), I.errors(yb, ref, mag))} | counted k={k}: worst |d| / bound {worst:.2f}")
        _worst("resize_" + mode, worst, nm)
        assert ok, (nm, worst)
    RAN.add(("resize_mixed", (mode, "up" if oh > h else "down", "v2" if v2 == "1" else "v1")))


@pytest.mark.parametrize("din,dout", C.MIXED_MODES, ids=["f32_to_bf16", "bf16_to_f32"])
def test_mixed_roi_align(din, dout):
    DONE.append(1)
    h, w, Cc = I.ROI_FEATS[1]
    f, rois = C.roi_operands(h, w, Cc, din, feat=False)
    ref, mag = I.roi_align_ref(f, rois, h, w, h / 112)
    f, rois = f.to(DEV), rois.to(DEV)
    buf, bb = _nan((5, h, w, 2 * Cc), dout), _nan((5, h, w, 2 * Cc), dout)
    _hip().roi_align(f, rois, buf[..., Cc:], h / 112, dtype=BF16)
    fake.roi_align(f, rois, bb[..., Cc:], h / 112)
    torch.cuda.synchronize()
    _written(buf, Cc, 2 * Cc)
    assert bool((buf[4, ..., Cc:] == 0).all()), "the RoI wholly outside the map is not zero"
    mode = f"{_tag(din)}_to_{_tag(dout)}"
    e, b = I.errors(buf[..., Cc:], ref, mag), I.errors(bb[..., Cc:], ref, mag)
    _log(_line(f"roi_align_{h}x{w}x{Cc}_{mode}", e, b))
    assert I.baseline_bar(e, b), (mode, e, b)
    RAN.add(("roi_align_mixed", mode))


def test_coverage():
    """every op and case family of the list above was graded -- checked when the whole module ran; prints the worst ratios of the run"""
    assert len({r for r in REQUIRED if r[0] == "bins_tail"}) == 10 + 12 + 6 + 1
    for op, (ratio, case) in sorted(WORST.items()):
        _log(f"worst {op}: {ratio:.3f} at {case}")
    if len(DONE) >= len(TAIL_CASES) + len(C.SEED_SHAPES) + 13 + 8 + 2 + 2 + 4 + 8 + 2:
        assert REQUIRED <= RAN, sorted(map(str, REQUIRED - RAN))
        assert RAN <= REQUIRED, sorted(map(str, RAN - REQUIRED))
