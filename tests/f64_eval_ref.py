"""Float64 references, operands, bars and planted defects of the kernels the project judges itself with (csrc/io.hip): depth_metrics_kernel (the 13 sums
of pf_depth_metrics), silog_sums_kernel / silog_finish_kernel (pf_silog_loss) and u8_bicubic_kernel (pf_u8_bicubic_to_f32).  Style and metric of
tests/f64_image_ref.py; used by tests/test_eval_grade_gpu.py, checked on the CPU by tests/test_f64_eval_ref_cpu.py.  No GPU needed.

The 13 sums.  0 count, 1-3 #(max(g/p, p/g) < 1.25^j), 4 sum |d|/g, 5 sum d^2/g, 6 sum d^2 (d = g - p), 7 sum (ln g - ln p)^2, 8 sum (ln p - ln g),
9 sum (ln p - ln g)^2, 10 sum |log10 g - log10 p|, 11 sum over the valid edge pixels of min over the 3 x 3 zero-filled shifts of |gt_shift - p|,
12 their count.  The kernel forms every term in float32 and adds the terms in float64 (2^14 .. 2^21 additions of 2^-53 relative each: below 2^-32 of
mag, not counted).

Exact sums.  On a prediction on the ground truth's own grid the terms of sums 0-6, 11, 12 use only + - * /, fabs, fmin, fmax: correctly rounded on
the device and in numpy alike, nothing a compiler could contract into a multiply-add, so the float32 terms are the same bits on both sides.  The
operands are chosen so that the float64 sum of those terms is exact in ANY order (budget(): 24 + band + ceil(log2 N) <= 52, band = the number of
binary exponents the non-zero terms span) and the kernel's sum must EQUAL the restatement's.  The same holds for a prediction at exactly half the
resolution (or with one dimension halved) whose values carry at most 10 significant bits: the source coordinates 0.5 (y + 0.5) - 0.5 are exact
fused or not, the weights are 1/4 and 3/4 and every product and sum of the blend is exact, contracted or not.  The counts (0-3, 12) are compared
with == in every case.

Counted sums.  |S - ref| <= K 2^-24 mag + spread, mag = the sum over the pixels of the magnitude m of the term.  g and p are the float32 operands
themselves on the same grid, so a rounding of d = g - p is relative to d and m is the term; each arithmetic rounding counts 1, each logf / log10f
L = L_LOG, a square doubles the relative error of what it squares:
  sum  4  |d| / g                     K = 2       subtraction, division                               m = |d| / g
  sum  5  d d / g                     K = 4       2 x the subtraction, product, division              m = d^2 / g
  sum  6  d d                         K = 3       2 x the subtraction, product                        m = d^2
  sum  7  (ln g - ln p)^2             K = 2L + 3  2 x (L on each logarithm + the difference), product  m = |e| (|ln g| + |ln p|), e = ln p - ln g
  sum  8  ln p - ln g                 K = L + 1   L on each logarithm, the difference                 m = |ln g| + |ln p|
  sum  9  (ln p - ln g)^2             K = 2L + 3  as sum 7                                            m = |e| (|ln g| + |ln p|)
  sum 10  |log10 g - log10 p|         K = L + 1   as sum 8                                            m = |log10 g| + |log10 p|
  sum 11  min |gt_shift - p|          K = 1       the subtraction (fabs and fmin are exact)           m = the term
L: the ROCm installation carries no accuracy table of the device library's logf / log10f (nothing under its documentation or headers states one),
so L_LOG = 4 for both, as agreed for that case.  The power of the bars does not rest on it: one mis-masked pixel moves a sum by mag / N.

The SILog sums.  g = fl(logf(fl(p + 1e-7f)) - logf(fl(t + 1e-7f))); the reference is ln(p + 1e-7f) - ln(t + 1e-7f) in float64 from the operands.  The
rounding of a logarithm's argument is an absolute 2^-24 on the logarithm, so m carries + 1 per logarithm:
  sum g       K = L + 1      L on each logarithm, the difference, the two arguments through the + 2   m = |ln p| + |ln t| + 2
  sum g^2     K = 2 (L + 1)  the square doubles it; the kernel squares in float64 (exact)             m = |g| (|ln p| + |ln t| + 2)
The loss is held by baseline_bar against the float32 torch restatement (oracle.pf_oracle.silog_loss on the CPU), that floored at 4 2^-24 |ref|.

Ragged resize ratios.  The kernel forms the source coordinate sy (y + 0.5) - 0.5 in float32; a compiler may fuse it into one multiply-add (the
product exact, one rounding) or not (the product rounded; the subtraction of 0.5 is then exact).  The two differ by an ulp of the coordinate in a
few rows and columns.  The reference evaluates all four combinations (rows, columns) of the two forms with a float64 blend, takes the midpoint of the
smallest and the largest prediction of a pixel as p, and widens the pixel's bound by eps_p = half their spread + K_BILERP 2^-24 sum_i w_i |v_i| (the
6 roundings of the float32 blend, f64_image_ref.K_BILERP), propagated through each term to first order: eps_p / g, 2 |d| eps_p / g, 2 |d| eps_p,
2 |e| eps_p / p (sums 7, 9), eps_p / p, eps_p / (p ln 10), eps_p (sum 11; a minimum of 1-Lipschitz functions; the clamp to [lo, hi] is 1-Lipschitz
too).  The counts stay exact: MetricRef.margin shows that no ratio comes closer to a threshold than 8 2^-24 + eps_p / p.

A NaN ground truth is invalid, but it still enters the soft-edge minimum of its eight neighbours: numpy's minimum propagates it (the reference's
np.minimum.reduce, oracle/io_oracle.soft_edge_error), so sum 11 is NaN when a valid edge pixel has one.  The case nan_gt_beside_edge holds that."""
import functools
import math

import numpy as np
import torch

from tests.f64_image_ref import FLOOR, K_BILERP, U            # noqa: F401

f32, f64 = np.float32, np.float64
INF = float("inf")
L_LOG = 4                                        # ulps of logf / log10f taken for the bars (see above)
COUNTS = (0, 1, 2, 3, 12)
EXACT_SUMS = (0, 1, 2, 3, 4, 5, 6, 11, 12)
K_SUM = {4: 2, 5: 4, 6: 3, 7: 2 * L_LOG + 3, 8: L_LOG + 1, 9: 2 * L_LOG + 3, 10: L_LOG + 1, 11: 1}
K_SILOG_G, K_SILOG_G2 = L_LOG + 1, 2 * (L_LOG + 1)
THRESHOLDS = (1.25, 1.5625, 1.953125)
LO, HI = 1e-3, 80.0
FORMS = ((False, False), (True, True), (False, True), (True, False))       # (rows fused, columns fused); the first two are what a compiler does


# ---------------- the resize of the metrics kernel (bilinear, align_corners=False, float32 coordinate) ----------------
def _taps(n_in, n_out, fused, align_corners=False):
    """-> i0, i1 (int64 [n_out]), l (float32 [n_out], exact): csrc/io.hip pred_at"""
    j = np.arange(n_out, dtype=f32)
    if align_corners:                                                        # planted defect
        c = (f32(n_in - 1) / f32(max(n_out - 1, 1))) * j
    else:
        s = f32(n_in) / f32(n_out)
        jh = j + f32(0.5)                                                    # exact
        if fused:
            c = (f64(s) * jh.astype(f64) - 0.5).astype(f32)                 # a 48-bit product, exact in float64, minus 0.5 (exact), rounded once
        else:
            c = s * jh - f32(0.5)
    assert c.dtype == f32
    c = np.maximum(c, f32(0))
    i0 = c.astype(np.int64)
    assert int(i0.max()) <= n_in - 1, "the kernel would read outside the prediction"
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, c - i0.astype(f32)


def resize32(pred, H, W, form=(False, False), align_corners=False):
    """the kernel's float32 blend, unfused, of pred [h, w] on the H x W grid"""
    if pred.shape == (H, W):
        return pred.copy()
    (y0, y1, ly), (x0, x1, lx) = _taps(pred.shape[0], H, form[0], align_corners), _taps(pred.shape[1], W, form[1], align_corners)
    ly, lx = ly[:, None], lx[None, :]
    hy, hx = f32(1) - ly, f32(1) - lx
    with np.errstate(invalid="ignore"):
        t0 = pred[y0][:, x0] * hx + pred[y0][:, x1] * lx
        t1 = pred[y1][:, x0] * hx + pred[y1][:, x1] * lx
        out = t0 * hy + t1 * ly
    assert out.dtype == f32
    return out


def resize64(pred, H, W, form):
    """-> (p, pmag) float64: the same taps and float32 weights, the blend in float64; pmag = sum_i w_i |v_i|"""
    if pred.shape == (H, W):
        return pred.astype(f64), np.abs(pred.astype(f64))
    (y0, y1, ly), (x0, x1, lx) = _taps(pred.shape[0], H, form[0]), _taps(pred.shape[1], W, form[1])
    ly, lx = ly.astype(f64)[:, None], lx.astype(f64)[None, :]
    out = []
    for v in (pred.astype(f64), np.abs(pred.astype(f64))):
        t0 = v[y0][:, x0] * (1 - lx) + v[y0][:, x1] * lx
        t1 = v[y1][:, x0] * (1 - lx) + v[y1][:, x1] * lx
        out.append(t0 * (1 - ly) + t1 * ly)
    return out[0], out[1]


def clamp(p, lo, hi, nan_to_hi=False, skip=False):
    """metric.py:100-103 in p's dtype: < lo -> lo, > hi -> hi (+inf too), nan -> lo"""
    if skip:
        return p
    q = p.copy()
    with np.errstate(invalid="ignore"):
        q[q < lo] = lo
        q[q > hi] = hi
    q[np.isnan(q)] = hi if nan_to_hi else lo
    return q


def soft_edge(p, g, radius=1, replicate=False):
    """min over the (2 r + 1)^2 shifts of g, zero-filled (replicate: planted defect), of |shift(g) - p| in p's dtype; NaN propagates (np.minimum)"""
    H, W = g.shape
    pad = np.pad(g, radius, mode="edge") if (replicate and radius) else np.pad(g, radius)
    out = None
    with np.errstate(invalid="ignore"):
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                d = np.abs(pad[radius - dy:radius - dy + H, radius - dx:radius - dx + W] - p)
                out = d if out is None else np.minimum(out, d)
    return out


def valid_mask(g, lo, hi, crop, extra, admit_hi=False):
    """g float32 [H, W]; lo, hi float32 -> bool [H, W]: lo < g < hi (NaN: invalid), rows [y0, y1) x columns [x0, x1), extra != 0"""
    H, W = g.shape
    with np.errstate(invalid="ignore"):
        m = (g > lo) & ((g <= hi) if admit_hi else (g < hi))
    y0, y1, x0, x1 = (max(int(v), 0) for v in crop)
    rect = np.zeros((H, W), bool)
    rect[y0:y1, x0:x1] = True
    m &= rect
    if extra is not None:
        m &= extra != 0
    return m


# ---------------- the float32 restatement (with planted defects) ----------------
DEFECTS = ("drop_pixel", "admit_hi", "le_threshold", "crop_y0", "crop_y1", "crop_x0", "crop_x1", "replicate_border", "radius0", "edges_at_invalid",
           "nan_to_hi", "align_corners", "no_clamp", "mask_ignored")


def terms32(c, form=(False, False), defect=None):
    """-> (terms float32 [13, n] over the valid pixels in raster order, valid bool [H, W]): the plain numpy restatement of the kernel's arithmetic
    (tests/fake_ops.py FakeOps.depth_metrics, term by term) on the case c (metric_cases()); defect: one of DEFECTS"""
    assert defect is None or defect in DEFECTS
    g = c["gt"]
    H, W = g.shape
    lo, hi = f32(c["lo"]), f32(c["hi"])
    crop = list(c["crop"])
    if defect and defect.startswith("crop_"):
        i = ("crop_y0", "crop_y1", "crop_x0", "crop_x1").index(defect)
        crop[i] += 1 if i in (0, 2) else -1
    valid = valid_mask(g, lo, hi, crop, None if defect == "mask_ignored" else c["extra"], admit_hi=defect == "admit_hi")
    if defect == "drop_pixel":
        valid.reshape(-1)[np.flatnonzero(valid)[valid.sum() // 2]] = False
    p = clamp(resize32(c["pred"], H, W, form, align_corners=defect == "align_corners"), lo, hi, nan_to_hi=defect == "nan_to_hi", skip=defect == "no_clamp")
    gv, pv = g[valid], p[valid]
    t = np.zeros((13, gv.size), f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        th = np.maximum(gv / pv, pv / gv)
        d = gv - pv
        lg, lp = np.log(gv), np.log(pv)
        e = lp - lg
        t[0] = 1
        for j, thr in enumerate(THRESHOLDS):
            t[1 + j] = (th <= f32(thr)) if (defect == "le_threshold" and j == 0) else (th < f32(thr))
        t[4], t[5], t[6] = np.abs(d) / gv, (d * d) / gv, d * d
        t[7], t[8], t[9] = (lg - lp) * (lg - lp), e, e * e
        t[10] = np.abs(np.log10(gv) - np.log10(pv))
    assert all(v.dtype == f32 for v in (th, d, lg, e))
    if c["edges"] is not None:
        me = (c["edges"] != 0) if defect == "edges_at_invalid" else (valid & (c["edges"] != 0))
        if defect == "edges_at_invalid":                                     # the edge pixels of the whole image, whatever the ground truth
            se = soft_edge(p, g)[me]
            extra_terms = np.zeros((13, se.size), f32)
            extra_terms[11], extra_terms[12] = se, 1
            return np.concatenate([t, extra_terms], 1), valid
        se = soft_edge(p, g, radius=0 if defect == "radius0" else 1, replicate=defect == "replicate_border")
        t[11] = np.where(me[valid], se[valid], f32(0))
        t[12] = me[valid]
    return t, valid


def sums_of(terms):
    with np.errstate(invalid="ignore"):
        return terms.astype(f64).sum(1)


def budget(terms_k):
    """24 + band + ceil(log2 N) of the non-zero float32 terms of one sum (0 when there is none): at most 52 -> every partial sum, in any order, is a
    float64 number (each term is a multiple of 2^(emin - 23) below 2^(emax + 1))"""
    v = np.abs(terms_k[(terms_k != 0) & np.isfinite(terms_k)].astype(f64))
    if v.size == 0:
        return 0
    e = np.frexp(v)[1]
    return 24 + int(e.max() - e.min() + 1) + int(math.ceil(math.log2(v.size)))


# ---------------- the float64 reference ----------------
class MetricRef:
    """ref, mag, bound [13] float64 (bound = K 2^-24 mag + the propagated eps_p; 0 for the counts), terms float32 [13, n] and valid [H, W] of the
    restatement (unfused coordinates), sums32 {form: [13]} the restatement's sums per coordinate form, n_forms_differ the number of valid pixels
    whose prediction depends on the form, margin the smallest distance of a ratio from a threshold in units of 2^-24 (after eps_p / p)"""


def depth_metrics_ref(c):
    g32 = c["gt"]
    H, W = g32.shape
    lo, hi = f32(c["lo"]), f32(c["hi"])
    valid = valid_mask(g32, lo, hi, c["crop"], c["extra"])
    same = c["pred"].shape == (H, W)
    forms = FORMS[:1] if same else FORMS
    ps = [resize64(c["pred"], H, W, f) for f in forms]
    pc = np.stack([clamp(p, f64(lo), f64(hi)) for p, _ in ps])
    p_lo, p_hi = pc.min(0), pc.max(0)
    p_all = 0.5 * (p_lo + p_hi)
    # a blend that float32 evaluates without a rounding (the half-grid predictions of 10 bits) carries no K_BILERP
    blend_exact = same or all(np.array_equal(resize32(c["pred"], H, W, f).astype(f64), p) for f, (p, _) in zip(forms, ps))
    eps_all = 0.5 * (p_hi - p_lo) + (0.0 if blend_exact else K_BILERP * U * np.stack([m for _, m in ps]).max(0))
    g_all = g32.astype(f64)
    g, p, eps = g_all[valid], p_all[valid], eps_all[valid]
    n = g.size
    r, m, prop = np.zeros((13, n)), np.zeros((13, n)), np.zeros((13, n))
    d = g - p
    lg, lp = np.log(g), np.log(p)
    e = lp - lg
    th = np.maximum(g / p, p / g)
    r[0] = 1
    for j, thr in enumerate(THRESHOLDS):
        r[1 + j] = th < thr
    r[4], r[5], r[6] = np.abs(d) / g, d * d / g, d * d
    r[7], r[8], r[9] = e * e, e, e * e
    r[10] = np.abs(np.log10(g) - np.log10(p))
    m[4], m[5], m[6] = r[4], r[5], r[6]
    m[7] = m[9] = np.abs(e) * (np.abs(lg) + np.abs(lp))
    m[8] = np.abs(lg) + np.abs(lp)
    m[10] = np.abs(np.log10(g)) + np.abs(np.log10(p))
    prop[4], prop[5], prop[6] = eps / g, 2 * np.abs(d) * eps / g, 2 * np.abs(d) * eps
    prop[7] = prop[9] = 2 * np.abs(e) * eps / p
    prop[8], prop[10] = eps / p, eps / (p * math.log(10.0))
    if c["edges"] is not None:
        me = (valid & (c["edges"] != 0))[valid]
        se = soft_edge(p_all, g_all)[valid]
        r[11] = m[11] = np.where(me, se, 0.0)
        r[12] = me
        prop[11] = np.where(me, eps, 0.0)
    R = MetricRef()
    with np.errstate(invalid="ignore"):
        R.ref, R.mag = r.sum(1), m.sum(1)
        R.bound = np.array([K_SUM.get(k, 0) * U * R.mag[k] + prop[k].sum() for k in range(13)])
    R.terms, R.valid = terms32(c, forms[0])[0], valid
    R.sums32 = {f: sums_of(terms32(c, f)[0]) for f in forms}
    R.n_forms_differ = int((p_hi > p_lo)[valid].sum())
    planted = np.isin(th, THRESHOLDS)                                        # float64 g / p of float32 operands: an exact 1.25 is a planted one
    rel = np.abs(th[~planted][None, :] / np.array(THRESHOLDS)[:, None] - 1) - (eps / p)[~planted][None, :] if (~planted).any() else np.array([INF])
    R.margin, R.n_planted = float(rel.min() / U), int(planted.sum())
    return R


def grade(S, R, exact):
    """S [13] float64 (the kernel's, or a defective restatement's) -> ratios [13]: the counts, and sums 4-6, 11 of an exact case, 0.0 when equal to
    the restatement's (both NaN counts as equal) and inf otherwise; a counted sum |S - ref| / bound (a bound of 0: equality with the reference).
    A sum passes when its ratio is at most 1."""
    S = np.asarray(S, f64)
    T = R.sums32[FORMS[0]]
    out = []
    for k in range(13):
        if k in COUNTS or (exact and k in EXACT_SUMS):
            same = S[k] == T[k] or (np.isnan(S[k]) and np.isnan(T[k]))
            out.append(0.0 if same else INF)
        elif np.isnan(R.ref[k]) or np.isnan(S[k]):
            out.append(0.0 if (np.isnan(R.ref[k]) and np.isnan(S[k])) else INF)
        elif R.bound[k] == 0:
            out.append(0.0 if S[k] == R.ref[k] else INF)
        else:
            out.append(abs(S[k] - R.ref[k]) / R.bound[k])
    return out


def form_probe(c):
    """the valid pixel of a ragged case whose float32 prediction differs most between the unfused and the fused coordinate -> (crop of that one
    pixel, {form name: its float32 term d d}, the gap in units of the blend's own rounding K_BILERP 2^-24 2 |d| p).  Sum 6 of a launch on that
    crop is the kernel's d d of that pixel: the form it lies nearest to is the form the device compiler chose."""
    g = c["gt"]
    H, W = g.shape
    lo, hi = f32(c["lo"]), f32(c["hi"])
    valid = valid_mask(g, lo, hi, c["crop"], c["extra"])
    pu, pf = (clamp(resize32(c["pred"], H, W, f), lo, hi) for f in FORMS[:2])
    gap = np.where(valid, np.abs(pu.astype(f64) - pf.astype(f64)), -1.0)
    y, x = np.unravel_index(int(gap.argmax()), gap.shape)
    d = {nm: (g[y, x] - p[y, x]) * (g[y, x] - p[y, x]) for nm, p in (("unfused", pu), ("fused", pf))}
    noise = K_BILERP * U * 2 * abs(float(g[y, x]) - float(pu[y, x])) * float(pu[y, x])
    return (int(y), int(y) + 1, int(x), int(x) + 1), d, abs(float(d["unfused"]) - float(d["fused"])) / noise


# ---------------- operands of the metrics cases ----------------
def base_gt(H=96, W=160, seed=0):
    """[3, 8] (eval_side_ref.metric_case's field), 3 % scattered zeros and a block of zeros; the four corners valid"""
    yy, xx = np.mgrid[0:H, 0:W].astype(f32)
    full = (4.0 + np.sin(xx / 13.0) * np.cos(yy / 9.0) + (xx > W // 2) * 3.0).astype(f32)
    gt = full.copy()
    gt[np.random.RandomState(seed).rand(H, W) < 0.03] = 0
    gt[20:30, 40:70] = 0
    for y in (0, -1):
        for x in (0, -1):
            gt[y, x] = full[y, x]
    return gt


def base_pred(h, w, seed, bits10=False):
    """[8.4, 32]; bits10: at most 10 significant bits (steps of 2^-6 below 16, of 2^-5 from there on)"""
    p = np.clip(8.4 + 23.6 * np.random.RandomState(seed).rand(h, w), 8.4, 32.0)
    if bits10:
        p = np.where(p < 16, np.round(p * 64) / 64, np.round(p * 32) / 32)
        p = np.clip(p, 8.40625, 32.0)
    return p.astype(f32)


def base_edges(gt, seed=1):
    """non-zero on the whole border ring; 8 % of the interior with values 1, 0.5, 2, -1; every pixel of the block of invalid ground truth"""
    H, W = gt.shape
    rs = np.random.RandomState(seed)
    e = np.where(rs.rand(H, W) < 0.08, rs.choice(np.array([1, 0.5, 2, -1], f32), (H, W)), f32(0)).astype(f32)
    e[0], e[-1], e[:, 0], e[:, -1] = 1, 1, 1, 1
    e[20:30, 40:70] = 1
    return e


PRED_SPECIALS = {"nan": ((40, 10), float("nan")), "pinf": ((41, 100), INF), "ninf": ((60, 30), -INF), "below_lo": ((70, 120), 5e-4),
                 "above_hi": ((80, 80), 100.0)}
THRESHOLD_PIXELS = (((50, 20), 5.0, 4.0), ((50, 90), 4.0, 5.0), ((52, 21), 6.25, 4.0), ((54, 95), 7.8125, 4.0))
GT_PIXELS = ((60, 50), (61, 100), (62, 60), (63, 110), (64, 70))          # == lo, == hi, NaN, just above lo, just below hi


BORDER_PIXELS = ((0, 0), (0, 159), (95, 0), (95, 159), (0, 77), (95, 31), (47, 0), (13, 159))


def _case(name, fam, gt, pred, edges, exact, crop=None, extra=None, lo=LO, hi=HI):
    H, W = gt.shape
    return dict(name=name, fam=fam, gt=np.ascontiguousarray(gt, f32), pred=np.ascontiguousarray(pred, f32),
                edges=None if edges is None else np.ascontiguousarray(edges, f32), exact=exact, crop=tuple(crop or (0, H, 0, W)),
                extra=None if extra is None else np.ascontiguousarray(extra, np.uint8), lo=lo, hi=hi)


def _gt_bounds(gt, pred, edges, lo, hi):
    gt, pred, edges = gt.copy(), pred.copy(), edges.copy()
    lo, hi = f32(lo), f32(hi)
    vals = (lo, hi, f32("nan"), np.nextafter(lo, f32(1e9)), np.nextafter(hi, f32(0)))
    for (y, x), v in zip(GT_PIXELS, vals):
        gt[y, x], pred[y, x] = v, 12.0
        edges[y - 1:y + 2, x - 1:x + 2] = 0                                 # no soft-edge minimum sees these values (nan_gt_beside_edge does)
    return gt, pred, edges


@functools.lru_cache(maxsize=None)
def metric_cases():
    """name -> case: dict(name, fam, gt, pred, edges, exact, crop, extra, lo, hi), float32 / uint8 numpy operands"""
    from patchfusion_amd.postprocess import crop_rectangle
    H, W = 96, 160
    gt, pred = base_gt(), base_pred(H, W, 10)
    for y, x in BORDER_PIXELS:                   # g > 2 p on the border: |0 - p| of a neighbour outside the image is the soft-edge minimum there
        gt[y, x], pred[y, x] = 7.5, 2.25 + 0.125 * ((y + x) % 3)
    edges = base_edges(gt)
    cs = [_case("plain", "same_grid", gt, pred, edges, True),
          _case("half_grid", "half_grid", gt, base_pred(48, 80, 11, True), edges, True),
          _case("ragged_up_37x50", "ragged_up", gt, base_pred(37, 50, 12), edges, False),
          _case("ragged_down_200x333", "ragged_down", gt, base_pred(200, 333, 16), edges, False),
          _case("one_dim_96x80", "one_dim", gt, base_pred(96, 80, 14, True), edges, True),
          _case("crop_garg", "crop_garg", gt, pred, edges, True, crop=crop_rectangle(H, W, True, False, "nyu")),
          _case("crop_eigen_kitti", "crop_eigen_kitti", gt, pred, edges, True, crop=crop_rectangle(H, W, False, True, "kitti")),
          _case("crop_eigen_other", "crop_eigen_other", gt, pred, edges, True, crop=crop_rectangle(H, W, False, True, "nyu")),
          _case("crop_empty", "crop_empty", gt, pred, edges, True, crop=(30, 30, 10, 100))]
    assert cs[-2]["crop"] == (45, 471, 41, 601)
    for nm, (y, x) in (("tl", (0, 0)), ("tr", (0, W - 1)), ("bl", (H - 1, 0)), ("br", (H - 1, W - 1))):
        cs.append(_case(f"crop_corner_{nm}", f"crop_corner_{nm}", gt, pred, edges, True, crop=(y, y + 1, x, x + 1)))
    rs = np.random.RandomState(3)
    cs.append(_case("mask_30pct", "mask_30pct", gt, pred, edges, True, extra=(rs.rand(H, W) >= 0.3)))
    cs.append(_case("mask_all_zero", "mask_all_zero", gt, pred, edges, True, extra=np.zeros((H, W))))
    # ground truth exactly at the bounds, NaN, just inside: at lo = 2, hi = 16 (float32 numbers; the terms stay in the band, so the image is exact) and
    # at the default bounds (g just above 1e-3 makes |d| / g 2e4: counted)
    g2, p2, e2 = _gt_bounds(gt, pred, edges, 2.0, 16.0)
    cs.append(_case("gt_bounds_2_16", "gt_bounds_exact", g2, p2, e2, True, lo=2.0, hi=16.0))
    g3, p3, e3 = _gt_bounds(gt, pred, edges, LO, HI)
    cs.append(_case("gt_bounds_default", "gt_bounds_default", g3, p3, e3, False))
    for i, (y, x) in enumerate(GT_PIXELS):
        cs.append(_case(f"gt_bounds_default_px{i}", "gt_bounds_pixel", g3, p3, e3, True, crop=(y, y + 1, x, x + 1)))
    e4 = e3.copy()
    y, x = GT_PIXELS[2]
    e4[y - 1:y + 2, x - 1:x + 2] = 1
    g4 = gt.copy()
    g4[y, x] = f32("nan")
    g4[y - 1, x - 1:x + 2], g4[y + 1, x - 1:x + 2], g4[y, x - 1], g4[y, x + 1] = 5.0, 5.5, 6.0, 4.5       # its eight neighbours valid edge pixels
    cs.append(_case("nan_gt_beside_edge", "nan_gt_beside_edge", g4, pred, e4, True))
    # predictions that the clamp moves, at valid pixels
    g5, p5 = gt.copy(), pred.copy()
    for (y, x), v in PRED_SPECIALS.values():
        g5[y, x], p5[y, x] = 5.0, v
    cs.append(_case("pred_special_all", "pred_special_all", g5, p5, edges, False))
    for nm, ((y, x), _) in PRED_SPECIALS.items():
        cs.append(_case(f"pred_special_{nm}", f"pred_special_{nm}", g5, p5, edges, True, crop=(y, y + 1, x, x + 1)))
    pc = p5.copy()
    for nm in ("nan", "pinf", "ninf"):
        pc[PRED_SPECIALS[nm][0]] = 20.0
    cs.append(_case("pred_outside_bounds", "pred_outside_bounds", g5, pc, edges, False))          # below lo and above hi only: the no-clamp defect
    # thresholds hit exactly
    g6, p6, e6 = gt.copy(), pred.copy(), edges.copy()
    for (y, x), gv, pv in THRESHOLD_PIXELS:
        g6[y, x], p6[y, x], e6[y, x] = gv, pv, 1
    cs.append(_case("thresholds_exact", "thresholds_exact", g6, p6, e6, True))
    # edges
    cs.append(_case("no_edges", "no_edges", gt, pred, None, True))
    cs.append(_case("edges_only_invalid", "edges_only_invalid", gt, pred, np.where(gt == 0, f32(1), f32(0)), True))
    for h, w in ((1, 1), (1, 7), (5, 1), (3, 3)):
        rs = np.random.RandomState(h * 10 + w)
        cs.append(_case(f"tiny_{h}x{w}", f"tiny_{h}x{w}", (3 + 5 * rs.rand(h, w)), base_pred(h, w, h + w), np.ones((h, w)), True))
    # more pixels than 8192 blocks x 256 threads: the grid-stride loop; 16 000 valid pixels anywhere and the last 300
    Hb, Wb = 1500, 1400
    rs = np.random.RandomState(5)
    gb, eb = np.zeros(Hb * Wb, f32), np.zeros(Hb * Wb, f32)
    idx = rs.choice(Hb * Wb - 300, 16000, replace=False)
    gb[idx] = 3 + 5 * rs.rand(idx.size)
    gb[-300:] = 3 + 5 * rs.rand(300)
    eb[idx[::4]], eb[-300:] = 1, 0.5
    cs.append(_case("grid_stride_1500x1400", "grid_stride", gb.reshape(Hb, Wb), np.maximum(base_pred(Hb, Wb, 15), f32(10)), eb.reshape(Hb, Wb), True))
    out = {c["name"]: c for c in cs}
    assert len(out) == len(cs)
    return out


@functools.lru_cache(maxsize=None)
def metric_ref(name):
    return depth_metrics_ref(metric_cases()[name])


METRIC_FAMILIES = ("same_grid", "half_grid", "ragged_up", "ragged_down", "one_dim", "crop_garg", "crop_eigen_kitti", "crop_eigen_other", "crop_empty",
                   "crop_corner_tl", "crop_corner_tr", "crop_corner_bl", "crop_corner_br", "mask_30pct", "mask_all_zero", "gt_bounds_exact",
                   "gt_bounds_default", "gt_bounds_pixel", "nan_gt_beside_edge", "pred_special_all", "pred_special_nan", "pred_special_pinf",
                   "pred_special_ninf", "pred_special_below_lo", "pred_special_above_hi", "pred_outside_bounds", "thresholds_exact", "no_edges",
                   "edges_only_invalid", "tiny_1x1", "tiny_1x7", "tiny_5x1", "tiny_3x3", "grid_stride")
# defect -> the case that must reject it
DEFECT_CASES = {"drop_pixel": "plain", "admit_hi": "gt_bounds_default", "le_threshold": "thresholds_exact", "crop_y0": "crop_garg", "crop_y1": "crop_garg",
                "crop_x0": "crop_garg", "crop_x1": "crop_garg", "replicate_border": "plain", "radius0": "plain", "edges_at_invalid": "plain",
                "nan_to_hi": "pred_special_all", "align_corners": "ragged_up_37x50", "no_clamp": "pred_outside_bounds", "mask_ignored": "mask_30pct"}


# ---------------- SILog ----------------
SILOG_DEFECTS = ("biased_variance", "beta_dropped", "nonstrict_lo", "nonstrict_hi", "no_eps_pred", "no_eps_target")
BETA = 0.15


def silog_ref(pred, target, lo=LO, hi=HI, beta=BETA):
    """pred, target float32 [n] -> dict(n, s1, s2 (float64 sums), m1, m2 (their magnitudes), loss): everything in float64 from the operands"""
    t32 = target.reshape(-1)
    with np.errstate(invalid="ignore"):
        v = (t32 > f32(lo)) & (t32 < f32(hi))
    p, t = pred.reshape(-1)[v].astype(f64), t32[v].astype(f64)
    e7 = float(f32(1e-7))
    lp, lt = np.log(p + e7), np.log(t + e7)
    g = lp - lt
    n = int(v.sum())
    w = np.abs(lp) + np.abs(lt) + 2
    out = dict(n=n, s1=float(g.sum()), s2=float((g * g).sum()), m1=float(w.sum()), m2=float((np.abs(g) * w).sum()), loss=0.0)
    if n > 1:
        mean = g.mean()
        out["loss"] = 10.0 * math.sqrt(((g - mean) ** 2).sum() / (n - 1) + float(f32(beta)) * mean * mean)
    return out


def silog32(pred, target, lo=LO, hi=HI, beta=BETA, defect=None):
    """the kernel's arithmetic in numpy: g in float32, the sums and the finish in float64 -> (n, s1, s2, loss float32)"""
    assert defect is None or defect in SILOG_DEFECTS
    t32, p32 = target.reshape(-1), pred.reshape(-1)
    with np.errstate(invalid="ignore"):
        v = ((t32 >= f32(lo)) if defect == "nonstrict_lo" else (t32 > f32(lo))) & ((t32 <= f32(hi)) if defect == "nonstrict_hi" else (t32 < f32(hi)))
    p, t = p32[v], t32[v]
    e7 = f32(1e-7)
    g = np.log(p if defect == "no_eps_pred" else p + e7) - np.log(t if defect == "no_eps_target" else t + e7)
    assert g.dtype == f32
    g = g.astype(f64)
    n, s1, s2 = float(v.sum()), float(g.sum()), float((g * g).sum())
    if n <= 1:
        return n, s1, s2, f32(0)
    mean = s1 / n
    var = max((s2 - s1 * s1 / n) / (n if defect == "biased_variance" else n - 1.0), 0.0)
    b = 1.0 if defect == "beta_dropped" else float(f32(beta))
    return n, s1, s2, f32(10.0 * math.sqrt(var + b * mean * mean))


def silog_torch32(pred, target, lo=LO, hi=HI, beta=BETA):
    """oracle.pf_oracle.silog_loss in float32 on the CPU -> float (the baseline of the loss); needs at least 2 valid targets"""
    from oracle import pf_oracle
    return float(pf_oracle.silog_loss(torch.from_numpy(pred.reshape(1, -1)), torch.from_numpy(target.reshape(1, -1)), lo, hi, beta))


def silog_grade(n, s1, s2, loss, R, base_loss=None):
    """-> ratios (count, sum g, sum g^2, loss): the count 0 / inf on equality, the sums |S - ref| / (K 2^-24 m), the loss |loss - ref| over
    2 max(|base - ref|, 4 2^-24 |ref|) (n <= 1: the loss must be exactly 0)"""
    def ratio(d, b):
        if not np.isfinite(d):
            return INF
        return 0.0 if d == 0 else (INF if b == 0 else d / b)
    out = [0.0 if n == R["n"] else INF, ratio(abs(s1 - R["s1"]), K_SILOG_G * U * R["m1"]), ratio(abs(s2 - R["s2"]), K_SILOG_G2 * U * R["m2"])]
    if R["n"] <= 1:
        out.append(0.0 if float(loss) == 0.0 else INF)
    else:
        out.append(ratio(abs(float(loss) - R["loss"]), 2 * max(abs(base_loss - R["loss"]), FLOOR * abs(R["loss"]))))
    return out


@functools.lru_cache(maxsize=None)
def silog_cases():
    """name -> (pred, target) float32, flat.  lo = 1e-3, hi = 80, beta = 0.15 throughout"""
    cs = {}
    for n in (255, 256, 257):
        rs = np.random.RandomState(n)
        t, p = (3 + 5 * rs.rand(n)).astype(f32), (8.4 + 23.6 * rs.rand(n)).astype(f32)
        t[3], t[4], t[5], t[-1] = f32(LO), f32(HI), f32("nan"), 7.5                    # both bounds exactly, NaN; the last element valid
        t[6], t[7] = np.nextafter(f32(LO), f32(1)), np.nextafter(f32(HI), f32(0))
        t[10:30] = 0
        cs[f"len{n}"] = (p, t)
    m = metric_cases()["plain"]
    cs["len15360_exact"] = (m["pred"].reshape(-1).copy(), m["gt"].reshape(-1).copy())
    n = 2100000
    rs = np.random.RandomState(7)
    t = np.zeros(n, f32)
    idx = rs.choice(n - 1, 2 ** 14 - 1, replace=False)
    t[idx] = 3 + 5 * rs.rand(idx.size)
    t[-1] = 6.0
    cs["len2100000"] = ((8.4 + 23.6 * rs.rand(n)).astype(f32), t)
    for k in (0, 1, 2):
        rs = np.random.RandomState(20 + k)
        t = np.zeros(257, f32)
        t[[100, 256][:k]] = [5.0, 7.0][:k]
        t[5] = f32("nan")
        cs[f"valid{k}"] = ((8.4 + 23.6 * rs.rand(257)).astype(f32), t)
    t = m["gt"].reshape(-1).copy()
    cs["const_ratio"] = ((2 * t).astype(f32), t)
    rs = np.random.RandomState(9)
    cs["near_lo"] = ((1.2e-3 + 0.8e-3 * rs.rand(15360)).astype(f32), (1.2e-3 + 0.8e-3 * rs.rand(15360)).astype(f32))
    return cs


SILOG_DEFECT_CASES = {"biased_variance": "len15360_exact", "beta_dropped": "len255", "nonstrict_lo": "len256", "nonstrict_hi": "len257",
                      "no_eps_pred": "near_lo", "no_eps_target": "near_lo"}


# ---------------- the bicubic image reader ----------------
# (H, W) -> (OH, OW)
BICUBIC_CASES = {"up_ragged": ((7, 9), (13, 31)), "down": ((40, 52), (17, 23)), "w1": ((5, 1), (9, 4)), "w2": ((5, 2), (9, 5)), "w3": ((5, 3), (9, 7)),
                 "w4": ((4, 4), (9, 9)), "h1": ((1, 6), (3, 11)), "oh1": ((6, 5), (1, 9)), "ow1": ((6, 5), (9, 1)), "identity": ((9, 11), (9, 11)),
                 "align_33x47": ((33, 47), (61, 83))}


def bicubic_image(H, W, seed=0):
    """random bytes [H, W, 3] uint8 with a row of 0 and a row of 255 (a single row: its two halves)"""
    img = np.random.RandomState(100 * H + W + seed).randint(0, 256, (H, W, 3)).astype(np.uint8)
    if H > 1:
        img[H // 2], img[-1] = 0, 255
    else:
        img[0, :W // 2], img[0, W // 2:] = 0, 255
    return img


def _cubic(t):
    A = -0.75
    c1 = lambda x: ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    c2 = lambda x: ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
    return [c2(t + 1.0), c1(t), c1(1.0 - t), c2((1.0 - t) + 1.0)]


def bicubic64(img, OH, OW, order=0):
    """float64 bicubic (A = -0.75, align_corners=True, border taps clamped) of img / 255.0 -> float32 [3, OH, OW].  order 0: torch's (the four
    horizontal taps first, each sum from tap 0 up); order 1: the vertical taps first, each sum from tap 3 down"""
    H, W, _ = img.shape
    v = img.astype(f64) / 255.0
    ry, rx = ((H - 1) / (OH - 1) if OH > 1 else 0.0) * np.arange(OH), ((W - 1) / (OW - 1) if OW > 1 else 0.0) * np.arange(OW)
    iy, ix = np.floor(ry).astype(np.int64), np.floor(rx).astype(np.int64)
    cy, cx = _cubic(ry - iy), _cubic(rx - ix)
    rows = [np.clip(iy - 1 + j, 0, H - 1) for j in range(4)]
    cols = [np.clip(ix - 1 + k, 0, W - 1) for k in range(4)]
    taps = range(4) if order == 0 else range(3, -1, -1)
    acc = None
    if order == 0:
        for j in taps:
            t = None
            for k in taps:
                o = v[rows[j]][:, cols[k]] * cx[k][None, :, None]
                t = o if t is None else t + o
            o = t * cy[j][:, None, None]
            acc = o if acc is None else acc + o
    else:
        for k in taps:
            t = None
            for j in taps:
                o = v[rows[j]][:, cols[k]] * cy[j][:, None, None]
                t = o if t is None else t + o
            o = t * cx[k][None, :, None]
            acc = o if acc is None else acc + o
    return np.ascontiguousarray(acc.astype(f32).transpose(2, 0, 1))


def bicubic_ref(img, OH, OW, reverse=False):
    """oracle.io_oracle.read_image_arith (torch double) -> float32 [3, OH, OW]; reverse: the planes in the order 2, 1, 0"""
    from oracle import io_oracle
    if OH == 1 or OW == 1:                       # read_image_arith squeezes a dimension of one away: its interpolation call, unsqueezed
        t = torch.nn.functional.interpolate(torch.tensor(img / 255.0).unsqueeze(0).permute(0, 3, 1, 2), (OH, OW), mode="bicubic", align_corners=True)
        r = t[0].permute(1, 2, 0).numpy()
    else:
        r = io_oracle.read_image_arith(img, (OH, OW))
    assert r.dtype == f64 and r.shape == (OH, OW, 3)
    r = np.ascontiguousarray(r.astype(f32).transpose(2, 0, 1))
    return np.ascontiguousarray(r[::-1]) if reverse else r


def close_f32(a, b, frac=1e-5):
    """the bar of tests/test_io_gpu.py _close_f32 -> (ok, largest ulp distance, share of elements off): at most 1 ulp on at most 1e-5 of the
    elements -- below 1e5 elements that is equality"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    ulp = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    ulp[np.abs(a.astype(f64) - b.astype(f64)) <= 1e-9] = 0
    return bool(ulp.max() <= 1 and (ulp > 0).mean() <= frac), int(ulp.max()), float((ulp > 0).mean())
