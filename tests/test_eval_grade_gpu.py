"""pytest -m gpu: the kernels the project judges itself with (csrc/io.hip) held to float64 -- pf_depth_metrics sum by sum, pf_silog_loss with its
three sums, pf_u8_bicubic_to_f32 element by element (tests/f64_eval_ref.py; references, operands, bars and planted defects are checked on the CPU in
tests/test_f64_eval_ref_cpu.py).  Style of tests/test_tail_grade_gpu.py: every output is NaN-filled inside a guarded buffer, and every case prints
one line (run with -s).

  * depth_metrics: the counts of every case, and sums 4-6 and 11 of every case declared exact (same grid, half grid of 10-bit values), EQUAL the
    float64 sums of the numpy restatement's float32 terms; every other sum within K 2^-24 mag (+ the coordinate spread and the blend's roundings on
    a ragged grid) of the float64 reference.  An exact case is launched twice: bit-identical.  A ragged case prints which form of the source
    coordinate (fused multiply-add or not) the kernel's sums lie nearest to.  Three images written into rows of one [4, 13] NaN buffer, as
    DepthEvaluator does, equal their standalone results and leave the fourth row NaN.
  * silog_loss_saved: the count equal, sum g and sum g^2 counted, the loss on baseline_bar against the float32 torch restatement; 0 and 1 valid
    pixel give exactly 0.0; pred = 2 target gives 10 sqrt(beta) ln 2, not NaN; two launches on the exact-sum operands give the same loss, count
    and sum g bit for bit (sum g^2 adds 48-bit squares, whose float64 sum depends on the order of the atomics in its last bits: 2^-40 relative).
  * u8_bicubic_to_f32: the bar of tests/test_io_gpu.py against the torch-double reference (below 1e5 elements: equality), both channel orders, the
    image at the very end of a byte buffer behind a guard pattern.

Measured on the MI355X (the record is in DESIGN.md): the kernel's coordinate is the fused form (sum 6 on the probe pixel of the 200 x 333 prediction
equals the fused restatement's d d, 4.3e-3 from the unfused one); worst |S - ref| / bound 0.33 (metrics, a one-pixel case), 0.22 (SILog loss), the
bicubic reader bit-equal at every case."""
import numpy as np
import pytest
import torch

from tests import f64_eval_ref as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
LOG = []
RAN = set()                      # (op, case family) of everything that was graded: test_coverage
WORST = {}                       # op -> (ratio, case)
DONE = []
GUARD = 16
BYTE_GUARD = 61                  # odd: the image starts on an odd address

METRIC_CASES = list(E.metric_cases())
SILOG_CASES = list(E.silog_cases())
EVALUATOR_ROWS = (("plain", 0), ("half_grid", 1), ("crop_garg", 3))
REQUIRED = ({("depth_metrics", f) for f in E.METRIC_FAMILIES} | {("depth_metrics", "evaluator_rows")} | {("silog_loss", n) for n in SILOG_CASES}
            | {("u8_bicubic", (n, r)) for n in E.BICUBIC_CASES for r in (False, True)})


def _hip():
    from patchfusion_amd.hip_ops import ops
    return ops


def _log(line):
    print(line)
    LOG.append(line)


def _worst(op, ratio, case):
    if ratio > WORST.get(op, (-1.0, None))[0]:
        WORST[op] = (ratio, case)


def _guarded(shape, dt):
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), NAN, dtype=dt, device=DEV)
    return flat, flat[GUARD:GUARD + n].view(shape)


def _guards_intact(flat):
    assert torch.isnan(flat[:GUARD]).all() and torch.isnan(flat[-GUARD:]).all(), "the kernel wrote outside its output"


# ---------------- depth_metrics ----------------
def _metric_operands(c):
    dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    return dev(c["gt"]), dev(c["pred"]), dev(c["edges"]), dev(c["extra"])


def _run_metrics(c, ops_dev, out=None):
    gt, pred, edges, extra = ops_dev
    flat = None
    if out is None:
        flat, out = _guarded((13,), torch.float64)
    _hip().depth_metrics(gt, pred, edges, c["lo"], c["hi"], c["crop"], out, extra)
    torch.cuda.synchronize()
    if flat is not None:
        _guards_intact(flat)
    return out


@pytest.mark.parametrize("name", METRIC_CASES)
def test_depth_metrics(name):
    DONE.append(1)
    c, R = E.metric_cases()[name], E.metric_ref(name)
    dev = _metric_operands(c)
    out = _run_metrics(c, dev)
    S = out.cpu().numpy()
    ratios = E.grade(S, R, c["exact"])
    counted = E.grade(S, R, False)
    form = ""
    if not c["exact"] and c["pred"].shape != c["gt"].shape:
        # one launch on the pixel where the two forms of the coordinate lie furthest apart: sum 6 is the kernel's d d there
        crop, dd, gap = E.form_probe(c)
        s6 = float(_run_metrics(dict(c, crop=crop), dev).cpu()[6])
        dist = {k: abs(s6 - float(v)) for k, v in dd.items()}
        nm = min(dist, key=dist.get) if gap > 4 else "indistinguishable"
        form = (f" | coordinate form at pixel ({crop[0]}, {crop[2]}): {nm} (|d d - unfused| {dist['unfused']:.3g}, |d d - fused| {dist['fused']:.3g},"
                f" gap {gap:.0f} blend roundings; {R.n_forms_differ} pixels differ)")
    _log(f"depth_metrics {name:26s} n {int(R.ref[0]):6d} {'exact  ' if c['exact'] else 'counted'} |S - ref| / bound "
         + " ".join(f"{r:.3f}" for r in counted) + form)
    assert max(ratios) <= 1.0, (name, ratios, S.tolist(), R.sums32[E.FORMS[0]].tolist())
    if c["fam"] in ("mask_all_zero", "crop_empty"):
        assert not S.any() and not np.signbit(S).any(), "no valid pixel: all 13 sums are +0.0"
    if c["fam"] in ("no_edges", "edges_only_invalid"):
        assert S[11] == 0 and S[12] == 0
    if c["fam"] == "nan_gt_beside_edge":
        assert np.isnan(S[11]) and S[12] == R.ref[12]
    if c["exact"]:
        again = _run_metrics(c, dev)
        k = list(E.EXACT_SUMS)
        assert np.array_equal(again.cpu().numpy()[k], S[k], equal_nan=True), "two launches differ"
    _worst("depth_metrics", max(r for r in counted if np.isfinite(r)), name)
    RAN.add(("depth_metrics", c["fam"]))


def test_depth_metrics_evaluator_rows():
    """DepthEvaluator hands the kernel a row of its [capacity, 13] buffer: rows 0, 1, 3 written, row 2 stays NaN, each row the standalone result.
    Every one of the 13 sums of these three cases is exact in any order (for the logarithmic sums: budget at most 51 on the restatement's terms,
    whose logarithms are within a few ulps of the kernel's), so the comparison is bit for bit."""
    DONE.append(1)
    flat, buf = _guarded((4, 13), torch.float64)
    alone = {}
    for name, row in EVALUATOR_ROWS:
        c, R = E.metric_cases()[name], E.metric_ref(name)
        assert all(E.budget(R.terms[k]) <= (52 if k in E.EXACT_SUMS else 51) for k in range(13))
        dev = _metric_operands(c)
        _run_metrics(c, dev, out=buf[row])
        alone[row] = _run_metrics(c, dev).clone()
    _guards_intact(flat)
    assert torch.isnan(buf[2]).all(), "an untouched row was written"
    for name, row in EVALUATOR_ROWS:
        same = torch.equal(buf[row], alone[row])
        _log(f"depth_metrics row {row} of [4, 13] ({name}) equals the standalone result: {same}")
        assert same, (name, buf[row].tolist(), alone[row].tolist())
    RAN.add(("depth_metrics", "evaluator_rows"))


# ---------------- silog ----------------
@pytest.mark.parametrize("name", SILOG_CASES)
def test_silog_loss(name):
    DONE.append(1)
    p, t = E.silog_cases()[name]
    R = E.silog_ref(p, t)
    pd, td = torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV)
    loss, ws = _hip().silog_loss_saved(pd, td, E.LO, E.HI, E.BETA)
    torch.cuda.synchronize()
    n, s1, s2 = ws.cpu().tolist()
    base = E.silog_torch32(p, t) if R["n"] > 1 else None
    ratios = E.silog_grade(n, s1, s2, float(loss), R, base)
    rest = E.silog_grade(*E.silog32(p, t), R, base)
    _log(f"silog_loss {name:16s} len {p.size:8d} valid {R['n']:6d} loss {float(loss):.9g} ref {R['loss']:.9g} | (count, sum g, sum g^2, loss) / bound "
         + " ".join(f"{r:.3f}" for r in ratios) + " | restatement " + " ".join(f"{r:.3f}" for r in rest))
    assert max(ratios) <= 1.0, (name, ratios)
    assert np.isfinite(float(loss))
    if R["n"] <= 1:
        assert float(loss) == 0.0
    if name == "len15360_exact":
        loss2, ws2 = _hip().silog_loss_saved(pd, td, E.LO, E.HI, E.BETA)
        torch.cuda.synchronize()
        assert torch.equal(loss, loss2) and torch.equal(ws[:2], ws2[:2]), "two launches differ"
        assert abs(float(ws[2]) - float(ws2[2])) <= 2.0 ** -40 * float(ws[2])
    _worst("silog_loss", max(ratios), name)
    RAN.add(("silog_loss", name))


# ---------------- bicubic ----------------
@pytest.mark.parametrize("reverse", [False, True], ids=["rgb", "reversed"])
@pytest.mark.parametrize("name", list(E.BICUBIC_CASES))
def test_u8_bicubic(name, reverse):
    DONE.append(1)
    (H, W), (OH, OW) = E.BICUBIC_CASES[name]
    img = E.bicubic_image(H, W)
    ref = E.bicubic_ref(img, OH, OW, reverse)
    buf = torch.full((BYTE_GUARD + H * W * 3,), 0xA5, dtype=torch.uint8, device=DEV)
    buf[BYTE_GUARD:] = torch.from_numpy(img.reshape(-1)).to(DEV)
    src = buf[BYTE_GUARD:].view(H, W, 3)                   # the image ends on the buffer's last byte
    flat, out = _guarded((3, OH, OW), torch.float32)
    _hip().u8_bicubic_to_f32(src, out, reverse_channels=reverse)
    torch.cuda.synchronize()
    _guards_intact(flat)
    assert torch.isfinite(out).all(), "an output element was not written"
    assert bool((buf[:BYTE_GUARD] == 0xA5).all())
    y = out.cpu().numpy()
    ok, ulp, share = E.close_f32(y, ref)
    _log(f"u8_bicubic {name:12s} {H}x{W} -> {OH}x{OW} {'reversed' if reverse else 'rgb     '} largest ulp distance {ulp} on a share of {share:.2e}"
         f" | bit-equal {np.array_equal(y, ref)}")
    assert ok, (name, ulp, share)
    if name == "identity":
        assert np.array_equal(y, ref)
    _worst("u8_bicubic", float(ulp), name)
    RAN.add(("u8_bicubic", (name, reverse)))


def test_coverage():
    """every op and case family of the lists above was graded -- checked when the whole module ran; prints the worst ratios of the run"""
    assert len({r for r in REQUIRED if r[0] == "depth_metrics"}) == len(E.METRIC_FAMILIES) + 1 == 35
    assert len({r for r in REQUIRED if r[0] == "silog_loss"}) == 10 and len({r for r in REQUIRED if r[0] == "u8_bicubic"}) == 22
    for op, (ratio, case) in sorted(WORST.items()):
        _log(f"worst {op}: {ratio:.3f} at {case}")
    if len(DONE) >= len(METRIC_CASES) + 1 + len(SILOG_CASES) + 2 * len(E.BICUBIC_CASES):
        assert REQUIRED <= RAN, sorted(map(str, REQUIRED - RAN))
        assert RAN <= REQUIRED, sorted(map(str, RAN - REQUIRED))
