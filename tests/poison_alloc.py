"""TEST INFRASTRUCTURE ONLY.  Poison every allocation the engine and the op wrappers make themselves, and compare whole runs bit for bit.

Property under test (tests/test_uninit_independence_gpu.py): no output depends on the initial contents of any allocation.  The per-kernel tests
pre-fill the OUTPUTS they hand in; the buffers `engine.py`, `midas_core.py` and the wrappers of `hip_ops.py` allocate with ``torch.empty`` (concat
buffers written slice by slice, padded tails, the Winograd arenas reused window after window, plane buffers, saved contexts) are out of their
reach, and what a kernel finds in a row, column, K-pad or tile tail nobody wrote is whatever the caching allocator hands back.

``poisoned(fill)`` replaces ``torch.empty``, ``torch.empty_like``, ``torch.empty_strided`` and ``torch.Tensor.new_empty`` for its duration and
fills every FLOATING tensor allocated on a listed device, in place on the current stream, before it is returned:

    "zero"   all bits zero
    "nan"    quiet NaN: propagates through every sum and product, so one read reaches the output
    "max"    torch.finfo(dtype).max: finite, so it survives what swallows a NaN -- ``fmaxf`` returns its other operand for a NaN, and so do
             ReLU-on-load, max-pool, the range pass and the channel maxima of the fp16x2 Winograd layers -- and it overflows as soon as it is
             multiplied or summed.  A stale 3e38 in a range pass costs every mantissa bit of the fp16 planes without producing one NaN.

Both poisons are needed: "nan" alone passes a read that goes through a maximum (tests/test_poison_alloc_cpu.py plants one), "max" alone can be
absorbed where a NaN is not (e.g. a product with an exact zero).

Integer and byte allocations are NOT touched: a value read from poison and used as an index or address could fault the device, which is not the
purpose.  The exception is INT_ALLOW below: sites whose contents, by reading the code, are never an address or an index.  They are poisoned only
when named in ``int_sites=`` and get the byte patterns 0x00 / 0xFF / 0x7F.

Every poisoned allocation is recorded as a :class:`Site`: file and line of the nearest stack frame inside ``patchfusion_amd/`` (for an engine
allocation that is ``HipOps.empty`` itself; ``caller`` is the next package frame up, the line in engine.py), dtype and bytes.  ``sites=`` is a
predicate on that record for bisecting a dependence: poison only these.

The patch is installed from inside test functions only and always removed in a ``finally``.
"""
import collections
import contextlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patchfusion_amd") + os.sep
MODES = ("zero", "nan", "max")
_BYTE = {"zero": 0x00, "nan": 0xFF, "max": 0x7F}

# integer / byte allocation sites that may be poisoned ("module.function" of the allocating frame), each with the reason its contents are never
# an address or an index
INT_ALLOW = {
    # uint32 bit patterns of float maxima, merged with atomicMax and turned into a power-of-two exponent (csrc/wino_f16x2.hip chan_exp)
    "hip_ops._cmax_buffer": "float bits of channel maxima: only compared (atomicMax) and converted to an ldexp exponent",
    # [fp16 filter planes | int32 column exponents | uint32 channel maxima] (csrc/winograd.hip f16x2_scratch): MFMA operands, ldexpf arguments and
    # maxima; the offsets into it are computed on the host from Cin and the row count, never read from it
    "hip_ops._f16x2_scratch": "fp16 filter planes, exponents for ldexpf and channel maxima: arithmetic operands only",
}

Site = collections.namedtuple("Site", "file line func dtype nbytes caller")
_ACTIVE = []


def fill_value(dtype, fill):
    """the value a floating tensor of `dtype` is filled with"""
    if fill == "zero":
        return 0.0
    if fill == "nan":
        return float("nan")
    if fill == "max":
        return torch.finfo(dtype).max
    raise ValueError(f"fill must be one of {MODES}, not {fill!r}")


def _int_fill_value(dtype, fill):
    size = torch.tensor([], dtype=dtype).element_size()
    signed = dtype in (torch.int8, torch.int16, torch.int32, torch.int64)
    return int.from_bytes(bytes([_BYTE[fill]]) * size, "little", signed=signed)


def _site(t):
    """the nearest frame inside patchfusion_amd/ (else the immediate caller of the patched function) and the next package frame above it"""
    f = sys._getframe(2)
    first, near, caller = f, None, None
    while f is not None:
        fn = f.f_code.co_filename
        if fn.startswith(PKG):
            if near is None:
                near = f
            else:
                caller = f"{os.path.relpath(fn, ROOT)}:{f.f_lineno}"
                break
        f = f.f_back
    f = near if near is not None else first
    return Site(os.path.relpath(f.f_code.co_filename, ROOT) if near is not None else f.f_code.co_filename, f.f_lineno, f.f_code.co_name,
                t.dtype, t.numel() * t.element_size(), caller)


def site_name(s):
    """'hip_ops._workspace' for a record whose nearest package frame is that function"""
    return f"{os.path.splitext(os.path.basename(s.file))[0]}.{s.func}"


@contextlib.contextmanager
def poisoned(fill, sites=None, devices=("cuda",), int_sites=()):
    """-> the list of Site records of this block (appended to as allocations happen).  `int_sites`: names out of INT_ALLOW to poison as well."""
    if fill not in MODES:
        raise ValueError(f"fill must be one of {MODES}, not {fill!r}")
    for n in int_sites:
        if n not in INT_ALLOW:
            raise ValueError(f"{n!r} is not on the integer allow-list (tests/poison_alloc.py INT_ALLOW: every entry needs a reason)")
    if _ACTIVE:
        raise RuntimeError("poisoned() does not nest")
    devices = tuple(devices)
    if "cuda" in devices and torch.cuda.is_available():
        # cached arenas and plans are re-allocated under the poison, and the allocator's free blocks go back to the driver
        from patchfusion_amd import hip_ops
        hip_ops.release_workspaces()
        torch.cuda.empty_cache()
    orig = {"empty": torch.empty, "empty_like": torch.empty_like, "empty_strided": torch.empty_strided}
    own_new_empty = "new_empty" in torch.Tensor.__dict__
    orig_new_empty = torch.Tensor.new_empty
    record = []

    def treat(t):
        if not isinstance(t, torch.Tensor) or t.device.type not in devices:
            return t
        if t.is_floating_point():
            s = _site(t)
            if sites is None or sites(s):
                t.fill_(fill_value(t.dtype, fill))
                record.append(s)
        elif int_sites and not t.is_complex() and t.dtype != torch.bool:
            s = _site(t)
            if site_name(s) in int_sites and (sites is None or sites(s)):
                t.fill_(_int_fill_value(t.dtype, fill))
                record.append(s)
        return t

    def empty(*a, **k):
        return treat(orig["empty"](*a, **k))

    def empty_like(*a, **k):
        return treat(orig["empty_like"](*a, **k))

    def empty_strided(*a, **k):
        return treat(orig["empty_strided"](*a, **k))

    def new_empty(self, *a, **k):
        return treat(orig_new_empty(self, *a, **k))

    _ACTIVE.append({"orig": orig})
    try:
        torch.empty, torch.empty_like, torch.empty_strided = empty, empty_like, empty_strided
        torch.Tensor.new_empty = new_empty
        yield record
    finally:
        torch.empty, torch.empty_like, torch.empty_strided = orig["empty"], orig["empty_like"], orig["empty_strided"]
        if own_new_empty:
            torch.Tensor.new_empty = orig_new_empty
        else:
            del torch.Tensor.new_empty
        _ACTIVE.clear()


def is_patched():
    return bool(_ACTIVE) or torch.empty.__module__ == __name__


# ---------------------------------------------------------------------------------------------------------------------------------------
# the comparison: whole runs, bit for bit
_INT_VIEW = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    """integer view of a tensor's bits (a NaN equals itself here; the finite check is what refuses it)"""
    t = t.detach().contiguous()
    if t.is_floating_point():
        return t.view(_INT_VIEW[t.element_size()])
    return t


def snapshot(named):
    """ordered {name: tensor} -> detached copies (the originals may be views of buffers a later launch rewrites)"""
    out = collections.OrderedDict()
    for k, v in named.items():
        if isinstance(v, (int, float)):
            v = torch.tensor(v, dtype=torch.float64)
        out[k] = v.detach().clone()
    return out


def first_mismatch(ref, got, reorder=None):
    """None, or (name, differing elements, elements) of the first entry in ref's order whose bits differ (a missing or reshaped entry counts whole).
    `reorder`: {name: relative bound} for entries that are sums accumulated with atomics in no fixed order -- no two runs of those agree to the last
    bit, poisoned or not; they are held to |a - b| <= bound * max(|a|, |b|), the bound coming from the number of terms and the format's unit
    roundoff (a read of poison moves them by NaN or 1e38, not by 1e-12)"""
    for k, a in ref.items():
        b = got.get(k)
        if b is None or b.shape != a.shape or b.dtype != a.dtype:
            return k, a.numel(), a.numel()
        if reorder and k in reorder:
            n = int(torch.logical_not((a - b).abs() <= reorder[k] * torch.maximum(a.abs(), b.abs())).sum())      # (a NaN counts as a difference)
        else:
            n = int((bits(a) != bits(b)).sum())
        if n:
            return k, n, a.numel()
    extra = [k for k in got if k not in ref]
    if extra:
        return extra[0], got[extra[0]].numel(), got[extra[0]].numel()
    return None


def non_finite(named):
    """names of the floating entries that hold a NaN or an infinity"""
    return [k for k, v in named.items() if v.is_floating_point() and not bool(torch.isfinite(v).all())]


def check_independent(run, devices=("cuda",), int_sites=(), must_reach=(), sites=None, label="", reorder=None):
    """The property: ``run()`` builds what it tests and returns an ordered {name: tensor} in forward order (final output included).  It is run under
    "zero" twice, then under "nan" and "max".  The zero runs must agree bit for bit (else the comparison means nothing), every entry must be finite,
    and both poisoned runs must equal the zero run bit for bit; the failure names the first differing entry and how many elements differ.
    `must_reach`: site names ('hip_ops._workspace') or predicates on a Site that every run's record must contain -- the guard that the patch is
    in effect where the configuration says it runs.  `reorder`: see first_mismatch.  -> {fill: (site count, bytes poisoned)}"""
    stats, outs = {}, []
    for fill in ("zero", "zero", "nan", "max"):
        with poisoned(fill, sites=sites, devices=devices, int_sites=int_sites) as rec:
            out = snapshot(run())
        assert not is_patched(), "torch left patched"
        names = {site_name(s) for s in rec}
        for want in must_reach:
            hit = want in names if isinstance(want, str) else any(want(s) for s in rec)
            assert hit, f"{label}: the {fill} run never allocated at {getattr(want, '__name__', want)}: the patch is not in effect there (sites seen: {sorted(names)})"
        stats[fill] = (len(rec), sum(s.nbytes for s in rec))
        outs.append((fill, out))
    z0, z1 = outs[0][1], outs[1][1]
    mm = first_mismatch(z0, z1, reorder)
    assert mm is None, (f"{label}: two runs under the SAME zero fill differ at {mm[0]} ({mm[1]} of {mm[2]} elements): the run is not deterministic, "
                        "so the comparison with the poisoned runs means nothing")
    bad = non_finite(z0)
    assert not bad, f"{label}: non-finite values under the zero fill in {bad}"
    for fill, out in outs[2:]:
        mm = first_mismatch(z0, out, reorder)
        assert mm is None, (f"{label}: the output depends on uninitialised memory -- under the {fill!r} fill the first differing tap is {mm[0]} "
                            f"({mm[1]} of {mm[2]} elements differ from the zero-filled run)")
        bad = non_finite(out)
        assert not bad, f"{label}: non-finite values under the {fill!r} fill in {bad}"
    return stats
