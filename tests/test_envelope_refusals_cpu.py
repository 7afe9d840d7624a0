"""The refusals of the inference engine's C entry points (tests/envelope.py), on a machine WITHOUT a device.

Every `refused` row of the table -- and, for every pointer argument, the null call and the call with the pointer off its boundary -- goes to the
library with made-up non-null addresses and must come back as exactly PF_ERR_ARG (queries: their "no" value).  With no device a call that slips
through the host checks ends in PF_ERR_LAUNCH = 2, so a missing refusal shows as a 2; with a device the same call would be a kernel launched on
made-up addresses, so the module skips itself when one is visible (the code under test is host code, identical on both machines).  The rows of one
source file run in a fresh child process that prints one JSON line: a host crash (the SIGFPE of pf_swin_window_attention(heads = 0) before its
check existed) fails that file's rows instead of ending the session.

The coverage test makes "every" mean every: each `extern "C"` entry point of the sources in scope has a prototype in include/pf_hip.h and a table
entry; each pointer argument is in the entry's pointer list, each integer argument (and each pf_conv_params field the entry point reads) in at least
one mutation; each launcher names its corner cases or says in a line why it has none."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import envelope as E

ROOT = E.ROOT
FILES = sorted(set(E.source_of().values()))


def _lib_or_skip():
    from patchfusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpf_hip.so not built")
    if torch.cuda.is_available():
        pytest.skip("a device is visible: refused calls are never sent to a GPU (the host checks are the same code on the CPU-only machine)")
    return _lib


# ------------------------------------------------------------------------------------------------------------------------------------------------
# coverage (no library needed)
# ------------------------------------------------------------------------------------------------------------------------------------------------
def test_every_entry_point_in_scope_has_a_prototype_and_a_table_entry():
    src, protos = E.source_of(), E.prototypes()
    assert len(src) == 78, sorted(src)                         # (pf_last_error, pf_version and pf_conv_last_variant among them: NO_ARGUMENTS)
    assert set(src) == set(protos), sorted(set(src) ^ set(protos))
    have = set(E.TABLE) | set(E.NO_ARGUMENTS)
    assert have == set(src), sorted(have ^ set(src))
    assert not (set(E.TABLE) & set(E.NO_ARGUMENTS))


@pytest.mark.parametrize("name", sorted(E.TABLE))
def test_entry_has_the_minimum_rows(name):
    e, proto = E.TABLE[name], E.prototypes()[name]
    mutated = set()
    for _, m in E.rows(name):
        mutated |= set(m)
    struct = [an for ct, an in proto if "pf_conv_params" in ct]
    for ctype, an in proto:
        if an in E.FREE or "pf_conv_params" in ctype:
            continue
        if "*" in ctype:
            if not e["query"]:
                assert an in e["ptrs"], f"{name}: pointer argument {an} is not in the entry's pointer list"
        else:
            assert an in mutated, f"{name}: no refused row changes {an}"
    for an in struct:
        assert an in mutated, f"{name}: no row passes a null {an}"
        if e["query"]:
            continue
        reads = e["reads"] if e["reads"] is not None else set(E.CONV_INT_FIELDS)
        for f in sorted(reads):
            if f"{an}.{f}" not in E.FREE:
                assert f"{an}.{f}" in mutated, f"{name}: no refused row changes {an}.{f}"
        for f in ("x", "y"):
            assert f"{an}.{f}" in e["ptrs"], f"{name}: {an}.{f} is not in the entry's pointer list"
    if not e["query"]:
        for p, width in e["ptrs"].items():
            ids = [rid for rid, m in E.rows(name) if p in m]
            assert any(i.startswith("null:") for i in ids) or p in e["optional"], (name, p)
            assert width == "host" or any(i.startswith("misaligned:") for i in ids), (name, p)
        assert bool(e["corners"]) != bool(e["no_corner"]), f"{name}: corners, or one line why there are none"
    else:
        assert not e["corners"], f"{name}: a query has no corner"


def test_corners_named_in_the_table_exist_in_the_corner_module():
    from tests import test_envelope_corners_gpu as G
    named = {c for e in E.TABLE.values() for c in e["corners"]}
    assert named <= set(G.CORNER_TESTS), sorted(named - set(G.CORNER_TESTS))
    for c in named:
        assert all(hasattr(G, t) for t in G.CORNER_TESTS[c]), c


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the rows, one child process per source file
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _child(src):
    """runs in the child: every row of the entries defined in `src` -> one JSON line {entry: {row: status}} (+ "good": the unmutated call)"""
    from patchfusion_amd import _lib
    assert not torch.cuda.is_available()
    L = _lib.load()
    for fn, restype in (("pf_wino_f16x2_scratch_bytes", C.c_long),):
        getattr(L, fn).restype = restype
    out = {}
    where = E.source_of()
    for name in sorted(E.TABLE):
        if where[name] != src:
            continue
        ptr = E.fake_pointers()
        res = {"good": E.call(L, _lib, name, ptr)}
        for rid, m in E.rows(name):
            res[rid] = E.call(L, _lib, name, E.fake_pointers(), m)
        out[name] = res
    print("ENVELOPE " + json.dumps(out))


_RESULTS = {}


def _results(src):
    if src not in _RESULTS:
        env = dict(os.environ)
        for v in ("PF_S3_TILE_NOW", "PF_S3_PERSIST", "PF_S3_T192", "PF_S3_GRID", "PF_WINO_F16X2_N256", "PF_F16_TILE"):
            env.pop(v, None)
        r = subprocess.run([sys.executable, "-m", "tests.test_envelope_refusals_cpu", src], cwd=ROOT, capture_output=True, text=True, timeout=300, env=env)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("ENVELOPE ")]
        _RESULTS[src] = (r.returncode, json.loads(line[-1][9:]) if line else None, r.stderr[-2000:])
    return _RESULTS[src]


@pytest.mark.parametrize("src", FILES)
def test_refused_rows_return_err_arg(src):
    _lib_or_skip()
    rc, res, err = _results(src)
    assert rc == 0 and res is not None, f"the child process of {src} ended with status {rc} (a negative status is a signal: a host crash)\n{err}"
    wrong = []
    for name, rows in res.items():
        e = E.TABLE[name]
        if not e["query"]:
            assert rows["good"] != E.PF_ERR_ARG, f"{name}: the unmutated call is refused -- the rows below it prove nothing"
        else:
            assert rows["good"] != e["no"], f"{name}: the unmutated query answers its 'no' value -- the rows below it prove nothing"
        for rid, status in rows.items():
            if rid != "good" and status != e["no"]:
                wrong.append(f"{name} [{rid}] returned {status}, expected {e['no']}")
    assert not wrong, "\n".join(wrong)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# consistency: a query's yes is a call its launcher takes; a plan's route takes the plan's own parameters
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _wino_params(_lib, B, H, W, cin, cout, x_ld=None, y_ld=None):
    p = _lib.ConvParams()
    p.x, p.y = 0x50000000, 0x58000000
    p.x_ld, p.B, p.H, p.W, p.Cin = x_ld or cin, B, H, W, cin
    p.y_ld, p.OH, p.OW, p.Cout = y_ld or cout, H, W, cout
    p.KH = p.KW = 3
    p.stride = p.pad = p.shuffle = 1
    return p


def test_a_supported_answer_is_a_call_the_launcher_takes():
    _lib = _lib_or_skip()
    L = _lib.load()
    vp = C.c_void_p
    U, V, M, S = vp(0x60000000), vp(0x61000000), vp(0x62000000), vp(0x63000000)
    yes = 0
    for B, H, W in ((1, 1, 1), (1, 5, 4), (8, 56, 74), (8, 224, 296)):
        for cin, cout in ((16, 4), (32, 4), (32, 8), (48, 36), (256, 256), (768, 768), (544, 544)):
            for x_ld, y_ld in ((None, None), (cin + 8, cout + 8), (cin - 4, None)):
                p = _wino_params(_lib, B, H, W, cin, cout, x_ld, y_ld)
                if L.pf_conv_winograd_fused_supported(C.byref(p)):
                    yes += 1
                    assert L.pf_conv_winograd_fused(C.byref(p), U, (cout + 63) // 64, 1, None) != E.PF_ERR_ARG, (B, H, W, cin, cout, x_ld, y_ld)
                rows = -(-cout // 16) * 16
                for given in (0, 1):
                    if L.pf_conv_winograd_f16x2_supported_ex(C.byref(p), rows, cin, 0, given):
                        yes += 1
                        assert L.pf_conv_winograd_f16x2_windowed_ex(C.byref(p), U, rows, cin, V, M, S, 0, vp(0x64000000) if given else None, None, 0, None) \
                            != E.PF_ERR_ARG, (B, H, W, cin, cout, x_ld, y_ld, given)
                if L.pf_conv_winograd_f16x2_supported(C.byref(p), rows, cin, 0):
                    yes += 1
                    assert L.pf_conv_winograd_f16x2_windowed(C.byref(p), U, rows, cin, V, M, S, 0, None) != E.PF_ERR_ARG, (B, H, W, cin, cout, x_ld, y_ld)
    assert yes >= 20, yes


def test_a_route_answer_is_a_call_the_launcher_takes():
    """the batched transform-domain product as csrc/winograd.hip issues it, and the fp16x2 linear: whichever kernel the route query names, the launcher
    takes the call (no device: it ends in PF_ERR_LAUNCH)"""
    _lib = _lib_or_skip()
    L = _lib.load()
    for T, K, N in ((1, 32, 8), (17, 32, 16), (33152, 768, 768), (33152, 512, 256), (165760, 544, 544)):
        p = _lib.ConvParams()
        p.x, p.w, p.y = 0x50000000, 0x58000000, 0x5c000000
        p.x_ld, p.B, p.H, p.W, p.Cin, p.w_rows, p.Kpad = K, 1, 1, T, K, -(-N // 16) * 16, K
        p.y_ld, p.OH, p.OW, p.Cout = N, 1, T, N
        p.KH = p.KW = p.stride = p.shuffle = 1
        p.dtype, p.out_f32, p.korder, p.batch = 1, 1, 6, 36
        p.x_bstride, p.w_bstride = 36 * T * K, 36 * p.w_rows * K
        assert L.pf_gemm_split3_route(C.byref(p), 256) >= 0
        assert L.pf_gemm_split3(C.byref(p), None) != E.PF_ERR_ARG, (T, K, N)
        r = L.pf_gemm_f16x2_points_route(C.byref(p), 256)
        ce = C.c_void_p(0x5e000000)
        if r == 3:
            assert L.pf_gemm_f16x2_points(C.byref(p), ce, 0, None) != E.PF_ERR_ARG, (T, K, N)
        if r == 2:
            assert L.pf_gemm_f16x2_points128(C.byref(p), ce, 0, None) != E.PF_ERR_ARG, (T, K, N)
        p.batch, p.col_exp = 0, 0x5e000000
        p.x_bstride, p.w_bstride = T * K, p.w_rows * K
        assert L.pf_gemm_f16x2_route(C.byref(p), 256) in (3, 4)
        assert L.pf_gemm_f16x2(C.byref(p), None) != E.PF_ERR_ARG, (T, K, N)


PLAN_LAYERS = [  # cin, cout, k, stride, pad, B, H, W, dtype, switches, the routes the plan may pick
    (32, 32, 1, 1, 0, 1, 5, 7, torch.float32, {}, {"direct"}),
    (96, 128, 1, 1, 0, 1, 37, 50, torch.float32, {"PF_CONV1X1_SPLIT3": "2"}, {"s3_1x1"}),
    (8, 4, 3, 2, 1, 1, 5, 7, torch.float32, {}, {"direct"}),
    (32, 8, 3, 1, 1, 1, 5, 4, torch.float32, {"PF_WINO_FUSED": "2"}, {"fused"}),
    (32, 8, 3, 1, 1, 1, 5, 4, torch.float32, {"PF_WINO_FUSED": "0"}, {"wino3", "wino", "wino3h", "direct"}),
    (64, 64, 3, 1, 1, 2, 13, 9, torch.float32, {"PF_WINO_FUSED": "0", "PF_WINO_SPLIT3": "0"}, {"wino", "direct"}),
    (512, 512, 1, 1, 0, 1, 32, 64, torch.bfloat16, {}, {"pp", "direct"}),
    (16, 16, 3, 1, 1, 1, 4, 4, torch.bfloat16, {}, {"direct"}),
]


@pytest.mark.parametrize("layer", PLAN_LAYERS, ids=lambda l: f"{l[0]}to{l[1]}_k{l[2]}s{l[3]}_{l[5]}x{l[6]}x{l[7]}_{str(l[8])[6:]}_{'_'.join(l[9].values()) or 'default'}")
def test_the_plan_of_a_layer_is_a_call_its_route_takes(monkeypatch, layer):
    """HipOps._conv_plan on host tensors (its device check replaced, as no device is there): the route it picks gets the plan's own parameters and must
    not refuse them"""
    _lib = _lib_or_skip()
    from patchfusion_amd import hip_ops, packing
    cin, cout, k, stride, pad, B, H, W, dt, switches, routes = layer
    for name, v in switches.items():
        monkeypatch.setenv(name, v)
    monkeypatch.setattr(hip_ops, "_p", lambda t: None if t is None else C.c_void_p(t.data_ptr()))
    if hasattr(hip_ops, "refresh_env"):
        hip_ops.refresh_env()
    g = torch.Generator().manual_seed(0)
    pw = packing.pack_conv(torch.randn(cout, cin, k, k, generator=g), torch.randn(cout, generator=g), dtype=dt)
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    x, y = torch.zeros(B, H, W, cin, dtype=dt), torch.zeros(B, OH, OW, cout, dtype=dt)
    try:
        route, p, extra = hip_ops.HipOps._conv_plan(x, pw, y, stride, pad, "relu" if k == 3 else None, False, None, None, None)
    finally:
        monkeypatch.undo()
        if hasattr(hip_ops, "refresh_env"):
            hip_ops.refresh_env()
    assert route in routes, route
    L, vp = _lib.load(), C.c_void_p
    V, M, S = vp(0x61000000), vp(0x62000000), vp(0x63000000)
    if route == "direct":
        rc = L.pf_conv(C.byref(p), None)
    elif route == "pp":
        rc = L.pf_gemm_bf16_pp(C.byref(p), None)
    elif route == "s3_1x1":
        rc = L.pf_conv1x1_split3(C.byref(p), extra[0], extra[1], None)
    elif route == "fused":
        rc = L.pf_conv_winograd_fused(C.byref(p), extra[0], extra[1], extra[2], None)
    elif route == "wino3":
        rc = L.pf_conv_winograd_split3_windowed(C.byref(p), extra[0], extra[1], extra[2], V, M, extra[5], None)
    elif route == "wino3h":
        rc = L.pf_conv_winograd_f16x2_windowed(C.byref(p), extra[0], extra[1], extra[2], V, M, S, extra[5], None)
    else:
        rc = L.pf_conv_winograd(C.byref(p), extra[0], extra[1], extra[2], extra[3], V, M, None)
    assert rc != E.PF_ERR_ARG, (route, L.pf_last_error())


if __name__ == "__main__":
    _child(sys.argv[1])
