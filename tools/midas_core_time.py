"""Timing of the native MiDaS DPT_BEiT_L_384 core (patchfusion_amd/midas_core.py) on one MI355X.

  attention  pf_vit_attention_split3_rpb against pf_vit_attention_split3_v2 (default pipelined kernel and the two-phase kernel the bias
             variant is built on, same queries per wave) at equal (B, 769, 16), interleaved in one process, median of rounds;
             --ab-lib PATH also times pf_vit_attention_split3_v2 (two-phase) of another build of attn_split3.hip, interleaved (before / after)
  attention_bf16  the bf16 mode's pf_qkv_split + pf_vit_attention_rpb_bf16 against pf_qkv_split + pf_vit_attention (unbiased) and against the float32
             mode's pf_vit_attention_split3_rpb, same shapes, interleaved
  core       the whole core in ms per 384x512 crop at B = 1, 4, 8 (seeded weights); --dtype fp32 | bf16 | both (both: two cores, interleaved in
             one process, every round times each once)
  configs4   one 2160x3840 image, 4x4 + r128 = 177 patches, native cores (--dtype as above; both: two models, alternating)

    python tools/midas_core_time.py [--ab-lib PATH] [--rounds 7] [--iters 20] [--dtype both] [--only core]
prints one JSON line per measurement."""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def attention(args):
    from patchfusion_amd import _lib
    from patchfusion_amd import packing as pk
    from patchfusion_amd.hip_ops import ops
    L = _lib.load()
    ab = None
    if args.ab_lib:
        ab = ctypes.CDLL(args.ab_lib)
        ab.pf_vit_attention_split3_v2.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long] + [ctypes.c_int] * 6 + [ctypes.c_void_p]
    th, tw, Hh = 24, 32, 16
    S, D = th * tw + 1, Hh * 64
    for B in (1, 4, 8):
        qkv3 = torch.randn(3, B * S, 3 * D, device="cuda").to(torch.bfloat16)
        out = torch.empty(3, B * S, D, dtype=torch.bfloat16, device="cuda")
        tab = pk.beit_rel_pos_table(torch.randn(47 * 47 + 3, Hh), 24, th, tw).cuda()
        st = torch.cuda.current_stream().cuda_stream
        qw = 32 if ((S + 127) // 128) * B * Hh >= 512 else 16
        p, q = qkv3.data_ptr(), out.data_ptr()
        runs = {
            "rpb": lambda: L.pf_vit_attention_split3_rpb(p, qkv3.stride(0), q, out.stride(0), 0, B, S, Hh, tab.data_ptr(), th, tw, qw, st),
            "v2_two_phase": lambda: L.pf_vit_attention_split3_v2(p, qkv3.stride(0), q, out.stride(0), 0, B, S, Hh, qw, 1, st),
            "v2_pipelined": lambda: L.pf_vit_attention_split3_v2(p, qkv3.stride(0), q, out.stride(0), 0, B, S, Hh, 0, 0, st),
        }
        if ab is not None:
            runs["v2_two_phase_ab_lib"] = lambda: ab.pf_vit_attention_split3_v2(p, qkv3.stride(0), q, out.stride(0), 0, B, S, Hh, qw, 1, st)
        for f in runs.values():
            assert f() == 0
        t = {k: [] for k in runs}
        for _ in range(args.rounds):                      # interleaved: every round times each kernel once
            for k, f in runs.items():
                t[k].append(_time(f, args.iters))
        med = {k: statistics.median(v) * 1e3 for k, v in t.items()}
        r = dict(what="attention", B=B, S=S, heads=Hh, queries_per_wave=qw, us=med,
                 rpb_over_two_phase=med["rpb"] / med["v2_two_phase"], rpb_over_pipelined=med["rpb"] / med["v2_pipelined"])
        if ab is not None:
            r["two_phase_this_over_ab_lib"] = med["v2_two_phase"] / med["v2_two_phase_ab_lib"]
        print(json.dumps(r), flush=True)


def attention_bf16(args):
    from patchfusion_amd import _lib
    from patchfusion_amd import packing as pk
    L = _lib.load()
    th, tw, Hh = 24, 32, 16
    S, D, Sp = th * tw + 1, Hh * 64, 832
    bf = torch.bfloat16
    for B in (1, 4, 8):
        qkv = torch.randn(B * S, 3 * D, device="cuda").to(bf)
        q, k = (torch.empty(B, Hh, S, 64, dtype=bf, device="cuda") for _ in range(2))
        vt = torch.empty(B, Hh, 64, Sp, dtype=bf, device="cuda")
        out = torch.empty(B * S, D, dtype=bf, device="cuda")
        qkv3 = torch.randn(3, B * S, 3 * D, device="cuda").to(bf)
        out3 = torch.empty(3, B * S, D, dtype=bf, device="cuda")
        tab = pk.beit_rel_pos_table(torch.randn(47 * 47 + 3, Hh), 24, th, tw).cuda()
        st = torch.cuda.current_stream().cuda_stream
        P = [x.data_ptr() for x in (qkv, q, k, vt, out, tab, qkv3, out3)]
        runs = {
            "qkv_split": lambda: L.pf_qkv_split(P[0], B, S, Hh, P[1], P[2], P[3], Sp, 0.125, 1, st),
            "rpb_bf16": lambda: L.pf_vit_attention_rpb_bf16(P[1], P[2], P[3], P[4], B, S, Sp, Hh, P[5], th, tw, st),
            "unbiased_bf16": lambda: L.pf_vit_attention(P[1], P[2], P[3], P[4], B, S, Sp, Hh, 1, st),
            "rpb_split3_fp32": lambda: L.pf_vit_attention_split3_rpb(P[6], qkv3.stride(0), P[7], out3.stride(0), 0, B, S, Hh, P[5], th, tw, 0, st),
        }
        for f in runs.values():
            assert f() == 0
        t = {n: [] for n in runs}
        for _ in range(args.rounds):
            for n, f in runs.items():
                t[n].append(_time(f, args.iters))
        med = {n: statistics.median(v) * 1e3 for n, v in t.items()}
        print(json.dumps(dict(what="attention_bf16", B=B, S=S, heads=Hh, us=med, rpb_over_unbiased=med["rpb_bf16"] / med["unbiased_bf16"],
                              rpb_bf16_with_split_over_fp32_rpb=(med["rpb_bf16"] + med["qkv_split"]) / med["rpb_split3_fp32"])), flush=True)


DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _dtypes(args):
    return ("fp32", "bf16") if args.dtype == "both" else (args.dtype,)


def _seeded_core(args):
    from patchfusion_amd.midas_core import MidasBeitCore
    from tests import midas_beit_ref as mb
    ref = mb.seeded(mb.settings(), seed=11, dtype=torch.float32)
    cores = {}
    for dt in _dtypes(args):
        cores[dt] = MidasBeitCore("DPT_BEiT_L_384").load_state_dict({"core." + k: v for k, v in ref.state_dict().items()})
        cores[dt].call_dtype = DTYPES[dt]
    return ref, cores


def core(args, ref_core):
    _, cores = ref_core
    for B in (1, 4, 8):
        img = torch.rand(B, 3, 384, 512, device="cuda")
        t = {dt: [] for dt in cores}
        with torch.no_grad():
            for c in cores.values():
                c(img)
            for _ in range(args.rounds):                  # interleaved: every round times each dtype once
                for dt, c in cores.items():
                    t[dt].append(_time(lambda: c(img), 3))
        for dt, v in t.items():
            ms = statistics.median(v)
            print(json.dumps(dict(what="core", dtype=dt, B=B, ms_per_call=ms, ms_per_crop=ms / B, min_ms_per_crop=min(v) / B, max_ms_per_crop=max(v) / B)),
                  flush=True)


def configs4(args, ref_core):
    from patchfusion_amd.config import make_zoe_config
    from patchfusion_amd.model import PatchFusion
    from patchfusion_amd.spec import patchfusion_spec, synthetic_state_dict
    ref, _ = ref_core
    cfg = make_zoe_config()
    models = {}
    for dt in _dtypes(args):
        m = PatchFusion(cfg, compute_dtype=dt, core_providers="native").eval()
        m.load_state_dict(synthetic_state_dict(patchfusion_spec(cfg), 0), strict=True)
        for p in m.core_providers:
            p.load_state_dict({"core." + k: v for k, v in ref.state_dict().items()})
        models[dt] = m.cuda()
    img = torch.rand(1, 3, 2160, 3840, generator=torch.Generator().manual_seed(7))
    lr, hr = next(iter(models.values())).resizer(img).cuda(), img.cuda()

    def run(m):
        random.seed(0)
        m(mode="infer", image_lr=lr, image_hr=hr, cai_mode="r128", process_num=4)
    t = {dt: [] for dt in models}
    with torch.no_grad():
        for m in models.values():
            run(m)
        for _ in range(3):                                # alternating
            for dt, m in models.items():
                t[dt].append(_time(lambda: run(m), 1))
    for dt, v in t.items():
        print(json.dumps(dict(what="configs4", dtype=dt, patches=177, ms_per_image=statistics.median(v), min_ms=min(v), max_ms=max(v),
                              peak_GiB=torch.cuda.max_memory_allocated() / 2 ** 30)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab-lib", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", choices=["attention", "attention_bf16", "core", "configs4"], default=None)
    ap.add_argument("--dtype", choices=["fp32", "bf16", "both"], default="fp32")
    args = ap.parse_args()
    if args.only in (None, "attention"):
        attention(args)
    if args.only in (None, "attention_bf16"):
        attention_bf16(args)
    if args.only in (None, "core", "configs4"):
        rc = _seeded_core(args)
        if args.only in (None, "core"):
            core(args, rc)
        if args.only in (None, "configs4"):
            configs4(args, rc)


if __name__ == "__main__":
    main()
