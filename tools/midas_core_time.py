"""Timing of the native MiDaS DPT_BEiT_L_384 core (patchfusion_amd/midas_core.py) on one MI355X.

  attention  pf_vit_attention_split3_rpb against pf_vit_attention_split3_v2 (default pipelined kernel and the two-phase kernel the bias
             variant is built on, same queries per wave) at equal (B, 769, 16), interleaved in one process, median of rounds;
             --ab-lib PATH also times pf_vit_attention_split3_v2 (two-phase) of another build of attn_split3.hip, interleaved (before / after)
  core       the whole core in ms per 384x512 crop at B = 1, 4, 8 (seeded weights)
  configs4   one 2160x3840 image, 4x4 + r128 = 177 patches, native cores

    python tools/midas_core_time.py [--ab-lib PATH] [--rounds 7] [--iters 20]
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


def _seeded_core():
    from patchfusion_amd.midas_core import MidasBeitCore
    from tests import midas_beit_ref as mb
    ref = mb.seeded(mb.settings(), seed=11, dtype=torch.float32)
    return ref, MidasBeitCore("DPT_BEiT_L_384").load_state_dict({"core." + k: v for k, v in ref.state_dict().items()})


def core(args, ref_core):
    _, c = ref_core
    for B in (1, 4, 8):
        img = torch.rand(B, 3, 384, 512, device="cuda")
        with torch.no_grad():
            ms = statistics.median(_time(lambda: c(img), 3) for _ in range(args.rounds))
        print(json.dumps(dict(what="core", B=B, ms_per_call=ms, ms_per_crop=ms / B)), flush=True)


def configs4(args, ref_core):
    from patchfusion_amd.config import make_zoe_config
    from patchfusion_amd.model import PatchFusion
    from patchfusion_amd.spec import patchfusion_spec, synthetic_state_dict
    ref, _ = ref_core
    cfg = make_zoe_config()
    m = PatchFusion(cfg, compute_dtype="fp32", core_providers="native").eval()
    m.load_state_dict(synthetic_state_dict(patchfusion_spec(cfg), 0), strict=True)
    for p in m.core_providers:
        p.load_state_dict({"core." + k: v for k, v in ref.state_dict().items()})
    m = m.cuda()
    img = torch.rand(1, 3, 2160, 3840, generator=torch.Generator().manual_seed(7))
    lr, hr = m.resizer(img).cuda(), img.cuda()

    def run():
        random.seed(0)
        m(mode="infer", image_lr=lr, image_hr=hr, cai_mode="r128", process_num=4)
    with torch.no_grad():
        run()
        ms = statistics.median(_time(run, 1) for _ in range(3))
    print(json.dumps(dict(what="configs4", patches=177, ms_per_image=ms, peak_GiB=torch.cuda.max_memory_allocated() / 2 ** 30)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab-lib", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", choices=["attention", "core", "configs4"], default=None)
    args = ap.parse_args()
    if args.only in (None, "attention"):
        attention(args)
    if args.only in (None, "core", "configs4"):
        rc = _seeded_core()
        if args.only in (None, "core"):
            core(args, rc)
        if args.only in (None, "configs4"):
            configs4(args, rc)


if __name__ == "__main__":
    main()
