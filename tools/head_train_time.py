"""Times one training step of the metric-bins head on the device -- engine.BinsHead forward with a context, SILog loss and its backward,
BinsHead.backward (csrc/head_bwd.hip), BinsHead.refresh -- at the ViT-L fusion head (C = 256, B = 4, 392 x 518) against torch.autograd
through the oracle head (oracle/pf_oracle.py bins_head + silog_loss) in float32 on the same GPU, interleaved in one process, and writes
profiles/head_train_time.json:

  * whole step: wall clock with a device synchronisation before and after; one warm-up of each path, then the median, minimum and maximum
    of --runs (>= 20) rounds.  The optimiser's own update is in neither path; the HIP path's repacking (refresh) is in its step;
  * per stage: the HIP path in a second run per round with a synchronisation after every stage (forward, loss, loss backward, head backward,
    refresh), the oracle path likewise (forward + loss, backward); medians over the rounds.
Before anything is timed the two paths' losses are compared (1e-4 relative).

    python tools/head_train_time.py [--runs 20] [--out profiles/head_train_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
from collections import OrderedDict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, C, SHAPE = 4, 256, (392, 518)
BCFG = dict(n_bins=64, bin_embedding_dim=128, n_attractors=[16, 8, 4, 1], min_temp=0.0212, max_temp=50.0, bin_centers_type="softplus",
            attractor_type="inv", attractor_kind="mean", min_depth=1e-3, max_depth=80.0)


def summary(values):
    ms = [1e3 * v for v in values]
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_train_time.json"))
    args = ap.parse_args()
    assert args.runs >= 20 and torch.cuda.is_available(), "a measurement needs a GPU and at least 20 runs"
    from oracle import pf_oracle
    from patchfusion_amd.config import pyramid_sizes
    from patchfusion_amd.engine import BinsHead
    from patchfusion_amd.hip_ops import ops
    from patchfusion_amd.spec import bins_head_spec, synthetic_state_dict
    dev = torch.device("cuda")
    spec = OrderedDict()
    bins_head_spec(spec, "", C, BCFG["n_bins"], BCFG["bin_embedding_dim"], BCFG["n_attractors"])
    sd = {k: v.to(dev) for k, v in synthetic_state_dict(spec, 0).items()}
    sizes = pyramid_sizes(SHAPE)[::-1]                                             # L0 .. L5, low -> high
    g = torch.Generator().manual_seed(1)
    feats = [torch.randn(B, h, w, C if i < 5 else 32, generator=g).to(dev) for i, (h, w) in enumerate(sizes)]
    target = (torch.rand(B, *SHAPE, generator=g) * 100.0 - 5.0).to(dev)
    head = BinsHead(sd, "", C, BCFG, torch.float32, dev, with_rel=False, min_depth=BCFG["min_depth"], max_depth=BCFG["max_depth"])
    lo, hi = BCFG["min_depth"], BCFG["max_depth"]
    names = BinsHead.param_names()

    def hip(stages=None):
        def mark(name, t0):
            if stages is not None:
                torch.cuda.synchronize()
                stages[name] = time.perf_counter() - t0
                return time.perf_counter()
            return t0
        t = time.perf_counter()
        clb = head.new_clb_buffer(ops, B, *SHAPE)
        ops.copy_channels(feats[5], clb[..., :32])
        ctx = {}
        depth = head.run(ops, feats[0], feats[1:5], clb, save=ctx)
        t = mark("forward", t)
        loss, sums = ops.silog_loss_saved(depth, target, lo, hi)
        t = mark("loss", t)
        d_depth = ops.silog_loss_bwd(depth, target, sums, ops.empty(tuple(depth.shape), torch.float32, dev), lo, hi)
        t = mark("loss_backward", t)
        grads, _ = head.backward(ops, ctx, d_depth)
        t = mark("head_backward", t)
        head.refresh(sd)
        mark("refresh", t)
        return loss, grads

    nchw = [f.permute(0, 3, 1, 2).contiguous() for f in feats]
    rel0 = torch.zeros(B, 1, *sizes[4], device=dev)

    def oracle(stages=None):
        t = time.perf_counter()
        leaf = {k: (sd[k].detach().requires_grad_(True) if k in names else sd[k]) for k in sd}
        xs = [f.detach().requires_grad_(True) for f in nchw]
        depth = pf_oracle.bins_head(leaf, "", xs[0], xs[1:5], xs[5], rel0, BCFG)
        loss = pf_oracle.silog_loss(depth, target.unsqueeze(1), lo, hi)
        if stages is not None:
            torch.cuda.synchronize()
            stages["forward_and_loss"] = time.perf_counter() - t
            t = time.perf_counter()
        loss.backward()
        if stages is not None:
            torch.cuda.synchronize()
            stages["backward"] = time.perf_counter() - t
        return loss.detach(), {k: leaf[k].grad for k in names}

    def timed(fn, stages=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(stages)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    (l_hip, g_hip), (l_ref, g_ref) = hip(), oracle()                               # warm-up of both, and the comparison
    assert abs(float(l_hip) - float(l_ref)) <= 1e-4 * abs(float(l_ref)), (float(l_hip), float(l_ref))
    worst = max(float((g_hip[k] - g_ref[k]).abs().max() / g_ref[k].abs().max()) for k in names)
    whole = {"hip": [], "oracle_autograd": []}
    stage = {"hip": {}, "oracle_autograd": {}}
    for _ in range(args.runs):
        for name, fn in (("hip", hip), ("oracle_autograd", oracle)):
            whole[name].append(timed(fn)[0])
            st = {}
            timed(fn, st)                                                          # the staged run synchronises per stage: timed apart
            for k, v in st.items():
                stage[name].setdefault(k, []).append(v)
    result = dict(tool="tools/head_train_time.py", device=torch.cuda.get_device_name(0), batch=B, channels=C, shape=list(SHAPE), runs=args.runs,
                  loss=dict(hip=float(l_hip), oracle_float32=float(l_ref)), worst_gradient_difference_hip_vs_float32_autograd=worst,
                  whole_step={k: summary(v) for k, v in whole.items()},
                  stages={n: {k: summary(v) for k, v in stage[n].items()} for n in stage})
    result["whole_step"]["oracle_over_hip"] = round(result["whole_step"]["oracle_autograd"]["median_ms"] / result["whole_step"]["hip"]["median_ms"], 2)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
