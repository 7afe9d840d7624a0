"""The backward formulas of the metric-bins head and of the SILog loss (csrc/head_bwd.hip, include/pf_hip.h) restated in plain torch WITHOUT
autograd, NHWC like the kernels, in whatever dtype the operands have (the tests use float64).  tests/test_head_bwd_ref_cpu.py holds every
function here against torch.autograd through oracle/pf_oracle.py; the GPU tests and the fake backward ops (tests/head_bwd_fake_ops.py) then
use them as the per-kernel statement of what is computed.

Softplus derivative from the output, 1 - exp(-y): equal to sigmoid(x) below torch's threshold of 20 (above it torch's derivative is exactly
1 and this one 1 - 2e-9, which is 1 in float32); the test data stay far below the threshold."""
import math

import torch
import torch.nn.functional as F


# ---------------- resize (align_corners=True) ----------------
def up_matrix(n_in, n_out, dtype=torch.float64):
    """[n_out, n_in] interpolation matrix of one axis: src = d (n_in - 1) / (n_out - 1), taps floor(src) and the next index inside the axis"""
    M = torch.zeros(n_out, n_in, dtype=dtype)
    scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    for d in range(n_out):
        src = scale * d
        i0 = min(int(src), n_in - 1)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        l1 = src - i0
        M[d, i0] += 1.0 - l1
        M[d, i1] += l1
    return M


def resize_fwd(x, OH, OW):
    """x [B,H,W,C] -> [B,OH,OW,C]"""
    My, Mx = up_matrix(x.shape[1], OH, x.dtype).to(x.device), up_matrix(x.shape[2], OW, x.dtype).to(x.device)
    return torch.einsum("oh,pw,bhwc->bopc", My, Mx, x)


def resize_bwd(dy, H, W):
    """the adjoint: dy [B,OH,OW,C] -> [B,H,W,C]"""
    My, Mx = up_matrix(H, dy.shape[1], dy.dtype).to(dy.device), up_matrix(W, dy.shape[2], dy.dtype).to(dy.device)
    return torch.einsum("oh,pw,bopc->bhwc", My, Mx, dy)


# ---------------- 1x1 layers ----------------
def wgrad(dy, x):
    """dW [N,K] = sum_p dy[p,n] x[p,k], db [N] = sum_p dy[p,n]"""
    d2, x2 = dy.reshape(-1, dy.shape[-1]), x.reshape(-1, x.shape[-1])
    return d2.t() @ x2, d2.sum(0)


def act_bwd(dy, ref, act):
    """dy * act'; ref = output for relu / softplus, pre-activation for gelu (exact erf form)"""
    if act == "relu":
        return dy * (ref > 0).to(dy.dtype)
    if act == "softplus":
        return dy * (1.0 - torch.exp(-ref))
    if act == "gelu":
        return dy * (0.5 * (1.0 + torch.erf(ref / math.sqrt(2.0))) + ref * torch.exp(-0.5 * ref * ref) / math.sqrt(2.0 * math.pi))
    raise ValueError(act)


# ---------------- attractor ----------------
def _dfdx(dx, attractor_type):
    q = 300.0 * dx * dx
    if attractor_type == "exp":
        return torch.exp(-q) * (1.0 - 2.0 * q)
    return (1.0 - q) / (1.0 + q) ** 2


def attractor_fwd(A, b_prev, attractor_type, kind):
    """A [B,h,w,n_attr], b_prev [B,hp,wp,n_bins] -> b_new [B,h,w,n_bins]"""
    c = resize_fwd(b_prev, A.shape[1], A.shape[2])
    dx = A.unsqueeze(-1) - c.unsqueeze(-2)                           # [B,h,w,i,j]
    d = torch.exp(-300.0 * dx * dx) * dx if attractor_type == "exp" else dx / (1.0 + 300.0 * dx * dx)
    return c + (d.mean(-2) if kind == "mean" else d.sum(-2))


def attractor_bwd(A, b_prev, g, attractor_type, kind):
    """-> (dA [B,h,w,n_attr], d_b_c [B,h,w,n_bins]); the gradient of b_prev is resize_bwd(d_b_c)"""
    c = resize_fwd(b_prev, A.shape[1], A.shape[2])
    fp = _dfdx(A.unsqueeze(-1) - c.unsqueeze(-2), attractor_type)    # [B,h,w,i,j]
    s = 1.0 / A.shape[-1] if kind == "mean" else 1.0
    return s * (fp * g.unsqueeze(-2)).sum(-1), g * (1.0 - s * fp.sum(-2))


# ---------------- log-binomial expectation ----------------
def _logbinom_parts(pt, n_bins, min_temp, max_temp):
    p0, p1, t0, t1 = (pt[..., i] + 1e-4 for i in range(4))
    prob, tt = p0 / (p0 + p1), t0 / (t0 + t1)
    t = (max_temp - min_temp) * tt + min_temp
    om_raw = 1.0 - prob
    xc, om = prob.clamp(1e-4, 1.0), om_raw.clamp(1e-4, 1.0)
    # (float32 constants like the oracle, whose k / n tensors are float32 whatever the input's dtype)
    k = torch.arange(n_bins, dtype=torch.float32, device=pt.device)
    eps = 1e-7
    n_ = torch.full((1,), float(n_bins - 1), device=pt.device) + eps
    k_ = k + eps
    logc = n_ * torch.log(n_) - k_ * torch.log(k_) - (n_ - k_) * torch.log(n_ - k_ + eps)
    y = logc + k * torch.log(xc).unsqueeze(-1) + (n_bins - 1 - k) * torch.log(om).unsqueeze(-1)
    return p0, p1, t0, t1, prob, t, om_raw, xc, om, k, y


def logbinom_fwd_up(pt, centers_up, min_temp, max_temp):
    """pt [B,h,w,4], centers_up [B,h,w,n_bins] (already at pt's grid) -> depth [B,h,w]"""
    *_, t, _, _, _, _, y = _logbinom_parts(pt, centers_up.shape[-1], min_temp, max_temp)
    return (torch.softmax(y / t.unsqueeze(-1), -1) * centers_up).sum(-1)


def logbinom_fwd(pt, centers, min_temp, max_temp):
    """pt [B,h,w,4], centers [B,hc,wc,n_bins] -> depth [B,h,w]"""
    return logbinom_fwd_up(pt, resize_fwd(centers, pt.shape[1], pt.shape[2]), min_temp, max_temp)


def logbinom_bwd(pt, centers, d_depth, min_temp, max_temp):
    """-> (d_pt [B,h,w,4], d_centers_up [B,h,w,n_bins]); the gradient of centers is resize_bwd(d_centers_up)"""
    n_bins = centers.shape[-1]
    p0, p1, t0, t1, prob, t, om_raw, xc, om, k, y = _logbinom_parts(pt, n_bins, min_temp, max_temp)
    probs = torch.softmax(y / t.unsqueeze(-1), -1)
    c = resize_fwd(centers, pt.shape[1], pt.shape[2])
    depth = (probs * c).sum(-1)
    g = d_depth.unsqueeze(-1)
    dz = probs * (c - depth.unsqueeze(-1)) * g
    s_k, s_nk, s_y = (dz * k).sum(-1), (dz * (n_bins - 1 - k)).sum(-1), (dz * y).sum(-1)
    dprob = torch.where((prob >= 1e-4) & (prob <= 1.0), s_k / t / xc, torch.zeros_like(prob)) \
        - torch.where((om_raw >= 1e-4) & (om_raw <= 1.0), s_nk / t / om, torch.zeros_like(prob))
    dtt = -(s_y / (t * t)) * (max_temp - min_temp)
    ps, ts = (p0 + p1) ** 2, (t0 + t1) ** 2
    return torch.stack([dprob * p1 / ps, -dprob * p0 / ps, dtt * t1 / ts, -dtt * t0 / ts], -1), probs * g


# ---------------- SILog ----------------
def silog_sums(pred, target, lo, hi):
    m = (target > lo) & (target < hi)
    g = torch.log(pred[m] + 1e-7) - torch.log(target[m] + 1e-7)
    return float(m.sum()), g.sum(), (g * g).sum()


def silog_bwd(pred, target, lo, hi, beta=0.15, d_loss=1.0):
    """dL/dpred on the prediction's own grid (same shape as target); zeros when at most one pixel is valid"""
    m = (target > lo) & (target < hi)
    n = int(m.sum())
    out = torch.zeros_like(pred)
    if n <= 1:
        return out
    g = torch.log(pred + 1e-7) - torch.log(target.clamp_min(1e-30) + 1e-7)
    gm = g[m]
    mean = gm.sum() / n
    var = ((gm * gm).sum() - gm.sum() ** 2 / n) / (n - 1)
    R = torch.sqrt(var + beta * mean * mean)
    d = (10.0 * d_loss / R) * ((g - mean) / (n - 1) + beta * mean / n) / (pred + 1e-7)
    return torch.where(m, d, out)


# ---------------- the whole head ----------------
def _lin(sd, name, x):
    return x @ sd[name + ".weight"].flatten(1).t() + sd[name + ".bias"]


def _mlp_fwd(sd, name, x, act_out, saved):
    h = torch.relu(_lin(sd, name + "._net.0", x))
    y = _lin(sd, name + "._net.2", h)
    if act_out == "softplus":
        y = F.softplus(y)
    saved[name] = (x, h, y, act_out)
    return y


def _mlp_bwd(sd, name, dy, saved, grads):
    x, h, y, act_out = saved[name]
    if act_out == "softplus":
        dy = act_bwd(dy, y, "softplus")
    grads[name + "._net.2.weight"], grads[name + "._net.2.bias"] = wgrad(dy, h)
    dh = act_bwd(dy @ sd[name + "._net.2.weight"].flatten(1), h, "relu")
    grads[name + "._net.0.weight"], grads[name + "._net.0.bias"] = wgrad(dh, x)
    return dh @ sd[name + "._net.0.weight"].flatten(1)


def head_forward(sd, p, x0, x_blocks, last, rel, bcfg):
    """oracle.bins_head ('softplus' centres) on NHWC tensors; rel [B,hr,wr,1] or None (the fusion head's zero relative depth).
    -> (depth [B,H,W], ctx)"""
    at, ak = bcfg.get("attractor_type", "inv"), bcfg.get("attractor_kind", "mean")
    sv = {}
    b_prev = _mlp_fwd(sd, p + "seed_bin_regressor", x0, "softplus", sv)
    prev_emb = _mlp_fwd(sd, p + "seed_projector", x0, None, sv)
    layers = []
    for i, xb in enumerate(x_blocks):
        emb = _mlp_fwd(sd, f"{p}projectors.{i}", xb, None, sv)
        xs = emb + resize_fwd(prev_emb, xb.shape[1], xb.shape[2])
        A = _mlp_fwd(sd, f"{p}attractors.{i}", xs, "softplus", sv)
        b_new = attractor_fwd(A, b_prev, at, ak)
        layers.append((A, b_prev, prev_emb.shape[1:3]))
        b_prev, prev_emb = b_new, emb
    B, H, W, _ = last.shape
    rel_up = torch.zeros(B, H, W, 1, dtype=last.dtype, device=last.device) if rel is None else resize_fwd(rel, H, W)
    clb = torch.cat([last, rel_up, resize_fwd(prev_emb, H, W)], -1)
    t_pre = _lin(sd, p + "conditional_log_binomial.mlp.0", clb)
    t = F.gelu(t_pre)
    pt = F.softplus(_lin(sd, p + "conditional_log_binomial.mlp.2", t))
    depth = logbinom_fwd(pt, b_prev, bcfg["min_temp"], bcfg["max_temp"])
    ctx = dict(sv=sv, layers=layers, clb=clb, t_pre=t_pre, t=t, pt=pt, centers=b_prev, emb_hw=prev_emb.shape[1:3], at=at, ak=ak,
               rel_hw=None if rel is None else rel.shape[1:3], C_last=last.shape[-1])
    return depth, ctx


def head_backward(sd, p, ctx, bcfg, d_depth):
    """-> (param_grads keyed by the checkpoint names, input_grads {'x0', 'x_blocks', 'last'[, 'rel']})"""
    sv, grads = ctx["sv"], {}
    m0, m2 = p + "conditional_log_binomial.mlp.0", p + "conditional_log_binomial.mlp.2"
    d_pt, d_cup = logbinom_bwd(ctx["pt"], ctx["centers"], d_depth, bcfg["min_temp"], bcfg["max_temp"])
    g = resize_bwd(d_cup, *ctx["centers"].shape[1:3])                # gradient of the last layer's centres
    d_pt = act_bwd(d_pt, ctx["pt"], "softplus")
    grads[m2 + ".weight"], grads[m2 + ".bias"] = wgrad(d_pt, ctx["t"])
    d_t = act_bwd(d_pt @ sd[m2 + ".weight"].flatten(1), ctx["t_pre"], "gelu")
    grads[m0 + ".weight"], grads[m0 + ".bias"] = wgrad(d_t, ctx["clb"])
    d_clb = d_t @ sd[m0 + ".weight"].flatten(1)
    C = ctx["C_last"]
    inp = {"last": d_clb[..., :C]}
    if ctx["rel_hw"] is not None:
        inp["rel"] = resize_bwd(d_clb[..., C:C + 1], *ctx["rel_hw"])
    d_emb = resize_bwd(d_clb[..., C + 1:], *ctx["emb_hw"])          # into the last projector's embedding
    d_blocks = [None] * len(ctx["layers"])
    for i in reversed(range(len(ctx["layers"]))):
        A, b_prev, prev_hw = ctx["layers"][i]
        dA, d_bc = attractor_bwd(A, b_prev, g, ctx["at"], ctx["ak"])
        g = resize_bwd(d_bc, *b_prev.shape[1:3])
        d_xs = _mlp_bwd(sd, f"{p}attractors.{i}", dA, sv, grads)
        d_blocks[i] = _mlp_bwd(sd, f"{p}projectors.{i}", d_emb + d_xs, sv, grads)
        d_emb = resize_bwd(d_xs, *prev_hw)
    inp["x0"] = _mlp_bwd(sd, p + "seed_projector", d_emb, sv, grads) + _mlp_bwd(sd, p + "seed_bin_regressor", g, sv, grads)
    inp["x_blocks"] = d_blocks
    if len(grads[m0 + ".weight"].shape) == 2:                        # the checkpoint's conv weights are [N, K, 1, 1]
        grads = {k: (v.reshape(sd[k].shape) if k.endswith(".weight") else v) for k, v in grads.items()}
    return grads, inp


# ---------------- the probe head shared by the CPU and the GPU tests ----------------
PROBE_SIZES = dict(x0=(2, 3), x_blocks=[(3, 5), (5, 7), (9, 13), (17, 25)], last=(33, 49))
PROBE_BCFG = dict(n_bins=64, bin_embedding_dim=128, n_attractors=[16, 8, 4, 1], min_temp=0.0212, max_temp=50.0, bin_centers_type="softplus",
                  attractor_type="inv", attractor_kind="mean", min_depth=1e-3, max_depth=80.0)


def probe_head(attractor_type="inv", attractor_kind="mean", with_rel=False, B=2, C=32, seed=0):
    """-> (sd float32 (checkpoint layout, no prefix), bcfg, inputs float32 NHWC dict(x0, x_blocks, last, rel | None), target [B,H,W]):
    C = 32, 128-wide embedding, 64 bins, n_attractors [16, 8, 4, 1]; the target is uniform on (-5, 95), so about a fifth of it is masked
    by (min_depth, max_depth) = (1e-3, 80)"""
    from collections import OrderedDict
    from patchfusion_amd.spec import bins_head_spec, synthetic_state_dict
    bcfg = dict(PROBE_BCFG, attractor_type=attractor_type, attractor_kind=attractor_kind)
    d = OrderedDict()
    bins_head_spec(d, "", C, bcfg["n_bins"], bcfg["bin_embedding_dim"], bcfg["n_attractors"])
    sd = synthetic_state_dict(d, seed)
    g = torch.Generator().manual_seed(100 + seed)
    rnd = lambda hw, c: torch.randn(B, hw[0], hw[1], c, generator=g)
    inputs = dict(x0=rnd(PROBE_SIZES["x0"], C), x_blocks=[rnd(s, C) for s in PROBE_SIZES["x_blocks"]], last=rnd(PROBE_SIZES["last"], 32),
                  rel=rnd(PROBE_SIZES["last"], 1).abs() if with_rel else None)       # (a branch writes its relative depth at the full grid)
    target = torch.rand(B, *PROBE_SIZES["last"], generator=g) * 100.0 - 5.0
    return sd, bcfg, inputs, target


def oracle_head_grads(sd, bcfg, inputs, target, dtype=torch.float64, device="cpu"):
    """autograd through oracle.pf_oracle.bins_head + silog_loss in `dtype` -> (loss, depth [B,H,W], param grads, input grads NHWC)"""
    from oracle import pf_oracle
    sdd = {k: (v.to(device=device, dtype=dtype).requires_grad_(True) if v.is_floating_point() and not k.endswith("K_minus_1") else v.to(device))
           for k, v in sd.items()}
    nchw = lambda t: t.to(device=device, dtype=dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    x0, xb, last = nchw(inputs["x0"]), [nchw(t) for t in inputs["x_blocks"]], nchw(inputs["last"])
    rel = nchw(inputs["rel"]) if inputs["rel"] is not None else None
    rel_in = rel if rel is not None else torch.zeros(last.shape[0], 1, *xb[-1].shape[2:], dtype=dtype, device=device)
    depth = pf_oracle.bins_head(sdd, "", x0, xb, last, rel_in, bcfg)
    loss = pf_oracle.silog_loss(depth, target.to(device=device, dtype=dtype).unsqueeze(1), bcfg["min_depth"], bcfg["max_depth"])
    loss.backward()
    pg = {k: v.grad for k, v in sdd.items() if isinstance(v, torch.Tensor) and v.requires_grad}
    nhwc = lambda t: t.grad.permute(0, 2, 3, 1)
    ig = dict(x0=nhwc(x0), x_blocks=[nhwc(t) for t in xb], last=nhwc(last))
    if rel is not None:
        ig["rel"] = nhwc(rel)
    return loss.detach(), depth.detach()[:, 0], pg, ig
