"""Network executors of the PatchFusion hot path on top of the HIP op set.

Organised around fused stages with explicit NHWC buffers, not nn.Modules: every method below is a
straight-line sequence of kernel launches (``ops.*`` -> C ABI -> hand-written HIP).  ``ops`` is the
op back-end object; the product always passes :data:`patchfusion_amd.hip_ops.ops` (tests substitute
a torch reference back-end from tests/fake_ops.py to validate the wiring and weight packing on CPU,
and to serve as the per-op reference for the HIP kernels on the GPU).

Reference functions restated here (paths under the reference repo):
  BranchNet      external/zoedepth/models/zoedepth/zoedepth_v1.py:125-233 (ZoeDepth.forward),
                 base_models/depth_anything.py:262-278, depth_anything/dpt.py:97-156, blocks.py:69-153,
                 torchhub/.../vision_transformer.py:212-231,297-321, dinov2/layers/{block,attention,mlp}.py
  G2LNet         estimator/models/blocks/swin_layers.py:218-268,325-355,410-432
  FusionNet      estimator/models/patchfusion.py:240-340, blocks/guided_fusion_model.py:163-207
  BinsHead       zoedepth_v1.py:173-219 == patchfusion.py:297-340; layers/{localbins,attractor,dist}_layers.py
"""
import math

import torch

from . import packing as pk
from .config import pyramid_sizes
from .spec import DPT_ARCH, VIT_ARCH, branch_channels

F32 = torch.float32


def linear_split3_enabled():
    """float32 mode: run the ViT block linears as split-precision GEMMs (csrc/gemm_split3.hip)?  PF_LINEAR_SPLIT3=0 / 1; default on"""
    import os
    return os.environ.get("PF_LINEAR_SPLIT3", "1") != "0"


def vit_f16x2_enabled(crops):
    """float32 mode with split-precision linears: run qkv / fc1 / fc2 of the ViT blocks on two scaled fp16 planes (packing.pack_conv_f16x2,
    csrc/gemm_split3.hip pf_gemm_f16x2: three MFMAs per product instead of six)?  Read once per engine build.  PF_VIT_F16X2: 0 = never,
    2 = every branch, 1 (default) = the branch that runs batches of crops.  Measured per launch (profiles/r8_vit_f16x2_linears.md): at 8 x 1037
    tokens 1.22-1.52x, at the coarse branch's single image (1037 tokens: 36-132 tiles of 192 x 192 on 256 CUs) 0.36-0.93x."""
    import os
    v = os.environ.get("PF_VIT_F16X2", "1")
    return v == "2" or (v != "0" and crops)


def vit_attn_f16x2_enabled():
    """with the fp16x2 block linears (vit_f16x2_enabled): also run the attention and the projection on two scaled fp16 planes (csrc/attn_split3.hip
    pf_vit_attention_f16x2, the projection through pf_gemm_f16x2)?  PF_VIT_ATTN_F16X2: 0 = the round-8 block (fp16x2 qkv / fc1 / fc2, bf16x3
    attention and projection); 1 = q / k / v on two fp16 planes and the fp16x2 attention, which writes the three bf16 planes of a
    projection that stays on bf16x3; 2 (default) = the attention's output and the projection on two fp16 planes as well.  Measured per launch at
    8 x 1037 tokens: attention 1.54x (three bf16 planes out) / 1.59x (two fp16 planes out) (profiles/r10_attn_f16x2_launches.md); the fp16x2
    projection was 0.96-0.98x of the bf16x3 one on 192 x 192 tiles (264 tiles on 256 CUs: two tile times) and is 2.1x on the 160 x 256 tile that
    pf_gemm_f16x2 now routes it to (0.0545 ms against 0.1147, profiles/r13_tile160_linears.md).  Image pass (profiles/r13_tile160_image_ab.md):
    2 on the new tile gains 3.2 ms over the 192-tile tree between alternating processes (3.2 times the largest within-arm spread) and 5.4 ms in
    the mean of both engine build orders in one process; max |depth difference| 4.8e-7.  Read once per engine build; crops branch only.
    -> 0, 1 (attention) or 2 (attention and projection)"""
    import os
    v = os.environ.get("PF_VIT_ATTN_F16X2", "2")
    return 0 if v == "0" else 1 if v == "1" else 2


def attention_split3_enabled():
    """float32 mode with split-precision linears: also run the ViT attention in split precision (pf_vit_attention_split3)?  PF_ATTN_SPLIT3=0 / 1"""
    import os
    return os.environ.get("PF_ATTN_SPLIT3", "1") != "0"


def bins_tail_enabled():
    """float32 mode: the fused metric-bins tail kernel (pf_bins_tail)?  PF_BINS_TAIL=0 keeps the four separate launches"""
    import os
    return os.environ.get("PF_BINS_TAIL", "1") != "0"


def _g(sd, name, device):
    return sd[name].detach().to(device=device, dtype=F32).contiguous()


def _copy_pack(dst, src):
    """overwrite the tensors of a packed layer (packing.PackedConv / BinsTail) with those of a fresh pack of the same shapes"""
    for k, v in vars(src).items():
        if isinstance(v, torch.Tensor):
            getattr(dst, k).copy_(v)


class BinsHead:
    """seed regressor/projector, 4 x (projector, attractor), conditional log-binomial, expectation."""

    def __init__(self, sd, prefix, C, bcfg, dtype, device, with_rel, min_depth=None, max_depth=None):
        self.dtype, self.device = dtype, device
        # bin_centers_type (zoedepth_v1.py:90-104 == patchfusion.py:132-146): bounded seed regressor for 'normed' / 'hybrid1', bounded
        # attractor layer for 'normed' / 'hybrid2'; min / max depth only matter for those (branch head: the branch config's own,
        # fusion head: the top-level config's, patchfusion.py:152-163)
        kind = bcfg.get("bin_centers_type", "softplus")
        if kind not in ("normed", "softplus", "hybrid1", "hybrid2"):
            raise ValueError("bin_centers_type should be one of 'normed', 'softplus', 'hybrid1', 'hybrid2'")
        self.seed_bounded, self.attr_bounded = kind in ("normed", "hybrid1"), kind in ("normed", "hybrid2")
        self.lo = float(bcfg.get("min_depth", 1e-3) if min_depth is None else min_depth)
        self.hi = float(bcfg.get("max_depth", 10) if max_depth is None else max_depth)
        # defaults of ZoeDepth.build for a branch head (zoedepth_v1.py:41: attractor_type 'exp', attractor_kind 'sum'); the fusion head
        # reads both straight from the config and fails without them (patchfusion.py:162)
        if not with_rel and not ("attractor_type" in bcfg and "attractor_kind" in bcfg):
            raise AttributeError("coarse_branch config needs attractor_type and attractor_kind for the fusion head (patchfusion.py:162)")
        self.attr_type, self.attr_kind = bcfg.get("attractor_type", "exp"), bcfg.get("attractor_kind", "sum")
        if self.attr_kind not in ("mean", "sum"):
            raise KeyError(self.attr_kind)                          # attractor.py:118 indexes a dict with it
        self.n_attr = list(bcfg["n_attractors"])
        self.n_bins = int(bcfg["n_bins"])
        self.emb = int(bcfg["bin_embedding_dim"])
        self.min_temp, self.max_temp = float(bcfg["min_temp"]), float(bcfg["max_temp"])
        self.with_rel = with_rel
        self.prefix = prefix
        self._pack(sd)

    def _pack(self, sd):
        prefix, dtype, device, with_rel = self.prefix, self.dtype, self.device, self.with_rel

        def pc(name, **kw):
            return pk.pack_conv(sd[prefix + name + ".weight"], sd[prefix + name + ".bias"], dtype=dtype, **kw).to(device)

        self.sbr0, self.sbr2 = pc("seed_bin_regressor._net.0"), pc("seed_bin_regressor._net.2")
        self.sp0, self.sp2 = pc("seed_projector._net.0"), pc("seed_projector._net.2")
        self.proj = [(pc(f"projectors.{i}._net.0"), pc(f"projectors.{i}._net.2")) for i in range(4)]
        self.attr = [(pc(f"attractors.{i}._net.0"), pc(f"attractors.{i}._net.2")) for i in range(4)]
        # CLB input buffer layout: [last 0..31 | emb 32..159 | rel 160 (+7 pad)]; the reference order is
        # cat([last(32), rel(1)], emb(128)) (zoedepth_v1.py:207-213, dist_layers.py:110)
        if with_rel:
            cmap, ctot = [(0, 32, 0), (32, 1, 32 + self.emb), (33, self.emb, 32)], 32 + self.emb + 8
        else:  # fusion head: rel_cond is all zeros (patchfusion.py:300) -> its column drops out exactly
            cmap, ctot = [(0, 32, 0), (33, self.emb, 32)], 32 + self.emb
        self.clb_channels, self.clb_map = ctot, cmap
        self.mlp0 = pc("conditional_log_binomial.mlp.0", cin_map=cmap, cin_total=ctot)
        self.mlp2 = pc("conditional_log_binomial.mlp.2")
        # float32: resize-into-CLB + mlp.0 + mlp.2 + log-binomial as ONE kernel (pf_bins_tail) when the head has the shipped shape
        self.tail = None
        if dtype == F32 and self.n_bins == 64 and bins_tail_enabled():
            self.tail = pk.bins_tail_weights(self.mlp0, self.mlp2, self.emb)
            if self.tail is not None:
                self.tail = self.tail.to(device)
        self._bwd = None                                            # transposed packs of the backward, built on its first use

    def refresh(self, sd):
        """repack the head's 22 layers (and the fused tail's weights) from updated parameters, e.g. after optimizer.step(); the rest of the
        engine is untouched.  ``sd``: a state dict with this head's keys under its prefix."""
        new = object.__new__(BinsHead)
        new.__dict__.update(self.__dict__)
        new._pack(sd)                                               # fresh packs on `new`; this head's own are overwritten IN PLACE below, so
        for a, b in zip(self._packs(), new._packs()):               # cached conv plans (hip_ops keys them by the pack object) stay valid
            _copy_pack(a, b)
        if self._bwd is not None:
            for k, (_, _, t0, t2) in self._bwd.items():
                _copy_pack(t0, new._bwd_packs()[k][2])
                _copy_pack(t2, new._bwd_packs()[k][3])

    def _packs(self):
        flat = [self.sbr0, self.sbr2, self.sp0, self.sp2] + [p for pair in self.proj + self.attr for p in pair] + [self.mlp0, self.mlp2]
        return flat + ([self.tail] if self.tail is not None else [])

    @staticmethod
    def param_names():
        """the head's 44 checkpoint tensors, below its prefix"""
        mlps = ["seed_bin_regressor", "seed_projector"] + [f"{k}.{i}" for k in ("projectors", "attractors") for i in range(4)]
        layers = [f"{m}._net.{j}" for m in mlps for j in (0, 2)] + [f"conditional_log_binomial.mlp.{j}" for j in (0, 2)]
        return [f"{l}.{t}" for l in layers for t in ("weight", "bias")]

    def check_trainable(self):
        """what :meth:`backward` does not cover, refused before any launch"""
        if self.seed_bounded or self.attr_bounded:
            raise NotImplementedError("head backward: bin_centers_type 'normed' / 'hybrid1' / 'hybrid2' (bounded centres: the backward would go "
                                      "through a sort) is not implemented; only 'softplus'")
        if self.dtype != F32:
            raise NotImplementedError("head backward: compute_dtype='bf16' is not implemented; build the model with compute_dtype='fp32'")

    def new_clb_buffer(self, ops, B, H, W):
        return ops.empty((B, H, W, self.clb_channels), self.dtype, self.device)

    def run(self, ops, x0, x_blocks, clb, taps=None, save=None):
        """x0 [B,h0,w0,C]; x_blocks 4 maps low->high; clb: buffer whose [..., :32] already holds `last`
        (and [..., 160:168] the relative depth when with_rel).  Returns depth f32 [B,H,W].
        ``save``: a dict that receives what :meth:`backward` needs (every layer's input, the attractor points A, each low-resolution b_prev,
        pt and the last centres).  With it the head takes the unfused route -- pf_bins_tail keeps no pt -- so its depth is bit for bit that
        of PF_BINS_TAIL=0; without it nothing changes."""
        dt, dev = self.dtype, self.device
        if save is not None:
            self.check_trainable()
            save.update(mlps={}, layers=[])
        B, h0, w0, _ = x0.shape
        t = ops.empty((B, h0, w0, self.sbr0.cout), dt, dev)
        ops.conv(x0, self.sbr0, t, act="relu")
        b_prev = ops.empty((B, h0, w0, self.n_bins), F32, dev)
        ops.conv(t, self.sbr2, b_prev, act="relu" if self.seed_bounded else "softplus")
        if save is not None:
            save["mlps"]["seed_bin_regressor"] = (x0, t, b_prev)
        if self.seed_bounded or self.attr_bounded:                  # localbins_layers.py:52-68, zoedepth_v1.py:178-182
            b_prev = ops.seed_bin_centers(b_prev, ops.empty((B, h0, w0, self.n_bins), F32, dev), self.lo, self.hi,
                                          bounded=self.seed_bounded, normalize=self.attr_bounded)
        t = ops.empty((B, h0, w0, self.sp0.cout), dt, dev)
        ops.conv(x0, self.sp0, t, act="relu")
        prev_emb = ops.empty((B, h0, w0, self.emb), dt, dev)
        ops.conv(t, self.sp2, prev_emb)
        if save is not None:
            save["mlps"]["seed_projector"] = (x0, t, prev_emb)
        emb = prev_emb
        for i, xb in enumerate(x_blocks):
            _, h, w, _ = xb.shape
            p0, p2 = self.proj[i]
            t = ops.empty((B, h, w, p0.cout), dt, dev)
            ops.conv(xb, p0, t, act="relu")
            emb = ops.empty((B, h, w, self.emb), dt, dev)
            ops.conv(t, p2, emb)
            if save is not None:
                save["mlps"][f"projectors.{i}"] = (xb, t, emb)
            xs = ops.empty((B, h, w, self.emb), dt, dev)
            ops.resize(prev_emb, xs, add=emb)                       # x = emb + up(prev_emb)
            a0, a2 = self.attr[i]
            t = ops.empty((B, h, w, a0.cout), dt, dev)
            ops.conv(xs, a0, t, act="relu")
            A = ops.empty((B, h, w, a2.cout), F32, dev)
            ops.conv(t, a2, A, act="relu" if self.attr_bounded else "softplus")
            b_new = ops.empty((B, h, w, self.n_bins), F32, dev)
            if self.attr_bounded:                                   # attractor.py:100-106: even channels, ReLU + 1e-3
                ops.attractor(A, self.n_attr[i], b_prev, b_new, a_stride=2, a_eps=1e-3, attractor_type=self.attr_type, kind=self.attr_kind)
            else:
                ops.attractor(A, self.n_attr[i], b_prev, b_new, attractor_type=self.attr_type, kind=self.attr_kind)
            if save is not None:
                save["mlps"][f"attractors.{i}"] = (xs, t, A)
                save["layers"].append((A, b_prev, tuple(prev_emb.shape[1:3])))
            b_prev, prev_emb = b_new, emb
            if taps is not None:
                taps[f"bins_centers{i}"] = b_new
        _, H, W, _ = clb.shape
        if self.tail is not None and emb.is_contiguous() and save is None:
            if self.attr_bounded:
                b_prev = ops.bounded_bin_centers(b_prev, ops.empty(tuple(b_prev.shape), F32, dev), self.lo, self.hi)
            depth = ops.empty((B, H, W), F32, dev)
            ops.bins_tail(clb, emb, self.tail, b_prev, depth, self.min_temp, self.max_temp)
            return depth
        ops.resize(emb, clb[..., 32:32 + self.emb])                 # b_embedding upsampled to (H, W)
        t = ops.empty((B, H, W, self.mlp0.cout), dt, dev)
        ops.conv(clb, self.mlp0, t, act="gelu")
        pt = ops.empty((B, H, W, self.mlp2.cout), F32, dev)
        ops.conv(t, self.mlp2, pt, act="softplus")
        depth = ops.empty((B, H, W), F32, dev)
        if self.attr_bounded:                                       # attractor.py:132-135: the last layer's scaled, sorted, clipped centres
            b_prev = ops.bounded_bin_centers(b_prev, ops.empty(tuple(b_prev.shape), F32, dev), self.lo, self.hi)
        ops.logbinom_depth(pt, b_prev, depth, self.min_temp, self.max_temp)
        if save is not None:
            save.update(clb=clb, t=t, pt=pt, centers=b_prev, emb_hw=tuple(emb.shape[1:3]))
        return depth

    # ---- backward (csrc/head_bwd.hip; float32, 'softplus' centres) ----
    def _bwd_packs(self):
        """W^T of every layer, packed like a forward weight: the data gradient dX = dY W is the forward 1x1 kernel on it.  Taken from the
        forward pack, so mlp.0's is in the CLB buffer's channel order.  Input channels (= the layer's outputs) are padded to 8 with zero
        weights; the gradient buffers are padded to match and zero there."""
        if self._bwd is None:
            def tr(pc):
                w = pc.w[:pc.cout_real, :pc.cin].float().t().contiguous()            # [cin_total, N]
                return pk.pack_conv(w, None, dtype=F32).to(self.device)
            named = {"seed_bin_regressor": (self.sbr0, self.sbr2), "seed_projector": (self.sp0, self.sp2)}
            for i in range(4):
                named[f"projectors.{i}"], named[f"attractors.{i}"] = self.proj[i], self.attr[i]
            self._bwd = {k: (p0, p2, tr(p0), tr(p2)) for k, (p0, p2) in named.items()}
            self._bwd["clb"] = (self.mlp0, self.mlp2, tr(self.mlp0), tr(self.mlp2))
        return self._bwd

    def _wgrad(self, ops, name, pc, dy, x, grads, cmap=None):
        """grads[name.weight / .bias] of one 1x1 layer: dy [..., N] (a view of the padded gradient buffer), x the layer's input buffer"""
        N, dev = pc.cout_real, self.device
        dw, db = ops.empty((N, x.shape[-1]), F32, dev), ops.empty((N,), F32, dev)
        ops.conv1x1_wgrad(dy, x, dw, db)
        if cmap is not None:                                        # mlp.0: from the CLB buffer's channel order back to the checkpoint's
            full = ops.zeros((N, 33 + self.emb), F32, dev)          # (the fusion head's rel column reads zeros: zero gradient)
            for s0, n, d0 in cmap:
                full[:, s0:s0 + n] = dw[:, d0:d0 + n]
            dw = full
        grads[name + ".weight"], grads[name + ".bias"] = dw.view(N, dw.shape[1], 1, 1), db

    def _mlp_bwd(self, ops, key, saved, dy_buf, grads, act_out=None, res=None):
        """backward of Conv1x1 - ReLU - Conv1x1 [- Softplus].  dy_buf: the gradient of the output, channels padded to 8 (zeros in the padding).
        -> the gradient of the input (+ res)"""
        p0, p2, p0t, p2t = self._bwd_packs()[key]
        x, h, y = saved[key]
        dy = dy_buf[..., :p2.cout_real]
        if act_out is not None:
            ops.act_bwd(dy, y, act_out)
        self._wgrad(ops, key + "._net.2", p2, dy, h, grads)
        dh = ops.empty(tuple(h.shape), F32, self.device)
        ops.conv(dy_buf, p2t, dh)
        ops.act_bwd(dh, h, "relu")
        self._wgrad(ops, key + "._net.0", p0, dh, x, grads)
        dx = ops.empty(tuple(x.shape), F32, self.device)
        ops.conv(dh, p0t, dx, res=res)
        return dx

    def backward(self, ops, ctx, d_depth):
        """ctx: the dict :meth:`run` filled through ``save``; d_depth f32 [B,H,W] (contiguous).  -> (param_grads, input_grads):
        param_grads keyed by the checkpoint names below this head's prefix ('seed_bin_regressor._net.0.weight', ...: 22 layers, 44 tensors),
        input_grads = {'x0', 'x_blocks' (list, low -> high), 'last'[, 'rel']} (NHWC; 'last' and 'rel' are channel slices of one buffer).
        Fixed summation orders throughout: two calls on one context give identical bits."""
        self.check_trainable()
        dev, sv, grads = self.device, ctx["mlps"], {}
        clb, pt, centers = ctx["clb"], ctx["pt"], ctx["centers"]
        B, H, W, _ = clb.shape
        mlp0, mlp2, mlp0t, mlp2t = self._bwd_packs()["clb"]
        # log-binomial expectation -> pt and the last centres
        d_pt = ops.zeros((B, H, W, 8), F32, dev)
        d_cup = ops.empty((B, H, W, self.n_bins), F32, dev)
        ops.logbinom_depth_bwd(pt, centers, d_depth, d_pt[..., :4], d_cup, self.min_temp, self.max_temp)
        g = ops.empty(tuple(centers.shape), F32, dev)
        ops.resize_bwd(d_cup, g)
        d_cup = None
        # mlp.2 (softplus), mlp.0 (gelu: the pre-activation is recomputed, the forward keeps only its output)
        ops.act_bwd(d_pt[..., :4], pt, "softplus")
        self._wgrad(ops, "conditional_log_binomial.mlp.2", mlp2, d_pt[..., :4], ctx["t"], grads)
        d_t = ops.empty(tuple(ctx["t"].shape), F32, dev)
        ops.conv(d_pt, mlp2t, d_t)
        t_pre = ops.empty(tuple(ctx["t"].shape), F32, dev)
        ops.conv(clb, mlp0, t_pre)
        ops.act_bwd(d_t, t_pre, "gelu")
        t_pre = None
        self._wgrad(ops, "conditional_log_binomial.mlp.0", mlp0, d_t, clb, grads, cmap=self.clb_map)
        d_clb = ops.empty(tuple(clb.shape), F32, dev)
        ops.conv(d_t, mlp0t, d_clb)
        inp = {"last": d_clb[..., :32]}
        if self.with_rel:
            inp["rel"] = d_clb[..., 32 + self.emb:33 + self.emb]
        d_emb_up = d_clb[..., 32:32 + self.emb]                     # gradient of the up-sampled embedding
        # attractor layers, last to first.  total gradient of emb_i = d_xs_i + up^T(what reads emb_i later): the later reader is the tail
        # (i = 3) or layer i + 1's x = emb_{i+1} + up(emb_i)
        later, d_blocks = d_emb_up, [None] * len(ctx["layers"])
        for i in reversed(range(len(ctx["layers"]))):
            A, b_prev, prev_hw = ctx["layers"][i]
            n_attr = self.n_attr[i]
            dA = ops.zeros(tuple(A.shape[:3]) + ((n_attr + 7) // 8 * 8,), F32, dev)
            d_bc = ops.empty(tuple(A.shape[:3]) + (self.n_bins,), F32, dev)
            ops.attractor_bwd(A, n_attr, b_prev, g, dA[..., :n_attr], d_bc, attractor_type=self.attr_type, kind=self.attr_kind)
            g = ops.empty(tuple(b_prev.shape), F32, dev)
            ops.resize_bwd(d_bc, g)
            d_xs = self._mlp_bwd(ops, f"attractors.{i}", sv, dA, grads, act_out="softplus")
            d_emb = ops.empty(tuple(d_xs.shape), F32, dev)
            ops.copy_channels(d_xs, d_emb)
            ops.resize_bwd(later, d_emb, accumulate=True)
            d_blocks[i] = self._mlp_bwd(ops, f"projectors.{i}", sv, d_emb, grads)
            later = d_xs
        d_prev = ops.empty((B,) + tuple(ctx["layers"][0][2]) + (self.emb,), F32, dev)
        ops.resize_bwd(later, d_prev)
        dx0 = self._mlp_bwd(ops, "seed_projector", sv, d_prev, grads)
        inp["x0"] = self._mlp_bwd(ops, "seed_bin_regressor", sv, g, grads, act_out="softplus", res=dx0)
        inp["x_blocks"] = d_blocks
        return grads, inp


class BranchNet:
    """One ZoeDepth branch with a Depth-Anything (DINOv2 ViT + DPT) core."""

    def __init__(self, sd, prefix, bcfg, process_shape, dtype, device, ops=None, crops=False):
        self.dtype, self.device = dtype, device
        enc = bcfg["midas_model_type"]
        self.D, self.depth, self.heads = VIT_ARCH[enc]
        self.C, self.oc = DPT_ARCH[enc]
        self.H, self.W = process_shape
        self.th, self.tw = self.H // 14, self.W // 14
        v = prefix + "core.core.pretrained."
        h = prefix + "core.core.depth_head."
        dev = device

        def pc(name, bias=True, **kw):
            return pk.pack_conv(sd[name + ".weight"], sd[name + ".bias"] if bias else None, dtype=dtype, **kw).to(dev)

        w = sd[v + "patch_embed.proj.weight"]
        self.pe = pk.pack_conv(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1), sd[v + "patch_embed.proj.bias"], dtype=dtype,
                               cin_total=592).to(dev)
        self.pos = pk.vit_pos_embed(sd[v + "pos_embed"], self.th, self.tw).to(dev)
        self.cls = _g(sd, v + "cls_token", dev).reshape(-1)
        # float32 compute: the encoder's four linear layers per block run as split-precision GEMMs on the bf16 matrix cores (x = h + m + l,
        # six partial products, float32 accumulation: csrc/gemm_split3.hip; float32-grade error, measured against float64 in
        # tests/op_checks.py gemm_split3).  PF_LINEAR_SPLIT3=0 keeps them on the float32 MFMA.
        self.split3 = dtype == F32 and linear_split3_enabled()
        if self.split3:
            def pc(name, bias=True, _pc=pc, **kw):           # (only the block linears below are re-routed)
                if ".blocks." in name:
                    return pk.pack_conv_split3(sd[name + ".weight"], sd[name + ".bias"] if bias else None, **kw).to(dev)
                return _pc(name, bias, **kw)
        # ... and, when the op set has the fp16x2 linears (the HIP ops do; PF_VIT_F16X2=0 keeps bf16x3), qkv / fc1 / fc2 run on two fp16 planes
        # with static power-of-two scales derived from the weights (packing.pack_conv_f16x2): only those planes are packed for them.  The
        # projection keeps the bf16x3 planes the attention writes unless the attention moves too (attn_f16x2 below).
        # (crops: this branch runs batches of crops -- the fine branch -- rather than one image per call)
        self.f16x2 = self.split3 and vit_f16x2_enabled(crops) and getattr(ops, "conv_f16x2", None) is not None
        # ... and with them (PF_VIT_ATTN_F16X2, crops only) the attention and the projection: q / k / v and the attention output then travel as two
        # fp16 planes as well, with static exponents (packing.vit_attn_f16x2_scales), and the projection's bf16x3 planes are not packed
        self.attn_f16x2 = (self.f16x2 and crops and vit_attn_f16x2_enabled() != 0 and attention_split3_enabled() and pk.split3_kmajor_enabled()
                           and getattr(ops, "vit_attention_f16x2", None) is not None)
        self.proj_f16x2 = self.attn_f16x2 and vit_attn_f16x2_enabled() == 2
        self.blocks = []
        for i in range(self.depth):
            b = f"{v}blocks.{i}."
            n1, n2 = (sd[b + "norm1.weight"], sd[b + "norm1.bias"]), (sd[b + "norm2.weight"], sd[b + "norm2.bias"])
            if self.f16x2:
                bn1, bn2 = pk.layernorm_bound(*n1), pk.layernorm_bound(*n2)
                w1, b1 = sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"]
                qkv = pk.pack_conv_f16x2(sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"], None, bn1).to(dev)
                fc1 = pk.pack_conv_f16x2(w1, b1, None, bn2).to(dev)
                fc2 = pk.pack_conv_f16x2(sd[b + "mlp.fc2.weight"], sd[b + "mlp.fc2.bias"], sd[b + "ls2.gamma"],
                                         pk.gelu_linear_bound(w1, b1, bn2)).to(dev)
            else:
                qkv, fc1, fc2 = pc(b + "attn.qkv"), pc(b + "mlp.fc1"), pc(b + "mlp.fc2", scale=sd[b + "ls2.gamma"])
            attn = None
            if self.attn_f16x2:
                attn = pk.vit_attn_f16x2_scales(sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"], bn1, self.heads)
                if self.proj_f16x2:
                    proj = pk.pack_conv_f16x2(sd[b + "attn.proj.weight"], sd[b + "attn.proj.bias"], sd[b + "ls1.gamma"], attn.v_bound).to(dev)
                else:
                    proj = pc(b + "attn.proj", scale=sd[b + "ls1.gamma"])
                attn = attn.to(dev)
            else:
                proj = pc(b + "attn.proj", scale=sd[b + "ls1.gamma"])
            self.blocks.append(dict(
                n1=(_g(sd, b + "norm1.weight", dev), _g(sd, b + "norm1.bias", dev)),
                qkv=qkv,
                attn=attn,
                proj=proj,
                n2=(_g(sd, b + "norm2.weight", dev), _g(sd, b + "norm2.bias", dev)),
                fc1=fc1,
                fc2=fc2))
        self.norm = (_g(sd, v + "norm.weight", dev), _g(sd, v + "norm.bias", dev))
        self.projects = [pc(f"{h}projects.{i}") for i in range(4)]
        self.up4 = pk.pack_conv_transpose(sd[h + "resize_layers.0.weight"], sd[h + "resize_layers.0.bias"], dtype=dtype).to(dev)
        self.up2 = pk.pack_conv_transpose(sd[h + "resize_layers.1.weight"], sd[h + "resize_layers.1.bias"], dtype=dtype).to(dev)
        self.down2 = pc(h + "resize_layers.3")
        self.rn = [pc(f"{h}scratch.layer{i + 1}_rn", bias=False) for i in range(4)]
        self.refine = {}
        for i in range(1, 5):
            r = f"{h}scratch.refinenet{i}."
            self.refine[i] = dict(out=pc(r + "out_conv"),
                                  u1=(pc(r + "resConfUnit1.conv1"), pc(r + "resConfUnit1.conv2")),
                                  u2=(pc(r + "resConfUnit2.conv1"), pc(r + "resConfUnit2.conv2")))
        self.oc1 = pc(h + "scratch.output_conv1")
        self.oc2a = pc(h + "scratch.output_conv2.0")
        self.oc2b = pk.pack_conv(sd[h + "scratch.output_conv2.2.weight"], sd[h + "scratch.output_conv2.2.bias"], dtype=dtype).to(dev)
        # widen the 1-channel relative-depth conv to 8 stored channels so it fills the CLB buffer's
        # padded tail [160:168) (zero weights / zero bias / ReLU -> zeros) without a memset
        self.oc2b.cout = 8
        self.conv2 = pc(prefix + "conv2")
        self.head = BinsHead(sd, prefix, self.C, bcfg, dtype, dev, with_rel=True)

    # ---- pieces ----
    def _rcu(self, ops, x, unit, extra_res=None):
        """x + conv2(relu(conv1(relu(x)))) [+ extra_res]  (blocks.py:69-92; ReLUs are non in-place)"""
        c1, c2 = unit
        t = ops.empty(x.shape[:3] + (c1.cout,), self.dtype, self.device)
        y = ops.empty(x.shape[:3] + (c2.cout,), self.dtype, self.device)
        chain = getattr(ops, "conv_chain", None)
        if chain is not None:                                      # t is read by conv2 alone: conv1 hands over its channel maxima (hip_ops.conv_chain)
            return chain(x, c1, t, c2, y, dict(pad=1, act="relu", relu_in=True), dict(pad=1, res=x, res2=extra_res))
        ops.conv(x, c1, t, pad=1, act="relu", relu_in=True)
        ops.conv(t, c2, y, pad=1, res=x, res2=extra_res)
        return y

    def _refine(self, ops, idx, x, skip, size):
        r = self.refine[idx]
        if skip is not None:
            x = self._rcu(ops, skip, r["u1"], extra_res=x)          # xs[0] + RCU1(xs[1])
        x = self._rcu(ops, x, r["u2"])
        B, _, _, Cc = x.shape
        u = ops.empty((B, size[0], size[1], Cc), self.dtype, self.device)
        ops.resize(x, u)
        y = ops.empty((B, size[0], size[1], r["out"].cout), self.dtype, self.device)
        ops.conv(u, r["out"], y)
        return y

    def vit(self, ops, img, taps=None):
        dt, dev = self.dtype, self.device
        B = img.shape[0]
        T, S, D = self.th * self.tw, self.th * self.tw + 1, self.D
        col = ops.empty((B * T, 592), dt, dev)
        ops.patch_im2col(img, col)
        emb = ops.empty((B * T, D), dt, dev)
        ops.conv(col, self.pe, emb)
        tok = ops.empty((B, S, D), dt, dev)
        ops.assemble_tokens(emb, tok, self.cls, self.pos)
        x = tok.view(B * S, D)
        if taps is not None:
            taps["vit_tokens_in"] = tok.clone()
        feats = []
        if self.split3:                                            # operands of the split GEMMs travel as three bf16 planes ...
            if pk.split3_kmajor_enabled():                         # ... chunk-major [3, K/32, rows, 32]: whole-cache-line DMA pieces (csrc/gemm_split3.hip)
                hbuf, att, mid = (ops.empty((3, n // 32, B * S, 32), torch.bfloat16, dev) for n in (D, D, 4 * D))
            else:
                hbuf, att, mid = (ops.empty((3, B * S, n), torch.bfloat16, dev) for n in (D, D, 4 * D))
            # ... and so do q / k / v (row-major: the attention kernel reads token rows): attention in split precision (csrc/vit.hip)
            qkv = ops.empty((3, B * S, 3 * D), torch.bfloat16, dev) if attention_split3_enabled() else ops.empty((B * S, 3 * D), dt, dev)
            if self.f16x2:                                         # LayerNorm outputs and the fc1 -> fc2 intermediate as two fp16 planes, chunk-major
                hbuf, mid = (ops.empty((2, n // 32, B * S, 32), torch.float16, dev) for n in (D, 4 * D))
            if self.attn_f16x2:                                    # ... and q / k / v (row-major); the attention output too when the projection follows suit
                qkv = ops.empty((2, B * S, 3 * D), torch.float16, dev)
                if self.proj_f16x2:
                    att = ops.empty((2, D // 32, B * S, 32), torch.float16, dev)
        else:
            hbuf = ops.empty((B * S, D), dt, dev)
            qkv = ops.empty((B * S, 3 * D), dt, dev)
            att = ops.empty((B * S, D), dt, dev)
            mid = ops.empty((B * S, 4 * D), dt, dev)
        for i, blk in enumerate(self.blocks):
            if self.f16x2:
                ops.layernorm_f16x2(x, hbuf, blk["n1"][0], blk["n1"][1], 1e-6, blk["qkv"].in_exp)
                if self.attn_f16x2:
                    ops.conv_f16x2(hbuf, blk["qkv"], qkv, out_exp=blk["attn"].out_exp)
                    if self.proj_f16x2:
                        ops.vit_attention_f16x2(qkv, att, B, S, self.heads, blk["attn"].qk_exp)
                        ops.conv_f16x2(att, blk["proj"], x, res=x)
                    else:
                        ops.vit_attention_f16x2(qkv, att, B, S, self.heads, blk["attn"].qk_exp, v_exp=blk["attn"].v_exp)
                        ops.conv_split3(att, blk["proj"], x, res=x)
                else:
                    ops.conv_f16x2(hbuf, blk["qkv"], qkv)
                    ops.vit_attention(qkv, att, B, S, self.heads)
                    ops.conv_split3(att, blk["proj"], x, res=x)
                ops.layernorm_f16x2(x, hbuf, blk["n2"][0], blk["n2"][1], 1e-6, blk["fc1"].in_exp)
                ops.conv_f16x2(hbuf, blk["fc1"], mid, act="gelu", out_exp=blk["fc2"].in_exp)
                ops.conv_f16x2(mid, blk["fc2"], x, res=x)
            elif self.split3:
                ops.layernorm_split3(x, hbuf, blk["n1"][0], blk["n1"][1], 1e-6)
                ops.conv_split3(hbuf, blk["qkv"], qkv)
                ops.vit_attention(qkv, att, B, S, self.heads)
                ops.conv_split3(att, blk["proj"], x, res=x)
                ops.layernorm_split3(x, hbuf, blk["n2"][0], blk["n2"][1], 1e-6)
                ops.conv_split3(hbuf, blk["fc1"], mid, act="gelu")
                ops.conv_split3(mid, blk["fc2"], x, res=x)
            else:
                ops.layernorm(x, hbuf, blk["n1"][0], blk["n1"][1], 1e-6)
                ops.conv(hbuf, blk["qkv"], qkv)
                ops.vit_attention(qkv, att, B, S, self.heads)
                ops.conv(att, blk["proj"], x, res=x)                   # x += ls1 * proj(attn)
                ops.layernorm(x, hbuf, blk["n2"][0], blk["n2"][1], 1e-6)
                ops.conv(hbuf, blk["fc1"], mid, act="gelu")
                ops.conv(mid, blk["fc2"], x, res=x)                    # x += ls2 * fc2(gelu(fc1))
            if taps is not None and i in (0, self.depth - 1):
                taps[f"vit_block{i}"] = x.view(B, S, D).clone()
            if i >= self.depth - 4:
                f = ops.empty((B, self.th, self.tw, D), dt, dev)
                ops.layernorm(x, f.view(B * T, D), self.norm[0], self.norm[1], 1e-6, batches=B, in_rows_per_batch=S,
                              in_row_offset=1, out_rows_per_batch=T)
                feats.append(f)
        return feats

    def forward(self, ops, img, taps=None, vit_feats=None, head_save=None):
        """img [B,3,H,W] float32 in [0,1] -> (depth f32 [B,H,W], feats low->high
        [x_d0, r4, r3, r2, r1, out_conv(32)]).  ``vit_feats``: the four encoder outputs of these B images when the caller has already
        run :meth:`vit` on a larger batch (all tiles of an image in one launch per layer: fewer, better-filled GEMM launches).
        ``head_save``: BinsHead.run's ``save``."""
        dt, dev = self.dtype, self.device
        B = img.shape[0]
        th, tw, C = self.th, self.tw, self.C
        feats = self.vit(ops, img, taps) if vit_feats is None else vit_feats
        if taps is not None:
            for i, f in enumerate(feats):
                taps[f"vit_out{i}"] = f
        maps = []
        for i, f in enumerate(feats):
            p = ops.empty((B, th, tw, self.projects[i].cout), dt, dev)
            ops.conv(f, self.projects[i], p)
            if i == 0:
                y = ops.empty((B, th * 4, tw * 4, self.oc[0]), dt, dev)
                ops.conv(p, self.up4, y)
            elif i == 1:
                y = ops.empty((B, th * 2, tw * 2, self.oc[1]), dt, dev)
                ops.conv(p, self.up2, y)
            elif i == 2:
                y = p
            else:
                y = ops.empty((B, (th + 1) // 2, (tw + 1) // 2, self.oc[3]), dt, dev)
                ops.conv(p, self.down2, y, stride=2, pad=1)
            maps.append(y)
        rn = []
        for i in range(4):
            y = ops.empty(maps[i].shape[:3] + (C,), dt, dev)
            ops.conv(maps[i], self.rn[i], y, pad=1)
            rn.append(y)
        r4 = self._refine(ops, 4, rn[3], None, rn[2].shape[1:3])
        r3 = self._refine(ops, 3, r4, rn[2], rn[1].shape[1:3])
        r2 = self._refine(ops, 2, r3, rn[1], rn[0].shape[1:3])
        r1 = self._refine(ops, 1, r2, rn[0], (rn[0].shape[1] * 2, rn[0].shape[2] * 2))
        o1 = ops.empty(r1.shape[:3] + (self.oc1.cout,), dt, dev)
        ops.conv(r1, self.oc1, o1, pad=1)
        H, W = th * 14, tw * 14
        o1u = ops.empty((B, H, W, self.oc1.cout), dt, dev)
        ops.resize(o1, o1u)
        clb = self.head.new_clb_buffer(ops, B, H, W)
        out_conv = clb[..., 0:32]
        ops.conv(o1u, self.oc2a, out_conv, pad=1, act="relu")        # hook 'out_conv'
        ops.conv(out_conv, self.oc2b, clb[..., 32 + self.head.emb:], act="relu")   # relative depth (+ zero tail)
        x_d0 = ops.empty(rn[3].shape[:3] + (C,), dt, dev)
        ops.conv(rn[3], self.conv2, x_d0)
        if taps is not None:
            taps.update(dpt_layer1_rn=rn[0], dpt_layer4_rn=rn[3], rel_depth=clb[..., 32 + self.head.emb:33 + self.head.emb])
        depth = self.head.run(ops, x_d0, [r4, r3, r2, r1], clb, taps, save=head_save)
        return depth, [x_d0, r4, r3, r2, r1, out_conv]


def _accepts_dtype(fn):
    """does a provider's forward_nhwc take the compute dtype (midas_core.MidasBeitCore does; an older provider object may not)?"""
    import inspect
    try:
        ps = inspect.signature(fn).parameters
    except (TypeError, ValueError):
        return False
    return "dtype" in ps or any(p.kind == p.VAR_KEYWORD for p in ps.values())


class ExternalCoreBranchNet:
    """ZoeDepth branch whose relative-depth core is EXTERNAL (type 'ZoeDepth': MiDaS DPT_BEiT_L_384, BASELINE configs[4]).

    The MiDaS/BEiT core is not in the reference tree (torch.hub repo AyaanShah2204/MiDaS, no commit pinned, midas.py:340), so
    it is supplied as a feature provider -- the reference's own injection point ``ZoeDepth.forward(hack_feature=(rel_depth,
    out))`` (zoedepth_v1.py:160-166):
        provider(img [B,3,H,W] float32 in [0,1]) -> (rel_depth [B,H,W] f32, [btlnck, x_block0..3, out_conv] NCHW f32)
    with btlnck at H/32 and the blocks at H/16 ... H/2 (256 channels), out_conv 32 channels at HxW.  Everything after the core --
    conv2 and the metric-bins head (zoedepth_v1.py:170-219) -- runs on the HIP op set exactly like the Depth-Anything branch."""

    def __init__(self, sd, prefix, bcfg, process_shape, dtype, device, provider):
        if provider is None:
            raise NotImplementedError(
                "branch type 'ZoeDepth' needs a relative-depth core: the MiDaS/BEiT encoder is an un-vendored torch.hub "
                "repository (midas.py:340).  Pass core_providers=(coarse, fine) to PatchFusion or call set_core_providers().")
        self.dtype, self.device, self.provider = dtype, device, provider
        self.C = branch_channels(bcfg)
        self.H, self.W = process_shape
        self.conv2 = pk.pack_conv(sd[prefix + "conv2.weight"], sd[prefix + "conv2.bias"], dtype=dtype).to(device)
        self.head = BinsHead(sd, prefix, self.C, bcfg, dtype, device, with_rel=True)

    def forward(self, ops, img, taps=None):
        dt, dev = self.dtype, self.device
        if hasattr(self.provider, "forward_nhwc"):               # a native core (midas_core.MidasBeitCore): NHWC straight into the clb buffer
            B, _, H, W = img.shape
            clb = self.head.new_clb_buffer(ops, B, H, W)
            if dt == F32:
                _, feats = self.provider.forward_nhwc(ops, img, out_conv=clb[..., :32], rel=clb[..., 32 + self.head.emb:])
            elif _accepts_dtype(self.provider.forward_nhwc):
                _, feats = self.provider.forward_nhwc(ops, img, out_conv=clb[..., :32], rel=clb[..., 32 + self.head.emb:], dtype=dt)
            else:
                raise NotImplementedError(f"this relative-depth core's forward_nhwc takes no dtype: it runs in float32 only (compute_dtype='fp32'), not {dt}")
            btl, blocks = feats[0], feats[1:5]
            x_d0 = ops.empty(btl.shape[:3] + (self.C,), dt, dev)
            ops.conv(btl, self.conv2, x_d0)
            depth = self.head.run(ops, x_d0, blocks, clb, taps)
            return depth, [x_d0] + blocks + [clb[..., :32]]
        rel, feats = self.provider(img)
        assert len(feats) == 6, "provider must return [btlnck, x_block0..3, out_conv]"
        nhwc = [f.detach().to(dev).permute(0, 2, 3, 1).contiguous().to(dt) for f in feats]      # re-layout only
        btl, blocks, outc = nhwc[0], nhwc[1:5], nhwc[5]
        B, H, W = rel.shape
        clb = self.head.new_clb_buffer(ops, B, H, W)            # [last 0..31 | emb 32..159 | rel 160 (+7 zero pad)]
        ops.copy_channels(outc, clb[..., :32])
        tail = torch.zeros((B, H, W, 8), dtype=dt, device=dev)
        tail[..., 0] = rel.detach().to(device=dev, dtype=dt)
        clb[..., 32 + self.head.emb:] = tail
        x_d0 = ops.empty(btl.shape[:3] + (self.C,), dt, dev)
        ops.conv(btl, self.conv2, x_d0)
        depth = self.head.run(ops, x_d0, blocks, clb, taps)
        return depth, [x_d0] + blocks + [clb[..., :32]]


class G2LNet:
    """The six global-to-local Swin stacks; input = whole-image coarse pyramid, i.e. patch invariant."""
    DEPTH = [4, 4, 3, 3, 2, 2]     # guided_fusion_model.py:109-110 defaults, reversed at :141-143
    HEADS = [32, 32, 16, 16, 8, 8]

    def __init__(self, sd, gcfg, dtype, device, prefix="guided_fusion."):
        self.dtype, self.device = dtype, device
        from .spec import GF_DEFAULT_IN_CHANNELS
        ch = list(gcfg.get("in_channels", GF_DEFAULT_IN_CHANNELS))[::-1]
        self.levels = []
        for i, C in enumerate(ch):
            g = f"{prefix}g2l_list.{i}."
            blocks = []
            for j in range(self.DEPTH[i]):
                b = f"{g}g2l_layer.blocks.{j}."

                def pc(name):
                    return pk.pack_conv(sd[b + name + ".weight"], sd[b + name + ".bias"], dtype=dtype).to(device)
                blocks.append(dict(n1=(_g(sd, b + "norm1.weight", device), _g(sd, b + "norm1.bias", device)),
                                   n2=(_g(sd, b + "norm2.weight", device), _g(sd, b + "norm2.bias", device)),
                                   qkv=pc("attn.qkv"), proj=pc("attn.proj"), fc1=pc("mlp.fc1"), fc2=pc("mlp.fc2"),
                                   bias_table=_g(sd, b + "attn.relative_position_bias_table", device),
                                   shift=0 if j % 2 == 0 else 6))
            self.levels.append(dict(C=C, heads=self.HEADS[i], blocks=blocks,
                                    ape=_g(sd, g + "absolute_pos_embed", device)[0],
                                    norm=(_g(sd, g + "g2l_layer_norm.weight", device), _g(sd, g + "g2l_layer_norm.bias", device))))

    def forward_level(self, ops, i, feat):
        dt, dev = self.dtype, self.device
        lv = self.levels[i]
        B, H, W, C = feat.shape
        Hp, Wp = int(math.ceil(H / 12)) * 12, int(math.ceil(W / 12)) * 12
        nt = B * Hp * Wp
        x = ops.empty((B, H, W, C), dt, dev)
        ops.copy_channels(feat, x)
        ops.add_rowwise(x.view(B, H * W, C), lv["ape"])
        xw = ops.empty((nt, C), dt, dev)
        qkv = ops.empty((nt, 3 * C), dt, dev)
        ao = ops.empty((nt, C), dt, dev)
        pr = ops.empty((nt, C), dt, dev)
        hbuf = ops.empty((B * H * W, C), dt, dev)
        mid = ops.empty((B * H * W, 4 * C), dt, dev)
        for blk in lv["blocks"]:
            ops.swin_ln_partition(x, xw, blk["n1"][0], blk["n1"][1], 1e-5, blk["shift"])
            ops.conv(xw, blk["qkv"], qkv)
            ops.swin_window_attention(qkv, ao, blk["bias_table"], B, Hp, Wp, C, lv["heads"], blk["shift"])
            ops.conv(ao, blk["proj"], pr)
            x2 = ops.empty((B, H, W, C), dt, dev)
            ops.swin_unpartition_add(pr, x, x2, blk["shift"])
            x = x2
            xf = x.view(B * H * W, C)
            ops.layernorm(xf, hbuf, blk["n2"][0], blk["n2"][1], 1e-5)
            ops.conv(hbuf, blk["fc1"], mid, act="gelu")
            ops.conv(mid, blk["fc2"], xf, res=xf)
        out = ops.empty((B, H, W, C), dt, dev)
        ops.layernorm(x.view(B * H * W, C), out.view(B * H * W, C), lv["norm"][0], lv["norm"][1], 1e-5)
        return out

    def forward(self, ops, coarse_feats):
        return [self.forward_level(ops, i, f) for i, f in enumerate(coarse_feats)]


class FusionNet:
    """fusion_conv_list + GuidedFusionPatchFusion U-Net + the fusion-side metric-bins head."""

    def __init__(self, sd, cfg, dtype, device):
        self.dtype, self.device = dtype, device
        fb = cfg["fine_branch"]
        self.C = branch_channels(fb)
        self.ps = tuple(cfg["patch_process_shape"])
        self.sizes = pyramid_sizes(self.ps, fb["type"])[::-1]       # L0..L5 (h, w)
        self.ch = [self.C] * 5 + [32]                               # channels per level L0..L5
        g = "guided_fusion."

        def pc(name, **kw):
            return pk.pack_conv(sd[name + ".weight"], sd.get(name + ".bias"), dtype=dtype, **kw).to(device)

        def bn(name):
            return tuple(sd[f"{name}.{k}"] for k in ("weight", "bias", "running_mean", "running_var"))

        self.fconv = [pc(f"fusion_conv_list.{i}") for i in range(6)]

        def dcbn(name, **kw):
            return (pc(name + ".double_conv.0", bn=bn(name + ".double_conv.1"), **kw),
                    pc(name + ".double_conv.3", bn=bn(name + ".double_conv.4")))

        def dcwobn(name):
            return (pc(name + ".double_conv.0"), pc(name + ".double_conv.2"))

        self.inc = dcbn(g + "inc", cin_total=8)
        self.down = [dcbn(f"{g}down_conv_list.{i}.maxpool_conv.1") for i in range(5)]
        self.upc = [dcwobn(f"{g}up_conv_list.{i}.conv") for i in range(5)]
        self.convs = [dcwobn(f"{g}convs.{i}") for i in range(6)]
        self.head = BinsHead(sd, "", self.C, cfg["coarse_branch"], dtype, device, with_rel=False,
                             min_depth=cfg["min_depth"], max_depth=cfg["max_depth"])

    def forward(self, ops, crops, rois, fine_depth, fine_feats, coarse_depth, coarse_feats, g2l, taps=None, head_save=None):
        """crops [B,3,H,W] f32; rois f32 [B,5] (batch index 0, box in process coordinates);
        fine_depth f32 [B,H,W]; coarse_depth f32 [1,1,H,W]; returns depth f32 [B,H,W]."""
        dt, dev = self.dtype, self.device
        B = crops.shape[0]
        H, W = self.ps
        ch, sizes = self.ch, self.sizes
        # --- coarse ROIs + fusion convs (patchfusion.py:240-267) ---
        cd_roi = ops.empty((B, 1, H, W), F32, dev)
        ops.roi_align_depth(coarse_depth, rois, cd_roi, 1.0)
        # Channel maxima for the fp16x2 Winograd layers (hip_ops.cmax_begin): where the conv that reads a concat buffer would run that form, the
        # kernels that WRITE the buffer merge the per-channel max |value| into one vector, slice by slice, and the conv skips its range pass (a second
        # read of the whole buffer).  The vector is None for every other layer and for an ops backend without cmax_begin: then nothing changes.
        begin = getattr(ops, "cmax_begin", None)
        chain = getattr(ops, "conv_chain", None)

        def cm_kw(cm, c0=None, c1=None):
            return {} if cm is None else {"cmax": cm[c0:c1]}

        def conv_pair(x, c0, t, c1, y, cm, cm_y=None):
            """y = relu(conv(relu(conv(x)))) of a DoubleConv; t is read by the second conv alone, so the first hands over its maxima (conv_chain)"""
            if chain is not None:
                kw = {} if cm is None and cm_y is None else dict(cmax_in=cm, cmax_out=cm_y)
                return chain(x, c0, t, c1, y, dict(pad=1, act="relu"), dict(pad=1, act="relu"), **kw)
            ops.conv(x, c0, t, pad=1, act="relu")
            ops.conv(t, c1, y, pad=1, act="relu")
            return y

        guide = []
        for i in range(6):
            h, w = sizes[i]
            cat = ops.empty((B, h, w, 2 * ch[i]), dt, dev)
            gc = ops.empty((B, h, w, ch[i]), dt, dev)
            cm = begin(cat, self.fconv[i], gc, "cat", pad=1) if begin is not None else None
            ops.roi_align(coarse_feats[i], rois, cat[..., :ch[i]], h / H, **cm_kw(cm, 0, ch[i]))
            ops.copy_channels(fine_feats[i], cat[..., ch[i]:], **cm_kw(cm, ch[i], 2 * ch[i]))
            ops.conv(cat, self.fconv[i], gc, pad=1, **({} if cm is None else {"cmax_in": cm}))
            guide.append(gc)
        # --- encoder (guided_fusion_model.py:178-184) ---
        inp = ops.empty((B, H, W, 8), dt, dev)
        ops.pack_fusion_input(cd_roi, fine_depth, crops, inp)
        u5 = ops.empty((B, H, W, ch[5] + 2 * ch[4]), dt, dev)       # Upv1 concat buffer of the last level
        t = ops.empty((B, H, W, 32), dt, dev)
        ops.conv(inp, self.inc[0], t, pad=1, act="relu")
        e = u5[..., :32]
        ops.conv(t, self.inc[1], e, pad=1, act="relu")
        enc = [e]
        for i in range(5):
            _, hh, ww, cc = enc[-1].shape
            mp = ops.empty((B, hh // 2, ww // 2, cc), dt, dev)
            ops.maxpool2(enc[-1], mp)
            c0, c1 = self.down[i]
            t = ops.empty((B, hh // 2, ww // 2, c0.cout), dt, dev)
            ops.conv(mp, c0, t, pad=1, act="relu")
            e = ops.empty((B, hh // 2, ww // 2, c1.cout), dt, dev)
            ops.conv(t, c1, e, pad=1, act="relu")
            enc.append(e)
        enc = enc[::-1]
        # --- decoder (guided_fusion_model.py:186-205) ---
        clb = self.head.new_clb_buffer(ops, B, H, W)
        fused, temp = [], None
        for i in range(6):
            h, w = sizes[i]
            c = ch[i]
            v = ops.empty((B, h, w, 2 * c), dt, dev)                 # cat[feat_enc, roi_align(g2l)]
            tv_shape = (B, h, w, self.convs[i][0].cout)
            # v's maxima: [the up conv's output transform | roi_align]  (the plan needs an output of tv's layout, not tv itself: it is allocated where
            # it always was, after the up convs, so the peak allocation stays what it was)
            cmv = begin(v, self.convs[i][0], ops.empty(tv_shape, dt, dev), "v", pad=1, act="relu") if begin is not None else None
            if i == 0:
                ops.resize(enc[0], v[..., :c], **cm_kw(cmv, 0, c))
            else:
                cp = ch[i - 1]
                u = u5 if i == 5 else ops.empty((B, h, w, c + 2 * cp), dt, dev)
                c0, c1 = self.upc[i - 1]
                t = ops.empty((B, h, w, c0.cout), dt, dev)
                cmu = begin(u, c0, t, "u", pad=1, act="relu") if begin is not None else None
                # Upv1 concat buffer [enc resized to the DPT grid | up(temp) | up(guide)] in ONE launch (whole rows of u);
                # at the last level enc already sits in u5[..., :32] (the inc conv wrote it there: its maxima take the range pass, on that slice alone)
                if i < 5:
                    ops.resize_concat([enc[i], temp, guide[i - 1]], u, **cm_kw(cmu))
                else:
                    if cmu is not None:
                        ops.absmax(u[..., :c], cmu[:c])
                    ops.resize_concat([temp, guide[i - 1]], u[..., c:], **cm_kw(cmu, c))
                conv_pair(u, c0, t, c1, v[..., :c], cmu, None if cmv is None else cmv[:c])
                t = None                                             # (free the up convs' intermediate before the next allocations, as before)
            ops.roi_align(g2l[i], rois, v[..., c:], h / H, **cm_kw(cmv, c, 2 * c))
            c0, c1 = self.convs[i]
            tv = ops.empty(tv_shape, dt, dev)
            temp = clb[..., :32] if i == 5 else ops.empty((B, h, w, c1.cout), dt, dev)
            conv_pair(v, c0, tv, c1, temp, cmv)
            fused.append(temp)
            if taps is not None:
                taps[f"gf_out{i}"] = temp
        return self.head.run(ops, fused[0], fused[1:5], clb, taps, save=head_save)
