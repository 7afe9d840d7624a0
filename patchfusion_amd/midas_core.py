"""Native relative-depth core of a type-'ZoeDepth' branch: MiDaS v3.1 DPT_BEiT_L_384 on the HIP op set.

The reference wraps this model in MidasCore (external/zoedepth/models/base_models/midas.py:189-316) after fetching it from an
un-vendored torch.hub repository (midas.py:340).  ``MidasBeitCore`` is an opt-in feature provider for engine.ExternalCoreBranchNet
(``PatchFusion(..., core_providers="native")`` or explicit instances); nothing changes for models without it.  It is pinned to the
plain-PyTorch restatement tests/midas_beit_ref.py, which is itself pinned against transformers' BEiT and the reference's own MidasCore
hooks -- not against MiDaS, whose source is not available.

compute_dtype="fp32" (below) is the float32-grade route; compute_dtype="bf16" is the fast mode: the same sequence on plain bfloat16 tensors
(LayerNorm -> bf16 GEMM -> pf_qkv_split + pf_vit_attention_rpb_bf16 -> bf16 GEMM with the residual ...), float32 accumulation, statistics and
bias tables.

Per crop: PrepForMidas normalisation fused into the 16x16 patch im2col (pf_patch_im2col_norm), 24 BEiT blocks whose linears run as
float32-grade split GEMMs (pf_gemm_split3) and whose attention adds the per-layer relative-position bias inside the split attention kernel
(pf_vit_attention_split3_rpb), the readout-'project' rows [token | cls] (pf_readout_concat) through Linear(2D -> D) + GELU at the four hook
blocks, the act_postprocess convs, and the DPT scratch decoder (the same RCU / fusion blocks as the Depth-Anything branch)."""
import torch

from . import packing as pk

F32 = torch.float32
BF16 = torch.bfloat16

# name -> depth, width, heads, hook blocks, reassemble widths, pretrain window, decoder features, input size (H, W)
MIDAS_BEIT_SETTINGS = {
    "DPT_BEiT_L_384": dict(depth=24, D=1024, heads=16, hooks=(5, 11, 17, 23), widths=(256, 512, 1024, 1024), pretrain=24, features=256,
                           img_size=(384, 512)),
}


def native_core_types():
    return tuple(MIDAS_BEIT_SETTINGS)


def checkpoint_keys(s):
    """the MiDaS / timm names of a DPT_BEiT core (without the branch's `core.` prefix), required for loading"""
    keys = ["pretrained.model.cls_token", "pretrained.model.patch_embed.proj.weight", "pretrained.model.patch_embed.proj.bias"]
    for i in range(s["depth"]):
        b = f"pretrained.model.blocks.{i}."
        keys += [b + n for n in ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.q_bias", "attn.v_bias", "attn.relative_position_bias_table",
                                 "attn.proj.weight", "attn.proj.bias", "gamma_1", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias",
                                 "mlp.fc2.weight", "mlp.fc2.bias", "gamma_2")]
    for i in range(4):
        p = f"pretrained.act_postprocess{i + 1}."
        keys += [p + "0.project.0.weight", p + "0.project.0.bias", p + "3.weight", p + "3.bias"]
        if i != 2:
            keys += [p + "4.weight", p + "4.bias"]
    keys += [f"scratch.layer{i + 1}_rn.weight" for i in range(4)]
    for i in range(1, 5):
        r = f"scratch.refinenet{i}."
        units = ("resConfUnit2",) if i == 4 else ("resConfUnit1", "resConfUnit2")
        keys += [f"{r}{u}.{c}.{t}" for u in units for c in ("conv1", "conv2") for t in ("weight", "bias")]
        keys += [r + "out_conv.weight", r + "out_conv.bias"]
    keys += [f"scratch.output_conv.{i}.{t}" for i in (0, 2, 4) for t in ("weight", "bias")]
    return keys


def _ignored(k):
    """checkpoint entries MiDaS creates but never uses: accepted and dropped"""
    return (k.endswith(".attn.relative_position_index") or k.startswith(("pretrained.model.norm.", "pretrained.model.fc_norm.",
                                                                         "pretrained.model.head.", "scratch.refinenet4.resConfUnit1.")))


class MidasBeitCore:
    """Feature provider: ``core(img [B,3,H,W] float32 in [0,1]) -> (rel_depth [B,H,W], [l4_rn, r4, r3, r2, r1, out_conv])`` NCHW, and
    ``forward_nhwc(ops, img, out_conv=None, rel=None, dtype=None)`` for engine.ExternalCoreBranchNet (writes out_conv / rel_depth into its
    buffers; ``dtype`` torch.float32 (default) or torch.bfloat16 = the branch's compute dtype).

    ``settings``: a name of MIDAS_BEIT_SETTINGS or a dict of the same fields.  Weights arrive through ``load_state_dict`` (the `core.`
    sub-dict PatchFusion._load_branch hands to providers, or MiDaS names directly); loading is strict.  In float32 the block linears
    follow PF_LINEAR_SPLIT3 (=0 is refused: the f32 kernel route is not built for this core); in bfloat16 that switch is not consulted.
    The packed weights are cached for ONE (device, dtype) at a time: a forward in the other dtype repacks (PatchFusion.set_compute_dtype)."""

    def __init__(self, settings="DPT_BEiT_L_384", device=None, ops=None):
        self.s = dict(MIDAS_BEIT_SETTINGS[settings]) if isinstance(settings, str) else dict(settings)
        self.device = torch.device(device) if device is not None else None
        self._ops = ops
        self._packed = None
        self._sd = None
        self.call_dtype = F32                    # compute dtype of the NCHW provider protocol (__call__); its results are float32 either way

    # ------------------------------------------------------------------ loading
    def load_state_dict(self, sd, strict=True):
        if not strict:
            raise ValueError("MidasBeitCore loads strictly: a MiDaS naming mistake must fail on the first real checkpoint")
        src = {}
        for k, v in sd.items():
            src[k[len("core."):] if k.startswith("core.") else k] = v
        need = checkpoint_keys(self.s)
        missing = [k for k in need if k not in src]
        known = set(need)
        unexpected = [k for k in src if k not in known and not _ignored(k)]
        if missing or unexpected:
            raise RuntimeError(f"MidasBeitCore.load_state_dict: Missing key(s): {missing[:8]}{' ...' if len(missing) > 8 else ''}; "
                               f"Unexpected key(s): {unexpected[:8]}{' ...' if len(unexpected) > 8 else ''}")
        self._sd = {k: src[k].detach().float().cpu() for k in need}
        self._packed = None
        return self

    def forget_packed(self):
        """drop the packed weights (they are rebuilt, for the dtype then asked for, at the next forward)"""
        self._packed = None

    def _pack(self, device, ops, dtype=F32):
        s, sd = self.s, self._sd
        if sd is None:
            raise RuntimeError("MidasBeitCore has no weights: load_state_dict() first")
        if dtype not in (F32, BF16):
            raise NotImplementedError(f"MidasBeitCore computes in float32 or bfloat16, not {dtype}")
        if dtype == F32 and not (getattr(ops, "conv_split3", None) is not None and _linear_split3_enabled()):
            raise NotImplementedError("MidasBeitCore runs its block linears as split-precision GEMMs only (PF_LINEAR_SPLIT3=0 is not built)")
        H, W = s["img_size"]
        th, tw, D = H // 16, W // 16, s["D"]

        def pc(name, bias=True, **kw):
            return pk.pack_conv(sd[name + ".weight"], sd[name + ".bias"] if bias else None, dtype=dtype, **kw).to(device)

        m = "pretrained.model."
        w = sd[m + "patch_embed.proj.weight"]
        P = dict(th=th, tw=tw)
        P["pe"] = pk.pack_conv(w.permute(0, 2, 3, 1).reshape(D, -1), sd[m + "patch_embed.proj.bias"], dtype=dtype).to(device)
        P["cls"] = sd[m + "cls_token"].reshape(-1).to(device)
        P["zpos"] = torch.zeros((th * tw + 1) * D, dtype=F32, device=device)          # BEiT-L has no absolute position embedding
        blocks = []
        for i in range(s["depth"]):
            b = f"{m}blocks.{i}."
            qb = torch.cat([sd[b + "attn.q_bias"], torch.zeros_like(sd[b + "attn.v_bias"]), sd[b + "attn.v_bias"]])   # k has no bias
            if dtype == BF16:
                blocks.append(pk.pack_beit_block_bf16(sd, b, qb, s["pretrain"], th, tw).to(device))
                continue
            blocks.append(dict(
                n1=(sd[b + "norm1.weight"].to(device), sd[b + "norm1.bias"].to(device)),
                qkv=pk.pack_conv_split3(sd[b + "attn.qkv.weight"], qb).to(device),
                tab=pk.beit_rel_pos_table(sd[b + "attn.relative_position_bias_table"], s["pretrain"], th, tw).to(device),
                proj=pk.pack_conv_split3(sd[b + "attn.proj.weight"], sd[b + "attn.proj.bias"], scale=sd[b + "gamma_1"]).to(device),
                n2=(sd[b + "norm2.weight"].to(device), sd[b + "norm2.bias"].to(device)),
                fc1=pk.pack_conv_split3(sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"]).to(device),
                fc2=pk.pack_conv_split3(sd[b + "mlp.fc2.weight"], sd[b + "mlp.fc2.bias"], scale=sd[b + "gamma_2"]).to(device)))
        P["blocks"] = blocks
        pp = []
        for i in range(4):
            p = f"pretrained.act_postprocess{i + 1}."
            e = dict(readout=pc(p + "0.project.0"), conv=pc(p + "3"))
            if i in (0, 1):
                e["post"] = pk.pack_conv_transpose(sd[p + "4.weight"], sd[p + "4.bias"], dtype=dtype).to(device)
            elif i == 3:
                e["post"] = pc(p + "4")
            pp.append(e)
        P["pp"] = pp
        P["rn"] = [pc(f"scratch.layer{i + 1}_rn", bias=False) for i in range(4)]
        P["refine"] = {}
        for i in range(1, 5):
            r = f"scratch.refinenet{i}."
            P["refine"][i] = dict(out=pc(r + "out_conv"), u2=(pc(r + "resConfUnit2.conv1"), pc(r + "resConfUnit2.conv2")),
                                  u1=None if i == 4 else (pc(r + "resConfUnit1.conv1"), pc(r + "resConfUnit1.conv2")))
        P["oc0"], P["oc2"], P["oc4"] = pc("scratch.output_conv.0"), pc("scratch.output_conv.2"), pc("scratch.output_conv.4")
        P["oc4"].cout = 8        # widen the 1-channel conv to 8 stored channels (zero rows / bias, ReLU -> zeros): fills a clb tail in one store
        P["device"], P["dtype"] = device, dtype
        self._packed = P
        return P

    # ------------------------------------------------------------------ forward
    def _ops_for(self, device):
        if self._ops is None:
            from .hip_ops import ops             # raises if libpf_hip.so is missing: no fallback
            self._ops = ops
        return self._ops

    def __call__(self, img):
        dev = self.device or img.device
        ops = self._ops_for(dev)
        img = img.to(device=dev, dtype=F32)
        rel, feats = self.forward_nhwc(ops, img, dtype=self.call_dtype)
        return rel[..., 0].float().contiguous(), [f.permute(0, 3, 1, 2).float().contiguous() for f in feats]

    def _rcu(self, ops, x, unit, extra_res=None):
        c1, c2 = unit
        t = ops.empty(x.shape[:3] + (c1.cout,), x.dtype, x.device)
        ops.conv(x, c1, t, pad=1, act="relu", relu_in=True)
        y = ops.empty(x.shape[:3] + (c2.cout,), x.dtype, x.device)
        ops.conv(t, c2, y, pad=1, res=x, res2=extra_res)
        return y

    def _refine(self, ops, r, x, skip, size):
        """FeatureFusionBlock_custom: [skip + RCU1(x_skip)] -> RCU2 -> bilinear (align_corners=True) to size -> out_conv"""
        if skip is not None:
            x = self._rcu(ops, skip, r["u1"], extra_res=x)
        x = self._rcu(ops, x, r["u2"])
        B, _, _, Cc = x.shape
        u = ops.empty((B, size[0], size[1], Cc), x.dtype, x.device)
        ops.resize(x, u)
        y = ops.empty((B, size[0], size[1], r["out"].cout), x.dtype, x.device)
        ops.conv(u, r["out"], y)
        return y

    def _hook(self, ops, P, i, x, rc, hooked, B, S, dt):
        th, tw, D = P["th"], P["tw"], self.s["D"]
        for k, hb in enumerate(self.s["hooks"]):                       # hooks: the block outputs themselves (no final LayerNorm)
            if hb == i:
                ops.readout_concat(x, rc, B, S)
                f = ops.empty((B, th, tw, D), dt, x.device)
                ops.conv(rc, P["pp"][k]["readout"], f.view(B * th * tw, D), act="gelu")
                hooked[k] = f

    def forward_nhwc(self, ops, img, out_conv=None, rel=None, dtype=None):
        """img float32 [B,3,H,W] in [0,1] on the GPU -> (rel [B,H,W,8] (channel 0 = rel_depth, 1..7 zero), [l4_rn, r4, r3, r2, r1, out_conv]
        NHWC in ``dtype`` (float32 by default, or bfloat16).  ``out_conv`` / ``rel``: NHWC views [B,H,W,32] / [B,H,W,8] of that dtype to write
        those two maps into (the branch's clb buffer)."""
        dev = img.device
        dt = F32 if dtype is None else dtype
        P = self._packed
        if P is None or P["device"] != dev or P["dtype"] != dt:
            P = self._pack(dev, ops, dt)
        s = self.s
        H, W = s["img_size"]
        B = img.shape[0]
        for buf, C in ((out_conv, 32), (rel, 8)):
            if buf is not None and buf.dtype != dt:
                raise ValueError(f"MidasBeitCore.forward_nhwc: output buffer is {buf.dtype}, the core computes in {dt}")
            if buf is not None and tuple(buf.shape) != (B, H, W, C):
                raise ValueError(f"MidasBeitCore.forward_nhwc: output buffer {tuple(buf.shape)} does not match img_size {(H, W)} (B = {B}, {C} channels)")
        if tuple(img.shape[2:]) != (H, W):              # PrepForMidas's resize (midas.py:171-173): bilinear, align_corners=True
            r = ops.empty((B, 3, H, W), F32, dev)
            src = img.contiguous()
            for b in range(B):
                for c in range(3):
                    ops.resize_bilinear_f32(src[b, c], r[b, c])
            img = r
        img = img.contiguous()
        th, tw, D, heads = P["th"], P["tw"], s["D"], s["heads"]
        T, S = th * tw, th * tw + 1
        col = ops.empty((B * T, 768), dt, dev)
        ops.patch_im2col_norm(img, col, 16, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
        emb = ops.empty((B * T, D), dt, dev)
        ops.conv(col, P["pe"], emb)
        tok = ops.empty((B, S, D), dt, dev)
        ops.assemble_tokens(emb, tok, P["cls"], P["zpos"])
        x = tok.view(B * S, D)
        if dt == BF16:                                   # plain bf16 rows, as BranchNet.vit's bf16 route
            hbuf, att, mid, qkv = (ops.empty((B * S, n), dt, dev) for n in (D, D, 4 * D, 3 * D))
        elif pk.split3_kmajor_enabled():
            hbuf, att, mid = (ops.empty((3, n // 32, B * S, 32), torch.bfloat16, dev) for n in (D, D, 4 * D))
        else:
            hbuf, att, mid = (ops.empty((3, B * S, n), torch.bfloat16, dev) for n in (D, D, 4 * D))
        if dt == F32:
            qkv = ops.empty((3, B * S, 3 * D), torch.bfloat16, dev)
        rc = ops.empty((B * T, 2 * D), dt, dev)
        hooked = [None] * 4
        for i, blk in enumerate(P["blocks"]):
            if dt == BF16:
                ops.layernorm(x, hbuf, blk.n1[0], blk.n1[1], 1e-6)
                ops.conv(hbuf, blk.qkv, qkv)
                ops.vit_attention_rpb_bf16(qkv, att, B, S, heads, blk.tab, th, tw)
                ops.conv(att, blk.proj, x, res=x)                       # x += gamma_1 * proj(attn): gamma folded into the packed weight
                ops.layernorm(x, hbuf, blk.n2[0], blk.n2[1], 1e-6)
                ops.conv(hbuf, blk.fc1, mid, act="gelu")
                ops.conv(mid, blk.fc2, x, res=x)                        # x += gamma_2 * fc2(gelu(fc1))
                self._hook(ops, P, i, x, rc, hooked, B, S, dt)
                continue
            ops.layernorm_split3(x, hbuf, blk["n1"][0], blk["n1"][1], 1e-6)
            ops.conv_split3(hbuf, blk["qkv"], qkv)
            ops.vit_attention_rpb(qkv, att, B, S, heads, blk["tab"], th, tw)
            ops.conv_split3(att, blk["proj"], x, res=x)                 # x += gamma_1 * proj(attn)
            ops.layernorm_split3(x, hbuf, blk["n2"][0], blk["n2"][1], 1e-6)
            ops.conv_split3(hbuf, blk["fc1"], mid, act="gelu")
            ops.conv_split3(mid, blk["fc2"], x, res=x)                  # x += gamma_2 * fc2(gelu(fc1))
            self._hook(ops, P, i, x, rc, hooked, B, S, dt)
        maps = []
        for k, f in enumerate(hooked):
            e = P["pp"][k]
            p = ops.empty((B, th, tw, e["conv"].cout), dt, dev)
            ops.conv(f, e["conv"], p)
            if k == 0:
                y = ops.empty((B, th * 4, tw * 4, e["conv"].cout), dt, dev)
                ops.conv(p, e["post"], y)
            elif k == 1:
                y = ops.empty((B, th * 2, tw * 2, e["conv"].cout), dt, dev)
                ops.conv(p, e["post"], y)
            elif k == 2:
                y = p
            else:
                y = ops.empty((B, (th + 1) // 2, (tw + 1) // 2, e["conv"].cout), dt, dev)
                ops.conv(p, e["post"], y, stride=2, pad=1)
            maps.append(y)
        rn = []
        for k in range(4):
            y = ops.empty(maps[k].shape[:3] + (P["rn"][k].cout,), dt, dev)
            ops.conv(maps[k], P["rn"][k], y, pad=1)
            rn.append(y)
        R = P["refine"]
        r4 = self._refine(ops, R[4], rn[3], None, rn[2].shape[1:3])
        r3 = self._refine(ops, R[3], r4, rn[2], rn[1].shape[1:3])
        r2 = self._refine(ops, R[2], r3, rn[1], rn[0].shape[1:3])
        r1 = self._refine(ops, R[1], r2, rn[0], (rn[0].shape[1] * 2, rn[0].shape[2] * 2))
        o0 = ops.empty(r1.shape[:3] + (P["oc0"].cout,), dt, dev)
        ops.conv(r1, P["oc0"], o0, pad=1)
        o0u = ops.empty((B, H, W, P["oc0"].cout), dt, dev)
        ops.resize(o0, o0u)
        if out_conv is None:
            out_conv = ops.empty((B, H, W, 32), dt, dev)
        ops.conv(o0u, P["oc2"], out_conv, pad=1, act="relu")          # hooked 'out_conv' (output_conv child 3)
        if rel is None:
            rel = ops.empty((B, H, W, 8), dt, dev)
        ops.conv(out_conv, P["oc4"], rel, act="relu")
        return rel, [rn[3], r4, r3, r2, r1, out_conv]


def _linear_split3_enabled():
    from .engine import linear_split3_enabled
    return linear_split3_enabled()


def native_providers(config):
    """``core_providers="native"``: one MidasBeitCore per type-'ZoeDepth' branch, from its midas_model_type (BEiT types only)"""
    out = []
    for br in ("coarse_branch", "fine_branch"):
        bc = config[br]
        if bc.get("type") != "ZoeDepth":
            out.append(None)
            continue
        mt = bc.get("midas_model_type", "DPT_BEiT_L_384")
        if mt not in MIDAS_BEIT_SETTINGS:
            raise NotImplementedError(f"core_providers='native' has no native core for midas_model_type {mt!r} (native: {list(MIDAS_BEIT_SETTINGS)}); "
                                      "pass a provider")
        s = dict(MIDAS_BEIT_SETTINGS[mt])
        if bc.get("img_size") is not None:        # MidasCore runs at the branch's img_size (midas.py:189-201, PrepForMidas)
            size = tuple(int(v) for v in bc["img_size"])
            if len(size) != 2 or size[0] % 32 or size[1] % 32:
                raise ValueError(f"core_providers='native': img_size {size} is not a pair of multiples of 32 (PrepForMidas ensure_multiple_of=32)")
            s["img_size"] = size
        out.append(MidasBeitCore(s))
    return tuple(out)
