"""TEST INFRASTRUCTURE: a plain-PyTorch restatement of MiDaS v3.1's DPT_BEiT_L_384 -- the relative-depth core of a type-'ZoeDepth'
branch (external/zoedepth/models/base_models/midas.py:189-316 wraps it; the model itself is the un-vendored torch.hub repository
named at midas.py:340).  Everything native (patchfusion_amd/midas_core.py, csrc/beit.hip) is pinned to THIS module, and this module
is pinned (tests/test_midas_beit_ref_cpu.py) against transformers' independent BEiT / DPT code and against the reference's own
MidasCore hooks and PrepForMidas -- not against MiDaS itself, whose source is not available.

Submodule names are the MiDaS / timm checkpoint names, so ``state_dict()`` is the key list MidasBeitCore.load_state_dict accepts
(under ``core.``).  The arithmetic restated:
  * timm BEiT blocks: LayerNorm eps 1e-6, qkv bias = [q_bias, 0, v_bias], per-layer relative-position bias whose table is
    interpolated bilinearly (align_corners=False) from the (2*24-1)^2 pretrain grid to (2*th-1, 2*tw-1) with MiDaS v3.1's
    ``reshape(1, old_width, old_height, -1)``, LayerScale gamma_1 / gamma_2, exact-erf GELU MLP; no absolute position embedding;
  * hooks = outputs of blocks [5, 11, 17, 23] (no final LayerNorm), readout 'project': Linear(2D -> D)(cat(token, cls)) + GELU;
  * act_postprocess 1x1 convs + ConvTranspose 4/4, 2/2, identity, 3x3 stride 2; scratch layerN_rn (3x3, no bias);
  * FeatureFusionBlock_custom refinenets (align_corners=True), output_conv = conv3x3, x2 bilinear (align_corners=True), conv3x3,
    ReLU (hooked: 'out_conv'), conv1x1, ReLU.
``provider(img)`` follows engine.ExternalCoreBranchNet's contract: img [B,3,H,W] in [0,1] -> (rel_depth [B,H,W],
[l4_rn, r4, r3, r2, r1, out_conv]) NCHW, after PrepForMidas (mean = std = 0.5, bilinear align_corners=True resize to img_size)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

# name -> (depth, width, heads, hooks, reassemble widths, pretrain window, img_size (H, W))
SETTINGS = {
    "DPT_BEiT_L_384": dict(depth=24, D=1024, heads=16, hooks=(5, 11, 17, 23), widths=(256, 512, 1024, 1024), pretrain=24,
                           features=256, img_size=(384, 512)),
}


def settings(name="DPT_BEiT_L_384", **override):
    s = dict(SETTINGS[name])
    s.update(override)
    return s


def reduced(depth=4, hooks=(0, 1, 2, 3), **kw):
    """full-width L_384 settings with fewer blocks (tests)"""
    return settings(depth=depth, hooks=hooks, **kw)


def gen_relative_position_index(th, tw):
    """generate_relative_position_index (MiDaS v3.1 / transformers BeitRelativePositionBias): [(th*tw+1)^2] into the table"""
    n = (2 * th - 1) * (2 * tw - 1) + 3
    coords = torch.stack(torch.meshgrid(torch.arange(th), torch.arange(tw), indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += th - 1
    rel[:, :, 1] += tw - 1
    rel[:, :, 0] *= 2 * tw - 1
    idx = torch.zeros((th * tw + 1,) * 2, dtype=torch.long)
    idx[1:, 1:] = rel.sum(-1)
    idx[0, 0:] = n - 3
    idx[0:, 0] = n - 2
    idx[0, 0] = n - 1
    return idx


def interpolate_table(table, pretrain, th, tw):
    """_get_rel_pos_bias's table interpolation: [(2p-1)^2 + 3, H] -> [(2th-1)(2tw-1) + 3, H] (same F.interpolate call)"""
    old = 2 * pretrain - 1
    sub = table[: old * old].reshape(1, old, old, -1).permute(0, 3, 1, 2)
    new = F.interpolate(sub, size=(2 * th - 1, 2 * tw - 1), mode="bilinear")
    new = new.permute(0, 2, 3, 1).reshape((2 * th - 1) * (2 * tw - 1), -1)
    return torch.cat([new, table[old * old:]])


def rel_pos_bias(table, pretrain, th, tw):
    """[heads, S, S] bias of one layer at window (th, tw)"""
    t = interpolate_table(table, pretrain, th, tw)
    S = th * tw + 1
    return t[gen_relative_position_index(th, tw).view(-1)].view(S, S, -1).permute(2, 0, 1).contiguous()


class Attention(nn.Module):
    def __init__(self, D, heads, pretrain):
        super().__init__()
        self.heads, self.pretrain = heads, pretrain
        self.qkv = nn.Linear(D, 3 * D, bias=False)
        self.q_bias = nn.Parameter(torch.zeros(D))
        self.v_bias = nn.Parameter(torch.zeros(D))
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * pretrain - 1) ** 2 + 3, heads))
        self.proj = nn.Linear(D, D)

    def forward(self, x, th, tw):
        B, N, C = x.shape
        bias = torch.cat((self.q_bias, torch.zeros_like(self.v_bias), self.v_bias))
        qkv = F.linear(x, self.qkv.weight, bias).reshape(B, N, 3, self.heads, -1).permute(2, 0, 3, 1, 4)
        q, k, v = qkv.unbind(0)
        q = q * (C // self.heads) ** -0.5
        a = q @ k.transpose(-2, -1) + rel_pos_bias(self.relative_position_bias_table, self.pretrain, th, tw).unsqueeze(0)
        return self.proj((a.softmax(-1) @ v).transpose(1, 2).reshape(B, N, C))


class Mlp(nn.Module):
    def __init__(self, D):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(D, 4 * D), nn.Linear(4 * D, D)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class Block(nn.Module):
    def __init__(self, D, heads, pretrain):
        super().__init__()
        self.norm1 = nn.LayerNorm(D, eps=1e-6)
        self.attn = Attention(D, heads, pretrain)
        self.gamma_1 = nn.Parameter(torch.ones(D))
        self.norm2 = nn.LayerNorm(D, eps=1e-6)
        self.mlp = Mlp(D)
        self.gamma_2 = nn.Parameter(torch.ones(D))

    def forward(self, x, th, tw):
        x = x + self.gamma_1 * self.attn(self.norm1(x), th, tw)
        return x + self.gamma_2 * self.mlp(self.norm2(x))


class PatchEmbed(nn.Module):
    def __init__(self, D):
        super().__init__()
        self.proj = nn.Conv2d(3, D, 16, 16)


class Beit(nn.Module):
    def __init__(self, s):
        super().__init__()
        self.cls_token = nn.Parameter(torch.zeros(1, 1, s["D"]))
        self.patch_embed = PatchEmbed(s["D"])
        self.blocks = nn.ModuleList(Block(s["D"], s["heads"], s["pretrain"]) for _ in range(s["depth"]))


class ProjectReadout(nn.Module):
    def __init__(self, D):
        super().__init__()
        self.project = nn.Sequential(nn.Linear(2 * D, D), nn.GELU())

    def forward(self, x):
        return self.project(torch.cat((x[:, 1:], x[:, :1].expand_as(x[:, 1:])), -1))


def _postprocess(D, w, i):
    m = nn.Sequential(ProjectReadout(D), nn.Identity(), nn.Identity(), nn.Conv2d(D, w, 1))   # readout, Transpose, Unflatten (in forward), 1x1
    if i == 0:
        m.append(nn.ConvTranspose2d(w, w, 4, 4))
    elif i == 1:
        m.append(nn.ConvTranspose2d(w, w, 2, 2))
    elif i == 3:
        m.append(nn.Conv2d(w, w, 3, 2, 1))
    return m


class Pretrained(nn.Module):
    def __init__(self, s):
        super().__init__()
        self.model = Beit(s)
        for i, w in enumerate(s["widths"]):
            setattr(self, f"act_postprocess{i + 1}", _postprocess(s["D"], w, i))


class RCU(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.conv1, self.conv2 = nn.Conv2d(C, C, 3, 1, 1), nn.Conv2d(C, C, 3, 1, 1)

    def forward(self, x):
        return self.conv2(F.relu(self.conv1(F.relu(x)))) + x


class Fusion(nn.Module):
    """FeatureFusionBlock_custom(features, ReLU, deconv=False, bn=False, expand=False, align_corners=True)"""

    def __init__(self, C):
        super().__init__()
        self.resConfUnit1, self.resConfUnit2 = RCU(C), RCU(C)
        self.out_conv = nn.Conv2d(C, C, 1)

    def forward(self, *xs, size=None):
        y = xs[0]
        if len(xs) == 2:
            y = y + self.resConfUnit1(xs[1])
        y = self.resConfUnit2(y)
        y = F.interpolate(y, **({"scale_factor": 2} if size is None else {"size": size}), mode="bilinear", align_corners=True)
        return self.out_conv(y)


class Interpolate(nn.Module):
    def forward(self, x):
        return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)


class Scratch(nn.Module):
    def __init__(self, s):
        super().__init__()
        C = s["features"]
        for i, w in enumerate(s["widths"]):
            setattr(self, f"layer{i + 1}_rn", nn.Conv2d(w, C, 3, 1, 1, bias=False))
        for i in range(1, 5):
            setattr(self, f"refinenet{i}", Fusion(C))
        self.output_conv = nn.Sequential(nn.Conv2d(C, C // 2, 3, 1, 1), Interpolate(), nn.Conv2d(C // 2, 32, 3, 1, 1), nn.ReLU(True),
                                         nn.Conv2d(32, 1, 1), nn.ReLU(True), nn.Identity())


class MidasBeitRef(nn.Module):
    """DPTDepthModel(backbone='beitl16_384', readout='project') -- forward(x normalised [B,3,H,W]) -> rel_depth [B,H,W]"""

    def __init__(self, s=None):
        super().__init__()
        self.s = s = s or settings()
        self.pretrained = Pretrained(s)
        self.scratch = Scratch(s)

    def encoder(self, x):
        m = self.pretrained.model
        B, _, H, W = x.shape
        th, tw = H // 16, W // 16
        t = m.patch_embed.proj(x).flatten(2).transpose(1, 2)
        t = torch.cat((m.cls_token.expand(B, -1, -1), t), 1)
        outs = {}
        for i, blk in enumerate(m.blocks):
            t = blk(t, th, tw)
            outs[i] = t
        hooks = [outs[i] for i in self.s["hooks"]]
        layers = []
        for i, h in enumerate(hooks):
            pp = getattr(self.pretrained, f"act_postprocess{i + 1}")
            y = pp[0](h).transpose(1, 2).unflatten(2, (th, tw))
            layers.append(pp[3:](y))
        return layers

    def forward(self, x, taps=None):
        sc = self.scratch
        l1, l2, l3, l4 = self.encoder(x)
        l1, l2, l3, l4 = sc.layer1_rn(l1), sc.layer2_rn(l2), sc.layer3_rn(l3), sc.layer4_rn(l4)
        r4 = sc.refinenet4(l4, size=l3.shape[2:])
        r3 = sc.refinenet3(r4, l3, size=l2.shape[2:])
        r2 = sc.refinenet2(r3, l2, size=l1.shape[2:])
        r1 = sc.refinenet1(r2, l1)
        oc = sc.output_conv
        out_conv = oc[3](oc[2](oc[1](oc[0](r1))))
        rel = oc[6](oc[5](oc[4](out_conv))).squeeze(1)
        if taps is not None:
            taps.update(l4_rn=l4, r4=r4, r3=r3, r2=r2, r1=r1, out_conv=out_conv)
        return rel

    def prep(self, img):
        """PrepForMidas(keep_aspect_ratio=False, img_size): bilinear align_corners=True resize (identity at img_size), then
        Normalize(0.5, 0.5)"""
        H, W = self.s["img_size"]
        if tuple(img.shape[-2:]) != (H, W):
            img = F.interpolate(img, (H, W), mode="bilinear", align_corners=True)
        return (img - 0.5) / 0.5

    def provider(self, img):
        """engine.ExternalCoreBranchNet's contract: (rel_depth [B,H,W], [l4_rn, r4, r3, r2, r1, out_conv])"""
        dt = next(self.parameters()).dtype
        taps = {}
        with torch.no_grad():
            rel = self(self.prep(img.to(dt)), taps)
        return rel, [taps[k] for k in ("l4_rn", "r4", "r3", "r2", "r1", "out_conv")]



def seeded(s=None, seed=0, dtype=torch.float64, table_std=1.0):
    """a MidasBeitRef with seeded weights of realistic scale: fan-in-scaled convs / linears, LayerScale ~0.1-1, wide relative-position
    tables (std ``table_std``, so the bias matters)"""
    m = MidasBeitRef(s)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("relative_position_bias_table"):
                p.copy_(torch.randn(p.shape, generator=g) * table_std)
            elif "gamma_" in name:
                p.copy_(0.1 + 0.9 * torch.rand(p.shape, generator=g))
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
            elif p.dim() >= 2 and name != "pretrained.model.cls_token":
                fan_in = p[0].numel() if not name.startswith("pretrained.act_postprocess1.4") and not name.startswith(
                    "pretrained.act_postprocess2.4") else p.shape[0]
                p.copy_(torch.randn(p.shape, generator=g) * (1.5 / fan_in) ** 0.5)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
    return m.to(dtype).eval()
