"""Pins the MiDaS DPT_BEiT_L_384 restatement (tests/midas_beit_ref.py) that the native core is held to:
  * against transformers' independent BEiT (BeitModel hidden states, BeitRelativePositionBias) at full width, 384x512, reduced depth;
  * its decoder against transformers' ZoeDepthNeck + ZoeDepthRelativeDepthEstimationHead, weights mapped from the MiDaS names;
  * against the reference's own MidasCore (midas.py:189-316: PrepForMidas, the six forward hooks) wrapped around the restatement;
  * mutant controls: a transposed table, swapped cls entries, a dropped v_bias, cls-first readout rows and exchanged refinenet units
    each fail the same bar."""
import os
import sys

import pytest
import torch

from tests import midas_beit_ref as mb

transformers = pytest.importorskip("transformers")

RES = (384, 512)
BAR = 1e-10          # float64 against float64


def _beit_config(s, pretrain):
    from transformers import BeitConfig
    return BeitConfig(hidden_size=s["D"], num_hidden_layers=s["depth"], num_attention_heads=s["heads"], intermediate_size=4 * s["D"],
                      image_size=16 * pretrain, patch_size=16, use_relative_position_bias=True, use_absolute_position_embeddings=False,
                      use_shared_relative_position_bias=False, layer_scale_init_value=0.1, layer_norm_eps=1e-6, use_mask_token=False,
                      hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, drop_path_rate=0.0)


def _to_hf(ref):
    """MiDaS / timm names -> transformers BeitModel names"""
    out = {}
    sd = ref.state_dict()
    p = "pretrained.model."
    out["embeddings.cls_token"] = sd[p + "cls_token"]
    out["embeddings.patch_embeddings.projection.weight"] = sd[p + "patch_embed.proj.weight"]
    out["embeddings.patch_embeddings.projection.bias"] = sd[p + "patch_embed.proj.bias"]
    D = ref.s["D"]
    for i in range(ref.s["depth"]):
        b, h = f"{p}blocks.{i}.", f"layers.{i}."
        w = sd[b + "attn.qkv.weight"]
        out.update({h + "attention.q_proj.weight": w[:D], h + "attention.k_proj.weight": w[D:2 * D], h + "attention.v_proj.weight": w[2 * D:],
                    h + "attention.q_proj.bias": sd[b + "attn.q_bias"], h + "attention.v_proj.bias": sd[b + "attn.v_bias"],
                    h + "attention.o_proj.weight": sd[b + "attn.proj.weight"], h + "attention.o_proj.bias": sd[b + "attn.proj.bias"],
                    h + "relative_position_bias.relative_position_bias_table": sd[b + "attn.relative_position_bias_table"],
                    h + "lambda_1": sd[b + "gamma_1"], h + "lambda_2": sd[b + "gamma_2"]})
        for a, m in (("norm1", "layernorm_before"), ("norm2", "layernorm_after"), ("mlp.fc1", "mlp.fc1"), ("mlp.fc2", "mlp.fc2")):
            out[h + m + ".weight"], out[h + m + ".bias"] = sd[b + a + ".weight"], sd[b + a + ".bias"]
    return out


@pytest.fixture(scope="module")
def small():
    s = mb.reduced(depth=3, hooks=(0, 1, 2))
    return s, mb.seeded(s, seed=3)


def _hf_hidden(ref):
    from transformers import BeitModel
    hf = BeitModel(_beit_config(ref.s, ref.s["pretrain"]), add_pooling_layer=False).double().eval()
    missing, unexpected = hf.load_state_dict(_to_hf(ref), strict=False)
    assert not unexpected and all("relative_position_index" in k or "k_bias" in k for k in missing), (missing, unexpected)
    return hf


def _restated_hidden(ref, x):
    m = ref.pretrained.model
    th, tw = x.shape[2] // 16, x.shape[3] // 16
    t = torch.cat((m.cls_token.expand(x.shape[0], -1, -1), m.patch_embed.proj(x).flatten(2).transpose(1, 2)), 1)
    hs = []
    for blk in m.blocks:
        t = blk(t, th, tw)
        hs.append(t)
    return hs


def test_blocks_match_transformers_beit(small):
    s, ref = small
    x = torch.randn(1, 3, *RES, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    hf = _hf_hidden(ref)
    with torch.no_grad():
        got = _restated_hidden(ref, x)
        want = hf(pixel_values=x, output_hidden_states=True, interpolate_pos_encoding=False).hidden_states[1:]
    assert len(got) == len(want) == s["depth"]
    for a, b in zip(got, want):
        err = float((a - b).abs().max() / b.abs().max())
        assert err < BAR, err


@pytest.mark.parametrize("pretrain", [24, 32])
def test_interpolated_bias_matches_transformers(pretrain):
    from transformers.models.beit.modeling_beit import BeitRelativePositionBias
    s = mb.settings(heads=16)
    rb = BeitRelativePositionBias(_beit_config(s, pretrain)).double()
    with torch.no_grad():
        rb.relative_position_bias_table.copy_(torch.randn(rb.relative_position_bias_table.shape, generator=torch.Generator().manual_seed(7)))
        want = rb((24, 32))
        got = mb.rel_pos_bias(rb.relative_position_bias_table, pretrain, 24, 32)
    assert got.shape == (16, 769, 769)
    assert float((got - want.reshape(got.shape)).abs().max()) == 0.0


def _mutant_bias(kind):
    real = mb.rel_pos_bias

    def f(table, pretrain, th, tw):
        if kind == "transposed":                          # table read as (width, height) the other way round
            old = 2 * pretrain - 1
            t = table[:old * old].reshape(old, old, -1).transpose(0, 1).reshape(old * old, -1)
            table = torch.cat([t, table[old * old:]])
        elif kind == "cls_swapped":                       # cls-row and cls-column entries exchanged
            table = table.clone()
            table[[-3, -2]] = table[[-2, -3]]
        return real(table, pretrain, th, tw)
    return f


@pytest.mark.parametrize("kind", ["transposed", "cls_swapped", "no_v_bias"])
def test_mutants_fail_the_bar(small, kind, monkeypatch):
    s, ref = small
    x = torch.randn(1, 3, *RES, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    hf = _hf_hidden(ref)
    if kind == "no_v_bias":
        for blk in ref.pretrained.model.blocks:
            monkeypatch.setattr(blk.attn, "v_bias", torch.nn.Parameter(torch.zeros_like(blk.attn.v_bias)))
    else:
        monkeypatch.setattr(mb, "rel_pos_bias", _mutant_bias(kind))
    with torch.no_grad():
        got = _restated_hidden(ref, x)
        want = hf(pixel_values=x, output_hidden_states=True).hidden_states[1:]
    err = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, want))
    assert err > 1e3 * BAR, (kind, err)


@pytest.mark.reference
def test_reference_midas_core_hooks_match_provider():
    """the reference's own MidasCore around the restatement: PrepForMidas (identity resize at 384x512, Normalize(0.5, 0.5)) and the
    hooks on output_conv child 3, refinenet1..4 and layer4_rn return the provider's tensors"""
    from oracle import ref_shim
    if not ref_shim.reference_available():
        pytest.skip("reference tree not present")
    ref_shim.install_stubs()
    ext = os.path.join(ref_shim.REF_ROOT, "external")
    if ext not in sys.path:
        sys.path.insert(0, ext)
    from zoedepth.models.base_models.midas import MidasCore
    ref = mb.seeded(mb.reduced(depth=2, hooks=(0, 0, 1, 1)), seed=5)
    core = MidasCore(ref, trainable=False, fetch_features=True, freeze_bn=True, keep_aspect_ratio=False, img_size=list(RES))
    img = torch.rand(2, 3, *RES, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    with torch.no_grad():
        rel, out = core(img, return_rel_depth=True)
    want_rel, want = ref.provider(img)
    assert rel.shape == (2, *RES)
    assert torch.equal(rel, want_rel)
    got = out[1:] + out[:1]               # MidasCore: (out_conv, l4_rn, r4..r1) -> provider (l4_rn, r4..r1, out_conv)
    shapes = [(2, 256, 12, 16), (2, 256, 24, 32), (2, 256, 48, 64), (2, 256, 96, 128), (2, 256, 192, 256), (2, 32, 384, 512)]
    for a, b, sh in zip(got, want, shapes):
        assert tuple(a.shape) == sh and torch.equal(a, b)
    # a non-native input size goes through the same bilinear align_corners=True resize as PrepForMidas's Resize
    img2 = torch.rand(1, 3, 300, 400, generator=torch.Generator().manual_seed(10), dtype=torch.float64)
    with torch.no_grad():
        r2, _ = core(img2, return_rel_depth=True)
    assert torch.equal(r2, ref.provider(img2)[0])


def test_state_dict_keys_are_the_checkpoint_names():
    ref = mb.MidasBeitRef(mb.reduced(depth=2, hooks=(0, 0, 1, 1)))
    keys = set(ref.state_dict())
    for k in ("pretrained.model.cls_token", "pretrained.model.patch_embed.proj.weight", "pretrained.model.blocks.1.attn.q_bias",
              "pretrained.model.blocks.1.attn.relative_position_bias_table", "pretrained.model.blocks.0.gamma_2",
              "pretrained.act_postprocess1.0.project.0.weight", "pretrained.act_postprocess1.4.weight", "pretrained.act_postprocess4.4.bias",
              "scratch.layer3_rn.weight", "scratch.refinenet2.resConfUnit1.conv2.bias", "scratch.refinenet4.out_conv.weight",
              "scratch.output_conv.4.bias"):
        assert k in keys, k
    assert "scratch.layer1_rn.bias" not in keys and "pretrained.model.blocks.0.attn.k_bias" not in keys
    assert "pretrained.act_postprocess3.4.weight" not in keys


def _zoe_neck_head(ref):
    """transformers' ZoeDepthNeck (readout 'project' reassemble, layerN_rn convs, fusion stage) + ZoeDepthRelativeDepthEstimationHead with
    the weights mapped from the MiDaS names"""
    from transformers import ZoeDepthConfig
    from transformers.models.zoedepth.modeling_zoedepth import ZoeDepthNeck, ZoeDepthRelativeDepthEstimationHead
    s = ref.s
    c = ZoeDepthConfig(readout_type="project", neck_hidden_sizes=list(s["widths"]), reassemble_factors=[4, 2, 1, 0.5],
                       fusion_hidden_size=s["features"], head_in_index=-1, add_projection=False, num_relative_features=32, hidden_act="gelu",
                       use_batch_norm_in_fusion_residual=False, use_bias_in_fusion_residual=None)
    c.backbone_hidden_size = s["D"]
    neck, head = ZoeDepthNeck(c).double().eval(), ZoeDepthRelativeDepthEstimationHead(c).double().eval()
    sd = ref.state_dict()
    n, h = {}, {}
    for i in range(4):
        p = f"pretrained.act_postprocess{i + 1}."
        for t in ("weight", "bias"):
            n[f"reassemble_stage.readout_projects.{i}.0.{t}"] = sd[p + "0.project.0." + t]
            n[f"reassemble_stage.layers.{i}.projection.{t}"] = sd[p + "3." + t]
            if i != 2:
                n[f"reassemble_stage.layers.{i}.resize.{t}"] = sd[p + "4." + t]
        n[f"convs.{i}.weight"] = sd[f"scratch.layer{i + 1}_rn.weight"]
    for j, r in enumerate((4, 3, 2, 1)):                  # the fusion stage runs deepest first: layer j = refinenet(4 - j)
        q = f"scratch.refinenet{r}."
        for t in ("weight", "bias"):
            n[f"fusion_stage.layers.{j}.projection.{t}"] = sd[q + "out_conv." + t]
            for u, m in ((1, "resConfUnit1"), (2, "resConfUnit2")):
                for k in (1, 2):
                    n[f"fusion_stage.layers.{j}.residual_layer{u}.convolution{k}.{t}"] = sd[f"{q}{m}.conv{k}.{t}"]
    for t in ("weight", "bias"):
        for k, i in ((1, 0), (2, 2), (3, 4)):
            h[f"conv{k}.{t}"] = sd[f"scratch.output_conv.{i}.{t}"]
    neck.load_state_dict(n, strict=True)
    head.load_state_dict(h, strict=True)
    return neck, head


def _neck_head_errors(ref, neck, head, x):
    with torch.no_grad():
        taps = {}
        rel = ref(x, taps)
        hs = _restated_hidden(ref, x)
        fused, l4 = neck([hs[i] for i in ref.s["hooks"]], x.shape[2] // 16, x.shape[3] // 16)
        hrel, hout = head(fused)
    pairs = [(rel, hrel), (taps["l4_rn"], l4), (taps["out_conv"], hout)] + [(taps[k], f) for k, f in zip(("r4", "r3", "r2", "r1"), fused)]
    return [float((a - b).abs().max() / b.abs().max()) for a, b in pairs]


@pytest.fixture(scope="module")
def neck_case():
    ref = mb.seeded(mb.reduced(depth=2, hooks=(0, 0, 1, 1)), seed=13)
    x = torch.randn(1, 3, *RES, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    return ref, x, _zoe_neck_head(ref)


def test_decoder_matches_transformers_zoedepth_neck_and_head(neck_case):
    """the decoder half: readout 'project' (cat order), act_postprocess 1-4, layerN_rn, the refinenets and output_conv"""
    ref, x, (neck, head) = neck_case
    errs = _neck_head_errors(ref, neck, head, x)
    assert max(errs) < BAR, errs


@pytest.mark.parametrize("kind", ["readout_cls_first", "refinenet_order"])
def test_decoder_mutants_fail_the_bar(neck_case, kind, monkeypatch):
    ref, x, (neck, head) = neck_case
    if kind == "readout_cls_first":                   # cat(cls, token) instead of cat(token, cls)
        monkeypatch.setattr(mb.ProjectReadout, "forward",
                            lambda self, t: self.project(torch.cat((t[:, :1].expand_as(t[:, 1:]), t[:, 1:]), -1)))
    else:                                              # RCU1 and RCU2 of every refinenet exchanged
        def fwd(self, *xs, size=None):
            y = xs[0]
            if len(xs) == 2:
                y = y + self.resConfUnit2(xs[1])
            y = self.resConfUnit1(y)
            y = torch.nn.functional.interpolate(y, **({"scale_factor": 2} if size is None else {"size": size}), mode="bilinear", align_corners=True)
            return self.out_conv(y)
        monkeypatch.setattr(mb.Fusion, "forward", fwd)
    assert max(_neck_head_errors(ref, neck, head, x)) > 1e3 * BAR
