"""The bf16 mode of the native MiDaS BEiT-L core, host side (no GPU):
  * a lane-level model of csrc/vit.hip vit_attention32_kernel<true>'s table-slice arithmetic ("which LDS entry does (query, key) read"), checked for
    EVERY (query, key) pair against tests/midas_beit_ref.gen_relative_position_index, and the slice size against the LDS bytes the library reserves;
  * the bf16 packing of a BEiT block (round-to-nearest-even of gamma * W from float64, the [q, 0, v] bias) next to the untouched float32 pack;
  * the surface: PatchFusion / BaselinePretrain with compute_dtype="bf16" and native cores construct, load and run on the fake op set."""
import numpy as np
import pytest
import torch

from patchfusion_amd import packing as pk
from patchfusion_amd.config import make_zoe_config
from patchfusion_amd.midas_core import MidasBeitCore
from patchfusion_amd.model import PatchFusion
from patchfusion_amd.spec import patchfusion_spec, synthetic_state_dict
from tests import midas_beit_ref as mb
from tests.fake_beit_ops import ops as fake_ops

PS, RAW, SPLIT = (96, 128), (384, 512), (2, 2)
SMALL = mb.reduced(depth=2, hooks=(0, 0, 1, 1), img_size=PS)
QB = 128                                                  # queries per block


def _slice(qb0, S, th, tw):
    """(y_lo, entries of the patch part) of the block whose first query is qb0 -- the kernel's prologue"""
    y_lo = (max(qb0, 1) - 1) // tw
    y_hi = (max(min(qb0 + QB, S) - 1, 1) - 1) // tw
    return y_lo, (y_hi - y_lo + th) * (2 * tw - 1)


def _lds_entry(qb0, q, keys, S, th, tw):
    """the kernel's arithmetic for query q of block qb0 and an array of keys (padded keys included): LDS entry each (query, key) logit gathers"""
    wq = 2 * tw - 1
    y_lo, nsub = _slice(qb0, S, th, tw)
    qi = min(q, S - 1)
    pi = max(qi - 1, 0)
    yi, xi = pi // tw, pi % tw
    qoff = (yi - y_lo + th - 1) * wq + xi + tw - 1
    kt, off = keys // 64, keys % 64
    f, jq, fh, i = off // 32, (off % 32) // 8, (off % 8) // 4, off % 4
    p0 = kt * 64 + 4 * fh - 1 + 32 * f + 8 * jq
    y0 = np.trunc((p0.astype(np.float32) + np.float32(0.5)) * (np.float32(1.0) / np.float32(tw))).astype(np.int64)
    wrap_at = tw - (p0 - y0 * tw)
    li = qoff - y0 * (tw - 1) - p0 - i - np.where(i >= wrap_at, tw - 1, 0)
    li = np.maximum(li, 0)
    cls_wave = (q // 32) * 32 == 0                        # the wave's first query is 0
    is_clsq = cls_wave and q % 32 == 0
    if is_clsq:
        li = np.full_like(li, nsub)                       # cls row
    li = np.where(keys == 0, nsub + (2 if is_clsq else 1), li)      # register 0 of fragment 0 of tile 0, lanes fh == 0
    return li, y_lo, nsub


@pytest.mark.parametrize("th,tw", [(24, 32), (12, 16), (10, 14)])
def test_table_slice_index_model_every_pair(th, tw):
    S = th * tw + 1
    wq, ntab = 2 * tw - 1, (2 * th - 1) * (2 * tw - 1) + 3
    want = mb.gen_relative_position_index(th, tw).numpy()
    Sp = (S + 63) // 64 * 64
    keys = np.arange(Sp)
    assert S % QB != 0                                    # every grid here ends in a partial query block
    worst = 0
    for qb0 in range(0, S, QB):
        for q in range(qb0, qb0 + QB):                    # lanes past the sequence included (clamped query)
            li, y_lo, nsub = _lds_entry(qb0, q, keys, S, th, tw)
            assert li.min() >= 0 and li.max() < nsub + 3, (qb0, q)          # padded keys too: the gather stays inside the slice
            worst = max(worst, nsub + 3)
            glob = np.where(li < nsub, y_lo * wq + li, ntab - 3 + (li - nsub))
            assert np.array_equal(glob[:S], want[min(q, S - 1)]), (qb0, q)
    # the slice the kernel stages starts inside the table and ends inside its patch part
    for qb0 in range(0, S, QB):
        y_lo, nsub = _slice(qb0, S, th, tw)
        assert y_lo * wq + nsub <= ntab - 3
    try:
        from patchfusion_amd import _lib
        L = _lib.load()
    except (ImportError, OSError) as e:
        pytest.skip(f"libpf_hip.so not built: {e}")
    assert L.pf_vit_attention_rpb_bf16_lds_bytes(S, th, tw) == 32768 + (worst * 4 + 15) // 16 * 16
    assert L.pf_vit_attention_rpb_bf16_lds_bytes(S + 1, th, tw) == -1 and L.pf_vit_attention_rpb_bf16_lds_bytes(3 * 3 + 1, 3, 3) == -1
    if (th, tw) == (24, 32):
        assert worst * 4 == 7068                          # 28 rows x 63 + 3 entries: 39.0 KiB per block with the stages, two blocks per CU by registers
    assert L.pf_vit_attention_rpb_bf16(None, None, None, None, 1, S, Sp, 16, None, th, tw, None) == 1      # PF_ERR_ARG


def _block_sd(seed=3, D=64):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    b = "blk."
    return b, {b + "norm1.weight": r(D), b + "norm1.bias": r(D), b + "attn.qkv.weight": r(3 * D, D), b + "attn.q_bias": r(D), b + "attn.v_bias": r(D),
               b + "attn.relative_position_bias_table": r(47 * 47 + 3, 1), b + "attn.proj.weight": r(D, D), b + "attn.proj.bias": r(D),
               b + "gamma_1": 1e-3 + r(D).abs(), b + "norm2.weight": r(D), b + "norm2.bias": r(D), b + "mlp.fc1.weight": r(4 * D, D),
               b + "mlp.fc1.bias": r(4 * D), b + "mlp.fc2.weight": r(D, 4 * D), b + "mlp.fc2.bias": r(D), b + "gamma_2": 1e-3 + r(D).abs()}


def test_bf16_block_packing_rounds_once_from_float64():
    b, sd = _block_sd()
    D = 64
    qb = torch.cat([sd[b + "attn.q_bias"], torch.zeros(D), sd[b + "attn.v_bias"]])
    blk = pk.pack_beit_block_bf16(sd, b, qb, 24, 6, 8)
    for pc, w, bias, gamma in ((blk.qkv, "attn.qkv.weight", qb, None), (blk.proj, "attn.proj.weight", sd[b + "attn.proj.bias"], sd[b + "gamma_1"]),
                               (blk.fc1, "mlp.fc1.weight", sd[b + "mlp.fc1.bias"], None), (blk.fc2, "mlp.fc2.weight", sd[b + "mlp.fc2.bias"], sd[b + "gamma_2"])):
        W = sd[b + w].double()
        bb = bias.double()
        if gamma is not None:
            W, bb = gamma.double()[:, None] * W, gamma.double() * bb
        n, k = W.shape
        assert pc.w.dtype == torch.bfloat16 and pc.scale is None and pc.cin == k and pc.cout == n
        assert torch.equal(pc.w[:n, :k], W.to(torch.bfloat16)), w           # round to nearest even of the float64 product
        assert float(pc.w[n:].float().abs().sum()) == 0 and float(pc.w[:, k:].float().abs().sum()) == 0
        assert torch.equal(pc.bias[:n], bb.float()), w
    assert torch.equal(blk.qkv.bias[D:2 * D], torch.zeros(D))               # k has no bias
    assert blk.tab.dtype == torch.float32 and torch.equal(blk.tab, pk.beit_rel_pos_table(sd[b + "attn.relative_position_bias_table"], 24, 6, 8))


def test_float32_pack_of_the_core_is_unchanged():
    """the float32 route packs what the parent packed: pack_conv_split3 planes of the raw weights with gamma as the epilogue scale, the same
    table, dict blocks -- and packing for bf16 afterwards replaces (not mixes into) it"""
    ref = mb.MidasBeitRef(SMALL)
    sd = ref.state_dict()
    core = MidasBeitCore(SMALL).load_state_dict({"core." + k: v for k, v in sd.items()})
    P = core._pack(torch.device("cpu"), fake_ops)
    assert P["dtype"] == torch.float32 and P["pe"].w.dtype == torch.float32
    for i, blk in enumerate(P["blocks"]):
        b = f"pretrained.model.blocks.{i}."
        assert isinstance(blk, dict)
        want = pk.pack_conv_split3(sd[b + "attn.proj.weight"], sd[b + "attn.proj.bias"], scale=sd[b + "gamma_1"])
        assert torch.equal(blk["proj"].w, want.w) and torch.equal(blk["proj"].scale, want.scale) and torch.equal(blk["proj"].bias, want.bias)
        want = pk.pack_conv_split3(sd[b + "mlp.fc2.weight"], sd[b + "mlp.fc2.bias"], scale=sd[b + "gamma_2"])
        assert torch.equal(blk["fc2"].w, want.w) and torch.equal(blk["fc2"].scale, want.scale)
        qb = torch.cat([sd[b + "attn.q_bias"], torch.zeros_like(sd[b + "attn.v_bias"]), sd[b + "attn.v_bias"]])
        want = pk.pack_conv_split3(sd[b + "attn.qkv.weight"], qb)
        assert torch.equal(blk["qkv"].w, want.w) and torch.equal(blk["qkv"].bias, want.bias) and blk["qkv"].scale is None
    assert P["refine"][1]["out"].w.dtype == torch.float32
    P2 = core._pack(torch.device("cpu"), fake_ops, torch.bfloat16)
    assert P2["dtype"] == torch.bfloat16 and P2["pe"].w.dtype == torch.bfloat16 and P2["refine"][1]["out"].w.dtype == torch.bfloat16
    assert isinstance(P2["blocks"][0], pk.BeitBlockBF16) and core._packed is P2


def test_bf16_pack_does_not_consult_linear_split3(monkeypatch):
    core = MidasBeitCore(SMALL).load_state_dict(mb.MidasBeitRef(SMALL).state_dict())
    monkeypatch.setenv("PF_LINEAR_SPLIT3", "0")
    with pytest.raises(NotImplementedError, match="split-precision"):
        core._pack(torch.device("cpu"), fake_ops)
    assert core._pack(torch.device("cpu"), fake_ops, torch.bfloat16)["dtype"] == torch.bfloat16


def _small_model(dtype):
    cfg = make_zoe_config(PS, RAW, SPLIT)
    ref = mb.seeded(SMALL, seed=5, dtype=torch.float32)
    cores = tuple(MidasBeitCore(SMALL).load_state_dict({"core." + k: v for k, v in ref.state_dict().items()}) for _ in range(2))
    m = PatchFusion(cfg, compute_dtype=dtype, ops=fake_ops, core_providers=cores).eval()
    m.load_state_dict(synthetic_state_dict(patchfusion_spec(cfg), 0), strict=True)
    return m, cores


def test_surface_constructs_loads_and_runs_in_bf16():
    cfg = make_zoe_config(PS, RAW, SPLIT)
    m = PatchFusion(cfg, compute_dtype="bf16", ops=fake_ops, core_providers="native")
    assert all(isinstance(p, MidasBeitCore) and p.s["depth"] == 24 for p in m.core_providers)
    m.load_state_dict(synthetic_state_dict(patchfusion_spec(cfg), 0), strict=True)
    from patchfusion_amd.baseline import BaselinePretrain
    from patchfusion_amd.config import zoe_midas_branch_config
    bc = zoe_midas_branch_config(PS)
    b = BaselinePretrain(bc, bc, None, 1e-3, 80, RAW, PS, SPLIT, target="fine", ops=fake_ops, core_provider="native", compute_dtype="bf16")
    assert isinstance(b.core_provider, MidasBeitCore) and b.compute_dtype == torch.bfloat16

    m, cores = _small_model("bf16")
    img = torch.rand(1, 3, *RAW, generator=torch.Generator().manual_seed(3))
    lr = m.resizer(img)
    with torch.no_grad():
        d, _ = m(mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=2)
    assert tuple(d.shape[-2:]) == (PS[0] * SPLIT[0], PS[1] * SPLIT[1]) and torch.isfinite(d).all()
    assert all(c._packed["dtype"] == torch.bfloat16 and isinstance(c._packed["blocks"][0], pk.BeitBlockBF16) for c in cores)
    # set_compute_dtype: the engine is forgotten and the cores' packs follow
    m.set_compute_dtype("fp32")
    assert all(c._packed is None for c in cores)
    with torch.no_grad():
        d32, _ = m(mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=2)
    assert all(c._packed["dtype"] == torch.float32 and isinstance(c._packed["blocks"][0], dict) for c in cores)
    assert torch.isfinite(d32).all()
    # the two modes compute the same map to bf16 accuracy (loose: wiring, not precision -- that is the GPU suite's job)
    assert float((d.float() - d32).abs().max()) < 0.1 * float(d32.abs().max())


def test_provider_without_dtype_argument_is_refused_clearly():
    class OldCore:
        def forward_nhwc(self, ops, img, out_conv=None, rel=None):
            raise AssertionError("must not be called in bf16")

    cfg = make_zoe_config(PS, RAW, SPLIT)
    m = PatchFusion(cfg, compute_dtype="bf16", ops=fake_ops, core_providers=(OldCore(), OldCore())).eval()
    m.load_state_dict(synthetic_state_dict(patchfusion_spec(cfg), 0), strict=True)
    img = torch.rand(1, 3, *RAW)
    with pytest.raises(NotImplementedError, match="float32 only"):
        m(mode="infer", image_lr=m.resizer(img), image_hr=img, cai_mode="m1", process_num=2)


def test_nchw_provider_protocol_returns_float32_in_both_modes():
    ref = mb.seeded(SMALL, seed=5, dtype=torch.float32)
    core = MidasBeitCore(SMALL, ops=fake_ops).load_state_dict(ref.state_dict())
    img = torch.rand(1, 3, *PS, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want, wf = ref.provider(img)
        r32, f32 = core(img)
        core.call_dtype = torch.bfloat16
        r16, f16 = core(img)
    assert r32.dtype == r16.dtype == torch.float32 and all(f.dtype == torch.float32 for f in f32 + f16)
    assert float((r32 - want).abs().max()) <= 1e-3 * float(want.abs().max())
    for a, w in zip([r16] + f16, [want] + wf):
        assert float((a - w).norm() / w.norm()) < 0.05
