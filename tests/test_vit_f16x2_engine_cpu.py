"""Wiring of the fp16x2 ViT route on CPU: the engine driven by an op set that extends tests/fake_ops.py with layernorm_f16x2 / conv_f16x2 (float32
math on the real fp16x2 planes and exponents of packing.pack_conv_f16x2) takes the route on the crop branch (PF_VIT_F16X2=1) or on both
(PF_VIT_F16X2=2), and matches the oracle with the bars of tests/test_engine_cpu.py.  Without those ops (plain fake_ops) the engine keeps bf16x3."""
import pytest
import torch
import torch.nn.functional as F

from oracle import pf_oracle
from patchfusion_amd import packing as pk
from patchfusion_amd.config import make_config
from patchfusion_amd.model import PatchFusion
from patchfusion_amd.spec import patchfusion_spec, synthetic_state_dict
from tests.fake_ops import FakeOps, _act, ops as fake_ops

TINY = ("vits", (112, 154), (448, 616), (2, 2))


class F16x2Ops(FakeOps):
    calls = {"layernorm_f16x2": 0, "conv_f16x2": 0}

    @staticmethod
    def _store2(y2, v, e):
        h, l = pk.split_f16x2(torch.ldexp(v.double(), -e.double()[None, :]).float())
        y2[:] = pk.rows_to_kmajor(torch.stack([h, l]))

    @staticmethod
    def layernorm_f16x2(x, y2, g, b, eps, in_exp):
        F16x2Ops.calls["layernorm_f16x2"] += 1
        F16x2Ops._store2(y2, F.layer_norm(x.float(), (x.shape[-1],), g, b, eps), in_exp)
        return y2

    @staticmethod
    def conv_f16x2(x2, pw, y, act=None, res=None, res2=None, out_exp=None):
        F16x2Ops.calls["conv_f16x2"] += 1
        x = pk.kmajor_to_rows(x2).float().sum(0)                     # x / 2^e_k (h + l is exact in float32)
        w = pk.kmajor_to_rows(pw.w).float().sum(0)[:pw.cout]        # W 2^(e_k - f_n)
        v = torch.ldexp(x @ w.t(), pw.col_exp[:pw.cout].float()[None, :])
        if pw.bias is not None:
            v = v + pw.bias[:pw.cout]
        v = _act(v, act)
        if pw.scale is not None:
            v = v * pw.scale[:pw.cout]
        if res is not None:
            v = v + res[:, :pw.cout].float()
        if res2 is not None:
            v = v + res2[:, :pw.cout].float()
        if y.dtype == torch.float16:
            F16x2Ops._store2(y, v, out_exp[:pw.cout])
        elif y.dtype == torch.bfloat16:
            FakeOps._store3(y[:, :, :pw.cout], v)
        else:
            y[:, :pw.cout] = v
        return y


@pytest.fixture(scope="module")
def tiny():
    cfg = make_config(*TINY)
    sd = synthetic_state_dict(patchfusion_spec(cfg), 0)
    img = torch.rand(1, 3, *TINY[2], generator=torch.Generator().manual_seed(1234))
    return cfg, sd, img


def _model(cfg, sd, ops, monkeypatch, route):
    monkeypatch.setenv("PF_VIT_F16X2", route)
    m = PatchFusion(cfg, compute_dtype="fp32", ops=ops).eval()
    m.load_state_dict(sd, strict=True)
    m._ensure_engine()
    return m


def test_route_needs_the_ops_and_follows_the_switch(tiny, monkeypatch):
    cfg, sd, _ = tiny
    m = _model(cfg, sd, fake_ops, monkeypatch, "2")
    assert not m._engine["coarse"].f16x2 and not m._engine["fine"].f16x2       # op set without fp16x2 ops: bf16x3 wiring
    assert m._engine["fine"].blocks[0]["fc1"].w.dtype == torch.bfloat16
    ext = F16x2Ops()
    for route, want in (("0", (False, False)), ("1", (False, True)), ("2", (True, True))):
        m = _model(cfg, sd, ext, monkeypatch, route)
        assert (m._engine["coarse"].f16x2, m._engine["fine"].f16x2) == want, route
        for br, on in zip(("coarse", "fine"), want):
            blk = m._engine[br].blocks[0]
            assert blk["proj"].w.dtype == torch.bfloat16                          # the projection stays on bf16x3
            for k in ("qkv", "fc1", "fc2"):                                       # only the planes of the route in use are packed
                assert blk[k].w.dtype == (torch.float16 if on else torch.bfloat16)
                assert (blk[k].col_exp is not None) == on


def test_branch_matches_oracle_on_the_fp16x2_route(tiny, monkeypatch):
    cfg, sd, img = tiny
    m = _model(cfg, sd, F16x2Ops(), monkeypatch, "2")
    F16x2Ops.calls.update(layernorm_f16x2=0, conv_f16x2=0)
    lr = m.resizer(img)
    ot, et = {}, {}
    od, of = pf_oracle.branch_forward(sd, "coarse_branch.", lr, cfg["coarse_branch"], ot)
    st = m._coarse(lr, et)
    depth = len(m._engine["coarse"].blocks)
    assert F16x2Ops.calls == {"layernorm_f16x2": 2 * depth, "conv_f16x2": 3 * depth}
    for k in ("vit_tokens_in", "vit_block0", "vit_block11"):
        assert (ot[k] - et[k]).abs().max() < 2e-4, k
    for i in range(4):
        a = ot[f"vit_out{i}"]
        assert (a - et[f"vit_out{i}"].reshape(a.shape)).abs().max() < 2e-4
    for i, (a, b) in enumerate(zip(of, st["feats"])):
        b = b.permute(0, 3, 1, 2) if b.dim() == 4 else b
        assert (a - b).abs().max() < 5e-4, i
    assert (od - st["depth"]).abs().max() < 1e-4
