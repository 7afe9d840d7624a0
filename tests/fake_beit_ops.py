"""TEST INFRASTRUCTURE ONLY.  tests/fake_ops.py's plain-PyTorch op set plus the ops only the MiDaS BEiT core uses (patch_im2col_norm,
readout_concat, the relative-position attention in its split-plane and bf16 forms), with hip_ops' signatures and buffer conventions, so that
midas_core.MidasBeitCore can be driven on the CPU."""
import math

import torch

from tests import midas_beit_ref as mb
from tests.fake_ops import FakeOps


def _rpb_attention(qkv, B, S, heads, tab, th, tw, round_q=None):
    D = qkv.shape[1] // 3
    q, k, v = qkv.float().view(B, S, 3, heads, D // heads).permute(2, 0, 3, 1, 4)
    q = q * (D // heads) ** -0.5
    if round_q is not None:
        q = q.to(round_q).float()
    idx = mb.gen_relative_position_index(th, tw).view(-1).to(qkv.device)
    bias = (tab.float() / math.log2(math.e)).t()[idx].view(S, S, heads).permute(2, 0, 1)
    a = (q @ k.transpose(-2, -1) + bias).softmax(dim=-1)
    return (a @ v).transpose(1, 2).reshape(B * S, D)


class FakeBeitOps(FakeOps):
    name = "fake-beit"

    @staticmethod
    def patch_im2col_norm(img, out, patch, mean, std):
        B, _, H, W = img.shape
        m = torch.tensor(mean, device=img.device).view(1, 3, 1, 1)
        s = torch.tensor(std, device=img.device).view(1, 3, 1, 1)
        th, tw = H // patch, W // patch
        x = ((img - m) / s).view(B, 3, th, patch, tw, patch).permute(0, 2, 4, 3, 5, 1).reshape(B * th * tw, 3 * patch * patch)
        out[:, :x.shape[1]] = x.to(out.dtype)
        out[:, x.shape[1]:] = 0

    @staticmethod
    def assemble_tokens(emb, tokens, cls, pos):
        FakeOps.assemble_tokens(emb, tokens, cls, pos.view(tokens.shape[1], tokens.shape[2]))      # (the core hands the kernel a flat table)

    @staticmethod
    def readout_concat(x, y, B, S):
        D = x.shape[1]
        xv = x.view(B, S, D)
        y[:] = torch.cat((xv[:, 1:], xv[:, :1].expand(-1, S - 1, -1)), -1).reshape(B * (S - 1), 2 * D)

    @staticmethod
    def vit_attention_rpb(qkv, out, B, S, heads, tab, th, tw):
        FakeOps._store3(out, _rpb_attention(FakeOps._rows(qkv), B, S, heads, tab, th, tw))

    @staticmethod
    def vit_attention_rpb_bf16(qkv, out, B, S, heads, tab, th, tw):
        assert qkv.dtype == out.dtype == torch.bfloat16 and tab.dtype == torch.float32
        out[:] = _rpb_attention(qkv, B, S, heads, tab, th, tw, round_q=torch.bfloat16).to(out.dtype)


ops = FakeBeitOps
