"""Float64 reference, per-element magnitudes, float32 restatement and seeded inputs of the ViT attention kernels (csrc/vit.hip, csrc/attn_split3.hip):
softmax(q k^T / 8 [+ bias]) v per head, head_dim 64, qkv rows [B*S, 3, heads, 64].  Style and metric of tests/f64_image_ref.py; used by
tests/test_attention_grade_gpu.py, checked on the CPU by tests/test_f64_attn_ref_cpu.py.  No GPU needed: every function computes on the device of
its operand and returns CPU tensors.

mag = sum_j p_ij |v_jd| (the convention of f64_image_ref.swin_window_attention_ref): an attention output is an average of V, 0.03 .. 0.3 at unit
variance, so max |y - ref| / max(1, max |ref|) (tests/op_checks.py) is an absolute bar on values ten to thirty times smaller than its denominator;
max |y - ref| / mag is relative to what the element was summed from.

Inputs (all seeded, float32 [B*S, 3*heads*64]):
  random    N(0, scale^2); hot = key S - 29 of every head times 8 (one key far above the rest late in the sequence: the deferred-rescale path)
  wide      random, then q channel c x s_c, k channel c / s_c (logits unchanged), v channel c x t_c; s over 1e-2 .. 1e2, t over 1e-3 .. 1e3
            (f64_ref.decade_spread): output columns span six decades, which a normwise metric reduces to the largest one
  one_hot   k, v ~ N(0, 1) (k rows at norm 8), q_i = 12 k_pi(i), pi a seeded permutation per (image, head): the winning logit leads by more than 26, the output is
            v[pi(i)] to 1e-11 -- a mis-indexed or unmasked key, a lost share of the keys or a dropped operand plane shows at full size
  uniform   q = 0: p = 1 / S, the output is the mean of V (errors only from the P planes, the PV accumulation and the normalisation)"""
import math
import zlib

import torch

from tests.f64_image_ref import FLOOR, baseline_bar, errors            # noqa: F401  (the bar and the metric, unchanged)
from tests.f64_ref import decade_spread

LOG2E = math.log2(math.e)


def _heads(x, B, S, heads):
    """[B*S, 3*heads*64] -> q, k, v [B, heads, S, 64]"""
    return x.view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)


def _rows(t, B, S, heads):
    return t.transpose(1, 2).reshape(B * S, heads * 64).cpu()


def attention_ref(qkv, B, S, heads, bias=None):
    """qkv [B*S, 3*heads*64] (any float dtype: its exact values), bias float64 [heads, S, S] or None -> (ref, mag) float64 [B*S, heads*64]"""
    q, k, v = _heads(qkv.detach().double(), B, S, heads)
    a = (q * 0.125) @ k.transpose(-2, -1)
    if bias is not None:
        a = a + bias.to(a.device).double()[None]
    p = a.softmax(-1)
    return _rows(p @ v, B, S, heads), _rows(p @ v.abs(), B, S, heads)


def restatement_f32(qkv, B, S, heads, bias=None):
    """the same attention in torch float32 on the same operands (qkv must hold float32 values; bias rounded to float32) -> float32 [B*S, heads*64]"""
    q, k, v = _heads(qkv.detach().float(), B, S, heads)
    a = (q * 0.125) @ k.transpose(-2, -1)
    if bias is not None:
        a = a + bias.to(a.device).float()[None]
    return _rows(a.softmax(-1) @ v, B, S, heads)


def rpb_index(th, tw):
    """generate_relative_position_index (BEiT) restated: [S, S], S = th tw + 1, cls first.  patch i = (yi, xi) against patch j:
    (yi - yj + th - 1)(2 tw - 1) + xi - xj + tw - 1; cls row n - 3, cls column n - 2, cls x cls n - 1, n = (2 th - 1)(2 tw - 1) + 3"""
    n = (2 * th - 1) * (2 * tw - 1) + 3
    t = torch.arange(th * tw)
    y, x = t // tw, t % tw
    idx = torch.empty(th * tw + 1, th * tw + 1, dtype=torch.long)
    idx[1:, 1:] = (y[:, None] - y[None, :] + th - 1) * (2 * tw - 1) + x[:, None] - x[None, :] + tw - 1
    idx[0, :] = n - 3
    idx[:, 0] = n - 2
    idx[0, 0] = n - 1
    return idx


def rpb_bias(tab2, th, tw):
    """packed table [heads, (2 th - 1)(2 tw - 1) + 3] (float32, times log2(e): packing.beit_rel_pos_table) -> float64 bias [heads, S, S] (CPU)"""
    t = tab2.detach().cpu().double() / LOG2E
    S = th * tw + 1
    assert t.shape[1] == (2 * th - 1) * (2 * tw - 1) + 3
    return t[:, rpb_index(th, tw).view(-1)].view(-1, S, S)


# ---------------- inputs ----------------
def seed_of(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def random(B, S, heads, scale, seed, hot=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * S, 3 * heads * 64, generator=g, dtype=torch.float64) * scale
    if hot:
        x.view(B, S, 3, heads, 64)[:, S - 29, 1] *= 8.0
    return x.float()


def wide(B, S, heads, seed):
    D = heads * 64
    x = random(B, S, heads, 1.0, seed).double().view(B * S, 3, D)
    s, t = decade_spread(D, 1e-2, 1e2, seed + 1), decade_spread(D, 1e-3, 1e3, seed + 2)
    x[:, 0] *= s
    x[:, 1] /= s
    x[:, 2] *= t
    return x.view(B * S, 3 * D).float()


def one_hot(B, S, heads, seed):
    """-> qkv, pi (LongTensor [B, heads, S]: the key query i selects).  Every key row is an N(0, 1) draw brought to the norm 8 = sqrt(64) such a
    row has on average: the winning logit is 12 * 64 / 8 = 96 for every query, the runner-up 96 cos(k_i, k_j).  With the lengths as drawn, a
    short key (|k|^2 = 30 occurs among a few thousand) wins by 1.5 |k|^2 = 45 at most and the lead falls below 26 at the larger shapes for
    every seed; the directions, and so every index the kernel has to get right, are the draw's."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, 3, heads, 64, generator=g, dtype=torch.float64)
    x[:, :, 1] *= 8.0 / x[:, :, 1].norm(dim=-1, keepdim=True)
    x = x.float()
    pi =torch.stack([torch.randperm(S, generator=g) for _ in range(B * heads)]).view(B, heads, S)
    k = x[:, :, 1].permute(0, 2, 1, 3)                                         # [B, heads, S, 64]
    x[:, :, 0] = (12.0 * torch.gather(k, 2, pi[..., None].expand(-1, -1, -1, 64))).permute(0, 2, 1, 3)
    return x.view(B * S, 3 * heads * 64), pi


def uniform(B, S, heads, seed):
    x = random(B, S, heads, 1.0, seed).view(B * S, 3, heads * 64)
    x[:, 0] = 0
    return x.view(B * S, -1)


def one_hot_margin(qkv, B, S, heads):
    """smallest lead of the winning logit over the runner-up (float64)"""
    q, k, _ = _heads(qkv.double(), B, S, heads)
    top = ((q * 0.125) @ k.transpose(-2, -1)).topk(min(2, S), dim=-1).values
    return float((top[..., 0] - top[..., 1]).min())


KINDS = ("random1", "random4hot", "wide", "one_hot", "uniform")


def build(kind, B, S, heads):
    """the seeded float32 qkv of a case (kind: one of KINDS, or 'random1.5')"""
    seed = seed_of(kind, B, S, heads)
    if kind == "random1":
        return random(B, S, heads, 1.0, seed)
    if kind == "random1.5":
        return random(B, S, heads, 1.5, seed)
    if kind == "random4hot":
        return random(B, S, heads, 4.0, seed, hot=True)
    if kind == "wide":
        return wide(B, S, heads, seed)
    if kind == "one_hot":
        return one_hot(B, S, heads, seed)[0]
    if kind == "uniform":
        return uniform(B, S, heads, seed)
    raise ValueError(kind)


# ---------------- cases shared by the CPU and the GPU test ----------------
# B, S, heads: S below one key block; one key past a 32-key block; an exact multiple of 64; one query past a 128-query block (NB = 5, no key split);
# key split with a 1-query tail, NB = 9, B heads % 8 != 0 (block-order fallback); key split with a tail of exactly 32, tail-first block order;
# a 44-query tail (no key split); the workload's S with B heads = 8
SHAPES = [(1, 13, 2), (1, 33, 1), (3, 64, 4), (1, 129, 1), (1, 257, 3), (1, 288, 8), (2, 300, 6), (2, 1037, 4)]
ALL_KINDS_AT = {(1, 33, 1), (1, 257, 3), (1, 288, 8)}


def kinds_of(shape, f16=False):
    """every kind at the two key-split shapes and at (1, 33, 1), random1 and one_hot elsewhere; the fp16x2 kernel: random1, one_hot, uniform"""
    kinds = KINDS if shape in ALL_KINDS_AT else ("random1", "one_hot")
    return tuple(k for k in kinds if not f16 or k in ("random1", "one_hot", "uniform"))


CASES = [(s, k) for s in SHAPES for k in kinds_of(s)]
F16_CASES = [(s, k) for s in SHAPES for k in kinds_of(s, f16=True)]
# the relative-position kernel: grids (th, tw), S = th tw + 1; a query block straddles many grid rows (40 x 5), less than one (5 x 40)
RPB_GRIDS = [(2, 3), (10, 14), (5, 40), (40, 5), (16, 17)]
RPB_CASES = [(B, g, k) for g in RPB_GRIDS for B in (1, 3) for k in ("random1.5", "one_hot")]
RPB_HEADS = 2


def rpb_table(th, tw, heads=RPB_HEADS):
    """a std-1 pretrain table [(2 * 24 - 1)^2 + 3, heads] through packing.beit_rel_pos_table -> float32 [heads, (2 th - 1)(2 tw - 1) + 3]"""
    from patchfusion_amd import packing as pk
    g = torch.Generator().manual_seed(seed_of("tab", th, tw))
    return pk.beit_rel_pos_table(torch.randn(47 * 47 + 3, heads, generator=g), 24, th, tw)
