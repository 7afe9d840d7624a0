"""Build-time guard for the MiDaS BEiT core kernels: the relative-position attention (both queries-per-wave forms) and csrc/beit.hip use no
scratch and at most 256 VGPRs; the unbiased two-phase v2 instantiations keep their register counts and stay free of the bias gather."""
import os
import re

from tests.test_wino_f16x2_resources import _compile, needs_hipcc


@needs_hipcc
def test_rpb_attention_resources(tmp_path):
    k = _compile(tmp_path, "attn_split3.hip", ("-save-temps=obj",))
    rpb = {n: r for n, r in k.items() if "rpb_kernel" in n}
    assert len(rpb) == 2, list(k)
    for n, (s, v, _) in rpb.items():
        assert s == 0 and v <= 256, (n, s, v)
    v2 = {n: r for n, r in k.items() if "split3_v2_kernel" in n}
    assert len(v2) == 2 and all(s == 0 for s, _, _ in v2.values()), v2
    listing = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    asm = open(tmp_path / listing[0]).read()
    for name in v2:                                    # the unbiased kernels read no table: no 4-byte LDS gathers (ds_read_b32)
        body = asm[asm.index(name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert not re.search(r"^\s*ds_read_b32", body, re.M), name
    for name in rpb:
        body = asm[asm.index(name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert re.search(r"^\s*ds_read_b32", body, re.M), name


@needs_hipcc
def test_beit_kernels_have_no_scratch(tmp_path):
    k = _compile(tmp_path, "beit.hip")
    assert len(k) == 2, list(k)
    assert all(s == 0 and v <= 256 for s, v, _ in k.values()), k
