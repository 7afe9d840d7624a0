"""Build-time guard for the bf16 mode of the MiDaS BEiT core: the bias form of the 32-queries-per-wave bf16 attention (csrc/vit.hip
vit_attention32_kernel<true>) uses no scratch and runs the two blocks per CU its design states (39 KiB of LDS per block at 24 x 32, at most 256
registers); the unbiased instantiation -- the kernel of the bf16 bench figure -- keeps its registers and reads no table; the two bf16 helpers of
csrc/beit_bf16.hip use no scratch."""
import os
import re

from tests.test_wino_f16x2_resources import _compile, needs_hipcc


@needs_hipcc
def test_bf16_rpb_attention_resources(tmp_path):
    k = _compile(tmp_path, "vit.hip", ("-save-temps=obj", "-Wno-unused-result"))
    a32 = {n: r for n, r in k.items() if "vit_attention32_kernel" in n}
    rpb = {n: r for n, r in a32.items() if "ILb1E" in n}
    plain = {n: r for n, r in a32.items() if "ILb0E" in n}
    assert len(rpb) == 1 and len(plain) == 1, list(k)
    for n, (s, v, o) in rpb.items():
        assert s == 0 and v <= 256 and o >= 2, (n, s, v, o)           # two waves per SIMD = two 256-thread blocks per CU
    for n, (s, v, o) in plain.items():
        assert s == 0 and v <= 146 and o >= 2, (n, s, v, o)           # the parent's count: the template flag costs the unbiased kernel nothing
    listing = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    asm = open(tmp_path / listing[0]).read()

    def body(name):
        b = asm[asm.index(name + ":"):]
        return b[:b.index(".Lfunc_end")]
    (pn,), (rn,) = list(plain), list(rpb)
    assert not re.search(r"^\s*ds_read_b32", body(pn), re.M)          # no table gather in the unbiased kernel
    assert len(re.findall(r"^\s*ds_read_b32", body(rn), re.M)) >= 32  # one 4-byte gather per logit of a 64-key tile
    for n in (pn, rn):
        assert len(re.findall(r"^\s*v_mfma_f32_32x32x16_bf16", body(n), re.M)) >= 16
    # two blocks per CU by LDS as well: 2 x (32 KiB + the 24 x 32 slice) <= 160 KiB
    assert 2 * (32768 + (28 * 63 + 3) * 4) <= 160 * 1024


@needs_hipcc
def test_beit_bf16_helpers_have_no_scratch(tmp_path):
    k = _compile(tmp_path, "beit_bf16.hip")
    assert len(k) == 2, list(k)
    assert all(s == 0 and v <= 256 for s, v, _ in k.values()), k
