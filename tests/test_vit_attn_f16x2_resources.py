"""Build-time guard for the fp16x2 attention (csrc/attn_split3.hip vit_attention_f16x2_pipe_kernel): no scratch, two waves per SIMD (two 48-KiB blocks
per CU: at most 256 registers), its only vector-memory waits are vmcnt(0) and the ring's hand-counted vmcnt(4) (the four LDS-DMA pieces a wave
issues per step), it multiplies on v_mfma_f32_32x32x16_f16 only, and its steady step comes out interleaved: 24 MFMAs and the sixteen exponentials
between two barriers with no long run of back-to-back MFMAs.  The row-major fp16x2 store form of the qkv GEMM lives in the kernel that
tests/test_vit_f16x2_resources.py guards."""
import os
import re

from tests.test_wino_f16x2_resources import _compile, needs_hipcc


@needs_hipcc
def test_f16x2_attention_resources_waits_and_interleave(tmp_path):
    k = _compile(tmp_path, "attn_split3.hip", ("-save-temps=obj",))
    att = {n: r for n, r in k.items() if "vit_attention_f16x2_pipe_kernel" in n}
    assert len(att) == 1, list(k)
    (name, (s, v, o)), = att.items()
    assert s == 0 and v <= 256 and o >= 2, (name, s, v, o)
    listing = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    asm = open(tmp_path / listing[0]).read()
    body = asm[asm.index(name + ":"):]
    body = body[:body.index(".Lfunc_end")]
    waits = set(re.findall(r"vmcnt\((\d+)\)", body))
    assert waits == {"0", "4"}, waits
    mfma = set(re.findall(r"v_mfma_\w+", body))
    assert mfma == {"v_mfma_f32_32x32x16_f16"}, mfma       # (bf16 appears only in the conversions of the three-plane output form)
    assert "scratch_" not in body
    ops = [ln.split()[0] for ln in body.splitlines() if ln.startswith("\t") and ln.strip() and not ln.strip().startswith((";", "."))]
    regions, cur = [], []
    for op in ops:
        if op == "s_barrier":
            regions.append(cur)
            cur = []
        else:
            cur.append(op)
    steady = [r for r in regions if sum(x.startswith("v_mfma") for x in r) == 24 and sum(x == "v_exp_f32_e32" for x in r) >= 16]
    assert len(steady) >= 2, [sum(x.startswith("v_mfma") for x in r) for r in regions]
    for r in steady:
        run = worst = 0
        for x in r:
            run = run + 1 if x.startswith("v_mfma") else 0
            worst = max(worst, run)
        assert worst <= 3, worst
