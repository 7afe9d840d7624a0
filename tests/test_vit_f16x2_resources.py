"""Build-time guard for the fp16x2 ViT linears: the epilogue form of gemm_split3_persist192_kernel<F16> (pf_gemm_f16x2) has no scratch, runs two waves
per SIMD, and its only vector-memory waits are vmcnt(0) and the ring's hand-counted vmcnt(6) (one chunk's six LDS-DMA pieces per wave); the
LayerNorm producer has no scratch."""
import os
import re

import pytest

from tests.test_wino_f16x2_resources import _compile, needs_hipcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@needs_hipcc
def test_f16x2_linear_gemm_resources_and_waits(tmp_path):
    k = _compile(tmp_path, "gemm_split3.hip", ("-save-temps=obj",))
    lin = {n: r for n, r in k.items() if "persist192" in n and "ILb0ELb1ELb1ELi3E" in n}
    assert len(lin) == 1, list(k)
    for n, (s, v, o) in lin.items():
        assert s == 0 and o >= 2, (n, s, v, o)
    listing = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    asm = open(tmp_path / listing[0]).read()
    body = asm[asm.index("persist192_kernelILb0ELb1ELb1ELi3EEEv14pf_conv_paramsiiiii:"):]
    body = body[:body.index(".Lfunc_end")]
    waits = set(re.findall(r"s_waitcnt vmcnt\((\d+)\)", body))
    assert waits <= {"0", "6"}, waits
    assert "6" in waits
    assert body.count("v_mfma_f32_16x16x32_f16") > 0 and "v_mfma_f32_16x16x32_bf16" not in body


@needs_hipcc
def test_layernorm_f16x2_has_no_scratch(tmp_path):
    k = _compile(tmp_path, "vit.hip")
    ln = {n: r for n, r in k.items() if "layernorm_f16x2" in n}
    assert len(ln) == 1, list(k)
    assert all(s == 0 for s, _, _ in ln.values()), ln
