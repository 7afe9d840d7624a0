"""Build-time guard for csrc/wino_f16x2_n256.hip: two kernels (the 128-tile fp16x2 product and the maxima-merging output transform), no register
spills; the product at its designed 160 VGPRs (+ 8 of margin; LDS gives two waves per SIMD: eight waves on 96 KiB), and the hand-counted LDS-DMA waits of its listing are the set its header comment states: vmcnt(4) = one chunk's four pieces
per wave, and vmcnt(0)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@needs_hipcc
def test_n256_gemm_has_no_scratch_and_counted_waits(tmp_path):
    src = os.path.join(ROOT, "patchfusion_amd", "csrc", "wino_f16x2_n256.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-c", src, "-o", str(tmp_path / "k.o"),
                        "-Rpass-analysis=kernel-resource-usage", "-save-temps=obj"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "warning:" not in r.stderr, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"VGPRs: (\d+)", r.stderr)]
    agprs = [int(x) for x in re.findall(r"AGPRs: (\d+)", r.stderr)]
    occ = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    assert len(names) == 2 and sum("gemm_f16x2_persist128_kernel" in n for n in names) == 1 and sum("wino_output_cmax_kernel" in n for n in names) == 1, names
    assert scratch == [0, 0], scratch
    g = [i for i, n in enumerate(names) if "gemm_f16x2_persist128_kernel" in n][0]
    assert vgprs[g] + agprs[g] <= 168 and occ[g] >= 3, (vgprs, agprs, occ)               # designed: 160 VGPRs, no AGPRs
    assert vgprs[1 - g] + agprs[1 - g] <= 256 and occ[1 - g] >= 2, (vgprs, agprs, occ)   # output transform: 242, two waves per SIMD like wino_output_kernel<4> (231)
    listing = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    assert listing
    asm = open(tmp_path / listing[0]).read()
    body = asm[asm.index("gemm_f16x2_persist128_kernelE14pf_conv_paramsiii:"):]
    body = body[:body.index(".Lfunc_end")]
    assert set(re.findall(r"s_waitcnt vmcnt\((\d+)\)", body)) == {"0", "4"}
    nm = len(re.findall(r"v_mfma_f32_16x16x32_f16", body))
    assert nm > 0 and nm % 24 == 0 and "v_mfma_f32_16x16x32_bf16" not in body
