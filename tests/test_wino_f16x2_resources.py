"""Build-time guard for the fp16x2 Winograd kernels (csrc/wino_f16x2.hip and the F16 instantiations of gemm_split3_persist192_kernel): no register
spills, the GEMM at two waves per SIMD, and none of its hand-counted LDS-DMA waits left without a matching piece count (the three-slot ring waits
vmcnt(6) = one chunk's pieces per wave, or vmcnt(0))."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def _compile(tmp_path, name, extra=()):
    src = os.path.join(ROOT, "patchfusion_amd", "csrc", name)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-c", src, "-o", str(tmp_path / "k.o"),
                        "-Rpass-analysis=kernel-resource-usage", *extra], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"VGPRs: (\d+)", r.stderr)]
    occ = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == len(occ)
    return {n: (s, v, o) for n, s, v, o in zip(names, scratch, vgprs, occ)}


@needs_hipcc
def test_f16x2_transform_kernels_have_no_scratch(tmp_path):
    k = _compile(tmp_path, "wino_f16x2.hip")
    assert len(k) == 3, list(k)                          # channel maxima, U' split, input transform
    assert not any(s for s, _, _ in k.values()), k
    assert max(v for _, v, _ in k.values()) <= 256, k


@needs_hipcc
def test_f16x2_gemm_has_no_scratch_and_counted_waits(tmp_path):
    k = _compile(tmp_path, "gemm_split3.hip", ("-save-temps=obj",))
    f16 = {n: r for n, r in k.items() if "persist192" in n and "ILb1ELb1ELb1E" in n}
    assert len(f16) == 2, list(k)                        # three-slot ring (default) and two slots (PF_F16_SLOTS=2)
    for n, (s, v, o) in f16.items():
        assert s == 0 and o >= 2, (n, s, v, o)
    listing = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    assert listing
    asm = open(tmp_path / listing[0]).read()
    body = asm[asm.index("persist192_kernelILb1ELb1ELb1ELi3EEEv14pf_conv_paramsiiiii:"):]
    body = body[:body.index(".Lfunc_end")]
    waits = set(re.findall(r"s_waitcnt vmcnt\((\d+)\)", body))
    assert waits <= {"0", "6"}, waits
    assert "6" in waits
