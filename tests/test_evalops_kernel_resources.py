"""Build-time guard for csrc/evalops.hip, modelled on tests/test_kernel_resources.py: the two evaluation-side kernels are plain
streaming code with a handful of registers; scratch would mean the compiler turned the small per-thread colour array or the LDS tile
loops into private memory."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_evalops_kernels_have_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "patchfusion_amd", "csrc", "evalops.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result", "-c", src,
                        "-o", str(tmp_path / "evalops.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"VGPRs: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == 2, names
    assert any("depth_boundaries_kernel" in n for n in names) and any("colorize_bgr_kernel" in n for n in names), names
    assert not any(scratch), dict(zip(names, scratch))
    assert max(vgprs) <= 64, dict(zip(names, vgprs))                  # eight waves per SIMD: the kernels hide latency by occupancy alone
