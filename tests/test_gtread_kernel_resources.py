"""Build-time guard for csrc/gtread.hip, modelled on tests/test_evalops_kernel_resources.py: the conversion kernels are streaming code
-- four samples in, one or two 16-byte stores out -- that hides latency by occupancy alone; scratch would mean the compiler turned the
small per-thread sample arrays into private memory.  The number of instantiations (five sample kinds x {vector loads, per-sample
loads}) is asserted so that a new one is noticed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_gtread_kernels_have_no_scratch_and_full_occupancy(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "patchfusion_amd", "csrc", "gtread.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result", "-c", src,
                        "-o", str(tmp_path / "gtread.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"VGPRs: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == 10, names
    assert all("gt_convert_kernel" in n for n in names) and len(set(names)) == 10, names
    assert not any(scratch), dict(zip(names, scratch))
    assert max(vgprs) <= 64, dict(zip(names, vgprs))                  # eight waves per SIMD
