"""Build-time guard for csrc/png_rle.hip in the manner of tests/test_png_kernel_resources.py: it compiles for gfx950 and none of its
kernels (six byte layouts each of the dual-histogram pass and of the run-match band encoder) uses scratch: a spill would mean the packed
bytes and head flags a lane carries from one chunk to the next, or the word it concatenates, went to private memory."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_png_rle_kernels_have_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "patchfusion_amd", "csrc", "png_rle.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result", "-c", src,
                        "-o", str(tmp_path / "png_rle.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"VGPRs: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == len(lds) == 12, names
    for kernel, count in (("png_rle_filter_hist_kernel", 6), ("png_rle_encode_band_kernel", 6)):
        assert sum(kernel in n for n in names) == count, (kernel, names)
    assert not any(scratch), dict(zip(names, scratch))
    assert max(vgprs) <= 128, dict(zip(names, vgprs))                 # four waves per SIMD at the least: a band is one 256-thread block
    assert max(lds) <= 8192, dict(zip(names, lds))                    # staging window + code table + head flags: many bands per CU
