"""Build-time guard for csrc/jpeg.hip, modelled on tests/test_png_kernel_resources.py: it compiles for gfx950 and none of its eight kernels
uses scratch.  In the two entropy kernels a spill would put the decoder state (p, b, k) into private memory inside the symbol loop; in the
inverse DCT it would mean the 64-value workspace of a block left the registers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("jpeg_sync_kernel", "jpeg_lane_scan_kernel", "jpeg_write_kernel", "jpeg_dc_partial_kernel", "jpeg_dc_carry_kernel",
           "jpeg_dc_apply_kernel", "jpeg_idct_kernel", "jpeg_color_store_kernel")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_jpeg_kernels_have_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "patchfusion_amd", "csrc", "jpeg.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result", "-c", src,
                        "-o", str(tmp_path / "jpeg.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"VGPRs: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == len(lds) == len(KERNELS), names
    for kernel in KERNELS:
        assert sum(kernel in n for n in names) == 1, (kernel, names)
    assert not any(scratch), dict(zip(names, scratch))
    by = lambda vals, k: next(v for n, v in zip(names, vals) if k in n)      # noqa: E731
    # the build reports 22 / 24 VGPRs for the entropy kernels and 8608 bytes of LDS: six decode tables of 1424 bytes + the zigzag table
    # (2152 words).  Eight waves per SIMD (which hide the dependent table reads of the symbol loop) hold up to 64 VGPRs; the bound stays
    # at 32 because a symbol loop that needs more than the state, the window and a table pointer has grown something it should not have.
    for k in ("jpeg_sync_kernel", "jpeg_write_kernel"):
        assert by(vgprs, k) <= 32 and by(lds, k) == 4 * 2152, (k, by(vgprs, k), by(lds, k))
    # one thread holds a whole 8 x 8 block in registers: 109 VGPRs reported = four waves per SIMD (512 / 128); above 128 it would be three
    assert by(vgprs, "jpeg_idct_kernel") <= 128
    # the scans stage 1024 words / 256 four-int aggregates in LDS (4096 bytes each); everything else is light
    assert max(v for n, v in zip(names, vgprs) if "idct" not in n) <= 32
    assert max(v for n, v in zip(names, lds) if "sync" not in n and "write" not in n) <= 4096
