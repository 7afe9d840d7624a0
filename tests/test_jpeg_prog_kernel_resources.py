"""Build-time guard for csrc/jpeg_prog.hip, in the style of tests/test_jpeg_kernel_resources.py: it compiles for gfx950 and none of its
kernels uses scratch.  In the entropy kernels a spill would put the decoder state (p, s) into private memory inside the symbol loop."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the sync and write kernels come once per scan kind (DC first, AC first); the carry kernel is jpeg_dev.h's
KERNELS = {"jpeg_prog_sync_kernel": 2, "jpeg_prog_write_kernel": 2, "jpeg_prog_lane_scan_kernel": 1, "jpeg_prog_dc_partial_kernel": 1,
           "jpeg_prog_dc_store_kernel": 1, "jpeg_prog_dc_refine_kernel": 1, "jpeg_prog_mask_kernel": 1, "jpeg_prog_apply_kernel": 1,
           "jpeg_dc_carry_kernel": 1}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_jpeg_prog_kernels_have_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "patchfusion_amd", "csrc", "jpeg_prog.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result", "-c", src,
                        "-o", str(tmp_path / "jpeg_prog.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"VGPRs: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == len(lds) == sum(KERNELS.values()), names
    for kernel, count in KERNELS.items():
        assert sum(kernel in n for n in names) == count, (kernel, names)
    assert not any(scratch), dict(zip(names, scratch))
    # the symbol loop holds the state, the window and a table pointer: the baseline kernels' bound (32 VGPRs, eight waves per SIMD with
    # room to spare) and their LDS (the 2152-word decode tables) hold here too
    for n, v, l in zip(names, vgprs, lds):
        if "sync" in n or "write" in n:
            assert v <= 32 and l == 4 * 2152, (n, v, l)
        else:
            # the mask kernel has its block's eight 16-byte loads in flight at once (32 VGPRs of data); 64 still is eight waves per SIMD
            assert v <= 64 and l <= 4096, (n, v, l)
