"""Build-time guard for csrc/png_inflate_par.hip, in the style of tests/test_png_decode_kernel_resources.py: it compiles for gfx950, holds
exactly the scan and the inflate kernel, neither uses scratch, their LDS is static and inside the 64 KiB a workgroup gets without
asking, and their registers fit the workgroup size: a workgroup of PF_PNGD_PAR_WINDOW threads is PF_PNGD_PAR_WINDOW / 64 waves on the four
SIMDs of one compute unit, each SIMD with 512 VGPRs per lane."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("pngd_scan_par_kernel", "pngd_inflate_par_kernel")


def window_threads():
    txt = open(os.path.join(ROOT, "patchfusion_amd", "csrc", "png_inflate.h")).read()
    return int(re.search(r"#define PF_PNGD_PAR_WINDOW (\d+)", txt).group(1))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_subsequence_kernels_have_no_scratch_static_lds_and_fit_their_workgroup(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "patchfusion_amd", "csrc", "png_inflate_par.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result", "-c", src,
                        "-o", str(tmp_path / "png_inflate_par.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"VGPRs: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    dynamic = re.findall(r"Dynamic Stack: (\w+)", r.stderr)
    assert len(names) == len(scratch) == len(vgprs) == len(lds) == len(KERNELS), names
    for kernel in KERNELS:
        assert sum(kernel in n for n in names) == 1, (kernel, names)
    assert not any(scratch) and all(d == "False" for d in dynamic), dict(zip(names, scratch))
    threads = window_threads()
    assert threads % 64 == 0 and 64 <= threads <= 1024
    waves_per_simd = -(-threads // 64 // 4)
    for n, v, l in zip(names, vgprs, lds):
        assert 0 < l <= 64 * 1024, (n, l)                   # tables, the double-buffered exits and flags, the sums
        assert v <= 512 // waves_per_simd, (n, v, threads)  # 128 at 1024 threads: the whole workgroup is resident on one compute unit
