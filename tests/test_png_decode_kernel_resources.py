"""Build-time guard for csrc/png_decode.hip, in the style of tests/test_jpeg_kernel_resources.py: it compiles for gfx950, none of its
kernels uses scratch (the finder keeps a whole dynamic header in registers; the decoders keep their tables in LDS), and every kernel's
LDS is static and inside the 64 KiB a block gets without asking."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the unfilter kernel comes once per filter distance (1, 2, 3, 4, 6, 8 bytes), the final conversion once per sample size
KERNELS = {"pngd_find_kernel": 1, "pngd_scan_kernel": 1, "pngd_inflate_kernel": 1, "pngd_jump_kernel": 1, "pngd_gather_kernel": 1,
           "pngd_adler_kernel": 1, "pngd_adler_final_kernel": 1, "pngd_unfilter_kernel": 6, "pngd_expand_bits_kernel": 1,
           "pngd_expand_16_kernel": 1, "pngd_to_rgb8_kernel": 2}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_png_decode_kernels_have_no_scratch_and_static_lds(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "patchfusion_amd", "csrc", "png_decode.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result", "-c", src,
                        "-o", str(tmp_path / "png_decode.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"VGPRs: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == len(lds) == sum(KERNELS.values()), names
    for kernel, count in KERNELS.items():
        assert sum(kernel in n for n in names) == count, (kernel, names)
    assert not any(scratch), dict(zip(names, scratch))
    for n, v, l in zip(names, vgprs, lds):
        if "scan" in n or "inflate" in n:
            assert l <= 4096 and v <= 64, (n, v, l)            # lengths, counts, symbols, a 10-bit and an 8-bit lookup: 32 one-wave blocks fit a CU's LDS
        elif "unfilter" in n:
            assert l <= 36 * 1024 and v <= 128, (n, v, l)      # the ring: (rows + 1) x (2 tiles of 64 pixels + pad)
        else:
            assert l == 0 and v <= 64, (n, v, l)
