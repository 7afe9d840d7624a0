"""Build-time guard for csrc/head_bwd.hip, modelled on tests/test_augment_kernel_resources.py: registers, LDS and scratch from the code
object's metadata, nothing else.
  * No kernel may use scratch: the per-lane bin arrays of the attractor and log-binomial kernels (four bins per lane) and the four MFMA
    accumulators of the weight-gradient kernel must stay in registers.
  * The weight-gradient kernel stages 32 pixels x 64 channels of both operands in rows padded to 80 floats: 2 x 32 x 80 x 4 = 20480 bytes of
    LDS (eight blocks would fit the 160 KiB of a CU).  It has no software pipeline: while one block waits for its global loads, the other
    blocks of the CU must keep the matrix pipe busy, so at least four blocks (one wave each per SIMD) stay resident: at most 128 VGPRs.
  * The log-binomial kernel keeps four bins per lane of y, the centre, the exponential and log C(n, k) (16 registers) next to three
    wave-wide reductions; it is bound by its expf / logf chains, not by memory latency: five waves per SIMD, at most 96 VGPRs
    (512 / 5 rounded down to the allocation granule of 8), as for the VALU-bound kernels of csrc/augment.hip.
  * Every other kernel is a gather or a per-pixel reduction hidden by resident waves alone: no LDS, at most 64 VGPRs (eight waves per SIMD).
The number of kernels is asserted so that a new one is noticed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_head_bwd_kernels_have_no_scratch_and_the_occupancy_they_need(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "patchfusion_amd", "csrc", "head_bwd.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result", "-c", src,
                        "-o", str(tmp_path / "head_bwd.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"VGPRs: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == len(lds) == 8 and len(set(names)) == 8, names
    for part in ("wgrad_partial_kernel", "wgrad_reduce_kernel", "resize_bwd_kernel", "logbinom_bwd_kernel", "act_bwd_kernel", "silog_bwd_kernel"):
        assert sum(part in n for n in names) == 1, (part, names)
    assert sum("attractor_bwd_kernel" in n for n in names) == 2, names
    table = dict(zip(names, zip(scratch, vgprs, lds)))
    assert not any(scratch), table
    for n, (_, v, l) in table.items():
        assert v <= (128 if "wgrad_partial_kernel" in n else 96 if "logbinom_bwd_kernel" in n else 64), table
        assert l == (2 * 32 * 80 * 4 if "wgrad_partial_kernel" in n else 0), table
