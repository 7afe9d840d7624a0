"""Build-time guard for csrc/augment.hip, modelled on tests/test_gtread_kernel_resources.py.  Both kernels are gather-and-stream -- a few
dependent byte or float loads per output pixel, one 16-byte store per plane and thread -- with no LDS and no software pipeline, so the
latency of the gathers is hidden by resident waves alone: scratch (the per-thread pixel arrays turned into private memory) or a register
count that halves the occupancy would show as time, not as a wrong result.
  * The plane kernels and the image kernels without the colour step are memory-latency bound: they must keep all eight waves per SIMD,
    i.e. at most 64 VGPRs (512 / 8).
  * The image kernels with the colour step evaluate twelve double-precision powers per thread; between the gathers of one group of pixels
    and those of the next lie a few thousand VALU cycles of that power (about 130 double-precision instructions each), against roughly
    900 cycles for a load that misses to HBM: the kernel is VALU bound, and a second wave per SIMD would already cover the gathers.  The
    bound asks for five waves, at most 96 VGPRs (512 / 5 rounded down to the allocation granule of 8), so that growth is noticed long
    before it matters.
The number of instantiations (image: colour x vector stores; planes: one or two planes x vector stores) is asserted so that a new one is
noticed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_augment_kernels_have_no_scratch_and_the_occupancy_they_need(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "patchfusion_amd", "csrc", "augment.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result", "-c", src,
                        "-o", str(tmp_path / "augment.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"VGPRs: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == len(lds) == 8 and len(set(names)) == 8, names
    image = [n for n in names if "aug_image_kernel" in n]
    assert len(image) == 4 and sum("aug_planes_kernel" in n for n in names) == 4, names
    assert not any(scratch) and not any(lds), dict(zip(names, zip(scratch, lds)))
    for n, v in zip(names, vgprs):
        coloured = "aug_image_kernelILb1E" in n                          # template <bool COLOUR, bool VEC>
        assert v <= (96 if coloured else 64), dict(zip(names, vgprs))
    assert sum("aug_image_kernelILb1E" in n for n in names) == 2
