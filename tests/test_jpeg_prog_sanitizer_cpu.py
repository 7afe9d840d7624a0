"""The progressive half of csrc/jpeg_host.h stand-alone under the host sanitizers (the pattern of tests/test_jpeg_sanitizer_cpu.py):
tests/host/jpeg_prog_host_main.cpp is built with AddressSanitizer and UBSan and run on fixture files and on truncated and bit-flipped
copies of them.  Host code only; nothing here is loaded into Python."""
import os
import shutil
import subprocess

import pytest

from tests import jpeg_prog_ref as G
from tests import jpeg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_progressive_host_code_stand_alone_under_host_sanitizers(tmp_path):
    exe = tmp_path / "jpeg_prog_host_main"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                        "-I", os.path.join(ROOT, "patchfusion_amd", "csrc"), os.path.join(ROOT, "tests", "host", "jpeg_prog_host_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = G.load_cases()
    names = ["100x75_smooth_420_q75", "100x75_smooth_420_rst", "37x53_noise_444_q95", "64x48_smooth_422_q50", "17x19_grey", "1x1", "64x64_constant",
             "orient6_17x19", "w_example2_script", "w_example3_script", "w_noninterleaved_dc", "w_long_eob_run", "refuse_incomplete",
             "refuse_no_first", "refuse_two_component_ac"]
    files = []
    for n in names:
        files.append(str(tmp_path / (n + ".jpg")))
        with open(files[-1], "wb") as f:
            f.write(cases[n][0])
    files.append(str(tmp_path / "baseline.jpg"))
    with open(files[-1], "wb") as f:
        f.write(R.load_cases()["17x19_smooth_422_opt"][0])
    r = subprocess.run([str(exe)] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.startswith("16 files, 12 decoded;"), r.stdout
