"""csrc/jpeg_host.h stand-alone under the host sanitizers (the pattern of tests/test_png_table_cpu.py): tests/host/jpeg_host_main.cpp is
built with AddressSanitizer and UBSan and run on fixture files and on truncated and bit-flipped copies of them.  Host code only; nothing
here is loaded into Python."""
import os
import shutil
import subprocess

import pytest

from tests import jpeg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_jpeg_host_header_stand_alone_under_host_sanitizers(tmp_path):
    exe = tmp_path / "jpeg_host_main"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                        "-I", os.path.join(ROOT, "patchfusion_amd", "csrc"), os.path.join(ROOT, "tests", "host", "jpeg_host_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = R.load_cases()
    names = ["37x53_noise_420_rst", "37x53_noise_444_q100", "17x19_smooth_422_opt", "17x19_noise_grey_q30", "64x48_smooth_rstrow", "1x1_noise_444_q30",
             "orient6_17x19", "256x256_smooth_q30", "refuse_progressive", "refuse_cmyk"]
    files = []
    for n in names:
        files.append(str(tmp_path / (n + ".jpg")))
        with open(files[-1], "wb") as f:
            f.write(cases[n][0])
    r = subprocess.run([str(exe)] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.startswith("10 files, 8 decoded;"), r.stdout
