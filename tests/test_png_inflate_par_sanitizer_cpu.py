"""The subsequence decode's host model stand-alone under the host sanitizers (the pattern of tests/test_png_decode_sanitizer_cpu.py):
tests/host/png_inflate_par_main.cpp is built with AddressSanitizer and UBSan and runs the lane decoder and the round schedule of
csrc/png_inflate.h / csrc/png_host.h -- the code the kernels of csrc/png_inflate_par.hip compile -- at lanes of 64 and 256 bits on intact
files, on the refusal files and, inside the program, on truncated and bit-flipped copies of their deflate data.  Host code only; nothing
here is loaded into Python."""
import os
import shutil
import subprocess

import pytest

from tests import png_decode_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_subsequence_host_model_stand_alone_under_host_sanitizers(tmp_path):
    exe = tmp_path / "png_inflate_par_main"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                        "-I", os.path.join(ROOT, "patchfusion_amd", "csrc"), os.path.join(ROOT, "tests", "host", "png_inflate_par_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    cases, fixture, refusals = R.device_cases(), R.load_cases(), R.refusal_cases()
    intact = ["many_blocks_48x64", "composite_150x200", "constant_64x64", "ramp_96x1024", "far_match", "paeth_130x3", "one_pixel", "fmt_ct3_d4_w13",
              "fmt_ct6_d16_w13"]
    files = [(n, cases[n]) for n in intact]
    files += [(n, fixture[n][0]) for n in ("pil_rgb_150x200_l1", "pil_i16_37x53", "encode_png_u16_24x40")]
    refused = ("truncated_idat", "adler_bit_flip", "one_row_short", "adam7", "fdict", "distance_before_start")
    files += [(n, refusals[n][0]) for n in refused]
    paths = []
    for n, data in files:
        paths.append(str(tmp_path / (n + ".png")))
        with open(paths[-1], "wb") as f:
            f.write(data)
    r = subprocess.run([str(exe)] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    # adam7 and fdict are refused by the parser; the other four refusal files parse and must not decode
    assert r.stdout.startswith("18 files, 16 parsed, 12 decoded;") and r.stdout.rstrip().endswith("0 records differ"), r.stdout
