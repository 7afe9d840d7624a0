"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/gt_readers.npz by running the REFERENCE'S OWN PYTHON for the ground-truth files
(csrc/gtread.hip, patchfusion_amd/groundtruth.py) on the cases of tests/gt_ref.py golden_cases():

  DepthMap   estimator/datasets/general_dataset.py:60-143   every dataset: `gt` and `edge`
  readPFM    estimator/datasets/utils.py:5-49               a grey and a colour file

Inputs are stored as the FILE'S BYTES (uint8), outputs as arrays; no case is larger than 37 x 53.  The driver (tests/gt_ref.py
run_reference) writes each case under a temporary directory laid out by the reference's path rules (val_gt / val_factor, gts / calibs),
stands in for cv2.imread / imageio.imread (stubs in the build container) with the samples the PNG was written from, and redirects
DepthMap's hard-coded 4032 x 6048 eth3d shape to the case's.

Run in the build container only:   python tools/make_golden_gt.py
NOTE: executes under the installed numpy (Python floats meet float32 arrays as weak scalars, as under the numpy the reference pins).
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402,F401
from tests import gt_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "gt_readers.npz")


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case in R.golden_cases():
            out[f"{case['name']}.file"] = np.frombuffer(case["data"], dtype=np.uint8)
            for k, v in R.run_reference(case, tmp).items():
                out[f"{case['name']}.{k}"] = v
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
