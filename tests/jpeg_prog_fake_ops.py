"""numpy stand-in for the progressive JPEG entry points of hip_ops (same arguments and buffers), built on tests/jpeg_prog_ref.py, so that
the progressive branch of preprocess.decode_jpeg can be checked without a GPU.  A baseline file goes to the base class."""
import numpy as np
import torch

from tests import jpeg_prog_ref as G
from tests import jpeg_ref as R
from tests.jpeg_fake_ops import FakeJpegOps


class FakeJpegProgOps(FakeJpegOps):
    def __init__(self, data):
        super().__init__(data)
        self.parsed = G.parse(data) if b"\xff\xc2" in data[:data.index(b"\xff\xda")] else None

    def _scan(self, scan):
        return next(s for s in self.parsed[1] if s.begin == scan.begin)

    def _apply(self, scan, coef):
        c = coef.numpy().astype(np.int64)
        G.decode_scan(self.parsed[0], self._scan(scan), self.data, c)
        coef.copy_(torch.from_numpy(c.astype(np.int16)))

    def jpeg_prog_workspace(self, nlanes, scan_blocks):
        return 16 + 36 * nlanes + 8 * scan_blocks

    def jpeg_prog_decode_scan(self, header, scan, data, lanes, segx, longest, tables, block_map, max_sync_rounds, workspace, coef):
        S = int(lanes[0, 1] - lanes[0, 0]) if lanes.shape[0] > 1 else 1 << 20
        rounds = G.sync_model(self.parsed[0], self._scan(scan), self.data, S)
        self.calls.append(("prog_scan", G.KINDS[scan.kind], S, int(max_sync_rounds), block_map is not None))
        if rounds > max_sync_rounds:
            return 64, max_sync_rounds
        self._apply(scan, coef)
        return 0, rounds

    def jpeg_prog_dc_refine(self, header, scan, data, segs, block_map, coef):
        self.calls.append(("prog_dc_refine", block_map is not None))
        self._apply(scan, coef)

    def jpeg_prog_nonzero_mask(self, header, scan, coef, block_map, masks):
        self.calls.append(("prog_mask", scan.comp[0]))
        m = G.nonzero_masks(self.parsed[0], self._scan(scan), coef.numpy())
        masks.copy_(torch.from_numpy(m.view(np.int64)))
        return masks

    def jpeg_prog_apply_refinement(self, header, scan, records, block_map, coef):
        self.calls.append(("prog_apply", scan.comp[0]))
        c = coef.numpy().copy()
        G.apply_records(self.parsed[0], self._scan(scan), c, records.numpy().view(np.uint64))
        coef.copy_(torch.from_numpy(c))

    def jpeg_reconstruct(self, header, coef, orientation, workspace, rgb):
        if self.parsed is None:
            return super().jpeg_reconstruct(header, coef, orientation, workspace, rgb)
        self.calls.append(("reconstruct", int(orientation)))
        rgb.copy_(torch.from_numpy(R.reconstruct(self.parsed[0], coef.numpy(), orientation)))
        return rgb
