"""FakePngDecodeOps plus the two subsequence entry points of hip_ops, run through the C host models (pf_pngd_scan_par_host,
pf_pngd_inflate_par_host: the lane decoder and round schedule the kernels compile, in plain loops), so that the host side of
decode_png(block_decode='subsequences') can be checked without a GPU."""
import numpy as np
import torch

import patchfusion_amd._lib as L
from tests.png_decode_fake_ops import FakePngDecodeOps


def _ptr(t):
    return t.data_ptr()


class FakePngInflateParOps(FakePngDecodeOps):
    def __init__(self, candidate_capacity=None):
        super().__init__(candidate_capacity)
        self.lib = L.load()

    def pngd_scan_par(self, words, nbits, starts, n, max_block_bits, expected, subsequence_bits, records, max_rounds):
        self.calls.append(("scan_par", int(n), int(max_block_bits), int(subsequence_bits)))
        assert words.is_contiguous() and starts.is_contiguous() and records.is_contiguous() and max_rounds.dtype == torch.int32
        rc = self.lib.pf_pngd_scan_par_host(_ptr(words), words.numel(), int(nbits), _ptr(starts), int(n), int(max_block_bits), int(expected),
                                            int(subsequence_bits), _ptr(records), _ptr(max_rounds))
        assert rc == 0, rc
        return records

    def pngd_inflate_par(self, words, nbits, blocks, expected, subsequence_bits, lit, ref, status, max_rounds):
        self.calls.append(("inflate_par", blocks.shape[0], int(subsequence_bits)))
        assert all(t.is_contiguous() for t in (words, blocks, lit, ref)) and status.dtype == torch.int32 and max_rounds.dtype == torch.int32
        flags = torch.zeros(1, dtype=torch.int32)
        flags[0] = status[0]
        lit.zero_()                                   # what a refused block leaves unwritten: the numpy resolve of the parent indexes with it
        ref.copy_(torch.arange(ref.numel(), dtype=torch.int32))
        rc = self.lib.pf_pngd_inflate_par_host(_ptr(words), words.numel(), int(nbits), _ptr(blocks), blocks.shape[0], int(expected),
                                               int(subsequence_bits), _ptr(lit), _ptr(ref), _ptr(flags), _ptr(max_rounds))
        assert rc == 0, rc
        status[0] = flags[0]


def host_words(deflate):
    """deflate bytes -> (int32 tensor of the padded words, nbits)"""
    n = len(deflate)
    w = np.zeros(4 * ((n + 3) // 4 + 2), dtype=np.uint8)
    w[:n] = np.frombuffer(bytes(deflate), dtype=np.uint8)
    return torch.from_numpy(w.view(np.int32)), 8 * n
