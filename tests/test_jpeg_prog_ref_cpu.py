"""The NumPy model of the progressive decoder and its writer (tests/jpeg_prog_ref.py) against PIL (libjpeg-turbo): the model decodes every
fixture file and freshly encoded files to PIL's pixels, and PIL decodes what the writer makes to the model's pixels."""
import numpy as np
import pytest

from tests import jpeg_prog_ref as G
from tests import jpeg_ref as R

CASES = G.load_cases()
SUPPORTED = [n for n in CASES if CASES[n][1] is not None]


def test_fixture_holds_the_cases():
    assert len(SUPPORTED) == 14 and sum(n.startswith("w_") for n in SUPPORTED) == 4 and len(CASES) == 17
    kinds = {G.KINDS[s.kind] for s in G.parse(CASES["100x75_smooth_420_q75"][0])[1]}
    assert kinds == set(G.KINDS)                                  # PIL's script covers all four scan kinds
    h, scans = G.parse(CASES["100x75_smooth_420_q75"][0])
    assert (scans[1].bx, scans[1].by, h.mcus_x * 2, h.mcus_y * 2) == (13, 10, 14, 10)


def test_model_equals_pil_on_every_fixture_file():
    bad = [n for n in SUPPORTED if not np.array_equal(G.decode(CASES[n][0]), CASES[n][1])]
    assert not bad, bad


@pytest.mark.parametrize("sub", ["4:4:4", "4:2:2", "4:2:0", None])
def test_model_equals_pil_live(sub):
    a = R.image("smooth", 37, 53, 31, grey=sub is None)
    for kw in (dict(quality=85), dict(quality=40, restart_blocks=2), dict(quality=97, optimize=True)):
        data = R.pil_encode(a, subsampling=sub, progressive=True, **kw)
        assert np.array_equal(G.decode(data), R.pil_decode(data)), (sub, kw)


def test_pil_decodes_writer_made_files_to_the_model_s_pixels():
    data = R.pil_encode(R.image("noise", 40, 56, 32), quality=92, subsampling="4:2:0", progressive=True)
    parsed = G.parse(data)
    coef = G.decode_entropy(data, parsed)
    scripts = [G.PIL_SCRIPT,
               [((0, 1, 2), 0, 0, 0, 0)] + [((c,), 1, 63, 0, 0) for c in range(3)],
               [((0,), 0, 0, 0, 2), ((1,), 0, 0, 0, 0), ((2,), 0, 0, 0, 0), ((0,), 0, 0, 2, 1), ((0,), 0, 0, 1, 0)] +
               [s for c in range(3) for s in (((c,), 1, 9, 0, 3), ((c,), 10, 63, 0, 1), ((c,), 1, 9, 3, 2), ((c,), 1, 9, 2, 1), ((c,), 1, 63, 1, 0))]]
    for script in scripts:
        made = G.write(parsed[0], coef, script)
        assert np.array_equal(R.pil_decode(made), G.decode(made))
        assert [(tuple(s.comps), s.ss, s.se, s.ah, s.al) for s in G.parse(made)[1]] == [tuple(s) for s in script]
    # interleaved DC covers the padded grid: the round trip gives the array back in full
    assert np.array_equal(G.decode_entropy(G.write(parsed[0], coef, G.PIL_SCRIPT)), coef)


def test_long_run_file_holds_a_long_run():
    """its luma AC-first scan is a few symbols: end-of-band runs that each cover many blocks"""
    data = CASES["w_long_eob_run"][0]
    h, scans = G.parse(data)
    s = scans[1]
    scan, segs = G.prepare_scan(data, s)
    assert s.kind == G.AC_FIRST and s.nblocks == 130 and segs[0][1] < 8 * 64        # 130 blocks in under 64 bytes
    assert G.sync_model(h, s, data, 32) >= 1
