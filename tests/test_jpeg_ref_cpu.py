"""The NumPy restatement of the JPEG decoder (tests/jpeg_ref.py) equals PIL (libjpeg-turbo) exactly, live and on the fixture, and its model
of the device decoder's subsequence rounds converges to the sequential decoder's states."""
import numpy as np
import pytest

from tests import jpeg_ref as R

CASES = R.load_cases()


def test_restatement_equals_the_fixture():
    bad = [n for n, (data, exp) in CASES.items() if exp is not None and not np.array_equal(R.decode(data), exp)]
    assert not bad, bad


@pytest.mark.parametrize("sub", ["4:4:4", "4:2:2", "4:2:0", None])
def test_restatement_equals_pil_live(sub):
    for (H, W), kind, kw in [((1, 1), "noise", dict(quality=30)), ((15, 16), "smooth", dict(quality=100)), ((33, 7), "noise", dict(quality=90, optimize=True)),
                             ((37, 53), "noise", dict(quality=90, restart_blocks=1)), ((64, 48), "smooth", dict(quality=90))]:
        data = R.pil_encode(R.image(kind, H, W, 21, grey=sub is None), subsampling=sub, **kw)
        assert np.array_equal(R.decode(data), R.pil_decode(data)), (H, W, kind, kw)


@pytest.mark.parametrize("S", [32, 64, 128, 1024])
def test_round_model_converges_to_the_sequential_states(S):
    for name in ("37x53_noise_420_q90", "17x19_smooth_444_q100", "64x48_smooth_rstrow", "256x256_smooth_q30"):
        states, rounds, truth = R.sync_model(CASES[name][0], S)
        assert states == truth, (name, S, rounds)


def test_noise_256_arrives_only_along_the_chain():
    """the q100 noise file never self-synchronises (63 coefficients in every block): its true states arrive one lane per round.  At
    S = 1024 that is 121 rounds, the count tests/test_jpeg_gpu.py holds the device to.  Convergence of this file at S = 32, 64 and 128 is not
    checked here for the model's running time alone (3948 rounds at S = 32 take the Python model over two minutes); the GPU test holds the
    device's coefficients to the host decoder's at those lengths."""
    states, rounds, truth = R.sync_model(CASES["256x256_noise_q100"][0], 1024)
    assert states == truth and rounds == 121


@pytest.mark.parametrize("name", ["256x256_noise_q100", "256x256_smooth_q30"])
def test_both_256_files_need_three_rounds_at_32_bits(name):
    """a condition on the inputs: without it the round loop is never exercised.  Three rounds of the model show it: the third still changed
    states if the model is not converged after it."""
    states, rounds, truth = R.sync_model(CASES[name][0], 32, max_rounds=3)
    assert rounds == 3 and states != truth
