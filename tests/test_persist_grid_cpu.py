"""The grid of the persistent GEMM launchers (csrc/pf_launch.h persist_grid, asked through pf_persist_grid: no launch, no GPU), against the rule of each
launcher restated here, one function per launcher.  Every rule starts from the CUs, then the caller's cap, then PF_S3_GRID, then at most one block per
tile, rounded down to a multiple of 8; they differ in which of the two knobs they honour and in what fewer than 8 blocks mean.  Answers: the grid,
FALLBACK = the one-tile kernel runs the call, REFUSED = PF_ERR_ARG."""
import itertools

import pytest

from patchfusion_amd import _lib

CAP, ENV, FLOOR8, FALLBACK_RULE, REFUSE_RULE = 1, 2, 4, 8, 16          # PF_GRID_* of include/pf_hip.h
FALLBACK, REFUSED = 0, -1
INT_MAX = 2 ** 31 - 1

CUS = (8, 104, 256, 304)
GRID_CAPS = (0, 7, 8, 100, 1000)
TOTALS = (1, 7, 8, 9, 255, 256, 257, 3672, 2 ** 31 - 1, 2 ** 31)
S3_GRIDS = (None, "0", "4", "8", "40", "x")


def _atoi(s):
    try:
        return int(s)
    except ValueError:
        return 0


def _blocks(cus, total, grid_cap=0, s3_grid=None):
    """CUs -> cap -> PF_S3_GRID (replaces both) -> at most one block per tile -> a multiple of 8 (possibly 0)"""
    grid = cus
    if 0 < grid_cap < grid:
        grid = grid_cap
    if s3_grid is not None:
        grid = _atoi(s3_grid)
    return min(grid, total) & ~7


def split3_128(cus, grid_cap, total, s3_grid):
    """launch_persist (pf_gemm_split3, 128 x 128 tiles): cap and PF_S3_GRID; fewer than 8 blocks fall back to the one-tile kernel"""
    if total > INT_MAX:
        return REFUSED
    return _blocks(cus, total, grid_cap, s3_grid) or FALLBACK


def split3_192(cus, grid_cap, total, s3_grid):
    """launch_persist192 (pf_gemm_split3, 192 x 192 tiles): as the 128-tile launcher"""
    if total > INT_MAX:
        return REFUSED
    return _blocks(cus, total, grid_cap, s3_grid) or FALLBACK


def f16x2_points_192(cus, grid_cap, total, s3_grid):
    """launch_persist192_f16 (pf_gemm_f16x2_points): the cap, no PF_S3_GRID; fewer than 8 blocks are refused"""
    if total > INT_MAX:
        return REFUSED
    return _blocks(cus, total, grid_cap) or REFUSED


def f16x2_linear_192(cus, grid_cap, total, s3_grid):
    """launch_persist192_f16_linear (pf_gemm_f16x2, 192 x 192 tiles): neither knob; never fewer than 8 blocks"""
    if total > INT_MAX:
        return REFUSED
    return max(_blocks(cus, total), 8)


def f16x2_linear_160(cus, grid_cap, total, s3_grid):
    """pf_launch_f16x2_tile160 (pf_gemm_f16x2, 160 x 256 tiles): PF_S3_GRID, no cap; never fewer than 8 blocks"""
    if total > INT_MAX:
        return REFUSED
    return max(_blocks(cus, total, 0, s3_grid), 8)


def f16x2_points_128(cus, grid_cap, total, s3_grid):
    """pf_gemm_f16x2_points128: the cap, no PF_S3_GRID; never fewer than 8 blocks"""
    if total > INT_MAX:
        return REFUSED
    return max(_blocks(cus, total, grid_cap), 8)


LAUNCHERS = [(split3_128, CAP | ENV | FALLBACK_RULE), (split3_192, CAP | ENV | FALLBACK_RULE), (f16x2_points_192, CAP | REFUSE_RULE),
             (f16x2_linear_192, FLOOR8), (f16x2_linear_160, ENV | FLOOR8), (f16x2_points_128, CAP | FLOOR8)]


@pytest.fixture
def no_s3_switches(monkeypatch):
    for v in ("PF_S3_TILE_NOW", "PF_S3_PERSIST", "PF_S3_T192", "PF_S3_GRID"):
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


@pytest.mark.parametrize("rule,policy", LAUNCHERS, ids=[r.__name__ for r, _ in LAUNCHERS])
def test_grid_of_every_launcher(no_s3_switches, rule, policy):
    L = _lib.load()
    seen = set()
    for s3_grid in S3_GRIDS:                                             # (read per call: the library sees the change without a reload)
        if s3_grid is None:
            no_s3_switches.delenv("PF_S3_GRID", raising=False)
        else:
            no_s3_switches.setenv("PF_S3_GRID", s3_grid)
        for cus, grid_cap, total in itertools.product(CUS, GRID_CAPS, TOTALS):
            want = rule(cus, grid_cap, total, s3_grid)
            got = L.pf_persist_grid(cus, grid_cap, total, policy)
            assert got == want, (rule.__name__, cus, grid_cap, total, s3_grid, got, want)
            assert got in (FALLBACK, REFUSED) or (got % 8 == 0 and 8 <= got <= max(8, total))
            seen.add("grid" if got > 0 else got)
    small = FALLBACK if policy & FALLBACK_RULE else REFUSED if policy & REFUSE_RULE else None
    assert seen == {"grid", REFUSED} | ({small} if small is not None else set())      # every answer the rule can give was met


def test_the_launchers_differ_where_the_table_says(no_s3_switches):
    """one input per column of the table on which the rules part: the cap, the switch, fewer than 8 blocks"""
    L = _lib.load()
    grids = lambda cus, cap, total: [L.pf_persist_grid(cus, cap, total, policy) for _, policy in LAUNCHERS]
    assert grids(256, 100, 3672) == [96, 96, 96, 256, 256, 96]
    assert grids(256, 0, 7) == [FALLBACK, FALLBACK, REFUSED, 8, 8, 8]
    no_s3_switches.setenv("PF_S3_GRID", "40")
    assert grids(256, 100, 3672) == [40, 40, 96, 256, 40, 96]
    no_s3_switches.setenv("PF_S3_GRID", "4")
    assert grids(256, 100, 3672) == [FALLBACK, FALLBACK, 96, 256, 8, 96]


def test_bad_queries_answer_minus_one(no_s3_switches):
    L = _lib.load()
    assert L.pf_persist_grid(256, 0, 3672, CAP | ENV | FALLBACK_RULE) == 256
    for cus, total, policy in ((0, 3672, FLOOR8), (-8, 3672, FLOOR8), (256, 0, FLOOR8), (256, -1, FLOOR8), (256, 3672, 0), (256, 3672, CAP | ENV),
                               (256, 3672, FLOOR8 | FALLBACK_RULE), (256, 3672, FALLBACK_RULE | REFUSE_RULE), (256, 3672, 32 | FLOOR8)):
        assert L.pf_persist_grid(cus, 0, total, policy) == REFUSED, (cus, total, policy)
