"""Host replays of the POINTS mode of the 160 x 256 fp16x2 tile (csrc/gemm_f16x2_t160.h persist160_body<true>, csrc/wino_f16x2_t160.hip): the walk
with the transform point in the tile index, the loader's piece addresses against the operand buffers, the barrier count of the two wave groups, and
the per-layer tile decision.  The ring's schedule and its hand-counted waits are those of the linear mode and are replayed by
tests/test_f16x2_tile160_model_cpu.py, whose model this file reuses.  Shapes: every case of tests/test_wino_f16x2_t160_gpu.py.  No GPU."""
import ctypes as C
import os

import pytest

from tests.test_f16x2_tile160_model_cpu import BM, BN, NW, XP, WP, persist160, piece_rows, pieces_of, simulate160

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_MOVES, NARROW_MOVES = 0, 1                         # what the measured rule does with the 768- and the 256-column class
# (T, K, N, u_rows, batch, grid_cap) -- the product-level cases of the GPU test
PRODUCT_CASES = [
    (8, 32, 256, 256, 36, 0),
    (152, 64, 256, 256, 36, 8),
    (160, 96, 512, 512, 36, 0),
    (168, 256, 768, 768, 36, 8),
    (325, 96, 768, 768, 36, 0),
    (325, 64, 256, 272, 36, 8),
    (325, 256, 512, 512, 2, 0),
    (168, 32, 768, 768, 1, 0),
    (160, 64, 768, 784, 2, 8),
    (325, 32, 256, 256, 1, 8),
    (152, 96, 512, 528, 36, 8),
]
IDS = ["T%d_K%d_N%d_r%d_b%d_cap%d" % c for c in PRODUCT_CASES]


def tiles(T, N):
    return -(-T // BM), -(-N // BN)


def launch_grid(total, cus, grid_cap):
    """pf_launch_f16x2_points160: PF_GRID_CAP | PF_GRID_FLOOR8 (csrc/pf_launch.h persist_grid)"""
    grid = cus
    if 0 < grid_cap < grid:
        grid = grid_cap
    grid = min(grid, total) & ~7
    return max(grid, 8)


def walk(batch, mt, nt, G):
    """per block: the (point, token tile, column tile) it visits, in order (the kernel's l_first / nb / decode with POINTS)"""
    total = batch * mt * nt
    out = []
    for b in range(G):
        xcd, nb = b & 7, (G - (b & 7) + 7) >> 3
        lo, hi = total * xcd // 8, total * (xcd + 1) // 8
        seq, l = [], lo + (b >> 3)
        while l < hi:
            z, r = divmod(l, mt * nt)
            seq.append((z, r // nt, r % nt))
            l += nb
        out.append(seq)
    return out


@pytest.mark.parametrize("case", PRODUCT_CASES, ids=IDS)
@pytest.mark.parametrize("G", [8, 64, 256])
def test_every_point_and_tile_is_computed_exactly_once(case, G):
    T, K, N, rows, batch, cap = case
    mt, nt = tiles(T, N)
    assert G == launch_grid(10 ** 9, G, 0)
    seen = [t for w in walk(batch, mt, nt, G) for t in w]
    assert len(seen) == batch * mt * nt == len(set(seen))
    assert set(seen) == {(z, m, n) for z in range(batch) for m in range(mt) for n in range(nt)}


@pytest.mark.parametrize("case", PRODUCT_CASES, ids=IDS)
def test_the_launch_grid_of_each_case_walks_every_tile_once(case):
    T, K, N, rows, batch, cap = case
    mt, nt = tiles(T, N)
    for cus in (256, 304, 64):
        G = launch_grid(batch * mt * nt, cus, cap)
        assert G % 8 == 0 and G >= 8
        walks = walk(batch, mt, nt, G)
        seen = [t for w in walks for t in w]
        assert len(seen) == batch * mt * nt == len(set(seen))
        if cap == 8 and batch * mt * nt > 8 * mt * nt:
            assert any(len({z for z, _, _ in w}) > 1 for w in walks), "grid_cap 8: a block must cross points"


def test_column_tiles_of_one_v_slab_are_neighbours():
    """the nt column tiles of a (point, token tile) are consecutive tile indices: one XCD's contiguous range holds them, except where a range ends"""
    mt, nt, batch = 60, 3, 36
    total = batch * mt * nt
    bounds = {total * x // 8 for x in range(9)}
    split = sum(1 for l0 in range(0, total, nt) if any(l0 < b < l0 + nt for b in bounds))
    assert split <= 7


# ---- piece addresses ---------------------------------------------------------------------------------------------------------------------------
def piece_span(case, z, tm, tn, kc, q, x_base, w_base):
    """[lowest, highest + 1) byte address the 64 lanes of stage piece q read for chunk kc of tile (z, tm, tn): setup_loader + kc advances"""
    T, K, N, rows, batch, cap = case
    op, pl, r0, _ = piece_rows(q)
    is_x = op == "x"
    lim = T if is_x else rows
    origin = tm * BM if is_x else tn * BN
    bstride = batch * lim * K                              # elements per plane (x_bstride / w_bstride)
    base = (x_base if is_x else w_base) + pl * bstride * 2 + z * lim * K * 2 + origin * 64 + kc * lim * 64
    last = lim - 1 - origin
    lo = hi = None
    for lane in range(64):
        r = r0 + (lane >> 2)
        row = q * 16 + (lane >> 2)
        j = (lane & 3) ^ ((row >> 1) & 3)
        a = base + min(r, last) * 64 + j * 16
        lo = a if lo is None else min(lo, a)
        hi = a + 16 if hi is None else max(hi, a + 16)
    return is_x, lo, hi


@pytest.mark.parametrize("case", PRODUCT_CASES, ids=IDS)
def test_every_piece_of_every_chunk_lies_inside_its_operand(case):
    T, K, N, rows, batch, cap = case
    mt, nt = tiles(T, N)
    x_base, w_base = 1 << 40, 1 << 41
    x_end, w_end = x_base + 2 * batch * (K // 32) * T * 64, w_base + 2 * batch * (K // 32) * rows * 64
    points = sorted({0, batch // 2, batch - 1})
    for z in points:
        for tm in range(mt):
            for tn in range(nt):
                assert tm * BM < T and tn * BN < rows       # the clamp min(r, last) needs last >= 0
                for kc in range(K // 32):
                    for q in range(XP + WP):
                        is_x, lo, hi = piece_span(case, z, tm, tn, kc, q, x_base, w_base)
                        if is_x:
                            assert x_base <= lo and hi <= x_end, (z, tm, tn, kc, q)
                        else:
                            assert w_base <= lo and hi <= w_end, (z, tm, tn, kc, q)
    # a point's slab really is its own: the first byte of point z, chunk 0, row 0 of plane h is z * rows * K * 2 past the operand
    assert piece_span(case, batch - 1, 0, 0, 0, 0, x_base, w_base)[1] == x_base + (batch - 1) * T * K * 2


# ---- the two groups meet at the same barriers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nk", [1, 2, 3, 8])
@pytest.mark.parametrize("my_tiles", [1, 2, 5])
def test_both_groups_pass_the_same_number_of_barriers(nk, my_tiles):
    chunks = nk * my_tiles
    simulate160(lambda w: persist160(chunks, nk, w, []), chunks)       # asserts one barrier count over the eight waves, reads after landings
    counts = []
    for w in range(NW):
        counts.append(sum(1 for ev in persist160(chunks, nk, w, []) if ev[0] == "barrier"))
    assert len(set(counts)) == 1 and counts[0] == 2 * chunks + 2, counts


@pytest.mark.parametrize("case", PRODUCT_CASES, ids=IDS)
def test_blocks_without_tiles_leave_before_any_barrier(case):
    """l_first >= hi returns ahead of the first barrier for ALL eight waves (the test is block-uniform); every other block has >= 1 tile"""
    T, K, N, rows, batch, cap = case
    mt, nt = tiles(T, N)
    total = batch * mt * nt
    G = launch_grid(total, 256, cap)
    for b, seq in enumerate(walk(batch, mt, nt, G)):
        xcd, nb = b & 7, (G - (b & 7) + 7) >> 3
        lo, hi = total * xcd // 8, total * (xcd + 1) // 8
        l_first = lo + (b >> 3)
        my_tiles = (hi - l_first + nb - 1) // nb if l_first < hi else 0
        assert my_tiles == len(seq)
    src = open(os.path.join(ROOT, "patchfusion_amd", "csrc", "gemm_f16x2_t160.h")).read()
    assert src.index("if (l_first >= hi) return;") < src.index("lds_barrier();")


# ---- the tile decision -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def decide(monkeypatch):
    from patchfusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpf_hip.so not built")
    L = _lib.load()
    monkeypatch.delenv("PF_WINO_F16_TILE", raising=False)

    def f(K, N, T, cus=256):
        """the product of a whole K -> N layer of T Winograd tiles, as csrc/winograd.hip f16x2_points_params fills it"""
        q = _lib.ConvParams()
        q.B, q.OH, q.OW, q.H, q.W, q.Cin, q.Cout, q.batch, q.w_rows = 1, 1, T, 1, T, K, N, 36, N
        q.x_ld, q.Kpad, q.y_ld, q.korder, q.out_f32 = K, K, N, 6, 1
        q.KH = q.KW = q.stride = q.shuffle = 1
        return L.pf_wino_f16x2_tile_route(C.byref(q), cus)
    f.L = L
    return f


# (K, N) -> the decision at default switches.  In scope and measured (profiles/r14_wino_t160_ab.md, r14_wino_t160_image_ab.md): 768 -> 256 and
# 512 -> 256 move; 768 -> 768 won per launch but missed the image-pass bar and stays.
# Out of scope, never moved: N = 544 (three column tiles for 2.1 tiles of columns), K = 256 (bound by V + M bytes), every other width.
DEFAULT = {(768, 768): WIDE_MOVES, (512, 768): WIDE_MOVES, (768, 256): NARROW_MOVES, (512, 256): NARROW_MOVES, (1024, 256): NARROW_MOVES,
           (544, 544): 0, (256, 256): 0, (256, 768): 0, (320, 256): 0, (768, 512): 0, (768, 1024): 0, (1024, 544): 0}
TILES = (312, 560, 924, 2128, 8288, 9600, 13056, 18048, 33152)       # whole layers and window sizes of the pass, and the layer tests' sizes
CUS = (64, 256, 304)


@pytest.mark.parametrize("K,N", sorted(DEFAULT))
def test_default_decision_per_layer_class(decide, K, N):
    """the rule at default switches, for every class at every size and CU count: it is a function of (K, N) alone today, so a layer and each
    of its windows -- whatever T a caller might pass -- run the same kernel"""
    for T in TILES:
        for cus in CUS:
            assert decide(K, N, T, cus) == DEFAULT[(K, N)], (K, N, T, cus)


@pytest.mark.parametrize("K,N", sorted(DEFAULT))
def test_switch_values(decide, monkeypatch, K, N):
    wide, narrow = int(N == 768 and K >= 512), int(N == 256 and K >= 512)
    for T in (312, 33152):
        for mode, want in (("0", 0), ("1", 1), ("2", wide), ("3", narrow)):
            monkeypatch.setenv("PF_WINO_F16_TILE", mode)
            assert decide(K, N, T) == want, (K, N, T, mode)
    assert decide.L.pf_wino_f16x2_tile_route(None, 256) == -1
    assert decide(K, N, 312, cus=0) == -1


def test_route_queries_keep_their_values(decide, monkeypatch):
    """the decision is separate from the route queries: whatever PF_WINO_F16_TILE says, they answer as before"""
    from patchfusion_amd import _lib
    L = decide.L
    q = _lib.ConvParams()
    q.B, q.OH, q.OW, q.H, q.W, q.Cin, q.Cout, q.batch, q.w_rows = 1, 1, 33152, 1, 33152, 768, 768, 36, 768
    q.out_f32, q.korder = 1, 6
    monkeypatch.delenv("PF_WINO_F16X2_N256", raising=False)
    for mode in (None, "0", "1"):
        if mode is None:
            monkeypatch.delenv("PF_WINO_F16_TILE", raising=False)
        else:
            monkeypatch.setenv("PF_WINO_F16_TILE", mode)
        assert L.pf_gemm_f16x2_points_route(C.byref(q), 256) == 3
        assert L.pf_gemm_f16x2_route(C.byref(q), 256) == 3                 # batch > 1: the 192-tile route
