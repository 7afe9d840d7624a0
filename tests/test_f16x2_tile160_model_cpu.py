"""Host replays of the 160 x 256 tile form of the fp16x2 linear (csrc/gemm_f16x2_t160.hip), in the style of tests/test_split3_schedule_model_cpu.py:
the block / XCD tile walk, the map of a stage's 52 LDS-DMA pieces onto the eight waves, the three-slot ring's schedule with its hand-counted waits
(group A counts six pieces per chunk, group B seven), and the dispatch rule pf_gemm_f16x2_route.  No GPU."""
import ctypes as C
import os

import pytest

NW, NS = 8, 3
BM, BN = 160, 256
XP, WP = 2 * BM // 16, 2 * BN // 16          # 20 X pieces, 32 W pieces per stage
PA, PB = 6, 7
STAGE = (XP + WP) * 1024
P192, T160 = 3, 4


# ---- tile walk ---------------------------------------------------------------------------------------------------------------------------------
def launch_grid(mt, nt, cus=256, s3_grid=None):
    """pf_launch_f16x2_tile160: one block per CU, PF_S3_GRID for tests, at most one block per tile, a multiple of 8, never fewer than 8"""
    total = mt * nt
    grid = cus if s3_grid is None else s3_grid
    grid = min(grid, total) & ~7
    return max(grid, 8)


def walk(mt, nt, G):
    """per block: the (tile_m, tile_n) it visits, in order (the kernel's l_first / nb / decode)"""
    total = mt * nt
    out = []
    for b in range(G):
        xcd, nb = b & 7, (G - (b & 7) + 7) >> 3
        lo, hi = total * xcd // 8, total * (xcd + 1) // 8
        seq, l = [], lo + (b >> 3)
        while l < hi:
            seq.append((l // nt, l % nt))
            l += nb
        out.append(seq)
    return out


@pytest.mark.parametrize("mt,nt,s3_grid", [(52, 4, None), (52, 4, 8), (7, 4, 8), (7, 4, None), (1, 1, None), (1, 4, None), (3, 2, None), (1, 2, 8), (2, 1, None),
                                           (7, 12, None), (52, 16, None), (3, 5, 16), (9, 3, 24)])
def test_walk_visits_every_tile_exactly_once(mt, nt, s3_grid):
    G = launch_grid(mt, nt, 256, s3_grid)
    assert G % 8 == 0 and G >= 8
    walks = walk(mt, nt, G)
    seen = [t for w in walks for t in w]
    assert len(seen) == mt * nt == len(set(seen))
    assert all(0 <= m < mt and 0 <= n < nt for m, n in seen)
    lens = [len(w) for w in walks]
    assert max(lens) - min(lens) <= 1 + (1 if (mt * nt) % 8 else 0), lens


def test_fc2_and_proj_are_one_round():
    """8296 rows x 1024 columns on 256 CUs: 52 x 4 = 208 tiles, every block at most one"""
    walks = walk(52, 4, launch_grid(52, 4))
    assert max(len(w) for w in walks) == 1 and sum(len(w) for w in walks) == 208


# ---- piece map ---------------------------------------------------------------------------------------------------------------------------------
def pieces_of(wave):
    """stage pieces q of a wave, in issue order (the kernel's piece_q)"""
    if wave < NW // 2:
        return [wave * (PA - 1) + i for i in range(PA - 1)] + [XP + 4 * PB + wave]
    return [XP + (wave - NW // 2) * PB + i for i in range(PB)]


def piece_rows(q):
    """(operand, plane, first row within the plane, LDS byte offset within the slot) of stage piece q: 16 rows of 64 B"""
    if q < XP:
        return "x", q // (BM // 16), (q % (BM // 16)) * 16, q * 1024
    pc = q - XP
    return "w", pc // (BN // 16), (pc % (BN // 16)) * 16, q * 1024


def test_piece_map_covers_a_stage_exactly_once():
    assert [len(pieces_of(w)) for w in range(NW)] == [PA] * 4 + [PB] * 4
    allq = [q for w in range(NW) for q in pieces_of(w)]
    assert sorted(allq) == list(range(XP + WP))
    rows, lds = [], []
    for q in allq:
        op, pl, r0, off = piece_rows(q)
        assert 0 <= off and off + 1024 <= STAGE
        lds.append(off)
        rows += [(op, pl, r0 + r) for r in range(16)]
    assert len(set(lds)) == len(lds)                    # 1-KiB destinations do not overlap
    want = [("x", pl, r) for pl in range(2) for r in range(BM)] + [("w", pl, r) for pl in range(2) for r in range(BN)]
    assert sorted(rows) == sorted(want)
    # the stage row a fragment read addresses = the row the loader wrote: [X h | X l | W h | W l]
    for q in allq:
        op, pl, r0, off = piece_rows(q)
        base = (pl * BM if op == "x" else 2 * BM + pl * BN) + r0
        assert off == base * 64
    assert NS * STAGE == 159744


def test_swizzle_of_a_stage_row_is_the_swizzle_of_its_operand_row():
    """the loader swizzles by the STAGE row (16 q + lane / 4), the fragment reads by the row within the wave tile: equal because every plane and every
    wave tile starts at a multiple of 8 rows"""
    for q in range(XP + WP):
        op, pl, r0, _ = piece_rows(q)
        for r in range(16):
            assert (((q * 16 + r) >> 1) & 3) == (((r0 + r) >> 1) & 3)
    assert BM % 8 == 0 and BN % 8 == 0 and (BM // 2) % 16 == 0 and (BN // 4) % 16 == 0


# ---- schedule ----------------------------------------------------------------------------------------------------------------------------------
def persist160(chunks, nk, wave, log):
    """statement by statement the control flow of one wave of gemm_f16x2_persist160_kernel.  Events: ("issue", chunk, pieces), ("wait", n) = vmcnt(n),
    ("read", chunk), ("mfma", chunk), ("barrier", drains_lds_reads)"""
    P = len(pieces_of(wave))
    st = {"issued": -1, "l_kc": -1, "tile": 0}
    cur = {"c_kc": 0, "epi": False, "l_comp": 0, "e_tile": None}

    def issue():
        st["issued"] += 1
        st["l_kc"] += 1
        if st["l_kc"] == nk:
            st["l_kc"] = 0
            st["tile"] += 1
        log.append(("load", st["issued"], st["tile"], st["l_kc"]))
        return ("issue", st["issued"], P)

    def tile_cursor():
        if cur["epi"]:
            log.append(("store", cur["e_tile"]))
            cur["epi"] = False
        if cur["c_kc"] == nk - 1:
            cur["e_tile"] = cur["l_comp"]
            cur["l_comp"] += 1

    def mfma(g):
        log.append(("mfma", g, cur["l_comp"] - 1 if cur["c_kc"] == nk - 1 else cur["l_comp"]))
        cur["c_kc"] += 1
        if cur["c_kc"] == nk:
            cur["c_kc"] = 0
            cur["epi"] = True
        return ("mfma", g)

    yield issue()
    if chunks > 1:
        yield issue()
        yield ("wait", P)
    else:
        yield ("wait", 0)
    yield ("barrier", True)
    if wave < NW // 2:
        for g in range(chunks):
            tile_cursor()
            if g + 2 < chunks:
                yield issue()
            yield ("read", g)
            yield ("barrier", True)
            yield mfma(g)
            yield ("wait", P if g + 2 < chunks else 0)
            yield ("barrier", False)
        yield ("barrier", False)
    else:
        yield ("barrier", False)
        for g in range(chunks):
            tile_cursor()
            if g + 2 < chunks:
                yield issue()
            yield ("read", g)
            yield ("wait", P if g + 2 < chunks else 0)
            yield ("barrier", True)
            yield mfma(g)
            yield ("barrier", False)
    assert cur["epi"]
    log.append(("store", cur["e_tile"]))


def simulate160(schedule, chunks):
    """barrier-stepped replay of the eight waves.  R1: a chunk is read only after EVERY wave waited for its own pieces of it in an earlier phase;
    R2: a slot is overwritten only after every wave's reads of its previous chunk were drained (lgkmcnt(0)) before an earlier barrier; W: after a
    counted wait the pieces still in flight are exactly the wave's pieces of ONE chunk, the newest, and everything older has landed"""
    gens = [schedule(w) for w in range(NW)]
    ppw = [len(pieces_of(w)) for w in range(NW)]
    issued = [[] for _ in range(NW)]
    landed = [dict() for _ in range(NW)]
    read_phase = [dict() for _ in range(NW)]
    read_done = [dict() for _ in range(NW)]
    issue_phase = [dict() for _ in range(NW)]
    mfma = [[] for _ in range(NW)]
    nbar = [0] * NW
    alive = [True] * NW
    counted = [0] * NW
    phase = 0
    while any(alive):
        for w in range(NW):
            if not alive[w]:
                continue
            pending = [c for c in read_phase[w] if c not in read_done[w]]
            while True:
                try:
                    ev = next(gens[w])
                except StopIteration:
                    alive[w] = False
                    break
                if ev[0] == "issue":
                    assert ev[2] == ppw[w]
                    issued[w] += [ev[1]] * ev[2]
                    issue_phase[w][ev[1]] = phase
                elif ev[0] == "wait":
                    n = ev[1]
                    assert n in (0, ppw[w]), f"wave {w} counts {n} pieces, it moves {ppw[w]} per chunk"
                    fly = issued[w][len(issued[w]) - n:] if n else []
                    done = issued[w][:len(issued[w]) - n] if n else issued[w]
                    if n:
                        counted[w] += 1
                        newest = issued[w][-1]
                        assert fly == [newest] * ppw[w], f"W: wave {w} leaves {fly} in flight"
                        assert set(done) == set(range(newest)), f"W: wave {w}: chunks landed {sorted(set(done))}, newest {newest}"
                    for c in set(done):
                        assert done.count(c) == ppw[w]
                        landed[w].setdefault(c, phase)
                elif ev[0] == "read":
                    assert ev[1] not in read_phase[w]
                    read_phase[w][ev[1]] = phase
                    pending.append(ev[1])
                elif ev[0] == "mfma":
                    assert ev[1] in read_phase[w]
                    mfma[w].append(ev[1])
                elif ev[0] == "barrier":
                    nbar[w] += 1
                    if ev[1]:
                        for c in pending:
                            read_done[w][c] = phase
                    break
        phase += 1
    assert len(set(nbar)) == 1, nbar
    for w in range(NW):
        assert mfma[w] == list(range(chunks)) and sorted(read_phase[w]) == list(range(chunks))
        assert all(issued[w].count(c) == ppw[w] for c in range(chunks))
        for c, ph in read_phase[w].items():
            for v in range(NW):
                assert c in landed[v] and landed[v][c] < ph, f"R1: wave {w} reads chunk {c} in phase {ph}, wave {v} waited in {landed[v].get(c)}"
        for c, ph in issue_phase[w].items():
            if c >= NS:
                for v in range(NW):
                    assert (c - NS) in read_done[v] and read_done[v][c - NS] < ph, f"R2: wave {w} overwrites chunk {c - NS} in phase {ph}"
    return counted


@pytest.mark.parametrize("chunks", range(1, 10))
def test_ring_is_hazard_free_and_counted_waits_leave_one_chunk_in_flight(chunks):
    counted = simulate160(lambda w: persist160(chunks, chunks, w, []), chunks)
    # one counted wait at the fill (two chunks issued) and one per chunk that still has a successor two ahead
    assert counted == [(1 if chunks > 1 else 0) + max(0, chunks - 2)] * NW


@pytest.mark.parametrize("nk,tiles", [(1, 1), (1, 2), (1, 5), (2, 1), (2, 3), (3, 1), (3, 4), (4, 3), (4, 7), (32, 2), (128, 1), (5, 8)])
def test_tile_switches_keep_the_cursors(nk, tiles):
    """the loader's cursor names tile g // nk, chunk g % nk for stream position g; every chunk is multiplied into the accumulators of its own tile;
    tile t is stored once, after its last chunk's MFMAs and before the first MFMAs of tile t + 1"""
    logs = [[] for _ in range(NW)]
    simulate160(lambda w: persist160(nk * tiles, nk, w, logs[w]), nk * tiles)
    for w in range(NW):
        loads = [r for r in logs[w] if r[0] == "load"]
        assert [(r[1], r[2], r[3]) for r in loads] == [(g, g // nk, g % nk) for g in range(nk * tiles)]
        stored = []
        for r in [r for r in logs[w] if r[0] != "load"]:
            if r[0] == "mfma":
                assert r[2] == r[1] // nk, r
                assert stored == list(range(r[2])), f"wave {w}: chunk {r[1]} of tile {r[2]} multiplied while tiles {stored} are stored"
            else:
                assert r[1] == len(stored)
                stored.append(r[1])
        assert stored == list(range(tiles))


def test_the_model_catches_a_wait_that_counts_the_other_groups_pieces():
    def broken(w):                                       # group A waiting with group B's count: one piece of chunk g+1 may still fly
        for ev in persist160(8, 8, w, []):
            yield ("wait", PB) if (w < NW // 2 and ev == ("wait", PA)) else ev
    with pytest.raises(AssertionError):
        simulate160(broken, 8)


def test_the_model_catches_an_issue_one_phase_early():
    def broken(w):                                       # chunk g+3 issued where g+2 belongs: the slot still holds the chunk being read
        evs = list(persist160(8, 8, w, []))
        out = []
        for ev in evs:
            out.append(("issue", ev[1] + 1, ev[2]) if ev[0] == "issue" and 2 <= ev[1] < 7 else ev)
        yield from out
    with pytest.raises(AssertionError):
        simulate160(broken, 8)


# ---- dispatch rule -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def route(monkeypatch):
    from patchfusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpf_hip.so not built")
    L = _lib.load()
    monkeypatch.delenv("PF_F16_TILE", raising=False)

    def f(M, K, N, out_f32=1, korder=6, cus=256):
        p = _lib.ConvParams()
        p.B, p.OH, p.OW, p.H, p.W, p.Cin, p.Cout, p.batch = 1, 1, M, 1, M, K, N, 1
        p.out_f32, p.korder = out_f32, korder
        return L.pf_gemm_f16x2_route(C.byref(p), cus)
    f.L = L
    return f


SHAPES = [  # (M, K, N, out_f32, korder, route at 256 CUs)
    (8296, 4096, 1024, 1, 6, T160),          # fc2: 264 tiles of 192 (two rounds) against 208 of 160 x 256 (one)
    (8296, 1024, 1024, 1, 6, T160),          # proj
    (8296, 1024, 3072, 1, 6, P192),          # qkv's shape with float32 out: 704 / 624 tiles, three rounds either way x 1.11
    (8296, 1024, 4096, 1, 6, P192),          # fc1's shape: 968 / 832 tiles, four rounds either way
    (8296, 1024, 3072, 0, 6 | 32, P192),     # qkv as it runs: fp16 row-major planes out
    (8296, 1024, 3072, 0, 6, P192),          # qkv, three bf16 planes out
    (8296, 1024, 4096, 0, 6 | 16, P192),     # fc1 as it runs: fp16 chunk-major planes out
    (1037, 4096, 1024, 1, 6, P192),          # the coarse branch's single image: one round either way
    (1037, 1024, 1024, 1, 6, P192),
    (1037, 1024, 3072, 1, 6, P192),
]


@pytest.mark.parametrize("M,K,N,out_f32,korder,want", SHAPES)
def test_route_table_at_256_cus(route, monkeypatch, M, K, N, out_f32, korder, want):
    assert route(M, K, N, out_f32, korder) == want
    monkeypatch.setenv("PF_F16_TILE", "0")
    assert route(M, K, N, out_f32, korder) == P192
    monkeypatch.setenv("PF_F16_TILE", "1")
    assert route(M, K, N, out_f32, korder) == (T160 if out_f32 and not (korder & 48) else P192)


def test_route_follows_the_cost_model(route):
    for cus in (8, 64, 128, 256, 304):
        for M in (1, 160, 1037, 4148, 8296, 16592):
            for N in (256, 260, 512, 1024, 3072, 4096):
                t192 = -(-M // 192) * -(-N // 192)
                t160 = -(-M // 160) * -(-N // 256)
                want = T160 if -(-t160 // cus) * 60 < -(-t192 // cus) * 54 else P192
                assert route(M, 1024, N, cus=cus) == want, (cus, M, N)
    assert route.L.pf_gemm_f16x2_route(None, 256) == -1
    p_cus0 = route(8296, 1024, 1024, cus=0)
    assert p_cus0 == -1
