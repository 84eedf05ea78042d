"""The cases of tests/dc_shapes.py, checked without a GPU: each reaches the levels of the DC scans it is named after (by the launch arithmetic
restated from csrc/dc.hip and csrc/packed.hip, whose constants the helper reads out of the sources), its carrier symbols sit in the tiles
they were meant for, and the oracle alone round-trips it.  tests/test_gpu_dc_levels.py hands the same arrays to the kernels."""
import numpy as np
import pytest

import dc_shapes as S

SINGLE_IDS = S.single_case_ids()
KIB = 1 << 10


def test_constants_are_the_sources():
    assert S.DC_TILE > 0 and S.DC_WAVES == 4 and S.DC_MAX_CHUNKS > 0 and S.DC_CARRY_BATCH > 0
    assert S.PK_TILE > 0 and S.PDC_TILE > 0 and S.PDC_MAX_CHUNKS > 0 and S.PDC_STEP == 64
    # the walk: tile 0 is the END of L, the last (ragged) tile its head
    n = 3 * S.DC_TILE + 5
    assert S.walk_tile(n, n - 1) == 0 and S.walk_tile(n, 0) == 3 and S.walk_tile_range(n, 3) == (0, 5) and S.walk_tile_range(n, 0) == (n - S.DC_TILE, n)
    for t in range(4):
        lo, hi = S.walk_tile_range(n, t)
        assert S.walk_tile(n, lo) == t and S.walk_tile(n, hi - 1) == t


def single_levels_missing():
    """names of the levels the issue's list of shapes no longer reaches (empty while the constants are what the shapes were chosen for)"""
    lvs = [S.single_levels(tiles * S.DC_TILE + r) for _, tiles, r in SINGLE_IDS]
    tpcs = {lv["tpc"] for lv in lvs}
    missing = ["tpc = %d" % t for t in (1, 2, 3, 9) if t not in tpcs]
    checks = {
        "a partial batch inside a chunk (k_dc_carry_a / _c: tpc > DC_CARRY_BATCH, not a multiple of it)": any(lv["partial_batch"] for lv in lvs),
        "more than one tile per chunk (tpc > 1)": any(lv["tpc"] > 1 for lv in lvs),
        "a short last chunk": any(lv["tpc"] > 1 and lv["last_chunk_tiles"] < lv["tpc"] for lv in lvs),
        "a short last chunk behind chunks of more than one batch": any(lv["partial_batch"] and lv["last_chunk_tiles"] < lv["tpc"] for lv in lvs),
        "an uneven fourth quarter (k_dc_carry_b)": any(0 < lv["quarter_lens"][3] < lv["per_q"] for lv in lvs),
        "quarters of more than one batch (k_dc_carry_b)": any(lv["per_q"] > S.DC_CARRY_BATCH for lv in lvs),
        "a quarter whose last batch is partial (k_dc_carry_b)": any(lv["per_q"] > S.DC_CARRY_BATCH and q % S.DC_CARRY_BATCH for lv in lvs for q in lv["quarter_lens"]),
        "runscan threads with 2 tiles": any(lv["rs_per"] == 2 for lv in lvs),
        "runscan threads with 5 or more tiles": any(lv["rs_per"] >= 5 for lv in lvs),
    }
    for k in (1, 2, 3, 5):
        checks["nchunks = %d (empty quarters)" % k] = any(lv["nchunks"] == k and 0 in lv["quarter_lens"] for lv in lvs if k < 4) or \
            any(lv["nchunks"] == k for lv in lvs if k >= 4)
    for k in (2, 3, 5):
        checks["nchunks = %d" % k] = any(lv["nchunks"] == k for lv in lvs)
    missing += [name for name, ok in checks.items() if not ok]
    return missing


def test_single_levels_reached():
    missing = single_levels_missing()
    assert not missing, "the single-block shapes no longer reach: " + "; ".join(missing)


def test_single_case_list_is_the_issues():
    ids = set(SINGLE_IDS)
    assert {t for _, t, _ in ids} == {1, 2, 3, 5, 511, 512, 1024, 4096} and {r for _, _, r in ids} == {0, 1, 4095}
    for tiles in (1, 2, 3, 5, 511, 512, 1024):
        for r in (0, 1, 4095):
            for b in ("sparse_alt", "sparse_runs", "whole_runs"):
                assert (b, tiles, r) in ids
    assert {(b, r) for b, t, r in ids if t == 4096} == {("sparse_alt", 1), ("sparse_runs", 1), ("whole_runs", 1)}
    assert {(t, r) for b, t, r in ids if b == "random256"} == {(t, r) for t in (512, 1024) for r in (0, 1, 4095)}


def roundtrip(orc, L):
    enc = orc.dc_encode(L)
    m = len(enc["d"])
    assert m == len(S.run_starts(L)), "the oracle's m is not the number of runs"
    back, used = orc.dc_decode(enc["init"], enc["d"], len(L))
    assert used == S.expected_used(L, m) and np.array_equal(back, L), "the oracle alone does not round-trip this array"
    return enc


@pytest.mark.parametrize("builder,tiles,r", SINGLE_IDS, ids=["%s-%d+%d" % i for i in SINGLE_IDS])
def test_single_case(orc, builder, tiles, r):
    c = S.single_case(builder, tiles, r)
    L, n, lv = c["L"], c["n"], c["levels"]
    assert L.dtype == np.uint8 and len(L) == n == tiles * S.DC_TILE + r and lv["ntiles"] == tiles + (r > 0)
    assert lv["last_tile_len"] == (r or S.DC_TILE)
    again = S.single_case(builder, tiles, r)
    assert np.array_equal(again["L"], L), "the builder is not deterministic"
    if builder.startswith("sparse"):
        bg = np.isin(L, S.BG)
        if builder == "sparse_alt":
            assert len(S.run_starts(L)) == n, "strictly alternating: every position is a run"
        else:
            st = S.run_starts(np.where(bg, L, 0))
            lens = np.diff(np.concatenate([st, [n]]))
            assert lens.max() <= 5 and np.count_nonzero(lens >= 3) > len(lens) // 2
        assert len({k["sym"] for k in c["carriers"]}) == len(c["carriers"]) and np.count_nonzero(~bg) == sum(len(k["pos"]) for k in c["carriers"])
        kinds = set()
        for k in c["carriers"]:
            hits = np.flatnonzero(L == k["sym"])
            assert tuple(sorted(hits.tolist())) == tuple(sorted(k["pos"])), k
            assert sorted(S.walk_tile(n, int(p)) for p in hits) == sorted(k["tiles"]), "carrier %r is not in its tiles" % (k,)
            if len(k["tiles"]) == 2 and k["tiles"][0] != k["tiles"][1]:
                got = S.crossing_kinds(lv, *k["tiles"])
                assert k["kind"] == "filler" or k["kind"] in got, "carrier %r does not cross what it is named after (%s)" % (k, sorted(got))
                kinds |= got
        missing = S.expected_kinds(lv) - kinds
        assert not missing, "no carrier crosses: %s" % sorted(missing)
        names = [k["kind"] for k in c["carriers"]]
        assert "once" in names and c["carriers"][0]["sym"] == 0xFF
        if lv["ntiles"] >= 3:
            assert len([k for k in c["carriers"] if len(k["tiles"]) == 2]) >= S.MIN_CARRIERS
        if r != 1:
            assert c["ragged_only"] and "last_tile_only" in names   # (r = 1: the one position of the ragged tile takes the whole-array carrier)
    elif builder == "whole_runs":
        R = L[::-1]
        starts = np.zeros(n, bool)
        starts[S.run_starts(R)] = True
        per_tile = np.add.reduceat(starts, np.arange(0, n, S.DC_TILE))
        assert (lv["ntiles"] >= 2) == bool(c["stretches"])
        ends = set()
        for s in c["stretches"]:
            a, b = s["first"], s["first"] + s["tiles"]
            assert not per_tile[a:b].any(), "stretch %r holds a run start" % (s,)
            assert per_tile[a - 1] > 0 and (R[a * S.DC_TILE:min(n, b * S.DC_TILE)] == s["byte"]).all()
            assert s["tiles"] <= 20 and (s["tiles"] >= 3 or lv["ntiles"] < 5)
            ends |= {a, b}
        if lv["nchunks"] >= 8:
            assert any(e % lv["tpc"] == 0 for e in ends), "no stretch ends at a chunk edge"
            assert np.count_nonzero(per_tile > 64) > lv["ntiles"] // 2, "the stretches are meant to lie between busy tiles"
        if lv["tpc"] > S.DC_CARRY_BATCH:
            assert any(e % lv["tpc"] == S.DC_CARRY_BATCH for e in ends), "no stretch ends at a batch edge inside a chunk"
    else:
        assert len(np.unique(L)) == 256 and lv["tpc"] in (1, 2, 3)
    roundtrip(orc, L)


# ---- packs ----
def pack_levels_missing(cases):
    lvs = [c["levels"] for c in cases.values()]
    checks = {"tpc = 1": any(lv["tpc"] == 1 for lv in lvs), "tpc = 2": any(lv["tpc"] == 2 for lv in lvs), "tpc = 5": any(lv["tpc"] == 5 for lv in lvs),
              "nchunks = 1 below a tpc above 1 (mtiles < tpc)": any(lv["nchunks"] == 1 and lv["mtiles"] < lv["tpc"] for lv in lvs),
              "every chunk of the launch in use at tpc > 1, the last one short": any(lv["full"] and lv["tpc"] > 1 and lv["last_chunk_tiles"] < lv["tpc"] for lv in lvs),
              "nchunks = PDC_MAX_CHUNKS": any(lv["nchunks"] == S.PDC_MAX_CHUNKS for lv in lvs),
              "two iterations of k_pk_scan_u32": any(lv["scan_iters"] == 2 for lv in lvs)}
    return [name for name, ok in checks.items() if not ok]


@pytest.fixture(scope="module")
def packs():
    return {name: make() for name, make in S.PACKS.items()}


def test_pack_levels_reached(packs):
    missing = pack_levels_missing(packs)
    assert not missing, "the packs no longer reach: " + "; ".join(missing)
    lv = packs["1m+1_all_runs"]["levels"]
    assert (lv["tpc"], lv["nchunks"], lv["last_chunk_tiles"]) == (2, S.PDC_MAX_CHUNKS // 2 + 1, 1)
    lv = packs["4m+tile+1"]["levels"]
    assert lv["total"] == (4 << 20) + 4097 and lv["tpc"] == 5 and lv["scan_iters"] == 2


def pack_run_starts(c):
    flat = np.concatenate(c["blocks"])
    starts = np.concatenate([[True], flat[1:] != flat[:-1]])
    starts[np.cumsum([len(b) for b in c["blocks"]])[:-1]] = True
    return flat, starts


@pytest.mark.parametrize("name", list(S.PACKS))
def test_pack_case(orc, packs, name):
    c = packs[name]
    blocks, lv, rb, ms = c["blocks"], c["levels"], c["rb"], c["ms"]
    sizes = np.array([len(b) for b in blocks])
    assert sizes.min() >= 1 and sizes.max() <= 16 << 20 and lv["total"] <= 12 << 20
    flat, starts = pack_run_starts(c)
    assert int(starts.sum()) == lv["m"] == int(rb[-1])
    T = S.PDC_TILE
    if name == "tiny":
        assert len(blocks) >= 2000 and sizes.max() <= 3 and set(sizes.tolist()) == {1, 2, 3}
        assert lv["mtiles"] >= 2 and np.count_nonzero(rb[:-1] < T) > 1000, "one tile of runs is meant to span many blocks"
        heads_in_first_step = np.count_nonzero(rb[:-1] < S.PDC_STEP)
        assert heads_in_first_step > 16, "one step of 64 runs is meant to span many blocks"
        a, b = c["same_byte"]
        assert b - a >= 100 and all(len(set(x.tolist())) == 1 and x[0] == blocks[a][0] for x in blocks[a:b]) and all(ms[i] == 1 for i in range(a, b))
    elif name == "prev_tail":
        for i in range(1, len(blocks)):
            prev, cur = blocks[i - 1], blocks[i]
            k = len(set(prev.tolist()))
            tail_runs = prev[S.run_starts(prev)][-k:]
            assert len(set(tail_runs.tolist())) == k, "block %d does not end in one run of each of its symbols" % (i - 1)
            assert set(cur.tolist()) <= set(tail_runs.tolist()), "a symbol of block %d did not occur in the block before" % i
        assert {len(set(b.tolist())) for b in blocks} >= {1, 2, 5, 12, 64, 256}
    elif name == "heads":
        assert lv["m"] == lv["total"]
        res = {int(x) % T for x in rb[:-1]}
        assert res >= {0, 1, S.PDC_STEP - 1, S.PDC_STEP, T - 1}, sorted(res)
        assert any(int(rb[i + 1]) % T == 0 and int(rb[i]) % T != 0 for i in range(len(blocks)))
        assert any(ms[i] > 2 * T and int(rb[i]) % T != 0 and (int(rb[i + 1]) - 1) // T - int(rb[i]) // T >= 2 for i in range(len(blocks)))
    elif name == "all256":
        full = [i for i, b in enumerate(blocks) if len(set(b.tolist())) == 256]
        assert len(full) >= 4
        for i in c["ff_last"]:
            assert i in full and blocks[i][-1] == 0xFF and ms[i] >= 256
        assert set(blocks[c["ff_only"]].tolist()) == {0xFF}
        assert any(ms[i] > 2 * 256 for i in full), "a permutation repeated: most runs have a previous occurrence"
    elif name in ("1m+1_all_runs", "1m_all_runs"):
        assert lv["m"] == lv["total"] and lv["full"] and sizes.min() >= 2 * KIB and sizes.max() <= 300 * KIB and len(blocks) >= 5
        assert lv["tpc"] == (2 if name == "1m+1_all_runs" else 1)
        x = c["cross_block"]
        assert (blocks[x["block"] - 1] == x["sym"]).any() and (blocks[x["block"]] == x["sym"]).any()
    elif name == "1m+1_long_runs":
        assert lv["total"] == packs["1m+1_all_runs"]["levels"]["total"] and lv["mtiles"] < lv["tpc"] and lv["nchunks"] == 1
    elif name == "4m+tile+1":
        assert sizes.max() >= 1 << 20
        per_tile = np.add.reduceat(starts, np.arange(0, lv["total"], S.PK_TILE))
        seam = c["seam_tile"]
        assert seam == S.PK_SCAN_THREADS and lv["ptiles"] > seam
        for a, b in c["empty_position_tiles"]:
            assert not per_tile[a:b + 1].any() and per_tile[a - 1] > 0, (a, b)
        assert any(b == seam - 1 for a, b in c["empty_position_tiles"]) and not starts[seam * S.PK_TILE] and 0 < per_tile[seam] < 64
        big = int(np.argmax(ms))
        assert ms[big] >= 1 << 20 and (int(rb[big + 1]) - int(rb[big])) // (T * lv["tpc"]) >= 50, "a block is meant to span many chunks"
    kinds = set()
    for k in c["carriers"]:
        off = int(sizes[:k["block"]].sum())
        hits = np.flatnonzero(blocks[k["block"]] == k["sym"]) + off
        assert tuple(hits.tolist()) == tuple(sorted(k["pos"])) and len(hits) == 2, k
        runs = np.cumsum(starts)[hits] - 1
        assert tuple(int(r) // T for r in runs) == k["tiles"], "carrier %r is not in its tiles of runs" % (k,)
        ca, cb = (t // lv["tpc"] for t in k["tiles"])
        if k["kind"] == "chunk_edge":
            assert cb == ca + 1 and k["tiles"][1] == k["tiles"][0] + 1
        elif k["kind"].startswith("odd_chunk"):
            assert ca % 2 == 1 and cb > ca
        kinds.add(k["kind"])
    if c["carriers"]:
        assert kinds == {"chunk_edge", "odd_chunk_to_later", "odd_chunk_to_next", "many_chunks"}
    for i, b in enumerate(blocks):
        enc = roundtrip(orc, b)
        assert len(enc["d"]) == ms[i]


def test_compact_texts():
    texts = S.compact_texts()
    sizes = sorted(len(t) for t in texts)
    assert len(texts) == 3002 and sizes[-2:] == [70000, 70000] and sizes[0] == 1 and sizes[-3] <= 40
    assert any((t == 0xFF).any() and len(set(t.tolist())) > 1 for t in texts) and any(set(t.tolist()) == {0xFF} for t in texts)
    seen, repeats = set(), 0
    for t in texts:
        repeats += t.tobytes() in seen and len(t) > 8
        seen.add(t.tobytes())
    assert repeats > 50 and len(np.unique(np.concatenate(texts))) <= 8
