"""The cases of tests/scan_levels.py, checked without a GPU: the constants its arithmetic mirrors are the sources', every case reaches the level
of its scan that it is named after, every case is SENSITIVE -- the plain model with one fault put into its scan (the carry between passes
dropped, the chunk bases zero, a short last chunk run in full, a 64-bit sum kept in 32 bits, per taken as 1) gives another answer than the model
without -- and the quick models equal the plain ones of the other test modules on small inputs of the same construction.
tests/test_gpu_scan_levels.py hands the same cases to the kernels."""
import re

import numpy as np
import pytest

import scan_levels as S
from fm_find_model import block_structures, find_model
from fm_locate_model import locate_structure, sa_plain
from fm_near_model import exact_classes, near_model
from fm_seams_model import seams_model
from lcp_model import lcp_kasai
from sa_match_model import smem_records

_sa = {}


def sa_of(orc, key, text):
    """the oracle's suffix array of a case's text, computed once"""
    if key not in _sa:
        _sa[key] = np.asarray(orc.sa_sais(text) if len(text) > 1 else [0], dtype=np.int64)  # (the oracle's SA-IS takes no text of one byte)
    return _sa[key]


# ---- 1. the constants ----------------------------------------------------------------------------------------------------------------------------------

def test_constants_are_the_sources():
    c = S.read_constants()
    assert c == dict(LCP_TILE=S.LCP_TILE, FM_BLOCK=S.FM_BLOCK, FM_MAX_CHUNKS=S.FM_MAX_CHUNKS, FM_FIND_ROW=S.FM_FIND_ROW, IB_TILE=S.IB_TILE,
                     IB_MAX_CHUNKS=S.IB_MAX_CHUNKS, SM_TILE=S.SM_TILE)
    lcp, bwt, saq, fmi = S._source("lcp.hip"), S._source("bwt.hip"), S._source("sa_query.hip"), S._source("fm_index.hip")
    # the one-workgroup spines: their width is in the launch, the launch bounds and the loop
    assert S.SPINE == 1024
    assert "k_lcp_spine<<<dim3(1), dim3(1024), 0, st>>>(agg, ntiles)" in lcp
    assert re.search(r"__launch_bounds__\(1024\) void k_lcp_spine\(", lcp) and "for (uint32_t base = 0; base < ntiles; base += 1024)" in lcp
    assert "k_loc_scan<<<dim3(1), dim3(1024), 0, st>>>(lc.marks, R)" in bwt
    assert re.search(r"__launch_bounds__\(1024\) void k_loc_scan\(", bwt) and "per = (rows + 1023u) / 1024u, r0 = min(threadIdx.x * per, rows)" in bwt
    # a locate row: 32 words of 32 slots, and the structure's carve
    assert S.LOC_ROW == 32 * 32 and "c += __popc(bits[32 * static_cast<size_t>(r) + k])" in bwt and "for (int k = 0; k < 32; ++k)" in bwt
    with open(S.os.path.join(S.ROOT, "dark_amd", "csrc", "context.hpp")) as f:
        assert "const size_t rows = div_up(total, 1024);\n    return FmLocate{" in f.read()
    # the SMEM scan's trips
    assert S.SM_TRIP == 256 and "for (uint32_t c = 0; c < ntiles; c += 256u)" in saq and "k_sa_smem_scan_b<<<dim3(1), dim3(256), 0, st>>>" in saq
    # the drivers' arithmetic, as restated in fm_levels, find_levels and ibwt_levels
    assert "const size_t rows = ix.rows, rpc = div_up(rows, FM_MAX_CHUNKS), nchunks = div_up(rows, rpc);" in fmi
    # (find, near and seams share fm_pairs: one place, and none of the three keeps arithmetic of its own)
    assert fmi.count("rows = div_up(npairs, FM_FIND_ROW), rpc = div_up(rows, FM_MAX_CHUNKS), nchunks = div_up(rows, rpc);") == 1
    assert fmi.count("const FmPairs g = fm_pairs(") == 3 and fmi.count("div_up(npairs, FM_FIND_ROW)") == 1
    assert "const size_t ntiles = div_up(total, IB_TILE), tpc = div_up(ntiles, IB_MAX_CHUNKS), nchunks = div_up(ntiles, tpc);" in bwt
    assert "const uint32_t stride = (phi - plo + 63u) >> 6" in fmi


def test_level_arithmetic_at_the_borders():
    assert S.lcp_levels(S.LCP_BORDER)["passes"] == 1 and S.lcp_levels(S.LCP_BORDER + 1) == dict(ntiles=1025, passes=2, last_pass_tiles=1)
    assert S.fm_levels(255 * 1024) == dict(rows=256, rpc=1, nchunks=256, last_chunk_rows=1)
    assert S.fm_levels((1 << 18) + 77) == dict(rows=258, rpc=2, nchunks=129, last_chunk_rows=2)  # what the suite reached before: full chunks
    assert S.fm_levels(1 << 20) == dict(rows=1025, rpc=5, nchunks=205, last_chunk_rows=5)
    assert S.find_levels(65536)["rpc"] == 1 and S.find_levels(65537)["rpc"] == 2
    assert [S.find_levels(n)["search_rounds"] for n in (1, 2, 64, 65, 4096, 4097, 262144, 262145)] == [0, 1, 1, 2, 2, 3, 3, 4]
    assert S.loc_levels(1 << 20)["per"] == 1 and S.loc_levels((1 << 20) + 1)["per"] == 2
    assert S.ibwt_levels(1 << 20)["tpc"] == 1 and S.ibwt_levels((1 << 20) + 1)["tpc"] == 2
    assert S.smem_levels(262144)["trips"] == 1 and S.smem_levels(262145)["trips"] == 2


# ---- A. the LCP spine ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", S.LCP_SINGLE)
def test_lcp_case(orc, name):
    t = S.lcp_text(name)
    n = len(t)
    lv = S.lcp_levels(n)
    sa = sa_of(orc, name, t)
    lcp = S.lcp_fast(t, sa)
    assert np.array_equal(S.lcp_by_scan([t], [sa], [lcp])[0], lcp), "the model of the scan is not the definition"
    broken = S.lcp_by_scan([t], [sa], [lcp], "second_from_zero")[0]
    rank = np.empty(n, np.int64)
    rank[sa] = np.arange(n)
    if name == "a1_straddle":
        assert n == S.A1_N and lv == dict(ntiles=1027, passes=2, last_pass_tiles=3)
        assert S.A1_START2 <= S.LCP_BORDER - 2 * S.LCP_TILE and S.A1_START2 + S.A1_PLANT >= S.LCP_BORDER + 2 * S.LCP_TILE
        inside = np.arange(S.A1_START2 + 1, S.A1_START2 + S.A1_PLANT)
        want = S.A1_PLANT - (inside - S.A1_START2)
        assert lcp[rank[S.A1_START2]] == S.A1_PLANT and np.array_equal(lcp[rank[inside]], want), "the second copy is not one falling chain"
        # every position of tiles 1024 and 1025 lies in the chain: no measured position there, the values come through the carry
        wrong = np.flatnonzero(broken != lcp)
        hit = np.sort(sa[wrong])
        assert hit[0] == S.LCP_BORDER and hit[-1] == S.A1_START2 + S.A1_PLANT - 1 and len(hit) == hit[-1] - hit[0] + 1
        assert len(hit) > 2 * S.LCP_TILE
    elif name == "a2_exact":
        assert n == S.LCP_BORDER and lv["passes"] == 1 and lcp.max() == 2000
        assert np.array_equal(broken, lcp)  # one pass: there is no carry to drop
    elif name == "a2_plus1":
        assert n == S.LCP_BORDER + 1 and lv == dict(ntiles=1025, passes=2, last_pass_tiles=1)
        assert lcp[rank[n - 1]] == 0  # a text's last position has no common prefix with the suffix in front (see scan_levels.lcp_text) ...
        assert np.array_equal(broken, lcp)  # ... so nothing in this text can depend on the carry; the case is there for its shape
    else:
        assert n == S.LCP_BORDER + 2 and lv == dict(ntiles=1025, passes=2, last_pass_tiles=1)
        assert lcp[rank[n - 3]] == 2 and lcp[rank[n - 2]] == 1 and t[n - 4] != t[4999]
        assert sa[rank[n - 2] - 1] == 5001, "position n - 2 is not reducible"
        assert sa[np.flatnonzero(broken != lcp)].tolist() == [S.LCP_BORDER] and broken[rank[n - 2]] == 0


def test_lcp_pack(orc):
    blocks = S.lcp_pack()
    sizes = [len(b) for b in blocks]
    off = np.concatenate([[0], np.cumsum(sizes)])
    assert tuple(sizes) == S.A3_SIZES and S.lcp_levels(sum(sizes))["passes"] == 2
    assert S.LCP_BORDER < off[1] < S.LCP_BORDER + S.LCP_TILE, "block 1 does not begin inside tile 1024"
    sas = [sa_of(orc, ("a3", k), b) for k, b in enumerate(blocks)]
    lcps = [S.lcp_fast(b, s) for b, s in zip(blocks, sas)]
    assert lcps[0].max() == 1500 and lcps[1].max() == 2500
    assert all(np.array_equal(g, w) for g, w in zip(S.lcp_by_scan(blocks, sas, lcps), lcps))
    broken = S.lcp_by_scan(blocks, sas, lcps, "second_from_zero")
    hit = np.sort(sas[0][np.flatnonzero(broken[0] != lcps[0])])
    assert hit[0] == S.LCP_BORDER and hit[-1] == S.LCP_BORDER - 700 + 1500 - 1 and len(hit) == 800  # block 0's plant behind the border
    for k in (1, 2, 3):  # a block's head is measured: nothing of the blocks behind reads the carry
        assert np.array_equal(broken[k], lcps[k])


def test_lcp_fast_is_kasai():
    rng = np.random.default_rng(3)
    texts = [S.planted_at(3000, 1500, 700, seed=1, start1=200), S.planted_at(400, 300, 40, seed=2, start1=5), rng.integers(0, 2, size=500, dtype=np.uint8),
             np.full(300, 7, np.uint8), np.tile(rng.integers(0, 250, size=90, dtype=np.uint8), 9), rng.integers(0, 250, size=1, dtype=np.uint8)]
    for t in texts:
        sa = np.array(sa_plain(t), dtype=np.int64)
        want = lcp_kasai(t, sa)
        assert np.array_equal(S.lcp_fast(t, sa), want)
        assert np.array_equal(S.lcp_by_scan([t], [sa], [want])[0], want)
    sas = [np.array(sa_plain(t), dtype=np.int64) for t in texts]
    lcps = [lcp_kasai(t, s) for t, s in zip(texts, sas)]
    assert all(np.array_equal(g, w) for g, w in zip(S.lcp_by_scan(texts, sas, lcps), lcps))


# ---- B. the FM build's scan ------------------------------------------------------------------------------------------------------------------------------

FM_WANT = {"rows256": dict(rows=256, rpc=1, nchunks=256, last_chunk_rows=1), "rows257": dict(rows=257, rpc=2, nchunks=129, last_chunk_rows=1),
           "rows259": dict(rows=259, rpc=2, nchunks=130, last_chunk_rows=1), "rows514": dict(rows=514, rpc=3, nchunks=172, last_chunk_rows=1),
           "rows768": dict(rows=768, rpc=3, nchunks=256, last_chunk_rows=3)}


@pytest.mark.parametrize("name", sorted(S.FM_TOTALS))
def test_fm_case(name):
    total = S.FM_TOTALS[name]
    lv = S.fm_levels(total)
    assert lv == FM_WANT[name]
    L = S.fm_bytes(total)
    assert len(np.unique(L)) == 256
    cp = S.fm_checkpoints(L)
    assert cp.shape == (lv["rows"], 256) and np.array_equal(cp[-1].astype(np.int64), np.bincount(L, minlength=256))
    for r in (1, 2, lv["rows"] // 2):  # prefix counts, literally
        assert np.array_equal(cp[r], np.bincount(L[:r * S.FM_BLOCK], minlength=256))
    good = S.fm_checkpoints_by_scan(L)
    assert np.array_equal(good[:lv["rows"]], cp) and (good[lv["rows"]:] == S.POISON).all()
    faults = ["bases_zero"] + (["full_last_chunk"] if lv["last_chunk_rows"] < lv["rpc"] else [])
    for fault in faults:
        bad = S.fm_checkpoints_by_scan(L, fault)
        assert not np.array_equal(bad, good), "%s leaves %s unchanged" % (fault, name)
        if fault == "bases_zero":
            assert np.array_equal(bad[:lv["rpc"]], good[:lv["rpc"]]) and (bad[lv["rpc"]:lv["rows"]] != good[lv["rpc"]:lv["rows"]]).any(axis=1).all()


def test_fm_pack_heads_lie_behind_chunk_0():
    sizes = S.fm_pack_sizes()
    lv = S.fm_levels(sum(sizes))
    assert sum(sizes) == S.FM_TOTALS["rows514"] and lv["rpc"] == 3 and min(sizes) > 0
    heads = np.cumsum(sizes)[:-1]
    chunks = heads // S.FM_BLOCK // lv["rpc"]
    assert (chunks >= 1).all() and len(set(chunks.tolist())) >= 3 and (heads % S.FM_BLOCK != 0).all()


def test_chunk_scan_on_small_tables():
    rng = np.random.default_rng(4)
    for rows in (1, 2, 5, 6, 7, 11):
        v = rng.integers(0, 100, size=(rows, 3))
        got = S.chunk_scan(v, 3)
        assert np.array_equal(got[:rows], np.cumsum(v, axis=0) - v)


# ---- C. the find family's scans ------------------------------------------------------------------------------------------------------------------------------

FIND_WANT = {"c1_full_list": dict(rows=259, rpc=2, nchunks=130, last_chunk_rows=1, last_row_pairs=3, search_rounds=3),
             "c2_64bit": dict(rows=274, rpc=2, nchunks=137, last_chunk_rows=2, last_row_pairs=112, search_rounds=3),
             "c3_fourth_round": dict(rows=1026, rpc=5, nchunks=206, last_chunk_rows=1, last_row_pairs=44, search_rounds=4)}


@pytest.mark.parametrize("name", S.FIND_CASES)
def test_find_case(name):
    c = S.find_case(name)
    lv = S.find_levels(c["npairs"])
    assert lv == FIND_WANT[name] and len(c["distinct"]) <= 64 and set(c["faults"]) <= set(S.FAULTS)
    occ, lo, recs, total = S.find_fast(c["sas"], c["Ls"], c["origins"], c["distinct"], c["which"], c["max_hits"])
    max_hits = c["max_hits"] or total + 1
    got, got_total, rounds = S.find_by_scan(occ, lo, c["sas"], max_hits)
    assert got_total == total and np.array_equal(got, recs) and rounds == lv["search_rounds"]
    if name == "c1_full_list":
        assert occ.shape == (22017, 3) and b"" in c["distinct"] and (occ[-1] > 0).all() and len(recs) == total < 1 << 20
        assert (occ.sum(axis=1) == 0).any() and (occ == np.array(S.C1_TEXT_SIZES)[None, :]).all(axis=1).sum() == 20
    elif name == "c2_64bit":
        assert occ.shape == (70000, 1) and (occ[:, 0] == 1 << 17).sum() == 40000 and total > 5.2e9 and total >= 1 << 32 and len(recs) == 4096
        assert (recs["pattern"] == 1).all() and np.array_equal(recs["slot"], np.arange(4096))  # pattern 0 is absent, pattern 1 the byte
    else:
        assert occ.shape[0] > 262144 and all(len(p) == 1 for p in c["distinct"]) and 0 < total < 1 << 20 and len(recs) == total
    for fault in c["faults"]:
        bad, bad_total, _ = S.find_by_scan(occ, lo, c["sas"], max_hits, fault)
        assert bad_total != total or len(bad) != len(recs) or (bad != recs).any(), "%s leaves %s unchanged" % (fault, name)
        if fault in ("full_last_chunk", "sum32"):
            assert bad_total != total
        else:
            assert len(bad) == len(recs) and (bad != recs).any()  # the total is right, the list is not
    if name != "c2_64bit":  # (a total below 2^32 is the same in 32 bits: only c2 can tell)
        assert S.find_by_scan(occ, lo, c["sas"], max_hits, "sum32")[1] == total


def test_near_and_seams_cases():
    """C4 is C1's grid through near (k = 0, one-bit classes), once more with a node limit; C5 the seams' grid"""
    c = S.find_case("c1_full_list")
    texts = S.c1_texts()
    assert all(np.array_equal(block_structures(t)[1], L) for t, L in zip(texts, c["Ls"]))
    f_occ, _, f_recs, f_total = S.find_fast(c["sas"], c["Ls"], c["origins"], c["distinct"], c["which"])
    occ, recs, total, cut, nodes = S.near_fast(texts, c["distinct"], c["which"], 0)
    assert total == f_total and cut == 0 and np.array_equal(occ, f_occ) and not recs["cost"].any()
    assert all(np.array_equal(recs[k], f_recs[k]) for k in ("pattern", "block", "position"))
    occ, recs, total, cut, nodes = S.near_fast(texts, c["distinct"], c["which"], 0, S.NEAR_NODE_LIMIT)
    flags = (nodes.reshape(-1) > S.NEAR_NODE_LIMIT).astype(np.int64)
    rpc_pairs = S.find_levels(len(flags))["rpc"] * S.FM_FIND_ROW
    assert cut == flags.sum() and flags[rpc_pairs:].sum() > 1000 and 0 < total < f_total
    assert S.find_scan(flags)[1] == cut and S.find_scan(flags, "full_last_chunk")[1] != cut
    good = S.list_by_scan(occ)
    for fault in ("bases_zero", "full_last_chunk"):
        bad = S.list_by_scan(occ, fault)
        assert bad[2] != good[2] or len(bad[0]) != len(good[0]) or (bad[0] != good[0]).any() or (bad[1] != good[1]).any(), fault
    s = S.seams_case()
    lv = S.find_levels(s["npairs"])
    assert s["npairs"] > 65536 and lv["rpc"] == 2 and lv["last_chunk_rows"] == 1 and len(s["distinct"]) == 64
    occ, recs, total = S.seams_fast(s["blocks"], s["prev"], s["distinct"], s["which"])
    assert total == len(recs) > 1000 and occ[-1].sum() > 0 and (occ.reshape(-1)[rpc_pairs:] > 0).sum() > 1000
    good = S.list_by_scan(occ)
    assert good[2] == total and (good[0] >= 0).all()
    for fault in s["faults"]:
        bad = S.list_by_scan(occ, fault)
        assert bad[2] != good[2] or len(bad[0]) != len(good[0]) or (bad[0] != good[0]).any() or (bad[1] != good[1]).any(), fault


def test_find_fast_is_find_model():
    rng = np.random.default_rng(6)
    texts = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n)) for n in (60, 1, 45)] + [b"AAAAAAA"]
    distinct = [b"", b"A", b"AC", b"GT", b"N", b"AAA", b"CG" * 40, texts[0][10:14], texts[0][-2:] + texts[1], b"C" + texts[0][:2]]
    which = rng.integers(0, len(distinct), size=70)
    pats = [distinct[k] for k in which]
    parts = [block_structures(t) for t in texts]
    sas, Ls, origins = [p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts]
    w_occ, w_recs, w_total = find_model(texts, pats)
    for max_hits in (None, 0, 1, w_total - 1, w_total, w_total + 5):
        occ, lo, recs, total = S.find_fast(sas, Ls, origins, distinct, which, max_hits)
        assert total == w_total and np.array_equal(occ, w_occ) and np.array_equal(recs, w_recs[:max_hits])
        got, got_total, _ = S.find_by_scan(occ, lo, sas, w_total + 5 if max_hits is None else max_hits)
        assert got_total == w_total and np.array_equal(got, recs)
    for node_limit in (None, 2):
        n_occ, n_recs, n_total, n_cut, _ = near_model(texts, [exact_classes(p) for p in pats], 0, node_limit)
        occ, recs, total, cut, _ = S.near_fast(texts, distinct, which, 0, node_limit)
        assert total == n_total and cut == n_cut and np.array_equal(occ, n_occ) and np.array_equal(recs, n_recs)
    s_occ, s_recs, s_total = seams_model(texts, pats, b"GTAC")
    occ, recs, total = S.seams_fast(texts, b"GTAC", distinct, which)
    assert total == s_total > 0 and np.array_equal(occ, s_occ) and np.array_equal(recs, s_recs)
    assert np.array_equal(S.seams_fast(texts, b"GTAC", distinct, which, 3)[1], s_recs[:3])


def test_pair_search_on_small_lists():
    rng = np.random.default_rng(7)
    for npairs in (1, 2, 63, 64, 65, 300, 4097):
        occ = rng.integers(0, 4, size=npairs) * (rng.integers(0, 3, size=npairs) == 0)
        offsets, total = S.find_scan(occ)
        pair, inside, rounds = S.find_pairs_of_hits(offsets, total)
        assert np.array_equal(pair, np.repeat(np.arange(npairs), occ)) and rounds <= S.find_levels(npairs)["search_rounds"]
        assert total == occ.sum() and np.array_equal(offsets.astype(np.int64), np.cumsum(occ) - occ)


# ---- D. the locate and extract builds ------------------------------------------------------------------------------------------------------------------------

D_WANT = {"per2": (dict(rows=1026, per=2, busy_threads=513), dict(ntiles=257, tpc=2, nchunks=129, last_chunk_tiles=1)),
          "per4": (dict(rows=3073, per=4, busy_threads=769), dict(ntiles=769, tpc=4, nchunks=193, last_chunk_tiles=1))}


@pytest.mark.parametrize("name", sorted(S.D_TOTALS))
def test_structure_case(orc, name):
    t = S.d_text(name)
    assert (S.loc_levels(len(t)), S.ibwt_levels(len(t))) == D_WANT[name]
    sa = sa_of(orc, name, t)
    L, origin = orc.bwt_forward(t, sa)
    marks = S.loc_marks(sa, S.D_STEP)
    assert len(marks) == S.loc_levels(len(t))["rows"] + 1 and marks[-1] == S.div_up(len(t), S.D_STEP)
    assert np.array_equal(S.loc_marks_by_scan(sa, S.D_STEP), marks)
    assert not np.array_equal(S.loc_marks_by_scan(sa, S.D_STEP, "per_one"), marks)
    good = S.ibwt_table_by_scan(L)
    assert np.array_equal(good[:S.ibwt_levels(len(t))["ntiles"]], S.ibwt_table(L))
    for fault in ("bases_zero", "full_last_chunk"):
        assert not np.array_equal(S.ibwt_table_by_scan(L, fault), good), fault


def test_loc_marks_are_the_locate_structures():
    rng = np.random.default_rng(8)
    for n, step in ((1, 1), (1023, 2), (1024, 4), (1025, 32), (5000, 3)):
        t = rng.integers(0, 4, size=n, dtype=np.uint8)
        sa = np.array(sa_plain(t), dtype=np.int64)
        marked, samples = locate_structure(None, None, sa, step)
        want = [int(marked[:r * S.LOC_ROW].sum()) for r in range(S.div_up(n, S.LOC_ROW))] + [int(marked.sum())]
        assert S.loc_marks(sa, step).tolist() == want == S.loc_marks_by_scan(sa, step).tolist() and want[-1] == len(samples)


# ---- E. the super-maximal matches' scan ------------------------------------------------------------------------------------------------------------------------

def test_smem_case(orc):
    t, q = S.smem_text(), S.smem_query()
    Q = S.E_COPIES * len(q)
    assert Q == 264000 and S.smem_levels(Q) == dict(ntiles=258, trips=2, last_trip_tiles=2)
    sa = sa_of(orc, "smem", t)
    one = np.array(smem_records(t, sa, [q], S.E_MIN_LEN, S.E_MAX_LEN), np.int64).reshape(-1, 4)
    recs = S.smem_repeat(one, len(q), S.E_COPIES)
    first = int((recs[:, 0] < S.SM_TRIP * S.SM_TILE).sum())
    assert 0 < first < len(recs) and (recs[:, 0] >= S.SM_TRIP * S.SM_TILE + S.SM_TILE).any(), "both tiles of the second trip hold records"
    for max_hits in (len(recs) + 1, first - 1, first, first + 1):
        listed, total = S.smem_list_by_scan(recs[:, 0], Q, max_hits)
        assert total == len(recs) and np.array_equal(listed, recs[:max_hits, 0])
        bad, bad_total = S.smem_list_by_scan(recs[:, 0], Q, max_hits, "second_from_zero")
        assert bad_total != total and not np.array_equal(bad, listed)


def test_smem_repeat_is_the_model_on_the_copies(orc):
    t = S.smem_text()[:3000]
    sa = np.array(sa_plain(t), dtype=np.int64)
    q = S.smem_query()[:150]
    for min_len in (0, 1, 6):
        one = smem_records(t, sa, [q], min_len, 1000)
        want = np.array(smem_records(t, sa, [q] * 5, min_len, 1000), np.int64).reshape(-1, 4)
        assert np.array_equal(S.smem_repeat(one, len(q), 5), want)
