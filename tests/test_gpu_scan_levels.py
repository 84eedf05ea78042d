"""The query-side scans past their first level (tests/scan_levels.py; checked without a GPU by tests/test_scan_levels_host.py, which also shows
that in every case the level decides the answer): k_lcp_spine's second pass, k_fm_scan_*'s chunks of two and three rows with a short last
chunk, k_fm_find_scan_*'s chunks of two and five rows under find, near and seams, a total beyond 2^32, the fourth round of k_fm_find_locate's
pair search, k_loc_scan's stretches of two and four rows, k_ibwt_scan_* with two and four tiles per chunk under the locate and extract builds,
and k_sa_smem_scan_b's second trip.  Every answer is compared whole with a plain model; every device output sits between guard words.

Where the suffix arrays come from: parts A1, A2 and D take the oracle's SA-IS (and its BWT); part A3 takes dev_suffix_array_packed, part E
dev_suffix_array; parts B and C need none (B: any bytes are an L; C: sorted suffixes of small blocks, and a^n)."""
import numpy as np
import pytest
import torch

import dark_amd
import scan_levels as S
from dark_amd.context import FM_HIT_DTYPE
from fm_extract_model import extract_rows
from fm_find_model import block_structures
from fm_model import fm_model_packed
from fm_near_model import exact_classes
from sa_match_model import smem_records
from test_gpu_fm import gpu_count, gpu_index
from test_gpu_fm_extract import gpu_anchors, gpu_extract
from test_gpu_fm_locate import gpu_structure, whole_sa
from test_gpu_fm_near import gpu_near
from test_gpu_fm_seams import gpu_seams
from test_gpu_lcp import FILL, Words, dev_text
from test_gpu_sa_match import depth_case, gpu_smems
from test_gpu_sa_search import gpu_sa

pytestmark = pytest.mark.gpu
CAP = max(S.A1_N, sum(S.A3_SIZES), S.LCP_BORDER + 2, max(S.D_TOTALS.values()), max(S.FM_TOTALS.values()))
HEADER_WORDS = 64  # of the index and of the locate structure


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


def put(words, values):
    words.t.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint32).view(np.int32)))
    return words


def first_bad(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, "%s: entry %d is %s, expected %s (%d wrong)" % (what, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]], bad.size)


# ---- A. the LCP spine ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", S.LCP_SINGLE)
def test_lcp_spine_single_block(ctx, orc, name):
    """a1: tiles 1024 and 1025 hold no measured position, their values come through the carry of the first pass.  a2: exactly one pass; one
    position and two positions in the second (the first of the two is reducible with the value 1)."""
    t = S.lcp_text(name)
    n = len(t)
    sa = np.asarray(orc.sa_sais(t), dtype=np.int64)
    want = S.lcp_fast(t, sa)
    d_sa, out = put(Words(n), sa), Words(n)
    ctx.dev_lcp(dev_text(t), n, d_sa.t, out.t)
    assert out.guards_intact() and d_sa.guards_intact(), "a store left the outputs"
    first_bad(out.host(), want, "%s, n = %d: LCP" % (name, n))


@pytest.mark.parametrize("one_call", [False, True])
def test_lcp_spine_pack(ctx, one_call):
    """block 0's plant straddles the border of the passes, block 1 begins inside tile 1024"""
    blocks = S.lcp_pack()
    sizes = [len(b) for b in blocks]
    total = sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    d_in, d_sa, d_lcp = dev_text(np.concatenate(blocks)), Words(total), Words(total)
    if one_call:
        ctx.dev_suffix_array_packed_lcp(d_in, sizes, d_sa.t, d_lcp.t)
    else:
        ctx.dev_suffix_array_packed(d_in, sizes, d_sa.t)
        ctx.dev_lcp_packed(d_in, sizes, d_sa.t, d_lcp.t)
    assert d_sa.guards_intact() and d_lcp.guards_intact(), "a store left the outputs"
    sa, lcp = d_sa.host().astype(np.int64), d_lcp.host()
    for k, b in enumerate(blocks):
        s = sa[off[k]:off[k + 1]]
        assert np.array_equal(np.sort(s), np.arange(len(b))), "block %d: no permutation" % k
        first_bad(lcp[off[k]:off[k + 1]], S.lcp_fast(b, s), "block %d of the pack: LCP" % k)
    assert lcp[:off[1]].max() == 1500 and lcp[off[1]:off[2]].max() == 2500  # (a wrong suffix array would not hold the plants)


# ---- B. the FM build's scan ------------------------------------------------------------------------------------------------------------------------------

def checkpoints_of(idx, rows):
    return idx.host()[HEADER_WORDS:HEADER_WORDS + 256 * rows].reshape(rows, 256)


@pytest.mark.parametrize("name", sorted(S.FM_TOTALS))
def test_fm_build_checkpoints(ctx, name):
    """the whole checkpoint table against prefix counts, and the rank kernel at every row border and beside it"""
    total = S.FM_TOTALS[name]
    rows = S.fm_levels(total)["rows"]
    L = S.fm_bytes(total)
    want = S.fm_checkpoints(L)
    d_bwt, idx = gpu_index(ctx, L, [total], [total // 3])
    first_bad(checkpoints_of(idx, rows), want, "%s: checkpoints" % name)
    syms = np.arange(0, 256, 17)
    border = np.arange(rows) * S.FM_BLOCK
    pos, occ = [], []
    for d in (-1, 0, 1):
        x = border + d
        ok = (x >= 0) & (x <= total)
        for c in syms:
            w = want[ok, c].astype(np.int64)
            if d == 1:
                w = w + (L[border[ok]] == c)
            elif d == -1:
                w = w - (L[x[ok]] == c)
            pos.append(np.stack([x[ok], np.full(ok.sum(), c)], axis=1))
            occ.append(w)
    pos, occ = np.concatenate(pos), np.concatenate(occ)
    d_pos = torch.from_numpy(pos[:, 0].astype(np.int32)).cuda()
    d_sym = torch.from_numpy(pos[:, 1].astype(np.uint8)).cuda()
    out = Words(len(pos))
    ctx.dbg_dev_fm_rank(d_bwt, total, idx.t, d_pos, d_sym, out.t)
    assert out.guards_intact() and idx.guards_intact()
    first_bad(out.host().astype(np.int64), occ, "%s: rank at the row borders" % name)


def test_fm_build_pack_heads_behind_chunk_0(ctx):
    """five blocks at rows 514: k_fm_heads reads checkpoints of chunks >= 1; a few patterns per block against fm_model"""
    sizes = S.fm_pack_sizes()
    total = sum(sizes)
    L = S.fm_bytes(total, seed=1)
    origins = [n // 2 for n in sizes]
    d_bwt, idx = gpu_index(ctx, L, sizes, origins)
    first_bad(checkpoints_of(idx, S.fm_levels(total)["rows"]), S.fm_checkpoints(L), "the pack's checkpoints")
    rng = np.random.default_rng(90)
    pats = [bytes(rng.integers(0, 256, size=int(m), dtype=np.uint8)) for _ in sizes for m in (0, 1, 1, 2, 2, 3)]
    where = [b for b in range(len(sizes)) for _ in range(6)]
    off = np.concatenate([[0], np.cumsum(sizes)])
    want = fm_model_packed([L[off[b]:off[b + 1]] for b in range(len(sizes))], origins, pats, where)
    got = gpu_count(ctx, d_bwt, sizes, idx, pats, where)
    assert got == want, [(q, g, w) for q, (g, w) in enumerate(zip(got, want)) if g != w][:4]


# ---- C. the find family's scans ------------------------------------------------------------------------------------------------------------------------------

def run_find(ctx, d_bwt, sizes, idx, loc, step, distinct, which, max_hits):
    """test_gpu_fm_find.gpu_find with the patterns uploaded from flat arrays (262 444 of them in c3)"""
    count, npat = len(sizes), len(which)
    flat, lens = S.flat_patterns(distinct, which)
    d_pat = dev_text(np.concatenate([flat, np.zeros(1, np.uint8)]))
    hits, occ = Words(4 * max_hits), Words(npat * count)
    args = (idx.t, loc.t, step, d_pat, lens.tolist(), max_hits, hits.t, occ.t)
    total = ctx.dev_fm_find_packed(d_bwt, sizes, *args) if count > 1 else ctx.dev_fm_find(d_bwt, sizes[0], *args)
    got = min(total, max_hits)
    raw = hits.host()
    assert hits.guards_intact() and (raw[4 * got:] == FILL).all(), "a record behind the first %d of %d (max_hits %d)" % (got, total, max_hits)
    assert idx.guards_intact() and loc.guards_intact() and occ.guards_intact(), "a store left the outputs"
    return occ.host().astype(np.int64).reshape(npat, count), raw[:4 * got].view(FM_HIT_DTYPE), total


def same_records(got, want, fields, what):
    assert len(got) == len(want), "%s: %d records, expected %d" % (what, len(got), len(want))
    for f in fields:
        first_bad(got[f], want[f], "%s: column %s" % (what, f))


def find_pack(ctx, c, step):
    sizes = [len(L) for L in c["Ls"]]
    d_bwt, idx = gpu_index(ctx, np.concatenate(c["Ls"]), sizes, c["origins"])
    return d_bwt, idx, gpu_structure(ctx, d_bwt, sizes, c["origins"], step), sizes


@pytest.mark.parametrize("name", S.FIND_CASES)
def test_find_scan(ctx, name):
    """c1: chunks of two rows, the last of one row of three pairs, every offset used.  c2: a total of 5.2e9, the list cut at 4096.  c3: chunks
    of five rows and the fourth round of the pair search."""
    c = S.find_case(name)
    step = 32 if name == "c2_64bit" else 4
    w_occ, _, w_recs, w_total = S.find_fast(c["sas"], c["Ls"], c["origins"], c["distinct"], c["which"], c["max_hits"])
    d_bwt, idx, loc, sizes = find_pack(ctx, c, step)
    occ, recs, total = run_find(ctx, d_bwt, sizes, idx, loc, step, c["distinct"], c["which"], c["max_hits"] or w_total + 1)
    assert total == w_total, "%s: total %d, expected %d" % (name, total, w_total)
    first_bad(occ, w_occ, name + ": occ")
    same_records(recs, w_recs, ("pattern", "block", "slot", "position"), name)


@pytest.fixture(scope="module")
def c1_near(ctx):
    """C1's blocks and patterns for near: the pack, the patterns as one-bit classes, and find's answer on the GPU"""
    c = S.find_case("c1_full_list")
    texts = S.c1_texts()
    d_bwt, idx, loc, sizes = find_pack(ctx, c, 4)
    cls_d = [exact_classes(p) for p in c["distinct"]]
    classes = [cls_d[k] for k in c["which"]]
    return dict(c=c, texts=texts, pack=(d_bwt, idx, loc, sizes), classes=classes)


def test_near_scan_is_find(ctx, c1_near):
    """C4: k = 0 and one-bit classes at C1's shape give find's records"""
    s = c1_near
    c = s["c"]
    d_bwt, idx, loc, sizes = s["pack"]
    f_occ, _, f_recs, f_total = S.find_fast(c["sas"], c["Ls"], c["origins"], c["distinct"], c["which"])
    occ, recs, total, cut = gpu_near(ctx, d_bwt, sizes, idx, loc, 4, s["classes"], 0, f_total + 1)
    assert total == f_total and cut == 0
    first_bad(occ, f_occ, "near: occ")
    same_records(recs, f_recs, ("pattern", "block", "position"), "near against find")
    assert not recs["cost"].any()


def test_near_scan_of_the_cut_pairs(ctx, c1_near):
    """C4 again with a node limit that cuts 24 000 pairs, nearly all of them in chunks >= 1: the second scan's total"""
    s = c1_near
    c = s["c"]
    d_bwt, idx, loc, sizes = s["pack"]
    w_occ, w_recs, w_total, w_cut, _ = S.near_fast(s["texts"], c["distinct"], c["which"], 0, S.NEAR_NODE_LIMIT)
    occ, recs, total, cut = gpu_near(ctx, d_bwt, sizes, idx, loc, 4, s["classes"], 0, w_total + 1, node_limit=S.NEAR_NODE_LIMIT)
    assert (total, cut) == (w_total, w_cut), "total %d cut %d, expected %d and %d" % (total, cut, w_total, w_cut)
    first_bad(occ, w_occ, "near with a node limit: occ")
    same_records(recs, w_recs, ("pattern", "block", "position", "cost"), "near with a node limit")


def test_seams_scan(ctx):
    """C5: 67 200 pairs, chunks of two rows, the last of one"""
    s = S.seams_case()
    texts = [bytes(b) for b in s["blocks"]]
    parts = [block_structures(t) for t in texts]
    sizes, origins = [len(t) for t in texts], [p[2] for p in parts]
    d_bwt, idx = gpu_index(ctx, np.concatenate([p[1] for p in parts]), sizes, origins)
    ext = gpu_anchors(ctx, d_bwt, sizes, origins, 4)
    w_occ, w_recs, w_total = S.seams_fast(s["blocks"], s["prev"], s["distinct"], s["which"])
    pats = [s["distinct"][k] for k in s["which"]]
    occ, recs, total = gpu_seams(ctx, d_bwt, sizes, idx, ext, 4, bytes(s["prev"]), pats, w_total + 1)
    assert total == w_total
    first_bad(occ, w_occ, "seams: occ")
    same_records(recs, w_recs, ("pattern", "block", "back", "reserved"), "seams")


# ---- D. the locate and extract builds above 2^20 -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=sorted(S.D_TOTALS))
def big_block(request, ctx, orc):
    """one block of random bytes, its suffix array and BWT from the oracle, the index on the GPU"""
    t = S.d_text(request.param)
    sa = np.asarray(orc.sa_sais(t), dtype=np.int64)
    L, origin = orc.bwt_forward(t, sa)
    d_bwt, idx = gpu_index(ctx, L, [len(t)], [int(origin)])
    return dict(name=request.param, t=t, sa=sa, origin=int(origin), d_bwt=d_bwt, idx=idx)


def test_locate_build_above_2_20(ctx, big_block):
    """the mark words against the suffix array, then every slot located: the whole suffix array through the empty pattern's range"""
    b = big_block
    n = len(b["t"])
    rows = S.loc_levels(n)["rows"]
    loc = gpu_structure(ctx, b["d_bwt"], [n], [b["origin"]], S.D_STEP)
    first_bad(loc.host()[HEADER_WORDS:HEADER_WORDS + rows + 1], S.loc_marks(b["sa"], S.D_STEP), "%s: mark words" % b["name"])
    got = whole_sa(ctx, b["d_bwt"], [n], b["idx"], loc, S.D_STEP)[0]
    first_bad(got, b["sa"], "%s: located positions" % b["name"])


def test_extract_build_above_2_20(ctx, big_block):
    """ranges whose chunks end at anchors in slots >= 2^20 (checkpoint rows >= 1024), at both ends of the text and across 2^20"""
    b = big_block
    t, sa = b["t"], b["sa"]
    n = len(t)
    ext = gpu_anchors(ctx, b["d_bwt"], [n], [b["origin"]], S.D_STEP)
    rank = np.empty(n, np.int64)
    rank[sa] = np.arange(n)
    ends = np.arange(S.D_STEP, n, S.D_STEP)
    high = ends[rank[ends] >= 1 << 20]
    assert len(high) >= 16  # (about (n - 2^20) / step of them: 32 at n = 2^20 + 1025)
    pick = high[np.linspace(0, len(high) - 1, min(200, len(high))).astype(np.int64)]
    ranges = [(int(e) - S.D_STEP, 100) for e in pick] + [(0, 100), (n - 50, 100), ((1 << 20) - 40, 100), (n - 1, 1), (n - S.D_STEP - 3, 70)]
    got = gpu_extract(ctx, b["d_bwt"], [n], b["idx"], ext, S.D_STEP, ranges, 100)
    first_bad(got, extract_rows(t, ranges, 100), "%s: extracted bytes" % b["name"])


# ---- E. the super-maximal matches' scan ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def smem_case(ctx):
    t, q = S.smem_text(), S.smem_query()
    assert np.array_equal(t, depth_case(1 << 16)[0])
    sa = gpu_sa(ctx, t)
    one = smem_records(t, sa.host(), [q], S.E_MIN_LEN, S.E_MAX_LEN)  # the model runs once; the 88 copies repeat its records
    want = S.smem_repeat(one, len(q), S.E_COPIES)
    first = int((want[:, 0] < S.SM_TRIP * S.SM_TILE).sum())
    return dict(t=t, sa=sa, queries=[q] * S.E_COPIES, want=want, first=first)


@pytest.mark.parametrize("which", ["all", "first trip - 1", "first trip", "first trip + 1"])
def test_smem_scan_second_trip(ctx, smem_case, which):
    """258 tiles: the second trip of k_sa_smem_scan_b holds two.  The list whole, and cut beside the first record of tile 256."""
    s = smem_case
    max_hits = {"all": len(s["want"]) + 1, "first trip - 1": s["first"] - 1, "first trip": s["first"], "first trip + 1": s["first"] + 1}[which]
    got, total = gpu_smems(ctx, s["t"], s["sa"], s["queries"], S.E_MIN_LEN, S.E_MAX_LEN, max_hits)
    assert total == len(s["want"]), "total %d, expected %d" % (total, len(s["want"]))
    first_bad(got, s["want"][:max_hits], "max_hits %d: records" % max_hits)
