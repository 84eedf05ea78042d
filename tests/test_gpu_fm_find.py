"""The FM-index's find on the GPU (csrc/fm_index.hip k_fm_find_*): dk_dev_fm_find / dk_dev_fm_find_packed / dk_fm_find,
fm.Index.find / grep and the C++ mirror.  Every pattern in every block; the answer is the occurrence matrix, the 64-bit total and one compact list
of hit records in the order (pattern, block, suffix-array slot).  The yardstick is tests/fm_find_model.py (brute force over sorted suffixes) for
small inputs, and dev_fm_count / dev_fm_locate on the replicated queries for large ones.  Every device output sits between guard words of 256
bytes (test_gpu_lcp.Words), and the hit buffer is pre-filled with the guard value, so a record written behind the list shows."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dark_amd
from conftest import ROOT
from dark_amd import datagen, fm
from dark_amd._lib import DK_E_ARG, FM_NO_HIT
from dark_amd.context import FM_HIT_DTYPE, fm_index_bytes, fm_locate_bytes
from fm_find_model import block_structures, find_model
from test_gpu_fm import gpu_bwt, gpu_count, gpu_index, words
from test_gpu_fm_locate import gpu_structure, whole_sa
from test_gpu_lcp import FILL, Words, dev_text, u8
from test_gpu_sa_search import cut_patterns, dev_patterns, gpu_sa

pytestmark = pytest.mark.gpu
CAP = (1 << 20) + 4096
TIMEOUT = 120
TUNING_LIB = os.path.join(ROOT, "dark_amd", "libdark_amd_tuning.so")


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


def gpu_find(ctx, d_bwt, sizes, idx, loc, step, patterns, max_hits, packed=None, want_occ=True):
    """-> (occ: npat x count int64 or None, the first min(total, max_hits) records, total).  packed: take the packed entry (default: for more
    than one block).  Checks that nothing but those records was written to the hit buffer or around any output."""
    count, npat = len(sizes), len(patterns)
    d_pat, lens = dev_patterns(patterns)
    hits = Words(4 * max_hits)
    occ = Words(npat * count) if want_occ else None
    args = (idx.t, None if loc is None else loc.t, step, d_pat, lens, max_hits, hits.t if max_hits else None, occ.t if want_occ else None)
    if count > 1 if packed is None else packed:
        total = ctx.dev_fm_find_packed(d_bwt, sizes, *args)
    else:
        total = ctx.dev_fm_find(d_bwt, sizes[0], *args)
    got = min(total, max_hits)
    raw = hits.host()
    assert hits.guards_intact() and (raw[4 * got:] == FILL).all(), "a record behind the first %d of %d (max_hits %d)" % (got, total, max_hits)
    assert idx.guards_intact() and (loc is None or loc.guards_intact()) and (occ is None or occ.guards_intact()), "a store left the outputs"
    return (occ.host().astype(np.int64).reshape(npat, count) if want_occ else None), raw[:4 * got].view(FM_HIT_DTYPE), total


def same_records(got, want, what=""):
    assert len(got) == len(want), "%s %d records, expected %d" % (what, len(got), len(want))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s record %d: %s, expected %s (%d wrong)" % (what, bad[0], got[bad[0]], want[bad[0]], bad.size)


def records_from(occ, los, sas):
    """the whole list from an occurrence matrix, the ranges' starts (npat x count) and the blocks' suffix arrays"""
    npat, count = occ.shape
    out = []
    for q in range(npat):
        for b in range(count):
            k, lo = int(occ[q, b]), int(los[q][b])
            if k:
                r = np.zeros(k, FM_HIT_DTYPE)
                r["pattern"], r["block"], r["slot"] = q, b, np.arange(lo, lo + k)
                r["position"] = np.asarray(sas[b])[lo:lo + k]
                out.append(r)
    return np.concatenate(out) if out else np.zeros(0, FM_HIT_DTYPE)


def pack_of(ctx, texts, step, shift=0):
    """L and origins from sorted suffixes (no GPU sort in the way), the index and the locate structure"""
    parts = [block_structures(t) for t in texts]
    sizes, origins = [len(p[1]) for p in parts], [p[2] for p in parts]
    d_bwt, idx = gpu_index(ctx, np.concatenate([p[1] for p in parts]), sizes, origins, shift)
    return d_bwt, idx, gpu_structure(ctx, d_bwt, sizes, origins, step), sizes


# ---- every short text as a block of one pack, every short pattern ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def short(ctx):
    texts, pats = words(b"ab", range(1, 9)), words(b"abc", range(0, 5))
    assert len(texts) == 510 and len(pats) == 121
    occ, recs, total = find_model(texts, pats)  # (computed once; nothing below changes it)
    d_bwt, idx, loc, sizes = pack_of(ctx, texts, 2)
    return dict(pats=pats, occ=occ.astype(np.int64), recs=recs, total=total, d_bwt=d_bwt, idx=idx, loc=loc, sizes=sizes)


def test_every_short_text_in_one_pack(ctx, short):
    s = short
    assert s["occ"].size == 61710 and s["total"] == len(s["recs"])
    occ, recs, total = gpu_find(ctx, s["d_bwt"], s["sizes"], s["idx"], s["loc"], 2, s["pats"], s["total"])
    assert total == s["total"] and np.array_equal(occ, s["occ"])
    same_records(recs, s["recs"])


@pytest.mark.parametrize("which", ["0", "1", "total - 1", "total", "total + 1"])
def test_truncation(ctx, short, which):
    s = short
    max_hits = {"0": 0, "1": 1, "total - 1": s["total"] - 1, "total": s["total"], "total + 1": s["total"] + 1}[which]
    occ, recs, total = gpu_find(ctx, s["d_bwt"], s["sizes"], s["idx"], s["loc"] if max_hits else None, 2, s["pats"], max_hits)
    assert total == s["total"] and np.array_equal(occ, s["occ"])
    same_records(recs, s["recs"][:max_hits], "max_hits = %s:" % which)  # (gpu_find has looked at everything behind them)
    _, recs, total = gpu_find(ctx, s["d_bwt"], s["sizes"], s["idx"], s["loc"], 2, s["pats"], max_hits, want_occ=False)  # d_occ is optional
    assert total == s["total"]
    same_records(recs, s["recs"][:max_hits])


# ---- the scan's borders ------------------------------------------------------------------------------------------------------------------------------

# pairs = patterns x blocks; 257 x 256 = 65 792 pairs are 257 rows of 256, two rows per chunk of the scan
GRIDS = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), 255: (15, 17), 256: (16, 16), 257: (257, 1), 4097: (17, 241), 65792: (257, 256)}


@pytest.mark.parametrize("pairs", sorted(GRIDS))
def test_scan_borders(ctx, pairs):
    """occ all zero, all one, and one pair of 2^16 hits among zeros; the offsets show in the records' (pattern, block) columns"""
    npat, count = GRIDS[pairs]
    assert npat * count == pairs
    n_big = 1 << 16
    d_bwt, idx, loc, sizes = pack_of(ctx, [b"a"] * count, 1)
    occ, recs, total = gpu_find(ctx, d_bwt, sizes, idx, loc, 1, [b"b"] * npat, 8, packed=True)
    assert total == 0 and not occ.any() and len(recs) == 0
    occ, recs, total = gpu_find(ctx, d_bwt, sizes, idx, loc, 1, [b"a"] * npat, pairs + 3, packed=True)
    assert total == pairs and (occ == 1).all()
    assert recs["pattern"].tolist() == [q for q in range(npat) for _ in range(count)] and recs["block"].tolist() == list(range(count)) * npat
    assert not recs["position"].any() and not recs["slot"].any()
    # block `at` is a^65536 among one-byte blocks "b", pattern `pq` is "a" among patterns "c": one pair with 2^16 hits.  (The empty pattern
    # would count every block's positions; it has the list to itself in the single-block case below.)
    at, pq = count // 2, npat - 1 - npat // 3
    sizes = [1] * count
    sizes[at] = n_big
    L = np.concatenate([np.full(n, 97 if b == at else 98, np.uint8) for b, n in enumerate(sizes)])
    origins = [n - 1 for n in sizes]
    d_bwt, idx = gpu_index(ctx, L, sizes, origins)
    loc = gpu_structure(ctx, d_bwt, sizes, origins, 32, packed=True)
    pats = [b"c"] * npat
    pats[pq] = b"a"
    occ, recs, total = gpu_find(ctx, d_bwt, sizes, idx, loc, 32, pats, n_big + 1, packed=True)
    want = np.zeros((npat, count), np.int64)
    want[pq, at] = n_big
    assert total == n_big and np.array_equal(occ, want)
    assert (recs["pattern"] == pq).all() and (recs["block"] == at).all()
    assert np.array_equal(recs["slot"], np.arange(n_big)) and np.array_equal(recs["position"], np.arange(n_big - 1, -1, -1))
    # one block of 2^16 bytes, the empty pattern among absent ones
    pats[pq] = b""
    d_one, idx_one = gpu_index(ctx, np.full(n_big, 97, np.uint8), [n_big], [n_big - 1])
    loc_one = gpu_structure(ctx, d_one, [n_big], [n_big - 1], 32)
    occ, recs, total = gpu_find(ctx, d_one, [n_big], idx_one, loc_one, 32, pats, n_big)
    assert total == n_big and occ[:, 0].tolist() == [n_big if q == pq else 0 for q in range(npat)]
    assert (recs["pattern"] == pq).all() and not recs["block"].any()
    assert np.array_equal(recs["slot"], np.arange(n_big)) and np.array_equal(recs["position"], np.arange(n_big - 1, -1, -1))


# ---- a total that needs 64 bits ------------------------------------------------------------------------------------------------------------------------

def test_total_beyond_32_bits(ctx):
    n, npat = 1 << 20, 8192
    t = np.random.default_rng(7).integers(97, 101, size=n, dtype=np.uint8)
    L, origin = gpu_bwt(ctx, t)
    sa = gpu_sa(ctx, t).host()
    d_bwt, idx = gpu_index(ctx, L, [n], [origin])
    loc = gpu_structure(ctx, d_bwt, [n], [origin], 32)
    occ, recs, total = gpu_find(ctx, d_bwt, [n], idx, loc, 32, [b""] * npat, 1000)
    assert total == 1 << 33 and occ.shape == (npat, 1) and (occ == n).all()
    assert not recs["pattern"].any() and not recs["block"].any()
    assert np.array_equal(recs["slot"], np.arange(1000)) and np.array_equal(recs["position"], sa[:1000])
    occ, recs, total = gpu_find(ctx, d_bwt, [n], idx, loc, 32, [b""] * 3, n + 5)  # the list crosses from one pair into the next
    assert total == 3 * n
    assert np.array_equal(recs["pattern"], np.concatenate([np.zeros(n, np.uint32), np.ones(5, np.uint32)]))
    assert np.array_equal(recs["position"], np.concatenate([sa, sa[:5]])) and np.array_equal(recs["slot"], np.concatenate([np.arange(n), np.arange(5)]))


# ---- one symbol ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_one_symbol(ctx, n):
    """a^n: the suffixes stand in order of ascending length, so a^m has the slots m - 1 .. n - 1 and slot x holds position n - 1 - x"""
    d_bwt, idx = gpu_index(ctx, np.full(n, 97, np.uint8), [n], [n - 1])
    loc = gpu_structure(ctx, d_bwt, [n], [n - 1], 32)
    lens = [1, 2, 1024]
    occ, recs, total = gpu_find(ctx, d_bwt, [n], idx, loc, 32, [b"a" * m for m in lens], 3 * n)
    want_occ = [max(n - m + 1, 0) for m in lens]
    assert occ[:, 0].tolist() == want_occ and total == sum(want_occ)
    want = records_from(np.array(want_occ)[:, None], [[m - 1] for m in lens], [np.arange(n - 1, -1, -1)])
    same_records(recs, want)


# ---- ordinary text: against count and locate on the replicated queries --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wiki(ctx):
    n = 1 << 18
    t = u8(datagen.wiki_like(n, seed=9))
    rng = np.random.default_rng(93)
    cut = [p for p in cut_patterns(t, rng, 256, list(range(1, 65)))[::2]]  # (the even ones: as they stand in the text)
    pats = cut + [rng.integers(0, 256, size=int(rng.integers(1, 65)), dtype=np.uint8) for _ in range(128)]
    assert len(pats) == 256 and all(1 <= len(p) <= 64 for p in pats)
    return dict(t=t, n=n, pats=pats)


def test_text_single_block(ctx, wiki):
    w = wiki
    n = w["n"]
    L, origin = gpu_bwt(ctx, w["t"])
    assert "lfirst" in ctx.stats()["routes"], ctx.stats()["routes"]
    d_bwt, idx = gpu_index(ctx, L, [n], [origin], shift=3)
    loc = gpu_structure(ctx, d_bwt, [n], [origin], 32)
    ranges = gpu_count(ctx, d_bwt, [n], idx, w["pats"])
    sa = whole_sa(ctx, d_bwt, [n], idx, loc, 32)[0]  # the rows of dev_fm_locate for the empty pattern's range: every slot's position
    want_occ = np.array([[hi - lo] for lo, hi in ranges], dtype=np.int64)
    occ, recs, total = gpu_find(ctx, d_bwt, [n], idx, loc, 32, w["pats"], int(want_occ.sum()) + 1)
    assert total == want_occ.sum() and np.array_equal(occ, want_occ) and (want_occ[:128] > 0).all()
    same_records(recs, records_from(want_occ, [[lo] for lo, _ in ranges], [sa]))
    tb = bytes(w["t"])
    for r in recs[:: max(1, len(recs) // 200)]:  # the definition itself: the pattern stands at the position
        p = bytes(w["pats"][int(r["pattern"])])
        assert tb[int(r["position"]):int(r["position"]) + len(p)] == p


def test_text_as_a_pack_of_16(ctx, wiki):
    w = wiki
    sizes = [w["n"] // 16] * 16
    d_L = torch.empty(w["n"], dtype=torch.uint8, device="cuda")
    origins = ctx.dev_bwt_forward_packed(dev_text(w["t"]), sizes, d_L)
    d_bwt, idx = gpu_index(ctx, d_L.cpu().numpy(), sizes, origins)
    loc = gpu_structure(ctx, d_bwt, sizes, origins, 32)
    every = [p for p in w["pats"] for _ in range(16)]
    where = [b for _ in w["pats"] for b in range(16)]
    ranges = gpu_count(ctx, d_bwt, sizes, idx, every, where)  # the replicated queries, q-major as the pairs are
    sas = whole_sa(ctx, d_bwt, sizes, idx, loc, 32)
    want_occ = np.array([hi - lo for lo, hi in ranges], dtype=np.int64).reshape(256, 16)
    los = np.array([lo for lo, _ in ranges], dtype=np.int64).reshape(256, 16)
    occ, recs, total = gpu_find(ctx, d_bwt, sizes, idx, loc, 32, w["pats"], int(want_occ.sum()))
    assert total == want_occ.sum() and np.array_equal(occ, want_occ)
    same_records(recs, records_from(want_occ, los, sas))


@pytest.mark.parametrize("step", [1, 32, 4096])
def test_single_form_equals_the_pack_of_one(ctx, step):
    t = u8(datagen.wiki_like(5000, seed=3))
    pats = [bytes(p) for p in cut_patterns(t, np.random.default_rng(5), 40, [1, 2, 3, 9])] + [b"", bytes(t), bytes(t) + b"a"]
    d_bwt, idx, loc, sizes = pack_of(ctx, [bytes(t)], step, shift=1)
    want_occ, want, want_total = find_model([bytes(t)], pats)
    for packed in (False, True):
        occ, recs, total = gpu_find(ctx, d_bwt, sizes, idx, loc, step, pats, want_total, packed=packed)
        assert total == want_total and np.array_equal(occ, want_occ)
        same_records(recs, want, "packed %s, step %d:" % (packed, step))


# ---- structures that are none ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("symbols", [2, 256])
def test_containment(ctx, symbols):
    """any bytes in L, then any words in the index, in d_loc, and in both: DK_OK, every field of every record inside its bound, guards intact"""
    rng = np.random.default_rng(171 + symbols)
    step = 4
    texts = [bytes(u8(datagen.wiki_like(2500, seed=3))), b"a", bytes(rng.integers(0, 256, size=1000, dtype=np.uint8)), b"a" * 596]
    d_bwt, idx, loc, sizes = pack_of(ctx, texts, step)
    total_bytes = sum(sizes)
    assert total_bytes == 4097
    pats = [bytes(p) for p in cut_patterns(u8(texts[0]), rng, 30, [1, 2, 3])] + [b"", b"a", b"\x00", bytes([symbols - 1])]
    limit = np.array(sizes, dtype=np.int64)

    def contained(what):
        for max_hits in (50000, 7):
            occ, recs, total = gpu_find(ctx, d_bwt, sizes, idx, loc, step, pats, max_hits)
            assert (occ >= 0).all() and (occ <= limit[None, :]).all() and total == occ.sum(), what
            assert len(recs) == min(total, max_hits), what
            assert (recs["pattern"] < len(pats)).all() and (recs["block"] < len(sizes)).all(), what
            nb = limit[recs["block"].astype(np.int64)]
            assert (recs["slot"] < nb).all() and ((recs["position"] < nb) | (recs["position"] == FM_NO_HIT)).all(), what
        occ, recs, total = gpu_find(ctx, d_bwt, [total_bytes], idx, loc, step, pats, 50000)  # the same words read as the structures of one block
        assert (recs["slot"] < total_bytes).all() and ((recs["position"] < total_bytes) | (recs["position"] == FM_NO_HIT)).all(), what
        assert (recs["pattern"] < len(pats)).all() and not recs["block"].any(), what

    good_idx, good_loc = idx.host(), loc.host()
    contained("good structures")
    d_bwt.copy_(torch.from_numpy(rng.integers(97 if symbols == 2 else 0, 99 if symbols == 2 else 256, size=total_bytes, dtype=np.uint8)))
    contained("an L that is none, the text's structures")
    ctx.dev_fm_build_packed(d_bwt, sizes, [0, 0, 999, 300], idx.t)
    contained("the index of that L")

    def noise(k):
        return torch.from_numpy(rng.integers(0, 1 << 32, size=k, dtype=np.uint64).astype(np.uint32).view(np.int32))
    loc.t.copy_(noise(len(good_loc)))
    contained("a random d_loc")
    idx.t.copy_(noise(len(good_idx)))
    contained("both random")
    loc.t.copy_(torch.from_numpy(good_loc.view(np.int32)))
    contained("a random index, the text's d_loc")


# ---- arguments -------------------------------------------------------------------------------------------------------------------------------------

def test_arguments(ctx):
    t = b"banana" * 50
    n = len(t)
    pats = [b"ana", b"nab", b"x"]
    d_bwt, idx, loc, _ = pack_of(ctx, [t], 8)
    want_occ, want, want_total = find_model([t], pats)
    d_pat, lens = dev_patterns(pats)
    hits, occ = Words(4 * 16), Words(3)
    lib, h = ctx._lib, ctx._h
    p_bwt, p_idx, p_loc, p_pat, p_hits, p_occ = (C.c_void_p(x.data_ptr()) for x in (d_bwt, idx.t, loc.t, d_pat, hits.t, occ.t))
    ns, ls, total = (C.c_size_t * 1)(n), (C.c_size_t * 3)(*lens), C.c_uint64(99)
    tot = C.byref(total)

    def off(x, k):
        return C.c_void_p(x.t.data_ptr() + k)

    def good():
        occ_g, recs, got = gpu_find(ctx, d_bwt, [n], idx, loc, 8, pats, 16)
        assert got == want_total and np.array_equal(occ_g, want_occ)
        same_records(recs, want[:16])
    good()
    single = ((None, n, p_idx, p_loc, 8, p_pat, 3, ls, 16, p_hits, p_occ, tot), (p_bwt, n, None, p_loc, 8, p_pat, 3, ls, 16, p_hits, p_occ, tot),
              (p_bwt, n, p_idx, None, 8, p_pat, 3, ls, 16, p_hits, p_occ, tot), (p_bwt, n, p_idx, p_loc, 8, None, 3, ls, 16, p_hits, p_occ, tot),
              (p_bwt, n, p_idx, p_loc, 8, p_pat, 3, None, 16, p_hits, p_occ, tot), (p_bwt, n, p_idx, p_loc, 8, p_pat, 3, ls, 16, None, p_occ, tot),
              (p_bwt, n, p_idx, p_loc, 8, p_pat, 3, ls, 16, p_hits, p_occ, None), (p_bwt, n, p_idx, p_loc, 8, p_pat, 3, ls, 0, None, p_occ, None),
              (p_bwt, 0, p_idx, p_loc, 8, p_pat, 3, ls, 16, p_hits, p_occ, tot), (p_bwt, CAP + 1, p_idx, p_loc, 8, p_pat, 3, ls, 16, p_hits, p_occ, tot),
              (p_bwt, n, off(idx, 2), p_loc, 8, p_pat, 3, ls, 16, p_hits, p_occ, tot), (p_bwt, n, p_idx, off(loc, 2), 8, p_pat, 3, ls, 16, p_hits, p_occ, tot),
              (p_bwt, n, p_idx, p_loc, 8, p_pat, 3, ls, 16, off(hits, 8), p_occ, tot), (p_bwt, n, p_idx, p_loc, 8, p_pat, 3, ls, 16, off(hits, 4), p_occ, tot),
              (p_bwt, n, p_idx, p_loc, 8, p_pat, 3, ls, 16, p_hits, off(occ, 2), tot), (p_bwt, n, p_idx, p_loc, 0, p_pat, 3, ls, 16, p_hits, p_occ, tot),
              (p_bwt, n, p_idx, p_loc, 12, p_pat, 3, ls, 16, p_hits, p_occ, tot), (p_bwt, n, p_idx, p_loc, 8192, p_pat, 3, ls, 16, p_hits, p_occ, tot),
              (p_bwt, n, p_idx, p_loc, 8, p_pat, 3, ls, (1 << 31) + 1, p_hits, p_occ, tot),
              (p_bwt, n, p_idx, p_loc, 8, p_pat, (1 << 24) + 1, ls, 16, p_hits, p_occ, tot))
    for args in single:
        assert lib.dk_dev_fm_find(h, *args) == DK_E_ARG, args
        assert lib.dk_dev_fm_find_packed(h, args[0], 1, ns if args[1] == n else (C.c_size_t * 1)(args[1]), *args[2:]) == DK_E_ARG, args
    assert lib.dk_dev_fm_find_packed(h, p_bwt, 1, None, p_idx, p_loc, 8, p_pat, 3, ls, 16, p_hits, p_occ, tot) == DK_E_ARG
    assert lib.dk_dev_fm_find_packed(h, p_bwt, 0, ns, p_idx, p_loc, 8, p_pat, 3, ls, 16, p_hits, p_occ, tot) == DK_E_ARG
    # 4097 blocks x 4096 patterns: one block more than DK_FM_FIND_MAX_PAIRS pairs (refused before the patterns are looked at)
    many = (C.c_size_t * 4097)(*([1] * 4097))
    assert lib.dk_dev_fm_find_packed(h, p_bwt, 4097, many, p_idx, p_loc, 8, p_pat, 4096, (C.c_size_t * 4096)(), 16, p_hits, p_occ, tot) == DK_E_ARG
    assert "DK_FM_FIND_MAX_PAIRS" in lib.dk_last_error(h).decode()
    assert total.value == 99 and hits.untouched() and occ.untouched()
    good()
    # the host form
    L = d_bwt.cpu().numpy()
    origin = block_structures(t)[2]
    h_hits, h_occ = np.zeros(16, FM_HIT_DTYPE), np.zeros(3, np.uint32)
    q_bwt, q_pat, q_hits, q_occ = (x.ctypes.data_as(C.c_void_p) for x in (L, u8(b"ananabx"), h_hits, h_occ))
    for args in ((None, n, origin, 8, q_pat, 3, ls, 16, q_hits, q_occ, tot), (q_bwt, 0, 0, 8, q_pat, 3, ls, 16, q_hits, q_occ, tot),
                 (q_bwt, CAP + 1, origin, 8, q_pat, 3, ls, 16, q_hits, q_occ, tot), (q_bwt, n, n, 8, q_pat, 3, ls, 16, q_hits, q_occ, tot),
                 (q_bwt, n, origin, 6, q_pat, 3, ls, 16, q_hits, q_occ, tot), (q_bwt, n, origin, 8, None, 3, ls, 16, q_hits, q_occ, tot),
                 (q_bwt, n, origin, 8, q_pat, 3, None, 16, q_hits, q_occ, tot), (q_bwt, n, origin, 8, q_pat, 3, ls, 16, None, q_occ, tot),
                 (q_bwt, n, origin, 8, q_pat, 3, ls, 16, q_hits, q_occ, None), (q_bwt, n, origin, 8, q_pat, 3, ls, (1 << 31) + 1, q_hits, q_occ, tot),
                 (q_bwt, n, origin, 8, q_pat, (1 << 24) + 1, ls, 16, q_hits, q_occ, tot)):
        assert lib.dk_fm_find(h, *args) == DK_E_ARG, args
    assert total.value == 99 and not h_occ.any() and not h_hits.view(np.uint32).any()
    # a workspace that cannot hold 16 bytes per pair; the context serves a good call afterwards
    with dark_amd.Context(1000, purpose="decoder") as small:
        size = small.stats()["ws_size_bytes"]
        npat = size // 16 + 1
        sd_bwt, sidx, sloc, _ = pack_of(small, [t], 8)
        for max_hits in (0, 4):
            with pytest.raises(dark_amd.DarkError) as e:
                gpu_find(small, sd_bwt, [n], sidx, sloc, 8, [b"a"] * npat, max_hits)
            assert e.value.code == DK_E_ARG and "workspace" in str(e.value)
            with pytest.raises(dark_amd.DarkError) as e:
                small.fm_find(L, origin, [b"a"] * npat, max_hits=max_hits, step=8)
            assert e.value.code == DK_E_ARG
        occ_g, recs, got = gpu_find(small, sd_bwt, [n], sidx, sloc, 8, pats, 16)
        assert got == want_total and np.array_equal(occ_g, want_occ)
        same_records(recs, want[:16])
    good()


def test_no_patterns(ctx):
    d_bwt, idx, loc, sizes = pack_of(ctx, [b"abab", b"b"], 2)
    for packed, ns in ((True, sizes), (False, [5])):
        occ, recs, total = gpu_find(ctx, d_bwt, ns, idx, loc, 2, [], 4, packed=packed)
        assert total == 0 and len(recs) == 0 and occ.size == 0


# ---- decoder contexts, and the workspace ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("purpose", ["decoder", "full"])
def test_contexts_sized_to_their_input(ctx, purpose):
    rng = np.random.default_rng(141)
    for n in (1, 1025, 65536):
        t = bytes(rng.integers(97, 101, size=n, dtype=np.uint8)) if n < 65536 else bytes(u8(datagen.wiki_like(n, seed=2)))
        pats = [b"", b"a", b"ab", t[:5], t[-3:], b"zz"]
        if n < 65536:
            want_occ, want, want_total = find_model([t], pats)
        with dark_amd.Context(n, purpose=purpose) as exact:
            if n < 65536:
                d_bwt, idx, loc, _ = pack_of(exact, [t], 32)
            else:  # (too long for sorted suffixes and the brute force: L from the module's context, count and locate of this one)
                L, origin = gpu_bwt(ctx, u8(t))
                d_bwt, idx = gpu_index(exact, L, [n], [origin])
                loc = gpu_structure(exact, d_bwt, [n], [origin], 32)
                ranges = gpu_count(exact, d_bwt, [n], idx, pats)
                want_occ = np.array([[hi - lo] for lo, hi in ranges], dtype=np.int64)
                want = records_from(want_occ, [[lo] for lo, _ in ranges], whole_sa(exact, d_bwt, [n], idx, loc, 32))
                want_total = int(want_occ.sum())
            occ, recs, total = gpu_find(exact, d_bwt, [n], idx, loc, 32, pats, want_total)
            assert total == want_total and np.array_equal(occ, want_occ)
            same_records(recs, want)
            st = exact.stats()
            assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], (purpose, n, st)
    texts = [bytes(rng.integers(97, 100, size=2000, dtype=np.uint8)) for _ in range(4)]
    pats = [b"", b"ab", b"abc", b"cab", b"d"]
    want_occ, want, want_total = find_model(texts, pats)
    with dark_amd.Context(8000, purpose=purpose, max_blocks=4) as exact:
        d_bwt, idx, loc, sizes = pack_of(exact, texts, 32)
        occ, recs, total = gpu_find(exact, d_bwt, sizes, idx, loc, 32, pats, want_total)
        assert total == want_total and np.array_equal(occ, want_occ)
        same_records(recs, want)
        st = exact.stats()
        assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], (purpose, st)
        if purpose == "decoder":
            with pytest.raises(dark_amd.DarkError) as e:  # five blocks on a context made for four
                gpu_find(exact, d_bwt, [1600] * 5, idx, loc, 32, pats, 4)
            assert e.value.code == DK_E_ARG
            for b in range(4):
                L, origin = block_structures(texts[b])[1:]
                assert bytes(exact.bwt_inverse(L, origin)) == texts[b]  # what the context was made for, after the queries


# ---- the host form and the layers above ----------------------------------------------------------------------------------------------------------------

def test_host_form(ctx):
    t = bytes(u8(datagen.wiki_like(5000, seed=3)))
    _, L, origin = block_structures(t)
    pats = [bytes(p) for p in cut_patterns(u8(t), np.random.default_rng(5), 40, [1, 2, 3, 9])] + [b"", t, t + b"a"]
    want_occ, want, want_total = find_model([t], pats)
    with dark_amd.Context(len(t), purpose="decoder") as dec:
        for c in (ctx, dec):
            # (on the decoder context the records share a workspace of about 15 n bytes with L and the structures: a prefix of the list)
            for max_hits in (want_total + 2 if c is ctx else 100, 5, 0):
                occ, recs, total = c.fm_find(L, origin, pats, max_hits=max_hits, step=32)
                assert total == want_total and np.array_equal(occ, want_occ[:, 0]) and recs.dtype == FM_HIT_DTYPE
                same_records(recs, want[:max_hits])
            occ, recs, total = c.fm_find(L, origin, [], max_hits=3)
            assert total == 0 and len(occ) == 0 and len(recs) == 0
        st = dec.stats()
        assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"]


def test_index_class(ctx):
    rng = np.random.default_rng(19)
    texts = [bytes(u8(datagen.wiki_like(3000, seed=s))) for s in (1, 2)] + [b"a", b"abcabcabc"]
    pats = [texts[0][:3], texts[0][-4:], texts[1][:2], b"abc", b"a", b"\x00\x00"]
    want_occ, want, want_total = find_model(texts, pats)
    parts = [block_structures(t) for t in texts]
    sizes, origins = [len(t) for t in texts], [p[2] for p in parts]
    d_L = dev_text(np.concatenate([p[1] for p in parts]))
    plain = fm.Index.from_bwt_packed(ctx, d_L, sizes, origins)
    occ, recs, total = plain.find(pats, max_hits=0)  # counting needs no locate structure
    assert total == want_total and np.array_equal(occ, want_occ) and occ.dtype == np.uint32 and len(recs) == 0
    for call in (lambda: plain.find(pats), lambda: plain.grep(pats, 1, 1)):
        with pytest.raises(dark_amd.DarkError) as e:
            call()
        assert e.value.code == DK_E_ARG
    index = fm.Index.from_bwt_packed(ctx, d_L, sizes, origins, locate_step=8, extract_step=16)
    occ, recs, total = index.find(pats)
    assert total == want_total and np.array_equal(occ, want_occ) and recs.dtype == FM_HIT_DTYPE
    same_records(recs, want)
    occ, recs, total = index.find(pats, max_hits=7)
    assert total == want_total
    same_records(recs, want[:7])
    assert index.find([])[2] == 0 and index.grep([], 3, 3) == []
    # windows at a block's head and end: pats[0] stands at position 0 of block 0, pats[1] at its end, "a" is the whole of block 2
    for before, after in ((5, 7), (0, 0), (4000, 4000)):
        got = index.grep(pats, before, after)
        assert len(got) == want_total
        for (q, b, at, text), r in zip(got, want):
            assert (q, b, at) == (int(r["pattern"]), int(r["block"]), int(r["position"]))
            assert text == texts[b][max(at - before, 0):at + len(pats[q]) + after], (q, b, at, before, after)
        assert any(at == 0 for _, _, at, _ in got) and any(at + len(pats[q]) == sizes[b] for q, b, at, _ in got)
    assert len(index.grep(pats, 2, 2, max_hits=3)) == 3
    one = fm.Index.from_bwt(ctx, parts[0][1], origins[0], locate_step=32, extract_step=32)  # a single block: no blocks to name
    occ, recs, total = one.find(pats)
    assert np.array_equal(occ[:, 0], want_occ[:, 0]) and total == want_occ[:, 0].sum()
    same_records(recs, want[want["block"] == 0])
    assert [(q, b, at) for q, b, at, _ in one.grep(pats, 3, 3)] == [(int(r["pattern"]), 0, int(r["position"])) for r in want[want["block"] == 0]]


def test_cpp_mirror(tmp_path):
    exe = str(tmp_path / "cpp_fm_find")
    lib_dir = os.path.join(ROOT, "dark_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_fm_find.cpp"),
                           "-L", lib_dir, "-ldark_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=TIMEOUT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cpp fm find ok" in out.stdout


# ---- a poisoned workspace behind a poisoned mailbox --------------------------------------------------------------------------------------------------

def test_poisoned_workspace_and_mailbox():
    """one run in a fresh process on the tuning build with DK_POISON=165, every call behind dk_dbg_mail_fill(165): tests/fm_find_poison_worker.py"""
    assert os.path.exists(TUNING_LIB), "build the tuning library: python dark_amd/build.py --tuning (__graft_entry__.build() does)"
    env = {k: v for k, v in os.environ.items() if not k.startswith("DK_")}
    env.update(DARK_AMD_LIB=TUNING_LIB, DK_POISON="165")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fm_find_poison_worker.py"), "fm_find", "165"], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=TIMEOUT)
    assert p.returncode == 0, "exit status %d\n%s" % (p.returncode, (p.stdout + p.stderr)[-3000:])
    report = json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    assert report["byte"] == 165 and report["contexts"] == 2 and report["fills"] > 0 and report["peeks"] >= 12 * report["contexts"], report
