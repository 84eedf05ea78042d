"""The FM-index's near on the GPU (csrc/fm_index.hip k_fm_near_*): dk_dev_fm_near / dk_dev_fm_near_packed and
fm.Index.near / near_grep.  Every pattern -- a sequence of byte classes -- in every block with at most k positions missed; the answer is the
occurrence matrix, the 64-bit total, the number of pairs cut at the node limit and one compact list of records (pattern, block, position, cost)
in the preorder of each pair's search tree.  The yardstick is tests/fm_near_model.py (brute force) for small inputs and dev_fm_find_packed for
large ones; every comparison is exact.  Every device output sits between guard words of 256 bytes (test_gpu_lcp.Words), and the hit buffer is
pre-filled with the guard value, so a record written behind the list shows."""
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
from dark_amd._lib import DK_E_ARG, FM_NEAR_MAX_PATTERN, FM_NO_HIT
from dark_amd.context import FM_NEAR_HIT_DTYPE
from fm_find_model import block_structures
from fm_near_model import exact_classes, near_model
from test_gpu_fm import gpu_bwt, gpu_index, words
from test_gpu_fm_find import gpu_find, pack_of, same_records
from test_gpu_fm_locate import gpu_structure
from test_gpu_lcp import FILL, Words, dev_text, u8
from test_gpu_sa_search import cut_patterns

pytestmark = pytest.mark.gpu
CAP = (1 << 18) + 4096
TIMEOUT = 120
TUNING_LIB = os.path.join(ROOT, "dark_amd", "libdark_amd_tuning.so")


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


def dev_classes(classes, shift=0):
    """-> (the classes back to back on the device, `shift` bytes off their place; the patterns' lengths)"""
    lens = [len(c) for c in classes]
    flat = np.concatenate([np.asarray(c, np.uint8).reshape(-1) for c in classes]) if sum(lens) else np.zeros(32, np.uint8)
    return dev_text(flat, shift), lens


def gpu_near(ctx, d_bwt, sizes, idx, loc, step, classes, k, max_hits, node_limit=0, packed=None, want_occ=True, shift=0):
    """-> (occ: npat x count int64 or None, the first min(total, max_hits) records, total, cut).  packed: take the packed entry (default: for
    more than one block).  Checks that nothing but those records was written to the hit buffer or around any output."""
    count, npat = len(sizes), len(classes)
    d_cls, lens = dev_classes(classes, shift)
    hits = Words(4 * max_hits)
    occ = Words(npat * count) if want_occ else None
    args = (idx.t, None if loc is None else loc.t, step, d_cls, lens, k, node_limit, max_hits, hits.t if max_hits else None, occ.t if want_occ else None)
    if count > 1 if packed is None else packed:
        total, cut = ctx.dev_fm_near_packed(d_bwt, sizes, *args)
    else:
        total, cut = ctx.dev_fm_near(d_bwt, sizes[0], *args)
    got = min(total, max_hits)
    raw = hits.host()
    assert hits.guards_intact() and (raw[4 * got:] == FILL).all(), "a record behind the first %d of %d (max_hits %d)" % (got, total, max_hits)
    assert idx.guards_intact() and (loc is None or loc.guards_intact()) and (occ is None or occ.guards_intact()), "a store left the outputs"
    return (occ.host().astype(np.int64).reshape(npat, count) if want_occ else None), raw[:4 * got].view(FM_NEAR_HIT_DTYPE), total, cut


def check(ctx, pack, classes, k, node_limit=None, what="", **kw):
    """one call against the model: occ, total, cut and the whole list"""
    d_bwt, idx, loc, sizes, texts, step = pack
    w_occ, w_recs, w_total, w_cut, nodes = near_model(texts, classes, k, node_limit)
    occ, recs, total, cut = gpu_near(ctx, d_bwt, sizes, idx, loc, step, classes, k, w_total + 1, node_limit or 0, **kw)
    assert total == w_total and cut == w_cut, "%s total %d cut %d, expected %d and %d" % (what, total, cut, w_total, w_cut)
    assert np.array_equal(occ, w_occ.astype(np.int64)), what
    same_records(recs, w_recs, what)
    return w_recs, nodes


def make_pack(ctx, texts, step):
    texts = [bytes(u8(t)) for t in texts]
    d_bwt, idx, loc, sizes = pack_of(ctx, texts, step)
    return d_bwt, idx, loc, sizes, texts, step


# ---- every short text as a block of one pack, every short pattern, every budget -----------------------------------------------------------------

@pytest.fixture(scope="module")
def short(ctx):
    texts = words(b"ab", range(1, 9))
    pats = words(b"ab", range(0, 5)) + [b"c", b"ac", b"cb", b"bcb", b"abca", b"cccc"]
    assert len(texts) == 510 and len(pats) == 37
    classes = [exact_classes(p) for p in pats]
    want = {k: near_model(texts, classes, k) for k in range(4)}  # (computed once; nothing below changes it)
    return dict(pack=make_pack(ctx, texts, 2), classes=classes, want=want)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_every_short_text_in_one_pack(ctx, short, k):
    """where wrap-around at the origin, a pattern at the text's end and patterns longer than the block go wrong"""
    d_bwt, idx, loc, sizes, _, step = short["pack"]
    w_occ, w_recs, w_total, w_cut, _ = short["want"][k]
    assert w_cut == 0 and w_total == len(w_recs) > 0
    occ, recs, total, cut = gpu_near(ctx, d_bwt, sizes, idx, loc, step, short["classes"], k, w_total, shift=k)  # (d_cls has any alignment)
    assert total == w_total and cut == 0 and np.array_equal(occ, w_occ.astype(np.int64))
    same_records(recs, w_recs, "k = %d:" % k)


@pytest.mark.parametrize("which", ["0", "1", "total - 1", "total", "total + 1"])
def test_truncation(ctx, short, which):
    d_bwt, idx, loc, sizes, _, step = short["pack"]
    w_occ, w_recs, w_total, _, _ = short["want"][1]
    max_hits = {"0": 0, "1": 1, "total - 1": w_total - 1, "total": w_total, "total + 1": w_total + 1}[which]
    occ, recs, total, cut = gpu_near(ctx, d_bwt, sizes, idx, loc if max_hits else None, step, short["classes"], 1, max_hits)
    assert total == w_total and cut == 0 and np.array_equal(occ, w_occ.astype(np.int64))
    same_records(recs, w_recs[:max_hits], "max_hits = %s:" % which)  # (gpu_near has looked at everything behind them)
    _, recs, total, _ = gpu_near(ctx, d_bwt, sizes, idx, loc, step, short["classes"], 1, max_hits, want_occ=False)  # d_occ is optional
    assert total == w_total
    same_records(recs, w_recs[:max_hits])


def test_truncation_inside_a_leaf(ctx):
    """a^300 holds a^4 297 times in one leaf: the list ends in the middle of its second round of 64 records, and in the middle of a later pair"""
    pack = make_pack(ctx, [b"a" * 300, b"a" * 200], 4)
    classes = [exact_classes(b"aaaa")]
    w_recs, _ = check(ctx, pack, classes, 1)
    assert len(w_recs) == 297 + 197
    d_bwt, idx, loc, sizes, _, step = pack
    for max_hits in (63, 64, 65, 100, 297, 298, 400):
        _, recs, total, _ = gpu_near(ctx, d_bwt, sizes, idx, loc, step, classes, 1, max_hits)
        assert total == 494
        same_records(recs, w_recs[:max_hits], "max_hits = %d:" % max_hits)


# ---- against find ------------------------------------------------------------------------------------------------------------------------------------

def keys(recs):
    return np.sort((recs["pattern"].astype(np.int64) << 44) | (recs["block"].astype(np.int64) << 32) | recs["position"].astype(np.int64))


def test_k_0_with_one_bit_classes_is_find(ctx):
    """2^18 bytes from the L-first path as one block, and the same bytes as a pack of 16"""
    n = 1 << 18
    t = u8(datagen.wiki_like(n, seed=9))
    rng = np.random.default_rng(93)
    pats = [bytes(p) for p in cut_patterns(t, rng, 96, [2, 3, 5, 8, 13, 24, 64, 128])[::2]] + [bytes(rng.integers(0, 256, size=6, dtype=np.uint8))]
    classes = [exact_classes(p) for p in pats]
    L, origin = gpu_bwt(ctx, t)
    assert "lfirst" in ctx.stats()["routes"], ctx.stats()["routes"]
    sizes16 = [n // 16] * 16
    d_L = torch.empty(n, dtype=torch.uint8, device="cuda")
    origins16 = ctx.dev_bwt_forward_packed(dev_text(t), sizes16, d_L)
    for sizes, Lb, origins in (([n], L, [origin]), (sizes16, d_L.cpu().numpy(), origins16)):
        d_bwt, idx = gpu_index(ctx, Lb, sizes, origins)
        loc = gpu_structure(ctx, d_bwt, sizes, origins, 32)
        f_occ, f_recs, f_total = gpu_find(ctx, d_bwt, sizes, idx, loc, 32, pats, 1 << 20)
        assert 0 < f_total < 1 << 20
        occ, recs, total, cut = gpu_near(ctx, d_bwt, sizes, idx, loc, 32, classes, 0, 1 << 20)
        assert total == f_total and cut == 0 and np.array_equal(occ, f_occ)
        assert not recs["cost"].any() and np.array_equal(keys(recs), keys(f_recs))


# ---- checkpoint rows, leaves of more than 64 hits -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_checkpoint_rows(ctx, n):
    """a^n and (ab)^n: ranges that straddle the rows of the index and are wider than one, one leaf with more than 64 hits"""
    classes = [exact_classes(b"aaaa"), exact_classes(b"abab")]
    pack = make_pack(ctx, [b"a" * n, b"ab" * n], 32)
    for k in (0, 1):
        w_recs, _ = check(ctx, pack, classes, k, what="n = %d k = %d:" % (n, k))
        assert len(w_recs) > 2 * n - 8
    for t in pack[4]:  # and each text as a single block, by the single entry
        check(ctx, make_pack(ctx, [t], 32), classes, 1, what="single, %d bytes:" % len(t))


# ---- all 256 symbols --------------------------------------------------------------------------------------------------------------------------------

def test_wide_alphabet(ctx):
    """presence sets over all four symbols of a lane, the class bits of bytes 0, 1 and 255"""
    rng = np.random.default_rng(201)
    t = bytes(rng.integers(0, 256, size=4096, dtype=np.uint8)) + bytes(range(256))
    pats = [t[i:i + 8] for i in rng.integers(0, len(t) - 8, size=10).tolist()] + [t[-8:], t[4096:4104], b"\x00" * 8, b"\xff" * 8,
                                                                                 b"\x00\x01\xfe\xff\x00\x01\xfe\xff", t[:3] + b"\x00\xff" + t[5:8]]
    classes = [exact_classes(p) for p in pats]
    pack = make_pack(ctx, [t], 8)
    for k in (1, 2):
        w_recs, nodes = check(ctx, pack, classes, k, what="k = %d:" % k)
        assert len(w_recs) >= 12 and nodes.max() > 256


# ---- classes -------------------------------------------------------------------------------------------------------------------------------------------

def wordlike(n, seed):
    rng = np.random.default_rng(seed)
    t = bytearray(datagen.wiki_like(n, seed=seed))
    for i in np.flatnonzero(rng.random(n) < 0.3).tolist():
        t[i] = ord(chr(t[i]).upper()) if t[i] < 128 else t[i]
    return bytes(t)


def test_classes(ctx):
    t = wordlike(6000, 4)
    assert t != t.lower() and t != t.upper()
    pack = make_pack(ctx, [t, t[1000:1300]], 8)
    low = t.lower()
    pats = [low[i:i + m] for i, m in ((10, 3), (500, 5), (2000, 4), (4000, 7), (5990, 10))] + [b"The", b"tHE "]
    folded = [fm.classes(p, ignore_case=True) for p in pats]
    w_recs, _ = check(ctx, pack, folded, 0, what="ignore_case:")
    for q, p in enumerate(pats):  # against enumeration on bytes.lower()
        for b, text in enumerate(pack[4]):
            want = [i for i in range(len(text) - len(p) + 1) if text.lower()[i:i + len(p)] == p.lower()]
            mine = w_recs[(w_recs["pattern"] == q) & (w_recs["block"] == b)]
            assert sorted(mine["position"].tolist()) == want, (p, b)
    assert any(t[int(r["position"]):int(r["position"]) + len(pats[int(r["pattern"])])] != pats[int(r["pattern"])] for r in w_recs if r["block"] == 0)
    check(ctx, pack, folded, 1, what="ignore_case, k = 1:")
    # a wildcard in the middle; four wildcards on 300 bytes: every position in [0, n - 4]
    wild = [fm.classes(t[10:13] + b"?" + t[14:17], wildcard=ord("?")), fm.classes(b"t??e", ignore_case=True, wildcard=63), fm.classes(b"????", wildcard=63)]
    w_recs, _ = check(ctx, pack, wild, 0, what="wildcards:")
    four = w_recs[(w_recs["pattern"] == 2) & (w_recs["block"] == 1)]
    assert sorted(four["position"].tolist()) == list(range(297)) and not four["cost"].any()
    assert (w_recs["pattern"] == 0).any()
    # an empty class at one position: no hit without budget, and with k = 1 that position always costs
    none = exact_classes(t[500:505])
    none[2] = 0
    w_recs, _ = check(ctx, pack, [none], 0, what="an empty class, k = 0:")
    assert len(w_recs) == 0
    w_recs, _ = check(ctx, pack, [none], 1, what="an empty class, k = 1:")
    assert len(w_recs) > 0 and (w_recs["cost"] == 1).all()


# ---- the deepest stack ------------------------------------------------------------------------------------------------------------------------------------

def test_depth(ctx):
    t = bytes(u8(datagen.wiki_like(4096, seed=12)))
    at = 1777
    p = bytearray(t[at:at + FM_NEAR_MAX_PATTERN])
    for i in (0, 61, FM_NEAR_MAX_PATTERN - 1):
        p[i] ^= 0x15
    assert len(p) == 128
    pack = make_pack(ctx, [t], 32)
    w_recs, _ = check(ctx, pack, [exact_classes(bytes(p))], 3, what="k = 3:")
    assert w_recs.tolist() == [(0, 0, at, 3)]
    w_recs, _ = check(ctx, pack, [exact_classes(bytes(p))], 2, what="k = 2:")
    assert len(w_recs) == 0


# ---- the node limit ---------------------------------------------------------------------------------------------------------------------------------------

def test_node_limit(ctx):
    """the limit of the call against pairs whose N the model gives; the empty pattern's pairs (N = 1) are never cut"""
    texts = [bytes(u8(datagen.wiki_like(600, seed=6))), b"mississippi" * 9, b"abra", b"ab" * 50]
    classes = [exact_classes(texts[0][100:106]), exact_classes(b""), exact_classes(b"issi")]
    pack = make_pack(ctx, texts, 4)
    whole, nodes = check(ctx, pack, classes, 2)
    N = int(nodes[2, 1])  # "issi" in (mississippi)^9: 27 hits with k = 2 in a tree of 21 nodes; the first pair's tree has several hundred
    all_of_it = whole[(whole["pattern"] == 2) & (whole["block"] == 1)]
    assert 3 < N < 64 < nodes[0, 0] and nodes[1].tolist() == [1, 1, 1, 1] and len(all_of_it) > 20
    seen = set()
    for limit in (1, 2, 3, 64, N - 1, N, N + 1, int(nodes.max()), int(nodes.max()) + 1):
        recs, _ = check(ctx, pack, classes, 2, node_limit=limit, what="limit %d:" % limit)
        seen.add(int((nodes > limit).sum()))
        mine = recs[(recs["pattern"] == 2) & (recs["block"] == 1)]
        assert np.array_equal(mine, all_of_it[:len(mine)]) and (limit < N or len(mine) == len(all_of_it))
    assert 0 in seen and 8 in seen and len(seen) > 3  # nothing cut, every pair with a pattern cut, and some in between
    # the default limit is DK_FM_NEAR_NODE_LIMIT: node_limit = 0 cuts nothing here
    d_bwt, idx, loc, sizes, _, step = pack
    assert gpu_near(ctx, d_bwt, sizes, idx, loc, step, classes, 2, 0)[3] == 0


# ---- the scan's borders -------------------------------------------------------------------------------------------------------------------------------

GRIDS = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), 257: (257, 1)}


@pytest.mark.parametrize("pairs", sorted(GRIDS))
def test_pair_counts(ctx, pairs):
    npat, count = GRIDS[pairs]
    texts = words(b"ab", [5])[3:3 + count] if count > 1 else [b"abaababaabaab"]
    pats = words(b"ab", range(0, 9))[:npat]
    assert len(texts) == count and len(pats) == npat
    check(ctx, make_pack(ctx, texts, 2), [exact_classes(p) for p in pats], 1, packed=True, what="%d pairs:" % pairs)


# ---- structures that are none ----------------------------------------------------------------------------------------------------------------------------

def test_containment(ctx):
    """any words in d_loc, then in the index, then any bytes in d_cls: the call returns, every field of every record is inside its bound and the
    guards are intact.  This checks clamps; nothing here is meant to fault.  (A small node limit: a tree that is none has no size of its own.)"""
    rng = np.random.default_rng(177)
    step, k, limit = 4, 2, 256
    texts = [bytes(u8(datagen.wiki_like(2500, seed=3))), b"a", bytes(rng.integers(0, 256, size=1000, dtype=np.uint8)), b"a" * 596]
    d_bwt, idx, loc, sizes = pack_of(ctx, texts, step)
    pats = [bytes(p) for p in cut_patterns(u8(texts[0]), rng, 12, [1, 2, 3, 9])] + [b"", b"a", b"\x00", b"\xff" * 128]
    classes = [exact_classes(p) for p in pats]
    limit_b = np.array(sizes, dtype=np.int64)

    def contained(what, cls):
        for max_hits in (50000, 7):
            occ, recs, total, cut = gpu_near(ctx, d_bwt, sizes, idx, loc, step, cls, k, max_hits, limit)
            assert (occ >= 0).all() and (occ <= limit_b[None, :]).all() and total == occ.sum() and 0 <= cut <= occ.size, what
            assert len(recs) == min(total, max_hits), what
            assert (recs["pattern"] < len(cls)).all() and (recs["block"] < len(sizes)).all() and (recs["cost"] <= k).all(), what
            nb = limit_b[recs["block"].astype(np.int64)]
            assert ((recs["position"] < nb) | (recs["position"] == FM_NO_HIT)).all(), what
        occ, recs, total, cut = gpu_near(ctx, d_bwt, [sum(sizes)], idx, loc, step, cls, k, 50000, limit)  # the same words as one block's structures
        assert ((recs["position"] < sum(sizes)) | (recs["position"] == FM_NO_HIT)).all() and (recs["cost"] <= k).all(), what
        assert (recs["pattern"] < len(cls)).all() and not recs["block"].any(), what

    def noise(n):
        return torch.from_numpy(rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.int32))
    contained("good structures", classes)
    loc.t.copy_(noise(len(loc.host())))
    contained("a random d_loc", classes)
    idx.t.copy_(noise(len(idx.host())))
    contained("a random index as well", classes)
    contained("and random classes", [rng.integers(0, 256, size=(len(p), 32), dtype=np.uint8) for p in pats])


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------------------------

def test_arguments(ctx):
    t = b"banana" * 50
    n = len(t)
    pats = [b"ana", b"nab", b"x"]
    classes = [exact_classes(p) for p in pats]
    pack = make_pack(ctx, [t], 8)
    d_bwt, idx, loc = pack[0], pack[1], pack[2]
    d_cls, lens = dev_classes(classes)
    hits, occ = Words(4 * 16), Words(3)
    lib, h = ctx._lib, ctx._h
    p_bwt, p_idx, p_loc, p_cls, p_hits, p_occ = (C.c_void_p(x.data_ptr()) for x in (d_bwt, idx.t, loc.t, d_cls, hits.t, occ.t))
    ns, ls, total, cut = (C.c_size_t * 1)(n), (C.c_size_t * 3)(*lens), C.c_uint64(99), C.c_uint64(98)
    tot, ct = C.byref(total), C.byref(cut)
    long_ls = (C.c_size_t * 3)(3, FM_NEAR_MAX_PATTERN + 1, 1)

    def off(x, nbytes):
        return C.c_void_p(x.t.data_ptr() + nbytes)

    def good():
        check(ctx, pack, classes, 1)
    good()
    #        bwt    n  index  loc  step cls   npat lens k limit max_hits hits occ total cut
    ok = [p_bwt, n, p_idx, p_loc, 8, p_cls, 3, ls, 1, 0, 16, p_hits, p_occ, tot, ct]
    bad = {0: [None], 1: [0, CAP + 1], 2: [None, off(idx, 2)], 3: [None, off(loc, 2)], 4: [0, 12, 8192], 5: [None], 6: [(1 << 24) + 1], 7: [None, long_ls],
           8: [4, 1 << 31], 10: [(1 << 31) + 1], 11: [None, off(hits, 8), off(hits, 4)], 12: [off(occ, 2)], 13: [None]}
    for at, values in sorted(bad.items()):
        for v in values:
            args = list(ok)
            args[at] = v
            assert lib.dk_dev_fm_near(h, *args) == DK_E_ARG, (at, v)
            assert lib.dk_dev_fm_near_packed(h, args[0], 1, ns if args[1] == n else (C.c_size_t * 1)(args[1]), *args[2:]) == DK_E_ARG, (at, v)
    assert lib.dk_dev_fm_near(h, *(ok[:8] + [4] + ok[9:])) == DK_E_ARG and "DK_FM_NEAR_MAX_K" in lib.dk_last_error(h).decode()
    assert lib.dk_dev_fm_near(h, *(ok[:7] + [long_ls] + ok[8:])) == DK_E_ARG and "DK_FM_NEAR_MAX_PATTERN" in lib.dk_last_error(h).decode()
    assert lib.dk_dev_fm_near_packed(h, p_bwt, 1, None, *ok[2:]) == DK_E_ARG and lib.dk_dev_fm_near_packed(h, p_bwt, 0, ns, *ok[2:]) == DK_E_ARG
    many = (C.c_size_t * 4097)(*([1] * 4097))  # 4097 blocks x 4096 patterns: one block more than DK_FM_FIND_MAX_PAIRS pairs
    assert lib.dk_dev_fm_near_packed(h, p_bwt, 4097, many, p_idx, p_loc, 8, p_cls, 4096, (C.c_size_t * 4096)(), 1, 0, 16, p_hits, p_occ, tot, ct) == DK_E_ARG
    assert "DK_FM_FIND_MAX_PAIRS" in lib.dk_last_error(h).decode()
    assert total.value == 99 and cut.value == 98 and hits.untouched() and occ.untouched()
    # what is allowed: counting without d_hits, d_loc and cut; only empty patterns without d_cls; no patterns at all
    assert lib.dk_dev_fm_near(h, p_bwt, n, p_idx, None, 8, p_cls, 3, ls, 1, 0, 0, None, p_occ, tot, None) == 0 and total.value == near_model([t], classes, 1)[2]
    assert lib.dk_dev_fm_near(h, p_bwt, n, p_idx, None, 8, None, 2, (C.c_size_t * 2)(0, 0), 3, 0, 0, None, None, tot, ct) == 0 and total.value == 2 * n
    assert lib.dk_dev_fm_near(h, p_bwt, n, p_idx, p_loc, 8, None, 0, ls, 0, 0, 16, p_hits, p_occ, tot, ct) == 0 and total.value == 0 and cut.value == 0
    good()
    # a workspace that cannot hold 16 bytes per pair; the context serves a good call afterwards
    with dark_amd.Context(1000, purpose="decoder") as small:
        npat = small.stats()["ws_size_bytes"] // 16 + 1
        spack = make_pack(small, [t], 8)
        for max_hits in (0, 4):
            with pytest.raises(dark_amd.DarkError) as e:
                gpu_near(small, spack[0], [n], spack[1], spack[2], 8, [exact_classes(b"a")] * npat, 1, max_hits)
            assert e.value.code == DK_E_ARG and "workspace" in str(e.value)
        check(small, spack, classes, 1)
    good()


# ---- decoder contexts sized to their input -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("purpose", ["decoder", "full"])
def test_contexts_sized_to_their_input(purpose):
    rng = np.random.default_rng(141)
    for n in (1, 1025):
        t = bytes(rng.integers(97, 101, size=n, dtype=np.uint8))
        classes = [exact_classes(p) for p in (b"", b"a", b"ab", t[:5], t[-3:], b"zz")]
        with dark_amd.Context(n, purpose=purpose) as exact:
            check(exact, make_pack(exact, [t], 32), classes, 1, what="%s, n = %d:" % (purpose, n))
            st = exact.stats()
            assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], (purpose, n, st)
    texts = [bytes(rng.integers(97, 100, size=700, dtype=np.uint8)) for _ in range(4)]
    classes = [exact_classes(p) for p in (b"", b"ab", b"abc", b"cab", b"d")]
    with dark_amd.Context(2800, purpose=purpose, max_blocks=4) as exact:
        pack = make_pack(exact, texts, 32)
        check(exact, pack, classes, 2, what="%s, the pack:" % purpose)
        st = exact.stats()
        assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], (purpose, st)
        if purpose == "decoder":
            with pytest.raises(dark_amd.DarkError) as e:  # five blocks on a context made for four
                gpu_near(exact, pack[0], [560] * 5, pack[1], pack[2], 32, classes, 1, 4)
            assert e.value.code == DK_E_ARG
            for b in range(4):
                L, origin = block_structures(texts[b])[1:]
                assert bytes(exact.bwt_inverse(L, origin)) == texts[b]  # what the context was made for, after the queries


# ---- the layer above -----------------------------------------------------------------------------------------------------------------------------------------

def test_index_class(ctx):
    texts = [wordlike(3000, s) for s in (1, 2)] + [b"a", b"abcabcabc"]
    low = texts[0].lower()
    pats = [low[:4], low[-5:], texts[1][:3], b"abc", b"a", b"\x00\x00"]
    parts = [block_structures(t) for t in texts]
    sizes, origins = [len(t) for t in texts], [p[2] for p in parts]
    d_L = dev_text(np.concatenate([p[1] for p in parts]))
    plain = fm.Index.from_bwt_packed(ctx, d_L, sizes, origins)
    for k, fold in ((0, False), (1, False), (0, True), (2, True)):
        cls = [fm.classes(p, ignore_case=fold) for p in pats]
        w_occ, w_recs, w_total, _, _ = near_model(texts, cls, k)
        occ, recs, total, cut = plain.near(pats, k, ignore_case=fold, max_hits=0)  # counting needs no locate structure
        assert total == w_total and cut == 0 and np.array_equal(occ, w_occ) and occ.dtype == np.uint32 and len(recs) == 0
    for call in (lambda: plain.near(pats, 1), lambda: plain.near_grep(pats, 1, 1, 1)):
        with pytest.raises(dark_amd.DarkError) as e:
            call()
        assert e.value.code == DK_E_ARG
    index = fm.Index.from_bwt_packed(ctx, d_L, sizes, origins, locate_step=8, extract_step=16)
    cls = [fm.classes(p, ignore_case=True) for p in pats]
    w_occ, w_recs, w_total, _, _ = near_model(texts, cls, 1)
    occ, recs, total, cut = index.near(pats, 1, ignore_case=True)
    assert total == w_total and cut == 0 and np.array_equal(occ, w_occ) and recs.dtype == FM_NEAR_HIT_DTYPE
    same_records(recs, w_recs)
    same_records(index.near(None, 1, classes=cls)[1], w_recs)  # ready-made classes in place of the patterns
    same_records(index.near(pats, 1, ignore_case=True, max_hits=7)[1], w_recs[:7])
    limited = index.near(pats, 1, ignore_case=True, node_limit=3)
    assert limited[3] > 0 and limited[2] < w_total
    assert index.near([])[2:] == (0, 0) and index.near_grep([], 3, 3) == []
    for before, after in ((5, 7), (0, 0), (4000, 4000)):  # against a slicing loop
        got = index.near_grep(pats, before, after, 1, ignore_case=True)
        assert len(got) == w_total
        for (q, b, at, cost, text), r in zip(got, w_recs):
            assert (q, b, at, cost) == (int(r["pattern"]), int(r["block"]), int(r["position"]), int(r["cost"]))
            assert text == texts[b][max(at - before, 0):at + len(pats[q]) + after], (q, b, at, before, after)
    assert len(index.near_grep(pats, 2, 2, 1, max_hits=3)) == 3
    wild = index.near([b"ab?abc"], wildcard=ord("?"))
    assert wild[2] == 2 and wild[1].tolist() == [(0, 3, 3, 0), (0, 3, 0, 0)]  # (one leaf, "abcabc": its slots in suffix order)
    one = fm.Index.from_bwt(ctx, parts[0][1], origins[0], locate_step=32, extract_step=32)  # a single block: the single entry
    same_records(one.near(pats, 1, ignore_case=True)[1], w_recs[w_recs["block"] == 0])


# ---- a poisoned workspace behind a poisoned mailbox ------------------------------------------------------------------------------------------------------

def test_poisoned_workspace_and_mailbox():
    """one run in a fresh process on the tuning build with DK_POISON=165, every call behind dk_dbg_mail_fill(165): tests/fm_near_poison_worker.py"""
    assert os.path.exists(TUNING_LIB), "build the tuning library: python dark_amd/build.py --tuning (__graft_entry__.build() does)"
    env = {k: v for k, v in os.environ.items() if not k.startswith("DK_")}
    env.update(DARK_AMD_LIB=TUNING_LIB, DK_POISON="165")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fm_near_poison_worker.py"), "fm_near", "165"], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=TIMEOUT)
    assert p.returncode == 0, "exit status %d\n%s" % (p.returncode, (p.stdout + p.stderr)[-3000:])
    report = json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    assert report["byte"] == 165 and report["contexts"] == 2 and report["fills"] > 0 and report["peeks"] >= 12 * report["contexts"], report
