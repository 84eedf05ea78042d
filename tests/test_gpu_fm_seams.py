"""The FM-index's seams on the GPU (csrc/fm_index.hip k_fm_seam_*): dk_dev_fm_seams / dk_dev_fm_seams_packed,
fm.Index.seams / tail and the C++ mirror.  Every pattern at every border of a pack, with the bytes carried over from the text in front; the
answer is the occurrence matrix, the 64-bit total and one compact list of records (pattern, block, back, 0) in the order (pattern, block, back
descending).  The yardstick is tests/fm_seams_model.py (brute force over the concatenation).  Every device output sits between guard words of
256 bytes (test_gpu_lcp.Words), and the hit buffer is pre-filled with the guard value, so a record written behind the list shows."""
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
from dark_amd._lib import DK_E_ARG, FM_SEAM_MAX_PATTERN
from dark_amd.context import FM_SEAM_HIT_DTYPE
from fm_find_model import block_structures
from fm_seams_model import found, seams_model
from test_gpu_fm import gpu_index, words
from test_gpu_fm_extract import gpu_anchors
from test_gpu_lcp import FILL, Words, dev_text, u8
from test_gpu_sa_search import dev_patterns

pytestmark = pytest.mark.gpu
CAP = (1 << 20) + 4096
TIMEOUT = 120
TUNING_LIB = os.path.join(ROOT, "dark_amd", "libdark_amd_tuning.so")


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


def gpu_seams(ctx, d_bwt, sizes, idx, ext, step, prev, patterns, max_hits, packed=None, want_occ=True):
    """-> (occ: npat x count int64 or None, the first min(total, max_hits) records, total).  packed: take the packed entry (default: for more
    than one block).  Checks that nothing but those records was written to the hit buffer or around any output."""
    count, npat = len(sizes), len(patterns)
    d_pat, lens = dev_patterns(patterns)
    d_prev = dev_text(u8(prev)) if len(prev) else None
    hits = Words(4 * max_hits)
    occ = Words(npat * count) if want_occ else None
    args = (idx.t, ext.t, step, d_prev, d_pat, lens, max_hits, hits.t if max_hits else None, occ.t if want_occ else None)
    if count > 1 if packed is None else packed:
        total = ctx.dev_fm_seams_packed(d_bwt, sizes, *args)
    else:
        total = ctx.dev_fm_seams(d_bwt, sizes[0], *args)
    got = min(total, max_hits)
    raw = hits.host()
    assert hits.guards_intact() and (raw[4 * got:] == FILL).all(), "a record behind the first %d of %d (max_hits %d)" % (got, total, max_hits)
    assert idx.guards_intact() and ext.guards_intact() and (occ is None or occ.guards_intact()), "a store left the outputs"
    return (occ.host().astype(np.int64).reshape(npat, count) if want_occ else None), raw[:4 * got].view(FM_SEAM_HIT_DTYPE), total


def same_records(got, want, what=""):
    assert len(got) == len(want), "%s %d records, expected %d" % (what, len(got), len(want))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s record %d: %s, expected %s (%d wrong)" % (what, bad[0], got[bad[0]], want[bad[0]], bad.size)


def pack_of(ctx, texts, step, shift=0):
    """L and origins from sorted suffixes (no GPU sort in the way), the index and the extract structure"""
    parts = [block_structures(t) for t in texts]
    sizes, origins = [len(p[1]) for p in parts], [p[2] for p in parts]
    d_bwt, idx = gpu_index(ctx, np.concatenate([p[1] for p in parts]), sizes, origins, shift)
    return d_bwt, idx, gpu_anchors(ctx, d_bwt, sizes, origins, step), sizes


def check(ctx, pack, texts, pats, prev, step, fast=False, what=""):
    d_bwt, idx, ext, sizes = pack
    want_occ, want, want_total = seams_model(texts, pats, prev, fast=fast)
    occ, recs, total = gpu_seams(ctx, d_bwt, sizes, idx, ext, step, prev, pats, want_total + 1)
    assert total == want_total, "%s total %d, model %d" % (what, total, want_total)
    assert np.array_equal(occ, want_occ), "%s occ differs at %s" % (what, np.argwhere(occ != want_occ)[:4].tolist())
    same_records(recs, want, what)
    return want_occ, want, want_total


# ---- every short text as a block of one pack, every short pattern ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def short(ctx):
    texts, pats = words(b"ab", range(1, 9)), words(b"ab", range(0, 7))
    assert len(texts) == 510 and len(pats) == 127
    return dict(texts=texts, pats=pats, pack=pack_of(ctx, texts, 2))


@pytest.mark.parametrize("prev", [b"", b"a", b"abab", b"bbbbb"])
def test_every_short_text_in_one_pack(ctx, short, prev):
    s = short
    want_occ, want, want_total = check(ctx, s["pack"], s["texts"], s["pats"], prev, 2, what="prev %r:" % prev)
    assert want_total > 5000 and (want_occ[:, 0].any() == bool(prev))


# ---- one-byte blocks: matches that span many borders, candidates at the edge of 64 lanes ----------------------------------------------------------------

@pytest.mark.parametrize("kind", ["abab", "aaaa"])
def test_tiny_blocks(ctx, kind):
    texts = [b"a" if kind == "aaaa" or i % 2 == 0 else b"b" for i in range(300)]
    whole = b"".join(texts)
    lens = (2, 3, 64, 65, 66, 130)
    pats = [whole[a:a + m] for m in lens for a in (0, 1)]
    pack = pack_of(ctx, texts, 1)
    for prev in (b"", whole[-129:] if kind == "aaaa" else b"b" + whole[:128]):
        want_occ, want, _ = check(ctx, pack, texts, pats, prev, 1, what="%s prev %d:" % (kind, len(prev)))
        # a match of 130 bytes crosses 129 borders and belongs to the last one; in a block of one byte back = m - 1
        assert want_occ[2 * lens.index(130)].sum() > 0 and set(want["back"].tolist()) == {1, 2, 63, 64, 65, 129}


# ---- block sizes around the strip's cases ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("longest", [5, 66])
@pytest.mark.parametrize("kind", ["period3", "random4"])
def test_block_sizes_around_the_strip(ctx, longest, kind):
    """n_b in {W - 1, W, W + 1, 2W - 1, 2W, 2W + 1, 5W}: whole blocks, blocks whose head and tail touch, blocks with a gap; every ordered pair of
    them as neighbours"""
    W = longest - 1
    kinds = [W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 5 * W]
    sizes = [n for a in kinds for b in kinds for n in (a, b)]
    assert {(a, b) for a, b in zip(sizes, sizes[1:])} >= {(a, b) for a in kinds for b in kinds}
    total = sum(sizes)
    rng = np.random.default_rng(longest)
    whole = (b"abc" * (total // 3 + 1))[:total] if kind == "period3" else bytes(rng.integers(97, 101, size=total, dtype=np.uint8))
    off = np.concatenate([[0], np.cumsum(sizes)])
    texts = [whole[off[b]:off[b + 1]] for b in range(len(sizes))]
    pats = []
    for m in sorted({2, 3, longest - 1, longest}):
        for b in rng.choice(np.arange(1, len(sizes)), size=6, replace=False):  # pieces of the text around a border: the border at every place inside them
            back = int(rng.integers(1, m))
            pats.append(whole[off[b] - back:off[b] - back + m])
    pats += [b"", b"a", whole[:longest], b"c" * longest]
    assert max(len(p) for p in pats) == longest
    pack = pack_of(ctx, texts, 4)
    for prev in (b"", whole[-W:], whole[-(W + 7):]):
        want_occ, _, want_total = check(ctx, pack, texts, pats, prev, 4, fast=True, what="%s longest %d prev %d:" % (kind, longest, len(prev)))
        assert want_total >= 24 and (kind != "period3" or (want_occ.sum(axis=0)[1:] > 0).all())


# ---- one symbol ------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ones(ctx):
    texts = [b"a" * 100] * 8
    pats = [b"a" * m for m in (2, 64, 65, 100, 101, 250)]
    want_occ, want, want_total = seams_model(texts, pats)
    return dict(texts=texts, pats=pats, pack=pack_of(ctx, texts, 32), occ=want_occ.astype(np.int64), recs=want, total=want_total)


def test_one_symbol(ctx, ones):
    o = ones
    # at block b >= 1 a^m has min(m - 1, 100 b) - max(1, m - 100) + 1 places: its last byte lies among the block's 100
    by_hand = [[0] + [max(min(m - 1, 100 * b) - max(1, m - 100) + 1, 0) for b in range(1, 8)] for m in (2, 64, 65, 100, 101, 250)]
    assert o["occ"].tolist() == by_hand and by_hand[5][1:4] == [0, 51, 100]
    d_bwt, idx, ext, sizes = o["pack"]
    occ, recs, total = gpu_seams(ctx, d_bwt, sizes, idx, ext, 32, b"", o["pats"], o["total"])
    assert total == o["total"] and np.array_equal(occ, o["occ"])
    same_records(recs, o["recs"])


@pytest.mark.parametrize("which", ["0", "1", "total - 1", "total", "total + 1"])
def test_truncation(ctx, ones, which):
    o = ones
    d_bwt, idx, ext, sizes = o["pack"]
    max_hits = {"0": 0, "1": 1, "total - 1": o["total"] - 1, "total": o["total"], "total + 1": o["total"] + 1}[which]
    occ, recs, total = gpu_seams(ctx, d_bwt, sizes, idx, ext, 32, b"", o["pats"], max_hits)
    assert total == o["total"] and np.array_equal(occ, o["occ"])
    same_records(recs, o["recs"][:max_hits], "max_hits = %s:" % which)  # (gpu_seams has looked at everything behind them)
    _, recs, total = gpu_seams(ctx, d_bwt, sizes, idx, ext, 32, b"", o["pats"], max_hits, want_occ=False)  # d_occ is optional
    assert total == o["total"]
    same_records(recs, o["recs"][:max_hits])


# ---- the invariant on real paths: find + seams = every occurrence ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wordy():
    n = 1 << 18
    t = bytes(u8(datagen.word_like(n, seed=5, vocab=2000, alpha=26)))
    rng = np.random.default_rng(77)
    pats = []
    for k in range(64):
        m = int(rng.integers(2, 41))
        if k % 2:  # centred on a border of the pack of 16 (which is a border of the pack of 4096 too)
            a = int(rng.integers(1, 16)) * (n // 16) - m // 2
        else:
            a = int(rng.integers(0, n - m))
        pats.append(t[a:a + m])
    return dict(t=t, n=n, pats=pats, counts=[len(found(t, p)) for p in pats])  # (computed once; nothing below changes it)


@pytest.mark.parametrize("count", [16, 4096])
def test_find_and_seams_are_every_occurrence(ctx, wordy, count):
    w = wordy
    n = w["n"]
    sizes = [n // count] * count
    d_L = torch.empty(n, dtype=torch.uint8, device="cuda")
    origins = ctx.dev_bwt_forward_packed(dev_text(u8(w["t"])), sizes, d_L)
    d_bwt, idx = gpu_index(ctx, d_L.cpu().numpy(), sizes, origins)
    ext = gpu_anchors(ctx, d_bwt, sizes, origins, 32)
    d_pat, lens = dev_patterns(w["pats"])
    inside = Words(64 * count)
    ctx.dev_fm_find_packed(d_bwt, sizes, idx.t, None, 32, d_pat, lens, 0, None, inside.t)
    texts = [w["t"][b * sizes[0]:(b + 1) * sizes[0]] for b in range(count)]
    occ, recs, total = gpu_seams(ctx, d_bwt, sizes, idx, ext, 32, b"", w["pats"], 1 << 16)
    assert total < 1 << 16
    assert (inside.host().astype(np.int64).reshape(64, count).sum(axis=1) + occ.sum(axis=1)).tolist() == w["counts"]
    assert all(occ[q].sum() > 0 for q in range(1, 64, 2))  # the patterns cut across a border are found there
    # the same pack behind an earlier copy of the text: its last 39 bytes are carried over
    prev = w["t"][-39:]
    want_occ, want, want_total = seams_model(texts, w["pats"], prev, fast=True)
    occ, recs, total = gpu_seams(ctx, d_bwt, sizes, idx, ext, 32, prev, w["pats"], want_total + 1)
    assert total == want_total and np.array_equal(occ, want_occ)
    same_records(recs, want)
    first = np.arange(count, dtype=np.int64) * sizes[0]
    starts = first[recs["block"]] - recs["back"].astype(np.int64)  # in the text; negative: in prev
    both = prev + w["t"]
    for q in range(64):
        mine = starts[recs["pattern"] == q] + len(prev)
        p = w["pats"][q]
        assert all(both[a:a + len(p)] == p for a in mine.tolist()) and len(set(mine.tolist())) == len(mine)


# ---- the single form -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("step", [1, 32, 4096])
def test_single_form_equals_the_pack_of_one(ctx, step):
    t = bytes(u8(datagen.wiki_like(5000, seed=3)))
    prev = bytes(u8(datagen.wiki_like(5000, seed=4)))[-60:] + t[:3]
    pats = [prev[-a:] + t[:b] for a in (1, 2, 7, 40, 63) for b in (1, 3, 30)] + [b"", t[:9], prev, prev + t[:4000], b"e ", b" t"]
    assert max(len(p) for p in pats) == 4063  # just below DK_FM_SEAM_MAX_PATTERN
    pack = pack_of(ctx, [t], step, shift=1)
    d_bwt, idx, ext, sizes = pack
    want_occ, want, want_total = seams_model([t], pats, prev, fast=True)
    assert want_total >= 15 and (want["block"] == 0).all()
    for packed in (False, True):
        occ, recs, total = gpu_seams(ctx, d_bwt, sizes, idx, ext, step, prev, pats, want_total + 3, packed=packed)
        assert total == want_total and np.array_equal(occ, want_occ)
        same_records(recs, want, "packed %s, step %d:" % (packed, step))
        assert gpu_seams(ctx, d_bwt, sizes, idx, ext, step, b"", pats, 4, packed=packed)[2] == 0  # no prev, no border


def test_no_patterns_and_patterns_too_short(ctx):
    d_bwt, idx, ext, sizes = pack_of(ctx, [b"abab", b"b"], 2)
    for packed, ns in ((True, sizes), (False, [5])):
        occ, recs, total = gpu_seams(ctx, d_bwt, ns, idx, ext, 2, b"ab", [], 4, packed=packed)
        assert total == 0 and len(recs) == 0 and occ.size == 0
        occ, recs, total = gpu_seams(ctx, d_bwt, ns, idx, ext, 2, b"ab", [b"", b"a", b"b"], 4, packed=packed)
        assert total == 0 and len(recs) == 0 and not occ.any()


# ---- structures that are none ----------------------------------------------------------------------------------------------------------------------

def test_containment(ctx):
    """any words in d_ext, then in the index too, then any bytes in d_prev: DK_OK, every field of every record inside its bound, guards intact"""
    rng = np.random.default_rng(171)
    step = 4
    texts = [bytes(u8(datagen.wiki_like(2500, seed=3))), b"a", b"ab", bytes(rng.integers(97, 99, size=1000, dtype=np.uint8)), b"a" * 594]
    d_bwt, idx, ext, sizes = pack_of(ctx, texts, step)
    whole = b"".join(texts)
    cuts = np.cumsum(sizes)[:-1]
    pats = [whole[c - a:c + b] for c in cuts.tolist() for a, b in ((1, 1), (2, 5), (30, 40))] + [b"aa", b"ab", b"a" * 300, b"", b"\x00\x00"]
    plen = np.array([len(p) for p in pats], dtype=np.int64)
    prev = bytearray(b"xyz" + whole[-20:])

    def contained(what):
        for max_hits in (50000, 7):
            occ, recs, total = gpu_seams(ctx, d_bwt, sizes, idx, ext, step, bytes(prev), pats, max_hits)
            assert (occ >= 0).all() and (occ < np.maximum(plen, 1)[:, None]).all() and total == occ.sum(), what
            assert len(recs) == min(total, max_hits), what
            assert (recs["pattern"] < len(pats)).all() and (recs["block"] < len(sizes)).all() and not recs["reserved"].any(), what
            assert (recs["back"] >= 1).all() and (recs["back"] < plen[recs["pattern"].astype(np.int64)]).all(), what
        return total

    def noise(k):
        return torch.from_numpy(rng.integers(0, 1 << 32, size=k, dtype=np.uint64).astype(np.uint32).view(np.int32))
    good = contained("good structures")
    assert good == seams_model(texts, pats, bytes(prev), fast=True)[2] > 10
    ext.t.copy_(noise(ext.n))
    contained("a random d_ext")
    idx.t.copy_(noise(idx.n))
    contained("both random")
    prev[:] = bytes(rng.integers(0, 256, size=len(prev), dtype=np.uint8))
    contained("a random prev as well")


# ---- arguments -------------------------------------------------------------------------------------------------------------------------------------

def test_arguments(ctx):
    t = b"banana" * 50
    n = len(t)
    prev = b"bana"
    pats = [b"anab", b"nab", b"x"]
    d_bwt, idx, ext, _ = pack_of(ctx, [t], 8)
    want_occ, want, want_total = seams_model([t], pats, prev)
    assert want_total == 2
    d_pat, lens = dev_patterns(pats)
    d_prev = dev_text(u8(prev))
    hits, occ = Words(4 * 16), Words(3)
    lib, h = ctx._lib, ctx._h
    p_bwt, p_idx, p_ext, p_prev, p_pat, p_hits, p_occ = (C.c_void_p(x.data_ptr()) for x in (d_bwt, idx.t, ext.t, d_prev, d_pat, hits.t, occ.t))
    ns, ls, total = (C.c_size_t * 1)(n), (C.c_size_t * 3)(*lens), C.c_uint64(99)
    tot = C.byref(total)

    def off(x, k):
        return C.c_void_p(x.t.data_ptr() + k)

    def good():
        occ_g, recs, got = gpu_seams(ctx, d_bwt, [n], idx, ext, 8, prev, pats, 16)
        assert got == want_total and np.array_equal(occ_g, want_occ)
        same_records(recs, want[:16])
    good()
    too_long = (C.c_size_t * 3)(4, FM_SEAM_MAX_PATTERN + 1, 1)
    # (d_bwt, n, d_index, d_ext, step, d_prev, prev_len, d_pat, npat, pat_len, max_hits, d_hits, d_occ, total)
    ok = [p_bwt, n, p_idx, p_ext, 8, p_prev, 4, p_pat, 3, ls, 16, p_hits, p_occ, tot]
    changes = [(0, None), (2, None), (3, None), (7, None), (9, None), (11, None), (13, None), (1, 0), (1, CAP + 1), (2, off(idx, 2)), (3, off(ext, 2)),
               (11, off(hits, 8)), (11, off(hits, 4)), (12, off(occ, 2)), (4, 0), (4, 12), (4, 8192), (10, (1 << 31) + 1), (8, (1 << 24) + 1),
               (5, None), (6, FM_SEAM_MAX_PATTERN), (9, too_long)]
    for at, value in changes:
        args = list(ok)
        args[at] = value
        assert lib.dk_dev_fm_seams(h, *args) == DK_E_ARG, (at, value)
        sizes = ns if args[1] == n else (C.c_size_t * 1)(args[1])
        assert lib.dk_dev_fm_seams_packed(h, args[0], 1, sizes, *args[2:]) == DK_E_ARG, (at, value)
    assert "DK_FM_SEAM_MAX_PATTERN" in lib.dk_last_error(h).decode()
    counting = list(ok)
    counting[10], counting[11], counting[13] = 0, None, None  # max_hits == 0 still needs `total`
    assert lib.dk_dev_fm_seams(h, *counting) == DK_E_ARG
    assert lib.dk_dev_fm_seams_packed(h, p_bwt, 1, None, *ok[2:]) == DK_E_ARG
    assert lib.dk_dev_fm_seams_packed(h, p_bwt, 0, ns, *ok[2:]) == DK_E_ARG
    # 4097 blocks x 4096 patterns: one block more than DK_FM_FIND_MAX_PAIRS pairs (refused before the patterns are looked at)
    many = (C.c_size_t * 4097)(*([1] * 4097))
    assert lib.dk_dev_fm_seams_packed(h, p_bwt, 4097, many, p_idx, p_ext, 8, p_prev, 4, p_pat, 4096, (C.c_size_t * 4096)(), 16, p_hits, p_occ, tot) == DK_E_ARG
    assert "DK_FM_FIND_MAX_PAIRS" in lib.dk_last_error(h).decode()
    assert total.value == 99 and hits.untouched() and occ.untouched()
    # prev_len just below the bound is served (only its last bytes can matter)
    long_prev = b"q" * (FM_SEAM_MAX_PATTERN - 1 - len(prev)) + prev
    occ_g, recs, got = gpu_seams(ctx, d_bwt, [n], idx, ext, 8, long_prev, pats, 16)
    assert got == want_total and np.array_equal(occ_g, want_occ)
    good()
    # a workspace that cannot hold 16 bytes per pair; the context serves a good call afterwards
    with dark_amd.Context(1000, purpose="decoder") as small:
        size = small.stats()["ws_size_bytes"]
        npat = size // 16 + 1
        sd_bwt, sidx, sext, _ = pack_of(small, [t], 8)
        for max_hits in (0, 4):
            with pytest.raises(dark_amd.DarkError) as e:
                gpu_seams(small, sd_bwt, [n], sidx, sext, 8, prev, [b"ab"] * npat, max_hits)
            assert e.value.code == DK_E_ARG and "workspace" in str(e.value)
        occ_g, recs, got = gpu_seams(small, sd_bwt, [n], sidx, sext, 8, prev, pats, 16)
        assert got == want_total and np.array_equal(occ_g, want_occ)
        same_records(recs, want[:16])
    good()


# ---- decoder contexts, and the workspace ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("purpose", ["decoder", "full"])
def test_contexts_sized_to_their_input(ctx, purpose):
    rng = np.random.default_rng(141)
    for n in (1, 2, 1025):
        t = bytes(rng.integers(97, 99, size=n, dtype=np.uint8))
        prev = b"abba" + t[-2:]
        pats = [b"", b"a", b"ab", b"ba", prev[-3:] + t[:3], prev + t, b"zz"]
        with dark_amd.Context(n, purpose=purpose) as exact:
            check(exact, pack_of(exact, [t], 32), [t], pats, prev, 32, what="%s n = %d:" % (purpose, n))
            st = exact.stats()
            assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], (purpose, n, st)
    texts = [bytes(rng.integers(97, 100, size=n, dtype=np.uint8)) for n in (2000, 1, 3, 1996)]
    whole = b"".join(texts)
    around = [whole[c - a:c + b] for c in (2000, 2001, 2004) for a, b in ((1, 1), (2, 3))]  # pieces of the text around its three borders
    pats = [b"", b"ab"] + around + [texts[0][-5:] + texts[1] + texts[2] + texts[3][:4], b"d", b"ca" + whole[:2]]
    with dark_amd.Context(4000, purpose=purpose, max_blocks=4) as exact:
        pack = pack_of(exact, texts, 32)
        _, _, want_total = check(exact, pack, texts, pats, b"ca", 32, what="%s pack:" % purpose)
        assert want_total >= 8  # every piece where it was cut, the long pattern over all three borders, the one against prev
        st = exact.stats()
        assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], (purpose, st)
        if purpose == "decoder":
            d_bwt, idx, ext, _ = pack
            with pytest.raises(dark_amd.DarkError) as e:  # five blocks on a context made for four
                gpu_seams(exact, d_bwt, [800] * 5, idx, ext, 32, b"", pats, 4)
            assert e.value.code == DK_E_ARG
            for b in range(4):
                L, origin = block_structures(texts[b])[1:]
                assert bytes(exact.bwt_inverse(L, origin)) == texts[b]  # what the context was made for, after the queries


# ---- the layers above ------------------------------------------------------------------------------------------------------------------------------------

def test_index_class(ctx):
    texts = [bytes(u8(datagen.wiki_like(3000, seed=s))) for s in (1, 2)] + [b"a", b"abcabcabc"]
    whole = b"".join(texts)
    prev = b"the quick brown fox " + texts[0][:2]
    pats = [whole[2998:3003], whole[5990:6004], b"aabc", prev[-4:] + whole[:3], b"a", b"\x00\x00", whole[5999:6010]]
    want_occ, want, want_total = seams_model(texts, pats, prev, fast=True)
    assert want_total >= 5
    parts = [block_structures(t) for t in texts]
    sizes, origins = [len(t) for t in texts], [p[2] for p in parts]
    d_L = dev_text(np.concatenate([p[1] for p in parts]))
    plain = fm.Index.from_bwt_packed(ctx, d_L, sizes, origins, locate_step=8)
    for call in (lambda: plain.seams(pats), lambda: plain.tail(3)):
        with pytest.raises(dark_amd.DarkError) as e:
            call()
        assert e.value.code == DK_E_ARG
    index = fm.Index.from_bwt_packed(ctx, d_L, sizes, origins, extract_step=16)
    occ, recs, total = index.seams(pats, prev)
    assert total == want_total and np.array_equal(occ, want_occ) and occ.dtype == np.uint32 and recs.dtype == FM_SEAM_HIT_DTYPE
    same_records(recs, want)
    occ, recs, total = index.seams(pats, b"x" * 5000 + prev, max_hits=3)  # a long prev: only its last bytes are uploaded
    assert total == want_total and np.array_equal(occ, want_occ)
    same_records(recs, want[:3])
    occ, recs, total = index.seams(pats, prev, max_hits=0)
    assert total == want_total and len(recs) == 0
    assert index.seams([])[2] == 0 and index.seams([], prev)[0].shape == (0, 4)
    n = len(whole)
    for nbytes in (0, 1, 9, 10, 11, 3015, n - 1, n, n + 1, 3 * n):  # below, equal to and above the blocks' ends and the total
        assert index.tail(nbytes) == (whole[-nbytes:] if 0 < nbytes < n else whole if nbytes else b""), nbytes
    one = fm.Index.from_bwt(ctx, parts[0][1], origins[0], extract_step=32)  # a single block: its only border is the one against prev
    occ, recs, total = one.seams(pats, prev)
    w1_occ, w1, w1_total = seams_model(texts[:1], pats, prev, fast=True)
    assert total == w1_total == 1 and np.array_equal(occ, w1_occ)
    same_records(recs, w1)
    assert one.tail(7) == texts[0][-7:] and one.tail(4000) == texts[0]


def test_cpp_mirror(tmp_path):
    exe = str(tmp_path / "cpp_fm_seams")
    lib_dir = os.path.join(ROOT, "dark_amd")
    # as tests/cpp_fm_find.cpp is built, and the HIP runtime besides: the entry has no host-memory form, so the mirror holds device memory
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp_fm_seams.cpp"), "-L", lib_dir, "-ldark_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=TIMEOUT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cpp fm seams ok" in out.stdout


# ---- a poisoned workspace behind a poisoned mailbox --------------------------------------------------------------------------------------------------

def test_poisoned_workspace_and_mailbox():
    """one run in a fresh process on the tuning build with DK_POISON=165, every call behind dk_dbg_mail_fill(165): tests/fm_seams_poison_worker.py"""
    assert os.path.exists(TUNING_LIB), "build the tuning library: python dark_amd/build.py --tuning (__graft_entry__.build() does)"
    env = {k: v for k, v in os.environ.items() if not k.startswith("DK_")}
    env.update(DARK_AMD_LIB=TUNING_LIB, DK_POISON="165")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fm_seams_poison_worker.py"), "fm_seams", "165"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0, "exit status %d\n%s" % (p.returncode, (p.stdout + p.stderr)[-3000:])
    report = json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    assert report["byte"] == 165 and report["contexts"] == 2 and report["fills"] > 0 and report["peeks"] >= 12 * report["contexts"], report
