"""Matching statistics and super-maximal matches on the GPU (dk_dev_sa_match*, dk_dev_sa_smems*, their host forms; csrc/sa_query.hip, DESIGN.md
section 4.19).  Every answer must equal the plain model of tests/sa_match_model.py (pinned by tests/test_sa_match_model.py) on the suffix array
dev_suffix_array gives.  Every device output sits between GUARD words.  The tuning build moves the border between the two kernels in a
subprocess, and one more subprocess runs the stage on a poisoned workspace behind a poisoned mailbox."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dark_amd
from conftest import ROOT
from dark_amd import datagen
from dark_amd._lib import DK_E_ARG
from dark_amd.context import SA_SMEM_DTYPE
from sa_match_model import match_model, smems_model
from test_gpu_lcp import Words, dev_text, u8
from test_gpu_sa_search import dev_patterns, gpu_sa, put

pytestmark = pytest.mark.gpu
CAP = 1 << 17
LANE_MAX = 256  # csrc/sa_query.hip: SA_SEARCH_LANE_MAX, the border between k_sa_match and k_sa_match_long
SM_TILE = 1024  # csrc/sa_query.hip: positions in one tile of the scan of the flags
TUNING_LIB = os.path.join(ROOT, "dark_amd", "libdark_amd_tuning.so")
TIMEOUT = 120
ENTRIES = ("dk_dev_sa_match", "dk_dev_sa_match_packed", "dk_sa_match", "dk_dev_sa_smems", "dk_dev_sa_smems_packed", "dk_sa_smems")


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


# ---- the calls, between guards --------------------------------------------------------------------------------------------------------------------

def gpu_match(ctx, t, sa, queries, max_len, shifts=(0, 0, 0, 0, 0), ranges=True, pack=None):
    """(len, lo, hi) over the positions through dev_sa_match (pack = (sizes, blocks): dev_sa_match_packed); sa: a Words; shifts: of the text, the
    queries (bytes), len, lo and hi (elements).  ranges=False: d_lo and d_hi null, and lo / hi come back as None"""
    d_q, lens = dev_patterns(queries, shifts[1])
    total = sum(lens)
    out = [Words(total, s) for s in shifts[2:]]
    d_lo, d_hi = (out[1].t, out[2].t) if ranges else (None, None)
    if pack:
        ctx.dev_sa_match_packed(dev_text(t, shifts[0]), pack[0], sa.t, d_q, lens, pack[1], max_len, out[0].t, d_lo, d_hi)
    else:
        ctx.dev_sa_match(dev_text(t, shifts[0]), len(t), sa.t, d_q, lens, max_len, out[0].t, d_lo, d_hi)
    assert all(w.guards_intact() for w in out) and sa.guards_intact(), "a store left the outputs"
    if not ranges:
        assert out[1].untouched() and out[2].untouched()
        return out[0].host().astype(np.int64), None, None
    return tuple(w.host().astype(np.int64) for w in out)


def gpu_smems(ctx, t, sa, queries, min_len, max_len, max_hits, pack=None):
    """(records as rows of at, len, lo, hi; total) through dev_sa_smems(_packed); nothing behind the last record written may be touched"""
    d_q, lens = dev_patterns(queries)
    hits = Words(4 * max_hits)
    d_hits = hits.t if max_hits else None
    if pack:
        total = ctx.dev_sa_smems_packed(dev_text(t), pack[0], sa.t, d_q, lens, pack[1], min_len, max_len, max_hits, d_hits)
    else:
        total = ctx.dev_sa_smems(dev_text(t), len(t), sa.t, d_q, lens, min_len, max_len, max_hits, d_hits)
    listed = min(total, max_hits)
    rest = Words(4 * (max_hits - listed))
    assert hits.guards_intact() and sa.guards_intact() and np.array_equal(hits.host()[4 * listed:], rest.host()), "a store behind the last record"
    return hits.host()[:4 * listed].astype(np.int64).reshape(-1, 4), total


def flat_model(t, sa_host, queries, max_len):
    rows = [r for q in match_model(t, sa_host, queries, max_len) for r in q]
    return np.array(rows, np.int64).reshape(-1, 3)


def check(ctx, t, queries, max_len, shifts=(0, 0, 0, 0, 0), sa=None):
    t = u8(t)
    sa = sa or gpu_sa(ctx, t)
    got = np.stack(gpu_match(ctx, t, sa, queries, max_len, shifts), axis=1)
    want = flat_model(t, sa.host(), queries, max_len)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert got.shape == want.shape and bad.size == 0, "position %d: (len, lo, hi) = %s, model %s (n = %d, max_len = %d, %d wrong)" % (
        bad[0], got[bad[0]], want[bad[0]], len(t), max_len, bad.size)
    return got


def smem_rows(stats, queries, min_len, max_len):
    """the model's records from the statistics (rows of len, lo, hi over the positions)"""
    ends = np.cumsum([len(q) for q in queries])
    per_query = [stats[e - len(q):e, 0].tolist() for q, e in zip(queries, ends)]
    return np.array([(at, ln, stats[at, 1], stats[at, 2]) for at, ln in smems_model(per_query, min_len, max_len)], np.int64).reshape(-1, 4)


def check_smems(ctx, t, queries, max_len, min_lens=(0, 1, 12), sa=None, cuts=False):
    t = u8(t)
    sa = sa or gpu_sa(ctx, t)
    stats = flat_model(t, sa.host(), queries, max_len)
    wants = {}
    for min_len in min_lens:
        want = wants[min_len] = smem_rows(stats, queries, min_len, max_len)
        for max_hits in (len(want) + 1, 9, 0) if cuts else (len(want) + 1,):
            got, total = gpu_smems(ctx, t, sa, queries, min_len, max_len, max_hits)
            assert total == len(want), (min_len, max_len, max_hits, total, len(want))
            assert np.array_equal(got, want[:max_hits]), (min_len, max_len, max_hits)
    return wants


# ---- 1. depth of the 64-ary search ------------------------------------------------------------------------------------------------------------------

MAX_LENS = [1, 3, 255, 256, 257, 300, 1000]


def depth_case(n):
    rng = np.random.default_rng(n)
    lo, hi = (65, 69) if n == 1 << 16 else (97, 99)
    t = rng.integers(lo, hi, size=n, dtype=np.uint8)
    if n == 1 << 16:
        t = np.frombuffer(bytes(t).translate(bytes.maketrans(b"ABCD", b"ACGT")), np.uint8)
    a = int(rng.integers(0, max(1, n - 600)))
    sym = np.unique(t) if n > 2 else u8(b"ab")
    return t, [sym[rng.integers(0, len(sym), size=3000)], t[a:a + 600].copy()]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4097, 1 << 16])
def test_depths_of_the_search(ctx, n):
    t, queries = depth_case(n)
    sa = gpu_sa(ctx, t)
    for max_len in MAX_LENS:
        got = check(ctx, t, queries, max_len, sa=sa)
        if max_len <= min(n, 600):
            assert (got[:, 0] == max_len).any(), "no match reaches the cap %d" % max_len
        if max_len == 1000 and n >= 600:
            assert (got[:, 0] > LANE_MAX).any() and got[3000, 0] == 600  # through the cut: k_sa_match_long


# ---- 2. the whole-wave compare --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def markov_sa(ctx):
    t = u8(datagen.wiki_like(1 << 15, seed=3))
    return t, gpu_sa(ctx, t)


def long_copy_queries(t):
    copy = t[4000:6500].copy()
    queries = [np.concatenate([u8(b"\x00\x01"), copy, u8(b"\x02")])]
    for at in (1023, 1024, 1025):  # around the second step of 64 x 16 bytes
        q = copy.copy()
        q[at] = 0
        queries.append(q)
    return queries


def test_a_match_of_2500_bytes(ctx, markov_sa):
    t, sa = markov_sa
    got = check(ctx, t, long_copy_queries(t), 4096, sa=sa)
    assert got[2, 0] == 2500 and got[2503 + 0, 0] == 1023 and got[2503 + 2500, 0] == 1024 and got[2503 + 5000, 0] == 1025


# ---- 3. the ends of the text ------------------------------------------------------------------------------------------------------------------------

END_CASES = [(b"a" * 100, [b"a" * 150]), (b"a" * 99 + b"b", [b"a" * 120, b"a" * 50 + b"ba"]), (b"abcabd", [b"abz", b"z", b"dabc"])]


@pytest.mark.parametrize("max_len", [1, 7, 1000])
def test_ends_of_the_text(ctx, max_len):
    for t, queries in END_CASES:
        got = check(ctx, t, queries, max_len)
        ends = np.cumsum([len(q) for q in queries]) - 1
        assert (got[ends, 0] <= 1).all()  # the last position of every query: a window of one byte
    got = check(ctx, b"abcabd", [b"abz", b"z"], max_len)
    assert got[2].tolist() == [0, 0, 6] and got[3].tolist() == [0, 0, 6]  # a byte the text lacks: nothing matches, every slot
    if max_len == 1000:
        assert check(ctx, b"a" * 100, [b"a" * 150], max_len)[:52, 0].tolist() == [100] * 51 + [99]


# ---- 4. several queries back to back ------------------------------------------------------------------------------------------------------------------

def border_queries(t):
    """lengths 0, 1, 2, 700: the one-byte and the two-byte query end with the first bytes of a stretch whose rest opens the query behind them"""
    return [t[:0], t[500:501], t[501:503], t[503:1203]]


def test_queries_back_to_back(ctx, markov_sa):
    t, sa = markov_sa
    got = check(ctx, t, border_queries(t), 1000, sa=sa)
    assert got[:3, 0].tolist() == [1, 2, 1] and got[3, 0] == 700  # not 703, 702, 701: no match runs into the next query
    check(ctx, t, [t[:0], t[:0]] + border_queries(t) + [t[:0]], 5, sa=sa)


# ---- 5. packs -----------------------------------------------------------------------------------------------------------------------------------

def pack_case():
    rng = np.random.default_rng(31)
    blocks = [rng.integers(97, 100, size=n, dtype=np.uint8) for n in (1, 2, 63, 64, 65, 5000)]
    whole = blocks[5][1000:1300].copy()  # occurs whole in block 5 only
    queries, where = [], []
    for b in (0, 1, 2, 2, 3, 5):  # every block but 4 ... one of them twice
        queries.append(np.concatenate([blocks[b][:40], rng.integers(97, 101, size=60, dtype=np.uint8)]))
        where.append(b)
    queries.append(whole)
    where.append(4)  # ... and block 4 gets the query that belongs to block 5
    queries.append(whole)
    where.append(5)
    return blocks, queries, where


def pack_model(blocks, sa, queries, where, max_len):
    off = np.concatenate([[0], np.cumsum([len(b) for b in blocks])])
    return np.concatenate([flat_model(blocks[b], sa[off[b]:off[b + 1]], [q], max_len) for q, b in zip(queries, where)])


def test_pack(ctx):
    blocks, queries, where = pack_case()
    sizes = [len(b) for b in blocks]
    t = np.concatenate(blocks)
    d_sa = Words(len(t))
    ctx.dev_suffix_array_packed(dev_text(t), sizes, d_sa.t)
    for max_len in (8, 1000):
        want = pack_model(blocks, d_sa.host(), queries, where, max_len)
        got = np.stack(gpu_match(ctx, t, d_sa, queries, max_len, pack=(sizes, where)), axis=1)
        assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:5]
        if max_len == 1000:
            assert got[-300, 0] == 300 and got[-600, 0] < 40  # whole in block 5, not in block 4
        for min_len in (0, 1, 12):
            rows = smem_rows(want, queries, min_len, max_len)
            recs, total = gpu_smems(ctx, t, d_sa, queries, min_len, max_len, len(rows) + 1, pack=(sizes, where))
            assert total == len(rows) and np.array_equal(recs, rows), (max_len, min_len)


# ---- 6. alignment ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shifts", [(1, 0, 0, 0, 0), (3, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 3, 0, 0, 0), (0, 0, 1, 3, 1), (3, 1, 3, 1, 3)])
def test_pointers_off_their_alignment(ctx, shifts):
    t = u8(datagen.wiki_like(5003, seed=5))
    queries = [t[100:420].copy(), np.random.default_rng(6).integers(97, 123, size=150, dtype=np.uint8), t[4990:]]
    for sa_shift in (0, 1, 3):
        check(ctx, t, queries, 300, shifts, sa=gpu_sa(ctx, t, sa_shift))


# ---- 7. the lengths alone ---------------------------------------------------------------------------------------------------------------------------

def test_without_the_ranges(ctx, markov_sa):
    t, sa = markov_sa
    queries = long_copy_queries(t)[:2] + border_queries(t)
    for max_len in (3, 300, 4096):
        want = flat_model(t, sa.host(), queries, max_len)[:, 0]
        got, lo, hi = gpu_match(ctx, t, sa, queries, max_len, ranges=False)
        assert lo is None and hi is None and np.array_equal(got, want), max_len


# ---- 8. the super-maximal matches -------------------------------------------------------------------------------------------------------------------

def test_smems_of_the_depth_cases(ctx):
    for n in (65, 4097):
        t, queries = depth_case(n)
        sa = gpu_sa(ctx, t)
        for max_len in (3, 300, 1000):
            check_smems(ctx, t, queries, max_len, sa=sa)


def test_smems_at_the_ends_and_across_queries(ctx, markov_sa):
    for t, queries in END_CASES:
        for max_len in (1, 7, 1000):
            check_smems(ctx, t, queries, max_len)
    t, sa = markov_sa
    check_smems(ctx, t, border_queries(t), 1000, sa=sa)


def test_smems_over_more_than_one_tile_and_cut_lists(ctx):
    t, _ = depth_case(1 << 16)
    q = u8(b"ACGT")[np.random.default_rng(8).integers(0, 4, size=20000)]
    wants = check_smems(ctx, t, [q], 1000, cuts=True)
    assert len(wants[1]) > SM_TILE and len(wants[0]) == len(wants[1])  # more records than one tile of the scan holds
    assert 9 < len(wants[12]) < len(wants[1])


def test_a_copy_longer_than_the_cap(ctx, markov_sa):
    t, sa = markov_sa
    q = np.concatenate([u8(b"\x00"), t[4000:6500], u8(b"\x00")])
    for max_len in (300, 100):  # on either side of the border between the kernels
        recs, total = gpu_smems(ctx, t, sa, [q], 50, max_len, 8)
        assert total == 1 and recs[0, :2].tolist() == [1, max_len] and recs[0, 3] > recs[0, 2]
        check_smems(ctx, t, [q], max_len, sa=sa)


# ---- 9. the tuning build: the border at four bytes ----------------------------------------------------------------------------------------------------

WORKER = r"""
import os, sys
root, d = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import dark_amd
from test_gpu_sa_match import CAP, gpu_match
from test_gpu_sa_search import gpu_sa
with dark_amd.Context(CAP) as ctx:
    for k in range(int(np.load(os.path.join(d, "count.npy")))):
        text, flat, lens, max_len = (np.load(os.path.join(d, "%d.%s.npy" % (k, x))) for x in ("text", "qry", "lens", "max_len"))
        want = np.load(os.path.join(d, "%d.want.npy" % k))
        ends = np.cumsum(lens)
        got = np.stack(gpu_match(ctx, text, gpu_sa(ctx, text), [flat[e - m:e] for m, e in zip(lens, ends)], int(max_len)), axis=1)
        assert np.array_equal(got, want), ("case", k)
print("RESULT ok")
"""


def test_lane_max_of_four_gives_the_same_answers(ctx, markov_sa, tmp_path):
    """DK_SA_SEARCH_LANE_MAX = 4: every match of four bytes or more goes on in k_sa_match_long; the answers of the default build are the model's
    (checked here)"""
    t0, sa0 = markov_sa
    cases = [(depth_case(4097), 300, None), (depth_case(65), 3, None), (depth_case(65), 1000, None), ((t0, long_copy_queries(t0)), 4096, sa0)]
    cases += [((u8(t), queries), 1000, None) for t, queries in END_CASES]
    for k, ((t, queries), max_len, sa) in enumerate(cases):
        queries = [u8(q) for q in queries]
        np.save(tmp_path / ("%d.text.npy" % k), u8(t))
        np.save(tmp_path / ("%d.qry.npy" % k), np.concatenate(queries))
        np.save(tmp_path / ("%d.lens.npy" % k), np.array([len(q) for q in queries], np.int64))
        np.save(tmp_path / ("%d.max_len.npy" % k), np.array(max_len, np.int64))
        np.save(tmp_path / ("%d.want.npy" % k), check(ctx, t, queries, max_len, sa=sa))
    np.save(tmp_path / "count.npy", np.array(len(cases), np.int64))
    assert os.path.exists(TUNING_LIB), "build the tuning library: python dark_amd/build.py --tuning"
    env = {k: v for k, v in os.environ.items() if not k.startswith("DK_")}
    env.update(DARK_AMD_LIB=TUNING_LIB, DK_SA_SEARCH_LANE_MAX="4")
    p = subprocess.run([sys.executable, "-c", WORKER, ROOT, str(tmp_path)], env=env, capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0, "%s%s" % (p.stdout[-2000:], p.stderr[-4000:])
    assert "RESULT ok" in p.stdout


# ---- 10. the host forms and the constructor -------------------------------------------------------------------------------------------------------------

def test_host_forms_and_constructor(ctx, markov_sa):
    t, sa = markov_sa
    queries = long_copy_queries(t)[:2] + border_queries(t)
    want = flat_model(t, sa.host(), queries, 300)
    ln, lo, hi = ctx.sa_match(t, sa.host(), queries, 300)
    assert ln.dtype == np.uint32 and np.array_equal(np.stack([ln, lo, hi], axis=1), want)
    rows = smem_rows(want, queries, 12, 300)
    recs, total = ctx.sa_smems(t, sa.host(), queries, 12, 300)
    assert recs.dtype == SA_SMEM_DTYPE and total == len(rows) and np.array_equal(recs.view(np.uint32).reshape(-1, 4), rows)
    recs, total = ctx.sa_smems(t, sa.host(), queries, 12, 300, max_hits=2)
    assert total == len(rows) and np.array_equal(recs.view(np.uint32).reshape(-1, 4), rows[:2])
    assert ctx.sa_smems(t, sa.host(), queries, 12, 300, max_hits=0)[1] == len(rows)
    assert [len(x) for x in ctx.sa_match(t, sa.host(), [], 300)] == [0, 0, 0] and ctx.sa_smems(t, sa.host(), [b""], 0, 300)[1] == 0
    con = dark_amd.saca.Constructor(len(t))
    try:
        per_query = con.match(t, con.compute(t), queries, 300)
        assert np.array_equal(np.concatenate([np.stack(x, axis=1) for x in per_query]), want) and [len(x[0]) for x in per_query] == [len(q) for q in queries]
        out, total = con.smems(t, sa.host(), queries, 12, 300)
        starts = np.cumsum([0] + [len(q) for q in queries])
        assert total == len(rows) and np.array_equal(out["at"], rows[:, 0]) and np.array_equal(out["len"], rows[:, 1])
        assert np.array_equal(starts[out["query"]] + out["pos"], rows[:, 0]) and (out["pos"] < np.array([len(q) for q in queries])[out["query"]]).all()
        with pytest.raises(ValueError):
            con.match(t[:-1], sa.host()[:-1], queries, 300)
    finally:
        con.context().close()
    # queries that do not fit a small context beside the text: refused, and the context serves the next call
    small_t = u8(b"banana" * 50)
    with dark_amd.Context(len(small_t)) as small:
        small_sa = small.suffix_array(small_t)
        big = np.zeros(small.stats()["ws_size_bytes"] // 8, np.uint8)
        for call in (lambda: small.sa_match(small_t, small_sa, [big], 5), lambda: small.sa_smems(small_t, small_sa, [big], 0, 5)):
            with pytest.raises(dark_amd.DarkError) as e:
                call()
            assert e.value.code == DK_E_ARG and "do not fit the workspace" in str(e.value)
        got = np.stack(small.sa_match(small_t, small_sa, [b"xbananab"], 5), axis=1)
        assert np.array_equal(got, flat_model(small_t, small_sa, [b"xbananab"], 5))


# ---- 11. arrays that are no suffix arrays ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["zero", "ones", "words", "reversed"])
def test_containment(ctx, kind):
    """results are unspecified, but len <= the window, lo <= hi <= n, and nothing outside the outputs is written"""
    n = 5000
    t = u8(datagen.wiki_like(n, seed=7))
    rng = np.random.default_rng(41)
    good = gpu_sa(ctx, t)
    v = {"zero": lambda: np.zeros(n, np.uint32), "ones": lambda: np.full(n, 0xFFFFFFFF, np.uint32),
         "words": lambda: rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32), "reversed": lambda: good.host()[::-1].copy()}[kind]()
    sa = Words(n)
    put(sa, v)
    queries = [t[1000:1700].copy(), rng.integers(97, 123, size=300, dtype=np.uint8), t[:40].copy()]
    for max_len in (5, 1000):
        window = np.concatenate([np.minimum(max_len, np.arange(len(q), 0, -1)) for q in queries])
        ln, lo, hi = gpu_match(ctx, t, sa, queries, max_len)
        assert (ln <= window).all() and (lo <= hi).all() and (hi <= n).all()
        recs, total = gpu_smems(ctx, t, sa, queries, 0, max_len, 64)
        assert total <= len(window) and (recs[:, 0] < len(window)).all() and (recs[:, 2] <= recs[:, 3]).all() and (recs[:, 3] <= n).all()
    check(ctx, t, queries, 1000, sa=good)  # the context is usable afterwards


# ---- 12. refusals -----------------------------------------------------------------------------------------------------------------------------------

def test_decoder_context_refuses():
    """all six entries of the header, by name: DK_E_ARG naming the entry, nothing allocated or written, and the context goes on serving the inverse"""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dark_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dk_[a-z0-9_]*sa_(?:match|smems)[a-z0-9_]*)\s*\(", header))
    t = u8(b"banana" * 50)
    n = len(t)
    d_in = dev_text(t)
    d_sa, d_len, d_lo, d_hi, d_hits = Words(n), Words(6), Words(6), Words(6), Words(16)
    d_q, lens = dev_patterns([b"ana", b"nab"])
    host_sa = np.zeros(n, np.uint32)
    with dark_amd.Context(CAP) as full:
        L, origin = full.bwt_forward(t)
    with dark_amd.Context(n, purpose="decoder") as dec:
        assert np.array_equal(dec.bwt_inverse(L, origin), t)
        calls = {"dk_dev_sa_match": lambda: dec.dev_sa_match(d_in, n, d_sa.t, d_q, lens, 5, d_len.t, d_lo.t, d_hi.t),
                 "dk_dev_sa_match_packed": lambda: dec.dev_sa_match_packed(d_in, [n], d_sa.t, d_q, lens, [0, 0], 5, d_len.t, d_lo.t, d_hi.t),
                 "dk_sa_match": lambda: dec.sa_match(t, host_sa, [b"ana"], 5),
                 "dk_dev_sa_smems": lambda: dec.dev_sa_smems(d_in, n, d_sa.t, d_q, lens, 0, 5, 4, d_hits.t),
                 "dk_dev_sa_smems_packed": lambda: dec.dev_sa_smems_packed(d_in, [n], d_sa.t, d_q, lens, [0, 0], 0, 5, 4, d_hits.t),
                 "dk_sa_smems": lambda: dec.sa_smems(t, host_sa, [b"ana"], 0, 5)}
        assert declared == set(calls) == set(ENTRIES), sorted(declared ^ set(calls))
        for name, call in calls.items():
            peak = dec.stats()["ws_peak_bytes"]
            with pytest.raises(dark_amd.DarkError) as e:
                call()
            msg = dec._lib.dk_last_error(dec._h).decode()
            assert e.value.code == DK_E_ARG and msg.startswith(name + ":") and "decoder context" in msg, msg
            assert dec.stats()["ws_peak_bytes"] == peak, name
            assert np.array_equal(dec.bwt_inverse(L, origin), t), "the inverse after the refused " + name
        assert all(w.untouched() for w in (d_sa, d_len, d_lo, d_hi, d_hits))


def test_arguments(ctx):
    t = u8(b"banana" * 50)
    n = len(t)
    d_in, sa = dev_text(t), gpu_sa(ctx, t)
    d_q, lens = dev_patterns([b"ana", b"nab"])
    ln, lo, hi, hits = Words(6), Words(6), Words(6), Words(17)
    with pytest.raises(dark_amd.DarkError) as e:
        ctx.dev_sa_match(d_in, n, sa.t, d_q, lens, 0, ln.t, lo.t, hi.t)
    assert e.value.code == DK_E_ARG and "max_len" in str(e.value)
    with pytest.raises(dark_amd.DarkError) as e:
        ctx.dev_sa_smems(d_in, n, sa.t, d_q, lens, 0, 0, 4, hits.t)
    assert e.value.code == DK_E_ARG and "max_len" in str(e.value)
    for a, b in ((lo.t, None), (None, hi.t)):
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.dev_sa_match(d_in, n, sa.t, d_q, lens, 5, ln.t, a, b)
        assert e.value.code == DK_E_ARG
    for blocks in ([0, 1], [7, 0]):
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.dev_sa_match_packed(d_in, [n], sa.t, d_q, lens, blocks, 5, ln.t, lo.t, hi.t)
        assert e.value.code == DK_E_ARG
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.dev_sa_smems_packed(d_in, [n], sa.t, d_q, lens, blocks, 0, 5, 4, hits.t)
        assert e.value.code == DK_E_ARG
    with pytest.raises(dark_amd.DarkError) as e:
        ctx.dev_sa_smems(d_in, n, sa.t, d_q, lens, 0, 5, 4, hits.t[1:])  # records off their 16 bytes
    assert e.value.code == DK_E_ARG and "16-byte aligned" in str(e.value)
    lib, h = ctx._lib, ctx._h
    p_in, p_sa, p_q, p_ln, p_hits = (C.c_void_p(x.data_ptr()) for x in (d_in, sa.t, d_q, ln.t, hits.t))
    ls, total = (C.c_size_t * 2)(3, 3), C.c_uint64(7)
    for args in ((None, n, p_sa, p_q, 2, ls, 5, p_ln, None, None), (p_in, 0, p_sa, p_q, 2, ls, 5, p_ln, None, None), (p_in, n, None, p_q, 2, ls, 5, p_ln, None, None),
                 (p_in, n, p_sa, None, 2, ls, 5, p_ln, None, None), (p_in, n, p_sa, p_q, 2, None, 5, p_ln, None, None), (p_in, n, p_sa, p_q, 2, ls, 5, None, None, None),
                 (p_in, n, p_sa, p_q, 2, (C.c_size_t * 2)(1 << 31, 1 << 31), 5, p_ln, None, None)):
        assert lib.dk_dev_sa_match(h, *args) == DK_E_ARG
    for args in ((p_in, n, p_sa, p_q, 2, ls, 0, 5, 4, None, C.byref(total)), (p_in, n, p_sa, p_q, 2, ls, 0, 5, 4, p_hits, None), (p_in, n, p_sa, None, 2, ls, 0, 5, 4, p_hits, C.byref(total))):
        assert lib.dk_dev_sa_smems(h, *args) == DK_E_ARG
    assert total.value == 7 and all(w.untouched() for w in (ln, lo, hi, hits))
    # nothing to do is DK_OK, writes nothing and counts nothing
    ctx.dev_sa_match(d_in, n, sa.t, d_q, [], 5, ln.t, lo.t, hi.t)
    ctx.dev_sa_match(d_in, n, sa.t, d_q, [0, 0], 5, ln.t, lo.t, hi.t)
    assert ctx.dev_sa_smems(d_in, n, sa.t, d_q, [], 0, 5, 4, hits.t) == 0 and ctx.dev_sa_smems(d_in, n, sa.t, d_q, [0], 0, 5, 4, hits.t) == 0
    assert all(w.untouched() for w in (ln, lo, hi, hits))
    assert ctx.dev_sa_smems(d_in, n, sa.t, d_q, lens, 0, 1 << 40, 0, None) == 2  # a cap above 2^32 - 1 counts as that; counting needs no records
    check(ctx, t, [b"ana", b"nab"], 5, sa=sa)


# ---- 13. a poisoned workspace behind a poisoned mailbox -------------------------------------------------------------------------------------------------

def test_poisoned_workspace_and_mailbox():
    """one run in a fresh process on the tuning build with DK_POISON=165, every call behind dk_dbg_mail_fill(165): tests/sa_match_poison_worker.py"""
    assert os.path.exists(TUNING_LIB), "build the tuning library: python dark_amd/build.py --tuning (__graft_entry__.build() does)"
    env = {k: v for k, v in os.environ.items() if not k.startswith("DK_")}
    env.update(DARK_AMD_LIB=TUNING_LIB, DK_POISON="165")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sa_match_poison_worker.py"), "sa_match", "165"], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=TIMEOUT)
    assert p.returncode == 0, "exit status %d\n%s" % (p.returncode, (p.stdout + p.stderr)[-3000:])
    report = json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    assert report["byte"] == 165 and report["contexts"] == 1 and report["fills"] > 0 and report["peeks"] >= 12, report


# ---- 14. the C++ mirror ---------------------------------------------------------------------------------------------------------------------------------

def test_cpp_mirror(tmp_path):
    exe = str(tmp_path / "cpp_sa_match")
    lib_dir = os.path.join(ROOT, "dark_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_sa_match.cpp"),
                           "-L", lib_dir, "-ldark_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=TIMEOUT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cpp sa match ok" in out.stdout
