"""Pattern search in a suffix array on the GPU (dk_dev_sa_search, its host and packed forms; csrc/sa_query.hip).  Every (lo, hi)
must equal the plain model of tests/sa_query_model.py (bisect over the cut suffixes; pinned by tests/test_sa_query_model.py) on the suffix array
dev_suffix_array gives.  Every device output sits between GUARD words, as in tests/test_gpu_lcp.py.  The tuning build moves the border between
the two kernels in a subprocess."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import dark_amd
from conftest import ROOT
from dark_amd import datagen
from dark_amd._lib import DK_E_ARG
from sa_query_model import OK, search_model
from test_gpu_lcp import Words, dev_text, u8

pytestmark = pytest.mark.gpu
CAP = 1 << 19
LANE_MAX = 256  # csrc/sa_query.hip: SA_SEARCH_LANE_MAX
TUNING_LIB = os.path.join(ROOT, "dark_amd", "libdark_amd_tuning.so")
TIMEOUT = 120


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


def put(words, values):
    words.t.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint32).view(np.int32)))


def gpu_sa(ctx, t, shift=0):
    sa = Words(len(t), shift)
    ctx.dev_suffix_array(dev_text(t), len(t), sa.t)
    assert sa.guards_intact()
    return sa


def dev_patterns(patterns, shift=0):
    keep = [u8(p) for p in patterns]
    return dev_text(np.concatenate(keep + [np.zeros(1, np.uint8)]), shift), [len(p) for p in keep]  # (one byte more: never an empty tensor)


def gpu_search(ctx, t, sa, patterns, shifts=(0, 0, 0, 0)):
    """[(lo, hi)] through dev_sa_search; sa: a Words holding the array; shifts: of the text, the patterns (bytes), lo and hi (elements)"""
    d_pat, lens = dev_patterns(patterns, shifts[1])
    lo, hi = Words(len(lens), shifts[2]), Words(len(lens), shifts[3])
    ctx.dev_sa_search(dev_text(t, shifts[0]), len(t), sa.t, d_pat, lens, lo.t, hi.t)
    assert lo.guards_intact() and hi.guards_intact() and sa.guards_intact(), "a store left the outputs"
    return list(zip(lo.host().tolist(), hi.host().tolist()))


def check(ctx, t, patterns, shifts=(0, 0, 0, 0), sa=None):
    t = u8(t)
    sa = sa or gpu_sa(ctx, t)
    got = gpu_search(ctx, t, sa, patterns, shifts)
    want = search_model(t, sa.host(), patterns)
    bad = [q for q in range(len(patterns)) if got[q] != want[q]]
    assert not bad, "pattern %d of %d bytes: %s, model %s (n = %d, %d wrong)" % (bad[0], len(patterns[bad[0]]), got[bad[0]], want[bad[0]], len(t), len(bad))
    return got


def cut_patterns(t, rng, count, lengths):
    """pieces of the text, and for every second one the same with its last byte changed"""
    t = u8(t)
    out = []
    for k in range(count):
        m = int(rng.choice(lengths))
        a = int(rng.integers(0, max(1, len(t) - m + 1)))
        p = t[a:a + m].copy()
        if k & 1 and len(p):
            p[-1] = (int(p[-1]) + int(rng.integers(1, 256))) & 255
        out.append(p)
    return out


# ---- small texts, every pattern ----------------------------------------------------------------------------------------------------------------

def test_every_short_pattern_of_a_small_text(ctx):
    t = bytes(np.random.default_rng(1).integers(97, 99, size=40, dtype=np.uint8))
    subs = sorted({t[a:a + m] for a in range(40) for m in range(1, 9) if a + m <= 40})
    pats = [b"", b"\x00", b"\xff", t, t + b"a", t + b"\x00", t[1:], t[:-1]] + subs + [s + c for s in subs for c in (b"a", b"b", b"c", b"\x00")]
    got = check(ctx, t, pats)
    assert got[0] == (0, 40) and got[1] == (0, 0) and got[2] == (40, 40) and got[3][1] - got[3][0] == 1 and got[4][0] == got[4][1]


def test_last_suffix_that_is_a_prefix_of_others(ctx):
    got = check(ctx, b"abab", [b"aba", b"ab", b"b", b"bab", b"abab", b"ababa", b"", b"a", b"ba"])
    assert got[0] == (1, 2) and got[1] == (0, 2)
    got = check(ctx, b"abracadabra", [b"abra", b"a", b"", b"abracadabra", b"abracadabraa", b"b", b"zz", b"\x00", b"ac"])  # the array of src/saca.rs:411
    assert got[:4] == [(1, 3), (0, 5), (0, 11), (2, 3)]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 300, 4097])
def test_one_symbol(ctx, n):
    """a^n: slot i holds the suffix of i + 1 bytes, so a^k has the slots from k - 1 on and a^(n+1) none"""
    ks = sorted({k for k in (1, 2, n - 1, n, n + 1, n + 300, LANE_MAX, LANE_MAX + 1) if k >= 1})
    got = check(ctx, b"a" * n, [b"a" * k for k in ks] + [b"a" * (n // 2) + b"b", b"\x00", b"b"])
    for k, g in zip(ks, got):
        assert g == ((k - 1, n) if k <= n else (n, n)), (k, g)


@pytest.mark.parametrize("m", [15, 16, 17, 31, 32, 33, LANE_MAX - 1, LANE_MAX, LANE_MAX + 1, 1023, 1024, 1025, 1040])
def test_pattern_lengths_around_the_steps(ctx, markov_sa, m):
    """16 bytes a step in a lane, lane_max between the kernels, 1024 bytes a step in a wave: occurring, and differing in the last byte"""
    t, sa = markov_sa
    pats = []
    for a in (0, 1, 777, 40000, len(t) - m):
        p = t[a:a + m].copy()
        pats.append(p)
        for d in (1, 255):
            q = p.copy()
            q[-1] = (int(q[-1]) + d) & 255
            pats.append(q)
    got = check(ctx, t, pats, sa=sa)
    assert all(hi > lo for lo, hi in got[::3])


@pytest.fixture(scope="module")
def markov_sa(ctx):
    t = u8(datagen.wiki_like(70000, seed=3))
    return t, gpu_sa(ctx, t)


# ---- sizes at which the number of 64-ary steps changes -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [63, 64, 65, 4095, 4096, 4097, 262143, 262144, 262145])
def test_sizes_around_the_step_counts(ctx, n):
    rng = np.random.default_rng(n)
    t = rng.integers(97, 101, size=n, dtype=np.uint8)
    pats = cut_patterns(t, rng, 60, [1, 2, 3, 5, 8, 12, 20]) + [b"", b"a", b"d", b"e", b"`", t[:300], t[n - 40:], np.concatenate([t[n - 40:], [97]])]
    got = check(ctx, t, pats)
    assert got[60] == (0, n) and got[63] == (n, n) and got[64] == (0, 0)


@pytest.mark.parametrize("npat", [1, 3, 4, 5, 255, 256, 257, 10000])
def test_pattern_counts(ctx, markov_sa, npat):
    t, sa = markov_sa
    rng = np.random.default_rng(npat)
    check(ctx, t, cut_patterns(t, rng, npat, [0, 1, 2, 3, 4, 6, 9, 14, 20, 300]), sa=sa)


def test_no_patterns(ctx, markov_sa):
    t, sa = markov_sa
    lo, hi = Words(4), Words(4)
    ctx.dev_sa_search(dev_text(t), len(t), sa.t, dev_text(u8(b"x")), [], lo.t, hi.t)
    assert lo.untouched() and hi.untouched()
    assert ctx._lib.dk_dev_sa_search(ctx._h, C.c_void_p(dev_text(t).data_ptr()), len(t), C.c_void_p(sa.t.data_ptr()), None, 0, None, None, None) == 0


@pytest.mark.parametrize("shifts", [(1, 0, 0, 0), (3, 0, 0, 0), (0, 1, 0, 0), (0, 3, 0, 0), (0, 0, 1, 3), (3, 1, 3, 1)])
def test_pointers_off_their_alignment(ctx, shifts):
    t = u8(datagen.wiki_like(20011, seed=5))
    rng = np.random.default_rng(6)
    for sa_shift in (0, 1, 3):
        check(ctx, t, cut_patterns(t, rng, 50, [1, 4, 15, 16, 17, 40, 300, 1500]), shifts, sa=gpu_sa(ctx, t, sa_shift))


# ---- long repeats ----------------------------------------------------------------------------------------------------------------------------

def halves_case():
    h = np.random.default_rng(8).integers(0, 256, size=70000, dtype=np.uint8)
    t = np.concatenate([h, h])
    long = t[1000:41000].copy()
    off = long.copy()
    off[-1] ^= 1
    early = long.copy()
    early[20000] ^= 1
    return t, [long, off, early, t[69000:71000], t[30000:30300], h, np.concatenate([h, h[:1]]), t, long[:LANE_MAX], long[:LANE_MAX + 1]]


def test_two_identical_halves_with_a_long_pattern(ctx):
    """40 000 bytes that occur twice, 70 000 bytes apart: the long kernel, and the bytes known from the borders on every later step"""
    t, pats = halves_case()
    got = check(ctx, t, pats)
    assert got[0][1] - got[0][0] == 2 and got[1][0] == got[1][1] and got[2][0] == got[2][1]
    assert got[3][1] - got[3][0] == 1 and got[5][1] - got[5][0] == 2 and got[6][1] - got[6][0] == 1 and got[7][1] - got[7][0] == 1


# ---- the tuning build: short patterns through the long kernel -----------------------------------------------------------------------------------

WORKER = r"""
import json, os, sys
root, d = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import dark_amd
from test_gpu_sa_search import CAP, gpu_sa, gpu_search
with dark_amd.Context(CAP) as ctx:
    for k in range(int(np.load(os.path.join(d, "count.npy")))):
        text, flat, lens = (np.load(os.path.join(d, "%d.%s.npy" % (k, x))) for x in ("text", "pat", "lens"))
        want = np.load(os.path.join(d, "%d.want.npy" % k))
        ends = np.cumsum(lens)
        got = gpu_search(ctx, text, gpu_sa(ctx, text), [flat[e - m:e] for m, e in zip(lens, ends)])
        assert np.array_equal(np.array(got, np.int64).reshape(-1, 2), want), ("case", k)
print("RESULT ok")
"""


def test_lane_max_of_four_gives_the_same_answers(ctx, markov_sa, tmp_path):
    """DK_SA_SEARCH_LANE_MAX = 4: everything from five bytes on takes k_sa_search_long; the answers of the default build are the model's (checked here)"""
    rng = np.random.default_rng(21)
    t0, sa0 = markov_sa
    small = rng.integers(97, 99, size=4097, dtype=np.uint8)
    halves, halves_pats = halves_case()
    cases = [(t0, cut_patterns(t0, rng, 400, [0, 1, 3, 4, 5, 6, 15, 16, 17, 64, 255, 256, 257, 1100]), sa0),
             (small, cut_patterns(small, rng, 400, [1, 2, 4, 5, 9, 30, 200]) + [b"", b"a" * 5, b"b" * 5, b"c" * 5, b"\x00" * 5], None),
             (u8(b"a" * 300), [b"a" * k for k in (1, 4, 5, 299, 300, 301)], None), (halves, halves_pats, None)]
    for k, (t, pats, sa) in enumerate(cases):
        pats = [u8(p) for p in pats]
        np.save(tmp_path / ("%d.text.npy" % k), u8(t))
        np.save(tmp_path / ("%d.pat.npy" % k), np.concatenate(pats))
        np.save(tmp_path / ("%d.lens.npy" % k), np.array([len(p) for p in pats], np.int64))
        np.save(tmp_path / ("%d.want.npy" % k), np.array(check(ctx, t, pats, sa=sa), np.int64).reshape(-1, 2))
    np.save(tmp_path / "count.npy", np.array(len(cases), np.int64))
    assert os.path.exists(TUNING_LIB), "build the tuning library: python dark_amd/build.py --tuning"
    env = {k: v for k, v in os.environ.items() if not k.startswith("DK_")}
    env.update(DARK_AMD_LIB=TUNING_LIB, DK_SA_SEARCH_LANE_MAX="4")
    p = subprocess.run([sys.executable, "-c", WORKER, ROOT, str(tmp_path)], env=env, capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0, "%s%s" % (p.stdout[-2000:], p.stderr[-4000:])
    assert "RESULT ok" in p.stdout


# ---- packs -----------------------------------------------------------------------------------------------------------------------------------

def test_pack(ctx):
    rng = np.random.default_rng(31)
    piece = rng.integers(97, 100, size=12, dtype=np.uint8)
    blocks = [u8(b"x"), np.concatenate([rng.integers(97, 100, size=500, dtype=np.uint8), piece, rng.integers(97, 100, size=88, dtype=np.uint8)]),
              u8(b"a"), np.concatenate([piece, piece, rng.integers(97, 100, size=4073, dtype=np.uint8)]), piece.copy(), u8(b"ab"),
              u8(datagen.wiki_like(65537, seed=4)), u8(b"\x00")]
    sizes = [len(b) for b in blocks]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    d_in = dev_text(np.concatenate(blocks))
    d_sa = Words(int(off[-1]))
    ctx.dev_suffix_array_packed(d_in, sizes, d_sa.t)
    sa = d_sa.host()
    pats, where = [], []
    for b in range(len(blocks)):  # the same patterns in every block: the piece, one byte, one byte more than the block, nothing
        for p in (piece, piece[:1], np.concatenate([blocks[b], [97]]), blocks[b], b"", b"x", b"a", b"\x00", piece[:5], blocks[6][1000:1300]):
            pats.append(u8(p))
            where.append(b)
    order = rng.permutation(len(pats))  # neighbours in the batch are in different blocks
    pats, where = [pats[i] for i in order], [where[i] for i in order]
    d_pat, lens = dev_patterns(pats)
    lo, hi = Words(len(pats)), Words(len(pats))
    ctx.dev_sa_search_packed(d_in, sizes, d_sa.t, d_pat, lens, where, lo.t, hi.t)
    assert lo.guards_intact() and hi.guards_intact() and d_sa.guards_intact()
    got = list(zip(lo.host().tolist(), hi.host().tolist()))
    for q, (p, b) in enumerate(zip(pats, where)):
        want = search_model(blocks[b], sa[off[b]:off[b + 1]], [p])[0]
        assert got[q] == want, "pattern %d of %d bytes in block %d: %s, model %s" % (q, len(p), b, got[q], want)
        one = gpu_search(ctx, blocks[b], gpu_sa(ctx, blocks[b]), [p])[0] if q < 12 else want
        assert one == want
    found = {b: got[q] for q, (p, b) in enumerate(zip(pats, where)) if len(p) == 12 and np.array_equal(p, piece)}
    assert [found[b][1] - found[b][0] for b in (0, 1, 2, 3, 4, 5)] == [0, 1, 0, 2, 1, 0]


# ---- arrays that are no suffix arrays ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["words", "below_2n", "zero", "reversed"])
def test_containment(ctx, markov_sa, kind):
    """results are unspecified, but lo <= hi <= n, and nothing outside the outputs is written"""
    t, good = markov_sa
    n = len(t)
    rng = np.random.default_rng(41)
    v = {"words": lambda: rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32), "below_2n": lambda: rng.integers(0, 2 * n, size=n, dtype=np.uint32),
         "zero": lambda: np.zeros(n, np.uint32), "reversed": lambda: good.host()[::-1].copy()}[kind]()
    sa = Words(n)
    put(sa, v)
    pats = cut_patterns(t, rng, 300, [0, 1, 2, 5, 16, 40, 300, 2000]) + [t[:5000], t[n - 3000:], t]
    got = np.array(gpu_search(ctx, t, sa, pats), np.int64)
    assert (got[:, 0] <= got[:, 1]).all() and (got[:, 1] <= n).all(), got[(got[:, 0] > got[:, 1]) | (got[:, 1] > n)][:5]
    sizes = [n // 3, n - n // 3]
    d_pat, lens = dev_patterns(pats)
    lo, hi = Words(len(pats)), Words(len(pats))
    blocks = [int(q & 1) for q in range(len(pats))]
    ctx.dev_sa_search_packed(dev_text(t), sizes, sa.t, d_pat, lens, blocks, lo.t, hi.t)
    assert lo.guards_intact() and hi.guards_intact() and sa.guards_intact()
    l, h = lo.host().astype(np.int64), hi.host().astype(np.int64)
    assert (l <= h).all() and (h <= np.array(sizes)[blocks]).all()
    check(ctx, t, pats[:20], sa=good)  # the context is usable afterwards


# ---- the host form and the mirror ------------------------------------------------------------------------------------------------------------

def test_host_form_and_constructor(ctx, markov_sa):
    t, sa = markov_sa
    rng = np.random.default_rng(51)
    pats = cut_patterns(t, rng, 200, [0, 1, 3, 8, 17, 300]) + [b""]
    want = search_model(t, sa.host(), pats)
    lo, hi = ctx.sa_search(t, sa.host(), pats)
    assert lo.dtype == np.uint32 and hi.dtype == np.uint32 and list(zip(lo.tolist(), hi.tolist())) == want
    lo, hi = ctx.sa_search(t, sa.host(), [])
    assert len(lo) == 0 and len(hi) == 0
    lo, hi = ctx.sa_search(t, sa.host(), [b"", b""])
    assert lo.tolist() == [0, 0] and hi.tolist() == [len(t)] * 2
    con = dark_amd.saca.Constructor(len(t))
    try:
        lo, hi = con.search(t, con.compute(t), pats)
        assert list(zip(lo.tolist(), hi.tolist())) == want
        with pytest.raises(ValueError):
            con.search(t[:-1], sa.host()[:-1], pats)
    finally:
        con.context().close()


# ---- arguments -------------------------------------------------------------------------------------------------------------------------------

def test_arguments(ctx):
    t = u8(b"banana" * 50)
    n = len(t)
    d_in, sa = dev_text(t), gpu_sa(ctx, t)
    d_pat, lens = dev_patterns([b"ana", b"nab"])
    lo, hi = Words(2), Words(2)
    lib, h = ctx._lib, ctx._h
    p_in, p_sa, p_pat, p_lo, p_hi = (C.c_void_p(x.data_ptr()) for x in (d_in, sa.t, d_pat, lo.t, hi.t))
    ns, ls, bs = (C.c_size_t * 1)(n), (C.c_size_t * 2)(3, 3), (C.c_uint32 * 2)(0, 0)
    host_sa, host_lo = sa.host(), np.zeros(2, np.uint32)
    q_in, q_sa, q_pat, q_lo = (x.ctypes.data_as(C.c_void_p) for x in (t, host_sa, u8(b"ananab"), host_lo))
    verdict, where = (C.c_uint32 * 1)(77), (C.c_uint32 * 1)(77)
    # the check
    for fn, a_in, a_sa in ((lib.dk_dev_sa_check, p_in, p_sa), (lib.dk_sa_check, q_in, q_sa)):
        for args in ((None, n, a_sa, verdict, where), (a_in, n, None, verdict, where), (a_in, n, a_sa, None, where), (a_in, n, a_sa, verdict, None),
                     (a_in, 0, a_sa, verdict, where), (a_in, CAP + 1, a_sa, verdict, where)):
            assert fn(h, *args) == DK_E_ARG
        assert fn(None, a_in, n, a_sa, verdict, where) == DK_E_ARG
    for args in ((None, 1, ns, p_sa, verdict, where), (p_in, 1, None, p_sa, verdict, where), (p_in, 1, ns, None, verdict, where), (p_in, 1, ns, p_sa, None, where),
                 (p_in, 1, ns, p_sa, verdict, None), (p_in, 0, ns, p_sa, verdict, where)):
        assert lib.dk_dev_sa_check_packed(h, *args) == DK_E_ARG
    for sizes in ([300, 0], [(1 << 24) + 1], [CAP, 1]):
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.dev_sa_check_packed(d_in, sizes, sa.t)
        assert e.value.code == DK_E_ARG
    assert verdict[0] == 77 and where[0] == 77
    # the search
    for fn, a_in, a_sa, a_pat, a_lo, a_hi in ((lib.dk_dev_sa_search, p_in, p_sa, p_pat, p_lo, p_hi), (lib.dk_sa_search, q_in, q_sa, q_pat, q_lo, q_lo)):
        for args in ((None, n, a_sa, a_pat, 2, ls, a_lo, a_hi), (a_in, n, None, a_pat, 2, ls, a_lo, a_hi), (a_in, n, a_sa, None, 2, ls, a_lo, a_hi),
                     (a_in, n, a_sa, a_pat, 2, None, a_lo, a_hi), (a_in, n, a_sa, a_pat, 2, ls, None, a_hi), (a_in, n, a_sa, a_pat, 2, ls, a_lo, None),
                     (a_in, 0, a_sa, a_pat, 2, ls, a_lo, a_hi), (a_in, CAP + 1, a_sa, a_pat, 2, ls, a_lo, a_hi)):
            assert fn(h, *args) == DK_E_ARG
        too_many = (C.c_size_t * 2)(1 << 31, 1 << 31)  # 2^32 bytes in all (refused before anything is read)
        assert fn(h, a_in, n, a_sa, a_pat, 2, too_many, a_lo, a_hi) == DK_E_ARG
    for args in ((None, 1, ns, p_sa, p_pat, 2, ls, bs, p_lo, p_hi), (p_in, 1, None, p_sa, p_pat, 2, ls, bs, p_lo, p_hi), (p_in, 1, ns, None, p_pat, 2, ls, bs, p_lo, p_hi),
                 (p_in, 1, ns, p_sa, None, 2, ls, bs, p_lo, p_hi), (p_in, 1, ns, p_sa, p_pat, 2, None, bs, p_lo, p_hi), (p_in, 1, ns, p_sa, p_pat, 2, ls, None, p_lo, p_hi),
                 (p_in, 1, ns, p_sa, p_pat, 2, ls, bs, None, p_hi), (p_in, 1, ns, p_sa, p_pat, 2, ls, bs, p_lo, None), (p_in, 0, ns, p_sa, p_pat, 2, ls, bs, p_lo, p_hi),
                 (p_in, 1, ns, p_sa, p_pat, 2, ls, (C.c_uint32 * 2)(0, 1), p_lo, p_hi)):  # the last: a block the pack does not have
        assert lib.dk_dev_sa_search_packed(h, *args) == DK_E_ARG
    assert lo.untouched() and hi.untouched() and not host_lo.any()
    # the host form: patterns that do not fit the workspace beside the block
    with dark_amd.Context(n) as small:
        size = small.stats()["ws_size_bytes"]
        big = np.zeros(size, np.uint8)
        with pytest.raises(dark_amd.DarkError) as e:
            small.sa_search(t, host_sa, [big])
        assert e.value.code == DK_E_ARG
        lo2, hi2 = small.sa_search(t, host_sa, [b"ana", b"nab"])
        assert (lo2.tolist(), hi2.tolist()) == tuple(map(list, zip(*search_model(t, host_sa, [b"ana", b"nab"]))))
    assert gpu_search(ctx, t, sa, [b"ana", b"nab"]) == search_model(t, host_sa, [b"ana", b"nab"])


def test_decoder_context_refuses():
    """all six entries of the header, by name: DK_E_ARG naming the entry, nothing allocated or written, and the context goes on serving the inverse"""
    header = open(os.path.join(ROOT, "include", "dark_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(dk_[a-z0-9_]*sa_(?:check|search)[a-z0-9_]*)\s*\(", header))
    t = u8(b"banana" * 50)
    n = len(t)
    d_in = dev_text(t)
    d_sa, d_lo, d_hi = Words(n), Words(2), Words(2)
    d_pat, lens = dev_patterns([b"ana", b"nab"])
    host_sa = np.zeros(n, np.uint32)
    with dark_amd.Context(CAP) as full:
        L, origin = full.bwt_forward(t)
    with dark_amd.Context(n, purpose="decoder") as dec:
        assert np.array_equal(dec.bwt_inverse(L, origin), t)
        calls = {"dk_dev_sa_check": lambda: dec.dev_sa_check(d_in, n, d_sa.t),
                 "dk_sa_check": lambda: dec.sa_check(t, host_sa),
                 "dk_dev_sa_check_packed": lambda: dec.dev_sa_check_packed(d_in, [n], d_sa.t),
                 "dk_dev_sa_search": lambda: dec.dev_sa_search(d_in, n, d_sa.t, d_pat, lens, d_lo.t, d_hi.t),
                 "dk_sa_search": lambda: dec.sa_search(t, host_sa, [b"ana"]),
                 "dk_dev_sa_search_packed": lambda: dec.dev_sa_search_packed(d_in, [n], d_sa.t, d_pat, lens, [0, 0], d_lo.t, d_hi.t)}
        assert declared == set(calls), sorted(declared ^ set(calls))
        for name, call in calls.items():
            peak = dec.stats()["ws_peak_bytes"]
            with pytest.raises(dark_amd.DarkError) as e:
                call()
            msg = dec._lib.dk_last_error(dec._h).decode()
            assert e.value.code == DK_E_ARG and msg.startswith(name + ":") and "decoder context" in msg, msg
            assert dec.stats()["ws_peak_bytes"] == peak, name
            assert np.array_equal(dec.bwt_inverse(L, origin), t), "the inverse after the refused " + name
        assert d_sa.untouched() and d_lo.untouched() and d_hi.untouched()


# ---- workspace -------------------------------------------------------------------------------------------------------------------------------

def test_workspace_of_exactly_sized_contexts():
    t = u8(datagen.wiki_like(200000, seed=17))
    n = len(t)
    rng = np.random.default_rng(61)
    pats = cut_patterns(t, rng, 2000, [1, 5, 20, 300])
    sizes = [1, 70000, 4097, n - 74098]
    with dark_amd.Context(n) as exact:
        def within():
            st = exact.stats()
            assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], st
        sa = gpu_sa(exact, t)
        assert exact.dev_sa_check(dev_text(t), n, sa.t) == (OK, n)
        within()
        assert exact.sa_check(t, sa.host()) == (OK, n)
        within()
        want = search_model(t, sa.host(), pats)
        assert gpu_search(exact, t, sa, pats) == want
        within()
        lo, hi = exact.sa_search(t, sa.host(), pats)
        within()
        assert list(zip(lo.tolist(), hi.tolist())) == want
        psa = Words(n)
        exact.dev_suffix_array_packed(dev_text(t), sizes, psa.t)
        assert exact.dev_sa_check_packed(dev_text(t), sizes, psa.t) == [(OK, k) for k in sizes]
        within()
        d_pat, lens = dev_patterns(pats)
        plo, phi = Words(len(pats)), Words(len(pats))
        exact.dev_sa_search_packed(dev_text(t), sizes, psa.t, d_pat, lens, [1] * len(pats), plo.t, phi.t)
        within()
        assert plo.guards_intact() and phi.guards_intact()
