"""The FM-index on the GPU (csrc/fm_index.hip): dk_dev_fm_build / dk_dev_fm_count, their packed and host forms, the rank
kernel on its own, decoder contexts, and the mirrors.  Every (lo, hi) must equal tests/fm_model.py; where a suffix array exists, also
search_model of tests/sa_query_model.py and dev_sa_search.  Every device output, and the index, sits between guard words."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

import dark_amd
from conftest import ROOT
from dark_amd import datagen, fm
from dark_amd._lib import DK_E_ARG
from dark_amd.context import fm_index_bytes
from fm_model import fm_model, fm_model_packed, rank_model
from sa_query_model import search_model
from test_gpu_lcp import Words, dev_text, u8
from test_gpu_sa_search import cut_patterns, dev_patterns, gpu_sa, gpu_search

pytestmark = pytest.mark.gpu
CAP = 1 << 19
FM_BLOCK = 1024  # csrc/fm_index.hip
HEADER_WORDS = 64
TIMEOUT = 120


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


def words(alphabet, lengths):
    return [bytes(w) for m in lengths for w in itertools.product(alphabet, repeat=m)]


def gpu_bwt(ctx, t):
    """-> (L as a numpy array, origin) through dev_bwt_forward"""
    d = torch.empty(len(t), dtype=torch.uint8, device="cuda")
    origin = ctx.dev_bwt_forward(dev_text(t), len(t), d)
    return d.cpu().numpy(), origin


def gpu_index(ctx, L, sizes, origins, shift=0, index_shift=0):
    """-> (L on the device, `shift` bytes off its place; the index in a Words)"""
    d_bwt = dev_text(L, shift)
    idx = Words(fm_index_bytes(len(L), len(sizes)) // 4, index_shift)
    if len(sizes) == 1:
        ctx.dev_fm_build(d_bwt, len(L), origins[0], idx.t)
    else:
        ctx.dev_fm_build_packed(d_bwt, sizes, origins, idx.t)
    assert idx.guards_intact(), "the build wrote outside the index"
    return d_bwt, idx


def gpu_count(ctx, d_bwt, sizes, idx, patterns, blocks=None, shifts=(0, 0, 0)):
    """[(lo, hi)] through dev_fm_count(_packed); shifts: of the patterns (bytes), lo and hi (elements)"""
    d_pat, lens = dev_patterns(patterns, shifts[0])
    lo, hi = Words(len(lens), shifts[1]), Words(len(lens), shifts[2])
    if blocks is None:
        ctx.dev_fm_count(d_bwt, sizes[0], idx.t, d_pat, lens, lo.t, hi.t)
    else:
        ctx.dev_fm_count_packed(d_bwt, sizes, idx.t, d_pat, lens, blocks, lo.t, hi.t)
    assert lo.guards_intact() and hi.guards_intact() and idx.guards_intact(), "a store left the outputs"
    return list(zip(lo.host().tolist(), hi.host().tolist()))


def first_difference(got, want, patterns):
    bad = [q for q in range(len(want)) if got[q] != want[q]]
    return "" if not bad else "pattern %d of %d bytes: %s, expected %s (%d wrong)" % (bad[0], len(patterns[bad[0]]), got[bad[0]], want[bad[0]], len(bad))


def check_text(ctx, t, patterns, shift=0, with_sa=True):
    """L of the text from the GPU; the count against fm_model, and against search_model and dev_sa_search on the text's suffix array"""
    t = u8(t)
    L, origin = gpu_bwt(ctx, t)
    d_bwt, idx = gpu_index(ctx, L, [len(t)], [origin], shift)
    got = gpu_count(ctx, d_bwt, [len(t)], idx, patterns)
    assert not first_difference(got, fm_model(L, origin, patterns), patterns), "n = %d, origin %d" % (len(t), origin)
    if with_sa:
        sa = gpu_sa(ctx, t)
        assert not first_difference(got, search_model(t, sa.host(), patterns), patterns), "against the suffix array's model, n = %d" % len(t)
        assert got == gpu_search(ctx, t, sa, patterns)
    return got, origin


# ---- the rank kernel alone -------------------------------------------------------------------------------------------------------------------

_rank_cases = {}


def rank_case(k, n):
    if (k, n) not in _rank_cases:
        L = np.random.default_rng(1000 * k + n).integers(0, k, size=n, dtype=np.uint8)
        present = np.unique(L)
        table = rank_model(L, present)
        pos = np.tile(np.arange(n + 1, dtype=np.int64), len(present))
        sym = np.repeat(present, n + 1)
        want = np.concatenate([table[int(c)] for c in present])
        _rank_cases[(k, n)] = (L, pos, sym, want)
    return _rank_cases[(k, n)]


@pytest.mark.parametrize("shift", [0, 1, 3, 8])
@pytest.mark.parametrize("n", [2100, 4097])
@pytest.mark.parametrize("k", [3, 256])
def test_rank_at_every_position(ctx, k, n, shift):
    """Occ_pack(c, i) for every i = 0 .. n and every symbol present: checkpoint borders, lane borders, every position mod 16"""
    L, pos, sym, want = rank_case(k, n)
    d_bwt, idx = gpu_index(ctx, L, [n], [0], shift)
    d_pos = torch.from_numpy(pos.astype(np.int32)).cuda()
    d_sym = torch.from_numpy(sym).cuda()
    out = Words(len(pos))
    ctx.dbg_dev_fm_rank(d_bwt, n, idx.t, d_pos, d_sym, out.t)
    assert out.guards_intact() and idx.guards_intact()
    got = out.host().astype(np.int64)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "symbol %d position %d: %d, expected %d (%d wrong)" % (sym[bad[0]], pos[bad[0]], got[bad[0]], want[bad[0]], bad.size)


# ---- every small text as a block of one pack --------------------------------------------------------------------------------------------------

def test_every_short_text_in_one_pack(ctx):
    """510 blocks of 1 .. 8 bytes: heads at every offset mod 16, hundreds of heads inside one checkpoint row; every pattern in every block"""
    blocks = [u8(t) for t in words(b"ab", range(1, 9))]
    sizes = [len(b) for b in blocks]
    assert len(blocks) == 510
    text = np.concatenate(blocks)
    off = np.concatenate([[0], np.cumsum(sizes)])
    d_in = dev_text(text)
    d_L = torch.empty(len(text), dtype=torch.uint8, device="cuda")
    d_sa = Words(len(text))
    origins = ctx.dev_suffix_array_packed(d_in, sizes, d_sa.t, d_L)
    d_L2 = torch.empty(len(text), dtype=torch.uint8, device="cuda")
    assert ctx.dev_bwt_forward_packed(d_in, sizes, d_L2) == origins and torch.equal(d_L, d_L2)
    L, sa = d_L.cpu().numpy(), d_sa.host()
    pats = words(b"abc", range(0, 5))
    every = [p for _ in blocks for p in pats]
    where = [b for b in range(len(blocks)) for _ in pats]
    d_bwt, idx = gpu_index(ctx, L, sizes, origins)
    got = gpu_count(ctx, d_bwt, sizes, idx, every, where)
    Ls = [L[off[b]:off[b + 1]] for b in range(len(blocks))]
    assert not first_difference(got, fm_model_packed(Ls, origins, every, where), every)
    want = [r for b in range(len(blocks)) for r in search_model(blocks[b], sa[off[b]:off[b + 1]], pats)]
    assert not first_difference(got, want, every)
    d_pat, lens = dev_patterns(every)
    lo, hi = Words(len(every)), Words(len(every))
    ctx.dev_sa_search_packed(d_in, sizes, d_sa.t, d_pat, lens, where, lo.t, hi.t)
    assert got == list(zip(lo.host().tolist(), hi.host().tolist()))


# ---- one symbol -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 3073])
def test_one_symbol(ctx, n):
    """a^k gives exactly (k - 1, n) for k <= n and (n, n) beyond; k chosen so that lo lands on and beside the checkpoint borders"""
    t = np.full(n, 97, np.uint8)
    ks = sorted(set(k for k in (1, 2, 3, 1024, 1025, 1026, 2048, 2049, n - 1, n, n + 1, n + 5) if k >= 1))
    pats = [b"a" * k for k in ks] + [b"", b"b", b"\x00", b"\xff", b"a" * (n // 2) + b"b", b"b" + b"a" * (n // 2), b"a" * (n // 2) + b"\x00"]
    got, origin = check_text(ctx, t, pats)
    assert origin == n - 1
    for k, r in zip(ks, got):
        assert r == ((k - 1, n) if k <= n else (n, n)), (n, k, r)
    assert got[len(ks)] == (0, n) and got[len(ks) + 1] == (n, n) and got[len(ks) + 2] == (0, 0) and got[len(ks) + 3] == (n, n)


# ---- the one-byte suffix and the origin -----------------------------------------------------------------------------------------------------------

def origin_cases():
    rng = np.random.default_rng(71)
    mid = rng.integers(98, 101, size=700, dtype=np.uint8)
    return {"slot 0": (np.concatenate([u8(b"a"), mid]), lambda n: 0),                            # the text is its own smallest suffix
            "slot n - 1": (np.concatenate([u8(b"z"), mid]), lambda n: n - 1),                    # ... its own largest
            "slot 1024": (np.concatenate([u8(b"b"), np.full(1024, 97, np.uint8), np.full(100, 99, np.uint8)]), lambda n: 1024),
            "slot 2048": (np.concatenate([u8(b"b"), np.full(2048, 97, np.uint8), rng.integers(99, 102, size=3000, dtype=np.uint8)]), lambda n: 2048),
            "banana": (u8(b"banana" * 300), None), "ends as it starts": (np.concatenate([u8(b"q"), mid, u8(b"q")]), None)}


@pytest.mark.parametrize("name", sorted(origin_cases()))
def test_last_byte_and_origin(ctx, name):
    t, where = origin_cases()[name]
    n = len(t)
    z = bytes(t[-1:])
    pats = [bytes(t), bytes(t) + b"a", bytes(t) + z, bytes(t[1:]), bytes(t[:-1]), z, z + z, z + bytes(t[:1]), bytes(t[:1]) + z, bytes(t[-2:]), bytes(t[-3:]),
            bytes(t[-40:]), z + bytes(t[:40]), bytes(t[-1:]) + bytes(t[-1:]) + bytes(t[-1:]), b""]
    pats += [z + p for p in words(bytes(np.unique(t)[:3]), range(1, 3))] + [p + z for p in words(bytes(np.unique(t)[:3]), range(1, 3))]
    pats += [bytes(t[a:a + m]) for a in (0, 1, n // 2, n - 9) for m in (1, 2, 3, 8)]
    got, origin = check_text(ctx, t, pats)
    if where:
        assert origin == where(n), (name, origin)
    assert got[0][1] - got[0][0] == 1 and got[0][0] == origin and got[1][0] == got[1][1]


# ---- bytes that are no BWT --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 3, 256])
def test_arbitrary_l(ctx, k):
    """the recurrence is defined for any L and any origin: the GPU equals the model, and lo <= hi <= n"""
    rng = np.random.default_rng(80 + k)
    for n in (1, 17, 5000):
        L = rng.integers(0, k, size=n, dtype=np.uint8)
        longest = 12 if k < 256 else 3
        pats = [rng.integers(0, k, size=int(rng.integers(0, longest + 1)), dtype=np.uint8) for _ in range(600)]
        pats += [L[a:a + 3][::-1].copy() for a in range(0, n, max(1, n // 50))]
        for origin in sorted({0, n - 1, int(rng.integers(0, n)), min(n - 1, 1024)}):
            d_bwt, idx = gpu_index(ctx, L, [n], [origin], shift=origin % 5)
            got = gpu_count(ctx, d_bwt, [n], idx, pats)
            assert not first_difference(got, fm_model(L, origin, pats), pats), (k, n, origin)
            assert all(lo <= hi <= n for lo, hi in got)


# ---- ordinary text --------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wiki(ctx):
    """text, its L and origin from the L-first path, the index, 4096 patterns and what the models say (computed once)"""
    t = u8(datagen.wiki_like((1 << 18) + 77, seed=9))
    L, origin = gpu_bwt(ctx, t)
    assert "lfirst" in ctx.stats()["routes"], ctx.stats()["routes"]
    rng = np.random.default_rng(91)
    pats = cut_patterns(t, rng, 4096, [1, 2, 8, 32, 300, 5000])
    want = fm_model(L, origin, pats)
    sa = gpu_sa(ctx, t)
    assert not first_difference(want, search_model(t, sa.host(), pats), pats), "the two models"
    d_bwt, idx = gpu_index(ctx, L, [len(t)], [origin], shift=3)
    return dict(t=t, L=L, origin=origin, pats=pats, want=want, sa=sa, d_bwt=d_bwt, idx=idx)


def test_text_from_the_lfirst_path(ctx, wiki):
    got = gpu_count(ctx, wiki["d_bwt"], [len(wiki["t"])], wiki["idx"], wiki["pats"], shifts=(1, 1, 3))
    assert not first_difference(got, wiki["want"], wiki["pats"])
    assert got == gpu_search(ctx, wiki["t"], wiki["sa"], wiki["pats"])
    found = sum(1 for lo, hi in got if hi > lo)
    assert 2048 <= found < 4096  # (the unchanged half occurs; of the changed half the short ones mostly do too)


@pytest.mark.parametrize("npat", [1, 3, 4, 5, 257])
def test_batches_around_a_workgroup(ctx, wiki, npat):
    for first in (0, 1000):
        pats = wiki["pats"][first:first + npat]
        assert gpu_count(ctx, wiki["d_bwt"], [len(wiki["t"])], wiki["idx"], pats) == wiki["want"][first:first + npat]


def test_no_patterns(ctx, wiki):
    lo, hi = Words(4), Words(4)
    ctx.dev_fm_count(wiki["d_bwt"], len(wiki["t"]), wiki["idx"].t, dev_text(u8(b"x")), [], lo.t, hi.t)
    ctx.dev_fm_count_packed(wiki["d_bwt"], [len(wiki["t"])], wiki["idx"].t, dev_text(u8(b"x")), [], [], lo.t, hi.t)
    assert lo.untouched() and hi.untouched()


# ---- packs ------------------------------------------------------------------------------------------------------------------------------------

def run_pack(ctx, blocks, pats_of, shift=0):
    """L and origins from dev_bwt_forward_packed; every pattern of pats_of(b) in block b, shuffled; against the model, and for every block
    against the single-block call"""
    sizes = [len(b) for b in blocks]
    off = np.concatenate([[0], np.cumsum(sizes)])
    d_in = dev_text(np.concatenate(blocks))
    d_L = torch.empty(int(off[-1]), dtype=torch.uint8, device="cuda")
    origins = ctx.dev_bwt_forward_packed(d_in, sizes, d_L)
    L = d_L.cpu().numpy()
    Ls = [L[off[b]:off[b + 1]] for b in range(len(blocks))]
    pats, where = [], []
    for b in range(len(blocks)):
        for p in pats_of(b):
            pats.append(u8(p))
            where.append(b)
    order = np.random.default_rng(len(pats)).permutation(len(pats))
    pats, where = [pats[i] for i in order], [where[i] for i in order]
    d_bwt, idx = gpu_index(ctx, L, sizes, origins, shift)
    got = gpu_count(ctx, d_bwt, sizes, idx, pats, where)
    assert not first_difference(got, fm_model_packed(Ls, origins, pats, where), pats)
    for b in range(len(blocks)):
        qs = [q for q in range(len(pats)) if where[q] == b]
        one_bwt, one_idx = gpu_index(ctx, Ls[b], [sizes[b]], [origins[b]])
        assert gpu_count(ctx, one_bwt, [sizes[b]], one_idx, [pats[q] for q in qs]) == [got[q] for q in qs], "block %d alone" % b
        want = search_model(blocks[b], np.array(sorted(range(sizes[b]), key=lambda i: bytes(blocks[b][i:]))), [pats[q] for q in qs]) if sizes[b] <= 3000 else None
        assert want is None or want == [got[q] for q in qs], "block %d against its suffix array" % b
    return got, pats, where


def test_pack_of_neighbours(ctx):
    """identical neighbours (nothing leaks across a head), a one-byte block between large ones, a one-symbol block"""
    rng = np.random.default_rng(101)
    piece = rng.integers(97, 100, size=12, dtype=np.uint8)
    same = np.concatenate([rng.integers(97, 100, size=1500, dtype=np.uint8), piece, rng.integers(97, 100, size=600, dtype=np.uint8)])
    big = u8(datagen.wiki_like(70001, seed=4))
    blocks = [same, same.copy(), same.copy(), big, u8(b"a"), big[:40000].copy(), np.full(2500, 97, np.uint8), u8(b"ab"), piece.copy(), u8(b"\x00")]

    def pats_of(b):
        t = blocks[b]
        return [piece, piece[:1], piece[:5], t, np.concatenate([t, [97]]), b"", b"a", b"aa", b"\x00", b"x", same[:300], same[-300:], big[1000:1300],
                bytes(t[-1:]) + bytes(t[:2]), b"a" * 1025, b"a" * 2500, b"a" * 2501]
    got, pats, where = run_pack(ctx, blocks, pats_of, shift=1)
    found = {b: got[q] for q, (p, b) in enumerate(zip(pats, where)) if len(p) == 12 and np.array_equal(p, piece)}
    assert [found[b][1] - found[b][0] for b in (0, 1, 2, 4, 8)] == [1, 1, 1, 0, 1]


def test_pack_fuzz(ctx):
    rng = np.random.default_rng(111)
    for trial in range(20):
        count = int(rng.integers(1, 24))
        k = int(rng.choice([1, 2, 4, 256]))
        lowest = 97 if k < 256 else 0
        blocks = [rng.integers(lowest, lowest + k, size=int(rng.choice([1, 2, 3, 15, 16, 17, 100, 1023, 1024, 1025, 2500])), dtype=np.uint8) for _ in range(count)]

        def pats_of(b):
            t = blocks[b]
            out = [b"", t, t[:1], t[-1:], np.concatenate([t[-1:], t[:1]])]
            for _ in range(6):
                a, m = int(rng.integers(0, len(t))), int(rng.choice([1, 2, 3, 8, 40]))
                p = t[a:a + m].copy()
                if rng.integers(0, 2):
                    p[-1] = lowest + (int(p[-1]) - lowest + 1) % max(k, 2)
                out.append(p)
            return out
        run_pack(ctx, blocks, pats_of, shift=trial % 4)


# ---- an index that is no index ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ["checkpoints", "everything"])
def test_containment(ctx, what):
    """results are unspecified but <= n_b, nothing outside the outputs is written, and the context goes on working"""
    rng = np.random.default_rng(121)
    blocks = [u8(datagen.wiki_like(5000, seed=3)), u8(b"a"), rng.integers(0, 256, size=3000, dtype=np.uint8), np.full(1500, 97, np.uint8)]
    sizes = [len(b) for b in blocks]
    total = sum(sizes)
    d_in = dev_text(np.concatenate(blocks))
    d_L = torch.empty(total, dtype=torch.uint8, device="cuda")
    origins = ctx.dev_bwt_forward_packed(d_in, sizes, d_L)
    d_bwt, idx = gpu_index(ctx, d_L.cpu().numpy(), sizes, origins)
    good = idx.host()
    rows = (total + FM_BLOCK - 1) // FM_BLOCK + 1
    bad = good.copy()
    span = slice(HEADER_WORDS, HEADER_WORDS + 256 * rows) if what == "checkpoints" else slice(0, len(bad))
    bad[span] = rng.integers(0, 1 << 32, size=len(bad[span]), dtype=np.uint64).astype(np.uint32)
    idx.t.copy_(torch.from_numpy(bad.view(np.int32)))
    pats, where = [], []
    for b in range(len(blocks)):
        for p in cut_patterns(blocks[b], rng, 60, [0, 1, 2, 5, 16, 300]) + [blocks[b]]:
            pats.append(p)
            where.append(b)
    got = np.array(gpu_count(ctx, d_bwt, sizes, idx, pats, where), np.int64)
    assert (got <= np.array(sizes)[where][:, None]).all()
    one = np.array(gpu_count(ctx, d_bwt, [total], idx, pats), np.int64)  # the same words read as the index of one block
    assert (one <= total).all()
    out = Words(64)
    ctx.dbg_dev_fm_rank(d_bwt, total, idx.t, torch.from_numpy(rng.integers(0, 1 << 31, size=64, dtype=np.int64).astype(np.int32)).cuda(),
                        torch.from_numpy(rng.integers(0, 256, size=64, dtype=np.uint8)).cuda(), out.t)
    assert out.guards_intact() and idx.guards_intact()
    idx.t.copy_(torch.from_numpy(good.view(np.int32)))
    Ls = np.split(d_L.cpu().numpy(), np.cumsum(sizes)[:-1])
    assert gpu_count(ctx, d_bwt, sizes, idx, pats, where) == fm_model_packed(Ls, origins, pats, where)


# ---- arguments -------------------------------------------------------------------------------------------------------------------------------------

def test_arguments(ctx):
    t = u8(b"banana" * 50)
    n = len(t)
    L, origin = gpu_bwt(ctx, t)
    d_bwt, idx = gpu_index(ctx, L, [n], [origin])
    before = idx.host()
    d_pat, lens = dev_patterns([b"ana", b"nab"])
    lo, hi = Words(2), Words(2)
    lib, h = ctx._lib, ctx._h
    p_bwt, p_idx, p_pat, p_lo, p_hi = (C.c_void_p(x.data_ptr()) for x in (d_bwt, idx.t, d_pat, lo.t, hi.t))
    ns, ls, bs, org = (C.c_size_t * 1)(n), (C.c_size_t * 2)(3, 3), (C.c_uint32 * 2)(0, 0), (C.c_uint32 * 1)(origin)
    odd = C.c_void_p(idx.t.data_ptr() + 2)
    # the build
    for args in ((None, n, origin, p_idx), (p_bwt, n, origin, None), (p_bwt, 0, 0, p_idx), (p_bwt, CAP + 1, origin, p_idx), (p_bwt, n, n, p_idx),
                 (p_bwt, n, 0xFFFFFFFF, p_idx), (p_bwt, n, origin, odd)):
        assert lib.dk_dev_fm_build(h, *args) == DK_E_ARG
    for args in ((None, 1, ns, org, p_idx), (p_bwt, 1, None, org, p_idx), (p_bwt, 1, ns, None, p_idx), (p_bwt, 1, ns, org, None), (p_bwt, 0, ns, org, p_idx),
                 (p_bwt, 1, ns, (C.c_uint32 * 1)(n), p_idx), (p_bwt, 1, ns, org, odd)):
        assert lib.dk_dev_fm_build_packed(h, *args) == DK_E_ARG
    for sizes, origins in (([300 - 1, 0], [0, 0]), ([(1 << 24) + 1], [0]), ([CAP, 1], [0, 0]), ([100, 200], [100, 0]), ([100, 200], [0, 200])):
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.dev_fm_build_packed(d_bwt, sizes, origins, idx.t)
        assert e.value.code == DK_E_ARG
    assert np.array_equal(idx.host(), before) and idx.guards_intact()
    # the count
    for args in ((None, n, p_idx, p_pat, 2, ls, p_lo, p_hi), (p_bwt, n, None, p_pat, 2, ls, p_lo, p_hi), (p_bwt, n, p_idx, None, 2, ls, p_lo, p_hi),
                 (p_bwt, n, p_idx, p_pat, 2, None, p_lo, p_hi), (p_bwt, n, p_idx, p_pat, 2, ls, None, p_hi), (p_bwt, n, p_idx, p_pat, 2, ls, p_lo, None),
                 (p_bwt, 0, p_idx, p_pat, 2, ls, p_lo, p_hi), (p_bwt, CAP + 1, p_idx, p_pat, 2, ls, p_lo, p_hi), (p_bwt, n, odd, p_pat, 2, ls, p_lo, p_hi),
                 (p_bwt, n, p_idx, p_pat, 2, (C.c_size_t * 2)(1 << 31, 1 << 31), p_lo, p_hi)):  # the last: 2^32 pattern bytes in all
        assert lib.dk_dev_fm_count(h, *args) == DK_E_ARG
    for args in ((None, 1, ns, p_idx, p_pat, 2, ls, bs, p_lo, p_hi), (p_bwt, 1, None, p_idx, p_pat, 2, ls, bs, p_lo, p_hi), (p_bwt, 1, ns, None, p_pat, 2, ls, bs, p_lo, p_hi),
                 (p_bwt, 1, ns, p_idx, None, 2, ls, bs, p_lo, p_hi), (p_bwt, 1, ns, p_idx, p_pat, 2, None, bs, p_lo, p_hi), (p_bwt, 1, ns, p_idx, p_pat, 2, ls, None, p_lo, p_hi),
                 (p_bwt, 1, ns, p_idx, p_pat, 2, ls, bs, None, p_hi), (p_bwt, 1, ns, p_idx, p_pat, 2, ls, bs, p_lo, None), (p_bwt, 0, ns, p_idx, p_pat, 2, ls, bs, p_lo, p_hi),
                 (p_bwt, 1, ns, p_idx, p_pat, 2, ls, (C.c_uint32 * 2)(0, 1), p_lo, p_hi)):  # the last: a block the pack does not have
        assert lib.dk_dev_fm_count_packed(h, *args) == DK_E_ARG
    # the rank
    d_pos, d_sym, out = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.uint8, device="cuda"), Words(2)
    p_pos, p_sym, p_out = (C.c_void_p(x.data_ptr()) for x in (d_pos, d_sym, out.t))
    for args in ((None, n, p_idx, p_pos, p_sym, 2, p_out), (p_bwt, n, None, p_pos, p_sym, 2, p_out), (p_bwt, n, p_idx, None, p_sym, 2, p_out),
                 (p_bwt, n, p_idx, p_pos, None, 2, p_out), (p_bwt, n, p_idx, p_pos, p_sym, 2, None), (p_bwt, 0, p_idx, p_pos, p_sym, 2, p_out)):
        assert lib.dk_dbg_dev_fm_rank(h, *args) == DK_E_ARG
    # the host form
    host_lo, host_hi = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    q_bwt, q_pat, q_lo, q_hi = (x.ctypes.data_as(C.c_void_p) for x in (L, u8(b"ananab"), host_lo, host_hi))
    for args in ((None, n, origin, q_pat, 2, ls, q_lo, q_hi), (q_bwt, 0, 0, q_pat, 2, ls, q_lo, q_hi), (q_bwt, CAP + 1, origin, q_pat, 2, ls, q_lo, q_hi),
                 (q_bwt, n, n, q_pat, 2, ls, q_lo, q_hi), (q_bwt, n, origin, None, 2, ls, q_lo, q_hi), (q_bwt, n, origin, q_pat, 2, None, q_lo, q_hi),
                 (q_bwt, n, origin, q_pat, 2, ls, None, q_hi), (q_bwt, n, origin, q_pat, 2, ls, q_lo, None)):
        assert lib.dk_fm_count(h, *args) == DK_E_ARG
    assert lo.untouched() and hi.untouched() and out.untouched() and not host_lo.any() and not host_hi.any()
    with dark_amd.Context(n, purpose="decoder") as small:  # patterns that do not fit the workspace beside L and its index
        big = np.zeros(small.stats()["ws_size_bytes"], np.uint8)
        with pytest.raises(dark_amd.DarkError) as e:
            small.fm_count(L, origin, [big])
        assert e.value.code == DK_E_ARG
        lo2, hi2 = small.fm_count(L, origin, [b"ana", b"nab"])
        assert list(zip(lo2.tolist(), hi2.tolist())) == fm_model(L, origin, [b"ana", b"nab"])
    assert gpu_count(ctx, d_bwt, [n], idx, [b"ana", b"nab"]) == fm_model(L, origin, [b"ana", b"nab"])


# ---- decoder contexts, and the workspace -----------------------------------------------------------------------------------------------------------

def test_decoder_context_serves_every_entry(ctx, wiki):
    t, L, origin, pats, want = wiki["t"], wiki["L"], wiki["origin"], wiki["pats"][:600], wiki["want"][:600]
    n = len(t)
    sizes = [1, 70000, 4097, n - 74098]
    off = np.concatenate([[0], np.cumsum(sizes)])
    d_PL = torch.empty(n, dtype=torch.uint8, device="cuda")
    origins = ctx.dev_bwt_forward_packed(dev_text(t), sizes, d_PL)
    PL = d_PL.cpu().numpy()
    where = [q % 4 for q in range(len(pats))]
    pack_want = fm_model_packed([PL[off[b]:off[b + 1]] for b in range(4)], origins, pats, where)
    for purpose in ("decoder", "full"):
        with dark_amd.Context(n, purpose=purpose, max_blocks=4) as exact:
            def within():
                st = exact.stats()
                assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], (purpose, st)
            d_bwt, idx = gpu_index(exact, L, [n], [origin])
            within()
            assert gpu_count(exact, d_bwt, [n], idx, pats) == want
            within()
            lo, hi = exact.fm_count(L, origin, pats)
            within()
            assert list(zip(lo.tolist(), hi.tolist())) == want
            p_bwt, p_idx = gpu_index(exact, PL, sizes, origins)
            within()
            assert gpu_count(exact, p_bwt, sizes, p_idx, pats, where) == pack_want
            within()
            if purpose == "decoder":
                assert np.array_equal(exact.bwt_inverse(L, origin), t)  # what the context was made for, after the queries
                with pytest.raises(dark_amd.DarkError) as e:  # five blocks on a context made for four
                    exact.dev_fm_build_packed(p_bwt, [1, 70000, 4097, 1000, n - 75098], origins + [0], Words(fm_index_bytes(n, 5) // 4).t)
                assert e.value.code == DK_E_ARG
                with pytest.raises(dark_amd.DarkError) as e:
                    exact.dev_fm_count_packed(p_bwt, [1, 70000, 4097, 1000, n - 75098], p_idx.t, dev_text(u8(b"ab")), [1], [0], Words(1).t, Words(1).t)
                assert e.value.code == DK_E_ARG


def test_tiny_decoder_contexts(ctx):
    """the build's chunk sums and the index of the host form fit the decoder workspace of the smallest blocks too"""
    for t in (b"a", b"ab", b"banana"):
        L, origin = gpu_bwt(ctx, u8(t))
        pats = words(b"abn", range(0, 4))
        with dark_amd.Context(len(t), purpose="decoder") as dec:
            lo, hi = dec.fm_count(L, origin, pats)
            assert list(zip(lo.tolist(), hi.tolist())) == fm_model(L, origin, pats)
            d_bwt, idx = gpu_index(dec, L, [len(t)], [origin])
            assert gpu_count(dec, d_bwt, [len(t)], idx, pats) == fm_model(L, origin, pats)
            st = dec.stats()
            assert st["ws_peak_bytes"] <= st["ws_size_bytes"]


# ---- the host form and the mirrors -----------------------------------------------------------------------------------------------------------------

def test_host_form_and_index_class(ctx, wiki):
    t, L, origin, pats, want = wiki["t"], wiki["L"], wiki["origin"], wiki["pats"][:500] + [b""], wiki["want"][:500] + [(0, len(wiki["t"]))]
    lo, hi = ctx.fm_count(L, origin, pats)
    assert lo.dtype == np.uint32 and hi.dtype == np.uint32 and list(zip(lo.tolist(), hi.tolist())) == want
    lo, hi = ctx.fm_count(L, origin, [])
    assert len(lo) == 0 and len(hi) == 0
    index = fm.Index.from_text(ctx, t)
    assert index.origins == [origin] and index.resident_bytes() <= 2 * len(t) + 4096
    lo, hi = index.count(pats)
    assert list(zip(lo.tolist(), hi.tolist())) == want
    assert index.occurrences(pats).tolist() == [h - l for l, h in want]
    with dark_amd.Context(len(t), purpose="decoder") as dec:
        index = fm.Index.from_bwt(dec, L, origin)  # (L, origin) in host memory, as a stream decoder leaves them
        assert index.occurrences(pats).tolist() == [h - l for l, h in want]
        sizes = [1000, len(t) - 1000]
        with pytest.raises(dark_amd.DarkError):  # a pack on a context made for one block
            fm.Index.from_bwt_packed(dec, index.d_bwt, sizes, [0, 0])
    packed = fm.Index.from_bwt_packed(ctx, index.d_bwt, [1000, len(t) - 1000], [5, 7])  # any bytes, any origins
    lo, hi = packed.count(pats[:50], [q & 1 for q in range(50)])
    assert list(zip(lo.tolist(), hi.tolist())) == fm_model_packed([L[:1000], L[1000:]], [5, 7], pats[:50], [q & 1 for q in range(50)])


def test_cpp_mirror(tmp_path):
    exe = str(tmp_path / "cpp_fm")
    lib_dir = os.path.join(ROOT, "dark_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_fm.cpp"),
                           "-L", lib_dir, "-ldark_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=TIMEOUT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cpp fm ok" in out.stdout
