"""The FM-index's locate on the GPU (csrc/bwt.hip fm_locate_build_device, csrc/fm_index.hip k_fm_locate):
dk_dev_fm_locate_build / dk_dev_fm_locate, their packed and host forms, decoder contexts, and the mirrors.  The yardstick is the suffix array:
from sorted suffixes for tiny inputs, from the GPU's suffix sort for larger ones.  The empty pattern's range [0, n) with max_hits = n gives the
whole suffix array, which is the main lever here.  Every device output, and both structures, sit between guard words."""
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
from dark_amd._lib import DK_E_ARG, DK_E_STREAM, FM_NO_HIT
from dark_amd.context import fm_index_bytes, fm_locate_bytes
from fm_locate_model import locate_rows, sa_plain
from fm_model import bwt_plain
from ibwt_model import invert
from test_gpu_fm import gpu_bwt, gpu_count, gpu_index, words
from test_gpu_lcp import Words, dev_text, u8
from test_gpu_sa_search import cut_patterns, gpu_sa

pytestmark = pytest.mark.gpu
CAP = 1 << 19
HEADER_WORDS = 64
TIMEOUT = 120


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


def gpu_structure(ctx, d_bwt, sizes, origins, step, shift=0, packed=None):
    """the locate structure of the pack in a Words; packed: take the packed entry (default: for more than one block)"""
    loc = Words(fm_locate_bytes(sum(sizes), len(sizes), step) // 4, shift)
    if len(sizes) > 1 if packed is None else packed:
        ctx.dev_fm_locate_build_packed(d_bwt, sizes, origins, step, loc.t)
    else:
        ctx.dev_fm_locate_build(d_bwt, sizes[0], origins[0], step, loc.t)
    assert loc.guards_intact(), "the build wrote outside the structure"
    return loc


def gpu_locate(ctx, d_bwt, sizes, idx, loc, step, ranges, max_hits, blocks=None, shift=0):
    """rows of dev_fm_locate(_packed) for (lo, hi) ranges, as an int64 array of len(ranges) x max_hits"""
    npat = len(ranges)
    lo, hi = Words(npat), Words(npat)
    r = np.array(ranges, dtype=np.int64).reshape(npat, 2)
    lo.t.copy_(torch.from_numpy(r[:, 0].astype(np.uint32).view(np.int32)))
    hi.t.copy_(torch.from_numpy(r[:, 1].astype(np.uint32).view(np.int32)))
    pos = Words(npat * max_hits, shift)
    if blocks is None:
        ctx.dev_fm_locate(d_bwt, sizes[0], idx.t, loc.t, step, lo.t, hi.t, npat, max_hits, pos.t)
    else:
        ctx.dev_fm_locate_packed(d_bwt, sizes, idx.t, loc.t, step, lo.t, hi.t, blocks, max_hits, pos.t)
    assert pos.guards_intact() and lo.guards_intact() and hi.guards_intact() and idx.guards_intact() and loc.guards_intact(), "a store left d_pos"
    return pos.host().astype(np.int64).reshape(npat, max_hits)


def whole_sa(ctx, d_bwt, sizes, idx, loc, step):
    """-> the suffix array of every block, through the range [0, n_b) of the empty pattern"""
    count, most = len(sizes), max(sizes)
    rows = gpu_locate(ctx, d_bwt, sizes, idx, loc, step, [(0, n) for n in sizes], most, None if count == 1 else list(range(count)))
    for b, n in enumerate(sizes):
        assert (rows[b, n:] == FM_NO_HIT).all(), "block %d: positions behind its %d slots" % (b, n)
    return [rows[b, :n] for b, n in enumerate(sizes)]


def same_rows(got, want, what=""):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s row %d hit %d: %d, expected %d (%d wrong)" % (what, bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])], len(bad))


def check_block(ctx, L, origin, sa, step, shift=0):
    """one block: both builds, then the whole suffix array"""
    n = len(L)
    d_bwt, idx = gpu_index(ctx, L, [n], [origin], shift)
    loc = gpu_structure(ctx, d_bwt, [n], [origin], step)
    got = whole_sa(ctx, d_bwt, [n], idx, loc, step)[0]
    same_rows(got[None, :], np.asarray(sa, dtype=np.int64)[None, :], "n = %d step %d origin %d:" % (n, step, origin))
    return d_bwt, idx, loc


# ---- every short text as a block of one pack -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def short_texts(ctx):
    """510 blocks of 1 .. 8 bytes, L and the suffix arrays from the packed sort, the index, the ranges of 121 patterns in every block"""
    blocks = [u8(t) for t in words(b"ab", range(1, 9))]
    sizes = [len(b) for b in blocks]
    assert len(blocks) == 510
    text = np.concatenate(blocks)
    off = np.concatenate([[0], np.cumsum(sizes)])
    d_L = torch.empty(len(text), dtype=torch.uint8, device="cuda")
    d_sa = Words(len(text))
    origins = ctx.dev_suffix_array_packed(dev_text(text), sizes, d_sa.t, d_L)
    sa = d_sa.host().astype(np.int64)
    sas = [sa[off[b]:off[b + 1]] for b in range(len(blocks))]
    for b in (0, 5, 200, 509):
        assert sas[b].tolist() == sa_plain(blocks[b])
    d_bwt, idx = gpu_index(ctx, d_L.cpu().numpy(), sizes, origins)
    pats = words(b"abc", range(0, 5))
    assert len(pats) == 121
    every = [p for _ in blocks for p in pats]
    where = [b for b in range(len(blocks)) for _ in pats]
    ranges = gpu_count(ctx, d_bwt, sizes, idx, every, where)
    want = np.concatenate([locate_rows(sas[b], ranges[121 * b:121 * (b + 1)], 8) for b in range(len(blocks))])
    return dict(sizes=sizes, origins=origins, sas=sas, d_bwt=d_bwt, idx=idx, ranges=ranges, where=where, want=want)


@pytest.mark.parametrize("step", [1, 2, 4, 64])
def test_every_short_text_in_one_pack(ctx, short_texts, step):
    s = short_texts
    sizes = s["sizes"]
    loc = gpu_structure(ctx, s["d_bwt"], sizes, s["origins"], step)
    got = whole_sa(ctx, s["d_bwt"], sizes, s["idx"], loc, step)
    for b in range(len(sizes)):
        assert got[b].tolist() == s["sas"][b].tolist(), "block %d step %d" % (b, step)
    same_rows(gpu_locate(ctx, s["d_bwt"], sizes, s["idx"], loc, step, s["ranges"], 8, s["where"]), s["want"], "step %d:" % step)


# ---- one symbol: the longest walks -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("step", [1, 32, 1024, 4096])
@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 2049])
def test_one_symbol(ctx, n, step):
    """a^n: the suffix array is n - 1 .. 0, and slot 0 is min(step, n) - 1 steps from its sample (step > n: only position 0 is sampled)"""
    check_block(ctx, np.full(n, 97, np.uint8), n - 1, np.arange(n - 1, -1, -1), step)


# ---- the inverse's two regimes, origins on and off the splitter grid ----------------------------------------------------------------------------

def regime_text(n, kind):
    rng = np.random.default_rng(n + len(kind))
    body = rng.integers(99, 102, size=n - 1, dtype=np.uint8)
    if kind == "origin 0":
        return np.concatenate([u8(b"a"), body]), 0               # the text is its own smallest suffix
    if kind == "origin n - 1":
        return np.concatenate([u8(b"z"), body]), n - 1           # ... its own largest
    k = 1024 if kind == "origin on the grid" else 1000           # b a^k ...: exactly the k suffixes that start with a are smaller than the text
    return np.concatenate([u8(b"b"), np.full(k, 97, np.uint8), body[:n - 1 - k]]), k


@pytest.mark.parametrize("kind", ["origin 0", "origin n - 1", "origin on the grid", "origin off the grid"])
@pytest.mark.parametrize("n", [65535, 65536])
def test_both_regimes_of_the_inverse(ctx, n, kind):
    """on both sides of the size at which the single-block inverse changes its splitter spacing (the structure's build has one spacing: nothing
    may depend on that border), with the origin's own splitter in every place it can take"""
    t, where = regime_text(n, kind)
    L, origin = gpu_bwt(ctx, t)
    assert origin == where and len(t) == n
    check_block(ctx, L, origin, gpu_sa(ctx, t).host(), 32, shift=n & 1)


# ---- ordinary text ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wiki(ctx):
    """2^18 + 77 bytes, L from the L-first path, both structures at step 32, the suffix array, 4096 patterns and their ranges (computed once)"""
    t = u8(datagen.wiki_like((1 << 18) + 77, seed=9))
    n = len(t)
    L, origin = gpu_bwt(ctx, t)
    assert "lfirst" in ctx.stats()["routes"], ctx.stats()["routes"]
    sa = gpu_sa(ctx, t).host().astype(np.int64)
    d_bwt, idx = gpu_index(ctx, L, [n], [origin], shift=3)
    loc = gpu_structure(ctx, d_bwt, [n], [origin], 32, shift=1)
    rng = np.random.default_rng(91)
    pats = cut_patterns(t, rng, 4096, [1, 2, 3, 8, 17, 32, 64])  # (every second one with its last byte changed: mostly absent from 8 bytes on)
    ranges = gpu_count(ctx, d_bwt, [n], idx, pats)
    return dict(t=t, n=n, L=L, origin=origin, sa=sa, d_bwt=d_bwt, idx=idx, loc=loc, pats=pats, ranges=ranges)


@pytest.mark.parametrize("max_hits", [1, 3, 16])
def test_text_from_the_lfirst_path(ctx, wiki, max_hits):
    w = wiki
    got = gpu_locate(ctx, w["d_bwt"], [w["n"]], w["idx"], w["loc"], 32, w["ranges"], max_hits, shift=max_hits & 1)
    same_rows(got, locate_rows(w["sa"], w["ranges"], max_hits))
    found = sum(1 for lo, hi in w["ranges"] if hi > lo)
    assert 2048 <= found < 4096
    for q in (0, 2, 100, 4094):  # the definition itself: the pattern stands at every position returned
        p = bytes(w["pats"][q])
        assert all(bytes(w["t"][a:a + len(p)]) == p for a in got[q] if a != FM_NO_HIT)


@pytest.mark.parametrize("items", [1, 3, 4, 5, 257])
def test_batches_around_a_workgroup(ctx, wiki, items):
    w = wiki
    for first in (0, 1000):
        ranges = w["ranges"][first:first + items]
        same_rows(gpu_locate(ctx, w["d_bwt"], [w["n"]], w["idx"], w["loc"], 32, ranges, 1), locate_rows(w["sa"], ranges, 1))
    same_rows(gpu_locate(ctx, w["d_bwt"], [w["n"]], w["idx"], w["loc"], 32, [(5, 5 + items)], items), locate_rows(w["sa"], [(5, 5 + items)], items))


def test_no_patterns(ctx, wiki):
    w = wiki
    lo, hi, pos = Words(4), Words(4), Words(4)
    ctx.dev_fm_locate(w["d_bwt"], w["n"], w["idx"].t, w["loc"].t, 32, lo.t, hi.t, 0, 4, pos.t)
    ctx.dev_fm_locate_packed(w["d_bwt"], [w["n"]], w["idx"].t, w["loc"].t, 32, lo.t, hi.t, [], 4, pos.t)
    assert pos.untouched()


# ---- packs -----------------------------------------------------------------------------------------------------------------------------------

def run_pack(ctx, blocks, step, shift=0):
    """L, origins and suffix arrays from the packed sort; every block's whole suffix array from the pack's structure and from the block's own"""
    sizes = [len(b) for b in blocks]
    off = np.concatenate([[0], np.cumsum(sizes)])
    d_L = torch.empty(int(off[-1]), dtype=torch.uint8, device="cuda")
    d_sa = Words(int(off[-1]))
    origins = ctx.dev_suffix_array_packed(dev_text(np.concatenate(blocks)), sizes, d_sa.t, d_L)
    L, sa = d_L.cpu().numpy(), d_sa.host().astype(np.int64)
    d_bwt, idx = gpu_index(ctx, L, sizes, origins, shift)
    loc = gpu_structure(ctx, d_bwt, sizes, origins, step, packed=True)
    got = whole_sa(ctx, d_bwt, sizes, idx, loc, step)
    for b in range(len(blocks)):
        want = sa[off[b]:off[b + 1]]
        assert np.array_equal(got[b], want), "block %d of %d bytes in the pack, step %d" % (b, sizes[b], step)
        one_bwt, one_idx = gpu_index(ctx, L[off[b]:off[b + 1]], [sizes[b]], [origins[b]])
        one_loc = gpu_structure(ctx, one_bwt, [sizes[b]], [origins[b]], step)
        assert np.array_equal(whole_sa(ctx, one_bwt, [sizes[b]], one_idx, one_loc, step)[0], want), "block %d alone" % b
    # a few ranges that a max_hits cuts, in shuffled blocks
    rng = np.random.default_rng(len(blocks))
    where = rng.integers(0, len(blocks), size=40).tolist()
    ranges = []
    for b in where:
        lo = int(rng.integers(0, sizes[b] + 1))
        ranges.append((lo, int(rng.integers(lo, sizes[b] + 1))))
    rows = gpu_locate(ctx, d_bwt, sizes, idx, loc, step, ranges, 5, where)
    want = np.concatenate([locate_rows(sa[off[b]:off[b + 1]], [r], 5) for b, r in zip(where, ranges)])
    same_rows(rows, want)


def test_pack_of_neighbours(ctx):
    """identical neighbours (nothing leaks across a head), a one-byte block between two of 70000 bytes, a one-symbol block"""
    rng = np.random.default_rng(101)
    same = rng.integers(97, 100, size=2100, dtype=np.uint8)
    big = u8(datagen.wiki_like(70000, seed=4))
    run_pack(ctx, [same, same.copy(), same.copy(), big, u8(b"a"), big[::-1].copy(), np.full(2500, 97, np.uint8), u8(b"ab"), u8(b"\x00")], 32, shift=1)


def test_pack_fuzz(ctx):
    rng = np.random.default_rng(111)
    for trial in range(20):
        count = int(rng.integers(1, 12))
        k = int(rng.choice([1, 2, 4, 256]))
        lowest = 97 if k < 256 else 0
        blocks = [rng.integers(lowest, lowest + k, size=int(rng.choice([1, 2, 3, 31, 32, 33, 63, 64, 65, 100, 1023, 1024, 1025, 2500])), dtype=np.uint8)
                  for _ in range(count)]
        run_pack(ctx, blocks, int(rng.choice([1, 2, 8, 32, 64, 4096])), shift=trial % 4)


# ---- bytes that are no BWT ---------------------------------------------------------------------------------------------------------------------

def every_short_l():
    return [(u8(bytes(w)), origin) for m in range(1, 7) for w in itertools.product(b"ab", repeat=m) for origin in range(m)]


def test_no_bwt(ctx):
    """every L of 1 .. 6 bytes over {a, b} with every origin: DK_E_STREAM exactly where the inverse's model finds no text, else the text's suffix array"""
    texts = 0
    for L, origin in every_short_l():
        n = len(L)
        text = invert(L, origin, S=64).text
        d_bwt = dev_text(L)
        if text is None:
            with pytest.raises(dark_amd.DarkError) as e:
                gpu_structure(ctx, d_bwt, [n], [origin], 2)
            assert e.value.code == DK_E_STREAM, (bytes(L), origin)
            with pytest.raises(dark_amd.DarkError) as e:  # ... exactly where the inverse gives it
                ctx.dev_bwt_inverse(d_bwt, n, origin, torch.empty(n, dtype=torch.uint8, device="cuda"))
            assert e.value.code == DK_E_STREAM
        else:
            texts += 1
            assert bwt_plain(text)[1] == origin and np.array_equal(bwt_plain(text)[0], L)
            check_block(ctx, L, origin, sa_plain(text), 2)
    assert texts == sum(2 ** m for m in range(1, 7))  # (every text has exactly one (L, origin))


def test_no_bwt_in_a_pack(ctx):
    """one bad block in a pack of three: the message names it; the same pack with a good block in its place builds"""
    good_t = u8(b"abracadabra")
    good_L, good_origin = bwt_plain(good_t)
    bad = [(L, origin) for L, origin in every_short_l() if invert(L, origin, S=64).text is None]
    assert len(bad) > 100
    for k, (L, origin) in enumerate(bad[::3]):
        at = k % 3
        Ls = [good_L, good_L, good_L]
        origins = [good_origin] * 3
        Ls[at], origins[at] = L, origin
        sizes = [len(x) for x in Ls]
        with pytest.raises(dark_amd.DarkError) as e:
            gpu_structure(ctx, dev_text(np.concatenate(Ls)), sizes, origins, 4)
        assert e.value.code == DK_E_STREAM and "block %d " % at in str(e.value), str(e.value)
    sizes = [len(good_L)] * 3
    d_bwt, idx = gpu_index(ctx, np.concatenate([good_L] * 3), sizes, [good_origin] * 3)
    loc = gpu_structure(ctx, d_bwt, sizes, [good_origin] * 3, 4)
    assert [x.tolist() for x in whole_sa(ctx, d_bwt, sizes, idx, loc, 4)] == [sa_plain(good_t)] * 3


# ---- structures that are none ----------------------------------------------------------------------------------------------------------------------

def test_containment(ctx):
    """any words in d_loc, then in the index too, then ranges that are none: DK_OK, every value < n_b or NO_HIT, nothing outside d_pos written"""
    rng = np.random.default_rng(131)
    step = 4
    blocks = [u8(datagen.wiki_like(2500, seed=3)), u8(b"a"), rng.integers(0, 256, size=1000, dtype=np.uint8), np.full(596, 97, np.uint8)]
    sizes = [len(b) for b in blocks]
    total = sum(sizes)
    assert total == 4097
    d_L = torch.empty(total, dtype=torch.uint8, device="cuda")
    origins = ctx.dev_bwt_forward_packed(dev_text(np.concatenate(blocks)), sizes, d_L)
    d_bwt, idx = gpu_index(ctx, d_L.cpu().numpy(), sizes, origins)
    loc = gpu_structure(ctx, d_bwt, sizes, origins, step)
    good_sa = whole_sa(ctx, d_bwt, sizes, idx, loc, step)
    good_loc, good_idx = loc.host(), idx.host()
    rows = (total + 1023) // 1024
    bits = slice(HEADER_WORDS + rows + 1, HEADER_WORDS + rows + 1 + 32 * rows)
    samples = slice(bits.stop, len(good_loc))
    where = [q % 4 for q in range(400)]
    limit = np.array(sizes)[where][:, None]

    def contained(ranges, what):
        got = gpu_locate(ctx, d_bwt, sizes, idx, loc, step, ranges, 7, where)
        assert ((got < limit) | (got == FM_NO_HIT)).all(), what
        one = gpu_locate(ctx, d_bwt, [total], idx, loc, step, ranges, 7)  # the same words read as the structures of one block
        assert ((one < total) | (one == FM_NO_HIT)).all(), what

    proper = []
    for b in where:
        lo = int(rng.integers(0, sizes[b] + 1))
        proper.append((lo, int(rng.integers(lo, sizes[b] + 1))))
    for what, span in (("mark bits", bits), ("samples", samples), ("everything", slice(0, len(good_loc)))):
        bad = good_loc.copy()
        bad[span] = rng.integers(0, 1 << 32, size=len(bad[span]), dtype=np.uint64).astype(np.uint32)
        loc.t.copy_(torch.from_numpy(bad.view(np.int32)))
        contained(proper, what)
    idx.t.copy_(torch.from_numpy(rng.integers(0, 1 << 32, size=len(good_idx), dtype=np.uint64).astype(np.uint32).view(np.int32)))
    contained(proper, "a random index as well")
    wild = [(int(a), int(b)) for a, b in rng.integers(0, 1 << 32, size=(400, 2), dtype=np.uint64)]
    wild[:8] = [(5, 3), (1, 0), (0, 1 << 31), (0, 0xFFFFFFFF), (0xFFFFFFFF, 0), (4096, 4098), (0, 4098), (1 << 31, 0xFFFFFFFF)]
    contained(wild, "ranges that are none")
    loc.t.copy_(torch.from_numpy(good_loc.view(np.int32)))
    idx.t.copy_(torch.from_numpy(good_idx.view(np.int32)))
    contained(wild, "ranges that are none, good structures")
    got = gpu_locate(ctx, d_bwt, sizes, idx, loc, step, wild[:2] + [(0, 1 << 31)], 7, [0, 0, 1])
    assert (got[:2] == FM_NO_HIT).all() and got[2].tolist() == good_sa[1].tolist() + [FM_NO_HIT] * 6  # hi < lo: no hits; hi > n: clamped
    assert all(np.array_equal(a, b) for a, b in zip(whole_sa(ctx, d_bwt, sizes, idx, loc, step), good_sa))


# ---- decoder contexts, and the workspace -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("purpose", ["decoder", "full"])
def test_contexts_sized_to_their_input(ctx, purpose):
    rng = np.random.default_rng(141)
    for n in (1, 1025, 65536):
        t = rng.integers(97, 101, size=n, dtype=np.uint8)
        L, origin = gpu_bwt(ctx, t)
        sa = gpu_sa(ctx, t).host()
        with dark_amd.Context(n, purpose=purpose) as exact:
            for step in (1, 32):
                check_block(exact, L, origin, sa, step)
                st = exact.stats()
                assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], (purpose, n, step, st)
            if purpose == "decoder":
                assert np.array_equal(exact.bwt_inverse(L, origin), t)  # what the context was made for, after the queries
    sizes = [20000] * 4
    t = rng.integers(97, 101, size=80000, dtype=np.uint8)
    d_L = torch.empty(80000, dtype=torch.uint8, device="cuda")
    d_sa = Words(80000)
    origins = ctx.dev_suffix_array_packed(dev_text(t), sizes, d_sa.t, d_L)
    sa = d_sa.host().astype(np.int64)
    with dark_amd.Context(80000, purpose=purpose, max_blocks=4) as exact:
        for step in (1, 32):
            d_bwt, idx = gpu_index(exact, d_L.cpu().numpy(), sizes, origins)
            loc = gpu_structure(exact, d_bwt, sizes, origins, step)
            got = whole_sa(exact, d_bwt, sizes, idx, loc, step)
            assert all(np.array_equal(got[b], sa[20000 * b:20000 * (b + 1)]) for b in range(4))
            st = exact.stats()
            assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], (purpose, step, st)
        if purpose == "decoder":
            with pytest.raises(dark_amd.DarkError) as e:  # five blocks on a context made for four
                exact.dev_fm_locate_build_packed(d_bwt, [16000] * 5, [0] * 5, 32, Words(fm_locate_bytes(80000, 5, 32) // 4).t)
            assert e.value.code == DK_E_ARG


# ---- arguments -------------------------------------------------------------------------------------------------------------------------------------

def test_arguments(ctx):
    t = u8(b"banana" * 50)
    n = len(t)
    L, origin = gpu_bwt(ctx, t)
    d_bwt, idx = gpu_index(ctx, L, [n], [origin])
    loc = gpu_structure(ctx, d_bwt, [n], [origin], 8)
    before = loc.host()
    lo, hi, pos = Words(2), Words(2), Words(8)
    lib, h = ctx._lib, ctx._h
    p_bwt, p_idx, p_loc, p_lo, p_hi, p_pos = (C.c_void_p(x.data_ptr()) for x in (d_bwt, idx.t, loc.t, lo.t, hi.t, pos.t))
    ns, bs, org = (C.c_size_t * 1)(n), (C.c_uint32 * 2)(0, 0), (C.c_uint32 * 1)(origin)

    def odd(x):
        return C.c_void_p(x.t.data_ptr() + 2)
    # the build: null pointers, n, origin, the step, alignment
    for args in ((None, n, origin, 8, p_loc), (p_bwt, n, origin, 8, None), (p_bwt, 0, 0, 8, p_loc), (p_bwt, CAP + 1, origin, 8, p_loc), (p_bwt, n, n, 8, p_loc),
                 (p_bwt, n, 0xFFFFFFFF, 8, p_loc), (p_bwt, n, origin, 8, odd(loc)), (p_bwt, n, origin, 0, p_loc), (p_bwt, n, origin, 3, p_loc),
                 (p_bwt, n, origin, 8192, p_loc)):
        assert lib.dk_dev_fm_locate_build(h, *args) == DK_E_ARG, args
    for args in ((None, 1, ns, org, 8, p_loc), (p_bwt, 1, None, org, 8, p_loc), (p_bwt, 1, ns, None, 8, p_loc), (p_bwt, 1, ns, org, 8, None),
                 (p_bwt, 0, ns, org, 8, p_loc), (p_bwt, 1, ns, (C.c_uint32 * 1)(n), 8, p_loc), (p_bwt, 1, ns, org, 8, odd(loc)), (p_bwt, 1, ns, org, 6, p_loc)):
        assert lib.dk_dev_fm_locate_build_packed(h, *args) == DK_E_ARG, args
    for sizes, origins in (([300 - 1, 0], [0, 0]), ([(1 << 24) + 1], [0]), ([CAP, 1], [0, 0]), ([100, 200], [100, 0]), ([100, 200], [0, 200])):
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.dev_fm_locate_build_packed(d_bwt, sizes, origins, 8, loc.t)
        assert e.value.code == DK_E_ARG
    assert np.array_equal(loc.host(), before) and loc.guards_intact()
    # the query: null and misaligned pointers, n, the step, max_hits, npat x max_hits, a block the pack does not have
    for args in ((None, n, p_idx, p_loc, 8, p_lo, p_hi, 2, 4, p_pos), (p_bwt, n, None, p_loc, 8, p_lo, p_hi, 2, 4, p_pos), (p_bwt, n, p_idx, None, 8, p_lo, p_hi, 2, 4, p_pos),
                 (p_bwt, n, p_idx, p_loc, 8, None, p_hi, 2, 4, p_pos), (p_bwt, n, p_idx, p_loc, 8, p_lo, None, 2, 4, p_pos), (p_bwt, n, p_idx, p_loc, 8, p_lo, p_hi, 2, 4, None),
                 (p_bwt, 0, p_idx, p_loc, 8, p_lo, p_hi, 2, 4, p_pos), (p_bwt, CAP + 1, p_idx, p_loc, 8, p_lo, p_hi, 2, 4, p_pos),
                 (p_bwt, n, odd(idx), p_loc, 8, p_lo, p_hi, 2, 4, p_pos), (p_bwt, n, p_idx, odd(loc), 8, p_lo, p_hi, 2, 4, p_pos),
                 (p_bwt, n, p_idx, p_loc, 8, odd(lo), p_hi, 2, 4, p_pos), (p_bwt, n, p_idx, p_loc, 8, p_lo, odd(hi), 2, 4, p_pos),
                 (p_bwt, n, p_idx, p_loc, 8, p_lo, p_hi, 2, 4, odd(pos)), (p_bwt, n, p_idx, p_loc, 5, p_lo, p_hi, 2, 4, p_pos),
                 (p_bwt, n, p_idx, p_loc, 8, p_lo, p_hi, 2, 0, p_pos), (p_bwt, n, p_idx, p_loc, 8, p_lo, p_hi, 2, (1 << 30) + 1, p_pos),
                 (p_bwt, n, p_idx, p_loc, 8, p_lo, p_hi, (1 << 31) + 1, 1, p_pos)):
        assert lib.dk_dev_fm_locate(h, *args) == DK_E_ARG, args
    for args in ((None, 1, ns, p_idx, p_loc, 8, p_lo, p_hi, 2, bs, 4, p_pos), (p_bwt, 1, None, p_idx, p_loc, 8, p_lo, p_hi, 2, bs, 4, p_pos),
                 (p_bwt, 1, ns, None, p_loc, 8, p_lo, p_hi, 2, bs, 4, p_pos), (p_bwt, 1, ns, p_idx, None, 8, p_lo, p_hi, 2, bs, 4, p_pos),
                 (p_bwt, 1, ns, p_idx, p_loc, 8, None, p_hi, 2, bs, 4, p_pos), (p_bwt, 1, ns, p_idx, p_loc, 8, p_lo, None, 2, bs, 4, p_pos),
                 (p_bwt, 1, ns, p_idx, p_loc, 8, p_lo, p_hi, 2, None, 4, p_pos), (p_bwt, 1, ns, p_idx, p_loc, 8, p_lo, p_hi, 2, bs, 4, None),
                 (p_bwt, 0, ns, p_idx, p_loc, 8, p_lo, p_hi, 2, bs, 4, p_pos), (p_bwt, 1, ns, p_idx, p_loc, 8, p_lo, p_hi, 2, bs, 0, p_pos),
                 (p_bwt, 1, ns, p_idx, p_loc, 7, p_lo, p_hi, 2, bs, 4, p_pos), (p_bwt, 1, ns, p_idx, p_loc, 8, p_lo, p_hi, 2, bs, 4, odd(pos)),
                 (p_bwt, 1, ns, p_idx, p_loc, 8, p_lo, p_hi, 2, (C.c_uint32 * 2)(0, 1), 4, p_pos)):
        assert lib.dk_dev_fm_locate_packed(h, *args) == DK_E_ARG, args
    # the host form
    host_lo, host_hi, host_pos = np.zeros(2, np.uint32), np.zeros(2, np.uint32), np.zeros(8, np.uint32)
    ls = (C.c_size_t * 2)(3, 3)
    q_bwt, q_pat, q_lo, q_hi, q_pos = (x.ctypes.data_as(C.c_void_p) for x in (L, u8(b"ananab"), host_lo, host_hi, host_pos))
    for args in ((None, n, origin, 8, q_pat, 2, ls, 4, q_lo, q_hi, q_pos), (q_bwt, 0, 0, 8, q_pat, 2, ls, 4, q_lo, q_hi, q_pos),
                 (q_bwt, CAP + 1, origin, 8, q_pat, 2, ls, 4, q_lo, q_hi, q_pos), (q_bwt, n, n, 8, q_pat, 2, ls, 4, q_lo, q_hi, q_pos),
                 (q_bwt, n, origin, 12, q_pat, 2, ls, 4, q_lo, q_hi, q_pos), (q_bwt, n, origin, 8, None, 2, ls, 4, q_lo, q_hi, q_pos),
                 (q_bwt, n, origin, 8, q_pat, 2, None, 4, q_lo, q_hi, q_pos), (q_bwt, n, origin, 8, q_pat, 2, ls, 0, q_lo, q_hi, q_pos),
                 (q_bwt, n, origin, 8, q_pat, 2, ls, 4, None, q_hi, q_pos), (q_bwt, n, origin, 8, q_pat, 2, ls, 4, q_lo, None, q_pos),
                 (q_bwt, n, origin, 8, q_pat, 2, ls, 4, q_lo, q_hi, None)):
        assert lib.dk_fm_locate(h, *args) == DK_E_ARG, args
    assert lo.untouched() and hi.untouched() and pos.untouched() and not host_lo.any() and not host_hi.any() and not host_pos.any()
    with dark_amd.Context(n, purpose="decoder") as small:  # a batch that does not fit the workspace beside L and the structures
        with pytest.raises(dark_amd.DarkError) as e:
            small.fm_locate(L, origin, [b""] * 64, max_hits=small.stats()["ws_size_bytes"] // 256, step=8)
        assert e.value.code == DK_E_ARG
    sa = sa_plain(t)
    same_rows(gpu_locate(ctx, d_bwt, [n], idx, loc, 8, [(0, n)], n), np.array(sa)[None, :])


# ---- the host form and the mirrors -----------------------------------------------------------------------------------------------------------------

def test_host_form(ctx, wiki):
    w = wiki
    pats = w["pats"][:500] + [b""]
    with dark_amd.Context(w["n"], purpose="decoder") as dec:
        for c in (ctx, dec):
            lo, hi, pos = c.fm_locate(w["L"], w["origin"], pats, max_hits=3, step=32)
            assert pos.dtype == np.uint32 and pos.shape == (501, 3)
            assert list(zip(lo.tolist(), hi.tolist())) == w["ranges"][:500] + [(0, w["n"])]
            same_rows(pos.astype(np.int64), locate_rows(w["sa"], list(zip(lo.tolist(), hi.tolist())), 3))
            lo, hi, pos = c.fm_locate(w["L"], w["origin"], [], max_hits=3)
            assert len(lo) == 0 and len(hi) == 0 and pos.shape == (0, 3)
        st = dec.stats()
        assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"]


def test_index_class(ctx, wiki):
    w = wiki
    pats, ranges = w["pats"][:500] + [b""], w["ranges"][:500] + [(0, w["n"])]
    plain = fm.Index.from_text(ctx, w["t"])
    with pytest.raises(dark_amd.DarkError) as e:
        plain.locate(pats)
    assert e.value.code == DK_E_ARG and plain.locate_step is None and plain.resident_bytes() == w["n"] + fm_index_bytes(w["n"])
    index = fm.Index.from_text(ctx, w["t"], locate_step=32)
    assert index.resident_bytes() == plain.resident_bytes() + fm_locate_bytes(w["n"], 1, 32) <= 2.27 * w["n"] + 4096
    lo, hi = index.count(pats)
    assert list(zip(lo.tolist(), hi.tolist())) == ranges
    for max_hits in (16, 2):  # (2 cuts most rows)
        got = index.locate(pats, max_hits=max_hits) if max_hits != 16 else index.locate(pats)
        assert len(got) == len(pats) and all(g.dtype == np.uint32 for g in got)
        for q, (lo_q, hi_q) in enumerate(ranges):
            assert got[q].tolist() == w["sa"][lo_q:min(hi_q, lo_q + max_hits)].tolist(), (q, max_hits)
    assert index.locate([]) == []
    with pytest.raises(dark_amd.DarkError) as e:
        fm.Index.from_text(ctx, w["t"][:1000], locate_step=48)
    assert e.value.code == DK_E_ARG
    with dark_amd.Context(w["n"], purpose="decoder", max_blocks=2) as dec:
        index = fm.Index.from_bwt(dec, w["L"], w["origin"], locate_step=64)  # (L, origin) in host memory, as a stream decoder leaves them
        assert [g.tolist() for g in index.locate(pats[:50], max_hits=4)] == [w["sa"][a:min(b, a + 4)].tolist() for a, b in ranges[:50]]
    blocks = [w["t"][:1000], w["t"][1000:5000]]
    sizes = [1000, 4000]
    d_L = torch.empty(5000, dtype=torch.uint8, device="cuda")
    d_sa = Words(5000)
    origins = ctx.dev_suffix_array_packed(dev_text(np.concatenate(blocks)), sizes, d_sa.t, d_L)
    sa = d_sa.host().astype(np.int64)
    packed = fm.Index.from_bwt_packed(ctx, d_L, sizes, origins, locate_step=8)
    where = [q & 1 for q in range(60)]
    some = [bytes(blocks[b][7 * q:7 * q + 1 + q % 3]) for q, b in enumerate(where)]
    lo, hi = packed.count(some, where)
    got = packed.locate(some, blocks=where, max_hits=5)
    for q, b in enumerate(where):
        assert hi[q] > lo[q] and got[q].tolist() == sa[1000 * b:][int(lo[q]):min(int(hi[q]), int(lo[q]) + 5)].tolist(), q
    with pytest.raises(dark_amd.DarkError):
        packed.locate(some)  # a pack needs the block of every pattern


def test_cpp_mirror(tmp_path):
    exe = str(tmp_path / "cpp_fm_locate")
    lib_dir = os.path.join(ROOT, "dark_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_fm_locate.cpp"),
                           "-L", lib_dir, "-ldark_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=TIMEOUT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cpp fm locate ok" in out.stdout
