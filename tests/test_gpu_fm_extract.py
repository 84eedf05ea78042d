"""The FM-index's extract on the GPU (csrc/bwt.hip fm_extract_build_device, csrc/fm_index.hip k_fm_extract):
dk_dev_fm_extract_build / dk_dev_fm_extract, their packed and host forms, decoder contexts, and the mirrors.  The yardstick is the text itself.
One range (0, n) with max_len = n gives the whole text, which is the main lever here.  Every device output, and all structures, sit between
guards; the rows are byte buffers shifted by 0, 1 and 3 bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import dark_amd
from conftest import ROOT
from dark_amd import datagen, fm
from dark_amd._lib import DK_E_ARG, DK_E_STREAM, FM_NO_HIT
from dark_amd.context import fm_extract_bytes, fm_index_bytes, fm_locate_bytes, workspace_bytes
from fm_extract_model import anchors, extract_rows
from fm_locate_model import sa_plain
from fm_model import bwt_plain
from ibwt_model import invert
from test_gpu_fm import gpu_bwt, gpu_count, gpu_index, words
from test_gpu_fm_locate import every_short_l, gpu_structure, regime_text
from test_gpu_lcp import Words, dev_text, u8
from test_gpu_sa_search import cut_patterns

pytestmark = pytest.mark.gpu
CAP = 1 << 19
HEADER_WORDS = 64
TIMEOUT = 120
GUARD_BYTES, FILL_BYTE = 64, 0xA5


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


class Rows:
    """a uint8 device array of n bytes with GUARD_BYTES of FILL_BYTE on each side, `shift` bytes off its natural place"""

    def __init__(self, n, shift=0):
        self.n, self.lo = n, GUARD_BYTES + shift
        self.buf = torch.full((n + 2 * GUARD_BYTES + shift,), FILL_BYTE, dtype=torch.uint8, device="cuda")
        self.t = self.buf[self.lo:self.lo + n]

    def host(self):
        return self.buf.cpu().numpy()[self.lo:self.lo + self.n].copy()

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return bool((b[:self.lo] == FILL_BYTE).all() and (b[self.lo + self.n:] == FILL_BYTE).all())

    def untouched(self):
        return bool((self.buf.cpu().numpy() == FILL_BYTE).all())


def gpu_anchors(ctx, d_bwt, sizes, origins, step, shift=0, packed=None):
    """the extract structure of the pack in a Words; packed: take the packed entry (default: for more than one block)"""
    ext = Words(fm_extract_bytes(sum(sizes), len(sizes), step) // 4, shift)
    if len(sizes) > 1 if packed is None else packed:
        ctx.dev_fm_extract_build_packed(d_bwt, sizes, origins, step, ext.t)
    else:
        ctx.dev_fm_extract_build(d_bwt, sizes[0], origins[0], step, ext.t)
    assert ext.guards_intact(), "the build wrote outside the structure"
    return ext


def block_anchors(ext, sizes, step):
    """-> the anchors of every block, cut out of the structure by the bases the host computes"""
    w = ext.host().astype(np.int64)
    out, base = [], HEADER_WORDS
    for n in sizes:
        k = (n + step - 1) // step
        out.append(w[base:base + k].tolist())
        base += k
    assert base <= len(w)
    return out


def gpu_extract(ctx, d_bwt, sizes, idx, ext, step, ranges, max_len, blocks=None, shift=0, lens=True):
    """rows of dev_fm_extract(_packed) for (pos, len) ranges as a uint8 array of len(ranges) x max_len; lens=False: d_len = NULL"""
    nrange = len(ranges)
    pos, length = Words(nrange), Words(nrange)
    r = np.array(ranges, dtype=np.int64).reshape(nrange, 2)
    pos.t.copy_(torch.from_numpy(r[:, 0].astype(np.uint32).view(np.int32)))
    length.t.copy_(torch.from_numpy(r[:, 1].astype(np.uint32).view(np.int32)))
    out = Rows(nrange * max_len, shift)
    if blocks is None:
        ctx.dev_fm_extract(d_bwt, sizes[0], idx.t, ext.t, step, pos.t, length.t if lens else None, nrange, max_len, out.t)
    else:
        ctx.dev_fm_extract_packed(d_bwt, sizes, idx.t, ext.t, step, pos.t, length.t if lens else None, blocks, max_len, out.t)
    assert out.guards_intact() and pos.guards_intact() and length.guards_intact() and idx.guards_intact() and ext.guards_intact(), "a store left d_out"
    return out.host().reshape(nrange, max_len)


def whole_text(ctx, d_bwt, sizes, idx, ext, step, shift=0):
    """-> the text of every block, through one range (0, n_b) each"""
    count, most = len(sizes), max(sizes)
    rows = gpu_extract(ctx, d_bwt, sizes, idx, ext, step, [(0, n) for n in sizes], most, None if count == 1 else list(range(count)), shift)
    for b, n in enumerate(sizes):
        assert not rows[b, n:].any(), "block %d: bytes behind its %d" % (b, n)
    return [rows[b, :n] for b, n in enumerate(sizes)]


def same_rows(got, want, what=""):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s row %d byte %d: %d, expected %d (%d wrong)" % (what, bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])], len(bad))


def check_block(ctx, L, origin, t, step, shift=0):
    """one block: both builds, then the whole text"""
    n = len(L)
    d_bwt, idx = gpu_index(ctx, L, [n], [origin], shift)
    ext = gpu_anchors(ctx, d_bwt, [n], [origin], step)
    got = whole_text(ctx, d_bwt, [n], idx, ext, step, shift)[0]
    same_rows(got[None, :], u8(t)[None, :], "n = %d step %d origin %d:" % (n, step, origin))
    return d_bwt, idx, ext


# ---- every short text as a block of one pack -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def short_texts(ctx):
    """510 blocks of 1 .. 8 bytes, L from the packed forward transform, the index, and every (a, len) of every block"""
    blocks = [u8(t) for t in words(b"ab", range(1, 9))]
    sizes = [len(b) for b in blocks]
    assert len(blocks) == 510
    d_L = torch.empty(sum(sizes), dtype=torch.uint8, device="cuda")
    origins = ctx.dev_bwt_forward_packed(dev_text(np.concatenate(blocks)), sizes, d_L)
    for b in (0, 5, 200, 509):
        assert bwt_plain(blocks[b])[1] == origins[b]
    d_bwt, idx = gpu_index(ctx, d_L.cpu().numpy(), sizes, origins)
    ranges, where = [], []
    for b, n in enumerate(sizes):
        for a in range(n + 1):
            for length in range(n + 2 - a):
                ranges.append((a, length))
                where.append(b)
    assert len(ranges) == 23038
    want = np.concatenate([extract_rows(blocks[b], [r], 9) for b, r in zip(where, ranges)])
    return dict(blocks=blocks, sizes=sizes, origins=origins, d_bwt=d_bwt, idx=idx, ranges=ranges, where=where, want=want)


@pytest.mark.parametrize("step", [1, 2, 4, 64])
def test_every_short_text_in_one_pack(ctx, short_texts, step):
    s = short_texts
    sizes = s["sizes"]
    ext = gpu_anchors(ctx, s["d_bwt"], sizes, s["origins"], step)
    got = block_anchors(ext, sizes, step)
    for b in range(len(sizes)):
        assert got[b] == anchors(sa_plain(s["blocks"][b]), step), "block %d step %d" % (b, step)
    header = ext.host()[:5].tolist()
    assert header[1:] == [sum(sizes), len(sizes), step, sum(len(a) for a in got)]
    same_rows(gpu_extract(ctx, s["d_bwt"], sizes, s["idx"], ext, step, s["ranges"], 9, s["where"], shift=step & 3), s["want"], "step %d:" % step)


# ---- one symbol: the longest walks -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("step", [1, 32, 1024, 4096])
@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 2049])
def test_one_symbol(ctx, n, step):
    """a^n: every chunk's walk takes its full min(step, n) - 1 steps, and every step of the last chunk after the origin's own"""
    t = np.full(n, 97, np.uint8)
    d_bwt, idx, ext = check_block(ctx, t, n - 1, t, step)
    assert block_anchors(ext, [n], step)[0] == [n - 1 - k * step for k in range((n + step - 1) // step)]
    ranges = set()
    for k in sorted({0, 1, 2, n // step, n // step - 1, (n + step - 1) // step}):
        for a in (k * step - 1, k * step, k * step + 1):
            for length in (1, step - 1, step, step + 1):
                if a >= 0:
                    ranges.add((a, length))
    for end in (n - 1, n, n + 5):
        for length in (1, 2, step, step + 1):
            if end >= length:
                ranges.add((end - length, length))
    ranges = sorted(ranges)
    for shift in (0, 1, 3):
        same_rows(gpu_extract(ctx, d_bwt, [n], idx, ext, step, ranges, step + 1, shift=shift), extract_rows(t, ranges, step + 1), "shift %d" % shift)


# ---- the inverse's two regimes, origins on and off the splitter grid ----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["origin 0", "origin n - 1", "origin on the grid", "origin off the grid"])
@pytest.mark.parametrize("n", [65535, 65536])
def test_both_regimes_of_the_inverse(ctx, n, kind):
    """on both sides of the size at which the single-block inverse changes its splitter spacing (the structure's build has one spacing: nothing
    may depend on that border), with the origin's own splitter in every place it can take; the whole text through one range"""
    t, where = regime_text(n, kind)
    L, origin = gpu_bwt(ctx, t)
    assert origin == where and len(t) == n
    check_block(ctx, L, origin, t, 32, shift=n & 1)


# ---- ordinary text ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wiki(ctx):
    """2^18 + 77 bytes, L from the L-first path, the index and the structures at steps 8 and 32, 4096 ranges (computed once)"""
    t = u8(datagen.wiki_like((1 << 18) + 77, seed=9))
    n = len(t)
    L, origin = gpu_bwt(ctx, t)
    assert "lfirst" in ctx.stats()["routes"], ctx.stats()["routes"]
    d_bwt, idx = gpu_index(ctx, L, [n], [origin], shift=3)
    ext = {step: gpu_anchors(ctx, d_bwt, [n], [origin], step, shift=1) for step in (8, 32)}
    rng = np.random.default_rng(191)
    ranges = [(int(a), int(m)) for a, m in zip(rng.integers(0, n, size=4096), rng.integers(0, 301, size=4096))]
    ranges[:6] = [(n - 1, 300), (n, 5), (n - 300, 300), (n - 299, 300), (0, 300), (FM_NO_HIT, 300)]
    return dict(t=t, n=n, L=L, origin=origin, d_bwt=d_bwt, idx=idx, ext=ext, ranges=ranges)


@pytest.mark.parametrize("step", [8, 32])
def test_whole_text_from_the_lfirst_path(ctx, wiki, step):
    w = wiki
    got = whole_text(ctx, w["d_bwt"], [w["n"]], w["idx"], w["ext"][step], step, shift=1)[0]
    same_rows(got[None, :], w["t"][None, :], "step %d:" % step)


@pytest.mark.parametrize("max_len", [1, 7, 64, 300])
@pytest.mark.parametrize("step", [8, 32])
def test_ranges_of_the_lfirst_text(ctx, wiki, step, max_len):
    w = wiki
    got = gpu_extract(ctx, w["d_bwt"], [w["n"]], w["idx"], w["ext"][step], step, w["ranges"], max_len, shift=max_len & 3)
    same_rows(got, extract_rows(w["t"], w["ranges"], max_len))
    got = gpu_extract(ctx, w["d_bwt"], [w["n"]], w["idx"], w["ext"][step], step, w["ranges"], max_len, shift=1, lens=False)
    same_rows(got, extract_rows(w["t"], [(a, None) for a, _ in w["ranges"]], max_len), "d_len = NULL:")


@pytest.mark.parametrize("items", [1, 3, 4, 5, 257])
def test_batches_around_a_workgroup(ctx, wiki, items):
    w = wiki
    for first in (0, 1000):
        ranges = w["ranges"][first:first + items]
        for max_len, step in ((1, 8), (40, 32)):
            got = gpu_extract(ctx, w["d_bwt"], [w["n"]], w["idx"], w["ext"][step], step, ranges, max_len, shift=3)
            same_rows(got, extract_rows(w["t"], ranges, max_len))
    # one range of `items` chunks
    same_rows(gpu_extract(ctx, w["d_bwt"], [w["n"]], w["idx"], w["ext"][8], 8, [(5, 8 * items - 7)], 8 * items), extract_rows(w["t"], [(5, 8 * items - 7)], 8 * items))


def test_no_ranges(ctx, wiki):
    w = wiki
    pos, length, out = Words(4), Words(4), Rows(16)
    ctx.dev_fm_extract(w["d_bwt"], w["n"], w["idx"].t, w["ext"][8].t, 8, pos.t, length.t, 0, 4, out.t)
    ctx.dev_fm_extract_packed(w["d_bwt"], [w["n"]], w["idx"].t, w["ext"][8].t, 8, pos.t, length.t, [], 4, out.t)
    assert out.untouched()


def test_locate_then_extract(ctx, wiki):
    """d_pos straight from dev_fm_locate, DK_FM_NO_HIT entries included: every row with a hit is its pattern, every other row zeros"""
    w = wiki
    n, max_hits = w["n"], 3
    loc = gpu_structure(ctx, w["d_bwt"], [n], [w["origin"]], 32)
    rng = np.random.default_rng(193)
    for m in (3, 8, 17):
        pats = cut_patterns(w["t"], rng, 512, [m])  # (every second one with its last byte changed: mostly absent from 8 bytes on)
        ranges = gpu_count(ctx, w["d_bwt"], [n], w["idx"], pats)
        lo, hi, pos = Words(512), Words(512), Words(512 * max_hits)
        lo.t.copy_(torch.tensor([r[0] for r in ranges], dtype=torch.int32))
        hi.t.copy_(torch.tensor([r[1] for r in ranges], dtype=torch.int32))
        ctx.dev_fm_locate(w["d_bwt"], n, w["idx"].t, loc.t, 32, lo.t, hi.t, 512, max_hits, pos.t)
        out = Rows(512 * max_hits * m, shift=m & 3)
        ctx.dev_fm_extract(w["d_bwt"], n, w["idx"].t, w["ext"][8].t, 8, pos.t, None, 512 * max_hits, m, out.t)
        assert out.guards_intact() and pos.guards_intact()
        rows, hits = out.host().reshape(512, max_hits, m), pos.host().reshape(512, max_hits)
        found = missing = 0
        for q, p in enumerate(pats):
            for j in range(max_hits):
                if hits[q, j] == FM_NO_HIT:
                    missing += 1
                    assert not rows[q, j].any(), (m, q, j)
                else:
                    found += 1
                    assert bytes(rows[q, j]) == bytes(p), (m, q, j)
        assert found >= 256 and missing >= 256, (m, found, missing)


# ---- packs -----------------------------------------------------------------------------------------------------------------------------------

def run_pack(ctx, blocks, step, shift=0):
    """L and origins from the packed forward transform; every block's text from the pack's structures, from the block's own, and from
    dev_bwt_inverse_packed; then ranges in shuffled blocks"""
    sizes = [len(b) for b in blocks]
    off = np.concatenate([[0], np.cumsum(sizes)])
    text = np.concatenate(blocks)
    d_L = torch.empty(int(off[-1]), dtype=torch.uint8, device="cuda")
    origins = ctx.dev_bwt_forward_packed(dev_text(text), sizes, d_L)
    L = d_L.cpu().numpy()
    d_bwt, idx = gpu_index(ctx, L, sizes, origins, shift)
    ext = gpu_anchors(ctx, d_bwt, sizes, origins, step, packed=True)
    got = whole_text(ctx, d_bwt, sizes, idx, ext, step, shift)
    d_inv = torch.empty(int(off[-1]), dtype=torch.uint8, device="cuda")
    ctx.dev_bwt_inverse_packed(d_bwt, sizes, origins, d_inv)
    inv = d_inv.cpu().numpy()
    assert np.array_equal(inv, text)
    pack_anchors = block_anchors(ext, sizes, step)
    for b in range(len(blocks)):
        assert np.array_equal(got[b], inv[off[b]:off[b + 1]]), "block %d of %d bytes in the pack, step %d" % (b, sizes[b], step)
        one_bwt, one_idx = gpu_index(ctx, L[off[b]:off[b + 1]], [sizes[b]], [origins[b]])
        one_ext = gpu_anchors(ctx, one_bwt, [sizes[b]], [origins[b]], step)
        assert block_anchors(one_ext, [sizes[b]], step)[0] == pack_anchors[b], "block %d: its anchors alone and in the pack" % b
        assert np.array_equal(whole_text(ctx, one_bwt, [sizes[b]], one_idx, one_ext, step)[0], blocks[b]), "block %d alone" % b
    rng = np.random.default_rng(len(blocks))
    where = rng.integers(0, len(blocks), size=40).tolist()
    ranges = [(int(rng.integers(0, sizes[b] + 2)), int(rng.integers(0, 80))) for b in where]
    rows = gpu_extract(ctx, d_bwt, sizes, idx, ext, step, ranges, 70, where, shift=shift)
    same_rows(rows, np.concatenate([extract_rows(blocks[b], [r], 70) for b, r in zip(where, ranges)]))


def test_pack_of_neighbours(ctx):
    """identical neighbours (nothing leaks across a head), a one-byte block between two of 70000 bytes, a one-symbol block"""
    rng = np.random.default_rng(101)
    same = rng.integers(97, 100, size=2100, dtype=np.uint8)
    big = u8(datagen.wiki_like(70000, seed=4))
    run_pack(ctx, [same, same.copy(), same.copy(), big, u8(b"a"), big[::-1].copy(), np.full(2500, 97, np.uint8), u8(b"ab"), u8(b"\x00")], 32, shift=1)


def test_pack_fuzz(ctx):
    rng = np.random.default_rng(211)
    for trial in range(20):
        count = int(rng.integers(1, 12))
        k = int(rng.choice([1, 2, 4, 256]))
        lowest = 97 if k < 256 else 0
        blocks = [rng.integers(lowest, lowest + k, size=int(rng.choice([1, 2, 3, 31, 32, 33, 63, 64, 65, 100, 1023, 1024, 1025, 2500])), dtype=np.uint8)
                  for _ in range(count)]
        run_pack(ctx, blocks, int(rng.choice([1, 2, 8, 32, 64, 4096])), shift=trial % 4)


# ---- bytes that are no BWT ---------------------------------------------------------------------------------------------------------------------

def test_no_bwt(ctx):
    """every L of 1 .. 6 bytes over {a, b} with every origin: DK_E_STREAM exactly where the inverse's model finds no text, else the text"""
    texts = 0
    for L, origin in every_short_l():
        n = len(L)
        text = invert(L, origin, S=64).text
        d_bwt = dev_text(L)
        if text is None:
            with pytest.raises(dark_amd.DarkError) as e:
                gpu_anchors(ctx, d_bwt, [n], [origin], 2)
            assert e.value.code == DK_E_STREAM, (bytes(L), origin)
            with pytest.raises(dark_amd.DarkError) as e:  # ... exactly where the locate build gives it
                gpu_structure(ctx, d_bwt, [n], [origin], 2)
            assert e.value.code == DK_E_STREAM
        else:
            texts += 1
            check_block(ctx, L, origin, text, 2)
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
            gpu_anchors(ctx, dev_text(np.concatenate(Ls)), sizes, origins, 4)
        assert e.value.code == DK_E_STREAM and "block %d " % at in str(e.value) and "fm_extract_build_packed" in str(e.value), str(e.value)
    sizes = [len(good_L)] * 3
    d_bwt, idx = gpu_index(ctx, np.concatenate([good_L] * 3), sizes, [good_origin] * 3)
    ext = gpu_anchors(ctx, d_bwt, sizes, [good_origin] * 3, 4)
    assert [bytes(x) for x in whole_text(ctx, d_bwt, sizes, idx, ext, 4)] == [b"abracadabra"] * 3


# ---- structures that are none ----------------------------------------------------------------------------------------------------------------------

def test_containment(ctx):
    """any words in d_ext, then in the index too, then starts and lengths that are none: DK_OK, the guards intact, and every byte of every row
    is zero or a byte that occurs in the block's L"""
    rng = np.random.default_rng(231)
    step = 4
    blocks = [u8(datagen.wiki_like(2500, seed=3)), u8(b"a"), rng.integers(0, 200, size=1000, dtype=np.uint8), np.full(596, 97, np.uint8)]
    sizes = [len(b) for b in blocks]
    total = sum(sizes)
    assert total == 4097
    d_L = torch.empty(total, dtype=torch.uint8, device="cuda")
    origins = ctx.dev_bwt_forward_packed(dev_text(np.concatenate(blocks)), sizes, d_L)
    L = d_L.cpu().numpy()
    d_bwt, idx = gpu_index(ctx, L, sizes, origins)
    ext = gpu_anchors(ctx, d_bwt, sizes, origins, step)
    good_ext, good_idx = ext.host(), idx.host()
    where = [q % 4 for q in range(400)]
    allowed = []
    for b in range(4):
        ok = np.zeros(256, bool)
        ok[0] = True
        ok[np.unique(blocks[b])] = True  # (the bytes of a block's L are those of its text)
        allowed.append(ok)
    whole = np.zeros(256, bool)
    whole[0] = True
    whole[np.unique(L)] = True
    assert not whole.all() and not allowed[0].all()

    def contained(ranges, what, lens=True):
        got = gpu_extract(ctx, d_bwt, sizes, idx, ext, step, ranges, 37, where, shift=1, lens=lens)
        for q, b in enumerate(where):
            assert allowed[b][got[q]].all(), (what, q)
        one = gpu_extract(ctx, d_bwt, [total], idx, ext, step, ranges, 37, shift=3, lens=lens)  # the same words read as the structures of one block
        assert whole[one].all(), what

    proper = [(int(rng.integers(0, sizes[b] + 1)), int(rng.integers(0, 60))) for b in where]
    for what, span in (("anchors", slice(HEADER_WORDS, len(good_ext))), ("everything", slice(0, len(good_ext)))):
        bad = good_ext.copy()
        bad[span] = rng.integers(0, 1 << 32, size=len(bad[span]), dtype=np.uint64).astype(np.uint32)
        ext.t.copy_(torch.from_numpy(bad.view(np.int32)))
        contained(proper, what)
    idx.t.copy_(torch.from_numpy(rng.integers(0, 1 << 32, size=len(good_idx), dtype=np.uint64).astype(np.uint32).view(np.int32)))
    contained(proper, "a random index as well")
    wild = [(int(a), int(b)) for a, b in rng.integers(0, 1 << 32, size=(400, 2), dtype=np.uint64)]
    wild[:8] = [(0, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (2499, 1 << 31), (2500, 1), (0xFFFFFFFE, 2), (4096, 4098), (1 << 31, 1 << 31), (3, 0)]
    wild[8:200] = [(int(a) % 3000, int(b)) for a, b in wild[8:200]]
    contained(wild, "starts and lengths that are none")
    contained(wild, "starts that are none, no lengths", lens=False)
    ext.t.copy_(torch.from_numpy(good_ext.view(np.int32)))
    idx.t.copy_(torch.from_numpy(good_idx.view(np.int32)))
    contained(wild, "starts and lengths that are none, good structures")
    got = gpu_extract(ctx, d_bwt, sizes, idx, ext, step, wild, 37, where)
    same_rows(got, np.concatenate([extract_rows(blocks[b], [r], 37) for b, r in zip(where, wild)]), "good structures:")
    assert all(np.array_equal(a, b) for a, b in zip(whole_text(ctx, d_bwt, sizes, idx, ext, step), blocks))


# ---- decoder contexts, and the workspace -----------------------------------------------------------------------------------------------------------

# dk_workspace_bytes of the commit before this feature (host arithmetic): neither purpose's workspace grows for it
WORKSPACE_BEFORE = {("full", 1, 1): 67108933, ("decoder", 1, 1): 71680, ("full", 1025, 1): 67180229, ("decoder", 1025, 1): 86032,
                    ("full", 65536, 1): 71671808, ("decoder", 65536, 1): 1044224, ("full", 80000, 4): 72678864, ("decoder", 80000, 4): 1260002}


@pytest.mark.parametrize("purpose", ["decoder", "full"])
def test_contexts_sized_to_their_input(ctx, purpose):
    rng = np.random.default_rng(241)
    for n in (1, 1025, 65536):
        assert workspace_bytes(purpose, n, 1) == WORKSPACE_BEFORE[purpose, n, 1]
        t = rng.integers(97, 101, size=n, dtype=np.uint8)
        L, origin = gpu_bwt(ctx, t)
        with dark_amd.Context(n, purpose=purpose) as exact:
            assert exact.stats()["ws_size_bytes"] == WORKSPACE_BEFORE[purpose, n, 1]
            for step in (1, 32):
                check_block(exact, L, origin, t, step)
                st = exact.stats()
                assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], (purpose, n, step, st)
            if purpose == "decoder":
                assert np.array_equal(exact.bwt_inverse(L, origin), t)  # what the context was made for, after the queries
    sizes = [20000] * 4
    assert workspace_bytes(purpose, 80000, 4) == WORKSPACE_BEFORE[purpose, 80000, 4]
    t = rng.integers(97, 101, size=80000, dtype=np.uint8)
    d_L = torch.empty(80000, dtype=torch.uint8, device="cuda")
    origins = ctx.dev_bwt_forward_packed(dev_text(t), sizes, d_L)
    with dark_amd.Context(80000, purpose=purpose, max_blocks=4) as exact:
        for step in (1, 32):
            d_bwt, idx = gpu_index(exact, d_L.cpu().numpy(), sizes, origins)
            ext = gpu_anchors(exact, d_bwt, sizes, origins, step)
            st = exact.stats()
            assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], (purpose, step, st)
            got = whole_text(exact, d_bwt, sizes, idx, ext, step)
            assert all(np.array_equal(got[b], t[20000 * b:20000 * (b + 1)]) for b in range(4))
            st = exact.stats()
            assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], (purpose, step, st)
        if purpose == "decoder":
            with pytest.raises(dark_amd.DarkError) as e:  # five blocks on a context made for four
                exact.dev_fm_extract_build_packed(d_bwt, [16000] * 5, [0] * 5, 32, Words(fm_extract_bytes(80000, 5, 32) // 4).t)
            assert e.value.code == DK_E_ARG


# ---- arguments -------------------------------------------------------------------------------------------------------------------------------------

def test_arguments(ctx):
    t = u8(b"banana" * 50)
    n = len(t)
    L, origin = gpu_bwt(ctx, t)
    d_bwt, idx = gpu_index(ctx, L, [n], [origin])
    ext = gpu_anchors(ctx, d_bwt, [n], [origin], 8)
    before = ext.host()
    pos, length, out = Words(2), Words(2), Rows(8, shift=1)
    lib, h = ctx._lib, ctx._h
    p_bwt, p_idx, p_ext, p_pos, p_len, p_out = (C.c_void_p(x.data_ptr()) for x in (d_bwt, idx.t, ext.t, pos.t, length.t, out.t))
    ns, bs, org = (C.c_size_t * 1)(n), (C.c_uint32 * 2)(0, 0), (C.c_uint32 * 1)(origin)

    def odd(x):
        return C.c_void_p(x.t.data_ptr() + 2)
    # the build: null pointers, n, origin, the step, alignment
    for args in ((None, n, origin, 8, p_ext), (p_bwt, n, origin, 8, None), (p_bwt, 0, 0, 8, p_ext), (p_bwt, CAP + 1, origin, 8, p_ext), (p_bwt, n, n, 8, p_ext),
                 (p_bwt, n, 0xFFFFFFFF, 8, p_ext), (p_bwt, n, origin, 8, odd(ext)), (p_bwt, n, origin, 0, p_ext), (p_bwt, n, origin, 3, p_ext),
                 (p_bwt, n, origin, 8192, p_ext)):
        assert lib.dk_dev_fm_extract_build(h, *args) == DK_E_ARG, args
    for args in ((None, 1, ns, org, 8, p_ext), (p_bwt, 1, None, org, 8, p_ext), (p_bwt, 1, ns, None, 8, p_ext), (p_bwt, 1, ns, org, 8, None),
                 (p_bwt, 0, ns, org, 8, p_ext), (p_bwt, 1, ns, (C.c_uint32 * 1)(n), 8, p_ext), (p_bwt, 1, ns, org, 8, odd(ext)), (p_bwt, 1, ns, org, 6, p_ext)):
        assert lib.dk_dev_fm_extract_build_packed(h, *args) == DK_E_ARG, args
    for sizes, origins in (([300 - 1, 0], [0, 0]), ([(1 << 24) + 1], [0]), ([CAP, 1], [0, 0]), ([100, 200], [100, 0]), ([100, 200], [0, 200])):
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.dev_fm_extract_build_packed(d_bwt, sizes, origins, 8, ext.t)
        assert e.value.code == DK_E_ARG
    assert np.array_equal(ext.host(), before) and ext.guards_intact()
    # the query: null and misaligned pointers, n, the step, max_len, nrange x max_len, a block the pack does not have
    for args in ((None, n, p_idx, p_ext, 8, p_pos, p_len, 2, 4, p_out), (p_bwt, n, None, p_ext, 8, p_pos, p_len, 2, 4, p_out), (p_bwt, n, p_idx, None, 8, p_pos, p_len, 2, 4, p_out),
                 (p_bwt, n, p_idx, p_ext, 8, None, p_len, 2, 4, p_out), (p_bwt, n, p_idx, p_ext, 8, p_pos, p_len, 2, 4, None),
                 (p_bwt, 0, p_idx, p_ext, 8, p_pos, p_len, 2, 4, p_out), (p_bwt, CAP + 1, p_idx, p_ext, 8, p_pos, p_len, 2, 4, p_out),
                 (p_bwt, n, odd(idx), p_ext, 8, p_pos, p_len, 2, 4, p_out), (p_bwt, n, p_idx, odd(ext), 8, p_pos, p_len, 2, 4, p_out),
                 (p_bwt, n, p_idx, p_ext, 8, odd(pos), p_len, 2, 4, p_out), (p_bwt, n, p_idx, p_ext, 8, p_pos, odd(length), 2, 4, p_out),
                 (p_bwt, n, p_idx, p_ext, 5, p_pos, p_len, 2, 4, p_out), (p_bwt, n, p_idx, p_ext, 0, p_pos, p_len, 2, 4, p_out),
                 (p_bwt, n, p_idx, p_ext, 8, p_pos, p_len, 2, 0, p_out), (p_bwt, n, p_idx, p_ext, 8, p_pos, p_len, 2, (1 << 30) + 1, p_out),
                 (p_bwt, n, p_idx, p_ext, 8, p_pos, p_len, (1 << 31) + 1, 1, p_out)):
        assert lib.dk_dev_fm_extract(h, *args) == DK_E_ARG, args
    for args in ((None, 1, ns, p_idx, p_ext, 8, p_pos, p_len, 2, bs, 4, p_out), (p_bwt, 1, None, p_idx, p_ext, 8, p_pos, p_len, 2, bs, 4, p_out),
                 (p_bwt, 1, ns, None, p_ext, 8, p_pos, p_len, 2, bs, 4, p_out), (p_bwt, 1, ns, p_idx, None, 8, p_pos, p_len, 2, bs, 4, p_out),
                 (p_bwt, 1, ns, p_idx, p_ext, 8, None, p_len, 2, bs, 4, p_out), (p_bwt, 1, ns, p_idx, p_ext, 8, p_pos, p_len, 2, None, 4, p_out),
                 (p_bwt, 1, ns, p_idx, p_ext, 8, p_pos, p_len, 2, bs, 4, None), (p_bwt, 0, ns, p_idx, p_ext, 8, p_pos, p_len, 2, bs, 4, p_out),
                 (p_bwt, 1, ns, p_idx, p_ext, 8, p_pos, p_len, 2, bs, 0, p_out), (p_bwt, 1, ns, p_idx, p_ext, 7, p_pos, p_len, 2, bs, 4, p_out),
                 (p_bwt, 1, ns, p_idx, p_ext, 8, odd(pos), p_len, 2, bs, 4, p_out), (p_bwt, 1, ns, p_idx, p_ext, 8, p_pos, odd(length), 2, bs, 4, p_out),
                 (p_bwt, 1, ns, p_idx, p_ext, 8, p_pos, p_len, 2, bs, (1 << 30) + 1, p_out),
                 (p_bwt, 1, ns, p_idx, p_ext, 8, p_pos, p_len, 2, (C.c_uint32 * 2)(0, 1), 4, p_out)):
        assert lib.dk_dev_fm_extract_packed(h, *args) == DK_E_ARG, args
    # the host form
    host_pos, host_len, host_out = np.array([0, 3], np.uint32), np.array([4, 4], np.uint32), np.zeros(8, np.uint8)
    q_bwt, q_pos, q_len, q_out = (x.ctypes.data_as(C.c_void_p) for x in (L, host_pos, host_len, host_out))
    for args in ((None, n, origin, 8, q_pos, q_len, 2, 4, q_out), (q_bwt, 0, 0, 8, q_pos, q_len, 2, 4, q_out), (q_bwt, CAP + 1, origin, 8, q_pos, q_len, 2, 4, q_out),
                 (q_bwt, n, n, 8, q_pos, q_len, 2, 4, q_out), (q_bwt, n, origin, 12, q_pos, q_len, 2, 4, q_out), (q_bwt, n, origin, 8, None, q_len, 2, 4, q_out),
                 (q_bwt, n, origin, 8, q_pos, q_len, 2, 0, q_out), (q_bwt, n, origin, 8, q_pos, q_len, 2, 4, None),
                 (q_bwt, n, origin, 8, q_pos, q_len, 2, (1 << 30) + 1, q_out)):
        assert lib.dk_fm_extract(h, *args) == DK_E_ARG, args
    assert pos.untouched() and length.untouched() and out.untouched() and not host_out.any()
    with dark_amd.Context(n, purpose="decoder") as small:  # rows that do not fit the workspace beside L and the structures
        with pytest.raises(dark_amd.DarkError) as e:
            small.fm_extract(L, origin, [0] * 64, None, small.stats()["ws_size_bytes"] // 64, step=8)
        assert e.value.code == DK_E_ARG
    same_rows(gpu_extract(ctx, d_bwt, [n], idx, ext, 8, [(0, n)], n), t[None, :])


# ---- the host form and the mirrors -----------------------------------------------------------------------------------------------------------------

def test_host_form(ctx, wiki):
    w = wiki
    ranges = w["ranges"][:500] + [(0, 0)]
    with dark_amd.Context(w["n"], purpose="decoder") as dec:
        for c in (ctx, dec):
            rows = c.fm_extract(w["L"], w["origin"], [a for a, _ in ranges], [m for _, m in ranges], 64, step=32)
            assert rows.dtype == np.uint8 and rows.shape == (501, 64)
            same_rows(rows, extract_rows(w["t"], ranges, 64))
            rows = c.fm_extract(w["L"], w["origin"], [a for a, _ in ranges], None, 5, step=8)
            same_rows(rows, extract_rows(w["t"], [(a, None) for a, _ in ranges], 5), "no lengths:")
            assert c.fm_extract(w["L"], w["origin"], [], None, 5).shape == (0, 5)
            whole = c.fm_extract(w["L"], w["origin"], [0], None, 4096, step=32)
            assert np.array_equal(whole[0], w["t"][:4096])
        st = dec.stats()
        assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"]


def find_all(t, p):
    """every place p occurs in t, by bytes.find"""
    out, at = [], t.find(p)
    while at >= 0:
        out.append(at)
        at = t.find(p, at + 1)
    return out


def test_index_class(ctx, wiki):
    w = wiki
    n, t = w["n"], bytes(w["t"])
    plain = fm.Index.from_text(ctx, w["t"], locate_step=32)
    for call in (lambda: plain.extract([0], 5), lambda: plain.text(), lambda: plain.snippets([b"the"], 3, 3)):
        with pytest.raises(dark_amd.DarkError) as e:
            call()
        assert e.value.code == DK_E_ARG
    assert plain.extract_step is None and plain.resident_bytes() == n + fm_index_bytes(n) + fm_locate_bytes(n, 1, 32)
    only = fm.Index.from_text(ctx, w["t"], extract_step=32)
    assert only.resident_bytes() == n + fm_index_bytes(n) + fm_extract_bytes(n, 1, 32) <= 2.13 * n + 4096
    with pytest.raises(dark_amd.DarkError) as e:
        only.snippets([b"the"], 3, 3)  # needs the locate structure too
    assert e.value.code == DK_E_ARG
    assert only.text() == t and only.extract([], 5) == []
    starts = [0, 1, 31, 32, 33, n - 40, n - 1, n, n + 9, FM_NO_HIT] + [a for a, _ in w["ranges"][:200]]
    assert only.extract(starts, 40) == [t[a:a + 40] for a in starts]
    index = fm.Index.from_text(ctx, w["t"], locate_step=32, extract_step=8)
    assert index.resident_bytes() == plain.resident_bytes() + fm_extract_bytes(n, 1, 8)
    rng = np.random.default_rng(251)
    pats = [bytes(p) for p in cut_patterns(w["t"], rng, 200, [2, 3, 5, 9])] + [t[:4], t[n - 4:], t[n - 1:]]
    for before, after, max_hits in ((5, 7, 16), (0, 0, 2), (300, 1, 3)):
        got = index.snippets(pats, before, after, max_hits=max_hits)
        assert len(got) == len(pats)
        for q, p in enumerate(pats):
            places = find_all(t, p)
            assert len(got[q]) == min(len(places), max_hits), (q, p)
            for at, snippet in got[q]:
                assert at in places and snippet == t[max(at - before, 0):at + len(p) + after], (q, p, at)
            assert len({at for at, _ in got[q]}) == len(got[q])
    assert index.snippets([], 3, 3) == []
    with pytest.raises(dark_amd.DarkError) as e:
        fm.Index.from_text(ctx, w["t"][:1000], extract_step=48)
    assert e.value.code == DK_E_ARG
    with dark_amd.Context(n, purpose="decoder", max_blocks=2) as dec:
        index = fm.Index.from_bwt(dec, w["L"], w["origin"], extract_step=64)  # (L, origin) in host memory, as a stream decoder leaves them
        assert index.extract(starts[:50], 100) == [t[a:a + 100] for a in starts[:50]]
    blocks = [w["t"][:1000], w["t"][1000:5000]]
    sizes = [1000, 4000]
    d_L = torch.empty(5000, dtype=torch.uint8, device="cuda")
    origins = ctx.dev_bwt_forward_packed(dev_text(np.concatenate(blocks)), sizes, d_L)
    packed = fm.Index.from_bwt_packed(ctx, d_L, sizes, origins, locate_step=8, extract_step=16)
    assert [packed.text(0), packed.text(1)] == [bytes(b) for b in blocks]
    where = [q & 1 for q in range(60)]
    at = [17 * q for q in range(60)]
    assert packed.extract(at, 33, blocks=where) == [bytes(blocks[b][a:a + 33]) for a, b in zip(at, where)]
    some = [bytes(blocks[b][7 * q:7 * q + 1 + q % 3]) for q, b in enumerate(where)]
    got = packed.snippets(some, 4, 6, blocks=where, max_hits=5)
    for q, b in enumerate(where):
        tb = bytes(blocks[b])
        places = find_all(tb, some[q])
        assert len(got[q]) == min(len(places), 5) > 0
        assert all(a in places and s == tb[max(a - 4, 0):a + len(some[q]) + 6] for a, s in got[q]), q
    with pytest.raises(dark_amd.DarkError):
        packed.extract(at, 33)  # a pack needs the block of every range


def test_cpp_mirror(tmp_path):
    exe = str(tmp_path / "cpp_fm_extract")
    lib_dir = os.path.join(ROOT, "dark_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_fm_extract.cpp"),
                           "-L", lib_dir, "-ldark_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=TIMEOUT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cpp fm extract ok" in out.stdout
