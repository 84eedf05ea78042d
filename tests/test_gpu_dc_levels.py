"""The DC stage on the arrays of tests/dc_shapes.py: every level of the carry scans of csrc/dc.hip (tiles per chunk 1, 2, 3 and 9, short last
chunk, quarters of k_dc_carry_b, tiles per runscan thread) and of the k_pdc_* pass of csrc/packed.hip (block heads against tiles and steps, carries
that must stop at a block head, 256 symbols in k_pdc_final, tiles per chunk 1, 2 and 5, two iterations of k_pk_scan_u32), each compared entry by entry
with the oracle's orc.dc_encode.  tests/test_dc_shapes_host.py checks the same arrays and the oracle's side of them without a GPU."""
import numpy as np
import pytest
import torch

import dark_amd
import dc_shapes as S
from dark_amd._lib import DK_FLAG_HAS_FF, DK_FLAG_SINGLE_SYMBOL

pytestmark = pytest.mark.gpu
CAP = 17 << 20
PACK_CAP = 12 << 20
SINGLE_IDS = S.single_case_ids()
GUARD32, GUARD8 = 0x5A5A5A5A, 0xA5


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pctx():
    c = dark_amd.Context(PACK_CAP)
    yield c
    c.close()


def check_single(L, got, want, where):
    """init, d, sym, rank and m of one block against the oracle's; the first difference is reported with its place in the walk"""
    assert len(got["d"]) == len(want["d"]), "%s: m = %d, the oracle's %d" % (where, len(got["d"]), len(want["d"]))
    for key in ("init", "d", "sym", "rank"):
        bad = np.flatnonzero(np.asarray(got[key]) != np.asarray(want[key]))
        if len(bad):
            i = int(bad[0])
            pytest.fail("%s: %s differs in %d entries, first at %d: got %d, want %d -- %s" % (
                where, key, len(bad), i, int(got[key][i]), int(want[key][i]), S.where_is(L, key, i)))


def check_decodes(orc, L, got, where):
    back, used = orc.dc_decode(got["init"], got["d"], len(L))
    assert used == S.expected_used(L, len(got["d"])), "%s: the decoder read %d of %d distances" % (where, used, len(got["d"]))
    assert np.array_equal(back, L), "%s: the oracle does not decode the GPU's arrays to L" % where


@pytest.mark.parametrize("builder,tiles,r", SINGLE_IDS, ids=["%s-%d+%d" % i for i in SINGLE_IDS])
def test_single_block(ctx, orc, builder, tiles, r):
    c = S.single_case(builder, tiles, r)
    L = c["L"]
    want = orc.dc_encode(L)
    got = ctx.dc_encode(L)
    check_single(L, got, want, c["name"])
    check_decodes(orc, L, got, c["name"])


def test_device_pointer_entry(ctx, orc):
    """dk_dev_dc_encode on the 2 MiB + 1 sparse case (two tiles per chunk, one position in the last chunk), with and without d_rank"""
    c = S.single_case("sparse_alt", 512, 1)
    L, n = c["L"], c["n"]
    assert c["levels"]["tpc"] == 2
    want = orc.dc_encode(L)
    d_bwt = torch.from_numpy(L).cuda()
    for with_rank in (True, False):
        d_dist = torch.full((n,), GUARD32, dtype=torch.int32, device="cuda")
        d_sym = torch.full((n,), GUARD8, dtype=torch.uint8, device="cuda")
        d_rank = torch.full((n,), GUARD8, dtype=torch.uint8, device="cuda") if with_rank else None
        init, m = ctx.dev_dc_encode(d_bwt, n, d_dist, d_sym, d_rank)
        got = dict(init=init, d=d_dist[:m].cpu().numpy().view(np.uint32), sym=d_sym[:m].cpu().numpy(),
                   rank=d_rank[:m].cpu().numpy() if with_rank else want["rank"])
        check_single(L, got, want, "%s, d_rank %s" % (c["name"], "given" if with_rank else "None"))
    check_decodes(orc, L, got, c["name"])


# ---- packs ----
def pack_reference(orc, c):
    """what the packed call must leave in arrays the caller filled with guard values: block i's entries at [off_i, off_i + m_i)"""
    sizes = [len(b) for b in c["blocks"]]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    dist = np.full(c["total"], GUARD32, np.uint32)
    sym = np.full(c["total"], GUARD8, np.uint8)
    rank = np.full(c["total"], GUARD8, np.uint8)
    inits = np.empty((len(sizes), 256), np.uint32)
    for i, b in enumerate(c["blocks"]):
        w = orc.dc_encode(b)
        m = len(w["d"])
        assert m == c["ms"][i]
        a = int(off[i])
        dist[a:a + m], sym[a:a + m], rank[a:a + m], inits[i] = w["d"], w["sym"], w["rank"], w["init"]
    return sizes, off, dict(dist=dist, sym=sym, rank=rank), inits


def pack_where(c, off, index):
    blk = int(np.searchsorted(off, index, side="right")) - 1
    j = index - int(off[blk])
    if j >= c["ms"][blk]:
        return "block %d (%d bytes, %d runs): entry %d, past the block's runs -- the caller's guard value was overwritten" % (
            blk, len(c["blocks"][blk]), c["ms"][blk], j)
    run = int(c["rb"][blk]) + j
    tpc = c["levels"]["tpc"]
    return "block %d (%d bytes, runs %d..%d of the pack): its run %d = run %d of the pack, tile %d (run %d of it, step %d), chunk %d (tile %d of it)" % (
        blk, len(c["blocks"][blk]), int(c["rb"][blk]), int(c["rb"][blk + 1]) - 1, j, run, run // S.PDC_TILE, run % S.PDC_TILE,
        run % S.PDC_TILE // S.PDC_STEP, run // S.PDC_TILE // tpc, run // S.PDC_TILE % tpc)


def check_pack(c, off, want, want_init, inits, ms, got, where):
    """what a packed call returned (inits, ms) and left in the caller's arrays (got: dist, sym and, where given, rank, each over the range
    pack_reference covers) against pack_reference's"""
    assert ms == c["ms"], "%s: m of block %d" % (where, next(i for i in range(len(ms)) if ms[i] != c["ms"][i]))
    got_init = np.array(inits)
    bad = np.argwhere(got_init != want_init)
    assert len(bad) == 0, "%s: init[%d] of block %d is %d, the oracle's %d" % (
        where, bad[0][1], bad[0][0], got_init[bad[0][0], bad[0][1]], want_init[bad[0][0], bad[0][1]])
    for key, g in got.items():
        bad = np.flatnonzero(g != want[key])
        if len(bad):
            i = int(bad[0])
            pytest.fail("%s: %s differs in %d entries, first at %d: got %d, want %d -- %s" % (
                where, key, len(bad), i, int(g[i]), int(want[key][i]), pack_where(c, off, i)))


@pytest.mark.parametrize("name", list(S.PACKS))
def test_packed(pctx, orc, name):
    c = S.PACKS[name]()
    sizes, off, want, want_init = pack_reference(orc, c)
    total = c["total"]
    assert total <= PACK_CAP
    d_bwt = torch.from_numpy(np.concatenate(c["blocks"])).cuda()
    for with_rank in (True, False):
        d_dist = torch.full((total,), GUARD32, dtype=torch.int32, device="cuda")
        d_sym = torch.full((total,), GUARD8, dtype=torch.uint8, device="cuda")
        d_rank = torch.full((total,), GUARD8, dtype=torch.uint8, device="cuda") if with_rank else None
        inits, ms = pctx.dev_dc_encode_packed(d_bwt, sizes, d_dist, d_sym, d_rank)
        where = "pack %s, d_rank %s" % (name, "given" if with_rank else "None")
        got = dict(dist=d_dist.cpu().numpy().view(np.uint32), sym=d_sym.cpu().numpy())
        if with_rank:
            got["rank"] = d_rank.cpu().numpy()
        check_pack(c, off, want, want_init, inits, ms, got, where)


def oracle_stream(orc, model, t):
    if len(t) == 1:   # the oracle's SA-IS, like the reference's, takes no one-byte text: the suffix array by sorting, the rest as ever
        return orc.block_dc_encode_bwt(model, *orc.bwt_forward(t, orc.sa_naive(t)))
    return orc.block_dc_encode(model, t)


def test_compact_layout(pctx, orc):
    """dk_dev_packed_encode lays the pack's DC arrays out at the global run indices (the layout of dk_batch_push_packed): every coded stream and
    every flag word of a pack of some 3000 tiny texts and two of 70 KB against the oracle's"""
    texts = S.compact_texts()
    sizes = [len(t) for t in texts]
    d_in = torch.from_numpy(np.concatenate(texts)).cuda()
    want_flags = [(DK_FLAG_HAS_FF if (t == 0xFF).any() else 0) | (DK_FLAG_SINGLE_SYMBOL if len(np.unique(t)) == 1 else 0) for t in texts]
    assert {0, DK_FLAG_HAS_FF, DK_FLAG_SINGLE_SYMBOL, DK_FLAG_HAS_FF | DK_FLAG_SINGLE_SYMBOL} == set(want_flags)
    for model in ("dark", "rawdc"):
        streams, flags = pctx.dev_packed_encode(model, d_in, sizes, host_threads=4)
        assert flags == want_flags, "%s: flags of block %d" % (model, next(i for i in range(len(flags)) if flags[i] != want_flags[i]))
        for i, t in enumerate(texts):
            assert bytes(streams[i]) == oracle_stream(orc, model, t), "%s stream of block %d (%d bytes)" % (model, i, len(t))
