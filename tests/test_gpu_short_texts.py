"""Every short text through the transform core, alone and in packs (tests/short_texts.py): suffix arrays, L and origins, LCP, the suffix-array
check, the inverse, distance coding and the coded streams of every binary text of 1 .. 15 bytes as one pack of 65 534 blocks (16 bits of block
id), of the same blocks behind other neighbours, of every short block in front of every 3-byte continuation, and of a pack that mixes three
alphabets with bytes 0x00 and 0xFF; every text of up to 10 bytes through the single-block entries; and every (L, origin) of up to 9 bytes,
text or not, through the inverse.  Whole concatenated arrays are compared with the plain models (tests/test_short_texts_host.py pins those
and shows that each pack tells the true model from three faulty ones); DC arrays and streams with the oracle.  The rounds a pack must take
are the host file's FIRST_KEY."""
import struct

import numpy as np
import pytest
import torch

import dark_amd
import dc_shapes as S
import ibwt_model as M
import short_texts as T
from dark_amd._lib import DK_E_STREAM
from test_gpu_dc_levels import GUARD32, GUARD8, check_pack, pack_reference
from test_gpu_inverse import FILL, Guarded, code_of, dev_at, judge, run_dev, run_host
from test_gpu_packed_sa import Outputs
from test_short_texts_host import FIRST_KEY, pairs_of

pytestmark = pytest.mark.gpu
MODELS = ("dark", "exp", "ybs", "simple")
ORACLE_BLOCKS = 8190   # of a bin15 pack's DC arrays the first 8190 blocks are compared with the oracle's, the rest by decoding
SINGLE_SETS = ("BIN10", "TER6", "EXT10")
OK = "ok"


@pytest.fixture(scope="module")
def ctx():
    """one full context, sized to the largest pack"""
    c = dark_amd.Context(max(sum(len(b) for b in T.pack(name).blocks) for name in T.PACK_NAMES))
    yield c
    c.close()


@pytest.fixture(scope="module")
def want():
    """name of a pack or of a text set -> its expected arrays, built once"""
    kept = {}

    def get(name):
        if name not in kept:
            kept[name] = T.expected(T.pack(name).blocks if name in T.PACK_NAMES else T.text_set(name))
        return kept[name]
    return get


def blocks_of(name):
    return T.pack(name).blocks if name in T.PACK_NAMES else T.text_set(name)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def dev_words(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).cuda()


def same(e, blocks, what, got, want_array):
    """whole arrays; a mismatch names the block, its text, the block behind it and the first differing entry"""
    got = np.asarray(got)
    assert got.shape == want_array.shape, what
    bad = np.flatnonzero(got != want_array)
    if len(bad):
        blk, j = T.block_of(e, int(bad[0]))
        pytest.fail("%s: %d entries differ, in %d blocks; the first in block %d (%r, %r behind it) at entry %d: got %d, want %d" % (
            what, len(bad), len(np.unique(np.searchsorted(e.off, bad, side="right"))), blk, blocks[blk],
            blocks[blk + 1] if blk + 1 < len(blocks) else None, j, int(got[bad[0]]), int(want_array[bad[0]])))


def same_origins(blocks, what, got, want_list):
    assert len(got) == len(want_list), what
    bad = np.flatnonzero(np.array(got, np.int64) != np.array(want_list, np.int64))
    if len(bad):
        i = int(bad[0])
        pytest.fail("%s: %d origins differ; the first is block %d (%r): got %d, want %d" % (what, len(bad), i, blocks[i], got[i], want_list[i]))


def sort_took(ctx, name, what):
    st = ctx.stats()
    assert st["rounds"] == FIRST_KEY[name][3], "%s: %d rounds, the first key of %d symbols asks for %d" % (what, st["rounds"], FIRST_KEY[name][2], FIRST_KEY[name][3])
    assert "packed_guard" not in st["routes"], what


# ---- a. packed suffix arrays, L and origins -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", T.PACK_NAMES)
def test_packed_suffix_arrays_and_l(ctx, want, name):
    e, blocks = want(name), blocks_of(name)
    d_in = dev(e.text)
    for with_bwt in (True, False):
        what = "pack %s, dev_suffix_array_packed %s L" % (name, "with" if with_bwt else "without")
        out = Outputs(e.total, with_bwt)
        origins = ctx.dev_suffix_array_packed(d_in, e.sizes, out.sa, out.bwt)
        sort_took(ctx, name, what)
        assert out.guards_intact(), what + ": a store left the outputs"
        same(e, blocks, what + ", suffix arrays", out.sa.cpu().numpy().view(np.uint32), e.sa)
        if with_bwt:
            same(e, blocks, what + ", L", out.bwt.cpu().numpy(), e.L)
            same_origins(blocks, what, origins, e.origin)
        else:
            assert origins is None
    what = "pack %s, dev_bwt_forward_packed" % name
    g = Guarded(e.total)
    origins = ctx.dev_bwt_forward_packed(d_in, e.sizes, g.view)
    sort_took(ctx, name, what)
    same(e, blocks, what + ", L", g.read(), e.L)
    same_origins(blocks, what, origins, e.origin)


# ---- b. packed LCP -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", T.PACK_NAMES)
def test_packed_lcp(ctx, want, name):
    e, blocks = want(name), blocks_of(name)
    d_in = dev(e.text)
    what = "pack %s, dev_suffix_array_packed_lcp" % name
    sa, lcp = Outputs(e.total, False), Outputs(e.total, False)
    ctx.dev_suffix_array_packed_lcp(d_in, e.sizes, sa.sa, lcp.sa)
    sort_took(ctx, name, what)
    assert sa.guards_intact() and lcp.guards_intact(), what + ": a store left the outputs"
    same(e, blocks, what + ", suffix arrays", sa.sa.cpu().numpy().view(np.uint32), e.sa)
    same(e, blocks, what + ", LCP", lcp.sa.cpu().numpy().view(np.uint32), e.lcp)
    what = "pack %s, dev_lcp_packed on the model's suffix arrays" % name
    lcp = Outputs(e.total, False)
    ctx.dev_lcp_packed(d_in, e.sizes, dev_words(e.sa), lcp.sa)
    assert lcp.guards_intact(), what + ": a store left the output"
    same(e, blocks, what, lcp.sa.cpu().numpy().view(np.uint32), e.lcp)


# ---- c. the suffix-array check -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", T.PACK_NAMES)
def test_packed_sa_check(ctx, want, name):
    e, blocks = want(name), blocks_of(name)
    got = ctx.dev_sa_check_packed(dev(e.text), e.sizes, dev_words(e.sa))
    bad = [i for i, (g, n) in enumerate(zip(got, e.sizes)) if g != (OK, n)]
    assert not bad, "pack %s: %d blocks' model suffix arrays refused; the first is block %d (%r): %r" % (name, len(bad), bad[0], blocks[bad[0]], got[bad[0]])


# ---- d. packed inverse -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", T.PACK_NAMES)
def test_packed_inverse(ctx, want, name):
    e, blocks = want(name), blocks_of(name)
    out = Guarded(e.total)
    ctx.dev_bwt_inverse_packed(dev(e.L), e.sizes, e.origin, out.view)
    same(e, blocks, "pack %s, dev_bwt_inverse_packed on the model's (L, origins)" % name, out.read(), e.text)


# ---- e. packed distance coding -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", T.PACK_NAMES)
def test_packed_dc(ctx, orc, want, name):
    """the arrays of dev_dc_encode_packed on the model's L, by tests/test_gpu_dc_levels.py's comparison with the oracle; of a bin15 pack the
    first ORACLE_BLOCKS blocks that way and every later block by what the oracle's decoder makes of its init table and distances"""
    e = want(name)
    count = len(e.sizes)
    head = ORACLE_BLOCKS if name.startswith("bin15") else count
    Ls = [e.L[e.off[i]:e.off[i + 1]] for i in range(count)]
    c = S._pack(name, Ls[:head])
    _, off, ref, ref_init = pack_reference(orc, c)
    d_bwt = dev(e.L)
    for with_rank in (True, False):
        d_dist = torch.full((e.total,), GUARD32, dtype=torch.int32, device="cuda")
        d_sym = torch.full((e.total,), GUARD8, dtype=torch.uint8, device="cuda")
        d_rank = torch.full((e.total,), GUARD8, dtype=torch.uint8, device="cuda") if with_rank else None
        inits, ms = ctx.dev_dc_encode_packed(d_bwt, e.sizes, d_dist, d_sym, d_rank)
        where = "pack %s, d_rank %s" % (name, "given" if with_rank else "None")
        dist = d_dist.cpu().numpy().view(np.uint32)
        got = dict(dist=dist[:c["total"]], sym=d_sym.cpu().numpy()[:c["total"]])
        if with_rank:
            got["rank"] = d_rank.cpu().numpy()[:c["total"]]
        check_pack(c, off, ref, ref_init, inits[:head], ms[:head], got, where)
        if with_rank:
            continue
        starts = np.concatenate([[True], e.L[1:] != e.L[:-1]])
        starts[e.off[:-1]] = True  # a run starts at every block head
        runs = np.add.reduceat(starts.astype(np.int64), e.off[:-1])
        assert ms == runs.tolist(), "%s: m of block %d" % (where, next(i for i in range(count) if ms[i] != runs[i]))
        for i in range(head, count):
            a = int(e.off[i])
            back, used = orc.dc_decode(inits[i], dist[a:a + ms[i]], e.sizes[i])
            assert used == S.expected_used(Ls[i], ms[i]) and np.array_equal(back, Ls[i]), \
                "%s: the oracle does not decode block %d (L = %r) from the GPU's arrays" % (where, i, Ls[i].tobytes())


# ---- f. coded streams of a pack ------------------------------------------------------------------------------------------------------------------

STREAMS = [("BIN10", m) for m in MODELS] + [("BIN12", "dark"), ("TER8", "dark"), ("EXT10", "dark"), ("EXT10", "dark+ff")]


@pytest.mark.parametrize("name,model", STREAMS, ids=["%s-%s" % s for s in STREAMS])
def test_packed_streams(ctx, orc, want, name, model):
    """every stream of dev_packed_encode is the oracle's for the model's (L, origin) -- one-symbol and one-byte blocks included, as in
    tests/test_gpu_parity.py::check_all_stages -- and dev_packed_decode gives the texts back (a plain stream cannot carry byte 0xFF; with the
    any-byte flag the stream is the u32 init[255] and then the plain stream)"""
    e, blocks = want(name), blocks_of(name)
    plain = model.split("+")[0]
    streams, _ = ctx.dev_packed_encode(model, dev(e.text), e.sizes, host_threads=8)
    for i, t in enumerate(blocks):
        L = e.L[e.off[i]:e.off[i + 1]]
        ref = orc.block_dc_encode_bwt(plain, L, e.origin[i])
        if model != plain:
            ref = struct.pack("<I", int(orc.dc_encode(L)["init"][255])) + ref
        assert bytes(streams[i]) == ref, "%s stream of block %d (%r) of %s" % (model, i, t, name)
    if model == plain and 0xFF in T.SETS[name][0]:
        return
    out = Guarded(e.total)
    ctx.dev_packed_decode(model, streams, e.sizes, out.view, host_threads=8)
    same(e, blocks, "%s: dev_packed_decode %s" % (name, model), out.read(), e.text)


# ---- g. the single-block entries ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def singles():
    """every text of SINGLE_SETS with the model's answers"""
    return [(t,) + T.answers(t) for name in SINGLE_SETS for t in T.text_set(name)]


def test_single_suffix_array(ctx, singles):
    for t, sa, L, origin, lcp in singles:
        assert ctx.suffix_array(t).tolist() == sa, t


def test_single_bwt_forward(ctx, singles):
    for t, sa, L, origin, lcp in singles:
        got, got_origin = ctx.bwt_forward(t)
        assert (got.tobytes(), got_origin) == (L, origin), t


def test_single_bwt_inverse(ctx, singles):
    for t, sa, L, origin, lcp in singles:
        assert ctx.bwt_inverse(L, origin).tobytes() == t, (t, L, origin)


def test_single_suffix_array_lcp(ctx, singles):
    for t, sa, L, origin, lcp in singles:
        got_sa, got_lcp = ctx.suffix_array_lcp(t)
        assert (got_sa.tolist(), got_lcp.tolist()) == (sa, lcp), t


def test_single_dc_encode(ctx, orc, singles):
    for t, sa, L, origin, lcp in singles:
        ref, got = orc.dc_encode(L), ctx.dc_encode(L)
        for key in ("init", "d", "sym", "rank"):
            assert np.array_equal(got[key], ref[key]), (t, L, key)


def test_single_device_pointers_off_alignment(ctx, orc, singles):
    """70 of the texts -- the six of one and two bytes over {a, b}, and 64 drawn -- through the dev_ entries, every byte pointer 1 byte past
    a 16-byte boundary, the outputs between guards"""
    assert [len(s[0]) for s in singles[:6]] == [1, 1, 2, 2, 2, 2]
    pick = list(range(6)) + sorted(6 + np.random.default_rng(70).choice(len(singles) - 6, size=64, replace=False)).copy()
    assert len(pick) == 70
    for k in pick:
        t, sa, L, origin, lcp = singles[int(k)]
        n = len(t)
        d_in, d_L = dev_at(np.frombuffer(t, np.uint8), 1), dev_at(np.frombuffer(L, np.uint8), 1)
        w = Outputs(n, False)
        ctx.dev_suffix_array(d_in, n, w.sa)
        assert w.guards_intact() and w.sa.cpu().numpy().tolist() == sa, ("dev_suffix_array", t)
        g = Guarded(n, 1)
        assert ctx.dev_bwt_forward(d_in, n, g.view) == origin and g.read().tobytes() == L, ("dev_bwt_forward", t)
        g = Guarded(n, 1)
        ctx.dev_bwt_inverse(d_L, n, origin, g.view)
        assert g.read().tobytes() == t, ("dev_bwt_inverse", t)
        w, w2 = Outputs(n, False), Outputs(n, False)
        ctx.dev_suffix_array_lcp(d_in, n, w.sa, w2.sa)
        assert w.guards_intact() and w2.guards_intact(), ("dev_suffix_array_lcp", t)
        assert (w.sa.cpu().numpy().tolist(), w2.sa.cpu().numpy().tolist()) == (sa, lcp), ("dev_suffix_array_lcp", t)
        ref = orc.dc_encode(L)
        w, g_sym, g_rank = Outputs(n, False), Guarded(n, 1), Guarded(n, 1)
        init, m = ctx.dev_dc_encode(d_L, n, w.sa, g_sym.view, g_rank.view)
        assert w.guards_intact() and m == len(ref["d"]) and np.array_equal(init, ref["init"]), ("dev_dc_encode", t)
        assert np.array_equal(w.sa.cpu().numpy().view(np.uint32)[:m], ref["d"]), ("dev_dc_encode d", t)
        assert np.array_equal(g_sym.read()[:m], ref["sym"]) and np.array_equal(g_rank.read()[:m], ref["rank"]), ("dev_dc_encode sym, rank", t)


# ---- h. every (L, origin) through the single-block inverse ---------------------------------------------------------------------------------------

PAIR_LENGTHS = [("ab", m) for m in range(1, 10)] + [("abc", m) for m in range(1, 6)]
BANANA = (np.frombuffer(b"nnbaaa", np.uint8), 3)


def all_pairs(ctx, alphabet, m, run, entry):
    """tests/test_gpu_inverse.py's invariant on every pair of length m: DK_OK means exactly the model's text, no text means DK_E_STREAM, the
    guard bytes stay (run checks them) either way; then the same context inverts a correct block"""
    texts, refused = 0, 0
    for L, origin in pairs_of(alphabet.encode(), m):
        L = np.frombuffer(L, np.uint8)
        v = M.invert(L, origin)
        rc, out, _ = run(ctx, L, origin)
        judge("L = %r, origin %d, %s" % (L.tobytes(), origin, entry), rc, out, v)
        texts += v.text is not None
        refused += rc == DK_E_STREAM
    assert (texts, refused) == (len(alphabet) ** m, (m - 1) * len(alphabet) ** m)
    assert ctx.bwt_inverse(*BANANA).tobytes() == b"banana", "the context does not invert a correct block after the last rejection"


@pytest.mark.parametrize("alphabet,m", PAIR_LENGTHS, ids=["%s%d" % p for p in PAIR_LENGTHS])
def test_pairs_host_inverse(ctx, alphabet, m):
    all_pairs(ctx, alphabet, m, run_host, "dk_bwt_inverse")


@pytest.mark.parametrize("alphabet,m", PAIR_LENGTHS, ids=["%s%d" % p for p in PAIR_LENGTHS])
def test_pairs_dev_inverse(ctx, alphabet, m):
    all_pairs(ctx, alphabet, m, run_dev, "dk_dev_bwt_inverse")


# ---- i. every pair that is no text, inside a pack ------------------------------------------------------------------------------------------------

def test_pairs_packed_inverse(ctx):
    """[good, good, bad, good]: DK_E_STREAM that names block 2 and writes nothing (include/dark_amd.h); the next call, with the bad block's
    place taken by the transform of a text of its length, gives all four texts"""
    good = [(b"nnbaaa", 3, b"banana")] + [T.answers(t)[1:3] + (t,) for t in (b"abracadabra", b"b")]
    bad = [(L, o) for m in range(1, 7) for L, o in pairs_of(b"ab", m) if M.invert(np.frombuffer(L, np.uint8), o).text is None]
    assert len(bad) == 516
    for L, o in bad:
        what = "L = %r, origin %d as block 2 of 4" % (L, o)
        fix = T.answers(L)[1:3] + (L,)  # L's bytes read as a text: a correct block of the same length
        for blk, refuse in ((L, o, None), True), (fix, False):
            pack = [good[0], good[1], blk, good[2]]
            sizes = [len(p[0]) for p in pack]
            out = Guarded(sum(sizes))
            rc, msg = code_of(ctx.dev_bwt_inverse_packed, dev_at(np.frombuffer(b"".join(p[0] for p in pack), np.uint8)), sizes,
                              [p[1] for p in pack], out.view)
            whole = out.read()
            if refuse:
                assert rc == DK_E_STREAM, "%s: no text, but the call returned %d" % (what, rc)
                assert "block 2 " in msg, msg
                assert (whole == FILL).all(), what + ": a rejected pack wrote to d_out"
            else:
                assert rc == 0, "%s: the call after the rejection returned %d (%s)" % (what, rc, msg)
                assert whole.tobytes() == b"".join(p[2] for p in pack), what + ": the call after the rejection"
