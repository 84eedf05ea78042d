"""One stage group on a poisoned workspace behind a poisoned mailbox: the process tests/test_gpu_poison_stages.py starts, once per (group, byte).

    python tests/poison_worker.py GROUP BYTE      with DARK_AMD_LIB = dark_amd/libdark_amd_tuning.so and DK_POISON = BYTE in the environment

Every context is opened by open_ctx: it proves that the library is the tuning build and that the poison is live (dbg_ws_peek returns BYTE for
every size asked, a multiple of 256 or not), then puts FillingLib between the context and the library, so that dk_dbg_mail_fill(BYTE) runs in
front of EVERY call that takes the context -- the helpers of the stage tests, imported from their files, need no change for that.  Results
are compared with the CPU models those helpers use (oracle/orc.py, ibwt_model, lcp_model, sa_query_model, fm_model, fm_locate_model,
fm_extract_model, rerank_model), never with another GPU run, unless a helper does both.  The shapes are the smallest that reach each route; a larger one
says why where it is defined."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dark_amd  # noqa: E402
from dark_amd import datagen  # noqa: E402
from dark_amd._lib import DK_E_ARG, DK_FLAG_HAS_FF, DK_FLAG_SINGLE_SYMBOL  # noqa: E402
from oracle import orc  # noqa: E402

TUNING_LIB = os.path.join(ROOT, "dark_amd", "libdark_amd_tuning.so")
GROUP, BYTE = sys.argv[1], int(sys.argv[2])
# entries that read a field of the context or end it: no fill in front of them (a fill is a call of its own and resets dk_last_error and
# dk_last_block_flags, as every call does)
ACCESSORS = {"dk_last_error", "dk_last_consumed", "dk_last_block_flags", "dk_capacity", "dk_ctx_purpose", "dk_get_stats", "dk_stats_reset",
             "dk_set_profiling", "dk_ctx_destroy", "dk_dbg_mail_fill", "dk_dbg_ws_peek"}
REPORT = dict(group=GROUP, byte=BYTE, contexts=0, peeks=0, fills=0, routes=set())


def say(what):
    sys.stderr.write("@@@ %s\n" % what)
    sys.stderr.flush()


class FillingLib:
    """the library as one context sees it: dk_dbg_mail_fill(BYTE) in front of every entry that is called with that context's handle (an open
    batch owns the mailbox: the fill, which the library refuses then, is left out)"""

    def __init__(self, lib, ctx):
        self._real, self._ctx = lib, ctx

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("dk_") or name in ACCESSORS:
            return fn

        def call(*args):
            c = self._ctx
            if args and args[0] is c._h and c._batch is None:
                rc = self._real.dk_dbg_mail_fill(c._h, BYTE)
                assert rc == 0, "dk_dbg_mail_fill in front of %s: %d" % (name, rc)
                REPORT["fills"] += 1
            return fn(*args)
        return call


def prove_poison(ctx):
    """every byte of a fresh allocation is BYTE, for sizes on and off the 256-byte grid and whatever the call before has left there"""
    size = ctx.stats()["ws_size_bytes"]
    for nbytes in (1, 255, 256, 257, 4097, 65536 + 3):
        got = ctx.dbg_ws_peek(min(nbytes, size))
        bad = np.flatnonzero(got != BYTE)
        assert bad.size == 0, "DK_POISON=%d is not live: byte %d of a fresh allocation of %d bytes is %d" % (BYTE, bad[0], len(got), got[bad[0]])
        REPORT["peeks"] += 1


def open_ctx(cap, purpose="full", max_blocks=1):
    ctx = dark_amd.Context(cap, purpose=purpose, max_blocks=max_blocks)
    real = ctx._lib
    assert os.path.realpath(real._name) == os.path.realpath(TUNING_LIB), "not the tuning library: %s" % real._name
    assert os.environ.get("DK_POISON") == str(BYTE)
    prove_poison(ctx)
    ctx._lib = FillingLib(real, ctx)
    REPORT["contexts"] += 1
    return ctx


def done_with(ctx):
    """the poison again, behind everything the group has run on the context; the peak inside the workspace"""
    prove_poison(ctx)
    st = ctx.stats()
    assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], st
    ctx.close()


def note_routes(ctx):
    REPORT["routes"] |= set(ctx.stats()["routes"])
    return ctx.stats()["routes"]


def u8(x):
    return np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8)


def oracle_sa(t):
    return orc.sa_sais(t) if len(t) > 1 else orc.sa_naive(t)


def oracle_bwt(t):
    return orc.bwt_forward(t, orc.sa_naive(t) if len(t) < 64 else None)


def oracle_stream(model, t):
    if len(t) == 1:  # (the oracle's SA-IS takes no one-byte text)
        return orc.block_dc_encode_bwt(model, *oracle_bwt(t))
    return orc.block_dc_encode(model, t)


def all_of(failures, what):
    assert not failures, "%s: %d failures\n%s" % (what, len(failures), "\n".join(failures[:20]))


# ---- DC: the carry levels of csrc/dc.hip and of the k_pdc_* pass ----------------------------------------------------------------------------
def group_dc():
    import dc_shapes as S
    from test_gpu_dc_levels import GUARD32, GUARD8, check_decodes, check_single, test_packed
    G = 64  # guard elements on each side of every output

    def dev_dc(ctx, L):
        n = len(L)
        bufs = [torch.full((n + 2 * G,), GUARD32, dtype=torch.int32, device="cuda")] + \
               [torch.full((n + 2 * G,), GUARD8, dtype=torch.uint8, device="cuda") for _ in range(2)]
        init, m = ctx.dev_dc_encode(torch.from_numpy(L).cuda(), n, *[b[G:G + n] for b in bufs])
        host = [b.cpu().numpy() for b in bufs]
        for h, fill in zip(host, (GUARD32, GUARD8, GUARD8)):
            h = h.view(np.uint32) if h.dtype == np.int32 else h
            assert (h[:G] == fill).all() and (h[G + n:] == fill).all(), "a store left the outputs"
        return dict(init=init, d=host[0].view(np.uint32)[G:G + m], sym=host[1][G:G + m], rank=host[2][G:G + m])

    # (builder, tiles, rest, tiles per chunk).  The levels of tests/dc_shapes.py are one, two, three and nine tiles per chunk: two tiles is the
    # smallest block with a carry at all; 2 MiB + 1, 4 MiB + 1 and 16 MiB + 1 are the first sizes of two and three tiles per chunk and of a
    # chunk with a second batch (each with a short last chunk).  No smaller block reaches those.
    singles = [("sparse_alt", 2, 0, 1), ("sparse_alt", 512, 1, 2), ("sparse_alt", 1024, 1, 3), ("sparse_alt", 4096, 1, 9)]
    packs = ["tiny", "all256", "1m+1_all_runs", "4m+tile+1"]  # one, two and five tiles per chunk, 256 symbols in k_pdc_final, a second scan iteration
    ctx = open_ctx(max(t * S.DC_TILE + r for _, t, r, _ in singles))
    for builder, tiles, r, tpc in singles:
        c = S.single_case(builder, tiles, r)
        say(c["name"])
        assert c["levels"]["tpc"] == tpc, c["levels"]
        want = orc.dc_encode(c["L"])
        for got in (ctx.dc_encode(c["L"]), dev_dc(ctx, c["L"])):
            check_single(c["L"], got, want, c["name"])
        check_decodes(orc, c["L"], got, c["name"])
    for name in packs:
        say("pack " + name)
        test_packed(ctx, orc, name)  # both layouts of d_rank, every entry against orc.dc_encode, the caller's guard values behind every block's runs
    done_with(ctx)


# ---- the inverse BWT, single and packed, full and decoder contexts ----------------------------------------------------------------------------
def group_inverse():
    import ibwt_model as M
    from test_gpu_inverse import check_correct, entry_dev, entry_packed, recovers, sample_text
    # 1: nothing to walk; 9 and 4097: splitters every 8 positions, one tile and two; 65537: splitters every 64 and the walk's records; and the
    # largest size of tests/test_gpu_inverse.py, 64 tiles and four thousand splitters, for "a few hundred thousand bytes"
    sizes = [1, 9, 4097, 65537, 262144 + 77]
    good = []
    for n, seed in ((3000, 7), (9001, 8)):
        t = sample_text(n, seed, 5)
        L, origin = oracle_bwt(t)
        good.append(dict(text=t, L=L, origin=origin))
    damaged = {}
    for n in (5000, 70000):
        _, _, _, cases = M.no_bwt_inputs(orc, n)
        damaged[n] = cases + [c for c in M.one_symbol() if M.spacing(len(c.L)) == M.spacing(n)]
        assert {c.kind for c in damaged[n]} >= set("abcdeg"), sorted({c.kind for c in damaged[n]})
    assert "f" in {c.kind for c in damaged[70000]}

    def no_bwt(ctx, n, what):
        failures = []
        for i, c in enumerate(damaged[n]):  # the verdict as ibwt_model says, the output untouched on DK_E_STREAM, a correct input afterwards
            for entry in (entry_dev, entry_packed):
                try:
                    entry(ctx, orc, good, c, i)
                except AssertionError as e:
                    failures.append(str(e).splitlines()[0])
        all_of(failures, "%s, n = %d" % (what, n))
        recovers(ctx, good)

    ctx = open_ctx(max(sizes) + 6)
    for n in sizes:
        say("correct n = %d" % n)
        check_correct(ctx, orc, sample_text(n, seed=n), "n = %d" % n)
    for n in damaged:
        say("no BWT n = %d" % n)
        no_bwt(ctx, n, "full context")
    done_with(ctx)
    for n in sizes:  # decoder contexts of exactly what check_correct sends: the block, and the pack of the block and six bytes
        say("decoder, correct n = %d" % n)
        dec = open_ctx(n + 6, "decoder", 2)
        check_correct(dec, orc, sample_text(n, seed=n), "decoder context, n = %d" % n)
        done_with(dec)
    for n in damaged:    # ... and of exactly the pack entry_packed sends: the input between the two good blocks
        say("decoder, no BWT n = %d" % n)
        dec = open_ctx(len(good[0]["L"]) + max(n, max(len(c.L) for c in damaged[n])) + len(good[1]["L"]), "decoder", 3)
        no_bwt(dec, n, "decoder context")
        done_with(dec)


# ---- the packed forward path, packed suffix arrays, the packed inverse and decode ------------------------------------------------------------------
def group_packed():
    import test_gpu_packed as PF
    import test_gpu_packed_decode as PD
    import test_gpu_packed_sa as PS
    from test_gpu_inverse import Guarded, run_packed

    def dc_reference(blocks):
        out = []
        for b in blocks:
            bwt, origin = oracle_bwt(b)
            w = orc.dc_encode(bwt)
            out.append(dict(bwt=bwt, origin=origin, init=w["init"], m=len(w["d"]), dist=w["d"], sym=w["sym"], rank=w["rank"]))
        return out

    fwd, sa_blocks, inv_blocks, dec_blocks = PF.mixed_blocks(), PS.mixed_blocks(), PD.mixed_blocks(orc), PD.decode_blocks()
    # Two identical halves that outlast the round limit.  The pack holds every byte value (9 bits a symbol) in two blocks (1 bit), so the first
    # key holds (64 - 1) / 9 = 7 symbols and twelve doublings compare 7 * 2^12 = 28 672: halves of 28 700 random bytes are the smallest round
    # number above it.
    half = np.random.default_rng(17).integers(0, 256, size=28700, dtype=np.uint8)
    guard_pack = [np.arange(256, dtype=np.uint8), np.concatenate([half, half])]
    # one pack for the five models: every tiny size, the tile's borders, periodic blocks, one symbol, bytes 0xFF
    models_pack = fwd[:7] + [u8(b"ab" * 3000), u8(b"abc" * 2000 + b"abd"), np.full(777, 0x41, np.uint8), u8(b"x\xffy\xff\xff" * 300)]
    ctx = open_ctx(max(sum(len(b) for b in p) for p in (fwd, sa_blocks, inv_blocks, dec_blocks, guard_pack, models_pack)))

    say("packed forward: mixed_blocks")
    PF.check_pack(ctx, fwd, ref=dc_reference(fwd))  # L, origin, init, m, dist, sym, rank of every block against the oracle's
    note_routes(ctx)
    say("packed suffix arrays: mixed_blocks")
    sas, bwts, origins, routes = PS.run_pack(ctx, sa_blocks, with_bwt=True)
    REPORT["routes"] |= set(routes)
    for i, b in enumerate(sa_blocks):
        assert np.array_equal(sas[i], oracle_sa(b)), "suffix array of block %d (%d bytes)" % (i, len(b))
        L, origin = oracle_bwt(b)
        assert np.array_equal(bwts[i], L) and origins[i] == origin, "L / origin of block %d" % i
    sas, _, _, _ = PS.run_pack(ctx, sa_blocks, with_bwt=False)
    for i, b in enumerate(sa_blocks):
        assert np.array_equal(sas[i], oracle_sa(b)), "suffix array of block %d without L" % i

    say("the packed guard")
    sas, bwts, origins, routes = PS.run_pack(ctx, guard_pack, with_bwt=True)
    assert "packed_guard" in routes, routes
    REPORT["routes"] |= set(routes)
    for i, b in enumerate(guard_pack):
        L, origin = oracle_bwt(b)
        assert np.array_equal(sas[i], oracle_sa(b)) and np.array_equal(bwts[i], L) and origins[i] == origin, "guard pack, block %d" % i
    PF.check_pack(ctx, guard_pack, ref=dc_reference(guard_pack))
    assert "packed_guard" in PF.check_pack.routes, PF.check_pack.routes

    say("packed inverse: mixed_blocks")
    pairs = [oracle_bwt(b) for b in inv_blocks]
    rc, outs, msg = run_packed(ctx, pairs)
    assert rc == 0, msg
    for i, b in enumerate(inv_blocks):
        assert np.array_equal(outs[i], b), "packed inverse, block %d (%d bytes, origin %d)" % (i, len(b), pairs[i][1])
    say("packed decode")
    sizes = [len(b) for b in dec_blocks]
    out = Guarded(sum(sizes))
    ctx.dev_packed_decode("exp", [oracle_stream("exp", b) for b in dec_blocks], sizes, out.view, host_threads=4)
    assert np.array_equal(out.read(), np.concatenate(dec_blocks)), "dev_packed_decode of the oracle's streams"

    say("packed encode, five models")
    sizes = [len(b) for b in models_pack]
    d_in = PF.dev(np.concatenate(models_pack))
    want_flags = [(DK_FLAG_HAS_FF if (b == 0xFF).any() else 0) | (DK_FLAG_SINGLE_SYMBOL if len(np.unique(b)) == 1 else 0) for b in models_pack]
    for model in PF.MODELS:
        streams, flags = ctx.dev_packed_encode(model, d_in, sizes, host_threads=4)
        assert flags == want_flags, (model, flags, want_flags)
        for i, b in enumerate(models_pack):
            assert bytes(streams[i]) == oracle_stream(model, b), "%s stream of block %d (%d bytes)" % (model, i, len(b))
    done_with(ctx)


# ---- LCP arrays, single and packed -----------------------------------------------------------------------------------------------------------
def group_lcp():
    from lcp_model import lcp_kasai
    from test_gpu_lcp import PACK_SIZES, WAVE_CAP, Words, dev_text, gpu_lcp, gpu_sa, planted, run_pack, the_pack

    def check(ctx, t, what):
        t = u8(t)
        sa, lcp, routes = gpu_lcp(ctx, t)
        REPORT["routes"] |= set(routes)
        assert np.array_equal(sa, oracle_sa(t)), what + ": the suffix array"
        want = lcp_kasai(t, sa)
        bad = np.flatnonzero(lcp != want)
        assert bad.size == 0, "%s: LCP[%d] = %d, model %d (%d wrong)" % (what, bad[0], lcp[bad[0]], want[bad[0]], bad.size)
        return routes

    ctx = open_ctx(sum(PACK_SIZES))  # (the lists are carved from what is left: the fill grows with the capacity)
    say("a^4097")
    assert "lcp_long" in check(ctx, np.full(4097, 97, np.uint8), "a^4097")
    say("planted, one byte over the wave cap")
    assert {"lcp_long", "lcp_giant"} <= check(ctx, planted(WAVE_CAP + 1, seed=WAVE_CAP + 1), "planted")
    say("markov")
    check(ctx, u8(datagen.wiki_like(20011, seed=5)), "markov")
    blocks = the_pack()
    for one_call in (False, True):
        say("the pack, one call: %s" % one_call)
        sas, lcps, routes = run_pack(ctx, blocks, one_call)
        REPORT["routes"] |= set(routes)
        assert {"packed_guard", "lcp_long", "lcp_giant"} <= routes, routes
        for i, b in enumerate(blocks):
            assert np.array_equal(sas[i], oracle_sa(b)), "pack, suffix array of block %d" % i
            assert np.array_equal(lcps[i], lcp_kasai(b, sas[i])), "pack, LCP array of block %d" % i
    say("a suffix array with an entry outside its block")
    t = u8(datagen.wiki_like(10000, seed=21))
    sa = gpu_sa(ctx, t)
    bad = sa.host()
    bad[5000] = len(t) + 7
    sa.t.copy_(torch.from_numpy(bad.view(np.int32)))
    out = Words(len(t))
    try:
        ctx.dev_lcp(dev_text(t), len(t), sa.t, out.t)
        raise AssertionError("an entry of n + 7 went through")
    except dark_amd.DarkError as e:
        assert e.code == DK_E_ARG and out.untouched(), e
    sizes = [4000, 6000]
    psa = Words(len(t))
    ctx.dev_suffix_array_packed(dev_text(t), sizes, psa.t)
    bad = psa.host()
    bad[100] = 4000  # in range for the whole text, not for its block
    psa.t.copy_(torch.from_numpy(bad.view(np.int32)))
    try:
        ctx.dev_lcp_packed(dev_text(t), sizes, psa.t, out.t)
        raise AssertionError("an entry outside its block went through")
    except dark_amd.DarkError as e:
        assert e.code == DK_E_ARG and out.untouched(), e
    check(ctx, t, "after the refusals")
    done_with(ctx)


# ---- suffix-array check and search -------------------------------------------------------------------------------------------------------------
def group_sa():
    import test_gpu_sa_check as SC
    import test_gpu_sa_search as SS
    from sa_query_model import OK, check_model
    from test_gpu_lcp import Words, dev_text

    t_halves, _ = SS.halves_case()
    ctx = open_ctx(len(t_halves))  # 140 000: halves_case() is the largest input here
    for name in sorted(SC.VALID):
        say("valid " + name)
        t = u8(SC.VALID[name]())
        sa = SC.gpu_sa(ctx, t)
        assert ctx.dev_sa_check(dev_text(t), len(t), sa.t) == (OK, len(t)), name
        assert sa.guards_intact() and np.array_equal(sa.host(), oracle_sa(t)) and check_model(t, sa.host()) == (OK, len(t)), name
    say("damaged")
    t = np.concatenate([np.maximum(SC.markov(20010, 6), 1), [0]]).astype(np.uint8)  # (the `base` of tests/test_gpu_sa_check.py)
    sa = oracle_sa(t)
    for kind in sorted(SC.DAMAGE):
        v = SC.damage(t, sa, kind)
        want = check_model(t, v)
        assert want[0] == SC.DAMAGE[kind], (kind, want)
        assert SC.gpu_check(ctx, t, v) == want, kind
    say("the pack")
    rng = np.random.default_rng(13)
    blocks = [rng.integers(97, 101, size=n, dtype=np.uint8) for n in SC.PACK_SIZES]
    blocks[4] = SC.markov(65537, 9)
    sizes = [len(b) for b in blocks]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pack = dict(blocks=blocks, sizes=sizes, off=off, d_in=dev_text(np.concatenate(blocks)), sa=np.concatenate([oracle_sa(b) for b in blocks]))
    d_sa = Words(int(off[-1]))
    ctx.dev_suffix_array_packed(pack["d_in"], sizes, d_sa.t)
    assert d_sa.guards_intact() and np.array_equal(d_sa.host(), pack["sa"]), "the pack's suffix arrays"
    SC.test_pack_valid(ctx, pack)
    SC.test_pack_entry_below_the_pack_but_outside_its_block(ctx, pack)
    for block in (1, 4, 7):
        SC.test_pack_damage_stays_in_its_block(ctx, pack, block)
    say("search: both sides of LANE_MAX, absent patterns")
    t = u8(datagen.wiki_like(70000, seed=3))
    markov_sa = (t, SS.gpu_sa(ctx, t))
    assert np.array_equal(markov_sa[1].host(), oracle_sa(t))
    for m in (SS.LANE_MAX - 1, SS.LANE_MAX, SS.LANE_MAX + 1, 1025):
        SS.test_pattern_lengths_around_the_steps(ctx, markov_sa, m)  # every pattern as it occurs and with its last byte changed
    absent = [b"\x00", b"\xff\xff", b"zzzzqqqq", bytes(t[:300]) + b"\x00", bytes(t[-5:]) + b"\x01" * SS.LANE_MAX, bytes(t) + b"a"]
    got = SS.check(ctx, t, absent + [b""], sa=markov_sa[1])  # (against search_model, as every call of check)
    assert got[-1] == (0, len(t)) and got[-2][0] == got[-2][1] and got[-3][0] == got[-3][1], got
    say("search: halves_case")
    SS.test_two_identical_halves_with_a_long_pattern(ctx)
    say("search: the pack")
    SS.test_pack(ctx)
    done_with(ctx)


# ---- the FM-index: build and count, locate, extract, snippets; full and decoder contexts ----------------------------------------------------------
def group_fm():
    import test_gpu_fm as F
    import test_gpu_fm_extract as FX
    import test_gpu_fm_locate as FL
    from dark_amd import fm
    from fm_model import fm_model, fm_model_packed
    from sa_query_model import search_model

    rng = np.random.default_rng(23)
    texts = [rng.integers(97, 101, size=n, dtype=np.uint8) for n in (1, 1023, 1024, 1025)] + [u8(datagen.wiki_like(5000, seed=3))]  # 5000: six rows
    same = rng.integers(97, 100, size=2100, dtype=np.uint8)
    pack = [same, same.copy(), u8(b"a"), np.full(2500, 97, np.uint8), u8(b"ab"), u8(b"\x00"), texts[-1][:3000].copy()]
    psizes = [len(b) for b in pack]

    def run(ctx, full):
        for t in texts:
            n = len(t)
            say("%s context, n = %d" % (ctx.purpose, n))
            (L, origin), sa = oracle_bwt(t), oracle_sa(t)
            pats = F.cut_patterns(t, rng, 60, [1, 2, 3, 8, 40]) + [b"", t, np.concatenate([t, [97]]), b"\x00", bytes(t[-1:]) + bytes(t[:2])]
            d_bwt, idx = F.gpu_index(ctx, L, [n], [origin])
            got = F.gpu_count(ctx, d_bwt, [n], idx, pats)
            assert not F.first_difference(got, fm_model(L, origin, pats), pats), "count, n = %d" % n
            assert not F.first_difference(got, search_model(t, sa, pats), pats), "count against the suffix array, n = %d" % n
            for step in (8, 32):
                FL.check_block(ctx, L, origin, sa, step)
                FX.check_block(ctx, L, origin, t, step)
        say("%s context, the pack" % ctx.purpose)
        pairs = [oracle_bwt(b) for b in pack]
        Ls, origins = [p[0] for p in pairs], [int(p[1]) for p in pairs]
        d_bwt, idx = F.gpu_index(ctx, np.concatenate(Ls), psizes, origins)
        pats, where = [], []
        for b, t in enumerate(pack):
            for p in (same[:12], same[:1], t, np.concatenate([t, [97]]), b"", b"a", b"\x00", b"a" * 1025):
                pats.append(u8(p))
                where.append(b)
        got = F.gpu_count(ctx, d_bwt, psizes, idx, pats, where)
        assert not F.first_difference(got, fm_model_packed(Ls, origins, pats, where), pats), "count in the pack"
        for step in (8, 32):
            loc = FL.gpu_structure(ctx, d_bwt, psizes, origins, step, packed=True)
            for b, rows in enumerate(FL.whole_sa(ctx, d_bwt, psizes, idx, loc, step)):
                assert np.array_equal(rows, oracle_sa(pack[b])), "locate: block %d of the pack, step %d" % (b, step)
            ext = FX.gpu_anchors(ctx, d_bwt, psizes, origins, step, packed=True)
            for b, rows in enumerate(FX.whole_text(ctx, d_bwt, psizes, idx, ext, step)):
                assert np.array_equal(rows, pack[b]), "extract: block %d of the pack, step %d" % (b, step)
            if full:  # L, origins and suffix arrays from the packed sort of the same context, every block also alone
                FL.run_pack(ctx, pack, step)
                FX.run_pack(ctx, pack, step)
        say("%s context, snippets" % ctx.purpose)
        t = texts[-1]
        L, origin = oracle_bwt(t)
        index = fm.Index.from_bwt(ctx, L, origin, locate_step=32, extract_step=8)
        pats = [bytes(p) for p in F.cut_patterns(t, rng, 40, [2, 3, 5, 9])] + [bytes(t[:4]), bytes(t[-4:]), bytes(t[-1:])]
        got = index.snippets(pats, 5, 7, max_hits=4)
        tb = bytes(t)
        for q, p in enumerate(pats):
            places = FX.find_all(tb, p)
            assert len(got[q]) == min(len(places), 4) and len({at for at, _ in got[q]}) == len(got[q]), (q, p)
            for at, snippet in got[q]:
                assert at in places and snippet == tb[max(at - 5, 0):at + len(p) + 7], (q, p, at)
        assert index.text() == tb

    total = max(sum(psizes), max(len(t) for t in texts))
    ctx = open_ctx(total)
    run(ctx, True)
    done_with(ctx)
    dec = open_ctx(total, "decoder", len(pack))
    run(dec, False)
    done_with(dec)


# ---- one regrouping of the suffix sort: rerank() and classify_and_read() ---------------------------------------------------------------------------
def group_rerank():
    import test_gpu_rerank_layer as R
    # 13 tiles and five slots with heads around every tile border, 40 tiles of sparse, dense and surviving-free tiles, a heavy-tailed mixture:
    # the flags are read for whole tiles (the last one's rest and k_rerank_apply_first's look at tiles it then skips) and the tile aggregates
    # are scanned in place; classify_and_read clears above_pl_slots itself, which only groups above PL_MAX add to.  Every form, the sort's own
    # shapes and stretches of 2, 3 and 64 tiles.
    ctx = open_ctx(41 * R.TILE)
    rng = np.random.default_rng(31)
    count = 13 * R.TILE + 5
    plan = [0, "pair", 0, 64, 65, R.TILE, 0, 0, 0, 2, 0, 0, R.TILE, 0, 5, 0] * 2 + [0] * 8
    lists = [("borders", R.sizes_from_heads(count, R.border_heads(rng, count)), R.FORMS), ("tile plan", R.tile_plan_sizes(plan), ("first", "narrow")),
             ("heavy tail", R.heavy_sizes(rng, 7 * R.TILE - 1), R.FORMS), ("nothing above PL_MAX", R.heavy_sizes(rng, 3 * R.TILE + 1, cap=R.M.PL_MAX), R.FORMS),
             ("all singletons", np.ones(2 * R.TILE + 9, np.int64), R.FORMS)]
    for name, sizes, forms in lists:
        for form in forms:
            say("%s, %s form" % (name, form))
            c = R.make_case(rng, sizes, form, zero="final", ls_max=R.M.PL_MAX)
            if name == "nothing above PL_MAX":
                assert R.expected(c)[0].above_pl_slots == 0
            R.check(ctx, c, name, overrides=R.OVERRIDES[1:4])
    done_with(ctx)


GROUPS = {"rerank": group_rerank, "dc": group_dc, "inverse": group_inverse, "packed": group_packed, "lcp": group_lcp, "sa": group_sa, "fm": group_fm}

if __name__ == "__main__":
    import time
    t0 = time.perf_counter()
    orc.lib()
    GROUPS[GROUP]()
    REPORT["seconds"] = round(time.perf_counter() - t0, 2)
    assert REPORT["contexts"] > 0 and REPORT["peeks"] >= 12 * REPORT["contexts"] and REPORT["fills"] > 0, REPORT
    REPORT["routes"] = sorted(REPORT["routes"])
    print("RESULT " + json.dumps(REPORT))
