"""The L-first kernels by themselves (csrc/lfirst.inc), bit-exact against plain models and over WHOLE arrays: every output holds 0xC3 bytes before a
call, with a pad behind, so what a call must not write is compared too.

First half: lf_rerank -- k_lf_reduce<u64 | u32>, k_lf_straddle, the scan (k_rerank_scan / _a / _c) and k_lf_apply -- through dk_dbg_dev_lf_rerank and
against tests/lf_rerank_model.py (tests/test_lf_rerank_model.py pins that on the CPU).  The lists are BUILT from group sizes (make_case, on the
builders of tests/test_gpu_rerank_layer.py): which group has a reason to stay live, which reason, and in which slot it stands is the case's choice,
so that a group's reason lies in the first, a middle or the last of the tiles it crosses, or nowhere.  Every case runs with 0 (the sort's own), 1,
2, 3 and 64 tiles per workgroup of k_lf_reduce -- the multi-tile stretch, which the sort takes from 2^25 slots -- and all runs must give the
model's bytes, hence the same ones.  The three-phase scan has no override: its case has 4097 tiles and is the only large one.

Second half: the refinement -- k_lf_finish, the big rounds (the sorts, lf_rerank again, k_lf_medium), k_lf_deep_wave, k_lf_deep_block and k_lf_lce --
through dk_dbg_dev_lf_refine, which runs lfirst_path from a list the test built, and against tests/lf_refine_model.py (plain comparison of
suffixes; tests/test_lf_refine_model.py pins it).  The texts and lists are those of tests/lf_refine_cases.py.  Their point: the symbol in front
is a FREE LABEL -- no kernel of lfirst.inc derives it from the text (none reads text[i - 1]; checked by reading k_lf_finish, k_lf_medium, both
deep kernels and k_lf_apply: each carries the list's symbol along) -- so every member gets a random one and nearly every misordering inside a
group shows in L, where end-to-end parity hides all misorderings between members with equal symbols.  L holds 0xC3 before a call and is compared
whole; each case asserts the route bits and counters that prove it reached the kernel it is named for.  The settings of the tuning build's
knobs (DK_LF_WAVE=0, DK_LF_SHORT_SLOTS=0, the give-ups, DK_POISON) run in processes of their own (tests/lf_refine_worker.py), as in
tests/test_gpu_fallbacks.py."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

import dark_amd
import lf_refine_cases as K
import lf_refine_model as RM
import lf_rerank_model as M
from conftest import ROOT
from dark_amd._lib import DK_E_ARG
from test_gpu_fallbacks import _call, _env
from test_gpu_rerank_layer import first_diff, heavy_sizes, sizes_from_groups, sizes_from_heads

pytestmark = pytest.mark.gpu
TILE = M.TILE
BIG_TILES = 4 * M.SCAN_CHUNK + 1
CAP = (BIG_TILES + 1) * TILE
PAD = 64
FILL8, FILL32 = 0xC3, 0xC3C3C3C3
ARRAYS = ("out_idx", "out_pos", "out_gid", "out_sym", "gstart", "gdepth", "sym", "bwt")
PER_WG = (0, 1, 2, 3, 64)
# (keys, later rerank?): 8-byte keys compared whole / above 8 bits of noise, 4-byte keys with bucket starts, 4-byte group ids (the take-over form),
# 8-byte keys that carry the symbol in their low byte (the big list's, with its depth rule), 8-byte keys in a later rerank
FORMS = (("wide0", False), ("wide8", False), ("narrow", False), ("keys32", True), ("from_key", True), ("wide0", True), ("keys32", False))


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


# ---- building a list from its groups ------------------------------------------------------------------------------------------------------------
def make_case(rng, sizes, form=("wide0", False), diff=(), zero_at=None, zero_by="idx", forced_groups=()):
    """-> a case for lf_rerank_model / Context.dbg_dev_lf_rerank: groups of these sizes, every member of a group with the group's symbol in front
    except the slots `diff` (another symbol: a reason in that slot -- or, for a group's head, in the slot behind it, where the kernel compares).
    zero_at: the slot of suffix 0, told by idx ("idx") or by the word *zero_slot ("slot").  forced_groups (narrow keys): groups whose head is a
    bucket start between equal words."""
    keys_form, later = form
    sizes = np.asarray(sizes, dtype=np.int64)
    count, ng = int(sizes.sum()), len(sizes)
    starts = np.cumsum(sizes) - sizes
    forced = np.zeros(ng, bool)
    forced[list(forced_groups)] = True
    assert keys_form == "narrow" or not forced.any()
    field = np.repeat(np.cumsum(~forced) + 2, sizes).astype(np.uint64)
    sym = np.repeat(((np.arange(ng) * 37 + 11) & 0xFF).astype(np.uint8), sizes)
    d = np.asarray(diff, dtype=np.int64)
    sym[d] ^= 0x55
    kw = dict(depth=11)
    if keys_form == "narrow":
        kw["keys"] = field.astype(np.uint32)
        f = starts[forced]
        assert len(f) <= 250
        rest = 256 - len(f)  # empty buckets: in front, behind, and the same start twice
        filler = np.concatenate([np.zeros(rest // 3, np.int64), np.full(rest // 3, count), np.resize(f if len(f) else [count + 9], rest - 2 * (rest // 3))])
        kw["bucket_starts"] = np.sort(np.concatenate([f, filler])).astype(np.uint32)
    elif keys_form == "keys32":
        kw["keys"] = (field + np.uint64(0x30000000)).astype(np.uint32)
    elif keys_form == "wide8":  # below the shift: noise that must not split anything
        kw["keys"], kw["cmp_shift"] = field << np.uint64(40) | rng.integers(0, 256, size=count, dtype=np.uint64), 8
    elif keys_form == "from_key":
        kw["keys"], kw["cmp_shift"], kw["sym_from_key"] = field << np.uint64(8) | sym.astype(np.uint64), 8, True
        kw["bigdepth"], kw["key_shift"], kw["depth_add"] = rng.integers(1, 1 << 20, size=(ng + 2) // 4 + 2).astype(np.uint32), 10, 5
        kw["depth"] = None
    else:
        kw["keys"] = field | np.uint64(0x5A5A << 40)
    kw["sym"] = None if keys_form == "from_key" else sym
    wide = count + 37
    idx = rng.permutation(wide)[:count].astype(np.uint32)
    idx[idx == 0] = wide
    if zero_at is not None and zero_by == "idx":
        idx[zero_at] = 0
    elif zero_at is not None:
        kw["zero_slot"] = int(zero_at)
    kw["idx"] = idx
    kw["pos_in"] = rng.permutation(wide)[:count].astype(np.uint32) if later else None
    return dict(form=form, count=count, kw=kw, bwt=np.full(wide, FILL8, np.uint8), origin=FILL32)


def expected(c):
    """the model's verdict on a case, once: (model, the arrays after the call)"""
    if "want" not in c:
        kw, n = c["kw"], c["count"]
        m = M.lf_rerank_model(**kw)
        lists = {name: np.full(n + PAD, FILL32, np.uint32) for name in ("out_idx", "out_pos", "out_gid")}
        before = dict(lists, out_sym=np.full(n + PAD, FILL8, np.uint8), gstart=np.full(n // 2 + 1 + PAD, FILL32, np.uint32),
                      gdepth=np.full(n // 2 + PAD, FILL32, np.uint32), sym=np.full(n, FILL8, np.uint8) if kw["sym"] is None else kw["sym"],
                      bwt=c["bwt"], origin=c["origin"])
        c["want"] = (m, M.apply_model(m, before))
    return c["want"]


def run(ctx, c, per_wg=0, shift=None):
    return ctx.dbg_dev_lf_rerank(bwt=c["bwt"], origin=c["origin"], reduce_tiles_per_wg=per_wg, shift=shift, fill=FILL8, pad=PAD, **c["kw"])


def judge(label, got, c):
    m, want = expected(c)
    assert got["counts"] == m.counts, "%s: counts %s, model %s (%s)" % (label, got["counts"], m.counts, ", ".join(M.COUNT_NAMES))
    for name in ARRAYS:
        d = first_diff(name, got[name], want[name])
        assert d is None, "%s: %s" % (label, d)
    assert got["origin"] == want["origin"], "%s: origin %r, model %r" % (label, got["origin"], want["origin"])


def check(ctx, c, label, per_wgs=PER_WG, shift=None):
    label = "%s, %s keys%s, %d slots" % (label, c["form"][0], ", later rerank" if c["form"][1] else "", c["count"])
    for per_wg in per_wgs:
        judge("%s, %d tiles per workgroup" % (label, per_wg), run(ctx, c, per_wg, shift), c)


def check_forms(ctx, seed, sizes, label, forms=FORMS, counts=None, groups=None, **kw):
    """the case in every form, each with its own suffixes and positions; counts / groups: what the model must say of it in every form -> the cases"""
    cases = [make_case(np.random.default_rng(seed * 16 + i), sizes, form, **kw) for i, form in enumerate(forms)]
    for c in cases:
        m = expected(c)[0]
        assert counts is None or m.counts == counts, (label, c["form"], m.counts)
        assert groups is None or m.groups == groups, (label, c["form"], m.groups)
        check(ctx, c, label)
    return cases


def group_at(count, start, size, fill=3):
    """sizes of a list of `count` slots: ONE group at [start, start + size) among groups of `fill` members (singletons where they do not fit)"""
    groups = [(a, min(fill, start - a)) for a in range(0, start, fill)] + [(start, size)]
    groups += [(a, min(fill, count - a)) for a in range(start + size, count, fill)]
    sizes = sizes_from_groups(count, groups)
    assert int(sizes.sum()) == count
    return sizes


# ---- groups inside one tile ------------------------------------------------------------------------------------------------------------------------
def test_each_reason_alone(ctx):
    """[0, 5) two symbols | [5, 9) one symbol and suffix 0 | [9, 12) one symbol: final | [12] a singleton | [13, 15) two symbols at its head"""
    sizes = [5, 4, 3, 1, 2] + [1] * 20
    for zero_by in ("idx", "slot"):
        for c in check_forms(ctx, 1, sizes, "reasons alone, suffix 0 by %s" % zero_by, counts=(11, 3, 0, 0), diff=[3, 13], zero_at=7, zero_by=zero_by):
            assert expected(c)[0].gstart.tolist() == [0, 5, 9, 11]
        # suffix 0 in a singleton is final (a later rerank then writes the origin); in a group of one symbol it is the only reason
        for c in check_forms(ctx, 2, sizes, "suffix 0 in a singleton, by %s" % zero_by, counts=(5, 1, 0, 0), diff=[3], zero_at=12, zero_by=zero_by):
            assert (expected(c)[1]["origin"] != FILL32) == (c["form"][1] and zero_by == "idx")
    check_forms(ctx, 3, sizes, "no suffix 0 at all", counts=(7, 2, 0, 0), diff=[3, 13])


def test_no_live_group_and_one_group(ctx):
    for count in (1, 2, 9, TILE, TILE + 1, 3 * TILE + 5):
        check_forms(ctx, count, np.ones(count, np.int64), "all singletons", counts=(0, 0, 0, 0), zero_at=count // 2)
        check_forms(ctx, count + 1, heavy_sizes(np.random.default_rng(count), count, cap=700), "groups of one symbol each", counts=(0, 0, 0, 0))
        if count > 1:
            check_forms(ctx, count + 2, [count], "one group, two symbols in its last slot", diff=[count - 1])
            check_forms(ctx, count + 3, [count], "one group, suffix 0 in its first slot", zero_at=0)
            check_forms(ctx, count + 4, [count], "one group of one symbol", counts=(0, 0, 0, 0))


# ---- groups across tile borders --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first stretch", "last stretch", "head on the tile's last slot", "nowhere"])
def test_one_border(ctx, where):
    """a group of 20 over the border between tiles 1 and 2, its reason on one side only; a group of 4 whose head is tile 1's last slot and differs
    from its members: the kernel sees that in the next tile's first slot"""
    count = 3 * TILE + 11
    start, size = (2 * TILE - 1, 4) if where.startswith("head") else (2 * TILE - 10, 20)
    slot = {"first stretch": start + 4, "last stretch": start + size - 3, "head on the tile's last slot": start, "nowhere": None}[where]
    sizes = group_at(count, start, size)
    for reason in ("symbols", "suffix 0"):
        if slot is None or (reason == "suffix 0" and where.startswith("head")):
            continue
        over = dict(diff=[slot]) if reason == "symbols" else dict(zero_at=slot)
        check_forms(ctx, 20, sizes, "reason (%s) in the %s" % (reason, where), counts=(size, 1, 0, 0), **over)
    if slot is None:
        check_forms(ctx, 21, sizes, "no reason", counts=(0, 0, 0, 0))


@pytest.mark.parametrize("tiles", [2, 3, 65, 66, 130])
def test_group_over_many_tiles(ctx, tiles):
    """three slots in tile 1, tiles - 2 whole tiles, three slots in the last: the 64-tile loop of k_lf_straddle finds the end in its first round
    (65), needs a second (66) and a third (130).  The reason stands in the first stretch, in the last, in a middle tile only, or nowhere"""
    start, size = 2 * TILE - 3, (tiles - 2) * TILE + 6
    count = start + size + TILE + 77
    sizes = group_at(count, start, size)
    forms = FORMS if tiles <= 3 else (FORMS[0], FORMS[2], FORMS[4], FORMS[3])
    spots = {"the first stretch": start + 1, "the last stretch": start + size - 1, "nowhere": None}
    if tiles > 2:
        spots["a middle tile"] = start + 3 + ((tiles - 2) // 2) * TILE + 1000
        spots["the last middle tile"] = start + 3 + (tiles - 2) * TILE - 1
    for name, slot in spots.items():
        over = {} if slot is None else dict(zero_at=slot) if name == "a middle tile" else dict(diff=[slot])
        counts = (0, 0, 0, 0) if slot is None else (size, 1, size, 1) if size > M.LS_MAX else (size, 1, 0, 0)
        check_forms(ctx, tiles, sizes, "a group over %d tiles, reason in %s" % (tiles, name), forms=forms, counts=counts, **over)
    # the same among live neighbours: small groups with two symbols each in front of it and behind
    diff = [a + 1 for a in range(0, start - 3, 3)] + [a + 1 for a in range(start + size, count - 3, 3)]
    check_forms(ctx, tiles + 1, sizes, "a group over %d tiles without a reason among live groups" % tiles, forms=forms[:2], diff=diff)
    check_forms(ctx, tiles + 2, sizes, "a group over %d tiles among live groups" % tiles, forms=forms[:2], diff=diff + [start + size - 2])


@pytest.mark.parametrize("rest", [0, 1, 5, 2047])
def test_group_that_ends_with_the_list(ctx, rest):
    """from tile 0's last three slots to the list's end, 2 or 67 tiles on: no head behind it (end_tile == ntiles)"""
    for whole in (2, 67):
        count = (whole + 1) * TILE + rest
        start = TILE - 3
        sizes = group_at(count, start, count - start)
        for name, slot in (("first stretch", start + 2), ("last slot", count - 1), ("a middle tile", 2 * TILE + 9), ("nowhere", None)):
            over = {} if slot is None else dict(zero_at=slot) if name == "last slot" else dict(diff=[slot])
            forms = FORMS if whole == 2 else FORMS[:1] + FORMS[3:5]
            check_forms(ctx, 40 + rest, sizes, "a group to the list's end, reason in %s" % name, forms=forms, groups=0 if slot is None else 1, **over)


def test_two_straddling_groups_meet_in_one_tile(ctx):
    """A from tile 0 into tile 2 (its first five slots), B from there into tile 3: tile 2's live_first is A's wave's word and its live_last B's"""
    count = 4 * TILE + 100
    a0, b0, b1 = TILE - 7, 2 * TILE + 5, 3 * TILE + 9
    sizes = sizes_from_groups(count, [(a0, b0 - a0), (b0, b1 - b0)])
    for name, diff, want in (("A live", [a0 + 3], 1), ("B live", [b1 - 1], 1), ("both", [b0 - 1, b0 + 1], 2), ("neither", [], 0),
                             ("A by its tail in tile 2, B by its head's slot", [b0 - 2, b0], 2)):
        check_forms(ctx, 50, sizes, "two straddling groups, %s" % name, groups=want, diff=diff)
    # ... and every tile border a group's border, a group's middle, or next to one
    rng = np.random.default_rng(51)
    heads = [np.flatnonzero(rng.random(9 * TILE + 3) < 0.002)]
    for i, b in enumerate(range(TILE, 9 * TILE, TILE)):
        heads.append([[b - 1], [b], [b - 1, b], [b + 1], [], [b - 2, b - 1, b, b + 1], [b - 1, b + 1], []][i])
    sizes = sizes_from_heads(9 * TILE + 3, np.concatenate([np.asarray(h, np.int64) for h in heads]))
    check_forms(ctx, 52, sizes, "heads around every tile border", diff=np.flatnonzero(rng.random(9 * TILE + 3) < 0.001), zero_at=5 * TILE)


# ---- sizes, forms and views ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 7, 8, 9, 2047, 2048, 2049, 3 * TILE, 3 * TILE + 1, 3 * TILE + 13, 4 * TILE - 1, 65 * TILE + 3])
def test_counts_and_random_groups(ctx, count):
    """a partial last tile at count % 8 != 0 and count % 2048 in {0, 1, 2047}; heavy-tailed group sizes, a reason in every 200th slot"""
    rng = np.random.default_rng(count)
    for a, p in ((1.5, 0.005), (3.0, 0.2)):
        sizes = heavy_sizes(rng, count, a=a, cap=5000)
        forced = rng.integers(1, len(sizes), size=min(100, len(sizes) // 2)) if len(sizes) > 2 else ()
        diff = np.flatnonzero(rng.random(count) < p)
        for i, form in enumerate(FORMS):
            c = make_case(np.random.default_rng(count + i), sizes, form, diff=diff, zero_at=int(rng.integers(0, count)), zero_by=("idx", "slot")[i % 2],
                          forced_groups=forced if form[0] == "narrow" else ())
            check(ctx, c, "random groups (Zipf %.1f)" % a)


def test_key_forms(ctx):
    """keys that differ only below cmp_shift are ONE group; the same keys compared whole split; bucket starts alone make heads; with sym_from_key
    the symbol array holds the keys' low bytes afterwards and the depths follow the big-list rule"""
    rng = np.random.default_rng(60)
    count = 2 * TILE + 77
    c = make_case(rng, [count], ("wide8", False), diff=[count - 5])
    assert len(np.unique(c["kw"]["keys"])) > 200 and expected(c)[0].counts == (count, 1, count, 1)
    check(ctx, c, "keys that differ below cmp_shift only")
    c = make_case(rng, [count], ("wide8", False), diff=[count - 5])
    c["kw"]["cmp_shift"] = 0
    assert expected(c)[0].head.sum() > count // 2
    check(ctx, c, "the same keys with cmp_shift 0")
    sizes = sizes_from_heads(count, [TILE - 1, TILE, TILE + 1, 2 * TILE, count - 1, 40, 41, 50])
    c = make_case(rng, sizes, ("narrow", False), diff=[3, 45, TILE + 7, 2 * TILE + 1], forced_groups=range(1, len(sizes)))
    assert len(np.unique(c["kw"]["keys"])) == 1 and expected(c)[0].head.sum() == len(sizes)
    check(ctx, c, "bucket starts alone")
    c = make_case(rng, heavy_sizes(rng, count, cap=900), ("from_key", True), diff=np.flatnonzero(rng.random(count) < 0.01))
    m, want = expected(c)
    assert (want["sym"] == (c["kw"]["keys"] & np.uint64(0xFF))).all() and len(set(m.gdepth.tolist())) > 3
    check(ctx, c, "symbols and depths from the keys")


@pytest.mark.parametrize("form", FORMS)
def test_unaligned_views(ctx, form):
    """idx, sym and pos_in an element behind their allocation, one at a time and together: the slot-by-slot branches of k_lf_reduce and k_lf_apply
    over whole arrays"""
    rng = np.random.default_rng(70)
    count = 5 * TILE + 3
    sizes = heavy_sizes(rng, count, cap=3000)
    c = make_case(rng, sizes, form, diff=np.flatnonzero(rng.random(count) < 0.01), zero_at=count // 3)
    for shift in (dict(idx=1), dict(sym=1), dict(pos_in=1), dict(keys=1), dict(idx=1, sym=1, pos_in=1), dict(idx=3, sym=7, pos_in=2, keys=1)):
        check(ctx, c, "views shifted by %s" % shift, per_wgs=(0, 3), shift=shift)


# ---- the three-phase scan --------------------------------------------------------------------------------------------------------------------------
def test_three_phase_scan(ctx):
    """4097 tiles (two chunks, the second of one tile): heavy-tailed groups, one across the chunk border, a fifth of them live"""
    count = BIG_TILES * TILE - 3
    rng = np.random.default_rng(80)
    edge = M.SCAN_CHUNK * TILE
    heads = np.flatnonzero(rng.random(count) < 0.3)
    heads = heads[(np.abs(heads - edge) > 40) & (np.abs(heads - 4 * edge) > 40)]
    sizes = sizes_from_heads(count, np.concatenate([heads, [edge - 1, 4 * edge - 30, 4 * edge + 30]]))
    c = make_case(rng, sizes, ("wide0", True), diff=np.flatnonzero(rng.random(count) < 0.1), zero_at=4 * edge + 2)
    assert expected(c)[0].groups > 100000
    check(ctx, c, "4097 tiles")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_lf_rerank_refusals_then_a_correct_call(ctx):
    lib, h = ctx._lib, ctx._h
    n = 5000
    filled = lambda words: torch.full((words,), -0x3C3C3C3D, dtype=torch.int32, device="cuda")  # noqa: E731  (0xC3C3C3C3)
    names = ("keys", "starts", "sym", "idx", "zero", "pos", "out_idx", "out_pos", "out_gid", "out_sym", "gstart", "bwt", "origin", "gdepth", "bigdepth")
    bufs = {name: filled(2 * n) for name in names}
    counts = np.full(4, FILL32, np.uint32)
    torch.cuda.synchronize()
    p = {k: C.c_void_p(v.data_ptr()) for k, v in bufs.items()}

    def call(ctx_h=h, key_bytes=8, count=n, cmp_shift=0, from_key=0, key_shift=0, per_wg=0, counts_p=C.c_void_p(counts.ctypes.data), **over):
        a = dict(p, starts=None, bigdepth=None)
        a.update(over)
        return lib.dk_dbg_dev_lf_rerank(ctx_h, a["keys"], key_bytes, a["starts"], cmp_shift, a["sym"], from_key, a["idx"], a["zero"], a["pos"], count,
                                        a["out_idx"], a["out_pos"], a["out_gid"], a["out_sym"], a["gstart"], a["bwt"], a["origin"], a["gdepth"], 7,
                                        a["bigdepth"], key_shift, 0, counts_p, per_wg)

    refused = [("null context", dict(ctx_h=None)), ("no slots", dict(count=0)), ("above the capacity", dict(count=CAP + 1)),
               ("above 2^31 - 2", dict(count=(1 << 31) - 1)), ("keys of 2 bytes", dict(key_bytes=2)), ("keys of 16 bytes", dict(key_bytes=16)),
               ("bucket starts with 8-byte keys", dict(starts=p["starts"])), ("cmp_shift with 4-byte keys", dict(key_bytes=4, cmp_shift=8)),
               ("cmp_shift 64", dict(cmp_shift=64)), ("cmp_shift -1", dict(cmp_shift=-1)), ("sym_from_key with 4-byte keys", dict(key_bytes=4, from_key=1)),
               ("a later rerank without d_bwt", dict(bwt=None)), ("a later rerank without d_origin", dict(origin=None)),
               ("the big-list rule with 4-byte keys", dict(key_bytes=4, bigdepth=p["bigdepth"])),
               ("the big-list rule without d_gdepth_out", dict(bigdepth=p["bigdepth"], gdepth=None)),
               ("key_shift 64", dict(bigdepth=p["bigdepth"], key_shift=64)), ("key_shift -1", dict(bigdepth=p["bigdepth"], key_shift=-1)),
               ("65 tiles per workgroup", dict(per_wg=65)), ("no counts", dict(counts_p=None))]
    refused += [("null " + name, {name: None}) for name in ("keys", "sym", "idx", "out_idx", "out_pos", "out_gid", "out_sym", "gstart")]
    for name, over in refused:
        assert call(**over) == DK_E_ARG, name
    assert b"lf_rerank" in lib.dk_last_error(h)
    with ctx.batch_begin("dark", host_threads=1):
        assert call() == DK_E_ARG, "an open batch"
    assert b"batch" in lib.dk_last_error(h)
    with dark_amd.Context(n, purpose="decoder") as dec:
        assert call(ctx_h=dec._h) == DK_E_ARG and b"decoder context" in lib.dk_last_error(dec._h)
    torch.cuda.synchronize()
    for name, t in bufs.items():
        assert bool((t == -0x3C3C3C3D).all()), "a refused call wrote to " + name
    assert (counts == FILL32).all()
    rng = np.random.default_rng(90)
    for form in FORMS:
        check(ctx, make_case(rng, heavy_sizes(rng, n, cap=400), form, diff=np.flatnonzero(rng.random(n) < 0.05), zero_at=77), "after refused calls")


# ==== second half: the refinement =====================================================================================================================
@pytest.fixture(scope="module")
def rctx():
    c = dark_amd.Context(1 << 19)
    yield c
    c.close()


def refine(rctx, c):
    got = rctx.dbg_dev_lf_refine(c.text, c.idx, c.pos, c.gid, c.sym, c.h0, c.period, fill=FILL8, origin=FILL32)
    L, origin = RM.lf_refine_model(c.text, c.idx, c.pos, c.gid, c.sym, np.full(len(c.text), FILL8, np.uint8), FILL32)
    return K.check_result(c, got, L, origin)


@pytest.mark.parametrize("labels", [256, 2])
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_refine(rctx, name, labels):
    """every case of tests/lf_refine_cases.py with 256 and with 2 symbols in front (2: stretches of a group stay uniform and are left unordered)"""
    c = K.CASES[name](labels=labels)
    facts = refine(rctx, c)
    if name in ("giant_pair", "giant_triple"):
        assert facts["giant_count"] == 0, facts  # (every giant extension was resolved: the last giant round left its list empty)


def test_tokens_and_text_agree(rctx):
    """the same list with period 1 (a token round) and with period 0 (text rounds, k_lf_medium, the deep list): both give the model's L"""
    a, b = K.CASES["run_tokens"](), K.CASES["run_text"]()
    assert np.array_equal(a.text, b.text) and np.array_equal(a.idx, b.idx) and np.array_equal(a.pos, b.pos) and np.array_equal(a.sym, b.sym)
    fa, fb = refine(rctx, a), refine(rctx, b)
    assert "period_round" in fa["routes"] and "period_round" not in fb["routes"] and fa["rounds"] == 1 and fb["rounds"] == 2


def worker(knobs, **spec):
    cmd = [sys.executable, os.path.join(ROOT, "tests", "lf_refine_worker.py"), ROOT, json.dumps(spec)]
    what = " ".join("%s=%s" % kv for kv in sorted(knobs.items()))
    p = _call(cmd, _env(knobs), what)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout + p.stderr
    return json.loads(line[-1][7:])


def test_wave_kernel_off():
    """DK_LF_WAVE=0: every case of the wave section through the workgroup kernels alone (and nothing is handed on: one entry less for the giant
    pair), with the model's L"""
    facts = worker(dict(DK_LF_WAVE=0), cases=list(K.WAVE_CASES) + ["block", "giant_triple"], by_wave=False)
    assert "lfirst_giant" in facts["giant_pair"]["routes"] and facts["giant_pair"]["deep_count"] == K.CASES["giant_pair"]().leavers[0]


def test_six_steps_of_k_lf_finish():
    """DK_LF_SHORT_SLOTS=0: the list gets LF_STEPS = 6 steps and LF_STUCK = 2 as they are; members that part at bytes 7, 8, 14, 15, 20 and 21 are
    settled by steps 2 and 3 of k_lf_finish, nothing goes the deep way"""
    facts = worker(dict(DK_LF_SHORT_SLOTS=0), cases=["finish", "finish_steps"], counters=dict(finish_steps=[0, 0]))
    assert "lfirst_deep" not in facts["finish_steps"]["routes"] and "lfirst_deep" not in facts["finish"]["routes"]


@pytest.mark.parametrize("knobs,gave_up,goes_on", [(dict(DK_LF_GIANT_ROUNDS=0), ["giant_pair"], ["finish", "wave"]),
                                                    (dict(DK_LF_GIANT_ROUNDS=1), ["giant_triple"], ["giant_pair"]),
                                                    (dict(DK_LF_GIANT_ROUNDS=2), [], ["giant_triple"]),
                                                    (dict(DK_LF_DEEP_CAP=0), ["wave", "block", "stall"], ["finish", "big_sizes"])])
def test_give_ups(knobs, gave_up, goes_on):
    """no giant round / no room on the deep list: START_OVER, and every byte of L outside the listed places is still 0xC3; the cases that need
    neither go on to the model's L.  One giant round is one too few for the triple of giant copies, two are enough"""
    facts = worker(knobs, cases=gave_up + goes_on, gave_up=gave_up)
    for name in gave_up:
        assert facts[name]["verdict"] == "start_over" and (facts[name]["fallback"] != 0 or knobs.get("DK_LF_GIANT_ROUNDS") == 0), facts[name]


def test_poisoned_workspace_and_stale_mailbox():
    """every case once more with DK_POISON=165 (every workspace allocation filled with 0xA5 first) and after dk_dbg_mail_fill(0xA5)"""
    facts = worker(dict(DK_POISON=165), cases=sorted(K.CASES), poison=165, mail_fill=0xA5)
    assert set(facts) == set(K.CASES)


def test_lf_refine_refusals_then_a_correct_call(rctx):
    lib, h = rctx._lib, rctx._h
    n = 70000
    filled = lambda words: torch.full((words,), -0x3C3C3C3D, dtype=torch.int32, device="cuda")  # noqa: E731  (0xC3C3C3C3)
    bufs = {name: filled(n) for name in ("text", "idx", "pos", "gid", "sym", "bwt", "origin")}
    out = np.full(8, FILL32, np.uint32)
    torch.cuda.synchronize()
    p = {k: C.c_void_p(v.data_ptr()) for k, v in bufs.items()}

    def call(ctx_h=h, n=n, count=1000, h0=4, period=0, out_p=C.c_void_p(out.ctypes.data), **over):
        a = dict(p)
        a.update(over)
        return lib.dk_dbg_dev_lf_refine(ctx_h, a["text"], n, a["idx"], a["pos"], a["gid"], a["sym"], count, h0, period, a["bwt"], a["origin"], out_p)

    refused = [("null context", dict(ctx_h=None)), ("a text of 63 bytes", dict(n=63, count=10)), ("above the capacity", dict(n=(1 << 19) + 1)),
               ("no slots", dict(count=0)), ("more slots than bytes", dict(count=n + 1)), ("depth 0", dict(h0=0)), ("a depth above n", dict(h0=n + 1)),
               ("period -1", dict(period=-1)), ("a period above h0", dict(period=5)), ("no out", dict(out_p=None))]
    refused += [("null " + name, {name: None}) for name in bufs]
    for name, over in refused:
        assert call(**over) == DK_E_ARG, name
    assert b"lf_refine" in lib.dk_last_error(h)
    with rctx.batch_begin("dark", host_threads=1):
        assert call() == DK_E_ARG, "an open batch"
    assert b"batch" in lib.dk_last_error(h)
    with dark_amd.Context(n, purpose="decoder") as dec:
        assert call(ctx_h=dec._h) == DK_E_ARG and b"decoder context" in lib.dk_last_error(dec._h)
    torch.cuda.synchronize()
    for name, t in bufs.items():
        assert bool((t == -0x3C3C3C3D).all()), "a refused call wrote to " + name
    assert (out == FILL32).all()
    refine(rctx, K.CASES["finish"]())
