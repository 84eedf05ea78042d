"""tests/rerank_model.py on the CPU: the vectorised model against the per-slot loop on small random lists of every form, and a prefix-doubling
suffix sort whose every regrouping is the model, against sorted(range(n), key=lambda i: t[i:]) -- the model means what the sort needs."""
import numpy as np

import rerank_model as M
from conftest import seeded_inputs

FILL = 0xC3C3C3C3


def random_case(rng):
    """a list of 1 .. 40 slots: few key values (long groups and singletons side by side), old groups that cut through equal keys, noise below
    cmp_shift, distinct suffixes and positions out of a range wider than the list"""
    n = int(rng.integers(1, 41))
    form = ["first", "first_shift", "narrow", "later", "later_gid"][int(rng.integers(0, 5))]
    kw = dict(ls_max=int(rng.integers(1, 5)))
    steps = rng.random(n) < rng.choice([0.1, 0.5, 0.9])
    field = np.cumsum(steps).astype(np.uint64) * np.uint64(rng.choice([1, 1 << 31, 1 << 33]))
    wide = n + int(rng.integers(0, 10))
    idx = rng.permutation(wide)[:n].astype(np.uint32)
    if form == "narrow":
        keys = (field & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        starts = np.sort(rng.integers(0, n + 1, size=256)).astype(np.uint32)
        starts[rng.random(256) < 0.9] = rng.choice([0, n])  # mostly empty buckets in front and behind, as a sort of few symbols leaves them
        kw["bucket_starts"] = np.sort(starts)
    elif form == "first_shift":
        kw["cmp_shift"] = 8
        keys = (field << np.uint64(8)) | rng.integers(0, 256, size=n, dtype=np.uint64)
    else:
        keys = field
    if form.startswith("later"):
        kw["pos_in"] = rng.permutation(wide)[:n].astype(np.uint32)
        if form == "later_gid":
            kw["gid_in"] = np.cumsum(rng.random(n) < 0.2).astype(np.uint32)
    with_bwt = rng.random() < 0.7
    if with_bwt:
        kw["bwt"] = rng.integers(0, 256, size=wide if form.startswith("later") else n, dtype=np.uint8)
        if form.startswith("later"):
            kw["sym_in"] = rng.integers(0, 256, size=n, dtype=np.uint8)
    return keys, idx, kw, wide


def test_model_against_the_per_slot_loop():
    forms, seen = set(), set()
    for case in range(4000):
        rng = np.random.default_rng(case)
        keys, idx, kw, wide = random_case(rng)
        m, r = M.rerank_model(keys, idx, **kw), M.rerank_loop(keys, idx, **kw)
        what = "case %d" % case
        for name in M.COUNT_NAMES:
            assert getattr(m, name) == r[name], (what, name)
        for name in ("out_idx", "out_pos", "out_gid", "gstart", "bigoff"):
            assert getattr(m, name).tolist() == r[name], (what, name)
        assert (m.sym_out is None and r["sym_out"] == []) or m.sym_out.tolist() == r["sym_out"], what
        assert dict(zip(m.big.tolist(), range(m.big_groups))) == r["bigidx"], what
        # the stores into the caller's arrays, through apply_model
        n = len(idx)
        before = dict(out_idx=np.full(n, FILL, np.uint32), out_pos=np.full(n, FILL, np.uint32), out_gid=np.full(n, FILL, np.uint32),
                      sym_out=np.full(n, 0xC3, np.uint8) if "bwt" in kw else None, gstart=np.full(n // 2 + 3, FILL, np.uint32),
                      bigidx=np.full(n // 2 + 2, FILL, np.uint32), bigoff=np.full(n // 2 + 2, FILL, np.uint32),
                      rank=np.full(wide, FILL, np.uint32), sa=np.full(wide, FILL, np.uint32), bwt=kw.get("bwt"), origin=FILL)
        after = M.apply_model(m, idx, before)
        want = {k: (None if v is None else v.copy() if isinstance(v, np.ndarray) else v) for k, v in before.items()}
        for name in ("out_idx", "out_pos", "out_gid", "sym_out", "gstart", "bigoff"):
            if want[name] is not None:
                want[name][:len(r[name])] = r[name]
        for g, j in r["bigidx"].items():
            want["bigidx"][g] = j
        for name in ("rank", "sa", "bwt"):
            for at, v in r[name].items():
                want[name][at] = v
        if r["origin"] is not None:
            want["origin"] = r["origin"]
        for name in want:
            assert np.array_equal(after[name], want[name]), (what, name)
        form = ("first" if m.first else "later") + ("+gid" if "gid_in" in kw else "") + ("+narrow" if "bucket_starts" in kw else "") + \
               ("+shift" if kw.get("cmp_shift") else "")
        forms.add((form, "bwt" in kw, m.groups > 0))
        seen |= {"big"} if m.big_groups else set()
        seen |= {"origin"} if m.origin is not None else set()
        seen |= {"kept ranks"} if not m.first and len(m.ranked) < n else set()
    # every form with and without symbols, with and without a survivor; big groups, a written origin and groups that keep their ranks
    assert forms == {(f, b, g) for f in ("first", "first+shift", "first+narrow", "later", "later+gid") for b in (False, True) for g in (False, True)}, sorted(forms)
    assert seen == {"big", "origin", "kept ranks"}, seen


def test_the_sentences_one_by_one():
    """a list small enough to read: old groups {0,1,2} {3,4,5,6} {7}; equal keys across the first border, a split inside the second group"""
    keys = np.array([5, 5, 7, 7, 7, 9, 9, 9], np.uint64)
    gid = np.array([0, 0, 0, 1, 1, 1, 1, 2], np.uint32)
    idx = np.array([10, 11, 0, 13, 14, 15, 16, 17], np.uint32)
    pos = np.array([20, 21, 22, 23, 24, 25, 26, 27], np.uint32)
    sym = np.arange(65, 73, dtype=np.uint8)
    m = M.rerank_model(keys, idx, pos_in=pos, gid_in=gid, sym_in=sym, bwt=np.zeros(30, np.uint8), ls_max=1)
    assert m.head.tolist() == [True, False, True, True, False, True, False, True]
    assert m.old_head.tolist() == [True, False, False, True, False, False, False, True]
    assert (m.active, m.groups) == (6, 3) and m.gstart.tolist() == [0, 2, 4, 6]
    assert m.out_idx.tolist() == [10, 11, 13, 14, 15, 16] and m.out_gid.tolist() == [0, 0, 1, 1, 2, 2] and m.sym_out.tolist() == [65, 66, 68, 69, 70, 71]
    assert m.final.tolist() == [2, 7] and m.origin == 22
    assert m.ranked.tolist() == [2, 5, 6] and m.rank_val.tolist() == [22, 25, 25]  # behind the new heads only
    assert (m.big_groups, m.big_slots, m.above_pl_slots) == (3, 6, 0) and m.bigoff.tolist() == [0, 2, 4]
    # without old groups slot 0 is a new head like any other, and the keys alone decide
    m = M.rerank_model(keys, idx, pos_in=pos)
    assert m.head.tolist() == [True, False, True, False, False, True, False, False] and m.ranked.tolist() == list(range(8))
    # the first rerank: positions are slots, the symbols come from L, nothing is final-stored
    m = M.rerank_model(keys << np.uint64(8) | np.arange(8, dtype=np.uint64), idx, cmp_shift=8, bwt=sym)
    assert m.out_pos.tolist() == list(range(8)) and m.sym_out.tolist() == sym.tolist() and m.origin is None and len(m.ranked) == 0
    # narrow: a bucket start splits equal words; starts at 0, at count and twice the same change nothing more
    starts = np.array([0] * 100 + [4] * 2 + [8] * 154, np.uint32)
    m = M.rerank_model(np.array([7] * 8, np.uint32), idx, bucket_starts=starts)
    assert m.head.tolist() == [True, False, False, False, True, False, False, False] and m.gstart.tolist() == [0, 4, 8]


def suffix_sort_through_the_model(t):
    """prefix doubling: sort by the first symbol, regroup (first rerank), then per round sort every group by the rank h symbols on and regroup
    (later reranks with the old groups, the rank and the suffix array) until no group survives.  Only the sort inside the groups is not the
    model's."""
    n = len(t)
    order = np.argsort(t, kind="stable")
    sa = order.astype(np.uint32)
    m = M.rerank_model(t[order].astype(np.uint64), sa)
    rank = np.empty(n, np.uint32)
    rank[sa] = np.arange(n, dtype=np.uint32)                  # finals: their own place
    rank[m.out_idx] = m.out_pos[m.gstart[m.out_gid]]          # survivors: the place of their group's head
    idx, pos, gid = m.out_idx, m.out_pos, m.out_gid
    h, rounds = 1, 0
    while len(idx):
        nxt = idx.astype(np.int64) + h
        key2 = np.where(nxt < n, rank[np.minimum(nxt, n - 1)].astype(np.uint64) + np.uint64(1), np.uint64(0))  # a suffix that ends goes first
        o = np.lexsort((key2, gid))
        m = M.rerank_model(key2[o], idx[o], pos_in=pos, gid_in=gid)
        after = M.apply_model(m, idx[o], dict(out_idx=None, out_pos=None, out_gid=None, gstart=np.zeros(m.groups + 1, np.uint32),
                                              bigidx=np.zeros(m.groups, np.uint32), bigoff=np.zeros(m.groups, np.uint32), rank=rank, sa=sa))
        rank, sa = after["rank"], after["sa"]
        idx, pos, gid = m.out_idx, m.out_pos, m.out_gid
        h *= 2
        rounds += 1
        assert rounds <= 20
    return sa


def test_prefix_doubling_through_the_model():
    for i, t in enumerate(seeded_inputs()):
        b = t.tobytes()
        want = sorted(range(len(b)), key=lambda j: b[j:])
        assert suffix_sort_through_the_model(t).tolist() == want, "input %d (%d bytes)" % (i, len(t))
