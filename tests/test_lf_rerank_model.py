"""tests/lf_rerank_model.py, the judge of tests/test_gpu_lfirst_layer.py, pinned on the CPU: the numpy model against the per-slot loop written from
the same sentences, against `brute` of tests/test_lfirst_logic.py (the definition k_lf_reduce's flag logic was written from) on random tiles, and
on a few lists small enough to state their answer by hand."""
import random

import numpy as np
import pytest

import lf_rerank_model as M
from test_lfirst_logic import TILE, brute


def random_list(rng, count, form, p_head=0.2, nsym=3, zero="idx"):
    """-> keyword arguments of the model for a random list in one of the key forms"""
    head = rng.random(count) < p_head
    head[0] = True
    field = np.cumsum(head).astype(np.uint64)
    kw = dict(idx=(rng.permutation(count + 5)[:count] + 1).astype(np.uint32), sym=rng.integers(0, nsym, size=count, dtype=np.uint8))
    if form == "narrow":
        forced = head & (rng.random(count) < 0.3)
        forced[0] = False
        starts = np.flatnonzero(forced)[:250]  # heads that only a bucket start makes: the words on both sides are equal
        kw["keys"] = np.cumsum(head & ~np.isin(np.arange(count), starts)).astype(np.uint32)
        kw["bucket_starts"] = np.sort(np.concatenate([starts, np.full(256 - len(starts), count + 3)])).astype(np.uint32)
    elif form == "keys32":
        kw["keys"] = field.astype(np.uint32)
    elif form == "shift8":
        kw["keys"] = field << np.uint64(8) | rng.integers(0, 256, size=count, dtype=np.uint64)
        kw["cmp_shift"] = 8
    else:
        kw["keys"] = field
    if form == "from_key":
        kw["keys"] = field << np.uint64(8) | kw["sym"].astype(np.uint64)
        kw["cmp_shift"], kw["sym_from_key"] = 8, True
        kw["bigdepth"], kw["key_shift"], kw["depth_add"] = rng.integers(1, 1000, size=int(field.max()) // 4 + 2).astype(np.uint32), 10, 5
    else:
        kw["depth"] = 9
    if form in ("from_key", "later"):
        kw["pos_in"] = rng.permutation(count + 9)[:count].astype(np.uint32)
    if zero == "idx":
        kw["idx"][int(rng.integers(0, count))] = 0
    elif zero == "slot":
        kw["zero_slot"] = int(rng.integers(0, count + 2))
    return kw


FORMS = ("wide", "shift8", "narrow", "keys32", "from_key", "later")


@pytest.mark.parametrize("form", FORMS)
def test_model_matches_the_loop(form):
    rng = np.random.default_rng(FORMS.index(form))
    for turn in range(40):
        count = int(rng.integers(1, 300))
        kw = random_list(rng, count, form, p_head=[0.05, 0.3, 0.7, 1.0][turn % 4], nsym=[1, 2, 3][turn % 3], zero=["idx", "slot", None][turn % 3])
        m, r = M.lf_rerank_model(ls_max=4, **kw), M.lf_rerank_loop(ls_max=4, **kw)
        for name in ("out_idx", "out_pos", "out_gid", "out_sym", "gstart"):
            assert getattr(m, name).tolist() == r[name], (form, turn, name)
        assert m.gdepth.tolist() == r["gdepth"] and m.live.tolist() == r["live"], (form, turn)
        assert m.counts == (r["active"], r["groups"], r["big_slots"], r["big_groups"]), (form, turn)
        assert m.origin == r["origin"], (form, turn)
        if not m.first:
            assert dict(zip(m.final_pos.tolist(), m.final_sym.tolist())) == r["bwt"], (form, turn)
        assert (m.sym_after is not None) == (form == "from_key")
        if form == "from_key":
            assert np.array_equal(m.sym_after, kw["sym"])


def test_liveness_of_a_tile_agrees_with_the_definition_of_the_flag_logic():
    """one tile that is the whole list (its first slot a head, the list's end closing its last group): brute's LF_SURV flags are the model's live
    slots, its surviving heads the model's groups"""
    random.seed(3)
    rng = np.random.default_rng(3)
    for trial in range(60):
        cnt = TILE if trial % 3 == 0 else random.randint(1, TILE)
        kw = random_list(rng, cnt, "wide", p_head=random.choice([0.001, 0.01, 0.1, 0.5, 0.9]), nsym=random.choice([1, 2, 5]), zero=["idx", None][trial % 2])
        m = M.lf_rerank_model(**kw)
        head = m.head.tolist() + [True] * (TILE - cnt)
        nu = [bool(a and not head[a] and kw["sym"][a] != kw["sym"][a - 1]) or kw["idx"][a] == 0 for a in range(cnt)] + [False] * (TILE - cnt)
        flags, ns, nh = brute(head, nu, cnt, True, True)
        assert [bool(f & 2) for f in flags[:cnt]] == m.live.tolist(), trial
        assert (ns, nh) == (m.active, m.groups), trial


def test_by_hand():
    # groups: [0,1,2] two symbols | [3] a singleton | [4,5] one symbol | [6,7] one symbol, suffix 0 | [8] suffix-free singleton
    keys = np.array([1, 1, 1, 2, 3, 3, 4, 4, 5], np.uint64)
    idx = np.array([10, 11, 12, 13, 14, 15, 16, 0, 17], np.uint32)
    sym = np.frombuffer(b"aabcddeef", np.uint8)
    pos = np.arange(100, 109, dtype=np.uint32)
    m = M.lf_rerank_model(keys, idx, sym, pos_in=pos, depth=7)
    assert m.live.tolist() == [True] * 3 + [False] * 3 + [True] * 2 + [False]
    assert m.out_idx.tolist() == [10, 11, 12, 16, 0] and m.out_pos.tolist() == [100, 101, 102, 106, 107] and m.out_gid.tolist() == [0, 0, 0, 1, 1]
    assert bytes(m.out_sym) == b"aabee" and m.gstart.tolist() == [0, 3, 5] and m.gdepth.tolist() == [7, 7] and m.counts == (5, 2, 0, 0)
    assert m.final_pos.tolist() == [103, 104, 105, 108] and bytes(m.final_sym) == b"cddf" and m.origin is None
    # suffix 0 in a singleton is final: the origin is its position; as *zero_slot it is looked for by slot, not by idx
    m = M.lf_rerank_model(keys, np.array([10, 11, 12, 0, 14, 15, 16, 18, 17], np.uint32), sym, pos_in=pos)
    assert m.origin == 103 and m.live.tolist() == [True] * 3 + [False] * 6
    m = M.lf_rerank_model(keys, idx, sym, zero_slot=4)
    assert m.live.tolist() == [True] * 3 + [False] + [True] * 2 + [False] * 3 and m.out_pos.tolist() == [0, 1, 2, 4, 5] and m.origin is None
    # the first rerank writes nothing into L: apply_model leaves bwt and the origin as they were
    before = dict(out_idx=np.zeros(12, np.uint32), out_pos=np.zeros(12, np.uint32), out_gid=np.zeros(12, np.uint32), out_sym=np.zeros(12, np.uint8),
                  gstart=np.full(8, 99, np.uint32), gdepth=None, sym=sym.copy(), bwt=np.full(9, 0xC3, np.uint8), origin=5)
    after = M.apply_model(m, before)
    assert (after["bwt"] == 0xC3).all() and after["origin"] == 5 and after["gstart"].tolist() == [0, 3, 5, 99, 99, 99, 99, 99]
    # a big group: more than ls_max members
    m = M.lf_rerank_model(np.ones(300, np.uint64), np.arange(1, 301, dtype=np.uint32), np.arange(300, dtype=np.uint8))
    assert m.counts == (300, 1, 300, 1) and M.lf_rerank_model(np.ones(256, np.uint64), np.arange(1, 257), np.arange(256, dtype=np.uint8)).counts == (256, 1, 0, 0)
