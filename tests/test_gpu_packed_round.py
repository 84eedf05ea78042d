"""The segmented suffix sort of csrc/packed.hip one step at a time, through dk_dbg_dev_packed_first (k_pk_hist, k_pk_codes, k_pk_init_keys, the
sort, the first regroup) and dk_dbg_dev_packed_round (k_pk_round_keys, the sort, k_pk_tile_sum / k_pk_spine / k_pk_tile_apply, k_pk_guard_mark) --
the same step functions packed_sort_device chains -- bit-exact against tests/packed_round_model.py (tests/test_packed_round_model.py pins the
model to the definition by prefixes, every case to what it is named for, and shows that every case can fail).

End-to-end parity is a weak instrument here: a block the rounds leave unresolved is redone alone by the guard, and two groups one round leaves
merged are split by the next -- a kernel that loses a head at a tile border or collides the two ranges of rank2 still gives the right L and SA.
A round on a state the test built has nothing behind it that heals.

Every device output holds 0xC3 before a call, with 64 guard entries in front and behind, and is compared WHOLE: the untouched tails of the
lists behind `live`, every rank of a suffix that is not listed, out and code."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

import dark_amd
import packed_round_cases as K
import packed_round_model as M
from conftest import ROOT
from dark_amd._lib import DK_E_ARG
from test_gpu_fallbacks import _call, _env
from test_gpu_packed_sa import want_sa

pytestmark = pytest.mark.gpu
CAP = 1 << 17


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(K.FIRST))
def test_first_keys(ctx, name):
    blocks = K.first_blocks(name)
    K.check_first(name, ctx.dbg_dev_packed_first(blocks, fill=0xC3, pad=K.PAD), M.first(blocks))


@pytest.mark.parametrize("name", sorted(K.ROUNDS))
def test_built_rounds(ctx, name):
    c = K.ROUNDS[name]()
    K.check_round(name, K.call_round(ctx, c), M.round_(c.act, c.rank, c.off, c.h), c.guard)


def test_two_spine_passes():
    """1025 tiles and one entry: k_pk_spine carries the last new head, the last old head and the live count from its first pass into its second;
    an old group and a new group lie across the border, tile 1024 holds no head, live entries on both sides"""
    c = K.large()
    t0 = time.time()
    m = M.round_(c.act, c.rank, c.off, c.h)
    t1 = time.time()
    with dark_amd.Context(len(c.rank)) as big:
        t2 = time.time()
        got = K.call_round(big, c)
        t3 = time.time()
    print("two_spine_passes: c = %d, model %.2f s, context %.2f s, call with copies %.2f s" % (len(c.act), t1 - t0, t2 - t1, t3 - t2))
    assert len(c.act) == K.LARGE_C and m.live > K.LARGE_C // 2
    K.check_round(c.name, got, m)


def test_chain_on_a_real_pack(orc):
    """first, then round until nothing is live, on the cut mixed pack: the state after every step is the model's, and the final ranks are the
    inverse of the oracle's suffix arrays -- what packed_sa_device emits from"""
    blocks = K.chain_blocks()
    f, rounds = M.chain(blocks)
    sizes = [len(b) for b in blocks]
    assert len(rounds) >= 8 and rounds[-1].live == 0
    with dark_amd.Context(int(f.off[-1])) as big:
        got = big.dbg_dev_packed_first(blocks, fill=0xC3, pad=K.PAD)
        K.check_first("chain", got, f)
        act, rank, h = got["act"][K.PAD:K.PAD + got["live"]], got["rank"][K.PAD:-K.PAD], f.k_used
        for i, m in enumerate(rounds):
            got = big.dbg_dev_packed_round(sizes, h, act, rank, fill=0xC3, pad=K.PAD)
            K.check_round("chain, round %d" % i, got, m)
            act, rank, h = got["next_act"][K.PAD:K.PAD + got["live"]], got["rank"][K.PAD:-K.PAD], 2 * h
    for b, o in zip(blocks, f.off[:-1]):
        sa = np.asarray(want_sa(orc, b), dtype=np.int64)
        assert (rank[o + sa] == o + np.arange(len(b))).all()


def test_refusals_leave_every_array_untouched(ctx):
    lib, h = ctx._lib, ctx._h
    n, c = 5000, 700
    filled = lambda nbytes: torch.full((nbytes,), 0xC3, dtype=torch.uint8, device="cuda")  # noqa: E731
    bufs = dict(keys=filled(8 * n), vals=filled(4 * n), rank=filled(4 * n), act=filled(4 * n), guard=filled(4 * 3))
    text = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    d_list = torch.arange(0, 2 * c, 2, dtype=torch.int32, device="cuda")
    d_rank_in = torch.zeros(n, dtype=torch.int32, device="cuda")
    code, out = np.full(256, 0xC3C3, np.uint16), np.full(8, K.FILL32, np.uint32)
    sizes = lambda *ns: (C.c_size_t * len(ns))(*ns)  # noqa: E731
    torch.cuda.synchronize()
    p = {k: C.c_void_p(v.data_ptr()) for k, v in bufs.items()}
    hp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def first(ctx_h=h, text_p=C.c_void_p(text.data_ptr()), count=3, ns=sizes(2000, 2500, 500), code_p=hp(code), out_p=hp(out), **over):
        a = dict(p, **over)
        return lib.dk_dbg_dev_packed_first(ctx_h, text_p, count, ns, a["keys"], a["vals"], a["rank"], a["act"], code_p, out_p)

    def round_(ctx_h=h, count=3, ns=sizes(2000, 2500, 500), hh=4, list_p=C.c_void_p(d_list.data_ptr()), cc=c, out_p=hp(out), **over):
        a = dict(p, **over)
        return lib.dk_dbg_dev_packed_round(ctx_h, count, ns, hh, list_p, cc, a["rank"], a["keys"], a["vals"], a["act"], a["guard"], out_p)

    layouts = [("no sizes", dict(ns=None)), ("count 0", dict(count=0)), ("65537 blocks", dict(count=65537, ns=sizes(*([1] * 65537)))),
               ("an empty block", dict(ns=sizes(2000, 0, 500))), ("a block above 2^24 bytes", dict(ns=sizes(2000, (1 << 24) + 1, 500))),
               ("a pack above the capacity", dict(ns=sizes(CAP - 10, 6, 5)))]
    refused = [("null context", dict(ctx_h=None)), ("null text", dict(text_p=None)), ("null keys", dict(keys=None)), ("null vals", dict(vals=None)),
               ("null rank", dict(rank=None)), ("null act", dict(act=None)), ("null code", dict(code_p=None)), ("null out", dict(out_p=None))] + layouts
    for name, over in refused:
        assert first(**over) == DK_E_ARG, name
    refused = [("null context", dict(ctx_h=None)), ("null list", dict(list_p=None)), ("null rank", dict(rank=None)), ("null keys", dict(keys=None)),
               ("null vals", dict(vals=None)), ("null next list", dict(act=None)), ("null out", dict(out_p=None)), ("c = 0", dict(cc=0)),
               ("c above the pack", dict(cc=n + 1)), ("h = 0", dict(hh=0)), ("h above 2^31", dict(hh=(1 << 31) + 1))] + layouts
    for name, over in refused:
        assert round_(**over) == DK_E_ARG, name
    assert round_(hh=0) == DK_E_ARG and b"packed_round" in lib.dk_last_error(h)
    assert first(act=None) == DK_E_ARG and b"packed_first" in lib.dk_last_error(h)
    with ctx.batch_begin("dark", host_threads=1):
        assert first() == DK_E_ARG and round_() == DK_E_ARG, "an open batch"
    assert b"batch" in lib.dk_last_error(h)
    with dark_amd.Context(n, purpose="decoder") as dec:
        assert first(ctx_h=dec._h) == DK_E_ARG and b"decoder context" in lib.dk_last_error(dec._h)
        assert round_(ctx_h=dec._h) == DK_E_ARG and b"decoder context" in lib.dk_last_error(dec._h)
    torch.cuda.synchronize()
    for name, t in bufs.items():
        assert bool((t == 0xC3).all()), "a refused call wrote to " + name
    assert (code == 0xC3C3).all() and (out == K.FILL32).all()
    bufs["rank"].view(torch.int32).copy_(d_rank_in)  # (valid ranks for the round: all zero, one old group)
    torch.cuda.synchronize()
    assert round_() == 0 and round_(hh=1 << 31) == 0 and round_(guard=None) == 0 and first() == 0  # the same arguments, served
    assert list(out) == [1, 1, 2, 62, n - 3 * 61, 64, 0, 0]  # (one symbol: the 61 shortest suffixes of every block are alone with their padding)
    for name in ("sigma_256", "count_65"):  # ... and the context serves the next calls
        blocks = K.first_blocks(name)
        K.check_first(name, ctx.dbg_dev_packed_first(blocks, fill=0xC3, pad=K.PAD), M.first(blocks))
    c2 = K.ROUNDS["singletons_and_pairs"]()
    K.check_round(c2.name, K.call_round(ctx, c2), M.round_(c2.act, c2.rank, c2.off, c2.h))


def test_a_context_of_exactly_total():
    """the sort's buffers fit a context whose capacity is the pack"""
    blocks = K.first_blocks("blocks_1_2_3_4095_4096_4097")
    c = K.ROUNDS["c_3_tiles_5_whole_pack"]()
    with dark_amd.Context(sum(len(b) for b in blocks)) as small:
        K.check_first("exactly total", small.dbg_dev_packed_first(blocks, fill=0xC3, pad=K.PAD), M.first(blocks))
    with dark_amd.Context(len(c.rank)) as small:
        K.check_round("exactly total", K.call_round(small, c), M.round_(c.act, c.rank, c.off, c.h))


WORKER_FIRST = ("sigma_256", "count_65", "block_shorter_than_the_key", "count_65536_of_one_byte")
WORKER_ROUNDS = ("pairs_across_every_border", "old_group_over_three_tiles", "collision_of_short_and_long", "guard_300_blocks", "c_17")


def test_poisoned_workspace_and_stale_mailbox():
    """a short list of the cases in a process of its own on the tuning library under DK_POISON=165 (proved to be in force: every workspace
    allocation filled with 0xA5 first) behind dk_dbg_mail_fill(0xA5): the model's answer every time"""
    knobs = dict(DK_POISON=165)
    spec = dict(first=list(WORKER_FIRST), rounds=list(WORKER_ROUNDS), poison=165, mail_fill=165)
    cmd = [sys.executable, os.path.join(ROOT, "tests", "packed_round_worker.py"), ROOT, json.dumps(spec)]
    p = _call(cmd, _env(knobs), "DK_POISON=165")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout + p.stderr
    res = json.loads(line[-1][7:])
    assert sorted(res) == sorted(WORKER_FIRST + WORKER_ROUNDS)
    assert res["count_65536_of_one_byte"] == 0 and res["collision_of_short_and_long"] == 0 and res["pairs_across_every_border"] > 2 * K.TILE
