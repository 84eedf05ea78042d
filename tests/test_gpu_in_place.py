"""The last stage of the suffix-array path by itself: k_to_inplace, the six pair-chain kernels, k_plateau_sort / _ranks and the compaction
(k_plateau_count / _scan / _compact) through dk_dbg_dev_in_place, which runs in_place_rounds on a list the test built, bit-exact against
tests/in_place_model.py (tests/test_in_place_model.py pins the model and what every case is named for on the CPU).

None of these kernels reads the text, so a state is built from the oracle's suffix array (tests/in_place_cases.py): groups at a depth h, ranks =
head positions, the groups in any list order the case wants -- a group of 256 across a tile edge, a chain at its walk limit, a list of 2049 slots.
The symbol in front is a free label, so nearly every misordering shows in L, where end-to-end parity hides those between equal symbols.

Every output array holds 0xC3 before a call, with a pad behind, and is compared WHOLE: idx, pos, rank, sa or bwt, the origin word, the counters.
meta and sym are compared at live slots only (a dead slot's word is whatever the ping-pong left).  Each exact case runs six ways -- the chains
only, one round, two rounds, to the end, to the end with a compaction behind every round read, two rounds with the compaction behind them as the
call's last step -- in both modes.  The cases whose record list is
full over several workgroups are checked for soundness only (which records fit depends on the order of the atomics) and are named sound_*."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

import dark_amd
import in_place_cases as K
from conftest import ROOT
from dark_amd._lib import DK_E_ARG
from test_gpu_fallbacks import _call, _env

pytestmark = pytest.mark.gpu
MODES = ("sa", "l")
CAP = 1 << 17


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", K.EXACT)
def test_exact(ctx, name, mode):
    c = K.CASES[name]()
    for plan_id, plan in zip(K.PLAN_IDS, K.PLANS):
        got = K.call(ctx, c, mode, **plan)
        K.check_exact(c, mode, got, K.expected(name, mode, plan_id))
        if "max_rounds" not in plan:
            K.check_complete(c, mode, got)  # (the undecided twin of a walk, the partial groups: finished by the rounds)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ("three_copies", "four_copies"))
def test_the_sorts_own_chain_group_is_four(ctx, name, mode):
    """a negative chain_group (what the cases above pass) and 4 are the same run"""
    c = K.CASES[name]()
    K.check_exact(c, mode, K.call(ctx, c, mode, chain_group=4, max_rounds=1), K.expected(name, mode, "one_round"))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", K.SOUND)
def test_sound_when_the_record_list_is_full(ctx, name, mode):
    c = K.CASES[name]()
    K.check_sound_chains(c, mode, K.call(ctx, c, mode, max_rounds=0))
    for plan in ({}, dict(always_compact=True)):
        got = K.call(ctx, c, mode, **plan)
        assert got["list_full"] == 1
        K.check_complete(c, mode, got)


@pytest.mark.parametrize("mode", MODES)
def test_the_sorts_own_compaction(ctx, mode):
    """95 000 slots, the chains settle the two halves (more than three quarters) and leave the five copies alive: in_place_compact as the sort calls
    it, its last tile ending inside the list"""
    c = K.CASES["own_compaction"]()
    for plan_id in ("two_rounds", "to_the_end"):
        got = K.call(ctx, c, mode, **K.PLANS[K.PLAN_IDS.index(plan_id)])
        assert got["compactions"] >= 1 and got["slots"] < c.count // 4 and got["slots"] % K.TILE != 0
        K.check_exact(c, mode, got, K.expected(c.name, mode, plan_id))
    K.check_complete(c, mode, got)


def test_the_spines_past_one_tile_per_thread():
    """two identical halves of 2 200 000 random bytes (a few bytes of the second changed, so that there is more than one chain): more than 2^21
    records and more than 2^21 slots, where the one-workgroup spines k_chain_spine and k_plateau_scan take more than one tile per thread.  The
    counters and the whole suffix array only; the one large case of this file (neither spine can go wrong below that size)"""
    half = K.rnd(60, 256, 2200000)
    second = half.copy()
    second[np.arange(1, 21) * 100003] ^= 0x5A
    c = K.build_state("large", K.cat(half, second), 6, 160)
    records = int((c.sizes * (c.sizes - 1) // 2).sum())
    assert records > 1 << 21 and c.count > 1 << 21 and c.sizes.max() <= 4
    with dark_amd.Context(c.n) as big:
        got = K.call(big, c, "sa")
    assert (got["records"], got["list_full"], got["settled"], got["live"], got["rounds"], got["compactions"]) == (records, 0, c.count, 0, 0, 0)
    assert np.array_equal(got["sa"], c.sa), K.first_diff(got["sa"], c.sa)
    assert np.array_equal(got["rank"][c.sa], np.arange(c.n, dtype=np.uint32))


def test_refusals_leave_every_array_untouched(ctx):
    lib, h = ctx._lib, ctx._h
    n, count, groups = 70000, 1000, 400
    filled = lambda words: torch.full((words,), -0x3C3C3C3D, dtype=torch.int32, device="cuda")  # noqa: E731  (0xC3C3C3C3)
    bufs = {name: filled(n) for name in ("idx", "pos", "gid", "gstart", "rank", "sa", "bwt", "sym", "origin", "out_idx", "out_meta", "out_sym", "out_pos")}
    out = np.full(8, K.FILL32, np.uint32)
    torch.cuda.synchronize()
    p = {k: C.c_void_p(v.data_ptr()) for k, v in bufs.items()}
    sa_mode, l_mode = dict(bwt=None, sym=None, origin=None, out_sym=None), dict(sa=None)

    def call(ctx_h=h, n=n, depth=6, count=count, groups=groups, chain_group=-1, record_cap=0, max_rounds=-1, always_compact=0, out_p=C.c_void_p(out.ctypes.data), **over):
        a = dict(p, **over)
        return lib.dk_dbg_dev_in_place(ctx_h, n, depth, count, a["idx"], a["pos"], a["gid"], a["gstart"], groups, a["rank"], a["sa"], a["bwt"], a["sym"], a["origin"],
                                       chain_group, record_cap, max_rounds, always_compact, a["out_idx"], a["out_meta"], a["out_sym"], a["out_pos"], out_p)

    refused = [("null context", dict(ctx_h=None, **sa_mode)), ("both modes", {}), ("neither mode", dict(sa_mode, sa=None)),
               ("half of the L mode: no d_sym", dict(l_mode, sym=None)), ("half of the L mode: no d_origin", dict(l_mode, origin=None)),
               ("half of the L mode: no d_out_sym", dict(l_mode, out_sym=None)), ("d_sa with d_sym", dict(sa_mode, sym=p["sym"]))]
    for mode in (sa_mode, l_mode):
        refused += [("n = 1", dict(mode, n=1, count=1, groups=1)), ("n above the capacity", dict(mode, n=CAP + 1)), ("no slots", dict(mode, count=0)),
                    ("more slots than suffixes", dict(mode, count=n + 1)), ("depth 0", dict(mode, depth=0)), ("chain_group 5", dict(mode, chain_group=5)),
                    ("no groups", dict(mode, groups=0)), ("more groups than slots", dict(mode, groups=count + 1)),
                    ("more groups than the table holds", dict(mode, count=n, groups=n // 2 + 2)), ("record_cap above n", dict(mode, record_cap=n + 1)),
                    ("no out", dict(mode, out_p=None))]
        refused += [("null " + name, dict(mode, **{name: None})) for name in ("idx", "pos", "gid", "gstart", "rank", "out_idx", "out_meta", "out_pos")]
    for name, over in refused:
        assert call(**over) == DK_E_ARG, name
    assert b"in_place" in lib.dk_last_error(h)
    with ctx.batch_begin("dark", host_threads=1):
        assert call(**sa_mode) == DK_E_ARG, "an open batch"
    assert b"batch" in lib.dk_last_error(h)
    with dark_amd.Context(n, purpose="decoder") as dec:
        assert call(ctx_h=dec._h, **sa_mode) == DK_E_ARG and b"decoder context" in lib.dk_last_error(dec._h)
    torch.cuda.synchronize()
    for name, t in bufs.items():
        assert bool((t == -0x3C3C3C3D).all()), "a refused call wrote to " + name
    assert (out == K.FILL32).all()
    c = K.CASES["two_halves"]()
    K.check_exact(c, "sa", K.call(ctx, c, "sa"), K.expected(c.name, "sa", "to_the_end"))  # ... and the context serves the next call


def test_a_context_of_exactly_n(ctx):
    """the sort's buffers for n fit a context whose capacity is n (DK_E_NOMEM has no way in from outside: n above the capacity is refused first)"""
    c = K.CASES["ends_two"]()
    with dark_amd.Context(c.n) as small:
        K.check_exact(c, "l", K.call(small, c, "l"), K.expected(c.name, "l", "to_the_end"))


def test_poisoned_workspace_and_stale_mailbox():
    """three of the cases once more in a process of its own on the tuning library with DK_POISON=165 (every workspace allocation filled with 0xA5
    first) and after dk_dbg_mail_fill(0xA5): the 256-member group with 128 members in front of slot 2048, the walk twin that is decided, one full
    list -- the same bytes as the plain run"""
    cmd = [sys.executable, os.path.join(ROOT, "tests", "in_place_worker.py"), ROOT, json.dumps(dict(cases=list(K.POISON), poison=165, mail_fill=0xA5))]
    p = _call(cmd, _env(dict(DK_POISON=165)), "DK_POISON=165")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout + p.stderr
    assert json.loads(line[-1][7:]) == {K.POISON[0]: 12, K.POISON[1]: 12, K.POISON[2]: 4}
