"""One general round of the suffix sort by itself: k_round_local<false> / <true>, the big list through the global sort, k_big_back and the rerank
behind them, through dk_dbg_dev_round, which runs general_round() on a list the test built -- bit-exact against tests/round_model.py
(tests/test_round_model.py pins the model and what every case is named for on the CPU).

A state is built from the oracle's suffix array (tests/round_cases.py): groups at a depth h, ranks = head positions, the members of every group
shuffled, the groups in any list order the case wants -- a group of 1024 across a tile edge, three big groups, a list of 2049 slots.  The symbol in
front is a free label, so a misordering between suffixes with the same symbol in front shows in L, where end-to-end parity hides it.

Every output array holds 0xC3 before a call, with a pad behind, and is compared WHOLE: the sorted state (keys, suffixes, symbols), the next list
(idx, pos, gid, gstart, sym), rank, sa or bwt, the origin word, the eight counters.  Each case runs in the suffix-array mode, where the big list's
keys carry no symbol, and with L carried along, where they do.  One check needs no model: inside every old group the new groups stand in true
suffix order."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

import dark_amd
import round_cases as K
from conftest import ROOT
from dark_amd._lib import DK_E_ARG
from test_gpu_fallbacks import _call, _env

pytestmark = pytest.mark.gpu
CAP = 1 << 17


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_exact(ctx, name, mode):
    c = K.CASES[name]()
    K.check(c, mode, K.call(ctx, c, mode), K.expected(name, mode)[1])


def test_a_context_of_exactly_n():
    """the sort's buffers for n fit a context whose capacity is n"""
    c = K.CASES["token_period_3"]()
    with dark_amd.Context(c.n) as small:
        K.check(c, "l", K.call(small, c, "l"), K.expected(c.name, "l")[1])


def test_refusals_leave_every_array_untouched(ctx):
    lib, h = ctx._lib, ctx._h
    n, count, groups = 70000, 1000, 400
    filled = lambda words: torch.full((words,), -0x3C3C3C3D, dtype=torch.int32, device="cuda")  # noqa: E731  (0xC3C3C3C3)
    names = ("text", "idx", "pos", "gid", "gstart", "rank", "nb", "sa", "bwt", "sym", "origin", "skeys", "sidx", "ssym", "oidx", "opos", "ogid", "ogstart", "osym")
    bufs = {name: filled(2 * n if name == "skeys" else n) for name in names}
    out = np.full(8, K.FILL32, np.uint32)
    torch.cuda.synchronize()
    p = {k: C.c_void_p(v.data_ptr()) for k, v in bufs.items()}
    sa_mode, l_mode = dict(bwt=None, sym=None, origin=None, ssym=None, osym=None), dict(sa=None)

    def call(ctx_h=h, n=n, depth=6, count=count, groups=groups, tsym=0, period=0, out_p=C.c_void_p(out.ctypes.data), **over):
        a = dict(dict(p, nb=None), **over)
        return lib.dk_dbg_dev_round(ctx_h, a["text"], n, depth, count, a["idx"], a["pos"], a["gid"], a["gstart"], groups, a["rank"], tsym, period, a["nb"], a["sa"],
                                    a["bwt"], a["sym"], a["origin"], a["skeys"], a["sidx"], a["ssym"], a["oidx"], a["opos"], a["ogid"], a["ogstart"], a["osym"], out_p)

    refused = [("null context", dict(ctx_h=None, **sa_mode)), ("both modes", {}), ("neither mode", dict(sa_mode, sa=None)),
               ("part of the L mode: no d_sym", dict(l_mode, sym=None)), ("part of the L mode: no d_origin", dict(l_mode, origin=None)),
               ("part of the L mode: no d_out_sorted_sym", dict(l_mode, ssym=None)), ("part of the L mode: no d_out_sym", dict(l_mode, osym=None)),
               ("d_sa with d_sym", dict(sa_mode, sym=p["sym"]))]
    for mode in (sa_mode, l_mode):
        refused += [("n = 1", dict(mode, n=1, count=1, groups=1)), ("n above the capacity", dict(mode, n=CAP + 1)), ("no slots", dict(mode, count=0)),
                    ("more slots than suffixes", dict(mode, count=n + 1)), ("depth 0", dict(mode, depth=0)), ("no groups", dict(mode, groups=0)),
                    ("more groups than slots", dict(mode, groups=count + 1)), ("more groups than the table holds", dict(mode, count=n, groups=n // 2 + 2)),
                    ("tsym below 0", dict(mode, tsym=-1)), ("tsym 64", dict(mode, tsym=64)), ("a doubling round without ranks", dict(mode, rank=None)),
                    ("a period below 0", dict(mode, tsym=8, period=-1, nb=p["nb"])), ("a period above the depth", dict(mode, tsym=8, period=7, nb=p["nb"])),
                    ("a period above 2^18", dict(mode, tsym=8, depth=1 << 19, period=(1 << 18) + 1, nb=p["nb"])),
                    ("a period without next breaks", dict(mode, tsym=8, period=2)), ("next breaks without a period", dict(mode, tsym=8, nb=p["nb"])),
                    ("a token round with tsym 4", dict(mode, tsym=4, period=2, nb=p["nb"])), ("a token round with tsym 0", dict(mode, period=2, nb=p["nb"])),
                    ("no out", dict(mode, out_p=None))]
        refused += [("null " + name, dict(mode, **{name: None})) for name in ("text", "idx", "pos", "gid", "gstart", "skeys", "sidx", "oidx", "opos", "ogid", "ogstart")]
    for name, over in refused:
        assert call(**over) == DK_E_ARG, name
    assert b"round" in lib.dk_last_error(h)
    with ctx.batch_begin("dark", host_threads=1):
        assert call(**sa_mode) == DK_E_ARG, "an open batch"
    assert b"batch" in lib.dk_last_error(h)
    with dark_amd.Context(n, purpose="decoder") as dec:
        assert call(ctx_h=dec._h, **sa_mode) == DK_E_ARG and b"decoder context" in lib.dk_last_error(dec._h)
    torch.cuda.synchronize()
    for name, t in bufs.items():
        assert bool((t == -0x3C3C3C3D).all()), "a refused call wrote to " + name
    assert (out == K.FILL32).all()
    c = K.CASES["rank_two_big"]()
    K.check(c, "sa", K.call(ctx, c, "sa"), K.expected(c.name, "sa")[1])  # ... and the context serves the next call


def test_poisoned_workspace_and_stale_mailbox():
    """three of the cases once more in a process of its own on the tuning library with DK_POISON=165 (every workspace allocation filled with 0xA5
    first) and after dk_dbg_mail_fill(0xA5) -- the group of 1024 with half in front of slot 2048, three big groups in a text round, a token
    round -- and one period case (tests/test_gpu_period.py): the same bytes as the plain run"""
    cmd = [sys.executable, os.path.join(ROOT, "tests", "round_worker.py"), ROOT, json.dumps(dict(cases=list(K.POISON), poison=165, mail_fill=0xA5))]
    p = _call(cmd, _env(dict(DK_POISON=165)), "DK_POISON=165")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout + p.stderr
    assert json.loads(line[-1][7:]) == dict({name: 2 for name in K.POISON}, period=1)
