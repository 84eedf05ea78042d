"""The period kernels and the text probes of the suffix sort by themselves, through dk_dbg_dev_period: k_period_first / _spine / _fill (the
next-break array the period round's token reads), k_run_probe, k_period_probe, k_period_count, k_period_search and k_prefix_probe (the counters the
host chooses its routes from) -- bit-exact against tests/period_model.py (tests/test_period_model.py pins the model and what every case is named
for on the CPU).  A wrong counter never makes a wrong suffix array, only a slower path, so no parity test notices one.

The next-break array holds 0xC3 before a call, with a pad behind, and is compared whole; the host words are compared whole.  The text stands at
any byte offset from an aligned address: the next breaks, the count and the search must not care, the run and period probes answer all zero
when their alignment (16 and 8 bytes) is not there."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import dark_amd
import period_cases as K
from dark_amd._lib import DK_E_ARG

pytestmark = pytest.mark.gpu
CAP = 1 << 17
SMALL = [name for name in sorted(K.CASES) if name not in K.LARGE]


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


@pytest.mark.parametrize("name", SMALL)
def test_exact(ctx, name):
    c = K.CASES[name]()
    K.check(c, K.call(ctx, c), K.expected(c))


@pytest.mark.parametrize("name", K.LARGE)
def test_the_spine_past_one_tile_per_chunk(name):
    """1025 tiles and a few bytes, 2049 tiles: the smallest texts at which a chunk of k_period_spine holds two and three tiles and its last chunks
    none (the spine cannot go wrong below that).  Bounded by the numpy model and the copies, which the output shows"""
    c = K.CASES[name]()
    t0 = time.time()
    want = K.expected(c)
    t1 = time.time()
    with dark_amd.Context(c.n) as big:
        t2 = time.time()
        got = K.call(big, c)
        t3 = time.time()
    print("%s: n = %d, model %.2f s, context %.2f s, call with copies %.2f s" % (name, c.n, t1 - t0, t2 - t1, t3 - t2))
    K.check(c, got, want)


def test_refusals_leave_every_array_untouched(ctx):
    lib, h = ctx._lib, ctx._h
    n = 70000
    text = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    nb = torch.full((n,), -0x3C3C3C3D, dtype=torch.int32, device="cuda")
    host = {name: np.full(32, K.FILL32, np.uint32) for name in ("run", "probe", "count", "found", "dups")}
    cands = np.array([4, 5, 6, 7], np.int32)
    torch.cuda.synchronize()
    hp = {k: C.c_void_p(v.ctypes.data) for k, v in host.items()}
    none = dict(run=None, probe=None, count=None, found=None, dups=None)

    def call(ctx_h=h, text_p=C.c_void_p(text.data_ptr()), n=n, period=0, nb_p=None, count_p=0, pmax=0, m=0, span=0, cands_p=None, ncands=0, **outs):
        o = dict(none, **outs)
        return lib.dk_dbg_dev_period(ctx_h, text_p, n, period, nb_p, o["run"], o["probe"], count_p, o["count"], pmax, o["found"], m, span, cands_p, ncands, o["dups"])

    nb_p, cands_p = C.c_void_p(nb.data_ptr()), C.c_void_p(cands.ctypes.data)
    prefix = dict(m=300, span=33, cands_p=cands_p, ncands=4, dups=hp["dups"])
    refused = [("null context", dict(ctx_h=None, run=hp["run"])), ("null text", dict(text_p=None, run=hp["run"])), ("n = 0", dict(n=0, run=hp["run"])),
               ("n above the capacity", dict(n=CAP + 1, run=hp["run"])), ("no part", {}), ("a period below 0", dict(period=-1, nb_p=nb_p)),
               ("a period above 2^18", dict(period=(1 << 18) + 1, nb_p=nb_p)), ("a period without d_next_break", dict(period=3)),
               ("d_next_break without a period", dict(nb_p=nb_p)), ("count_p without count_out", dict(count_p=3)), ("count_out without count_p", dict(count=hp["count"])),
               ("search_pmax without found_out", dict(pmax=100)), ("found_out without search_pmax", dict(found=hp["found"])),
               ("search_pmax 8", dict(pmax=8, found=hp["found"])), ("search_pmax above 2^18", dict(pmax=(1 << 18) + 1, found=hp["found"])),
               ("no candidates", dict(prefix, ncands=0)), ("five candidates", dict(prefix, ncands=5)), ("null candidates", dict(prefix, cands_p=None)),
               ("no samples", dict(prefix, m=0)), ("more samples than bytes", dict(prefix, m=n + 1)), ("span 0", dict(prefix, span=0)),
               ("prefix arguments without dups_out", dict(prefix, dups=None, run=hp["run"]))]
    for name, over in refused:
        assert call(**over) == DK_E_ARG, name
    assert b"period" in lib.dk_last_error(h)
    with ctx.batch_begin("dark", host_threads=1):
        assert call(run=hp["run"]) == DK_E_ARG, "an open batch"
    assert b"batch" in lib.dk_last_error(h)
    with dark_amd.Context(n, purpose="decoder") as dec:
        assert call(ctx_h=dec._h, run=hp["run"]) == DK_E_ARG and b"decoder context" in lib.dk_last_error(dec._h)
    # a candidate the text's alphabet has no room for is refused once the alphabet is known: one byte value, one-bit codes, 64 symbols in a key
    long_cands = np.array([4, 57], np.int32)
    assert call(**dict(prefix, cands_p=C.c_void_p(long_cands.ctypes.data), ncands=2)) == DK_E_ARG and b"56 bits" in lib.dk_last_error(h)
    torch.cuda.synchronize()
    assert bool((nb == -0x3C3C3C3D).all()), "a refused call wrote to d_next_break"
    for name, a in host.items():
        assert (a == K.FILL32).all(), "a refused call wrote to " + name
    c = K.CASES["all_parts_at_once"]()
    K.check(c, K.call(ctx, c), K.expected(c))  # ... and the context serves the next call
