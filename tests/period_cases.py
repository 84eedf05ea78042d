"""TEST HELPER: the texts of tests/test_gpu_period.py, shared with tests/test_period_model.py (which pins on the CPU what each case is named for)
and with the poison worker (tests/round_worker.py).  A case is a text, the byte offset of its first byte from an aligned address, and the parts of
dk_dbg_dev_period it asks for; expected() is tests/period_model.py's answer to exactly those parts."""
import functools
from types import SimpleNamespace

import numpy as np

import period_model as P

FILL32 = 0xC3C3C3C3
PAD = 64
TILE = P.PB_TILE


def rnd(seed, sigma, n):
    return np.random.default_rng(seed).integers(0, sigma, size=n, dtype=np.uint8)


def stretches(n, p, seed, flips):
    """a text of period p (a random period string; p above n: random bytes) with the bytes at `flips` changed: the breaks are where a flip is
    compared with its partner, p in front of it and at it"""
    unit = rnd(seed, 200, max(1, min(p, n)))
    t = np.tile(unit, n // len(unit) + 1)[:n].copy()
    f = np.asarray([x for x in flips if 0 <= x < n], dtype=np.int64)
    t[f] ^= 0x80
    return t


CASES = {}


def case(name, text, offset=0, **parts):
    def make():
        t = np.ascontiguousarray(text(), dtype=np.uint8)
        return SimpleNamespace(name=name, text=t, n=len(t), offset=offset, parts=parts)
    CASES[name] = functools.lru_cache(maxsize=None)(make)


# ---- next breaks ------------------------------------------------------------------------------------------------------------------------------
NB_SIZES = (1, 15, 16, 17, 4095, 4096, 4097, 2 * TILE + 5)
for n in NB_SIZES:
    for p in sorted({q for q in (1, 7, 8, 9, 300, n - 1, n) if q >= 1}):
        # breaks a third and two thirds in, and at the last position a 16-byte load of the partner still has (n - p - 16 + 15)
        case("nb_n%d_p%d" % (n, p), functools.partial(stretches, n, p, 1000 + n + p, (n // 3, 2 * n // 3, n - 17)), period=p)
        if p in (1, 8, 9) and p < n:
            # zero bytes: T[n - p] equals the zero a load behind the text's end gives, so only the end-of-text mask makes n - p a break
            case("nb_zeros_n%d_p%d" % (n, p), functools.partial(np.zeros, n, np.uint8), period=p)
case("nb_quiet_tiles", functools.partial(stretches, 3 * TILE + 5, 3, 31, (2 * TILE + 100,)), period=3)          # no break in [0, 2 TILE + 97)
case("nb_break_ends_a_tile", functools.partial(stretches, 3 * TILE + 5, 5, 32, (TILE - 1 + 5,)), period=5)       # T[4095] != T[4100]
for off in (1, 8):
    for p in (1, 8, 9, 300):
        case("nb_offset_%d_p%d" % (off, p), functools.partial(stretches, 2 * TILE + 5, p, 40 + p, (TILE // 3, TILE + 7, 2 * TILE - 1)), offset=off, period=p)
# above 1024 tiles a chunk of the spine holds two tiles (1025 tiles: 513 chunks and 511 empty ones), above 2048 three; flips that leave stretches
# across several chunks, a chunk of its own without a break, and a break in the first and the last tile of a chunk
SPINE_FLIPS = (5, 3 * TILE + 1, 4 * TILE - 3, 700 * TILE + 9, 1023 * TILE, 1024 * TILE + 4000, 2047 * TILE - 1, 2048 * TILE + 2)
case("nb_spine_1025_tiles", functools.partial(stretches, 1025 * TILE + 7, 2, 51, SPINE_FLIPS), period=2)
case("nb_spine_2049_tiles", functools.partial(stretches, 2049 * TILE, 3, 52, SPINE_FLIPS), period=3)
LARGE = ("nb_spine_1025_tiles", "nb_spine_2049_tiles")


# ---- probes -----------------------------------------------------------------------------------------------------------------------------------
def runs_in_text(n=70000):
    """random bytes with runs of zeros: 600 from a multiple of 256 on (two whole windows), 600 from 7 behind one (one), 40 (pieces only)"""
    t = rnd(61, 256, n)
    for start, length in ((10 * 256, 600), (40 * 256 + 7, 600), (90 * 256 + 16, 40), (n - 300, 300)):
        t[start:start + length] = 0
    return t


def table(rows, width=1000, seed=62):
    return lambda: np.tile(rnd(seed, 256, width), rows)


BOTH = dict(run=True, probe=True)
case("probe_all_equal", lambda: np.full(70000, 7, np.uint8), count_p=5, **BOTH)
case("probe_period_3", functools.partial(stretches, 70000, 3, 63, (20000, 50001)), count_p=3, **BOTH)
case("probe_period_3_count_6", functools.partial(stretches, 70000, 3, 63, (20000, 50001)), count_p=6)
case("probe_random", lambda: rnd(64, 256, 70000), count_p=4, **BOTH)
case("probe_runs", runs_in_text, count_p=1, **BOTH)
for n in (71, 72, 73, 135, 136, 137, 255, 256, 257, 511, 512, 513):
    case("probe_n%d" % n, functools.partial(np.full, n, 9, np.uint8), count_p=8, **BOTH)
for n in (72, 73, 74, 1063, 1064, 1065):
    case("count_n%d" % n, functools.partial(np.full, n, 9, np.uint8), count_p=9 if n < 100 else 1000)
for off in (1, 4, 8, 16):
    case("probe_runs_offset_%d" % off, runs_in_text, offset=off, count_p=1, **BOTH)
# the search: every sample of a table of 1000-byte rows sees 1000, 2000, 3000 and 4000 (the smallest must win), none where the sample is cut off
case("search_table", table(64), search_pmax=4096, count_p=1000)
case("search_table_cut_off", table(12), search_pmax=4096)
case("search_none", lambda: rnd(65, 256, 70000), search_pmax=4096)
case("search_period_above_pmax", table(64), search_pmax=999)
case("search_smallest_pmax", functools.partial(stretches, 4000, 9, 66, ()), search_pmax=9)
# the prefix probe as the sort would ask: about 10 sqrt(n) samples n / m apart, the lengths that four to seven radix passes cover
case("prefix_random", lambda: rnd(67, 256, 100000), prefix=(3000, 33, (4, 5, 6, 7)))
case("prefix_acgt", lambda: np.tile(rnd(68, 4, 5000), 20) + 65, prefix=(3000, 33, (16, 20, 24, 28)))   # twenty copies of 5000 bytes
case("prefix_acgt_random", lambda: rnd(68, 4, 100000) + 65, prefix=(3000, 33, (4, 8, 16)))
case("prefix_two_lengths_past_the_end", lambda: rnd(69, 4, 3000), prefix=(310, 10, (3, 28)))  # the last ten samples stand behind the text

# every part in one call: the prefix probe reads the alphabet first, which clears the words the run and period probes count in
def runs_under_a_sample():
    t = runs_in_text()
    t[9800:10300] = 0  # (the sample at 9 * 70000 // 64 = 9843 stands in it)
    return t


case("all_parts_at_once", runs_under_a_sample, period=1, count_p=1, search_pmax=600, prefix=(500, 140, (4, 7)), **BOTH)

POISON = "all_parts_at_once"


def call(ctx, c):
    return ctx.dbg_dev_period(c.text, text_offset=c.offset, fill=0xC3, pad=PAD, **c.parts)


def expected(c):
    want = dict(next_break=None, run=None, probe=None, count=None, found=None, dups=None)
    if c.parts.get("period"):
        want["next_break"] = np.concatenate([P.next_break(c.text, c.parts["period"]), np.full(PAD, FILL32, np.uint32)])
    if c.parts.get("run"):
        want["run"] = P.run_probe(c.text, c.offset)
    if c.parts.get("probe"):
        want["probe"] = P.period_probe(c.text, c.offset)
    if c.parts.get("count_p"):
        want["count"] = P.period_count(c.text, c.parts["count_p"])
    if c.parts.get("search_pmax"):
        want["found"] = P.period_search(c.text, c.parts["search_pmax"])
    if c.parts.get("prefix"):
        want["dups"] = P.prefix_probe(c.text, *c.parts["prefix"])
    return want


def check(c, got, want):
    for name, w in want.items():
        if w is None:
            assert got[name] is None, (c.name, name)
        elif isinstance(w, int):
            assert got[name] == w, (c.name, name, got[name], w)
        else:
            d = np.flatnonzero(got[name] != w)
            assert got[name].dtype == w.dtype and got[name].shape == w.shape and not len(d), (c.name, name, len(d), d[:1], got[name][d[:1]], w[d[:1]])
