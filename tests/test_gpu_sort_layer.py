"""The sort layer by itself (csrc/radix_sort.hip): the three-launch LSD sort, the one-workgroup sort, the group-by-group sort and the inverse
permutation through LDS windows, each through its debug entry point and against the plain models of tests/sort_model.py
(tests/test_sort_model.py pins those on the CPU).  Bit-exact everywhere.  Keys carry random bits below begin_bit and from end_bit up unless a
case says otherwise: a sort on [begin_bit, end_bit) orders by exactly those bits.  Values are `arange` in half of the cases (stability shows)
and random in the other half (a kernel that rebuilt values from positions would show).

The shapes are the smallest that reach a route: 8192 / 8193 pairs (one workgroup | three launches), 2^20 (digit plane), 4 194 304 / 4 194 305
pairs (1024 | 1025 tiles: tiles_per_chunk 1 | 2); groups around 2048 (block size 256 | 1024) and 8192; windows of 1024 .. 2048 words, one and
two levels for the inverse permutation.  Three levels need more than 2^27 entries and stay with tests/test_gpu_fullsize.py."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dark_amd
import sort_model as M
from conftest import ROOT
from dark_amd._lib import DK_E_ARG

pytestmark = pytest.mark.gpu
CAP = 6 << 20
TUNING_LIB = os.path.join(ROOT, "dark_amd", "libdark_amd_tuning.so")
TIMEOUT = 120  # seconds per subprocess; a setting takes a few
KEY_FILL, VAL_FILL = 0xC3C3C3C3C3C3C3C3, 0xC3C3C3C3  # what an output holds before a call that must leave parts of it alone
BIG = 4194304 + 3 * 4096 + 17

OLD_RANGES = [(0, 64), (0, 8), (8, 24), (0, 40), (16, 64)]
ODD_RANGES = [(0, 1), (0, 5), (0, 12), (8, 29), (3, 16), (13, 34), (57, 64), (0, 33)]


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool():
    """BIG random 64-bit keys and random values, made once; a case takes a prefix (and never writes to it)"""
    rng = np.random.default_rng(20)
    keys = rng.integers(0, 1 << 64, size=BIG, dtype=np.uint64)
    vals = rng.integers(0, 1 << 32, size=BIG, dtype=np.uint32)
    keys.flags.writeable = vals.flags.writeable = False
    return keys, vals


def first_diff(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "%s: %d entries, want %d" % (what, len(got), len(want))
    bad = np.flatnonzero(got != want)
    if len(bad) == 0:
        return None
    i = int(bad[0])
    return "%s: %d of %d differ, first at %d: got %#x want %#x" % (what, len(bad), len(got), i, int(got[i]), int(want[i]))


def check_pairs(label, got, want):
    (gk, gv), (wk, wv) = got, want
    d = first_diff("keys", gk, wk) or first_diff("values", gv, wv)
    assert d is None, "%s: %s" % (label, d)


def values(pool_vals, n, random):
    return pool_vals[:n] if random else np.arange(n, dtype=np.uint32)


def check_sort(ctx, keys, vals, lo, hi, label, entry="dev"):
    got = (ctx.dbg_dev_sort_pairs if entry == "dev" else ctx.dbg_sort_pairs)(keys, vals, lo, hi)
    check_pairs("%s %d pairs bits [%d, %d) %s entry" % (label, len(keys), lo, hi, entry), got, M.sort_pairs_model(keys, vals, lo, hi))


# ---- sort_pairs: counts --------------------------------------------------------------------------------------------------------------
SMALL_COUNTS = [1, 2, 63, 64, 65, 511, 512, 513, 8191, 8192]      # one workgroup
CLASSIC_COUNTS = [8193, 12289, 36865]                              # 3, 4 and 9 tiles: the XCD grid of 8 or 16 workgroups leaves some idle


@pytest.mark.parametrize("count", SMALL_COUNTS + CLASSIC_COUNTS)
def test_sort_pairs_every_range(ctx, pool, count):
    for i, (lo, hi) in enumerate(OLD_RANGES + ODD_RANGES):
        check_sort(ctx, pool[0][:count], values(pool[1], count, (i + count) % 2 == 1), lo, hi, "uniform")


@pytest.mark.parametrize("count", [(1 << 20) - 1, 1 << 20, (1 << 20) + 1])
def test_sort_pairs_where_the_digit_plane_starts(ctx, pool, count):
    """(0,5) and (0,8): one pass, no plane.  (0,12): the plane is written by the first pass and read by the last, whose digit is narrow.
    (8,29), (13,34): three passes, the middle one reads and writes the plane.  (0,33): five passes.  (0,64): all eight."""
    for i, (lo, hi) in enumerate([(0, 5), (0, 8), (0, 12), (8, 29), (13, 34), (0, 33), (0, 64)]):
        check_sort(ctx, pool[0][:count], values(pool[1], count, (i + count) % 2 == 1), lo, hi, "uniform")


@pytest.mark.parametrize("count", [4194304, 4194305, BIG])
def test_sort_pairs_where_a_chunk_takes_two_tiles(ctx, pool, count):
    """1024 tiles: a histogram workgroup per tile.  1025: two tiles per workgroup, the last chunk holds one.  BIG: 1028 tiles, an odd tail.
    At most two passes each (the host reference stays short): a narrow last digit behind the plane, one off the byte grid, a single pass."""
    for i, (lo, hi) in enumerate([(0, 12), (3, 16), (57, 64)]):
        check_sort(ctx, pool[0][:count], values(pool[1], count, (i + count) % 2 == 1), lo, hi, "uniform")


def test_sort_pairs_host_entry_matches_device_entry(ctx, pool):
    for count, lo, hi in ((5000, 8, 29), (12289, 13, 34), (12289, 0, 64)):
        keys, vals = pool[0][:count], pool[1][:count]
        check_sort(ctx, keys, vals, lo, hi, "uniform", entry="host")
        check_pairs("host against device entry", ctx.dbg_sort_pairs(keys, vals, lo, hi), ctx.dbg_dev_sort_pairs(keys, vals, lo, hi))


# ---- sort_pairs: key shapes ------------------------------------------------------------------------------------------------------------
def shaped_field(shape, rng, n, w):
    """n fields of w bits (uint64) of the named shape"""
    top = (1 << w) - 1
    rnd = rng.integers(0, 1 << 64, size=n, dtype=np.uint64) & np.uint64(top)
    if shape == "uniform":
        return rnd
    if shape == "equal":
        return np.full(n, int(rnd[0]), np.uint64)
    if shape == "ones":  # the padding key of the LDS kernels
        return np.full(n, top, np.uint64)
    if shape == "sorted":
        return np.sort(rnd)
    if shape == "reverse":
        return np.sort(rnd)[::-1].copy()
    if shape == "alternating":
        return np.where(np.arange(n) % 2 == 0, rnd[0], rnd[n // 2]).astype(np.uint64)
    if shape == "duplicates":
        return rnd & np.uint64(0x00FF00FF00FF00FF)
    if shape == "skewed":  # one value of every digit holds all but 1 % of the pairs, in every pass
        return np.where(rng.random(n) < 0.99, np.uint64(0x5A5A5A5A5A5A5A5A & top), rnd).astype(np.uint64)
    raise ValueError(shape)


def keys_with_field(rng, f, lo, hi):
    """the field at bits [lo, hi), random bits everywhere else"""
    w = hi - lo
    inside = ((1 << w) - 1) << lo
    noise = rng.integers(0, 1 << 64, size=len(f), dtype=np.uint64) & np.uint64(~inside & 0xFFFFFFFFFFFFFFFF)
    return (f << np.uint64(lo)) | noise


SHAPES = ["uniform", "equal", "ones", "sorted", "reverse", "alternating", "duplicates", "skewed"]


@pytest.mark.parametrize("count", [5000, 20011])  # one workgroup | five tiles, the last one short
@pytest.mark.parametrize("shape", SHAPES)
def test_sort_pairs_key_shapes(ctx, pool, shape, count):
    rng = np.random.default_rng(SHAPES.index(shape) * 7 + count)
    for i, (lo, hi) in enumerate([(0, 64), (0, 12), (8, 29), (13, 34), (16, 64), (0, 5)]):
        keys = keys_with_field(rng, shaped_field(shape, rng, count, hi - lo), lo, hi)
        check_sort(ctx, keys, values(pool[1], count, i % 2 == 1), lo, hi, shape)


# ---- sort_pairs: which kernels ran ---------------------------------------------------------------------------------------------------------
def test_sort_pairs_routes_and_pass_counts(ctx, pool):
    """launches are counted while profiling is on (csrc/context.hpp LaunchScope); sort_passes always"""
    ctx.set_profiling(True)
    try:
        for count in (1, 2, 64, 8191, 8192, 8193, 12289, (1 << 20) + 1):
            for lo, hi in ((0, 64), (0, 5), (0, 12), (8, 29), (13, 34), (0, 33)):
                ctx.stats_reset()
                check_sort(ctx, pool[0][:count], pool[1][:count], lo, hi, "uniform")
                st = ctx.stats()
                launches = {k: v["launches"] for k, v in st["kernels"].items()}
                passes = -(-(hi - lo) // 8)
                if count == 1:  # nothing to sort: no launch at all
                    assert launches == {} and st["sort_passes"] == 0, (count, lo, hi, launches)
                    continue
                assert st["sort_passes"] == passes, (count, lo, hi, st["sort_passes"])
                if count <= 8192:
                    assert launches == {"k_radix_sort_small": 1}, (count, lo, hi, launches)
                else:
                    assert launches == {"k_radix_hist": passes, "k_radix_scan": passes, "k_radix_scatter": passes}, (count, lo, hi, launches)
    finally:
        ctx.set_profiling(False)


# ---- local sort ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 8191, 8192, 8193, 3 * 8192 + 5])
def test_local_sort(ctx, pool, count):
    for i, (lo, hi) in enumerate([(0, 64), (8, 21), (0, 5)]):
        keys, vals = pool[0][:count], values(pool[1], count, (i + count) % 2 == 1)
        check_pairs("local sort of %d pairs bits [%d, %d)" % (count, lo, hi), ctx.dbg_dev_local_sort(keys, vals, lo, hi),
                    M.local_sort_model(keys, vals, lo, hi))


# ---- sort_groups -----------------------------------------------------------------------------------------------------------------------
GROUP_SIZES = [0, 1, 2, 255, 256, 257, 511, 512, 513, 1024, 1025, 2047, 2048, 2049, 3072, 4096, 4097, 8191, 8192, 8193, 20000]
TAIL = 37  # pairs behind the last group: no group's, never written


def group_pack(rng, above, lo, hi, random_above=False):
    """-> (keys, vals, starts, sizes): the sizes around every limit of k_sort_groups (class bounds `above`, 2048, 8192; block sizes; one pair
    per thread more) in shuffled order, then 300 groups of 257 .. 400 members (many workgroups of the small class side by side), then TAIL
    pairs outside every group.  Below lo the keys are random; from hi up they hold a per-group constant, as the L-first caller's do
    (random_above: random bits there too)."""
    sizes = GROUP_SIZES + [above, above + 1]
    sizes = [sizes[i] for i in rng.permutation(len(sizes))] + rng.integers(257, 401, size=300).tolist()
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    n = int(starts[-1]) + TAIL
    keys = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    if hi < 64 and not random_above:
        per_group = rng.integers(0, 1 << 64, size=len(sizes) + 1, dtype=np.uint64)
        group_of = np.repeat(np.arange(len(sizes) + 1), sizes + [TAIL])
        below_hi = np.uint64((1 << hi) - 1)
        keys = (keys & below_hi) | (per_group[group_of] & ~below_hi)
    return keys, rng.integers(0, 1 << 32, size=n, dtype=np.uint32), starts, sizes


def run_group_pack(ctx, rng, above, lo, hi, in_place, random_values=True, random_above=False):
    keys, vals, starts, sizes = group_pack(rng, above, lo, hi, random_above)
    n = len(keys)
    if not random_values:
        vals = np.arange(n, dtype=np.uint32)
    if in_place:
        before = (keys, vals)
        got = ctx.dbg_dev_sort_groups(keys, vals, starts, above, lo, hi)
    else:
        before = (np.full(n, KEY_FILL, np.uint64), np.full(n, VAL_FILL, np.uint32))
        got = ctx.dbg_dev_sort_groups(keys, vals, starts, above, lo, hi, kout=before[0], vout=before[1])
    label = "sort_groups above %d bits [%d, %d) %s" % (above, lo, hi, "in place" if in_place else "out of place")
    check_pairs(label, got, M.sort_groups_model(keys, vals, before[0], before[1], starts, above, lo, hi))
    return got, starts, sizes


@pytest.mark.parametrize("above", [0, 64, 256, 2048, 3000])  # 3000: the large class starts at max(above, 2048)
def test_sort_groups(ctx, above):
    rng = np.random.default_rng(100 + above)
    for i, (lo, hi) in enumerate([(8, 8 + 13), (0, 64), (8, 16), (0, 5)]):
        for in_place in (False, True):
            run_group_pack(ctx, rng, above, lo, hi, in_place, random_values=(i + in_place) % 2 == 0)


def test_sort_groups_random_bits_above_the_range(ctx):
    rng = np.random.default_rng(7)
    for lo, hi in ((8, 8 + 13), (0, 5)):
        for in_place in (False, True):
            run_group_pack(ctx, rng, 256, lo, hi, in_place, random_above=True)


def test_sort_groups_leaves_other_classes_alone(ctx):
    """out of place with above = 256: what the output held survives in the groups of 0, 1, 2, 255, 256, 8193 and 20 000 members and behind
    the last group (the comparison with the model says the same; this names the places)"""
    (kout, vout), starts, sizes = run_group_pack(ctx, np.random.default_rng(8), 256, 8, 21, in_place=False)
    seen = set()
    for g, size in enumerate(sizes):
        a, b = int(starts[g]), int(starts[g + 1])
        if size in (0, 1, 2, 255, 256, 8193, 20000):
            seen.add(size)
            assert (kout[a:b] == KEY_FILL).all() and (vout[a:b] == VAL_FILL).all(), "group of %d members was written" % size
        elif size <= 8192:
            assert not (kout[a:b] == KEY_FILL).all(), "group of %d members was not written" % size
    assert seen == {0, 1, 2, 255, 256, 8193, 20000}
    assert (kout[-TAIL:] == KEY_FILL).all() and (vout[-TAIL:] == VAL_FILL).all()


# ---- inverse permutation -----------------------------------------------------------------------------------------------------------------
def permutations(rng, n):
    """identity: a tile of the split falls into one bin | reverse | random | p * 65537 mod n: a tile spreads over every bin"""
    out = [("identity", np.arange(n, dtype=np.uint32)), ("reverse", np.arange(n - 1, -1, -1, dtype=np.uint32)),
           ("random", rng.permutation(n).astype(np.uint32))]
    if math.gcd(n, 65537) == 1:
        out.append(("stride", (np.arange(n, dtype=np.uint64) * np.uint64(65537) % np.uint64(n)).astype(np.uint32)))
    return out


def check_inverse(ctx, label, sa, marked_val=None):
    d = first_diff("rank", ctx.dbg_dev_inverse_permutation(sa, marked_val), M.inverse_permutation_model(sa, marked_val))
    assert d is None, "inverse permutation, %s, n = %d: %s" % (label, len(sa), d)


ISA_SIZES = [1, 2, 3, 5, 1023, 1024, 1025, 1027,       # the odd tail and the sub-quad tail of k_isa_assemble
             4095, 4096, 4097,                          # the split's tile
             65535, 65536, 65537,                       # 64 windows of 1024 words: one level | sections
             65536 + 4096 * 3 + 5, 1000003,
             1 << 22, (1 << 22) + 1]                    # windows of 1024 | 2048 words


@pytest.mark.parametrize("n", ISA_SIZES)
def test_inverse_permutation(ctx, n):
    rng = np.random.default_rng(n)
    for name, sa in permutations(rng, n):
        check_inverse(ctx, name, sa)
        marked = sa.copy()
        marked[rng.random(n) < 1 / 3] |= np.uint32(M.MARK)
        check_inverse(ctx, name + ", a third marked", marked, rng.integers(0, 1 << 32, size=n, dtype=np.uint32))


@pytest.mark.parametrize("n", [5, 4097, 65536 + 4096 * 3 + 5])
def test_inverse_permutation_all_marked_and_none_marked(ctx, n):
    rng = np.random.default_rng(n + 1)
    sa = rng.permutation(n).astype(np.uint32)
    mv = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    check_inverse(ctx, "every entry marked", sa | np.uint32(M.MARK), mv)
    check_inverse(ctx, "values given, nothing marked", sa, mv)


# ---- errors, then correct ------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_then_a_correct_sort(ctx, pool):
    lib, h = ctx._lib, ctx._h
    n = 100
    dk = torch.zeros(n, dtype=torch.int64, device="cuda")
    dv = torch.zeros(n, dtype=torch.int32, device="cuda")
    k, v = C.c_void_p(dk.data_ptr()), C.c_void_p(dv.data_ptr())
    starts = np.array([0, 10, 30, 100], np.uint32)
    sp = C.c_void_p(starts.ctypes.data)
    torch.cuda.synchronize()
    for fn in (lib.dk_dbg_dev_sort_pairs, lib.dk_dbg_dev_local_sort):
        assert fn(None, k, v, n, 0, 64) == DK_E_ARG
        assert fn(h, None, v, n, 0, 64) == DK_E_ARG
        assert fn(h, k, None, n, 0, 64) == DK_E_ARG
        assert fn(h, k, v, 0, 0, 64) == DK_E_ARG
    groups = lib.dk_dbg_dev_sort_groups
    assert groups(None, k, v, k, v, sp, 3, n, 0, 0, 64) == DK_E_ARG
    for bad in range(5):
        args = [k, v, k, v, sp]
        args[bad] = None
        assert groups(h, *args, 3, n, 0, 0, 64) == DK_E_ARG, bad
    assert groups(h, k, v, k, v, sp, 0, n, 0, 0, 64) == DK_E_ARG   # no group
    assert groups(h, k, v, k, v, sp, 3, 0, 0, 0, 64) == DK_E_ARG   # no pair
    assert groups(h, k, v, k, v, sp, 3, 99, 0, 0, 64) == DK_E_ARG  # the last group ends behind the pairs
    for bad_starts in ([0, 30, 10, 100], [5, 0, 0, 0], [0, 10, 30, 29]):
        b = np.array(bad_starts, np.uint32)
        assert groups(h, k, v, k, v, C.c_void_p(b.ctypes.data), 3, n, 0, 0, 64) == DK_E_ARG, bad_starts
    assert b"starts" in lib.dk_last_error(h)
    assert groups(h, k, v, k, v, sp, 3, n, 0, 8, 65) == DK_E_ARG
    inv = lib.dk_dbg_dev_inverse_permutation
    assert inv(None, v, n, v, None) == DK_E_ARG
    assert inv(h, None, n, v, None) == DK_E_ARG
    assert inv(h, v, n, None, None) == DK_E_ARG
    assert inv(h, v, 0, v, None) == DK_E_ARG
    assert (dk == 0).all() and (dv == 0).all()  # none of the refused calls wrote
    # the context still works
    for count in (5000, 12289):
        check_sort(ctx, pool[0][:count], pool[1][:count], 8, 29, "after refused calls")
    run_group_pack(ctx, np.random.default_rng(9), 64, 8, 21, in_place=True)
    check_inverse(ctx, "after refused calls", np.random.default_rng(10).permutation(4097).astype(np.uint32))


# ---- the tuning build's variants of these kernels -------------------------------------------------------------------------------------------
def reduced_matrix():
    """what every variant must still get right; runs in a process of its own (the switches are read once per process)"""
    rng = np.random.default_rng(30)
    keys = rng.integers(0, 1 << 64, size=4194305, dtype=np.uint64)
    vals = rng.integers(0, 1 << 32, size=4194305, dtype=np.uint32)
    with dark_amd.Context(CAP) as ctx:
        for count, ranges in ((8193, [(0, 12), (8, 29)]), ((1 << 20) + 1, [(0, 12), (8, 29)]), (4194305, [(0, 12), (3, 16)])):
            for i, (lo, hi) in enumerate(ranges):
                check_sort(ctx, keys[:count], values(vals, count, i == 0), lo, hi, "uniform")
        for in_place in (False, True):
            run_group_pack(ctx, rng, 256, 8, 21, in_place)
        sa = rng.permutation(1000003).astype(np.uint32)
        sa[rng.random(len(sa)) < 1 / 3] |= np.uint32(M.MARK)
        check_inverse(ctx, "random, a third marked", sa, rng.integers(0, 1 << 32, size=len(sa), dtype=np.uint32))
    print("ok")


VARIANT_SNIPPET = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_sort_layer as T; T.reduced_matrix()" % (ROOT, os.path.join(ROOT, "tests"))


@pytest.mark.parametrize("env", [{"DK_SCATTER_BLOCK": "512"}, {"DK_XCD": "0"}, {"DK_DIGIT_PLANE": "0"}, {"DK_DIGIT_PLANE": "2"},
                                 {"DK_SCATTER_PROBE": "1"}, {"DK_POISON": "165"}], ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_tuning_variants(env):
    assert os.path.exists(TUNING_LIB), "build the tuning library: python dark_amd/build.py --tuning (__graft_entry__.build() does)"
    e = dict(os.environ)
    e.update(env)
    e["DARK_AMD_LIB"] = TUNING_LIB
    out = subprocess.run([sys.executable, "-c", VARIANT_SNIPPET], env=e, capture_output=True, text=True, timeout=TIMEOUT)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-3000:]
