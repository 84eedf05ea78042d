"""The suffix-array check on the GPU (dk_dev_sa_check, its host and packed forms; csrc/sa_query.hip).  Valid arrays come from
dev_suffix_array and must be found in order; damaged ones must give exactly the (verdict, where) of the plain model of tests/sa_query_model.py
(pinned by tests/test_sa_query_model.py).  The arrays sit between GUARD words, as in tests/test_gpu_lcp.py."""
import os
import subprocess
import time

import numpy as np
import pytest
import torch

import dark_amd
from conftest import ROOT
from dark_amd import datagen
from sa_query_model import BAD_ORDER, BAD_RANGE, NOT_PERMUTATION, OK, check_model
from test_gpu_lcp import Words, dev_text, fibonacci_word, u8

pytestmark = pytest.mark.gpu
CAP = 1 << 20
TIMEOUT = 120
PACK_SIZES = [1, 2, 300, 4097, 65537, 1, 300, 2]  # the one-byte head keeps every later block off the 256-slot tiles


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


def put(words, values):
    words.t.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint32).view(np.int32)))


def gpu_sa(ctx, t, shift=0):
    sa = Words(len(t), shift)
    ctx.dev_suffix_array(dev_text(t), len(t), sa.t)
    assert sa.guards_intact()
    return sa


def gpu_check(ctx, t, values, shifts=(0, 0)):
    """(verdict, where) of dev_sa_check for `values` as the array of text t"""
    sa = Words(len(t), shifts[1])
    put(sa, values)
    got = ctx.dev_sa_check(dev_text(t, shifts[0]), len(t), sa.t)
    assert sa.guards_intact() and np.array_equal(sa.host(), np.asarray(values, dtype=np.uint32)), "the check wrote to its input"
    return got


def markov(n, seed):
    return u8(datagen.wiki_like(n, seed=seed))


# ---- valid arrays ----------------------------------------------------------------------------------------------------------------------------

def two_halves():
    h = np.random.default_rng(8).integers(0, 256, size=20000, dtype=np.uint8)
    return np.concatenate([h, h])


VALID = {
    "n1": lambda: b"a", "n1_ff": lambda: b"\xff", "n2_aa": lambda: b"aa", "n2_ab": lambda: b"ab", "n2_ba": lambda: b"ba",
    "n3_aaa": lambda: b"aaa", "n3_aba": lambda: b"aba", "n3_cba": lambda: b"cba",
    **{"a_%d" % n: (lambda n=n: b"a" * n) for n in (255, 256, 257, 4095, 4096, 4097)},
    "abab": lambda: b"ab" * 3000 + b"a",
    "fibonacci": lambda: fibonacci_word(10946),
    "two_halves": two_halves,
    "random_5000": lambda: np.random.default_rng(3).integers(0, 256, size=5000, dtype=np.uint8),
    "markov_70000": lambda: markov(70000, 4),
}


@pytest.mark.parametrize("name", sorted(VALID))
def test_valid(ctx, name):
    t = u8(VALID[name]())
    n = len(t)
    sa = gpu_sa(ctx, t)
    assert ctx.dev_sa_check(dev_text(t), n, sa.t) == (OK, n)
    assert sa.guards_intact()
    assert check_model(t, sa.host()) == (OK, n)


@pytest.mark.parametrize("shifts", [(1, 0), (3, 0), (0, 1), (0, 3), (1, 3), (3, 1)])
def test_valid_off_their_alignment(ctx, shifts):
    """the text moved by 1 and 3 bytes, the array by 1 and 3 of its elements"""
    t = markov(20011, 5)
    sa = gpu_sa(ctx, t).host()
    assert gpu_check(ctx, t, sa, shifts) == (OK, len(t))
    sa[[100, 15000]] = sa[[15000, 100]]
    assert gpu_check(ctx, t, sa, shifts) == check_model(t, sa)


# ---- damaged arrays --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def base(ctx):
    """a text that ends in its smallest byte, and its suffix array"""
    t = np.concatenate([np.maximum(markov(20010, 6), 1), [0]]).astype(np.uint8)
    sa = gpu_sa(ctx, t).host()
    assert check_model(t, sa) == (OK, len(t)) and sa[0] == len(t) - 1
    return t, sa


def by_first_byte(t, reverse_bucket):
    """sorted by the first byte only, positions rising inside a bucket -- and falling in one: no pair of neighbours differs in its first byte the wrong
    way, only the order behind it (condition (c)) shows it"""
    sa = np.argsort(t, kind="stable").astype(np.uint32)
    inside = np.flatnonzero(t[sa] == reverse_bucket)
    sa[inside] = sa[inside][::-1].copy()
    return sa


def damage(t, sa, kind):
    n = len(t)
    v = sa.copy()
    if kind.startswith("entry_n_"):
        v[{"first": 0, "middle": n // 2, "last": n - 1}[kind[8:]]] = n
    elif kind == "entry_huge":
        v[7] = 0xFFFFFFFF
    elif kind == "duplicated":
        v[1234] = v[4321]
    elif kind == "duplicated_twice":
        v[1234] = v[4321]
        v[10] = v[11]
    elif kind == "adjacent_swapped":
        v[[5000, 5001]] = v[[5001, 5000]]
    elif kind == "distant_swapped":
        v[[17, n - 9]] = v[[n - 9, 17]]
    elif kind == "first_byte_only":
        v = by_first_byte(t, int(np.bincount(t).argmax()))
    elif kind == "last_suffix_one_up":
        v[[0, 1]] = v[[1, 0]]
    elif kind == "random_permutation":
        v = np.random.default_rng(11).permutation(n).astype(np.uint32)
    elif kind == "reversed":
        v = v[::-1].copy()
    elif kind == "range_and_duplicate":
        v[300] = v[301]
        v[9000] = n + 5
    else:
        raise KeyError(kind)
    return v


DAMAGE = {"entry_n_first": BAD_RANGE, "entry_n_middle": BAD_RANGE, "entry_n_last": BAD_RANGE, "entry_huge": BAD_RANGE, "duplicated": NOT_PERMUTATION,
          "duplicated_twice": NOT_PERMUTATION, "adjacent_swapped": BAD_ORDER, "distant_swapped": BAD_ORDER, "first_byte_only": BAD_ORDER,
          "last_suffix_one_up": BAD_ORDER, "random_permutation": BAD_ORDER, "reversed": BAD_ORDER, "range_and_duplicate": BAD_RANGE}


@pytest.mark.parametrize("kind", sorted(DAMAGE))
def test_damaged(ctx, base, kind):
    t, sa = base
    v = damage(t, sa, kind)
    want = check_model(t, v)
    assert want[0] == DAMAGE[kind], want  # (the test's own input is of the kind it is named after)
    assert gpu_check(ctx, t, v) == want


def test_array_of_another_text(ctx, base):
    t, _ = base
    other = np.concatenate([np.maximum(markov(len(t) - 1, 7), 1), [0]]).astype(np.uint8)
    v = gpu_sa(ctx, other).host()
    want = check_model(t, v)
    assert want[0] == BAD_ORDER
    assert gpu_check(ctx, t, v) == want


def test_end_rule(ctx):
    for t, v in ((b"aa", [0, 1]), (b"aa", [1, 0]), (b"aaa", [2, 0, 1]), (b"aba", [2, 0, 1]), (b"abab", [0, 2, 3, 1]), (b"abab", [2, 0, 1, 3])):
        assert gpu_check(ctx, u8(t), np.array(v, np.uint32)) == check_model(t, v), (t, v)
    assert gpu_check(ctx, u8(b"aa"), np.array([0, 1], np.uint32)) == (BAD_ORDER, 1)


def test_every_permutation_of_short_texts(ctx):
    """every permutation of every text of length 4 over `ab`, and of some of length 5, as one pack per text"""
    import itertools
    for n, texts in ((4, [bytes(x) for x in itertools.product(b"ab", repeat=4)]), (5, [b"ababa", b"aabaa", b"bbbbb", b"babab"])):
        perms = list(itertools.permutations(range(n)))
        for t in texts:
            d_in = dev_text(u8(t * len(perms)))
            sa = Words(n * len(perms))
            put(sa, np.array(perms, np.uint32).ravel())
            got = ctx.dev_sa_check_packed(d_in, [n] * len(perms), sa.t)
            assert got == [check_model(t, p) for p in perms], t
            assert sum(g == (OK, n) for g in got) == 1


def test_random_arrays_of_2p20_entries(ctx):
    """Arrays that fail at nearly every slot: random words (range), random entries below n (permutation), a random permutation (order).  Each
    answer is the model's.  The time of each is bounded against the valid array of the same size: the same three kernels pass over the same
    bytes (the order kernel stops at once for the first two), and on top a wave sends at most one atomic per block it covers, and only while
    its candidate is below the word -- so a damaged array should cost no more than the valid one.  The bound is four times that (the shortest
    of five calls each), against the noise of calls of a few hundred microseconds; an atomic per failing lane on one address costs tens
    of times the whole pass."""
    n = 1 << 20
    rng = np.random.default_rng(12)
    t = rng.integers(0, 256, size=n, dtype=np.uint8)
    d_in = dev_text(t)
    good = gpu_sa(ctx, t)

    def timed(words):
        best, got = None, None
        for _ in range(5):
            t0 = time.perf_counter()
            got = ctx.dev_sa_check(d_in, n, words.t)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return got, best

    got, t_valid = timed(good)
    assert got == (OK, n)
    cases = {"words": rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32), "below_n": rng.integers(0, n, size=n, dtype=np.uint32),
             "permutation": rng.permutation(n).astype(np.uint32)}
    kinds = {"words": BAD_RANGE, "below_n": NOT_PERMUTATION, "permutation": BAD_ORDER}
    for name, v in cases.items():
        w = Words(n)
        put(w, v)
        got, t_bad = timed(w)
        want = check_model(t, v)
        print("%s: %.3f ms, the valid array %.3f ms" % (name, 1e3 * t_bad, 1e3 * t_valid))
        assert want[0] == kinds[name] and got == want, (name, got, want)
        assert w.guards_intact()
        assert t_bad <= 4 * t_valid, (name, t_bad, t_valid)


# ---- packs -----------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pack(ctx):
    rng = np.random.default_rng(13)
    blocks = [rng.integers(97, 101, size=n, dtype=np.uint8) for n in PACK_SIZES]
    blocks[4] = markov(65537, 9)
    sizes = [len(b) for b in blocks]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    d_in = dev_text(np.concatenate(blocks))
    d_sa = Words(int(off[-1]))
    ctx.dev_suffix_array_packed(d_in, sizes, d_sa.t)
    sa = d_sa.host()
    return dict(blocks=blocks, sizes=sizes, off=off, d_in=d_in, sa=sa)


def check_pack_against_model(ctx, pack, values):
    w = Words(len(values))
    put(w, values)
    got = ctx.dev_sa_check_packed(pack["d_in"], pack["sizes"], w.t)
    assert w.guards_intact()
    off = pack["off"]
    want = [check_model(b, values[off[i]:off[i + 1]]) for i, b in enumerate(pack["blocks"])]
    assert got == want
    return got


def test_pack_valid(ctx, pack):
    got = check_pack_against_model(ctx, pack, pack["sa"])
    assert got == [(OK, n) for n in PACK_SIZES]


@pytest.mark.parametrize("block", [1, 2, 3, 4, 6, 7])
def test_pack_damage_stays_in_its_block(ctx, pack, block):
    off, n = pack["off"], PACK_SIZES[block]
    v = pack["sa"].copy()
    a, b = off[block], off[block] + n - 1
    v[[a, b]] = v[[b, a]]
    got = check_pack_against_model(ctx, pack, v)
    assert [g[0] for i, g in enumerate(got) if i != block] == [OK] * (len(PACK_SIZES) - 1) and got[block][0] == BAD_ORDER


def test_pack_entry_below_the_pack_but_outside_its_block(ctx, pack):
    off = pack["off"]
    v = pack["sa"].copy()
    v[off[2] + 17] = 300     # n of block 2
    v[off[5]] = 1            # a one-byte block: only 0 is in range
    v[off[3] + 4096] = 65536  # in range for block 4, not for block 3
    got = check_pack_against_model(ctx, pack, v)
    assert got[2] == (BAD_RANGE, 17) and got[5] == (BAD_RANGE, 0) and got[3] == (BAD_RANGE, 4096)
    assert [got[i][0] for i in (0, 1, 4, 6, 7)] == [OK] * 5


def test_pack_array_of_a_block_of_equal_length(ctx, pack):
    off = pack["off"]
    v = pack["sa"].copy()
    v[off[6]:off[7]] = pack["sa"][off[2]:off[3]]  # blocks 2 and 6: 300 bytes each, different texts
    got = check_pack_against_model(ctx, pack, v)
    assert got[6][0] == BAD_ORDER and got[2] == (OK, 300)


def test_pack_fuzz(ctx):
    rng = np.random.default_rng(2026)
    for k in range(20):
        blocks = []
        for _ in range(int(rng.integers(1, 12))):
            n = int(rng.choice([rng.integers(1, 20), rng.integers(1, 600), rng.integers(1, 5000)]))
            b = rng.integers(0, int(rng.choice([1, 2, 4, 256])), size=n, dtype=np.uint8)
            if rng.integers(0, 3) == 0:
                b = np.tile(b[:max(1, n // 5)], 5)[:n]
            blocks.append(b)
        sizes = [len(b) for b in blocks]
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        d_in = dev_text(np.concatenate(blocks))
        d_sa = Words(int(off[-1]))
        ctx.dev_suffix_array_packed(d_in, sizes, d_sa.t)
        v = d_sa.host()
        for i, n in enumerate(sizes):  # two blocks in three are damaged
            how, s = int(rng.integers(0, 6)), off[i]
            if how == 0:
                v[s + rng.integers(0, n)] = n + int(rng.integers(0, 3))
            elif how == 1 and n > 1:
                v[s + rng.integers(0, n)] = v[s + rng.integers(0, n)]
            elif how == 2 and n > 1:
                a, b = rng.integers(0, n, size=2)
                v[[s + a, s + b]] = v[[s + b, s + a]]
            elif how == 3:
                v[s:s + n] = rng.permutation(n)
        put(d_sa, v)
        got = ctx.dev_sa_check_packed(d_in, sizes, d_sa.t)
        assert d_sa.guards_intact()
        assert got == [check_model(b, v[off[i]:off[i + 1]]) for i, b in enumerate(blocks)], "pack %d" % k


# ---- the host form and the mirrors -----------------------------------------------------------------------------------------------------------

def test_host_form_and_constructor(ctx, base):
    t, sa = base
    assert ctx.sa_check(t, sa) == (OK, len(t))
    v = damage(t, sa, "duplicated")
    assert ctx.sa_check(t, v) == check_model(t, v)
    con = dark_amd.saca.Constructor(len(t))
    try:
        assert con.check(t, con.compute(t)) == (OK, len(t))
        v = damage(t, sa, "first_byte_only")
        assert con.check(t, v) == check_model(t, v)
        with pytest.raises(ValueError):
            con.check(t[:-1], sa[:-1])
    finally:
        con.context().close()


def test_cpp_mirror_check_and_search(tmp_path):
    exe = str(tmp_path / "cpp_sa_query")
    lib_dir = os.path.join(ROOT, "dark_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_sa_query.cpp"),
                           "-L", lib_dir, "-ldark_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=TIMEOUT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cpp sa query ok" in out.stdout
