"""The enumerations, packs and plain models of tests/short_texts.py, checked without a GPU: the closed-form counts; the models against the oracle
and the other models on every text of the smaller sets; the (L, origin) pairs that are a text, counted and named; every pack DECIDES between
the true model and each fault model of short_texts.FAULTS (a pack that a fault leaves unchanged tests nothing about that fault); and the
first-key arithmetic of pk_first (csrc/packed.hip) restated per pack, with the number of rounds that follows from it and from the model's LCP.
tests/test_gpu_short_texts.py imports FIRST_KEY from here and hands the same packs to the kernels."""
import itertools
import os

import numpy as np
import pytest

import ibwt_model
import short_texts as T
from conftest import ROOT
from dark_amd._lib import DK_PACKED_MAX_BLOCKS
from lcp_model import lcp_kasai

# per pack: (blk_bits, bits, symbols in the first key, rounds) -- what pk_first chooses and what packed_sort_device then needs
FIRST_KEY = {
    "bin15":          (16, 2, 24, 0),  # 65 534 blocks, 2 symbols: (64 - 16) / 2 = 24 >= 15, every suffix final after the first sort
    "bin15_wide":     (16, 9, 5, 2),   # 65 535 blocks, 256 symbols: (64 - 16) / 9 = 5; a^15 shares 14: rounds at h = 5 and h = 10
    "bin15_reversed": (16, 9, 5, 2),
    "bin15_shuffled": (16, 9, 5, 2),
    "neighbours":     (13, 9, 5, 1),   # 8161 blocks: (64 - 13) / 9 = 5; a^8 shares 7: the round at h = 5
    "mixed":          (14, 3, 16, 0),  # 13 932 blocks, 5 symbols (codes 1..5, 3 bits): (64 - 14) / 3 = 16 >= 10
}


def ceil_log2(v):
    """smallest b with (1 << b) >= v (ceil_log2_u64, csrc/context.hpp)"""
    b = 0
    while (1 << b) < v:
        b += 1
    return b


def first_key(blocks):
    """pk_first's choices for a pack, in its own expressions"""
    total = sum(len(b) for b in blocks)
    sigma = len(set(b"".join(blocks)))
    bits = max(1, ceil_log2(sigma + 1))          # f->bits: codes 1 .. sigma, 0 is the padding
    blk_bits = ceil_log2(len(blocks))            # f->blk_bits
    k = max(1, (64 - blk_bits) // bits)
    k_used = min(k, max(1, total))               # f->k_used
    return blk_bits, bits, k_used


def rounds_needed(k, longest):
    """two suffixes of a block share a first key exactly when they share k symbols (they differ in length, and the padding code is no
    symbol's); a round at depth h settles what differs within 2 h, and h starts at k and doubles"""
    r, h = 0, k
    while h <= longest:
        h *= 2
        r += 1
    return r


@pytest.fixture(scope="module")
def true_arrays():
    """expected arrays per pack, built on demand and kept"""
    kept = {}

    def get(name):
        if name not in kept:
            kept[name] = T.expected(T.pack(name).blocks)
        return kept[name]
    return get


# ---- 1. counts and totals --------------------------------------------------------------------------------------------------------------------

def test_counts_and_totals():
    for m in range(1, 16):
        assert T.count_and_bytes(2, m) == (2 ** (m + 1) - 2, (m - 1) * 2 ** (m + 1) + 2)
    want = dict(BIN15=65534, BIN12=8190, BIN10=2046, TER8=9840, EXT10=2046)
    for name, count in want.items():
        alphabet, lo, hi = T.SETS[name]
        ts = T.text_set(name)
        assert lo == 1 and (len(ts), sum(len(t) for t in ts)) == T.count_and_bytes(len(alphabet), hi) and len(ts) == count, name
        assert len(set(ts)) == len(ts) and ts == sorted(ts, key=lambda t: (len(t), t)), name + ": (length, lexicographic) order, no text twice"
        assert set(b"".join(ts)) == set(alphabet)
    assert sum(len(t) for t in T.text_set("BIN15")) == 917506
    bin15 = T.count_and_bytes(2, 15)
    shapes = {"bin15": bin15, "bin15_wide": (bin15[0] + 1, bin15[1] + 256), "bin15_reversed": (bin15[0] + 1, bin15[1] + 256),
              "bin15_shuffled": (bin15[0] + 1, bin15[1] + 256),
              "neighbours": (2 * 8 * 510 + 1, 8 * T.count_and_bytes(2, 8)[1] + 3 * 8 * 510 + 256),
              "mixed": tuple(sum(x) for x in zip(T.count_and_bytes(3, 8), T.count_and_bytes(2, 10), T.count_and_bytes(2, 10)))}
    assert set(shapes) == set(T.PACK_NAMES) == set(FIRST_KEY)
    for name, (count, total) in shapes.items():
        blocks = T.pack(name).blocks
        assert (len(blocks), sum(len(b) for b in blocks)) == (count, total), name
        assert count <= DK_PACKED_MAX_BLOCKS and total <= 1 << 20, name
    assert shapes["bin15"][0] == DK_PACKED_MAX_BLOCKS - 2 and shapes["neighbours"][0] == 8161
    wide = T.pack("bin15_wide").blocks
    assert sorted(T.pack("bin15_reversed").blocks) == sorted(T.pack("bin15_shuffled").blocks) == sorted(wide)
    assert T.pack("bin15_reversed").blocks == wide[::-1] and T.pack("bin15_shuffled").blocks not in (wide, wide[::-1])
    # neighbours: every u of 1 .. 8 bytes directly in front of every v of 3 bytes
    nb = T.pack("neighbours").blocks
    assert {(nb[i], nb[i + 1]) for i in range(0, len(nb) - 1, 2)} == {(u, v) for u in T.text_set("BIN8") for v in T.texts((T.A, T.B), 3, 3)}


# ---- 2. the models against the oracle and the other models -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["BIN12", "TER8", "EXT10"])
def test_models_against_the_oracle(orc, name):
    for t in T.text_set(name):
        s, L, origin, lc = T.answers(t)
        assert s == orc.sa_naive(t).tolist(), ("sa", t)
        oL, oorigin = orc.bwt_forward(t, np.array(s, np.uint32))
        assert (L, origin) == (oL.tobytes(), oorigin), ("bwt", t)
        assert orc.bwt_inverse(np.frombuffer(L, np.uint8), origin).tobytes() == t, ("the oracle's inverse of the model's (L, origin)", t)
        assert lc == lcp_kasai(t, s).tolist(), ("lcp", t)


# ---- 3. (L, origin) pairs ----------------------------------------------------------------------------------------------------------------------

PAIR_SETS = [((T.A, T.B), 9), ((T.A, T.B, T.C), 5)]


def pairs_of(alphabet, m):
    """every L of m bytes over the alphabet with every origin"""
    return [(bytes(p), o) for p in itertools.product(sorted(alphabet), repeat=m) for o in range(m)]


def forward_transforms(alphabet, m):
    return {T.answers(t)[1:3]: t for t in T.texts(alphabet, m, m)}


@pytest.mark.parametrize("alphabet,top", PAIR_SETS, ids=["ab9", "abc5"])
def test_pairs_that_are_a_text(alphabet, top):
    """of the m sigma^m pairs of length m exactly sigma^m are a text, they are exactly the forward transforms, and the model inverts each to
    the text it is the transform of: "valid" and "is a BWT" coincide"""
    sigma = len(alphabet)
    for m in range(1, top + 1):
        fwd = forward_transforms(alphabet, m)
        assert len(fwd) == sigma ** m, "two texts of %d bytes with one transform" % m
        pairs = pairs_of(alphabet, m)
        assert len(pairs) == m * sigma ** m
        accepted = {}
        for L, o in pairs:
            v = ibwt_model.invert(np.frombuffer(L, np.uint8), o)
            if v.text is not None:
                accepted[(L, o)] = v.text.tobytes()
        assert len(accepted) == sigma ** m, "m = %d: the model accepts %d pairs" % (m, len(accepted))
        assert accepted == fwd, "m = %d: the accepted pairs are not the forward transforms, or invert to another text" % m


# ---- 4. every fault decides --------------------------------------------------------------------------------------------------------------------

def differs(true, faulty):
    return [k for k in ("sa", "L", "origin", "lcp") if not np.array_equal(getattr(true, k), getattr(faulty, k))]


@pytest.mark.parametrize("fault", list(T.FAULTS))
def test_every_fault_decides(true_arrays, fault):
    """the fault model's arrays for `neighbours`, and for one of the bin15 packs at least, are not the true ones"""
    changed = differs(true_arrays("neighbours"), T.expected(T.pack("neighbours").blocks, fault))
    assert changed, "pack neighbours does not see the fault %s" % fault
    assert ("origin" in changed) if fault.startswith("origin") else ("sa" in changed), changed
    assert any(differs(true_arrays(name), T.expected(T.pack(name).blocks, fault)) for name in T.PACK_NAMES if name.startswith("bin15")), \
        "no bin15 pack sees the fault %s" % fault


def test_reads_next_block_is_seen_for_every_continuation(true_arrays):
    """what `neighbours` is for.  The order of two suffixes x and x y of u can change only where y v sorts before v.  No y does that to
    v = aaa; for every other v, y = a does (u = aa), so seven of the eight continuations change some u.  A u can change only if its last byte
    occurs in it before (some suffix is a proper prefix of another)"""
    blocks = T.pack("neighbours").blocks
    true, faulty = true_arrays("neighbours"), T.expected(blocks, "reads_next_block")
    hit_v, hit_u = set(), set()
    for i in range(0, len(blocks) - 1, 2):
        a, b = int(true.off[i]), int(true.off[i + 1])
        if not np.array_equal(true.sa[a:b], faulty.sa[a:b]):
            hit_v.add(blocks[i + 1])
            hit_u.add(blocks[i])
    assert hit_v == set(T.texts((T.A, T.B), 3, 3)) - {b"aaa"}
    assert b"aa" in hit_u
    can_change = {u for u in T.text_set("BIN8") if u[-1] in u[:-1]}
    assert hit_u <= can_change


# ---- 5. first-key arithmetic -------------------------------------------------------------------------------------------------------------------

def test_first_key_expressions_are_the_sources():
    with open(os.path.join(ROOT, "dark_amd", "csrc", "packed.hip")) as f:
        src = f.read()
    for line in ("f->bits = static_cast<int>(std::max(1u, ceil_log2_u64(static_cast<uint64_t>(f->sigma) + 1)));",
                 "f->blk_bits = static_cast<int>(ceil_log2_u64(s.cnt));",
                 "const int k = std::max(1, (64 - f->blk_bits) / f->bits);",
                 "f->k_used = static_cast<int>(std::min<uint64_t>(k, std::max<uint64_t>(1, total)));",
                 "uint64_t h = static_cast<uint64_t>(f.k_used);",
                 "h *= 2;"):
        assert line in src, line
    assert [ceil_log2(v) for v in (1, 2, 3, 4, 5, 8161, 8192, 8193, 65534, 65535, 65536, 65537)] == [0, 1, 2, 2, 3, 13, 13, 14, 16, 16, 16, 17]


@pytest.mark.parametrize("name", T.PACK_NAMES)
def test_first_key_and_rounds(true_arrays, name):
    blk_bits, bits, k, rounds = FIRST_KEY[name]
    blocks = T.pack(name).blocks
    assert first_key(blocks) == (blk_bits, bits, k), name
    longest = int(true_arrays(name).lcp.max())
    assert longest == {"neighbours": 7, "mixed": 9}.get(name, 14)  # a^n shares n - 1 with its next suffix
    assert rounds_needed(k, longest) == rounds, name


def test_round_counts_the_issue_states():
    assert [FIRST_KEY[name][3] for name in ("bin15", "bin15_wide", "bin15_reversed", "bin15_shuffled", "neighbours")] == [0, 2, 2, 2, 1]
    assert [rounds_needed(5, x) for x in (4, 5, 9, 10, 19, 20)] == [0, 1, 1, 2, 2, 3]
