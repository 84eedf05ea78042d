"""tests/fm_seams_model.py on hand-worked cases, and the invariant of DESIGN.md section 4.17: for any cutting of a text into blocks and packs, the
occurrences inside the blocks and the seam hits (prev = what stands in front of the pack) are together every occurrence, each once."""
import itertools

import numpy as np

from fm_seams_model import SEAM_DTYPE, found, seam_starts, seam_starts_fast, seams_model


def words(alphabet, lengths):
    return [bytes(w) for m in lengths for w in itertools.product(alphabet, repeat=m)]


def test_ab_ab():
    occ, recs, total = seams_model([b"ab", b"ab"], [b"ab", b"ba", b"bab"])
    assert occ.dtype == np.uint32 and recs.dtype == SEAM_DTYPE and recs.dtype.itemsize == 16
    # "ab" stands inside the blocks only; "ba" = the last byte of block 0 and the first of block 1; "bab" starts one byte back, ends at byte 1
    assert occ.tolist() == [[0, 0], [0, 1], [0, 1]] and total == 2
    assert recs.tolist() == [(1, 1, 1, 0), (2, 1, 1, 0)]


def test_five_one_byte_blocks():
    blocks = [b"a", b"b", b"a", b"b", b"a"]
    occ, recs, total = seams_model(blocks, [b"ab", b"aba", b"ababa", b"a", b"", b"bb"])
    # every occurrence of two bytes or more is a seam hit and belongs to the block of its last byte
    assert occ.tolist() == [[0, 1, 0, 1, 0], [0, 0, 1, 0, 1], [0, 0, 0, 0, 1], [0] * 5, [0] * 5, [0] * 5] and total == 5
    assert recs.tolist() == [(0, 1, 1, 0), (0, 3, 1, 0), (1, 2, 2, 0), (1, 4, 2, 0), (2, 4, 4, 0)]


def test_prev_only():
    # one block: the only border is the one against prev
    occ, recs, total = seams_model([b"cab"], [b"ab", b"abc", b"bca", b"abcab", b"ca"], prev=b"abab")
    assert occ.tolist() == [[0], [1], [1], [1], [0]] and total == 3  # "ab" in prev and "ab" in the block are no seam hits
    assert recs.tolist() == [(1, 0, 2, 0), (2, 0, 1, 0), (3, 0, 2, 0)]
    # without prev a single block has no seam
    assert seams_model([b"cab"], [b"ab", b"ca"])[2] == 0


def test_a_to_the_n():
    # a^3 | a^2 | a^4, pattern a^m: at block b the candidates back = 1 .. m - 1 with m - back <= n_b and back <= the bytes in front
    blocks = [b"aaa", b"aa", b"aaaa"]
    occ, recs, total = seams_model(blocks, [b"a" * m for m in (2, 3, 4, 5, 9, 10)])
    assert occ.tolist() == [[0, 1, 1], [0, 2, 2], [0, 2, 3], [0, 1, 4], [0, 0, 1], [0, 0, 0]]
    # a^5 at block 1 (two bytes, three in front): back <= 3 and 5 - back <= 2 leave back = 3 alone
    assert recs[recs["pattern"] == 3].tolist() == [(3, 1, 3, 0), (3, 2, 4, 0), (3, 2, 3, 0), (3, 2, 2, 0), (3, 2, 1, 0)]
    # with prev = a^2 the first block has a border too, and a^9 reaches back over three of them
    occ, recs, total = seams_model(blocks, [b"a" * 9], prev=b"aa")
    assert occ.tolist() == [[0, 0, 3]] and recs["back"].tolist() == [7, 6, 5]


def test_order_and_ranges():
    blocks = words(b"ab", range(1, 5))
    pats = words(b"ab", range(0, 5))
    occ, recs, total = seams_model(blocks, pats, prev=b"abba")
    assert total == len(recs) == int(occ.sum()) > 0 and not recs["reserved"].any()
    keys = [(int(r["pattern"]), int(r["block"]), -int(r["back"])) for r in recs]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    plen = np.array([len(p) for p in pats])[recs["pattern"]]
    assert (recs["back"] >= 1).all() and (recs["back"] < plen).all()
    assert not occ[:, 0][np.array([len(p) for p in pats]) > 4].any()
    for front in (b"", b"a", b"abba"):
        assert seam_starts_fast(blocks, pats, front) == seam_starts(blocks, pats, front)
    assert seam_starts_fast([b"a"] * 9, [b"aaa", b"a" * 9, b"a" * 10], b"aa") == seam_starts([b"a"] * 9, [b"aaa", b"a" * 9, b"a" * 10], b"aa")


def test_the_invariant():
    """a text cut into blocks, the blocks cut into packs: per pattern, in-block occurrences + seam hits with prev = the text in front of the
    pack = the overlapping bytes.find count of the whole text, and the starts are the same set"""
    rng = np.random.default_rng(23)
    for trial in range(60):
        n = int(rng.integers(1, 60))
        text = bytes(rng.integers(97, 99 + trial % 2, size=n, dtype=np.uint8))
        cuts = sorted(set(rng.integers(1, n, size=int(rng.integers(0, 12))).tolist())) if n > 1 else []
        blocks = [text[a:b] for a, b in zip([0] + cuts, cuts + [n])]
        assert b"".join(blocks) == text and all(blocks)
        per_pack = int(rng.integers(1, 5))
        packs = [blocks[i:i + per_pack] for i in range(0, len(blocks), per_pack)]
        pats = [text[a:a + m] for a in range(0, n, 3) for m in (1, 2, 3, 7)] + [b"ab", b"aa", b"", b"ba" * 3]
        for q, p in enumerate(pats):
            if not p:
                continue
            starts, done = [], 0
            for pack in packs:
                for t in pack:
                    starts += [done + i for i in found(t, p)]
                    done += len(t)
                front = done - sum(len(t) for t in pack)
                keep = int(rng.integers(max(len(p) - 1, 0), len(p) + 4))  # at least the last m - 1 bytes: more of them change nothing
                prev = text[max(front - keep, 0):front]
                starts += [front - len(prev) + s for _, _, s, _ in seam_starts(pack, [p], prev)]
            assert sorted(starts) == found(text, p), (text, blocks, per_pack, p)
