"""TEST HELPER: plain numpy model of the period kernels and the text probes of the suffix sort -- what dk_dbg_dev_period runs: k_period_first / _spine /
_fill, k_run_probe, k_period_probe, k_period_count, k_period_search, k_prefix_probe of csrc/suffix_array.hip -- written from the definitions below and
not from the kernels.  tests/test_period_model.py pins every function against a brute-force loop.  Integers only, no tolerance anywhere.

  next breaks    nb[i] = min { j >= i : j + p >= n or T[j] != T[j + p] }  (the last position is always a break, so every i has one)
  run probe      over the whole 256-byte windows [256 w, 256 w + 256) with 256 w + 256 <= n: [0] = 1 if one of them holds one byte value only, else 0;
                 [1] = their 16-byte pieces (sixteen per window, at multiples of 16) that hold one byte value only.  A text whose first byte is
                 not 16-byte aligned: both zero
  period probe   [p - 1] for p = 1 .. 8 = the windows w with 64 w + 72 <= n and T[64 w + k] == T[64 w + k + p] for all k < 64.  A text whose first
                 byte is not 8-byte aligned: all zero
  period count   the windows w with 64 w + 64 + p <= n and T[64 w + k] == T[64 w + k + p] for all k < 64, any alignment
  period search  for each of the 32 samples b: x = (2 b + 1) n // 64; the smallest p in [9, pmax] with T[x + k] == T[x + p + k] for all k < 48;
                 NONE if there is none or x + pmax + 48 > n
  prefix probe   sample i < m stands at i * span + hash(i) % span, hash(i) = v ^ (v >> 15) with v = i * 2654435761 mod 2^32, and counts if that is
                 below n; its prefix of L symbols is the codes (round_model.alphabet) of T[pos .. pos + L), zero behind the text's end;
                 dups[c] = the samples that count minus their distinct prefixes of lengths[c] symbols (zero from len(lengths) on)"""
import numpy as np

from round_model import alphabet

NONE = 0xFFFFFFFF
SAMPLES = 32
PB_TILE = 4096     # positions per workgroup of k_period_first / _fill
SPINE = 1024       # chunks of tiles of the one-workgroup k_period_spine: above SPINE tiles a chunk holds more than one


def breaks(text, p):
    """break[j] = j + p >= n or T[j] != T[j + p]"""
    n = len(text)
    brk = np.ones(n, bool)
    if p < n:
        brk[:n - p] = text[:n - p] != text[p:]
    return brk


def next_break(text, p):
    text = np.asarray(text, dtype=np.uint8)
    n = len(text)
    at = np.where(breaks(text, p), np.arange(n, dtype=np.int64), n)
    return np.minimum.accumulate(at[::-1])[::-1].astype(np.uint32)


def follows(text, p, width):
    """f[w] = the window [width w, width w + width) lies with its partner p further on inside the text and equals it"""
    n = len(text)
    windows = (n - p) // width if n >= p else 0
    if windows <= 0:
        return np.zeros(0, bool)
    a = text[:windows * width].reshape(windows, width)
    b = text[p:p + windows * width].reshape(windows, width)
    return (a == b).all(axis=1)


def run_probe(text, offset=0):
    text = np.asarray(text, dtype=np.uint8)
    if offset % 16:
        return np.zeros(2, np.uint32)
    windows = len(text) // 256
    pieces = text[:windows * 256].reshape(windows * 16, 16)
    one = (pieces == pieces[:, :1]).all(axis=1)
    whole = text[:windows * 256].reshape(windows, 256)
    return np.array([int((whole == whole[:, :1]).all(axis=1).any()) if windows else 0, int(one.sum())], np.uint32)


def period_probe(text, offset=0):
    text = np.asarray(text, dtype=np.uint8)
    out = np.zeros(8, np.uint32)
    if offset % 8 or len(text) < 72:
        return out
    windows = (len(text) - 72) // 64 + 1
    for p in range(1, 9):
        out[p - 1] = int(follows(text, p, 64)[:windows].sum())
    return out


def period_count(text, p):
    return int(follows(np.asarray(text, dtype=np.uint8), p, 64).sum())


def period_search(text, pmax):
    text = np.asarray(text, dtype=np.uint8)
    n = len(text)
    found = np.full(SAMPLES, NONE, np.uint32)
    for b in range(SAMPLES):
        x = (2 * b + 1) * n // (2 * SAMPLES)
        if x + pmax + 48 > n:
            continue
        eq = np.ones(pmax - 8, bool)  # for p = 9 .. pmax
        for k in range(48):
            eq &= text[x + 9 + k:x + pmax + 1 + k] == text[x + k]
        hit = np.flatnonzero(eq)
        if len(hit):
            found[b] = 9 + hit[0]
    return found


def sample_positions(m, span):
    i = np.arange(m, dtype=np.uint64)
    v = (i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(15)
    return (i * np.uint64(span) + v % np.uint64(span)).astype(np.int64)


def prefix_probe(text, m, span, lengths):
    text = np.asarray(text, dtype=np.uint8)
    n = len(text)
    code, _, _ = alphabet(text)
    pos = sample_positions(m, span)
    pos = pos[pos < n]
    longest = max(lengths)
    coded = np.concatenate([code[text], np.zeros(longest, np.uint8)])
    rows = coded[pos[:, None] + np.arange(longest)[None, :]]
    dups = np.zeros(4, np.uint32)
    for c, length in enumerate(lengths):
        dups[c] = len(pos) - len(np.unique(rows[:, :length], axis=0))
    return dups
