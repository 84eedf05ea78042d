"""Plain models of the suffix-array check and search (csrc/sa_query.hip), the yardsticks of tests/test_gpu_sa_check.py
and tests/test_gpu_sa_search.py.  tests/test_sa_query_model.py pins both against the definitions.

Order: no sentinel, a suffix that is a proper prefix of another sorts first (src/saca.rs:105-113) -- Python's order of bytes objects.

check_model is the three conditions of Burkhardt and Kärkkäinen exactly as the kernels evaluate them, in numpy so that 2^20 entries take
milliseconds; search_model is bisect over the suffixes cut to the pattern's length."""
import bisect

import numpy as np

OK, BAD_RANGE, NOT_PERMUTATION, BAD_ORDER = "ok", "bad_range", "not_permutation", "bad_order"
NONE = -1


def _u8(x):
    return np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8)


def check_model(text, sa):
    """-> (verdict, where): the first of the three kinds that fails, and the lowest slot (NOT_PERMUTATION: text position) at which it does;
    (OK, n) for the suffix array of the text"""
    t = _u8(text)
    sa = np.asarray(sa, dtype=np.int64)
    n = len(t)
    assert len(sa) == n and n > 0
    # (a) every entry below n; isa[SA[i]] = i over an array preset to NONE (where two slots name one position either value may stay)
    bad = np.flatnonzero(sa >= n)
    if bad.size:
        return BAD_RANGE, int(bad[0])
    isa = np.full(n, NONE, np.int64)
    isa[sa] = np.arange(n)
    # (b) n entries in range over n positions hit all of them exactly when they are a permutation
    missing = np.flatnonzero(isa == NONE)
    if missing.size:
        return NOT_PERMUTATION, int(missing[0])
    # (c) slot i >= 1, a = SA[i-1], b = SA[i]
    a, b = sa[:-1], sa[1:]
    ta, tb = t[a], t[b]
    nxt_a, nxt_b = isa[np.minimum(a + 1, n - 1)], isa[np.minimum(b + 1, n - 1)]
    in_order = np.where(ta != tb, ta < tb,                      # the first bytes decide
                        np.where(a + 1 == n, True,              # equal bytes and a is the last position: the empty suffix is the smallest
                                 np.where(b + 1 == n, False,    # ... and b is: the pair is the wrong way round
                                          nxt_a < nxt_b)))      # otherwise the suffixes behind the first bytes decide, by their slots
    bad = np.flatnonzero(~in_order)
    if bad.size:
        return BAD_ORDER, int(bad[0]) + 1
    return OK, n


def check_model_packed(blocks, sas):
    return [check_model(b, s) for b, s in zip(blocks, sas)]


class _Cut:
    """the suffixes in suffix-array order, each cut to m bytes, made when bisect asks for one"""

    def __init__(self, t, sa, m):
        self.t, self.sa, self.m = t, sa, m

    def __len__(self):
        return len(self.sa)

    def __getitem__(self, i):
        v = self.sa[i]
        return self.t[v:v + self.m]


def search_model(text, sa, patterns):
    """-> (lo, hi) per pattern for a VALID suffix array: slots whose suffix, cut to len(P) bytes, is smaller than / not greater than P.  The cut
    suffixes are sorted because the suffixes are."""
    t = bytes(_u8(text))
    sa = [int(v) for v in sa]
    out = []
    for p in patterns:
        p = bytes(_u8(p))
        cut = _Cut(t, sa, len(p))
        out.append((bisect.bisect_left(cut, p), bisect.bisect_right(cut, p)))
    return out


def occurrences(text, pattern):
    """definition: every place the pattern starts (the empty pattern: every position)"""
    t, p = bytes(_u8(text)), bytes(_u8(pattern))
    return sorted(i for i in range(len(t)) if t[i:i + len(p)] == p)


def suffix_array_plain(text):
    t = bytes(_u8(text))
    return np.array(sorted(range(len(t)), key=lambda i: t[i:]), dtype=np.uint32)
