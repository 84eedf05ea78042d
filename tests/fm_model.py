"""Plain models of the backward search of csrc/fm_index.hip, the yardsticks of tests/test_gpu_fm.py.
tests/test_fm_model.py pins them against search_model and occurrences of tests/sa_query_model.py.

Conventions: L[i] = T[SA[i] - 1], and T[n - 1] at the slot `origin` where SA[origin] = 0; no sentinel, a proper prefix sorts first.
  hist[c] = occurrences of c in L, C[c] = sum of hist below c, last = L[origin], Occ(c, i) = #{k < i : L[k] = c},
  Occ'(c, i) = Occ(c, i) - [c == last and origin < i]
  first step (c = P[m-1]):  lo = C[c], hi = C[c] + hist[c];   later steps (c = P[j]):  x <- C[c] + [c == last] + Occ'(c, x)  for x = lo, hi
The recurrence is defined for any bytes L and any origin < n, a BWT or not.

fm_model_plain is the recurrence word for word (for small inputs); fm_model is the same numbers with every pattern stepped at once and
C[c] + Occ(c, i) read off the stable sort of L by one searchsorted, so that thousands of long patterns take a second."""
import numpy as np


def _u8(x):
    return np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8)


def bwt_plain(text):
    """-> (L, origin) of a text, from its sorted suffixes"""
    t = bytes(_u8(text))
    n = len(t)
    sa = sorted(range(n), key=lambda i: t[i:])
    return np.array([t[i - 1] for i in sa], dtype=np.uint8), sa.index(0)


def fm_model_plain(L, origin, patterns):
    L = _u8(L)
    n = len(L)
    assert 0 <= origin < n
    last = int(L[origin])
    hist = np.bincount(L, minlength=256)
    cum = np.concatenate([[0], np.cumsum(hist)])

    def occ1(c, i):  # Occ'(c, i)
        return int((L[:i] == c).sum()) - (1 if c == last and origin < i else 0)

    out = []
    for p in patterns:
        p = _u8(p)
        m = len(p)
        lo, hi = 0, n
        for j in range(m - 1, -1, -1):
            c = int(p[j])
            if j == m - 1:
                lo, hi = int(cum[c]), int(cum[c] + hist[c])
            else:
                lo = int(cum[c]) + (c == last) + occ1(c, lo)
                hi = int(cum[c]) + (c == last) + occ1(c, hi)
        out.append((lo, hi))
    return out


def fm_model(L, origin, patterns):
    L = _u8(L)
    n = len(L)
    assert 0 <= origin < n
    last = int(L[origin])
    order = np.argsort(L, kind="stable").astype(np.int64)
    keys = L[order].astype(np.int64) * (n + 1) + order  # sorted: searchsorted(keys, c (n + 1) + i) = C[c] + Occ(c, i)
    keep = [_u8(p) for p in patterns]
    npat = len(keep)
    lens = np.array([len(p) for p in keep], dtype=np.int64)
    flat = np.concatenate(keep + [np.zeros(1, np.uint8)]).astype(np.int64)
    ends = np.cumsum(lens)  # pattern q ends at flat[ends[q] - 1]
    lo, hi = np.zeros(npat, np.int64), np.full(npat, n, np.int64)
    for t in range(int(lens.max()) if npat else 0):
        act = np.flatnonzero(lens > t)
        c = flat[ends[act] - 1 - t]
        if t == 0:
            lo[act] = np.searchsorted(keys, c * (n + 1))
            hi[act] = np.searchsorted(keys, c * (n + 1) + n)
        else:
            is_last = (c == last).astype(np.int64)
            for x in (lo, hi):
                x[act] = np.searchsorted(keys, c * (n + 1) + x[act]) + is_last - (is_last & (origin < x[act]))
    return list(zip(lo.tolist(), hi.tolist()))


def fm_model_packed(Ls, origins, patterns, blocks):
    """pattern q in block blocks[q]; results local to the block"""
    out = [None] * len(patterns)
    for b in sorted(set(int(x) for x in blocks)):
        qs = [q for q in range(len(patterns)) if int(blocks[q]) == b]
        for q, r in zip(qs, fm_model(Ls[b], origins[b], [patterns[q] for q in qs])):
            out[q] = r
    return out


def rank_model(L, symbols):
    """-> {c: Occ(c, i) for i = 0 .. n} as arrays of n + 1 entries"""
    L = _u8(L)
    return {int(c): np.concatenate([[0], np.cumsum(L == c)]).astype(np.int64) for c in symbols}
