"""A plain model of the LCP array: Kasai's algorithm over the inverse suffix array (Kasai, Lee, Arimura, Arikawa, Park, CPM 2001), the
yardstick of tests/test_gpu_lcp.py.  LCP[0] = 0; LCP[i] = the number of leading bytes the suffixes SA[i-1] and SA[i] share; no sentinel, so a
common prefix ends where the shorter suffix ends.  tests/test_lcp_model.py pins it against brute-force prefix comparison.

The loop is Kasai's, with its one serial dependency (h falls by at most one from a position to the next) kept and the byte-by-byte extension
done in numpy chunks, so that inputs with long repeats (a^n, two identical halves) take milliseconds, not minutes."""
import numpy as np


def _extend(t, a, b, h):
    """the largest h' >= h with t[a:a+h'] == t[b:b+h']"""
    n = len(t)
    room = n - max(a, b)
    step = 64
    while h < room:
        k = min(step, room - h)
        x, y = t[a + h:a + h + k], t[b + h:b + h + k]
        if x.tobytes() == y.tobytes():
            h += k
            step = min(step * 4, 1 << 22)
            continue
        return h + int(np.flatnonzero(x != y)[0])
    return room


def lcp_kasai(text, sa):
    t = np.ascontiguousarray(np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
    sa = np.asarray(sa, dtype=np.int64)
    n = len(t)
    assert len(sa) == n
    rank = np.empty(n, np.int64)
    rank[sa] = np.arange(n)
    lcp = np.zeros(n, np.uint32)
    rank_l, sa_l, t_l = rank.tolist(), sa.tolist(), t.tolist()
    h = 0
    for p in range(n):
        r = rank_l[p]
        if r == 0:
            h = 0
            continue
        q = sa_l[r - 1]
        room = n - max(p, q)
        # the common case in a plain loop, long extensions in chunks
        k = 0
        while h < room and k < 32 and t_l[p + h] == t_l[q + h]:
            h += 1
            k += 1
        if k == 32:
            h = _extend(t, p, q, h)
        lcp[r] = h
        if h > 0:
            h -= 1
    return lcp


def lcp_kasai_packed(blocks, sas):
    """the per-block form: every block on its own"""
    return [lcp_kasai(b, s) for b, s in zip(blocks, sas)]


def lcp_brute(text, sa):
    """definition, byte by byte (tiny inputs only)"""
    t = bytes(text)
    n = len(t)
    out = [0] * n
    for i in range(1, n):
        a, b = t[sa[i - 1]:], t[sa[i]:]
        k = 0
        while k < len(a) and k < len(b) and a[k] == b[k]:
            k += 1
        out[i] = k
    return np.array(out, np.uint32)
