"""Plain models of the FM-index's locate (csrc/bwt.hip k_pib_locate, csrc/fm_index.hip k_fm_locate), the yardsticks of
tests/test_gpu_fm_locate.py.  tests/test_fm_locate_model.py pins them against sorted suffixes.

Conventions of tests/fm_model.py: L[i] = T[SA[i] - 1], T[n - 1] at the slot `origin` where SA[origin] = 0; no sentinel.  For a slot x != origin
with c = L[x]:
  LF(x) = C[c] + [c == last] - [c == last and origin < x] + Occ(c, x),   and   SA[LF(x)] = SA[x] - 1
-- the count's later step applied to a slot.  A slot is MARKED when SA[x] % step == 0 (position 0 always is, so no walk steps from the origin);
to locate x, LF steps are taken until a marked slot y is met after k of them: SA[x] = sample(y) + k, and k <= min(step, n) - 1."""
import numpy as np

NO_HIT = 0xFFFFFFFF


def _u8(x):
    return np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8)


def sa_plain(text):
    """the suffix array from sorted suffixes (a proper prefix sorts first)"""
    t = bytes(_u8(text))
    return sorted(range(len(t)), key=lambda i: t[i:])


def lf(L, origin, x):
    """LF(x) by the formula, word for word"""
    L = _u8(L)
    c, last = int(L[x]), int(L[origin])
    below = int((L < c).sum())
    occ = int((L[:x] == c).sum())
    return below + (1 if c == last else 0) - (1 if c == last and origin < x else 0) + occ


def locate_structure(L, origin, sa, step):
    """-> (marked: bool per slot, samples: SA[x] // step of the marked slots in slot order).  From the suffix array: what the build must equal."""
    sa = np.asarray(sa, dtype=np.int64)
    marked = sa % step == 0
    return marked, (sa[marked] // step)


def locate_slot(L, origin, marked, samples, step, x):
    """-> (SA[x], LF steps taken) by the sampled walk"""
    n = len(L)
    rank = np.concatenate([[0], np.cumsum(marked)])
    k = 0
    while not marked[x]:
        assert x != origin and k < min(step, n), "the walk left its bound"
        x = lf(L, origin, x)
        k += 1
    return int(samples[rank[x]]) * step + k, k


def locate_rows(sa, ranges, max_hits):
    """rows of dk_dev_fm_locate for (lo, hi) ranges: SA[lo + j] for j < min(hi - lo, max_hits), NO_HIT behind"""
    sa = np.asarray(sa, dtype=np.int64)
    out = np.full((len(ranges), max_hits), NO_HIT, dtype=np.int64)
    for q, (lo, hi) in enumerate(ranges):
        k = max(0, min(hi - lo, max_hits))
        out[q, :k] = sa[lo:lo + k]
    return out
