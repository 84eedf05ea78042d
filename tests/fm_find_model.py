"""A plain model of the FM-index's find (csrc/fm_index.hip k_fm_find_*), the yardstick of tests/test_gpu_fm_find.py.
tests/test_fm_find_model.py pins it against enumeration with bytes.find and against tests/fm_model.py.

Every pattern q in every block b: the occurrences by brute force (the pattern compared at every position), ordered by the block's sorted
suffixes.  occ[q][b] = their number, total = the sum, and the hits in ascending order of (q, b, j) are the records
(q, b, position of the j-th occurrence in suffix order, lo + j) with [lo, hi) the range tests/fm_model.py gives for q in b."""
import numpy as np

from fm_locate_model import sa_plain
from fm_model import fm_model

HIT_DTYPE = np.dtype([("pattern", np.uint32), ("block", np.uint32), ("position", np.uint32), ("slot", np.uint32)])


def _b(x):
    return x if isinstance(x, bytes) else bytes(bytearray(np.asarray(x, dtype=np.uint8).tolist()))


def block_structures(text):
    """-> (suffix array, L, origin) of one block from its sorted suffixes"""
    t = _b(text)
    sa = sa_plain(t)
    return sa, np.array([t[i - 1] for i in sa], dtype=np.uint8), sa.index(0)


def find_model(texts, patterns):
    """-> (occ: npat x count uint32, records: HIT_DTYPE array of ALL hits in order, total)"""
    texts, patterns = [_b(t) for t in texts], [_b(p) for p in patterns]
    count, npat = len(texts), len(patterns)
    occ = np.zeros((npat, count), dtype=np.uint32)
    per_pair = {}
    for b, t in enumerate(texts):
        n = len(t)
        sa, L, origin = block_structures(t)
        rank = [0] * n
        for slot, i in enumerate(sa):
            rank[i] = slot
        ranges = fm_model(L, origin, patterns)
        for q, p in enumerate(patterns):
            m = len(p)
            at = sorted((i for i in range(n) if t[i:i + m] == p), key=lambda i: rank[i])  # (the empty pattern stands at every position)
            occ[q, b] = len(at)
            if at:
                per_pair[(q, b)] = [(q, b, i, ranges[q][0] + j) for j, i in enumerate(at)]
    flat = [r for key in sorted(per_pair) for r in per_pair[key]]
    return occ, np.array(flat, dtype=HIT_DTYPE) if flat else np.zeros(0, HIT_DTYPE), int(occ.astype(np.int64).sum())
