"""A plain model of the FM-index's seams (csrc/fm_index.hip k_fm_seam_*), the yardstick of tests/test_gpu_fm_seams.py.
tests/test_fm_seams_model.py pins it on hand-worked cases and against a plain overlapping bytes.find count.

`prev` (piece -1) and the blocks 0 .. count - 1 are the consecutive pieces of one text.  Every occurrence of every pattern in that text is
enumerated by brute force; a SEAM HIT is one whose first and last byte lie in different pieces.  It belongs to the block of its last byte, and
`back` is the number of its bytes in front of that block's first byte.  The hits are ordered by (pattern, block, start): inside a pair that is
back descending."""
import numpy as np

SEAM_DTYPE = np.dtype([("pattern", np.uint32), ("block", np.uint32), ("back", np.uint32), ("reserved", np.uint32)])


def _b(x):
    return x if isinstance(x, bytes) else bytes(bytearray(np.asarray(x, dtype=np.uint8).tolist()))


def found(t, p):
    """every position of p in t, overlapping ones included, by bytes.find"""
    out, i = [], t.find(p)
    while i >= 0 and i < len(t):
        out.append(i)
        i = t.find(p, i + 1)
    return out


def seam_starts(blocks, patterns, prev=b""):
    """-> a list of (pattern, block of the last byte, start in prev + text, start of that block in prev + text), ordered by (pattern, block, start)"""
    blocks, patterns, prev = [_b(t) for t in blocks], [_b(p) for p in patterns], _b(prev)
    whole = prev + b"".join(blocks)
    piece = [-1] * len(prev)  # the piece of every byte
    first = []                # where every block starts in `whole`
    for b, t in enumerate(blocks):
        first.append(len(piece))
        piece += [b] * len(t)
    out = []
    for q, p in enumerate(patterns):
        m = len(p)
        if m < 2:
            continue
        for i in range(len(whole) - m + 1):
            if whole[i:i + m] == p and piece[i] != piece[i + m - 1]:
                b = piece[i + m - 1]
                out.append((q, b, i, first[b]))
    return sorted(out)


def seam_starts_fast(blocks, patterns, prev=b""):
    """seam_starts for long texts: the occurrences by bytes.find, their pieces by bisection (tests/test_fm_seams_model.py pins it to seam_starts)"""
    import bisect
    blocks, patterns, prev = [_b(t) for t in blocks], [_b(p) for p in patterns], _b(prev)
    whole = prev + b"".join(blocks)
    first = [len(prev)]
    for t in blocks[:-1]:
        first.append(first[-1] + len(t))
    out = []
    for q, p in enumerate(patterns):
        m = len(p)
        if m < 2:
            continue
        for i in found(whole, p):
            a, b = bisect.bisect_right(first, i) - 1, bisect.bisect_right(first, i + m - 1) - 1  # (-1: prev)
            if a != b:
                out.append((q, b, i, first[b]))
    return sorted(out)


def seams_model(blocks, patterns, prev=b"", fast=False):
    """-> (occ: npat x count uint32, records: SEAM_DTYPE array of ALL seam hits in order, total).  fast: through seam_starts_fast"""
    occ = np.zeros((len(patterns), len(blocks)), dtype=np.uint32)
    flat = []
    for q, b, start, first in (seam_starts_fast if fast else seam_starts)(blocks, patterns, prev):
        occ[q, b] += 1
        flat.append((q, b, first - start, 0))
    return occ, np.array(flat, dtype=SEAM_DTYPE) if flat else np.zeros(0, SEAM_DTYPE), len(flat)
