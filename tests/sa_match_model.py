"""Plain models of the matching statistics and the super-maximal matches (csrc/sa_query.hip), the yardsticks of
tests/test_gpu_sa_match.py.  tests/test_sa_match_model.py pins both against the definitions by brute force.

match_model: a lower-bound bisect of the window over the cut suffixes ends between the two suffixes that share the most with the window, so the
longest prefix that occurs is the larger of the two common prefixes; its range is search_model's.  smems_model is the three conditions of
include/dark_amd.h, literally."""
import bisect

from sa_query_model import _Cut, _u8


def common_prefix(a, b):
    lo, hi = 0, min(len(a), len(b))  # a[:lo] == b[:lo] always; bisect over the length (slices compare at memcmp speed)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if a[:mid] == b[:mid]:
            lo = mid
        else:
            hi = mid - 1
    return lo


def match_model(text, sa, queries, max_len):
    """-> per query a list of (len, lo, hi), one per position, for a VALID suffix array"""
    t = bytes(_u8(text))
    sa = [int(v) for v in sa]
    out = []
    for q in queries:
        q = bytes(_u8(q))
        rows = []
        for i in range(len(q)):
            window = q[i:i + max_len]  # (a slice ends with the query)
            slot = bisect.bisect_left(_Cut(t, sa, len(window)), window)
            ln = 0
            if slot > 0:
                ln = max(ln, common_prefix(window, t[sa[slot - 1]:]))
            if slot < len(sa):
                ln = max(ln, common_prefix(window, t[sa[slot]:]))
            cut = _Cut(t, sa, ln)  # (search_model's two bisects, without its conversion of the array for every position)
            rows.append((ln, bisect.bisect_left(cut, window[:ln]), bisect.bisect_right(cut, window[:ln])))
        out.append(rows)
    return out


def smems_model(lens_per_query, min_len, max_len):
    """lens_per_query: the len column of match_model, one list per query -> [(at, len)] in rising order of at, at = the offset into the queries
    back to back"""
    out, base = [], 0
    for lens in lens_per_query:
        for i, ln in enumerate(lens):
            long_enough = ln >= max(min_len, 1)
            not_contained = i == 0 or lens[i - 1] <= ln
            continues_a_capped_copy = i > 0 and lens[i - 1] == max_len and ln == max_len
            if long_enough and not_contained and not continues_a_capped_copy:
                out.append((base + i, ln))
        base += len(lens)
    return out


def smem_records(text, sa, queries, min_len, max_len):
    """-> [(at, len, lo, hi)]: what dk_dev_sa_smems* lists, uncut"""
    rows = match_model(text, sa, queries, max_len)
    flat = [r for q in rows for r in q]
    return [(at, ln) + flat[at][1:] for at, ln in smems_model([[r[0] for r in q] for q in rows], min_len, max_len)]
