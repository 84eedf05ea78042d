"""TEST HELPER: plain model of the L-first path's refinement from a caller's list -- what dk_dbg_dev_lf_refine (lfirst_path of csrc/lfirst.inc in
its take-over form) leaves in L -- written from the rule below and from nothing in the kernels.  tests/test_lf_refine_model.py pins it on the CPU.

The list: slot a holds the suffix idx[a], its place pos[a] in L, its group gid[a] (a group is a run of equal words) and the symbol sym[a] in front
of the suffix.  The members of a group are equal in their first h0 symbols by construction; the model does not care.

The rule.  For every group: order the members by their suffixes -- plain byte comparison, a proper prefix is smaller -- and take the group's
places pos[a] in LIST order.  Then L[k-th place] = sym of the k-th smallest member, and origin = the place of suffix 0 if it is listed.  Groups of
one member and groups with one symbol in front (finals of the path's first filter) follow the same rule: their result does not depend on the
order.  Every other byte of L and the origin word stay as they were.

sym is a free label: no kernel of the path derives it from the text, so a test may give every member a random one and make every misordering
between two members of a group show in L."""
from functools import cmp_to_key

import numpy as np


def suffix_cmp(t, i, j):
    """-1 / 0 / 1: the suffixes of bytes t at i and j, compared in growing chunks (bytes compare as the rule says: a proper prefix is smaller)"""
    k = 64
    while i != j:
        a, b = t[i:i + k], t[j:j + k]
        if a != b:
            return -1 if a < b else 1
        i, j, k = i + k, j + k, 2 * k  # (equal chunks are full ones: two suffixes of different lengths differ by then)
    return 0


def groups_of(gid):
    """-> (start, end) of every run of equal words"""
    gid = np.asarray(gid)
    heads = np.flatnonzero(np.concatenate([[True], gid[1:] != gid[:-1]]))
    return list(zip(heads.tolist(), np.append(heads[1:], len(gid)).tolist()))


def lf_refine_model(text, idx, pos, gid, sym, bwt_before, origin_before):
    """-> (L, origin) after the call"""
    t = bytes(np.ascontiguousarray(text, dtype=np.uint8))
    idx, pos, sym = (np.asarray(x) for x in (idx, pos, sym))
    L = np.array(bwt_before, dtype=np.uint8, copy=True)
    origin = origin_before
    key = cmp_to_key(lambda a, b: suffix_cmp(t, int(idx[a]), int(idx[b])))
    for s, e in groups_of(gid):
        order = sorted(range(s, e), key=key)
        L[pos[s:e]] = sym[order]
        for k, a in enumerate(order):
            if idx[a] == 0:
                origin = int(pos[s + k])
    return L, origin
