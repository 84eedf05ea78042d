"""A plain model of the FM-index's near (csrc/fm_index.hip k_fm_near_*), the yardstick of tests/test_gpu_fm_near.py.
tests/test_fm_near_model.py pins it against an independent enumeration and against tests/fm_find_model.py.

A pattern is a list of byte classes, an m x 32 uint8 array: bit c & 7 of byte c >> 3 of row j is set when byte value c matches position j.
Per (pattern, block) the model computes the Hamming cost at every position by brute force and builds the search tree as the header defines it:
a node is (j, w), w a string of m - j bytes that occurs wholly inside the block with cost <= k against the classes j .. m - 1; the children
of (j, w) are the nodes (j - 1, c w) in ascending order of c.  It walks the tree in preorder, counts the nodes, and lists the hits of the
leaves among the first node_limit nodes, inside a leaf in the order of the block's sorted suffixes."""
import numpy as np

from fm_locate_model import sa_plain

NEAR_HIT_DTYPE = np.dtype([("pattern", np.uint32), ("block", np.uint32), ("position", np.uint32), ("cost", np.uint32)])


def _b(x):
    return x if isinstance(x, bytes) else bytes(bytearray(np.asarray(x, dtype=np.uint8).tolist()))


def exact_classes(pattern):
    """the one-bit classes of a byte string"""
    p = _b(pattern)
    out = np.zeros((len(p), 32), dtype=np.uint8)
    for j, c in enumerate(p):
        out[j, c >> 3] = 1 << (c & 7)
    return out


def class_masks(cls):
    """rows of 32 bytes -> a list of 256-bit integers, bit c = byte value c matches"""
    rows = np.asarray(cls, dtype=np.uint8).reshape(-1, 32)
    return [int.from_bytes(r.tobytes(), "little") for r in rows]


def costs(text, masks):
    """the Hamming cost of the pattern at every position 0 .. n - m (empty where the pattern is longer than the text)"""
    t, m = _b(text), len(masks)
    return [sum(1 for i in range(m) if not (masks[i] >> t[p + i]) & 1) for p in range(len(t) - m + 1)]


def pair_walk(text, masks, k, rank):
    """-> (N, leaves): the number of nodes of the pair's tree and its leaves in preorder as (number of the leaf among the nodes, counted from
    1, cost, positions in suffix order)"""
    t, m, n = _b(text), len(masks), len(_b(text))
    if m == 0:
        return 1, [(1, 0, sorted(range(n), key=lambda p: rank[p]))]
    leaves, count = [], [1]  # the root is node 1

    def visit(j, ends, cost):
        # ends: the positions x at which the node's string w stands, t[x : x + m - j] == w; the children put one byte in front
        by_symbol = {}
        for x in ends:
            if x >= 1:
                by_symbol.setdefault(t[x - 1], []).append(x - 1)
        for c in sorted(by_symbol):
            child_cost = cost + (0 if (masks[j - 1] >> c) & 1 else 1)
            if child_cost > k:
                continue
            count[0] += 1
            if j - 1 == 0:
                leaves.append((count[0], child_cost, sorted(by_symbol[c], key=lambda p: rank[p])))
            else:
                visit(j - 1, by_symbol[c], child_cost)

    visit(m, list(range(1, n + 1)), 0)  # the empty string stands behind every byte
    return count[0], leaves


def near_model(texts, classes, k, node_limit=None):
    """-> (occ: npat x count uint32, records: NEAR_HIT_DTYPE array of ALL listed hits in order, total, cut, nodes: npat x count int64 = N of
    every pair).  node_limit None: no limit."""
    texts = [_b(t) for t in texts]
    all_masks = [class_masks(c) for c in classes]
    count, npat = len(texts), len(all_masks)
    occ = np.zeros((npat, count), dtype=np.uint32)
    nodes = np.zeros((npat, count), dtype=np.int64)
    per_pair, cut = {}, 0
    for b, t in enumerate(texts):
        sa = sa_plain(t)
        rank = [0] * len(t)
        for slot, i in enumerate(sa):
            rank[i] = slot
        for q, masks in enumerate(all_masks):
            N, leaves = pair_walk(t, masks, k, rank)
            nodes[q, b] = N
            if node_limit is not None and N > node_limit:
                cut += 1
                leaves = [leaf for leaf in leaves if leaf[0] <= node_limit]
            recs = [(q, b, p, cost) for _, cost, at in leaves for p in at]
            occ[q, b] = len(recs)
            if recs:
                per_pair[(q, b)] = recs
    flat = [r for key in sorted(per_pair) for r in per_pair[key]]
    return occ, np.array(flat, dtype=NEAR_HIT_DTYPE) if flat else np.zeros(0, NEAR_HIT_DTYPE), int(occ.astype(np.int64).sum()), cut, nodes
