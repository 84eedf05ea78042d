"""Mirror of the reference's `saca` module (src/saca.rs:344-384)."""
import numpy as np

from .context import Context


class Constructor:
    """saca::Constructor: `new(max_n)`, `capacity()`, `compute(input) -> suffix array`; `compute_packed(inputs)` is this library's packed form; `compute_lcp` /
    `compute_packed_lcp` give the LCP arrays with the suffix arrays; `check` verifies a suffix array and `search` finds patterns with one;
    `match` gives the matching statistics of query texts against the data and `smems` their super-maximal exact matches."""

    def __init__(self, max_n, device=0):
        self._ctx = Context(max_n, device)
        self._n = max_n

    def capacity(self):
        return self._ctx.capacity()

    def compute(self, data):
        if len(data) != self._n:  # src/saca.rs:369 assert_eq!(input.len(), self.n)
            raise ValueError("Constructor sized for %d bytes got %d" % (self._n, len(data)))
        return self._ctx.suffix_array(data)

    def compute_packed(self, inputs):
        """compute for many small inputs at once: a list of suffix arrays, one per input, from one segmented device pass.  The inputs
        together must fit the capacity (each alone need not have the constructor's exact size)."""
        total = sum(len(x) for x in inputs)
        if total > self.capacity():
            raise ValueError("Constructor sized for %d bytes got a pack of %d" % (self.capacity(), total))
        return self._ctx.suffix_array_packed(inputs)

    def compute_lcp(self, data):
        """compute, and the LCP array with it: (suffix array, LCP array), LCP[0] = 0"""
        if len(data) != self._n:
            raise ValueError("Constructor sized for %d bytes got %d" % (self._n, len(data)))
        return self._ctx.suffix_array_lcp(data)

    def compute_packed_lcp(self, inputs):
        """compute_packed, and every input's LCP array with it: a list of (suffix array, LCP array), from one segmented device pass"""
        total = sum(len(x) for x in inputs)
        if total > self.capacity():
            raise ValueError("Constructor sized for %d bytes got a pack of %d" % (self.capacity(), total))
        return self._ctx.suffix_array_packed_lcp(inputs)

    def check(self, data, suffixes):
        """is `suffixes` what compute(data) returns?  -> (verdict, where): ("ok", n), or the first kind of fault -- "bad_range",
        "not_permutation", "bad_order" -- and the lowest slot (text position for "not_permutation") that shows it.  The reference has no counterpart."""
        if len(data) != self._n:
            raise ValueError("Constructor sized for %d bytes got %d" % (self._n, len(data)))
        return self._ctx.sa_check(data, suffixes)

    def search(self, data, suffixes, patterns):
        """(lo, hi) per pattern: suffixes[lo[q]:hi[q]] are exactly the places patterns[q] occurs in data.  `suffixes` is trusted (see check)."""
        if len(data) != self._n:
            raise ValueError("Constructor sized for %d bytes got %d" % (self._n, len(data)))
        return self._ctx.sa_search(data, suffixes, patterns)

    def match(self, data, suffixes, queries, max_len):
        """the matching statistics of every query against data: a list of (len, lo, hi), one per query, arrays over its positions -- len[i] = the
        longest prefix of query[i:i + max_len] that occurs in data, suffixes[lo[i]:hi[i]] = where it does.  `suffixes` is trusted (see check)."""
        if len(data) != self._n:
            raise ValueError("Constructor sized for %d bytes got %d" % (self._n, len(data)))
        ln, lo, hi = self._ctx.sa_match(data, suffixes, queries, max_len)
        out, at = [], 0
        for q in queries:
            out.append((ln[at:at + len(q)], lo[at:at + len(q)], hi[at:at + len(q)]))
            at += len(q)
        return out

    def smems(self, data, suffixes, queries, min_len, max_len, max_hits=65536):
        """(records, total): the super-maximal exact matches of the queries in data, those of at least min_len bytes -- a structured array with the
        fields query, pos (the match starts at queries[query][pos]), at (the same as an offset into the queries back to back), len, lo, hi
        (suffixes[lo:hi] = where it occurs); the first min(total, max_hits) in the order (query, pos).  A copy longer than max_len is reported
        once, with len = max_len."""
        if len(data) != self._n:
            raise ValueError("Constructor sized for %d bytes got %d" % (self._n, len(data)))
        recs, total = self._ctx.sa_smems(data, suffixes, queries, min_len, max_len, max_hits)
        lens = np.array([len(q) for q in queries], dtype=np.int64)
        ends = np.cumsum(lens)
        out = np.zeros(len(recs), dtype=[("query", np.uint32), ("pos", np.uint32)] + [(k, np.uint32) for k in ("at", "len", "lo", "hi")])
        for k in ("at", "len", "lo", "hi"):
            out[k] = recs[k]
        if len(recs):
            at = recs["at"].astype(np.int64)
            query = np.searchsorted(ends, at, side="right")  # the first query that ends behind the position (empty ones end at it)
            out["query"] = query
            out["pos"] = at - (ends - lens)[query]
        return out, total

    def context(self):
        """the analogue of reuse(): the device workspace is lent to the later stages through the context"""
        return self._ctx
