"""Mirror of the reference's `saca` module (src/saca.rs:344-384)."""
from .context import Context


class Constructor:
    """saca::Constructor: `new(max_n)`, `capacity()`, `compute(input) -> suffix array`; `compute_packed(inputs)` is this library's packed form; `compute_lcp` /
    `compute_packed_lcp` give the LCP arrays with the suffix arrays; `check` verifies a suffix array and `search` finds patterns with one."""

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

    def context(self):
        """the analogue of reuse(): the device workspace is lent to the later stages through the context"""
        return self._ctx
