"""TEST HELPER: a plain model of what the inverse BWT owes its caller for ANY (L, origin) with origin < n, and a seeded generator of inputs
that are no BWT.  numpy and integers only, no tolerance anywhere.  Written from the rule in DESIGN.md section 4.4 (stable counting sort of
L, the origin element first in its symbol class); it shares no code with the kernels or with oracle/, and tests/test_ibwt_model.py pins it
against both before tests/test_gpu_inverse.py lets it judge the device path.

The successor table is a permutation with one entry replaced by END, so it is always ONE path that starts at `origin` plus zero or more
cycles.  (L, origin) is a text exactly when the path has n entries."""
from collections import namedtuple

import numpy as np

END = -1
IB_REC = 256            # bytes a splitter's walk records (csrc/bwt.hip); longer walks take the resume branch of the copy kernels
S_SWITCH = 1 << 16      # the single-block inverse places a splitter every 8 positions below this n, every 64 from it on


def spacing(n):
    """splitter spacing S of the single-block inverse for a block of n bytes"""
    return 8 if n < S_SWITCH else 64


Verdict = namedtuple("Verdict", "text d cycle_has_splitter longest_cycle longest_walk")
# text               the n bytes (numpy uint8) when (L, origin) is a text, else None
# d                  entries on the path from origin to END (d == n exactly for a text)
# cycle_has_splitter some position left over in a cycle is a multiple of S (names the case in a failure message, nothing more)
# longest_cycle      entries of the longest leftover cycle (0 for a text)
# longest_walk       the longest stretch of the path between two splitters (multiples of S, origin) or a splitter and END


def successor_table(L, origin):
    """psi, sym: psi[dest[i]] = i and sym[dest[i]] = L[i], where dest[i] = number of symbols below L[i] + rank of i among the equal symbols;
    the origin element goes first in its class and the equal symbols in front of it move up by one.  The origin element's entry is END."""
    L = np.ascontiguousarray(L, dtype=np.uint8)
    n = len(L)
    if not 0 <= origin < n:
        raise ValueError("origin %d outside a block of %d bytes" % (origin, n))
    count = np.bincount(L, minlength=256)
    below = np.concatenate([[0], np.cumsum(count)[:-1]])
    dest = np.empty(n, dtype=np.int64)
    for c in np.flatnonzero(count):
        at = np.flatnonzero(L == c)
        dest[at] = below[c] + np.arange(len(at))
    c0 = int(L[origin])
    dest[(L == c0) & (np.arange(n) < origin)] += 1
    dest[origin] = below[c0]
    psi = np.empty(n, dtype=np.int64)
    sym = np.empty(n, dtype=np.uint8)
    psi[dest] = np.arange(n)
    sym[dest] = L
    psi[dest[origin]] = END
    return psi, sym


def invert(L, origin, S=None):
    """walk from cur = origin: every step emits the symbol stored with psi[cur] and moves there, until END"""
    n = len(L)
    S = spacing(n) if S is None else S
    psi, sym = successor_table(L, origin)
    nxt = psi.tolist()
    path = []
    cur = origin
    while cur != END:
        path.append(cur)
        cur = nxt[cur]
        if len(path) > n:
            raise AssertionError("the model's path is longer than n: its table is no permutation")
    d = len(path)
    path = np.array(path, dtype=np.int64)
    marks = np.flatnonzero(path % S == 0)
    if len(marks) == 0 or marks[0] != 0:
        marks = np.concatenate([[0], marks])  # the origin is a splitter wherever it lies
    longest_walk = int(np.diff(np.concatenate([marks, [d]])).max())
    if d == n:
        return Verdict(sym[path], d, False, 0, longest_walk)
    left = np.ones(n, dtype=bool)
    left[path] = False
    rest = np.flatnonzero(left)
    has_splitter = bool((rest % S == 0).any())
    longest, seen = 0, set()
    for p in rest.tolist():
        if p in seen:
            continue
        k, q = 0, p
        while q not in seen:
            seen.add(q)
            q = nxt[q]
            k += 1
        longest = max(longest, k)
    return Verdict(None, d, has_splitter, longest, longest_walk)


Case = namedtuple("Case", "kind L origin verdict")
# kind: "a" one byte changed, "b" two unequal bytes swapped, "c" wrong origin, "d" random L (no 0xFF), "e" adjacent unequal swap at short text distance
# that leaves only cycles without a splitter, "f" the same with a leftover cycle longer than IB_REC, "g" one-symbol L with a wrong origin


def case(kind, L, origin, S=None):
    L = np.ascontiguousarray(L, dtype=np.uint8)
    return Case(kind, L, int(origin), invert(L, int(origin), S))


def random_damage(L, origin, seed, each=4):
    """classes a-d, `each` inputs per class; the model labels every one (a swap or a changed byte can leave a text)"""
    rng = np.random.default_rng(seed)
    n = len(L)
    out = []
    for _ in range(each):
        x = L.copy()
        i = int(rng.integers(0, n))
        x[i] = (int(x[i]) + int(rng.integers(1, 255))) % 255  # another value, never 0xFF (the block format cannot carry it)
        out.append(case("a", x, origin))
    for _ in range(each):
        while True:
            i, j = (int(v) for v in rng.integers(0, n, size=2))
            if L[i] != L[j]:
                break
        x = L.copy()
        x[i], x[j] = x[j], x[i]
        out.append(case("b", x, origin))
    for _ in range(each):
        out.append(case("c", L, (origin + int(rng.integers(1, n))) % n))
    for _ in range(each):
        out.append(case("d", rng.integers(0, 255, size=n, dtype=np.uint8), origin))
    return out


def adjacent_swaps(L, origin, sa, max_distance=40):
    """class e: EVERY i with L[i] != L[i+1] whose suffixes start at most max_distance text positions apart, kept when the model says
    "no text, no splitter in any leftover cycle".  One transposition of the table cuts a cycle out of the path whose length is the text
    distance of the two suffixes; a short cycle misses every multiple of S with probability about (1 - 1/S)^length."""
    sa = np.asarray(sa, dtype=np.int64)
    near = np.flatnonzero((L[:-1] != L[1:]) & (np.abs(sa[:-1] - sa[1:]) <= max_distance))
    out = []
    for i in near.tolist():
        x = L.copy()
        x[i], x[i + 1] = x[i + 1], x[i]
        c = case("e", x, origin)
        if c.verdict.text is None and not c.verdict.cycle_has_splitter:
            out.append(c)
    return out


def long_cycle_swaps(L, origin, sa, limit=3):
    """class f: adjacent unequal swaps whose leftover cycle is longer than IB_REC and still holds no splitter (at most `limit` of them).
    Candidates are screened by counting the multiples of S among the slots of the text positions strictly between the two suffixes;
    the model decides."""
    n = len(L)
    S = spacing(n)
    sa = np.asarray(sa, dtype=np.int64)
    isa = np.empty(n, dtype=np.int64)
    isa[sa] = np.arange(n)
    marks = np.concatenate([[0], np.cumsum(isa % S == 0)])  # marks[t] = multiples of S among the slots of text positions < t
    lo, hi = np.minimum(sa[:-1], sa[1:]), np.maximum(sa[:-1], sa[1:])
    far = np.flatnonzero((L[:-1] != L[1:]) & (hi - lo > IB_REC) & (marks[np.maximum(hi - 1, 0)] - marks[np.minimum(lo + 2, n)] <= 0))
    out = []
    for i in far.tolist():
        x = L.copy()
        x[i], x[i + 1] = x[i + 1], x[i]
        c = case("f", x, origin)
        if c.verdict.text is None and not c.verdict.cycle_has_splitter and c.verdict.longest_cycle > IB_REC:
            out.append(c)
            if len(out) == limit:
                break
    return out


def one_symbol():
    """class g: one-symbol L with origin = n - 2 and origin = 0, at n = 10 (S = 8) and n = 70000 (S = 64).  Only origin = n - 1 is a text."""
    return [case("g", np.full(n, 0x61, np.uint8), o) for n in (10, 70000) for o in (n - 2, 0)]


def word_text(n):
    """the text the damaged inputs start from: word-like, no byte 0xFF (so that its streams decode)"""
    from dark_amd import datagen
    return np.ascontiguousarray(datagen.word_like(n, seed=5, vocab=2000))


def no_bwt_inputs(orc, n, seed=1):
    """(text, L, origin, cases): a correct BWT of a word-like text of n bytes and classes a-f made from it"""
    text = word_text(n)
    sa = orc.sa_sais(text)
    L, origin = orc.bwt_forward(text, sa)
    cases = random_damage(L, origin, seed) + adjacent_swaps(L, origin, sa) + long_cycle_swaps(L, origin, sa)
    return text, L, origin, cases
