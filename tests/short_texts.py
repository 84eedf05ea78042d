"""TEST HELPER: every short text over a small alphabet, the packs made of them, and plain models of what the transform core owes for each --
suffix array, (L, origin) and LCP.  Integers and `bytes` only, written from the definitions in DESIGN.md section 4.4 and 4.11; no code is shared
with the kernels, with oracle/ or with the other models.  tests/test_short_texts_host.py pins the models against the oracle and proves that every
pack decides between the true model and each of FAULTS; tests/test_gpu_short_texts.py gives the packs to the kernels.

A pack is what one packed call takes: blocks back to back.  Packed suffix arrays and LCP arrays are local to their block."""
import itertools
from collections import namedtuple

import numpy as np

A, B, C = 0x61, 0x62, 0x63


def texts(alphabet, lo, hi):
    """every text of lo .. hi bytes over `alphabet`, in (length, lexicographic) order"""
    alphabet = sorted(alphabet)
    return [bytes(p) for m in range(lo, hi + 1) for p in itertools.product(alphabet, repeat=m)]


_sets = {}
SETS = dict(BIN15=((A, B), 1, 15), BIN12=((A, B), 1, 12), BIN10=((A, B), 1, 10), BIN8=((A, B), 1, 8), TER8=((A, B, C), 1, 8), TER6=((A, B, C), 1, 6),
            EXT10=((0x00, 0xFF), 1, 10))


def text_set(name):
    """one of SETS by name, enumerated once"""
    if name not in _sets:
        _sets[name] = texts(*SETS[name])
    return _sets[name]


def count_and_bytes(sigma, m):
    """closed forms for the texts of 1 .. m bytes over sigma symbols: how many, and their bytes in all (sum of k sigma^k)"""
    count = (sigma ** (m + 1) - sigma) // (sigma - 1)
    total = sigma * (1 - (m + 1) * sigma ** m + m * sigma ** (m + 1)) // (sigma - 1) ** 2
    return count, total


# ---- the plain models ------------------------------------------------------------------------------------------------------------------------

def sa(t):
    """the suffixes sorted by byte comparison, a proper prefix smaller (Python's order of bytes)"""
    return sorted(range(len(t)), key=lambda i: t[i:])


def bwt(t, s):
    """(L, origin): L[j] = t[sa[j] - 1], t[n - 1] where sa[j] == 0, and origin is that j"""
    return bytes(t[i - 1] for i in s), s.index(0)


def lcp(t, s):
    """lcp[0] = 0, lcp[j] = leading bytes the suffixes sa[j - 1] and sa[j] share; a common prefix ends where the shorter suffix ends"""
    out = [0] * len(t)
    for j in range(1, len(t)):
        x, y = t[s[j - 1]:], t[s[j]:]
        k = 0
        while k < len(x) and k < len(y) and x[k] == y[k]:
            k += 1
        out[j] = k
    return out


# ---- fault models (host test only): each is one line of a model above, changed -----------------------------------------------------------------

def _sa_reads_next_block(t, after):
    return sorted(range(len(t)), key=lambda i: t[i:] + after)          # the comparison runs on into the block behind


def _sa_prefix_is_larger(t, after):
    return sorted(range(len(t)), key=lambda i: tuple(t[i:]) + (256,))  # a proper prefix sorts last


def _origin_plus_one(s):
    return s.index(0) + 1


FAULTS = {"reads_next_block": dict(sa=_sa_reads_next_block), "prefix_is_larger": dict(sa=_sa_prefix_is_larger),
          "origin_is_sa_zero_plus_one": dict(origin=_origin_plus_one)}

_answers = {}


def answers(t, after=b"", fault=None):
    """(sa, L, origin, lcp) of one block; `after` = the bytes behind it in its pack, which only a fault model looks at"""
    if fault is None and t in _answers:
        return _answers[t]
    f = FAULTS[fault] if fault else {}
    s = f["sa"](t, after) if "sa" in f else sa(t)
    L, origin = bwt(t, s)
    if "origin" in f:
        origin = f["origin"](s)
    out = (s, L, origin, lcp(t, s))
    if fault is None:
        _answers[t] = out
    return out


Expected = namedtuple("Expected", "sizes off total text sa L origin lcp")
# sizes, off   the blocks' lengths and their offsets in the pack (count + 1 entries, int64)
# text, L      the pack's bytes and the blocks' L back to back (numpy uint8)
# sa, lcp      the blocks' arrays back to back, entries local to the block (numpy uint32)
# origin       one per block (list)


def expected(blocks, fault=None):
    """the arrays a packed call writes for `blocks`: the per-block answers back to back"""
    sizes = [len(b) for b in blocks]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(off[-1])
    if fault is None:
        per = [answers(b) for b in blocks]
    else:
        per = [answers(b, blocks[i + 1] if i + 1 < len(blocks) else b"", fault) for i, b in enumerate(blocks)]
    flat = lambda k: np.fromiter(itertools.chain.from_iterable(p[k] for p in per), dtype=np.uint32, count=total)  # noqa: E731
    return Expected(sizes, off, total, np.frombuffer(b"".join(blocks), np.uint8), flat(0), np.frombuffer(b"".join(p[1] for p in per), np.uint8),
                    [p[2] for p in per], flat(3))


def block_of(e, index):
    """the block that entry `index` of a concatenated array belongs to, and its place in it"""
    blk = int(np.searchsorted(e.off, index, side="right")) - 1
    return blk, int(index - e.off[blk])


# ---- the packs ---------------------------------------------------------------------------------------------------------------------------------

Pack = namedtuple("Pack", "name blocks")
ALL256 = bytes(range(256))
SHUFFLE_SEED = 15


def _bin15_wide():
    return text_set("BIN15") + [ALL256]


def _bin15_shuffled():
    blocks = _bin15_wide()
    return [blocks[i] for i in np.random.default_rng(SHUFFLE_SEED).permutation(len(blocks)).tolist()]


def _neighbours():
    blocks = []
    for u in text_set("BIN8"):
        for v in texts((A, B), 3, 3):
            blocks += [u, v]
    return blocks + [ALL256]


_BUILDERS = {
    "bin15": lambda: list(text_set("BIN15")),
    "bin15_wide": _bin15_wide,
    "bin15_reversed": lambda: _bin15_wide()[::-1],
    "bin15_shuffled": _bin15_shuffled,
    "neighbours": _neighbours,
    "mixed": lambda: text_set("TER8") + text_set("EXT10") + text_set("BIN10"),
}
PACK_NAMES = tuple(_BUILDERS)
_packs = {}


def pack(name):
    if name not in _packs:
        _packs[name] = Pack(name, _BUILDERS[name]())
    return _packs[name]
