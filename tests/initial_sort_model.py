"""TEST HELPER: plain numpy model of the suffix sort's initial sort -- what dk_dbg_dev_initial_sort runs: one sort_pairs() of csrc/radix_sort.hip
with the text keys and the final destinations of initial_sort() -- written from the definition below and not from the kernels.
tests/test_initial_sort_model.py pins it against a per-position Python loop before tests/test_gpu_initial_sort.py lets it judge the device.
Integers only, no tolerance anywhere.

The input is a text T of n bytes, a table code[256] of codes below 2^bits, a prefix length spk, and with the carry a table inv[256].  B = bits spk.

  window(i)   the codes of T[i .. i + spk) packed big-endian, `bits` each; a position from n on contributes the code 0
  key(i)      window(i); with the carry window(i) << 8 | code[T[i - 1]], where T[-1] is T[n - 1]
  order       stable by window: ties stand in position order (an LSD sort on exactly the window's B bits whose input is in position order; the
              carried byte has no say)
  sa[slot]    the position at that slot; keys[slot] its key; the NARROW word is the window's low 32 bits instead
  L[slot]     inv[key & 0xFF]; origin = the slot of position 0 (carry only)
  passes      ceil(B / 8); sorted_elements = n passes
  bucket_starts[d]   (narrow only) the pairs whose LAST-PASS digit is below d.  That digit is what the passes before it leave of the window: its top
              B - 8 (passes - 1) bits.  From the largest digit present upward the value is n
  packed      the route bit DK_ROUTE_PACKED_PAIRS, by the rule of sort_pairs_classic restated: 8 < B <= 32, and the position (ceil(log2 n) bits)
              and, with the carry, a code (`bits` bits) share one 32-bit word; the tuning build's DK_PACKED_SORT=0 switches the form off"""
from types import SimpleNamespace

import numpy as np

ROUTE_PACKED_PAIRS = 0x10000
TILE = 4096        # RS_TILE: positions per tile of the sort's kernels
TEXT_AHEAD = 80    # RS_TEXT_AHEAD: a tile takes the 16-byte loads only if the text goes on for this many bytes behind it


def ceil_log2(v):
    """smallest b with 2^b >= v"""
    b = 0
    while (1 << b) < v:
        b += 1
    return b


def packed_rule(n, bits, spk, with_prev, packed_sort=True):
    sorted_bits = bits * spk
    return bool(packed_sort and 8 < sorted_bits <= 32 and (bits if with_prev else 0) + ceil_log2(n) <= 32)


def passes_of(bits, spk):
    return (bits * spk + 7) // 8


def windows(text, code, bits, spk):
    """window(i) for every position -> uint64"""
    text = np.asarray(text, dtype=np.uint8)
    n = len(text)
    c = np.zeros(n + spk, np.uint64)
    c[:n] = np.asarray(code, dtype=np.uint8)[text]
    w = np.zeros(n, np.uint64)
    for j in range(spk):
        w = (w << np.uint64(bits)) | c[j:j + n]  # (the first of 64 / bits steps shifts zeros out: nothing is lost)
    return w


def initial_sort_model(text, code, bits, spk, inv=None, narrow=False, packed_sort=True):
    """-> namespace: sa (uint32), keys (uint64, or the uint32 words when narrow), wide_keys (uint64 always), window (uint64, sorted), bwt and origin
    (None without inv), bucket_starts (256 words, None unless narrow), passes, sorted_elements, packed, route"""
    text = np.asarray(text, dtype=np.uint8)
    code = np.asarray(code, dtype=np.uint8)
    n, with_prev = len(text), inv is not None
    sorted_bits = bits * spk
    assert 1 <= bits <= 8 and spk >= 1 and sorted_bits + (8 if with_prev else 0) <= 64 and int(code.max()) < (1 << bits) and n >= 1
    assert not narrow or sorted_bits <= 40
    w = windows(text, code, bits, spk)
    idx_bits = ceil_log2(n)
    if sorted_bits + idx_bits <= 64:  # (window, position) in one word: distinct, so a plain sort of them is the stable order, and quicker to get
        both = np.sort((w << np.uint64(idx_bits)) | np.arange(n, dtype=np.uint64))
        order = (both & np.uint64((1 << idx_bits) - 1)).astype(np.int64)
    else:
        order = np.argsort(w, kind="stable")
    m = SimpleNamespace(passes=passes_of(bits, spk), packed=packed_rule(n, bits, spk, with_prev, packed_sort))
    m.sa = order.astype(np.uint32)
    m.window = w[order]
    if with_prev:
        prev = code[np.roll(text, 1)].astype(np.uint64)
        m.wide_keys = (m.window << np.uint64(8)) | prev[order]
        m.bwt = np.asarray(inv, dtype=np.uint8)[(m.wide_keys & np.uint64(0xFF)).astype(np.uint8)]
        m.origin = int(np.flatnonzero(order == 0)[0])
    else:
        m.wide_keys, m.bwt, m.origin = m.window, None, None
    m.keys = m.window.astype(np.uint32) if narrow else m.wide_keys
    m.bucket_starts = None
    if narrow:
        digit = m.window >> np.uint64(8 * (m.passes - 1))  # non-decreasing: the window's top bits
        m.bucket_starts = np.searchsorted(digit, np.arange(256, dtype=np.uint64), side="left").astype(np.uint32)
    m.sorted_elements = n * m.passes
    m.route = ROUTE_PACKED_PAIRS if m.packed else 0
    return m


def heads_by_window(window):
    """slots whose window differs from the slot's in front (slot 0 included): the groups the first rerank must find"""
    head = np.ones(len(window), bool)
    head[1:] = window[1:] != window[:-1]
    return head


def heads_by_narrow(words, bucket_starts):
    """the same from what a narrow sort leaves: the word changes, or the slot is a bucket start"""
    n = len(words)
    head = np.ones(n, bool)
    head[1:] = words[1:] != words[:-1]
    s = np.asarray(bucket_starts, dtype=np.int64)
    head[s[s < n]] = True
    return head


# ---- the same, one position at a time (tests/test_initial_sort_model.py compares the two) ---------------------------------------------------
def initial_sort_loop(text, code, bits, spk, inv=None, narrow=False):
    """-> dict of plain lists and numbers under initial_sort_model's names, straight from the sentences of the module docstring"""
    t = [int(x) for x in text]
    n = len(t)
    code = [int(x) for x in code]
    win = []
    for i in range(n):
        w = 0
        for j in range(spk):
            w = (w << bits) | (code[t[i + j]] if i + j < n else 0)
        win.append(w)
    order = [i for _, i in sorted((win[i], i) for i in range(n))]
    r = dict(sa=order, window=[win[i] for i in order], bwt=None, origin=None, bucket_starts=None)
    if inv is not None:
        r["wide_keys"] = [(win[i] << 8) | code[t[i - 1]] for i in order]  # (t[-1] is the last byte)
        r["bwt"] = [int(inv[k & 0xFF]) for k in r["wide_keys"]]
        r["origin"] = order.index(0)
    else:
        r["wide_keys"] = list(r["window"])
    r["keys"] = [w & 0xFFFFFFFF for w in r["window"]] if narrow else r["wide_keys"]
    r["passes"] = -(-bits * spk // 8)
    r["sorted_elements"] = n * r["passes"]
    if narrow:
        top = bits * spk - 8 * (r["passes"] - 1)
        digit = [w >> (bits * spk - top) for w in win]
        r["bucket_starts"] = [sum(1 for x in digit if x < d) for d in range(256)]
    return r
