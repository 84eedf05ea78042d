"""Plain models of the FM-index's extract (csrc/bwt.hip k_pib_anchors, csrc/fm_index.hip k_fm_extract), the yardsticks of
tests/test_gpu_fm_extract.py.  tests/test_fm_extract_model.py pins them against slices of the text.

Conventions of tests/fm_locate_model.py: L[i] = T[SA[i] - 1], T[n - 1] at the slot `origin` where SA[origin] = 0; no sentinel; LF(x) for
x != origin as `lf` there, and SA[LF(x)] = SA[x] - 1.
  anchor[k] = ISA[k * step] for k < ceil(n / step): the slot of the suffix that starts at position k * step; anchor[0] = origin.
  A chunk is [k * step, e), e = min((k + 1) * step, n).  Start at x = anchor[k + 1] when e < n, at x = origin when e = n: L[x] = T[e - 1].  Then
  x <- LF(x) and L[x] give T[e - 2], T[e - 3], ... down to T[k * step]: at most min(step, n) - 1 LF steps.
  The one step that starts AT the origin is not the formula: LF(origin) = C[last], the slot of the one-byte suffix T[n - 1 ..], first of its class
  (the formula would add the [c == last] term)."""
import numpy as np

from fm_locate_model import NO_HIT, _u8, lf


def anchors(sa, step):
    """anchor[k] = the slot x with SA[x] = k * step, from a plain suffix array: what the build must equal"""
    sa = np.asarray(sa, dtype=np.int64)
    isa = np.empty(len(sa), dtype=np.int64)
    isa[sa] = np.arange(len(sa))
    return isa[::step].tolist()


def lf_from_origin(L, origin):
    """C[last]: where the walk goes from the origin's slot"""
    L = _u8(L)
    return int((L < L[origin]).sum())


def chunk(L, origin, anchor, step, k, down_to=None, special=True):
    """-> (the bytes T[max(k * step, down_to) : e) of chunk k, LF steps taken).  special=False: the walk without the origin's own step."""
    L = _u8(L)
    n = len(L)
    e = min((k + 1) * step, n)
    lo = k * step if down_to is None else max(k * step, down_to)
    x = anchor[k + 1] if e < n else origin
    out, steps = [int(L[x])], 0
    for _ in range(e - 1 - lo):
        x = lf_from_origin(L, origin) if special and x == origin else lf(L, origin, x)
        steps += 1
        out.append(int(L[x]))
    assert steps <= min(step, n) - 1, "the walk left its bound"
    return bytes(reversed(out)), steps


def extract(L, origin, anchor, step, a, length, special=True):
    """T[a : a + length) cut at n, chunk by chunk as the kernel's items do"""
    n = len(L)
    end = min(a + length, n)
    out = b""
    for k in range(a // step, (max(end, a + 1) - 1) // step + 1):
        if k * step >= end:
            break
        piece, _ = chunk(L, origin, anchor, step, k, down_to=a, special=special)
        out += piece[:end - max(k * step, a)]
    return out


def extract_rows(text, ranges, max_len):
    """rows of dk_dev_fm_extract for (pos, len) ranges (len None: max_len): T[pos : pos + min(len, max_len, n - pos)), zeros behind; nothing for
    pos >= n, NO_HIT included.  A uint8 array of len(ranges) x max_len."""
    t = _u8(text)
    n = len(t)
    out = np.zeros((len(ranges), max_len), dtype=np.uint8)
    for q, (pos, length) in enumerate(ranges):
        if pos >= n:
            continue
        got = min(max_len if length is None else length, max_len, n - pos)
        out[q, :got] = t[pos:pos + got]
    return out


__all__ = ["NO_HIT", "anchors", "chunk", "extract", "extract_rows", "lf_from_origin"]
