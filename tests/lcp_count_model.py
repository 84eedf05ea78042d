"""A plain model of the two counters an LCP pass keeps while profiling is on (dk_stats.lcp_measured and lcp_bytes_compared, include/dark_amd.h),
restated from the rules of the kernels in csrc/lcp.hip, not from what they give.  No test here: tests/test_lcp_count_model.py pins count_model
against the per-position loop count_loop and shows that the cases below tell the model from three wrong ones; tests/test_gpu_profiling.py
hands the same cases to the kernels.

The rules, for a block T of n bytes with suffix array SA (a pack: every block on its own, the counters summed):
  which positions count   p = SA[i], i >= 1, with q = Phi[p] = SA[i-1], unless p is REDUCIBLE: p > 0, q > 0 and T[p-1] == T[q-1] (k_lcp_measure
                          marks those and k_lcp_fill derives them).  SA[0] has no suffix in front of it: k_lcp_phi stores its finished
                          answer and no kernel counts it.
  measured                the number of such positions: each is settled exactly once, by the lane (k_lcp_measure), by a wave (k_lcp_wave) or by
                          the grid (k_lcp_giant, whose workgroup 0 counts it), as long as no list overflows (lcp_passes == 1).
  bytes_compared          with L = LCP(p, q) and room = n - max(p, q):
                            lane   min(L, lane_cap); it hands on when L >= lane_cap and room > lane_cap
                            wave   min(L, wave_cap) - lane_cap; it hands on when L >= wave_cap and room > wave_cap (the wave stops AT the cap and
                                   has not seen the byte behind it)
                          so min(L, wave_cap) below the grid's kernel.  k_lcp_giant goes on at done = wave_cap in chunks of LCP_GIANT_CHUNK bytes,
                          chunk k at o0 = done + k * CHUNK for o0 < room, chunk k by workgroup k mod G of the G = LCP_GIANT_GRID launched; a
                          workgroup that compares a chunk counts min(room - o0, CHUNK) for it, whole, and a chunk is compared at most once.
                            at least   every chunk with o0 <= L: a workgroup stops in front of a chunk only when o0 >= the best answer so far,
                                       and no answer is below L
                            at most    those, and one more chunk per workgroup: a workgroup that compares a chunk behind L either finds a
                                       difference in it and stops, or -- the bytes being equal again there -- looks at the best answer before its
                                       next chunk.  With no more chunks than workgroups (every input of at most G * CHUNK = 4 MiB behind the
                                       cap, so every case here) no workgroup has a second chunk at all and the bound is exact reasoning; with
                                       more it rests on the workgroup of L's chunk being no full turn of the grid late.
                          count_model returns the closed interval [bytes_lo, bytes_hi]; the two are equal when nothing reaches the grid."""
import os
import re

import numpy as np

from lcp_model import lcp_kasai

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANE_CAP, WAVE_CAP, GIANT_CHUNK, COUNTERS, GIANT_GRID = 256, 65536, 4096, 256, 1024  # pinned by test_lcp_count_model.py::test_constants
VARIANTS = ("reducible_too",  # counts the reducible positions as well
            "no_wave",        # forgets the wave's part of the bytes
            "first_too")      # counts every block's first suffix


def read_constants():
    """the constants the model mirrors, as csrc/lcp.hip has them"""
    with open(os.path.join(ROOT, "dark_amd", "csrc", "lcp.hip")) as f:
        src = f.read()

    def constant(name):
        m = re.search(r"constexpr\s+\w+\s+(?:\w+\s*=\s*[^,;]+,\s*)*%s\s*=\s*([^,;]+)[,;]" % name, src)
        assert m, name
        return m.group(1).strip()
    out = {k: int(constant(k)) for k in ("LCP_LANE_CAP", "LCP_WAVE_CAP", "LCP_COUNTERS", "LCP_BLOCK")}
    assert constant("LCP_GIANT_CHUNK") == "16 * LCP_BLOCK"
    out["LCP_GIANT_CHUNK"] = 16 * out["LCP_BLOCK"]
    m = re.search(r"k_lcp_giant<<<dim3\((\d+)\), dim3\(LCP_BLOCK\)", src)
    assert m, "the launch of k_lcp_giant"
    out["LCP_GIANT_GRID"] = int(m.group(1))
    return out


def u8(x):
    return np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8)


def giant_interval(L, room, done, chunk=GIANT_CHUNK, grid=GIANT_GRID):
    """bytes k_lcp_giant counts for one listed pair: (at least, at most)"""
    starts = list(range(done, room, chunk))
    size = [min(room - o0, chunk) for o0 in starts]
    must = sum(1 for o0 in starts if o0 <= L)
    lo = sum(size[:must])
    return lo, lo + sum(size[must:must + grid])


def count_model(blocks, sas, lane_cap=LANE_CAP, wave_cap=WAVE_CAP, chunk=GIANT_CHUNK, grid=GIANT_GRID, variant=None, lcps=None):
    """-> dict(measured, bytes_lo, bytes_hi, longs, giants) for a pack (a single block: lists of one); lcps: the blocks' LCP arrays if the
    caller has them (lcp_kasai otherwise).  variant: one of VARIANTS, a model with that one mistake."""
    assert variant is None or variant in VARIANTS
    wave_cap = max(wave_cap, lane_cap)
    measured = lo = hi = longs = giants = 0
    for k, (t, sa) in enumerate(zip(blocks, sas)):
        t, sa = u8(t), np.asarray(sa, dtype=np.int64)
        n = len(t)
        lcp = np.asarray(lcps[k] if lcps is not None else lcp_kasai(t, sa), dtype=np.int64)
        if variant == "first_too":
            measured += 1  # (nothing in front of it to compare with: no bytes)
        if n < 2:
            continue
        p, q, L = sa[1:], sa[:-1], lcp[1:]
        both = (p > 0) & (q > 0)
        reducible = both & (t[np.where(both, p - 1, 0)] == t[np.where(both, q - 1, 0)])
        keep = np.ones(n - 1, bool) if variant == "reducible_too" else ~reducible
        p, q, L = p[keep], q[keep], L[keep]
        room = n - np.maximum(p, q)
        measured += len(p)
        lane = np.minimum(L, lane_cap)
        to_wave = (L >= lane_cap) & (room > lane_cap)
        wave = np.where(to_wave, np.minimum(L, wave_cap) - lane_cap, 0)
        to_grid = to_wave & (L >= wave_cap) & (room > wave_cap)
        longs += int(to_wave.sum())
        giants += int(to_grid.sum())
        below = int(lane.sum()) + (0 if variant == "no_wave" else int(wave.sum()))
        lo += below
        hi += below
        for j in np.flatnonzero(to_grid):
            a, b = giant_interval(int(L[j]), int(room[j]), wave_cap, chunk, grid)
            lo += a
            hi += b
    return dict(measured=measured, bytes_lo=lo, bytes_hi=hi, longs=longs, giants=giants)


def count_loop(blocks, sas, lane_cap, wave_cap, chunk, grid):
    """the same, one position at a time and one byte at a time, the three kernels in the order they run (small inputs only)"""
    wave_cap = max(wave_cap, lane_cap)
    measured = lo = hi = longs = giants = 0
    for t, sa in zip(blocks, sas):
        t, sa = bytes(u8(t)), [int(v) for v in sa]
        n = len(t)
        phi = {sa[i]: sa[i - 1] for i in range(1, n)}
        for p in range(n):
            if p not in phi:  # the block's first slot
                continue
            q = phi[p]
            if p > 0 and q > 0 and t[p - 1] == t[q - 1]:
                continue
            room = n - max(p, q)
            # k_lcp_measure
            lim, l = min(room, lane_cap), 0
            while l < lim and t[p + l] == t[q + l]:
                l += 1
            lo, hi = lo + l, hi + l
            if not (l == lane_cap and room > lane_cap):
                measured += 1
                continue
            # k_lcp_wave
            longs += 1
            lim, start = min(room, wave_cap), l
            while l < lim and t[p + l] == t[q + l]:
                l += 1
            lo, hi = lo + l - start, hi + l - start
            if l < lim or room <= wave_cap:
                measured += 1
                continue
            # k_lcp_giant: the chunks in order; `best` as the quickest and as the slowest grid would see it
            giants += 1
            measured += 1
            first = l
            while first < room and t[p + first] == t[q + first]:
                first += 1
            extra = 0
            for k, o0 in enumerate(range(l, room, chunk)):
                if o0 <= first:
                    lo, hi = lo + min(room - o0, chunk), hi + min(room - o0, chunk)
                elif extra < grid:  # one more per workgroup: the chunks right behind, every one another workgroup's
                    hi += min(room - o0, chunk)
                    extra += 1
    return dict(measured=measured, bytes_lo=lo, bytes_hi=hi, longs=longs, giants=giants)


# ---- the cases of tests/test_gpu_profiling.py --------------------------------------------------------------------------------------------------

def single_cases():
    """name -> (text, the routes the LCP call must report: a subset of {"lcp_long", "lcp_giant"}, or None where test_gpu_lcp.py asserts none)"""
    from test_gpu_lcp import HANDOFFS, fibonacci_word, handoff_routes, planted
    cases = {"planted%d" % length: (planted(length, seed=length), handoff_routes(length)) for length, _ in HANDOFFS}
    cases["planted90000"] = (planted(90000, seed=90000), {"lcp_long", "lcp_giant"})  # six chunks behind the cap, random bytes behind the passage
    h = np.random.default_rng(8).integers(0, 256, size=70000, dtype=np.uint8)
    cases["two_halves"] = (np.concatenate([h, h]), {"lcp_long", "lcp_giant"})
    cases["a4097"] = (np.full(4097, 97, np.uint8), {"lcp_long"})
    cases["a70000"] = (np.full(70000, 97, np.uint8), {"lcp_long", "lcp_giant"})
    cases["fibonacci"] = (u8(fibonacci_word(75025)), None)
    return cases


def pack_cases():
    """name -> (blocks, routes): the pack of test_gpu_lcp.py, and the single cases' texts as the blocks of packs of PACK_SIZES' kind (tiny blocks
    between them, a byte-identical neighbour)"""
    from test_gpu_lcp import PACK_SIZES, the_pack
    s = single_cases()
    rng = np.random.default_rng(12)
    tiny = [rng.integers(0, 256, size=k, dtype=np.uint8) for k in PACK_SIZES[:2]]
    cases = {"the_pack": (the_pack(), {"lcp_long", "lcp_giant"})}
    cases["lane_and_wave"] = ([tiny[0], s["planted255"][0], s["planted256"][0], tiny[1], s["planted257"][0], s["a4097"][0], s["a4097"][0].copy()],
                              {"lcp_long"})
    cases["around_the_wave_cap"] = ([s["planted65535"][0], tiny[0], s["planted65536"][0], s["planted65537"][0]], {"lcp_long", "lcp_giant"})
    cases["giants"] = ([tiny[1], s["planted90000"][0], s["a70000"][0], s["fibonacci"][0], tiny[0]], {"lcp_long", "lcp_giant"})
    return cases
