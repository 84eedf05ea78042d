"""Cases that drive the query-side scans past their first level, with the level arithmetic of each scan restated from its host driver and plain
models quick enough for inputs of megabytes.  No test here: tests/test_scan_levels_host.py pins the constants against the sources, shows that
every case reaches the levels it is named after and that the level DECIDES its answer (the model with one fault in its scan gives another
answer), and tests/test_gpu_scan_levels.py hands the same cases to the kernels.

The scans (DESIGN.md sections 4.11, 4.13 - 4.16, 4.19):
  k_lcp_spine       (lcp.hip)      one workgroup, passes of SPINE tiles of LCP_TILE positions, a carry from pass to pass
  k_fm_scan_a/b/c   (fm_index.hip) rows = ceil(total / FM_BLOCK) + 1, chunks of rpc = ceil(rows / FM_MAX_CHUNKS) rows
  k_fm_find_scan_*  (fm_index.hip) 64-bit sums over rows of FM_FIND_ROW pairs, chunks of rpc rows; k_fm_find_locate's 64-ary pair search
  k_loc_scan        (bwt.hip)      one workgroup, per = ceil(rows / SPINE) rows of LOC_ROW slots per thread
  k_ibwt_scan_*     (bwt.hip)      tiles of IB_TILE symbols, chunks of tpc = ceil(tiles / IB_MAX_CHUNKS) tiles
  k_sa_smem_scan_b  (sa_query.hip) one workgroup, trips of SM_TRIP tiles of SM_TILE positions

The faults a model can carry (FAULTS): the mistakes such scans make when they are wrong only above their first level."""
import os
import re

import numpy as np

from lcp_model import _extend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0x5A5A5A5A  # what a read behind an array's end sees in the models: the guard words of the GPU tests

FAULTS = ("second_from_zero",  # the second pass or trip starts from zero
          "bases_zero",        # the chunk bases of chunks >= 1 are zero
          "full_last_chunk",   # a short last chunk runs its full rpc rows
          "sum32",             # a 64-bit sum is kept in 32 bits
          "per_one")           # per is taken as 1


def _source(name):
    with open(os.path.join(ROOT, "dark_amd", "csrc", name)) as f:
        return f.read()


def _constant(src, name):
    m = re.search(r"constexpr\s+\w+\s+(?:\w+\s*=\s*[^,;]+,\s*)*%s\s*=\s*([^,;]+)[,;]" % name, src)
    assert m, name
    return m.group(1).strip()


def read_constants():
    """the constants the arithmetic below mirrors, as the sources have them"""
    lcp, fmi, bwt, saq = _source("lcp.hip"), _source("fm_index.hip"), _source("bwt.hip"), _source("sa_query.hip")
    out = {}
    assert _constant(lcp, "LCP_TILE") == "LCP_BLOCK * LCP_IPT"
    out["LCP_TILE"] = int(_constant(lcp, "LCP_BLOCK")) * int(_constant(lcp, "LCP_IPT"))
    out["FM_BLOCK"] = int(_constant(fmi, "FM_BLOCK"))
    out["FM_MAX_CHUNKS"] = int(_constant(fmi, "FM_MAX_CHUNKS"))
    out["FM_FIND_ROW"] = int(_constant(fmi, "FM_FIND_ROW"))
    assert _constant(bwt, "IB_TILE") == "IB_BLOCK * IB_SPT"
    out["IB_TILE"] = int(_constant(bwt, "IB_BLOCK")) * int(_constant(bwt, "IB_SPT"))
    out["IB_MAX_CHUNKS"] = int(_constant(bwt, "IB_MAX_CHUNKS"))
    out["SM_TILE"] = int(_constant(saq, "SM_TILE"))
    return out


LCP_TILE, FM_BLOCK, FM_MAX_CHUNKS, FM_FIND_ROW, IB_TILE, IB_MAX_CHUNKS, SM_TILE = 4096, 1024, 256, 256, 4096, 256, 1024
SPINE = 1024     # threads of the one-workgroup spines k_lcp_spine and k_loc_scan
LOC_ROW = 1024   # slots per row of the locate structure's marks (32 words of 32 bits, k_loc_rows)
SM_TRIP = 256    # tiles per trip of k_sa_smem_scan_b
LCP_BORDER = SPINE * LCP_TILE  # the first position of the spine's second pass


def div_up(a, b):
    return -(-a // b)


def u8(x):
    return np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8)


# ---- the level arithmetic ---------------------------------------------------------------------------------------------------------------------------

def lcp_levels(total):
    ntiles = div_up(total, LCP_TILE)
    return dict(ntiles=ntiles, passes=div_up(ntiles, SPINE), last_pass_tiles=ntiles - (div_up(ntiles, SPINE) - 1) * SPINE)


def chunked(rows, max_chunks):
    rpc = div_up(rows, max_chunks)
    nchunks = div_up(rows, rpc)
    return dict(rows=rows, rpc=rpc, nchunks=nchunks, last_chunk_rows=rows - (nchunks - 1) * rpc)


def fm_levels(total):
    return chunked(div_up(total, FM_BLOCK) + 1, FM_MAX_CHUNKS)


def find_levels(npairs):
    lv = chunked(div_up(npairs, FM_FIND_ROW), FM_MAX_CHUNKS)
    lv["last_row_pairs"] = npairs - (lv["rows"] - 1) * FM_FIND_ROW
    rounds, width = 0, npairs
    while width > 1:  # k_fm_find_locate: the stretch shrinks to ceil(width / 64) per round
        width = div_up(width, 64)
        rounds += 1
    lv["search_rounds"] = rounds
    return lv


def loc_levels(total):
    rows = div_up(total, LOC_ROW)
    per = div_up(rows, SPINE)
    return dict(rows=rows, per=per, busy_threads=div_up(rows, per))


def ibwt_levels(total):
    lv = chunked(div_up(total, IB_TILE), IB_MAX_CHUNKS)
    return dict(ntiles=lv["rows"], tpc=lv["rpc"], nchunks=lv["nchunks"], last_chunk_tiles=lv["last_chunk_rows"])


def smem_levels(Q):
    ntiles = div_up(Q, SM_TILE)
    return dict(ntiles=ntiles, trips=div_up(ntiles, SM_TRIP), last_trip_tiles=ntiles - (div_up(ntiles, SM_TRIP) - 1) * SM_TRIP)


# ---- LCP ------------------------------------------------------------------------------------------------------------------------------------------

def lcp_fast(text, sa):
    """the LCP array by definition: every pair of neighbours in the suffix array compared byte by byte, all pairs at once while many are still
    equal, the few long ones (a planted passage) one by one in chunks"""
    t, sa = u8(text), np.asarray(sa, dtype=np.int64)
    n = len(t)
    lcp = np.zeros(n, np.uint32)
    if n < 2:
        return lcp
    a, b = sa[:-1], sa[1:]
    h = np.zeros(n - 1, np.int64)
    act = np.arange(n - 1)
    for _ in range(12):
        x, y = a[act] + h[act], b[act] + h[act]
        ok = (x < n) & (y < n)
        ok[ok] = t[x[ok]] == t[y[ok]]
        act = act[ok]
        if act.size == 0:
            break
        h[act] += 1
    for i in act.tolist():
        h[i] = _extend(t, int(a[i]), int(b[i]), int(h[i]))
    lcp[1:] = h
    return lcp


def lcp_by_scan(blocks, sas, lcps, fault=None):
    """The LCP arrays of a pack the way csrc/lcp.hip makes them, given the true ones: Phi from the suffix arrays, the measured positions (block
    heads, first slots, positions whose pair differs in the byte in front) keep their true value, every other position p takes
    value(p0) - (p - p0) from the last measured p0 <= p, which k_lcp_tile_sum / k_lcp_spine / k_lcp_fill find by a max-scan over tiles.
    Without a fault this returns `lcps`; `second_from_zero` drops the spine's carry between passes.  -> list of arrays"""
    assert fault in (None, "second_from_zero")
    sizes = [len(b) for b in blocks]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(off[-1])
    t = np.concatenate([u8(b) for b in blocks])
    measured = np.zeros(total, bool)
    val = np.zeros(total, np.int64)
    for k, (sa, lcp) in enumerate(zip(sas, lcps)):
        s, sa = int(off[k]), np.asarray(sa, dtype=np.int64)
        p, q = s + sa[1:], s + sa[:-1]
        measured[s + sa[0]] = True
        m = (p == s) | (q == s)
        both = ~m
        m[both] = t[p[both] - 1] != t[q[both] - 1]
        measured[p] = m
        val[s + sa] = np.asarray(lcp, dtype=np.int64)
    ntiles = div_up(total, LCP_TILE)
    idx1 = np.zeros(ntiles * LCP_TILE, np.int64)
    idx1[:total] = np.where(measured, np.arange(1, total + 1), 0)
    in_tile = np.maximum.accumulate(idx1.reshape(ntiles, LCP_TILE), axis=1)
    agg = in_tile[:, -1].copy()
    excl, carry = np.zeros(ntiles, np.int64), 0
    for base in range(0, ntiles, SPINE):  # k_lcp_spine
        x = agg[base:base + SPINE]
        ex = np.concatenate([[0], np.maximum.accumulate(x)[:-1]])
        excl[base:base + SPINE] = np.maximum(carry, ex)
        carry = max(carry, int(x.max()))
        if fault == "second_from_zero":
            carry = 0
    prev = np.maximum(in_tile, excl[:, None]).reshape(-1)[:total]
    p0 = np.maximum(prev - 1, 0)
    plcp = np.where(prev > 0, np.maximum(val[p0] - (np.arange(total) - p0), 0), 0)
    plcp[measured] = val[measured]
    out = []
    for k, sa in enumerate(sas):
        s = int(off[k])
        got = plcp[s + np.asarray(sa, dtype=np.int64)].astype(np.uint32)
        got[0] = 0
        out.append(got)
    return out


def planted_at(n, start2, length, seed, start1=1000):
    """n random bytes below 250 with one passage of `length` bytes twice, at start1 and at start2, each copy between two fence bytes of its own
    (251 .. 254): one irreducible common prefix of `length` bytes at the second copy's first position, every later position of that copy
    reducible, and nothing else of more than a few bytes in common"""
    assert start1 >= 1 and start1 + length + 1 < start2 and start2 + length + 1 <= n
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 250, size=n, dtype=np.uint8)
    t[start2:start2 + length] = t[start1:start1 + length]
    t[start1 - 1], t[start1 + length], t[start2 - 1], t[start2 + length] = 251, 252, 253, 254
    return t


A1_PLANT = 18000
A1_START2 = LCP_BORDER - 2 * LCP_TILE - 8  # the second copy: two tiles and a little in front of the border ...
A1_N = A1_START2 + A1_PLANT + 300          # ... to 9800 bytes behind it: tiles 1024 and 1025 lie inside the copy


def lcp_text(name):
    """the single-block texts of part A"""
    if name == "a1_straddle":
        return planted_at(A1_N, A1_START2, A1_PLANT, seed=41)
    if name == "a2_exact":  # one pass exactly; the plant ends with the text's last tile
        return planted_at(LCP_BORDER, LCP_BORDER - 3000, 2000, seed=42)
    if name in ("a2_plus1", "a2_plus2"):
        # The last position of a text has PLCP 0 whatever the text is (a one-byte suffix is the first of its class), so the single position of
        # tile 1024 at n = border + 1 cannot hold a value that the carry decides: that size is run for its shape.  At n = border + 2 the
        # first position of tile 1024 can: the text ends in 251 252 253, and 251 252 7 stands once elsewhere, behind another byte.  Then
        # PLCP[n - 3] = 2 is measured in tile 1023 and position n - 2 = border is reducible with the value 1.
        n = LCP_BORDER + (1 if name == "a2_plus1" else 2)
        t = np.random.default_rng(43).integers(0, 250, size=n, dtype=np.uint8)
        t[n - 3:] = (251, 252, 253)
        t[5000:5003] = (251, 252, 7)
        t[4999] = (int(t[n - 4]) + 1) % 250
        return t
    raise KeyError(name)


LCP_SINGLE = ("a1_straddle", "a2_exact", "a2_plus1", "a2_plus2")
A3_SIZES = (LCP_BORDER + 1000, 9000, 1, 5000)  # block 1's head at border + 1000, inside tile 1024


def lcp_pack():
    """part A3: block 0's plant straddles the border; block 1 begins inside tile 1024 and has a plant of its own behind its head, so the values
    there come from block 1's measured positions and not from block 0's carry"""
    b0 = planted_at(A3_SIZES[0], LCP_BORDER - 700, 1500, seed=44)
    b1 = planted_at(A3_SIZES[1], 4000, 2500, seed=45, start1=100)
    rng = np.random.default_rng(46)
    return [b0, b1, rng.integers(0, 250, size=1, dtype=np.uint8), rng.integers(0, 4, size=A3_SIZES[3], dtype=np.uint8)]


# ---- FM build ---------------------------------------------------------------------------------------------------------------------------------------

FM_TOTALS = {"rows256": 255 * 1024, "rows257": 255 * 1024 + 1, "rows259": 257 * 1024 + 1, "rows514": 512 * 1024 + 5, "rows768": 767 * 1024}


def fm_bytes(total, seed=0):
    return np.random.default_rng(9000 + seed + total).integers(0, 256, size=total, dtype=np.uint8)


def fm_row_hist(L, rows):
    L = u8(L)
    h = np.bincount((np.arange(len(L)) // FM_BLOCK) * 256 + L, minlength=rows * 256)
    return h.reshape(rows, 256).astype(np.int64)


def fm_checkpoints(L):
    """row k = occurrences of every symbol in L[0, k FM_BLOCK): prefix counts, nothing else"""
    rows = div_up(len(L), FM_BLOCK) + 1
    h = fm_row_hist(L, rows)
    return (np.cumsum(h, axis=0) - h).astype(np.uint32)


def chunk_scan(values, max_chunks, fault=None, bits=32):
    """The exclusive scan down the rows of `values` (rows x columns) the way k_fm_scan_a/b/c and k_ibwt_scan_a/b/c do it: chunk sums, their
    exclusive scan, every chunk again from its base.  -> rows' x columns, rows' = nchunks * rpc: the rows behind `rows` hold POISON unless
    `full_last_chunk` makes the last chunk write them (and read POISON there)."""
    assert fault in (None, "bases_zero", "full_last_chunk")
    values = np.asarray(values, dtype=np.int64)
    lv = chunked(values.shape[0], max_chunks)
    rows, rpc, nchunks = lv["rows"], lv["rpc"], lv["nchunks"]
    padded = np.full((nchunks * rpc, values.shape[1]), POISON, np.int64)
    padded[:rows] = values
    seen = padded.copy() if fault == "full_last_chunk" else np.where(np.arange(nchunks * rpc)[:, None] < rows, padded, 0)
    per_chunk = seen.reshape(nchunks, rpc, -1)
    sums = per_chunk.sum(axis=1)
    bases = np.cumsum(sums, axis=0) - sums
    if fault == "bases_zero":
        bases[1:] = 0
    out = (bases[:, None, :] + np.cumsum(per_chunk, axis=1) - per_chunk).reshape(nchunks * rpc, -1) & ((1 << bits) - 1)
    if fault != "full_last_chunk":
        out[rows:] = POISON
    return out


def fm_checkpoints_by_scan(L, fault=None):
    rows = div_up(len(L), FM_BLOCK) + 1
    return chunk_scan(fm_row_hist(L, rows), FM_MAX_CHUNKS, fault)


def fm_pack_sizes():
    """several blocks at rows 514 (rpc 3): every head behind the first lies behind chunk 0, none on a row's border"""
    total = FM_TOTALS["rows514"]
    sizes = [170 * 1024 + 37, 85 * 1024 + 500, 3, 256 * 1024 - 211]
    return sizes + [total - sum(sizes)]


# ---- the find family's scan ---------------------------------------------------------------------------------------------------------------------------

def find_scan(occ, fault=None):
    """offset[p] = sum of occ below p and the grand total, the way k_fm_find_scan_a/b/c make them.  -> (offsets uint64, total).  A read behind
    the pairs sees POISON."""
    assert fault in (None, "bases_zero", "full_last_chunk", "sum32")
    occ = np.asarray(occ, dtype=np.uint64).reshape(-1)
    npairs = len(occ)
    lv = find_levels(npairs)
    rpc, nchunks = lv["rpc"], lv["nchunks"]
    padded = np.zeros(nchunks * rpc * FM_FIND_ROW, np.uint64)
    padded[:npairs] = occ
    if fault == "full_last_chunk":
        padded[npairs:] = POISON
    mask = np.uint64(0xFFFFFFFF if fault == "sum32" else 0xFFFFFFFFFFFFFFFF)
    sums = padded.reshape(nchunks, -1).sum(axis=1, dtype=np.uint64) & mask
    bases = (np.cumsum(sums, dtype=np.uint64) - sums) & mask
    total = int(sums.sum(dtype=np.uint64) & mask)
    if fault == "bases_zero":
        bases[1:] = 0
    inner = padded.reshape(nchunks, -1)
    offsets = ((bases[:, None] + np.cumsum(inner, axis=1, dtype=np.uint64) - inner) & mask).reshape(-1)[:npairs]
    return offsets, total


def find_pairs_of_hits(offsets, nhits):
    """k_fm_find_locate's 64-ary search, lane for lane: -> (the pair of every hit h < nhits, h - offset[pair], the most rounds a hit took)"""
    offsets = np.asarray(offsets, dtype=np.uint64)
    npairs = len(offsets)
    h = np.arange(nhits, dtype=np.uint64)
    plo, phi = np.zeros(nhits, np.int64), np.full(nhits, npairs, np.int64)
    lanes = np.arange(64, dtype=np.int64)[None, :]
    rounds = 0
    while True:
        act = np.flatnonzero(phi - plo > 1)
        if act.size == 0:
            break
        rounds += 1
        lo, hi = plo[act], phi[act]
        stride = (hi - lo + 63) >> 6
        idx = lo[:, None] + lanes * stride[:, None]
        ok = idx < hi[:, None]
        ok[ok] = offsets[idx[ok]] <= np.broadcast_to(h[act][:, None], idx.shape)[ok]
        k = np.maximum(ok.sum(axis=1) - 1, 0)
        lo = lo + k * stride
        plo[act] = lo
        phi[act] = np.where(hi - lo > stride, lo + stride, hi)
    pair = np.minimum(plo, npairs - 1)
    return pair, (h - offsets[pair]).astype(np.int64) if nhits else np.zeros(0, np.int64), rounds


HIT_DTYPE = np.dtype([("pattern", np.uint32), ("block", np.uint32), ("position", np.uint32), ("slot", np.uint32)])


def find_by_scan(occ, los, sas, max_hits, fault=None):
    """find's answer from the pairs' (lo, occ) through the scan and the pair search, as the device does it: -> (records, total, search rounds).
    occ, los: npat x count; sas: the blocks' suffix arrays.  A slot is clamped to its block as in k_fm_find_locate."""
    occ = np.asarray(occ, dtype=np.int64)
    npat, count = occ.shape
    offsets, total = find_scan(occ, fault)
    nhits = int(min(total, max_hits))
    pair, inside, rounds = find_pairs_of_hits(offsets, nhits)
    rec = np.zeros(nhits, HIT_DTYPE)
    q, b = pair // count, pair % count
    sizes = np.array([len(s) for s in sas], dtype=np.int64)
    lo = np.minimum(np.asarray(los, dtype=np.int64).reshape(-1)[pair], sizes[b])
    x = np.where(lo + inside < sizes[b], lo + inside, sizes[b] - 1)  # (inside < 0 from a wrapped offset: a huge unsigned number on the device)
    x = np.where(inside < 0, sizes[b] - 1, x)
    rec["pattern"], rec["block"], rec["slot"] = q, b, x
    flat = np.concatenate([np.asarray(s, dtype=np.int64) for s in sas])
    starts = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    rec["position"] = flat[starts[b] + x]
    return rec, total, rounds


def find_fast(sas, Ls, origins, distinct, which, max_hits=None):
    """find's answer by the definition: the range of every DISTINCT pattern in every block from fm_model, broadcast to the patterns which[q],
    the records in the order (pattern, block, slot).  -> (occ npat x count int64, lo npat x count, the first max_hits records, total)"""
    from fm_model import fm_model
    which = np.asarray(which, dtype=np.int64)
    count = len(sas)
    lo_d = np.zeros((len(distinct), count), np.int64)
    occ_d = np.zeros((len(distinct), count), np.int64)
    for b in range(count):
        r = np.array(fm_model(Ls[b], origins[b], distinct), dtype=np.int64).reshape(len(distinct), 2)
        lo_d[:, b], occ_d[:, b] = r[:, 0], r[:, 1] - r[:, 0]
    occ, lo = occ_d[which], lo_d[which]
    total = int(occ.sum())
    flat_occ, flat_lo = occ.reshape(-1), lo.reshape(-1)
    keep = total if max_hits is None else min(total, max_hits)
    ends = np.cumsum(flat_occ)
    pairs_needed = int(np.searchsorted(ends, keep, side="left")) + 1 if keep else 0
    o, l = flat_occ[:pairs_needed], flat_lo[:pairs_needed]
    pair = np.repeat(np.arange(pairs_needed), o)[:keep]
    first = (np.cumsum(o) - o)
    inside = np.arange(len(pair)) - first[pair] if keep else np.zeros(0, np.int64)
    rec = np.zeros(keep, HIT_DTYPE)
    q, b = pair // count, pair % count
    rec["pattern"], rec["block"], rec["slot"] = q, b, l[pair] + inside
    sizes = np.array([len(s) for s in sas], dtype=np.int64)
    flat = np.concatenate([np.asarray(s, dtype=np.int64) for s in sas])
    starts = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    rec["position"] = flat[starts[b] + rec["slot"]] if keep else 0
    return occ, lo, rec, total


def equal_bytes_block(n, byte=97):
    """-> (suffix array, L, origin) of byte^n: suffix n - 1 sorts first"""
    return np.arange(n - 1, -1, -1, dtype=np.int64), np.full(n, byte, np.uint8), n - 1


def find_case(name):
    """Part C.  -> dict(texts or None, sas, Ls, origins, distinct, which, max_hits, faults): the blocks' structures from sorted suffixes, at
    most 64 distinct patterns (present, absent, empty) and the index of the distinct pattern every pattern is."""
    from fm_find_model import block_structures
    rng = np.random.default_rng({"c1_full_list": 51, "c2_64bit": 52, "c3_fourth_round": 53}[name])
    if name == "c1_full_list":
        texts = [rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n) for n in (1500, 2100, 1800)]
        parts = [block_structures(t) for t in texts]
        cat = np.concatenate(texts)
        distinct = [b""]
        for k in range(40):  # present somewhere
            a, m = int(rng.integers(0, len(cat) - 8)), int(rng.integers(4, 7))
            distinct.append(bytes(cat[a:a + m]))
        for k in range(23):  # absent
            p = bytearray(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(rng.integers(1, 7))).tobytes())
            p[int(rng.integers(0, len(p)))] = ord("N")
            distinct.append(bytes(p))
        npat = 22017
        which = rng.integers(1, 64, size=npat)
        which[rng.choice(npat - 1, size=20, replace=False)] = 0  # the empty pattern: every slot of every block, twenty times
        which[npat - 1] = 1                                      # the last row's three pairs have hits
        max_hits = None
        faults = ("bases_zero", "full_last_chunk")
    elif name == "c2_64bit":
        n = 1 << 17
        parts = [equal_bytes_block(n)]
        distinct = [b"a", b"b", b"ba", b"c", b"a" * 300]
        npat = 70000
        which = rng.integers(1, 4, size=npat)
        which[rng.choice(npat, size=40000, replace=False)] = 0
        which[:3] = (1, 0, 2)
        which[rng.choice(np.flatnonzero(which != 0)[3:], size=5, replace=False)] = 4
        max_hits = 4096
        faults = ("bases_zero", "full_last_chunk", "sum32")
    else:
        t = rng.integers(60, 100, size=64, dtype=np.uint8)
        parts = [block_structures(t)]
        distinct = [bytes([c]) for c in range(50, 114)]
        npat = 262144 + 300
        which = rng.integers(0, 64, size=npat)
        max_hits = None
        faults = ("bases_zero", "full_last_chunk")
    return dict(sas=[np.asarray(p[0], dtype=np.int64) for p in parts], Ls=[u8(p[1]) for p in parts], origins=[int(p[2]) for p in parts],
                distinct=distinct, which=which, max_hits=max_hits, faults=faults, npairs=npat * len(parts))


FIND_CASES = ("c1_full_list", "c2_64bit", "c3_fourth_round")


def broadcast(occ_d, recs_d, which, max_hits=None):
    """The answer for the patterns which[q] from the answer for the distinct ones: occ_d is ndistinct x count, recs_d their records in the order
    (pattern, block) with occ_d[d, b] records per pair.  -> (occ npat x count, the first max_hits records with `pattern` renumbered, total)"""
    occ_d = np.asarray(occ_d, dtype=np.int64)
    which = np.asarray(which, dtype=np.int64)
    count = occ_d.shape[1]
    start_d = np.cumsum(occ_d.reshape(-1)) - occ_d.reshape(-1)
    occ = occ_d[which]
    total = int(occ.sum())
    keep = total if max_hits is None else min(total, max_hits)
    src = (which[:, None] * count + np.arange(count)[None, :]).reshape(-1)
    cnt = occ.reshape(-1)
    first = np.cumsum(cnt) - cnt
    pair = np.repeat(np.arange(len(cnt)), cnt)[:keep]
    recs = recs_d[start_d[src[pair]] + np.arange(keep) - first[pair]].copy() if keep else recs_d[:0].copy()
    recs["pattern"] = pair // count
    return occ, recs, total


C1_TEXT_SIZES = (1500, 2100, 1800)
NEAR_NODE_LIMIT = 5  # k = 0, one-bit classes: a pair's tree is a path of one node per suffix of the pattern that occurs; 5 cuts what matches 5 bytes


def c1_texts():
    rng = np.random.default_rng(51)  # (find_case draws the same bytes first)
    return [rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n) for n in C1_TEXT_SIZES]


def near_fast(texts, distinct, which, k, node_limit=None, max_hits=None):
    """near's answer for patterns given as byte strings (one-bit classes), through near_model on the distinct ones.
    -> (occ, records, total, cut)"""
    from fm_near_model import exact_classes, near_model
    occ_d, recs_d, _, _, nodes_d = near_model(texts, [exact_classes(p) for p in distinct], k, node_limit)
    occ, recs, total = broadcast(occ_d, recs_d, which, max_hits)
    cut = int((nodes_d[np.asarray(which)] > node_limit).sum()) if node_limit is not None else 0
    return occ, recs, total, cut, nodes_d[np.asarray(which)]


def seams_case():
    """Part C5: 24 blocks of about 100 bytes ACGT behind a piece of 50, 2800 patterns of 2 .. 6 bytes out of 64 distinct ones: 67 200 pairs"""
    rng = np.random.default_rng(55)
    sym = np.frombuffer(b"ACGT", np.uint8)
    blocks = [rng.choice(sym, size=int(rng.integers(80, 130))) for _ in range(24)]
    prev = rng.choice(sym, size=50)
    whole = np.concatenate([prev] + blocks)
    borders = np.cumsum([len(prev)] + [len(b) for b in blocks])[:-1]
    distinct = [b"A"]  # too short for a seam
    for k in range(50):  # cut across a border
        at, m = int(borders[k % len(borders)]), int(rng.integers(2, 7))
        a = at - int(rng.integers(1, m))
        distinct.append(bytes(whole[a:a + m]))
    for k in range(13):
        distinct.append(bytes(rng.choice(sym, size=int(rng.integers(2, 5)))) + (b"N" if k & 1 else b""))
    which = rng.integers(0, 64, size=2800)
    which[-1] = 1
    return dict(blocks=blocks, prev=prev, distinct=distinct, which=which, npairs=2800 * 24, faults=("bases_zero", "full_last_chunk"))


def seams_fast(blocks, prev, distinct, which, max_hits=None):
    from fm_seams_model import seams_model
    occ_d, recs_d, _ = seams_model([bytes(u8(b)) for b in blocks], distinct, bytes(u8(prev)), fast=True)
    return broadcast(occ_d, recs_d, which, max_hits)


def list_by_scan(occ, fault=None, max_hits=None):
    """what a list filled from the find family's scan looks like, without the records' own content: -> (for every listed place the pair that
    owns it and its rank inside the pair, total).  The emit kernels of near and seams store record j of pair p at offset[p] + j while that is
    below min(total, max_hits); a later store wins (the order of the device is not defined there, but then the list is wrong anyway)."""
    occ = np.asarray(occ, dtype=np.int64).reshape(-1)
    offsets, total = find_scan(occ, fault)
    nhits = int(min(total, int(occ.sum()) + 1 if max_hits is None else max_hits))  # (no limit: the buffer of a test that expects them all)
    pair = np.repeat(np.arange(len(occ)), occ)
    first = np.cumsum(occ) - occ
    inside = np.arange(len(pair)) - first[pair]
    at = offsets[pair].astype(np.int64) + inside
    ok = (at >= 0) & (at < nhits)
    owner, rank = np.full(nhits, -1, np.int64), np.full(nhits, -1, np.int64)
    owner[at[ok]], rank[at[ok]] = pair[ok], inside[ok]
    return owner, rank, total


# ---- locate and extract builds (part D) ---------------------------------------------------------------------------------------------------------------

D_TOTALS = {"per2": (1 << 20) + 1025, "per4": 3 * (1 << 20) + 5}
D_STEP = 32


def d_text(name):
    return np.random.default_rng(60 + D_TOTALS[name] % 7).integers(0, 256, size=D_TOTALS[name], dtype=np.uint8)


def loc_marks(sa, step):
    """the rows + 1 mark words of a locate structure: marked slots (SA[x] % step == 0) in front of every row of LOC_ROW slots, and their number"""
    marked = np.asarray(sa, dtype=np.int64) % step == 0
    rows = div_up(len(marked), LOC_ROW)
    per_row = np.add.reduceat(marked.astype(np.int64), np.arange(0, len(marked), LOC_ROW))
    assert len(per_row) == rows
    return np.concatenate([[0], np.cumsum(per_row)]).astype(np.uint32)


def loc_marks_by_scan(sa, step, fault=None):
    """the same the way k_loc_rows and k_loc_scan make them: a stretch of `per` rows for each of SPINE threads"""
    assert fault in (None, "per_one")
    marked = np.asarray(sa, dtype=np.int64) % step == 0
    rows = div_up(len(marked), LOC_ROW)
    marks = np.zeros(rows + 1, np.int64)
    marks[:rows] = np.add.reduceat(marked.astype(np.int64), np.arange(0, len(marked), LOC_ROW))
    per = 1 if fault == "per_one" else div_up(rows, SPINE)
    r0 = np.minimum(np.arange(SPINE) * per, rows)
    r1 = np.minimum(r0 + per, rows)
    sums = np.array([marks[a:b].sum() for a, b in zip(r0, r1)])
    run = np.cumsum(sums) - sums
    out = marks.copy()
    for t in range(SPINE):
        v = marks[r0[t]:r1[t]]
        out[r0[t]:r1[t]] = run[t] + np.cumsum(v) - v
    out[rows] = sums.sum()
    return out.astype(np.uint32)


def ibwt_table_by_scan(L, fault=None):
    """the tile table of the structure builds' front part (fm_walks_device): per tile of IB_TILE symbols the count of every symbol in front of it,
    through k_ibwt_scan_a/b/c's chunks.  Every successor entry, and so every walk, is computed from it."""
    L = u8(L)
    ntiles = div_up(len(L), IB_TILE)
    h = np.bincount((np.arange(len(L)) // IB_TILE) * 256 + L, minlength=ntiles * 256).reshape(ntiles, 256)
    return chunk_scan(h, IB_MAX_CHUNKS, fault)


def ibwt_table(L):
    L = u8(L)
    ntiles = div_up(len(L), IB_TILE)
    h = np.bincount((np.arange(len(L)) // IB_TILE) * 256 + L, minlength=ntiles * 256).reshape(ntiles, 256)
    return np.cumsum(h, axis=0) - h


# ---- super-maximal matches (part E) ---------------------------------------------------------------------------------------------------------------------

E_COPIES, E_QUERY, E_MAX_LEN, E_MIN_LEN = 88, 3000, 1000, 1


def smem_text():
    """the text of test_gpu_sa_match.depth_case(1 << 16): 2^16 bytes ACGT"""
    t = np.random.default_rng(1 << 16).integers(65, 69, size=1 << 16, dtype=np.uint8)
    return np.frombuffer(bytes(t).translate(bytes.maketrans(b"ABCD", b"ACGT")), np.uint8)


def smem_query():
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(70).integers(0, 4, size=E_QUERY)]


def smem_repeat(one, qlen, copies):
    """the records of `copies` equal queries back to back from those of one: rows (at, len, lo, hi), `at` shifted by the query's length"""
    one = np.asarray(one, dtype=np.int64).reshape(-1, 4)
    out = np.tile(one, (copies, 1))
    out[:, 0] += np.repeat(np.arange(copies) * qlen, len(one))
    return out


def smem_list_by_scan(flag_positions, Q, max_hits, fault=None):
    """k_sa_smem_scan_a/b and k_sa_smem_emit on the flagged positions: -> (the flagged position stored at every place of the list, -1 where
    nothing is stored; total)"""
    assert fault in (None, "second_from_zero")
    flag = np.zeros(div_up(Q, SM_TILE) * SM_TILE, np.int64)
    flag[np.asarray(flag_positions, dtype=np.int64)] = 1
    ntiles = div_up(Q, SM_TILE)
    tile_sum = flag.reshape(ntiles, SM_TILE).sum(axis=1)
    tile_at, run = np.zeros(ntiles, np.int64), 0
    for c in range(0, ntiles, SM_TRIP):
        v = tile_sum[c:c + SM_TRIP]
        tile_at[c:c + SM_TRIP] = (run & 0xFFFFFFFF) + np.cumsum(v) - v
        run = (0 if fault == "second_from_zero" else run) + int(v.sum())
    total = run
    nhits = min(total, max_hits)
    g = np.flatnonzero(flag)
    inside = np.arange(len(g)) - (np.cumsum(tile_sum) - tile_sum)[g // SM_TILE]
    at = tile_at[g // SM_TILE] + inside
    listed = np.full(nhits, -1, np.int64)
    ok = (tile_at[g // SM_TILE] < nhits) & (at < nhits)
    listed[at[ok]] = g[ok]
    return listed, total


def flat_patterns(distinct, which):
    """the patterns distinct[which[q]] back to back and their lengths, without a Python loop over the patterns"""
    parts = [u8(p) for p in distinct]
    lens_d = np.array([len(p) for p in parts], dtype=np.int64)
    cat = np.concatenate(parts + [np.zeros(1, np.uint8)])
    start_d = np.cumsum(lens_d) - lens_d
    which = np.asarray(which, dtype=np.int64)
    lens = lens_d[which]
    first = np.cumsum(lens) - lens
    q = np.repeat(np.arange(len(which)), lens)
    return cat[start_d[which[q]] + np.arange(int(lens.sum())) - first[q]], lens
