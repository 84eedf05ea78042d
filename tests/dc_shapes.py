"""Byte arrays built to reach every level of the distance-coding scans (csrc/dc.hip, the k_pdc_* pass of csrc/packed.hip).  No test, no GPU.

The constants the shapes depend on are read out of the two sources; the level arithmetic of dc_encode_device and packed_dc_device is restated
below, and every builder places its symbols by that arithmetic.  tests/test_dc_shapes_host.py checks on the CPU that the levels a case is named
after are the ones it reaches and that the oracle alone round-trips it; tests/test_gpu_dc_levels.py runs the same cases through the kernels."""
import os
import re
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dark_amd", "csrc")


# ---- constants, out of the sources -----------------------------------------------------------------------------------------------------
def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _constants(text, where):
    """every `constexpr <integer type> NAME = <expression>;` of the file, evaluated in order (an expression may name earlier constants)"""
    out = {}
    for name, expr in re.findall(r"constexpr\s+(?:int|uint32_t|size_t|unsigned)\s+(\w+)\s*=\s*([^;]+);", text):
        if not re.fullmatch(r"[\w\s+\-*/()]+", expr):
            continue
        try:
            out[name] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(out)))
        except Exception:
            pass
    if not out:
        raise RuntimeError("no constants found in " + where)
    return out


def _need(pattern, text, what):
    m = re.search(pattern, text)
    if m is None:
        raise RuntimeError("tests/dc_shapes.py no longer finds %s in the source: restate it here" % what)
    return m


_DC_SRC, _PK_SRC = _read("dc.hip"), _read("packed.hip")
_DC, _PK = _constants(_DC_SRC, "dc.hip"), _constants(_PK_SRC, "packed.hip")
DC_TILE, DC_WAVES, DC_MAX_CHUNKS, DC_CARRY_BATCH = _DC["DC_TILE"], _DC["DC_WAVES"], _DC["DC_MAX_CHUNKS"], _DC["DC_CARRY_BATCH"]
PK_TILE, PDC_TILE, PDC_MAX_CHUNKS = _PK["PK_TILE"], _PK["PDC_TILE"], _PK["PDC_MAX_CHUNKS"]
# numbers the kernels spell as literals
DC_RUNSCAN_THREADS = int(_need(r"__launch_bounds__\((\d+)\)\s*void\s+k_dc_runscan", _DC_SRC, "k_dc_runscan's workgroup size").group(1))
_m = _need(r"per\s*=\s*\(nchunks\s*\+\s*(\d+)\)\s*/\s*(\d+)", _DC_SRC, "k_dc_carry_b's quarter length")
DC_QUARTERS = int(_m.group(2))
assert int(_m.group(1)) == DC_QUARTERS - 1
PK_SCAN_THREADS = int(_need(r"__launch_bounds__\((\d+)\)\s*void\s+k_pk_scan_u32", _PK_SRC, "k_pk_scan_u32's workgroup size").group(1))
PDC_STEP = int(_need(r"cb\s*<\s*m;\s*cb\s*\+=\s*(\d+)", _PK_SRC, "k_pdc_main's step").group(1))
# the single-block kernels walk R[p] = L[n-1-p]; a tile "of the walk" is a tile of R
_need(r"rev_at\([^)]*\)\s*\{\s*return\s+L\[n\s*-\s*1\s*-\s*p\];", _DC_SRC, "rev_at (the walk's direction)")
_need(r"init\[threadIdx\.x\]\s*=\s*fp\s*\?\s*n\s*-\s*fp\s*:\s*n", _DC_SRC, "k_dc_init (init = n - last)")
WALK_BACKWARDS = True


def div_up(a, b):
    return (a + b - 1) // b


# ---- level arithmetic -----------------------------------------------------------------------------------------------------------------
def single_levels(n):
    """dc_encode_device's launch arithmetic for a block of n positions"""
    ntiles = div_up(n, DC_TILE)
    tpc = div_up(ntiles, DC_MAX_CHUNKS)
    nchunks = div_up(ntiles, tpc)
    per_q = div_up(nchunks, DC_QUARTERS)
    quarters = [(min(q * per_q, nchunks), min(min(q * per_q, nchunks) + per_q, nchunks)) for q in range(DC_QUARTERS)]
    return dict(n=n, ntiles=ntiles, tpc=tpc, nchunks=nchunks, per_q=per_q, quarters=quarters,
                quarter_lens=[b - a for a, b in quarters],
                last_chunk_tiles=ntiles - (nchunks - 1) * tpc,
                partial_batch=tpc > DC_CARRY_BATCH and tpc % DC_CARRY_BATCH != 0,  # a full batch and then a short one inside a chunk
                rs_per=div_up(ntiles, DC_RUNSCAN_THREADS),
                last_tile_len=n - (ntiles - 1) * DC_TILE)


def pack_levels(total, m):
    """packed_dc_device's launch arithmetic for a pack of `total` positions and m runs"""
    ptiles = div_up(total, PK_TILE)
    rtiles = div_up(total, PDC_TILE)
    tpc = div_up(rtiles, PDC_MAX_CHUNKS)
    mtiles = div_up(m, PDC_TILE)
    nchunks = div_up(mtiles, tpc)
    return dict(total=total, m=m, ptiles=ptiles, rtiles=rtiles, tpc=tpc, mtiles=mtiles, nchunks=nchunks,
                full=nchunks == div_up(rtiles, tpc), last_chunk_tiles=mtiles - (nchunks - 1) * tpc,
                scan_iters=div_up(ptiles, PK_SCAN_THREADS))


def walk_tile(n, pos):
    """tile of the walk that position pos of L falls in"""
    return (n - 1 - pos) // DC_TILE if WALK_BACKWARDS else pos // DC_TILE


def walk_tile_range(n, t):
    """[lo, hi): the positions of L that tile t of the walk covers"""
    if WALK_BACKWARDS:
        return max(0, n - (t + 1) * DC_TILE), n - t * DC_TILE
    return t * DC_TILE, min(n, (t + 1) * DC_TILE)


def locate_tile(lv, t):
    chunk = t // lv["tpc"]
    quarter = min(chunk // lv["per_q"], DC_QUARTERS - 1)
    return dict(tile=t, chunk=chunk, in_chunk=t % lv["tpc"], quarter=quarter, in_quarter=chunk - lv["quarters"][quarter][0],
                thread=t // lv["rs_per"])


def locate(n, pos):
    """tile, chunk, quarter and runscan thread of the walk that handle position pos of L"""
    return locate_tile(single_levels(n), walk_tile(n, pos))


def run_starts(L):
    L = np.asarray(L)
    return np.flatnonzero(np.concatenate([[True], L[1:] != L[:-1]]))


def expected_used(L, m):
    """distances the reference's decoder reads for a block of m runs: all of them, but none when the block holds one symbol only (its
    "redundant alphabet" case fills the block from init alone)"""
    return m if m > 1 else 0


def where_is(L, key, index):
    """words for a failure message: entry `index` of output `key` of a single block -> its place in the walk"""
    n = len(L)
    if key == "init":
        hits = np.flatnonzero(np.asarray(L) == index)
        if len(hits) == 0:
            return "symbol %d does not occur" % index
        pos = int(hits[0])
    else:
        st = run_starts(L)
        if index >= len(st):
            return "run %d is past the block's %d runs" % (index, len(st))
        pos = int(st[index])
    at = locate(n, pos)
    return "position %d of L: walk tile %d, chunk %d (tile %d of it), quarter %d, runscan thread %d" % (
        pos, at["tile"], at["chunk"], at["in_chunk"], at["quarter"], at["thread"])


def crossing_kinds(lv, ta, tb):
    """which edges of the scans a carry from walk tile ta to walk tile tb (ta < tb, the symbol's rows empty in between) travels over"""
    a, b = locate_tile(lv, ta), locate_tile(lv, tb)
    k = set()
    if ta == tb:
        return k
    B = DC_CARRY_BATCH
    if tb == ta + 1:
        k.add("tile_edge")
        if a["chunk"] == b["chunk"] and b["in_chunk"] % B == 0:
            k.add("batch_edge_in_chunk")
        if b["chunk"] == a["chunk"] + 1:
            k.add("chunk_edge")
        if b["thread"] == a["thread"] + 1:
            k.add("thread_edge")
    if b["chunk"] > a["chunk"]:
        if b["in_chunk"] >= B:
            k.add("chunk_edge_into_late_batch")
        if b["chunk"] == lv["nchunks"] - 1:
            k.add("into_last_chunk")
        if b["chunk"] == a["chunk"] + 1 and b["quarter"] == a["quarter"] + 1:
            k.add("quarter_edge")
        if b["chunk"] == a["chunk"] + 1 and b["quarter"] == a["quarter"] and b["in_quarter"] % B == 0:
            k.add("quarter_batch_edge")
        if b["quarter"] == DC_QUARTERS - 1 and a["quarter"] < b["quarter"]:
            k.add("into_fourth_quarter")
        if b["quarter"] >= a["quarter"] + 2:
            k.add("skip_quarter")
    if ta == 0 and tb == lv["ntiles"] - 1:
        k.add("whole_array")
    return k


def expected_kinds(lv):
    """the crossings a block of these levels has at all"""
    k = set()
    if lv["ntiles"] >= 2:
        k |= {"tile_edge", "whole_array", "thread_edge"}
    if lv["nchunks"] >= 2:
        k |= {"chunk_edge", "into_last_chunk"}
    if lv["tpc"] > DC_CARRY_BATCH:
        k |= {"batch_edge_in_chunk", "chunk_edge_into_late_batch"}
    if lv["quarter_lens"][1] > 0:
        k.add("quarter_edge")
    if lv["per_q"] > DC_CARRY_BATCH:
        k.add("quarter_batch_edge")
    if lv["quarter_lens"][DC_QUARTERS - 1] > 0:
        k.add("into_fourth_quarter")
    if lv["quarter_lens"][2] > 0:
        k.add("skip_quarter")
    return k


def _targets(lv, rng):
    """(kind, ta, tb) in walk tiles, derived from the levels: one or more carriers per edge the scans have at this size"""
    nt, tpc, nch, per_q, B = lv["ntiles"], lv["tpc"], lv["nchunks"], lv["per_q"], DC_CARRY_BATCH
    out = []
    last = nt - 1
    roomy_last = last if lv["last_tile_len"] >= 64 or nt == 1 else last - 1  # a ragged last tile of one position holds one carrier only
    if nt >= 2:
        out.append(("whole_array", 0, last))
        for k in sorted({1, nt // 2, max(1, last - 1)}):
            t = k * lv["rs_per"]
            if 1 <= t <= roomy_last:
                out.append(("thread_edge", t - 1, t))
    if nch >= 2:
        for c in sorted({1, nch // 3, nch // 2, nch - 1}):
            if 1 <= c < nch and c * tpc <= roomy_last:
                out.append(("chunk_edge", c * tpc - 1, c * tpc))
        out.append(("into_last_chunk", (nch - 2) * tpc, roomy_last if roomy_last >= (nch - 1) * tpc else last))
    if tpc > B:
        for c in sorted({0, nch // 2, nch - 2}):
            for kb in range(1, div_up(tpc, B)):
                if 0 <= c < nch and c * tpc + kb * B <= roomy_last and kb * B < (lv["last_chunk_tiles"] if c == nch - 1 else tpc):
                    out.append(("batch_edge_in_chunk", c * tpc + kb * B - 1, c * tpc + kb * B))
        for c in sorted({1, nch // 2, nch - 2}):
            if 1 <= c < nch - (1 if lv["last_chunk_tiles"] <= B else 0):
                out.append(("chunk_edge_into_late_batch", c * tpc - 1, c * tpc + B))
                out.append(("chunk_edge_into_late_batch", max(0, (c - 3) * tpc), c * tpc + tpc - 1))
    for q in range(1, DC_QUARTERS):
        g0, g1 = lv["quarters"][q]
        if g1 > g0:
            tb = g0 * tpc
            if tb > roomy_last:
                tb = last
            out.append(("quarter_edge", g0 * tpc - 1, tb))
            out.append(("quarter_edge", (g0 - 1) * tpc, min(tb + tpc - 1, roomy_last) if tb != last else last))
    if per_q > B:
        for q in range(DC_QUARTERS):
            g0, g1 = lv["quarters"][q]
            for kb in (1, (g1 - g0 - 1) // B):
                g = g0 + kb * B
                if kb >= 1 and g < g1 and g * tpc <= roomy_last:
                    out.append(("quarter_batch_edge", g * tpc - 1, g * tpc))
    g0, g1 = lv["quarters"][DC_QUARTERS - 1]
    if g1 > g0:
        tb = (g1 - 1) * tpc
        out.append(("into_fourth_quarter", max(0, g0 * tpc - 1), tb if tb <= roomy_last else last))
        if lv["quarter_lens"][2] > 0:
            out.append(("skip_quarter", int(rng.integers(0, lv["quarters"][0][1] * tpc)), g0 * tpc if g0 * tpc <= roomy_last else last))
    elif lv["quarter_lens"][2] > 0:
        out.append(("skip_quarter", 0, min(lv["quarters"][2][0] * tpc, last)))
    return [(k, a, b) for k, a, b in out if 0 <= a < b <= last]


# ---- single blocks ---------------------------------------------------------------------------------------------------------------------
BG = (0x61, 0x62)          # the two background symbols of the sparse cases
MIN_CARRIERS = 24


def _seed(name):
    return zlib.crc32(name.encode())


class _Placer:
    """puts single bytes into L, never twice at one position and (where the range allows) never next to another placed byte"""

    def __init__(self, L, rng):
        self.L, self.rng, self.used = L, rng, {}

    def put(self, lo, hi, sym):
        if hi - lo <= 4:
            cands = [p for p in range(lo, hi) if p not in self.used]
            if not cands:
                return None
            p = cands[0]
        else:
            for _ in range(200):
                p = int(self.rng.integers(lo, hi))
                if p not in self.used and p - 1 not in self.used and p + 1 not in self.used:
                    break
            else:
                return None
        self.used[p] = self.L[p]
        self.L[p] = sym
        return p

    def undo(self, p):
        self.L[p] = self.used.pop(p)


def build_sparse(n, variant, name):
    """two-symbol background (variant "alt": strictly alternating, so every position is a run; "runs": runs of 3 to 5) with rare symbols on top,
    each in exactly two tiles of the walk (a single-tile block: twice in its one tile)"""
    lv = single_levels(n)
    rng = np.random.default_rng(_seed(name))
    if variant == "alt":
        L = (BG[0] + (np.arange(n) & 1)).astype(np.uint8)
    else:
        lens = rng.integers(3, 6, size=n // 3 + 2)
        L = np.repeat((BG[0] + (np.arange(len(lens)) & 1)).astype(np.uint8), lens)[:n].copy()
    rest = [s for s in range(255) if s not in BG]
    rng.shuffle(rest)
    pool = [0xFF] + rest   # 0xFF first: it carries over the whole array
    placer = _Placer(L, rng)
    carriers = []
    nt = lv["ntiles"]

    def place(kind, tiles):
        sym = pool[len(carriers)]
        pos = []
        for t in tiles:
            lo, hi = walk_tile_range(n, t)
            p = placer.put(lo, hi, sym)
            if p is None:
                for q in pos:   # no room (a ragged last tile of one position)
                    placer.undo(q)
                return False
            pos.append(p)
        carriers.append(dict(sym=sym, kind=kind, tiles=tuple(tiles), pos=tuple(pos)))
        return True

    targets = _targets(lv, rng)
    if nt == 1:
        targets = [("same_tile", 0, 0)]
    for kind, ta, tb in targets:
        place(kind, (ta, tb))
    # a symbol that occurs once only (its init and nothing else), one that lives in the last tile of the walk only (ragged unless r = 0)
    place("once", (int(rng.integers(0, nt)),)) or place("once", (0,))
    ragged_only = lv["last_tile_len"] >= 4 and place("last_tile_only", (nt - 1, nt - 1))
    while len(carriers) < MIN_CARRIERS + 2:
        if nt >= 3:
            ta = int(rng.integers(0, nt - 2))
            tb = int(rng.integers(ta + 1, nt - 1))
        elif nt == 2:
            ta, tb = 0, (1 if lv["last_tile_len"] >= 64 else 0)
        else:
            ta = tb = 0
        if not place("filler", (ta, tb)):
            break
    return dict(name=name, builder="sparse_" + variant, L=L, n=n, levels=lv, carriers=carriers, ragged_only=bool(ragged_only), stretches=[])


def _stretch_plan(lv, rng):
    """(first tile, tiles) of stretches of whole tiles inside one run, their ends on the scans' edges; at least one busy tile between two"""
    nt, tpc, nch, B = lv["ntiles"], lv["tpc"], lv["nchunks"], DC_CARRY_BATCH
    wants = []  # (edge tile, "end" | "start")
    for c in sorted({1, nch // 4, nch // 2, (3 * nch) // 4, nch - 1}):
        if 1 <= c < nch:
            wants.append((c * tpc, "end" if c & 1 else "start"))
    if tpc > B:
        for c in sorted({0, nch // 3, nch - 2}):
            if 0 <= c < nch:
                wants.append((c * tpc + B, "end"))
                wants.append((c * tpc + B, "start") if c != nch // 3 else (c * tpc + tpc - 1, "end"))
    for q in range(1, DC_QUARTERS):
        g0, g1 = lv["quarters"][q]
        if g1 > g0:
            wants.append((g0 * tpc, "end" if q != 2 else "start"))
    for k in sorted({nt // (3 * lv["rs_per"]), (2 * nt) // (3 * lv["rs_per"])}):
        if k >= 1:
            wants.append((k * lv["rs_per"] + 1, "end"))   # over a thread edge of the run scan
    wants.append((nt, "end"))  # up to the array's last tile (ragged unless r = 0)
    taken = []
    for edge, side in wants:
        k = int(rng.integers(3, 21))
        k = min(k, max(1, nt - 2))
        s = edge - k if side == "end" else edge
        s = max(1, s)   # tile 0 always holds a run start: position 0
        e = min(nt, s + k)
        if e - s < (3 if nt >= 5 else 1) or any(not (e + 1 <= a or b + 1 <= s) for a, b in taken):
            continue
        taken.append((s, e))
    return sorted(taken)


def build_whole_runs(n, name):
    """busy tiles with stretches of 3 to 20 whole tiles inside one run between them (k_dc_summary counts no run start in those: tile_runs = 0)"""
    lv = single_levels(n)
    rng = np.random.default_rng(_seed(name))
    T = DC_TILE
    R = (0x63 + rng.integers(0, 6, size=n)).astype(np.uint8)       # the array in walk order; six symbols: tiles that keep the bitmap
    plan = _stretch_plan(lv, rng)
    edges = [0] + [e for _, e in plan]
    for i, (s, e) in enumerate(plan):
        if i & 1:   # the busy region before every second stretch has three symbols: with the run's byte the four-symbol route
            lo = edges[i] * T
            R[lo:s * T] = 0x63 + (R[lo:s * T] - 0x63) % 3
    stretches = []
    for i, (s, e) in enumerate(plan):
        byte = (0x63 + i % 6) if i % 3 else (0xF0 + i % 16)       # a symbol of the busy tiles, or one of its own (0xFF among them)
        if i == 2:
            byte = 0xFF
        lo = s * T - int(rng.integers(1, 70))
        hi = min(n, e * T + int(rng.integers(0, 70)))
        R[lo:hi] = byte
        if R[lo - 1] == byte:
            R[lo - 1] = 0x63 if byte != 0x63 else 0x64
        stretches.append(dict(first=s, tiles=e - s, byte=byte))
    L = np.ascontiguousarray(R[::-1]) if WALK_BACKWARDS else R
    return dict(name=name, builder="whole_runs", L=L, n=n, levels=lv, carriers=[], ragged_only=False, stretches=stretches)


def build_random256(n, name):
    rng = np.random.default_rng(_seed(name))
    return dict(name=name, builder="random256", L=rng.integers(0, 256, size=n, dtype=np.uint8), n=n, levels=single_levels(n), carriers=[],
                ragged_only=False, stretches=[])


# The sizes are the ones the levels change shape at with the constants as they are: 2 MiB (one tile per chunk ends), 4 MiB (one tile per
# runscan thread ends), 16 MiB (a chunk gets a second batch).  They are fixed here, not derived: tests/test_dc_shapes_host.py names the level
# that drops out when a constant in the sources moves, instead of the shapes silently moving along (and past the GPU test's context).
SINGLE_TILES = (1, 2, 3, 5, 511, 512, 1024, 4096)
SINGLE_REST = (0, 1, 4095)
RANDOM_TILES = (512, 1024)
_BUILDERS = {"sparse_alt": lambda n, name: build_sparse(n, "alt", name), "sparse_runs": lambda n, name: build_sparse(n, "runs", name),
             "whole_runs": build_whole_runs, "random256": build_random256}


def single_case_ids():
    """(builder, tiles, r) of every single-block case.  Random bytes only at the two shapes where one tile per chunk and one tile per
    runscan thread end; the largest shape only one past its last full tile and without random bytes (the oracle needs seconds for those)."""
    out = []
    for tiles in SINGLE_TILES:
        for r in SINGLE_REST:
            if tiles == SINGLE_TILES[-1] and r != 1:
                continue
            for b in ("sparse_alt", "sparse_runs", "whole_runs", "random256"):
                if b == "random256" and tiles not in RANDOM_TILES:
                    continue
                out.append((b, tiles, r))
    return out


def single_case(builder, tiles, r):
    n = tiles * DC_TILE + r
    return _BUILDERS[builder](n, "%s-%dx%d+%d" % (builder, tiles, DC_TILE, r))


# ---- packs -----------------------------------------------------------------------------------------------------------------------------
def no_equal_neighbours(rng, k, sigma=5, base=0x61):
    """k bytes over sigma symbols, no two neighbours equal: every position starts a run"""
    return (base + np.cumsum(rng.integers(1, sigma, size=k)) % sigma).astype(np.uint8)


def long_runs(rng, k, lo=500, hi=3000, sigma=5, base=0x61):
    lens = rng.integers(lo, hi, size=k // lo + 2)
    return np.repeat(no_equal_neighbours(rng, len(lens), sigma, base), lens)[:k].copy()


def pack_runs(blocks):
    """per block its number of runs and the global index of its first run (a run starts at every block head)"""
    ms = [len(run_starts(b)) for b in blocks]
    rb = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    return ms, rb


def _pack(name, blocks, **meta):
    blocks = [np.ascontiguousarray(b, dtype=np.uint8) for b in blocks]
    ms, rb = pack_runs(blocks)
    total = int(sum(len(b) for b in blocks))
    d = dict(name=name, blocks=blocks, total=total, ms=ms, rb=rb, levels=pack_levels(total, int(rb[-1])), carriers=[])
    d.update(meta)
    return d


def pack_tiny():
    """thousands of blocks of 1 to 3 bytes: one tile of runs and one step span many blocks; a stretch of blocks that are the same single byte"""
    rng = np.random.default_rng(_seed("tiny"))
    blocks = []
    for i in range(6000):
        k = int(rng.integers(1, 4))
        blocks.append(np.full(k, 0x71, np.uint8) if 2500 <= i < 2900 else (0x61 + rng.integers(0, 4, size=k)).astype(np.uint8))
    return _pack("tiny", blocks, same_byte=(2500, 2900))


def pack_prev_tail():
    """every symbol of a block last occurred among the last runs of the block before it: nothing may be carried in"""
    rng = np.random.default_rng(_seed("prev_tail"))
    order = rng.permutation(256)
    blocks = []
    for k, count in ((256, 12), (64, 40), (12, 150), (5, 200), (2, 150), (1, 60)):
        syms = order[:k].astype(np.uint8)
        for _ in range(count):
            head = np.repeat(rng.permutation(syms), rng.integers(1, 4, size=k))
            mid = syms[rng.integers(0, k, size=int(rng.integers(0, 3 * k + 1)))]
            tail = np.repeat(rng.permutation(syms), rng.integers(1, 3, size=k))
            blocks.append(np.concatenate([head, mid, tail]) if rng.integers(0, 4) else tail)
    return _pack("prev_tail", blocks)


HEAD_RESIDUES = (1, PDC_STEP - 1, PDC_STEP, PDC_TILE - 1, 0)


def pack_heads():
    """block heads at chosen run indices mod the tile of k_pdc_main; blocks without equal neighbours, so a run index is a position"""
    rng = np.random.default_rng(_seed("heads"))
    sizes, cur = [], 0
    for res in HEAD_RESIDUES:          # the first head is at 0; the block before residue 0 ends exactly at a multiple of the tile
        k = (res - cur) % PDC_TILE or PDC_TILE
        sizes.append(k)
        cur += k
    sizes.append(1000)
    sizes.append(2 * PDC_TILE + 500)   # from 1000 past a tile edge: crosses two tile edges
    sizes.append(777)
    return _pack("heads", [no_equal_neighbours(rng, k) for k in sizes])


def pack_all256():
    """blocks that hold all 256 byte values: k_pdc_final with f = 256"""
    rng = np.random.default_rng(_seed("all256"))

    def perms(reps, last=None):
        seq = np.concatenate([rng.permutation(256).astype(np.uint8) for _ in range(reps)])   # (equal neighbours at a seam: one longer run)
        if last is not None:   # the block's last run is `last`
            i = len(seq) - 256 + int(np.flatnonzero(seq[-256:] == last)[0])
            seq[i], seq[-1] = seq[-1], seq[i]
        return np.repeat(seq, rng.integers(1, 5, size=len(seq)))

    blocks = [perms(3), perms(2, last=0xFF), np.full(37, 0xFF, np.uint8), np.arange(256, dtype=np.uint8), perms(1, last=0xFF), perms(4),
              np.frombuffer(b"ab", np.uint8), np.arange(255, -1, -1, dtype=np.uint8)]
    return _pack("all256", blocks, ff_last=(1, 4), ff_only=2)


def _split(total, sizes):
    assert sum(sizes) < total
    return list(sizes) + [total - sum(sizes)]


def _place_pack_carriers(case, blk, pairs, rng):
    """rare symbols inside block blk (no equal neighbours: run index = position), each at two global tiles of runs"""
    blocks, off = case["blocks"], int(sum(len(b) for b in case["blocks"][:blk]))
    assert case["rb"][blk] == off
    b = blocks[blk]
    placer = _Placer(b, rng)
    for i, (kind, ta, tb) in enumerate(pairs):
        sym = 0xFF - i
        pos = []
        for t in (ta, tb):
            lo, hi = max(off, t * PDC_TILE) - off, min(off + len(b), (t + 1) * PDC_TILE) - off
            assert lo < hi, (kind, t)
            pos.append(placer.put(lo, hi, sym) + off)
        case["carriers"].append(dict(sym=sym, kind=kind, block=blk, tiles=(ta, tb), pos=tuple(pos)))


def pack_positions_all_runs(total, name, big=1):
    """a pack of `total` positions without equal neighbours (m = total: every chunk the launch can have is used), several blocks of 2 to 300 KiB,
    and in block `big` rare symbols whose two occurrences lie on either side of a chunk edge"""
    rng = np.random.default_rng(_seed(name))
    sizes = _split(total, [2048, 300 << 10, (77 << 10) + 1, 200 << 10, 150 << 10, 3 << 10])
    case = _pack(name, [no_equal_neighbours(rng, k) for k in sizes])
    lv = case["levels"]
    tpc = lv["tpc"]
    t0 = div_up(int(case["rb"][big]), PDC_TILE)
    t1 = int(case["rb"][big + 1]) // PDC_TILE - 1        # whole tiles of runs inside the block: t0 .. t1
    c0, c1 = div_up(t0, tpc), t1 // tpc
    pairs = []
    for c in sorted({c0 + 1, c0 + 2, (c0 + c1) // 2, (c0 + c1) // 2 + 1, c1 - 1, c1}):
        pairs.append(("chunk_edge", c * tpc - 1, c * tpc))
    odd = c0 + 1 + ((c0 + 1) & 1 == 0)
    pairs.append(("odd_chunk_to_later", odd * tpc, (odd + 3) * tpc + tpc - 1))
    pairs.append(("odd_chunk_to_next", odd * tpc + tpc - 1, (odd + 1) * tpc + tpc - 1))
    pairs.append(("many_chunks", t0, t1))
    _place_pack_carriers(case, big, pairs, rng)
    # one rare symbol in the block before as well: block `big` must not see it
    prev = case["blocks"][big - 1]
    prev[len(prev) - 3] = 0xFF
    case["cross_block"] = dict(sym=0xFF, block=big)
    return case


def pack_1m_runs():
    return pack_positions_all_runs(PDC_MAX_CHUNKS * PDC_TILE + 1, "1m+1_all_runs")      # tpc = 2, a short last chunk


def pack_1m_exact():
    return pack_positions_all_runs(PDC_MAX_CHUNKS * PDC_TILE, "1m_all_runs")           # tpc = 1 and all PDC_MAX_CHUNKS chunks


def pack_1m_long_runs():
    """the same total made of long runs: fewer tiles of runs than tiles per chunk, one chunk"""
    rng = np.random.default_rng(_seed("1m_long"))
    total = PDC_MAX_CHUNKS * PDC_TILE + 1
    sizes = _split(total, [2048, 300 << 10, (77 << 10) + 1, 200 << 10, 150 << 10, 3 << 10])
    return _pack("1m+1_long_runs", [long_runs(rng, k) for k in sizes])


def pack_4m():
    """two iterations of k_pk_scan_u32; tiles of positions without a run start around the position where its second iteration begins; a block
    of 1.5 MiB of runs that spans many chunks, with carriers across its chunk edges"""
    rng = np.random.default_rng(_seed("4m"))
    total = (PK_SCAN_THREADS + 1) * PK_TILE + 1
    sizes = _split(total, [(3 << 19) + 5, 200 << 10])
    blocks = [no_equal_neighbours(rng, k) for k in sizes]
    off2 = sizes[0] + sizes[1]
    seam = PK_SCAN_THREADS * PK_TILE
    empties = []
    b = blocks[2]
    # (first tile, last tile) of positions without a run start, the run's byte, and how far the run reaches into the tile after them.  The
    # first ends 49 positions before the end of the seam's tile, so that tile's few run starts and the sentinel behind them take the scan's carry
    for first, last, byte, into in ((seam // PK_TILE - 4, seam // PK_TILE - 1, 0x61, PK_TILE - 49), (600, 611, 0xFF, 17), (800, 802, 0x63, 0),
                                    (seam // PK_TILE - 40, seam // PK_TILE - 38, 0x62, 1)):
        lo, hi = first * PK_TILE - int(rng.integers(1, 30)) - off2, (last + 1) * PK_TILE + into - off2
        b[lo:hi] = byte
        for edge in (lo - 1, hi):
            if b[edge] == byte:
                b[edge] = 0x64 if byte != 0x64 else 0x65
        empties.append((first, last))
    case = _pack("4m+tile+1", blocks, empty_position_tiles=empties, seam_tile=seam // PK_TILE)
    tpc = case["levels"]["tpc"]
    t1 = sizes[0] // PDC_TILE - 1
    c1 = t1 // tpc
    pairs = [("chunk_edge", c * tpc - 1, c * tpc) for c in (1, 2, c1 // 2, c1)]
    pairs += [("odd_chunk_to_later", 3 * tpc + 1, 9 * tpc + tpc - 1), ("odd_chunk_to_next", 5 * tpc + tpc - 1, 6 * tpc + tpc - 1), ("many_chunks", 0, t1)]
    _place_pack_carriers(case, 0, pairs, rng)
    return case


PACKS = {"tiny": pack_tiny, "prev_tail": pack_prev_tail, "heads": pack_heads, "all256": pack_all256, "1m+1_all_runs": pack_1m_runs,
         "1m_all_runs": pack_1m_exact, "1m+1_long_runs": pack_1m_long_runs, "4m+tile+1": pack_4m}


def compact_texts():
    """about 3000 texts of 1 to 40 bytes over a small alphabet, repeated ones among them, and two of 70 KB (the pack handed to dev_packed_encode)"""
    rng = np.random.default_rng(_seed("compact"))
    texts = []
    for i in range(3000):
        k = int(rng.integers(1, 41))
        if i % 11 == 3 and texts:
            texts.append(texts[int(rng.integers(0, len(texts)))].copy())        # a repeated block
        elif i % 17 == 5:
            texts.append(np.full(k, 0x61 + i % 3, np.uint8))                      # one symbol
        elif i % 29 == 7:
            texts.append(np.where(rng.integers(0, 3, size=k) == 0, 0xFF, 0x61 + rng.integers(0, 2, size=k)).astype(np.uint8))   # may hold 0xFF
        elif i % 97 == 11:
            texts.append(np.full(k, 0xFF, np.uint8))
        else:
            texts.append((0x61 + rng.integers(0, 4, size=k)).astype(np.uint8))
    words = [bytes((0x61 + rng.integers(0, 4, size=int(rng.integers(2, 9)))).astype(np.uint8)) for _ in range(300)]
    for at in (1000, 2000):
        big = b" ".join(words[int(j)] for j in rng.integers(0, 300, size=20000))[:70000]
        texts.insert(at, np.frombuffer(big, np.uint8).copy())
    return texts
