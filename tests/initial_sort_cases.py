"""TEST HELPER: the cases of tests/test_gpu_initial_sort.py, shared with tests/test_initial_sort_model.py (which pins on the CPU what the grid and
each case are built for) and with the knob worker (tests/initial_sort_worker.py).  A case is a text, the byte offset of its first byte from an
aligned address, a code table with its (bits, spk), the carry's table or None, and narrow or not; expected() is tests/initial_sort_model.py's
answer, check() compares every output whole, guards included.

The (bits, spk, carry) grid is exactly what choose_prefix() of csrc/suffix_array.hip can hand the initial sort -- prefixes(), its arithmetic
restated.  Nothing outside it is ever run: the first pass's histogram and scatter derive their digit separately, and a disagreement on a
combination the product never uses would be a wild store in a test, not a finding about the product."""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

import initial_sort_model as M

FILL32 = 0xC3C3C3C3
PAD = 64
TILE = M.TILE
GRID_N = 3 * TILE + 85  # a few tiles, no multiple of 16; the last tile and the one in front of it stage byte by byte


# ---- what choose_prefix can choose ------------------------------------------------------------------------------------------------------------
def prefixes(bits):
    """-> (prefix lengths without the carry, with it) for an alphabet of `bits` bits per symbol"""
    full = 64 // bits
    ks = {full}
    for p in range(4, 8):  # the short prefixes: what four to seven radix passes cover
        k = (8 * p) // bits
        if 1 <= k < full:
            ks.add(k)
    for q in range(1, 9):  # a block of period q nearly everywhere: the passes that cover q symbols
        p = (q * bits + 7) // 8
        k = min(full, (8 * p) // bits)
        if k >= q:
            ks.add(k)
    return sorted(ks), sorted({min(k, 56 // bits) for k in ks})  # (the carried byte takes the key's low eight bits)


GRID = [(bits, spk, carry) for bits in range(1, 9) for carry in (False, True) for spk in prefixes(bits)[int(carry)]]


def category(n, bits, spk, carry, narrow):
    """the path a case is built to reach"""
    b, packed = bits * spk, M.packed_rule(n, bits, spk, carry)
    if b < 8:
        return "one pass, B < 8"
    if b == 8:
        return "one pass, B = 8"
    if packed:
        return "B = 32 packed" if b == 32 else "two packed passes" if b <= 16 else "packed with middle passes"
    if b <= 32:
        return "unpacked at most 32 bits"
    if b <= 40:
        return "33..40 bits, unpacked and narrow" if narrow else "33..40 bits, wide"
    return "more than 40 bits"


CATEGORIES = ("one pass, B < 8", "one pass, B = 8", "two packed passes", "packed with middle passes", "B = 32 packed", "33..40 bits, unpacked and narrow",
              "more than 40 bits")


# ---- alphabets, tables, texts -----------------------------------------------------------------------------------------------------------------
def alphabet(bits, rng):
    """2^bits byte values that are not contiguous, 0x00 and 0xFF among them"""
    m = 1 << bits
    if m == 256:
        return np.arange(256, dtype=np.uint8)
    inner = rng.choice(np.arange(1, 255), size=m - 2, replace=False)
    return np.sort(np.concatenate([[0, 255], inner])).astype(np.uint8)


def tables(bits, vals, free, rng):
    """-> (code, inv, zero): a random permutation of the values onto 0 .. 2^bits - 1 with its inverse, or (free) a random non-injective table and
    any inv; zero = a value of the alphabet whose code is 0"""
    m = 1 << bits
    if free:
        code = rng.integers(0, m, size=256).astype(np.uint8)
        zero = int(vals[rng.integers(0, len(vals))])
        code[zero] = 0
        twins = [int(v) for v in vals if int(v) != zero][:2]
        if len(twins) == 2:  # (from four values on; a random table of two bits is a permutation one time in eleven)
            code[twins[1]] = code[twins[0]]
        inv = rng.integers(0, 256, size=256).astype(np.uint8)
    else:
        code = np.zeros(256, np.uint8)
        code[vals] = rng.permutation(m).astype(np.uint8)
        zero = int(vals[np.flatnonzero(code[vals] == 0)[0]])
        inv = rng.integers(0, 256, size=256).astype(np.uint8)
        inv[code[vals]] = vals
    return code, inv, zero


def make_text(kind, n, vals, zero, spk, rng):
    """random: every byte drawn from the alphabet.  low: a short period with runs and a few flips, so that many full windows tie.  mixed: random
    with a periodic eighth in the middle.  Every text ends in at least spk copies of the symbol coded 0 and has an interior run of it longer than
    spk (as far as n has room): the zero-padded keys of the tail then tie with real ones"""
    if kind == "low":
        unit = vals[rng.integers(0, len(vals), size=int(rng.integers(2, 8)))]
        t = np.tile(unit, n // len(unit) + 1)[:n].copy()
        for _ in range(max(1, n // 1500)):
            a, length = int(rng.integers(0, n)), int(rng.integers(10, 300))
            t[a:a + length] = vals[rng.integers(0, len(vals))]
        flips = rng.integers(0, n, size=max(1, n // 400))
        t[flips] = vals[rng.integers(0, len(vals), size=len(flips))]
    else:
        t = vals[rng.integers(0, len(vals), size=n)]
        if kind == "mixed":
            unit = vals[rng.integers(0, len(vals), size=5)]
            t[n // 2:n // 2 + n // 8] = np.tile(unit, n // 40 + 1)[:n // 8]
    if n > 4 * (spk + 5):
        t[5], t[6] = vals[0], vals[-1]  # 0x00 and 0xFF occur
        t[n // 3:n // 3 + spk + 5] = zero
    t[n - min(spk + 2, n // 2):] = zero
    return np.ascontiguousarray(t, dtype=np.uint8)


def build(name, n, bits, spk, carry, narrow, kind="random", free=False, offset=0, text_seed=None):
    """text_seed: cases that share it (and bits, spk, kind, free, n) share their text and tables, whatever their offset, carry and narrow"""
    seed = zlib.crc32(repr((text_seed if text_seed is not None else name, n, bits, spk, kind, free)).encode())
    rng = np.random.default_rng(seed)
    vals = alphabet(bits, rng)
    code, inv, zero = tables(bits, vals, free, rng)
    text = make_text(kind, n, vals, zero, spk, rng)
    return SimpleNamespace(name=name, text=text, n=n, offset=offset, code=code, bits=bits, spk=spk, inv=inv if carry else None, narrow=narrow,
                           kind=kind, free=free, category=category(n, bits, spk, carry, narrow), want_packed=M.packed_rule(n, bits, spk, carry),
                           want_passes=M.passes_of(bits, spk), model_key=(seed, carry, narrow))


CASES = {}


def case(name, *args, **kw):
    CASES[name] = functools.lru_cache(maxsize=None)(functools.partial(build, name, *args, **kw))


# the whole grid at one size: narrow wherever the sort has at most 40 bits, and wide keys there as well
for i, (bits, spk, carry) in enumerate(GRID):
    for narrow in ((True, False) if bits * spk <= 40 else (False,)):
        case("grid_b%d_k%d_%s_%s" % (bits, spk, "carry" if carry else "plain", "narrow" if narrow else "wide"), GRID_N, bits, spk, carry, narrow,
             kind=("random", "low")[i % 2], free=bool((i // 2) % 2), text_seed=("grid", bits, spk, carry))
GRID_CASES = sorted(CASES)

# sizes and alignments: four grid points that between them are packed, narrow-unpacked and wide, with and without the carry
POINTS = {"packed_carry_narrow": (2, 16, True, True), "packed_plain_wide": (4, 6, False, False), "b40_plain_narrow": (8, 5, False, True),
          "b56_carry_wide": (8, 7, True, False)}
SIZES = (2, 3, 15, 16, 17, 63, 64, 65, 80, 81, 4095, 4096, 4097, 4175, 4176, 4177, 8191, 8192, 8193, 8271, 8272, 8273, 12289, 36865)
OFFSETS = (0, 1, 8, 15)


@functools.lru_cache(maxsize=None)
def sized(point, n, offset=0):
    bits, spk, carry, narrow = POINTS[point]
    return build("%s_n%d_at%d" % (point, n, offset), n, bits, spk, carry, narrow, kind=("random", "low")[n % 2], free=bool(n % 3 == 0), offset=offset,
                 text_seed=("sized", point))


# above the thresholds
N_PLANE = (1 << 20) + 1            # from 2^20 pairs on the passes leave a digit plane for the next histogram
N_TWO_TILES = (1 << 22) + 3 * TILE + 17  # 1028 tiles: a histogram workgroup walks two, and the last tile stages byte by byte behind a fast one
N_FAST_THEN_SLOW = (1 << 22) + 3 * TILE + 85  # 1028 tiles again, the last of 85 bytes: the last workgroup's two tiles are a fast one and the slow last one
N_PACKED_EDGE = 1 << 24            # bits = 8 with the carry: 8 + 24 bits fill the packed word; one byte more and they do not
LARGE = {
    "two_tiles_fast_then_slow": (N_FAST_THEN_SLOW, 8, 7, True, False, 0),
    "plane_unpacked_7_passes": (N_PLANE, 8, 7, True, False, 0),
    "plane_packed_4_passes": (N_PLANE, 2, 16, True, True, 0),
    "two_tiles_b56_aligned": (N_TWO_TILES, 8, 7, True, False, 0),
    "two_tiles_b56_offset_1": (N_TWO_TILES, 8, 7, True, False, 1),
    "two_tiles_packed_aligned": (N_TWO_TILES, 4, 8, True, True, 0),
    "two_tiles_packed_offset_1": (N_TWO_TILES, 4, 8, True, True, 1),
    "edge_packed_2_24": (N_PACKED_EDGE, 8, 4, True, True, 0),
    "edge_unpacked_2_24_plus_1": (N_PACKED_EDGE + 1, 8, 4, True, True, 0),
}


def large(name):
    n, bits, spk, carry, narrow, offset = LARGE[name]
    return build(name, n, bits, spk, carry, narrow, kind="mixed", offset=offset, text_seed=("large", n))


HANDOFF = ("grid_b4_k8_carry_narrow", "grid_b8_k5_carry_narrow")  # narrow and packed | narrow at 40 bits: the bucket starts carry information
# the knob worker's short list: one pass, packed in two / three / four passes (unpacked under DK_PACKED_SORT=0), 40 bits narrow, 56 and 64 bits
WORKER = ("grid_b1_k8_plain_narrow", "grid_b2_k8_carry_narrow", "grid_b4_k6_plain_wide", "grid_b2_k16_carry_narrow", "grid_b8_k5_carry_narrow",
          "grid_b8_k7_carry_wide", "grid_b8_k8_plain_wide")


# ---- call, expect, compare --------------------------------------------------------------------------------------------------------------------
def call(ctx, c, narrow=None):
    return ctx.dbg_dev_initial_sort(c.text, c.code, c.bits, c.spk, inv=c.inv, narrow=c.narrow if narrow is None else narrow, text_offset=c.offset, fill=0xC3,
                                    pad=PAD)


_models = {}


def expected(c, packed_sort=True, narrow=None, keep=True):
    """the model's answer (kept per text, tables and form: the alignment has no say)"""
    narrow = c.narrow if narrow is None else narrow
    key = (c.model_key[0], c.model_key[1], narrow, packed_sort)
    if key in _models:
        return _models[key]
    m = M.initial_sort_model(c.text, c.code, c.bits, c.spk, inv=c.inv, narrow=narrow, packed_sort=packed_sort)
    if keep:
        _models[key] = m
    return m


def guarded(a, dtype, pad=PAD):
    fill = np.frombuffer(b"\xc3" * 8, dtype=dtype)[0]
    return np.concatenate([np.full(pad, fill, dtype), np.asarray(a, dtype=dtype), np.full(pad, fill, dtype)])


def same(name, what, got, want):
    d = np.flatnonzero(got != want) if got.shape == want.shape else np.arange(1)
    assert got.dtype == want.dtype and got.shape == want.shape and not len(d), (name, what, len(d), int(d[0]), got[d[:2]], want[d[:2]])


def check(c, got, m, want_packed=None):
    """every output whole, the 0xC3 guards in front and behind included"""
    want_packed = c.want_packed if want_packed is None else want_packed
    assert (got["route"], got["passes"]) == (M.ROUTE_PACKED_PAIRS if want_packed else 0, c.want_passes), (c.name, hex(got["route"]), got["passes"], c.category)
    assert (m.route, m.passes) == (got["route"], got["passes"]), (c.name, "the model's route and passes")
    assert got["sorted_elements"] == m.sorted_elements & 0xFFFFFFFF and int(got["out"][3]) == 0, (c.name, got["out"])
    same(c.name, "keys", got["keys"], guarded(m.keys, m.keys.dtype))
    same(c.name, "sa", got["sa"], guarded(m.sa, np.uint32))
    if m.bwt is None:
        assert got["bwt"] is None and got["origin"] is None, c.name
    else:
        same(c.name, "bwt", got["bwt"], guarded(m.bwt, np.uint8))
        same(c.name, "origin", got["origin"], np.array([FILL32, m.origin, FILL32], np.uint32))
    if m.bucket_starts is None:
        assert got["bucket_starts"] is None, c.name
    else:
        same(c.name, "bucket_starts", got["bucket_starts"], m.bucket_starts)
