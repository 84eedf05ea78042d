// What a caller does with a suffix array, for one block or a pack: verify it, and search patterns in it.  Nothing in the
// reference corresponds (src/saca.rs stops at the array).  Conventions are those of lcp.hip: block b is text[off_b, e_b), its suffix array sits at
// sa[off_b, e_b) with entries local to the block, a single block is a pack of one; order as in src/saca.rs:105-113 -- no sentinel, a suffix that
// is a proper prefix of another sorts first.
//
// THE CHECK (Burkhardt, Kärkkäinen: Fast lightweight suffix array construction and checking, CPM 2003) is linear and compares no stretch of text:
//   k_sa_check_scatter  a thread per slot i: an entry >= n_b is a RANGE failure; otherwise isa[off_b + SA[i]] = i (plain stores; where two slots
//                       name one position either value may stay).  isa starts as NONE everywhere.
//   k_sa_check_missing  a thread per position p: isa[p] == NONE is a PERMUTATION failure.  n_b entries in range over n_b positions name every one
//                       of them exactly when they are a permutation.
//   k_sa_check_order    a thread per slot i >= 1 of a block without the two failures above, a = SA[i-1], b = SA[i]: T[a] < T[b] is in order,
//                       T[a] > T[b] is an ORDER failure; with equal bytes the pair is in order when a is the block's last position (the empty
//                       suffix behind it is the smallest), a failure when b is, and otherwise in order exactly when isa[a+1] < isa[b+1].
// Every block has three words (range, permutation, order), preset to all ones, that take the LOWEST failing slot / position / slot by atomicMin;
// the host reads them back once and the first kind that failed decides.  A wave reports one candidate per block it covers (its lowest: slots
// and positions rise with the lane), and only when it lies below what the word already holds -- an array of random entries fails at nearly
// every slot, and one atomic per failing lane on one address is the mistake of DESIGN.md section 4.1 item 9.
//
// THE SEARCH.  For pattern P of m bytes in block b, lo = slots whose suffix, cut to m bytes, is smaller than P; hi = slots where it is not
// greater: SA[lo, hi) are the occurrences.  Both are found by searching the slots for the end of a monotone predicate:
//   k_sa_search       a wave per pattern, 64-ary: over the candidate range [l, r) the lanes take 64 pivots spread evenly (the slots themselves
//                     once the range has at most 64), each lane compares its suffix with P, 16 bytes a step; one ballot and a population count
//                     give the next range, the two lanes at its borders the bytes matched there.
//   k_sa_search_long  patterns of more than lane_max bytes (a wave waits for its slowest lane: the reasoning of LCP_LANE_CAP): a wave per
//                     pattern, plain binary search, all 64 lanes compare 64 x 16 bytes of the one pivot a step, first difference by ballot.
// Every suffix between two slots that share kl and kr bytes with P shares min(kl, kr) with it, so a compare starts there (Manber, Myers 1993,
// without an LCP array); the ends of the block count 0.  The upper bound is a second search of the same kind behind lo, and is skipped when
// the suffix at lo does not start with P.
// Containment for an sa that is no suffix array: an entry >= n_b is the empty suffix and the text is not read at it, every compare stops at
// min(m, n_b - SA[slot]) whatever is "known", and every step shrinks the range: results are unspecified, but lo <= hi <= n_b.
//
// MATCHING STATISTICS.  For every position g of a batch of queries: the longest prefix of the window at g (at most
// max_len bytes, never past its query's end) that occurs in the block, and the search's range of that prefix.  A lower-bound search of the
// window ends between the two suffixes that share the most with it: the length is max(kl, kr), which the search above computes and drops.
//   k_sa_match       a wave per position: the window cut to lane_max bytes, by the 64-ary lane search; then the bracket of the matched prefix,
//                    a lower bound in front of the insertion slot and an upper bound behind it, from the bytes known at their borders
//   k_sa_match_long  only the positions whose match ran through the cut (len == lane_max < m): inside the range of the lane_max-byte prefix,
//                    lane_max bytes known, by the whole-wave compare and binary search.  The route is what MATCHED, not the window's length:
//                    windows are max_len long, most matches a few dozen bytes, and a lane's compare stops at its first difference.
//   k_sa_smem_mark   the super-maximal matches among them, a flag per position from len[g - 1] and len[g] inside one query;
//   k_sa_smem_scan_a/b, k_sa_smem_emit   the exclusive scan of the flags over tiles of 1024 positions (no atomics: every run gives the same
//                    bytes), the total to the mailbox, and the first min(total, max_hits) records {at, len, lo, hi}, a 16-byte store each.
#include <algorithm>

#include "context.hpp"
#include "device_util.hpp"

namespace dk {
namespace {

constexpr uint32_t SQ_NONE = 0xFFFFFFFFu;
// Patterns of more bytes than this go to k_sa_search_long.  UNMEASURED: the value and the reasoning are LCP_LANE_CAP's (lcp.hip) -- a lane's
// compare costs its wave as many steps as its longest member takes, 256 bytes = 16 steps.
constexpr int SA_SEARCH_LANE_MAX = 256;
constexpr uint32_t SQ_WAVES = 4;  // patterns per workgroup of the search kernels

typedef uint64_t __attribute__((aligned(1))) unaligned_u64;
typedef const unaligned_u64 __attribute__((address_space(1))) *gptr8;

// bytes x[k] == y[k] for k = 0, 1, ... below min(16, lim) (lce16 of lcp.hip for two arrays); the caller guarantees lim bytes behind both
__device__ __forceinline__ uint32_t match16(const uint8_t *__restrict__ x, const uint8_t *__restrict__ y, uint32_t lim) {
    if (lim >= 16) {
        const uint64_t lo = *(gptr8)(x) ^ *(gptr8)(y);
        if (lo) return static_cast<uint32_t>(__builtin_ctzll(lo)) >> 3;
        const uint64_t hi = *(gptr8)(x + 8) ^ *(gptr8)(y + 8);
        return hi ? 8u + (static_cast<uint32_t>(__builtin_ctzll(hi)) >> 3) : 16u;
    }
    uint32_t k = 0;
    while (k < lim && x[k] == y[k]) ++k;
    return k;
}

// ---- the check ------------------------------------------------------------------------------------------------------------------------------

// `value` rises with the lane and so does `b`: of the failing lanes of one block the first holds the lowest value.  Called by whole waves.
__device__ __forceinline__ void report_lowest(uint32_t *words, uint32_t kind, bool fail, uint32_t b, uint32_t value) {
    const int lane = threadIdx.x & 63;
    const uint64_t before = __ballot(fail) & lanemask_lt(lane);
    const int prev = before ? 63 - __builtin_clzll(before) : lane;  // the failing lane in front of this one
    const uint32_t prev_b = static_cast<uint32_t>(__shfl(static_cast<int>(b), prev, kWave));
    if (fail && (!before || prev_b != b)) {
        uint32_t *w = words + 3u * b + kind;
        if (value < __atomic_load_n(w, __ATOMIC_RELAXED)) atomicMin(w, value);
    }
}

__global__ __launch_bounds__(256) void k_sa_check_scatter(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ off, uint32_t count, uint32_t total,
                                                          uint32_t *__restrict__ isa, uint32_t *words) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool fail = false;
    uint32_t b = 0, s = 0;
    if (i < total) {
        b = seg_of(off, count, i);
        s = off[b];
        const uint32_t v = sa[i];
        if (v >= off[b + 1] - s) fail = true;
        else isa[s + v] = i;
    }
    report_lowest(words, 0u, fail, b, i - s);
}

__global__ __launch_bounds__(256) void k_sa_check_missing(const uint32_t *__restrict__ isa, const uint32_t *__restrict__ off, uint32_t count, uint32_t total,
                                                          uint32_t *words) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    const bool fail = p < total && isa[p] == SQ_NONE;
    uint32_t b = 0, s = 0;
    if (__ballot(fail) == 0) return;  // (the whole wave: a valid array never looks its blocks up here)
    if (fail) {
        b = seg_of(off, count, p);
        s = off[b];
    }
    report_lowest(words, 1u, fail, b, p - s);
}

__global__ __launch_bounds__(256) void k_sa_check_order(const uint8_t *__restrict__ t, const uint32_t *__restrict__ sa, const uint32_t *__restrict__ off,
                                                        uint32_t count, uint32_t total, const uint32_t *__restrict__ isa, uint32_t *words) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool fail = false;
    uint32_t b = 0, s = 0;
    if (i < total) {
        b = seg_of(off, count, i);
        s = off[b];
        // (the two words are final: the kernels that write them are done.  Without either failure the block's entries are a permutation of its
        //  positions, so both reads of isa below hit a slot of this block.)
        if (i > s && words[3u * b] == SQ_NONE && words[3u * b + 1u] == SQ_NONE) {
            const uint32_t len = off[b + 1] - s, x = sa[i - 1], y = sa[i];
            const uint8_t cx = t[static_cast<size_t>(s) + x], cy = t[static_cast<size_t>(s) + y];
            if (cx != cy) fail = cx > cy;
            else if (x + 1u == len) fail = false;
            else if (y + 1u == len) fail = true;
            else fail = !(isa[s + x + 1u] < isa[s + y + 1u]);
        }
    }
    report_lowest(words, 2u, fail, b, i - s);
}

// ---- the search -----------------------------------------------------------------------------------------------------------------------------

// What a compare leaves: the bytes of P matched, and whether the suffix cut to m bytes is smaller than / equal to P.
struct SqCmp { uint32_t matched; bool lt, eq; };

__device__ __forceinline__ SqCmp sq_verdict(const uint8_t *__restrict__ suffix, const uint8_t *__restrict__ pat, uint32_t m, uint32_t lim, uint32_t k) {
    if (k < lim) return SqCmp{k, suffix[k] < pat[k], false};
    return SqCmp{k, lim != m, lim == m};  // the suffix ends inside P: a proper prefix, smaller
}

// one lane, one suffix: bytes [known, lim) 16 a step.  tb / nb: the block's text and length; v: the suffix-array entry
__device__ __forceinline__ SqCmp sq_compare_lane(const uint8_t *__restrict__ tb, uint32_t nb, uint32_t v, const uint8_t *__restrict__ pat, uint32_t m,
                                                 uint32_t known) {
    const uint32_t avail = v < nb ? nb - v : 0u, lim = avail < m ? avail : m;
    const uint8_t *suffix = tb + (v < nb ? v : 0u);
    uint32_t k = known < lim ? known : lim;
    while (k < lim) {
        const uint32_t d = match16(suffix + k, pat + k, lim - k);
        k += d;
        if (d < 16) break;
    }
    return sq_verdict(suffix, pat, m, lim, k);
}

// the whole wave, one suffix: 64 x 16 bytes a step (the compare of k_lcp_wave); every lane gets the same answer
__device__ __forceinline__ SqCmp sq_compare_wave(const uint8_t *__restrict__ tb, uint32_t nb, uint32_t v, const uint8_t *__restrict__ pat, uint32_t m,
                                                 uint32_t known, uint32_t lane) {
    const uint32_t avail = v < nb ? nb - v : 0u, lim = avail < m ? avail : m;
    const uint8_t *suffix = tb + (v < nb ? v : 0u);
    uint32_t k = known < lim ? known : lim;
    while (k < lim) {
        const uint32_t o = k + 16u * lane;
        uint32_t d = 16;
        bool diff = false;
        if (o < lim) {
            const uint32_t left = lim - o;
            d = match16(suffix + o, pat + o, left);
            diff = d < (left < 16u ? left : 16u);
        }
        const uint64_t mask = __ballot(diff);
        if (mask) {
            const int first = __ffsll(static_cast<unsigned long long>(mask)) - 1;
            k += 16u * static_cast<uint32_t>(first) + static_cast<uint32_t>(__shfl(static_cast<int>(d), first, kWave));
            break;
        }
        k = lim - k > 64u * 16u ? k + 64u * 16u : lim;
    }
    return sq_verdict(suffix, pat, m, lim, k);
}

// The candidate range of a bound: every slot below l satisfies the predicate, no slot from r on does; kl / kr = bytes of P matched by the
// suffixes at slots l - 1 and r (0 at the block's ends).
struct SqRange { uint32_t l, r, kl, kr; };

// the number of slots that satisfy the predicate (UPPER: not greater than P; else: smaller than P), 64 pivots a step
template <bool UPPER>
__device__ __forceinline__ SqRange sq_bound_lanes(const uint8_t *__restrict__ tb, const uint32_t *__restrict__ sab, uint32_t nb, const uint8_t *__restrict__ pat,
                                                  uint32_t m, SqRange g, uint32_t lane) {
    while (g.l < g.r) {
        const uint32_t w = g.r - g.l, nact = w < 64u ? w : 64u;
        const uint32_t slot = w <= 64u ? g.l + lane : g.l + static_cast<uint32_t>((static_cast<uint64_t>(lane) * w) >> 6);  // distinct: w / 64 > 1
        bool pred = false;
        uint32_t k = 0;
        if (lane < nact) {
            const SqCmp c = sq_compare_lane(tb, nb, sab[slot], pat, m, g.kl < g.kr ? g.kl : g.kr);
            pred = UPPER ? (c.lt || c.eq) : c.lt;
            k = c.matched;
        }
        const uint32_t c = static_cast<uint32_t>(__popcll(__ballot(pred)));  // monotone over the slots: lanes 0 .. c-1 (only active lanes: c <= nact)
        const int left = c ? static_cast<int>(c) - 1 : 0, right = c < 64u ? static_cast<int>(c) : 63;
        const uint32_t slot_l = static_cast<uint32_t>(__shfl(static_cast<int>(slot), left, kWave)), k_l = static_cast<uint32_t>(__shfl(static_cast<int>(k), left, kWave));
        const uint32_t slot_r = static_cast<uint32_t>(__shfl(static_cast<int>(slot), right, kWave)), k_r = static_cast<uint32_t>(__shfl(static_cast<int>(k), right, kWave));
        // (whatever the ballot says, the range shrinks: c > 0 moves l up, c < nact moves r down, and c = 0 gives r = pivot 0 = l)
        if (c) { g.l = slot_l + 1u; g.kl = k_l; }
        if (c < nact) { g.r = slot_r; g.kr = k_r; }
    }
    return g;
}

// the same with one pivot a step, compared by the whole wave
template <bool UPPER>
__device__ __forceinline__ SqRange sq_bound_wave(const uint8_t *__restrict__ tb, const uint32_t *__restrict__ sab, uint32_t nb, const uint8_t *__restrict__ pat,
                                                 uint32_t m, SqRange g, uint32_t lane) {
    while (g.l < g.r) {
        const uint32_t slot = g.l + ((g.r - g.l) >> 1);
        const SqCmp c = sq_compare_wave(tb, nb, sab[slot], pat, m, g.kl < g.kr ? g.kl : g.kr, lane);
        if (UPPER ? (c.lt || c.eq) : c.lt) { g.l = slot + 1u; g.kl = c.matched; }
        else { g.r = slot; g.kr = c.matched; }
    }
    return g;
}

// pattern q = pat[pat_off[q], pat_off[q + 1]), searched in block pat_blk[q] (null: block 0).  A wave per pattern, walked with a grid stride; LONG
// picks the patterns of more than lane_max bytes and leaves the others to the other kernel.
struct SqArgs {
    const uint8_t *t; const uint32_t *sa, *off; const uint8_t *pat; const uint32_t *pat_off, *pat_blk; uint32_t npat, lane_max; uint32_t *out_lo, *out_hi;
};
template <bool LONG>
__device__ __forceinline__ void sq_search(const SqArgs &a) {
    const uint8_t *__restrict__ t = a.t, *__restrict__ pat = a.pat;
    const uint32_t *__restrict__ sa = a.sa, *__restrict__ off = a.off, *__restrict__ pat_off = a.pat_off, *__restrict__ pat_blk = a.pat_blk;
    const uint32_t npat = a.npat, lane_max = a.lane_max;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * SQ_WAVES;
    for (uint64_t q = static_cast<uint64_t>(blockIdx.x) * SQ_WAVES + (threadIdx.x >> 6); q < npat; q += nwaves) {
        const uint32_t po = pat_off[q], m = pat_off[q + 1] - po;
        if ((m > lane_max) != LONG) continue;
        const uint32_t b = pat_blk ? pat_blk[q] : 0u, s = off[b], nb = off[b + 1] - s;
        const uint8_t *tb = t + s, *p = pat + po;
        const uint32_t *sab = sa + s;
        uint32_t lo = 0, hi = nb;
        if (m) {  // (the empty pattern: every suffix, cut to nothing, equals it)
            SqRange g{0u, nb, 0u, 0u};
            g = LONG ? sq_bound_wave<false>(tb, sab, nb, p, m, g, lane) : sq_bound_lanes<false>(tb, sab, nb, p, m, g, lane);
            lo = hi = g.l;
            // kr == m: the suffix at slot lo matched all of P (the block's end counts 0 < m).  Only then is anything equal to P behind lo.
            if (g.kr == m) {
                SqRange h{lo + 1u, nb, m, 0u};
                h = LONG ? sq_bound_wave<true>(tb, sab, nb, p, m, h, lane) : sq_bound_lanes<true>(tb, sab, nb, p, m, h, lane);
                hi = h.l;
            }
        }
        if (lane == 0) {
            a.out_lo[q] = lo;
            a.out_hi[q] = hi;
        }
    }
}
__global__ __launch_bounds__(256) void k_sa_search(SqArgs a) { sq_search<false>(a); }
__global__ __launch_bounds__(256) void k_sa_search_long(SqArgs a) { sq_search<true>(a); }

// ---- matching statistics and super-maximal matches --------------------------------------------------------------------

// Position g of the queries (back to back in qry; query j = [q_off[j], q_off[j + 1]), matched against block q_blk[j], null: block 0): its window
// is the m = min(max_len, q_off[j + 1] - g) bytes from g on.  len[g] = the longest prefix of the window that occurs in the block, lo[g] / hi[g]
// (both or neither) = what the search gives for that prefix.
struct SmArgs {
    const uint8_t *t; const uint32_t *sa, *off; const uint8_t *qry; const uint32_t *q_off, *q_blk; uint32_t nq, Q, max_len, lane_max; uint32_t *len, *lo, *hi;
};
struct SmWindow { uint32_t m, s, nb; };
__device__ __forceinline__ SmWindow sm_window(const SmArgs &a, uint32_t g) {
    const uint32_t j = seg_of(a.q_off, a.nq, g);  // (an empty query shares its offset with the next one: the largest j is the one that holds g)
    const uint32_t left = a.q_off[j + 1] - g, b = a.q_blk ? a.q_blk[j] : 0u, s = a.off[b];
    return SmWindow{left < a.max_len ? left : a.max_len, s, a.off[b + 1] - s};
}

// The window P of m bytes inside the slots [L, H), whose suffixes all start with the first `known` bytes of P (L = 0, H = n_b, known = 0: the
// whole block).  One lower bound of P: the suffixes on either side of the insertion slot are the two that share the most with P, so the longest
// prefix of P that occurs is max(kl, kr) bytes long (a border that never moved still holds `known`, which the other, moved in a range that is
// not empty, reaches at least).  Then the bracket of that prefix: a lower bound in front of the slot where the left neighbour has all of it, an
// upper bound behind the slot where the suffix at the slot has; both start from the bytes known at their borders.  For any array: a border
// holds more than `known` only once it has moved, so L <= slot - 1 and slot + 1 <= H where they are used, and L <= lo <= hi <= H.
struct SmOut { uint32_t len, lo, hi; };
template <bool WAVE>
__device__ __forceinline__ SmOut sm_position(const uint8_t *__restrict__ tb, const uint32_t *__restrict__ sab, uint32_t nb, const uint8_t *__restrict__ p,
                                             uint32_t m, uint32_t L, uint32_t H, uint32_t known, uint32_t lane) {
    SqRange g{L, H, known, known};
    g = WAVE ? sq_bound_wave<false>(tb, sab, nb, p, m, g, lane) : sq_bound_lanes<false>(tb, sab, nb, p, m, g, lane);
    const uint32_t slot = g.l, len = g.kl > g.kr ? g.kl : g.kr;
    SmOut o{len, L, H};
    if (len > known) {
        o.lo = o.hi = slot;
        if (g.kl == len) {
            const SqRange x{L, slot - 1u, known, len};
            o.lo = (WAVE ? sq_bound_wave<false>(tb, sab, nb, p, len, x, lane) : sq_bound_lanes<false>(tb, sab, nb, p, len, x, lane)).l;
        }
        if (g.kr == len) {
            const SqRange x{slot + 1u, H, len, known};
            o.hi = (WAVE ? sq_bound_wave<true>(tb, sab, nb, p, len, x, lane) : sq_bound_lanes<true>(tb, sab, nb, p, len, x, lane)).l;
        }
    }
    return o;
}

// A wave per position, walked with a grid stride: the window cut to lane_max bytes, by the 64-ary lane search.  A match that runs through the
// cut (len == lane_max < m) is finished by k_sa_match_long.
__global__ __launch_bounds__(256) void k_sa_match(SmArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * SQ_WAVES;
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * SQ_WAVES + (threadIdx.x >> 6); g < a.Q; g += nwaves) {
        const SmWindow w = sm_window(a, static_cast<uint32_t>(g));
        const uint32_t mc = w.m < a.lane_max ? w.m : a.lane_max;
        const SmOut o = sm_position<false>(a.t + w.s, a.sa + w.s, w.nb, a.qry + g, mc, 0u, w.nb, 0u, lane);
        if (lane == 0) {
            a.len[g] = o.len;
            if (a.lo) { a.lo[g] = o.lo; a.hi[g] = o.hi; }
        }
    }
}

// Only the positions whose match ran through the cut: a wave reads 64 lengths at a time and takes the marked ones in turn, each inside the
// range of its lane_max-byte prefix (lo / hi of k_sa_match; without them the whole block, nothing known) by the whole-wave compare.
__global__ __launch_bounds__(256) void k_sa_match_long(SmArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * SQ_WAVES * 64u;
    for (uint64_t base = (static_cast<uint64_t>(blockIdx.x) * SQ_WAVES + (threadIdx.x >> 6)) * 64u; base < a.Q; base += stride) {
        uint64_t todo = __ballot(base + lane < a.Q && a.len[base + lane] == a.lane_max);
        while (todo) {
            const uint32_t g = static_cast<uint32_t>(base) + static_cast<uint32_t>(__builtin_ctzll(todo));
            todo &= todo - 1u;
            const SmWindow w = sm_window(a, g);
            if (w.m <= a.lane_max) continue;  // (the window ended at the cut: len is final)
            uint32_t L = 0, H = w.nb, known = 0;
            if (a.lo) {
                H = a.hi[g] < w.nb ? a.hi[g] : w.nb;
                L = a.lo[g] < H ? a.lo[g] : H;
                known = a.lane_max;
            }
            const SmOut o = sm_position<true>(a.t + w.s, a.sa + w.s, w.nb, a.qry + g, w.m, L, H, known, lane);
            if (lane == 0) {
                a.len[g] = o.len;
                if (a.lo) { a.lo[g] = o.lo; a.hi[g] = o.hi; }
            }
        }
    }
}

// The super-maximal matches: position g at offset i of its query is one when len[g] >= max(min_len, 1), the match one byte earlier does not
// contain it (i == 0 or len[g - 1] <= len[g]), and it is not the continuation of a copy longer than max_len (both at the cap).
constexpr uint32_t SM_TILE = 1024;  // positions per workgroup of the scan: 256 threads x 4
__global__ __launch_bounds__(256) void k_sa_smem_mark(const uint32_t *__restrict__ len, const uint32_t *__restrict__ q_off, uint32_t nq, uint32_t Q, uint32_t min_len,
                                                      uint32_t max_len, uint32_t *__restrict__ flag) {
    const uint64_t g64 = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (g64 >= Q) return;
    const uint32_t g = static_cast<uint32_t>(g64), l = len[g];
    const bool first = g == q_off[seg_of(q_off, nq, g)];
    const uint32_t prev = first ? 0u : len[g - 1];
    flag[g] = l >= (min_len ? min_len : 1u) && prev <= l && !(!first && prev == max_len && l == max_len);
}
// the exclusive scan of the flags: a tile's sum, one workgroup over the sums (the grand total to the mailbox, a plain store on every launch) ...
__device__ __forceinline__ uint4 sm_flags(const uint32_t *__restrict__ flag, uint32_t Q, uint64_t g0) {
    if (g0 + 3u < Q) return *reinterpret_cast<const uint4 *>(flag + g0);  // (flag: a workspace allocation, 256-byte aligned; g0 a multiple of 4)
    return uint4{g0 < Q ? flag[g0] : 0u, g0 + 1u < Q ? flag[g0 + 1u] : 0u, g0 + 2u < Q ? flag[g0 + 2u] : 0u, g0 + 3u < Q ? flag[g0 + 3u] : 0u};
}
__global__ __launch_bounds__(256) void k_sa_smem_scan_a(const uint32_t *__restrict__ flag, uint32_t Q, uint32_t *__restrict__ tile_sum) {
    __shared__ uint32_t s_tmp[5];
    const uint4 f = sm_flags(flag, Q, static_cast<uint64_t>(blockIdx.x) * SM_TILE + 4u * threadIdx.x);
    uint32_t all;
    block_excl_sum<4>(f.x + f.y + f.z + f.w, s_tmp, &all);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
}
__global__ __launch_bounds__(256) void k_sa_smem_scan_b(uint32_t *__restrict__ tile_sum, uint32_t ntiles, uint64_t *__restrict__ grand_total) {
    __shared__ uint32_t s_tmp[5];
    uint64_t run = 0;
    for (uint32_t c = 0; c < ntiles; c += 256u) {  // (the same trip count for every thread)
        const uint32_t i = c + threadIdx.x, v = i < ntiles ? tile_sum[i] : 0u;
        uint32_t all;
        const uint32_t ex = block_excl_sum<4>(v, s_tmp, &all);
        if (i < ntiles) tile_sum[i] = static_cast<uint32_t>(run) + ex;  // (an exclusive offset is below the total, and that below 2^32)
        run += all;
    }
    if (threadIdx.x == 0) *grand_total = run;
}
// ... and the records: flagged position g at place `before` of the list, while that is below nhits = min(total, max_hits); one 16-byte store
__global__ __launch_bounds__(256) void k_sa_smem_emit(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ len, const uint32_t *__restrict__ lo,
                                                      const uint32_t *__restrict__ hi, uint32_t Q, const uint32_t *__restrict__ tile_sum, uint32_t nhits,
                                                      uint4 *__restrict__ hits) {
    __shared__ uint32_t s_tmp[5];
    const uint32_t tile_at = tile_sum[blockIdx.x];
    if (tile_at >= nhits) return;  // (the whole workgroup: the list is cut in front of this tile)
    const uint64_t g0 = static_cast<uint64_t>(blockIdx.x) * SM_TILE + 4u * threadIdx.x;
    const uint4 f = sm_flags(flag, Q, g0);
    const uint32_t fl[4] = {f.x, f.y, f.z, f.w};
    uint32_t at = tile_at + block_excl_sum<4>(f.x + f.y + f.z + f.w, s_tmp, nullptr);
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        if (!fl[k]) continue;
        const uint32_t g = static_cast<uint32_t>(g0) + k;
        if (at < nhits) hits[at] = uint4{g, len[g], lo[g], hi[g]};
        ++at;
    }
}

}  // namespace

int sa_check_device(dk_ctx *ctx, const PackView &text, const uint32_t *d_sa, uint32_t *h_words) {
    hipStream_t st = ctx->stream;
    const size_t count = text.count, total = text.total;
    const uint32_t cnt = static_cast<uint32_t>(count), T = static_cast<uint32_t>(total);
    const unsigned grid = static_cast<unsigned>(div_up(total, 256));
    const size_t mark = ctx->ws_mark();
    uint32_t *isa = ctx->ws_alloc<uint32_t>(total), *words = ctx->ws_alloc<uint32_t>(3 * count);
    if (!isa || !words) return DK_E_NOMEM;
    DK_HIP(ctx, hipMemsetAsync(isa, 0xFF, total * sizeof(uint32_t), st));
    DK_HIP(ctx, hipMemsetAsync(words, 0xFF, 3 * count * sizeof(uint32_t), st));
    {
        LaunchScope ls(ctx, K_BWT_GATHER, 12.0 * total);  // SA 4 n, a scattered 4-byte store per slot, the preset 4 n
        k_sa_check_scatter<<<dim3(grid), dim3(256), 0, st>>>(d_sa, text.d_off, cnt, T, isa, words);
    }
    {
        LaunchScope ls(ctx, K_BWT_GATHER, 4.0 * total);
        k_sa_check_missing<<<dim3(grid), dim3(256), 0, st>>>(isa, text.d_off, cnt, T, words);
    }
    {
        LaunchScope ls(ctx, K_BWT_GATHER, 18.0 * total);  // SA twice 8 n, two gathered bytes, two gathered words of isa (where the bytes are equal)
        k_sa_check_order<<<dim3(grid), dim3(256), 0, st>>>(text.bytes, d_sa, text.d_off, cnt, T, isa, words);
    }
    DK_HIP(ctx, hipGetLastError());
    DK_HIP(ctx, hipMemcpyAsync(h_words, words, 3 * count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DK_HIP(ctx, hipStreamSynchronize(st));
    ctx->ws_release(mark);
    return DK_OK;
}

int sa_search_device(dk_ctx *ctx, const PackView &text, const uint32_t *d_sa, const ItemView &pat, uint32_t *d_lo, uint32_t *d_hi) {
    hipStream_t st = ctx->stream;
    // (tuning build: DK_SA_SEARCH_LANE_MAX moves the border between the two kernels -- tests send short patterns down the long one with it)
    const uint32_t lane_max = static_cast<uint32_t>(std::max(0, std::min(1 << 20, DK_KNOB("DK_SA_SEARCH_LANE_MAX", SA_SEARCH_LANE_MAX))));
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(div_up(pat.count, SQ_WAVES), 1u << 20));
    const SqArgs a{text.bytes, d_sa, text.d_off, pat.bytes, pat.d_off, pat.d_blk, static_cast<uint32_t>(pat.count), lane_max, d_lo, d_hi};
    if (pat.shortest <= lane_max) {
        LaunchScope ls(ctx, K_CHAIN, 8.0 * pat.count);
        k_sa_search<<<dim3(grid), dim3(64 * SQ_WAVES), 0, st>>>(a);
    }
    if (pat.longest > lane_max) {
        LaunchScope ls(ctx, K_CHAIN, 8.0 * pat.count);
        k_sa_search_long<<<dim3(grid), dim3(64 * SQ_WAVES), 0, st>>>(a);
    }
    DK_HIP(ctx, hipGetLastError());
    return DK_OK;
}

int sa_match_device(dk_ctx *ctx, const PackView &text, const uint32_t *d_sa, const ItemView &qry, size_t max_len, uint32_t *d_len, uint32_t *d_lo, uint32_t *d_hi) {
    hipStream_t st = ctx->stream;
    const size_t qbytes = qry.nbytes;
    // (the border is the search's, and so is its knob: a match that reaches it goes on in k_sa_match_long, whatever the window's length)
    const uint32_t lane_max = static_cast<uint32_t>(std::max(0, std::min(1 << 20, DK_KNOB("DK_SA_SEARCH_LANE_MAX", SA_SEARCH_LANE_MAX))));
    const uint32_t cap = static_cast<uint32_t>(std::min<size_t>(max_len, 0xFFFFFFFFull));
    const SmArgs a{text.bytes, d_sa, text.d_off, qry.bytes, qry.d_off, qry.d_blk, static_cast<uint32_t>(qry.count), static_cast<uint32_t>(qbytes), cap, lane_max,
                   d_len, d_lo, d_hi};
    {
        // per position three searches of about three steps of 64 slots and 64 short compares; the three results
        LaunchScope ls(ctx, K_CHAIN, qbytes * (9.0 * 64 * 20 + 12.0));
        const unsigned grid = static_cast<unsigned>(std::min<size_t>(div_up(qbytes, SQ_WAVES), 1u << 20));
        k_sa_match<<<dim3(grid), dim3(64 * SQ_WAVES), 0, st>>>(a);
    }
    if (cap > lane_max) {
        LaunchScope ls(ctx, K_CHAIN, 4.0 * qbytes);  // the lengths read; what the marked positions compare is theirs alone
        const unsigned grid = static_cast<unsigned>(std::min<size_t>(div_up(qbytes, 64 * SQ_WAVES), 1u << 20));
        k_sa_match_long<<<dim3(grid), dim3(64 * SQ_WAVES), 0, st>>>(a);
    }
    DK_HIP(ctx, hipGetLastError());
    return DK_OK;
}

size_t sa_smems_workspace(size_t qbytes) {
    return 4 * ws_round(4 * qbytes) + ws_round(4 * div_up(qbytes, SM_TILE));
}

int sa_smems_device(dk_ctx *ctx, const PackView &text, const uint32_t *d_sa, const ItemView &qry, size_t min_len, size_t max_len, const HitSink &out) {
    hipStream_t st = ctx->stream;
    const size_t qbytes = qry.nbytes;
    const size_t ntiles = div_up(qbytes, SM_TILE), mark = ctx->ws_mark();
    uint32_t *d_len = ctx->ws_alloc<uint32_t>(qbytes), *d_lo = ctx->ws_alloc<uint32_t>(qbytes), *d_hi = ctx->ws_alloc<uint32_t>(qbytes);
    uint32_t *d_flag = ctx->ws_alloc<uint32_t>(qbytes), *tile_sum = ctx->ws_alloc<uint32_t>(ntiles);
    if (!d_len || !d_lo || !d_hi || !d_flag || !tile_sum) return DK_E_NOMEM;
    DK_TRY(sa_match_device(ctx, text, d_sa, qry, max_len, d_len, d_lo, d_hi));
    const uint32_t Q = static_cast<uint32_t>(qbytes), T = static_cast<uint32_t>(ntiles);
    {
        LaunchScope ls(ctx, K_CHAIN, 20.0 * qbytes);  // the lengths and the flags, the flags read twice more
        k_sa_smem_mark<<<dim3(static_cast<unsigned>(div_up(qbytes, 256))), dim3(256), 0, st>>>(
            d_len, qry.d_off, static_cast<uint32_t>(qry.count), Q, static_cast<uint32_t>(std::min<size_t>(min_len, 0xFFFFFFFFull)),
            static_cast<uint32_t>(std::min<size_t>(max_len, 0xFFFFFFFFull)), d_flag);
        k_sa_smem_scan_a<<<dim3(T), dim3(256), 0, st>>>(d_flag, Q, tile_sum);
        k_sa_smem_scan_b<<<dim3(1), dim3(256), 0, st>>>(tile_sum, T, &ctx->d_mail->sa_match.total);
    }
    DK_HIP(ctx, hipGetLastError());
    DK_TRY(ctx->mail_read(&ctx->h_mail->sa_match.total));
    const size_t nhits = out.take(ctx->h_mail->sa_match.total);
    if (nhits) {
        {
            LaunchScope ls(ctx, K_CHAIN, 4.0 * qbytes + 28.0 * nhits);
            k_sa_smem_emit<<<dim3(T), dim3(256), 0, st>>>(d_flag, d_len, d_lo, d_hi, Q, tile_sum, static_cast<uint32_t>(nhits), static_cast<uint4 *>(out.d_hits));
        }
        DK_HIP(ctx, hipGetLastError());
        DK_HIP(ctx, hipStreamSynchronize(st));
    }
    ctx->ws_release(mark);
    return DK_OK;
}

}  // namespace dk
