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

}  // namespace

int sa_check_device(dk_ctx *ctx, const uint8_t *d_text, const uint32_t *d_off, size_t count, size_t total, const uint32_t *d_sa, uint32_t *h_words) {
    hipStream_t st = ctx->stream;
    const uint32_t cnt = static_cast<uint32_t>(count), T = static_cast<uint32_t>(total);
    const unsigned grid = static_cast<unsigned>(div_up(total, 256));
    const size_t mark = ctx->ws_mark();
    uint32_t *isa = ctx->ws_alloc<uint32_t>(total), *words = ctx->ws_alloc<uint32_t>(3 * count);
    if (!isa || !words) return DK_E_NOMEM;
    DK_HIP(ctx, hipMemsetAsync(isa, 0xFF, total * sizeof(uint32_t), st));
    DK_HIP(ctx, hipMemsetAsync(words, 0xFF, 3 * count * sizeof(uint32_t), st));
    {
        LaunchScope ls(ctx, K_BWT_GATHER, 12.0 * total);  // SA 4 n, a scattered 4-byte store per slot, the preset 4 n
        k_sa_check_scatter<<<dim3(grid), dim3(256), 0, st>>>(d_sa, d_off, cnt, T, isa, words);
    }
    {
        LaunchScope ls(ctx, K_BWT_GATHER, 4.0 * total);
        k_sa_check_missing<<<dim3(grid), dim3(256), 0, st>>>(isa, d_off, cnt, T, words);
    }
    {
        LaunchScope ls(ctx, K_BWT_GATHER, 18.0 * total);  // SA twice 8 n, two gathered bytes, two gathered words of isa (where the bytes are equal)
        k_sa_check_order<<<dim3(grid), dim3(256), 0, st>>>(d_text, d_sa, d_off, cnt, T, isa, words);
    }
    DK_HIP(ctx, hipGetLastError());
    DK_HIP(ctx, hipMemcpyAsync(h_words, words, 3 * count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DK_HIP(ctx, hipStreamSynchronize(st));
    ctx->ws_release(mark);
    return DK_OK;
}

int sa_search_device(dk_ctx *ctx, const uint8_t *d_text, const uint32_t *d_off, const uint32_t *d_sa, const uint8_t *d_pat, const uint32_t *d_pat_off,
                     const uint32_t *d_pat_blk, size_t npat, size_t longest, size_t shortest, uint32_t *d_lo, uint32_t *d_hi) {
    hipStream_t st = ctx->stream;
    // (tuning build: DK_SA_SEARCH_LANE_MAX moves the border between the two kernels -- tests send short patterns down the long one with it)
    const uint32_t lane_max = static_cast<uint32_t>(std::max(0, std::min(1 << 20, DK_KNOB("DK_SA_SEARCH_LANE_MAX", SA_SEARCH_LANE_MAX))));
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(div_up(npat, SQ_WAVES), 1u << 20));
    const SqArgs a{d_text, d_sa, d_off, d_pat, d_pat_off, d_pat_blk, static_cast<uint32_t>(npat), lane_max, d_lo, d_hi};
    if (shortest <= lane_max) {
        LaunchScope ls(ctx, K_CHAIN, 8.0 * npat);
        k_sa_search<<<dim3(grid), dim3(64 * SQ_WAVES), 0, st>>>(a);
    }
    if (longest > lane_max) {
        LaunchScope ls(ctx, K_CHAIN, 8.0 * npat);
        k_sa_search_long<<<dim3(grid), dim3(64 * SQ_WAVES), 0, st>>>(a);
    }
    DK_HIP(ctx, hipGetLastError());
    return DK_OK;
}

}  // namespace dk
