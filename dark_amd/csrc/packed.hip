// Packed forward path: many independent blocks laid back to back in one device buffer go through ONE segmented suffix sort and ONE
// segmented distance coding, so a pack costs O(rounds) launches instead of O(blocks).  The reference treats every
// block as self-contained (src/block/dc.rs:30-37,53); the per-block contract is src/saca.rs:368-378 for L / origin and src/block/dc.rs:41-91
// for the DC arrays.
//
// Conventions: block i is text[off_i, off_i + n_i), e_i = off_i + n_i, off_0 = 0, off_count = T.  A position's block comes from a binary
// search in the offsets table (or from the block of a thread's first position, advanced linearly); no n-sized block-id array.
//
// Segmented suffix sort (prefix doubling, ranks global):
//   initial key   block id, then the first k symbols of the block's suffix under the pack's order-preserving code (0 = past e_i: the
//                 no-sentinel rule of src/saca.rs:105-113, a suffix that is a prefix of another sorts first).  The block id in the top bits
//                 makes block i's suffixes occupy exactly the slots [off_i, e_i).
//   rank[p]       slot of the first member of p's group (a singleton's rank is its final slot)
//   round (h)     live suffixes only (members of groups of two or more): key = rank[p] << rbits | rank2,
//                 rank2 = rank[p+h] + h, or e_i - 1 - p when p + h >= e_i (shorter suffix first).  Sorted by the existing LSD radix sort.
//   k_pk_tile_sum / k_pk_spine / k_pk_tile_apply   one scan over the sorted list: new group heads, old group heads and live counts; a member
//                 at list index k of an old group that starts at list index ks and slot g gets the slot g + (head of its new group - ks);
//                 singletons leave, the other members are compacted (order kept) into the next round's list.
//   k_pk_scatter  L[rank[p]] = text[p-1] (text[e_i-1] in front of off_i), origin_i = rank[off_i] - off_i.
//   k_pk_emit     the packed suffix arrays (packed_sa_device): after the rounds rank is the inverse suffix array of
//                 the whole pack, so SA[rank[p]] = p - off_i; the same thread writes L and the origin when they are wanted too.  The sort
//                 (packed_sort_device: everything up to the guard) is shared; packed_bwt_device and packed_sa_device differ in the emit alone.
// Segmented DC over the runs of L, in L order (the single-block kernels of dc.hip walk R; the results are the same):
//   k_pdc_count / k_pk_scan_u32 / k_pdc_runs   runs (a run never crosses a block head), their start, symbol and each block's first run rb_i
//   k_pdc_summary / k_pdc_carry_*              per tile of 4096 runs the last run of every symbol, exclusive max-scan over tiles: the last
//                 occurrence of every symbol before each tile.  Run indices are global and grow with the block, so the scan needs no segments:
//                 an entry below the current block's first run is simply "absent".
//   k_pdc_main    one wave per tile, 64 runs per step: previous occurrence of each run's symbol, its MTF rank = distinct symbols between
//                 (table entries past the previous occurrence + earlier lanes of the step that are the first of their symbol past it),
//                 the distance of the previous run of the symbol, init[] for first occurrences
//   k_pdc_finlist / k_pdc_final                the final sweep: a block's last run of each symbol gets e - end - rank - 1 with rank = the
//                 number of last runs after it; m_i and the DK_FLAG_* bits per block.
#include <algorithm>

#include "context.hpp"
#include "device_util.hpp"

namespace dk {
namespace {

constexpr int PK_BLOCK = 256;
constexpr int PK_IPT = 16;
constexpr int PK_TILE = PK_BLOCK * PK_IPT;  // list entries / positions per workgroup of the scans
constexpr int PDC_TILE = 4096;              // runs per wave in k_pdc_summary / k_pdc_main
constexpr int PDC_WAVES = 4;
constexpr int PDC_MAX_CHUNKS = 256;

// ---- suffix sort ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pk_hist(const uint8_t *__restrict__ t, size_t n, uint32_t *__restrict__ present) {
    __shared__ uint32_t s[256];
    s[threadIdx.x] = 0;
    __syncthreads();
    for (size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < n; p += static_cast<size_t>(gridDim.x) * blockDim.x) s[t[p]] = 1;
    __syncthreads();
    if (s[threadIdx.x]) atomicOr(&present[threadIdx.x], 1u);
}

// code[c] = 1 + number of present symbols below c; out[0] = number of present symbols
__global__ __launch_bounds__(256) void k_pk_codes(const uint32_t *__restrict__ present, uint16_t *__restrict__ code, uint32_t *__restrict__ out) {
    __shared__ uint32_t s[256];
    const int c = threadIdx.x;
    s[c] = present[c] ? 1u : 0u;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint32_t v = c >= d ? s[c - d] : 0u;
        __syncthreads();
        s[c] += v;
        __syncthreads();
    }
    code[c] = static_cast<uint16_t>(present[c] ? s[c] : 0u);  // up to 256: nine bits with all symbols present
    if (c == 255) out[0] = s[255];
}

__global__ __launch_bounds__(256) void k_pk_init_keys(const uint8_t *__restrict__ t, const uint32_t *__restrict__ off, uint32_t count, uint32_t total,
                                                      const uint16_t *__restrict__ code, int bits, int k, uint64_t *__restrict__ keys,
                                                      uint32_t *__restrict__ vals) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    const uint32_t blk = seg_of(off, count, p);
    const uint32_t e = off[blk + 1];
    uint64_t key = blk;
    for (int j = 0; j < k; ++j) key = (key << bits) | (p + j < e ? code[t[p + j]] : 0u);
    keys[p] = key;
    vals[p] = p;
}

__global__ __launch_bounds__(256) void k_pk_round_keys(const uint32_t *__restrict__ act, uint32_t c, const uint32_t *__restrict__ rank,
                                                       const uint32_t *__restrict__ off, uint32_t count, uint32_t h, int rbits,
                                                       uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= c) return;
    const uint32_t p = act[k];
    const uint32_t e = off[seg_of(off, count, p) + 1];
    const uint64_t r2 = (static_cast<uint64_t>(p) + h < e) ? static_cast<uint64_t>(rank[p + h]) + h : static_cast<uint64_t>(e - 1 - p);
    keys[k] = (static_cast<uint64_t>(rank[p]) << rbits) | r2;
    vals[k] = p;
}

// (last new head, last old head, live count) over a tile; combine = (max, max, sum)
struct GroupAgg { uint32_t nh, oh, live, pad; };

__device__ __forceinline__ GroupAgg agg_combine(GroupAgg a, GroupAgg b) {
    return GroupAgg{a.nh > b.nh ? a.nh : b.nh, a.oh > b.oh ? a.oh : b.oh, a.live + b.live, 0u};
}

// exclusive scan of one value per thread over the workgroup (Hillis-Steele through LDS); *total = the workgroup's aggregate
__device__ __forceinline__ GroupAgg block_excl_agg(GroupAgg v, GroupAgg *s, GroupAgg *total) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < PK_BLOCK; d <<= 1) {
        const GroupAgg o = t >= d ? s[t - d] : GroupAgg{0u, 0u, 0u, 0u};
        __syncthreads();
        s[t] = agg_combine(o, s[t]);
        __syncthreads();
    }
    const GroupAgg incl_prev = t > 0 ? s[t - 1] : GroupAgg{0u, 0u, 0u, 0u};
    *total = s[PK_BLOCK - 1];
    __syncthreads();
    return incl_prev;
}

__device__ __forceinline__ uint64_t old_group(uint64_t key, int rbits) { return rbits >= 64 ? 0ull : key >> rbits; }

// flags of list entry i: bit 0 new head, bit 1 old head, bit 2 live (member of a group of two or more)
__device__ __forceinline__ uint32_t entry_flags(const uint64_t *__restrict__ keys, uint32_t c, uint32_t i, int rbits) {
    const uint64_t k = keys[i];
    const bool nh = i == 0 || keys[i - 1] != k;
    const bool oh = i == 0 || old_group(keys[i - 1], rbits) != old_group(k, rbits);
    const bool single = nh && (i + 1 == c || keys[i + 1] != k);
    return (nh ? 1u : 0u) | (oh ? 2u : 0u) | (single ? 0u : 4u);
}

__global__ __launch_bounds__(PK_BLOCK) void k_pk_tile_sum(const uint64_t *__restrict__ keys, uint32_t c, int rbits, GroupAgg *__restrict__ agg) {
    __shared__ GroupAgg s[PK_BLOCK];
    const uint32_t i0 = blockIdx.x * PK_TILE + threadIdx.x * PK_IPT;
    GroupAgg a{0u, 0u, 0u, 0u};
    for (int j = 0; j < PK_IPT; ++j) {
        const uint32_t i = i0 + j;
        if (i >= c) break;
        const uint32_t f = entry_flags(keys, c, i, rbits);
        if (f & 1u) a.nh = i;
        if (f & 2u) a.oh = i;
        a.live += (f >> 2) & 1u;
    }
    GroupAgg total;
    (void)block_excl_agg(a, s, &total);
    if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

// exclusive scan of the tile aggregates in place; *live_out = live entries in all
__global__ __launch_bounds__(1024) void k_pk_spine(GroupAgg *__restrict__ agg, uint32_t ntiles, uint32_t *__restrict__ live_out) {
    __shared__ GroupAgg s[1024];
    const uint32_t t = threadIdx.x;
    GroupAgg carry{0u, 0u, 0u, 0u};
    for (uint32_t base = 0; base < ntiles; base += 1024) {
        const GroupAgg v = base + t < ntiles ? agg[base + t] : GroupAgg{0u, 0u, 0u, 0u};
        s[t] = v;
        __syncthreads();
        for (uint32_t d = 1; d < 1024; d <<= 1) {
            const GroupAgg o = t >= d ? s[t - d] : GroupAgg{0u, 0u, 0u, 0u};
            __syncthreads();
            s[t] = agg_combine(o, s[t]);
            __syncthreads();
        }
        if (base + t < ntiles) agg[base + t] = agg_combine(carry, t > 0 ? s[t - 1] : GroupAgg{0u, 0u, 0u, 0u});
        carry = agg_combine(carry, s[1023]);
        __syncthreads();
    }
    if (t == 0) *live_out = carry.live;
}

// ranks of every entry of the sorted list, and the live entries compacted (in order) into next_act
__global__ __launch_bounds__(PK_BLOCK) void k_pk_tile_apply(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t c,
                                                            int rbits, const GroupAgg *__restrict__ agg, uint32_t *__restrict__ rank,
                                                            uint32_t *__restrict__ next_act) {
    __shared__ GroupAgg s[PK_BLOCK];
    const uint32_t i0 = blockIdx.x * PK_TILE + threadIdx.x * PK_IPT;
    uint32_t fl[PK_IPT];
    GroupAgg a{0u, 0u, 0u, 0u};
    for (int j = 0; j < PK_IPT; ++j) {
        const uint32_t i = i0 + j;
        fl[j] = i < c ? entry_flags(keys, c, i, rbits) : 0u;
        if (fl[j] & 1u) a.nh = i;
        if (fl[j] & 2u) a.oh = i;
        a.live += (fl[j] >> 2) & 1u;
    }
    GroupAgg total;
    GroupAgg run = agg_combine(agg[blockIdx.x], block_excl_agg(a, s, &total));
    for (int j = 0; j < PK_IPT; ++j) {
        const uint32_t i = i0 + j;
        if (i >= c) break;
        if (fl[j] & 1u) run.nh = i;
        if (fl[j] & 2u) run.oh = i;
        const uint32_t p = vals[i];
        const uint32_t g = static_cast<uint32_t>(old_group(keys[i], rbits));
        rank[p] = g + (run.nh - run.oh);
        if (fl[j] & 4u) next_act[run.live++] = p;
    }
}

__global__ __launch_bounds__(256) void k_pk_guard_mark(const uint32_t *__restrict__ act, uint32_t c, const uint32_t *__restrict__ off, uint32_t count,
                                                       uint32_t *__restrict__ guard) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < c) guard[seg_of(off, count, act[k])] = 1u;
}

__global__ __launch_bounds__(256) void k_pk_scatter(const uint8_t *__restrict__ t, const uint32_t *__restrict__ off, uint32_t count, uint32_t total,
                                                    const uint32_t *__restrict__ rank, uint8_t *__restrict__ L, uint32_t *__restrict__ origin) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    const uint32_t blk = seg_of(off, count, p);
    const uint32_t s = off[blk];
    const uint32_t slot = rank[p];
    L[slot] = t[p == s ? off[blk + 1] - 1 : p - 1];
    if (p == s) origin[blk] = slot - s;
}

// The suffix arrays of the pack: SA[rank[p]] = p - off_blk, entries local to the block; with L != nullptr the same thread also writes what
// k_pk_scatter writes (rank[p] and the block search are loaded once for both).  rank[p] lies in [off_blk, e_blk) for every suffix of the
// block, resolved or not, so no store leaves the block's own stretch of the outputs.  The members of a group still unresolved at the round
// limit share one rank: several threads then store to the same slot with plain stores and other slots of the block stay unwritten.  That
// is harmless: the block is marked in the guard words and the caller redoes its whole stretch alone.
__global__ __launch_bounds__(256) void k_pk_emit(const uint8_t *__restrict__ t, const uint32_t *__restrict__ off, uint32_t count, uint32_t total,
                                                 const uint32_t *__restrict__ rank, uint32_t *__restrict__ sa, uint8_t *__restrict__ L,
                                                 uint32_t *__restrict__ origin) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    const uint32_t blk = seg_of(off, count, p);
    const uint32_t s = off[blk];
    const uint32_t slot = rank[p];
    sa[slot] = p - s;
    if (L) {
        L[slot] = t[p == s ? off[blk + 1] - 1 : p - 1];
        if (p == s) origin[blk] = slot - s;
    }
}

// ---- distance coding -------------------------------------------------------------------------------------------------------------------
// run starts among the PK_IPT positions of this thread: a position starts a run at a block head or where the symbol changes
__device__ __forceinline__ uint32_t run_starts(const uint8_t *__restrict__ L, const uint32_t *__restrict__ off, uint32_t count, uint32_t total,
                                               uint32_t p0, uint32_t &blk0) {
    uint32_t bits = 0;
    if (p0 >= total) return 0u;
    uint32_t blk = seg_of(off, count, p0);
    blk0 = blk;
    for (int j = 0; j < PK_IPT; ++j) {
        const uint32_t p = p0 + j;
        if (p >= total) break;
        while (off[blk + 1] <= p) ++blk;
        if (p == off[blk] || L[p] != L[p - 1]) bits |= 1u << j;
    }
    return bits;
}

__global__ __launch_bounds__(PK_BLOCK) void k_pdc_count(const uint8_t *__restrict__ L, const uint32_t *__restrict__ off, uint32_t count, uint32_t total,
                                                        uint32_t *__restrict__ tile_cnt) {
    __shared__ uint32_t s_tmp[PK_BLOCK / 64 + 1];
    uint32_t blk0 = 0;
    const uint32_t bits = run_starts(L, off, count, total, blockIdx.x * PK_TILE + threadIdx.x * PK_IPT, blk0);
    uint32_t tot = 0;
    (void)block_excl_sum<PK_BLOCK / 64>(static_cast<uint32_t>(__popc(bits)), s_tmp, &tot);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
}

// exclusive sum in place
__global__ __launch_bounds__(1024) void k_pk_scan_u32(uint32_t *__restrict__ v, uint32_t nv) {
    __shared__ uint32_t s_tmp[1024 / 64 + 1];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nv; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t x = i < nv ? v[i] : 0u;
        uint32_t tot = 0;
        const uint32_t ex = block_excl_sum<1024 / 64>(x, s_tmp, &tot);
        if (i < nv) v[i] = carry + ex;
        carry += tot;
        __syncthreads();
    }
}

__global__ __launch_bounds__(PK_BLOCK) void k_pdc_runs(const uint8_t *__restrict__ L, const uint32_t *__restrict__ off, uint32_t count, uint32_t total,
                                                       const uint32_t *__restrict__ tile_cnt, uint32_t *__restrict__ run_st, uint8_t *__restrict__ run_sym,
                                                       uint32_t *__restrict__ rb) {
    __shared__ uint32_t s_tmp[PK_BLOCK / 64 + 1];
    const uint32_t p0 = blockIdx.x * PK_TILE + threadIdx.x * PK_IPT;
    uint32_t blk = 0;
    const uint32_t bits = run_starts(L, off, count, total, p0, blk);
    uint32_t tot = 0;
    uint32_t r = tile_cnt[blockIdx.x] + block_excl_sum<PK_BLOCK / 64>(static_cast<uint32_t>(__popc(bits)), s_tmp, &tot);
    for (int j = 0; j < PK_IPT; ++j) {
        const uint32_t p = p0 + j;
        if (p >= total) break;
        while (off[blk + 1] <= p) ++blk;
        if (bits & (1u << j)) {
            run_st[r] = p;
            run_sym[r] = L[p];
            if (p == off[blk]) rb[blk] = r;
            ++r;
        }
        if (p + 1 == total) {  // sentinels: the end of the last run, and the run count
            run_st[r] = total;
            rb[count] = r;
        }
    }
}

__global__ __launch_bounds__(PK_BLOCK) void k_pdc_summary(const uint8_t *__restrict__ run_sym, uint32_t m, uint32_t *__restrict__ tile_last) {
    __shared__ uint32_t s_last[256];
    s_last[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t r0 = blockIdx.x * PDC_TILE;
    for (uint32_t j = threadIdx.x; j < PDC_TILE; j += PK_BLOCK) {
        const uint32_t r = r0 + j;
        if (r < m) atomicMax(&s_last[run_sym[r]], r + 1);
    }
    __syncthreads();
    tile_last[static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x] = s_last[threadIdx.x];
}

__global__ __launch_bounds__(256) void k_pdc_carry_a(const uint32_t *__restrict__ tile_last, uint32_t ntiles, uint32_t tpc, uint32_t *__restrict__ chunk_max) {
    uint32_t mx = 0;
    const uint32_t t0 = blockIdx.x * tpc;
    for (uint32_t t = t0; t < t0 + tpc && t < ntiles; ++t) mx = max(mx, tile_last[static_cast<size_t>(t) * 256 + threadIdx.x]);
    chunk_max[blockIdx.x * 256 + threadIdx.x] = mx;
}

__global__ __launch_bounds__(256) void k_pdc_carry_b(uint32_t *__restrict__ chunk_max, uint32_t nchunks) {
    uint32_t run = 0;
    for (uint32_t ch = 0; ch < nchunks; ++ch) {
        const uint32_t v = chunk_max[ch * 256 + threadIdx.x];
        chunk_max[ch * 256 + threadIdx.x] = run;
        run = max(run, v);
    }
}

__global__ __launch_bounds__(256) void k_pdc_carry_c(uint32_t *__restrict__ tile_last, uint32_t ntiles, uint32_t tpc, const uint32_t *__restrict__ chunk_max) {
    uint32_t run = chunk_max[blockIdx.x * 256 + threadIdx.x];
    const uint32_t t0 = blockIdx.x * tpc;
    for (uint32_t t = t0; t < t0 + tpc && t < ntiles; ++t) {
        const size_t at = static_cast<size_t>(t) * 256 + threadIdx.x;
        const uint32_t v = tile_last[at];
        tile_last[at] = run;
        run = max(run, v);
    }
}

__global__ __launch_bounds__(256) void k_pdc_init_fill(const uint32_t *__restrict__ off, uint32_t *__restrict__ init) {
    const uint32_t blk = blockIdx.x;
    init[static_cast<size_t>(blk) * 256 + threadIdx.x] = off[blk + 1] - off[blk];
}

// compact = true: entries at their global run index (block i at [rb_i, rb_i + m_i)); false: at [off_i, off_i + m_i)
__global__ __launch_bounds__(PDC_WAVES * 64) void k_pdc_main(const uint32_t *__restrict__ run_st, const uint8_t *__restrict__ run_sym, uint32_t m,
                                                              const uint32_t *__restrict__ rb, const uint32_t *__restrict__ off, uint32_t count,
                                                              const uint32_t *__restrict__ tile_carry, int compact, uint32_t *__restrict__ dist,
                                                              uint8_t *__restrict__ sym, uint8_t *__restrict__ rank_out, uint32_t *__restrict__ run_end,
                                                              uint8_t *__restrict__ has_next, uint32_t *__restrict__ init) {
    __shared__ uint32_t s_table[PDC_WAVES][256];
    __shared__ uint32_t s_prev[PDC_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t tile = blockIdx.x * PDC_WAVES + wave;
    const uint32_t ntiles = (m + PDC_TILE - 1) / PDC_TILE;
    if (tile >= ntiles) return;  // whole wave
    uint32_t *table = s_table[wave];
    uint32_t *sp = s_prev[wave];
    for (int k = 0; k < 4; ++k) table[k * 64 + lane] = tile_carry[static_cast<size_t>(tile) * 256 + k * 64 + lane];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t base = tile * PDC_TILE;
    for (uint32_t cb = base; cb < base + PDC_TILE && cb < m; cb += 64) {
        const uint32_t q = cb + lane;
        const bool valid = q < m;
        const uint32_t c = valid ? run_sym[q] : 0u;
        uint64_t same = __ballot(valid);
        for (int b = 0; b < 8; ++b) {
            const uint64_t bm = __ballot((c >> b) & 1u);
            same &= ((c >> b) & 1u) ? bm : ~bm;
        }
        const uint64_t lower = same & lanemask_lt(lane);
        const uint32_t prevv = lower ? cb + (63u - static_cast<uint32_t>(__builtin_clzll(lower))) + 1u : table[c];  // previous run of c, + 1
        const uint32_t blk = valid ? seg_of(rb, count, q) : 0u;
        const uint32_t rbq = rb[blk];
        const bool hasprev = valid && prevv > rbq;
        sp[lane] = prevv;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        uint32_t rank = 0;
        // symbols whose last occurrence before this step lies past the previous run of c (prevv - 1)
        const bool need = hasprev && prevv <= cb;
        if (__any(need)) {
            for (int i = 0; i < 256; ++i) rank += (need && table[i] > prevv) ? 1u : 0u;
        }
        // earlier lanes of this step past prevv - 1 whose own symbol did not occur since then
        for (int j = 0; j < lane; ++j) rank += (hasprev && cb + j >= prevv && sp[j] <= prevv) ? 1u : 0u;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint64_t higher = same & ~(lanemask_lt(lane) | (1ull << lane));
        if (valid && !higher) table[c] = q + 1;
        if (valid) {
            const uint32_t s = off[blk];
            const uint32_t o = compact ? q : s + (q - rbq);
            sym[o] = static_cast<uint8_t>(c);
            if (rank_out) rank_out[o] = static_cast<uint8_t>(hasprev ? rank : 0u);
            if (run_end) run_end[o] = run_st[q + 1] - 1 - s;
            if (hasprev) {
                const uint32_t b = prevv - 1;
                dist[compact ? b : s + (b - rbq)] = run_st[q] - run_st[b + 1] - rank;
                has_next[b] = 1;
            } else {
                init[static_cast<size_t>(blk) * 256 + c] = run_st[q] - s;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// every block's last run of each symbol, listed at [rb_i, rb_i + distinct_i)
__global__ __launch_bounds__(256) void k_pdc_finlist(const uint8_t *__restrict__ has_next, uint32_t m, const uint32_t *__restrict__ rb, uint32_t count,
                                                     uint32_t *__restrict__ fcnt, uint32_t *__restrict__ flist) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m || has_next[r]) return;
    const uint32_t blk = seg_of(rb, count, r);
    flist[rb[blk] + atomicAdd(&fcnt[blk], 1u)] = r;
}

// one workgroup per block: the final sweep's distances, m_i and the flags
__global__ __launch_bounds__(256) void k_pdc_final(const uint32_t *__restrict__ run_st, const uint8_t *__restrict__ run_sym, const uint32_t *__restrict__ rb,
                                                   const uint32_t *__restrict__ off, const uint32_t *__restrict__ fcnt, const uint32_t *__restrict__ flist,
                                                   int compact, uint32_t *__restrict__ dist, uint32_t *__restrict__ m_out, uint32_t *__restrict__ flags_out) {
    __shared__ uint32_t s_ff;
    const uint32_t blk = blockIdx.x;
    const uint32_t f = fcnt[blk], r0 = rb[blk];
    if (threadIdx.x == 0) s_ff = 0;
    __syncthreads();
    if (threadIdx.x < f) {
        const uint32_t r = flist[r0 + threadIdx.x];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < f; ++j) rank += flist[r0 + j] > r ? 1u : 0u;
        dist[compact ? r : off[blk] + (r - r0)] = off[blk + 1] - run_st[r + 1] - rank;
        if (run_sym[r] == 0xFF) s_ff = 1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        m_out[blk] = rb[blk + 1] - r0;
        flags_out[blk] = (s_ff ? DK_FLAG_HAS_FF : 0u) | (f == 1 ? DK_FLAG_SINGLE_SYMBOL : 0u);
    }
}

// The buffers of one segmented sort over `entries` list entries (the first step: the whole pack), and the pack they belong to.
struct PkSort {
    dk_ctx *ctx;
    const uint32_t *d_off;
    uint32_t cnt;
    size_t total;
    uint64_t *keys, *keys_alt;  // the sorted list stands in keys / vals behind every step (sort_pairs swaps each pair as it needs)
    uint32_t *vals, *vals_alt;
    GroupAgg *agg;              // one per tile of the list
};

// what the first step chose: the pack's alphabet, the key's layout and the bit the sort ended at
struct PkFirst { uint32_t sigma; int bits, blk_bits, k_used, end_bit; };

// one scan over the sorted list keys / vals of c entries: ranks written, live entries (order kept) into next_act; *live = their number
int pk_regroup(const PkSort &s, uint32_t c, int rbits, uint32_t *rank, uint32_t *next_act, uint32_t *live) {
    dk_ctx *ctx = s.ctx;
    hipStream_t st = ctx->stream;
    uint32_t *d_live = &ctx->d_mail->packed.live;
    const uint32_t ntiles = static_cast<uint32_t>(div_up(c, PK_TILE));
    {
        LaunchScope ls(ctx, K_RERANK_REDUCE, 8.0 * c);
        k_pk_tile_sum<<<dim3(ntiles), dim3(PK_BLOCK), 0, st>>>(s.keys, c, rbits, s.agg);
    }
    {
        LaunchScope ls(ctx, K_RERANK_SCAN, 32.0 * ntiles);
        k_pk_spine<<<dim3(1), dim3(1024), 0, st>>>(s.agg, ntiles, d_live);
    }
    {
        LaunchScope ls(ctx, K_RERANK_APPLY, 20.0 * c);
        k_pk_tile_apply<<<dim3(ntiles), dim3(PK_BLOCK), 0, st>>>(s.keys, s.vals, c, rbits, s.agg, rank, next_act);
    }
    DK_HIP(ctx, hipGetLastError());
    DK_TRY(ctx->mail_read(&ctx->h_mail->packed.live));
    *live = ctx->h_mail->packed.live;
    return DK_OK;
}

// The first step: the pack's code table (present: 256 words, code: 256 codes, both on the device), the first keys of every suffix, their sort and
// the first regroup: rank[p] for every p, the members of groups of two or more into act.
int pk_first(PkSort &s, const uint8_t *d_text, uint32_t *present, uint16_t *code, uint32_t *rank, uint32_t *act, PkFirst *f, uint32_t *live) {
    dk_ctx *ctx = s.ctx;
    hipStream_t st = ctx->stream;
    const size_t total = s.total;
    uint32_t *d_live = &ctx->d_mail->packed.live;
    DK_HIP(ctx, hipMemsetAsync(present, 0, 256 * sizeof(uint32_t), st));
    {
        LaunchScope ls(ctx, K_SYM_HIST, 1.0 * total);
        k_pk_hist<<<dim3(static_cast<unsigned>(std::min<size_t>(div_up(total, 256), 1024))), dim3(256), 0, st>>>(d_text, total, present);
        k_pk_codes<<<dim3(1), dim3(256), 0, st>>>(present, code, d_live);
    }
    DK_HIP(ctx, hipGetLastError());
    DK_TRY(ctx->mail_read(&ctx->h_mail->packed.live));
    f->sigma = ctx->h_mail->packed.live;
    f->bits = static_cast<int>(std::max(1u, ceil_log2_u64(static_cast<uint64_t>(f->sigma) + 1)));
    f->blk_bits = static_cast<int>(ceil_log2_u64(s.cnt));
    const int k = std::max(1, (64 - f->blk_bits) / f->bits);
    // a key of k symbols resolves k symbols: no point in more than the longest block
    f->k_used = static_cast<int>(std::min<uint64_t>(k, std::max<uint64_t>(1, total)));
    f->end_bit = f->blk_bits + f->bits * f->k_used;
    {
        LaunchScope ls(ctx, K_RADIX_SCATTER_TEXT, 9.0 * total);
        k_pk_init_keys<<<dim3(static_cast<unsigned>(div_up(total, 256))), dim3(256), 0, st>>>(d_text, s.d_off, s.cnt, static_cast<uint32_t>(total), code, f->bits,
                                                                                             f->k_used, s.keys, s.vals);
    }
    DK_HIP(ctx, hipGetLastError());
    DK_TRY(sort_pairs(ctx, s.keys, s.keys_alt, s.vals, s.vals_alt, total, 0, f->end_bit));
    return pk_regroup(s, static_cast<uint32_t>(total), 64, rank, act, live);
}

// One round at depth h on the list act[0, c): the round keys, their sort, the regroup.  next_act may be act itself (the keys are complete before
// the scan writes the next list).  *rbits_out (may be null): the width of rank2 in the key.
int pk_round(PkSort &s, const uint32_t *act, uint32_t c, uint64_t h, uint32_t *rank, uint32_t *next_act, int *rbits_out, uint32_t *live) {
    dk_ctx *ctx = s.ctx;
    const int rbits = static_cast<int>(ceil_log2_u64(s.total + h));
    const int gbits = static_cast<int>(ceil_log2_u64(s.total));
    {
        LaunchScope ls(ctx, K_ROUND_LOCAL, 20.0 * c);
        k_pk_round_keys<<<dim3(static_cast<unsigned>(div_up(c, 256))), dim3(256), 0, ctx->stream>>>(act, c, rank, s.d_off, s.cnt, static_cast<uint32_t>(h), rbits,
                                                                                                    s.keys, s.vals);
    }
    DK_HIP(ctx, hipGetLastError());
    DK_TRY(sort_pairs(ctx, s.keys, s.keys_alt, s.vals, s.vals_alt, c, 0, rbits + gbits));
    if (rbits_out) *rbits_out = rbits;
    return pk_regroup(s, c, rbits, rank, next_act, live);
}

// The guard: d_guard[i] = 1 for the blocks that hold a suffix of act[0, live), 0 for the others
int pk_guard(const PkSort &s, const uint32_t *act, uint32_t live, uint32_t *d_guard) {
    dk_ctx *ctx = s.ctx;
    DK_HIP(ctx, hipMemsetAsync(d_guard, 0, s.cnt * sizeof(uint32_t), ctx->stream));
    if (live > 0) {
        LaunchScope ls(ctx, K_RERANK_APPLY, 8.0 * live);
        k_pk_guard_mark<<<dim3(static_cast<unsigned>(div_up(live, 256))), dim3(256), 0, ctx->stream>>>(act, live, s.d_off, s.cnt, d_guard);
    }
    DK_HIP(ctx, hipGetLastError());
    return DK_OK;
}

// The segmented suffix sort, up to and including the guard: *rank_out[p] = the final slot of suffix p (the first slot of its group for the
// members of a group still unresolved after max_rounds), d_guard[i] = 1 for the blocks that hold such a group, *guarded = their suffixes.
// rank lives in the workspace together with the sort's temporaries: the caller takes ws_mark() before the call and releases it once it
// has emitted what it wants from rank.  The steps are pk_first, pk_round and pk_guard, which dk_dbg_dev_packed_first / _round run one at a time.
int packed_sort_device(dk_ctx *ctx, const uint8_t *d_text, const uint32_t *d_off, size_t count, size_t total, uint32_t *d_guard, int max_rounds,
                       const uint32_t **rank_out, size_t *guarded) {
    uint64_t *keys = ctx->ws_alloc<uint64_t>(total), *keys_alt = ctx->ws_alloc<uint64_t>(total);
    uint32_t *vals = ctx->ws_alloc<uint32_t>(total), *vals_alt = ctx->ws_alloc<uint32_t>(total);
    uint32_t *act = ctx->ws_alloc<uint32_t>(total), *rank = ctx->ws_alloc<uint32_t>(total);
    GroupAgg *agg = ctx->ws_alloc<GroupAgg>(div_up(total, PK_TILE));
    uint32_t *present = ctx->ws_alloc<uint32_t>(256);
    uint16_t *code = ctx->ws_alloc<uint16_t>(256);
    if (!keys || !keys_alt || !vals || !vals_alt || !act || !rank || !agg || !present || !code) return DK_E_NOMEM;
    PkSort s{ctx, d_off, static_cast<uint32_t>(count), total, keys, keys_alt, vals, vals_alt, agg};
    PkFirst f{};
    uint32_t live = 0;
    DK_TRY(pk_first(s, d_text, present, code, rank, act, &f, &live));
    uint64_t h = static_cast<uint64_t>(f.k_used);
    uint32_t rounds = 0;
    while (live > 0 && static_cast<int>(rounds) < max_rounds) {
        DK_TRY(pk_round(s, act, live, h, rank, act, nullptr, &live));
        h *= 2;
        ++rounds;
    }
    ctx->stats.rounds = rounds;
    DK_TRY(pk_guard(s, act, live, d_guard));
    *rank_out = rank;
    *guarded = live;
    return DK_OK;
}

}  // namespace

int packed_bwt_device(dk_ctx *ctx, const uint8_t *d_text, const uint32_t *d_off, size_t count, size_t total, uint8_t *d_bwt, uint32_t *d_origin,
                      uint32_t *d_guard, int max_rounds, size_t *guarded) {
    const size_t mark = ctx->ws_mark();
    const uint32_t *rank = nullptr;
    DK_TRY(packed_sort_device(ctx, d_text, d_off, count, total, d_guard, max_rounds, &rank, guarded));
    {
        LaunchScope ls(ctx, K_BWT_GATHER, 6.0 * total);
        k_pk_scatter<<<dim3(static_cast<unsigned>(div_up(total, 256))), dim3(256), 0, ctx->stream>>>(
            d_text, d_off, static_cast<uint32_t>(count), static_cast<uint32_t>(total), rank, d_bwt, d_origin);
    }
    DK_HIP(ctx, hipGetLastError());
    ctx->ws_release(mark);
    return DK_OK;
}

int packed_sa_device(dk_ctx *ctx, const uint8_t *d_text, const uint32_t *d_off, size_t count, size_t total, uint32_t *d_sa, uint8_t *d_bwt,
                     uint32_t *d_origin, uint32_t *d_guard, int max_rounds, size_t *guarded, uint32_t *d_phi) {
    const size_t mark = ctx->ws_mark();
    const uint32_t *rank = nullptr;
    DK_TRY(packed_sort_device(ctx, d_text, d_off, count, total, d_guard, max_rounds, &rank, guarded));
    {
        LaunchScope ls(ctx, K_BWT_GATHER, (d_bwt ? 10.0 : 8.0) * total);
        k_pk_emit<<<dim3(static_cast<unsigned>(div_up(total, 256))), dim3(256), 0, ctx->stream>>>(
            d_text, d_off, static_cast<uint32_t>(count), static_cast<uint32_t>(total), rank, d_sa, d_bwt, d_origin);
    }
    DK_HIP(ctx, hipGetLastError());
    if (d_phi) DK_TRY(lcp_phi_from_rank_device(ctx, rank, d_sa, d_off, count, total, d_phi));  // rank is the inverse suffix array: no second one
    ctx->ws_release(mark);
    return DK_OK;
}

// dk_dbg_dev_packed_first (abi.cpp has checked the arguments): pk_first() on the caller's pack.  rank and act are the caller's arrays; the sort's
// four buffers, the tile aggregates and the code table are the workspace's, the sorted list and the table are copied out.
int dbg_packed_first_device(dk_ctx *ctx, const DbgPackedFirst &a, uint32_t out[8]) {
    const size_t total = a.total, mark = ctx->ws_mark();
    hipStream_t st = ctx->stream;
    uint64_t *keys = ctx->ws_alloc<uint64_t>(total), *keys_alt = ctx->ws_alloc<uint64_t>(total);
    uint32_t *vals = ctx->ws_alloc<uint32_t>(total), *vals_alt = ctx->ws_alloc<uint32_t>(total);
    GroupAgg *agg = ctx->ws_alloc<GroupAgg>(div_up(total, PK_TILE));
    uint32_t *present = ctx->ws_alloc<uint32_t>(256);
    uint16_t *code = ctx->ws_alloc<uint16_t>(256);
    if (!keys || !keys_alt || !vals || !vals_alt || !agg || !present || !code) return DK_E_NOMEM;
    PkSort s{ctx, a.off, static_cast<uint32_t>(a.count), total, keys, keys_alt, vals, vals_alt, agg};
    PkFirst f{};
    uint32_t live = 0;
    DK_TRY(pk_first(s, a.text, present, code, a.rank, a.act, &f, &live));
    DK_HIP(ctx, hipMemcpyAsync(a.keys, s.keys, total * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    DK_HIP(ctx, hipMemcpyAsync(a.vals, s.vals, total * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    uint16_t h_code[256];
    DK_HIP(ctx, hipMemcpyAsync(h_code, code, sizeof h_code, hipMemcpyDeviceToHost, st));
    DK_HIP(ctx, hipStreamSynchronize(st));
    std::copy(h_code, h_code + 256, a.code_out);
    out[0] = f.sigma, out[1] = static_cast<uint32_t>(f.bits), out[2] = static_cast<uint32_t>(f.blk_bits), out[3] = static_cast<uint32_t>(f.k_used);
    out[4] = live, out[5] = static_cast<uint32_t>(f.end_bit), out[6] = 0, out[7] = 0;
    ctx->ws_release(mark);
    return DK_OK;
}

// dk_dbg_dev_packed_round (abi.cpp has checked the arguments): pk_round() on the caller's list and ranks, then pk_guard() on the next list when
// the guard words are asked for.  The sort's buffers for c entries are the workspace's; the sorted list is copied out.
int dbg_packed_round_device(dk_ctx *ctx, const DbgPackedRound &a, uint32_t out[8]) {
    const size_t c = a.c, mark = ctx->ws_mark();
    hipStream_t st = ctx->stream;
    uint64_t *keys = ctx->ws_alloc<uint64_t>(c), *keys_alt = ctx->ws_alloc<uint64_t>(c);
    uint32_t *vals = ctx->ws_alloc<uint32_t>(c), *vals_alt = ctx->ws_alloc<uint32_t>(c);
    GroupAgg *agg = ctx->ws_alloc<GroupAgg>(div_up(c, PK_TILE));
    if (!keys || !keys_alt || !vals || !vals_alt || !agg) return DK_E_NOMEM;
    PkSort s{ctx, a.off, static_cast<uint32_t>(a.count), a.total, keys, keys_alt, vals, vals_alt, agg};
    int rbits = 0;
    uint32_t live = 0;
    DK_TRY(pk_round(s, a.act, static_cast<uint32_t>(c), a.h, a.rank, a.next_act, &rbits, &live));
    if (a.guard) DK_TRY(pk_guard(s, a.next_act, live, a.guard));
    DK_HIP(ctx, hipMemcpyAsync(a.keys, s.keys, c * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    DK_HIP(ctx, hipMemcpyAsync(a.vals, s.vals, c * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    DK_HIP(ctx, hipStreamSynchronize(st));
    out[0] = static_cast<uint32_t>(rbits), out[1] = ceil_log2_u64(a.total), out[2] = live;
    for (int i = 3; i < 8; ++i) out[i] = 0;
    ctx->ws_release(mark);
    return DK_OK;
}

int packed_dc_device(dk_ctx *ctx, const uint8_t *d_bwt, const uint32_t *d_off, size_t count, size_t total, bool compact, uint32_t *d_dist,
                     uint8_t *d_sym, uint8_t *d_rank, uint32_t *d_run_end, uint32_t *d_m, uint32_t *d_flags, uint32_t *d_rb, uint32_t *d_init) {
    hipStream_t st = ctx->stream;
    const uint32_t cnt = static_cast<uint32_t>(count), T = static_cast<uint32_t>(total);
    const size_t mark = ctx->ws_mark();
    const uint32_t ptiles = static_cast<uint32_t>(div_up(total, PK_TILE));
    // runs are at most the positions: every run-sized array is sized by the pack
    const uint32_t rtiles = static_cast<uint32_t>(div_up(total, PDC_TILE));
    const uint32_t tpc = static_cast<uint32_t>(div_up(rtiles, PDC_MAX_CHUNKS));
    uint32_t *tile_cnt = ctx->ws_alloc<uint32_t>(ptiles);
    uint32_t *run_st = ctx->ws_alloc<uint32_t>(total + 1);
    uint8_t *run_sym = ctx->ws_alloc<uint8_t>(total);
    uint8_t *has_next = ctx->ws_alloc<uint8_t>(total);
    uint32_t *tile_last = ctx->ws_alloc<uint32_t>(static_cast<size_t>(rtiles) * 256);
    uint32_t *chunk_max = ctx->ws_alloc<uint32_t>(static_cast<size_t>(PDC_MAX_CHUNKS) * 256);
    uint32_t *fcnt = ctx->ws_alloc<uint32_t>(count);
    uint32_t *flist = ctx->ws_alloc<uint32_t>(total);
    if (!tile_cnt || !run_st || !run_sym || !has_next || !tile_last || !chunk_max || !fcnt || !flist) return DK_E_NOMEM;
    {
        LaunchScope ls(ctx, K_DC_SUMMARY, 1.0 * total);
        k_pdc_count<<<dim3(ptiles), dim3(PK_BLOCK), 0, st>>>(d_bwt, d_off, cnt, T, tile_cnt);
    }
    {
        LaunchScope ls(ctx, K_DC_CARRY, 8.0 * ptiles);
        k_pk_scan_u32<<<dim3(1), dim3(1024), 0, st>>>(tile_cnt, ptiles);
    }
    {
        LaunchScope ls(ctx, K_DC_SUMMARY, 6.0 * total);
        k_pdc_runs<<<dim3(ptiles), dim3(PK_BLOCK), 0, st>>>(d_bwt, d_off, cnt, T, tile_cnt, run_st, run_sym, d_rb);
    }
    DK_HIP(ctx, hipGetLastError());
    // the run count is not read back: kernels over the runs are sized by the pack and read the count from d_rb[count]
    DK_TRY(ctx->mail_read(&ctx->h_mail->packed.dc_runs, d_rb + count));
    const uint32_t m = ctx->h_mail->packed.dc_runs;
    const uint32_t mtiles = static_cast<uint32_t>(div_up(m, PDC_TILE));
    const uint32_t nchunks = static_cast<uint32_t>(div_up(mtiles, tpc));
    DK_HIP(ctx, hipMemsetAsync(has_next, 0, m, st));
    DK_HIP(ctx, hipMemsetAsync(fcnt, 0, count * sizeof(uint32_t), st));
    {
        LaunchScope ls(ctx, K_DC_SUMMARY, 1.0 * m + 1024.0 * mtiles);
        k_pdc_summary<<<dim3(mtiles), dim3(PK_BLOCK), 0, st>>>(run_sym, m, tile_last);
    }
    {
        LaunchScope ls(ctx, K_DC_CARRY, 3.0 * 1024.0 * mtiles);
        k_pdc_carry_a<<<dim3(nchunks), dim3(256), 0, st>>>(tile_last, mtiles, tpc, chunk_max);
        k_pdc_carry_b<<<dim3(1), dim3(256), 0, st>>>(chunk_max, nchunks);
        k_pdc_carry_c<<<dim3(nchunks), dim3(256), 0, st>>>(tile_last, mtiles, tpc, chunk_max);
    }
    {
        LaunchScope ls(ctx, K_DC_INIT, 1024.0 * count);
        k_pdc_init_fill<<<dim3(cnt), dim3(256), 0, st>>>(d_off, d_init);
    }
    {
        LaunchScope ls(ctx, K_DC_MAIN, 15.0 * m + 1024.0 * mtiles);
        k_pdc_main<<<dim3(static_cast<unsigned>(div_up(mtiles, PDC_WAVES))), dim3(PDC_WAVES * 64), 0, st>>>(
            run_st, run_sym, m, d_rb, d_off, cnt, tile_last, compact ? 1 : 0, d_dist, d_sym, d_rank, d_run_end, has_next, d_init);
    }
    {
        LaunchScope ls(ctx, K_DC_INIT, 9.0 * m);
        k_pdc_finlist<<<dim3(static_cast<unsigned>(div_up(m, 256))), dim3(256), 0, st>>>(has_next, m, d_rb, cnt, fcnt, flist);
        k_pdc_final<<<dim3(cnt), dim3(256), 0, st>>>(run_st, run_sym, d_rb, d_off, fcnt, flist, compact ? 1 : 0, d_dist, d_m, d_flags);
    }
    DK_HIP(ctx, hipGetLastError());
    ctx->stats.dc_runs = m;
    ctx->ws_release(mark);
    return DK_OK;
}

}  // namespace dk
