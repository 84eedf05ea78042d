// Counting the occurrences of patterns in a BWT without the text and without a suffix array: backward search (Ferragina, Manzini: Opportunistic
// data structures with applications, FOCS 2000) on L itself, for one block or a pack.  Nothing in the reference
// corresponds.  Conventions are those of bwt.hip: L[i] = T[SA[i] - 1], and T[n - 1] at the slot `origin` where SA[origin] = 0; no sentinel, a
// suffix that is a proper prefix of another sorts first.  Block b's L sits at bwt[off_b, off_b + n_b); a single block is a pack of one.
//
// THE RECURRENCE.  hist[c] = occurrences of c in L, C[c] = sum of hist below c, last = L[origin] = T[n - 1], Occ(c, i) = #{k < i : L[k] = c},
// Occ'(c, i) = Occ(c, i) - [c == last && origin < i] (the origin's symbol is a wrap-around, not a predecessor).  For P of m bytes, from its last
// byte to its first:  first step  lo = C[c], hi = C[c] + hist[c];  every later step  x <- C[c] + [c == last] + Occ'(c, x)  for x = lo and hi (the
// [c == last] term is the one-byte suffix T[n-1..], first of its class, which has no slot to come from).  lo = suffixes <m P, hi = suffixes <=m P:
// the numbers of sa_query.hip.  With base_b[c] = C_b[c] - Occ_pack(c, off_b) (the cancellation of section 4.8) a step is
//     x <- base_b[c] + [c == last_b] - [c == last_b && origin_b < x] + Occ_pack(c, off_b + x)
// and the first step is that very step from (0, n_b) with the [c == last_b] term left out of lo: C_b[c] = base_b[c] + Occ_pack(c, off_b), and
// origin_b < n_b cancels the two terms of hi.  So the index holds no per-block histogram.
//
// THE INDEX (32-bit words; fm_index_words is its size):
//   [0, 64)                        header: magic, total, count, rows
//   [64, 64 + 256 rows)            checkpoints: row k = Occ_pack(c, k * FM_BLOCK) for every c, rows = ceil(total / FM_BLOCK) + 1, on a grid over the
//                                  whole pack (blocks are not aligned to it)
//   [.., + 4 count)                per block {off, n, origin, last}
//   [.., + 256 count)              per block base_b[256]
// Occ_pack(c, x) = checkpoint[x / FM_BLOCK][c] + occurrences of c in L[x / FM_BLOCK * FM_BLOCK, x): one gathered word, and at most FM_BLOCK - 1
// bytes of L of which every lane of a wave compares 16.
//
// BUILD    k_fm_hist       a workgroup per four rows, a wave per row: the histogram of the row's FM_BLOCK bytes in LDS, four copies per wave
//                          (L is made of runs: LDS atomics of one instruction on one counter are serialised)
//          k_fm_scan_a/b/c the column-wise exclusive scan of the rows in at most FM_MAX_CHUNKS chunks (the shape of k_ibwt_scan_*)
//          k_fm_heads      a workgroup per block, a lane per symbol: Occ_pack at the block's head and end from the checkpoints plus at most one
//                          row's bytes each, their difference scanned over the symbols = C_b; writes base_b and the block's four words
// COUNT    k_fm_count      a wave per pattern, FM_WAVES per workgroup, grid stride; m dependent steps of one or two ranks
//          k_fm_rank       the same rank for given (position, symbol) pairs -- the tests' view of it
// LOCATE   k_fm_locate     a wave per (pattern, hit); at most min(step, n_b) dependent LF steps down to a sampled slot (section 4.14; the sampled
//                          suffix array it reads is built in bwt.hip by the inverse's kernels: fm_locate_build_device)
// EXTRACT  k_fm_extract    a wave per (range, chunk of `step` positions): from the chunk's end, whose slot is an anchor, at most min(step, n_b) - 1
//                          of the same LF steps backwards, a text byte per step (section 4.15; anchors built in bwt.hip: fm_extract_build_device)
// SEAMS    k_fm_seam_count a wave per pair (pattern, block): the candidates `back` of the border in front of the block, 64 at a time, compared
//                          against an edge strip that k_fm_extract filled (section 4.17); k_fm_find_scan_a/b/c; k_fm_seam_emit the same
//                          compare again, every hit lane stores its record at the pair's offset plus its rank in the ballot
// FIND     k_fm_find_count a wave per pair (pattern, block) of the grid npat x count: the count's search, lo and occ of the pair (section 4.16)
//          k_fm_find_scan_a/b/c  the exclusive scan of occ over the pairs in 64-bit sums, the grand total to the mailbox
//          k_fm_find_locate a wave per hit: the pair from the offsets by a 64-ary search, then the walk of k_fm_locate; one 16-byte record
// NEAR     k_fm_near_count a wave per pair: backward search that branches over byte classes and a budget of mismatches, depth first with a
//                          stack in LDS (section 4.18); k_fm_find_scan_a/b/c; k_fm_near_emit the same walk again, every leaf's records at the
//                          pair's offset; k_fm_near_locate a wave per record, the walk of k_fm_locate from the staged slot
// Containment: the geometry (off, n, total) comes from the caller, never from the index; every position is clamped to [0, n_b] before it is used
// and a rank reads L only below the position it counts to.  With an index or an L that is not what the build made the results are unspecified
// but <= n_b, and nothing outside L, the index, the patterns and the two results is touched.
#include <algorithm>

#include "context.hpp"
#include "device_util.hpp"

namespace dk {

size_t fm_index_words(size_t total, size_t count) {
    return 64 + 256 * (div_up(total, 1024) + 1) + 4 * count + 256 * count;
}

namespace {

// Positions per checkpoint row.  UNMEASURED: chosen so that one 16-byte load per lane of a wave covers a row, and the checkpoints cost
// 256 * 4 / 1024 = 1 byte per byte of L.
constexpr uint32_t FM_BLOCK = 1024;
constexpr uint32_t FM_SHIFT = 10;
static_assert(FM_BLOCK == 64 * 16 && (1u << FM_SHIFT) == FM_BLOCK, "a lane compares 16 bytes of a row");
constexpr uint32_t FM_WAVES = 4;          // rows per workgroup of k_fm_hist; patterns per workgroup of k_fm_count
constexpr size_t FM_MAX_CHUNKS = 256;
constexpr uint32_t FM_MAGIC = 0x31494D46u;  // "FMI1"
constexpr uint32_t FM_HEADER = 64;

struct FmIndex { uint32_t *blocks, *base, *cp; size_t rows; };
FmIndex fm_carve(void *d_index, size_t total, size_t count) {
    uint32_t *w = static_cast<uint32_t *>(d_index);
    const size_t rows = div_up(total, FM_BLOCK) + 1;
    return FmIndex{w + FM_HEADER + 256 * rows, w + FM_HEADER + 256 * rows + 4 * count, w + FM_HEADER, rows};
}

typedef uint64_t __attribute__((aligned(1))) unaligned_u64;
typedef const unaligned_u64 __attribute__((address_space(1))) *gptr8;

// the 16 bytes at L[s, s + 16) as two little-endian words; only the first k <= 16 of them are looked at afterwards.  L has any alignment.
// Where 16 bytes do not fit below `total` the k bytes are read one by one (k <= total - s: the caller's).
__device__ __forceinline__ void fm_load16(const uint8_t *__restrict__ L, uint32_t total, uint32_t s, uint32_t k, uint64_t &a, uint64_t &b) {
    a = b = 0;
    if (k == 0) return;
    if (total - s >= 16u) {
        a = *(gptr8)(L + s);
        b = *(gptr8)(L + s + 8);
    } else {
        for (uint32_t i = 0; i < k; ++i) {
            const uint64_t v = L[s + i];
            if (i < 8) a |= v << (8 * i);
            else b |= v << (8 * (i - 8));
        }
    }
}
// one bit (the top one) per byte of v that equals the byte spread over `cc`
__device__ __forceinline__ uint64_t fm_eq8(uint64_t v, uint64_t cc) {
    const uint64_t x = v ^ cc, low7 = 0x7F7F7F7F7F7F7F7Full;
    return ~(((x & low7) + low7) | x | low7);
}
// how many of the first k <= 16 bytes of (a, b) equal the symbol
__device__ __forceinline__ uint32_t fm_count16(uint64_t a, uint64_t b, uint64_t cc, uint32_t k) {
    const uint32_t ka = k < 8u ? k : 8u, kb = k - ka;
    const uint64_t ma = ka == 8u ? ~0ull : (1ull << (8 * ka)) - 1ull, mb = kb == 8u ? ~0ull : (1ull << (8 * kb)) - 1ull;
    return static_cast<uint32_t>(__popcll(fm_eq8(a, cc) & ma) + __popcll(fm_eq8(b, cc) & mb));
}
// of the row's bytes below x (x - row start <= FM_BLOCK... < FM_BLOCK by construction), how many this lane looks at
__device__ __forceinline__ uint32_t fm_lane_bytes(uint32_t x, uint32_t s) { return x > s ? (x - s < 16u ? x - s : 16u) : 0u; }

// Occ_pack(c, x) and Occ_pack(c, y) for x <= y <= total, by the whole wave; every lane gets both.  The loads of both positions are issued
// before either is used; one load serves both where they share a row.  (x > y, from an index that is no index: still inside L, both <= total.)
__device__ __forceinline__ void fm_rank2(const uint8_t *__restrict__ L, uint32_t total, const uint32_t *__restrict__ cp, uint32_t c, uint32_t x, uint32_t y,
                                         uint32_t lane, uint32_t &rx, uint32_t &ry) {
    const uint32_t row_x = x >> FM_SHIFT, row_y = y >> FM_SHIFT;
    const uint64_t cc = 0x0101010101010101ull * c;
    const uint32_t sx = (row_x << FM_SHIFT) + 16u * lane, sy = (row_y << FM_SHIFT) + 16u * lane;
    const uint32_t kx = fm_lane_bytes(x, sx), ky = fm_lane_bytes(y, sy);
    const uint32_t base_x = cp[static_cast<size_t>(row_x) * 256 + c];
    uint32_t base_y = base_x, packed;
    uint64_t a, b;
    if (row_x == row_y) {
        fm_load16(L, total, sx, kx > ky ? kx : ky, a, b);
        packed = fm_count16(a, b, cc, kx) | (fm_count16(a, b, cc, ky) << 16);
    } else {
        uint64_t a2, b2;
        base_y = cp[static_cast<size_t>(row_y) * 256 + c];
        fm_load16(L, total, sx, kx, a, b);
        fm_load16(L, total, sy, ky, a2, b2);
        packed = fm_count16(a, b, cc, kx) | (fm_count16(a2, b2, cc, ky) << 16);
    }
    packed = wave_sum(packed);  // (each half stays below FM_BLOCK)
    rx = base_x + (packed & 0xFFFFu);
    ry = base_y + (packed >> 16);
}
__device__ __forceinline__ uint32_t fm_rank1(const uint8_t *__restrict__ L, uint32_t total, const uint32_t *__restrict__ cp, uint32_t c, uint32_t x,
                                             uint32_t lane) {
    const uint32_t row = x >> FM_SHIFT, s = (row << FM_SHIFT) + 16u * lane, k = fm_lane_bytes(x, s);
    uint64_t a, b;
    fm_load16(L, total, s, k, a, b);
    return cp[static_cast<size_t>(row) * 256 + c] + wave_sum(fm_count16(a, b, 0x0101010101010101ull * c, k));
}

// ---- build ----------------------------------------------------------------------------------------------------------------------------------

// row r of cp = the histogram of L[r * FM_BLOCK, (r + 1) * FM_BLOCK) (nothing behind `total`: the last row, and every row a grid rounded up
// to FM_WAVES adds, count no byte -- the rows behind `rows` are not written)
__global__ __launch_bounds__(64 * FM_WAVES) void k_fm_hist(const uint8_t *__restrict__ L, uint32_t total, uint32_t *__restrict__ cp, uint32_t rows) {
    __shared__ uint32_t h[FM_WAVES][4][256];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < FM_WAVES * 4 * 256; i += 64 * FM_WAVES) (&h[0][0][0])[i] = 0;
    __syncthreads();
    const uint32_t row = blockIdx.x * FM_WAVES + wave;
    const uint64_t s64 = (static_cast<uint64_t>(row) << FM_SHIFT) + 16u * lane;
    if (row < rows && s64 < total) {
        const uint32_t s = static_cast<uint32_t>(s64), k = total - s < 16u ? total - s : 16u;
        uint64_t a, b;
        fm_load16(L, total, s, k, a, b);
        uint32_t *mine = h[wave][lane & 3u];
        for (uint32_t i = 0; i < k; ++i) atomicAdd(&mine[((i < 8 ? a >> (8 * i) : b >> (8 * (i - 8)))) & 0xFFu], 1u);
    }
    __syncthreads();
    if (row < rows) {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t c = lane + 64u * j;
            cp[static_cast<size_t>(row) * 256 + c] = h[wave][0][c] + h[wave][1][c] + h[wave][2][c] + h[wave][3][c];
        }
    }
}
// exclusive scan down every column of the rows, in chunks of rpc rows
__global__ __launch_bounds__(256) void k_fm_scan_a(const uint32_t *__restrict__ cp, size_t rows, size_t rpc, uint32_t *__restrict__ chunk_sum) {
    const size_t g = blockIdx.x, r0 = g * rpc, r1 = r0 + rpc < rows ? r0 + rpc : rows;
    uint32_t s = 0;
#pragma unroll 8
    for (size_t r = r0; r < r1; ++r) s += cp[r * 256 + threadIdx.x];
    chunk_sum[g * 256 + threadIdx.x] = s;
}
__global__ __launch_bounds__(256) void k_fm_scan_b(uint32_t *__restrict__ chunk_sum, size_t nchunks) {
    uint32_t run = 0;
    for (size_t g = 0; g < nchunks; ++g) {
        const uint32_t v = chunk_sum[g * 256 + threadIdx.x];
        chunk_sum[g * 256 + threadIdx.x] = run;
        run += v;
    }
}
__global__ __launch_bounds__(256) void k_fm_scan_c(uint32_t *__restrict__ cp, size_t rows, size_t rpc, const uint32_t *__restrict__ chunk_sum) {
    const size_t g = blockIdx.x, r0 = g * rpc, r1 = r0 + rpc < rows ? r0 + rpc : rows;
    uint32_t run = chunk_sum[g * 256 + threadIdx.x];
    for (size_t r = r0; r < r1; ++r) {
        const uint32_t v = cp[r * 256 + threadIdx.x];
        cp[r * 256 + threadIdx.x] = run;
        run += v;
    }
}
// block b = blockIdx.x, thread = symbol.  off / org: count + 1 / count words in the workspace (org[b] < n_b: the caller's check)
__global__ __launch_bounds__(256) void k_fm_heads(const uint8_t *__restrict__ L, const uint32_t *__restrict__ off, const uint32_t *__restrict__ org,
                                                  const uint32_t *__restrict__ cp, uint32_t *__restrict__ blocks, uint32_t *__restrict__ base) {
    __shared__ uint32_t h[2][256];
    __shared__ uint32_t s_tmp[4 + 1];
    const uint32_t b = blockIdx.x, c = threadIdx.x, s = off[b], e = off[b + 1];
    h[0][c] = h[1][c] = 0;
    __syncthreads();
    const uint32_t row_s = s >> FM_SHIFT, row_e = e >> FM_SHIFT;
    for (uint32_t q = (row_s << FM_SHIFT) + c; q < s; q += 256u) atomicAdd(&h[0][L[q]], 1u);
    for (uint32_t q = (row_e << FM_SHIFT) + c; q < e; q += 256u) atomicAdd(&h[1][L[q]], 1u);
    __syncthreads();
    const uint32_t occ_s = cp[static_cast<size_t>(row_s) * 256 + c] + h[0][c], occ_e = cp[static_cast<size_t>(row_e) * 256 + c] + h[1][c];
    const uint32_t cb = block_excl_sum<4>(occ_e - occ_s, s_tmp, nullptr);
    base[static_cast<size_t>(b) * 256 + c] = cb - occ_s;  // (modulo 2^32, as the step adds it back)
    if (c == 0) {
        uint32_t *w = blocks + 4 * static_cast<size_t>(b);
        w[0] = s;
        w[1] = e - s;
        w[2] = org[b];
        w[3] = L[s + org[b]];
    }
}

// ---- count ----------------------------------------------------------------------------------------------------------------------------------

struct FmArgs {
    const uint8_t *L; const uint32_t *off, *blocks, *base, *cp; const uint8_t *pat; const uint32_t *pat_off, *pat_blk; uint32_t npat, total, count;
    uint32_t *out_lo, *out_hi;
};
// ONE STEP of the backward search in block b = L[s, s + nb), by the whole wave: [lo, hi) of a string w becomes that of c w, as the header derives
// it; first = 1 for the step from the empty string's (0, nb).  lo and hi are clamped to [0, nb].  Shared by fm_search and the branching search
// of near (section 4.18): the recurrence stands here and nowhere else.
__device__ __forceinline__ void fm_step(const uint8_t *__restrict__ L, uint32_t total, const uint32_t *__restrict__ cp, const uint32_t *__restrict__ base,
                                        uint32_t origin, uint32_t last, uint32_t s, uint32_t nb, uint32_t c, uint32_t first, uint32_t lane, uint32_t &lo,
                                        uint32_t &hi) {
    const uint32_t is_last = c == last ? 1u : 0u, bc = base[c];
    if (lo != hi || first) {
        uint32_t rl, rh;
        fm_rank2(L, total, cp, c, s + lo, s + hi, lane, rl, rh);
        lo = bc + (is_last & ~first) - (is_last & (origin < lo ? 1u : 0u)) + rl;
        hi = bc + is_last - (is_last & (origin < hi ? 1u : 0u)) + rh;
    } else {
        lo = hi = bc + is_last - (is_last & (origin < lo ? 1u : 0u)) + fm_rank1(L, total, cp, c, s + lo, lane);
    }
    lo = lo < nb ? lo : nb;
    hi = hi < nb ? hi : nb;
}
// The backward search of the pattern p[0, m) in block b = L[s, s + nb), by the whole wave: lo / hi as the header derives them, clamped to
// [0, nb] behind every step.  Shared by k_fm_count and k_fm_find_count.
__device__ __forceinline__ void fm_search(const uint8_t *__restrict__ L, uint32_t total, const uint32_t *__restrict__ cp, const uint32_t *__restrict__ blocks,
                                          const uint32_t *__restrict__ base_all, uint32_t b, uint32_t s, uint32_t nb, const uint8_t *__restrict__ p, uint32_t m,
                                          uint32_t lane, uint32_t &lo_out, uint32_t &hi_out) {
    const uint32_t origin = blocks[4 * static_cast<size_t>(b) + 2], last = blocks[4 * static_cast<size_t>(b) + 3];
    const uint32_t *__restrict__ base = base_all + static_cast<size_t>(b) * 256;
    uint32_t lo = 0, hi = nb;
    for (uint32_t j = m; j-- > 0;) fm_step(L, total, cp, base, origin, last, s, nb, p[j], j + 1u == m ? 1u : 0u, lane, lo, hi);
    lo_out = lo;
    hi_out = hi;
}
__global__ __launch_bounds__(64 * FM_WAVES) void k_fm_count(FmArgs a) {
    const uint8_t *__restrict__ L = a.L, *__restrict__ pat = a.pat;
    const uint32_t *__restrict__ off = a.off, *__restrict__ cp = a.cp, *__restrict__ pat_off = a.pat_off, *__restrict__ pat_blk = a.pat_blk;
    const uint32_t lane = threadIdx.x & 63u, total = a.total;
    const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * FM_WAVES;
    for (uint64_t q = static_cast<uint64_t>(blockIdx.x) * FM_WAVES + (threadIdx.x >> 6); q < a.npat; q += nwaves) {
        const uint32_t po = pat_off[q], m = pat_off[q + 1] - po;
        const uint32_t b = pat_blk ? pat_blk[q] : 0u, s = off[b], nb = off[b + 1] - s;  // (b < count: the caller's check)
        uint32_t lo, hi;
        fm_search(L, total, cp, a.blocks, a.base, b, s, nb, pat + po, m, lane, lo, hi);
        if (lane == 0) {
            a.out_lo[q] = lo;
            a.out_hi[q] = hi;
        }
    }
}
// out[q] = Occ_pack(sym[q], min(pos[q], total))
__global__ __launch_bounds__(64 * FM_WAVES) void k_fm_rank(const uint8_t *__restrict__ L, uint32_t total, const uint32_t *__restrict__ cp,
                                                          const uint32_t *__restrict__ pos, const uint8_t *__restrict__ sym, uint32_t nq,
                                                          uint32_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * FM_WAVES;
    for (uint64_t q = static_cast<uint64_t>(blockIdx.x) * FM_WAVES + (threadIdx.x >> 6); q < nq; q += nwaves) {
        const uint32_t x = pos[q] < total ? pos[q] : total;
        const uint32_t r = fm_rank1(L, total, cp, sym[q], x, lane);
        if (lane == 0) out[q] = r;
    }
}

// ---- the LF step of a slot, shared by locate and extract ---------------------------------------------------------------------------------------
// (v0, v1): this lane's 16 bytes of the row of g = off_b + x, loaded with fm_lane_bytes(g + 1, sl) so that they hold the byte at g.
// c = L[g], taken from the lane that holds it by a cross-lane read
__device__ __forceinline__ uint32_t fm_symbol_at(uint64_t v0, uint64_t v1, uint32_t g) {
    const uint32_t at = g & 15u;
    return static_cast<uint32_t>(__shfl(static_cast<uint32_t>((at < 8u ? v0 >> (8u * at) : v1 >> (8u * (at - 8u))) & 0xFFu), (g & (FM_BLOCK - 1u)) >> 4, 64));
}
// LF(x) for x != origin_b with c = L[g]: the count's later step applied to the slot; the checkpoint word, base_b[c] and one butterfly sum.
// Clamped to [0, n_b).
__device__ __forceinline__ uint32_t fm_lf(const uint32_t *__restrict__ cp, const uint32_t *__restrict__ base, uint32_t origin, uint32_t last, uint32_t nb,
                                          uint32_t x, uint32_t g, uint32_t sl, uint32_t c, uint64_t v0, uint64_t v1) {
    const uint32_t is_last = c == last ? 1u : 0u;
    const uint32_t occ = cp[static_cast<size_t>(g >> FM_SHIFT) * 256 + c] + wave_sum(fm_count16(v0, v1, 0x0101010101010101ull * c, fm_lane_bytes(g, sl)));
    const uint32_t y = base[c] + is_last - (is_last & (origin < x ? 1u : 0u)) + occ;
    return y < nb ? y : nb - 1u;
}

// ---- locate ----------------------------------------------------------------------------------------------------------

struct FmLocArgs {
    const uint8_t *L; const uint32_t *off, *blocks, *base, *cp, *marks, *bits, *samples, *lo, *hi, *pat_blk;
    uint32_t npat, max_hits, total, step_shift, nsamp; uint32_t *pos;
};
// A wave per item (q, j): the text position of slot lo[q] + j of the pattern's block.  From the slot, LF steps (the count's step applied to the
// slot's own symbol) until a marked slot is met after k of them: its sample * step + k.  Every load of a step but the checkpoint word and base_b[c]
// depends on the slot alone -- the row's 16 bytes per lane, which hold c = L[slot] in one lane, and the row's 32 mark words in the lower lanes
// -- so they are issued together and c is taken from its lane; the checkpoint word, which needs c, is the second and last round trip of a step.
// Containment: lo, hi are clamped to [0, n_b], every slot to [0, n_b), the sample's index to the samples; at most min(step, n_b) steps.
// THE WALK ITSELF is fm_locate_walk, shared by k_fm_locate and k_fm_find_locate: from slot x < nb of block b = L[s, s + nb) down to a marked
// slot, by the whole wave -> the text position of x, or DK_FM_NO_HIT where no mark is met within min(step, nb) steps or the sample lies outside
// the block.
struct FmWalk { const uint8_t *L; const uint32_t *blocks, *base, *cp, *marks, *bits, *samples; uint32_t total, step_shift, nsamp; };
__device__ __forceinline__ uint32_t fm_locate_walk(const FmWalk &w, uint32_t b, uint32_t s, uint32_t nb, uint32_t x, uint32_t lane) {
    const uint8_t *__restrict__ L = w.L;
    const uint32_t *__restrict__ cp = w.cp, *__restrict__ bits = w.bits;
    const uint32_t total = w.total, step = 1u << w.step_shift;
    const uint32_t origin = w.blocks[4 * static_cast<size_t>(b) + 2], last = w.blocks[4 * static_cast<size_t>(b) + 3];
    const uint32_t *__restrict__ base = w.base + static_cast<size_t>(b) * 256;
    const uint32_t bound = step < nb ? step : nb;
    uint32_t out = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < bound; ++k) {
        const uint32_t g = s + x, row = g >> FM_SHIFT, sl = (row << FM_SHIFT) + 16u * lane;
        const uint32_t mine = lane < 32u ? bits[static_cast<size_t>(row) * 32 + lane] : 0u;
        uint64_t v0, v1;
        fm_load16(L, total, sl, fm_lane_bytes(g + 1u, sl), v0, v1);  // (the bytes below g and the one at g, which is below total)
        const uint32_t word = (g & (FM_BLOCK - 1u)) >> 5, bit = g & 31u;
        if ((static_cast<uint32_t>(__shfl(mine, word, 64)) >> bit) & 1u) {
            const uint32_t below = lane < word ? __popc(mine) : (lane == word ? __popc(mine & ((1u << bit) - 1u)) : 0u);
            uint32_t r = w.marks[row] + wave_sum(below);
            r = r < w.nsamp ? r : w.nsamp - 1u;
            const uint64_t p = (static_cast<uint64_t>(w.samples[r]) << w.step_shift) + k;
            if (p < nb) out = static_cast<uint32_t>(p);
            break;
        }
        x = fm_lf(cp, base, origin, last, nb, x, g, sl, fm_symbol_at(v0, v1, g), v0, v1);
    }
    return out;
}
__global__ __launch_bounds__(64 * FM_WAVES) void k_fm_locate(FmLocArgs a) {
    const uint32_t *__restrict__ off = a.off, *__restrict__ pat_blk = a.pat_blk;
    const uint32_t lane = threadIdx.x & 63u;
    const FmWalk w{a.L, a.blocks, a.base, a.cp, a.marks, a.bits, a.samples, a.total, a.step_shift, a.nsamp};
    const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * FM_WAVES, nitems = static_cast<uint64_t>(a.npat) * a.max_hits;
    for (uint64_t item = static_cast<uint64_t>(blockIdx.x) * FM_WAVES + (threadIdx.x >> 6); item < nitems; item += nwaves) {
        const uint32_t q = static_cast<uint32_t>(item / a.max_hits), j = static_cast<uint32_t>(item - static_cast<uint64_t>(q) * a.max_hits);
        const uint32_t b = pat_blk ? pat_blk[q] : 0u, s = off[b], nb = off[b + 1] - s;  // (b < count: the caller's check)
        const uint32_t lo = a.lo[q] < nb ? a.lo[q] : nb, hi = a.hi[q] < nb ? a.hi[q] : nb;
        uint32_t out = 0xFFFFFFFFu;
        if (lo < hi && j < hi - lo) out = fm_locate_walk(w, b, s, nb, lo + j, lane);
        if (lane == 0) a.pos[item] = out;
    }
}

// ---- find: every pattern in every block, as a compact list of hit records in the order (pattern, block, slot) ----------
// Pair p = q * count + b.  k_fm_find_count leaves lo[p] and occ[p]; the scan gives offset[p] = the sum of occ below p in 64 bits and the grand
// total; k_fm_find_locate takes hit h, finds the pair with offset[p] <= h < offset[p + 1] and walks from slot lo[p] + h - offset[p].  No atomics.
constexpr uint32_t FM_FIND_ROW = 256;  // pairs per row of the scan: one per thread of a workgroup

struct FmFindArgs {
    const uint8_t *L; const uint32_t *off, *blocks, *base, *cp; const uint8_t *pat; const uint32_t *pat_off; uint32_t npat, total, count;
    uint32_t *lo, *occ, *out_occ;
};
// A wave per pair, grid stride over the pairs in their own order: the waves in flight together hold one pattern and neighbouring blocks
// (q-major; UNMEASURED against b-major).  occ = hi - lo, 0 where an index that is none gives hi < lo.
__global__ __launch_bounds__(64 * FM_WAVES) void k_fm_find_count(FmFindArgs a) {
    const uint8_t *__restrict__ L = a.L, *__restrict__ pat = a.pat;
    const uint32_t *__restrict__ off = a.off, *__restrict__ cp = a.cp, *__restrict__ pat_off = a.pat_off;
    const uint32_t lane = threadIdx.x & 63u, total = a.total, count = a.count;
    const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * FM_WAVES, npairs = static_cast<uint64_t>(a.npat) * count;
    for (uint64_t p = static_cast<uint64_t>(blockIdx.x) * FM_WAVES + (threadIdx.x >> 6); p < npairs; p += nwaves) {
        const uint32_t q = static_cast<uint32_t>(p / count), b = static_cast<uint32_t>(p - static_cast<uint64_t>(q) * count);
        const uint32_t po = pat_off[q], m = pat_off[q + 1] - po, s = off[b], nb = off[b + 1] - s;
        uint32_t lo, hi;
        fm_search(L, total, cp, a.blocks, a.base, b, s, nb, pat + po, m, lane, lo, hi);
        if (lane == 0) {
            const uint32_t occ = hi > lo ? hi - lo : 0u;
            a.lo[p] = lo;
            a.occ[p] = occ;
            if (a.out_occ) a.out_occ[p] = occ;
        }
    }
}
// exclusive sum of 64-bit values over the 256 threads of a workgroup; s_tmp: 4 words.  Two __syncthreads().
__device__ __forceinline__ uint64_t fm_block_excl_sum64(uint64_t v, uint64_t *s_tmp, uint64_t *all_out) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const uint32_t l = __shfl_up(static_cast<uint32_t>(inc), o, 64), h = __shfl_up(static_cast<uint32_t>(inc >> 32), o, 64);
        if (lane >= o) inc += (static_cast<uint64_t>(h) << 32) | l;
    }
    if (lane == 63u) s_tmp[wave] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint64_t t = s_tmp[k];
        if (k < wave) before += t;
        all += t;
    }
    *all_out = all;
    __syncthreads();
    return before + inc - v;
}
// the scan of occ over the pairs: chunk g = rows [g rpc, (g + 1) rpc) of FM_FIND_ROW pairs (the shape of k_fm_scan_*, in 64-bit sums)
__global__ __launch_bounds__(256) void k_fm_find_scan_a(const uint32_t *__restrict__ occ, uint32_t npairs, uint32_t rpc, uint64_t *__restrict__ chunk_sum) {
    __shared__ uint64_t s_tmp[4];
    const uint64_t p0 = static_cast<uint64_t>(blockIdx.x) * rpc * FM_FIND_ROW, p1 = p0 + static_cast<uint64_t>(rpc) * FM_FIND_ROW < npairs ? p0 + static_cast<uint64_t>(rpc) * FM_FIND_ROW : npairs;
    uint64_t sum = 0, all;
    for (uint64_t p = p0 + threadIdx.x; p < p1; p += FM_FIND_ROW) sum += occ[p];
    fm_block_excl_sum64(sum, s_tmp, &all);
    if (threadIdx.x == 0) chunk_sum[blockIdx.x] = all;
}
// one workgroup over the at most FM_MAX_CHUNKS sums; the grand total to the mailbox (a plain store on every launch)
__global__ __launch_bounds__(256) void k_fm_find_scan_b(uint64_t *__restrict__ chunk_sum, uint32_t nchunks, uint64_t *__restrict__ grand_total) {
    __shared__ uint64_t s_tmp[4];
    const uint64_t v = threadIdx.x < nchunks ? chunk_sum[threadIdx.x] : 0;
    uint64_t all;
    const uint64_t ex = fm_block_excl_sum64(v, s_tmp, &all);
    if (threadIdx.x < nchunks) chunk_sum[threadIdx.x] = ex;
    if (threadIdx.x == 0) *grand_total = all;
}
__global__ __launch_bounds__(256) void k_fm_find_scan_c(const uint32_t *__restrict__ occ, uint32_t npairs, uint32_t rpc, const uint64_t *__restrict__ chunk_sum,
                                                        uint64_t *__restrict__ offset) {
    __shared__ uint64_t s_tmp[4];
    const uint64_t p0 = static_cast<uint64_t>(blockIdx.x) * rpc * FM_FIND_ROW;
    uint64_t run = chunk_sum[blockIdx.x];
    for (uint32_t r = 0; r < rpc; ++r) {
        const uint64_t p = p0 + static_cast<uint64_t>(r) * FM_FIND_ROW + threadIdx.x;
        if (p0 + static_cast<uint64_t>(r) * FM_FIND_ROW >= npairs) break;  // (the same for every thread)
        uint64_t all;
        const uint64_t ex = fm_block_excl_sum64(p < npairs ? occ[p] : 0u, s_tmp, &all);
        if (p < npairs) offset[p] = run + ex;
        run += all;
    }
}

struct FmFindLocArgs {
    FmWalk w; const uint32_t *off, *lo; const uint64_t *offset; uint32_t npairs, count, nhits; uint4 *hits;
};
// A wave per hit h < nhits = min(total, max_hits).  The pair: the last one whose offset is <= h (behind it only pairs without hits share that
// offset), by a 64-ary search -- every lane probes one offset, the ballot's population count picks the stretch -- in at most four rounds for
// 2^24 pairs.  Then the walk of k_fm_locate from slot lo + (h - offset), and lane 0 stores the record with one 16-byte store.
// Containment: the pair stays inside [0, npairs) by construction of the search, lo is clamped to [0, n_b] and the slot to [0, n_b).
__global__ __launch_bounds__(64 * FM_WAVES) void k_fm_find_locate(FmFindLocArgs a) {
    const uint32_t *__restrict__ off = a.off;
    const uint64_t *__restrict__ offset = a.offset;
    const uint32_t lane = threadIdx.x & 63u, count = a.count;
    const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * FM_WAVES;
    for (uint64_t h = static_cast<uint64_t>(blockIdx.x) * FM_WAVES + (threadIdx.x >> 6); h < a.nhits; h += nwaves) {
        uint32_t plo = 0, phi = a.npairs;  // offset[plo] <= h, and the pair is in [plo, phi)
        while (phi - plo > 1u) {
            const uint32_t stride = (phi - plo + 63u) >> 6, idx = plo + lane * stride;
            uint32_t k = static_cast<uint32_t>(__popcll(__ballot(idx < phi && offset[idx] <= h)));
            k = k ? k - 1u : 0u;
            plo += k * stride;
            phi = phi - plo > stride ? plo + stride : phi;
        }
        const uint32_t pair = plo < a.npairs ? plo : a.npairs - 1u;
        const uint32_t q = pair / count, b = pair - q * count, s = off[b], nb = off[b + 1] - s;
        const uint32_t lo = a.lo[pair] < nb ? a.lo[pair] : nb;
        const uint64_t x64 = lo + (h - offset[pair]);
        const uint32_t x = x64 < nb ? static_cast<uint32_t>(x64) : nb - 1u;
        const uint32_t pos = fm_locate_walk(a.w, b, s, nb, x, lane);
        if (lane == 0) a.hits[h] = make_uint4(q, b, pos, x);
    }
}

// ---- extract ---------------------------------------------------------------------------------------------------------

struct FmExtArgs {
    const uint8_t *L; const uint32_t *off, *abase, *blocks, *base, *cp, *anchors, *pos, *len, *rng_blk;
    uint32_t nrange, max_len, per, total, step_shift; uint8_t *out;
    const uint32_t *out_off;  // null: row q starts at out + q max_len.  Otherwise at out + out_off[q] (the seams' ragged strip, section 4.17)
};
// A wave per item (q, i), i < per = ceil(max_len / step) + 1: chunk k = pos[q] / step + i of the range's block, [k step, e) with e = min((k + 1)
// step, n_b), where it meets the range [pos, pos + got).  From the slot of suffix e -- anchor k + 1, or the origin when e = n_b -- L[x] = T[e - 1],
// and every LF step (locate's, without the marks) gives the byte in front: T[e - 2], ... down to max(k step, pos).  The one step FROM the origin
// is not the general formula: LF(origin) = C[last] = base_b[last] + Occ_pack(last, off_b), one rank at the block's head.  The byte of step j stays
// in lane j mod 64; after 64 steps and at the chunk's end every lane stores its own where it lies below pos + got: byte stores from consecutive
// lanes to consecutive addresses, so a row of any alignment is served.  The rows were zeroed by a memset in front of the kernel.
// Containment: the anchor index is clamped to the block's anchors, every slot to [0, n_b), `last` to a byte, at most min(step, n_b) steps per item; a store goes
// to out[q max_len + p - pos] (out[out_off[q] + p - pos] for the seams' strip, whose planner gives every range len[q] bytes of its own) with
// pos <= p < pos + got <= pos + min(len[q], max_len), and what is stored is a byte of block b's L.
__global__ __launch_bounds__(64 * FM_WAVES) void k_fm_extract(FmExtArgs a) {
    const uint8_t *__restrict__ L = a.L;
    const uint32_t *__restrict__ off = a.off, *__restrict__ cp = a.cp, *__restrict__ rng_blk = a.rng_blk;
    const uint32_t lane = threadIdx.x & 63u, total = a.total, shift = a.step_shift, step = 1u << shift;
    const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * FM_WAVES, nitems = static_cast<uint64_t>(a.nrange) * a.per;
    for (uint64_t item = static_cast<uint64_t>(blockIdx.x) * FM_WAVES + (threadIdx.x >> 6); item < nitems; item += nwaves) {
        const uint32_t q = static_cast<uint32_t>(item / a.per), i = static_cast<uint32_t>(item - static_cast<uint64_t>(q) * a.per);
        const uint32_t b = rng_blk ? rng_blk[q] : 0u, s = off[b], nb = off[b + 1] - s;  // (b < count: the caller's check)
        const uint32_t pos = a.pos[q];
        if (pos >= nb) continue;
        uint32_t got = a.len ? a.len[q] : a.max_len;
        got = got < a.max_len ? got : a.max_len;
        got = got < nb - pos ? got : nb - pos;
        const uint64_t cs64 = (static_cast<uint64_t>(pos >> shift) + i) << shift;
        if (got == 0 || cs64 >= static_cast<uint64_t>(pos) + got) continue;  // an empty range; a chunk behind the range
        const uint32_t cs = static_cast<uint32_t>(cs64), k = cs >> shift;
        const uint32_t e = nb - cs > step ? cs + step : nb, lo = cs > pos ? cs : pos, hi = pos + got, steps = e - lo;  // 1 <= steps <= min(step, n_b)
        // (last indexes base_b and a checkpoint row in the origin's step: cut to a byte, whatever the index holds)
        const uint32_t origin = a.blocks[4 * static_cast<size_t>(b) + 2], last = a.blocks[4 * static_cast<size_t>(b) + 3] & 0xFFu;
        const uint32_t *__restrict__ base = a.base + static_cast<size_t>(b) * 256;
        const uint32_t nanch = (nb + step - 1u) >> shift;
        uint32_t x;
        bool at_origin = e == nb;
        if (at_origin) {
            x = origin;
        } else {
            const uint32_t idx = k + 1u < nanch ? k + 1u : nanch - 1u;
            x = a.anchors[(a.abase ? a.abase[b] : 0u) + idx];
        }
        x = x < nb ? x : nb - 1u;
        uint8_t *row_out = a.out + (a.out_off ? static_cast<size_t>(a.out_off[q]) : static_cast<size_t>(q) * a.max_len);
        uint32_t mine = 0;
        for (uint32_t j = 0; j < steps; ++j) {
            const uint32_t g = s + x, sl = ((g >> FM_SHIFT) << FM_SHIFT) + 16u * lane;
            uint64_t v0, v1;
            fm_load16(L, total, sl, fm_lane_bytes(g + 1u, sl), v0, v1);  // (the bytes below g and the one at g, which is below total)
            const uint32_t c = fm_symbol_at(v0, v1, g);
            if ((j & 63u) == lane) mine = c;
            if ((j & 63u) == 63u || j + 1u == steps) {
                // this lane's byte is that of step j0 + lane, text position e - 1 - (j0 + lane)
                const uint32_t j0 = j & ~63u;
                if (j0 + lane <= j) {
                    const uint32_t p = e - 1u - (j0 + lane);
                    if (p < hi) row_out[p - pos] = static_cast<uint8_t>(mine);
                }
                if (j + 1u == steps) break;
            }
            if (at_origin) {
                const uint32_t y = base[last] + fm_rank1(L, total, cp, last, s, lane);
                x = y < nb ? y : nb - 1u;
                at_origin = false;
            } else {
                x = fm_lf(cp, base, origin, last, nb, x, g, sl, c, v0, v1);
            }
        }
    }
}

// ---- seams: the matches that straddle block borders ---------------------------------------------------------------------
// The strip: prev, then of every block its whole text (n_b <= 2 W) or its first W and its last W bytes, W = longest pattern - 1.  geo[3 b ..]:
// sb = the strip offset of block b's first byte, head = min(n_b, W), rs = where the contiguous run that reaches sb starts.  A seam hit of
// pattern q (m bytes) in block b with `back` bytes in front of the block stands at strip[sb - back, sb - back + m): back <= min(m - 1, sb - rs)
// keeps its front inside the run, m - back <= head keeps its last byte inside the block.  The candidates of a pair are therefore
// back = hi, hi - 1, ..., lo with hi = min(m - 1, sb - rs) and lo = max(1, m - head): file order of the starts.
struct FmSeamArgs {
    const uint8_t *strip; const uint32_t *geo; const uint8_t *pat; const uint32_t *pat_off; uint32_t npat, count, strip_len;
    uint32_t *occ, *out_occ; const uint64_t *offset; uint32_t nhits; uint4 *hits;
};
struct FmSeamPair { uint32_t q, b, m, sb, hi, ncand; const uint8_t *p; };
// the pair's candidates, every strip offset clamped to the strip: ncand = 0 where nothing can match
__device__ __forceinline__ FmSeamPair fm_seam_pair(const FmSeamArgs &a, uint64_t pair) {
    FmSeamPair r;
    r.q = static_cast<uint32_t>(pair / a.count);
    r.b = static_cast<uint32_t>(pair - static_cast<uint64_t>(r.q) * a.count);
    const uint32_t po = a.pat_off[r.q];
    r.m = a.pat_off[r.q + 1] - po;
    r.p = a.pat + po;
    const uint32_t sb = a.geo[3 * static_cast<size_t>(r.b)], head = a.geo[3 * static_cast<size_t>(r.b) + 1], rs = a.geo[3 * static_cast<size_t>(r.b) + 2];
    r.sb = sb < a.strip_len ? sb : a.strip_len;
    const uint32_t reach = rs < r.sb ? r.sb - rs : 0u, room = a.strip_len - r.sb, fit = head < room ? head : room;
    r.hi = r.m < 2u ? 0u : (r.m - 1u < reach ? r.m - 1u : reach);
    const uint32_t lo = r.m > fit ? r.m - fit : 1u;
    r.ncand = r.hi >= lo ? r.hi - lo + 1u : 0u;
    return r;
}
// does the pattern stand at s[0, m)?  Eight bytes at a time (neither side is aligned: every lane's candidate starts one byte on), then the rest.
__device__ __forceinline__ bool fm_seam_equal(const uint8_t *__restrict__ s, const uint8_t *__restrict__ p, uint32_t m) {
    uint32_t j = 0;
    for (; j + 8u <= m; j += 8u)
        if (*(gptr8)(s + j) != *(gptr8)(p + j)) return false;
    for (; j < m; ++j)
        if (s[j] != p[j]) return false;
    return true;
}
// round r of a pair: lane l takes candidate k = 64 r + l, back = hi - k; the ballot of the hits.  (hi - k >= lo >= 1 and sb - back + m <= strip_len
// by fm_seam_pair.)
__device__ __forceinline__ uint64_t fm_seam_round(const uint8_t *__restrict__ strip, const FmSeamPair &r, uint32_t round, uint32_t lane, uint32_t &back) {
    const uint32_t k = round * 64u + lane;
    back = k < r.ncand ? r.hi - k : 0u;
    return __ballot(k < r.ncand && fm_seam_equal(strip + (r.sb - back), r.p, r.m));
}
__global__ __launch_bounds__(64 * FM_WAVES) void k_fm_seam_count(FmSeamArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * FM_WAVES, npairs = static_cast<uint64_t>(a.npat) * a.count;
    for (uint64_t pair = static_cast<uint64_t>(blockIdx.x) * FM_WAVES + (threadIdx.x >> 6); pair < npairs; pair += nwaves) {
        const FmSeamPair r = fm_seam_pair(a, pair);
        uint32_t occ = 0, back;
        for (uint32_t round = 0; round * 64u < r.ncand; ++round) occ += static_cast<uint32_t>(__popcll(fm_seam_round(a.strip, r, round, lane, back)));
        if (lane == 0) {
            a.occ[pair] = occ;
            if (a.out_occ) a.out_occ[pair] = occ;
        }
    }
}
// A wave per pair again, not per hit: a pair's hits come out of one more pass over its candidates, where a wave per hit would repeat that pass
// occ times (a^m on a^n has occ = m - 1).  Hit lanes store {pattern, block, back, 0} at offset[pair] + their rank, below nhits only.
__global__ __launch_bounds__(64 * FM_WAVES) void k_fm_seam_emit(FmSeamArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * FM_WAVES, npairs = static_cast<uint64_t>(a.npat) * a.count;
    for (uint64_t pair = static_cast<uint64_t>(blockIdx.x) * FM_WAVES + (threadIdx.x >> 6); pair < npairs; pair += nwaves) {
        uint64_t at = a.offset[pair];
        if (a.occ[pair] == 0 || at >= a.nhits) continue;
        const FmSeamPair r = fm_seam_pair(a, pair);
        for (uint32_t round = 0; round * 64u < r.ncand && at < a.nhits; ++round) {
            uint32_t back;
            const uint64_t hit = fm_seam_round(a.strip, r, round, lane, back);
            const uint64_t idx = at + static_cast<uint32_t>(__popcll(hit & ((1ull << lane) - 1ull)));
            if (((hit >> lane) & 1ull) && idx < a.nhits) a.hits[idx] = make_uint4(r.q, r.b, back, 0u);
            at += static_cast<uint32_t>(__popcll(hit));
        }
    }
}

// ---- near: backward search that branches -- byte classes and a budget of k mismatches ----------------------------------
// Position j of pattern q is a set of byte values, 32 bytes at cls + 32 (pat_off[q] + j): bit c & 7 of byte c >> 3.  A NODE is (j, w): w a string
// of m - j bytes that occurs inside block b, whose cost against cls[j, m) -- the positions whose byte is outside its class -- is <= k.  Its
// range [lo, hi) is not empty.  The root is (m, ""), the children of (j, w) are the nodes (j - 1, c w) in ascending order of c, the leaves are
// the nodes with j = 0, and the walk is the tree's preorder, at most node_limit nodes of it (the root is the first).  A leaf's slots are hits.
// A wave walks one pair's tree depth first.  The node it stands at lives in registers: lo, hi, cost and the symbols still to try as four
// 64-bit masks (symbol 64 j + bit).  Going down pushes them to the wave's stack in LDS, level d = the m - j of the node, at most m - 1 <= 127
// levels (a leaf is never pushed); every lane stores and loads the same words, so no lane reads what another one wrote.
constexpr uint32_t FM_NEAR_MAX_M = DK_FM_NEAR_MAX_PATTERN;
// Which symbols to try at a node.  Without budget left and with a class of at most FM_NEAR_FEW symbols: the class itself -- a rank each, an
// empty child is dropped behind it.  Otherwise the symbols that occur in L[s + lo, s + hi) (a superset of those with a child: the origin's
// symbol is among them), cut to the class where no budget is left.  Up to FM_NEAR_ROW bytes the lanes look at the bytes themselves, 16 each;
// above, at the checkpoint rows around the range.  Both thresholds are REASONED, NOT MEASURED: a presence pass costs about what one rank
// costs, and a row is what one load per lane covers.
constexpr uint32_t FM_NEAR_FEW = 2, FM_NEAR_ROW = FM_BLOCK;
struct FmNearStack {
    uint32_t lo[FM_NEAR_MAX_M], hi[FM_NEAR_MAX_M], cost[FM_NEAR_MAX_M];
    uint64_t set[FM_NEAR_MAX_M][4];
    uint32_t seen[64];  // the presence table of the narrow form, a byte per symbol
};
static_assert(sizeof(FmNearStack) * FM_WAVES <= 24 * 1024, "four waves' stacks stay at about 23 KB of LDS");

struct FmNearArgs {
    const uint8_t *L; const uint32_t *off, *blocks, *base, *cp; const uint8_t *cls; const uint32_t *pat_off; uint32_t npat, total, count, rows, k, limit;
    uint32_t *occ, *cut, *out_occ;                          // count
    const uint64_t *offset; uint32_t nhits; uint4 *hits;    // emit
};
__device__ __forceinline__ void fm_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// the class at cls32[0, 32) as masks: every lane tests its symbol of each quarter
__device__ __forceinline__ void fm_near_class(const uint8_t *__restrict__ cls32, uint32_t lane, uint64_t m[4]) {
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t c = 64u * j + lane;
        m[j] = __ballot((cls32[c >> 3] >> (c & 7u)) & 1u);
    }
}
// the symbols of L[s + lo, s + hi), lo < hi <= nb, or a superset of them
__device__ __forceinline__ void fm_near_present(const uint8_t *__restrict__ L, uint32_t total, const uint32_t *__restrict__ cp, uint32_t rows, uint32_t s,
                                                uint32_t lo, uint32_t hi, uint32_t lane, uint32_t *seen, uint64_t m[4]) {
    if (hi - lo > FM_NEAR_ROW) {
        // row k counts L[0, k FM_BLOCK): the rows at and below s + lo and at and above s + hi (the last row covers `total`)
        const uint32_t row_lo = (s + lo) >> FM_SHIFT, up = (s + hi + FM_BLOCK - 1u) >> FM_SHIFT, row_hi = up < rows ? up : rows - 1u;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t c = 64u * j + lane;
            m[j] = __ballot(cp[static_cast<size_t>(row_hi) * 256 + c] != cp[static_cast<size_t>(row_lo) * 256 + c]);
        }
        return;
    }
    const uint32_t len = hi - lo, mine = len > 16u * lane ? (len - 16u * lane < 16u ? len - 16u * lane : 16u) : 0u;
    uint64_t a, b;
    fm_load16(L, total, s + lo + 16u * lane, mine, a, b);  // (s + hi <= total: the geometry is the caller's)
    seen[lane] = 0;
    fm_wave_sync();
    uint8_t *flag = reinterpret_cast<uint8_t *>(seen);
    for (uint32_t i = 0; i < mine; ++i) flag[(i < 8u ? a >> (8u * i) : b >> (8u * (i - 8u))) & 0xFFu] = 1;  // (racing stores all write 1)
    fm_wave_sync();
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) m[j] = __ballot(flag[64u * j + lane] != 0);
    fm_wave_sync();  // (the next call clears the table)
}
// The walk of pair (q, b).  Returns the pair's hits; cut = 1 where a node beyond the limit exists.  EMIT: the records of the hits are stored at
// hits[at + their number in the walk], below nhits only, the slot staged in `position`; the walk ends once nothing below nhits is left.
// hits never passes nb (it cannot, where the index is one: a position has one text behind it) so that any index gives a count within the block.
template <bool EMIT>
__device__ __forceinline__ uint32_t fm_near_walk(const FmNearArgs &a, FmNearStack &st, uint32_t q, uint32_t b, uint32_t lane, uint64_t at, uint32_t &cut) {
    const uint8_t *__restrict__ L = a.L;
    const uint32_t *__restrict__ cp = a.cp;
    const uint32_t po = a.pat_off[q], m_all = a.pat_off[q + 1] - po, m = m_all < FM_NEAR_MAX_M ? m_all : FM_NEAR_MAX_M;
    const uint32_t s = a.off[b], nb = a.off[b + 1] - s, total = a.total, k = a.k;
    const uint32_t origin = a.blocks[4 * static_cast<size_t>(b) + 2], last = a.blocks[4 * static_cast<size_t>(b) + 3];
    const uint32_t *__restrict__ base = a.base + static_cast<size_t>(b) * 256;
    const uint8_t *__restrict__ cls = a.cls + 32 * static_cast<size_t>(po);
    uint32_t hits = 0, nodes = 1, d = 0, lo = 0, hi = nb, cost = 0;
    uint64_t set[4];
    cut = 0;
    // the symbols to try at the node in (lo, hi, cost) whose children stand at pattern position pos
    auto candidates = [&](uint32_t pos) {
        uint64_t in[4];
        fm_near_class(cls + 32 * static_cast<size_t>(pos), lane, in);
        const uint32_t few = static_cast<uint32_t>(__popcll(in[0]) + __popcll(in[1]) + __popcll(in[2]) + __popcll(in[3])) <= FM_NEAR_FEW ? 1u : 0u;
        if (cost == k && few) {
            set[0] = in[0], set[1] = in[1], set[2] = in[2], set[3] = in[3];
            return;
        }
        fm_near_present(L, total, cp, a.rows, s, lo, hi, lane, st.seen, set);
        if (cost == k) set[0] &= in[0], set[1] &= in[1], set[2] &= in[2], set[3] &= in[3];
    };
    // a leaf's slots [x, y), its cost: the records of those that still count
    auto leaf = [&](uint32_t x, uint32_t y, uint32_t leaf_cost) {
        const uint32_t take = y - x < nb - hits ? y - x : nb - hits;
        if (EMIT) {
            for (uint32_t i = lane; i < take; i += 64u) {
                const uint64_t idx = at + hits + i;
                if (idx < a.nhits) a.hits[idx] = make_uint4(q, b, x + i, leaf_cost);
            }
        }
        hits += take;
    };
    if (m == 0) {  // the root is the only node, and a leaf
        leaf(lo, hi, 0u);
        return hits;
    }
    candidates(m - 1u);
    for (;;) {
        uint32_t c;
        if (set[0]) c = static_cast<uint32_t>(__builtin_ctzll(set[0])), set[0] &= set[0] - 1ull;
        else if (set[1]) c = 64u + static_cast<uint32_t>(__builtin_ctzll(set[1])), set[1] &= set[1] - 1ull;
        else if (set[2]) c = 128u + static_cast<uint32_t>(__builtin_ctzll(set[2])), set[2] &= set[2] - 1ull;
        else if (set[3]) c = 192u + static_cast<uint32_t>(__builtin_ctzll(set[3])), set[3] &= set[3] - 1ull;
        else {  // every child of this node has been walked: back to its parent
            if (d == 0) break;
            --d;
            lo = st.lo[d], hi = st.hi[d], cost = st.cost[d];
            set[0] = st.set[d][0], set[1] = st.set[d][1], set[2] = st.set[d][2], set[3] = st.set[d][3];
            continue;
        }
        const uint32_t pos = m - 1u - d;  // the pattern position of the children
        uint32_t x = lo, y = hi;
        fm_step(L, total, cp, base, origin, last, s, nb, c, d == 0 ? 1u : 0u, lane, x, y);
        if (x >= y) continue;  // no such string in the block
        const uint32_t child_cost = cost + (((cls[32 * static_cast<size_t>(pos) + (c >> 3)] >> (c & 7u)) & 1u) ^ 1u);
        if (child_cost > k) continue;
        if (nodes >= a.limit) {  // a node beyond the limit: the walk stops in front of it
            cut = 1;
            break;
        }
        ++nodes;
        if (pos == 0) {
            leaf(x, y, child_cost);
            if (EMIT && at + hits >= a.nhits) break;
            continue;
        }
        st.lo[d] = lo, st.hi[d] = hi, st.cost[d] = cost;
        st.set[d][0] = set[0], st.set[d][1] = set[1], st.set[d][2] = set[2], st.set[d][3] = set[3];
        ++d;
        lo = x, hi = y, cost = child_cost;
        candidates(pos - 1u);
    }
    return hits;
}
// A wave per pair p = q count + b, grid stride in find's order.  Lane 0 stores the pair's hits and whether it was cut.
__global__ __launch_bounds__(64 * FM_WAVES) void k_fm_near_count(FmNearArgs a) {
    __shared__ FmNearStack st[FM_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, count = a.count;
    const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * FM_WAVES, npairs = static_cast<uint64_t>(a.npat) * count;
    for (uint64_t p = static_cast<uint64_t>(blockIdx.x) * FM_WAVES + wave; p < npairs; p += nwaves) {
        const uint32_t q = static_cast<uint32_t>(p / count), b = static_cast<uint32_t>(p - static_cast<uint64_t>(q) * count);
        uint32_t cut;
        const uint32_t occ = fm_near_walk<false>(a, st[wave], q, b, lane, 0, cut);
        if (lane == 0) {
            a.occ[p] = occ;
            a.cut[p] = cut;
            if (a.out_occ) a.out_occ[p] = occ;
        }
    }
}
// A wave per pair with hits below nhits: the same walk with the same limit visits the same nodes, and every leaf's records go to the pair's
// offset plus the hits so far.  The pair's work is repeated once, not once per hit (the seam emit's decision, section 4.17).
__global__ __launch_bounds__(64 * FM_WAVES) void k_fm_near_emit(FmNearArgs a) {
    __shared__ FmNearStack st[FM_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, count = a.count;
    const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * FM_WAVES, npairs = static_cast<uint64_t>(a.npat) * count;
    for (uint64_t p = static_cast<uint64_t>(blockIdx.x) * FM_WAVES + wave; p < npairs; p += nwaves) {
        const uint64_t at = a.offset[p];
        if (a.occ[p] == 0 || at >= a.nhits) continue;
        const uint32_t q = static_cast<uint32_t>(p / count), b = static_cast<uint32_t>(p - static_cast<uint64_t>(q) * count);
        uint32_t cut;
        fm_near_walk<true>(a, st[wave], q, b, lane, at, cut);
    }
}
// A wave per record below nhits: the walk of k_fm_locate from the staged slot; lane 0 rewrites `position`.
struct FmNearLocArgs { FmWalk w; const uint32_t *off; uint32_t count, nhits; uint4 *hits; };
__global__ __launch_bounds__(64 * FM_WAVES) void k_fm_near_locate(FmNearLocArgs a) {
    const uint32_t *__restrict__ off = a.off;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * FM_WAVES;
    for (uint64_t h = static_cast<uint64_t>(blockIdx.x) * FM_WAVES + (threadIdx.x >> 6); h < a.nhits; h += nwaves) {
        const uint4 r = a.hits[h];
        const uint32_t b = r.y < a.count ? r.y : a.count - 1u, s = off[b], nb = off[b + 1] - s, x = r.z < nb ? r.z : nb - 1u;
        const uint32_t pos = fm_locate_walk(a.w, b, s, nb, x, lane);
        if (lane == 0) reinterpret_cast<uint32_t *>(a.hits + h)[2] = pos;
    }
}

// ---- what the host stages share: the caller's structures carved, the pairs' geometry, the scan over the pairs ---------------------------------
FmIndex fm_carve(const FmView &fm) { return fm_carve(const_cast<void *>(fm.index), fm.L.total, fm.L.count); }
// the walk's record: the index and the locate structure fm.loc, sampled at fm.step
FmWalk fm_walk(const FmView &fm, const FmIndex &ix) {
    const FmLocate lc = fm_locate_carve(const_cast<void *>(fm.loc), fm.L.total, fm.L.count, fm.step);
    return FmWalk{fm.L.bytes, ix.blocks, ix.base, ix.cp, lc.marks, lc.bits, lc.samples, static_cast<uint32_t>(fm.L.total),
                  static_cast<uint32_t>(ceil_log2_u64(fm.step)), static_cast<uint32_t>(lc.nsamp)};
}
// the (pattern, block) pairs of find, near and seams, and their scan's shape: rows of FM_FIND_ROW pairs in nchunks chunks of rpc rows
struct FmPairs { size_t npairs, rows, rpc, nchunks; };
FmPairs fm_pairs(size_t npat, size_t count) {
    const size_t npairs = npat * count, rows = div_up(npairs, FM_FIND_ROW), rpc = div_up(rows, FM_MAX_CHUNKS), nchunks = div_up(rows, rpc);
    return FmPairs{npairs, rows, rpc, nchunks};
}
// k_fm_find_scan_a / _b / _c over d_cnt: *d_total (a field of the device mailbox) = the sum of all, d_offset[p] = the sum below pair p;
// d_offset null: _a / _b alone, the total.  chunk_sum: FM_MAX_CHUNKS sums.  Enqueues inside the caller's bracket and opens none.
void fm_scan_pairs(dk_ctx *ctx, const FmPairs &g, const uint32_t *d_cnt, uint64_t *chunk_sum, uint64_t *d_total, uint64_t *d_offset) {
    const uint32_t P = static_cast<uint32_t>(g.npairs), R = static_cast<uint32_t>(g.rpc), C = static_cast<uint32_t>(g.nchunks);
    k_fm_find_scan_a<<<dim3(C), dim3(256), 0, ctx->stream>>>(d_cnt, P, R, chunk_sum);
    k_fm_find_scan_b<<<dim3(1), dim3(256), 0, ctx->stream>>>(chunk_sum, C, d_total);
    if (d_offset) k_fm_find_scan_c<<<dim3(C), dim3(256), 0, ctx->stream>>>(d_cnt, P, R, chunk_sum, d_offset);
}

}  // namespace

size_t fm_build_workspace(size_t total, size_t count) {
    const size_t rows = div_up(total, FM_BLOCK) + 1, rpc = div_up(rows, FM_MAX_CHUNKS), nchunks = div_up(rows, rpc);
    return ws_round(nchunks * 256 * 4) + ws_round(4 * (count + 1)) + ws_round(4 * count);
}

int fm_build_device(dk_ctx *ctx, const uint8_t *d_bwt, const std::vector<uint32_t> &off, const uint32_t *origin, void *d_index) {
    hipStream_t st = ctx->stream;
    const size_t count = off.size() - 1, total = off.back();
    const FmIndex ix = fm_carve(d_index, total, count);
    const size_t rows = ix.rows, rpc = div_up(rows, FM_MAX_CHUNKS), nchunks = div_up(rows, rpc);
    const size_t mark = ctx->ws_mark();
    uint32_t *chunk_sum = ctx->ws_alloc<uint32_t>(nchunks * 256), *d_off = ctx->ws_alloc<uint32_t>(count + 1), *d_org = ctx->ws_alloc<uint32_t>(count);
    if (!chunk_sum || !d_off || !d_org) return DK_E_NOMEM;
    const uint32_t header[4] = {FM_MAGIC, static_cast<uint32_t>(total), static_cast<uint32_t>(count), static_cast<uint32_t>(rows)};
    DK_HIP(ctx, hipMemsetAsync(d_index, 0, FM_HEADER * sizeof(uint32_t), st));
    DK_HIP(ctx, hipMemcpyAsync(d_index, header, sizeof(header), hipMemcpyHostToDevice, st));
    DK_HIP(ctx, hipMemcpyAsync(d_off, off.data(), (count + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    int rc = ctx->hip_ok(hipMemcpyAsync(d_org, origin, count * sizeof(uint32_t), hipMemcpyHostToDevice, st), "origins");
    if (rc == DK_OK) {
        const uint32_t T = static_cast<uint32_t>(total), R = static_cast<uint32_t>(rows);
        {
            LaunchScope ls(ctx, K_IBWT_HIST, 1.0 * total + 3.0 * 1024 * rows);  // L once; the rows written, then read twice and written once by the scans
            k_fm_hist<<<dim3(static_cast<unsigned>(div_up(rows, FM_WAVES))), dim3(64 * FM_WAVES), 0, st>>>(d_bwt, T, ix.cp, R);
            k_fm_scan_a<<<dim3(static_cast<unsigned>(nchunks)), dim3(256), 0, st>>>(ix.cp, rows, rpc, chunk_sum);
            k_fm_scan_b<<<dim3(1), dim3(256), 0, st>>>(chunk_sum, nchunks);
            k_fm_scan_c<<<dim3(static_cast<unsigned>(nchunks)), dim3(256), 0, st>>>(ix.cp, rows, rpc, chunk_sum);
        }
        {
            LaunchScope ls(ctx, K_IBWT_HIST, 3088.0 * count);  // two checkpoint rows, at most a row of L twice, base_b and four words
            k_fm_heads<<<dim3(static_cast<unsigned>(count)), dim3(256), 0, st>>>(d_bwt, d_off, d_org, ix.cp, ix.blocks, ix.base);
        }
        rc = ctx->hip_ok(hipGetLastError(), "fm build");
    }
    const hipError_t e = hipStreamSynchronize(st);  // (also on failure: the copies above read `off`, `origin` and `header`)
    DK_TRY(rc);
    DK_HIP(ctx, e);
    ctx->ws_release(mark);
    return DK_OK;
}

int fm_count_device(dk_ctx *ctx, const FmView &fm, const ItemView &pat, uint32_t *d_lo, uint32_t *d_hi) {
    const FmIndex ix = fm_carve(fm);
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(div_up(pat.count, FM_WAVES), 1u << 20));
    const FmArgs a{fm.L.bytes, fm.L.d_off, ix.blocks, ix.base, ix.cp, pat.bytes, pat.d_off, pat.d_blk, static_cast<uint32_t>(pat.count),
                   static_cast<uint32_t>(fm.L.total), static_cast<uint32_t>(fm.L.count), d_lo, d_hi};
    {
        // per step at most two gathered checkpoint words and two rows of L; the pattern bytes, the offsets and the two results
        LaunchScope ls(ctx, K_CHAIN, 16.0 * pat.count + pat.nbytes * (1.0 + 2.0 * (FM_BLOCK + 64)));
        k_fm_count<<<dim3(grid), dim3(64 * FM_WAVES), 0, ctx->stream>>>(a);
    }
    DK_HIP(ctx, hipGetLastError());
    return DK_OK;
}

int fm_rank_device(dk_ctx *ctx, const FmView &fm, const uint32_t *d_pos, const uint8_t *d_sym, size_t nq, uint32_t *d_out) {
    const FmIndex ix = fm_carve(const_cast<void *>(fm.index), fm.L.total, 0);  // (the checkpoints lie in front of everything that depends on the count)
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(div_up(nq, FM_WAVES), 1u << 20));
    {
        LaunchScope ls(ctx, K_CHAIN, nq * (9.0 + FM_BLOCK + 64));
        k_fm_rank<<<dim3(grid), dim3(64 * FM_WAVES), 0, ctx->stream>>>(fm.L.bytes, static_cast<uint32_t>(fm.L.total), ix.cp, d_pos, d_sym,
                                                                       static_cast<uint32_t>(nq), d_out);
    }
    DK_HIP(ctx, hipGetLastError());
    return DK_OK;
}

int fm_locate_device(dk_ctx *ctx, const FmView &fm, const uint32_t *d_lo, const uint32_t *d_hi, const uint32_t *d_pat_blk, size_t npat, size_t max_hits,
                     uint32_t *d_pos) {
    const FmWalk w = fm_walk(fm, fm_carve(fm));
    const size_t nitems = npat * max_hits;
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(div_up(nitems, FM_WAVES), 1u << 20));
    const FmLocArgs a{w.L, fm.L.d_off, w.blocks, w.base, w.cp, w.marks, w.bits, w.samples, d_lo, d_hi, d_pat_blk, static_cast<uint32_t>(npat),
                      static_cast<uint32_t>(max_hits), w.total, w.step_shift, w.nsamp, d_pos};
    {
        // per item about step / 2 steps of a row of L, a row of mark words and a checkpoint word; the range, the sample and the result
        LaunchScope ls(ctx, K_CHAIN, nitems * (20.0 + 0.5 * fm.step * (FM_BLOCK + 128 + 64)));
        k_fm_locate<<<dim3(grid), dim3(64 * FM_WAVES), 0, ctx->stream>>>(a);
    }
    DK_HIP(ctx, hipGetLastError());
    return DK_OK;
}

size_t fm_find_workspace(size_t npairs) { return 2 * ws_round(4 * npairs) + ws_round(8 * npairs) + ws_round(8 * FM_MAX_CHUNKS); }

int fm_find_device(dk_ctx *ctx, const FmView &fm, const ItemView &pat, const HitSink &out) {
    hipStream_t st = ctx->stream;
    const FmIndex ix = fm_carve(fm);
    const FmPairs g = fm_pairs(pat.count, fm.L.count);
    const size_t npairs = g.npairs, count = fm.L.count, mark = ctx->ws_mark();
    uint32_t *d_lo = ctx->ws_alloc<uint32_t>(npairs), *d_cnt = ctx->ws_alloc<uint32_t>(npairs);
    uint64_t *d_offset = ctx->ws_alloc<uint64_t>(npairs), *chunk_sum = ctx->ws_alloc<uint64_t>(FM_MAX_CHUNKS);
    if (!d_lo || !d_cnt || !d_offset || !chunk_sum) return DK_E_NOMEM;
    {
        // per pair the count's traffic for its pattern (pat.nbytes / pat.count on average), the three words written
        LaunchScope ls(ctx, K_CHAIN, 20.0 * npairs + static_cast<double>(count) * pat.nbytes * (1.0 + 2.0 * (FM_BLOCK + 64)));
        const FmFindArgs a{fm.L.bytes, fm.L.d_off, ix.blocks, ix.base, ix.cp, pat.bytes, pat.d_off, static_cast<uint32_t>(pat.count),
                           static_cast<uint32_t>(fm.L.total), static_cast<uint32_t>(count), d_lo, d_cnt, out.d_occ};
        const unsigned grid = static_cast<unsigned>(std::min<size_t>(div_up(npairs, FM_WAVES), 1u << 20));
        k_fm_find_count<<<dim3(grid), dim3(64 * FM_WAVES), 0, st>>>(a);
    }
    {
        LaunchScope ls(ctx, K_CHAIN, 16.0 * npairs);  // occ read twice, the offsets written
        fm_scan_pairs(ctx, g, d_cnt, chunk_sum, &ctx->d_mail->fm_find.total, d_offset);
    }
    DK_HIP(ctx, hipGetLastError());
    DK_TRY(ctx->mail_read(&ctx->h_mail->fm_find.total));
    const size_t nhits = out.take(ctx->h_mail->fm_find.total);
    if (nhits) {
        const FmFindLocArgs a{fm_walk(fm, ix), fm.L.d_off, d_lo, d_offset, static_cast<uint32_t>(npairs), static_cast<uint32_t>(count),
                              static_cast<uint32_t>(nhits), static_cast<uint4 *>(out.d_hits)};
        const unsigned grid = static_cast<unsigned>(std::min<size_t>(div_up(nhits, FM_WAVES), 1u << 20));
        {
            // per hit four rounds of 64 offsets, the walk of k_fm_locate and the record
            LaunchScope ls(ctx, K_CHAIN, nhits * (4.0 * 512 + 36.0 + 0.5 * fm.step * (FM_BLOCK + 128 + 64)));
            k_fm_find_locate<<<dim3(grid), dim3(64 * FM_WAVES), 0, st>>>(a);
        }
        DK_HIP(ctx, hipGetLastError());
        DK_HIP(ctx, hipStreamSynchronize(st));
    }
    ctx->ws_release(mark);
    return DK_OK;
}

size_t fm_near_workspace(size_t npairs) { return 2 * ws_round(4 * npairs) + ws_round(8 * npairs) + 2 * ws_round(8 * FM_MAX_CHUNKS); }

int fm_near_device(dk_ctx *ctx, const FmView &fm, const ItemView &cls, uint32_t k, uint32_t node_limit, const HitSink &out, uint64_t *cut_out) {
    hipStream_t st = ctx->stream;
    const FmIndex ix = fm_carve(fm);
    const FmPairs g = fm_pairs(cls.count, fm.L.count);
    const size_t npairs = g.npairs, count = fm.L.count, mark = ctx->ws_mark();
    uint32_t *d_cnt = ctx->ws_alloc<uint32_t>(npairs), *d_cut = ctx->ws_alloc<uint32_t>(npairs);
    uint64_t *d_offset = ctx->ws_alloc<uint64_t>(npairs), *chunk_sum = ctx->ws_alloc<uint64_t>(FM_MAX_CHUNKS), *cut_sum = ctx->ws_alloc<uint64_t>(FM_MAX_CHUNKS);
    if (!d_cnt || !d_cut || !d_offset || !chunk_sum || !cut_sum) return DK_E_NOMEM;
    FmNearArgs a{fm.L.bytes, fm.L.d_off, ix.blocks, ix.base, ix.cp, cls.bytes, cls.d_off, static_cast<uint32_t>(cls.count), static_cast<uint32_t>(fm.L.total),
                 static_cast<uint32_t>(count), static_cast<uint32_t>(ix.rows), k, node_limit ? node_limit : DK_FM_NEAR_NODE_LIMIT,
                 d_cnt, d_cut, out.d_occ, d_offset, 0u, static_cast<uint4 *>(out.d_hits)};
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(div_up(npairs, FM_WAVES), 1u << 20));
    // What a pair's tree costs is the answer itself.  The bytes given are those of the one path a search without branching takes -- find's, with
    // 32 bytes of class per position -- so the slot's GB/s is a lower bound.
    const double path_bytes = static_cast<double>(count) * cls.nbytes * (32.0 + 2.0 * (FM_BLOCK + 64));
    {
        LaunchScope ls(ctx, K_CHAIN, 20.0 * npairs + path_bytes);
        k_fm_near_count<<<dim3(grid), dim3(64 * FM_WAVES), 0, st>>>(a);
    }
    {
        LaunchScope ls(ctx, K_CHAIN, 24.0 * npairs);  // occ read twice, the cut flags once, the offsets written
        fm_scan_pairs(ctx, g, d_cnt, chunk_sum, &ctx->d_mail->fm_find.total, d_offset);
        fm_scan_pairs(ctx, g, d_cut, cut_sum, &ctx->d_mail->fm_find.near_cut, nullptr);
    }
    DK_HIP(ctx, hipGetLastError());
    DK_TRY(ctx->mail_read(&ctx->h_mail->fm_find));
    if (cut_out) *cut_out = ctx->h_mail->fm_find.near_cut;
    a.nhits = static_cast<uint32_t>(out.take(ctx->h_mail->fm_find.total));
    if (a.nhits) {
        const FmNearLocArgs l{fm_walk(fm, ix), fm.L.d_off, static_cast<uint32_t>(count), a.nhits, static_cast<uint4 *>(out.d_hits)};
        {
            LaunchScope ls(ctx, K_CHAIN, 12.0 * npairs + path_bytes + 16.0 * a.nhits);  // the pairs' walks again, and the records
            k_fm_near_emit<<<dim3(grid), dim3(64 * FM_WAVES), 0, st>>>(a);
        }
        {
            // per record the walk of k_fm_locate; the record read, its position written
            LaunchScope ls(ctx, K_CHAIN, a.nhits * (36.0 + 0.5 * fm.step * (FM_BLOCK + 128 + 64)));
            const unsigned lgrid = static_cast<unsigned>(std::min<size_t>(div_up(a.nhits, FM_WAVES), 1u << 20));
            k_fm_near_locate<<<dim3(lgrid), dim3(64 * FM_WAVES), 0, st>>>(l);
        }
        DK_HIP(ctx, hipGetLastError());
        DK_HIP(ctx, hipStreamSynchronize(st));
    }
    ctx->ws_release(mark);
    return DK_OK;
}

int fm_extract_device(dk_ctx *ctx, const FmView &fm, const uint32_t *d_pos, const uint32_t *d_len, const uint32_t *d_rng_blk, size_t nrange, size_t max_len,
                      uint8_t *d_out) {
    const FmIndex ix = fm_carve(fm);
    const size_t per = div_up(max_len, fm.step) + 1, nitems = nrange * per;  // the most chunks a range of max_len bytes can touch
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(div_up(nitems, FM_WAVES), 1u << 20));
    const FmExtArgs a{fm.L.bytes, fm.L.d_off, fm.d_abase, ix.blocks, ix.base, ix.cp, static_cast<const uint32_t *>(fm.ext) + FM_EXT_HEADER, d_pos, d_len,
                      d_rng_blk, static_cast<uint32_t>(nrange), static_cast<uint32_t>(max_len), static_cast<uint32_t>(per),
                      static_cast<uint32_t>(fm.L.total), static_cast<uint32_t>(ceil_log2_u64(fm.step)), d_out};
    DK_HIP(ctx, hipMemsetAsync(d_out, 0, nrange * max_len, ctx->stream));  // the zeros behind every range: the kernel stores text bytes only
    {
        // per range its two words and its row, twice (zeros, bytes); per byte and per step / 2 bytes walked in vain a row of L and a checkpoint word
        LaunchScope ls(ctx, K_CHAIN, nrange * (8.0 + 2.0 * max_len + (max_len + 0.5 * fm.step) * (FM_BLOCK + 64)));
        k_fm_extract<<<dim3(grid), dim3(64 * FM_WAVES), 0, ctx->stream>>>(a);
    }
    DK_HIP(ctx, hipGetLastError());
    return DK_OK;
}

FmSeamPlan fm_seam_plan(const std::vector<uint32_t> &off, size_t prev_len, size_t W) {
    FmSeamPlan pl;
    const size_t count = off.size() - 1;
    std::vector<uint32_t> geo(3 * count), blk, pos, len, out;
    size_t at = prev_len, run = 0;
    pl.max_len = 1;
    auto range = [&](size_t b, size_t p, size_t l) {
        blk.push_back(static_cast<uint32_t>(b)), pos.push_back(static_cast<uint32_t>(p)), len.push_back(static_cast<uint32_t>(l));
        out.push_back(static_cast<uint32_t>(at));
        pl.max_len = std::max(pl.max_len, l);
        at += l;
    };
    for (size_t b = 0; b < count; ++b) {
        const size_t nb = off[b + 1] - off[b];
        geo[3 * b] = static_cast<uint32_t>(at), geo[3 * b + 1] = static_cast<uint32_t>(std::min(nb, W)), geo[3 * b + 2] = static_cast<uint32_t>(run);
        if (b + 1 == count) {
            range(b, 0, std::min(nb, W));  // nothing follows the last block: its head is all a match can need
        } else if (nb <= 2 * W) {
            range(b, 0, nb);
        } else {
            range(b, 0, W);
            run = at;  // the run breaks here: the block's middle is not in the strip
            range(b, nb - W, W);
        }
    }
    pl.nrange = blk.size();
    pl.strip_len = at;
    pl.words = std::move(geo);
    for (const auto *v : {&blk, &pos, &len, &out}) pl.words.insert(pl.words.end(), v->begin(), v->end());
    return pl;
}

size_t fm_seams_workspace(const FmSeamPlan &pl, size_t npairs) {
    return ws_round(std::max<size_t>(pl.strip_len, 1)) + ws_round(4 * pl.words.size()) + ws_round(4 * npairs) + ws_round(8 * npairs) + ws_round(8 * FM_MAX_CHUNKS);
}

int fm_seams_device(dk_ctx *ctx, const FmView &fm, const uint8_t *d_prev, size_t prev_len, const FmSeamPlan &pl, const ItemView &pat, const HitSink &out) {
    hipStream_t st = ctx->stream;
    const FmIndex ix = fm_carve(fm);
    const FmPairs g = fm_pairs(pat.count, fm.L.count);
    const size_t npairs = g.npairs, count = fm.L.count, mark = ctx->ws_mark(), nr = pl.nrange;
    uint8_t *strip = ctx->ws_alloc<uint8_t>(std::max<size_t>(pl.strip_len, 1));
    uint32_t *d_plan = ctx->ws_alloc<uint32_t>(pl.words.size()), *d_cnt = ctx->ws_alloc<uint32_t>(npairs);
    uint64_t *d_offset = ctx->ws_alloc<uint64_t>(npairs), *chunk_sum = ctx->ws_alloc<uint64_t>(FM_MAX_CHUNKS);
    if (!strip || !d_plan || !d_cnt || !d_offset || !chunk_sum) return DK_E_NOMEM;
    const uint32_t *d_geo = d_plan, *d_blk = d_plan + 3 * count, *d_pos = d_blk + nr, *d_len = d_pos + nr, *d_out_off = d_len + nr;
    // (pl outlives the copy: mail_read below synchronises, and so does every caller on failure)
    DK_HIP(ctx, hipMemcpyAsync(d_plan, pl.words.data(), pl.words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    DK_HIP(ctx, hipMemsetAsync(strip, 0, std::max<size_t>(pl.strip_len, 1), st));
    if (prev_len) DK_HIP(ctx, hipMemcpyAsync(strip, d_prev, prev_len, hipMemcpyDeviceToDevice, st));
    {
        const size_t per = div_up(pl.max_len, fm.step) + 1, nitems = nr * per;
        const FmExtArgs e{fm.L.bytes, fm.L.d_off, fm.d_abase, ix.blocks, ix.base, ix.cp, static_cast<const uint32_t *>(fm.ext) + FM_EXT_HEADER, d_pos, d_len,
                          d_blk, static_cast<uint32_t>(nr), static_cast<uint32_t>(pl.max_len), static_cast<uint32_t>(per),
                          static_cast<uint32_t>(fm.L.total), static_cast<uint32_t>(ceil_log2_u64(fm.step)), strip, d_out_off};
        const unsigned grid = static_cast<unsigned>(std::min<size_t>(div_up(nitems, FM_WAVES), 1u << 20));
        // extract's traffic for the strip's bytes: per byte, and per step / 2 bytes walked in vain per range, a row of L and a checkpoint word
        LaunchScope ls(ctx, K_CHAIN, 16.0 * nr + 2.0 * pl.strip_len + (static_cast<double>(pl.strip_len) + 0.5 * fm.step * nr) * (FM_BLOCK + 64));
        k_fm_extract<<<dim3(grid), dim3(64 * FM_WAVES), 0, st>>>(e);
    }
    FmSeamArgs a{strip, d_geo, pat.bytes, pat.d_off, static_cast<uint32_t>(pat.count), static_cast<uint32_t>(count), static_cast<uint32_t>(pl.strip_len),
                 d_cnt, out.d_occ, d_offset, 0u, static_cast<uint4 *>(out.d_hits)};
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(div_up(npairs, FM_WAVES), 1u << 20));
    {
        // per pair its three words, the pattern's first word per candidate (a mismatch ends a compare; pat.nbytes / pat.count candidates at most) and occ
        LaunchScope ls(ctx, K_CHAIN, 24.0 * npairs + 16.0 * static_cast<double>(count) * pat.nbytes);
        k_fm_seam_count<<<dim3(grid), dim3(64 * FM_WAVES), 0, st>>>(a);
    }
    {
        LaunchScope ls(ctx, K_CHAIN, 16.0 * npairs);  // occ read twice, the offsets written
        fm_scan_pairs(ctx, g, d_cnt, chunk_sum, &ctx->d_mail->fm_find.total, d_offset);
    }
    DK_HIP(ctx, hipGetLastError());
    DK_TRY(ctx->mail_read(&ctx->h_mail->fm_find.total));
    a.nhits = static_cast<uint32_t>(out.take(ctx->h_mail->fm_find.total));
    if (a.nhits) {
        {
            // per pair occ and its offset; per hit the pair's compare again and the record
            LaunchScope ls(ctx, K_CHAIN, 12.0 * npairs + a.nhits * 48.0);
            k_fm_seam_emit<<<dim3(grid), dim3(64 * FM_WAVES), 0, st>>>(a);
        }
        DK_HIP(ctx, hipGetLastError());
        DK_HIP(ctx, hipStreamSynchronize(st));
    }
    ctx->ws_release(mark);
    return DK_OK;
}

}  // namespace dk
