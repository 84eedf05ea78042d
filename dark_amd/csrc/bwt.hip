// Forward BWT emit and inverse BWT.
//
// Forward: replaces compress::bwt::TransformIterator as driven by src/block/dc.rs:45-50 (known answers
// src/saca.rs:411-412): L[j] = T[SA[j]-1], L[j] = T[n-1] where SA[j] == 0, origin = that j.
//
// Inverse: replaces compress::bwt::decode as driven by src/block/dc.rs:154-156 (in-repo analogue
// etc/dark-c/src/archon3.cpp:70-86).  The serial "follow the jump table n times" becomes
//   k_ibwt_hist / scan   per-tile symbol histograms -> stable counting-sort offsets (one 8-bit radix pass over L)
//   k_ibwt_lf            psi[LF(i)] = i, with the origin element placed first in its symbol class (same rule as
//                        the reference's table build), psi[class start of L[origin]] = END
//   k_ibwt_walk          every position that is a multiple of S (plus origin) is a splitter; one lane per splitter
//                        walks psi to the next splitter and records (next splitter, steps)
//   k_ibwt_rank          pointer jumping over the reduced list -> text offset of every splitter
//   k_ibwt_emit          one lane per splitter re-walks its sub-list and writes the text bytes
// Packed inverse (k_pib_*): the same stages over many blocks laid back to back, segmented by the offsets table.
// The FM-index's locate structure (fm_locate_build_device): the packed inverse's table, walk and jumps, then k_pib_locate
// twice where the inverse writes the text -- the walk knows the text position of every slot it passes.  The extract structure
// (fm_extract_build_device, section 4.15) is the same front part and one such walk, k_pib_anchors.
#include <algorithm>

#include "context.hpp"
#include "device_util.hpp"

namespace dk {
namespace {

// ---- forward ------------------------------------------------------------------------------------------------------
constexpr int BG_PER_THREAD = 16;  // gathers in flight per thread (all addresses first, then all symbols): the kernel is latency-bound
__global__ __launch_bounds__(256) void k_bwt_gather(const uint8_t *__restrict__ t, const uint32_t *__restrict__ sa, size_t n,
                                                     uint8_t *__restrict__ bwt, uint32_t *__restrict__ origin) {
    const size_t j0 = (static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x) * BG_PER_THREAD;
    if (j0 >= n) return;
    if (j0 + BG_PER_THREAD <= n && (reinterpret_cast<uintptr_t>(bwt) & 15) == 0 && (reinterpret_cast<uintptr_t>(sa) & 15) == 0) {
        uint32_t p[BG_PER_THREAD];
#pragma unroll
        for (int q = 0; q < BG_PER_THREAD / 4; ++q) {
            const uint4 v = reinterpret_cast<const uint4 *>(sa + j0)[q];
            p[4 * q] = v.x; p[4 * q + 1] = v.y; p[4 * q + 2] = v.z; p[4 * q + 3] = v.w;
        }
        uint8_t c[BG_PER_THREAD];
#pragma unroll
        for (int k = 0; k < BG_PER_THREAD; ++k) c[k] = t[p[k] ? p[k] - 1 : n - 1];
        uint32_t w[BG_PER_THREAD / 4];
#pragma unroll
        for (int q = 0; q < BG_PER_THREAD / 4; ++q)
            w[q] = c[4 * q] | (static_cast<uint32_t>(c[4 * q + 1]) << 8) | (static_cast<uint32_t>(c[4 * q + 2]) << 16) | (static_cast<uint32_t>(c[4 * q + 3]) << 24);
#pragma unroll
        for (int k = 0; k < BG_PER_THREAD; ++k)
            if (p[k] == 0) *origin = static_cast<uint32_t>(j0 + k);
        *reinterpret_cast<uint4 *>(bwt + j0) = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
    for (size_t j = j0; j < n && j < j0 + BG_PER_THREAD; ++j) {
        const uint32_t p = sa[j];
        if (p == 0) { bwt[j] = t[n - 1]; *origin = static_cast<uint32_t>(j); } else { bwt[j] = t[p - 1]; }
    }
}

// ---- inverse ------------------------------------------------------------------------------------------------------
constexpr uint32_t IB_END = 0xFFFFFFFFu;
constexpr int IB_BLOCK = 256;
constexpr int IB_WAVES = IB_BLOCK / 64;
constexpr int IB_SPT = 16;                    // symbols per thread
constexpr int IB_TILE = IB_BLOCK * IB_SPT;    // 4096 symbols per workgroup
constexpr int IB_MAX_CHUNKS = 256;

// 16 private copies of the histogram (copy = lane mod 16): the BWT is made of runs, and LDS atomics of one wave instruction that hit the
// same counter are serialised (one copy: 0.25 ms per 1e8 bytes; the radix sort's digit-plane histogram has the same shape)
__global__ __launch_bounds__(IB_BLOCK) void k_ibwt_hist(const uint8_t *__restrict__ bwt, size_t n, uint32_t *__restrict__ tile_hist) {
    __shared__ uint32_t h[16][256];
    const int tid = threadIdx.x;
    for (int i = tid; i < 16 * 256; i += IB_BLOCK) (&h[0][0])[i] = 0;
    __syncthreads();
    uint32_t *mine = h[tid & 15];
    const size_t base = static_cast<size_t>(blockIdx.x) * IB_TILE;
    static_assert(IB_TILE == IB_BLOCK * 16, "one 16-byte load per thread");
    if (base + IB_TILE <= n && (reinterpret_cast<uintptr_t>(bwt) & 15) == 0) {
        const uint4 v = reinterpret_cast<const uint4 *>(bwt + base)[tid];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int b = 0; b < 4; ++b) atomicAdd(&mine[(w[k] >> (8 * b)) & 0xFFu], 1u);
        }
    } else {
#pragma unroll
        for (int k = 0; k < IB_SPT; ++k) {
            const size_t i = base + static_cast<size_t>(k) * IB_BLOCK + tid;
            if (i < n) atomicAdd(&mine[bwt[i]], 1u);
        }
    }
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) sum += h[c][tid];
    tile_hist[static_cast<size_t>(blockIdx.x) * 256 + tid] = sum;
}
// digit-major exclusive scan of tile_hist, same three phases as the radix sort; class_start[256] also exported
__global__ __launch_bounds__(256) void k_ibwt_scan_a(const uint32_t *__restrict__ tile_hist, size_t ntiles, size_t tpc,
                                                      uint32_t *__restrict__ chunk_sum) {
    const size_t g = blockIdx.x, t0 = g * tpc, t1 = t0 + tpc < ntiles ? t0 + tpc : ntiles;
    uint32_t s = 0;
#pragma unroll 8
    for (size_t t = t0; t < t1; ++t) s += tile_hist[t * 256 + threadIdx.x];
    chunk_sum[g * 256 + threadIdx.x] = s;
}
__global__ __launch_bounds__(256) void k_ibwt_scan_b(uint32_t *__restrict__ chunk_sum, size_t nchunks, uint32_t *__restrict__ class_start) {
    __shared__ uint32_t s_tmp[IB_WAVES + 1];
    const int d = threadIdx.x;
    uint32_t run = 0;
#pragma unroll 8
    for (size_t g = 0; g < nchunks; ++g) {
        const uint32_t v = chunk_sum[g * 256 + d];
        chunk_sum[g * 256 + d] = run;
        run += v;
    }
    const uint32_t base = block_excl_sum<IB_WAVES>(run, s_tmp, nullptr);
    class_start[d] = base;
#pragma unroll 8
    for (size_t g = 0; g < nchunks; ++g) chunk_sum[g * 256 + d] += base;
}
__global__ __launch_bounds__(256) void k_ibwt_scan_c(uint32_t *__restrict__ tile_hist, size_t ntiles, size_t tpc,
                                                      const uint32_t *__restrict__ chunk_sum) {
    const size_t g = blockIdx.x, t0 = g * tpc, t1 = t0 + tpc < ntiles ? t0 + tpc : ntiles;
    uint32_t run = chunk_sum[g * 256 + threadIdx.x];
    for (size_t t = t0; t < t1; ++t) {
        const uint32_t v = tile_hist[t * 256 + threadIdx.x];
        tile_hist[t * 256 + threadIdx.x] = run;
        run += v;
    }
}

// psi[LF(i)] = i.  LF is the stable counting-sort destination of L[i], except that the origin element goes first in
// its class (it is the suffix consisting of the last text symbol alone, the smallest of its class).
__global__ __launch_bounds__(IB_BLOCK) void k_ibwt_lf(const uint8_t *__restrict__ bwt, size_t n, uint32_t origin,
                                                       const uint32_t *__restrict__ tile_offs, const uint32_t *__restrict__ class_start,
                                                       uint64_t *__restrict__ psi) {
    __shared__ uint32_t s_cnt[IB_WAVES][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t tile_base = static_cast<size_t>(blockIdx.x) * IB_TILE;
    for (int i = tid; i < IB_WAVES * 256; i += IB_BLOCK) (&s_cnt[0][0])[i] = 0;
    const uint32_t wbase = static_cast<uint32_t>(wave) * (64 * IB_SPT);
    uint32_t sym[IB_SPT], rnk[IB_SPT];
#pragma unroll
    for (int k = 0; k < IB_SPT; ++k) {
        const size_t i = tile_base + wbase + k * 64 + lane;
        sym[k] = i < n ? bwt[i] : 0x100u;  // 0x100 = padding, ranked but never stored
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < IB_SPT; ++k) {
        const uint32_t d = sym[k] & 0xFFu;
        const bool pad = sym[k] > 0xFFu;
        const LaneSet same = wave_match<8>(d, __ballot(!pad));
        const uint32_t before = same.before();
        const uint32_t old = pad ? 0u : s_cnt[wave][d];
        __builtin_amdgcn_wave_barrier();
        if (!pad && before == 0) s_cnt[wave][d] = old + same.count();
        __builtin_amdgcn_wave_barrier();
        rnk[k] = old + before;
    }
    __syncthreads();
    {
        const int d = tid;
        uint32_t run = tile_offs[static_cast<size_t>(blockIdx.x) * 256 + d];
#pragma unroll
        for (int w = 0; w < IB_WAVES; ++w) {
            const uint32_t c = s_cnt[w][d];
            s_cnt[w][d] = run;
            run += c;
        }
    }
    __syncthreads();
    const uint32_t c0 = bwt[origin];
    const uint32_t c0_start = class_start[c0];
#pragma unroll
    for (int k = 0; k < IB_SPT; ++k) {
        const size_t i = tile_base + wbase + k * 64 + lane;
        if (i >= n) continue;
        uint32_t dest = s_cnt[wave][sym[k]] + rnk[k];
        if (i == origin) dest = c0_start;
        else if (sym[k] == c0 && i < origin) dest += 1;
        // the origin element has no successor: following it ends the text (the reference stores table[..] = 0 there).
        // The entry also carries the symbol the step emits (L[i]), so that a walk makes ONE dependent random load per step.
        psi[dest] = (static_cast<uint64_t>(sym[k]) << 32) | (i == origin ? IB_END : static_cast<uint32_t>(i));
    }
}

// Splitters: positions that are multiples of S, and origin (the start of the text).  Splitter id of position p:
// p / S for p % S == 0; id nsplit-1 is reserved for origin when origin is not a multiple of S.
__device__ __forceinline__ bool is_splitter(uint32_t p, uint32_t S, uint32_t origin) { return (p % S) == 0 || p == origin; }
__device__ __forceinline__ uint32_t splitter_id(uint32_t p, uint32_t S, uint32_t origin, uint32_t nreg) {
    return (p == origin && (p % S) != 0) ? nreg : p / S;
}
// the splitter the text starts at: its chain to END is the whole text, n entries, exactly when (L, origin) describes one
__device__ __forceinline__ uint32_t origin_splitter(uint32_t origin, uint32_t S, uint32_t nreg) { return splitter_id(origin, S, origin, nreg); }

// Text step k visits position cur_k: cur_0 = origin, cur_{k+1} = psi[cur_k]... with the reference's convention the
// text symbol k is L[psi[cur_k]], and the last symbol is L[origin] when psi hits END.
// rec (may be null): the walk also RECORDS the symbols it passes -- the first IB_REC of them, eight at a time, into the splitter's own
// IB_REC-byte stretch of `rec` -- and the position a longer walk stands at after IB_REC steps (resume); k_ibwt_copy then writes the text
// from these records instead of walking the successor table a second time (one random 64-byte line per text byte saved).
constexpr uint32_t IB_REC = 256;
__global__ __launch_bounds__(256) void k_ibwt_walk(const uint64_t *__restrict__ psi, uint32_t n, uint32_t origin, uint32_t S,
                                                    uint32_t nreg, uint32_t nsplit, uint32_t *__restrict__ nxt,
                                                    uint32_t *__restrict__ len, uint32_t *__restrict__ len_keep, uint8_t *__restrict__ rec,
                                                    uint32_t *__restrict__ resume) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsplit) return;
    uint32_t cur;
    if (s == nreg) {
        cur = origin;  // only exists when origin % S != 0
    } else {
        cur = s * S;
        if (cur >= n) { nxt[s] = IB_END; len[s] = 0; if (len_keep) len_keep[s] = 0; return; }
    }
    uint32_t steps = 0, to = IB_END;
    uint64_t acc = 0;
    uint64_t *out = rec ? reinterpret_cast<uint64_t *>(rec + static_cast<size_t>(s) * IB_REC) : nullptr;
    for (;;) {
        const uint64_t e = psi[cur];
        const uint32_t p = static_cast<uint32_t>(e);
        if (rec && steps < IB_REC) {
            acc |= (e >> 32 & 0xFFull) << (8 * (steps & 7u));  // the symbol this step emits
            if ((steps & 7u) == 7u) { out[steps >> 3] = acc; acc = 0; }
        }
        ++steps;  // this step emits one text symbol
        if (p == IB_END) break;
        if (is_splitter(p, S, origin)) { to = splitter_id(p, S, origin, nreg); break; }
        cur = p;
        if (rec && steps == IB_REC) resume[s] = cur;  // where a walk longer than the record goes on
        if (steps > n) break;  // corrupt input: never spin
    }
    if (rec && steps < IB_REC && (steps & 7u)) out[steps >> 3] = acc;  // the last, partial word (the stretch is the splitter's own)
    nxt[s] = to;
    len[s] = steps;
    if (len_keep) len_keep[s] = steps;
}

// pointer jumping: dist_to_end[s] = len[s] + dist_to_end[nxt[s]]
__global__ __launch_bounds__(256) void k_ibwt_jump(const uint32_t *__restrict__ nxt_in, const uint32_t *__restrict__ acc_in,
                                                    uint32_t *__restrict__ nxt_out, uint32_t *__restrict__ acc_out, uint32_t nsplit,
                                                    uint32_t *__restrict__ pending) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsplit) return;
    const uint32_t to = nxt_in[s];
    uint32_t a = acc_in[s];
    if (to == IB_END) {
        nxt_out[s] = IB_END;
        acc_out[s] = a;
        return;
    }
    a += acc_in[to];
    const uint32_t to2 = nxt_in[to];
    nxt_out[s] = to2;
    acc_out[s] = a;
    if (to2 != IB_END) *pending = 1;
}

__global__ __launch_bounds__(256) void k_ibwt_emit(const uint8_t *__restrict__ bwt, const uint64_t *__restrict__ psi, uint32_t n,
                                                    uint32_t origin, uint32_t S, uint32_t nreg, uint32_t nsplit,
                                                    const uint32_t *__restrict__ dist_to_end, uint8_t *__restrict__ out,
                                                    uint32_t *__restrict__ bad) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsplit) return;
    uint32_t cur;
    if (s == nreg) cur = origin;
    else { cur = s * S; if (cur >= n) return; }
    const uint32_t d = dist_to_end[s];
    // not on the text cycle, or the origin's chain is shorter than the block: the rest sits in cycles that hold no splitter and that no lane
    // visits, and text[0 .. n - d) would stay unwritten (corrupt input)
    if (d > n || (s == origin_splitter(origin, S, nreg) && d != n)) { *bad = 1; return; }
    uint32_t k = n - d;  // text offset of the first symbol this splitter emits
    // bytes are gathered into a 64-bit word and leave as one aligned 8-byte store (single bytes only at the ragged ends)
    const bool wide = (reinterpret_cast<uintptr_t>(out) & 7) == 0;
    uint64_t acc = 0;
    uint32_t have = 0;
    auto put = [&](uint8_t b) {
        if (wide && (have > 0 || (k & 7u) == 0)) {
            acc |= static_cast<uint64_t>(b) << (8 * have);
            ++have;
            ++k;
            if (have == 8) {
                *reinterpret_cast<uint64_t *>(out + k - 8) = acc;
                acc = 0;
                have = 0;
            }
        } else {
            out[k++] = b;
        }
    };
    for (;;) {
        const uint64_t e = psi[cur];
        const uint32_t p = static_cast<uint32_t>(e);
        const uint8_t symbol = static_cast<uint8_t>(e >> 32);  // = L[p], or L[origin] on the terminal entry
        if (p == IB_END) { if (k < n) put(symbol); else *bad = 1; break; }
        if (k >= n) { *bad = 1; break; }
        put(symbol);
        if (is_splitter(p, S, origin)) break;
        cur = p;
    }
    for (uint32_t jj = 0; jj < have; ++jj) out[k - have + jj] = static_cast<uint8_t>(acc >> (8 * jj));
}

// the text from the walk's records: splitter s owns text[n - dist_to_end[s] .. + len[s]); its first IB_REC bytes are in its record, the
// rest (walks longer than the record: 2 % of them at S = 64) is walked from resume[s] as k_ibwt_emit does
__global__ __launch_bounds__(256) void k_ibwt_copy(const uint64_t *__restrict__ psi, uint32_t n, uint32_t origin, uint32_t S, uint32_t nreg,
                                                    uint32_t nsplit, const uint32_t *__restrict__ dist_to_end, const uint32_t *__restrict__ len,
                                                    const uint8_t *__restrict__ rec, const uint32_t *__restrict__ resume,
                                                    uint8_t *__restrict__ out, uint32_t *__restrict__ bad) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsplit) return;
    if (s != nreg && static_cast<uint64_t>(s) * S >= n) return;
    const uint32_t d = dist_to_end[s], total = len[s];
    // not on the text cycle, or (as in k_ibwt_emit) the origin's chain does not cover the whole block (corrupt input)
    if (d > n || total > d || (s == origin_splitter(origin, S, nreg) && d != n)) { *bad = 1; return; }
    uint32_t k = n - d;
    const bool wide = (reinterpret_cast<uintptr_t>(out) & 7) == 0;
    uint64_t acc = 0;
    uint32_t have = 0;
    auto put = [&](uint8_t b) {
        if (wide && (have > 0 || (k & 7u) == 0)) {
            acc |= static_cast<uint64_t>(b) << (8 * have);
            ++have;
            ++k;
            if (have == 8) {
                *reinterpret_cast<uint64_t *>(out + k - 8) = acc;
                acc = 0;
                have = 0;
            }
        } else {
            out[k++] = b;
        }
    };
    const uint64_t *src = reinterpret_cast<const uint64_t *>(rec + static_cast<size_t>(s) * IB_REC);
    const uint32_t recorded = total < IB_REC ? total : IB_REC;
    for (uint32_t j = 0; j < recorded; j += 8) {
        const uint64_t w = src[j >> 3];
        const uint32_t cnt = recorded - j < 8 ? recorded - j : 8;
        for (uint32_t b = 0; b < cnt; ++b) put(static_cast<uint8_t>(w >> (8 * b)));
    }
    if (total > IB_REC) {
        uint32_t cur = resume[s], left = total - IB_REC;
        while (left--) {
            const uint64_t e = psi[cur];
            put(static_cast<uint8_t>(e >> 32));
            cur = static_cast<uint32_t>(e);
            if (cur == IB_END && left) { *bad = 1; break; }
        }
    }
    for (uint32_t jj = 0; jj < have; ++jj) out[k - have + jj] = static_cast<uint8_t>(acc >> (8 * jj));
}

// ---- packed inverse ------------------------------------------------------------------------------------------
// Block i of a pack is [off_i, e_i), e_i = off_{i+1}, with origin o_i (local).  Positions, psi entries and splitter ids are pack-global.
// G(p, c) = class_start[c] + occurrences of c in the pack before p: what k_ibwt_hist and the three scans give over the whole pack.  Block i's
// LF is base_i[c] + G(p, c) with base_i[c] = off_i + (symbols below c in block i) - G(off_i, c): the pack-wide class start cancels, so the
// single-block histogram and scans serve the pack unchanged and the only per-block table is base (count x 256).
// Splitters of block i are [sb_i, sb_{i+1}): local positions j S for j < nreg_i = ceil(n_i / S), then o_i when it is no multiple of S.

// largest i in [lo, hi) with off[i] <= p (off[lo] <= p < off[hi])
__device__ __forceinline__ uint32_t pib_seg(const uint32_t *__restrict__ off, uint32_t lo, uint32_t hi, uint32_t p) {
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

struct PibBlock { uint32_t blk, first, s0, n, org, nreg; };  // block of a splitter: its index, first splitter, first position, size, origin

__device__ __forceinline__ PibBlock pib_block(const uint32_t *__restrict__ off, const uint32_t *__restrict__ org, const uint32_t *__restrict__ sb,
                                              uint32_t count, uint32_t S, uint32_t s) {
    PibBlock b;
    b.blk = pib_seg(sb, 0, count, s);
    b.first = sb[b.blk];
    b.s0 = off[b.blk];
    b.n = off[b.blk + 1] - b.s0;
    b.org = org[b.blk];
    b.nreg = (b.n + S - 1) / S;
    return b;
}
__device__ __forceinline__ uint32_t pib_start(const PibBlock &b, uint32_t S, uint32_t s) {
    const uint32_t j = s - b.first;
    return b.s0 + (j == b.nreg ? b.org : j * S);
}
// splitter id of position p of block b, IB_END when p is none
__device__ __forceinline__ uint32_t pib_splitter_at(const PibBlock &b, uint32_t S, uint32_t p) {
    const uint32_t l = p - b.s0;
    if (l % S == 0) return b.first + l / S;
    return l == b.org ? b.first + b.nreg : IB_END;
}

// G(p, c) for c = threadIdx.x: the scanned offsets of p's tile plus an LDS histogram of the tile's bytes before p (p = total: the last tile)
__device__ __forceinline__ uint32_t pib_occ_before(const uint8_t *__restrict__ bwt, uint32_t p, uint32_t ntiles, const uint32_t *__restrict__ tile_offs,
                                                   uint32_t *h) {
    const uint32_t t = min(p / IB_TILE, ntiles - 1);
    h[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t q = t * IB_TILE + threadIdx.x; q < p; q += IB_BLOCK) atomicAdd(&h[bwt[q]], 1u);
    __syncthreads();
    const uint32_t g = tile_offs[static_cast<size_t>(t) * 256 + threadIdx.x] + h[threadIdx.x];
    __syncthreads();
    return g;
}

// one workgroup per block, one lane per symbol: base_i[c], and cls0_i = where block i's origin element goes (first of its class)
__global__ __launch_bounds__(256) void k_pib_heads(const uint8_t *__restrict__ bwt, const uint32_t *__restrict__ off, const uint32_t *__restrict__ org,
                                                    uint32_t ntiles, const uint32_t *__restrict__ tile_offs, uint32_t *__restrict__ base,
                                                    uint32_t *__restrict__ cls0) {
    __shared__ uint32_t h[256];
    __shared__ uint32_t s_tmp[IB_WAVES + 1];
    const uint32_t i = blockIdx.x, c = threadIdx.x;
    const uint32_t s = off[i], e = off[i + 1];
    const uint32_t g0 = pib_occ_before(bwt, s, ntiles, tile_offs, h);
    const uint32_t g1 = pib_occ_before(bwt, e, ntiles, tile_offs, h);
    const uint32_t below = block_excl_sum<IB_WAVES>(g1 - g0, s_tmp, nullptr);
    base[static_cast<size_t>(i) * 256 + c] = s + below - g0;  // (mod 2^32: only base + G is ever used)
    if (c == bwt[s + org[i]]) cls0[i] = s + below;
}

// k_ibwt_lf over the pack: the rank of every position among its symbol is the same tile/wave computation; the block of a position comes
// from a binary search over the few blocks that meet this tile
__global__ __launch_bounds__(IB_BLOCK) void k_pib_lf(const uint8_t *__restrict__ bwt, uint32_t total, const uint32_t *__restrict__ off, uint32_t count,
                                                      const uint32_t *__restrict__ org, const uint32_t *__restrict__ tile_offs,
                                                      const uint32_t *__restrict__ base, const uint32_t *__restrict__ cls0, uint64_t *__restrict__ psi) {
    __shared__ uint32_t s_cnt[IB_WAVES][256];
    __shared__ uint32_t s_blk[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t tile_base = blockIdx.x * IB_TILE;
    for (int i = tid; i < IB_WAVES * 256; i += IB_BLOCK) (&s_cnt[0][0])[i] = 0;
    if (tid == 0) {
        const uint32_t lo = pib_seg(off, 0, count, tile_base);
        s_blk[0] = lo;
        s_blk[1] = pib_seg(off, lo, count, min(tile_base + IB_TILE, total) - 1) + 1;
    }
    const uint32_t wbase = static_cast<uint32_t>(wave) * (64 * IB_SPT);
    uint32_t sym[IB_SPT], rnk[IB_SPT];
#pragma unroll
    for (int k = 0; k < IB_SPT; ++k) {
        const uint32_t i = tile_base + wbase + k * 64 + lane;
        sym[k] = i < total ? bwt[i] : 0x100u;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < IB_SPT; ++k) {
        const uint32_t d = sym[k] & 0xFFu;
        const bool pad = sym[k] > 0xFFu;
        const LaneSet same = wave_match<8>(d, __ballot(!pad));
        const uint32_t before = same.before();
        const uint32_t old = pad ? 0u : s_cnt[wave][d];
        __builtin_amdgcn_wave_barrier();
        if (!pad && before == 0) s_cnt[wave][d] = old + same.count();
        __builtin_amdgcn_wave_barrier();
        rnk[k] = old + before;
    }
    __syncthreads();
    {
        const int d = tid;
        uint32_t run = tile_offs[static_cast<size_t>(blockIdx.x) * 256 + d];
#pragma unroll
        for (int w = 0; w < IB_WAVES; ++w) {
            const uint32_t c = s_cnt[w][d];
            s_cnt[w][d] = run;
            run += c;
        }
    }
    __syncthreads();
    const uint32_t blo = s_blk[0], bhi = s_blk[1];
#pragma unroll
    for (int k = 0; k < IB_SPT; ++k) {
        const uint32_t i = tile_base + wbase + k * 64 + lane;
        if (i >= total) continue;
        const uint32_t d = sym[k];
        const uint32_t blk = pib_seg(off, blo, bhi, i);
        const uint32_t o = off[blk] + org[blk];
        uint32_t dest = base[static_cast<size_t>(blk) * 256 + d] + s_cnt[wave][d] + rnk[k];
        if (i == o) dest = cls0[blk];
        else if (i < o && d == bwt[o]) dest += 1;
        psi[dest] = (static_cast<uint64_t>(d) << 32) | (i == o ? IB_END : i);
    }
}

// k_ibwt_walk per splitter of the pack; the walk stops at its block's splitters and END, and never runs past n_i steps
__global__ __launch_bounds__(256) void k_pib_walk(const uint64_t *__restrict__ psi, const uint32_t *__restrict__ off, const uint32_t *__restrict__ org,
                                                   const uint32_t *__restrict__ sb, uint32_t count, uint32_t S, uint32_t nsplit,
                                                   uint32_t *__restrict__ nxt, uint32_t *__restrict__ len, uint32_t *__restrict__ len_keep,
                                                   uint8_t *__restrict__ rec, uint32_t *__restrict__ resume) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsplit) return;
    const PibBlock b = pib_block(off, org, sb, count, S, s);
    uint32_t cur = pib_start(b, S, s);
    uint32_t steps = 0, to = IB_END;
    uint64_t acc = 0;
    uint64_t *out = rec ? reinterpret_cast<uint64_t *>(rec + static_cast<size_t>(s) * IB_REC) : nullptr;
    for (;;) {
        const uint64_t e = psi[cur];
        const uint32_t p = static_cast<uint32_t>(e);
        if (rec && steps < IB_REC) {
            acc |= (e >> 32 & 0xFFull) << (8 * (steps & 7u));
            if ((steps & 7u) == 7u) { out[steps >> 3] = acc; acc = 0; }
        }
        ++steps;
        if (p == IB_END) break;
        if (p - b.s0 >= b.n) { steps = b.n + 1; break; }  // (LF maps a block onto itself: never taken; keeps every read inside the block)
        const uint32_t id = pib_splitter_at(b, S, p);
        if (id != IB_END) { to = id; break; }
        cur = p;
        if (rec && steps == IB_REC) resume[s] = cur;
        if (steps > b.n) break;  // corrupt input: never spin
    }
    if (rec && steps < IB_REC && (steps & 7u)) out[steps >> 3] = acc;
    nxt[s] = to;
    len[s] = steps;
    if (len_keep) len_keep[s] = steps;
}

// after the jumps, before anything is written: every splitter resolved, within its block, and the origin's chain covers the whole block
// (a shorter one means a second cycle).  bad = the lowest failing block
__global__ __launch_bounds__(256) void k_pib_check(const uint32_t *__restrict__ off, const uint32_t *__restrict__ org, const uint32_t *__restrict__ sb,
                                                    uint32_t count, uint32_t S, uint32_t nsplit, const uint32_t *__restrict__ nxt,
                                                    const uint32_t *__restrict__ dist, const uint32_t *__restrict__ len_keep, uint32_t *__restrict__ bad) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsplit) return;
    const PibBlock b = pib_block(off, org, sb, count, S, s);
    const uint32_t j = s - b.first, d = dist[s];
    const bool at_origin = j == b.nreg || (b.org % S == 0 && j == b.org / S);
    if (nxt[s] != IB_END || d > b.n || (len_keep && len_keep[s] > d) || (at_origin && d != b.n)) atomicMin(bad, b.blk);
}

// byte writer of one lane: aligned 8-byte stores where all eight bytes are this lane's, single bytes at the ragged ends
struct PibPut {
    uint8_t *out;
    uint32_t k;
    bool wide;
    uint64_t acc = 0;
    uint32_t have = 0;
    __device__ PibPut(uint8_t *o, uint32_t at) : out(o), k(at), wide((reinterpret_cast<uintptr_t>(o) & 7) == 0) {}
    __device__ __forceinline__ void put(uint8_t v) {
        if (wide && (have > 0 || (k & 7u) == 0)) {
            acc |= static_cast<uint64_t>(v) << (8 * have);
            ++have;
            ++k;
            if (have == 8) {
                *reinterpret_cast<uint64_t *>(out + k - 8) = acc;
                acc = 0;
                have = 0;
            }
        } else {
            out[k++] = v;
        }
    }
    __device__ __forceinline__ void flush() {
        for (uint32_t jj = 0; jj < have; ++jj) out[k - have + jj] = static_cast<uint8_t>(acc >> (8 * jj));
    }
};

__global__ __launch_bounds__(256) void k_pib_emit(const uint64_t *__restrict__ psi, const uint32_t *__restrict__ off, const uint32_t *__restrict__ org,
                                                   const uint32_t *__restrict__ sb, uint32_t count, uint32_t S, uint32_t nsplit,
                                                   const uint32_t *__restrict__ dist_to_end, uint8_t *__restrict__ out, uint32_t *__restrict__ bad) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsplit) return;
    const PibBlock b = pib_block(off, org, sb, count, S, s);
    const uint32_t d = dist_to_end[s], end = b.s0 + b.n;
    if (d > b.n) { atomicMin(bad, b.blk); return; }
    uint32_t cur = pib_start(b, S, s);
    PibPut w(out, end - d);
    for (;;) {
        const uint64_t e = psi[cur];
        const uint32_t p = static_cast<uint32_t>(e);
        const uint8_t symbol = static_cast<uint8_t>(e >> 32);
        if (p == IB_END) { if (w.k < end) w.put(symbol); else atomicMin(bad, b.blk); break; }
        if (w.k >= end || p - b.s0 >= b.n) { atomicMin(bad, b.blk); break; }
        w.put(symbol);
        if (pib_splitter_at(b, S, p) != IB_END) break;
        cur = p;
    }
    w.flush();
}

__global__ __launch_bounds__(256) void k_pib_copy(const uint64_t *__restrict__ psi, const uint32_t *__restrict__ off, const uint32_t *__restrict__ org,
                                                   const uint32_t *__restrict__ sb, uint32_t count, uint32_t S, uint32_t nsplit,
                                                   const uint32_t *__restrict__ dist_to_end, const uint32_t *__restrict__ len,
                                                   const uint8_t *__restrict__ rec, const uint32_t *__restrict__ resume, uint8_t *__restrict__ out,
                                                   uint32_t *__restrict__ bad) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsplit) return;
    const PibBlock b = pib_block(off, org, sb, count, S, s);
    const uint32_t d = dist_to_end[s], total = len[s];
    if (d > b.n || total > d) { atomicMin(bad, b.blk); return; }
    PibPut w(out, b.s0 + b.n - d);
    const uint64_t *src = reinterpret_cast<const uint64_t *>(rec + static_cast<size_t>(s) * IB_REC);
    const uint32_t recorded = total < IB_REC ? total : IB_REC;
    for (uint32_t j = 0; j < recorded; j += 8) {
        const uint64_t v = src[j >> 3];
        const uint32_t cnt = recorded - j < 8 ? recorded - j : 8;
        for (uint32_t q = 0; q < cnt; ++q) w.put(static_cast<uint8_t>(v >> (8 * q)));
    }
    if (total > IB_REC) {
        uint32_t cur = resume[s], left = total - IB_REC;
        while (left--) {
            const uint64_t e = psi[cur];
            w.put(static_cast<uint8_t>(e >> 32));
            cur = static_cast<uint32_t>(e);
            if ((cur == IB_END || cur - b.s0 >= b.n) && left) { atomicMin(bad, b.blk); break; }
        }
    }
    w.flush();
}

// ---- the FM-index's locate structure (layout: context.hpp fm_locate_words) ----------------------------------------
// The splitter at position cur with dist_to_end d is the slot of suffix n_b - d of its block, and every psi step from it that of the next
// suffix: the walk of k_pib_emit, which here looks at text positions instead of writing text bytes.  Two passes of one kernel.  MARK sets the
// bit of every slot whose (block-local) text position is a multiple of the step, with a vector atomicOr on zeroed words (32 slots of a word
// belong to as many lanes).  After the rows' counts are scanned, SAMPLE stores position / step at the slot's rank among the marks; every
// marked slot has its own entry, so these are plain stores.  Both run behind k_pib_check: every d is in [1, n_b] and every walk stays in
// its block; the tests below keep a walk inside the block and the entry inside the samples whatever the tables hold.
template <bool SAMPLE>
__global__ __launch_bounds__(256) void k_pib_locate(const uint64_t *__restrict__ psi, const uint32_t *__restrict__ off, const uint32_t *__restrict__ org,
                                                     const uint32_t *__restrict__ sb, uint32_t count, uint32_t S, uint32_t nsplit,
                                                     const uint32_t *__restrict__ dist_to_end, uint32_t step_shift, uint32_t *__restrict__ bits,
                                                     const uint32_t *__restrict__ marks, uint32_t *__restrict__ samples, uint32_t nsamp) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsplit) return;
    const PibBlock b = pib_block(off, org, sb, count, S, s);
    const uint32_t d = dist_to_end[s], mask = (1u << step_shift) - 1u;
    if (d == 0 || d > b.n) return;
    uint32_t cur = pib_start(b, S, s), pos = b.n - d;
    for (;;) {
        if ((pos & mask) == 0) {
            const uint32_t word = cur >> 5, bit = 1u << (cur & 31u);
            if (!SAMPLE) {
                atomicOr(&bits[word], bit);
            } else {
                uint32_t r = marks[cur >> 10] + __popc(bits[word] & (bit - 1u));
                for (uint32_t w = word & ~31u; w < word; ++w) r += __popc(bits[w]);
                if (r < nsamp) samples[r] = pos >> step_shift;
            }
        }
        const uint32_t p = static_cast<uint32_t>(psi[cur]);
        if (p == IB_END || p - b.s0 >= b.n || pib_splitter_at(b, S, p) != IB_END || ++pos >= b.n) break;
        cur = p;
    }
}
// The extract structure: the walk of k_pib_locate once more.  Where the text position is a multiple of the step, the
// slot the walk stands on -- the slot of the suffix that starts there -- is that position's anchor.  Every position belongs to one walk, so every
// anchor has one writer: plain stores, no atomics.  abase[b] = block b's first anchor (the host's prefix of ceil(n_i / step)).  Runs behind
// k_pib_check like k_pib_locate, with its tests: a walk stays in its block, a store inside the nanch anchors, whatever the tables hold.
__global__ __launch_bounds__(256) void k_pib_anchors(const uint64_t *__restrict__ psi, const uint32_t *__restrict__ off, const uint32_t *__restrict__ org,
                                                      const uint32_t *__restrict__ sb, uint32_t count, uint32_t S, uint32_t nsplit,
                                                      const uint32_t *__restrict__ dist_to_end, uint32_t step_shift, const uint32_t *__restrict__ abase,
                                                      uint32_t *__restrict__ anchors, uint32_t nanch) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsplit) return;
    const PibBlock b = pib_block(off, org, sb, count, S, s);
    const uint32_t d = dist_to_end[s], mask = (1u << step_shift) - 1u;
    if (d == 0 || d > b.n) return;
    const uint32_t a0 = abase[b.blk];
    uint32_t cur = pib_start(b, S, s), pos = b.n - d;
    for (;;) {
        if ((pos & mask) == 0) {
            const uint32_t at = a0 + (pos >> step_shift);
            if (at < nanch) anchors[at] = cur - b.s0;
        }
        const uint32_t p = static_cast<uint32_t>(psi[cur]);
        if (p == IB_END || p - b.s0 >= b.n || pib_splitter_at(b, S, p) != IB_END || ++pos >= b.n) break;
        cur = p;
    }
}

// marks[r] = set bits of row r (32 words of 32 slots)
__global__ __launch_bounds__(256) void k_loc_rows(const uint32_t *__restrict__ bits, uint32_t rows, uint32_t *__restrict__ marks) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) c += __popc(bits[32 * static_cast<size_t>(r) + k]);  // (words: d_loc is only 4-byte aligned)
    marks[r] = c;
}
// exclusive scan of marks[0, rows) in place, marks[rows] = all marks.  One workgroup: a stretch of rows per thread, summed, scanned over the
// workgroup, written back (one column where k_fm_scan_a/b/c have 256: 4 bytes per KiB of L, no chunk sums to keep)
__global__ __launch_bounds__(1024) void k_loc_scan(uint32_t *__restrict__ marks, uint32_t rows) {
    __shared__ uint32_t s_tmp[16 + 1];
    const uint32_t per = (rows + 1023u) / 1024u, r0 = min(threadIdx.x * per, rows), r1 = min(r0 + per, rows);
    uint32_t sum = 0, all = 0;
    for (uint32_t r = r0; r < r1; ++r) sum += marks[r];
    uint32_t run = block_excl_sum<16>(sum, s_tmp, &all);
    for (uint32_t r = r0; r < r1; ++r) {
        const uint32_t v = marks[r];
        marks[r] = run;
        run += v;
    }
    if (threadIdx.x == 0) marks[rows] = all;
}

}  // namespace

// the origin word back: some kernel has stored the slot of suffix 0 there, whichever way L was written
static int read_origin(dk_ctx *ctx, size_t n, uint32_t *origin) {
    DK_TRY(ctx->mail_read(&ctx->h_mail->origin));
    *origin = ctx->h_mail->origin;
    if (*origin >= n) return ctx->fail(DK_E_INTERNAL, "bwt_forward: no suffix 0 in the suffix array");
    return DK_OK;
}

int bwt_gather_device(dk_ctx *ctx, const uint8_t *d_text, const uint32_t *d_sa, size_t n, uint8_t *d_bwt, uint32_t *origin) {
    hipStream_t st = ctx->stream;
    uint32_t *d_origin = &ctx->d_mail->origin;
    DK_TRY(ctx->mail_fill(d_origin, 0xFF));
    {
        LaunchScope ls(ctx, K_BWT_GATHER, 6.0 * n);
        k_bwt_gather<<<dim3(div_up(div_up(n, BG_PER_THREAD), 256)), dim3(256), 0, st>>>(d_text, d_sa, n, d_bwt, d_origin);
    }
    DK_HIP(ctx, hipGetLastError());
    return read_origin(ctx, n, origin);
}

// suffix sort + BWT: the gather is skipped when the sort already wrote L (suffix_array_device, short-prefix path)
int bwt_forward_device(dk_ctx *ctx, const uint8_t *d_text, size_t n, uint32_t *d_sa, uint8_t *d_bwt, uint32_t *origin) {
    hipStream_t st = ctx->stream;
    uint32_t *d_origin = &ctx->d_mail->origin;
    DK_TRY(ctx->mail_fill(d_origin, 0xFF));
    bool written = false;
    Timer t;
    DK_TRY(suffix_array_device(ctx, d_text, n, d_sa, d_bwt, d_origin, &written));
    DK_HIP(ctx, hipStreamSynchronize(st));
    ctx->stats.ms_sa = t.ms();
    Timer t2;
    if (!written) DK_TRY(bwt_gather_device(ctx, d_text, d_sa, n, d_bwt, origin));
    else DK_TRY(read_origin(ctx, n, origin));
    ctx->stats.ms_bwt = t2.ms();
    return DK_OK;
}

int bwt_inverse_device(dk_ctx *ctx, const uint8_t *d_bwt, size_t n, uint32_t origin, uint8_t *d_out) {
    if (n == 0 || n > 0xFFFFFFF0ull || origin >= n) return ctx->fail(DK_E_ARG, "bwt_inverse: bad n / origin");
    hipStream_t st = ctx->stream;
    const size_t mark = ctx->ws_mark();
    const size_t ntiles = div_up(n, IB_TILE);
    const size_t tpc = div_up(ntiles, IB_MAX_CHUNKS);
    const size_t nchunks = div_up(ntiles, tpc);
    uint32_t *tile_hist = ctx->ws_alloc<uint32_t>(ntiles * 256);
    uint32_t *chunk_sum = ctx->ws_alloc<uint32_t>(nchunks * 256);
    uint32_t *class_start = ctx->ws_alloc<uint32_t>(256);
    uint64_t *psi = ctx->ws_alloc<uint64_t>(n);
    if (!tile_hist || !chunk_sum || !class_start || !psi) return DK_E_NOMEM;
    {
        LaunchScope ls(ctx, K_IBWT_HIST, 1.0 * n);
        k_ibwt_hist<<<dim3(ntiles), dim3(IB_BLOCK), 0, st>>>(d_bwt, n, tile_hist);
        k_ibwt_scan_a<<<dim3(nchunks), dim3(256), 0, st>>>(tile_hist, ntiles, tpc, chunk_sum);
        k_ibwt_scan_b<<<dim3(1), dim3(256), 0, st>>>(chunk_sum, nchunks, class_start);
        k_ibwt_scan_c<<<dim3(nchunks), dim3(256), 0, st>>>(tile_hist, ntiles, tpc, chunk_sum);
    }
    {
        LaunchScope ls(ctx, K_IBWT_LF, 5.0 * n);
        k_ibwt_lf<<<dim3(ntiles), dim3(IB_BLOCK), 0, st>>>(d_bwt, n, origin, tile_hist, class_start, psi);
    }
    DK_HIP(ctx, hipGetLastError());
    // splitters
    const uint32_t S = n < (1u << 16) ? 8u : 64u;  // measured at 1e8: 16 / 32 / 64 / 128 / 256 -> 11.6 / 8.9 / 7.9 / 8.1 / 8.6 ms
    const uint32_t nreg = static_cast<uint32_t>(div_up(n, S));
    const uint32_t nsplit = nreg + ((origin % S) != 0 ? 1u : 0u);
    uint32_t *nxt = ctx->ws_alloc<uint32_t>(nsplit), *nxt_alt = ctx->ws_alloc<uint32_t>(nsplit);
    uint32_t *acc = ctx->ws_alloc<uint32_t>(nsplit), *acc_alt = ctx->ws_alloc<uint32_t>(nsplit);
    if (!nxt || !nxt_alt || !acc || !acc_alt) return DK_E_NOMEM;
    // records of the walk (IB_REC bytes per splitter = 4 n bytes at S = 64): the text is then copied from them instead of walked again
    const bool record = DK_KNOB("DK_IBWT_RECORD", 1) != 0 && S == 64;
    uint32_t *len_keep = record ? ctx->ws_alloc<uint32_t>(nsplit) : nullptr;
    uint32_t *resume = record ? ctx->ws_alloc<uint32_t>(nsplit) : nullptr;
    uint8_t *rec = record ? ctx->ws_alloc<uint8_t>(static_cast<size_t>(nsplit) * IB_REC) : nullptr;
    if (record && (!len_keep || !resume || !rec)) return DK_E_NOMEM;
    {
        LaunchScope ls(ctx, K_IBWT_WALK, (record ? 5.0 : 4.0) * n);
        k_ibwt_walk<<<dim3(div_up(nsplit, 256)), dim3(256), 0, st>>>(psi, static_cast<uint32_t>(n), origin, S, nreg, nsplit, nxt, acc, len_keep, rec, resume);
    }
    DK_HIP(ctx, hipGetLastError());
    // Pointer jumping halves every chain per step: ceil(log2(nsplit)) + 1 steps finish any single path through the splitters.
    // They are enqueued back to back (no host round trip per step); only the last one reports whether something is still
    // unresolved, which can only mean a cycle (corrupt input).
    uint32_t *d_pending = &ctx->d_mail->ibwt_pending;
    const int steps = static_cast<int>(ceil_log2_u64(nsplit)) + 1;
    for (int it = 0; it < steps; ++it) {
        if (it == steps - 1) DK_TRY(ctx->mail_fill(d_pending, 0));
        {
            LaunchScope ls(ctx, K_IBWT_JUMP, 24.0 * nsplit);
            k_ibwt_jump<<<dim3(div_up(nsplit, 256)), dim3(256), 0, st>>>(nxt, acc, nxt_alt, acc_alt, nsplit, d_pending);
        }
        std::swap(nxt, nxt_alt);
        std::swap(acc, acc_alt);
    }
    DK_HIP(ctx, hipGetLastError());
    DK_TRY(ctx->mail_read(&ctx->h_mail->ibwt_pending));
    if (ctx->h_mail->ibwt_pending != 0) return ctx->fail(DK_E_STREAM, "bwt_inverse: successor table has a cycle (corrupt input)");
    uint32_t *d_bad = &ctx->d_mail->ibwt_bad;
    DK_TRY(ctx->mail_fill(d_bad, 0));
    {
        LaunchScope ls(ctx, K_IBWT_EMIT, (record ? 2.0 : 6.0) * n);
        if (record)
            k_ibwt_copy<<<dim3(div_up(nsplit, 256)), dim3(256), 0, st>>>(psi, static_cast<uint32_t>(n), origin, S, nreg, nsplit, acc, len_keep, rec, resume,
                                                                          d_out, d_bad);
        else
            k_ibwt_emit<<<dim3(div_up(nsplit, 256)), dim3(256), 0, st>>>(d_bwt, psi, static_cast<uint32_t>(n), origin, S, nreg, nsplit, acc,
                                                                          d_out, d_bad);
    }
    DK_HIP(ctx, hipGetLastError());
    DK_TRY(ctx->mail_read(&ctx->h_mail->ibwt_bad));
    ctx->ws_release(mark);
    if (ctx->h_mail->ibwt_bad) return ctx->fail(DK_E_STREAM, "bwt_inverse: BWT/origin do not describe a single text cycle");
    return DK_OK;
}

int packed_ibwt_device(dk_ctx *ctx, const uint8_t *d_bwt, const std::vector<uint32_t> &off, const uint32_t *origin, uint8_t *d_out) {
    hipStream_t st = ctx->stream;
    const size_t count = off.size() - 1, total = off.back();
    const uint32_t cnt = static_cast<uint32_t>(count), T = static_cast<uint32_t>(total);
    const size_t mark = ctx->ws_mark();
    // S = 64 as for large single blocks: a pack is one large walk problem whatever its block size
    constexpr uint32_t S = 64;
    // one upload: off (count + 1) | origin (count) | first splitter of every block (count + 1, the last = all splitters)
    std::vector<uint32_t> aux(3 * count + 2);
    std::copy(off.begin(), off.end(), aux.begin());
    uint32_t *h_org = aux.data() + count + 1, *h_sb = h_org + count;
    uint32_t nsplit = 0, max_split = 1;
    for (size_t i = 0; i < count; ++i) {
        h_org[i] = origin[i];
        h_sb[i] = nsplit;
        const uint32_t k = static_cast<uint32_t>(div_up(off[i + 1] - off[i], S)) + (origin[i] % S ? 1u : 0u);
        max_split = std::max(max_split, k);
        nsplit += k;
    }
    h_sb[count] = nsplit;
    const size_t ntiles = div_up(total, IB_TILE);
    const size_t tpc = div_up(ntiles, IB_MAX_CHUNKS);
    const size_t nchunks = div_up(ntiles, tpc);
    // records of the walk (IB_REC bytes per splitter) where the splitters are sparse enough that they cost at most 8 bytes per position: packs of
    // blocks that average 2 KiB or more.  Packs of tiny blocks have walks of a few steps and take k_pib_emit.
    const bool record = DK_KNOB("DK_IBWT_RECORD", 1) != 0 && static_cast<size_t>(nsplit) * 32 <= total;
    uint32_t *d_aux = ctx->ws_alloc<uint32_t>(aux.size());
    uint32_t *tile_hist = ctx->ws_alloc<uint32_t>(ntiles * 256);
    uint32_t *chunk_sum = ctx->ws_alloc<uint32_t>(nchunks * 256);
    uint32_t *class_start = ctx->ws_alloc<uint32_t>(256);
    uint32_t *base = ctx->ws_alloc<uint32_t>(count * 256);
    uint32_t *cls0 = ctx->ws_alloc<uint32_t>(count);
    uint64_t *psi = ctx->ws_alloc<uint64_t>(total);
    uint32_t *nxt = ctx->ws_alloc<uint32_t>(nsplit), *nxt_alt = ctx->ws_alloc<uint32_t>(nsplit);
    uint32_t *acc = ctx->ws_alloc<uint32_t>(nsplit), *acc_alt = ctx->ws_alloc<uint32_t>(nsplit);
    if (!d_aux || !tile_hist || !chunk_sum || !class_start || !base || !cls0 || !psi || !nxt || !nxt_alt || !acc || !acc_alt) return DK_E_NOMEM;
    uint32_t *len_keep = record ? ctx->ws_alloc<uint32_t>(nsplit) : nullptr;
    uint32_t *resume = record ? ctx->ws_alloc<uint32_t>(nsplit) : nullptr;
    uint8_t *rec = record ? ctx->ws_alloc<uint8_t>(static_cast<size_t>(nsplit) * IB_REC) : nullptr;
    if (record && (!len_keep || !resume || !rec)) return DK_E_NOMEM;
    const uint32_t *d_off = d_aux, *d_org = d_aux + count + 1, *d_sb = d_org + count;
    DK_HIP(ctx, hipMemcpyAsync(d_aux, aux.data(), aux.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    {
        LaunchScope ls(ctx, K_IBWT_HIST, 1.0 * total + 2048.0 * count);
        k_ibwt_hist<<<dim3(ntiles), dim3(IB_BLOCK), 0, st>>>(d_bwt, total, tile_hist);
        k_ibwt_scan_a<<<dim3(nchunks), dim3(256), 0, st>>>(tile_hist, ntiles, tpc, chunk_sum);
        k_ibwt_scan_b<<<dim3(1), dim3(256), 0, st>>>(chunk_sum, nchunks, class_start);
        k_ibwt_scan_c<<<dim3(nchunks), dim3(256), 0, st>>>(tile_hist, ntiles, tpc, chunk_sum);
        k_pib_heads<<<dim3(cnt), dim3(256), 0, st>>>(d_bwt, d_off, d_org, static_cast<uint32_t>(ntiles), tile_hist, base, cls0);
    }
    {
        LaunchScope ls(ctx, K_IBWT_LF, 5.0 * total);
        k_pib_lf<<<dim3(ntiles), dim3(IB_BLOCK), 0, st>>>(d_bwt, T, d_off, cnt, d_org, tile_hist, base, cls0, psi);
    }
    DK_HIP(ctx, hipGetLastError());
    const unsigned sgrid = static_cast<unsigned>(div_up(nsplit, 256));
    {
        LaunchScope ls(ctx, K_IBWT_WALK, (record ? 5.0 : 4.0) * total);
        k_pib_walk<<<dim3(sgrid), dim3(256), 0, st>>>(psi, d_off, d_org, d_sb, cnt, S, nsplit, nxt, acc, len_keep, rec, resume);
    }
    DK_HIP(ctx, hipGetLastError());
    // every chain lies inside one block: the longest block's splitter count decides the number of jumps
    uint32_t *d_pending = &ctx->d_mail->packed.ibwt_pending, *d_bad = &ctx->d_mail->packed.ibwt_bad;
    const uint32_t &bad = ctx->h_mail->packed.ibwt_bad;  // (valid behind every mail_read below)
    const int steps = static_cast<int>(ceil_log2_u64(max_split)) + 1;
    for (int it = 0; it < steps; ++it) {
        {
            LaunchScope ls(ctx, K_IBWT_JUMP, 24.0 * nsplit);
            k_ibwt_jump<<<dim3(sgrid), dim3(256), 0, st>>>(nxt, acc, nxt_alt, acc_alt, nsplit, d_pending);
        }
        std::swap(nxt, nxt_alt);
        std::swap(acc, acc_alt);
    }
    DK_TRY(ctx->mail_fill(d_bad, 0xFF));
    {
        LaunchScope ls(ctx, K_IBWT_JUMP, 12.0 * nsplit);
        k_pib_check<<<dim3(sgrid), dim3(256), 0, st>>>(d_off, d_org, d_sb, cnt, S, nsplit, nxt, acc, len_keep, d_bad);
    }
    DK_HIP(ctx, hipGetLastError());
    DK_TRY(ctx->mail_read(&ctx->h_mail->packed.ibwt_bad));
    // nothing has been written to d_out yet: a corrupt block fails the whole call and leaves the output as it was
    if (bad != IB_END) return ctx->fail(DK_E_STREAM, "bwt_inverse_packed: block %u of the pack: BWT/origin do not describe a single text cycle", bad);
    {
        LaunchScope ls(ctx, K_IBWT_EMIT, (record ? 2.0 : 6.0) * total);
        if (record)
            k_pib_copy<<<dim3(sgrid), dim3(256), 0, st>>>(psi, d_off, d_org, d_sb, cnt, S, nsplit, acc, len_keep, rec, resume, d_out, d_bad);
        else
            k_pib_emit<<<dim3(sgrid), dim3(256), 0, st>>>(psi, d_off, d_org, d_sb, cnt, S, nsplit, acc, d_out, d_bad);
    }
    DK_HIP(ctx, hipGetLastError());
    DK_TRY(ctx->mail_read(&ctx->h_mail->packed.ibwt_bad));
    ctx->ws_release(mark);
    if (bad != IB_END) return ctx->fail(DK_E_STREAM, "bwt_inverse_packed: block %u of the pack: BWT/origin do not describe a single text cycle", bad);
    return DK_OK;
}

// The front part of both FM-index structure builds: packed_ibwt_device's table, walk (no records), jumps and check.  A single block is a pack of
// one here (S = 64 at every size): the workspace is the packed inverse's without its records, which every context that can invert the block or
// pack holds.  Afterwards psi is the successor table, dist[s] the distance of splitter s from its block's end, and every walk from a splitter
// stays in its block.  Synchronises; DK_E_STREAM in the words of `what` for a block that is no BWT (the workspace is then released to `mark`).
namespace {
constexpr uint32_t FMB_S = 64;
struct FmWalks { const uint64_t *psi; const uint32_t *off, *org, *sb, *dist; uint32_t nsplit; unsigned sgrid; };
int fm_walks_device(dk_ctx *ctx, const uint8_t *d_bwt, const std::vector<uint32_t> &off, const uint32_t *origin, const char *what, bool packed,
                    size_t mark, FmWalks &out) {
    hipStream_t st = ctx->stream;
    const size_t count = off.size() - 1, total = off.back();
    const uint32_t cnt = static_cast<uint32_t>(count), T = static_cast<uint32_t>(total);
    constexpr uint32_t S = FMB_S;
    std::vector<uint32_t> aux(3 * count + 2);  // off | origin | first splitter of every block, as in packed_ibwt_device
    std::copy(off.begin(), off.end(), aux.begin());
    uint32_t *h_org = aux.data() + count + 1, *h_sb = h_org + count;
    uint32_t nsplit = 0, max_split = 1;
    for (size_t i = 0; i < count; ++i) {
        h_org[i] = origin[i];
        h_sb[i] = nsplit;
        const uint32_t k = static_cast<uint32_t>(div_up(off[i + 1] - off[i], S)) + (origin[i] % S ? 1u : 0u);
        max_split = std::max(max_split, k);
        nsplit += k;
    }
    h_sb[count] = nsplit;
    const size_t ntiles = div_up(total, IB_TILE), tpc = div_up(ntiles, IB_MAX_CHUNKS), nchunks = div_up(ntiles, tpc);
    uint32_t *d_aux = ctx->ws_alloc<uint32_t>(aux.size());
    uint32_t *tile_hist = ctx->ws_alloc<uint32_t>(ntiles * 256);
    uint32_t *chunk_sum = ctx->ws_alloc<uint32_t>(nchunks * 256);
    uint32_t *class_start = ctx->ws_alloc<uint32_t>(256);
    uint32_t *base = ctx->ws_alloc<uint32_t>(count * 256);
    uint32_t *cls0 = ctx->ws_alloc<uint32_t>(count);
    uint64_t *psi = ctx->ws_alloc<uint64_t>(total);
    uint32_t *nxt = ctx->ws_alloc<uint32_t>(nsplit), *nxt_alt = ctx->ws_alloc<uint32_t>(nsplit);
    uint32_t *acc = ctx->ws_alloc<uint32_t>(nsplit), *acc_alt = ctx->ws_alloc<uint32_t>(nsplit);
    if (!d_aux || !tile_hist || !chunk_sum || !class_start || !base || !cls0 || !psi || !nxt || !nxt_alt || !acc || !acc_alt) return DK_E_NOMEM;
    const uint32_t *d_off = d_aux, *d_org = d_aux + count + 1, *d_sb = d_org + count;
    int rc = ctx->hip_ok(hipMemcpyAsync(d_aux, aux.data(), aux.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st), "pack geometry");
    const unsigned sgrid = static_cast<unsigned>(div_up(nsplit, 256));
    uint32_t *d_bad = &ctx->d_mail->packed.ibwt_bad;
    if (rc == DK_OK) {
        {
            LaunchScope ls(ctx, K_IBWT_HIST, 1.0 * total + 2048.0 * count);
            k_ibwt_hist<<<dim3(ntiles), dim3(IB_BLOCK), 0, st>>>(d_bwt, total, tile_hist);
            k_ibwt_scan_a<<<dim3(nchunks), dim3(256), 0, st>>>(tile_hist, ntiles, tpc, chunk_sum);
            k_ibwt_scan_b<<<dim3(1), dim3(256), 0, st>>>(chunk_sum, nchunks, class_start);
            k_ibwt_scan_c<<<dim3(nchunks), dim3(256), 0, st>>>(tile_hist, ntiles, tpc, chunk_sum);
            k_pib_heads<<<dim3(cnt), dim3(256), 0, st>>>(d_bwt, d_off, d_org, static_cast<uint32_t>(ntiles), tile_hist, base, cls0);
        }
        {
            LaunchScope ls(ctx, K_IBWT_LF, 5.0 * total);
            k_pib_lf<<<dim3(ntiles), dim3(IB_BLOCK), 0, st>>>(d_bwt, T, d_off, cnt, d_org, tile_hist, base, cls0, psi);
        }
        {
            LaunchScope ls(ctx, K_IBWT_WALK, 4.0 * total);
            k_pib_walk<<<dim3(sgrid), dim3(256), 0, st>>>(psi, d_off, d_org, d_sb, cnt, S, nsplit, nxt, acc, nullptr, nullptr, nullptr);
        }
        const int steps = static_cast<int>(ceil_log2_u64(max_split)) + 1;
        for (int it = 0; it < steps; ++it) {
            {
                LaunchScope ls(ctx, K_IBWT_JUMP, 24.0 * nsplit);
                k_ibwt_jump<<<dim3(sgrid), dim3(256), 0, st>>>(nxt, acc, nxt_alt, acc_alt, nsplit, &ctx->d_mail->packed.ibwt_pending);
            }
            std::swap(nxt, nxt_alt);
            std::swap(acc, acc_alt);
        }
        rc = ctx->mail_fill(d_bad, 0xFF);
    }
    if (rc == DK_OK) {
        LaunchScope ls(ctx, K_IBWT_JUMP, 12.0 * nsplit);
        k_pib_check<<<dim3(sgrid), dim3(256), 0, st>>>(d_off, d_org, d_sb, cnt, S, nsplit, nxt, acc, nullptr, d_bad);
    }
    if (rc == DK_OK) rc = ctx->hip_ok(hipGetLastError(), what);
    const hipError_t e = hipStreamSynchronize(st);  // (also on failure: the copy above reads `aux`)
    DK_TRY(rc);
    DK_HIP(ctx, e);
    DK_TRY(ctx->mail_read(&ctx->h_mail->packed.ibwt_bad));
    const uint32_t bad = ctx->h_mail->packed.ibwt_bad;
    if (bad != IB_END) {
        ctx->ws_release(mark);
        if (packed) return ctx->fail(DK_E_STREAM, "%s_packed: block %u of the pack: BWT/origin do not describe a single text cycle", what, bad);
        return ctx->fail(DK_E_STREAM, "%s: BWT/origin do not describe a single text cycle", what);
    }
    out = FmWalks{psi, d_off, d_org, d_sb, acc, nsplit, sgrid};
    return DK_OK;
}
}  // namespace

// The locate structure: the front part above, then k_pib_locate twice where the inverse writes the text.
int fm_locate_build_device(dk_ctx *ctx, const uint8_t *d_bwt, const std::vector<uint32_t> &off, const uint32_t *origin, uint32_t step, void *d_loc,
                           bool packed) {
    hipStream_t st = ctx->stream;
    const size_t count = off.size() - 1, total = off.back();
    const uint32_t cnt = static_cast<uint32_t>(count), T = static_cast<uint32_t>(total);
    const FmLocate lc = fm_locate_carve(d_loc, total, count, step);
    const size_t mark = ctx->ws_mark();
    const uint32_t header[6] = {FM_LOC_MAGIC, T, cnt, step, static_cast<uint32_t>(lc.rows), static_cast<uint32_t>(lc.nsamp)};
    // the header, the marks and the mark bits start as zeros (the samples are written one by one)
    DK_HIP(ctx, hipMemsetAsync(d_loc, 0, (FM_LOC_HEADER + 33 * lc.rows + 1) * sizeof(uint32_t), st));
    {
        const hipError_t e = hipMemcpyAsync(d_loc, header, sizeof(header), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st);
            DK_HIP(ctx, e);
        }
    }
    FmWalks w;
    {
        const int rc = fm_walks_device(ctx, d_bwt, off, origin, "fm_locate_build", packed, mark, w);
        if (rc == DK_E_NOMEM) (void)hipStreamSynchronize(st);  // (every other return has synchronised: the copy above reads `header`)
        DK_TRY(rc);
    }
    const uint32_t shift = static_cast<uint32_t>(ceil_log2_u64(step)), R = static_cast<uint32_t>(lc.rows), NS = static_cast<uint32_t>(lc.nsamp);
    {
        // both walks: a successor entry per position (a random 64-byte line each); the marks' words, the samples
        LaunchScope ls(ctx, K_IBWT_EMIT, 2.0 * 64.0 * total + total / 4.0 + 8.0 * (total >> shift));
        k_pib_locate<false><<<dim3(w.sgrid), dim3(256), 0, st>>>(w.psi, w.off, w.org, w.sb, cnt, FMB_S, w.nsplit, w.dist, shift, lc.bits, lc.marks, lc.samples, NS);
        k_loc_rows<<<dim3(static_cast<unsigned>(div_up(lc.rows, 256))), dim3(256), 0, st>>>(lc.bits, R, lc.marks);
        k_loc_scan<<<dim3(1), dim3(1024), 0, st>>>(lc.marks, R);
        k_pib_locate<true><<<dim3(w.sgrid), dim3(256), 0, st>>>(w.psi, w.off, w.org, w.sb, cnt, FMB_S, w.nsplit, w.dist, shift, lc.bits, lc.marks, lc.samples, NS);
    }
    DK_HIP(ctx, hipGetLastError());
    DK_HIP(ctx, hipStreamSynchronize(st));
    ctx->ws_release(mark);
    return DK_OK;
}

// The extract structure: the same front part, then one walk that stores the slot it stands on at every position that is a multiple of the step.
int fm_extract_build_device(dk_ctx *ctx, const uint8_t *d_bwt, const std::vector<uint32_t> &off, const uint32_t *origin, uint32_t step, void *d_ext,
                            bool packed) {
    hipStream_t st = ctx->stream;
    const size_t count = off.size() - 1, total = off.back();
    const uint32_t cnt = static_cast<uint32_t>(count);
    const std::vector<uint32_t> abase = fm_extract_bases(off, step);
    uint32_t *anchors = static_cast<uint32_t *>(d_ext) + FM_EXT_HEADER;
    const size_t mark = ctx->ws_mark();
    uint32_t *d_abase = ctx->ws_alloc<uint32_t>(count + 1);
    if (!d_abase) return DK_E_NOMEM;
    FmWalks w;
    DK_TRY(fm_walks_device(ctx, d_bwt, off, origin, "fm_extract_build", packed, mark, w));
    const uint32_t header[5] = {FM_EXT_MAGIC, static_cast<uint32_t>(total), cnt, step, abase.back()};
    const uint32_t shift = static_cast<uint32_t>(ceil_log2_u64(step));
    int rc = ctx->hip_ok(hipMemsetAsync(d_ext, 0, FM_EXT_HEADER * sizeof(uint32_t), st), "extract header");
    if (rc == DK_OK) rc = ctx->hip_ok(hipMemcpyAsync(d_ext, header, sizeof(header), hipMemcpyHostToDevice, st), "extract header");
    if (rc == DK_OK) rc = ctx->hip_ok(hipMemcpyAsync(d_abase, abase.data(), abase.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st), "anchor bases");
    if (rc == DK_OK) {
        // a successor entry per position (a random 64-byte line each); the anchors
        LaunchScope ls(ctx, K_IBWT_EMIT, 64.0 * total + 4.0 * abase.back());
        k_pib_anchors<<<dim3(w.sgrid), dim3(256), 0, st>>>(w.psi, w.off, w.org, w.sb, cnt, FMB_S, w.nsplit, w.dist, shift, d_abase, anchors, abase.back());
        rc = ctx->hip_ok(hipGetLastError(), "fm extract build");
    }
    const hipError_t e = hipStreamSynchronize(st);  // (also on failure: the copies above read `header` and `abase`)
    DK_TRY(rc);
    DK_HIP(ctx, e);
    ctx->ws_release(mark);
    return DK_OK;
}

// ---- what the two inverses above take from the workspace (a decoder context is sized by these: abi.cpp decoder_workspace_bytes) ----------
namespace {
// tile histograms, chunk sums, class starts and the successor table of `total` positions.  The chunk count itself is not monotone in the tile
// count (257 tiles make 129 chunks, 256 tiles 256): min(tiles, IB_MAX_CHUNKS) bounds it and is.
size_t ibwt_tables(size_t total) {
    const size_t ntiles = div_up(total, IB_TILE);
    return ws_round(ntiles * 256 * 4) + ws_round(std::min<size_t>(ntiles, IB_MAX_CHUNKS) * 256 * 4) + ws_round(256 * 4) + ws_round(total * 8);
}
size_t ibwt_records(size_t nsplit) { return 2 * ws_round(nsplit * 4) + ws_round(nsplit * IB_REC); }  // len_keep, resume, rec
}  // namespace

size_t bwt_inverse_workspace(size_t max_n) {
    // blocks below 2^16: S = 8, four splitter arrays, no records; from 2^16: S = 64, four splitter arrays + records.  One more splitter for an
    // origin off the grid in both.  A context for max_n serves every smaller block, so both forms count, each at its largest block.
    const size_t small_n = std::min<size_t>(max_n, (1u << 16) - 1);
    size_t bytes = ibwt_tables(small_n) + 4 * ws_round((div_up(small_n, 8) + 1) * 4);
    if (max_n >= (1u << 16)) {
        const size_t nsplit = div_up(max_n, 64) + 1;
        bytes = std::max(bytes, ibwt_tables(max_n) + 4 * ws_round(nsplit * 4) + ibwt_records(nsplit));
    }
    return bytes;
}

size_t packed_ibwt_workspace(size_t max_total, size_t max_blocks) {
    // Every block holds at least one byte: count <= total.  A block of n_i bytes has ceil(n_i / 64) splitters and one more for an origin off
    // the grid (only where n_i > 1): at most n_i of them, and at most n_i / 64 + 2.  Records are taken only when nsplit * 32 <= total.
    const size_t count = std::min(max_blocks, max_total);
    const size_t nsplit = std::min(max_total, max_total / 64 + 2 * count);
    const size_t nrec = std::min(nsplit, max_total / 32);
    return ws_round((3 * count + 2) * 4) /* aux */ + ibwt_tables(max_total) + ws_round(count * 256 * 4) /* base */ + ws_round(count * 4) /* cls0 */ +
           4 * ws_round(nsplit * 4) + ibwt_records(nrec);
}

size_t fm_locate_build_workspace(size_t total, size_t count) {
    // fm_locate_build_device: the packed inverse's buffers without its records, for this very pack
    const size_t nsplit = std::min(total, total / 64 + 2 * count);
    return ws_round((3 * count + 2) * 4) + ibwt_tables(total) + ws_round(count * 256 * 4) + ws_round(count * 4) + 4 * ws_round(nsplit * 4);
}

}  // namespace dk
