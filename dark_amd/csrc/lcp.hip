// Longest-common-prefix arrays from a text and its suffix array, for one block or a pack: the Phi algorithm with
// irreducible positions (Kärkkäinen, Manzini, Puglisi, CPM 2009).  LCP[i] = number of leading bytes the suffixes SA[i-1] and SA[i] share,
// LCP[0] = 0, no sentinel (src/saca.rs:105-113): a common prefix ends where the shorter suffix ends.
//
// Conventions are those of packed.hip: block b is text[off_b, e_b), its suffix array sits at sa[off_b, e_b) with entries local to the block, and
// a single block is a pack of one.  Positions below are global (off_b + local).  PLCP[p] = LCP of suffix p with the suffix in front of it in the
// suffix array, Phi[p]; one array of one word per position holds first Phi, then PLCP, in place:
//   k_lcp_phi      a thread per slot: phi[off_b + SA[i]] = off_b + SA[i-1]; the block's first slot stores the finished answer MARK | 0.  Checks
//                  every entry against its block's length (Mail::Lcp::bad_sa).
//   k_lcp_measure  a thread per position p, q = phi[p].  p is REDUCIBLE when it is not its block's first position, q is not either and
//                  T[p-1] == T[q-1]: then PLCP[p] = PLCP[p-1] - 1 and nothing is measured.  Otherwise the lane compares T[p..] with T[q..], 16 bytes
//                  a step, up to the block's end or lane_cap bytes, and stores MARK | length -- bit 31 says "measured" (n <= 2^31 - 2).
//   k_lcp_wave     what was still equal at lane_cap is listed; a wave per listed position goes on at 64 x 16 bytes a step up to wave_cap ...
//   k_lcp_giant    ... and what is still equal then is measured by the whole grid, 4 KiB per workgroup and step, first difference by atomicMin
//                  straight into phi[p] (as k_lf_lce does for the L-first path).  No lane and no wave walks a long repeat alone.
//   a full list    leaves the position as it was (phi[p] = q); lcp_device runs measure / wave / giant again, and only such positions do
//                  anything then.  Every pass settles at least one listed position, so the attempts counted by the first pass bound the loop.
//   k_lcp_tile_sum / k_lcp_spine / k_lcp_fill   "last marked position" max-scan over tiles of 4096 positions (the pattern of k_pk_tile_sum /
//                  k_pk_spine / k_pk_tile_apply): a reducible p takes PLCP[p0] - (p - p0) from the nearest measured p0 <= p.  A block's first
//                  position is always measured, so p0 lies in p's block.
//   k_lcp_gather   a thread per slot: LCP[i] = PLCP[off_b + SA[i]].
// Word states of phi: bit 31 set = measured (value in the low 31 bits; OPEN = all ones while a wave or the grid works on it); REDUCIBLE
// (0x7FFFFFFF, no position: q <= 2^31 - 3); anything else = q, not settled yet.
// Containment for an sa that is in range but no suffix array: every q is checked against its block before the text is read at it, every
// compare stops at e_b - max(p, q), every subtraction saturates, and phi starts as MARK | 0 everywhere: the values are unspecified but <= n_b.
#include <algorithm>

#include "context.hpp"
#include "device_util.hpp"

namespace dk {
namespace {

constexpr uint32_t LCP_MARK = 0x80000000u, LCP_VALUE = 0x7FFFFFFFu, LCP_REDUCIBLE = 0x7FFFFFFFu, LCP_OPEN = 0xFFFFFFFFu;
// The caps.  A lane's loop costs its whole wave as many steps as its longest member takes: 256 bytes = 16 steps bounds that
// while irreducible values of text (mean of some tens of bytes) end inside it.  A wave reads 1 KiB a step; at 64 KiB = 64 steps the grid
// takes over -- the threshold at which the L-first path hands a common extension to k_lf_lce.
constexpr int LCP_LANE_CAP = 256;
constexpr int LCP_WAVE_CAP = 65536;
constexpr int LCP_BLOCK = 256, LCP_IPT = 16, LCP_TILE = LCP_BLOCK * LCP_IPT;
constexpr uint32_t LCP_GIANT_CHUNK = 16 * LCP_BLOCK;  // bytes a workgroup of k_lcp_giant compares per step
constexpr uint32_t LCP_GIANT_MAX = 65536;             // entries of the giant list at most
// While profiling the kernels count what they measure: LCP_COUNTERS pairs (bytes compared, positions measured) in the workspace, a workgroup
// adds to the pair of its index -- one pair for all would put every wave's atomic on one address (24 ms for a 64 MiB pack; 2.8 ms without).
constexpr uint32_t LCP_COUNTERS = 256;
__device__ __forceinline__ void lcp_count(unsigned long long *__restrict__ cnt, unsigned long long compared, unsigned long long measured) {
    unsigned long long *c = cnt + 2u * (blockIdx.x & (LCP_COUNTERS - 1u));
    if (compared) atomicAdd(c, compared);
    if (measured) atomicAdd(c + 1, measured);
}

struct LcpLong { uint32_t p, q; };
struct LcpGiant { uint32_t p, q, done, end; };  // done: bytes known to be equal; end: e_b

typedef uint64_t __attribute__((aligned(1))) unaligned_u64;
typedef const unaligned_u64 __attribute__((address_space(1))) *gptr8;

// bytes T[x + k] == T[y + k] for k = 0, 1, ... below min(16, lim); the caller guarantees x + lim and y + lim do not pass the block's end
__device__ __forceinline__ uint32_t lce16(const uint8_t *__restrict__ t, size_t x, size_t y, size_t lim) {
    if (lim >= 16) {
        const uint64_t lo = *(gptr8)(t + x) ^ *(gptr8)(t + y);
        if (lo) return static_cast<uint32_t>(__builtin_ctzll(lo)) >> 3;
        const uint64_t hi = *(gptr8)(t + x + 8) ^ *(gptr8)(t + y + 8);
        return hi ? 8u + (static_cast<uint32_t>(__builtin_ctzll(hi)) >> 3) : 16u;
    }
    uint32_t k = 0;
    while (k < lim && t[x + k] == t[y + k]) ++k;
    return k;
}

// slots [lo, hi) of the pack (all of it, or the stretch of one block)
__global__ __launch_bounds__(256) void k_lcp_phi(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ off, uint32_t count, uint32_t lo, uint32_t hi,
                                                 uint32_t *__restrict__ phi, Mail::Lcp *__restrict__ mail) {
    const uint32_t i = lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hi) return;
    const uint32_t b = seg_of(off, count, i), s = off[b], len = off[b + 1] - s;
    const uint32_t v = sa[i];
    if (v >= len) { mail->bad_sa = 1u; return; }
    if (i == s) { phi[s + v] = LCP_MARK; return; }  // no suffix in front of the block's first: PLCP = 0, settled
    const uint32_t u = sa[i - 1];
    if (u >= len) return;  // its own thread reports it
    phi[s + v] = s + u;
}

// The same from the inverse suffix array the packed sort ends with (rank[p] = the slot of suffix p, packed.hip): a thread per position, the
// suffix in front read from the suffix array k_pk_emit has just written.  A block that left the pack for the guard has no final ranks and
// nothing valid in its stretch of sa: whatever is out of range becomes MARK | 0, and lcp_phi_block_device redoes the stretch afterwards.
__global__ __launch_bounds__(256) void k_lcp_phi_rank(const uint32_t *__restrict__ rank, const uint32_t *__restrict__ sa, const uint32_t *__restrict__ off,
                                                      uint32_t count, uint32_t total, uint32_t *__restrict__ phi) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    const uint32_t b = seg_of(off, count, p), s = off[b], e = off[b + 1];
    const uint32_t r = rank[p];
    uint32_t x = LCP_MARK;
    if (r > s && r < e) {
        const uint32_t u = sa[r - 1];
        if (u < e - s) x = s + u;
    }
    phi[p] = x;
}

__global__ __launch_bounds__(256) void k_lcp_measure(const uint8_t *__restrict__ t, const uint32_t *__restrict__ off, uint32_t count, uint32_t total,
                                                     uint32_t *__restrict__ phi, uint32_t lane_cap, LcpLong *__restrict__ list, uint32_t list_cap,
                                                     Mail::Lcp *__restrict__ mail, unsigned long long *__restrict__ cnt) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t compared = 0, measured = 0;
    const uint32_t x = p < total ? phi[p] : LCP_MARK;
    if (x < LCP_REDUCIBLE) {  // a position: not settled yet
        const uint32_t b = seg_of(off, count, p), s = off[b], e = off[b + 1], q = x;
        if (q < s || q >= e) {
            phi[p] = LCP_MARK;  // (never from k_lcp_phi)
        } else if (p > s && q > s && t[p - 1] == t[q - 1]) {
            phi[p] = LCP_REDUCIBLE;
        } else {
            const uint32_t room = e - (p > q ? p : q), lim = room < lane_cap ? room : lane_cap;
            uint32_t l = 0;
            while (l < lim) {
                const uint32_t d = lce16(t, static_cast<size_t>(p) + l, static_cast<size_t>(q) + l, lim - l);
                l += d;
                if (d < 16) break;
            }
            compared = l;
            if (l == lane_cap && room > lane_cap) {  // still equal at the cap: a wave goes on
                const uint32_t k = atomicAdd(&mail->lists.long_count, 1u);
                if (k < list_cap) {
                    list[k] = LcpLong{p, q};
                    phi[p] = LCP_OPEN;
                }  // a full list: phi[p] stays q and the next pass takes it
            } else {
                phi[p] = LCP_MARK | l;
                measured = 1;
            }
        }
    }
    if (cnt) {
        compared = wave_sum(compared);
        measured = wave_sum(measured);
        if ((threadIdx.x & 63) == 0) lcp_count(cnt, compared, measured);
    }
}

// a wave per listed position, the list walked with a grid stride (the count is on the device only)
__global__ __launch_bounds__(256) void k_lcp_wave(const uint8_t *__restrict__ t, const uint32_t *__restrict__ off, uint32_t count, uint32_t *__restrict__ phi,
                                                  const LcpLong *__restrict__ list, uint32_t list_cap, uint32_t lane_cap, uint32_t wave_cap,
                                                  LcpGiant *__restrict__ giant, uint32_t giant_cap, Mail::Lcp *__restrict__ mail,
                                                  unsigned long long *__restrict__ cnt) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t listed = mail->lists.long_count < list_cap ? mail->lists.long_count : list_cap;
    const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t g = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; g < listed; g += nwaves) {
        const LcpLong en = list[g];
        const uint32_t e = off[seg_of(off, count, en.p) + 1];
        const uint32_t room = e - (en.p > en.q ? en.p : en.q), lim = room < wave_cap ? room : wave_cap;
        uint32_t l = lane_cap;  // the lane found this much equal (lane_cap < room, lane_cap <= wave_cap)
        bool differs = false;
        while (l < lim) {
            const uint32_t o = l + 16u * lane;
            uint32_t d = 16;
            bool diff = false;
            if (o < lim) {
                const uint32_t left = lim - o;
                d = lce16(t, static_cast<size_t>(en.p) + o, static_cast<size_t>(en.q) + o, left);
                diff = d < (left < 16u ? left : 16u);
            }
            const uint64_t m = __ballot(diff);
            if (m) {
                const int first = __ffsll(static_cast<unsigned long long>(m)) - 1;
                l += 16u * static_cast<uint32_t>(first) + static_cast<uint32_t>(__shfl(static_cast<int>(d), first, kWave));
                differs = true;
                break;
            }
            l = lim - l > 64u * 16u ? l + 64u * 16u : lim;
        }
        if (lane == 0) {
            const bool settled = differs || room <= wave_cap;
            if (cnt) lcp_count(cnt, l - lane_cap, settled ? 1u : 0u);
            if (settled) {
                phi[en.p] = LCP_MARK | l;  // (no difference: l == lim == room)
            } else {  // still equal at the cap: the grid goes on
                const uint32_t k = atomicAdd(&mail->lists.giant_count, 1u);
                if (k < giant_cap) giant[k] = LcpGiant{en.p, en.q, l, e};  // phi[p] stays OPEN: k_lcp_giant's atomicMin starts from it
                else phi[en.p] = en.q;                                     // a full list: back to "not settled", the next pass takes it
            }
        }
    }
}

// The listed pairs one after another, every one by the whole grid: the workgroups take the 4 KiB chunks behind `done` in turn and stop at the
// first chunk behind the best answer so far.  phi[p] is OPEN = MARK | 0x7FFFFFFF on entry and takes MARK | length by atomicMin.
__global__ __launch_bounds__(LCP_BLOCK) void k_lcp_giant(const uint8_t *__restrict__ t, uint32_t *__restrict__ phi, const LcpGiant *__restrict__ giant,
                                                         uint32_t listed, unsigned long long *__restrict__ cnt) {
    __shared__ uint32_t s_mis, s_best;
    const uint32_t tid = threadIdx.x;
    for (uint32_t g = 0; g < listed; ++g) {
        const LcpGiant en = giant[g];
        const uint32_t room = en.end - (en.p > en.q ? en.p : en.q);
        uint32_t *r = phi + en.p;
        for (size_t chunk = blockIdx.x;; chunk += gridDim.x) {
            const size_t o0 = en.done + chunk * LCP_GIANT_CHUNK;
            __syncthreads();
            if (tid == 0) { s_best = __atomic_load_n(r, __ATOMIC_RELAXED) & LCP_VALUE; s_mis = 0xFFFFFFFFu; }
            __syncthreads();
            if (o0 >= room) { if (tid == 0) atomicMin(r, LCP_MARK | room); break; }  // no difference up to the end of the shorter suffix
            if (o0 >= s_best) break;  // another workgroup has found a difference in front of this chunk
            const size_t o = o0 + 16u * tid;
            if (o < room) {
                const size_t left = room - o;
                const uint32_t d = lce16(t, en.p + o, en.q + o, left);
                if (d < (left < 16 ? left : 16)) atomicMin(&s_mis, 16u * tid + d);
            }
            if (cnt && tid == 0) lcp_count(cnt, room - o0 < LCP_GIANT_CHUNK ? room - o0 : LCP_GIANT_CHUNK, 0u);
            __syncthreads();
            const uint32_t found = s_mis;
            if (found != 0xFFFFFFFFu) { if (tid == 0) atomicMin(r, LCP_MARK | static_cast<uint32_t>(o0 + found)); break; }
        }
        __syncthreads();
        if (cnt && blockIdx.x == 0 && tid == 0) lcp_count(cnt, 0u, 1u);
    }
}

// ---- the fill: 1 + the last measured position, max-scanned over the tiles ------------------------------------------------------------------
__device__ __forceinline__ void lcp_load_tile(const uint32_t *__restrict__ phi, uint32_t total, uint32_t i0, uint32_t (&v)[LCP_IPT]) {
    if (i0 + LCP_IPT <= total) {  // phi is a workspace allocation (256-byte aligned) and i0 a multiple of 16: four 16-byte loads
        const uint4 *src = reinterpret_cast<const uint4 *>(phi + i0);
#pragma unroll
        for (int j = 0; j < LCP_IPT / 4; ++j) {
            const uint4 w = src[j];
            v[4 * j] = w.x; v[4 * j + 1] = w.y; v[4 * j + 2] = w.z; v[4 * j + 3] = w.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < LCP_IPT; ++j) v[j] = i0 + j < total ? phi[i0 + j] : 0u;
    }
}

__global__ __launch_bounds__(LCP_BLOCK) void k_lcp_tile_sum(const uint32_t *__restrict__ phi, uint32_t total, uint32_t *__restrict__ agg) {
    __shared__ uint32_t s_tmp[LCP_BLOCK / 64 + 1];
    const uint32_t i0 = blockIdx.x * LCP_TILE + threadIdx.x * LCP_IPT;
    uint32_t v[LCP_IPT], last = 0;
    lcp_load_tile(phi, total, i0, v);
#pragma unroll
    for (int j = 0; j < LCP_IPT; ++j)
        if (v[j] & LCP_MARK) last = i0 + j + 1;
    uint32_t all = 0;
    (void)block_excl_max<LCP_BLOCK / 64>(last, s_tmp, &all);
    if (threadIdx.x == 0) agg[blockIdx.x] = all;
}

// exclusive max-scan of the tile aggregates in place
__global__ __launch_bounds__(1024) void k_lcp_spine(uint32_t *__restrict__ agg, uint32_t ntiles) {
    __shared__ uint32_t s_tmp[1024 / 64 + 1];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < ntiles; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t x = i < ntiles ? agg[i] : 0u;
        uint32_t all = 0;
        const uint32_t ex = block_excl_max<1024 / 64>(x, s_tmp, &all);
        if (i < ntiles) agg[i] = carry > ex ? carry : ex;
        carry = carry > all ? carry : all;
        __syncthreads();
    }
}

// PLCP of the reducible positions, in place.  Measured words are never changed (a thread of another tile may be reading one as its p0); the
// mark stays on them and k_lcp_gather cuts it off.
__global__ __launch_bounds__(LCP_BLOCK) void k_lcp_fill(uint32_t *__restrict__ phi, uint32_t total, const uint32_t *__restrict__ agg) {
    __shared__ uint32_t s_tmp[LCP_BLOCK / 64 + 1];
    const uint32_t i0 = blockIdx.x * LCP_TILE + threadIdx.x * LCP_IPT;
    uint32_t v[LCP_IPT], last = 0;
    lcp_load_tile(phi, total, i0, v);
#pragma unroll
    for (int j = 0; j < LCP_IPT; ++j)
        if (v[j] & LCP_MARK) last = i0 + j + 1;
    const uint32_t before = block_excl_max<LCP_BLOCK / 64>(last, s_tmp, nullptr), tiles_before = agg[blockIdx.x];
    const uint32_t prev = before > tiles_before ? before : tiles_before;  // 1 + the last measured position in front of i0 (0: none)
    if (i0 >= total) return;
    uint32_t p0 = prev ? prev - 1 : i0, val0 = 0;
    if (prev && !(v[0] & LCP_MARK)) val0 = phi[p0] & LCP_VALUE;
#pragma unroll
    for (int j = 0; j < LCP_IPT; ++j) {
        const uint32_t i = i0 + j;
        if (i >= total) break;
        if (v[j] & LCP_MARK) {
            p0 = i;
            val0 = v[j] & LCP_VALUE;
        } else {
            const uint32_t back = i - p0;
            phi[i] = val0 > back ? val0 - back : 0u;
        }
    }
}

__global__ __launch_bounds__(256) void k_lcp_gather(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ off, uint32_t count, uint32_t total,
                                                    const uint32_t *__restrict__ plcp, uint32_t *__restrict__ lcp) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const uint32_t b = seg_of(off, count, i), s = off[b], len = off[b + 1] - s;
    const uint32_t v = sa[i];
    lcp[i] = (i == s || v >= len) ? 0u : plcp[s + v] & LCP_VALUE;
}

}  // namespace

int lcp_phi_from_rank_device(dk_ctx *ctx, const uint32_t *d_rank, const uint32_t *d_sa, const uint32_t *d_off, size_t count, size_t total, uint32_t *d_phi) {
    LaunchScope ls(ctx, K_BWT_GATHER, 12.0 * total);  // rank 4 n, a gathered SA entry per position, phi 4 n
    k_lcp_phi_rank<<<dim3(static_cast<unsigned>(div_up(total, 256))), dim3(256), 0, ctx->stream>>>(d_rank, d_sa, d_off, static_cast<uint32_t>(count),
                                                                                                 static_cast<uint32_t>(total), d_phi);
    DK_HIP(ctx, hipGetLastError());
    return DK_OK;
}

int lcp_phi_block_device(dk_ctx *ctx, const uint32_t *d_sa, const uint32_t *d_off, size_t count, size_t lo, size_t hi, uint32_t *d_phi) {
    DK_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_phi + lo), static_cast<int>(LCP_MARK), hi - lo, ctx->stream));
    LaunchScope ls(ctx, K_BWT_GATHER, 12.0 * (hi - lo));
    k_lcp_phi<<<dim3(static_cast<unsigned>(div_up(hi - lo, 256))), dim3(256), 0, ctx->stream>>>(d_sa, d_off, static_cast<uint32_t>(count), static_cast<uint32_t>(lo),
                                                                                              static_cast<uint32_t>(hi), d_phi, &ctx->d_mail->lcp);
    DK_HIP(ctx, hipGetLastError());
    return DK_OK;
}

int lcp_device(dk_ctx *ctx, const PackView &text, const uint32_t *d_sa, uint32_t *d_lcp, uint32_t *d_phi_ready) {
    hipStream_t st = ctx->stream;
    const uint8_t *d_text = text.bytes;
    const size_t total = text.total;
    const uint32_t cnt = static_cast<uint32_t>(text.count), T = static_cast<uint32_t>(total);
    const unsigned grid = static_cast<unsigned>(div_up(total, 256)), ntiles = static_cast<unsigned>(div_up(total, LCP_TILE));
    // (tuning build: the caps and the lists' capacity come from the environment -- tests send the same inputs down the other routes with them)
    const uint32_t lane_cap = static_cast<uint32_t>(std::max(16, std::min(1 << 20, DK_KNOB("DK_LCP_LANE_CAP", LCP_LANE_CAP))));
    const uint32_t wave_cap = std::max(lane_cap, static_cast<uint32_t>(std::max(16, std::min(1 << 24, DK_KNOB("DK_LCP_WAVE_CAP", LCP_WAVE_CAP)))));
    const size_t knob_cap = static_cast<size_t>(std::max(1, DK_KNOB("DK_LCP_LIST_CAP", 1 << 30)));
    const size_t mark = ctx->ws_mark();
    uint32_t *phi = d_phi_ready ? d_phi_ready : ctx->ws_alloc<uint32_t>(total), *agg = ctx->ws_alloc<uint32_t>(ntiles);
    if (!phi || !agg) return DK_E_NOMEM;
    // The lists, from what is left.  A listed position has an irreducible value of at least lane_cap; those values sum to at most n log2 n, so
    // total / 8 entries hold them all at the default cap (log2 n < 32) and a valid input never sees a second pass there.
    const size_t left = ctx->ws_size - ctx->ws_used;
    const size_t long_cap = std::min({total / 8 + 4096, left / 2 / sizeof(LcpLong), knob_cap});
    const size_t giant_cap = std::min({static_cast<size_t>(LCP_GIANT_MAX), left / 4 / sizeof(LcpGiant), knob_cap});
    if (!long_cap || !giant_cap) return ctx->fail(DK_E_NOMEM, "no workspace left for the LCP pass's lists");
    LcpLong *d_long = ctx->ws_alloc<LcpLong>(long_cap);
    LcpGiant *d_giant = ctx->ws_alloc<LcpGiant>(giant_cap);
    if (!d_long || !d_giant) return DK_E_NOMEM;
    Mail::Lcp *d_mail = &ctx->d_mail->lcp;
    const Mail::Lcp *h_mail = &ctx->h_mail->lcp;
    unsigned long long *d_cnt = ctx->profiling ? ctx->ws_alloc<unsigned long long>(2 * LCP_COUNTERS) : nullptr;
    if (ctx->profiling && !d_cnt) return DK_E_NOMEM;
    if (d_cnt) DK_HIP(ctx, hipMemsetAsync(d_cnt, 0, 2 * LCP_COUNTERS * sizeof(unsigned long long), st));
    DK_TRY(ctx->mail_fill(d_mail, 0));
    if (!d_phi_ready) {
        DK_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(phi), static_cast<int>(LCP_MARK), total, st));
        LaunchScope ls(ctx, K_BWT_GATHER, 12.0 * total);  // SA 4 n, a scattered 4-byte store per slot, the preset 4 n
        k_lcp_phi<<<dim3(grid), dim3(256), 0, st>>>(d_sa, text.d_off, cnt, 0u, T, phi, d_mail);
    }
    DK_HIP(ctx, hipGetLastError());
    uint32_t passes = 0, route = 0;
    uint64_t limit = 1;
    for (;;) {
        if (passes) DK_TRY(ctx->mail_fill(&d_mail->lists, 0));
        {
            LaunchScope ls(ctx, K_CHAIN, 10.0 * total);  // phi read and written, T[p-1] and a line of text at q
            k_lcp_measure<<<dim3(grid), dim3(256), 0, st>>>(d_text, text.d_off, cnt, T, phi, lane_cap, d_long, static_cast<uint32_t>(long_cap), d_mail, d_cnt);
        }
        {
            LaunchScope ls(ctx, K_CHAIN, 0.0);
            k_lcp_wave<<<dim3(512), dim3(256), 0, st>>>(d_text, text.d_off, cnt, phi, d_long, static_cast<uint32_t>(long_cap), lane_cap, wave_cap, d_giant,
                                                        static_cast<uint32_t>(giant_cap), d_mail, d_cnt);
        }
        DK_HIP(ctx, hipGetLastError());
        DK_TRY(ctx->mail_read(&ctx->h_mail->lcp));
        if (h_mail->bad_sa) {
            ctx->ws_release(mark);
            return ctx->fail(DK_E_ARG, "the suffix array holds an entry outside its block");
        }
        const uint32_t longs = h_mail->lists.long_count, giants = h_mail->lists.giant_count;
        if (longs) route |= DK_ROUTE_LCP_LONG;
        if (giants) {
            route |= DK_ROUTE_LCP_GIANT;
            LaunchScope ls(ctx, K_CHAIN, 0.0);
            k_lcp_giant<<<dim3(1024), dim3(LCP_BLOCK), 0, st>>>(d_text, phi, d_giant, static_cast<uint32_t>(std::min<size_t>(giants, giant_cap)), d_cnt);
        }
        DK_HIP(ctx, hipGetLastError());
        if (!passes++) limit += longs;  // every pass settles at least one of the positions the first pass wanted to list
        if (longs <= long_cap && giants <= giant_cap) break;
        if (passes > limit) {
            DK_HIP(ctx, hipStreamSynchronize(st));  // (k_lcp_giant may still be walking the list that the release below gives away)
            ctx->ws_release(mark);
            return ctx->fail(DK_E_INTERNAL, "the LCP pass's lists did not drain");
        }
    }
    {
        LaunchScope ls(ctx, K_RERANK_REDUCE, 4.0 * total);
        k_lcp_tile_sum<<<dim3(ntiles), dim3(LCP_BLOCK), 0, st>>>(phi, T, agg);
    }
    {
        LaunchScope ls(ctx, K_RERANK_SCAN, 8.0 * ntiles);
        k_lcp_spine<<<dim3(1), dim3(1024), 0, st>>>(agg, ntiles);
    }
    {
        LaunchScope ls(ctx, K_RERANK_APPLY, 8.0 * total);
        k_lcp_fill<<<dim3(ntiles), dim3(LCP_BLOCK), 0, st>>>(phi, T, agg);
    }
    {
        LaunchScope ls(ctx, K_BWT_GATHER, 12.0 * total);  // SA 4 n, a gathered word per slot, LCP 4 n
        k_lcp_gather<<<dim3(grid), dim3(256), 0, st>>>(d_sa, text.d_off, cnt, T, phi, d_lcp);
    }
    DK_HIP(ctx, hipGetLastError());
    ctx->stats.sa_route |= route;
    ctx->stats.lcp_passes = passes;
    ctx->stats.lcp_measured = ctx->stats.lcp_bytes_compared = 0;
    if (d_cnt) {
        std::vector<unsigned long long> h_cnt(2 * LCP_COUNTERS);
        DK_HIP(ctx, hipMemcpyAsync(h_cnt.data(), d_cnt, h_cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        DK_HIP(ctx, hipStreamSynchronize(st));
        for (uint32_t k = 0; k < LCP_COUNTERS; ++k) {
            ctx->stats.lcp_bytes_compared += h_cnt[2 * k];
            ctx->stats.lcp_measured += h_cnt[2 * k + 1];
        }
    }
    ctx->ws_release(mark);
    return DK_OK;
}

}  // namespace dk
