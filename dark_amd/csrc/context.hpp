// dk_ctx: one (host thread, GPU) pair.  Owns the HIP stream, the device workspace and the statistics.
// Mirrors the ownership of saca::Constructor (src/saca.rs:344-384: one storage buffer sized for max_n and reused
// across calls) plus block::dc::{Encoder,Decoder} (src/block/dc.rs:21-26,96-102).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/dark_amd.h"
#include "mailbox.hpp"

namespace dk {

// kernel slots for dk_stats (index into kernel_ms / kernel_bytes / kernel_launches)
enum KernelSlot : int {
    K_SYM_HIST = 0,
    K_RADIX_HIST,
    K_RADIX_SCAN,      // k_radix_scan
    K_RADIX_SCATTER,
    K_RERANK_REDUCE,
    K_RERANK_SCAN,
    K_RERANK_APPLY,
    K_ROUND_LOCAL,
    K_BWT_GATHER,
    K_DC_SUMMARY,
    K_DC_CARRY,        // k_dc_runscan + k_dc_carry_a/_b/_c + k_fill_u32
    K_DC_MAIN,
    K_DC_INIT,
    K_IBWT_HIST,       // k_ibwt_hist + k_ibwt_scan_a/_b/_c; the FM-index build: k_fm_hist + k_fm_scan_a/_b/_c + k_fm_heads
    K_IBWT_LF,
    K_IBWT_WALK,
    K_IBWT_JUMP,
    K_IBWT_EMIT,       // k_ibwt_emit / _copy, k_pib_emit / _copy; the locate structure: k_pib_locate x 2 + k_loc_rows + k_loc_scan; the extract structure: k_pib_anchors
    K_LF_FINISH,           // k_lf_finish (slot 18: k_bucket_store's until round 5)
    K_BIG_CLASSIFY,    // k_big_reduce + k_big_spine + k_big_apply
    K_BIG_BACK,
    K_PREFIX_PROBE,
    K_PLACE_ACTIVE,    // k_place_active + k_rank_active
    K_PLATEAU_SORT,
    K_PLATEAU_RANKS,   // k_plateau_ranks, k_to_inplace, k_plateau_count/_scan/_compact
    K_RADIX_SORT_SMALL,
    K_RADIX_HIST_TEXT,     // k_radix_hist<HS_TEXT>: first pass, digits straight from the text (1 B per key)
    K_RADIX_SCATTER_TEXT,  // k_radix_scatter<false, true>: first pass, keys built from the text (13 B per pair)
    K_ISA_PARTITION,       // k_isa_init + k_isa_split<true> + k_isa_split<false> (inverse permutation through LDS windows)
    K_ISA_ASSEMBLE,        // k_isa_assemble
    K_CHAIN,               // k_chain_extract + _ends + _tiles + _spine + _verdicts + _apply (pair chains; their sort is in the radix slots); k_sa_search*, k_sa_match*, k_sa_smem_*, k_fm_count, k_fm_locate, k_fm_extract, k_fm_find_*, k_fm_seam_*, k_fm_near_*
    K_PERIOD,              // k_period_first + _spine + _fill (next break of the block's dominant period, for the period round)
    K_SLOT_COUNT
};
static_assert(K_SLOT_COUNT <= DK_NUM_KERNEL_SLOTS, "grow DK_NUM_KERNEL_SLOTS");
const char *kernel_slot_name(int slot);

struct Timer {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

}  // namespace dk

struct dk_ctx {
    int device = -1;
    int numa_node = -1;  // memory node the GPU hangs on (/sys/bus/pci/devices/<bdf>/numa_node; -1: unknown): where the host coder looks for its L3 group first
    size_t max_n = 0;
    int purpose = DK_CTX_FULL;                 // DK_CTX_DECODER: the workspace holds the inverse path only, and begin_call refuses every other entry
    size_t max_blocks = DK_PACKED_MAX_BLOCKS;  // most blocks a packed call may hold (a decoder context's workspace is sized for its own limit)
    hipStream_t stream = nullptr;
    // a second stream for work that needs nothing from what the main stream does meanwhile (the L-first path's deep groups, ordered beside the
    // rounds that follow), forked from and joined to the main stream with the two events
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // device workspace: one allocation, bump-allocated per API call (all stages of a call run in sequence)
    char *ws = nullptr;
    size_t ws_size = 0, ws_used = 0, ws_peak = 0;
    // the mailbox (mailbox.hpp is its map): the small results of the device stages, and their pinned host twins
    dk::Mail *h_mail = nullptr;   // hipHostMalloc
    dk::Mail *d_mail = nullptr;
    // All three on `stream`.  mail_fetch enqueues *h_field = its twin in d_mail (or d_src: any device address holding a T); h_field points into
    // h_mail and is valid after the next synchronise of the stream.  mail_read synchronises at once.  mail_fill fills a member or group of d_mail.
    template <class T> int mail_fetch(T *h_field, const void *d_src = nullptr) {
        if (!d_src) d_src = reinterpret_cast<const char *>(d_mail) + (reinterpret_cast<const char *>(h_field) - reinterpret_cast<const char *>(h_mail));
        return hip_ok(hipMemcpyAsync(h_field, d_src, sizeof(T), hipMemcpyDeviceToHost, stream), "mailbox copy");
    }
    template <class T> int mail_read(T *h_field, const void *d_src = nullptr) {
        const int rc = mail_fetch(h_field, d_src);
        return rc != DK_OK ? rc : hip_ok(hipStreamSynchronize(stream), "mailbox wait");
    }
    template <class T> int mail_fill(T *d_field, int byte) { return hip_ok(hipMemsetAsync(d_field, byte, sizeof(T), stream), "mailbox fill"); }
    // pinned staging for D2H of the DC stream
    char *h_stage = nullptr;
    size_t h_stage_size = 0;
    // extra pinned staging slots for the batch entry point (one block being coded per host thread, one being filled)
    struct StageSlot { char *h = nullptr; size_t cap = 0; };
    std::vector<StageSlot> slots;
    int ensure_slot(size_t index, size_t bytes);
    std::string err;
    struct dk_batch *live_batch = nullptr;  // the streaming batch open on this context (dk_batch_begin .. dk_batch_finish), if any
    // D2H of a large block's distance stream in pieces: a host function behind every piece moves the frontier the host coder waits at
    struct D2hMark { std::atomic<size_t> *frontier; size_t value; };
    std::atomic<size_t> d2h_ready{0};
    std::vector<D2hMark> d2h_marks;
    unsigned last_flags = 0;   // DK_FLAG_* of the block the last block encode coded
    size_t last_consumed = 0;  // bytes of coded stream the last block decode read (records can be concatenated)
    dk_stats stats{};
    bool profiling = false;
    hipEvent_t round_ev[dk::LIVE_RING] = {};  // suffix sort: one per in-place round in flight (live count read back one round late)
    std::vector<hipEvent_t> ev_pool;
    struct Pending { int slot; hipEvent_t a, b; double bytes; hipStream_t on; };
    std::vector<Pending> ev_pending;
    size_t ev_next = 0;

    int fail(int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
    int hip_ok(hipError_t e, const char *what) { return e == hipSuccess ? DK_OK : fail(DK_E_HIP, "%s: %s", what, hipGetErrorString(e)); }

    void ws_reset() { ws_used = 0; }
    // 256-byte aligned bump allocation (dk::ws_round, below: what one takes); returns nullptr (and records the error) when the workspace is exhausted
    void *ws_alloc_bytes(size_t bytes);
    template <class T> T *ws_alloc(size_t count) { return static_cast<T *>(ws_alloc_bytes(count * sizeof(T))); }
    // the same for OPTIONAL buffers (a faster variant that can be done without): nullptr when it does not fit, no error recorded
    void *ws_try_alloc_bytes(size_t bytes);
    void ws_poison(void *p, size_t bytes);  // tuning build: DK_POISON
    template <class T> T *ws_try_alloc(size_t count) { return static_cast<T *>(ws_try_alloc_bytes(count * sizeof(T))); }
    size_t ws_mark() const { return ws_used; }
    void ws_release(size_t mark) { ws_used = mark; }

    // profiling: bracket a kernel launch with events on the context's stream
    void prof_begin(int slot, double bytes, hipStream_t on = nullptr);  // on: the stream the bracketed launches go to (default: `stream`)
    void prof_end();
    void prof_collect();  // after a stream sync: fold finished event pairs into stats
    int ensure_stage(size_t bytes);
};

namespace dk {

inline size_t ws_round(size_t bytes) { return (bytes + 255) & ~size_t(255); }  // what one ws_alloc of `bytes` takes: the *_workspace functions' arithmetic

#define DK_HIP(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) return (ctx)->fail(DK_E_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

#define DK_TRY(expr)            \
    do {                        \
        int rc_ = (expr);       \
        if (rc_ != DK_OK) return rc_; \
    } while (0)

// RAII kernel bracket: DK_LAUNCH(ctx, slot, bytes) { kernel<<<...>>>(...); }
struct LaunchScope {
    dk_ctx *c;
    LaunchScope(dk_ctx *ctx, int slot, double bytes, hipStream_t on = nullptr) : c(ctx) { if (c->profiling) c->prof_begin(slot, bytes, on); }
    ~LaunchScope() { if (c->profiling) c->prof_end(); }
};

// A/B switches of the kernels' variants (DK_XCD, DK_PREFIX, DK_RADIX_WIDE ...): read from the environment only in the TUNING build
// (-DDK_TUNING: dark_amd/libdark_amd_tuning.so, what tests/test_env_variants.py and tools/stage_time.py load); the product library has
// every switch compiled in as its default and never looks at the environment for them.
#ifdef DK_TUNING
int tuning_knob(const char *name, int dflt);
#define DK_KNOB(name, dflt) ([] { static const int v_ = dk::tuning_knob(name, dflt); return v_; }())
#else
#define DK_KNOB(name, dflt) (dflt)
#endif

inline size_t div_up(size_t a, size_t b) { return (a + b - 1) / b; }
inline unsigned ceil_log2_u64(uint64_t v) {  // smallest b with (1 << b) >= v
    unsigned b = 0;
    while (b < 64 && (1ull << b) < v) ++b;
    return b;
}

// ---- device stages (each enqueues on ctx->stream; the ones returning host values synchronise) -------------------
// radix_sort.hip
// first pass of the suffix sort's initial sort straight from the text: key(i) = packed codes of T[i .. i+spk) (<< 8 | code of T[i-1])
struct TextKeys { const uint8_t *t = nullptr; size_t n = 0; const uint8_t *code = nullptr; int bits = 0, spk = 0, with_prev = 0; };
// What the LAST pass of a sort writes beside the sorted keys (the suffix sort's initial sort): the values go to `vals` (the suffix array:
// every suffix at its slot) instead of the ping-pong buffer, and -- when bwt is given -- L[slot] = inv_code[low byte of the key] (the
// symbol in front of the suffix rides in the key's low byte) and *origin = the slot of value 0.  A later stage overwrites the entries of
// suffixes that are not final yet.
// narrow_shift >= 0 (sorts of at most 40 bits = five passes): the sorted keys are only ever compared with their neighbours afterwards, so
// the last pass writes them as 32-bit words, (key >> narrow_shift) cut to 32 bits, into the key buffer it would have written (viewed as
// u32) -- half the bytes to write and to read back.  What a fifth pass sorts by is exactly the bits cut off: two neighbours can differ in
// them only where its digit changes, and those 256 places go to bucket_starts (global index of the first pair of every digit).
struct SortFinalOut {
    uint32_t *vals = nullptr; uint8_t *bwt = nullptr; const uint8_t *inv_code = nullptr; uint32_t *origin = nullptr;
    int narrow_shift = -1; uint32_t *bucket_starts = nullptr;
};
// sort_pairs / sort_groups / local_sort_tiles: stable, on EXACTLY the key bits [begin_bit, end_bit) -- eight per pass, and a last pass of fewer when the
// width is no multiple of eight (its digit is masked to the bits below end_bit).  Bits outside the range travel with the pair and have no say.
// final_out (may be null; only with the sort of more than 8192 pairs): see SortFinalOut; then `vals` / `vals_alt` are both free on return
int sort_pairs(dk_ctx *ctx, uint64_t *&keys, uint64_t *&keys_alt, uint32_t *&vals, uint32_t *&vals_alt, size_t count,
               int begin_bit, int end_bit, const TextKeys *text = nullptr, const SortFinalOut *final_out = nullptr);
int sort_groups(dk_ctx *ctx, const uint64_t *kin, const uint32_t *vin, uint64_t *kout, uint32_t *vout, const uint32_t *starts, size_t ngroups, size_t npairs,
                uint32_t above, int begin_bit, int end_bit);
int local_sort_tiles(dk_ctx *ctx, uint64_t *d_keys, uint32_t *d_vals, size_t count, int begin_bit, int end_bit);  // experiment hook
// rank[sa[p]] = p for a permutation sa of 0 .. n-1, through LDS windows (radix_sort.hip); scratch_a / scratch_b: n u64 each.
// marked_val (may be null): entries of sa with bit 31 set stand for sa[p] & 0x7FFFFFFF and take their value from marked_val[p] instead of p
int inverse_permutation(dk_ctx *ctx, const uint32_t *sa, size_t n, uint64_t *scratch_a, uint64_t *scratch_b, uint32_t *rank, const uint32_t *marked_val = nullptr);
bool inverse_through_windows(size_t n);  // does the inverse of a permutation of n entries take the LDS-window form?
// suffix_array.hip: d_sa_out may alias nothing in the workspace; d_text is caller or ctx owned
// d_bwt / d_origin / bwt_written (all three or none): a caller that wants L.  The sort carries the symbol in front of every suffix along and
// writes L and the origin word itself; it then sets *bwt_written -- and d_sa_out is SCRATCH WITH UNDEFINED CONTENTS on return (the L-first path
// never completes a suffix array; on the rank path nobody writes SA entries once the ranks exist, and a period round keeps its next-break
// positions there).  Only when *bwt_written comes back false does d_sa_out hold the suffix array (the caller gathers L: bwt_forward_device).
int suffix_array_device(dk_ctx *ctx, const uint8_t *d_text, size_t n, uint32_t *d_sa_out, uint8_t *d_bwt = nullptr,
                        uint32_t *d_origin = nullptr, bool *bwt_written = nullptr);
int bwt_forward_device(dk_ctx *ctx, const uint8_t *d_text, size_t n, uint32_t *d_sa, uint8_t *d_bwt, uint32_t *origin);
// dk_dbg_dev_rerank's arguments under the names of the header: one rerank() and the classify_and_read() behind it on the caller's arrays.
// keys: 32-bit words when bucket_starts is given.  counts_out: active, groups, big_slots, big_groups, above_pl_slots.  Synchronises.
struct DbgRerank {
    const uint64_t *keys; const uint32_t *bucket_starts, *idx, *pos_in, *gid_in; int cmp_shift; size_t count;
    uint32_t *rank, *sa; uint8_t *bwt; const uint8_t *sym_in; uint8_t *sym_out; uint32_t *origin;
    uint32_t *out_idx, *out_pos, *out_gid, *gstart, *bigidx, *bigoff; uint32_t ls_max;
    uint32_t reduce_tiles_per_wg, first_tiles_per_wg; int sparse_max;
};
int dbg_rerank_device(dk_ctx *ctx, const DbgRerank &args, uint32_t counts_out[5]);
// dk_dbg_dev_lf_rerank's arguments under the names of the header: one lf_rerank() (lfirst.inc) on the caller's arrays and the classification behind
// it as lfirst_path runs it after its first rerank.  keys: 32-bit words when key_bytes is 4 (with bucket_starts: the narrow first rerank; without:
// group ids, the take-over form).  bigdepth != nullptr: the big-list depth rule.  counts_out: active, groups, big_slots, big_groups.  Synchronises.
struct DbgLfRerank {
    const void *keys; int key_bytes; const uint32_t *bucket_starts; int cmp_shift; uint8_t *sym; int sym_from_key;
    const uint32_t *idx, *zero_slot, *pos_in; size_t count;
    uint32_t *out_idx, *out_pos, *out_gid; uint8_t *out_sym; uint32_t *gstart; uint8_t *bwt; uint32_t *origin;
    uint32_t *gdepth_out; uint32_t depth_uniform; const uint32_t *bigdepth; int key_shift; uint32_t depth_add;
    uint32_t reduce_tiles_per_wg;
};
int dbg_lf_rerank_device(dk_ctx *ctx, const DbgLfRerank &args, uint32_t counts_out[4]);
// dk_dbg_dev_lf_refine's arguments: lfirst_path() from the caller's list (count slots of groups equal in their first h0 symbols) to its end.
// out: verdict, sa_route, rounds, deep_count, arena_used, giant_count[0], fallback, giant_count[1].  Synchronises.
struct DbgLfRefine {
    const uint8_t *text; size_t n; const uint32_t *idx, *pos, *gid; const uint8_t *sym; size_t count; uint32_t h0; int period;
    uint8_t *bwt; uint32_t *origin;
};
int dbg_lf_refine_device(dk_ctx *ctx, const DbgLfRefine &args, uint32_t out[8]);
// dk_dbg_dev_in_place's arguments under the names of the header: in_place_rounds() on the caller's list.  sa, or bwt + sym + origin (+ out_sym).
// out: slots, live, chain records, list full, settled by the chains, rounds launched, compactions, sa_route.  Synchronises.
struct DbgInPlace {
    size_t n; uint32_t h; size_t count; const uint32_t *idx, *pos, *gid, *gstart; size_t groups;
    uint32_t *rank, *sa; uint8_t *bwt; const uint8_t *sym; uint32_t *origin;
    int chain_group; uint32_t record_cap; int max_rounds, always_compact;
    uint32_t *out_idx, *out_meta; uint8_t *out_sym; uint32_t *out_pos;
};
int dbg_in_place_device(dk_ctx *ctx, const DbgInPlace &args, uint32_t out[8]);
// dk_dbg_dev_round's arguments under the names of the header: one general_round() on the caller's list.  sa, or bwt + sym + origin (+ out_sym, out_sorted_sym).
// out: active, groups, big slots, big groups, slots above PL_MAX, symbols advanced, sa_route, kb.  Synchronises.
struct DbgRound {
    const uint8_t *text; size_t n; uint32_t h; size_t count; const uint32_t *idx, *pos, *gid, *gstart; size_t groups;
    uint32_t *rank; int tsym, period; const uint32_t *next_break;
    uint32_t *sa; uint8_t *bwt; const uint8_t *sym; uint32_t *origin;
    uint64_t *out_sorted_keys; uint32_t *out_sorted_idx; uint8_t *out_sorted_sym;
    uint32_t *out_idx, *out_pos, *out_gid, *out_gstart; uint8_t *out_sym;
};
int dbg_round_device(dk_ctx *ctx, const DbgRound &args, uint32_t out[8]);
// dk_dbg_dev_period's arguments under the names of the header: the period kernels and the probes on the caller's text, each part switched on by its
// output (next_break: by period > 0).  Synchronises.
struct DbgPeriod {
    const uint8_t *text; size_t n; int period; uint32_t *next_break;
    uint32_t *run_out, *probe_out; uint32_t count_p, *count_out; uint32_t search_pmax, *found_out;
    uint32_t m, span; const int *cands; int ncands; uint32_t *dups_out;
};
int dbg_period_device(dk_ctx *ctx, const DbgPeriod &args);
// dk_dbg_dev_initial_sort's arguments under the names of the header: one sort_pairs() with the TextKeys and the SortFinalOut that initial_sort()
// builds, the code tables the caller's.  inv, bwt and origin: all three or none (their presence is with_prev).  keys_out: n words of 8 bytes, of 4
// when narrow.  bucket_starts_out (host, 256 words): narrow only.  out: sa_route bits the sort set | sort_passes | sorted_elements (low word) | 0.
// Synchronises.
struct DbgInitialSort {
    const uint8_t *text; size_t n; const uint8_t *code; int bits, spk; const uint8_t *inv; int narrow;
    void *keys_out; uint32_t *sa; uint8_t *bwt; uint32_t *origin; uint32_t *bucket_starts_out;
};
int dbg_initial_sort_device(dk_ctx *ctx, const DbgInitialSort &args, uint32_t out[4]);
// bwt.hip
int bwt_gather_device(dk_ctx *ctx, const uint8_t *d_text, const uint32_t *d_sa, size_t n, uint8_t *d_bwt, uint32_t *origin);
int bwt_inverse_device(dk_ctx *ctx, const uint8_t *d_bwt, size_t n, uint32_t origin, uint8_t *d_out);
// packed inverse: block i's text at d_out[off[i], off[i+1]) from its L at d_bwt[off[i], ...) and origin[i] (host, < n_i, checked by the caller);
// off on the host, off[count] = total.  DK_E_STREAM naming the lowest corrupt block, and then nothing is written to d_out.
int packed_ibwt_device(dk_ctx *ctx, const uint8_t *d_bwt, const std::vector<uint32_t> &off, const uint32_t *origin, uint8_t *d_out);
// Workspace the two calls above take at most, every ws_alloc rounded up to 256 bytes: bwt_inverse_device for ANY block of at most max_n bytes
// and any origin, packed_ibwt_device for ANY pack of at most max_total bytes in at most max_blocks blocks.  Non-decreasing in every argument.
// Host arithmetic only (abi.cpp: decoder_workspace_bytes).
size_t bwt_inverse_workspace(size_t max_n);
size_t packed_ibwt_workspace(size_t max_total, size_t max_blocks);
// dc.hip: d_run_end may be null
int dc_encode_device(dk_ctx *ctx, const uint8_t *d_bwt, size_t n, uint32_t init_host[256], uint32_t *d_dist, uint8_t *d_sym,
                     uint8_t *d_rank, uint32_t *d_run_end, size_t *m);
// packed.hip: `count` blocks back to back in d_text, block i at [d_off[i], d_off[i+1]) (d_off on the device, d_off[count] = total).
// packed_bwt_device: L of every block at its own range of d_bwt, d_origin[i] (device) = block i's origin; rounds stop after max_rounds and
// d_guard[i] = 1 marks the blocks that were still unresolved then (their L / origin are NOT valid: the caller re-runs them alone);
// *guarded = the number of suffixes left unresolved (0: every block is done).
int packed_bwt_device(dk_ctx *ctx, const uint8_t *d_text, const uint32_t *d_off, size_t count, size_t total, uint8_t *d_bwt, uint32_t *d_origin,
                      uint32_t *d_guard, int max_rounds, size_t *guarded);
// packed_sa_device: the same sort, then block i's suffix array at d_sa[off_i, off_i + n_i), entries local to the block; d_bwt / d_origin (both
// or neither) as from packed_bwt_device, written by the same kernel.  Guarded blocks' stretches are NOT valid, as above.
// d_phi (may be null; total words): Phi for the LCP pass, from the sort's rank before it is released (lcp_phi_from_rank_device).
int packed_sa_device(dk_ctx *ctx, const uint8_t *d_text, const uint32_t *d_off, size_t count, size_t total, uint32_t *d_sa, uint8_t *d_bwt,
                     uint32_t *d_origin, uint32_t *d_guard, int max_rounds, size_t *guarded, uint32_t *d_phi = nullptr);
// dk_dbg_dev_packed_first's arguments under the names of the header: the first step of the segmented sort (code table, first keys, their sort, the
// first regroup) on the caller's pack; off on the device.  keys / vals / rank: total entries, act: its first `live`.  code_out (host, 256 codes).
// out: sigma | bits | blk_bits | k_used | live | the sort's end bit | 0 | 0.  Synchronises; releases its workspace.
struct DbgPackedFirst {
    const uint8_t *text; const uint32_t *off; size_t count, total;
    uint64_t *keys; uint32_t *vals, *rank, *act; uint16_t *code_out;
};
int dbg_packed_first_device(dk_ctx *ctx, const DbgPackedFirst &args, uint32_t out[8]);
// dk_dbg_dev_packed_round's arguments under the names of the header: one round of the segmented sort at depth h on the caller's list act[0, c) and
// the caller's ranks, and the guard step on the next list when guard (count words) is given.  out: rbits | gbits | live | 0 ...  Synchronises;
// releases its workspace.
struct DbgPackedRound {
    const uint32_t *off; size_t count, total; uint32_t h; const uint32_t *act; size_t c; uint32_t *rank;
    uint64_t *keys; uint32_t *vals, *next_act, *guard;
};
int dbg_packed_round_device(dk_ctx *ctx, const DbgPackedRound &args, uint32_t out[8]);
// ---- the views the query stages take: aggregates of device pointers and sizes, filled on the host by abi_query.cpp; they own nothing ------
// PackView: `count` blocks back to back in `bytes` (text or L), block i at [d_off[i], d_off[i + 1]), d_off[count] = total, as in
// packed_sa_device; a single block is a pack of one (d_off = {0, n}).
struct PackView { const uint8_t *bytes; const uint32_t *d_off; size_t count, total; };
// FmView: a packed L and what was built from it: the index (fm_build_device), the locate and the extract structure of sampling step `step`
// (null where the stage reads none), d_abase = the blocks' anchor bases (fm_extract_bases; null: one block, base 0).
struct FmView { PackView L; const void *index, *loc, *ext; uint32_t step; const uint32_t *d_abase; };
// ItemView: `count` items -- patterns, queries, rows of byte classes -- back to back in `bytes`, item q at [d_off[q], d_off[q + 1]), d_off[count] =
// nbytes, for block d_blk[q] (checked by the caller; null: block 0, or every block where the stage says so).  longest / shortest: of their lengths.
struct ItemView { const uint8_t *bytes; const uint32_t *d_off, *d_blk; size_t count, nbytes, longest, shortest; };
// HitSink: where a stage that lists hits leaves them: *total_out (host) = their number, d_hits (16-byte aligned records of 16 bytes) = the
// first min(total, max_hits) of them (max_hits == 0: not looked at), d_occ (may be null) = the hits of every (item, block) pair.
struct HitSink {
    size_t max_hits; void *d_hits; uint32_t *d_occ; uint64_t *total_out;
    size_t take(uint64_t total) const { *total_out = total; return static_cast<size_t>(total < max_hits ? total : max_hits); }  // -> records to write
};
// lcp.hip: d_lcp[i] = common prefix of the suffixes at slots i - 1 and i of their block, 0 at a block's first slot; d_sa /
// d_lcp laid out as the text.  DK_E_ARG, with d_lcp untouched, for an entry of d_sa outside its block.  Synchronises (the lists' counters are
// read back); ORs DK_ROUTE_LCP_* into stats.sa_route.  Takes 4 total + total / 1024 bytes of workspace and sizes its two lists from what is
// left; releases all of it.
// d_phi_ready (may be null; total words, the caller's): Phi as lcp_phi_from_rank_device / lcp_phi_block_device left it -- d_sa is not checked then.
int lcp_device(dk_ctx *ctx, const PackView &text, const uint32_t *d_sa, uint32_t *d_lcp, uint32_t *d_phi_ready = nullptr);
// Phi of the whole pack from the packed sort's rank (the inverse suffix array) and the suffix arrays k_pk_emit wrote from it; the stretches of
// guarded blocks hold nothing useful afterwards ...
int lcp_phi_from_rank_device(dk_ctx *ctx, const uint32_t *d_rank, const uint32_t *d_sa, const uint32_t *d_off, size_t count, size_t total, uint32_t *d_phi);
// ... and are redone here, one block's slots [lo, hi) at a time, from the suffix array the guard has written
int lcp_phi_block_device(dk_ctx *ctx, const uint32_t *d_sa, const uint32_t *d_off, size_t count, size_t lo, size_t hi, uint32_t *d_phi);
// sa_query.hip; d_sa laid out as the text.
// sa_check_device: h_words (host, 3 count) = per block the lowest slot whose entry is outside the block, the lowest position no slot names, the lowest
// slot whose suffix is not greater than the one in front of it; all ones: none.  The order is evaluated only for blocks without the first two.
// Synchronises.  Takes 4 total + 12 count bytes of workspace and releases them.
int sa_check_device(dk_ctx *ctx, const PackView &text, const uint32_t *d_sa, uint32_t *h_words);
// sa_search_device: d_lo[q] / d_hi[q] = slots of pattern q's block whose suffix, cut to the pattern's length, is smaller than / not greater than
// the pattern.  The longest and the shortest length decide the kernels launched.  Enqueues only; takes no workspace.
int sa_search_device(dk_ctx *ctx, const PackView &text, const uint32_t *d_sa, const ItemView &pat, uint32_t *d_lo, uint32_t *d_hi);
// sa_match_device: for every position g < qry.nbytes, d_len[g] = the longest prefix of its window (at most max_len
// bytes, inside its query) that occurs in the query's block, d_lo[g] / d_hi[g] (both or neither) = sa_search_device's numbers for that prefix.
// Enqueues only; takes no workspace.
int sa_match_device(dk_ctx *ctx, const PackView &text, const uint32_t *d_sa, const ItemView &qry, size_t max_len, uint32_t *d_len, uint32_t *d_lo, uint32_t *d_hi);
// sa_smems_device: the super-maximal matches of those statistics, records {at, len, lo, hi} (at = the position g) in rising order of at;
// out.d_occ is not looked at.  Takes sa_smems_workspace(qry.nbytes) bytes (16 per query byte and a word per 1024, every ws_alloc rounded
// up) and releases them.  Synchronises.
size_t sa_smems_workspace(size_t qbytes);
int sa_smems_device(dk_ctx *ctx, const PackView &text, const uint32_t *d_sa, const ItemView &qry, size_t min_len, size_t max_len, const HitSink &out);
// fm_index.hip: the FM-index of a packed L and the backward search in it; a single block is a pack of one.
// fm_index_words: 32-bit words of the index (host arithmetic).  fm_build_workspace: what fm_build_device takes, every ws_alloc rounded up.
size_t fm_index_words(size_t total, size_t count);
size_t fm_build_workspace(size_t total, size_t count);
// off (host, count + 1) and origin (host, count; origin[i] < n_i checked by the caller) describe the pack.  Synchronises; releases its workspace.
int fm_build_device(dk_ctx *ctx, const uint8_t *d_bwt, const std::vector<uint32_t> &off, const uint32_t *origin, void *d_index);
// d_lo[q] / d_hi[q] are the numbers sa_search_device gives, by backward search in L.  Enqueues only; takes no workspace.
int fm_count_device(dk_ctx *ctx, const FmView &fm, const ItemView &pat, uint32_t *d_lo, uint32_t *d_hi);
// d_out[q] = occurrences of d_sym[q] in L[0, min(d_pos[q], total)), by the count kernel's rank: of fm, the bytes, the total and the index's
// checkpoints are read and nothing else.  Enqueues only.
int fm_rank_device(dk_ctx *ctx, const FmView &fm, const uint32_t *d_pos, const uint8_t *d_sym, size_t nq, uint32_t *d_out);
// The locate structure of a packed L (bwt.hip builds it, fm_index.hip reads it): 32-bit words, over the whole pack.
//   [0, 64) header | rows + 1 marks before each 1024-slot row | 32 rows mark bits | total / step + count samples, in slot order
// step: a power of two in [1, 4096] (the caller's check).  Host arithmetic, and the one place that knows the layout.
constexpr uint32_t FM_LOC_MAGIC = 0x314C4D46u;  // "FML1"
constexpr uint32_t FM_LOC_HEADER = 64;
struct FmLocate { uint32_t *marks, *bits, *samples; size_t rows, nsamp; };
inline size_t fm_locate_words(size_t total, size_t count, size_t step) { return FM_LOC_HEADER + 33 * div_up(total, 1024) + 1 + total / step + count; }
inline FmLocate fm_locate_carve(void *d_loc, size_t total, size_t count, size_t step) {
    uint32_t *w = static_cast<uint32_t *>(d_loc);
    const size_t rows = div_up(total, 1024);
    return FmLocate{w + FM_LOC_HEADER, w + FM_LOC_HEADER + rows + 1, w + FM_LOC_HEADER + rows + 1 + 32 * rows, rows, total / step + count};
}
// bwt.hip: the structure from (L, origin) alone, by the packed inverse's table, walk and jumps and two more walks (a single block is a pack of
// one).  off / origin as for fm_build_device.  DK_E_STREAM, naming the lowest such block when `packed`, for a block that is no BWT; d_loc is
// then unspecified.  Synchronises; takes at most fm_locate_build_workspace(total, count) <= packed_ibwt_workspace(total, count), releases it.
int fm_locate_build_device(dk_ctx *ctx, const uint8_t *d_bwt, const std::vector<uint32_t> &off, const uint32_t *origin, uint32_t step, void *d_loc,
                           bool packed);
size_t fm_locate_build_workspace(size_t total, size_t count);  // an upper bound of what it takes, every ws_alloc rounded up; host arithmetic
// fm_index.hip: item (q, j), j < max_hits, of pattern q with the range [d_lo[q], d_hi[q]) in block d_pat_blk[q] (null: block 0):
// d_pos[q * max_hits + j] = SA_b[lo + j], DK_FM_NO_HIT behind the range.  Reads fm.loc.  Enqueues only; takes no workspace.
int fm_locate_device(dk_ctx *ctx, const FmView &fm, const uint32_t *d_lo, const uint32_t *d_hi, const uint32_t *d_pat_blk, size_t npat, size_t max_hits,
                     uint32_t *d_pos);
// fm_index.hip: every pattern in every block (pat.d_blk is not looked at).  Pair p = q * count + b: out.d_occ[p] = its
// occurrences; the records {pattern, block, position, slot} stand in the order (q, b, slot), position as fm_locate_device gives it.
// out.max_hits == 0: fm.loc is not looked at either.  Takes fm_find_workspace(pat.count * count) bytes (16 per pair and the chunk sums, every
// ws_alloc rounded up) and releases them.  Synchronises.
size_t fm_find_workspace(size_t npairs);
int fm_find_device(dk_ctx *ctx, const FmView &fm, const ItemView &pat, const HitSink &out);
// fm_index.hip: every pattern in every block again, the pattern's positions byte classes (cls.bytes: 32 bytes per
// position, so cls.d_off counts positions) and up to k of them missed.  Pairs, out.d_occ and fm.loc as for fm_find_device; inside a pair the
// hits stand in the preorder of the search tree, of which at most node_limit nodes (0: DK_FM_NEAR_NODE_LIMIT) are visited.  *cut_out (host,
// may be null) = the pairs that stopped there.  Records {pattern, block, position, cost}.  Takes fm_near_workspace(cls.count * count) bytes
// (16 per pair and two rows of chunk sums) and releases them.  Synchronises.
size_t fm_near_workspace(size_t npairs);
int fm_near_device(dk_ctx *ctx, const FmView &fm, const ItemView &cls, uint32_t k, uint32_t node_limit, const HitSink &out, uint64_t *cut_out);
// The extract structure of a packed L (bwt.hip builds it, fm_index.hip reads it): 32-bit words, over the whole pack.
//   [0, 64) header: magic, total, count, step, anchors | total / step + count anchors
// Block b's anchors are the ceil(n_b / step) words from its anchor base, the sum of ceil(n_i / step) over the blocks in front of it: anchor k =
// the slot (local to the block) of the suffix that starts at position k * step, so anchor 0 = origin_b.  The bases are not stored: the host
// computes them from the sizes at every call (fm_extract_bases), as it does the offsets.  total / step + count >= their sum.
constexpr uint32_t FM_EXT_MAGIC = 0x31584D46u;  // "FMX1"
constexpr uint32_t FM_EXT_HEADER = 64;
inline size_t fm_extract_words(size_t total, size_t count, size_t step) { return FM_EXT_HEADER + total / step + count; }
inline std::vector<uint32_t> fm_extract_bases(const std::vector<uint32_t> &off, uint32_t step) {  // count + 1 words; the last one = all anchors
    std::vector<uint32_t> abase(off.size(), 0);
    for (size_t i = 0; i + 1 < off.size(); ++i) abase[i + 1] = abase[i] + static_cast<uint32_t>(div_up(off[i + 1] - off[i], step));
    return abase;
}
// bwt.hip: the structure from (L, origin) alone: fm_locate_build_device's front part, then one walk that stores the anchors.  Arguments, errors
// and synchronisation as there; takes at most fm_locate_build_workspace(total, count) + 4 (count + 1) bytes (rounded up) and releases them.
int fm_extract_build_device(dk_ctx *ctx, const uint8_t *d_bwt, const std::vector<uint32_t> &off, const uint32_t *origin, uint32_t step, void *d_ext,
                            bool packed);
// fm_index.hip: row q of d_out (nrange x max_len bytes, any alignment) = T_b[pos, pos + got) of block d_rng_blk[q] (null: block 0), where pos =
// d_pos[q] and got = min(d_len[q] (null: max_len), max_len, n_b - pos), 0 for pos >= n_b; zeros behind.  Reads fm.ext and fm.d_abase.  Enqueues
// a memset of the rows and one kernel; takes no workspace.
int fm_extract_device(dk_ctx *ctx, const FmView &fm, const uint32_t *d_pos, const uint32_t *d_len, const uint32_t *d_rng_blk, size_t nrange, size_t max_len,
                      uint8_t *d_out);
// fm_index.hip: the matches that straddle the borders of a pack whose text is preceded by prev_len bytes d_prev.
// fm_seam_plan lays out the edge strip for W = longest pattern - 1 (host arithmetic): words = 3 per block {strip offset of the block's first byte,
// min(n_b, W), start of the contiguous run that reaches it}, then block, start, length and strip offset of each of the nrange <= 2 count - 1
// extract ranges.  fm_seams_device fills the strip through k_fm_extract (fm.ext, fm.d_abase), counts, scans and emits as fm_find_device does:
// pairs and out.d_occ as there, records {pattern, block, back, 0} in the order (q, b, back descending).  Takes fm_seams_workspace bytes and
// releases them.  Synchronises.
struct FmSeamPlan { std::vector<uint32_t> words; size_t nrange = 0, strip_len = 0, max_len = 1; };
FmSeamPlan fm_seam_plan(const std::vector<uint32_t> &off, size_t prev_len, size_t W);
size_t fm_seams_workspace(const FmSeamPlan &pl, size_t npairs);
int fm_seams_device(dk_ctx *ctx, const FmView &fm, const uint8_t *d_prev, size_t prev_len, const FmSeamPlan &pl, const ItemView &pat, const HitSink &out);
// packed_dc_device: the DC arrays of every block of a packed L.  compact: block i's entries at [rb_i, rb_i + m_i) (global run order, rb on the
// device in d_rb[0 .. count], d_rb[count] = all runs); otherwise at [off_i, off_i + m_i).  d_m / d_flags: count words, d_init: count x 256.
int packed_dc_device(dk_ctx *ctx, const uint8_t *d_bwt, const uint32_t *d_off, size_t count, size_t total, bool compact, uint32_t *d_dist,
                     uint8_t *d_sym, uint8_t *d_rank, uint32_t *d_run_end, uint32_t *d_m, uint32_t *d_flags, uint32_t *d_rb, uint32_t *d_init);

}  // namespace dk
