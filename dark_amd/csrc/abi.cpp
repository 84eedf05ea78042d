// extern "C" boundary (include/dark_amd.h): contexts, the codec, batches, the packed stages and the debug entries; the query entries (LCP,
// suffix-array check / search, FM-index) are in abi_query.cpp.  Thin: argument checks, workspace carving, stage sequencing, timing.
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "abi_common.hpp"
#include <cstdlib>
#include <atomic>
#include "entropy.hpp"

using namespace dk;

int dk::begin_call(dk_ctx *ctx, const char *forward_entry) {
    if (!ctx) return DK_E_ARG;
    if (forward_entry && ctx->purpose == DK_CTX_DECODER)
        return ctx->fail(DK_E_ARG, "%s: not served by a decoder context (dk_ctx_create_decoder sizes the workspace for the inverse path only)", forward_entry);
    // a streaming batch owns the workspace and the staging slots until it is finished: any other call would pull them from under
    // the coding threads
    if (ctx->live_batch) return ctx->fail(DK_E_ARG, "a streaming batch is open on this context: call dk_batch_finish first");
    ctx->err.clear();
    ctx->last_flags = 0;
    ctx->ws_reset();
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(DK_E_HIP, "hipSetDevice(%d) failed", ctx->device);
    return DK_OK;
}

namespace {

#ifndef DK_D2H_OVERLAP
#define DK_D2H_OVERLAP 1  // the distance stream of a large single block leaves the GPU in pieces while the host coder already runs (0: A/B builds)
#endif

size_t workspace_bytes(size_t max_n) {
    // Peak of the bump allocator, reached inside the suffix sort of a host-pointer block call (every term is one ws_alloc of the call):
    //   text copy                                   n     (host entry points only)
    //   L                                           n
    //   SA                                         4 n
    //   suffix sort: keys x3 24 n, suffix lists x3 12 n, rank 4 n, slot positions x2 8 n, group ids x2 8 n,
    //                gstart + bigidx 4 n, big-group offsets n / 8, symbols in front x2 2 n            = 62.1 n
    //   on top of that, one of (never two at a time: each is released before the next is taken)
    //     radix sort: per-tile digit tables n / 4 (256 counters per 4096 pairs) + digit plane n (optional, from 2^20 pairs:
    //                 ws_try_alloc -- the sort runs without it when it does not fit)                  = 1.25 n
    //     rerank:     one flag byte per slot n + tile aggregates n / 64 (L-first: + n / 128)          = 1.03 n
    //     pair chains: one verdict byte per record, at most n / 2
    //   and, for the whole of the L-first path (lfirst_path: held TOGETHER with the sort's and the rerank's temporaries above):
    //     the list of deep groups 16 MiB, two giant lists with their arenas 5.6 MiB, the grid-wide measure's results 1 MiB = 23 MiB
    //     (its arena of deep members, the depth tables and the next-break positions live in buffers of the 62.1 n that the path does not use otherwise)
    // = 69.4 n + 23 MiB; every allocation is rounded up to 256 bytes (about forty of them: < 16 KiB).  The DC arrays (10 n) and the inverse
    // BWT's successor table (8 n) are allocated after the sort's temporaries are released and take their place.
    // The packed inverse (dk_dev_packed_decode: L n, successor table 8 n, walk records at most 8 n, splitter arrays at most 32 n, per-block words
    // 16 count <= 16 n) stays below 65 n; its table of every block's symbol bases (count x 1 KiB, at most 64 MiB) fits the constant term.
    // The packed suffix arrays (dk_suffix_array_packed: text n, SA 4 n, the pack's temporaries 32 n + the sort's 1.25 n) stay below 39 n.  Their guard
    // runs after those temporaries are released, straight into the block's stretch of the output: text + SA 5 n and the single-block sort
    // 63.4 n_i (no L from the sort, so the L-first path and its 23 MiB never run) = at most 68.4 n.
    // The LCP pass (lcp.hip: lcp_device) runs after the sort's temporaries are released: Phi / PLCP 4 n in place, tile aggregates n / 1024, and
    // two lists sized from what is left (at most n + 1 MiB + 32 KiB).  Around it SA 4 n and LCP 4 n (+ text n) in the host-pointer form: below 15 n.
    // In dk_dev_suffix_array_packed_lcp the 4 n of Phi are held across the packed sort (32 n + 1.25 n) and its guard (63.4 n_i): at most 67.4 n.
    // tests/test_gpu_lcp.py checks peak <= size for the single and the packed one-call forms on contexts sized exactly to their input.
    // The suffix-array check (sa_query.hip: sa_check_device) takes the inverse array 4 n and 12 bytes per block, beside text and SA (5 n) in the
    // host-pointer form: 9 n + 12 count <= 21 n.  The search takes 8 bytes per pattern; its host-pointer form, which also holds the patterns and
    // two result words per pattern, refuses a batch that does not fit beside the 5 n (DK_E_ARG).  Both are far below the sort's peak, so this
    // size does not grow for them; tests/test_gpu_sa_search.py checks peak <= size on contexts sized exactly to their input.
    // The FM-index (fm_index.hip) keeps its index in the caller's memory: its build takes at most 256 KiB + 8 bytes per block, its count 8 bytes per
    // pattern, and its host-pointer form L and the index (2 n + 3 KiB) beside a batch that it refuses when it does not fit (DK_E_ARG).
    // tests/test_gpu_parity.py::test_workspace_accounting checks peak <= size on contexts sized exactly to their block, and
    // tests/test_gpu_fullsize.py checks the n-proportional term where the constant is negligible (peak - 64 MiB <= 69.4 n at 1e8 bytes).
    const size_t sort_temporaries = 62 * max_n + max_n / 8, io = 6 * max_n, on_top = max_n / 4 + max_n;
    return sort_temporaries + io + on_top + max_n / 4 /* headroom */ + (64u << 20);
}
size_t decoder_workspace_bytes(size_t max_n, size_t max_blocks) {
    // Peak of the bump allocator over the calls a decoder context serves (every term is one ws_alloc of the call, rounded up to 256 bytes):
    //   bwt_inverse_device (bwt.hip: bwt_inverse_workspace)
    //     tile histograms  256 counters per 4096 positions                                            n / 4
    //     chunk sums       at most 256 chunks x 256 counters                                          256 KiB at most
    //     class starts                                                                                1 KiB
    //     successor table                                                                             8 n
    //     blocks below 2^16 (S = 8):  four splitter arrays of ceil(n / 8) + 1 words, no records       2 n
    //     blocks from 2^16 (S = 64):  four splitter arrays of ceil(n / 64) + 1 words                  n / 4
    //                                 len_keep + resume, one word per splitter each                   n / 8
    //                                 records, IB_REC = 256 bytes per splitter                        4 n
    //     = 12.625 n from 2^16 bytes (10.25 n below)
    //   around it, at most two block-sized buffers: L + the output copy (dk_bwt_inverse, dk_block_decode, dk_raw_block_decode); L alone in
    //   dk_dev_block_decode and dk_dev_batch_decode; none in dk_dev_bwt_inverse                       2 n
    //   = 14.625 n for a single block.
    //   packed_ibwt_device (bwt.hip: packed_ibwt_workspace), count <= max_blocks blocks of `total` <= max_n bytes together
    //     aux              off | origin | first splitter of every block: 3 count + 2 words
    //     tile histograms, chunk sums, class starts, successor table over the pack                    8.25 total
    //     base             count x 256 words                                                          1 KiB per block
    //     cls0             count words
    //     four splitter arrays of nsplit <= min(total, total / 64 + 2 count) words (sum of ceil(n_i / 64), + 1 per origin off the grid)
    //     len_keep + resume + records only where nsplit * 32 <= total                                 8.25 total at most
    //   around it the pack-sized L of dk_dev_packed_decode                                            total
    //   = 13.625 total for one block, 33.5 total + 1 KiB per block for a pack of one-byte blocks.
    // The larger of the two, + n / 64 + 64 KiB of headroom.  The pinned staging (ensure_stage, ensure_slot) is host memory and not part of this.
    // The FM-index entries (fm_index.hip) are served too and stay below all of that: the build takes chunk sums of at most min(256 KiB, n + 2 KiB)
    // and 8 bytes per block, the host-pointer form 2 n + 3 KiB beside them (tests/test_gpu_fm.py checks peak <= size on both purposes).
    // The locate structure's build (bwt.hip: fm_locate_build_device) is the packed inverse above without its records, for one block too, so it
    // fits whatever fits `packed`; dk_fm_locate refuses what does not fit (tests/test_gpu_fm_locate.py checks peak <= size on both purposes).
    // The extract structure's build (fm_extract_build_device) is that front part and 4 bytes per block more, far below the records left out.
    // Find (fm_find_device) takes 16 bytes per (pattern, block) pair and 2 KiB: the caller's choice, not the block's, so this size does not grow
    // for it and dk_dev_fm_find* refuse a grid that does not fit (tests/test_gpu_fm_find.py checks peak <= size on both purposes).
    // tests/test_gpu_decoder_ctx.py checks peak <= size on contexts sized exactly to their block or pack, through every entry above.
    const size_t single = 2 * ((max_n + 255) & ~size_t(255)) + bwt_inverse_workspace(max_n);
    const size_t packed = ((max_n + 255) & ~size_t(255)) + packed_ibwt_workspace(max_n, max_blocks);
    return std::max(single, packed) + max_n / 64 /* headroom */ + (64u << 10);
}
bool good_ctx_size(int purpose, size_t max_n, size_t max_blocks) {
    if (max_n == 0 || max_n > 0x7FFFFFFEull) return false;
    return purpose == DK_CTX_FULL || (purpose == DK_CTX_DECODER && max_blocks >= 1 && max_blocks <= DK_PACKED_MAX_BLOCKS);
}
// device-resident forward path up to the compact DC stream in pinned host memory
struct ForwardResult {
    uint32_t init[256];
    uint32_t origin = 0;
    size_t m = 0;
    const uint32_t *dist = nullptr;
    const uint8_t *sym = nullptr;
    const uint8_t *rank = nullptr;
    const uint32_t *run_end = nullptr;
    const std::atomic<size_t> *ready = nullptr;  // set: dist / sym are still arriving (forward_to_stream with overlap)
};

// slot < 0: the context's single staging buffer; otherwise the batch staging slot of that index
// overlap: the caller can work with a stream that is still arriving (ForwardResult::ready) and synchronises the stream afterwards
int forward_to_stream(dk_ctx *ctx, const uint8_t *d_text, size_t n, bool want_ctx_fields, ForwardResult *fr, int slot = -1, bool overlap = false) {
    hipStream_t st = ctx->stream;
    uint8_t *d_bwt = ctx->ws_alloc<uint8_t>(n);
    if (!d_bwt) return DK_E_NOMEM;
    {
        const size_t mark = ctx->ws_mark();
        uint32_t *d_sa = ctx->ws_alloc<uint32_t>(n);
        if (!d_sa) return DK_E_NOMEM;
        DK_TRY(bwt_forward_device(ctx, d_text, n, d_sa, d_bwt, &fr->origin));  // sets stats.ms_sa / ms_bwt
        ctx->ws_release(mark);
    }
    // the DC arrays take the place of the suffix sort's temporaries (only L survives the sort)
    uint32_t *d_dist = ctx->ws_alloc<uint32_t>(n);
    uint8_t *d_sym = ctx->ws_alloc<uint8_t>(n);
    uint8_t *d_rank = want_ctx_fields ? ctx->ws_alloc<uint8_t>(n) : nullptr;
    uint32_t *d_run_end = want_ctx_fields ? ctx->ws_alloc<uint32_t>(n) : nullptr;
    if (!d_dist || !d_sym || (want_ctx_fields && (!d_rank || !d_run_end))) return DK_E_NOMEM;
    Timer t3;
    DK_TRY(dc_encode_device(ctx, d_bwt, n, fr->init, d_dist, d_sym, d_rank, d_run_end, &fr->m));
    ctx->stats.ms_dc = t3.ms();
    Timer t4;
    const size_t m = fr->m;
    const size_t off_sym = 4 * m, off_rank = off_sym + ((m + 15) & ~size_t(15)), off_end = off_rank + ((m + 15) & ~size_t(15));
    char *stage;
    if (slot < 0) {
        DK_TRY(ctx->ensure_stage(off_end + 4 * m + 64));
        stage = ctx->h_stage;
    } else {
        DK_TRY(ctx->ensure_slot(static_cast<size_t>(slot), off_end + 4 * m + 64));
        stage = ctx->slots[static_cast<size_t>(slot)].h;
    }
    fr->ready = nullptr;
    if (DK_D2H_OVERLAP && overlap && !want_ctx_fields && m >= (size_t(1) << 21)) {
        // A large single block: the entropy stage starts on the first piece while the rest is on its way.  Every piece's two copies are
        // followed by a host function that moves the frontier (DcStream::ready); the stream is synchronised by the caller after coding.
        // If anything fails to enqueue, whatever was enqueued is waited for before the error is returned: its host functions point into
        // this context (d2h_marks, d2h_ready), which the next call reuses.
        constexpr size_t PIECES = 16;
        ctx->d2h_ready.store(0, std::memory_order_relaxed);
        ctx->d2h_marks.resize(PIECES);
        hipError_t e = hipSuccess;
        for (size_t c = 0; c < PIECES && e == hipSuccess; ++c) {
            const size_t k0 = m * c / PIECES, k1 = m * (c + 1) / PIECES;
            e = hipMemcpyAsync(stage + 4 * k0, d_dist + k0, 4 * (k1 - k0), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(stage + off_sym + k0, d_sym + k0, k1 - k0, hipMemcpyDeviceToHost, st);
            ctx->d2h_marks[c] = dk_ctx::D2hMark{&ctx->d2h_ready, k1};
            if (e == hipSuccess)
                e = hipLaunchHostFunc(st, [](void *p) {
                    auto *mk = static_cast<dk_ctx::D2hMark *>(p);
                    mk->frontier->store(mk->value, std::memory_order_release);
                }, &ctx->d2h_marks[c]);
        }
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st);
            ctx->d2h_ready.store(dk::DC_STREAM_POISON, std::memory_order_release);
            return ctx->fail(DK_E_HIP, "D2H of the distance stream: %s", hipGetErrorString(e));
        }
        ctx->stats.ms_d2h = t4.ms();  // time to enqueue; block_encode_common adds what it waits for the stream after coding
        fr->dist = reinterpret_cast<const uint32_t *>(stage);
        fr->sym = reinterpret_cast<const uint8_t *>(stage + off_sym);
        fr->ready = &ctx->d2h_ready;
        return DK_OK;
    }
    DK_HIP(ctx, hipMemcpyAsync(stage, d_dist, 4 * m, hipMemcpyDeviceToHost, st));
    DK_HIP(ctx, hipMemcpyAsync(stage + off_sym, d_sym, m, hipMemcpyDeviceToHost, st));
    if (want_ctx_fields) {
        DK_HIP(ctx, hipMemcpyAsync(stage + off_rank, d_rank, m, hipMemcpyDeviceToHost, st));
        DK_HIP(ctx, hipMemcpyAsync(stage + off_end, d_run_end, 4 * m, hipMemcpyDeviceToHost, st));
    }
    DK_HIP(ctx, hipStreamSynchronize(st));
    ctx->stats.ms_d2h = t4.ms();
    fr->dist = reinterpret_cast<const uint32_t *>(stage);
    fr->sym = reinterpret_cast<const uint8_t *>(stage + off_sym);
    if (want_ctx_fields) {
        fr->rank = reinterpret_cast<const uint8_t *>(stage + off_rank);
        fr->run_end = reinterpret_cast<const uint32_t *>(stage + off_end);
    }
    return DK_OK;
}

unsigned block_flags(const uint32_t init[256], size_t n) {
    unsigned present = 0;
    for (int c = 0; c < 256; ++c) present += init[c] < n ? 1u : 0u;
    return (init[255] < n ? DK_FLAG_HAS_FF : 0u) | (present == 1 ? DK_FLAG_SINGLE_SYMBOL : 0u);
}

int block_encode_common(dk_ctx *ctx, int model_id, const uint8_t *d_text, size_t n, uint8_t *out, size_t out_cap, size_t *out_len) {
    if (model_max_block(model_id) == 0) return ctx->fail(DK_E_MODEL, "unknown model id %d", model_id);
    if (n > model_max_block(model_id))
        return ctx->fail(DK_E_MODEL, "model %d cannot code blocks of %zu bytes without losing bits (limit %llu)", model_id, n,
                         static_cast<unsigned long long>(model_max_block(model_id)));
    ForwardResult fr;
    DK_TRY(forward_to_stream(ctx, d_text, n, dk::model_base(model_id) == DK_MODEL_RAWDC, &fr, -1, true));
    ctx->last_flags = block_flags(fr.init, n);
    Timer t;
    DcStream s;
    s.n = n; s.init = fr.init; s.dist = fr.dist; s.sym = fr.sym; s.rank = fr.rank; s.run_end = fr.run_end; s.m = fr.m; s.origin = fr.origin;
    s.ready = fr.ready;
    dk::set_preferred_numa(ctx->numa_node);
    int rc = encode_block_stream(model_id, s, out, out_cap, out_len);
    double ms_wait = 0.0;
    if (fr.ready) {  // (a coder that gave up early must not leave copies and host functions of this call behind)
        Timer tw;
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess && !rc) rc = DK_E_HIP;
        ms_wait = tw.ms();
        ctx->stats.ms_d2h += ms_wait;
    }
    ctx->stats.ms_entropy = t.ms() - ms_wait;
    ctx->stats.entropy_threads = static_cast<uint32_t>(dk::last_entropy_threads());
    ctx->stats.entropy_l3_group = dk::last_entropy_group();
    ctx->stats.entropy_l3_numa = static_cast<int16_t>(dk::last_entropy_group_numa());
    ctx->stats.gpu_numa = static_cast<int16_t>(ctx->numa_node);
    if (rc == DK_E_CAPACITY) return ctx->fail(rc, "output buffer of %zu bytes is too small", out_cap);
    if (rc) return ctx->fail(rc, "entropy stage failed (%d)", rc);
    return DK_OK;
}

int block_decode_common(dk_ctx *ctx, int model_id, const uint8_t *in, size_t in_len, size_t n, uint8_t *d_out) {
    if (dk::model_base(model_id) == DK_MODEL_RAWDC || model_max_block(model_id) == 0) return ctx->fail(DK_E_MODEL, "model %d cannot decode", model_id);
    hipStream_t st = ctx->stream;
    DK_TRY(ctx->ensure_stage(n + 64));
    uint8_t *h_bwt = reinterpret_cast<uint8_t *>(ctx->h_stage);
    uint32_t origin = 0;
    int single = 0;
    Timer t;
    int rc = decode_block_stream(model_id, in, in_len, n, h_bwt, &origin, &single, &ctx->last_consumed);
    ctx->stats.ms_entropy = t.ms();
    if (rc) return ctx->fail(rc, "stream does not decode (corrupt, truncated, wrong model/size, or a block containing byte 0xFF, "
                                 "which the reference format cannot represent without DK_MODEL_ANYBYTE: src/block/dc.rs:57-73)");
    Timer t2;
    uint8_t *d_bwt = ctx->ws_alloc<uint8_t>(n);
    if (!d_bwt) return DK_E_NOMEM;
    DK_HIP(ctx, hipMemcpyAsync(d_bwt, h_bwt, n, hipMemcpyHostToDevice, st));
    ctx->stats.ms_h2d = t2.ms();
    if (single) {
        // One-symbol block.  The reference mis-reads origin here (it skips the one sweep distance the encoder wrote) and
        // its bwt::decode then yields a single byte; the text is unambiguous, so return all n bytes.
        DK_HIP(ctx, hipMemcpyAsync(d_out, d_bwt, n, hipMemcpyDeviceToDevice, st));
        DK_HIP(ctx, hipStreamSynchronize(st));
        return DK_OK;
    }
    if (origin >= n) return ctx->fail(DK_E_STREAM, "decoded origin %u is outside the block", origin);
    Timer t3;
    DK_TRY(bwt_inverse_device(ctx, d_bwt, n, origin, d_out));
    ctx->stats.ms_ibwt = t3.ms();
    return DK_OK;
}

}  // namespace

extern "C" {

const char *dk_version(void) { return "dark_amd 0.1 (gfx950, HIP)"; }

}  // extern "C"

namespace {
int ctx_create(int purpose, int hip_device, size_t max_n, size_t max_blocks, dk_ctx **out) {
    if (!out || !good_ctx_size(purpose, max_n, max_blocks)) return DK_E_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return DK_E_NODEVICE;
    if (hip_device < 0 || hip_device >= count) return DK_E_NODEVICE;  // -1 would mean "CPU": there is no such backend
    dk_ctx *c = new (std::nothrow) dk_ctx();
    if (!c) return DK_E_NOMEM;
    c->device = hip_device;
    c->max_n = max_n;
    c->purpose = purpose;
    if (purpose == DK_CTX_DECODER) c->max_blocks = max_blocks;
    bool ok = hipSetDevice(hip_device) == hipSuccess && hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess;
    {   // the GPU's memory node: the host coder claims its last-level-cache group there first (entropy.cpp: l3_claim_order)
        char bdf[32] = {0};
        if (ok && hipDeviceGetPCIBusId(bdf, sizeof bdf, hip_device) == hipSuccess) {
            for (char *q = bdf; *q; ++q) *q = static_cast<char>(std::tolower(static_cast<unsigned char>(*q)));
            const std::string path = std::string("/sys/bus/pci/devices/") + bdf + "/numa_node";
            if (FILE *f = std::fopen(path.c_str(), "r")) {
                int node = -1;
                if (std::fscanf(f, "%d", &node) == 1) c->numa_node = node;
                std::fclose(f);
            }
        }
    }
    c->ws_size = purpose == DK_CTX_DECODER ? decoder_workspace_bytes(max_n, max_blocks) : workspace_bytes(max_n);
    ok = ok && hipMalloc(reinterpret_cast<void **>(&c->ws), c->ws_size) == hipSuccess;
    ok = ok && hipMalloc(reinterpret_cast<void **>(&c->d_mail), sizeof(dk::Mail)) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void **>(&c->h_mail), sizeof(dk::Mail), hipHostMallocDefault) == hipSuccess;
    // (on the context's own stream, and waited for: a memset on the null stream may still be on its way when the first call's kernels -- on a
    //  non-blocking stream, which the null stream does not order -- have written the mailbox: the first suffix sort of a fresh context then read an
    //  empty symbol histogram, one run in four of a test that starts with a tiny block)
    ok = ok && hipMemsetAsync(c->d_mail, 0, sizeof(dk::Mail), c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess;
    for (hipEvent_t &e : c->round_ev) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        dk_ctx_destroy(c);
        return DK_E_NOMEM;
    }
    *out = c;
    return DK_OK;
}
}  // namespace

extern "C" {

int dk_ctx_create(int hip_device, size_t max_n, dk_ctx **out) { return ctx_create(DK_CTX_FULL, hip_device, max_n, 0, out); }
int dk_ctx_create_decoder(int hip_device, size_t max_n, size_t max_blocks, dk_ctx **out) {
    return ctx_create(DK_CTX_DECODER, hip_device, max_n, max_blocks, out);
}
int dk_ctx_purpose(const dk_ctx *ctx) { return ctx ? ctx->purpose : DK_E_ARG; }
size_t dk_workspace_bytes(int purpose, size_t max_n, size_t max_blocks) {
    if (!good_ctx_size(purpose, max_n, max_blocks)) return 0;
    return purpose == DK_CTX_DECODER ? decoder_workspace_bytes(max_n, max_blocks) : workspace_bytes(max_n);
}

void dk_ctx_destroy(dk_ctx *c) {
    if (!c) return;
    // a batch left open (an error path that never reached dk_batch_finish): its coding threads still read the pinned staging slots
    // freed below -- join them first
    if (c->live_batch) (void)dk_batch_finish(c->live_batch);
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->round_ev) if (e) (void)hipEventDestroy(e);
    if (c->side_stream) { (void)hipStreamSynchronize(c->side_stream); (void)hipStreamDestroy(c->side_stream); }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->ws) (void)hipFree(c->ws);
    if (c->d_mail) (void)hipFree(c->d_mail);
    if (c->h_mail) (void)hipHostFree(c->h_mail);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    for (auto &sl : c->slots) if (sl.h) (void)hipHostFree(sl.h);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

size_t dk_capacity(const dk_ctx *ctx) { return ctx ? ctx->max_n : 0; }
size_t dk_last_consumed(const dk_ctx *ctx) { return ctx ? ctx->last_consumed : 0; }
unsigned dk_last_block_flags(const dk_ctx *ctx) { return ctx ? ctx->last_flags : 0; }
const char *dk_last_error(const dk_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

// ---- device-resident entry points ------------------------------------------------------------------------------------
int dk_dev_suffix_array(dk_ctx *ctx, const uint8_t *d_in, size_t n, uint32_t *d_sa_out) {
    DK_TRY(begin_call(ctx, "dk_dev_suffix_array"));
    ScopedCall sc(ctx);
    if (!d_in || !d_sa_out) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_n(ctx, n));
    Timer t;
    DK_TRY(suffix_array_device(ctx, d_in, n, d_sa_out));
    DK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stats.ms_sa = ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dk_dev_bwt_forward(dk_ctx *ctx, const uint8_t *d_in, size_t n, uint8_t *d_bwt_out, uint32_t *origin) {
    DK_TRY(begin_call(ctx, "dk_dev_bwt_forward"));
    ScopedCall sc(ctx);
    if (!d_in || !d_bwt_out || !origin) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_n(ctx, n));
    Timer t;
    uint32_t *d_sa = ctx->ws_alloc<uint32_t>(n);
    if (!d_sa) return DK_E_NOMEM;
    DK_TRY(bwt_forward_device(ctx, d_in, n, d_sa, d_bwt_out, origin));
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dk_dev_bwt_inverse(dk_ctx *ctx, const uint8_t *d_bwt, size_t n, uint32_t origin, uint8_t *d_out) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    if (!d_bwt || !d_out) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_n(ctx, n));
    if (origin >= n) return ctx->fail(DK_E_ARG, "origin %u outside the block of %zu bytes", origin, n);
    Timer t;
    DK_TRY(bwt_inverse_device(ctx, d_bwt, n, origin, d_out));
    ctx->stats.ms_ibwt = ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dk_dev_dc_encode(dk_ctx *ctx, const uint8_t *d_bwt, size_t n, uint32_t init[256], uint32_t *d_dist, uint8_t *d_sym, uint8_t *d_rank,
                     size_t *m) {
    DK_TRY(begin_call(ctx, "dk_dev_dc_encode"));
    ScopedCall sc(ctx);
    if (!d_bwt || !init || !d_dist || !d_sym || !m) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_n(ctx, n));
    Timer t;
    DK_TRY(dc_encode_device(ctx, d_bwt, n, init, d_dist, d_sym, d_rank, nullptr, m));
    ctx->stats.ms_dc = ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dk_dev_block_encode(dk_ctx *ctx, int model_id, const uint8_t *d_in, size_t n, uint8_t *out, size_t out_cap, size_t *out_len) {
    DK_TRY(begin_call(ctx, "dk_dev_block_encode"));
    ScopedCall sc(ctx);
    if (!d_in || !out || !out_len) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_n(ctx, n));
    Timer t;
    ctx->stats.ms_h2d = 0;
    int rc = block_encode_common(ctx, model_id, d_in, n, out, out_cap, out_len);
    ctx->stats.ms_total = t.ms();
    return rc;
}

int dk_dev_block_decode(dk_ctx *ctx, int model_id, const uint8_t *in, size_t in_len, size_t n, uint8_t *d_out) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    if (!in || !d_out) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_n(ctx, n));
    Timer t;
    int rc = block_decode_common(ctx, model_id, in, in_len, n, d_out);
    ctx->stats.ms_total = t.ms();
    return rc;
}

// Batch of independent blocks on one GPU: the device stages run block after block on the context's stream while a pool of host
// threads codes the distance streams of the blocks already done (the "one block per core, pipelined against the GPU work of
// the next block" deployment of SURVEY.md section 7.8).  Every out[i] is byte-identical to a dk_dev_block_encode of block i.
// Streaming form: dk_batch_begin starts the coding threads, dk_batch_push runs the device stages of one more block on the calling
// thread (it waits while every staging slot is busy) and queues its coding, dk_batch_finish waits for the coders.
}  // extern "C"

struct dk_batch {
    dk_ctx *ctx = nullptr;
    int model_id = 0;
    struct Job { size_t block; int slot; ForwardResult fr; size_t n; uint8_t *out; size_t cap; size_t *out_len; };
    std::mutex mu;
    std::condition_variable cv_job, cv_slot;
    std::deque<Job> queue;
    std::vector<int> free_slots;
    std::vector<size_t> slot_refs;  // jobs still reading each staging slot (a packed push queues several on one slot)
    std::vector<std::thread> pool;
    bool done = false;
    size_t pushed = 0;
    int first_rc = DK_OK;
    size_t first_bad = 0;
    void worker() {
        for (;;) {
            Job job;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_job.wait(lk, [&] { return done || !queue.empty(); });
                if (queue.empty()) return;
                job = queue.front();
                queue.pop_front();
            }
            DcStream s;
            s.n = job.n; s.init = job.fr.init; s.dist = job.fr.dist; s.sym = job.fr.sym; s.rank = job.fr.rank;
            s.run_end = job.fr.run_end; s.m = job.fr.m; s.origin = job.fr.origin;
            const int rc = encode_block_stream(model_id, s, job.out, job.cap, job.out_len, 1);
            {
                std::lock_guard<std::mutex> lk(mu);
                if (rc != DK_OK && first_rc == DK_OK) { first_rc = rc; first_bad = job.block; }
                if (--slot_refs[static_cast<size_t>(job.slot)] == 0) free_slots.push_back(job.slot);
            }
            cv_slot.notify_one();
        }
    }
};

extern "C" {

}  // extern "C"

// dk_batch_begin for the entry points that are built on it: `entry` is the name a decoder context's refusal carries
static int batch_begin(dk_ctx *ctx, int model_id, int host_threads, dk_batch **out, const char *entry) {
    DK_TRY(begin_call(ctx, entry));
    if (!out) return ctx->fail(DK_E_ARG, "null pointer");
    *out = nullptr;
    if (model_max_block(model_id) == 0) return ctx->fail(DK_E_MODEL, "unknown model id %d", model_id);
    dk_batch *b = new (std::nothrow) dk_batch();
    if (!b) return DK_E_NOMEM;
    b->ctx = ctx;
    b->model_id = model_id;
    const size_t workers = static_cast<size_t>(std::max(1, host_threads));
    for (size_t k = 0; k < workers + 1; ++k) b->free_slots.push_back(static_cast<int>(k));
    b->slot_refs.assign(workers + 1, 0);
    for (size_t w = 0; w < workers; ++w) b->pool.emplace_back([b] { b->worker(); });
    ctx->live_batch = b;
    *out = b;
    return DK_OK;
}

extern "C" {

int dk_batch_begin(dk_ctx *ctx, int model_id, int host_threads, dk_batch **out) { return batch_begin(ctx, model_id, host_threads, out, "dk_batch_begin"); }

int dk_batch_push(dk_batch *b, const uint8_t *d_in, size_t n, uint8_t *out, size_t out_cap, size_t *out_len) {
    if (!b) return DK_E_ARG;
    dk_ctx *ctx = b->ctx;
    if (!d_in || !out || !out_len) return ctx->fail(DK_E_ARG, "null pointer in block %zu", b->pushed);
    DK_TRY(check_n(ctx, n));
    if (n > model_max_block(b->model_id)) return ctx->fail(DK_E_MODEL, "model %d cannot code a block of %zu bytes", b->model_id, n);
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(DK_E_HIP, "hipSetDevice(%d) failed", ctx->device);
    int slot;
    {
        std::unique_lock<std::mutex> lk(b->mu);
        b->cv_slot.wait(lk, [&] { return !b->free_slots.empty(); });
        slot = b->free_slots.back();
        b->free_slots.pop_back();
    }
    dk_batch::Job job;
    job.block = b->pushed++;
    job.slot = slot;
    job.n = n; job.out = out; job.cap = out_cap; job.out_len = out_len;
    ctx->ws_reset();
    const int rc = forward_to_stream(ctx, d_in, n, dk::model_base(b->model_id) == DK_MODEL_RAWDC, &job.fr, slot);
    if (ctx->profiling) ctx->prof_collect();
    if (rc != DK_OK) {
        std::lock_guard<std::mutex> lk(b->mu);
        b->free_slots.push_back(slot);
        return rc;
    }
    {
        std::lock_guard<std::mutex> lk(b->mu);
        b->slot_refs[static_cast<size_t>(slot)] = 1;
        b->queue.push_back(job);
    }
    b->cv_job.notify_one();
    return DK_OK;
}

int dk_batch_finish(dk_batch *b) {
    if (!b) return DK_E_ARG;
    {
        std::lock_guard<std::mutex> lk(b->mu);
        b->done = true;
    }
    b->cv_job.notify_all();
    for (auto &th : b->pool) th.join();
    b->ctx->live_batch = nullptr;
    int rc = b->first_rc;
    if (rc != DK_OK) rc = b->ctx->fail(rc, "entropy stage of block %zu failed (%d)", b->first_bad, rc);
    delete b;
    return rc;
}

}  // extern "C"

// ---- packed forward path (csrc/packed.hip) ----------------------------------------------------------------------
namespace {

// Rounds of the segmented suffix sort before the blocks still unresolved leave the pack for the single-block path.  With k symbols in the
// initial key (6 to 8 for text-sized alphabets) R rounds resolve common prefixes of k * 2^R symbols.  tools/packed_throughput.py measured
// at most 10 rounds on its text shapes (wiki_like; english_like 2, random bytes 0), so 12 leaves two rounds of headroom.
constexpr int PACKED_MAX_ROUNDS = 12;

}  // namespace

// L of every block into d_bwt and the origins into h_origin (host, count): one segmented pass, then the guard's blocks one by one.
// d_sa (may be null): the suffix arrays too, from the same pass (dk_dev_suffix_array_packed); then d_bwt / d_origin may both be null.
// d_phi (may be null, only with d_sa): Phi of the pack for the LCP pass -- from the sort's rank, and for the guard's blocks from their suffix arrays.
int dk::packed_forward(dk_ctx *ctx, const uint8_t *d_in, const std::vector<uint32_t> &off, const uint32_t *d_off, uint8_t *d_bwt, uint32_t *d_origin,
                       std::vector<std::pair<size_t, uint32_t>> *fixed, uint32_t *d_sa, uint32_t *d_phi) {
    hipStream_t st = ctx->stream;
    const size_t count = off.size() - 1, total = off.back();
    Timer t;
    ctx->stats.sa_route = 0;
    uint32_t *d_guard = ctx->ws_alloc<uint32_t>(count);
    if (!d_guard) return DK_E_NOMEM;
    size_t unresolved = 0;
    // (tuning build: DK_PACKED_ROUNDS lowers the limit, clamped to [0, PACKED_MAX_ROUNDS] -- a test hook that sends blocks through the guard)
    const int max_rounds = std::max(0, std::min(PACKED_MAX_ROUNDS, DK_KNOB("DK_PACKED_ROUNDS", PACKED_MAX_ROUNDS)));
    if (d_sa) DK_TRY(packed_sa_device(ctx, d_in, d_off, count, total, d_sa, d_bwt, d_origin, d_guard, max_rounds, &unresolved, d_phi));
    else DK_TRY(packed_bwt_device(ctx, d_in, d_off, count, total, d_bwt, d_origin, d_guard, max_rounds, &unresolved));
    fixed->clear();
    if (unresolved) {
        std::vector<uint32_t> guard(count);
        DK_HIP(ctx, hipMemcpyAsync(guard.data(), d_guard, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        DK_HIP(ctx, hipStreamSynchronize(st));
        const uint32_t rounds = ctx->stats.rounds;
        for (size_t i = 0; i < count; ++i) {
            if (!guard[i]) continue;
            const size_t mark = ctx->ws_mark(), n = off[i + 1] - off[i];
            uint32_t origin = 0;
            if (d_sa) {
                // The complete suffix array is wanted: not bwt_forward_device, whose L-first route never fills one.  The block's stretches of
                // the text and of the output have any alignment, as the caller's own buffers of dk_dev_suffix_array do: every 16-byte access
                // of the single-block sort and of k_bwt_gather to either checks the address first and goes element by element otherwise.
                uint32_t *d_one = d_sa + off[i];
                DK_TRY(suffix_array_device(ctx, d_in + off[i], n, d_one));
                if (d_bwt) DK_TRY(bwt_gather_device(ctx, d_in + off[i], d_one, n, d_bwt + off[i], &origin));
                if (d_phi) DK_TRY(lcp_phi_block_device(ctx, d_sa, d_off, count, off[i], off[i + 1], d_phi));
            } else {
                uint32_t *d_one = ctx->ws_alloc<uint32_t>(n);
                if (!d_one) return DK_E_NOMEM;
                DK_TRY(bwt_forward_device(ctx, d_in + off[i], n, d_one, d_bwt + off[i], &origin));
            }
            fixed->emplace_back(i, origin);
            ctx->ws_release(mark);
        }
        ctx->stats.rounds = rounds;
        ctx->stats.sa_route = DK_ROUTE_PACKED_GUARD;
    }
    DK_HIP(ctx, hipStreamSynchronize(st));
    ctx->stats.ms_sa = t.ms();
    ctx->stats.ms_bwt = 0;
    return DK_OK;
}

extern "C" {

int dk_dev_bwt_forward_packed(dk_ctx *ctx, const uint8_t *d_in, size_t count, const size_t *n, uint8_t *d_bwt_out, uint32_t *origin) {
    DK_TRY(begin_call(ctx, "dk_dev_bwt_forward_packed"));
    ScopedCall sc(ctx);
    if (!d_in || !n || !d_bwt_out || !origin) return ctx->fail(DK_E_ARG, "null pointer");
    Layout lay(count, n);
    DK_TRY(lay.check(ctx));
    std::vector<std::pair<size_t, uint32_t>> fixed;
    Upload up(ctx);
    Timer t;
    hipStream_t st = ctx->stream;
    const uint32_t *d_off = lay.device(up);
    uint32_t *d_origin = ctx->ws_alloc<uint32_t>(count);
    if (!d_off || !d_origin) return up.failed();
    DK_TRY(packed_forward(ctx, d_in, lay.off(), d_off, d_bwt_out, d_origin, &fixed));
    up.synchronised();  // (packed_forward ends with a wait)
    DK_HIP(ctx, hipMemcpyAsync(origin, d_origin, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DK_HIP(ctx, hipStreamSynchronize(st));
    for (const auto &f : fixed) origin[f.first] = f.second;
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dk_dev_suffix_array_packed(dk_ctx *ctx, const uint8_t *d_in, size_t count, const size_t *n, uint32_t *d_sa_out, uint8_t *d_bwt_out,
                               uint32_t *origin) {
    DK_TRY(begin_call(ctx, "dk_dev_suffix_array_packed"));
    ScopedCall sc(ctx);
    if (!d_in || !n || !d_sa_out) return ctx->fail(DK_E_ARG, "null pointer");
    if ((d_bwt_out == nullptr) != (origin == nullptr)) return ctx->fail(DK_E_ARG, "d_bwt_out and origin go together: both or neither");
    Layout lay(count, n);
    DK_TRY(lay.check(ctx));
    std::vector<std::pair<size_t, uint32_t>> fixed;
    Upload up(ctx);
    Timer t;
    hipStream_t st = ctx->stream;
    const uint32_t *d_off = lay.device(up);
    uint32_t *d_origin = d_bwt_out ? ctx->ws_alloc<uint32_t>(count) : nullptr;
    if (!d_off || (d_bwt_out && !d_origin)) return up.failed();
    DK_TRY(packed_forward(ctx, d_in, lay.off(), d_off, d_bwt_out, d_origin, &fixed, d_sa_out));
    up.synchronised();  // (packed_forward ends with a wait)
    if (d_bwt_out) {
        DK_HIP(ctx, hipMemcpyAsync(origin, d_origin, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        DK_HIP(ctx, hipStreamSynchronize(st));
        for (const auto &f : fixed) origin[f.first] = f.second;
    }
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dk_dev_dc_encode_packed(dk_ctx *ctx, const uint8_t *d_bwt, size_t count, const size_t *n, uint32_t *init, uint32_t *d_dist, uint8_t *d_sym,
                            uint8_t *d_rank, size_t *m) {
    DK_TRY(begin_call(ctx, "dk_dev_dc_encode_packed"));
    ScopedCall sc(ctx);
    if (!d_bwt || !n || !init || !d_dist || !d_sym || !m) return ctx->fail(DK_E_ARG, "null pointer");
    Layout lay(count, n);
    DK_TRY(lay.check(ctx));
    Upload up(ctx);
    Timer t;
    hipStream_t st = ctx->stream;
    // read-back block: m | flags | rb (count + 1) | init (count x 256)
    const size_t words = 3 * count + 1 + 256 * count;
    const uint32_t *d_off = lay.device(up);
    uint32_t *d_res = ctx->ws_alloc<uint32_t>(words);
    if (!d_off || !d_res) return up.failed();
    DK_TRY(packed_dc_device(ctx, d_bwt, d_off, count, lay.total(), false, d_dist, d_sym, d_rank, nullptr, d_res, d_res + count, d_res + 2 * count,
                            d_res + 3 * count + 1));
    std::vector<uint32_t> res(words);
    DK_HIP(ctx, hipMemcpyAsync(res.data(), d_res, words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DK_TRY(up.sync());
    for (size_t i = 0; i < count; ++i) m[i] = res[i];
    std::memcpy(init, res.data() + 3 * count + 1, 256 * count * sizeof(uint32_t));
    ctx->stats.ms_dc = ctx->stats.ms_total = t.ms();
    return DK_OK;
}

}  // extern "C"

namespace {

// device stages of a pack for an open batch: everything up to the distance streams in staging slot `slot`, then one coding job per block
int push_packed_body(dk_batch *b, int slot, const uint8_t *d_in, const Layout &lay, uint8_t *const *out, const size_t *out_cap, size_t *out_len,
                     unsigned *flags) {
    dk_ctx *ctx = b->ctx;
    hipStream_t st = ctx->stream;
    const std::vector<uint32_t> &off = lay.off();
    const size_t count = lay.count(), total = lay.total();
    std::vector<std::pair<size_t, uint32_t>> fixed;
    Upload up(ctx);
    const bool want = dk::model_base(b->model_id) == DK_MODEL_RAWDC;
    // read-back block: origin | m | flags | rb (count + 1) | init (count x 256)
    const size_t words = 4 * count + 1 + 256 * count;
    const uint32_t *d_off = lay.device(up);
    uint32_t *d_res = ctx->ws_alloc<uint32_t>(words);
    uint8_t *d_bwt = ctx->ws_alloc<uint8_t>(total);
    if (!d_off || !d_res || !d_bwt) return up.failed();
    {
        const size_t mark = ctx->ws_mark();
        DK_TRY(packed_forward(ctx, d_in, off, d_off, d_bwt, d_res, &fixed));
        up.synchronised();  // (packed_forward ends with a wait)
        ctx->ws_release(mark);
    }
    uint32_t *d_dist = ctx->ws_alloc<uint32_t>(total);
    uint8_t *d_sym = ctx->ws_alloc<uint8_t>(total);
    uint8_t *d_rank = want ? ctx->ws_alloc<uint8_t>(total) : nullptr;
    uint32_t *d_run_end = want ? ctx->ws_alloc<uint32_t>(total) : nullptr;
    if (!d_dist || !d_sym || (want && (!d_rank || !d_run_end))) return DK_E_NOMEM;
    Timer t3;
    uint32_t *d_m = d_res + count, *d_flags = d_res + 2 * count, *d_rb = d_res + 3 * count, *d_init = d_res + 4 * count + 1;
    DK_TRY(packed_dc_device(ctx, d_bwt, d_off, count, total, true, d_dist, d_sym, d_rank, d_run_end, d_m, d_flags, d_rb, d_init));
    std::vector<uint32_t> res(words);
    DK_HIP(ctx, hipMemcpyAsync(res.data(), d_res, words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DK_HIP(ctx, hipStreamSynchronize(st));
    ctx->stats.ms_dc = t3.ms();
    for (const auto &f : fixed) res[f.first] = f.second;
    const uint32_t *h_origin = res.data(), *h_m = res.data() + count, *h_flags = res.data() + 2 * count, *h_rb = res.data() + 3 * count;
    const uint32_t *h_init = res.data() + 4 * count + 1;
    Timer t4;
    const size_t m = h_rb[count];
    const size_t off_sym = 4 * m, off_rank = off_sym + ((m + 15) & ~size_t(15)), off_end = off_rank + ((m + 15) & ~size_t(15));
    DK_TRY(ctx->ensure_slot(static_cast<size_t>(slot), off_end + 4 * m + 64));
    char *stage = ctx->slots[static_cast<size_t>(slot)].h;
    DK_HIP(ctx, hipMemcpyAsync(stage, d_dist, 4 * m, hipMemcpyDeviceToHost, st));
    DK_HIP(ctx, hipMemcpyAsync(stage + off_sym, d_sym, m, hipMemcpyDeviceToHost, st));
    if (want) {
        DK_HIP(ctx, hipMemcpyAsync(stage + off_rank, d_rank, m, hipMemcpyDeviceToHost, st));
        DK_HIP(ctx, hipMemcpyAsync(stage + off_end, d_run_end, 4 * m, hipMemcpyDeviceToHost, st));
    }
    DK_HIP(ctx, hipStreamSynchronize(st));
    ctx->stats.ms_d2h = t4.ms();
    ctx->stats.dc_runs = m;
    std::vector<dk_batch::Job> jobs(count);
    for (size_t i = 0; i < count; ++i) {
        dk_batch::Job &job = jobs[i];
        job.slot = slot;
        job.n = off[i + 1] - off[i]; job.out = out[i]; job.cap = out_cap[i]; job.out_len = &out_len[i];
        std::memcpy(job.fr.init, h_init + 256 * i, sizeof job.fr.init);
        job.fr.origin = h_origin[i];
        job.fr.m = h_m[i];
        job.fr.dist = reinterpret_cast<const uint32_t *>(stage) + h_rb[i];
        job.fr.sym = reinterpret_cast<const uint8_t *>(stage + off_sym) + h_rb[i];
        if (want) {
            job.fr.rank = reinterpret_cast<const uint8_t *>(stage + off_rank) + h_rb[i];
            job.fr.run_end = reinterpret_cast<const uint32_t *>(stage + off_end) + h_rb[i];
        }
        if (flags) flags[i] = h_flags[i];
    }
    {
        std::lock_guard<std::mutex> lk(b->mu);
        for (auto &job : jobs) {
            job.block = b->pushed++;
            b->queue.push_back(job);
        }
        b->slot_refs[static_cast<size_t>(slot)] = count;
    }
    b->cv_job.notify_all();
    return DK_OK;
}

}  // namespace

extern "C" {

int dk_batch_push_packed(dk_batch *b, const uint8_t *d_in, size_t count, const size_t *n, uint8_t *const *out, const size_t *out_cap,
                         size_t *out_len, unsigned *flags) {
    if (!b) return DK_E_ARG;
    dk_ctx *ctx = b->ctx;
    if (!d_in || !n || !out || !out_cap || !out_len) return ctx->fail(DK_E_ARG, "null pointer");
    Layout lay(count, n);
    DK_TRY(lay.check(ctx));
    for (size_t i = 0; i < count; ++i) {
        if (!out[i]) return ctx->fail(DK_E_ARG, "null output for block %zu of the pack", i);
        if (n[i] > model_max_block(b->model_id)) return ctx->fail(DK_E_MODEL, "model %d cannot code a block of %zu bytes", b->model_id, n[i]);
    }
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(DK_E_HIP, "hipSetDevice(%d) failed", ctx->device);
    int slot;
    {
        std::unique_lock<std::mutex> lk(b->mu);
        b->cv_slot.wait(lk, [&] { return !b->free_slots.empty(); });
        slot = b->free_slots.back();
        b->free_slots.pop_back();
    }
    ctx->ws_reset();
    Timer t;
    const int rc = push_packed_body(b, slot, d_in, lay, out, out_cap, out_len, flags);
    ctx->stats.ms_total = t.ms();
    if (ctx->profiling) ctx->prof_collect();
    if (rc != DK_OK) {
        std::lock_guard<std::mutex> lk(b->mu);
        b->free_slots.push_back(slot);
        return rc;
    }
    return DK_OK;
}

int dk_dev_packed_encode(dk_ctx *ctx, int model_id, const uint8_t *d_in, size_t count, const size_t *n, uint8_t *const *out, const size_t *out_cap,
                         size_t *out_len, unsigned *flags, int host_threads) {
    if (!ctx) return DK_E_ARG;
    Timer t;
    dk_batch *b = nullptr;
    const int threads = static_cast<int>(std::max<size_t>(1, std::min<size_t>(static_cast<size_t>(std::max(1, host_threads)), std::max<size_t>(1, count))));
    DK_TRY(batch_begin(ctx, model_id, threads, &b, "dk_dev_packed_encode"));
    const int rc = dk_batch_push_packed(b, d_in, count, n, out, out_cap, out_len, flags);
    const std::string err = ctx->err;
    const int rc2 = dk_batch_finish(b);
    if (rc != DK_OK) ctx->err = err;  // the push's text, not the finish's
    ctx->stats.ms_total = t.ms();
    return rc != DK_OK ? rc : rc2;
}

int dk_dev_batch_encode(dk_ctx *ctx, int model_id, size_t count, const uint8_t *const *d_in, const size_t *n, uint8_t *const *out,
                        const size_t *out_cap, size_t *out_len, int host_threads) {
    if (!ctx) return DK_E_ARG;
    if (ctx->purpose == DK_CTX_DECODER) return begin_call(ctx, "dk_dev_batch_encode");
    if (!d_in || !n || !out || !out_cap || !out_len || count == 0) { ctx->err.clear(); return ctx->fail(DK_E_ARG, "null pointer or empty batch"); }
    Timer t;
    dk_batch *b = nullptr;
    DK_TRY(batch_begin(ctx, model_id, std::max(1, std::min<int>(host_threads, static_cast<int>(count))), &b, "dk_dev_batch_encode"));
    int rc = DK_OK;
    for (size_t i = 0; i < count && rc == DK_OK; ++i) rc = dk_batch_push(b, d_in[i], n[i], out[i], out_cap[i], &out_len[i]);
    const int rc2 = dk_batch_finish(b);
    ctx->stats.ms_total = t.ms();
    return rc != DK_OK ? rc : rc2;
}

// Inverse of dk_dev_batch_encode: host threads decode the streams (range decoder + dc::decode, serial per block) into pinned
// slots while the calling thread uploads finished BWTs and runs the inverse BWT on the GPU.
int dk_dev_batch_decode(dk_ctx *ctx, int model_id, size_t count, const uint8_t *const *in, const size_t *in_len, const size_t *n,
                        uint8_t *const *d_out, int host_threads) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    if (!in || !in_len || !n || !d_out || count == 0) return ctx->fail(DK_E_ARG, "null pointer or empty batch");
    if (dk::model_base(model_id) == DK_MODEL_RAWDC || model_max_block(model_id) == 0) return ctx->fail(DK_E_MODEL, "model %d cannot decode", model_id);
    size_t max_n = 0;
    for (size_t i = 0; i < count; ++i) {
        if (!in[i] || !d_out[i]) return ctx->fail(DK_E_ARG, "null pointer in block %zu", i);
        DK_TRY(check_n(ctx, n[i]));
        max_n = std::max(max_n, n[i]);
    }
    Timer t;
    const size_t workers = static_cast<size_t>(std::max(1, std::min<int>(host_threads, static_cast<int>(count))));
    const size_t nslots = workers + 1;
    for (size_t k = 0; k < nslots; ++k) DK_TRY(ctx->ensure_slot(k, max_n + 64));
    struct Done { size_t block; int slot; uint32_t origin; int single; int rc; };
    std::mutex mu;
    std::condition_variable cv_slot, cv_done;
    std::vector<int> free_slots;
    for (size_t k = 0; k < nslots; ++k) free_slots.push_back(static_cast<int>(k));
    std::deque<Done> finished;
    size_t next_block = 0;
    auto worker = [&] {
        for (;;) {
            size_t block;
            int slot;
            {
                std::unique_lock<std::mutex> lk(mu);
                if (next_block >= count) return;
                block = next_block++;
                cv_slot.wait(lk, [&] { return !free_slots.empty(); });
                slot = free_slots.back();
                free_slots.pop_back();
            }
            Done d{block, slot, 0, 0, DK_OK};
            d.rc = decode_block_stream(model_id, in[block], in_len[block], n[block], reinterpret_cast<uint8_t *>(ctx->slots[slot].h), &d.origin,
                                       &d.single);
            {
                std::lock_guard<std::mutex> lk(mu);
                finished.push_back(d);
            }
            cv_done.notify_one();
        }
    };
    std::vector<std::thread> pool;
    for (size_t w = 0; w < workers; ++w) pool.emplace_back(worker);
    int rc = DK_OK;
    size_t bad_block = 0;
    hipStream_t st = ctx->stream;
    for (size_t done_count = 0; done_count < count; ++done_count) {
        Done d;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv_done.wait(lk, [&] { return !finished.empty(); });
            d = finished.front();
            finished.pop_front();
        }
        if (rc == DK_OK && d.rc != DK_OK) { rc = d.rc; bad_block = d.block; }
        if (rc == DK_OK) {
            ctx->ws_reset();
            const size_t nb = n[d.block];
            uint8_t *d_bwt = ctx->ws_alloc<uint8_t>(nb);
            hipError_t e = d_bwt ? hipMemcpyAsync(d_bwt, ctx->slots[d.slot].h, nb, hipMemcpyHostToDevice, st) : hipErrorOutOfMemory;
            if (e == hipSuccess) e = hipStreamSynchronize(st);  // the slot may be refilled from here on
            if (e != hipSuccess) { rc = ctx->fail(DK_E_HIP, "batch decode upload: %s", hipGetErrorString(e)); }
            {
                std::lock_guard<std::mutex> lk(mu);
                free_slots.push_back(d.slot);
            }
            cv_slot.notify_one();
            if (rc == DK_OK) {
                if (d.single) {
                    if (hipMemcpyAsync(d_out[d.block], d_bwt, nb, hipMemcpyDeviceToDevice, st) != hipSuccess) rc = ctx->fail(DK_E_HIP, "copy failed");
                } else if (d.origin >= nb) {
                    rc = ctx->fail(DK_E_STREAM, "decoded origin %u is outside block %zu", d.origin, d.block);
                } else {
                    rc = bwt_inverse_device(ctx, d_bwt, nb, d.origin, d_out[d.block]);
                }
            }
        } else {
            std::lock_guard<std::mutex> lk(mu);
            free_slots.push_back(d.slot);
            cv_slot.notify_one();
        }
    }
    for (auto &th : pool) th.join();
    (void)hipStreamSynchronize(st);
    ctx->stats.ms_total = t.ms();
    if (rc != DK_OK && ctx->err.empty()) return ctx->fail(rc, "stream of block %zu does not decode (%d)", bad_block, rc);
    return rc;
}

// ---- packed inverse (csrc/bwt.hip packed_ibwt_device) ------------------------------------------------------------
int dk_dev_bwt_inverse_packed(dk_ctx *ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const uint32_t *origin, uint8_t *d_out) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    if (!d_bwt || !n || !origin || !d_out) return ctx->fail(DK_E_ARG, "null pointer");
    Layout lay(count, n);
    DK_TRY(lay.check(ctx));
    DK_TRY(lay.check_origins(ctx, origin));
    Timer t;
    DK_TRY(packed_ibwt_device(ctx, d_bwt, lay.off(), origin, d_out));
    ctx->stats.ms_ibwt = ctx->stats.ms_total = t.ms();
    return DK_OK;
}

// Host threads decode every stream of the pack into ONE pinned slot (block i at off_i), then one upload and one packed inverse.
int dk_dev_packed_decode(dk_ctx *ctx, int model_id, size_t count, const uint8_t *const *in, const size_t *in_len, const size_t *n,
                         uint8_t *d_out, int host_threads) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    if (!in || !in_len || !n || !d_out) return ctx->fail(DK_E_ARG, "null pointer");
    if (dk::model_base(model_id) == DK_MODEL_RAWDC || model_max_block(model_id) == 0) return ctx->fail(DK_E_MODEL, "model %d cannot decode", model_id);
    Layout lay(count, n);
    DK_TRY(lay.check(ctx));
    const std::vector<uint32_t> &off = lay.off();
    for (size_t i = 0; i < count; ++i)
        if (!in[i]) return ctx->fail(DK_E_ARG, "null stream for block %zu of the pack", i);
    Timer t;
    const size_t total = lay.total();
    DK_TRY(ctx->ensure_slot(0, total + 64));
    uint8_t *h_bwt = reinterpret_cast<uint8_t *>(ctx->slots[0].h);
    std::vector<uint32_t> origin(count);
    std::vector<int> rcs(count, DK_OK);
    std::atomic<size_t> next{0};
    auto worker = [&] {
        for (size_t i; (i = next.fetch_add(1, std::memory_order_relaxed)) < count;) {
            int single = 0;
            rcs[i] = decode_block_stream(model_id, in[i], in_len[i], n[i], h_bwt + off[i], &origin[i], &single);
            // One-symbol block (its origin is not read: DESIGN.md quirks).  L = c^n is inverted with origin n - 1, which gives c^n back.
            if (rcs[i] == DK_OK && single) origin[i] = static_cast<uint32_t>(n[i] - 1);
        }
    };
    const size_t workers = static_cast<size_t>(std::max(1, std::min<int>(host_threads, static_cast<int>(count))));
    std::vector<std::thread> pool;
    for (size_t w = 0; w < workers; ++w) pool.emplace_back(worker);
    for (auto &th : pool) th.join();
    ctx->stats.ms_entropy = t.ms();
    for (size_t i = 0; i < count; ++i) {
        if (rcs[i] != DK_OK)
            return ctx->fail(DK_E_STREAM, "stream of block %zu of the pack does not decode (%d: corrupt, truncated, wrong model/size, or a block "
                                          "containing byte 0xFF)", i, rcs[i]);
        if (origin[i] >= n[i]) return ctx->fail(DK_E_STREAM, "decoded origin %u is outside block %zu of the pack", origin[i], i);
    }
    Timer t2;
    uint8_t *d_bwt = ctx->ws_alloc<uint8_t>(total);
    if (!d_bwt) return DK_E_NOMEM;
    DK_HIP(ctx, hipMemcpyAsync(d_bwt, h_bwt, total, hipMemcpyHostToDevice, ctx->stream));
    ctx->stats.ms_h2d = t2.ms();
    Timer t3;
    DK_TRY(packed_ibwt_device(ctx, d_bwt, off, origin.data(), d_out));
    ctx->stats.ms_ibwt = t3.ms();
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

// ---- host-pointer entry points: stage in, run the device path, stage out ---------------------------------------------
int dk_suffix_array(dk_ctx *ctx, const uint8_t *in, size_t n, uint32_t *sa_out) {
    DK_TRY(begin_call(ctx, "dk_suffix_array"));
    ScopedCall sc(ctx);
    Upload up(ctx);
    if (!in || !sa_out) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_n(ctx, n));
    Timer t;
    uint8_t *d_text = ctx->ws_alloc<uint8_t>(n);
    uint32_t *d_sa = ctx->ws_alloc<uint32_t>(n);
    if (!d_text || !d_sa) return DK_E_NOMEM;
    DK_TRY(up.copy(d_text, in, n, "text"));
    DK_TRY(suffix_array_device(ctx, d_text, n, d_sa));
    DK_HIP(ctx, hipMemcpyAsync(sa_out, d_sa, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dk_suffix_array_packed(dk_ctx *ctx, const uint8_t *in, size_t count, const size_t *n, uint32_t *sa_out) {
    DK_TRY(begin_call(ctx, "dk_suffix_array_packed"));
    ScopedCall sc(ctx);
    if (!in || !n || !sa_out) return ctx->fail(DK_E_ARG, "null pointer");
    Layout lay(count, n);
    DK_TRY(lay.check(ctx));
    std::vector<std::pair<size_t, uint32_t>> fixed;
    Upload up(ctx);
    Timer t;
    hipStream_t st = ctx->stream;
    const size_t total = lay.total();
    const uint8_t *d_text = up.stage(in, total, "text");
    uint32_t *d_sa = ctx->ws_alloc<uint32_t>(total);
    const uint32_t *d_off = lay.device(up);
    if (!d_text || !d_sa || !d_off) return up.failed();
    DK_TRY(packed_forward(ctx, d_text, lay.off(), d_off, nullptr, nullptr, &fixed, d_sa));
    DK_HIP(ctx, hipMemcpyAsync(sa_out, d_sa, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dk_bwt_forward(dk_ctx *ctx, const uint8_t *in, size_t n, uint8_t *bwt_out, uint32_t *origin) {
    DK_TRY(begin_call(ctx, "dk_bwt_forward"));
    ScopedCall sc(ctx);
    Upload up(ctx);
    if (!in || !bwt_out || !origin) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_n(ctx, n));
    Timer t;
    uint8_t *d_text = ctx->ws_alloc<uint8_t>(n);
    uint8_t *d_bwt = ctx->ws_alloc<uint8_t>(n);
    uint32_t *d_sa = ctx->ws_alloc<uint32_t>(n);
    if (!d_text || !d_bwt || !d_sa) return DK_E_NOMEM;
    DK_TRY(up.copy(d_text, in, n, "text"));
    DK_TRY(bwt_forward_device(ctx, d_text, n, d_sa, d_bwt, origin));
    DK_HIP(ctx, hipMemcpyAsync(bwt_out, d_bwt, n, hipMemcpyDeviceToHost, ctx->stream));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dk_bwt_inverse(dk_ctx *ctx, const uint8_t *bwt, size_t n, uint32_t origin, uint8_t *out) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    Upload up(ctx);
    if (!bwt || !out) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_n(ctx, n));
    if (origin >= n) return ctx->fail(DK_E_ARG, "origin %u outside the block of %zu bytes", origin, n);
    Timer t;
    uint8_t *d_bwt = ctx->ws_alloc<uint8_t>(n);
    uint8_t *d_out = ctx->ws_alloc<uint8_t>(n);
    if (!d_bwt || !d_out) return DK_E_NOMEM;
    DK_TRY(up.copy(d_bwt, bwt, n, "L"));
    DK_TRY(bwt_inverse_device(ctx, d_bwt, n, origin, d_out));
    DK_HIP(ctx, hipMemcpyAsync(out, d_out, n, hipMemcpyDeviceToHost, ctx->stream));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dk_dc_encode(dk_ctx *ctx, const uint8_t *bwt, size_t n, uint32_t init[256], uint32_t *dist, uint8_t *sym, uint8_t *rank, size_t *m) {
    DK_TRY(begin_call(ctx, "dk_dc_encode"));
    ScopedCall sc(ctx);
    Upload up(ctx);
    if (!bwt || !init || !dist || !sym || !m) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_n(ctx, n));
    Timer t;
    uint8_t *d_bwt = ctx->ws_alloc<uint8_t>(n);
    uint32_t *d_dist = ctx->ws_alloc<uint32_t>(n);
    uint8_t *d_sym = ctx->ws_alloc<uint8_t>(n);
    uint8_t *d_rank = ctx->ws_alloc<uint8_t>(n);
    if (!d_bwt || !d_dist || !d_sym || !d_rank) return DK_E_NOMEM;
    DK_TRY(up.copy(d_bwt, bwt, n, "L"));
    DK_TRY(dc_encode_device(ctx, d_bwt, n, init, d_dist, d_sym, d_rank, nullptr, m));
    DK_HIP(ctx, hipMemcpyAsync(dist, d_dist, *m * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    DK_HIP(ctx, hipMemcpyAsync(sym, d_sym, *m, hipMemcpyDeviceToHost, ctx->stream));
    if (rank) DK_HIP(ctx, hipMemcpyAsync(rank, d_rank, *m, hipMemcpyDeviceToHost, ctx->stream));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dk_dc_decode(dk_ctx *ctx, const uint32_t init[256], const uint32_t *dist, size_t m, uint8_t *bwt_out, size_t n, size_t *consumed) {
    if (!init || (!dist && m) || !bwt_out || n == 0) return ctx ? ctx->fail(DK_E_ARG, "null pointer or empty block") : DK_E_ARG;
    int rc = dc_decode_array(init, dist, m, bwt_out, n, consumed);
    if (rc && ctx) return ctx->fail(rc, "distance stream does not rebuild a BWT of %zu bytes", n);
    return rc;
}

int dk_block_encode(dk_ctx *ctx, int model_id, const uint8_t *in, size_t n, uint8_t *out, size_t out_cap, size_t *out_len) {
    DK_TRY(begin_call(ctx, "dk_block_encode"));
    ScopedCall sc(ctx);
    Upload up(ctx);
    if (!in || !out || !out_len) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_n(ctx, n));
    Timer t;
    uint8_t *d_text = ctx->ws_alloc<uint8_t>(n);
    if (!d_text) return DK_E_NOMEM;
    DK_TRY(up.copy(d_text, in, n, "text"));
    DK_TRY(up.sync());
    ctx->stats.ms_h2d = t.ms();
    int rc = block_encode_common(ctx, model_id, d_text, n, out, out_cap, out_len);
    ctx->stats.ms_total = t.ms();
    return rc;
}

int dk_block_decode(dk_ctx *ctx, int model_id, const uint8_t *in, size_t in_len, size_t n, uint8_t *out) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    if (!in || !out) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_n(ctx, n));
    Timer t;
    uint8_t *d_out = ctx->ws_alloc<uint8_t>(n);
    if (!d_out) return DK_E_NOMEM;
    DK_TRY(block_decode_common(ctx, model_id, in, in_len, n, d_out));
    Timer t2;
    DK_HIP(ctx, hipMemcpyAsync(out, d_out, n, hipMemcpyDeviceToHost, ctx->stream));
    DK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stats.ms_d2h = t2.ms();
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

// block::raw::Encoder::encode (src/block/raw.rs:35-59): SA -> BWT on the GPU; origin + L then go through the RawModel -- the dump model
// Out (into `dump`) or the bbb coding model (into `out`; host, bit-serial)
int dk_raw_block_encode(dk_ctx *ctx, int raw_model, const uint8_t *in, size_t n, uint8_t *out, size_t out_cap, size_t *out_len, uint8_t *dump,
                        size_t dump_cap, size_t *dump_len) {
    DK_TRY(begin_call(ctx, "dk_raw_block_encode"));
    ScopedCall sc(ctx);
    Upload up(ctx);
    if (!in || !out || !out_len) return ctx->fail(DK_E_ARG, "null pointer");
    if (raw_model != DK_RAWMODEL_OUT && raw_model != DK_RAWMODEL_BBB) return ctx->fail(DK_E_MODEL, "unknown raw model %d", raw_model);
    if (raw_model == DK_RAWMODEL_OUT && (!dump || !dump_len)) return ctx->fail(DK_E_ARG, "the Out model needs a dump buffer");
    DK_TRY(check_n(ctx, n));
    if (raw_model == DK_RAWMODEL_OUT && (dump_cap < n + 4 || out_cap < 4)) return ctx->fail(DK_E_CAPACITY, "dump needs n + 4 bytes, out 4 bytes");
    Timer t;
    uint8_t *d_text = ctx->ws_alloc<uint8_t>(n);
    uint8_t *d_bwt = ctx->ws_alloc<uint8_t>(n);
    uint32_t *d_sa = ctx->ws_alloc<uint32_t>(n);
    if (!d_text || !d_bwt || !d_sa) return DK_E_NOMEM;
    DK_TRY(up.copy(d_text, in, n, "text"));
    uint32_t origin = 0;
    DK_TRY(bwt_forward_device(ctx, d_text, n, d_sa, d_bwt, &origin));
    if (raw_model == DK_RAWMODEL_OUT) {
        DK_HIP(ctx, hipMemcpyAsync(dump + 4, d_bwt, n, hipMemcpyDeviceToHost, ctx->stream));
        DK_TRY(up.sync());
        for (int i = 0; i < 4; ++i) dump[i] = static_cast<uint8_t>(origin >> (24 - 8 * i));  // src/block/raw.rs:48-51
        *dump_len = n + 4;
        std::memset(out, 0, 4);  // ari::Encoder::finish of a coder nothing was coded with: low = 0, four bytes
        *out_len = 4;
    } else {
        DK_TRY(ctx->ensure_stage(n + 64));
        uint8_t *h_bwt = reinterpret_cast<uint8_t *>(ctx->h_stage);
        DK_HIP(ctx, hipMemcpyAsync(h_bwt, d_bwt, n, hipMemcpyDeviceToHost, ctx->stream));
        DK_TRY(up.sync());
        Timer te;
        const int rc = raw_bbb_encode_stream(h_bwt, n, origin, out, out_cap, out_len);
        ctx->stats.ms_entropy = te.ms();
        if (rc == DK_E_CAPACITY) return ctx->fail(rc, "output buffer of %zu bytes is too small", out_cap);
        if (rc) return ctx->fail(rc, "bbb coding failed (%d)", rc);
        if (dump_len) *dump_len = 0;
    }
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dk_raw_block_decode(dk_ctx *ctx, int raw_model, const uint8_t *in, size_t in_len, size_t n, uint8_t *out) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    if (!in || !out) return ctx->fail(DK_E_ARG, "null pointer");
    if (raw_model != DK_RAWMODEL_OUT && raw_model != DK_RAWMODEL_BBB) return ctx->fail(DK_E_MODEL, "unknown raw model %d", raw_model);
    DK_TRY(check_n(ctx, n));
    if (raw_model == DK_RAWMODEL_OUT) {
        std::memset(out, 0, n);  // Out::decode returns symbol 0 ("not supported", src/model/raw.rs:71-75): origin 0, a BWT of zeros -> n zeros
        return DK_OK;
    }
    Timer t;
    DK_TRY(ctx->ensure_stage(n + 64));
    uint8_t *h_bwt = reinterpret_cast<uint8_t *>(ctx->h_stage);
    uint32_t origin = 0;
    const int rc = raw_bbb_decode_stream(in, in_len, n, h_bwt, &origin, &ctx->last_consumed);
    ctx->stats.ms_entropy = t.ms();
    if (rc) return ctx->fail(rc, "bbb stream does not decode");
    if (origin >= n) return ctx->fail(DK_E_STREAM, "decoded origin %u is outside the block", origin);
    uint8_t *d_bwt = ctx->ws_alloc<uint8_t>(n);
    uint8_t *d_out = ctx->ws_alloc<uint8_t>(n);
    if (!d_bwt || !d_out) return DK_E_NOMEM;
    DK_HIP(ctx, hipMemcpyAsync(d_bwt, h_bwt, n, hipMemcpyHostToDevice, ctx->stream));
    DK_TRY(bwt_inverse_device(ctx, d_bwt, n, origin, d_out));
    DK_HIP(ctx, hipMemcpyAsync(out, d_out, n, hipMemcpyDeviceToHost, ctx->stream));
    DK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

}  // extern "C" (the helper below is a template)

// ---- several GPUs in one call: one host thread + one context per listed device ---------------------------------------------------------
namespace {
struct DeviceBuffers {  // input / output blocks of one sub-batch in HBM
    std::vector<uint8_t *> ptr;
    ~DeviceBuffers() { for (uint8_t *p : ptr) if (p) (void)hipFree(p); }
};
template <class Work>
int run_per_device(int purpose, const int *devices, int ndev, size_t count, const size_t *n, char *err, size_t err_cap, Work work) {
    if (!devices || ndev <= 0 || count == 0 || !n) return DK_E_ARG;
    std::vector<int> rcs(static_cast<size_t>(ndev), DK_OK);
    std::vector<std::string> msgs(static_cast<size_t>(ndev));
    std::vector<std::thread> threads;
    for (int r = 0; r < ndev; ++r) {
        threads.emplace_back([&, r] {
            std::vector<size_t> mine;
            size_t max_n = 0;
            for (size_t i = static_cast<size_t>(r); i < count; i += static_cast<size_t>(ndev)) { mine.push_back(i); max_n = std::max(max_n, n[i]); }
            if (mine.empty()) return;
            dk_ctx *ctx = nullptr;
            int rc = purpose == DK_CTX_DECODER ? dk_ctx_create_decoder(devices[r], max_n, 1, &ctx) : dk_ctx_create(devices[r], max_n, &ctx);
            if (rc != DK_OK) { rcs[r] = rc; msgs[r] = "dk_ctx_create failed on device " + std::to_string(devices[r]); return; }
            rc = work(ctx, mine);
            if (rc != DK_OK) { rcs[r] = rc; msgs[r] = dk_last_error(ctx); }
            dk_ctx_destroy(ctx);
        });
    }
    for (auto &t : threads) t.join();
    for (int r = 0; r < ndev; ++r)
        if (rcs[r] != DK_OK) {
            if (err && err_cap) snprintf(err, err_cap, "device %d: %s", devices[r], msgs[r].c_str());
            return rcs[r];
        }
    if (err && err_cap) err[0] = 0;
    return DK_OK;
}
}  // namespace

extern "C" {

int dk_multi_block_encode(const int *devices, int ndev, int model_id, size_t count, const uint8_t *const *in, const size_t *n, uint8_t *const *out,
                          const size_t *out_cap, size_t *out_len, int host_threads_per_gpu, char *err, size_t err_cap) {
    if (!in || !out || !out_cap || !out_len) return DK_E_ARG;
    const size_t group = static_cast<size_t>(std::max(1, host_threads_per_gpu)) + 1;  // blocks resident in HBM per sub-batch
    return run_per_device(DK_CTX_FULL, devices, ndev, count, n, err, err_cap, [&](dk_ctx *ctx, const std::vector<size_t> &mine) -> int {
        for (size_t lo = 0; lo < mine.size(); lo += group) {
            const size_t cnt = std::min(group, mine.size() - lo);
            DeviceBuffers db;
            std::vector<const uint8_t *> d_in(cnt);
            std::vector<size_t> ns(cnt), caps(cnt), lens(cnt);
            std::vector<uint8_t *> outs(cnt);
            Upload up(ctx);  // (behind db: the uploads have landed before their destinations are freed)
            for (size_t k = 0; k < cnt; ++k) {
                const size_t i = mine[lo + k];
                uint8_t *p = nullptr;
                if (!in[i] || !out[i] || n[i] == 0) return ctx->fail(DK_E_ARG, "null pointer or empty block %zu", i);
                if (hipMalloc(reinterpret_cast<void **>(&p), n[i]) != hipSuccess) return ctx->fail(DK_E_NOMEM, "hipMalloc of block %zu failed", i);
                db.ptr.push_back(p);
                if (up.copy(p, in[i], n[i], "upload") != DK_OK) return ctx->fail(DK_E_HIP, "upload of block %zu failed", i);  // (ordered with the kernels that read it)
                d_in[k] = p; ns[k] = n[i]; caps[k] = out_cap[i]; outs[k] = out[i];
            }
            const int rc = dk_dev_batch_encode(ctx, model_id, cnt, d_in.data(), ns.data(), outs.data(), caps.data(), lens.data(), host_threads_per_gpu);
            if (rc != DK_OK) return rc;
            up.synchronised();  // (every stream of the batch is coded: its blocks were read long ago)
            for (size_t k = 0; k < cnt; ++k) out_len[mine[lo + k]] = lens[k];
        }
        return DK_OK;
    });
}

int dk_multi_block_decode(const int *devices, int ndev, int model_id, size_t count, const uint8_t *const *in, const size_t *in_len, const size_t *n,
                          uint8_t *const *out, int host_threads_per_gpu, char *err, size_t err_cap) {
    if (!in || !in_len || !out) return DK_E_ARG;
    const size_t group = static_cast<size_t>(std::max(1, host_threads_per_gpu)) + 1;
    return run_per_device(DK_CTX_DECODER, devices, ndev, count, n, err, err_cap, [&](dk_ctx *ctx, const std::vector<size_t> &mine) -> int {
        for (size_t lo = 0; lo < mine.size(); lo += group) {
            const size_t cnt = std::min(group, mine.size() - lo);
            DeviceBuffers db;
            std::vector<const uint8_t *> ins(cnt);
            std::vector<size_t> lens(cnt), ns(cnt);
            std::vector<uint8_t *> d_out(cnt);
            for (size_t k = 0; k < cnt; ++k) {
                const size_t i = mine[lo + k];
                uint8_t *p = nullptr;
                if (!in[i] || !out[i] || n[i] == 0) return ctx->fail(DK_E_ARG, "null pointer or empty block %zu", i);
                if (hipMalloc(reinterpret_cast<void **>(&p), n[i]) != hipSuccess) return ctx->fail(DK_E_NOMEM, "hipMalloc of block %zu failed", i);
                db.ptr.push_back(p);
                ins[k] = in[i]; lens[k] = in_len[i]; ns[k] = n[i]; d_out[k] = p;
            }
            const int rc = dk_dev_batch_decode(ctx, model_id, cnt, ins.data(), lens.data(), ns.data(), d_out.data(), host_threads_per_gpu);
            if (rc != DK_OK) return rc;
            for (size_t k = 0; k < cnt; ++k)
                if (hipMemcpy(out[mine[lo + k]], d_out[k], ns[k], hipMemcpyDeviceToHost) != hipSuccess) return ctx->fail(DK_E_HIP, "download of block %zu failed", mine[lo + k]);
        }
        return DK_OK;
    });
}

// ---- model / coder level (host only) --------------------------------------------------------------------------------------
int dk_model_encode(int model_id, const uint32_t *dist, const uint8_t *sym, size_t m, uint8_t *out, size_t out_cap, size_t *out_len) {
    if ((!dist || !sym) && m) return DK_E_ARG;
    if (!out || !out_len) return DK_E_ARG;
    return model_encode_stream(model_id, dist, sym, m, out, out_cap, out_len);
}
int dk_model_decode(int model_id, const uint8_t *in, size_t in_len, const uint8_t *sym, size_t m, uint32_t *dist) {
    if (!in || ((!sym || !dist) && m)) return DK_E_ARG;
    return model_decode_stream(model_id, in, in_len, sym, m, dist);
}
int dk_bitcoder_encode(const uint8_t *bits, const uint16_t *flat, size_t nbits, uint8_t *out, size_t out_cap, size_t *out_len) {
    if (((!bits || !flat) && nbits) || !out || !out_len) return DK_E_ARG;
    return bitcoder_encode(bits, flat, nbits, out, out_cap, out_len);
}
int dk_bitcoder_decode(const uint8_t *in, size_t in_len, const uint16_t *flat, size_t nbits, uint8_t *bits) {
    if (!in || ((!flat || !bits) && nbits)) return DK_E_ARG;
    return bitcoder_decode(in, in_len, flat, nbits, bits);
}
int dk_stream_encode(int model_id, size_t n, const uint32_t init[256], const uint32_t *dist, const uint8_t *sym, const uint8_t *rank,
                     const uint32_t *run_end, size_t m, uint32_t origin, uint8_t *out, size_t out_cap, size_t *out_len) {
    DcStream s;
    s.n = n; s.init = init; s.dist = dist; s.sym = sym; s.rank = rank; s.run_end = run_end; s.m = m; s.origin = origin;
    return encode_block_stream(model_id, s, out, out_cap, out_len);
}
int dk_stream_decode(int model_id, const uint8_t *in, size_t in_len, size_t n, uint8_t *bwt_out, uint32_t *origin, int *single_symbol,
                     size_t *consumed) {
    int single = 0;
    int rc = decode_block_stream(model_id, in, in_len, n, bwt_out, origin, &single, consumed);
    if (single_symbol) *single_symbol = single;
    return rc;
}

int dk_raw_stream_encode(int raw_model, const uint8_t *bwt, size_t n, uint32_t origin, uint8_t *out, size_t out_cap, size_t *out_len) {
    if (!bwt || !out || !out_len || n == 0) return DK_E_ARG;
    if (raw_model != DK_RAWMODEL_BBB) return DK_E_MODEL;
    return raw_bbb_encode_stream(bwt, n, origin, out, out_cap, out_len);
}
int dk_raw_stream_decode(int raw_model, const uint8_t *in, size_t in_len, size_t n, uint8_t *bwt_out, uint32_t *origin, size_t *consumed) {
    if (!in || !bwt_out || !origin || n == 0) return DK_E_ARG;
    if (raw_model != DK_RAWMODEL_BBB) return DK_E_MODEL;
    return raw_bbb_decode_stream(in, in_len, n, bwt_out, origin, consumed);
}

// ---- measurement ----------------------------------------------------------------------------------------------------------
int dk_set_profiling(dk_ctx *ctx, int enabled) {
    if (!ctx) return DK_E_ARG;
    ctx->profiling = enabled != 0;
    return DK_OK;
}
int dk_stats_reset(dk_ctx *ctx) {
    if (!ctx) return DK_E_ARG;
    ctx->stats = dk_stats{};
    return DK_OK;
}
int dk_get_stats(const dk_ctx *ctx, dk_stats *out) {
    if (!ctx || !out) return DK_E_ARG;
    *out = ctx->stats;
    out->ws_peak_bytes = ctx->ws_peak;
    out->ws_size_bytes = ctx->ws_size;
    return DK_OK;
}
const char *dk_kernel_name(int slot) { return kernel_slot_name(slot); }

// ---- host coding threads ------------------------------------------------------------------------------------------------------
int dk_set_entropy_threads(int mode) { return set_entropy_thread_mode(mode); }
int dk_host_l3_groups(int min_cores) { return host_l3_groups(min_cores); }
int dk_dbg_l3_claim_order(const int *group_numa, int ngroups, int own, int preferred_numa, int *order_out) {
    if (!group_numa || !order_out || ngroups <= 0 || own < 0 || own >= ngroups) return DK_E_ARG;
    const std::vector<size_t> order = l3_claim_order(std::vector<int>(group_numa, group_numa + ngroups), static_cast<size_t>(own), preferred_numa);
    for (size_t i = 0; i < order.size(); ++i) order_out[i] = static_cast<int>(order[i]);
    return static_cast<int>(order.size());
}
void dk_set_entropy_numa_node(int node) { dk::set_preferred_numa(node); }
void dk_last_entropy_info(int *threads, int *l3_group) {
    if (threads) *threads = last_entropy_threads();
    if (l3_group) *l3_group = last_entropy_group();
}

// ---- debug ------------------------------------------------------------------------------------------------------------------
int dk_dbg_stream_encode_gated(int model_id, size_t n, const uint32_t init[256], const uint32_t *dist, const uint8_t *sym, size_t m, uint32_t origin,
                               uint8_t *out, size_t out_cap, size_t *out_len, const size_t *ready, unsigned stall_ms, int host_threads) {
    if (!ready) return DK_E_ARG;
    static_assert(sizeof(std::atomic<size_t>) == sizeof(size_t) && std::atomic<size_t>::is_always_lock_free, "the caller's word is read as an atomic");
    DcStream s;
    s.n = n; s.init = init; s.dist = dist; s.sym = sym; s.m = m; s.origin = origin;
    s.ready = reinterpret_cast<const std::atomic<size_t> *>(ready);
    s.stall_ms = stall_ms;
    return encode_block_stream(model_id, s, out, out_cap, out_len, host_threads);
}
// Both serve every purpose of a context (no forward_entry): the stages of a decoder context are poisoned through them too.
int dk_dbg_mail_fill(dk_ctx *ctx, int byte) {
    DK_TRY(begin_call(ctx));  // (refuses an open batch: its stages are between their clears and their reads)
    if (byte < 0 || byte > 255) return ctx->fail(DK_E_ARG, "dk_dbg_mail_fill: %d is no byte", byte);
    // every word: no stage takes one over from the call before it (mailbox.hpp), so there is nothing to leave out
    DK_TRY(ctx->mail_fill(ctx->d_mail, byte));  // (the whole struct as one "member")
    DK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memset(ctx->h_mail, byte, sizeof *ctx->h_mail);
    return DK_OK;
}
int dk_dbg_ws_peek(dk_ctx *ctx, size_t nbytes, uint8_t *host_out) {
    DK_TRY(begin_call(ctx));
    if (!host_out || nbytes == 0) return ctx->fail(DK_E_ARG, "dk_dbg_ws_peek: null pointer or nothing to read");
    // as a stage does: an allocation nobody needs first (released again, so that the next one starts where a call's second allocation would,
    // on bytes an earlier allocation has owned), then the one that is read back before anything has written it
    const size_t mark = ctx->ws_mark();
    if (!ctx->ws_alloc_bytes(1)) return DK_E_NOMEM;
    ctx->ws_release(mark);
    const uint8_t *p = static_cast<const uint8_t *>(ctx->ws_alloc_bytes(nbytes));
    if (!p) return DK_E_NOMEM;
    const hipError_t e = hipMemcpyAsync(host_out, p, nbytes, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    ctx->ws_release(mark);
    DK_HIP(ctx, e);
    DK_HIP(ctx, e2);
    return DK_OK;
}
int dk_dbg_dev_local_sort(dk_ctx *ctx, uint64_t *d_keys, uint32_t *d_vals, size_t count, int begin_bit, int end_bit) {
    DK_TRY(begin_call(ctx, "dk_dbg_dev_local_sort"));
    ScopedCall sc(ctx);
    if (!d_keys || !d_vals) return ctx->fail(DK_E_ARG, "null pointer");
    return local_sort_tiles(ctx, d_keys, d_vals, count, begin_bit, end_bit);
}
int dk_dbg_dev_sort_pairs(dk_ctx *ctx, uint64_t *d_keys, uint32_t *d_vals, size_t count, int begin_bit, int end_bit) {
    DK_TRY(begin_call(ctx, "dk_dbg_dev_sort_pairs"));
    ScopedCall sc(ctx);
    if (!d_keys || !d_vals || count == 0) return ctx->fail(DK_E_ARG, "null pointer or empty input");
    uint64_t *k0 = d_keys, *k1 = ctx->ws_alloc<uint64_t>(count);
    uint32_t *v0 = d_vals, *v1 = ctx->ws_alloc<uint32_t>(count);
    if (!k1 || !v1) return DK_E_NOMEM;
    DK_TRY(sort_pairs(ctx, k0, k1, v0, v1, count, begin_bit, end_bit));
    if (k0 != d_keys) {
        DK_HIP(ctx, hipMemcpyAsync(d_keys, k0, count * 8, hipMemcpyDeviceToDevice, ctx->stream));
        DK_HIP(ctx, hipMemcpyAsync(d_vals, v0, count * 4, hipMemcpyDeviceToDevice, ctx->stream));
    }
    DK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DK_OK;
}
int dk_dbg_dev_sort_groups(dk_ctx *ctx, const uint64_t *d_kin, const uint32_t *d_vin, uint64_t *d_kout, uint32_t *d_vout, const uint32_t *starts,
                           size_t ngroups, size_t npairs, uint32_t above, int begin_bit, int end_bit) {
    DK_TRY(begin_call(ctx, "dk_dbg_dev_sort_groups"));
    ScopedCall sc(ctx);
    Upload up(ctx);
    if (!d_kin || !d_vin || !d_kout || !d_vout || !starts || ngroups == 0 || npairs == 0) return ctx->fail(DK_E_ARG, "null pointer or empty input");
    if (npairs > 0xFFFFFFFFull || begin_bit < 0 || end_bit > 64 || begin_bit > end_bit) return ctx->fail(DK_E_ARG, "sort_groups: %zu pairs, bits [%d, %d)", npairs, begin_bit, end_bit);
    for (size_t g = 0; g < ngroups; ++g)
        if (starts[g] > starts[g + 1]) return ctx->fail(DK_E_ARG, "sort_groups: starts[%zu] = %u > starts[%zu] = %u", g, starts[g], g + 1, starts[g + 1]);
    if (starts[ngroups] > npairs) return ctx->fail(DK_E_ARG, "sort_groups: the last group ends at %u of %zu pairs", starts[ngroups], npairs);
    uint32_t *d_starts = ctx->ws_alloc<uint32_t>(ngroups + 1);
    if (!d_starts) return DK_E_NOMEM;
    DK_TRY(up.copy(d_starts, starts, (ngroups + 1) * sizeof(uint32_t), "group starts"));
    DK_TRY(sort_groups(ctx, d_kin, d_vin, d_kout, d_vout, d_starts, ngroups, npairs, above, begin_bit, end_bit));
    DK_TRY(up.sync());
    return DK_OK;
}
int dk_dbg_dev_rerank(dk_ctx *ctx, const void *d_keys, int key_bytes, const uint32_t *d_bucket_starts, const uint32_t *d_idx, const uint32_t *d_pos_in,
                      const uint32_t *d_gid_in, int cmp_shift, size_t count, uint32_t *d_rank, uint32_t *d_sa, uint8_t *d_bwt, const uint8_t *d_sym_in,
                      uint8_t *d_sym_out, uint32_t *d_origin, uint32_t *d_out_idx, uint32_t *d_out_pos, uint32_t *d_out_gid, uint32_t *d_gstart,
                      uint32_t *d_bigidx, uint32_t *d_bigoff, uint32_t ls_max, uint32_t counts_out[5], unsigned reduce_tiles_per_wg,
                      unsigned first_tiles_per_wg, int sparse_max) {
    DK_TRY(begin_call(ctx, "dk_dbg_dev_rerank"));
    ScopedCall sc(ctx);
    if (!d_keys || !d_idx || !d_out_idx || !d_out_pos || !d_out_gid || !d_gstart || !d_bigidx || !d_bigoff || !counts_out)
        return ctx->fail(DK_E_ARG, "rerank: null pointer");
    if (count == 0 || count > ctx->max_n || count > 0x7FFFFFFEull) return ctx->fail(DK_E_ARG, "rerank: %zu slots (context capacity %zu)", count, ctx->max_n);
    if (key_bytes != 4 && key_bytes != 8) return ctx->fail(DK_E_ARG, "rerank: keys of %d bytes", key_bytes);
    if ((key_bytes == 4) != (d_bucket_starts != nullptr)) return ctx->fail(DK_E_ARG, "rerank: bucket starts go with 4-byte keys, and only with them");
    if (key_bytes == 4 && (d_pos_in || d_gid_in)) return ctx->fail(DK_E_ARG, "rerank: narrow keys only in the first rerank (no d_pos_in, no d_gid_in)");
    if (d_rank && !d_pos_in) return ctx->fail(DK_E_ARG, "rerank: the first rerank (no d_pos_in) writes no ranks");
    if (cmp_shift < 0 || cmp_shift > 63 || (cmp_shift && (d_pos_in || key_bytes == 4)))
        return ctx->fail(DK_E_ARG, "rerank: cmp_shift %d (0 .. 63, and only the first rerank of 8-byte keys leaves low bits out)", cmp_shift);
    if (d_bwt && (!d_sym_out || (d_pos_in && (!d_sym_in || !d_origin)))) return ctx->fail(DK_E_ARG, "rerank: d_bwt without the rest of the carry");
    if (reduce_tiles_per_wg > 64 || first_tiles_per_wg > 64)
        return ctx->fail(DK_E_ARG, "rerank: %u / %u tiles per workgroup (at most 64)", reduce_tiles_per_wg, first_tiles_per_wg);
    if (sparse_max > 2048) return ctx->fail(DK_E_ARG, "rerank: sparse_max %d (a tile holds 2048 slots)", sparse_max);
    const DbgRerank a{static_cast<const uint64_t *>(d_keys), d_bucket_starts, d_idx, d_pos_in, d_gid_in, cmp_shift, count, d_rank, d_sa, d_bwt, d_sym_in, d_sym_out,
                      d_origin, d_out_idx, d_out_pos, d_out_gid, d_gstart, d_bigidx, d_bigoff, ls_max, reduce_tiles_per_wg, first_tiles_per_wg, sparse_max};
    return dbg_rerank_device(ctx, a, counts_out);
}
int dk_dbg_dev_lf_rerank(dk_ctx *ctx, const void *d_keys, int key_bytes, const uint32_t *d_bucket_starts, int cmp_shift, uint8_t *d_sym, int sym_from_key,
                         const uint32_t *d_idx, const uint32_t *d_zero_slot, const uint32_t *d_pos_in, size_t count, uint32_t *d_out_idx, uint32_t *d_out_pos,
                         uint32_t *d_out_gid, uint8_t *d_out_sym, uint32_t *d_gstart, uint8_t *d_bwt, uint32_t *d_origin, uint32_t *d_gdepth_out,
                         uint32_t depth_uniform, const uint32_t *d_bigdepth, int key_shift, uint32_t depth_add, uint32_t counts_out[4],
                         unsigned reduce_tiles_per_wg) {
    DK_TRY(begin_call(ctx, "dk_dbg_dev_lf_rerank"));
    ScopedCall sc(ctx);
    if (!d_keys || !d_sym || !d_idx || !d_out_idx || !d_out_pos || !d_out_gid || !d_out_sym || !d_gstart || !counts_out)
        return ctx->fail(DK_E_ARG, "lf_rerank: null pointer");
    if (count == 0 || count > ctx->max_n || count > 0x7FFFFFFEull) return ctx->fail(DK_E_ARG, "lf_rerank: %zu slots (context capacity %zu)", count, ctx->max_n);
    if (key_bytes != 4 && key_bytes != 8) return ctx->fail(DK_E_ARG, "lf_rerank: keys of %d bytes", key_bytes);
    if (key_bytes == 8 && d_bucket_starts) return ctx->fail(DK_E_ARG, "lf_rerank: bucket starts go with 4-byte keys only");
    if (cmp_shift < 0 || cmp_shift > 63 || (cmp_shift && key_bytes == 4))
        return ctx->fail(DK_E_ARG, "lf_rerank: cmp_shift %d (0 .. 63, and only 8-byte keys leave low bits out)", cmp_shift);
    if (sym_from_key && key_bytes == 4) return ctx->fail(DK_E_ARG, "lf_rerank: only 8-byte keys carry the symbol in their low byte");
    if (d_pos_in && (!d_bwt || !d_origin)) return ctx->fail(DK_E_ARG, "lf_rerank: a later rerank (d_pos_in) writes its finals: d_bwt and d_origin");
    if (d_bigdepth && (key_bytes != 8 || !d_gdepth_out || key_shift < 0 || key_shift > 63))
        return ctx->fail(DK_E_ARG, "lf_rerank: the big-list depth rule reads 8-byte keys above key_shift 0 .. 63 and writes d_gdepth_out");
    if (reduce_tiles_per_wg > 64) return ctx->fail(DK_E_ARG, "lf_rerank: %u tiles per workgroup (at most 64)", reduce_tiles_per_wg);
    const DbgLfRerank a{d_keys, key_bytes, d_bucket_starts, cmp_shift, d_sym, sym_from_key, d_idx, d_zero_slot, d_pos_in, count, d_out_idx, d_out_pos, d_out_gid,
                        d_out_sym, d_gstart, d_bwt, d_origin, d_gdepth_out, depth_uniform, d_bigdepth, key_shift, depth_add, reduce_tiles_per_wg};
    return dbg_lf_rerank_device(ctx, a, counts_out);
}
int dk_dbg_dev_lf_refine(dk_ctx *ctx, const uint8_t *d_text, size_t n, const uint32_t *d_idx, const uint32_t *d_pos, const uint32_t *d_gid, const uint8_t *d_sym,
                         size_t count, uint32_t h0, int period, uint8_t *d_bwt, uint32_t *d_origin, uint32_t out[8]) {
    DK_TRY(begin_call(ctx, "dk_dbg_dev_lf_refine"));
    ScopedCall sc(ctx);
    if (!d_text || !d_idx || !d_pos || !d_gid || !d_sym || !d_bwt || !d_origin || !out) return ctx->fail(DK_E_ARG, "lf_refine: null pointer");
    if (n < 64 || n > ctx->max_n || n > 0x7FFFFFFEull) return ctx->fail(DK_E_ARG, "lf_refine: text of %zu bytes (64 .. the context capacity %zu)", n, ctx->max_n);
    if (count == 0 || count > n) return ctx->fail(DK_E_ARG, "lf_refine: %zu slots for a text of %zu bytes", count, n);
    if (h0 == 0 || h0 > n) return ctx->fail(DK_E_ARG, "lf_refine: depth %u of a text of %zu bytes", h0, n);
    if (period < 0 || (period > 0 && static_cast<uint32_t>(period) > h0))
        return ctx->fail(DK_E_ARG, "lf_refine: period %d (0: no tokens; otherwise 1 .. h0 = %u: the members of a group share the period string)", period, h0);
    const DbgLfRefine a{d_text, n, d_idx, d_pos, d_gid, d_sym, count, h0, period, d_bwt, d_origin};
    return dbg_lf_refine_device(ctx, a, out);
}
int dk_dbg_dev_in_place(dk_ctx *ctx, size_t n, uint32_t h, size_t count, const uint32_t *d_idx, const uint32_t *d_pos, const uint32_t *d_gid, const uint32_t *d_gstart,
                        size_t groups, uint32_t *d_rank, uint32_t *d_sa, uint8_t *d_bwt, const uint8_t *d_sym, uint32_t *d_origin, int chain_group, uint32_t record_cap,
                        int max_rounds, int always_compact, uint32_t *d_out_idx, uint32_t *d_out_meta, uint8_t *d_out_sym, uint32_t *d_out_pos, uint32_t out[8]) {
    DK_TRY(begin_call(ctx, "dk_dbg_dev_in_place"));
    ScopedCall sc(ctx);
    if (!d_idx || !d_pos || !d_gid || !d_gstart || !d_rank || !d_out_idx || !d_out_meta || !d_out_pos || !out) return ctx->fail(DK_E_ARG, "in_place: null pointer");
    const bool sa_mode = d_sa && !d_bwt && !d_sym && !d_origin && !d_out_sym, l_mode = !d_sa && d_bwt && d_sym && d_origin && d_out_sym;
    if (!sa_mode && !l_mode) return ctx->fail(DK_E_ARG, "in_place: exactly one of d_sa and (d_bwt, d_sym, d_origin, d_out_sym)");
    if (n < 2 || n > ctx->max_n || n > 0x7FFFFFFEull) return ctx->fail(DK_E_ARG, "in_place: text of %zu bytes (2 .. the context capacity %zu)", n, ctx->max_n);
    if (count == 0 || count > n) return ctx->fail(DK_E_ARG, "in_place: %zu slots for a text of %zu bytes", count, n);
    if (groups == 0 || groups > count || groups > n / 2 + 1) return ctx->fail(DK_E_ARG, "in_place: %zu groups of %zu slots (the table holds n / 2 + 2 words)", groups, count);
    if (h == 0) return ctx->fail(DK_E_ARG, "in_place: depth 0");
    if (chain_group > 4) return ctx->fail(DK_E_ARG, "in_place: chain_group %d (0: no chains, 2 .. 4, negative: the sort's own)", chain_group);
    if (record_cap > n) return ctx->fail(DK_E_ARG, "in_place: record_cap %u above n = %zu, what the record buffers hold", record_cap, n);
    const DbgInPlace a{n, h, count, d_idx, d_pos, d_gid, d_gstart, groups, d_rank, d_sa, d_bwt, d_sym, d_origin, chain_group, record_cap, max_rounds, always_compact,
                       d_out_idx, d_out_meta, d_out_sym, d_out_pos};
    return dbg_in_place_device(ctx, a, out);
}
int dk_dbg_dev_round(dk_ctx *ctx, const uint8_t *d_text, size_t n, uint32_t h, size_t count, const uint32_t *d_idx, const uint32_t *d_pos, const uint32_t *d_gid,
                     const uint32_t *d_gstart, size_t groups, uint32_t *d_rank, int tsym, int period, const uint32_t *d_next_break, uint32_t *d_sa, uint8_t *d_bwt,
                     const uint8_t *d_sym, uint32_t *d_origin, uint64_t *d_out_sorted_keys, uint32_t *d_out_sorted_idx, uint8_t *d_out_sorted_sym, uint32_t *d_out_idx,
                     uint32_t *d_out_pos, uint32_t *d_out_gid, uint32_t *d_out_gstart, uint8_t *d_out_sym, uint32_t out[8]) {
    DK_TRY(begin_call(ctx, "dk_dbg_dev_round"));
    ScopedCall sc(ctx);
    if (!d_text || !d_idx || !d_pos || !d_gid || !d_gstart || !d_out_sorted_keys || !d_out_sorted_idx || !d_out_idx || !d_out_pos || !d_out_gid || !d_out_gstart || !out)
        return ctx->fail(DK_E_ARG, "round: null pointer");
    const bool sa_mode = d_sa && !d_bwt && !d_sym && !d_origin && !d_out_sorted_sym && !d_out_sym;
    const bool l_mode = !d_sa && d_bwt && d_sym && d_origin && d_out_sorted_sym && d_out_sym;
    if (!sa_mode && !l_mode) return ctx->fail(DK_E_ARG, "round: exactly one of d_sa and (d_bwt, d_sym, d_origin, d_out_sorted_sym, d_out_sym)");
    if (n < 2 || n > ctx->max_n || n > 0x7FFFFFFEull) return ctx->fail(DK_E_ARG, "round: text of %zu bytes (2 .. the context capacity %zu)", n, ctx->max_n);
    if (count == 0 || count > n) return ctx->fail(DK_E_ARG, "round: %zu slots for a text of %zu bytes", count, n);
    if (groups == 0 || groups > count || groups > n / 2 + 1) return ctx->fail(DK_E_ARG, "round: %zu groups of %zu slots (the table holds n / 2 + 2 words)", groups, count);
    if (h == 0) return ctx->fail(DK_E_ARG, "round: depth 0");
    if (tsym < 0 || tsym > 63) return ctx->fail(DK_E_ARG, "round: tsym %d (0: a doubling round, 1 .. 63 symbols of text)", tsym);
    if (tsym == 0 && !d_rank) return ctx->fail(DK_E_ARG, "round: a doubling round without d_rank");
    if (period < 0 || static_cast<uint32_t>(period) > h || period > (1 << 18)) return ctx->fail(DK_E_ARG, "round: period %d (0 .. min(h, 2^18))", period);
    if ((period > 0) != (d_next_break != nullptr)) return ctx->fail(DK_E_ARG, "round: d_next_break goes with a period, and only with one");
    if (period > 0 && tsym != 8) return ctx->fail(DK_E_ARG, "round: a token round has tsym 8, as the sort passes it (got %d)", tsym);
    const DbgRound a{d_text, n, h, count, d_idx, d_pos, d_gid, d_gstart, groups, d_rank, tsym, period, d_next_break, d_sa, d_bwt, d_sym, d_origin,
                     d_out_sorted_keys, d_out_sorted_idx, d_out_sorted_sym, d_out_idx, d_out_pos, d_out_gid, d_out_gstart, d_out_sym};
    return dbg_round_device(ctx, a, out);
}
int dk_dbg_dev_period(dk_ctx *ctx, const uint8_t *d_text, size_t n, int period, uint32_t *d_next_break, uint32_t run_out[2], uint32_t probe_out[8], uint32_t count_p,
                      uint32_t *count_out, uint32_t search_pmax, uint32_t *found_out, uint32_t m, uint32_t span, const int *cands, int ncands, uint32_t dups_out[4]) {
    DK_TRY(begin_call(ctx, "dk_dbg_dev_period"));
    ScopedCall sc(ctx);
    if (!d_text) return ctx->fail(DK_E_ARG, "period: null text");
    if (n == 0 || n > ctx->max_n || n > 0x7FFFFFFEull) return ctx->fail(DK_E_ARG, "period: text of %zu bytes (1 .. the context capacity %zu)", n, ctx->max_n);
    if (period < 0 || period > (1 << 18) || (period > 0) != (d_next_break != nullptr))
        return ctx->fail(DK_E_ARG, "period: period %d (0: no next breaks, 1 .. 2^18 with d_next_break, and d_next_break only with one)", period);
    if ((count_p != 0) != (count_out != nullptr)) return ctx->fail(DK_E_ARG, "period: count_out goes with a period to count, and only with one");
    if ((search_pmax != 0) != (found_out != nullptr) || (search_pmax != 0 && (search_pmax < 9 || search_pmax > (1u << 18))))
        return ctx->fail(DK_E_ARG, "period: search_pmax %u (0: no search, 9 .. 2^18 with found_out, and found_out only with one)", search_pmax);
    if (dups_out) {
        if (!cands || ncands < 1 || ncands > 4) return ctx->fail(DK_E_ARG, "period: %d candidate lengths (1 .. 4)", ncands);
        if (m == 0 || m > n || m > (1u << 24) || span == 0) return ctx->fail(DK_E_ARG, "period: %u samples (1 .. min(n, 2^24)) a span of %u (at least 1) apart", m, span);
    } else if (m || span || cands || ncands) {
        return ctx->fail(DK_E_ARG, "period: prefix-probe arguments without dups_out");
    }
    if (period == 0 && !run_out && !probe_out && !count_out && !found_out && !dups_out) return ctx->fail(DK_E_ARG, "period: no part asked for");
    const DbgPeriod a{d_text, n, period, d_next_break, run_out, probe_out, count_p, count_out, search_pmax, found_out, m, span, cands, ncands, dups_out};
    return dbg_period_device(ctx, a);
}
int dk_dbg_dev_initial_sort(dk_ctx *ctx, const uint8_t *d_text, size_t n, const uint8_t code[256], int bits, int spk, const uint8_t inv[256], int narrow, void *d_keys_out,
                            uint32_t *d_sa, uint8_t *d_bwt, uint32_t *d_origin, uint32_t bucket_starts_out[256], uint32_t out[4]) {
    DK_TRY(begin_call(ctx, "dk_dbg_dev_initial_sort"));
    ScopedCall sc(ctx);
    if (!d_text || !code || !d_keys_out || !d_sa || !out) return ctx->fail(DK_E_ARG, "initial_sort: null pointer");
    const bool with_prev = inv && d_bwt && d_origin;
    if (!with_prev && (inv || d_bwt || d_origin)) return ctx->fail(DK_E_ARG, "initial_sort: inv, d_bwt and d_origin are the carry: all three or none");
    if (n == 0 || n > ctx->max_n || n > 0x7FFFFFFEull) return ctx->fail(DK_E_ARG, "initial_sort: text of %zu bytes (1 .. the context capacity %zu)", n, ctx->max_n);
    if (bits < 1 || bits > 8) return ctx->fail(DK_E_ARG, "initial_sort: codes of %d bits (1 .. 8)", bits);
    if (spk < 1 || spk > 64 || bits * spk + (with_prev ? 8 : 0) > 64)
        return ctx->fail(DK_E_ARG, "initial_sort: %d symbols of %d bits%s (at least one, and a key holds 64 bits)", spk, bits, with_prev ? " and the carried byte" : "");
    for (int c = 0; c < 256; ++c)
        if (code[c] >> bits) return ctx->fail(DK_E_ARG, "initial_sort: code[%d] = %d has more than %d bits", c, code[c], bits);
    if (narrow != 0 && narrow != 1) return ctx->fail(DK_E_ARG, "initial_sort: narrow is 0 or 1 (got %d)", narrow);
    if (narrow && bits * spk > 40) return ctx->fail(DK_E_ARG, "initial_sort: narrow keys behind a sort of %d bits (at most 40: five passes)", bits * spk);
    if ((narrow != 0) != (bucket_starts_out != nullptr)) return ctx->fail(DK_E_ARG, "initial_sort: bucket_starts_out goes with narrow keys, and only with them");
    const DbgInitialSort a{d_text, n, code, bits, spk, with_prev ? inv : nullptr, narrow, d_keys_out, d_sa, d_bwt, d_origin, bucket_starts_out};
    return dbg_initial_sort_device(ctx, a, out);
}
int dk_dbg_dev_packed_first(dk_ctx *ctx, const uint8_t *d_text, size_t count, const size_t *n, uint64_t *d_keys, uint32_t *d_vals, uint32_t *d_rank,
                            uint32_t *d_act, uint16_t code[256], uint32_t out[8]) {
    DK_TRY(begin_call(ctx, "dk_dbg_dev_packed_first"));
    ScopedCall sc(ctx);
    if (!d_text || !n || !d_keys || !d_vals || !d_rank || !d_act || !code || !out) return ctx->fail(DK_E_ARG, "packed_first: null pointer");
    Layout lay(count, n);
    DK_TRY(lay.check(ctx));
    Upload up(ctx);
    const uint32_t *d_off = lay.device(up);
    if (!d_off) return up.failed();
    const DbgPackedFirst a{d_text, d_off, count, lay.total(), d_keys, d_vals, d_rank, d_act, code};
    DK_TRY(dbg_packed_first_device(ctx, a, out));
    up.synchronised();  // (the stage ends with a wait)
    return DK_OK;
}
int dk_dbg_dev_packed_round(dk_ctx *ctx, size_t count, const size_t *n, uint32_t h, const uint32_t *d_act, size_t c, uint32_t *d_rank, uint64_t *d_keys,
                            uint32_t *d_vals, uint32_t *d_next_act, uint32_t *d_guard, uint32_t out[8]) {
    DK_TRY(begin_call(ctx, "dk_dbg_dev_packed_round"));
    ScopedCall sc(ctx);
    if (!n || !d_act || !d_rank || !d_keys || !d_vals || !d_next_act || !out) return ctx->fail(DK_E_ARG, "packed_round: null pointer");
    Layout lay(count, n);
    DK_TRY(lay.check(ctx));
    if (c == 0 || c > lay.total()) return ctx->fail(DK_E_ARG, "packed_round: a list of %zu suffixes of a pack of %zu bytes", c, lay.total());
    if (h == 0 || h > (1u << 31)) return ctx->fail(DK_E_ARG, "packed_round: depth %u (1 .. 2^31)", h);
    Upload up(ctx);
    const uint32_t *d_off = lay.device(up);
    if (!d_off) return up.failed();
    const DbgPackedRound a{d_off, count, lay.total(), h, d_act, c, d_rank, d_keys, d_vals, d_next_act, d_guard};
    DK_TRY(dbg_packed_round_device(ctx, a, out));
    up.synchronised();  // (the stage ends with a wait)
    return DK_OK;
}
int dk_dbg_dev_inverse_permutation(dk_ctx *ctx, const uint32_t *d_sa, size_t n, uint32_t *d_rank, const uint32_t *d_marked_val) {
    DK_TRY(begin_call(ctx, "dk_dbg_dev_inverse_permutation"));
    ScopedCall sc(ctx);
    if (!d_sa || !d_rank || n == 0) return ctx->fail(DK_E_ARG, "null pointer or empty input");
    if (n > (size_t(1) << 31)) return ctx->fail(DK_E_ARG, "inverse_permutation: %zu entries (bit 31 of an entry is its mark)", n);
    uint64_t *a = ctx->ws_alloc<uint64_t>(n), *b = a ? ctx->ws_alloc<uint64_t>(n) : nullptr;
    if (!a || !b) return DK_E_NOMEM;
    DK_TRY(inverse_permutation(ctx, d_sa, n, a, b, d_rank, d_marked_val));
    DK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DK_OK;
}
int dk_dbg_sort_pairs(dk_ctx *ctx, uint64_t *keys, uint32_t *vals, size_t count, int begin_bit, int end_bit) {
    DK_TRY(begin_call(ctx, "dk_dbg_sort_pairs"));
    ScopedCall sc(ctx);
    Upload up(ctx);
    if (!keys || !vals || count == 0) return ctx->fail(DK_E_ARG, "null pointer or empty input");
    uint64_t *k0 = ctx->ws_alloc<uint64_t>(count), *k1 = ctx->ws_alloc<uint64_t>(count);
    uint32_t *v0 = ctx->ws_alloc<uint32_t>(count), *v1 = ctx->ws_alloc<uint32_t>(count);
    if (!k0 || !k1 || !v0 || !v1) return DK_E_NOMEM;
    DK_TRY(up.copy(k0, keys, count * 8, "keys"));
    DK_TRY(up.copy(v0, vals, count * 4, "values"));
    DK_TRY(sort_pairs(ctx, k0, k1, v0, v1, count, begin_bit, end_bit));
    DK_HIP(ctx, hipMemcpyAsync(keys, k0, count * 8, hipMemcpyDeviceToHost, ctx->stream));
    DK_HIP(ctx, hipMemcpyAsync(vals, v0, count * 4, hipMemcpyDeviceToHost, ctx->stream));
    DK_TRY(up.sync());
    return DK_OK;
}

}  // extern "C"
