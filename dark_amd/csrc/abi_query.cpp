// extern "C" boundary (include/dark_amd.h), the query entries: LCP arrays, suffix-array check, search and matching statistics, the FM-index.  Thin, as abi.cpp is:
// argument checks, workspace carving, stage sequencing, timing.  An entry names its blocks with a Layout and sends every host array to the
// device through an Upload (abi_common.hpp); the single-block and the packed form of an entry are one body behind two Layouts.
#include <algorithm>
#include <vector>

#include "abi_common.hpp"

using namespace dk;

namespace {

// ---- argument checks more than one entry makes --------------------------------------------------------------------------------------------
uintptr_t addr(const void *p) { return reinterpret_cast<uintptr_t>(p); }
// addrs: the addresses ORed together; subject: "the index is", "the ranges or the positions are" ...
int check_aligned(dk_ctx *ctx, uintptr_t addrs, unsigned bytes, const char *subject) {
    if (addrs & (bytes - 1)) return ctx->fail(DK_E_ARG, "%s not %u-byte aligned", subject, bytes);
    return DK_OK;
}
int check_index(dk_ctx *ctx, const void *d_index) { return check_aligned(ctx, addr(d_index), 4, "the index is"); }
bool good_step(uint32_t step) { return step >= 1 && step <= 4096 && (step & (step - 1)) == 0; }
int check_step(dk_ctx *ctx, uint32_t step) {
    if (!good_step(step)) return ctx->fail(DK_E_ARG, "the sampling step %u is no power of two in [1, 4096]", step);
    return DK_OK;
}
// a sampled structure beside the index (subject: "the locate structure is", "the extract structure is"): its step, then its address
int check_sampled(dk_ctx *ctx, uint32_t step, const void *d_structure, const char *subject) {
    DK_TRY(check_step(ctx, step));
    return check_aligned(ctx, addr(d_structure), 4, subject);
}
// `rows` rows of at most `each` items: 1 .. 2^31 items in all; fmt takes the two numbers
int check_cap(dk_ctx *ctx, size_t rows, size_t each, const char *fmt) {
    if (each == 0 || rows > 0xFFFFFFFEull || each > (size_t(1) << 31) || rows * each > (size_t(1) << 31)) return ctx->fail(DK_E_ARG, fmt, rows, each);
    return DK_OK;
}
int fm_locate_hits(dk_ctx *ctx, size_t npat, size_t max_hits) {
    return check_cap(ctx, npat, max_hits, "%zu patterns of at most %zu hits: 1 .. 2^31 positions in all");
}
int fm_extract_rows(dk_ctx *ctx, size_t nrange, size_t max_len) {
    return check_cap(ctx, nrange, max_len, "%zu ranges of at most %zu bytes: 1 .. 2^31 bytes in all");
}
// the block every item (noun: "pattern", "range") of a packed call names
int check_blocks(dk_ctx *ctx, const uint32_t *block, size_t nitems, size_t count, const char *noun) {
    for (size_t q = 0; q < nitems; ++q)
        if (block[q] >= count) return ctx->fail(DK_E_ARG, "%s %zu names block %u of a pack of %zu", noun, q, block[q], count);
    return DK_OK;
}
// the hit records of find and seams: their number, the (pattern, block) pairs (pairs_fmt takes npat and count) and the records' address --
// align = 16 for records on the device, 1 for the host's, which may stand anywhere
int check_records(dk_ctx *ctx, size_t npat, size_t count, const char *pairs_fmt, size_t max_hits, const void *hits, unsigned align) {
    if (max_hits > (size_t(1) << 31)) return ctx->fail(DK_E_ARG, "at most 2^31 hit records in one call, not %zu", max_hits);
    if (npat > DK_FM_FIND_MAX_PAIRS || npat * count > DK_FM_FIND_MAX_PAIRS) return ctx->fail(DK_E_ARG, pairs_fmt, npat, count);
    if (max_hits && !hits) return ctx->fail(DK_E_ARG, "null pointer");
    return max_hits ? check_aligned(ctx, addr(hits), align, "the hit records are") : DK_OK;
}

// pattern offsets (npat + 1 words) from the caller's lengths, and the checks on the batch
struct Patterns {
    std::vector<uint32_t> off;
    size_t longest = 0, shortest = ~size_t(0);
    size_t count() const { return off.size() - 1; }
    size_t bytes() const { return off.back(); }
    // the batch as the stages take it, d_bytes the items' bytes on the device: the offsets and, where the items name blocks, these go to the
    // workspace (8 bytes per item).  view.d_off null: up.failed()
    ItemView view(Upload &up, const uint8_t *d_bytes, const uint32_t *block = nullptr, const char *blocks_are = "pattern blocks") const {
        ItemView v{d_bytes, up.stage(off.data(), off.size(), "pattern offsets"), nullptr, count(), bytes(), longest, shortest};
        if (block && !(v.d_blk = up.stage(block, count(), blocks_are))) v.d_off = nullptr;
        return v;
    }
};
int check_patterns(dk_ctx *ctx, size_t npat, const size_t *pat_len, const uint32_t *pat_block, size_t count, Patterns &p) {
    if (!pat_len) return ctx->fail(DK_E_ARG, "null pointer");
    if (npat > 0xFFFFFFFEull) return ctx->fail(DK_E_ARG, "%zu patterns in one call", npat);
    p.off.assign(npat + 1, 0);
    uint64_t total = 0;
    for (size_t q = 0; q < npat; ++q) {
        if (pat_block && pat_block[q] >= count) return ctx->fail(DK_E_ARG, "pattern %zu names block %u of %zu", q, pat_block[q], count);
        total += pat_len[q];
        if (pat_len[q] > 0xFFFFFFFFull || total > 0xFFFFFFFFull) return ctx->fail(DK_E_ARG, "the patterns hold more than 2^32 - 1 bytes together");
        p.off[q + 1] = static_cast<uint32_t>(total);
        p.longest = std::max(p.longest, pat_len[q]);
        p.shortest = std::min(p.shortest, pat_len[q]);
    }
    return DK_OK;
}

// The *_run helpers below upload through their caller's guard and run their stage; none of them adds a wait for the stream of its own.  Their
// callers wait, once, behind whatever else they enqueue (sa_check_device has handed its words to the host: nothing is left to wait for).
int lcp_run(Upload &up, const Layout &lay, const uint8_t *d_text, const uint32_t *d_sa, uint32_t *d_lcp) {
    const PackView text = lay.view(up, d_text);
    return text.d_off ? lcp_device(up.c, text, d_sa, d_lcp) : up.failed();
}
// the three words of every block (sa_check_device) -> the first kind that failed and where; where = n_i for a block that is in order
int sa_check_run(Upload &up, const Layout &lay, const uint8_t *d_text, const uint32_t *d_sa, uint32_t *verdict, uint32_t *where) {
    const std::vector<uint32_t> &off = lay.off();
    const PackView text = lay.view(up, d_text);
    if (!text.d_off) return up.failed();
    std::vector<uint32_t> words(3 * lay.count());
    DK_TRY(sa_check_device(up.c, text, d_sa, words.data()));
    up.synchronised();  // (`words` has arrived)
    for (size_t i = 0; i < lay.count(); ++i) {
        const uint32_t *w = &words[3 * i];
        const uint32_t kind = w[0] != 0xFFFFFFFFu ? DK_SA_BAD_RANGE : w[1] != 0xFFFFFFFFu ? DK_SA_NOT_PERMUTATION : w[2] != 0xFFFFFFFFu ? DK_SA_BAD_ORDER : DK_SA_OK;
        verdict[i] = kind;
        where[i] = kind == DK_SA_OK ? off[i + 1] - off[i] : w[kind - 1];
    }
    return DK_OK;
}

// ---- LCP arrays (csrc/lcp.hip) ----------------------------------------------------------------------
int dev_lcp(dk_ctx *ctx, const char *entry, const uint8_t *d_in, Layout &&lay, const uint32_t *d_sa, uint32_t *d_lcp_out) {
    DK_TRY(begin_call(ctx, entry));
    ScopedCall sc(ctx);
    if (!d_in || lay.null() || !d_sa || !d_lcp_out) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(lay.check(ctx));
    Upload up(ctx);
    Timer t;
    ctx->stats.sa_route = 0;
    DK_TRY(lcp_run(up, lay, d_in, d_sa, d_lcp_out));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

}  // namespace

extern "C" {

int dk_dev_lcp(dk_ctx *ctx, const uint8_t *d_in, size_t n, const uint32_t *d_sa, uint32_t *d_lcp_out) {
    return dev_lcp(ctx, "dk_dev_lcp", d_in, Layout(&n), d_sa, d_lcp_out);
}
int dk_dev_lcp_packed(dk_ctx *ctx, const uint8_t *d_in, size_t count, const size_t *n, const uint32_t *d_sa, uint32_t *d_lcp_out) {
    return dev_lcp(ctx, "dk_dev_lcp_packed", d_in, Layout(count, n), d_sa, d_lcp_out);
}

int dk_dev_suffix_array_lcp(dk_ctx *ctx, const uint8_t *d_in, size_t n, uint32_t *d_sa_out, uint32_t *d_lcp_out) {
    DK_TRY(begin_call(ctx, "dk_dev_suffix_array_lcp"));
    ScopedCall sc(ctx);
    if (!d_in || !d_sa_out || !d_lcp_out) return ctx->fail(DK_E_ARG, "null pointer");
    Layout lay(&n);
    DK_TRY(lay.check(ctx));
    Upload up(ctx);
    Timer t;
    const size_t mark = ctx->ws_mark();
    DK_TRY(suffix_array_device(ctx, d_in, n, d_sa_out));
    ctx->ws_release(mark);  // the LCP pass takes the place of the sort's temporaries
    DK_TRY(up.sync());
    ctx->stats.ms_sa = t.ms();
    DK_TRY(lcp_run(up, lay, d_in, d_sa_out, d_lcp_out));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dk_suffix_array_lcp(dk_ctx *ctx, const uint8_t *in, size_t n, uint32_t *sa_out, uint32_t *lcp_out) {
    DK_TRY(begin_call(ctx, "dk_suffix_array_lcp"));
    ScopedCall sc(ctx);
    if (!in || !sa_out || !lcp_out) return ctx->fail(DK_E_ARG, "null pointer");
    Layout lay(&n);
    DK_TRY(lay.check(ctx));
    Upload up(ctx);
    Timer t;
    hipStream_t st = ctx->stream;
    uint8_t *d_text = up.stage(in, n, "text");
    uint32_t *d_sa = ctx->ws_alloc<uint32_t>(n);
    if (!d_text || !d_sa) return up.failed();
    const size_t mark = ctx->ws_mark();
    DK_TRY(suffix_array_device(ctx, d_text, n, d_sa));
    ctx->ws_release(mark);
    uint32_t *d_lcp = ctx->ws_alloc<uint32_t>(n);  // (after the sort: its 63.4 n and the 9 n around it would not fit together)
    if (!d_lcp) return DK_E_NOMEM;
    DK_TRY(lcp_run(up, lay, d_text, d_sa, d_lcp));
    DK_HIP(ctx, hipMemcpyAsync(sa_out, d_sa, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DK_HIP(ctx, hipMemcpyAsync(lcp_out, d_lcp, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dk_dev_suffix_array_packed_lcp(dk_ctx *ctx, const uint8_t *d_in, size_t count, const size_t *n, uint32_t *d_sa_out, uint32_t *d_lcp_out) {
    DK_TRY(begin_call(ctx, "dk_dev_suffix_array_packed_lcp"));
    ScopedCall sc(ctx);
    if (!d_in || !n || !d_sa_out || !d_lcp_out) return ctx->fail(DK_E_ARG, "null pointer");
    Layout lay(count, n);
    DK_TRY(lay.check(ctx));
    Upload up(ctx);
    Timer t;
    const PackView text = lay.view(up, d_in);
    uint32_t *d_phi = ctx->ws_alloc<uint32_t>(lay.total());
    if (!text.d_off || !d_phi) return up.failed();
    std::vector<std::pair<size_t, uint32_t>> fixed;
    DK_TRY(packed_forward(ctx, d_in, lay.off(), text.d_off, nullptr, nullptr, &fixed, d_sa_out, d_phi));
    DK_TRY(lcp_device(ctx, text, d_sa_out, d_lcp_out, d_phi));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dk_suffix_array_packed_lcp(dk_ctx *ctx, const uint8_t *in, size_t count, const size_t *n, uint32_t *sa_out, uint32_t *lcp_out) {
    DK_TRY(begin_call(ctx, "dk_suffix_array_packed_lcp"));
    ScopedCall sc(ctx);
    if (!in || !n || !sa_out || !lcp_out) return ctx->fail(DK_E_ARG, "null pointer");
    Layout lay(count, n);
    DK_TRY(lay.check(ctx));
    Upload up(ctx);
    Timer t;
    hipStream_t st = ctx->stream;
    const size_t total = lay.total();
    uint8_t *d_text = up.stage(in, total, "text");
    uint32_t *d_sa = ctx->ws_alloc<uint32_t>(total), *d_phi = ctx->ws_alloc<uint32_t>(total);
    const PackView text = lay.view(up, d_text);
    if (!d_text || !d_sa || !d_phi || !text.d_off) return up.failed();
    std::vector<std::pair<size_t, uint32_t>> fixed;
    DK_TRY(packed_forward(ctx, d_text, lay.off(), text.d_off, nullptr, nullptr, &fixed, d_sa, d_phi));
    // (after the sort and its guard: text, SA and Phi are 9 total, and a guarded block's sort 63.4 n_i with n_i <= 2^24 -- the constant term covers
    //  the 2.8 n_i by which a pack that is one such block would pass 69.6 total)
    uint32_t *d_lcp = ctx->ws_alloc<uint32_t>(total);
    if (!d_lcp) return DK_E_NOMEM;
    DK_TRY(lcp_device(ctx, text, d_sa, d_lcp, d_phi));
    DK_HIP(ctx, hipMemcpyAsync(sa_out, d_sa, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DK_HIP(ctx, hipMemcpyAsync(lcp_out, d_lcp, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

// ---- suffix-array check and search (csrc/sa_query.hip) -----------------------------------------------
}  // extern "C"

namespace {
int dev_sa_check(dk_ctx *ctx, const char *entry, const uint8_t *d_in, Layout &&lay, const uint32_t *d_sa, uint32_t *verdict, uint32_t *where) {
    DK_TRY(begin_call(ctx, entry));
    ScopedCall sc(ctx);
    if (!d_in || lay.null() || !d_sa || !verdict || !where) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(lay.check(ctx));
    Upload up(ctx);
    Timer t;
    DK_TRY(sa_check_run(up, lay, d_in, d_sa, verdict, where));
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}
int dev_sa_search(dk_ctx *ctx, const char *entry, const uint8_t *d_in, Layout &&lay, const uint32_t *d_sa, const uint8_t *d_pat, size_t npat,
                  const size_t *pat_len, const uint32_t *pat_block, uint32_t *d_lo, uint32_t *d_hi) {
    DK_TRY(begin_call(ctx, entry));
    ScopedCall sc(ctx);
    if (!d_in || lay.null() || !d_sa) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(lay.check(ctx));
    if (npat == 0) return DK_OK;
    if (lay.packed() && !pat_block) return ctx->fail(DK_E_ARG, "null pointer");
    Timer t;
    Patterns p;
    DK_TRY(check_patterns(ctx, npat, pat_len, pat_block, lay.count(), p));
    if ((!d_pat && p.bytes()) || !d_lo || !d_hi) return ctx->fail(DK_E_ARG, "null pointer");
    Upload up(ctx);
    const PackView text = lay.view(up, d_in);
    const ItemView pats = p.view(up, d_pat, pat_block);
    if (!text.d_off || !pats.d_off) return up.failed();
    DK_TRY(sa_search_device(ctx, text, d_sa, pats, d_lo, d_hi));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}
}  // namespace

extern "C" {

int dk_dev_sa_check(dk_ctx *ctx, const uint8_t *d_in, size_t n, const uint32_t *d_sa, uint32_t *verdict, uint32_t *where) {
    return dev_sa_check(ctx, "dk_dev_sa_check", d_in, Layout(&n), d_sa, verdict, where);
}
int dk_dev_sa_check_packed(dk_ctx *ctx, const uint8_t *d_in, size_t count, const size_t *n, const uint32_t *d_sa, uint32_t *verdict, uint32_t *where) {
    return dev_sa_check(ctx, "dk_dev_sa_check_packed", d_in, Layout(count, n), d_sa, verdict, where);
}

int dk_sa_check(dk_ctx *ctx, const uint8_t *in, size_t n, const uint32_t *sa, uint32_t *verdict, uint32_t *where) {
    DK_TRY(begin_call(ctx, "dk_sa_check"));
    ScopedCall sc(ctx);
    if (!in || !sa || !verdict || !where) return ctx->fail(DK_E_ARG, "null pointer");
    Layout lay(&n);
    DK_TRY(lay.check(ctx));
    Upload up(ctx);
    Timer t;
    const uint8_t *d_text = up.stage(in, n, "text");
    const uint32_t *d_sa = up.stage(sa, n, "suffix array");
    if (!d_text || !d_sa) return up.failed();
    DK_TRY(sa_check_run(up, lay, d_text, d_sa, verdict, where));
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dk_dev_sa_search(dk_ctx *ctx, const uint8_t *d_in, size_t n, const uint32_t *d_sa, const uint8_t *d_pat, size_t npat, const size_t *pat_len,
                     uint32_t *d_lo, uint32_t *d_hi) {
    return dev_sa_search(ctx, "dk_dev_sa_search", d_in, Layout(&n), d_sa, d_pat, npat, pat_len, nullptr, d_lo, d_hi);
}
int dk_dev_sa_search_packed(dk_ctx *ctx, const uint8_t *d_in, size_t count, const size_t *n, const uint32_t *d_sa, const uint8_t *d_pat, size_t npat,
                            const size_t *pat_len, const uint32_t *pat_block, uint32_t *d_lo, uint32_t *d_hi) {
    return dev_sa_search(ctx, "dk_dev_sa_search_packed", d_in, Layout(count, n), d_sa, d_pat, npat, pat_len, pat_block, d_lo, d_hi);
}

int dk_sa_search(dk_ctx *ctx, const uint8_t *in, size_t n, const uint32_t *sa, const uint8_t *pat, size_t npat, const size_t *pat_len, uint32_t *lo,
                 uint32_t *hi) {
    DK_TRY(begin_call(ctx, "dk_sa_search"));
    ScopedCall sc(ctx);
    if (!in || !sa) return ctx->fail(DK_E_ARG, "null pointer");
    Layout lay(&n);
    DK_TRY(lay.check(ctx));
    if (npat == 0) return DK_OK;
    Timer t;
    Patterns p;
    DK_TRY(check_patterns(ctx, npat, pat_len, nullptr, 1, p));
    if ((!pat && p.bytes()) || !lo || !hi) return ctx->fail(DK_E_ARG, "null pointer");
    // text n, SA 4 n, the two offsets of the block; then the patterns, their offsets and the two results
    const size_t need = ws_round(n) + ws_round(4 * n) + 256 + ws_round(p.bytes()) + ws_round(4 * (npat + 1)) + 2 * ws_round(4 * npat);
    if (need > ctx->ws_size) return ctx->fail(DK_E_ARG, "%zu patterns of %zu bytes and their offsets do not fit the workspace beside the block", npat, p.bytes());
    Upload up(ctx);
    hipStream_t st = ctx->stream;
    const uint8_t *d_text = up.stage(in, n, "text"), *d_pat = up.stage(pat, p.bytes(), "patterns");
    const uint32_t *d_sa = up.stage(sa, n, "suffix array");
    uint32_t *d_lo = ctx->ws_alloc<uint32_t>(npat), *d_hi = ctx->ws_alloc<uint32_t>(npat);
    if (!d_text || !d_pat || !d_sa || !d_lo || !d_hi) return up.failed();
    const PackView text = lay.view(up, d_text);
    const ItemView pats = p.view(up, d_pat);
    if (!text.d_off || !pats.d_off) return up.failed();
    DK_TRY(sa_search_device(ctx, text, d_sa, pats, d_lo, d_hi));
    DK_HIP(ctx, hipMemcpyAsync(lo, d_lo, npat * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DK_HIP(ctx, hipMemcpyAsync(hi, d_hi, npat * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

// ---- matching statistics and super-maximal matches (csrc/sa_query.hip) ------------------------------------------------
}  // extern "C"

namespace {
// what the two device entries check in front of the queries themselves
int check_match_call(dk_ctx *ctx, const uint8_t *d_in, Layout &lay, const uint32_t *d_sa, size_t max_len) {
    if (!d_in || lay.null() || !d_sa) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(lay.check(ctx));
    if (max_len == 0) return ctx->fail(DK_E_ARG, "max_len is 0: a window holds one byte at least");
    return DK_OK;
}
int check_match_outputs(dk_ctx *ctx, const void *query, const void *len, const void *lo, const void *hi) {
    if (!query || !len) return ctx->fail(DK_E_ARG, "null pointer");
    if (!lo != !hi) return ctx->fail(DK_E_ARG, "one of the two range arrays is null: both, or neither for the lengths alone");
    return DK_OK;
}
int dev_sa_match(dk_ctx *ctx, const char *entry, const uint8_t *d_in, Layout &&lay, const uint32_t *d_sa, const uint8_t *d_query, size_t nq,
                 const size_t *query_len, const uint32_t *query_block, size_t max_len, uint32_t *d_len, uint32_t *d_lo, uint32_t *d_hi) {
    DK_TRY(begin_call(ctx, entry));
    ScopedCall sc(ctx);
    DK_TRY(check_match_call(ctx, d_in, lay, d_sa, max_len));
    if (nq == 0) return DK_OK;
    if (lay.packed() && !query_block) return ctx->fail(DK_E_ARG, "null pointer");
    Timer t;
    Patterns p;
    DK_TRY(check_patterns(ctx, nq, query_len, query_block, lay.count(), p));
    if (p.bytes() == 0) return DK_OK;
    DK_TRY(check_match_outputs(ctx, d_query, d_len, d_lo, d_hi));
    Upload up(ctx);
    const PackView text = lay.view(up, d_in);
    const ItemView qry = p.view(up, d_query, query_block, "query blocks");
    if (!text.d_off || !qry.d_off) return up.failed();
    DK_TRY(sa_match_device(ctx, text, d_sa, qry, max_len, d_len, d_lo, d_hi));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}
int dev_sa_smems(dk_ctx *ctx, const char *entry, const uint8_t *d_in, Layout &&lay, const uint32_t *d_sa, const uint8_t *d_query, size_t nq,
                 const size_t *query_len, const uint32_t *query_block, size_t min_len, size_t max_len, size_t max_hits, dk_sa_smem *d_hits,
                 uint64_t *total) {
    DK_TRY(begin_call(ctx, entry));
    ScopedCall sc(ctx);
    DK_TRY(check_match_call(ctx, d_in, lay, d_sa, max_len));
    if (!total || (max_hits && !d_hits)) return ctx->fail(DK_E_ARG, "null pointer");
    if (max_hits) DK_TRY(check_aligned(ctx, addr(d_hits), 16, "the match records are"));
    if (nq == 0) {
        *total = 0;
        return DK_OK;
    }
    if (lay.packed() && !query_block) return ctx->fail(DK_E_ARG, "null pointer");
    Timer t;
    Patterns p;
    DK_TRY(check_patterns(ctx, nq, query_len, query_block, lay.count(), p));
    if (p.bytes() == 0) {
        *total = 0;
        return DK_OK;
    }
    if (!d_query) return ctx->fail(DK_E_ARG, "null pointer");
    if (ws_round(4 * (lay.count() + 1)) + ws_round(4 * (nq + 1)) + (query_block ? ws_round(4 * nq) : 0) + sa_smems_workspace(p.bytes()) > ctx->ws_size)
        return ctx->fail(DK_E_ARG, "%zu queries of %zu bytes do not fit the workspace (16 bytes per query byte)", nq, p.bytes());
    Upload up(ctx);
    const PackView text = lay.view(up, d_in);
    const ItemView qry = p.view(up, d_query, query_block, "query blocks");
    if (!text.d_off || !qry.d_off) return up.failed();
    DK_TRY(sa_smems_device(ctx, text, d_sa, qry, min_len, max_len, HitSink{max_hits, d_hits, nullptr, total}));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}
}  // namespace

extern "C" {

int dk_dev_sa_match(dk_ctx *ctx, const uint8_t *d_in, size_t n, const uint32_t *d_sa, const uint8_t *d_query, size_t nq, const size_t *query_len,
                    size_t max_len, uint32_t *d_len, uint32_t *d_lo, uint32_t *d_hi) {
    return dev_sa_match(ctx, "dk_dev_sa_match", d_in, Layout(&n), d_sa, d_query, nq, query_len, nullptr, max_len, d_len, d_lo, d_hi);
}
int dk_dev_sa_match_packed(dk_ctx *ctx, const uint8_t *d_in, size_t count, const size_t *n, const uint32_t *d_sa, const uint8_t *d_query, size_t nq,
                           const size_t *query_len, const uint32_t *query_block, size_t max_len, uint32_t *d_len, uint32_t *d_lo, uint32_t *d_hi) {
    return dev_sa_match(ctx, "dk_dev_sa_match_packed", d_in, Layout(count, n), d_sa, d_query, nq, query_len, query_block, max_len, d_len, d_lo, d_hi);
}
int dk_dev_sa_smems(dk_ctx *ctx, const uint8_t *d_in, size_t n, const uint32_t *d_sa, const uint8_t *d_query, size_t nq, const size_t *query_len,
                    size_t min_len, size_t max_len, size_t max_hits, dk_sa_smem *d_hits, uint64_t *total) {
    return dev_sa_smems(ctx, "dk_dev_sa_smems", d_in, Layout(&n), d_sa, d_query, nq, query_len, nullptr, min_len, max_len, max_hits, d_hits, total);
}
int dk_dev_sa_smems_packed(dk_ctx *ctx, const uint8_t *d_in, size_t count, const size_t *n, const uint32_t *d_sa, const uint8_t *d_query, size_t nq,
                           const size_t *query_len, const uint32_t *query_block, size_t min_len, size_t max_len, size_t max_hits, dk_sa_smem *d_hits,
                           uint64_t *total) {
    return dev_sa_smems(ctx, "dk_dev_sa_smems_packed", d_in, Layout(count, n), d_sa, d_query, nq, query_len, query_block, min_len, max_len, max_hits,
                        d_hits, total);
}

int dk_sa_match(dk_ctx *ctx, const uint8_t *in, size_t n, const uint32_t *sa, const uint8_t *query, size_t nq, const size_t *query_len, size_t max_len,
                uint32_t *len, uint32_t *lo, uint32_t *hi) {
    DK_TRY(begin_call(ctx, "dk_sa_match"));
    ScopedCall sc(ctx);
    Layout lay(&n);
    DK_TRY(check_match_call(ctx, in, lay, sa, max_len));
    if (nq == 0) return DK_OK;
    Timer t;
    Patterns p;
    DK_TRY(check_patterns(ctx, nq, query_len, nullptr, 1, p));
    const size_t Q = p.bytes();
    if (Q == 0) return DK_OK;
    DK_TRY(check_match_outputs(ctx, query, len, lo, hi));
    // text n, SA 4 n, the two offsets of the block; then the queries, their offsets and the results
    const size_t need = ws_round(n) + ws_round(4 * n) + 256 + ws_round(Q) + ws_round(4 * (nq + 1)) + (lo ? 3 : 1) * ws_round(4 * Q);
    if (need > ctx->ws_size) return ctx->fail(DK_E_ARG, "%zu queries of %zu bytes and their statistics do not fit the workspace beside the block", nq, Q);
    Upload up(ctx);
    hipStream_t st = ctx->stream;
    const uint8_t *d_text = up.stage(in, n, "text"), *d_query = up.stage(query, Q, "queries");
    const uint32_t *d_sa = up.stage(sa, n, "suffix array");
    uint32_t *d_len = ctx->ws_alloc<uint32_t>(Q), *d_lo = lo ? ctx->ws_alloc<uint32_t>(Q) : nullptr, *d_hi = lo ? ctx->ws_alloc<uint32_t>(Q) : nullptr;
    if (!d_text || !d_query || !d_sa || !d_len || (lo && (!d_lo || !d_hi))) return up.failed();
    const PackView text = lay.view(up, d_text);
    const ItemView qry = p.view(up, d_query);
    if (!text.d_off || !qry.d_off) return up.failed();
    DK_TRY(sa_match_device(ctx, text, d_sa, qry, max_len, d_len, d_lo, d_hi));
    DK_HIP(ctx, hipMemcpyAsync(len, d_len, Q * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (lo) {
        DK_HIP(ctx, hipMemcpyAsync(lo, d_lo, Q * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        DK_HIP(ctx, hipMemcpyAsync(hi, d_hi, Q * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dk_sa_smems(dk_ctx *ctx, const uint8_t *in, size_t n, const uint32_t *sa, const uint8_t *query, size_t nq, const size_t *query_len, size_t min_len,
                size_t max_len, size_t max_hits, dk_sa_smem *hits, uint64_t *total) {
    DK_TRY(begin_call(ctx, "dk_sa_smems"));
    ScopedCall sc(ctx);
    Layout lay(&n);
    DK_TRY(check_match_call(ctx, in, lay, sa, max_len));
    if (!total || (max_hits && !hits)) return ctx->fail(DK_E_ARG, "null pointer");
    *total = 0;
    if (nq == 0) return DK_OK;
    Timer t;
    Patterns p;
    DK_TRY(check_patterns(ctx, nq, query_len, nullptr, 1, p));
    const size_t Q = p.bytes();
    if (Q == 0) return DK_OK;
    if (!query) return ctx->fail(DK_E_ARG, "null pointer");
    // text n, SA 4 n, the two offsets of the block; the queries and their offsets; the stage's workspace; the records -- never more than positions
    const size_t cap = std::min(max_hits, Q);
    const size_t need = ws_round(n) + ws_round(4 * n) + 256 + ws_round(Q) + ws_round(4 * (nq + 1)) + sa_smems_workspace(Q) + ws_round(16 * cap);
    if (need > ctx->ws_size)
        return ctx->fail(DK_E_ARG, "%zu queries of %zu bytes and %zu match records do not fit the workspace beside the block", nq, Q, cap);
    Upload up(ctx);
    const uint8_t *d_text = up.stage(in, n, "text"), *d_query = up.stage(query, Q, "queries");
    const uint32_t *d_sa = up.stage(sa, n, "suffix array");
    dk_sa_smem *d_hits = cap ? ctx->ws_alloc<dk_sa_smem>(cap) : nullptr;
    if (!d_text || !d_query || !d_sa || (cap && !d_hits)) return up.failed();
    const PackView text = lay.view(up, d_text);
    const ItemView qry = p.view(up, d_query);
    if (!text.d_off || !qry.d_off) return up.failed();
    DK_TRY(sa_smems_device(ctx, text, d_sa, qry, min_len, max_len, HitSink{cap, d_hits, nullptr, total}));
    const size_t nhits = static_cast<size_t>(std::min<uint64_t>(*total, cap));
    if (nhits) DK_HIP(ctx, hipMemcpyAsync(hits, d_hits, nhits * sizeof(dk_sa_smem), hipMemcpyDeviceToHost, ctx->stream));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

// ---- FM-index (csrc/fm_index.hip).  Served by contexts of either purpose: begin_call without a forward entry. --------
}  // extern "C"

namespace {
// What the host-pointer forms (dk_fm_count, _locate, _extract, _find) share: the block's L staged, its index allocated and built, beside it the
// sampled structure asked for, the block's two offsets -> fm.  The builds take their workspace on top of what the caller holds by then.
enum Sampled { JUST_INDEX, WITH_LOCATE, WITH_EXTRACT };
int host_fm(Upload &up, const Layout &lay, const uint8_t *bwt, uint32_t origin, uint32_t step, Sampled sampled, FmView &fm) {
    const size_t n = lay.total();
    uint32_t *d_index = up.c->ws_alloc<uint32_t>(fm_index_words(n, 1));
    uint32_t *d_loc = sampled == WITH_LOCATE ? up.c->ws_alloc<uint32_t>(fm_locate_words(n, 1, step)) : nullptr;
    uint32_t *d_ext = sampled == WITH_EXTRACT ? up.c->ws_alloc<uint32_t>(fm_extract_words(n, 1, step)) : nullptr;
    fm = FmView{lay.view(up, up.stage(bwt, n, "L")), d_index, d_loc, d_ext, step};
    if (!fm.L.bytes || !fm.L.d_off || !d_index || (sampled == WITH_LOCATE && !d_loc) || (sampled == WITH_EXTRACT && !d_ext)) return up.failed();
    DK_TRY(fm_build_device(up.c, fm.L.bytes, lay.off(), &origin, d_index));
    if (d_loc) DK_TRY(fm_locate_build_device(up.c, fm.L.bytes, lay.off(), &origin, step, d_loc, false));
    if (d_ext) DK_TRY(fm_extract_build_device(up.c, fm.L.bytes, lay.off(), &origin, step, d_ext, false));
    return DK_OK;
}
int dev_fm_build(dk_ctx *ctx, const uint8_t *d_bwt, Layout &&lay, const uint32_t *origin, void *d_index) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    if (!d_bwt || lay.null() || !origin || !d_index) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_index(ctx, d_index));
    DK_TRY(lay.check(ctx));
    DK_TRY(lay.check_origins(ctx, origin));
    Timer t;
    DK_TRY(fm_build_device(ctx, d_bwt, lay.off(), origin, d_index));
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}
int dev_fm_count(dk_ctx *ctx, const uint8_t *d_bwt, Layout &&lay, const void *d_index, const uint8_t *d_pat, size_t npat, const size_t *pat_len,
                 const uint32_t *pat_block, uint32_t *d_lo, uint32_t *d_hi) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    if (!d_bwt || lay.null() || !d_index) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_index(ctx, d_index));
    DK_TRY(lay.check(ctx));
    if (npat == 0) return DK_OK;
    if (lay.packed() && !pat_block) return ctx->fail(DK_E_ARG, "null pointer");
    Timer t;
    Patterns p;
    DK_TRY(check_patterns(ctx, npat, pat_len, pat_block, lay.count(), p));
    if ((!d_pat && p.bytes()) || !d_lo || !d_hi) return ctx->fail(DK_E_ARG, "null pointer");
    Upload up(ctx);
    const FmView fm{lay.view(up, d_bwt), d_index};
    const ItemView pats = p.view(up, d_pat, pat_block);
    if (!fm.L.d_off || !pats.d_off) return up.failed();
    DK_TRY(fm_count_device(ctx, fm, pats, d_lo, d_hi));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}
}  // namespace

extern "C" {

size_t dk_fm_index_bytes(size_t total, size_t count) {
    if (total == 0 || total > 0x7FFFFFFEull || count == 0 || count > DK_PACKED_MAX_BLOCKS || count > total) return 0;
    return fm_index_words(total, count) * sizeof(uint32_t);
}

int dk_dev_fm_build(dk_ctx *ctx, const uint8_t *d_bwt, size_t n, uint32_t origin, void *d_index) {
    return dev_fm_build(ctx, d_bwt, Layout(&n), &origin, d_index);
}
int dk_dev_fm_build_packed(dk_ctx *ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const uint32_t *origin, void *d_index) {
    return dev_fm_build(ctx, d_bwt, Layout(count, n), origin, d_index);
}

int dk_dev_fm_count(dk_ctx *ctx, const uint8_t *d_bwt, size_t n, const void *d_index, const uint8_t *d_pat, size_t npat, const size_t *pat_len,
                    uint32_t *d_lo, uint32_t *d_hi) {
    return dev_fm_count(ctx, d_bwt, Layout(&n), d_index, d_pat, npat, pat_len, nullptr, d_lo, d_hi);
}
int dk_dev_fm_count_packed(dk_ctx *ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const void *d_index, const uint8_t *d_pat, size_t npat,
                           const size_t *pat_len, const uint32_t *pat_block, uint32_t *d_lo, uint32_t *d_hi) {
    return dev_fm_count(ctx, d_bwt, Layout(count, n), d_index, d_pat, npat, pat_len, pat_block, d_lo, d_hi);
}

int dk_fm_count(dk_ctx *ctx, const uint8_t *bwt, size_t n, uint32_t origin, const uint8_t *pat, size_t npat, const size_t *pat_len, uint32_t *lo,
                uint32_t *hi) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    if (!bwt) return ctx->fail(DK_E_ARG, "null pointer");
    Layout lay(&n);
    DK_TRY(lay.check(ctx));
    DK_TRY(lay.check_origins(ctx, &origin));
    if (npat == 0) return DK_OK;
    Timer t;
    Patterns p;
    DK_TRY(check_patterns(ctx, npat, pat_len, nullptr, 1, p));
    if ((!pat && p.bytes()) || !lo || !hi) return ctx->fail(DK_E_ARG, "null pointer");
    // L n, the index, the two offsets of the block; then the patterns, their offsets and the two results; the build's workspace while it runs
    const size_t index_words = fm_index_words(n, 1);
    const size_t need = ws_round(n) + ws_round(4 * index_words) + 256 + ws_round(p.bytes()) + ws_round(4 * (npat + 1)) + 2 * ws_round(4 * npat) + fm_build_workspace(n, 1);
    if (need > ctx->ws_size) return ctx->fail(DK_E_ARG, "%zu patterns of %zu bytes and their offsets do not fit the workspace beside L and its index", npat, p.bytes());
    Upload up(ctx);
    hipStream_t st = ctx->stream;
    const uint8_t *d_pat = up.stage(pat, p.bytes(), "patterns");
    uint32_t *d_lo = ctx->ws_alloc<uint32_t>(npat), *d_hi = ctx->ws_alloc<uint32_t>(npat);
    if (!d_pat || !d_lo || !d_hi) return up.failed();
    FmView fm;
    DK_TRY(host_fm(up, lay, bwt, origin, 0, JUST_INDEX, fm));
    const ItemView pats = p.view(up, d_pat);
    if (!pats.d_off) return up.failed();
    DK_TRY(fm_count_device(ctx, fm, pats, d_lo, d_hi));
    DK_HIP(ctx, hipMemcpyAsync(lo, d_lo, npat * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DK_HIP(ctx, hipMemcpyAsync(hi, d_hi, npat * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

// ---- locate and extract (4.15): a sampled structure beside the index, built from (L, origin) alone ---------------------
}  // extern "C"

namespace {
const char LOCATE_IS[] = "the locate structure is", EXTRACT_IS[] = "the extract structure is";
using SampledBuild = int (*)(dk_ctx *, const uint8_t *, const std::vector<uint32_t> &, const uint32_t *, uint32_t, void *, bool);
int dev_fm_sampled_build(dk_ctx *ctx, const uint8_t *d_bwt, Layout &&lay, const uint32_t *origin, uint32_t step, void *d_structure, const char *subject,
                         SampledBuild build) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    if (!d_bwt || lay.null() || !origin || !d_structure) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_sampled(ctx, step, d_structure, subject));
    DK_TRY(lay.check(ctx));
    DK_TRY(lay.check_origins(ctx, origin));
    Timer t;
    DK_TRY(build(ctx, d_bwt, lay.off(), origin, step, d_structure, lay.packed()));
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dev_fm_locate(dk_ctx *ctx, const uint8_t *d_bwt, Layout &&lay, const void *d_index, const void *d_loc, uint32_t step, const uint32_t *d_lo,
                  const uint32_t *d_hi, size_t npat, const uint32_t *pat_block, size_t max_hits, uint32_t *d_pos) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    if (!d_bwt || lay.null() || !d_index || !d_loc) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_index(ctx, d_index));
    DK_TRY(check_sampled(ctx, step, d_loc, LOCATE_IS));
    DK_TRY(lay.check(ctx));
    if (npat == 0) return DK_OK;
    DK_TRY(fm_locate_hits(ctx, npat, max_hits));
    if ((lay.packed() && !pat_block) || !d_lo || !d_hi || !d_pos) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_aligned(ctx, addr(d_lo) | addr(d_hi) | addr(d_pos), 4, "the ranges or the positions are"));
    if (lay.packed()) DK_TRY(check_blocks(ctx, pat_block, npat, lay.count(), "pattern"));
    Upload up(ctx);
    Timer t;
    const FmView fm{lay.view(up, d_bwt), d_index, d_loc, nullptr, step};
    const uint32_t *d_blk = lay.packed() ? up.stage(pat_block, npat, "pattern blocks") : nullptr;
    if (!fm.L.d_off || (lay.packed() && !d_blk)) return up.failed();
    DK_TRY(fm_locate_device(ctx, fm, d_lo, d_hi, d_blk, npat, max_hits, d_pos));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dev_fm_extract(dk_ctx *ctx, const uint8_t *d_bwt, Layout &&lay, const void *d_index, const void *d_ext, uint32_t step, const uint32_t *d_pos,
                   const uint32_t *d_len, size_t nrange, const uint32_t *range_block, size_t max_len, uint8_t *d_out) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    if (!d_bwt || lay.null() || !d_index || !d_ext) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_index(ctx, d_index));
    DK_TRY(check_sampled(ctx, step, d_ext, EXTRACT_IS));
    DK_TRY(lay.check(ctx));
    if (nrange == 0) return DK_OK;
    DK_TRY(fm_extract_rows(ctx, nrange, max_len));
    if ((lay.packed() && !range_block) || !d_pos || !d_out) return ctx->fail(DK_E_ARG, "null pointer");  // (d_len may be null: every range max_len long)
    DK_TRY(check_aligned(ctx, addr(d_pos) | addr(d_len), 4, "the positions or the lengths are"));
    if (lay.packed()) DK_TRY(check_blocks(ctx, range_block, nrange, lay.count(), "range"));
    Upload up(ctx);
    Timer t;
    // a pack: the offsets and the anchor bases in one array; a single block has the base 0 and needs none
    FmView fm{lay.packed() ? PackView{d_bwt, nullptr, lay.count(), lay.total()} : lay.view(up, d_bwt), d_index, nullptr, d_ext, step};
    if (lay.packed()) lay.device_with_bases(up, fm);
    const uint32_t *d_blk = lay.packed() ? up.stage(range_block, nrange, "range blocks") : nullptr;
    if (!fm.L.d_off || (lay.packed() && !d_blk)) return up.failed();
    DK_TRY(fm_extract_device(ctx, fm, d_pos, d_len, d_blk, nrange, max_len, d_out));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}
}  // namespace

extern "C" {

size_t dk_fm_locate_bytes(size_t total, size_t count, uint32_t step) {
    if (dk_fm_index_bytes(total, count) == 0 || !good_step(step)) return 0;
    return fm_locate_words(total, count, step) * sizeof(uint32_t);
}
size_t dk_fm_extract_bytes(size_t total, size_t count, uint32_t step) {
    if (dk_fm_index_bytes(total, count) == 0 || !good_step(step)) return 0;
    return fm_extract_words(total, count, step) * sizeof(uint32_t);
}

int dk_dev_fm_locate_build(dk_ctx *ctx, const uint8_t *d_bwt, size_t n, uint32_t origin, uint32_t step, void *d_loc) {
    return dev_fm_sampled_build(ctx, d_bwt, Layout(&n), &origin, step, d_loc, LOCATE_IS, fm_locate_build_device);
}
int dk_dev_fm_locate_build_packed(dk_ctx *ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const uint32_t *origin, uint32_t step, void *d_loc) {
    return dev_fm_sampled_build(ctx, d_bwt, Layout(count, n), origin, step, d_loc, LOCATE_IS, fm_locate_build_device);
}
int dk_dev_fm_extract_build(dk_ctx *ctx, const uint8_t *d_bwt, size_t n, uint32_t origin, uint32_t step, void *d_ext) {
    return dev_fm_sampled_build(ctx, d_bwt, Layout(&n), &origin, step, d_ext, EXTRACT_IS, fm_extract_build_device);
}
int dk_dev_fm_extract_build_packed(dk_ctx *ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const uint32_t *origin, uint32_t step, void *d_ext) {
    return dev_fm_sampled_build(ctx, d_bwt, Layout(count, n), origin, step, d_ext, EXTRACT_IS, fm_extract_build_device);
}

int dk_dev_fm_locate(dk_ctx *ctx, const uint8_t *d_bwt, size_t n, const void *d_index, const void *d_loc, uint32_t step, const uint32_t *d_lo,
                     const uint32_t *d_hi, size_t npat, size_t max_hits, uint32_t *d_pos) {
    return dev_fm_locate(ctx, d_bwt, Layout(&n), d_index, d_loc, step, d_lo, d_hi, npat, nullptr, max_hits, d_pos);
}
int dk_dev_fm_locate_packed(dk_ctx *ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const void *d_index, const void *d_loc, uint32_t step,
                            const uint32_t *d_lo, const uint32_t *d_hi, size_t npat, const uint32_t *pat_block, size_t max_hits, uint32_t *d_pos) {
    return dev_fm_locate(ctx, d_bwt, Layout(count, n), d_index, d_loc, step, d_lo, d_hi, npat, pat_block, max_hits, d_pos);
}

int dk_fm_locate(dk_ctx *ctx, const uint8_t *bwt, size_t n, uint32_t origin, uint32_t step, const uint8_t *pat, size_t npat, const size_t *pat_len,
                 size_t max_hits, uint32_t *lo, uint32_t *hi, uint32_t *pos) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    if (!bwt) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_step(ctx, step));
    Layout lay(&n);
    DK_TRY(lay.check(ctx));
    DK_TRY(lay.check_origins(ctx, &origin));
    if (npat == 0) return DK_OK;
    DK_TRY(fm_locate_hits(ctx, npat, max_hits));
    Timer t;
    Patterns p;
    DK_TRY(check_patterns(ctx, npat, pat_len, nullptr, 1, p));
    if ((!pat && p.bytes()) || !lo || !hi || !pos) return ctx->fail(DK_E_ARG, "null pointer");
    // L, the index, the structure and the block's two offsets; the patterns, their offsets, the two results and the positions; the larger of
    // the two builds' workspaces while it runs
    const size_t index_words = fm_index_words(n, 1), loc_words = fm_locate_words(n, 1, step), nitems = npat * max_hits;
    const size_t need = ws_round(n) + ws_round(4 * index_words) + ws_round(4 * loc_words) + 256 + ws_round(p.bytes()) + ws_round(4 * (npat + 1)) +
                        2 * ws_round(4 * npat) + ws_round(4 * nitems) + std::max(fm_build_workspace(n, 1), fm_locate_build_workspace(n, 1));
    if (need > ctx->ws_size)
        return ctx->fail(DK_E_ARG, "%zu patterns of %zu bytes with %zu positions each do not fit the workspace beside L, its index and the locate build",
                         npat, p.bytes(), max_hits);
    Upload up(ctx);
    hipStream_t st = ctx->stream;
    const uint8_t *d_pat = up.stage(pat, p.bytes(), "patterns");
    uint32_t *d_lo = ctx->ws_alloc<uint32_t>(npat), *d_hi = ctx->ws_alloc<uint32_t>(npat), *d_pos = ctx->ws_alloc<uint32_t>(nitems);
    if (!d_pat || !d_lo || !d_hi || !d_pos) return up.failed();
    FmView fm;
    DK_TRY(host_fm(up, lay, bwt, origin, step, WITH_LOCATE, fm));
    const ItemView pats = p.view(up, d_pat);
    if (!pats.d_off) return up.failed();
    DK_TRY(fm_count_device(ctx, fm, pats, d_lo, d_hi));
    DK_TRY(fm_locate_device(ctx, fm, d_lo, d_hi, nullptr, npat, max_hits, d_pos));
    DK_HIP(ctx, hipMemcpyAsync(lo, d_lo, npat * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DK_HIP(ctx, hipMemcpyAsync(hi, d_hi, npat * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DK_HIP(ctx, hipMemcpyAsync(pos, d_pos, nitems * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

int dk_dev_fm_extract(dk_ctx *ctx, const uint8_t *d_bwt, size_t n, const void *d_index, const void *d_ext, uint32_t step, const uint32_t *d_pos,
                      const uint32_t *d_len, size_t nrange, size_t max_len, uint8_t *d_out) {
    return dev_fm_extract(ctx, d_bwt, Layout(&n), d_index, d_ext, step, d_pos, d_len, nrange, nullptr, max_len, d_out);
}
int dk_dev_fm_extract_packed(dk_ctx *ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const void *d_index, const void *d_ext, uint32_t step,
                             const uint32_t *d_pos, const uint32_t *d_len, size_t nrange, const uint32_t *range_block, size_t max_len, uint8_t *d_out) {
    return dev_fm_extract(ctx, d_bwt, Layout(count, n), d_index, d_ext, step, d_pos, d_len, nrange, range_block, max_len, d_out);
}

int dk_fm_extract(dk_ctx *ctx, const uint8_t *bwt, size_t n, uint32_t origin, uint32_t step, const uint32_t *pos, const uint32_t *len, size_t nrange,
                  size_t max_len, uint8_t *out) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    if (!bwt) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_step(ctx, step));
    Layout lay(&n);
    DK_TRY(lay.check(ctx));
    DK_TRY(lay.check_origins(ctx, &origin));
    if (nrange == 0) return DK_OK;
    DK_TRY(fm_extract_rows(ctx, nrange, max_len));
    if (!pos || !out) return ctx->fail(DK_E_ARG, "null pointer");  // (len may be null)
    Timer t;
    // L, the index, the structure and the block's two offsets; the positions, the lengths and the rows; the larger of the two builds' workspaces
    // while it runs
    const size_t index_words = fm_index_words(n, 1), ext_words = fm_extract_words(n, 1, step), nbytes = nrange * max_len;
    const size_t need = ws_round(n) + ws_round(4 * index_words) + ws_round(4 * ext_words) + 256 + 2 * ws_round(4 * nrange) + ws_round(nbytes) +
                        std::max(fm_build_workspace(n, 1), fm_locate_build_workspace(n, 1) + ws_round(8));
    if (need > ctx->ws_size)
        return ctx->fail(DK_E_ARG, "%zu ranges of at most %zu bytes do not fit the workspace beside L, its index and the extract build", nrange, max_len);
    Upload up(ctx);
    uint8_t *d_out = ctx->ws_alloc<uint8_t>(nbytes);
    const uint32_t *d_pos = up.stage(pos, nrange, "positions");
    uint32_t *d_len = ctx->ws_alloc<uint32_t>(nrange);
    if (!d_out || !d_pos || !d_len) return up.failed();
    if (len) DK_TRY(up.copy(d_len, len, nrange * sizeof(uint32_t), "lengths"));
    FmView fm;
    DK_TRY(host_fm(up, lay, bwt, origin, step, WITH_EXTRACT, fm));
    DK_TRY(fm_extract_device(ctx, fm, d_pos, len ? d_len : nullptr, nullptr, nrange, max_len, d_out));
    DK_HIP(ctx, hipMemcpyAsync(out, d_out, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

// ---- find: every pattern in every block, as a compact list of hit records and the occurrence matrix ------------------
}  // extern "C"

namespace {
// what dk_dev_fm_find* and dk_dev_fm_near* check in front of the patterns themselves
int check_find_call(dk_ctx *ctx, const uint8_t *d_bwt, Layout &lay, const void *d_index, const void *d_loc, uint32_t step, size_t npat, const HitSink &out) {
    if (!d_bwt || lay.null() || !d_index || (out.max_hits && !d_loc)) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_index(ctx, d_index));
    DK_TRY(lay.check(ctx));
    if (!out.total_out) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_step(ctx, step));
    DK_TRY(check_records(ctx, npat, lay.count(), "%zu patterns in %zu blocks: more than DK_FM_FIND_MAX_PAIRS pairs", out.max_hits, out.d_hits, 16));
    if (out.max_hits) DK_TRY(check_aligned(ctx, addr(d_loc), 4, LOCATE_IS));
    return check_aligned(ctx, addr(out.d_occ), 4, "the occurrence matrix is");
}
int dev_fm_find(dk_ctx *ctx, const uint8_t *d_bwt, Layout &&lay, const void *d_index, const void *d_loc, uint32_t step, const uint8_t *d_pat, size_t npat,
                const size_t *pat_len, size_t max_hits, dk_fm_hit *d_hits, uint32_t *d_occ, uint64_t *total) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    const HitSink out{max_hits, d_hits, d_occ, total};
    DK_TRY(check_find_call(ctx, d_bwt, lay, d_index, d_loc, step, npat, out));
    const size_t count = lay.count();
    if (npat == 0) {
        *total = 0;
        return DK_OK;
    }
    Timer t;
    Patterns p;
    DK_TRY(check_patterns(ctx, npat, pat_len, nullptr, count, p));
    if (!d_pat && p.bytes()) return ctx->fail(DK_E_ARG, "null pointer");
    if (ws_round(4 * (count + 1)) + ws_round(4 * (npat + 1)) + fm_find_workspace(npat * count) > ctx->ws_size) {
        if (lay.packed()) return ctx->fail(DK_E_ARG, "%zu patterns in %zu blocks do not fit the workspace (16 bytes per pair)", npat, count);
        return ctx->fail(DK_E_ARG, "%zu patterns do not fit the workspace (16 bytes per pair)", npat);
    }
    Upload up(ctx);
    const FmView fm{lay.view(up, d_bwt), d_index, d_loc, nullptr, step};
    const ItemView pats = p.view(up, d_pat);
    if (!fm.L.d_off || !pats.d_off) return up.failed();
    DK_TRY(fm_find_device(ctx, fm, pats, out));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}
}  // namespace

extern "C" {

int dk_dev_fm_find(dk_ctx *ctx, const uint8_t *d_bwt, size_t n, const void *d_index, const void *d_loc, uint32_t step, const uint8_t *d_pat, size_t npat,
                   const size_t *pat_len, size_t max_hits, dk_fm_hit *d_hits, uint32_t *d_occ, uint64_t *total) {
    return dev_fm_find(ctx, d_bwt, Layout(&n), d_index, d_loc, step, d_pat, npat, pat_len, max_hits, d_hits, d_occ, total);
}
int dk_dev_fm_find_packed(dk_ctx *ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const void *d_index, const void *d_loc, uint32_t step,
                          const uint8_t *d_pat, size_t npat, const size_t *pat_len, size_t max_hits, dk_fm_hit *d_hits, uint32_t *d_occ, uint64_t *total) {
    return dev_fm_find(ctx, d_bwt, Layout(count, n), d_index, d_loc, step, d_pat, npat, pat_len, max_hits, d_hits, d_occ, total);
}

int dk_fm_find(dk_ctx *ctx, const uint8_t *bwt, size_t n, uint32_t origin, uint32_t step, const uint8_t *pat, size_t npat, const size_t *pat_len,
               size_t max_hits, dk_fm_hit *hits, uint32_t *occ, uint64_t *total) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    if (!bwt) return ctx->fail(DK_E_ARG, "null pointer");
    Layout lay(&n);
    DK_TRY(lay.check(ctx));
    DK_TRY(lay.check_origins(ctx, &origin));
    if (!total) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_step(ctx, step));
    DK_TRY(check_records(ctx, npat, 1, "%zu patterns: more than DK_FM_FIND_MAX_PAIRS pairs", max_hits, hits, 1));
    if (npat == 0) {
        *total = 0;
        return DK_OK;
    }
    Timer t;
    Patterns p;
    DK_TRY(check_patterns(ctx, npat, pat_len, nullptr, 1, p));
    if (!pat && p.bytes()) return ctx->fail(DK_E_ARG, "null pointer");
    // L, the index, the structure (only where records are asked for) and the block's two offsets; the patterns, their offsets and the occurrence
    // words; the larger of the builds' and the stage's workspaces.  The records come last, once their number is known.
    const size_t index_words = fm_index_words(n, 1), loc_words = max_hits ? fm_locate_words(n, 1, step) : 0;
    const size_t fixed = ws_round(n) + ws_round(4 * index_words) + ws_round(4 * loc_words) + 256 + ws_round(p.bytes()) + ws_round(4 * (npat + 1)) +
                         ws_round(4 * npat);
    const size_t need = fixed + std::max(fm_find_workspace(npat), std::max(fm_build_workspace(n, 1), max_hits ? fm_locate_build_workspace(n, 1) : 0));
    if (need > ctx->ws_size)
        return ctx->fail(DK_E_ARG, "%zu patterns of %zu bytes do not fit the workspace beside L, its index and the locate build", npat, p.bytes());
    Upload up(ctx);
    hipStream_t st = ctx->stream;
    const uint8_t *d_pat = up.stage(pat, p.bytes(), "patterns");
    uint32_t *d_occ = ctx->ws_alloc<uint32_t>(npat);
    const ItemView pats = p.view(up, d_pat);
    if (!d_pat || !d_occ || !pats.d_off) return up.failed();
    FmView fm;
    DK_TRY(host_fm(up, lay, bwt, origin, step, max_hits ? WITH_LOCATE : JUST_INDEX, fm));
    // the count and the scan alone first: how many records there are decides what the records take
    DK_TRY(fm_find_device(ctx, fm, pats, HitSink{0, nullptr, d_occ, total}));
    const size_t nhits = static_cast<size_t>(std::min<uint64_t>(*total, max_hits));
    if (nhits) {
        if (ctx->ws_used + ws_round(16 * nhits) + fm_find_workspace(npat) > ctx->ws_size)
            return ctx->fail(DK_E_ARG, "%zu hit records do not fit the workspace beside L, its index and the patterns", nhits);
        dk_fm_hit *d_hits = ctx->ws_alloc<dk_fm_hit>(nhits);
        if (!d_hits) return DK_E_NOMEM;
        DK_TRY(fm_find_device(ctx, fm, pats, HitSink{nhits, d_hits, nullptr, total}));
        DK_HIP(ctx, hipMemcpyAsync(hits, d_hits, nhits * sizeof(dk_fm_hit), hipMemcpyDeviceToHost, st));
    }
    if (occ) DK_HIP(ctx, hipMemcpyAsync(occ, d_occ, npat * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}

// ---- seams: the matches that straddle the borders of a pack, with the bytes carried over from the text in front ---------
}  // extern "C"

namespace {
int dev_fm_seams(dk_ctx *ctx, const uint8_t *d_bwt, Layout &&lay, const void *d_index, const void *d_ext, uint32_t step, const uint8_t *d_prev,
                 size_t prev_len, const uint8_t *d_pat, size_t npat, const size_t *pat_len, size_t max_hits, dk_fm_seam_hit *d_hits, uint32_t *d_occ,
                 uint64_t *total) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    if (!d_bwt || lay.null() || !d_index || !d_ext) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_index(ctx, d_index));
    DK_TRY(check_sampled(ctx, step, d_ext, EXTRACT_IS));
    DK_TRY(lay.check(ctx));
    Timer t;
    const size_t count = lay.count();
    if (!total) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_records(ctx, npat, count, "%zu patterns at %zu borders: more than DK_FM_FIND_MAX_PAIRS pairs", max_hits, d_hits, 16));
    DK_TRY(check_aligned(ctx, addr(d_occ), 4, "the occurrence matrix is"));
    if (prev_len >= DK_FM_SEAM_MAX_PATTERN) return ctx->fail(DK_E_ARG, "%zu carried bytes: fewer than DK_FM_SEAM_MAX_PATTERN can matter", prev_len);
    if (prev_len && !d_prev) return ctx->fail(DK_E_ARG, "null pointer");
    if (npat == 0) {
        *total = 0;
        ctx->stats.ms_total = t.ms();
        return DK_OK;
    }
    Patterns p;
    DK_TRY(check_patterns(ctx, npat, pat_len, nullptr, count, p));
    if (p.longest > DK_FM_SEAM_MAX_PATTERN) return ctx->fail(DK_E_ARG, "a pattern of %zu bytes: more than DK_FM_SEAM_MAX_PATTERN", p.longest);
    if (!d_pat && p.bytes()) return ctx->fail(DK_E_ARG, "null pointer");
    if (p.longest < 2) {  // no pattern can straddle a border
        *total = 0;
        if (d_occ) DK_HIP(ctx, hipMemsetAsync(d_occ, 0, npat * count * sizeof(uint32_t), ctx->stream));
        DK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->stats.ms_total = t.ms();
        return DK_OK;
    }
    const FmSeamPlan pl = fm_seam_plan(lay.off(), prev_len, p.longest - 1);
    if (pl.strip_len > 0xFFFFFFFFull) return ctx->fail(DK_E_ARG, "the edge strip of %zu bytes cannot be addressed", pl.strip_len);
    // the offsets and the anchor bases in one array of 2 count + 1 words, as dk_dev_fm_extract_packed lays them out
    if (ws_round(4 * (2 * count + 1)) + ws_round(4 * (npat + 1)) + fm_seams_workspace(pl, npat * count) > ctx->ws_size)
        return ctx->fail(DK_E_ARG, "%zu patterns at %zu borders do not fit the workspace (a strip of %zu bytes, 52 bytes per block, 16 per pair)", npat,
                         count, pl.strip_len);
    Upload up(ctx);
    FmView fm{PackView{d_bwt, nullptr, count, lay.total()}, d_index, nullptr, d_ext, step};
    lay.device_with_bases(up, fm);
    const ItemView pats = p.view(up, d_pat);
    if (!fm.L.d_off || !pats.d_off) return up.failed();
    up.covers_stage();  // (the stage uploads `pl`)
    DK_TRY(fm_seams_device(ctx, fm, d_prev, prev_len, pl, pats, HitSink{max_hits, d_hits, d_occ, total}));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}
}  // namespace

extern "C" {

int dk_dev_fm_seams(dk_ctx *ctx, const uint8_t *d_bwt, size_t n, const void *d_index, const void *d_ext, uint32_t step, const uint8_t *d_prev,
                    size_t prev_len, const uint8_t *d_pat, size_t npat, const size_t *pat_len, size_t max_hits, dk_fm_seam_hit *d_hits, uint32_t *d_occ,
                    uint64_t *total) {
    return dev_fm_seams(ctx, d_bwt, Layout(&n), d_index, d_ext, step, d_prev, prev_len, d_pat, npat, pat_len, max_hits, d_hits, d_occ, total);
}
int dk_dev_fm_seams_packed(dk_ctx *ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const void *d_index, const void *d_ext, uint32_t step,
                           const uint8_t *d_prev, size_t prev_len, const uint8_t *d_pat, size_t npat, const size_t *pat_len, size_t max_hits,
                           dk_fm_seam_hit *d_hits, uint32_t *d_occ, uint64_t *total) {
    return dev_fm_seams(ctx, d_bwt, Layout(count, n), d_index, d_ext, step, d_prev, prev_len, d_pat, npat, pat_len, max_hits, d_hits, d_occ, total);
}

// ---- near: byte classes and a budget of mismatches; find's checks, layout and guard ------------------------------------
}  // extern "C"

namespace {
int dev_fm_near(dk_ctx *ctx, const uint8_t *d_bwt, Layout &&lay, const void *d_index, const void *d_loc, uint32_t step, const uint8_t *d_cls, size_t npat,
                const size_t *pat_len, uint32_t k, uint32_t node_limit, size_t max_hits, dk_fm_near_hit *d_hits, uint32_t *d_occ, uint64_t *total,
                uint64_t *cut) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    const HitSink out{max_hits, d_hits, d_occ, total};
    DK_TRY(check_find_call(ctx, d_bwt, lay, d_index, d_loc, step, npat, out));
    const size_t count = lay.count();
    if (k > DK_FM_NEAR_MAX_K) return ctx->fail(DK_E_ARG, "a budget of %u mismatches: more than DK_FM_NEAR_MAX_K", k);
    if (npat == 0) {
        *total = 0;
        if (cut) *cut = 0;
        return DK_OK;
    }
    Timer t;
    Patterns p;
    DK_TRY(check_patterns(ctx, npat, pat_len, nullptr, count, p));
    if (p.longest > DK_FM_NEAR_MAX_PATTERN) return ctx->fail(DK_E_ARG, "a pattern of %zu positions: more than DK_FM_NEAR_MAX_PATTERN", p.longest);
    if (!d_cls && p.bytes()) return ctx->fail(DK_E_ARG, "null pointer");
    if (ws_round(4 * (count + 1)) + ws_round(4 * (npat + 1)) + fm_near_workspace(npat * count) > ctx->ws_size) {
        if (lay.packed()) return ctx->fail(DK_E_ARG, "%zu patterns in %zu blocks do not fit the workspace (16 bytes per pair)", npat, count);
        return ctx->fail(DK_E_ARG, "%zu patterns do not fit the workspace (16 bytes per pair)", npat);
    }
    Upload up(ctx);
    const FmView fm{lay.view(up, d_bwt), d_index, d_loc, nullptr, step};
    const ItemView cls = p.view(up, d_cls);
    if (!fm.L.d_off || !cls.d_off) return up.failed();
    DK_TRY(fm_near_device(ctx, fm, cls, k, node_limit, out, cut));
    DK_TRY(up.sync());
    ctx->stats.ms_total = t.ms();
    return DK_OK;
}
}  // namespace

extern "C" {

int dk_dev_fm_near(dk_ctx *ctx, const uint8_t *d_bwt, size_t n, const void *d_index, const void *d_loc, uint32_t step, const uint8_t *d_cls, size_t npat,
                   const size_t *pat_len, uint32_t k, uint32_t node_limit, size_t max_hits, dk_fm_near_hit *d_hits, uint32_t *d_occ, uint64_t *total,
                   uint64_t *cut) {
    return dev_fm_near(ctx, d_bwt, Layout(&n), d_index, d_loc, step, d_cls, npat, pat_len, k, node_limit, max_hits, d_hits, d_occ, total, cut);
}
int dk_dev_fm_near_packed(dk_ctx *ctx, const uint8_t *d_bwt, size_t count, const size_t *n, const void *d_index, const void *d_loc, uint32_t step,
                          const uint8_t *d_cls, size_t npat, const size_t *pat_len, uint32_t k, uint32_t node_limit, size_t max_hits,
                          dk_fm_near_hit *d_hits, uint32_t *d_occ, uint64_t *total, uint64_t *cut) {
    return dev_fm_near(ctx, d_bwt, Layout(count, n), d_index, d_loc, step, d_cls, npat, pat_len, k, node_limit, max_hits, d_hits, d_occ, total, cut);
}

int dk_dbg_dev_fm_rank(dk_ctx *ctx, const uint8_t *d_bwt, size_t total, const void *d_index, const uint32_t *d_pos, const uint8_t *d_sym, size_t nq,
                       uint32_t *d_out) {
    DK_TRY(begin_call(ctx));
    ScopedCall sc(ctx);
    if (!d_bwt || !d_index) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(check_index(ctx, d_index));
    DK_TRY(check_n(ctx, total));
    if (nq == 0) return DK_OK;
    if (!d_pos || !d_sym || !d_out || nq > 0xFFFFFFFEull) return ctx->fail(DK_E_ARG, "null pointer");
    DK_TRY(fm_rank_device(ctx, FmView{PackView{d_bwt, nullptr, 0, total}, d_index}, d_pos, d_sym, nq, d_out));
    DK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DK_OK;
}

}  // extern "C"
