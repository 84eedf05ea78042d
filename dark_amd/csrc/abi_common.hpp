// What the two files of the extern "C" boundary share (abi.cpp: contexts, codec, batches and the packed stages; abi_query.cpp: LCP, suffix-array
// check / search and the FM-index): the call bracket, the upload guard and the block layout.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "context.hpp"

namespace dk {

// abi.cpp.  forward_entry: the name of an entry point that needs the suffix sort's workspace (everything but the inverse path and the FM-index).
// A decoder context refuses it here, before anything is reset, allocated, launched or copied.
int begin_call(dk_ctx *ctx, const char *forward_entry = nullptr);
struct ScopedCall {
    dk_ctx *c;
    explicit ScopedCall(dk_ctx *ctx) : c(ctx) {}
    ~ScopedCall() { if (c->profiling) c->prof_collect(); }
};

inline int check_n(dk_ctx *ctx, size_t n) {
    if (n == 0) return ctx->fail(DK_E_ARG, "empty block (the reference panics at src/saca.rs:107)");
    if (n > ctx->max_n) return ctx->fail(DK_E_ARG, "block of %zu bytes exceeds the context capacity %zu", n, ctx->max_n);
    return DK_OK;
}

// The upload guard.  Every host-to-device copy whose source is host memory that is only good for the length of the call -- a Layout's offsets, a
// pattern batch's offsets, the caller's arrays, a seam plan -- is enqueued through copy() or stage().  The guard remembers that such a copy is
// on its way, and its destructor waits for the stream on every path that has not synchronised since: every early return of DK_TRY and DK_HIP
// included.  So no such copy outlives its source, whatever fails behind it.
// Where it stands: it owns nothing, so it is declared LAST among the host arrays of its scope (behind the Layout, the Patterns, the plan): it is
// then destroyed, and has waited, before they are.  A helper that takes the guard by reference uploads only what its caller declared in front.
// The views of context.hpp (PackView, FmView, ItemView) are filled through the guard, so they too are declared behind it.
struct Upload {
    dk_ctx *c;
    bool pending = false;
    int rc = DK_OK;  // the first copy or fill that could not be enqueued
    explicit Upload(dk_ctx *ctx) : c(ctx) {}
    Upload(const Upload &) = delete;
    Upload &operator=(const Upload &) = delete;
    ~Upload() { if (pending) (void)hipStreamSynchronize(c->stream); }
    int copy(void *d_dst, const void *src, size_t bytes, const char *what) {
        pending = true;
        return note(c->hip_ok(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, c->stream), what));
    }
    int fill(uint32_t *d_word, uint32_t value) {  // (no host memory behind it: nothing to wait for)
        return note(c->hip_ok(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_word), static_cast<int>(value), 1, c->stream), "fill"));
    }
    // one allocation of the workspace with src[0, count) on its way into it (an empty source still gets an address: one element); null: failed()
    template <class T> T *stage(const T *src, size_t count, const char *what) {
        T *d = c->ws_alloc<T>(std::max<size_t>(count, 1));
        return d && (count == 0 || copy(d, src, count * sizeof(T), what) == DK_OK) ? d : nullptr;
    }
    int failed() const { return rc != DK_OK ? rc : DK_E_NOMEM; }  // what a null pointer from stage(), Layout::device() or ws_alloc stands for
    int note(int r) { if (rc == DK_OK) rc = r; return r; }
    void covers_stage() { pending = true; }  // in front of a device stage that enqueues such a copy itself (fm_seams_device: the plan)
    void synchronised() { pending = false; }  // behind a device stage that has handed results to the host: the stream is drained
    int sync() {
        pending = false;
        return c->hip_ok(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    }
};

// The blocks of a call: one block of n bytes, or a pack of `count` blocks back to back.  The device stages take (d_off, count, total) and know
// no difference -- a single block is a pack of one; the limits differ on purpose: a single block may fill the context (max_n), a packed one is
// bounded by DK_PACKED_MAX_BLOCK_BYTES and the pack by the context's max_blocks.  An entry names its blocks when it constructs the layout and
// checks them where its order of checks has that check (check()); everything else is valid only behind a check() that returned DK_OK.
class Layout {
    const size_t count_, *const n_;
    const bool packed_;
    std::vector<uint32_t> off_, geo_;  // block i at [off_[i], off_[i + 1]); geo_: what device_with_bases uploads

public:
    explicit Layout(const size_t *n) : count_(1), n_(n), packed_(false) {}             // the entry's own n: a single block
    Layout(size_t count, const size_t *n) : count_(count), n_(n), packed_(true) {}     // the caller's sizes: a pack
    bool packed() const { return packed_; }
    bool null() const { return !n_; }
    int check(dk_ctx *ctx) {
        if (!packed_) {
            DK_TRY(check_n(ctx, *n_));
            off_ = {0u, static_cast<uint32_t>(*n_)};
            return DK_OK;
        }
        if (!n_) return ctx->fail(DK_E_ARG, "null pointer");
        if (count_ == 0 || count_ > ctx->max_blocks) return ctx->fail(DK_E_ARG, "a pack holds 1 .. %zu blocks, not %zu", ctx->max_blocks, count_);
        off_.assign(count_ + 1, 0);
        size_t total = 0;
        for (size_t i = 0; i < count_; ++i) {
            if (n_[i] == 0) return ctx->fail(DK_E_ARG, "empty block %zu in the pack (the reference panics at src/saca.rs:107)", i);
            if (n_[i] > DK_PACKED_MAX_BLOCK_BYTES) return ctx->fail(DK_E_ARG, "block %zu of %zu bytes exceeds DK_PACKED_MAX_BLOCK_BYTES", i, n_[i]);
            total += n_[i];
            if (total > ctx->max_n) return ctx->fail(DK_E_ARG, "the pack exceeds the context capacity %zu", ctx->max_n);
            off_[i + 1] = static_cast<uint32_t>(total);
        }
        return DK_OK;
    }
    size_t count() const { return count_; }
    size_t total() const { return off_.back(); }
    const std::vector<uint32_t> &off() const { return off_; }

    // origin: one per block, each inside its block
    int check_origins(dk_ctx *ctx, const uint32_t *origin) const {
        for (size_t i = 0; i < count_; ++i) {
            if (origin[i] < n_[i]) continue;
            if (packed_) return ctx->fail(DK_E_ARG, "origin %u of block %zu is outside its %zu bytes", origin[i], i, n_[i]);
            return ctx->fail(DK_E_ARG, "origin %u is outside the block of %zu bytes", origin[i], n_[i]);
        }
        return DK_OK;
    }
    // d_off: the count + 1 offsets in the workspace (one allocation).  A single block's two words are written by two fills, so no host memory
    // stands behind a copy; a pack's are copied from this layout, which therefore stands in front of the guard.  Null: up.failed().
    uint32_t *device(Upload &up) const {
        if (packed_) return up.stage(off_.data(), off_.size(), "block offsets");
        uint32_t *d = up.c->ws_alloc<uint32_t>(2);
        return d && up.fill(d, 0) == DK_OK && up.fill(d + 1, off_[1]) == DK_OK ? d : nullptr;
    }
    // the pack of `bytes` (text or L) as the query stages take it: device() beside the sizes.  view.d_off null: up.failed()
    PackView view(Upload &up, const uint8_t *bytes) const { return PackView{bytes, device(up), count_, total()}; }
    // the same for the stages that read fm.ext: the offsets and the anchor bases of the extract structure (fm_extract_bases, at fm.step) in one
    // array of 2 count + 1 words, fm.L.d_off = its first count + 1, fm.d_abase = the rest.  fm.L.d_off null: up.failed()
    void device_with_bases(Upload &up, FmView &fm) {
        geo_ = off_;
        const std::vector<uint32_t> abase = fm_extract_bases(off_, fm.step);
        geo_.insert(geo_.end(), abase.begin(), abase.end() - 1);
        fm.L.d_off = up.stage(geo_.data(), geo_.size(), "block offsets and anchor bases");
        fm.d_abase = fm.L.d_off ? fm.L.d_off + count_ + 1 : nullptr;
    }
};

// L of every block into d_bwt and the origins into d_origin, or the suffix arrays (abi.cpp; dk_dev_suffix_array_packed_lcp takes Phi from it)
int packed_forward(dk_ctx *ctx, const uint8_t *d_in, const std::vector<uint32_t> &off, const uint32_t *d_off, uint8_t *d_bwt, uint32_t *d_origin,
                   std::vector<std::pair<size_t, uint32_t>> *fixed, uint32_t *d_sa = nullptr, uint32_t *d_phi = nullptr);

}  // namespace dk
