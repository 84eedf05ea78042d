// dark.hpp -- C++ mirror of the reference's Rust interface for the hot path, a thin layer over the C ABI (dark_amd.h).
// The reference is compiled code (Rust); its toolchain is not in this image, so the host side a Rust caller would write is
// given here in C++ with the same names, argument meaning and error behaviour:
//   dark::saca::Constructor            src/saca.rs:344-384   new(max_n) / capacity() / compute(input); check / search are this library's
//   dark::fm::Index                    this library's: count patterns in (L, origin) -- from_text / Index(bwt, origin) / count / occurrences
//   dark::block::dc::Encoder<Model>    src/block/dc.rs:21-92  new(n, model) / encode(input, writer) -> (writer, result)
//   dark::block::dc::Decoder<Model>    src/block/dc.rs:96-161 new(n, model) / decode(reader, writer) -> (reader, writer, result)
//   dark::block::raw::Encoder<Model> / Decoder<Model>   src/block/raw.rs:17-105 (Model = model::bbb::Model or model::raw::Out)
//   dark::model::{dark,exp,ybs,simple,bbb}::Model, dark::model::raw::Out   src/model/*.rs  (the state lives in the library; the type selects it)
// Where the Rust code panics (assert!/unwrap) this throws dark::Error; io::Result becomes dark::Result{ok, message}.
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "dark_amd.h"

namespace dark {

struct Error : std::runtime_error { int code; Error(int c, const std::string &m) : std::runtime_error(m), code(c) {} };
struct Result { bool ok = true; std::string message; explicit operator bool() const { return ok; } void unwrap() const { if (!ok) throw Error(DK_E_STREAM, message); } };

namespace detail {
class Ctx {
public:
    // purpose DK_CTX_DECODER: the inverse path's workspace only (dk_ctx_create_decoder, one block per call)
    Ctx(size_t max_n, int device, int purpose = DK_CTX_FULL) {
        int rc = purpose == DK_CTX_DECODER ? dk_ctx_create_decoder(device, max_n, 1, &h_) : dk_ctx_create(device, max_n, &h_);
        if (rc != DK_OK) throw Error(rc, "dk_ctx_create failed (no GPU, or out of memory)");
    }
    ~Ctx() { dk_ctx_destroy(h_); }
    Ctx(const Ctx &) = delete;
    Ctx &operator=(const Ctx &) = delete;
    dk_ctx *get() const { return h_; }
    int purpose() const { return dk_ctx_purpose(h_); }
    std::string error() const { return dk_last_error(h_); }
private:
    dk_ctx *h_ = nullptr;
};
}  // namespace detail

namespace model {
namespace dark { struct Model { static constexpr int ID = DK_MODEL_DARK; void reset() {} }; }
namespace exp { struct Model { static constexpr int ID = DK_MODEL_EXP; void reset() {} }; }
namespace ybs { struct Model { static constexpr int ID = DK_MODEL_YBS; void reset() {} }; }
namespace simple { struct Model { static constexpr int ID = DK_MODEL_SIMPLE; void reset() {} }; }
namespace bbb { struct Model { static constexpr int RAW_ID = DK_RAWMODEL_BBB; void reset() {} }; }   // src/model/bbb.rs
namespace raw { struct Out { static constexpr int RAW_ID = DK_RAWMODEL_OUT; std::vector<uint8_t> dumped; void reset() {} }; }  // src/model/raw.rs:46-76: "out.raw"
}  // namespace model

namespace saca {
using Symbol = uint8_t;   // src/saca.rs:18
using Suffix = uint32_t;  // src/saca.rs:20
class Constructor {
public:
    explicit Constructor(size_t max_n, int device = 0) : ctx_(max_n, device), suffixes_(max_n), n_(max_n) {}  // Constructor::new
    size_t capacity() const { return dk_capacity(ctx_.get()); }
    // Constructor::compute: asserts input.len() == n (src/saca.rs:369)
    const std::vector<Suffix> &compute(const std::vector<Symbol> &input) {
        if (input.size() != n_) throw Error(DK_E_ARG, "assertion failed: input.len() == self.n");
        int rc = dk_suffix_array(ctx_.get(), input.data(), input.size(), suffixes_.data());
        if (rc != DK_OK) throw Error(rc, ctx_.error());
        return suffixes_;
    }
    // compute for many small inputs at once (dk_suffix_array_packed): the suffix array of inputs[i], entries local to it, at result[i].
    // The inputs together must fit the capacity; each alone need not have the constructor's exact size.
    std::vector<std::vector<Suffix>> compute_packed(const std::vector<std::vector<Symbol>> &inputs) {
        std::vector<size_t> sizes;
        std::vector<Symbol> text;
        for (const auto &in : inputs) {
            sizes.push_back(in.size());
            text.insert(text.end(), in.begin(), in.end());
        }
        if (text.size() > capacity()) throw Error(DK_E_ARG, "assertion failed: total input length <= self.capacity()");
        std::vector<Suffix> all(text.size());
        int rc = dk_suffix_array_packed(ctx_.get(), text.data(), sizes.size(), sizes.data(), all.data());
        if (rc != DK_OK) throw Error(rc, ctx_.error());
        std::vector<std::vector<Suffix>> out;
        size_t at = 0;
        for (size_t n : sizes) {
            out.emplace_back(all.begin() + static_cast<std::ptrdiff_t>(at), all.begin() + static_cast<std::ptrdiff_t>(at + n));
            at += n;
        }
        return out;
    }
    // compute, and the LCP array with it (dk_suffix_array_lcp): lcp[0] = 0, lcp[i] = leading symbols the suffixes sa[i-1] and sa[i] share.
    // Nothing in the reference corresponds; the suffix array is the one compute returns.
    std::pair<const std::vector<Suffix> &, const std::vector<uint32_t> &> compute_lcp(const std::vector<Symbol> &input) {
        if (input.size() != n_) throw Error(DK_E_ARG, "assertion failed: input.len() == self.n");
        lcp_.resize(n_);
        int rc = dk_suffix_array_lcp(ctx_.get(), input.data(), input.size(), suffixes_.data(), lcp_.data());
        if (rc != DK_OK) throw Error(rc, ctx_.error());
        return {suffixes_, lcp_};
    }
    // compute_packed with every input's LCP array (dk_suffix_array_packed_lcp): result[i] = (suffix array, LCP array) of inputs[i]
    std::vector<std::pair<std::vector<Suffix>, std::vector<uint32_t>>> compute_packed_lcp(const std::vector<std::vector<Symbol>> &inputs) {
        std::vector<size_t> sizes;
        std::vector<Symbol> text;
        for (const auto &in : inputs) {
            sizes.push_back(in.size());
            text.insert(text.end(), in.begin(), in.end());
        }
        if (text.size() > capacity()) throw Error(DK_E_ARG, "assertion failed: total input length <= self.capacity()");
        std::vector<Suffix> all(text.size());
        std::vector<uint32_t> lcp(text.size());
        int rc = dk_suffix_array_packed_lcp(ctx_.get(), text.data(), sizes.size(), sizes.data(), all.data(), lcp.data());
        if (rc != DK_OK) throw Error(rc, ctx_.error());
        std::vector<std::pair<std::vector<Suffix>, std::vector<uint32_t>>> out;
        size_t at = 0;
        for (size_t n : sizes) {
            const auto lo = static_cast<std::ptrdiff_t>(at), hi = static_cast<std::ptrdiff_t>(at + n);
            out.emplace_back(std::vector<Suffix>(all.begin() + lo, all.begin() + hi), std::vector<uint32_t>(lcp.begin() + lo, lcp.begin() + hi));
            at += n;
        }
        return out;
    }
    // Is `suffixes` what compute(input) returns (dk_sa_check)?  {DK_SA_OK, n}, or the first kind of fault and the lowest slot (DK_SA_NOT_PERMUTATION:
    // text position) that shows it.  Nothing in the reference corresponds; "no" is an answer, not an Error.
    std::pair<uint32_t, uint32_t> check(const std::vector<Symbol> &input, const std::vector<Suffix> &suffixes) {
        if (input.size() != n_ || suffixes.size() != n_) throw Error(DK_E_ARG, "assertion failed: input.len() == self.n");
        uint32_t verdict = 0, where = 0;
        int rc = dk_sa_check(ctx_.get(), input.data(), input.size(), suffixes.data(), &verdict, &where);
        if (rc != DK_OK) throw Error(rc, ctx_.error());
        return {verdict, where};
    }
    // result[q] = (lo, hi): suffixes[lo .. hi) are exactly the places patterns[q] occurs in input; lo == hi = the insertion slot of a pattern
    // that does not occur (dk_sa_search).  `suffixes` is trusted: check() verifies one.
    std::vector<std::pair<uint32_t, uint32_t>> search(const std::vector<Symbol> &input, const std::vector<Suffix> &suffixes,
                                                      const std::vector<std::vector<Symbol>> &patterns) {
        if (input.size() != n_ || suffixes.size() != n_) throw Error(DK_E_ARG, "assertion failed: input.len() == self.n");
        std::vector<size_t> lens;
        std::vector<Symbol> bytes(1);  // (one byte so that data() is never null)
        for (const auto &p : patterns) {
            lens.push_back(p.size());
            bytes.insert(bytes.end(), p.begin(), p.end());
        }
        std::vector<uint32_t> lo(patterns.size() + 1), hi(patterns.size() + 1);
        int rc = dk_sa_search(ctx_.get(), input.data(), input.size(), suffixes.data(), bytes.data() + 1, patterns.size(), lens.data(), lo.data(), hi.data());
        if (rc != DK_OK) throw Error(rc, ctx_.error());
        std::vector<std::pair<uint32_t, uint32_t>> out;
        for (size_t q = 0; q < patterns.size(); ++q) out.emplace_back(lo[q], hi[q]);
        return out;
    }
    // The matching statistics of the queries against input (dk_sa_match), over the positions of the queries back to back: len[g] = the longest
    // prefix of the window at g (at most max_len symbols, inside its query) that occurs in input, suffixes[lo[g] .. hi[g]) = where it does.
    struct Matches { std::vector<uint32_t> len, lo, hi; };
    Matches match(const std::vector<Symbol> &input, const std::vector<Suffix> &suffixes, const std::vector<std::vector<Symbol>> &queries, size_t max_len) {
        if (input.size() != n_ || suffixes.size() != n_) throw Error(DK_E_ARG, "assertion failed: input.len() == self.n");
        std::vector<size_t> lens;
        std::vector<Symbol> bytes(1);  // (one byte so that data() is never null)
        for (const auto &q : queries) {
            lens.push_back(q.size());
            bytes.insert(bytes.end(), q.begin(), q.end());
        }
        const size_t total = bytes.size() - 1;
        Matches m{std::vector<uint32_t>(total + 1), std::vector<uint32_t>(total + 1), std::vector<uint32_t>(total + 1)};
        int rc = dk_sa_match(ctx_.get(), input.data(), input.size(), suffixes.data(), bytes.data() + 1, queries.size(), lens.data(), max_len, m.len.data(),
                             m.lo.data(), m.hi.data());
        if (rc != DK_OK) throw Error(rc, ctx_.error());
        m.len.resize(total);
        m.lo.resize(total);
        m.hi.resize(total);
        return m;
    }
    // The super-maximal exact matches of at least min_len symbols (dk_sa_smems): hits = the first min(total, max_hits) records {at, len, lo, hi}
    // in rising order of at, the offset into the queries back to back.  A copy longer than max_len is reported once, with len = max_len.
    struct Smems { std::vector<dk_sa_smem> hits; uint64_t total = 0; };
    Smems smems(const std::vector<Symbol> &input, const std::vector<Suffix> &suffixes, const std::vector<std::vector<Symbol>> &queries, size_t min_len,
                size_t max_len, size_t max_hits = 65536) {
        if (input.size() != n_ || suffixes.size() != n_) throw Error(DK_E_ARG, "assertion failed: input.len() == self.n");
        std::vector<size_t> lens;
        std::vector<Symbol> bytes(1);
        for (const auto &q : queries) {
            lens.push_back(q.size());
            bytes.insert(bytes.end(), q.begin(), q.end());
        }
        Smems s;
        s.hits.resize(std::min(max_hits, bytes.size() - 1) + 1);  // (never more records than positions)
        int rc = dk_sa_smems(ctx_.get(), input.data(), input.size(), suffixes.data(), bytes.data() + 1, queries.size(), lens.data(), min_len, max_len,
                             max_hits, s.hits.data(), &s.total);
        if (rc != DK_OK) throw Error(rc, ctx_.error());
        s.hits.resize(static_cast<size_t>(std::min<uint64_t>(s.total, max_hits)));
        return s;
    }
    detail::Ctx &context() { return ctx_; }  // plays reuse(): later stages share the device workspace through it
private:
    detail::Ctx ctx_;
    std::vector<Suffix> suffixes_;
    std::vector<uint32_t> lcp_;
    size_t n_;
};
}  // namespace saca

namespace block {
namespace dc {
template <class M>
class Encoder {
public:
    M model;  // public like the reference's field (src/block/dc.rs:25)
    // any_byte (extension, DK_MODEL_ANYBYTE): the stream starts with four more bytes, the first position of byte 0xFF in the BWT, so that
    // blocks with that byte decode; a Decoder must be given the same option.  The model must be one of the four coding models.
    Encoder(size_t n, M m, int device = 0, bool any_byte = false) : model(m), ctx_(n, device), id_(M::ID | (any_byte ? DK_MODEL_ANYBYTE : 0)) { model.reset(); }
    // encode(&input, writer) -> (writer, io::Result<()>); the writer here is any byte container with insert()
    template <class W>
    std::pair<W, Result> encode(const std::vector<uint8_t> &input, W writer) {
        if (input.size() > dk_capacity(ctx_.get())) throw Error(DK_E_ARG, "assertion failed: block_size <= self.sac.capacity()");
        std::vector<uint8_t> out(2 * input.size() + 4096 + 4);
        size_t len = 0;
        int rc = dk_block_encode(ctx_.get(), id_, input.data(), input.size(), out.data(), out.size(), &len);
        if (rc != DK_OK) return {std::move(writer), Result{false, ctx_.error()}};
        writer.insert(writer.end(), out.begin(), out.begin() + static_cast<std::ptrdiff_t>(len));
        return {std::move(writer), Result{}};
    }
private:
    detail::Ctx ctx_;
    int id_;
};

template <class M>
class Decoder {
public:
    M model;
    Decoder(size_t n, M m, int device = 0, bool any_byte = false) : model(m), ctx_(n, device, DK_CTX_DECODER), n_(n), id_(M::ID | (any_byte ? DK_MODEL_ANYBYTE : 0)) { model.reset(); }
    // decode(reader, writer) -> (reader, writer, io::Result<()>)
    template <class W>
    std::tuple<std::vector<uint8_t>, W, Result> decode(std::vector<uint8_t> reader, W writer) {
        std::vector<uint8_t> out(n_);
        int rc = dk_block_decode(ctx_.get(), id_, reader.data(), reader.size(), n_, out.data());
        if (rc != DK_OK) return {std::move(reader), std::move(writer), Result{false, ctx_.error()}};
        writer.insert(writer.end(), out.begin(), out.end());
        return {std::move(reader), std::move(writer), Result{}};
    }
    detail::Ctx &context() { return ctx_; }  // Decoder::new makes a decoder context: context().purpose() == DK_CTX_DECODER
private:
    detail::Ctx ctx_;
    size_t n_;
    int id_;
};
}  // namespace dc

namespace raw {  // src/block/raw.rs
template <class M>
class Encoder {
public:
    M model;
    Encoder(size_t n, M m, int device = 0) : model(m), ctx_(n, device) { model.reset(); }
    template <class W>
    std::pair<W, Result> encode(const std::vector<uint8_t> &input, W writer) {
        if (input.size() > dk_capacity(ctx_.get())) throw Error(DK_E_ARG, "assertion failed: block_size <= self.sac.capacity()");
        std::vector<uint8_t> out(2 * input.size() + 4096), dump(input.size() + 4);
        size_t len = 0, dumped = 0;
        int rc = dk_raw_block_encode(ctx_.get(), M::RAW_ID, input.data(), input.size(), out.data(), out.size(), &len, dump.data(), dump.size(), &dumped);
        if (rc != DK_OK) return {std::move(writer), Result{false, ctx_.error()}};
        keep_dump(model, dump, dumped);
        writer.insert(writer.end(), out.begin(), out.begin() + static_cast<std::ptrdiff_t>(len));
        return {std::move(writer), Result{}};
    }
private:
    static void keep_dump(model::raw::Out &m, const std::vector<uint8_t> &d, size_t k) { m.dumped.assign(d.begin(), d.begin() + static_cast<std::ptrdiff_t>(k)); }
    template <class Other> static void keep_dump(Other &, const std::vector<uint8_t> &, size_t) {}
    detail::Ctx ctx_;
};
template <class M>
class Decoder {
public:
    M model;
    Decoder(size_t n, M m, int device = 0) : model(m), ctx_(n, device, DK_CTX_DECODER), n_(n) { model.reset(); }
    template <class W>
    std::tuple<std::vector<uint8_t>, W, Result> decode(std::vector<uint8_t> reader, W writer) {
        std::vector<uint8_t> out(n_);
        int rc = dk_raw_block_decode(ctx_.get(), M::RAW_ID, reader.data(), reader.size(), n_, out.data());
        if (rc != DK_OK) return {std::move(reader), std::move(writer), Result{false, ctx_.error()}};
        writer.insert(writer.end(), out.begin(), out.end());
        return {std::move(reader), std::move(writer), Result{}};
    }
    detail::Ctx &context() { return ctx_; }  // Decoder::new makes a decoder context: context().purpose() == DK_CTX_DECODER
private:
    detail::Ctx ctx_;
    size_t n_;
};
}  // namespace raw
}  // namespace block

namespace bwt {  // the pieces of crate `compress` the reference's tests call next to saca (src/saca.rs:398-405)
inline std::pair<std::vector<uint8_t>, size_t> transform(detail::Ctx &ctx, const std::vector<uint8_t> &input) {
    std::vector<uint8_t> out(input.size());
    uint32_t origin = 0;
    int rc = dk_bwt_forward(ctx.get(), input.data(), input.size(), out.data(), &origin);
    if (rc != DK_OK) throw Error(rc, ctx.error());
    return {out, origin};
}
inline std::vector<uint8_t> decode(detail::Ctx &ctx, const std::vector<uint8_t> &bwt, size_t origin) {
    std::vector<uint8_t> out(bwt.size());
    int rc = dk_bwt_inverse(ctx.get(), bwt.data(), bwt.size(), static_cast<uint32_t>(origin), out.data());
    if (rc != DK_OK) throw Error(rc, ctx.error());
    return out;
}
}  // namespace bwt

namespace fm {
// Counting patterns in a BWT without the text and without a suffix array (dk_fm_count): the index of (L, origin) as
// bwt::transform or a stream decoder leaves them.  It lives on a DECODER context: nothing here needs the suffix sort's workspace.  Nothing in the
// reference corresponds.  (This host-memory form builds the device index anew in every count; a caller that keeps L on the GPU uses
// dk_dev_fm_build once and dk_dev_fm_count after it.)
// locate_step (0: none, count only; else a power of two in [1, 4096]): the distance of the sampled text positions of `locate` (dk_fm_locate,
// section 4.14), which says WHERE the patterns occur -- still without the text and without a full suffix array.
// extract_step (0: none; else a power of two in [1, 4096]): the distance of the anchored text positions of `extract` (dk_fm_extract, section
// 4.15), which says WHAT the text is at given positions -- so L and the structures stand in for the text in every query.
class Index {
public:
    Index(std::vector<uint8_t> bwt, size_t origin, int device = 0, uint32_t locate_step = 0, uint32_t extract_step = 0)
        : ctx_(bwt.size(), device, DK_CTX_DECODER), bwt_(std::move(bwt)), origin_(origin), step_(locate_step), ext_step_(extract_step), device_(device) {
        if (origin_ >= bwt_.size()) throw Error(DK_E_ARG, "assertion failed: origin < bwt.len()");
        if (step_ && dk_fm_locate_bytes(bwt_.size(), 1, step_) == 0) throw Error(DK_E_ARG, "locate_step is no power of two in [1, 4096]");
        if (ext_step_ && dk_fm_extract_bytes(bwt_.size(), 1, ext_step_) == 0) throw Error(DK_E_ARG, "extract_step is no power of two in [1, 4096]");
    }
    // the index of a text: forward BWT on a full context that is released again, then as above
    static Index from_text(const std::vector<uint8_t> &text, int device = 0, uint32_t locate_step = 0, uint32_t extract_step = 0) {
        detail::Ctx full(text.size(), device);
        auto lo = bwt::transform(full, text);
        return Index(std::move(lo.first), lo.second, device, locate_step, extract_step);
    }
    size_t len() const { return bwt_.size(); }
    // device bytes that answer a query: L and the index, and the locate and extract structures where they were asked for
    size_t resident_bytes() const {
        return bwt_.size() + dk_fm_index_bytes(bwt_.size(), 1) + (step_ ? dk_fm_locate_bytes(bwt_.size(), 1, step_) : 0) +
               (ext_step_ ? dk_fm_extract_bytes(bwt_.size(), 1, ext_step_) : 0);
    }
    // result[q] = (lo, hi) as from saca::Constructor::search on the text; hi - lo = the number of places patterns[q] occurs
    std::vector<std::pair<uint32_t, uint32_t>> count(const std::vector<std::vector<uint8_t>> &patterns) {
        std::vector<size_t> lens;
        std::vector<uint8_t> bytes(1);  // (one byte so that data() is never null)
        for (const auto &p : patterns) {
            lens.push_back(p.size());
            bytes.insert(bytes.end(), p.begin(), p.end());
        }
        std::vector<uint32_t> lo(patterns.size() + 1), hi(patterns.size() + 1);
        int rc = dk_fm_count(ctx_.get(), bwt_.data(), bwt_.size(), static_cast<uint32_t>(origin_), bytes.data() + 1, patterns.size(), lens.data(), lo.data(), hi.data());
        if (rc != DK_OK) throw Error(rc, ctx_.error());
        std::vector<std::pair<uint32_t, uint32_t>> out;
        for (size_t q = 0; q < patterns.size(); ++q) out.emplace_back(lo[q], hi[q]);
        return out;
    }
    std::vector<uint32_t> occurrences(const std::vector<std::vector<uint8_t>> &patterns) {
        std::vector<uint32_t> out;
        for (const auto &r : count(patterns)) out.push_back(r.second - r.first);
        return out;
    }
    // result[q] = the first min(occurrences, max_hits) text positions of patterns[q], in suffix-array order
    std::vector<std::vector<uint32_t>> locate(const std::vector<std::vector<uint8_t>> &patterns, size_t max_hits = 16) {
        if (!step_) throw Error(DK_E_ARG, "the index was made without a locate structure (locate_step = 0)");
        std::vector<size_t> lens;
        std::vector<uint8_t> bytes(1);
        for (const auto &p : patterns) {
            lens.push_back(p.size());
            bytes.insert(bytes.end(), p.begin(), p.end());
        }
        std::vector<uint32_t> lo(patterns.size() + 1), hi(patterns.size() + 1), pos(patterns.size() * max_hits + 1);
        int rc = dk_fm_locate(ctx_.get(), bwt_.data(), bwt_.size(), static_cast<uint32_t>(origin_), step_, bytes.data() + 1, patterns.size(), lens.data(),
                              max_hits, lo.data(), hi.data(), pos.data());
        if (rc != DK_OK) throw Error(rc, ctx_.error());
        std::vector<std::vector<uint32_t>> out(patterns.size());
        for (size_t q = 0; q < patterns.size(); ++q)
            for (size_t j = 0; j < max_hits && pos[q * max_hits + j] != DK_FM_NO_HIT; ++j) out[q].push_back(pos[q * max_hits + j]);
        return out;
    }
    // result[q] = the text at [positions[q], positions[q] + length), cut at the text's end (empty from there on)
    std::vector<std::vector<uint8_t>> extract(const std::vector<uint32_t> &positions, size_t length) {
        if (!ext_step_) throw Error(DK_E_ARG, "the index was made without an extract structure (extract_step = 0)");
        std::vector<uint8_t> rows(positions.size() * length + 1);
        std::vector<uint32_t> pos(positions);
        pos.push_back(0);
        int rc = dk_fm_extract(ctx_.get(), bwt_.data(), bwt_.size(), static_cast<uint32_t>(origin_), ext_step_, pos.data(), nullptr, positions.size(),
                               length, rows.data());
        if (rc != DK_OK) throw Error(rc, ctx_.error());
        std::vector<std::vector<uint8_t>> out(positions.size());
        for (size_t q = 0; q < positions.size(); ++q) {
            const size_t got = positions[q] < bwt_.size() ? std::min<size_t>(length, bwt_.size() - positions[q]) : 0;
            out[q].assign(rows.begin() + static_cast<std::ptrdiff_t>(q * length), rows.begin() + static_cast<std::ptrdiff_t>(q * length + got));
        }
        return out;
    }
    // Every pattern at once as one list (dk_fm_find, section 4.16): occ[q] = the occurrences of patterns[q], total their sum, hits the first
    // min(total, max_hits) records {pattern, block = 0, position, slot} in the order (pattern, suffix-array slot).  max_hits = 0 needs no
    // locate structure.  The default of 65536 records is a choice, not a measurement.
    struct Found { std::vector<uint32_t> occ; std::vector<dk_fm_hit> hits; uint64_t total = 0; };
    Found find(const std::vector<std::vector<uint8_t>> &patterns, size_t max_hits = 65536) {
        if (max_hits && !step_) throw Error(DK_E_ARG, "the index was made without a locate structure (locate_step = 0)");
        std::vector<size_t> lens;
        std::vector<uint8_t> bytes(1);
        for (const auto &p : patterns) {
            lens.push_back(p.size());
            bytes.insert(bytes.end(), p.begin(), p.end());
        }
        Found out;
        out.occ.resize(patterns.size() + 1);
        out.hits.resize(max_hits + 1);
        int rc = dk_fm_find(ctx_.get(), bwt_.data(), bwt_.size(), static_cast<uint32_t>(origin_), step_ ? step_ : 32u, bytes.data() + 1, patterns.size(),
                            lens.data(), max_hits, out.hits.data(), out.occ.data(), &out.total);
        if (rc != DK_OK) throw Error(rc, ctx_.error());
        out.occ.resize(patterns.size());
        out.hits.resize(static_cast<size_t>(std::min<uint64_t>(out.total, max_hits)));
        return out;
    }
#ifdef DARK_WITH_HIP
    // The matches of `patterns` in prev + text that start in prev and end in the text (dk_dev_fm_seams, section 4.17) -- for a single block the
    // only border there is; with find() they are every occurrence in prev + text that does not lie inside prev.  occ[q] = their number, total
    // the sum, hits the first min(total, max_hits) records {pattern, block = 0, back, 0} in the order (pattern, back descending), back = the
    // match's bytes in front of the text.  Needs an extract structure (extract_step).  The entry has no host-memory form, so this one holds
    // L, the index and the structure in device memory of its own for the call: it is compiled only where DARK_WITH_HIP is defined in front of
    // this header (the HIP runtime's headers on the include path, amdhip64 on the link line).
    struct Seams { std::vector<uint32_t> occ; std::vector<dk_fm_seam_hit> hits; uint64_t total = 0; };
    Seams seams(const std::vector<std::vector<uint8_t>> &patterns, const std::vector<uint8_t> &prev = {}, size_t max_hits = 65536) {
        if (!ext_step_) throw Error(DK_E_ARG, "the index was made without an extract structure (extract_step = 0)");
        struct Dev {  // device bytes, at least one
            void *p = nullptr;
            explicit Dev(size_t bytes) { if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) throw Error(DK_E_NOMEM, "hipMalloc failed"); }
            ~Dev() { (void)hipFree(p); }
            Dev(const Dev &) = delete;
            Dev &operator=(const Dev &) = delete;
            void put(const void *src, size_t bytes) { if (bytes && hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) != hipSuccess) throw Error(DK_E_HIP, "upload failed"); }
            void get(void *dst, size_t bytes) { if (bytes && hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost) != hipSuccess) throw Error(DK_E_HIP, "download failed"); }
        };
        if (hipSetDevice(device_) != hipSuccess) throw Error(DK_E_NODEVICE, "hipSetDevice failed");
        std::vector<size_t> lens;
        std::vector<uint8_t> bytes;
        size_t longest = 1;
        for (const auto &p : patterns) {
            lens.push_back(p.size());
            bytes.insert(bytes.end(), p.begin(), p.end());
            longest = std::max(longest, p.size());
        }
        const size_t n = bwt_.size(), keep = std::min(prev.size(), longest - 1);  // only the last longest - 1 bytes of prev can matter
        Dev d_bwt(n), d_index(dk_fm_index_bytes(n, 1)), d_ext(dk_fm_extract_bytes(n, 1, ext_step_)), d_prev(keep), d_pat(bytes.size());
        Dev d_hits(max_hits * sizeof(dk_fm_seam_hit)), d_occ(patterns.size() * sizeof(uint32_t));
        d_bwt.put(bwt_.data(), n);
        d_prev.put(prev.data() + (prev.size() - keep), keep);
        d_pat.put(bytes.data(), bytes.size());
        Seams out;
        int rc = dk_dev_fm_build(ctx_.get(), static_cast<const uint8_t *>(d_bwt.p), n, static_cast<uint32_t>(origin_), d_index.p);
        if (rc == DK_OK) rc = dk_dev_fm_extract_build(ctx_.get(), static_cast<const uint8_t *>(d_bwt.p), n, static_cast<uint32_t>(origin_), ext_step_, d_ext.p);
        if (rc == DK_OK)
            rc = dk_dev_fm_seams(ctx_.get(), static_cast<const uint8_t *>(d_bwt.p), n, d_index.p, d_ext.p, ext_step_, static_cast<const uint8_t *>(d_prev.p), keep,
                                 static_cast<const uint8_t *>(d_pat.p), patterns.size(), lens.data(), max_hits, static_cast<dk_fm_seam_hit *>(d_hits.p),
                                 static_cast<uint32_t *>(d_occ.p), &out.total);
        if (rc != DK_OK) throw Error(rc, ctx_.error());
        out.occ.resize(patterns.size());
        out.hits.resize(static_cast<size_t>(std::min<uint64_t>(out.total, max_hits)));
        d_occ.get(out.occ.data(), out.occ.size() * sizeof(uint32_t));
        d_hits.get(out.hits.data(), out.hits.size() * sizeof(dk_fm_seam_hit));
        return out;
    }
#endif
    detail::Ctx &context() { return ctx_; }  // context().purpose() == DK_CTX_DECODER
private:
    detail::Ctx ctx_;
    std::vector<uint8_t> bwt_;
    size_t origin_;
    uint32_t step_, ext_step_;
    int device_;
};
}  // namespace fm

}  // namespace dark
