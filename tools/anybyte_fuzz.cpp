// Robustness of the any-byte stream form (DK_MODEL_ANYBYTE), meant to be built with -fsanitize=address,undefined (CPU only):
//   clang++ -O1 -g -fsanitize=address,undefined -std=c++17 -march=x86-64-v3 -Iinclude -o /tmp/anybyte_fuzz tools/anybyte_fuzz.cpp dark_amd/csrc/entropy.cpp -lpthread
// Round-trips flagged streams of run strings with symbol 0xFF present, absent and alone through every model, then decodes thousands of streams
// with a mutated or truncated prefix or body and a claimed n that may lie: every call must return DK_OK or DK_E_STREAM and write nothing
// outside bwt_out[0, n).
#include "../dark_amd/csrc/entropy.hpp"
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
using namespace dk;

namespace {
constexpr size_t GUARD = 64;
constexpr uint8_t CANARY = 0xC7;

struct Dc {
    std::vector<uint32_t> init, dist;
    std::vector<uint8_t> sym;
};

// bwt::dc::encode restated by brute force for the fuzzer's own use (O(n * sigma), small n): one entry per run, in position order
Dc dc_of(const std::vector<uint8_t> &l) {
    const size_t n = l.size();
    Dc r;
    r.init.assign(256, static_cast<uint32_t>(n));
    std::vector<long> last(256, -1);
    std::vector<uint32_t> sparse(n, static_cast<uint32_t>(n));
    auto rank_of = [&](int c) {
        unsigned rank = 0;
        for (int o = 0; o < 256; ++o) rank += (o != c && last[o] > last[c]);
        return rank;
    };
    for (size_t i = 0; i < n; ++i) {
        const uint8_t c = l[i];
        if (i > 0 && l[i - 1] == c) { last[c] = static_cast<long>(i); continue; }
        if (last[c] < 0) r.init[c] = static_cast<uint32_t>(i);
        else sparse[static_cast<size_t>(last[c])] = static_cast<uint32_t>(i - static_cast<size_t>(last[c]) - rank_of(c) - 1);
        last[c] = static_cast<long>(i);
    }
    for (int c = 0; c < 256; ++c)
        if (last[c] >= 0) sparse[static_cast<size_t>(last[c])] = static_cast<uint32_t>(n - static_cast<size_t>(last[c]) - rank_of(c) - 1);
    for (size_t i = 0; i < n; ++i)
        if (sparse[i] != n) { r.dist.push_back(sparse[i]); r.sym.push_back(l[i]); }
    return r;
}

// decode into a buffer with canaries on both sides of [0, n); returns the code, *clean = the canaries are untouched
int guarded_decode(int model, const std::vector<uint8_t> &in, size_t n, std::vector<uint8_t> *out, uint32_t *origin, int *single, size_t *consumed,
                   bool *clean) {
    std::vector<uint8_t> buf(n + 2 * GUARD, CANARY);
    // (an empty input still needs a non-null pointer: null is DK_E_ARG, not a stream error)
    static const uint8_t none = 0;
    const int rc = decode_block_stream(model, in.empty() ? &none : in.data(), in.size(), n, buf.data() + GUARD, origin, single, consumed);
    *clean = true;
    for (size_t k = 0; k < GUARD; ++k) *clean = *clean && buf[k] == CANARY && buf[GUARD + n + k] == CANARY;
    if (out) out->assign(buf.begin() + static_cast<long>(GUARD), buf.begin() + static_cast<long>(GUARD + n));
    return rc;
}

void put_u32(std::vector<uint8_t> &s, uint32_t v) {
    for (int i = 0; i < 4; ++i) s[static_cast<size_t>(i)] = static_cast<uint8_t>(v >> (8 * i));
}
}  // namespace

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 400;
    std::mt19937_64 rng(4242);
    size_t failures = 0, decoded_ok = 0, errors = 0, blocks = 0;
    // kind 0: 0xFF among other symbols; 1: no 0xFF; 2: nothing but 0xFF; 3: 0xFF and one other symbol; 4: every byte value
    for (int kind = 0; kind < 5; ++kind) {
        for (int rep = 0; rep < 6; ++rep) {
            const size_t n = rep == 0 ? 1 : rep == 1 ? 2 + rng() % 15 : 17 + rng() % 9000;
            std::vector<uint8_t> l(n);
            for (size_t i = 0; i < n;) {
                uint8_t s;
                switch (kind) {
                case 0: s = (rng() % 5 == 0) ? 0xFF : static_cast<uint8_t>(rng() % 40); break;
                case 1: s = static_cast<uint8_t>(rng() % 255); break;
                case 2: s = 0xFF; break;
                case 3: s = (rng() % 2) ? 0xFF : 0xFE; break;
                default: s = static_cast<uint8_t>(rng()); break;
                }
                size_t len = 1 + rng() % 6;
                while (len-- && i < n) l[i++] = s;
            }
            if (kind == 0) l[rng() % n] = 0xFF;  // present for certain
            const Dc dc = dc_of(l);
            const uint32_t first_ff = dc.init[255];  // n when absent
            size_t distinct = 0;
            for (int c = 0; c < 256; ++c) distinct += dc.init[static_cast<size_t>(c)] < n;
            const uint32_t want_origin = static_cast<uint32_t>(rng() % n);
            DcStream st;
            st.n = n; st.init = dc.init.data(); st.dist = dc.dist.data(); st.sym = dc.sym.data(); st.m = dc.dist.size(); st.origin = want_origin;
            ++blocks;
            for (int model = 0; model < 4; ++model) {
                const int flagged = model | DK_MODEL_ANYBYTE;
                std::vector<uint8_t> plain(8 * dc.dist.size() + 8192), out(plain.size() + 4);
                size_t plain_len = 0, len = 0;
                int rc = encode_block_stream(model, st, plain.data(), plain.size(), &plain_len, 1);
                if (rc) { printf("kind %d n %zu model %d: plain encode rc=%d\n", kind, n, model, rc); ++failures; continue; }
                rc = encode_block_stream(flagged, st, out.data(), out.size(), &len, 1);
                if (rc || len != plain_len + 4) { printf("kind %d n %zu model %d: encode rc=%d len %zu / %zu\n", kind, n, model, rc, len, plain_len); ++failures; continue; }
                out.resize(len);
                uint32_t prefix = 0;
                for (int i = 0; i < 4; ++i) prefix |= static_cast<uint32_t>(out[static_cast<size_t>(i)]) << (8 * i);
                if (prefix != first_ff || !std::equal(out.begin() + 4, out.end(), plain.begin())) {
                    printf("kind %d n %zu model %d: prefix %u (want %u) or body differs\n", kind, n, model, prefix, first_ff);
                    ++failures;
                }
                std::vector<uint8_t> back, with_tail(out);
                with_tail.insert(with_tail.end(), 9, 0x5A);  // the next record
                uint32_t origin = 0; int single = 0; size_t consumed = 0; bool clean = false;
                rc = guarded_decode(flagged, with_tail, n, &back, &origin, &single, &consumed, &clean);
                if (rc || !clean || back != l || origin != want_origin || consumed != len || single != (distinct == 1)) {
                    printf("kind %d n %zu model %d: round trip failed rc=%d clean=%d origin %u/%u consumed %zu/%zu single %d\n", kind, n, model, rc, clean,
                           origin, want_origin, consumed, len, single);
                    ++failures;
                }
                // corrupt inputs
                const uint32_t nn = static_cast<uint32_t>(n);
                const uint32_t prefixes[] = {0u, first_ff - 1u, first_ff + 1u, nn, nn + 1u, 0xFFFFFFFFu, nn - 1u, 0x80000000u};
                for (int r = 0; r < rounds; ++r) {
                    std::vector<uint8_t> bad(out);
                    const int what = static_cast<int>(rng() % 6);
                    bool prefix_past_n = false;
                    if (what == 0) {
                        bad.resize(rng() % 8 < 3 ? rng() % 5 : rng() % (len + 1));  // truncation, often inside the prefix
                    } else if (what == 1 || what == 2) {
                        put_u32(bad, prefixes[rng() % 8]);
                        if (what == 2 && len > 4) bad[4 + rng() % (len - 4)] ^= static_cast<uint8_t>(1u << (rng() % 8));
                    } else if (what == 3) {
                        put_u32(bad, static_cast<uint32_t>(rng()));
                    } else if (what == 4) {
                        for (int k = 0; k < 1 + static_cast<int>(rng() % 4); ++k) bad[rng() % len] ^= static_cast<uint8_t>(1u << (rng() % 8));
                    } else {
                        for (size_t k = 4 + rng() % (len - 3); k < len; k += 1 + rng() % 97) bad[k] = static_cast<uint8_t>(rng());
                        bad.resize(len + rng() % 32, 0x33);
                    }
                    const size_t claim_n = (rng() % 6 == 0) ? 1 + rng() % (2 * n) : n;  // the record's n may lie too
                    if (bad.size() >= 4) {
                        uint32_t p = 0;
                        for (int i = 0; i < 4; ++i) p |= static_cast<uint32_t>(bad[static_cast<size_t>(i)]) << (8 * i);
                        prefix_past_n = p > claim_n;
                    }
                    rc = guarded_decode(flagged, bad, claim_n, nullptr, &origin, &single, &consumed, &clean);
                    if (!clean) { printf("kind %d n %zu model %d: a write outside bwt_out[0, %zu)\n", kind, n, model, claim_n); ++failures; }
                    if (rc != DK_OK && rc != DK_E_STREAM) { printf("kind %d n %zu model %d: rc=%d\n", kind, n, model, rc); ++failures; }
                    if ((bad.size() < 4 || prefix_past_n) && rc != DK_E_STREAM) {
                        printf("kind %d n %zu model %d: %zu bytes, prefix past n %d -> rc=%d\n", kind, n, model, bad.size(), prefix_past_n, rc);
                        ++failures;
                    }
                    if (rc == DK_OK && consumed > bad.size()) { printf("kind %d n %zu model %d: consumed %zu of %zu\n", kind, n, model, consumed, bad.size()); ++failures; }
                    if (rc) ++errors; else ++decoded_ok;
                }
            }
        }
    }
    // the flag where it does not belong
    {
        std::vector<uint8_t> l(100, 7);
        const Dc dc = dc_of(l);
        DcStream st;
        st.n = 100; st.init = dc.init.data(); st.dist = dc.dist.data(); st.sym = dc.sym.data(); st.m = dc.dist.size(); st.origin = 3;
        std::vector<uint8_t> out(4096), back(100);
        size_t len = 0;
        uint32_t origin = 0; int single = 0;
        const int ids[] = {DK_MODEL_RAWDC | DK_MODEL_ANYBYTE, 5 | DK_MODEL_ANYBYTE, 0x200, 0x300, -1};
        for (int id : ids) {
            if (encode_block_stream(id, st, out.data(), out.size(), &len, 1) != DK_E_MODEL) { printf("model id %d: encode accepted\n", id); ++failures; }
            if (decode_block_stream(id, out.data(), 64, 100, back.data(), &origin, &single, nullptr) != DK_E_MODEL) { printf("model id %d: decode accepted\n", id); ++failures; }
        }
        uint32_t d = 1; uint8_t s = 1;
        if (model_encode_stream(DK_MODEL_DARK | DK_MODEL_ANYBYTE, &d, &s, 1, out.data(), out.size(), &len) != DK_E_MODEL) { printf("model level: encode accepted\n"); ++failures; }
        if (model_decode_stream(DK_MODEL_DARK | DK_MODEL_ANYBYTE, out.data(), 16, &s, 1, &d) != DK_E_MODEL) { printf("model level: decode accepted\n"); ++failures; }
    }
    printf("blocks %zu, failures %zu, corrupt inputs: %zu rejected, %zu decoded to something\n", blocks, failures, errors, decoded_ok);
    return failures ? 1 : 0;
}
