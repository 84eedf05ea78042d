// dark::fm::Index::locate (include/dark.hpp) against the definition -- every place a pattern occurs -- and against the suffix array.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "dark.hpp"

using Bytes = std::vector<uint8_t>;

static Bytes bytes(const std::string &s) { return Bytes(s.begin(), s.end()); }

int main() {
    Bytes big(5000);
    uint32_t x = 4321;
    for (auto &c : big) { x = x * 1664525u + 1013904223u; c = static_cast<uint8_t>('a' + (x >> 24) % 4); }
    for (size_t i = 0; i < 700; ++i) big[4000 + i] = big[100 + i];
    for (const Bytes &t : {bytes("banana"), bytes("abracadabra"), bytes("z"), bytes("abab"), Bytes(1500, 'a'), big}) {
        const size_t n = t.size();
        dark::saca::Constructor con(n);
        const std::vector<uint32_t> sa = con.compute(t);
        for (uint32_t step : {1u, 32u, 4096u}) {
            dark::fm::Index index = dark::fm::Index::from_text(t, 0, step);
            if (index.context().purpose() != DK_CTX_DECODER) { std::printf("context\n"); return 1; }
            if (index.resident_bytes() != n + dk_fm_index_bytes(n, 1) + dk_fm_locate_bytes(n, 1, step)) { std::printf("resident bytes\n"); return 1; }
            std::vector<Bytes> pats = {Bytes(), t, Bytes{0}, Bytes{t.back()}, Bytes{t.front()}};
            for (size_t a = 0; a < n; a += 1 + n / 23)
                for (size_t m : {size_t(1), size_t(2), size_t(5), size_t(40)})
                    pats.emplace_back(t.begin() + static_cast<std::ptrdiff_t>(a), t.begin() + static_cast<std::ptrdiff_t>(std::min(n, a + m)));
            const auto ranges = index.count(pats);
            // (the whole suffix array through the empty pattern alone: the batch has to fit a decoder context of n bytes beside the structures)
            const auto whole = index.locate({Bytes()}, n);
            if (whole.size() != 1 || whole[0] != sa) { std::printf("n = %zu step %u: the empty pattern does not give the suffix array\n", n, step); return 1; }
            for (size_t max_hits : {size_t(1), size_t(7)}) {
                const auto got = index.locate(pats, max_hits);
                if (got.size() != pats.size()) { std::printf("locate\n"); return 1; }
                for (size_t q = 0; q < pats.size(); ++q) {
                    const Bytes &p = pats[q];
                    const size_t want = std::min<size_t>(ranges[q].second - ranges[q].first, max_hits);
                    bool ok = got[q].size() == want;
                    for (size_t j = 0; ok && j < want; ++j) {
                        const uint32_t at = got[q][j];
                        ok = at == sa[ranges[q].first + j] && at + p.size() <= n && std::equal(p.begin(), p.end(), t.begin() + at);
                    }
                    if (!ok) { std::printf("n = %zu step %u max_hits %zu pattern %zu of %zu bytes\n", n, step, max_hits, q, p.size()); return 1; }
                }
            }
            if (!index.locate({}).empty()) { std::printf("no patterns\n"); return 1; }
        }
        try {
            dark::fm::Index::from_text(t).locate({Bytes()});
            std::printf("located without a structure\n");
            return 1;
        } catch (const dark::Error &e) {
            if (e.code != DK_E_ARG) return 1;
        }
    }
    try {
        dark::fm::Index bad(bytes("abc"), 0, 0, 3);
        std::printf("a step of 3 was taken\n");
        return 1;
    } catch (const dark::Error &e) {
        if (e.code != DK_E_ARG) return 1;
    }
    std::printf("cpp fm locate ok\n");
    return 0;
}
