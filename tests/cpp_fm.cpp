// dark::fm::Index (include/dark.hpp) against the definitions and against dark::saca::Constructor::search on small inputs.
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
        dark::fm::Index index = dark::fm::Index::from_text(t);
        if (index.context().purpose() != DK_CTX_DECODER || index.len() != n) { std::printf("context\n"); return 1; }
        if (index.resident_bytes() > 2 * n + 4096) { std::printf("n = %zu: %zu resident bytes\n", n, index.resident_bytes()); return 1; }
        std::vector<Bytes> pats = {Bytes(), t, Bytes{0}, Bytes{255}, Bytes{t.back()}, Bytes{t.back(), t.back()}};
        pats.push_back(t);
        pats.back().push_back('a');
        for (size_t a = 0; a < n; a += 1 + n / 37)
            for (size_t m : {size_t(1), size_t(2), size_t(5), size_t(17), size_t(300)}) {  // (the batch fits a decoder context of n bytes beside L and the index)
                Bytes p(t.begin() + static_cast<std::ptrdiff_t>(a), t.begin() + static_cast<std::ptrdiff_t>(std::min(n, a + m)));
                pats.push_back(p);
                p.push_back('b');
                pats.push_back(p);
            }
        const auto got = index.count(pats);
        const auto occ = index.occurrences(pats);
        if (got.size() != pats.size() || occ.size() != pats.size()) { std::printf("count\n"); return 1; }
        dark::saca::Constructor con(n);
        const std::vector<uint32_t> sa = con.compute(t);
        const auto want = con.search(t, sa, pats);
        for (size_t q = 0; q < pats.size(); ++q) {
            const Bytes &p = pats[q];
            size_t places = 0;
            for (size_t i = 0; i < n && i + p.size() <= n; ++i)
                if (std::equal(p.begin(), p.end(), t.begin() + static_cast<std::ptrdiff_t>(i))) ++places;
            if (got[q] != want[q] || occ[q] != places) {
                std::printf("n = %zu pattern %zu of %zu bytes: (%u, %u), the search has (%u, %u), the definition %zu places\n", n, q, p.size(), got[q].first,
                            got[q].second, want[q].first, want[q].second, places);
                return 1;
            }
        }
        if (!index.count({}).empty()) { std::printf("no patterns\n"); return 1; }
    }
    try {
        dark::fm::Index bad(bytes("abc"), 3);
        std::printf("an origin outside the block was taken\n");
        return 1;
    } catch (const dark::Error &e) {
        if (e.code != DK_E_ARG) return 1;
    }
    std::printf("cpp fm ok\n");
    return 0;
}
