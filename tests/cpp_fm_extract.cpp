// dark::fm::Index::extract (include/dark.hpp) against the text itself: the whole text through one range, and ranges around every chunk border.
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
        for (uint32_t step : {1u, 32u, 4096u}) {
            dark::fm::Index index = dark::fm::Index::from_text(t, 0, 0, step);
            if (index.context().purpose() != DK_CTX_DECODER) { std::printf("context\n"); return 1; }
            if (index.resident_bytes() != n + dk_fm_index_bytes(n, 1) + dk_fm_extract_bytes(n, 1, step)) { std::printf("resident bytes\n"); return 1; }
            const auto whole = index.extract({0}, n);
            if (whole.size() != 1 || whole[0] != t) { std::printf("n = %zu step %u: the range (0, n) does not give the text\n", n, step); return 1; }
            std::vector<uint32_t> starts = {0, static_cast<uint32_t>(n - 1), static_cast<uint32_t>(n), static_cast<uint32_t>(n + 7), DK_FM_NO_HIT};
            for (size_t a = 0; a < n; a += 1 + n / 29) starts.push_back(static_cast<uint32_t>(a));
            for (size_t k = 1; k * step < n && k < 8; ++k)
                for (size_t d : {size_t(0), size_t(1), size_t(2)}) starts.push_back(static_cast<uint32_t>(k * step + d - 1));
            for (size_t length : {size_t(1), size_t(7), size_t(33), size_t(300)}) {
                const auto got = index.extract(starts, length);
                if (got.size() != starts.size()) { std::printf("extract\n"); return 1; }
                for (size_t q = 0; q < starts.size(); ++q) {
                    const size_t a = starts[q], e = a < n ? std::min(n, a + length) : a;
                    const Bytes want = a < n ? Bytes(t.begin() + static_cast<std::ptrdiff_t>(a), t.begin() + static_cast<std::ptrdiff_t>(e)) : Bytes();
                    if (got[q] != want) { std::printf("n = %zu step %u length %zu range %zu at %zu\n", n, step, length, q, a); return 1; }
                }
            }
            if (!index.extract({}, 5).empty()) { std::printf("no ranges\n"); return 1; }
        }
        try {
            dark::fm::Index::from_text(t, 0, 32).extract({0}, 1);
            std::printf("extracted without a structure\n");
            return 1;
        } catch (const dark::Error &e) {
            if (e.code != DK_E_ARG) return 1;
        }
    }
    // locate, then extract at the hits: every snippet starts with its pattern
    {
        dark::fm::Index index = dark::fm::Index::from_text(big, 0, 32, 8);
        const Bytes p(big.begin() + 100, big.begin() + 110);
        const auto hits = index.locate({p}, 4);
        if (hits.size() != 1 || hits[0].size() < 2) { std::printf("the repeated stretch has two places\n"); return 1; }
        for (const Bytes &row : index.extract(hits[0], p.size()))
            if (row != p) { std::printf("a snippet is not its pattern\n"); return 1; }
    }
    try {
        dark::fm::Index bad(bytes("abc"), 0, 0, 0, 3);
        std::printf("a step of 3 was taken\n");
        return 1;
    } catch (const dark::Error &e) {
        if (e.code != DK_E_ARG) return 1;
    }
    std::printf("cpp fm extract ok\n");
    return 0;
}
