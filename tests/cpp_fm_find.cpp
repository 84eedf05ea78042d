// dark::fm::Index::find (include/dark.hpp) against the definition -- every place a pattern occurs -- and against count and the suffix array.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "dark.hpp"

using Bytes = std::vector<uint8_t>;

static Bytes bytes(const std::string &s) { return Bytes(s.begin(), s.end()); }

int main() {
    static_assert(sizeof(dk_fm_hit) == 16, "a record is 16 bytes");
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
            std::vector<Bytes> pats = {Bytes(), t, Bytes{0}, Bytes{t.back()}, Bytes{t.front()}};
            for (size_t a = 0; a < n; a += 1 + n / 23)
                for (size_t m : {size_t(1), size_t(2), size_t(5), size_t(40)})
                    pats.emplace_back(t.begin() + static_cast<std::ptrdiff_t>(a), t.begin() + static_cast<std::ptrdiff_t>(std::min(n, a + m)));
            const auto ranges = index.count(pats);
            uint64_t total = 0;
            for (const auto &r : ranges) total += r.second - r.first;
            // (the records have to fit a decoder context of n bytes beside the structures: a prefix of the list, not all of it)
            for (size_t max_hits : {size_t(64), size_t(7), size_t(0)}) {
                const auto got = index.find(pats, max_hits);
                if (got.total != total || got.occ.size() != pats.size() || got.hits.size() != std::min<uint64_t>(total, max_hits)) {
                    std::printf("n = %zu step %u max_hits %zu: total %llu, expected %llu\n", n, step, max_hits, static_cast<unsigned long long>(got.total),
                                static_cast<unsigned long long>(total));
                    return 1;
                }
                size_t h = 0;
                for (size_t q = 0; q < pats.size(); ++q) {
                    const Bytes &p = pats[q];
                    if (got.occ[q] != ranges[q].second - ranges[q].first) { std::printf("occ of pattern %zu\n", q); return 1; }
                    for (uint32_t slot = ranges[q].first; slot < ranges[q].second && h < got.hits.size(); ++slot, ++h) {
                        const dk_fm_hit &r = got.hits[h];
                        const bool ok = r.pattern == q && r.block == 0 && r.slot == slot && r.position == sa[slot] && r.position + p.size() <= n &&
                                        std::equal(p.begin(), p.end(), t.begin() + r.position);
                        if (!ok) { std::printf("n = %zu step %u max_hits %zu record %zu (pattern %zu of %zu bytes)\n", n, step, max_hits, h, q, p.size()); return 1; }
                    }
                }
                if (h != got.hits.size()) { std::printf("records behind the last range\n"); return 1; }
            }
            const auto none = index.find({});
            if (none.total != 0 || !none.occ.empty() || !none.hits.empty()) { std::printf("no patterns\n"); return 1; }
        }
        dark::fm::Index plain = dark::fm::Index::from_text(t);
        if (plain.find({Bytes()}, 0).total != n) { std::printf("counting without a structure\n"); return 1; }
        try {
            plain.find({Bytes()});
            std::printf("found without a structure\n");
            return 1;
        } catch (const dark::Error &e) {
            if (e.code != DK_E_ARG) return 1;
        }
    }
    std::printf("cpp fm find ok\n");
    return 0;
}
