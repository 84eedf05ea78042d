// dark::fm::Index::seams (include/dark.hpp) against the definition: the occurrences in prev + text that start in prev and end in the text; with
// find they are every occurrence that does not lie inside prev.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#define DARK_WITH_HIP
#include "dark.hpp"

using Bytes = std::vector<uint8_t>;

static Bytes bytes(const std::string &s) { return Bytes(s.begin(), s.end()); }
static Bytes join(const Bytes &a, const Bytes &b) { Bytes out(a); out.insert(out.end(), b.begin(), b.end()); return out; }
static std::vector<size_t> places(const Bytes &t, const Bytes &p) {
    std::vector<size_t> out;
    for (size_t i = 0; i + p.size() <= t.size(); ++i)
        if (std::equal(p.begin(), p.end(), t.begin() + static_cast<std::ptrdiff_t>(i))) out.push_back(i);
    return out;
}

int main() {
    static_assert(sizeof(dk_fm_seam_hit) == 16, "a record is 16 bytes");
    Bytes big(5000);
    uint32_t x = 4321;
    for (auto &c : big) { x = x * 1664525u + 1013904223u; c = static_cast<uint8_t>('a' + (x >> 24) % 3); }
    const std::vector<std::pair<Bytes, Bytes>> cases = {{bytes("ban"), bytes("anabanana")}, {bytes("abab"), bytes("cab")}, {Bytes(70, 'a'), Bytes(150, 'a')},
                                                        {Bytes(big.begin(), big.begin() + 90), Bytes(big.begin() + 90, big.end())}, {Bytes(), bytes("abab")}};
    for (const auto &c : cases) {
        const Bytes &prev = c.first, &t = c.second, whole = join(prev, t);
        for (uint32_t step : {1u, 32u, 4096u}) {
            dark::fm::Index index = dark::fm::Index::from_text(t, 0, step, step);
            const Bytes most(whole.begin(), whole.begin() + static_cast<std::ptrdiff_t>(std::min<size_t>(whole.size(), 4000)));  // (below the bound)
            std::vector<Bytes> pats = {Bytes(), most, Bytes{t.front()}, bytes("an"), bytes("aa"), Bytes(66, 'a'), Bytes(71, 'a'), Bytes(221, 'a')};
            for (size_t back : {size_t(1), size_t(2), size_t(40)})
                for (size_t ahead : {size_t(1), size_t(3), size_t(30)})
                    if (back <= prev.size() && ahead <= t.size())
                        pats.emplace_back(whole.begin() + static_cast<std::ptrdiff_t>(prev.size() - back), whole.begin() + static_cast<std::ptrdiff_t>(prev.size() + ahead));
            // the definition: starts in front of the text, ends inside it; in file order of the starts = back descending
            std::vector<dk_fm_seam_hit> want;
            std::vector<uint32_t> want_occ(pats.size(), 0);
            for (size_t q = 0; q < pats.size(); ++q)
                for (size_t i : places(whole, pats[q]))
                    if (pats[q].size() >= 2 && i < prev.size() && i + pats[q].size() > prev.size()) {
                        want.push_back(dk_fm_seam_hit{static_cast<uint32_t>(q), 0u, static_cast<uint32_t>(prev.size() - i), 0u});
                        ++want_occ[q];
                    }
            const auto inside = index.find(pats, 0);
            for (size_t q = 1; q < pats.size(); ++q) {  // find + seams + what lies inside prev = every occurrence
                const size_t in_prev = places(prev, pats[q]).size();
                if (inside.occ[q] + want_occ[q] + in_prev != places(whole, pats[q]).size()) { std::printf("the invariant, pattern %zu\n", q); return 1; }
            }
            for (size_t max_hits : {want.size() + 2, size_t(3), size_t(0)}) {
                const auto got = index.seams(pats, prev, max_hits);
                if (got.total != want.size() || got.occ != want_occ || got.hits.size() != std::min(want.size(), max_hits)) {
                    std::printf("n = %zu prev %zu step %u max_hits %zu: total %llu, expected %zu\n", t.size(), prev.size(), step, max_hits,
                                static_cast<unsigned long long>(got.total), want.size());
                    return 1;
                }
                for (size_t h = 0; h < got.hits.size(); ++h) {
                    const dk_fm_seam_hit &r = got.hits[h], &w = want[h];
                    if (r.pattern != w.pattern || r.block != 0 || r.back != w.back || r.reserved != 0) {
                        std::printf("n = %zu prev %zu step %u max_hits %zu record %zu\n", t.size(), prev.size(), step, max_hits, h);
                        return 1;
                    }
                }
            }
            // a longer prev changes nothing: only its last bytes can matter
            if (index.seams(pats, join(Bytes(5000, 'q'), prev)).total != want.size()) { std::printf("a long prev\n"); return 1; }
            const auto none = index.seams({}, prev);
            if (none.total != 0 || !none.occ.empty() || !none.hits.empty()) { std::printf("no patterns\n"); return 1; }
        }
        dark::fm::Index plain = dark::fm::Index::from_text(t, 0, 32);
        try {
            plain.seams({bytes("ab")}, prev);
            std::printf("seams without a structure\n");
            return 1;
        } catch (const dark::Error &e) {
            if (e.code != DK_E_ARG) return 1;
        }
    }
    std::printf("cpp fm seams ok\n");
    return 0;
}
