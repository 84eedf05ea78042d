// dark::saca::Constructor::match / smems (include/dark.hpp) on "banana" x 50 and a batch of two queries, against the answers of
// tests/sa_match_model.py (match_model / smem_records on suffix_array_plain), written down here.
#include <cstdio>
#include <string>
#include <vector>

#include "dark.hpp"

using Bytes = std::vector<uint8_t>;
using Words = std::vector<uint32_t>;

static Bytes bytes(const std::string &s) { return Bytes(s.begin(), s.end()); }

struct Want { size_t max_len; Words len, lo, hi; std::vector<dk_sa_smem> smems; };

int main() {
    Bytes t;
    for (int k = 0; k < 50; ++k)
        for (char c : std::string("banana")) t.push_back(static_cast<uint8_t>(c));
    const std::vector<Bytes> queries = {bytes("xbananab"), bytes("ananas")};
    const Want wants[2] = {
        {5, {0, 5, 5, 5, 4, 3, 2, 1, 5, 4, 3, 2, 1, 0}, {0, 150, 100, 251, 51, 201, 1, 150, 100, 250, 50, 200, 0, 0},
         {300, 200, 150, 300, 100, 250, 50, 200, 150, 300, 150, 300, 150, 300}, {{1, 5, 150, 200}, {8, 5, 100, 150}}},
        {1000, {0, 7, 6, 5, 4, 3, 2, 1, 5, 4, 3, 2, 1, 0}, {0, 151, 101, 251, 51, 201, 1, 150, 100, 250, 50, 200, 0, 0},
         {300, 200, 150, 300, 100, 250, 50, 200, 150, 300, 150, 300, 150, 300}, {{1, 7, 151, 200}, {8, 5, 100, 150}}}};
    dark::saca::Constructor con(t.size());
    const Words sa = con.compute(t);
    for (const Want &w : wants) {
        const auto m = con.match(t, sa, queries, w.max_len);
        if (m.len != w.len || m.lo != w.lo || m.hi != w.hi) { std::printf("match at max_len %zu\n", w.max_len); return 1; }
        for (size_t max_hits : {size_t(65536), size_t(1), size_t(0)}) {
            const auto s = con.smems(t, sa, queries, 2, w.max_len, max_hits);  // (min_len 2: the lone "a" and "b" matches fall out)
            if (s.total != w.smems.size() || s.hits.size() != std::min(max_hits, w.smems.size())) { std::printf("smems: %zu of %llu\n", s.hits.size(), static_cast<unsigned long long>(s.total)); return 1; }
            for (size_t k = 0; k < s.hits.size(); ++k)
                if (s.hits[k].at != w.smems[k].at || s.hits[k].len != w.smems[k].len || s.hits[k].lo != w.smems[k].lo || s.hits[k].hi != w.smems[k].hi) {
                    std::printf("smem %zu at max_len %zu\n", k, w.max_len);
                    return 1;
                }
        }
    }
    if (!con.match(t, sa, {}, 5).len.empty() || con.smems(t, sa, {Bytes()}, 0, 5).total != 0) { std::printf("no queries\n"); return 1; }
    try {
        con.match(t, sa, queries, 0);
        std::printf("max_len 0 was taken\n");
        return 1;
    } catch (const dark::Error &e) {
        if (e.code != DK_E_ARG) return 1;
    }
    try {
        con.smems(t, Words(t.size() + 1), queries, 0, 5);
        std::printf("a wrong size was taken\n");
        return 1;
    } catch (const dark::Error &e) {
        if (e.code != DK_E_ARG) return 1;
    }
    std::printf("cpp sa match ok\n");
    return 0;
}
