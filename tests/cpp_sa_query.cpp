// dark::saca::Constructor::check / search (include/dark.hpp) against the definitions on small inputs.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "dark.hpp"

using Bytes = std::vector<uint8_t>;

static Bytes bytes(const std::string &s) { return Bytes(s.begin(), s.end()); }

int main() {
    Bytes big(5000);
    uint32_t x = 12345;
    for (auto &c : big) { x = x * 1664525u + 1013904223u; c = static_cast<uint8_t>('a' + (x >> 24) % 4); }
    for (size_t i = 0; i < 700; ++i) big[4000 + i] = big[100 + i];  // a repeat longer than a lane compares
    for (const Bytes &t : {bytes("banana"), bytes("abracadabra"), bytes("z"), bytes("abab"), big}) {
        const size_t n = t.size();
        dark::saca::Constructor con(n);
        const std::vector<uint32_t> sa = con.compute(t);
        if (n == 6 && sa != std::vector<uint32_t>{5, 3, 1, 0, 4, 2}) { std::printf("banana\n"); return 1; }
        auto r = con.check(t, sa);
        if (r.first != DK_SA_OK || r.second != n) { std::printf("a valid array: %u %u\n", r.first, r.second); return 1; }
        if (n > 1) {
            std::vector<uint32_t> bad = sa;
            std::swap(bad[0], bad[n - 1]);
            r = con.check(t, bad);
            if (r.first != DK_SA_BAD_ORDER || r.second < 1 || r.second >= n) { std::printf("swapped: %u %u\n", r.first, r.second); return 1; }
            bad = sa;
            bad[n / 2] = static_cast<uint32_t>(n);
            r = con.check(t, bad);
            if (r.first != DK_SA_BAD_RANGE || r.second != n / 2) { std::printf("range: %u %u\n", r.first, r.second); return 1; }
            bad = sa;
            bad[1] = bad[0];
            r = con.check(t, bad);
            if (r.first != DK_SA_NOT_PERMUTATION || r.second != sa[1]) { std::printf("duplicate: %u %u\n", r.first, r.second); return 1; }
        }
        // patterns: pieces of the text, the same with a byte appended, the empty one, the whole text and more
        std::vector<Bytes> pats = {Bytes(), t, Bytes{0}, Bytes{255}};
        pats.push_back(t);
        pats.back().push_back('a');
        for (size_t a = 0; a < n; a += 1 + n / 37)
            for (size_t m : {size_t(1), size_t(2), size_t(5), size_t(17), size_t(300), size_t(800)}) {
                Bytes p(t.begin() + static_cast<std::ptrdiff_t>(a), t.begin() + static_cast<std::ptrdiff_t>(std::min(n, a + m)));
                pats.push_back(p);
                p.push_back('b');
                pats.push_back(p);
            }
        const auto got = con.search(t, sa, pats);
        if (got.size() != pats.size()) { std::printf("count\n"); return 1; }
        for (size_t q = 0; q < pats.size(); ++q) {
            const Bytes &p = pats[q];
            std::vector<uint32_t> want, have(sa.begin() + got[q].first, sa.begin() + got[q].second);
            for (size_t i = 0; i < n && i + p.size() <= n; ++i)  // (the empty pattern: at every position)
                if (std::equal(p.begin(), p.end(), t.begin() + static_cast<std::ptrdiff_t>(i))) want.push_back(static_cast<uint32_t>(i));
            std::sort(have.begin(), have.end());
            if (have != want) { std::printf("n = %zu pattern %zu of %zu bytes: %zu places, the definition has %zu\n", n, q, p.size(), have.size(), want.size()); return 1; }
            // where nothing occurs, lo == hi is the insertion slot
            const auto cut = [&](uint32_t slot) { return Bytes(t.begin() + sa[slot], t.begin() + static_cast<std::ptrdiff_t>(std::min<size_t>(n, sa[slot] + p.size()))); };
            if (got[q].first > 0 && !(cut(got[q].first - 1) < p)) { std::printf("n = %zu pattern %zu: the slot in front of lo\n", n, q); return 1; }
            if (got[q].second < n && !(p < cut(got[q].second))) { std::printf("n = %zu pattern %zu: the slot at hi\n", n, q); return 1; }
        }
        if (!con.search(t, sa, {}).empty()) { std::printf("no patterns\n"); return 1; }
        try {
            con.check(t, std::vector<uint32_t>(n + 1));
            std::printf("a wrong size was taken\n");
            return 1;
        } catch (const dark::Error &e) {
            if (e.code != DK_E_ARG) return 1;
        }
    }
    std::printf("cpp sa query ok\n");
    return 0;
}
