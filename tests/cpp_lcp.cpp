// dark::saca::Constructor::compute_lcp / compute_packed_lcp (include/dark.hpp) against the definition, byte by byte.
#include <cstdio>
#include <vector>

#include "dark.hpp"

static bool check(const std::vector<uint8_t> &t, const std::vector<uint32_t> &sa, const std::vector<uint32_t> &lcp) {
    if (sa.size() != t.size() || lcp.size() != t.size() || lcp[0] != 0) return false;
    for (size_t i = 1; i < t.size(); ++i) {
        size_t a = sa[i - 1], b = sa[i], k = 0;
        while (a + k < t.size() && b + k < t.size() && t[a + k] == t[b + k]) ++k;
        if (lcp[i] != k) return false;
    }
    return true;
}

int main() {
    std::vector<std::vector<uint8_t>> inputs;
    const char *words[] = {"banana", "z", "abracadabra", "mississippi", "abababababab", "banana"};
    for (const char *w : words) inputs.emplace_back(w, w + std::char_traits<char>::length(w));
    std::vector<uint8_t> big(5000);
    uint32_t x = 12345;
    for (auto &c : big) { x = x * 1664525u + 1013904223u; c = static_cast<uint8_t>('a' + (x >> 24) % 4); }
    for (size_t i = 0; i < 700; ++i) big[4000 + i] = big[100 + i];  // a repeat longer than a lane measures
    inputs.push_back(big);
    {
        dark::saca::Constructor one(6);
        const auto r = one.compute_lcp(inputs[0]);
        const std::vector<uint32_t> sa = {5, 3, 1, 0, 4, 2}, lcp = {0, 1, 3, 0, 0, 2};
        if (r.first != sa || r.second != lcp) { std::printf("banana\n"); return 1; }
        try {
            one.compute_lcp(inputs[1]);
            std::printf("a wrong size was taken\n");
            return 1;
        } catch (const dark::Error &e) {
            if (e.code != DK_E_ARG) return 1;
        }
    }
    size_t total = 0;
    for (const auto &in : inputs) total += in.size();
    dark::saca::Constructor packed(total);
    const auto got = packed.compute_packed_lcp(inputs);
    if (got.size() != inputs.size()) { std::printf("count\n"); return 1; }
    for (size_t i = 0; i < inputs.size(); ++i) {
        if (!check(inputs[i], got[i].first, got[i].second)) { std::printf("packed input %zu\n", i); return 1; }
        dark::saca::Constructor one(inputs[i].size());
        const auto r = one.compute_lcp(inputs[i]);
        if (r.first != got[i].first || r.second != got[i].second) { std::printf("input %zu differs from the pack\n", i); return 1; }
    }
    std::printf("cpp lcp ok\n");
    return 0;
}
