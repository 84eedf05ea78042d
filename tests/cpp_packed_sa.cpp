// dark::saca::Constructor::compute_packed (include/dark.hpp) against compute on every input alone.
#include <cstdio>
#include <vector>

#include "dark.hpp"

int main() {
    std::vector<std::vector<uint8_t>> inputs;
    const char *words[] = {"banana", "z", "abracadabra", "mississippi", "abababababab"};
    for (const char *w : words) inputs.emplace_back(w, w + std::char_traits<char>::length(w));
    std::vector<uint8_t> big(5000);
    uint32_t x = 12345;
    for (auto &c : big) { x = x * 1664525u + 1013904223u; c = static_cast<uint8_t>('a' + (x >> 24) % 4); }
    inputs.push_back(big);
    size_t total = 0;
    for (const auto &in : inputs) total += in.size();
    dark::saca::Constructor packed(total);
    const auto got = packed.compute_packed(inputs);
    if (got.size() != inputs.size()) { std::printf("count\n"); return 1; }
    for (size_t i = 0; i < inputs.size(); ++i) {
        dark::saca::Constructor one(inputs[i].size());
        if (one.compute(inputs[i]) != got[i]) { std::printf("input %zu differs\n", i); return 1; }
    }
    inputs.push_back({'x'});
    try {
        packed.compute_packed(inputs);
        std::printf("a pack above the capacity was taken\n");
        return 1;
    } catch (const dark::Error &e) {
        if (e.code != DK_E_ARG) return 1;
    }
    std::printf("cpp packed sa ok\n");
    return 0;
}
