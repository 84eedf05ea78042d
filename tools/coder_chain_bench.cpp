// The range coder's loop alone, no threads and no rings: (a) the loop code_uniform had before the quotient was taken from the previous
// quotient (r -> s = r * w -> mulhi(s, inv') -> select, copied here as it was) against (b) code_uniform_batch as the library has it now
// (r -> (imul || mulx) -> add -> select).  Reads dc_stream.bin (tools/make_dc_sample.py), builds the uniform event array of
// the dark model once, codes it both ways in the pipeline's batches of 2048 events -- over cache-resident windows (2 000 and 12 000 events
// at five offsets of the stream) and over the whole array --, demands equal bytes (and RangeState::narrow's bytes for the whole array) and
// prints ns per decision: minimum, median and maximum of the repeats.
//   clang++ -O3 -std=c++17 -march=x86-64-v3 -mllvm -inline-threshold=20000 -falign-loops=32 -falign-functions=64 -Iinclude \
//       -o coder_chain_bench tools/coder_chain_bench.cpp dark_amd/csrc/bbb.cpp -lpthread
#include "../dark_amd/csrc/entropy.cpp"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <vector>
using namespace dk;

struct UVecSink {
    std::vector<UEvent> u;
    const uint64_t *inv = reciprocal_table();
    bool put(uint32_t total, uint32_t from, uint32_t to) { u.push_back(UEvent{total < (1u << 14) ? inv[total] : reciprocal64(total), from, to}); return true; }
    bool put_pow2(unsigned shift, uint32_t from, uint32_t to) { u.push_back(UEvent{1ull << (64 - shift), from, to}); return true; }
    bool put_bit12(uint32_t zero, bool one) { u.push_back(UEvent{1ull << 52, one ? zero : 0u, one ? 4096u : zero}); return true; }
    bool finish() { return true; }
    int error() const { return 0; }
};

// (a): the fast path of code_uniform before this tool existed, word for word
__attribute__((noinline)) static int old_batch(const UEvent *ev, uint32_t count, RangeState &rs, uint8_t **pp) {
    int err = DK_OK;
    uint8_t *p = *pp;
    uint32_t low = rs.low, span = rs.hi - rs.low;
    uint32_t r = count ? static_cast<uint32_t>((static_cast<unsigned __int128>(span) * ev[0].inv) >> 64) : 0u;
    for (uint32_t k = 0; k < count; ++k) {
        const uint64_t inv_next = ev[k + 1 < count ? k + 1 : k].inv;
        uint32_t lo = low + r * ev[k].from, h = low + r * ev[k].to, s = r * (ev[k].to - ev[k].from);
        const uint32_t r_stay = static_cast<uint32_t>((static_cast<unsigned __int128>(s) * inv_next) >> 64);
        uint32_t r_byte = static_cast<uint32_t>((static_cast<unsigned __int128>(static_cast<uint64_t>(s) << 8) * inv_next) >> 64);
        uint32_t r_stay_ = r_stay;
        __asm__("" : "+r"(r_stay_), "+r"(r_byte));
        const uint32_t x = lo ^ h;
        if (__builtin_expect(r == 0 || x == 0, 0)) { err = DK_E_INTERNAL; break; }
        const unsigned sh = static_cast<unsigned>(__builtin_clz(x)) & 24u;
        const uint32_t be = __builtin_bswap32(lo);
        std::memcpy(p, &be, 4);
        p += sh >> 3;
        lo <<= sh;
        s <<= sh;
        r = sh ? r_byte : r_stay_;
        if (__builtin_expect(sh > 8u || s <= kRangeThreshold, 0)) {
            if (s <= kRangeThreshold) {
                h = lo + s;
                int shifted = static_cast<int>(sh >> 3);
                for (;;) {
                    const uint32_t lim = h & kTopMask;
                    if (h - lim >= lim - lo) lo = lim; else h = lim - 1;
                    const uint32_t x2 = lo ^ h;
                    if (x2 == 0) { err = DK_E_INTERNAL; break; }
                    const unsigned sh2 = static_cast<unsigned>(__builtin_clz(x2)) & 24u;
                    const uint32_t be2 = __builtin_bswap32(lo);
                    std::memcpy(p, &be2, 4);
                    p += sh2 >> 3;
                    shifted += static_cast<int>(sh2 >> 3);
                    if (shifted > 4) { err = DK_E_INTERNAL; break; }
                    lo <<= sh2;
                    h <<= sh2;
                    if (h - lo > kRangeThreshold) break;
                }
                if (err) break;
                s = h - lo;
            }
            r = static_cast<uint32_t>((static_cast<unsigned __int128>(s) * inv_next) >> 64);
        }
        low = lo;
        span = s;
    }
    rs.low = low;
    rs.hi = low + span;
    *pp = p;
    return err;
}

typedef int (*BatchFn)(const UEvent *, uint32_t, RangeState &, uint8_t **);
static double now_ns() { return std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// codes ev[0 .. count) from a fresh coder state in batches of URing::kBatch; bytes written, or 0 after an error
static size_t code_all(BatchFn fn, const UEvent *ev, size_t count, uint8_t *out) {
    RangeState rs;
    uint8_t *p = out;
    for (size_t at = 0; at < count; at += URing::kBatch) {
        const uint32_t c = static_cast<uint32_t>(std::min<size_t>(URing::kBatch, count - at));
        if (fn(ev + at, c, rs, &p) != DK_OK) return 0;
    }
    for (int i = 0; i < 4; ++i) *p++ = static_cast<uint8_t>(rs.low >> (24 - 8 * i));
    return static_cast<size_t>(p - out);
}

struct Stat { double lo, med, hi; };
static Stat time_it(BatchFn fn, const UEvent *ev, size_t count, uint8_t *out, int repeats, int inner, size_t *len) {
    std::vector<double> t;
    for (int rep = 0; rep < repeats; ++rep) {
        const double t0 = now_ns();
        for (int i = 0; i < inner; ++i) *len = code_all(fn, ev, count, out);
        t.push_back((now_ns() - t0) / (static_cast<double>(inner) * static_cast<double>(count)));
    }
    std::sort(t.begin(), t.end());
    return Stat{t.front(), t[t.size() / 2], t.back()};
}

int main(int argc, char **argv) {
    const char *path = argc > 1 ? argv[1] : "dc_stream.bin";
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s (tools/make_dc_sample.py writes it)\n", path); return 2; }
    size_t n = 0, m = 0;
    uint32_t origin = 0, init[256];
    if (fread(&n, 8, 1, f) != 1 || fread(&m, 8, 1, f) != 1 || fread(&origin, 4, 1, f) != 1 || fread(init, 4, 256, f) != 256) { fprintf(stderr, "short header\n"); return 2; }
    std::vector<uint32_t> d(m);
    std::vector<uint8_t> s(m);
    if (fread(d.data(), 4, m, f) != m || fread(s.data(), 1, m, f) != m) { fprintf(stderr, "short body\n"); return 2; }
    fclose(f);
    DcStream st;
    st.n = n; st.init = init; st.dist = d.data(); st.sym = s.data(); st.m = m; st.origin = origin;
    UVecSink sink;
    sink.u.reserve(m * 5);
    {
        auto model = std::make_unique<DarkModel>();
        model->reset();
        const int rc = write_stream(*model, st, sink);
        if (rc != DK_OK) { fprintf(stderr, "write_stream: %d\n", rc); return 2; }
    }
    const std::vector<UEvent> &ev = sink.u;
    const size_t count = ev.size();
    printf("%zu distances, %zu decisions (%.2f per distance), %.1f MB of events\n", m, count, static_cast<double>(count) / static_cast<double>(m), 16e-6 * static_cast<double>(count));
    std::vector<uint8_t> out_a(4 * count + 64), out_b(4 * count + 64), out_r(4 * count + 64);
    int bad = 0;

    // the reference: RangeState::narrow, one decision at a time
    size_t len_r;
    {
        RangeState rs;
        uint8_t *p = out_r.data();
        for (const UEvent &x : ev) {
            const uint32_t r = static_cast<uint32_t>((static_cast<unsigned __int128>(rs.hi - rs.low) * x.inv) >> 64);
            const int nb = rs.narrow(r, x.from, x.to, p);
            if (nb < 0) { fprintf(stderr, "narrow failed\n"); return 2; }
            p += nb;
        }
        for (int i = 0; i < 4; ++i) *p++ = static_cast<uint8_t>(rs.low >> (24 - 8 * i));
        len_r = static_cast<size_t>(p - out_r.data());
    }

    for (const size_t window : {size_t(2000), size_t(12000)}) {
        for (int o = 0; o < 5; ++o) {
            const size_t at = (count - window) / 5 * static_cast<size_t>(o);
            const int inner = static_cast<int>(4000000 / window);
            size_t la = 0, lb = 0;
            // (a) and (b) take turns twice, so that a drift of the clock shows in both
            const Stat a1 = time_it(old_batch, ev.data() + at, window, out_a.data(), 5, inner, &la);
            const Stat b1 = time_it(code_uniform_batch, ev.data() + at, window, out_b.data(), 5, inner, &lb);
            const Stat a2 = time_it(old_batch, ev.data() + at, window, out_a.data(), 5, inner, &la);
            const Stat b2 = time_it(code_uniform_batch, ev.data() + at, window, out_b.data(), 5, inner, &lb);
            const bool same = la != 0 && la == lb && std::equal(out_a.begin(), out_a.begin() + static_cast<long>(la), out_b.begin());
            bad += same ? 0 : 1;
            printf("window %6zu at %10zu: (a) min %.3f med %.3f max %.3f | %.3f %.3f %.3f   (b) min %.3f med %.3f max %.3f | %.3f %.3f %.3f ns/decision, %zu bytes %s\n",
                   window, at, a1.lo, a1.med, a1.hi, a2.lo, a2.med, a2.hi, b1.lo, b1.med, b1.hi, b2.lo, b2.med, b2.hi, la, same ? "same" : "DIFFERENT");
        }
    }
    {
        size_t la = 0, lb = 0;
        const Stat a1 = time_it(old_batch, ev.data(), count, out_a.data(), 3, 1, &la);
        const Stat b1 = time_it(code_uniform_batch, ev.data(), count, out_b.data(), 3, 1, &lb);
        const Stat a2 = time_it(old_batch, ev.data(), count, out_a.data(), 3, 1, &la);
        const Stat b2 = time_it(code_uniform_batch, ev.data(), count, out_b.data(), 3, 1, &lb);
        const bool same = la != 0 && la == lb && la == len_r && std::equal(out_a.begin(), out_a.begin() + static_cast<long>(la), out_b.begin()) &&
                          std::equal(out_r.begin(), out_r.begin() + static_cast<long>(la), out_b.begin());
        bad += same ? 0 : 1;
        printf("whole array (events from memory): (a) min %.3f med %.3f max %.3f | %.3f %.3f %.3f   (b) min %.3f med %.3f max %.3f | %.3f %.3f %.3f ns/decision, %zu bytes %s (narrow: %zu)\n",
               a1.lo, a1.med, a1.hi, a2.lo, a2.med, a2.hi, b1.lo, b1.med, b1.hi, b2.lo, b2.med, b2.hi, la, same ? "same" : "DIFFERENT", len_r);
    }
    printf("bad: %d\n", bad);
    return bad != 0;
}
