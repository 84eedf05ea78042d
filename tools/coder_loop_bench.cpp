// What binds the range coder's loop: its dependent chain (seven cycles) or what the core retires per cycle?  No threads and no
// rings.  Reads dc_stream.bin (tools/make_dc_sample.py), builds the dark model's uniform events once, pins itself to one core of the L3 group
// the product would claim, and codes the events three ways:
//   (u)   code_uniform_batch, the library's loop over 16-byte uniform events (M = (to - from) * inv_next is formed inside the loop);
//   (p16) code_prepared_batch over the library's 16-byte prepared events (from, to, M_lo, M_hi, M_hi << 8 all loaded, nothing derived);
//   (p24) the same loop over a plain 24-byte prepared event (every field a word of its own), defined here.
// Cache-resident windows of 2 048 and 12 288 events at five offsets, and the whole array from memory in batches of 2 048, 4 096 and 8 192.
// Every timing stands between two runs of a dependent-multiply loop on the same core (imul: three cycles), which give the cycle time.
// Prints ns and cycles per decision (minimum, median, maximum of the repeats), the decision mix, and demands RangeState::narrow's bytes.
//   clang++ -O3 -std=c++17 -march=x86-64-v3 -mllvm -inline-threshold=20000 -falign-loops=32 -falign-functions=64 -Iinclude \
//       -o coder_loop_bench tools/coder_loop_bench.cpp dark_amd/csrc/bbb.cpp -lpthread
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

// the plain layout: 24 bytes, every factor a word of its own
struct PEvent24 {
    uint64_t m_lo;
    uint32_t from_, to_, m_hi_, m_hi8_;
    static PEvent24 pack(uint32_t from, uint32_t to, uint64_t m_lo, uint64_t m_hi) { return PEvent24{m_lo, from, to, static_cast<uint32_t>(m_hi), static_cast<uint32_t>(m_hi << 8)}; }
    uint32_t from() const { return from_; }
    uint32_t to() const { return to_; }
    uint32_t m_hi() const { return m_hi_; }
    uint32_t m_hi8() const { return m_hi8_; }
};
static_assert(sizeof(PEvent24) == 24, "plain prepared event is 24 bytes");

static double now_ns() { return std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ns per cycle: a chain of dependent 64-bit multiplies, three cycles each on every x86 core this runs on
static double cycle_ns() {
    uint64_t x = 0x9E3779B97F4A7C15ull;
    const int n = 6000000;
    const double t0 = now_ns();
    for (int i = 0; i < n; i += 8) {
#pragma GCC unroll 8
        for (int j = 0; j < 8; ++j) { x *= 0xD1342543DE82EF95ull; __asm__("" : "+r"(x)); }
    }
    const double dt = now_ns() - t0;
    __asm__ volatile("" : : "r"(x));
    return dt / (3.0 * n);
}

// one way of coding an event array in batches of `batch`: the events as that loop wants them, laid out once
struct Way {
    const char *name;
    std::vector<UEvent> u;
    std::vector<PEvent> p16;
    std::vector<PEvent24> p24;
    std::vector<uint64_t> inv;
    int kind;  // 0 u, 1 p16, 2 p24
    size_t bytes_per_event() const { return kind == 2 ? 24 : 16; }
    void build(int k, const UEvent *ev, size_t count, size_t batch) {
        kind = k;
        name = k == 0 ? "u" : (k == 1 ? "p16" : "p24");
        if (k == 0) { u.assign(ev, ev + count); return; }
        inv.resize(count);
        if (k == 1) p16.resize(count); else p24.resize(count);
        for (size_t at = 0; at < count; at += batch) {
            const uint32_t c = static_cast<uint32_t>(std::min(batch, count - at));
            const bool ok = k == 1 ? prepare_batch(ev + at, c, p16.data() + at, inv.data() + at) : prepare_batch(ev + at, c, p24.data() + at, inv.data() + at);
            if (!ok) { fprintf(stderr, "an event outside the prepared layout's bounds\n"); exit(2); }
        }
    }
    size_t code(size_t count, size_t batch, uint8_t *out) const {
        RangeState rs;
        uint8_t *p = out;
        for (size_t at = 0; at < count; at += batch) {
            const uint32_t c = static_cast<uint32_t>(std::min(batch, count - at));
            const int rc = kind == 0 ? code_uniform_batch(u.data() + at, c, rs, &p)
                         : kind == 1 ? code_prepared_batch(p16.data() + at, inv.data() + at, c, rs, &p)
                                     : code_prepared_batch(p24.data() + at, inv.data() + at, c, rs, &p);
            if (rc != DK_OK) return 0;
        }
        for (int i = 0; i < 4; ++i) *p++ = static_cast<uint8_t>(rs.low >> (24 - 8 * i));
        return static_cast<size_t>(p - out);
    }
};

struct Stat { double lo, med, hi, cyc; };
static Stat time_it(const Way &w, size_t count, size_t batch, uint8_t *out, int repeats, int inner, size_t *len) {
    std::vector<double> t;
    double cyc = 0;
    for (int rep = 0; rep < repeats; ++rep) {
        const double c0 = cycle_ns();
        const double t0 = now_ns();
        for (int i = 0; i < inner; ++i) *len = w.code(count, batch, out);
        t.push_back((now_ns() - t0) / (static_cast<double>(inner) * static_cast<double>(count)));
        cyc += 0.5 * (c0 + cycle_ns());
    }
    std::sort(t.begin(), t.end());
    return Stat{t.front(), t[t.size() / 2], t.back(), cyc / repeats};
}
static void show(const Stat &s, const char *name) {
    printf("  (%s) %.3f %.3f %.3f ns = %.2f %.2f %.2f cycles of %.4f ns", name, s.lo, s.med, s.hi, s.lo / s.cyc, s.med / s.cyc, s.hi / s.cyc, s.cyc);
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

    // one core of the L3 group the pipeline would claim (six cores, else five, else wherever this thread is)
    ThreadPair tp;
    const bool claimed = tp.acquire(6) || tp.acquire(5);
#if defined(__linux__)
    if (claimed) {
        for (int c = 0; c < CPU_SETSIZE; ++c)
            if (CPU_ISSET(c, &tp.group)) {
                cpu_set_t one;
                CPU_ZERO(&one);
                CPU_SET(c, &one);
                (void)pthread_setaffinity_np(pthread_self(), sizeof(one), &one);
                break;
            }
    }
    printf("pinned to cpu %d (L3 group of cpu %d%s)\n", sched_getcpu(), tp.me, claimed ? "" : ": none claimed");
#endif

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
    printf("%zu distances, %zu decisions (%.2f per distance)\n", m, count, static_cast<double>(count) / static_cast<double>(m));
    std::vector<uint8_t> out(4 * count + 64), out_r(4 * count + 64);
    int bad = 0;

    // the reference, RangeState::narrow one decision at a time, and the decision mix on the way
    size_t len_r;
    {
        size_t table = 0, flat = 0, shift[5] = {0, 0, 0, 0, 0}, cuts = 0, stay_small = 0;
        RangeState rs;
        uint8_t *p = out_r.data();
        for (const UEvent &x : ev) {
            const uint32_t r = static_cast<uint32_t>((static_cast<unsigned __int128>(rs.hi - rs.low) * x.inv) >> 64);
            table += x.inv != (1ull << 52) ? 1 : 0;
            flat += x.inv == (1ull << 52) && x.to - x.from == 2048u && (x.from == 0 || x.from == 2048u) ? 1 : 0;  // (a learned probability of exactly 1/2 counts too)
            const uint32_t lo = rs.low + r * x.from, h = rs.low + r * x.to;
            const unsigned sh = (lo ^ h) ? static_cast<unsigned>(__builtin_clz(lo ^ h)) >> 3 : 4u;
            shift[sh] += 1;
            cuts += ((h - lo) << (8 * (sh & 3u))) <= kRangeThreshold ? 1 : 0;
            stay_small += sh == 0 && h - lo < (1u << 24) ? 1 : 0;
            const int nb = rs.narrow(r, x.from, x.to, p);
            if (nb < 0) { fprintf(stderr, "narrow failed\n"); return 2; }
            p += nb;
        }
        for (int i = 0; i < 4; ++i) *p++ = static_cast<uint8_t>(rs.low >> (24 - 8 * i));
        len_r = static_cast<size_t>(p - out_r.data());
        const double c = 100.0 / static_cast<double>(count);
        printf("mix: table %.1f %%, binary %.1f %% (flat bits %.1f %% of all); first-round shift of 0 / 1 / 2 / 3 bytes %.2f / %.2f / %.3f / %.4f %%, threshold cuts %.4f %%, "
               "no shift with a span below 2^24 %.1f %%\n", c * table, c * (count - table), c * flat, c * shift[0], c * shift[1], c * shift[2], c * shift[3], c * cuts, c * stay_small);
    }

    for (const size_t window : {size_t(2048), size_t(12288)}) {
        for (int o = 0; o < 5; ++o) {
            const size_t at = (count - window) / 5 * static_cast<size_t>(o);
            const int inner = static_cast<int>(4000000 / window);
            Way w[3];
            for (int k = 0; k < 3; ++k) w[k].build(k, ev.data() + at, window, URing::kBatch);
            printf("window %5zu at %9zu:", window, at);
            size_t len[3] = {0, 0, 0};
            for (int turn = 0; turn < 2; ++turn)  // the three take turns twice, so that a drift of the clock shows in all
                for (int k = 0; k < 3; ++k) {
                    const Stat st1 = time_it(w[k], window, URing::kBatch, out.data(), 5, inner, &len[k]);
                    show(st1, w[k].name);
                }
            const bool same = len[0] != 0 && len[0] == len[1] && len[0] == len[2];
            bad += same ? 0 : 1;
            printf("  %zu bytes %s\n", len[0], same ? "same length" : "DIFFERENT");
        }
    }
    for (const size_t batch : {size_t(2048), size_t(4096), size_t(8192)}) {
        printf("whole array, batches of %zu:", batch);
        for (int k = 0; k < 3; ++k) {
            Way w;
            w.build(k, ev.data(), count, batch);
            size_t len = 0;
            const Stat st1 = time_it(w, count, batch, out.data(), 3, 1, &len);
            show(st1, w.name);
            const bool same = len == len_r && std::equal(out_r.begin(), out_r.begin() + static_cast<long>(len_r), out.begin());
            bad += same ? 0 : 1;
            printf(" %s", same ? "narrow's bytes" : "DIFFERENT");
        }
        printf("  (%zu bytes)\n", len_r);
    }
    if (claimed) tp.release();
    printf("bad: %d\n", bad);
    return bad != 0;
}
