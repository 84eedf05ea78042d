// Stand-alone checker of the host pipeline's range coder (tests/test_coder_chain_host.py builds it under the sanitizers):
//   events: code_uniform / code_uniform_batch over crafted streams of uniform events against RangeState::narrow, byte for byte;
//   forms <dc stream file>: every thread form of encode_block_stream against the one-thread form on a DC stream of real shape.
#include "../dark_amd/csrc/entropy.cpp"
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>
using namespace dk;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); ++g_bad; } } while (0)

static UEvent event(uint32_t total, uint32_t from, uint32_t to) { return UEvent{reciprocal64(total), from, to}; }

struct Coverage { size_t shift[4] = {0, 0, 0, 0}, cuts = 0, m_hi = 0, w1 = 0; };

// the reference: one decision at a time through RangeState::narrow, then the four bytes of the tail
static std::vector<uint8_t> reference(const std::vector<UEvent> &ev, Coverage &cov) {
    std::vector<uint8_t> out;
    RangeState rs;
    for (size_t k = 0; k < ev.size(); ++k) {
        const UEvent &x = ev[k];
        const uint32_t r = static_cast<uint32_t>((static_cast<unsigned __int128>(rs.hi - rs.low) * x.inv) >> 64);
        {   // what the first round of the renormalisation will do: bytes shifted, threshold cut or not
            const uint32_t lo = rs.low + r * x.from, h = rs.low + r * x.to;
            const unsigned sh = (lo ^ h) ? static_cast<unsigned>(__builtin_clz(lo ^ h)) & 24u : 0u;
            cov.shift[sh >> 3] += 1;
            cov.cuts += ((h - lo) << sh) <= kRangeThreshold ? 1 : 0;
            cov.w1 += x.to - x.from == 1 ? 1 : 0;
            if (k + 1 < ev.size()) cov.m_hi += static_cast<uint64_t>((static_cast<unsigned __int128>(ev[k + 1].inv) * (x.to - x.from)) >> 64) ? 1 : 0;
        }
        uint8_t tmp[8];
        const int nb = r ? rs.narrow(r, x.from, x.to, tmp) : -1;
        if (nb < 0) { CHECK(false, "the reference refuses event %zu", k); return out; }
        out.insert(out.end(), tmp, tmp + nb);
    }
    for (int i = 0; i < 4; ++i) out.push_back(static_cast<uint8_t>(rs.low >> (24 - 8 * i)));
    return out;
}

// the events through a ring filled by a second thread (whole batches, or the merger's way: up to four at a time, batches that end early)
static int through_ring(const std::vector<UEvent> &ev, bool in_fours, uint8_t *out, size_t cap, size_t *len) {
    URing ring;
    std::thread producer([&] {
        USink sink(ring);
        std::mt19937 rng(static_cast<uint32_t>(ev.size()));
        for (size_t k = 0; k < ev.size();) {
            if (!in_fours) { sink.raw(ev[k++]); continue; }
            const uint32_t c = static_cast<uint32_t>(std::min<size_t>(1 + rng() % 4, ev.size() - k));
            UEvent *o = sink.tail(4);
            for (uint32_t j = 0; j < c; ++j) o[j] = ev[k + j];
            sink.advance(c);
            k += c;
        }
        sink.finish();
    });
    const int rc = code_uniform(ring, out, cap, len);
    producer.join();
    return rc;
}

static void check_stream(const char *name, const std::vector<UEvent> &ev, Coverage &cov) {
    const std::vector<uint8_t> ref = reference(ev, cov);
    if (ref.size() < 4) return;
    // exact-size heap blocks, so that a byte written behind `cap` is seen by the address sanitizer
    struct Cap { size_t cap; int want; };
    const Cap caps[] = {{ref.size() + 4 * ev.size() + 64, DK_OK},  // the fast path to the end
                        {ref.size() + 100, DK_OK},                 // ends inside the slow path near the buffer's end
                        {ref.size(), DK_OK},                       // ... with not a byte to spare
                        {ref.size() - 1, DK_E_CAPACITY}};          // one byte too little
    for (const Cap &c : caps)
        for (int in_fours = 0; in_fours < 2; ++in_fours) {
            std::vector<uint8_t> out(c.cap);
            size_t len = 0;
            const int rc = through_ring(ev, in_fours != 0, out.data(), c.cap, &len);
            CHECK(rc == c.want, "%s (%zu events, cap %zu, fours %d): rc %d, expected %d", name, ev.size(), c.cap, in_fours, rc, c.want);
            CHECK(len <= c.cap, "%s: length %zu beyond the capacity %zu", name, len, c.cap);
            if (c.want == DK_OK && rc == DK_OK)
                CHECK(len == ref.size() && std::memcmp(out.data(), ref.data(), len) == 0, "%s (%zu events, cap %zu, fours %d): bytes differ (%zu against %zu)", name, ev.size(),
                      c.cap, in_fours, len, ref.size());
        }
    // code_uniform_batch alone, the stream cut into batches of every small size and of sizes around the ring's batch
    for (const size_t batch : {size_t(1), size_t(2), size_t(3), size_t(7), size_t(2047), size_t(2048)}) {
        if (batch > 7 && ev.size() > 6000) continue;
        if (batch <= 7 && ev.size() > 3000) continue;
        std::vector<uint8_t> out(ref.size() + 4 * ev.size() + 64);
        RangeState rs;
        uint8_t *p = out.data();
        int rc = DK_OK;
        for (size_t at = 0; at < ev.size() && rc == DK_OK; at += batch) rc = code_uniform_batch(ev.data() + at, static_cast<uint32_t>(std::min(batch, ev.size() - at)), rs, &p);
        for (int i = 0; i < 4; ++i) *p++ = static_cast<uint8_t>(rs.low >> (24 - 8 * i));
        const size_t len = static_cast<size_t>(p - out.data());
        CHECK(rc == DK_OK && len == ref.size() && std::memcmp(out.data(), ref.data(), len) == 0, "%s in batches of %zu: rc %d, %zu bytes against %zu", name, batch, rc, len, ref.size());
    }
}

static int run_events() {
    std::mt19937 rng(12345);
    Coverage cov;
    const uint32_t totals[] = {2, 3, 4095, 4096, 4097, 3u * 4096u - 1u};
    auto any = [&](uint32_t total) {  // a random interval of a given total
        const uint32_t from = rng() % total, to = from + 1 + rng() % (total - from);
        return event(total, from, to);
    };
    auto narrow1 = [&](uint32_t total) { const uint32_t from = rng() % total; return event(total, from, from + 1); };  // w = 1
    auto wide = [&](uint32_t total) { const uint32_t from = rng() % 2; return event(total, from, std::max<uint32_t>(from + 1, total - static_cast<uint32_t>(rng() % 2))); };  // w >= total - 2
    auto bit = [&] { const uint32_t zero = 1 + rng() % 4095; const bool one = rng() & 1; return UEvent{1ull << 52, one ? zero : 0u, one ? 4096u : zero}; };
    // the lengths: one event, around one batch of 2048, one batch and a stretch more, more than the ring's sixteen slots hold
    const size_t lengths[] = {1, 2, 5, 2047, 2048, 2049, 2048 + 611, 4096, 4097, 3 * 2048 + 1, 17 * 2048 + 300};
    for (const size_t count : lengths) {
        std::vector<UEvent> ev;
        // every total beside every other, any width
        ev.clear();
        for (size_t k = 0; k < count; ++k) ev.push_back(rng() % 5 ? any(totals[rng() % 6]) : bit());
        check_stream("mixed totals", ev, cov);
        // wide intervals in front of small totals: w >= total_next, M >= 2^64
        ev.clear();
        for (size_t k = 0; k < count; ++k) ev.push_back(k % 2 == 0 ? wide(totals[2 + rng() % 4]) : any(totals[rng() % 2]));
        check_stream("wide before small", ev, cov);
        // w = 1 under large totals: the span falls to one or two units per decision -- shifts of two and three bytes, threshold cuts
        ev.clear();
        for (size_t k = 0; k < count; ++k) ev.push_back(rng() % 3 ? narrow1(totals[2 + rng() % 4]) : wide(totals[rng() % 6]));
        check_stream("w = 1", ev, cov);
        // full intervals (from = 0, to = total): nothing narrows, nothing is shifted out
        ev.clear();
        for (size_t k = 0; k < count; ++k) { const uint32_t t = totals[rng() % 6]; ev.push_back(rng() % 4 ? event(t, 0, t) : narrow1(t)); }
        check_stream("full intervals", ev, cov);
    }
    // borders that straddle a byte border with a narrow span: cuts at the top byte, several rounds
    {
        std::vector<UEvent> ev;
        for (size_t k = 0; k < 5000; ++k) {
            const uint32_t b = rng() % 2;
            ev.push_back(k % 3 == 0 ? event(4096, 2047, 2049) : (k % 3 == 1 ? event(4097, 2048, 2049) : event(2, b, b + 1)));
        }
        check_stream("straddling", ev, cov);
    }
    printf("first-round shifts of 0 / 1 / 2 / 3 bytes: %zu / %zu / %zu / %zu, threshold cuts %zu, w = 1: %zu, M >= 2^64: %zu\n", cov.shift[0], cov.shift[1], cov.shift[2],
           cov.shift[3], cov.cuts, cov.w1, cov.m_hi);
    CHECK(cov.shift[0] && cov.shift[1] && cov.shift[2] && cov.shift[3] && cov.cuts && cov.w1 && cov.m_hi, "the crafted streams do not reach every case");
    // an empty interval is an error, not a loop or a wild write
    {
        std::vector<UEvent> ev(100, event(4096, 5, 9));
        ev[50] = UEvent{reciprocal64(4096), 7, 7};
        std::vector<uint8_t> out(4096);
        size_t len = 0;
        CHECK(through_ring(ev, false, out.data(), out.size(), &len) == DK_E_INTERNAL, "an empty interval must be refused");
    }
    return g_bad;
}

static int run_forms(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { printf("cannot open %s\n", path); return 2; }
    size_t n = 0, m = 0;
    uint32_t origin = 0, init[256];
    if (fread(&n, 8, 1, f) != 1 || fread(&m, 8, 1, f) != 1 || fread(&origin, 4, 1, f) != 1 || fread(init, 4, 256, f) != 256) { printf("short header\n"); return 2; }
    std::vector<uint32_t> d(m);
    std::vector<uint8_t> s(m);
    if (fread(d.data(), 4, m, f) != m || fread(s.data(), 1, m, f) != m) { printf("short body\n"); return 2; }
    fclose(f);
    const size_t smallest = size_t(1) << 21;  // what the automatic choice takes for a large block
    if (m < smallest + 4096) { printf("the stream holds %zu distances, fewer than %zu\n", m, smallest + 4096); return 2; }
    for (const size_t count : {smallest, smallest + 4096}) {
        DcStream st;
        st.n = n; st.init = init; st.dist = d.data(); st.sym = s.data(); st.m = count; st.origin = origin;
        std::vector<uint8_t> ref(4 * count + 8192), out(4 * count + 8192);
        size_t rl = 0, ol = 0;
        int rc = encode_block_stream(0, st, ref.data(), ref.size(), &rl, 1);
        CHECK(rc == DK_OK && last_entropy_threads() == 1, "one thread: rc %d", rc);
        for (const int mode : {0, 2, 4, 5}) {
            rc = encode_block_stream(0, st, out.data(), out.size(), &ol, mode);
            const int threads = last_entropy_threads();
            CHECK(rc == DK_OK && ol == rl && std::memcmp(ref.data(), out.data(), rl) == 0, "%zu distances, mode %d (%d threads): rc %d, %zu bytes against %zu", count, mode, threads, rc, ol, rl);
            if (mode && threads != mode) CHECK(host_l3_groups(mode) == 0, "mode %d: the host has a group for it, but %d threads coded", mode, threads);
            printf("%zu distances, mode %d: %d threads, %zu bytes\n", count, mode, threads, ol);
            if (count != smallest) continue;
            // one byte too little: every form reports it and ends
            rc = encode_block_stream(0, st, out.data(), rl - 1, &ol, mode);
            CHECK(rc == DK_E_CAPACITY, "%zu distances, mode %d with one byte too little: rc %d", count, mode, rc);
        }
    }
    return g_bad;
}

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "events";
    const int rc = what == "forms" && argc > 2 ? run_forms(argv[2]) : run_events();
    printf("bad: %d\n", g_bad);
    return rc != 0 || g_bad != 0;
}
