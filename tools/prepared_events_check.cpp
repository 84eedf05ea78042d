// Stand-alone checker of the host coder's prepared events and its six-stage form (tests/test_prepared_events.py builds it plain and under
// the sanitizers).  It includes entropy.cpp and calls encode_six_stages directly, so the gate of 2^21 distances does not apply:
//   steps:   one decision of code_prepared_batch from chosen quotients r (1, 2^12 +- 1, 2^24 +- 1, 2^31 - 1, random) and random event pairs
//            against RangeState::narrow: the same (low, span, bytes);
//   events:  crafted uniform events through ring U, the prepare stage and code_prepared on three threads against RangeState::narrow --
//            threshold cuts and shifts of two and three bytes in consecutive decisions and at a batch's first and last event;
//   streams: DC streams through the six-stage form against the one-thread form -- distances all zero, distances up to 2^31 - 2 (unary
//            extensions to log 31), 2048 k - 1, 2048 k and 2048 k + 1 decisions for k = 1, 2, 17, a frontier that advances in pieces, a
//            poisoned frontier (every thread ends, DK_E_HIP), one byte too little.
//   clang++ -O1 -g -std=c++17 -march=x86-64-v3 -Iinclude -o prepared_events_check tools/prepared_events_check.cpp dark_amd/csrc/bbb.cpp -lpthread
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
static uint32_t quotient(uint32_t span, uint64_t inv) { return static_cast<uint32_t>((static_cast<unsigned __int128>(span) * inv) >> 64); }

// what the first round of the renormalisation does with a decision: bytes shifted out (4: an empty interval), threshold cut or not
struct Kind { unsigned shift; bool cut; bool rare() const { return shift >= 2 || cut; } };
static Kind kind_of(const RangeState &rs, const UEvent &x) {
    const uint32_t r = quotient(rs.hi - rs.low, x.inv), lo = rs.low + r * x.from, h = rs.low + r * x.to;
    if (!(lo ^ h)) return Kind{4, false};
    const unsigned sh = static_cast<unsigned>(__builtin_clz(lo ^ h)) & 24u;
    return Kind{sh >> 3, ((h - lo) << sh) <= kRangeThreshold};
}

// ---------------------------------------------------------------------------------------------------------------- steps
static int run_steps() {
    std::mt19937_64 rng(2024);
    const uint32_t edge_r[] = {1u, (1u << 12) - 1, (1u << 12) + 1, (1u << 24) - 1, (1u << 24) + 1, 0x7FFFFFFFu};
    const uint32_t totals[] = {2, 3, 4, 255, 256, 4095, 4096, 4097, 12287, 32767};
    size_t done = 0, rare = 0, byte_out = 0;
    for (int trial = 0; trial < 120000; ++trial) {
        // a coder state whose quotient under the first event's total is the chosen r: span = r * total + rest, above the threshold
        const uint32_t want_r = trial % 2 ? edge_r[(trial / 2) % 6] : static_cast<uint32_t>(rng() >> (33 + rng() % 31));
        if (want_r == 0) continue;
        uint32_t total0 = 0;
        for (int tries = 0; tries < 64 && !total0; ++tries) {
            const uint32_t t = totals[rng() % 10];
            const uint64_t span = static_cast<uint64_t>(want_r) * t;
            if (span > kRangeThreshold && span + t - 1 <= 0xFFFFFFFFull) total0 = t;
        }
        if (!total0) continue;
        RangeState start;
        const uint64_t span0 = static_cast<uint64_t>(want_r) * total0 + rng() % total0;
        start.low = static_cast<uint32_t>(rng() % (0x100000000ull - span0));
        start.hi = start.low + static_cast<uint32_t>(span0);
        UEvent ev[3];
        for (int k = 0; k < 3; ++k) {
            const uint32_t t = k == 0 ? total0 : totals[rng() % 10];
            const uint32_t from = static_cast<uint32_t>(rng() % t), width = rng() % 3 == 0 ? 1u : 1u + static_cast<uint32_t>(rng() % (t - from));
            ev[k] = (t == 4096 && rng() % 2) ? UEvent{1ull << 52, from, from + width} : event(t, from, from + width);
        }
        CHECK(quotient(start.hi - start.low, ev[0].inv) == want_r, "trial %d: the state does not give r = %u", trial, want_r);
        // the reference: three decisions through narrow
        RangeState ref = start;
        uint8_t ref_out[32], out[32];
        std::memset(ref_out, 0xEE, sizeof ref_out);
        std::memset(out, 0xEE, sizeof out);
        size_t ref_len = 0;
        bool ok = true;
        for (int k = 0; k < 3 && ok; ++k) {
            const Kind kd = kind_of(ref, ev[k]);
            if (k < 2) { rare += kd.rare() ? 1 : 0; byte_out += kd.shift == 1 ? 1 : 0; }
            const uint32_t r = quotient(ref.hi - ref.low, ev[k].inv);
            uint8_t tmp[8];
            const int nb = r ? ref.narrow(r, ev[k].from, ev[k].to, tmp) : -1;
            if (nb < 0) { ok = false; break; }
            std::memcpy(ref_out + ref_len, tmp, static_cast<size_t>(nb));
            ref_len += static_cast<size_t>(nb);
        }
        PEvent pe[3];
        uint64_t inv[3];
        CHECK(prepare_batch(ev, 3, pe, inv), "trial %d: prepare_batch refuses events inside the bounds", trial);
        for (int k = 0; k < 3; ++k)
            CHECK(pe[k].from() == ev[k].from && pe[k].to() == ev[k].to && inv[k] == ev[k].inv && pe[k].m_hi8() == pe[k].m_hi() << 8 && pe[k].m_hi() < (1u << 14),
                  "trial %d: event %d does not come back out of its prepared form", trial, k);
        RangeState rs = start;
        uint8_t *p = out;
        const int rc = code_prepared_batch(pe, inv, 3, rs, &p);
        if (!ok) { CHECK(rc == DK_E_INTERNAL, "trial %d: the reference refuses, the prepared step gives %d", trial, rc); continue; }
        const size_t len = static_cast<size_t>(p - out);
        CHECK(rc == DK_OK && rs.low == ref.low && rs.hi - rs.low == ref.hi - ref.low && len == ref_len && std::memcmp(out, ref_out, len) == 0,
              "trial %d (r = %u): rc %d, low %08x / %08x, span %08x / %08x, %zu / %zu bytes", trial, want_r, rc, rs.low, ref.low, rs.hi - rs.low, ref.hi - ref.low, len, ref_len);
        ++done;
    }
    printf("steps: %zu triples compared, %zu rare-path decisions, %zu one-byte shifts\n", done, rare, byte_out);
    CHECK(done > 50000 && rare > 100 && byte_out > 1000, "the step check does not reach every path");
    return g_bad;
}

// ---------------------------------------------------------------------------------------------------------------- events
static std::vector<uint8_t> reference(const std::vector<UEvent> &ev) {
    std::vector<uint8_t> out;
    RangeState rs;
    for (size_t k = 0; k < ev.size(); ++k) {
        const uint32_t r = quotient(rs.hi - rs.low, ev[k].inv);
        uint8_t tmp[8];
        const int nb = r ? rs.narrow(r, ev[k].from, ev[k].to, tmp) : -1;
        if (nb < 0) { CHECK(false, "the reference refuses event %zu", k); return out; }
        out.insert(out.end(), tmp, tmp + nb);
    }
    for (int i = 0; i < 4; ++i) out.push_back(static_cast<uint8_t>(rs.low >> (24 - 8 * i)));
    return out;
}

// ring U filled by one thread, prepared by a second, coded by the caller
static int through_prepared(const std::vector<UEvent> &ev, uint8_t *out, size_t cap, size_t *len) {
    URing ring_u;
    PRing ring_p;
    int rc_p = DK_OK;
    std::thread producer([&] {
        USink sink(ring_u);
        for (const UEvent &x : ev) sink.raw(x);
        sink.finish();
    });
    std::thread preparer([&] { rc_p = prepare_uniform(ring_u, ring_p); });
    const int rc = code_prepared(ring_p, out, cap, len);
    preparer.join();
    producer.join();
    return rc_p ? rc_p : rc;
}

static void check_events(const char *name, const std::vector<UEvent> &ev) {
    const std::vector<uint8_t> ref = reference(ev);
    if (ref.size() < 4) return;
    struct Cap { size_t cap; int want; };
    const Cap caps[] = {{ref.size() + 4 * ev.size() + 64, DK_OK}, {ref.size() + 100, DK_OK}, {ref.size(), DK_OK}, {ref.size() - 1, DK_E_CAPACITY}};
    for (const Cap &c : caps) {  // exact-size heap blocks: a byte written behind `cap` is seen by the address sanitizer
        std::vector<uint8_t> out(c.cap);
        size_t len = 0;
        const int rc = through_prepared(ev, out.data(), c.cap, &len);
        CHECK(rc == c.want && len <= c.cap, "%s (%zu events, cap %zu): rc %d, expected %d, %zu bytes", name, ev.size(), c.cap, rc, c.want, len);
        if (c.want == DK_OK && rc == DK_OK) CHECK(len == ref.size() && std::memcmp(out.data(), ref.data(), len) == 0, "%s (%zu events, cap %zu): bytes differ", name, ev.size(), c.cap);
    }
}

static int run_events() {
    std::mt19937 rng(99);
    const uint32_t totals[] = {2, 3, 4095, 4096, 4097, 3u * 4096u - 1u};
    auto any = [&](uint32_t total) { const uint32_t from = rng() % total; return event(total, from, from + 1 + rng() % (total - from)); };
    auto narrow1 = [&](uint32_t total) { const uint32_t from = rng() % total; return event(total, from, from + 1); };
    // A stream that puts rare-path decisions (cuts, shifts of two and three bytes) where they hurt: the last event of a batch, the first of
    // the next, and runs of them in a row.  The coder's state is followed along, and at such a place candidates are tried until one does it.
    const size_t count = 17 * 2048 + 300;
    std::vector<UEvent> ev;
    RangeState rs;
    size_t at_first = 0, at_last = 0, in_a_row = 0, shift2 = 0, shift3 = 0, cuts = 0;
    bool previous_rare = false;
    for (size_t k = 0; k < count; ++k) {
        const size_t in_batch = k % 2048;
        const bool want_rare = in_batch >= 2044 || in_batch <= 3 || (k % 97) < 3;
        UEvent x = rng() % 4 ? any(totals[rng() % 6]) : narrow1(totals[2 + rng() % 4]);
        if (want_rare) {
            const unsigned want_shift = 2 + k % 2;  // a shift of two or three bytes, else a cut, else whatever is rare
            int grade = -1;
            for (int tries = 0; tries < 4000; ++tries) {
                const UEvent c = tries % 3 == 2 ? event(2, rng() % 2, (rng() % 2) + 1) : narrow1(totals[2 + rng() % 4]);
                if (c.from >= c.to) continue;
                const Kind kd = kind_of(rs, c);
                const int g = kd.shift == 4 ? -1 : (kd.shift == want_shift ? 3 : (kd.cut ? 2 : (kd.rare() ? 1 : 0)));
                if (g > grade) { grade = g; x = c; }
                if (grade == 3 || (grade == 2 && tries > 400)) break;
            }
        } else if (kind_of(rs, x).shift == 4) {
            x = event(2, 0, 2);  // (never an empty interval here: that is run_events' last case)
        }
        const Kind kd = kind_of(rs, x);
        at_first += kd.rare() && in_batch == 0 ? 1 : 0;
        at_last += kd.rare() && in_batch == 2047 ? 1 : 0;
        in_a_row += kd.rare() && previous_rare ? 1 : 0;
        shift2 += kd.shift == 2 ? 1 : 0;
        shift3 += kd.shift == 3 ? 1 : 0;
        cuts += kd.cut ? 1 : 0;
        previous_rare = kd.rare();
        uint8_t tmp[8];
        const uint32_t r = quotient(rs.hi - rs.low, x.inv);
        if (!r || rs.narrow(r, x.from, x.to, tmp) < 0) { CHECK(false, "the crafted stream stops at event %zu", k); break; }
        ev.push_back(x);
    }
    printf("events: rare-path decisions at a batch's first event %zu, at its last %zu, behind another %zu; shifts of two bytes %zu, of three %zu, cuts %zu\n", at_first,
           at_last, in_a_row, shift2, shift3, cuts);
    CHECK(at_first >= 4 && at_last >= 4 && in_a_row >= 50 && shift2 >= 50 && shift3 >= 5 && cuts >= 50, "the crafted stream does not reach every case");
    check_events("rare paths at the batch borders", ev);
    for (const size_t n : {size_t(1), size_t(2), size_t(2047), size_t(2048), size_t(2049), size_t(4096), size_t(4097)}) {
        std::vector<UEvent> part(ev.begin() + 2040, ev.begin() + 2040 + static_cast<long>(n));  // (starts on the rare events in front of a border)
        check_events("a stretch of the crafted stream", part);
    }
    {   // an empty interval, and an event outside the layout's bounds, are errors -- not loops or wild writes
        std::vector<UEvent> bad(3000, event(4096, 5, 9));
        bad[2500] = UEvent{reciprocal64(4096), 7, 7};
        std::vector<uint8_t> out(16384);
        size_t len = 0;
        CHECK(through_prepared(bad, out.data(), out.size(), &len) == DK_E_INTERNAL, "an empty interval must be refused");
        bad[2500] = UEvent{reciprocal64(4096), 7, 70000};
        CHECK(through_prepared(bad, out.data(), out.size(), &len) == DK_E_INTERNAL, "an event wider than 2^15 must be refused");
    }
    return g_bad;
}

// ---------------------------------------------------------------------------------------------------------------- streams
struct CountSink {
    size_t count = 0;
    bool put(uint32_t, uint32_t, uint32_t) { ++count; return true; }
    bool put_pow2(unsigned, uint32_t, uint32_t) { ++count; return true; }
    bool put_bit12(uint32_t, bool) { ++count; return true; }
    bool finish() { return true; }
    int error() const { return 0; }
};
static size_t decisions_of(const DcStream &st) {
    auto model = std::make_unique<DarkModel>();
    model->reset();
    CountSink sink;
    if (write_stream(*model, st, sink) != DK_OK) return 0;
    return sink.count;
}

static bool g_claim = true;  // false: the host has no L3 group with six usable cores -- the same six threads, unconfined
static int six(const DcStream &st, uint8_t *out, size_t cap, size_t *len) {
    auto model = std::make_unique<DarkModel>();
    model->reset();
    return encode_six_stages(*model, st, out, cap, len, g_claim);
}

struct Stream {
    std::vector<uint32_t> d;
    std::vector<uint8_t> s;
    uint32_t init[256];
    size_t n = 0x7FFFFFFEu;  // the largest block the dark model takes
    DcStream view() const {
        DcStream st;
        st.n = n; st.init = init; st.dist = d.data(); st.sym = s.data(); st.m = d.size(); st.origin = 4242;
        return st;
    }
};

static void check_stream(const char *name, const Stream &sm, bool short_buffer) {
    const DcStream st = sm.view();
    std::vector<uint8_t> ref(8 * st.m + 8192), out(8 * st.m + 8192);
    size_t rl = 0, ol = 0;
    int rc = encode_block_stream(0, st, ref.data(), ref.size(), &rl, 1);
    CHECK(rc == DK_OK, "%s: one thread rc %d", name, rc);
    if (rc != DK_OK) return;
    rc = six(st, out.data(), out.size(), &ol);
    CHECK(rc == DK_OK && ol == rl && std::memcmp(ref.data(), out.data(), rl) == 0, "%s (%zu distances): six stages rc %d, %zu bytes against %zu", name, st.m, rc, ol, rl);
    if (short_buffer) {
        std::vector<uint8_t> tight(rl - 1);  // an exact heap block
        rc = six(st, tight.data(), tight.size(), &ol);
        CHECK(rc == DK_E_CAPACITY && ol <= tight.size(), "%s with one byte too little: rc %d, %zu bytes", name, rc, ol);
    }
}

static int run_streams() {
    std::mt19937_64 rng(5);
    {
        std::vector<uint8_t> out(4096);
        size_t len = 0;
        Stream probe;
        for (int i = 0; i < 256; ++i) probe.init[i] = i < 4 ? static_cast<uint32_t>(i) : static_cast<uint32_t>(probe.n);
        probe.d.assign(10, 0);
        probe.s.assign(10, 1);
        const int rc = six(probe.view(), out.data(), out.size(), &len);
        if (rc == DK_E_NODEVICE) { g_claim = false; printf("streams: no L3 group with six usable cores here: the six threads run unconfined\n"); }
        else printf("streams: the six threads run inside one L3 group (%d groups with six cores)\n", host_l3_groups(6));
    }
    auto fresh = [&](int symbols) {
        Stream sm;
        for (int i = 0; i < 256; ++i) sm.init[i] = i < symbols ? static_cast<uint32_t>(3 * i) : static_cast<uint32_t>(sm.n);
        return sm;
    };
    {   // distances all zero
        Stream sm = fresh(7);
        sm.d.assign(50000, 0);
        sm.s.resize(50000);
        for (auto &c : sm.s) c = static_cast<uint8_t>(rng() % 7);
        check_stream("all zero", sm, true);
    }
    {   // every bit length up to 31, the largest distance the model takes (2^31 - 2) among them: unary extensions to log 31
        Stream sm = fresh(200);
        for (int k = 0; k < 60000; ++k) {
            const unsigned bits = 1 + static_cast<unsigned>(rng() % 31);
            uint32_t v = static_cast<uint32_t>(rng()) >> (32 - bits);
            if (k % 1000 == 0) v = 0x7FFFFFFEu;
            if (v > 0x7FFFFFFEu) v = 0x7FFFFFFEu;
            sm.d.push_back(v);
            sm.s.push_back(static_cast<uint8_t>(rng() % 200));
        }
        check_stream("up to 2^31 - 2", sm, true);
    }
    for (const size_t k : {size_t(1), size_t(2), size_t(17)})
        for (const int off : {-1, 0, 1}) {  // exactly 2048 k - 1, 2048 k, 2048 k + 1 decisions: a distance of zero is one decision
            const size_t want = 2048 * k + static_cast<size_t>(off);
            Stream sm = fresh(3);
            for (int j = 0; j < 150; ++j) { sm.d.push_back(static_cast<uint32_t>(rng() % 50)); sm.s.push_back(static_cast<uint8_t>(rng() % 3)); }  // at most six decisions each
            const size_t base = decisions_of(sm.view());
            CHECK(base && base < want, "the base stream has %zu decisions, %zu wanted", base, want);
            if (!base || base >= want) continue;
            sm.d.insert(sm.d.end(), want - base, 0u);
            sm.s.insert(sm.s.end(), want - base, 1);
            const size_t got = decisions_of(sm.view());
            CHECK(got == want, "%zu decisions, %zu wanted", got, want);
            char name[64];
            snprintf(name, sizeof name, "%zu decisions", want);
            check_stream(name, sm, k == 2);
        }
    {   // a stream that is still arriving: the frontier advances in pieces of every size while the six threads wait at it
        Stream sm = fresh(100);
        for (int k = 0; k < 120000; ++k) { sm.d.push_back(static_cast<uint32_t>(rng() % (1u << (rng() % 20)))); sm.s.push_back(static_cast<uint8_t>(rng() % 100)); }
        DcStream st = sm.view();
        std::vector<uint8_t> ref(8 * st.m + 8192), out(8 * st.m + 8192);
        size_t rl = 0, ol = 0;
        int rc = encode_block_stream(0, st, ref.data(), ref.size(), &rl, 1);
        CHECK(rc == DK_OK, "gated: one thread rc %d", rc);
        std::atomic<size_t> ready{0};
        st.ready = &ready;
        std::thread feeder([&] {
            std::mt19937 r2(3);
            for (size_t have = 0; have < st.m;) {
                have = std::min(st.m, have + 1 + r2() % 4096);
                ready.store(have, std::memory_order_release);
                std::this_thread::yield();
            }
        });
        rc = six(st, out.data(), out.size(), &ol);
        feeder.join();
        CHECK(rc == DK_OK && ol == rl && std::memcmp(ref.data(), out.data(), rl) == 0, "gated: six stages rc %d, %zu bytes against %zu", rc, ol, rl);
        // the producer gives up half way: every thread ends, and the pass says DK_E_HIP
        ready.store(0);
        std::thread poisoner([&] {
            ready.store(st.m / 3, std::memory_order_release);
            std::this_thread::yield();
            ready.store(DC_STREAM_POISON, std::memory_order_release);
        });
        rc = six(st, out.data(), out.size(), &ol);
        poisoner.join();
        CHECK(rc == DK_E_HIP, "poisoned frontier: rc %d, expected DK_E_HIP", rc);
    }
    return g_bad;
}

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "all";
    if (what == "steps" || what == "all") run_steps();
    if (what == "events" || what == "all") run_events();
    if (what == "streams" || what == "all") run_streams();
    printf("bad: %d\n", g_bad);
    return g_bad != 0;
}
