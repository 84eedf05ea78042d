// L-FIRST: the BWT without the suffix array.  (Included by suffix_array.hip inside its anonymous namespace.)
//
// A caller that wants L and the origin (compress::bwt::TransformIterator as driven by src/block/dc.rs:45-50) never looks at the order
// of the suffixes themselves.  After the initial sort every slot of L already holds the symbol in front of the suffix standing there
// (BwtCarry), and a group of suffixes -- equal in the symbols sorted so far -- whose members all have the SAME symbol in front is done:
// whatever order its members end up in, its stretch of L is that symbol repeated.  Only groups with different symbols in front (and the
// group of suffix 0, whose exact place is the origin) have to be refined further, and since nobody needs ranks for that -- a group is
// refined from the TEXT behind its members, independently of every other group -- the refinement of a group that fits a workgroup's
// LDS runs to its end inside ONE kernel: no rank array, no inverse permutation, no rank scatter, no compaction between rounds.
// Inside long repeats (the plateau of prefix doubling: copied passages, boilerplate) the symbol in front is the same by construction;
// only the first suffix of a repeat has to be told apart from its copies, by comparing the text behind them directly.
//
//   lf_rerank       heads where the key changes; a group is LIVE when it has more than one member and (two different symbols in front, or
//                   suffix 0 among its members).  k_lf_reduce decides groups inside a tile, k_lf_straddle the groups that cross tile borders,
//                   the scan and k_lf_apply compact the live groups into the active list (finals: L is written, nothing else is)
//   k_lf_finish     every live group of at most LF_CAP members: seven more bytes of text per step, inside LDS, until every subgroup is a
//                   singleton or has one symbol in front; members of bigger groups are copied to the big list (global sort, next lf_rerank)
//   k_lf_deep       groups that did not split for three steps (long repeats; short runs, periodic stretches): every member is measured against
//                   one of them -- bytes in common, and who is smaller where they part -- and the group is ordered by that
//   k_lf_lce        ... and where they have more than 64 KiB in common (copies of whole files) the whole grid does the measuring
// Everything else (periodic or run-dominated input, giant groups that do not shrink) falls back to the suffix-array path above: the result is
// the same L either way.  DESIGN.md section 4.1, item 10; the models the kernels were written from: tests/test_lfirst_logic.py.

constexpr uint32_t LF_HEAD = 1, LF_SURV = 2, LF_EDGE_FIRST = 8, LF_EDGE_LAST = 16;
struct LfTile {
    uint32_t n_first;   // slots of the tile in front of its first head (the whole tile when it has none): tail of a group that began earlier
    uint32_t n_last;    // slots from the tile's last head to its end (0: the tile has no head, or its last group ends with the list)
    uint8_t c_first, c_last;        // those stretches hold a reason to stay live (two symbols in front / suffix 0)
    uint8_t has_head;
    uint8_t live_first, live_last;  // k_lf_straddle: the groups those stretches belong to are live
    uint8_t pad[3];
};
static_assert(sizeof(LfTile) == 16, "LfTile");

// k_lf_reduce: flags of every slot, aggregates of the groups that lie inside one tile, LfTile for the rest.
//   keys   sorted keys, compared above cmp_shift (K = uint32_t: narrow words, heads forced at bucket_starts -- see k_rerank_reduce)
//   sym    symbol in front of the suffix in slot a (first rerank: L itself); sym_from_key: taken from the key's low byte instead and
//          written to sym (the big list carries it there through the global sort)
//   suffix 0 keeps its group live until it is alone (its slot is the origin): zero_slot (first rerank: the word the initial sort's last
//          pass left, slot = SA position) or, when that is null, idx (the suffix in every slot)
// Like k_rerank_reduce: a thread owns RR_IPT consecutive slots and fetches them with 16-byte loads, a workgroup takes tiles_per_wg tiles
// with the next tile's loads in flight (one tile per workgroup with scalar loads: 1.22 ms for the 2^28 slots of the {A,C,G,T} block where
// k_rerank_reduce takes 0.32).
template <typename K>
struct LfSlice { K k[RR_IPT + 2]; uint64_t s8; uint32_t sprev; uint32_t zero_bits; };

template <typename K>
__global__ __launch_bounds__(RR_BLOCK) void k_lf_reduce(const K *__restrict__ keys, size_t count, int cmp_shift, uint8_t *__restrict__ sym,
                                                         int sym_from_key, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ zero_slot,
                                                         RerankAgg *__restrict__ agg, LfTile *__restrict__ tiles, uint8_t *__restrict__ flags_out,
                                                         const uint32_t *__restrict__ bucket_starts, uint32_t ntiles, uint32_t tiles_per_wg) {
    constexpr bool NARROW = sizeof(K) == 4;
    __shared__ uint32_t s_forced[NARROW ? 256 : 1];
    __shared__ uint32_t s_nforced;
    // two sets (tile parity): a set is written again two tiles later, behind the barriers of the tile between.  Per wave: has a head | OR of
    // the reasons behind its last head (or all) | OR in front of its first head (or all) | first head slot | end of last head slot
    __shared__ uint32_t s_w[2][RR_WAVES][5];
    __shared__ uint32_t s_red[2][3][RR_WAVES];
    __shared__ uint32_t s_closed[2];  // the slot behind the tile is a head: the tile's last group ends with the tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t t0 = blockIdx.x * tiles_per_wg;
    const uint32_t t1 = t0 + tiles_per_wg < ntiles ? t0 + tiles_per_wg : ntiles;
    if (NARROW) {  // (bucket_starts == nullptr: plain 32-bit keys -- the group ids of a list that is being filtered)
        if (tid == 0) s_nforced = 0;
        __syncthreads();
        const uint64_t s = bucket_starts ? bucket_starts[tid] : ~0ull;
        if (s >= static_cast<uint64_t>(t0) * RR_TILE && s <= static_cast<uint64_t>(t1) * RR_TILE) s_forced[atomicAdd(&s_nforced, 1u)] = static_cast<uint32_t>(s);
        __syncthreads();
    }
    const uint32_t zslot = zero_slot ? *zero_slot : 0xFFFFFFFFu;
    const bool aligned = (reinterpret_cast<uintptr_t>(keys) & 15) == 0 && (reinterpret_cast<uintptr_t>(sym) & 7) == 0 && (reinterpret_cast<uintptr_t>(idx) & 15) == 0;
    auto load_slice = [&](uint32_t tile, LfSlice<K> &r) {
        const size_t a0 = static_cast<size_t>(tile) * RR_TILE + static_cast<size_t>(tid) * RR_IPT;
        r.zero_bits = 0;
        if (a0 >= 1 && a0 + RR_IPT + 1 <= count && aligned) {
            constexpr int PER = 16 / sizeof(K);
            const uint4 *p = reinterpret_cast<const uint4 *>(keys + a0);
#pragma unroll
            for (int q = 0; q < RR_IPT / PER; ++q) {
                const uint4 v = p[q];
                if (NARROW) {
                    r.k[1 + 4 * q] = static_cast<K>(v.x); r.k[2 + 4 * q] = static_cast<K>(v.y); r.k[3 + 4 * q] = static_cast<K>(v.z); r.k[4 + 4 * q] = static_cast<K>(v.w);
                } else {
                    r.k[1 + 2 * q] = static_cast<K>((static_cast<uint64_t>(v.y) << 32) | v.x);
                    r.k[2 + 2 * q] = static_cast<K>((static_cast<uint64_t>(v.w) << 32) | v.z);
                }
            }
            r.k[0] = keys[a0 - 1];
            r.k[RR_IPT + 1] = keys[a0 + RR_IPT];
            if (sym_from_key) {
                r.s8 = 0;
#pragma unroll
                for (int jj = 0; jj < RR_IPT; ++jj) r.s8 |= (static_cast<uint64_t>(r.k[jj + 1]) & 0xFFull) << (8 * jj);
                r.sprev = static_cast<uint32_t>(r.k[0]) & 0xFFu;
            } else {
                r.s8 = *reinterpret_cast<const uint64_t *>(sym + a0);
                r.sprev = sym[a0 - 1];
            }
            if (!zero_slot) {
                const uint4 i0 = *reinterpret_cast<const uint4 *>(idx + a0), i1 = *reinterpret_cast<const uint4 *>(idx + a0 + 4);
                r.zero_bits = (i0.x == 0u ? 1u : 0u) | (i0.y == 0u ? 2u : 0u) | (i0.z == 0u ? 4u : 0u) | (i0.w == 0u ? 8u : 0u) | (i1.x == 0u ? 16u : 0u) |
                              (i1.y == 0u ? 32u : 0u) | (i1.z == 0u ? 64u : 0u) | (i1.w == 0u ? 128u : 0u);
            }
        } else {  // the list's ends (or an unaligned list)
            r.s8 = 0;
            r.sprev = 0;
#pragma unroll
            for (int jj = 0; jj < RR_IPT + 2; ++jj) {
                const size_t a = a0 + jj;  // slot a - 1
                const bool in = a >= 1 && a - 1 < count;
                r.k[jj] = in ? keys[a - 1] : K(0);
                if (jj <= RR_IPT) {
                    const uint32_t sv = !in ? 0u : sym_from_key ? (static_cast<uint32_t>(r.k[jj]) & 0xFFu) : sym[a - 1];
                    if (jj == 0) r.sprev = sv; else r.s8 |= static_cast<uint64_t>(sv) << (8 * (jj - 1));
                    if (jj >= 1 && in && !zero_slot && idx[a - 1] == 0u) r.zero_bits |= 1u << (jj - 1);
                }
            }
        }
        if (zero_slot) {
            const uint64_t rel = static_cast<uint64_t>(zslot) - a0;
            if (rel < RR_IPT) r.zero_bits = 1u << rel;
        }
    };
    if (t0 >= t1) return;
    LfSlice<K> cur, nxt;
    load_slice(t0, cur);
    for (uint32_t tile = t0; tile < t1; ++tile) {
        if (tile + 1 < t1) load_slice(tile + 1, nxt);
        const int set = tile & 1u;
        const size_t t_base = static_cast<size_t>(tile) * RR_TILE;
        const size_t a0 = t_base + static_cast<size_t>(tid) * RR_IPT;
        const bool last_tile = tile + 1 == ntiles;
        if (sym_from_key && a0 < count) {  // the symbols leave the keys: the apply phase (and the next round's list) read them from here
            if (a0 + RR_IPT <= count && aligned) *reinterpret_cast<uint64_t *>(sym + a0) = cur.s8;
            else for (int jj = 0; jj < RR_IPT && a0 + jj < count; ++jj) sym[a0 + jj] = static_cast<uint8_t>(cur.s8 >> (8 * jj));
        }
        uint32_t forced = 0;  // bit j: slot a0 + j - 1 starts a bucket
        if (NARROW) {
            const uint32_t nf = s_nforced;
            for (uint32_t i = 0; i < nf; ++i) {
                const uint64_t rel = static_cast<uint64_t>(s_forced[i]) + 1 - a0;
                if (rel < RR_IPT + 2) forced |= 1u << rel;
            }
        }
        // H: heads; a slot past the list counts as a head (the list's end closes the last group); NU: reasons to stay live
        uint32_t H = 0, NU = 0, valid = 0;
        bool next_head = true;  // is slot a0 + RR_IPT a head (or past the list)?
#pragma unroll
        for (int j = 0; j <= RR_IPT; ++j) {
            const size_t a = a0 + j;
            bool head = true;
            if (a < count) {
                const K prev = NARROW ? cur.k[j] : static_cast<K>(cur.k[j] >> cmp_shift), here = NARROW ? cur.k[j + 1] : static_cast<K>(cur.k[j + 1] >> cmp_shift);
                head = a == 0 || here != prev || ((forced >> (j + 1)) & 1u);
            }
            if (j == RR_IPT) { next_head = head; break; }
            if (a < count) valid |= 1u << j;
            if (head) H |= 1u << j;
            const uint32_t sy_here = static_cast<uint32_t>(cur.s8 >> (8 * j)) & 0xFFu, sy_prev = j ? static_cast<uint32_t>(cur.s8 >> (8 * (j - 1))) & 0xFFu : cur.sprev;
            if (a < count && ((!head && sy_here != sy_prev) || ((cur.zero_bits >> j) & 1u))) NU |= 1u << j;
        }
        // ---- which groups reach beyond this thread, and what do the rest of them hold?
        const bool hasH = H != 0;
        const int first = hasH ? __builtin_ctz(H) : RR_IPT, last = hasH ? 31 - __builtin_clz(H) : -1;
        const bool pre_or = (NU & ((1u << first) - 1u)) != 0;           // my slots in front of my first head
        const bool suf_or = hasH ? (NU >> last) != 0 : NU != 0;         // my slots from my last head on
        const uint64_t BH = __ballot(hasH), BA = __ballot(NU != 0), BS = __ballot(suf_or), BP = __ballot(pre_or);
        const uint64_t lt = lanemask_lt(lane), gt = lane == 63 ? 0ull : ~((2ull << lane) - 1ull);
        if (lane == 0) {
            const bool wh = BH != 0;
            const int pl = wh ? 63 - __builtin_clzll(BH) : 0, pf = wh ? __builtin_ctzll(BH) : 0;
            s_w[set][wave][0] = wh ? 1u : 0u;
            s_w[set][wave][1] = wh ? ((((BS >> pl) & 1ull) != 0) || (pl < 63 && (BA >> (pl + 1)) != 0) ? 1u : 0u) : (BA != 0 ? 1u : 0u);
            s_w[set][wave][2] = wh ? ((((BP >> pf) & 1ull) != 0) || (BA & lanemask_lt(pf)) != 0 ? 1u : 0u) : (BA != 0 ? 1u : 0u);
        }
        {   // slot numbers (inside the tile) of the wave's first head and of the end of its last head
            uint32_t mf = hasH ? static_cast<uint32_t>(tid * RR_IPT + first) : 0xFFFFFFFFu;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const uint32_t tf = __shfl_xor(mf, o, kWave);
                mf = mf < tf ? mf : tf;
            }
            if (lane == 0) s_w[set][wave][3] = mf;
        }
        if (tid == RR_BLOCK - 1) s_closed[set] = next_head ? 1u : 0u;
        __syncthreads();
        // forward: reasons between the head of the group that is open at my first slot and my first slot; was that head in this tile?
        bool fwd_val, head_before;
        {
            const uint64_t hb = BH & lt;
            if (hb) {
                const int p = 63 - __builtin_clzll(hb);
                fwd_val = ((BS >> p) & 1ull) != 0 || (BA & lt & ~((2ull << p) - 1ull)) != 0;
                head_before = true;
            } else {
                fwd_val = (BA & lt) != 0;
                head_before = false;
                for (int v = wave - 1; v >= 0 && !head_before; --v) {
                    fwd_val = fwd_val || s_w[set][v][1] != 0;
                    head_before = s_w[set][v][0] != 0;
                }
            }
        }
        // backward: reasons between my last slot and the end of the group that is open there; does that group end in this tile?
        bool bwd_val, head_after;
        {
            const uint64_t ha = BH & gt;
            if (ha) {
                const int q = __builtin_ctzll(ha);
                bwd_val = ((BP >> q) & 1ull) != 0 || (BA & gt & lanemask_lt(q)) != 0;
                head_after = true;
            } else {
                bwd_val = (BA & gt) != 0;
                head_after = false;
                for (int v = wave + 1; v < RR_WAVES && !head_after; ++v) {
                    bwd_val = bwd_val || s_w[set][v][2] != 0;
                    head_after = s_w[set][v][0] != 0;
                }
                if (!head_after && (last_tile || s_closed[set])) head_after = true;  // the list's end / a head right behind the tile closes the group
            }
        }
        // ---- flags of my slots
        uint64_t fl8 = 0;
        uint32_t ns = 0, nh = 0, lh = 0;
        {
            int j = 0;
            // (1) slots in front of my first head: the tail (or the middle) of a group that began before this thread
            if (first > 0) {
                const bool goes_on = !hasH;  // ... and continues behind it
                const bool reason = fwd_val || pre_or || (goes_on && bwd_val);
                const bool edge_f = !head_before, edge_l = goes_on && !head_after;
                const uint32_t f = edge_f || edge_l ? (edge_f ? LF_EDGE_FIRST : 0u) | (edge_l ? LF_EDGE_LAST : 0u) : (reason ? LF_SURV : 0u);
                for (; j < first; ++j) {
                    if (!((valid >> j) & 1u)) break;
                    fl8 |= static_cast<uint64_t>(f) << (8 * j);
                    ns += (f & LF_SURV) ? 1u : 0u;
                }
                j = first;
            }
            // (2) groups that begin at one of my heads
            while (j < RR_IPT && ((valid >> j) & 1u)) {  // j is a head
                const uint32_t rest = H >> (j + 1);
                const int nxt_h = rest ? j + 1 + __builtin_ctz(rest) : RR_IPT;  // my next head (RR_IPT: the group reaches my last slot)
                const bool open_end = nxt_h == RR_IPT && !next_head;           // ... and goes on in the next thread
                const bool reason = ((NU >> j) & ((1u << (nxt_h - j)) - 1u)) != 0 || (open_end && bwd_val);
                const bool single = nxt_h == j + 1 && (nxt_h < RR_IPT || next_head);
                const bool edge_l = open_end && !head_after;
                const uint32_t f = edge_l ? LF_EDGE_LAST : (reason && !single ? LF_SURV : 0u);
                lh = static_cast<uint32_t>(a0 + j) << 1;
                nh += (f & LF_SURV) ? 1u : 0u;
                for (int q = j; q < nxt_h; ++q) {
                    if (!((valid >> q) & 1u)) break;
                    fl8 |= static_cast<uint64_t>(f | (q == j ? LF_HEAD : 0u)) << (8 * q);
                    ns += (f & LF_SURV) ? 1u : 0u;
                }
                j = nxt_h;
            }
        }
        *reinterpret_cast<uint64_t *>(flags_out + a0) = fl8;  // whole tiles are stored: zero past `count`
        ns = wave_sum(ns);
        nh = wave_sum(nh);
        lh = wave_max(lh);
        if (lane == 0) { s_red[set][0][wave] = ns; s_red[set][1][wave] = nh; s_red[set][2][wave] = lh; }
        __syncthreads();
        if (tid == 0) {
            RerankAgg r{0, 0, 0, 0};
            for (int w = 0; w < RR_WAVES; ++w) {
                r.surv += s_red[set][0][w];
                r.heads += s_red[set][1][w];
                r.last_head = r.last_head > s_red[set][2][w] ? r.last_head : s_red[set][2][w];
            }
            agg[tile] = r;
            // the tile's own stretches of groups that cross its borders
            const uint32_t in_tile = static_cast<uint32_t>(count - t_base < static_cast<size_t>(RR_TILE) ? count - t_base : RR_TILE);
            LfTile t{};
            uint32_t first_head = 0xFFFFFFFFu;
            bool c_first = false, c_last = false, seen = false;
            for (int w = 0; w < RR_WAVES; ++w) {
                if (!seen) c_first = c_first || s_w[set][w][2] != 0;
                if (s_w[set][w][0]) {
                    if (!seen) first_head = s_w[set][w][3];
                    seen = true;
                    c_last = s_w[set][w][1] != 0;
                } else if (seen) {
                    c_last = c_last || s_w[set][w][1] != 0;
                }
            }
            const bool has_head = seen && first_head < in_tile;  // (slots past the list are heads in H: they are not heads of the tile)
            const uint32_t last_head_slot = has_head ? static_cast<uint32_t>(r.last_head >> 1) - static_cast<uint32_t>(t_base) : 0u;
            t.has_head = has_head ? 1 : 0;
            t.n_first = has_head ? first_head : in_tile;
            t.c_first = c_first ? 1 : 0;
            t.n_last = has_head && !last_tile && !s_closed[set] ? in_tile - last_head_slot : 0u;
            t.c_last = has_head ? (c_last ? 1 : 0) : t.c_first;
            tiles[tile] = t;
        }
        if (tile + 1 < t1) cur = nxt;
    }
}

// k_lf_straddle: one wave per tile with a head.  The group that begins at the tile's last head and runs over the tile's end: its other
// stretches lie in the following tiles (whole tiles without a head, then the slots in front of the next tile's first head).  Live when it
// has more than one member and a reason; then its slots and its head are added to the aggregates of the tiles they lie in.
__global__ __launch_bounds__(256) void k_lf_straddle(LfTile *__restrict__ tiles, RerankAgg *__restrict__ agg, uint32_t ntiles) {
    const uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= ntiles) return;
    const LfTile mine = tiles[t];
    if (!mine.has_head || mine.n_last == 0) return;
    bool reason = mine.c_last != 0;
    uint64_t size = mine.n_last;
    uint32_t end_tile = ntiles;  // the tile that holds the next head
    for (uint32_t base = t + 1; base < ntiles; base += 64) {
        const uint32_t v = base + lane;
        LfTile o{};
        o.has_head = 1;
        if (v < ntiles) o = tiles[v];
        const uint64_t B = __ballot(o.has_head != 0);
        const int stop = B ? __builtin_ctzll(B) : 64;
        const bool mine_in = v < ntiles && lane <= stop;
        reason = reason || __ballot(mine_in && o.c_first) != 0;
        uint32_t add = mine_in ? o.n_first : 0u;
        add = wave_sum(add);
        size += add;
        if (stop < 64) { end_tile = base + stop; break; }
    }
    const bool live = reason && size > 1;
    if (lane == 0) tiles[t].live_last = live ? 1 : 0;
    const uint32_t stop_tile = end_tile < ntiles ? end_tile : ntiles - 1;  // the last tile that holds a stretch of the group
    for (uint32_t v = t + 1 + lane; v <= stop_tile && v < ntiles; v += 64) {
        const LfTile o = tiles[v];
        if (v < end_tile) { tiles[v].live_first = live ? 1 : 0; tiles[v].live_last = live ? 1 : 0; }
        else tiles[v].live_first = live ? 1 : 0;
        if (live && o.n_first) atomicAdd(&agg[v].surv, o.n_first);
    }
    if (lane == 0 && live) {
        atomicAdd(&agg[t].surv, mine.n_last);
        atomicAdd(&agg[t].heads, 1u);
    }
}

// The depth a new group is known to -- every group of the list carries its own (gdepth[group]): the first rerank gives every group the initial
// sort's, a rerank of the big list (parent's depth) + (symbols the round sorted by), and a group whose parent was PERIODIC through its depth in a
// round that keyed such groups by the token of their stretch's end (k_lf_finish) is equal as far as the stretch goes, its break included: the next
// round goes on behind the break instead of walking through the stretch five symbols at a time (real text: indentation, rulers of '-' and '#').
struct LfDepthRule {
    uint32_t *gdepth_out;        // per new group (nullptr: the caller fills the table itself -- the first rerank, whose every group has the initial sort's depth)
    uint32_t uniform;            // keys == nullptr: every group gets this
    const uint64_t *keys;        // the sorted big list: (dense index of the parent group) above bit key_shift
    int key_shift;
    const uint32_t *bigdepth;    // per parent (dense index): its depth
    uint32_t add;                // symbols the round sorted by
    const uint32_t *next_break;  // != nullptr: the round keyed periodic parents by tokens (period, text length n)
    int period;
    uint32_t n;
    const uint8_t *bigper;       // ... per parent: was it periodic through its depth (k_lf_periodic_groups)
};
__device__ __forceinline__ uint32_t lf_new_depth(const LfDepthRule &dr, size_t slot, uint32_t suffix) {
    if (!dr.keys) return dr.uniform;
    const uint32_t bj = static_cast<uint32_t>(dr.keys[slot] >> dr.key_shift), parent = dr.bigdepth[bj];
    if (dr.next_break && dr.bigper[bj] && static_cast<uint64_t>(suffix) + parent <= dr.n)
        return dr.next_break[suffix] - suffix + static_cast<uint32_t>(dr.period) + 1u;  // equal through the break symbol (the token holds it)
    return parent + dr.add;
}

// k_lf_apply: the flags decide; finals of a later rerank write L at their SA positions (the first rerank's finals stand in L already),
// live slots are compacted into the active list (suffix, SA position, dense group id, symbol in front; gstart per group).
// pos_in == nullptr: slot a is SA position a (first rerank).
__global__ __launch_bounds__(RR_BLOCK) void k_lf_apply(const uint8_t *__restrict__ flags, const LfTile *__restrict__ tiles,
                                                        const uint32_t *__restrict__ idx, const uint32_t *__restrict__ pos_in,
                                                        const uint8_t *__restrict__ sym, size_t count, const RerankAgg *__restrict__ agg,
                                                        uint32_t *__restrict__ out_idx, uint32_t *__restrict__ out_pos,
                                                        uint32_t *__restrict__ out_gid, uint8_t *__restrict__ out_sym,
                                                        uint32_t *__restrict__ gstart, uint8_t *__restrict__ bwt, uint32_t *__restrict__ origin, LfDepthRule dr) {
    __shared__ __attribute__((aligned(16))) uint32_t s_out[3 * RR_TILE];  // compacted idx | pos | gid
    __shared__ __attribute__((aligned(8))) uint8_t s_osym[RR_TILE];
    __shared__ uint32_t s_tmp[RR_WAVES + 1];
    const int tid = threadIdx.x;
    const uint32_t tile = blockIdx.x;
    const size_t a0 = static_cast<size_t>(tile) * RR_TILE + static_cast<size_t>(tid) * RR_IPT;
    const LfTile tl = tiles[tile];
    uint64_t fl = *reinterpret_cast<const uint64_t *>(flags + a0);
    {   // the groups that cross the tile's borders: k_lf_straddle decided
        constexpr uint64_t ONES = 0x0101010101010101ull;
        const uint64_t ef = (fl >> 3) & ONES, el = (fl >> 4) & ONES;
        const uint64_t live = (tl.live_first ? ef : 0ull) | (tl.live_last ? el : 0ull);
        fl = (fl & ~(ONES * (LF_EDGE_FIRST | LF_EDGE_LAST))) | (live << 1);
    }
    const RerankAgg base = agg[tile];
    // a tile without any live slot and (first rerank) nothing to write: done
    const RerankAgg nextb = tile + 1 < gridDim.x ? agg[tile + 1] : RerankAgg{0xFFFFFFFFu, 0, 0, 0};
    if (!pos_in && nextb.surv == base.surv && tile + 1 < gridDim.x) return;
    uint32_t ns = 0, nh = 0;
#pragma unroll
    for (int j = 0; j < RR_IPT; ++j) {
        const uint32_t f = static_cast<uint32_t>(fl >> (8 * j)) & 0xFFu;
        ns += (f & LF_SURV) ? 1u : 0u;
        nh += ((f & LF_HEAD) && (f & LF_SURV)) ? 1u : 0u;
    }
    uint32_t block_surv;
    const uint32_t both = block_excl_sum<RR_WAVES>(ns | (nh << 16), s_tmp, &block_surv);
    block_surv &= 0xFFFFu;
    uint32_t es = both & 0xFFFFu;
    uint32_t eh = base.heads + (both >> 16);
    uint32_t *s_oidx = s_out, *s_opos = s_out + RR_TILE, *s_ogid = s_out + 2 * RR_TILE;
    if (ns || pos_in) {
        // the thread's eight slots with 16-byte loads (a scalar load per live slot: lanes 32 bytes apart, a quarter of every line used)
        uint32_t my_idx[RR_IPT], my_pos[RR_IPT];
        uint64_t sym8 = 0;
        if (a0 + RR_IPT <= count && (reinterpret_cast<uintptr_t>(idx) & 15) == 0 && (reinterpret_cast<uintptr_t>(sym) & 7) == 0 &&
            (reinterpret_cast<uintptr_t>(pos_in) & 15) == 0) {
            const uint4 i0 = *reinterpret_cast<const uint4 *>(idx + a0), i1 = *reinterpret_cast<const uint4 *>(idx + a0 + 4);
            my_idx[0] = i0.x; my_idx[1] = i0.y; my_idx[2] = i0.z; my_idx[3] = i0.w; my_idx[4] = i1.x; my_idx[5] = i1.y; my_idx[6] = i1.z; my_idx[7] = i1.w;
            sym8 = *reinterpret_cast<const uint64_t *>(sym + a0);
            if (pos_in) {
                const uint4 p0 = *reinterpret_cast<const uint4 *>(pos_in + a0), p1 = *reinterpret_cast<const uint4 *>(pos_in + a0 + 4);
                my_pos[0] = p0.x; my_pos[1] = p0.y; my_pos[2] = p0.z; my_pos[3] = p0.w; my_pos[4] = p1.x; my_pos[5] = p1.y; my_pos[6] = p1.z; my_pos[7] = p1.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < RR_IPT; ++j) {
                const size_t a = a0 + j;
                my_idx[j] = a < count ? idx[a] : 0u;
                my_pos[j] = a < count && pos_in ? pos_in[a] : 0u;
                if (a < count) sym8 |= static_cast<uint64_t>(sym[a]) << (8 * j);
            }
        }
#pragma unroll
        for (int j = 0; j < RR_IPT; ++j) {
            const size_t a = a0 + j;
            if (a >= count) break;
            const uint32_t f = static_cast<uint32_t>(fl >> (8 * j)) & 0xFFu;
            const uint8_t sy = static_cast<uint8_t>(sym8 >> (8 * j));
            if (f & LF_SURV) {
                if (f & LF_HEAD) { gstart[eh] = base.surv + es; if (dr.gdepth_out) dr.gdepth_out[eh] = lf_new_depth(dr, a, my_idx[j]); ++eh; }
                s_oidx[es] = my_idx[j];
                s_opos[es] = pos_in ? my_pos[j] : static_cast<uint32_t>(a);
                s_ogid[es] = eh - 1;
                s_osym[es] = sy;
                ++es;
            } else if (pos_in) {  // final: its symbol goes to its place in L (the order inside a group with one symbol in front is irrelevant)
                bwt[my_pos[j]] = sy;
                if (my_idx[j] == 0u) *origin = my_pos[j];
            }
        }
    }
    __syncthreads();
    for (uint32_t o = tid; o < block_surv; o += RR_BLOCK) {
        out_idx[base.surv + o] = s_oidx[o];
        out_pos[base.surv + o] = s_opos[o];
        out_gid[base.surv + o] = s_ogid[o];
        out_sym[base.surv + o] = s_osym[o];
    }
}

// rerank of the L-first path: keys sorted (the first rerank: the initial sort's keys, possibly narrow; later: the big list's keys, symbol
// in the low byte) -> active list of the live groups.  The counts come back through classify_and_read like after rerank().
int lf_rerank(dk_ctx *ctx, const uint64_t *keys, int cmp_shift, const uint32_t *narrow_starts, uint8_t *sym, int sym_from_key, const uint32_t *idx,
              const uint32_t *zero_slot, const uint32_t *pos_in, size_t count, uint32_t *out_idx, uint32_t *out_pos, uint32_t *out_gid, uint8_t *out_sym,
              uint32_t *gstart, uint8_t *bwt, uint32_t *origin, const LfDepthRule &dr, bool keys32 = false, uint32_t reduce_tiles_per_wg = 0) {
    const size_t ntiles = div_up(count, RR_TILE);
    const size_t mark = ctx->ws_mark();
    RerankAgg *agg = ctx->ws_alloc<RerankAgg>(ntiles);
    LfTile *tiles = ctx->ws_alloc<LfTile>(ntiles);
    uint8_t *flags = ctx->ws_alloc<uint8_t>(ntiles * RR_TILE);
    if (!agg || !tiles || !flags) return DK_E_NOMEM;
    hipStream_t st = ctx->stream;
    {
        LaunchScope ls(ctx, K_RERANK_REDUCE, ((narrow_starts || keys32 ? 4.0 : 8.0) + (zero_slot ? 0.0 : 4.0) + 1.0 + 1.0) * count);
        // (reduce_tiles_per_wg: a launch shape a test may set, dk_dbg_dev_lf_rerank -- the multi-tile stretch starts at 2^25 slots; the outputs do not depend on it)
        const uint32_t per_wg = reduce_tiles_per_wg ? reduce_tiles_per_wg : static_cast<uint32_t>(std::min<size_t>(std::max<size_t>(ntiles / 16384, 1), 64));
        const dim3 grid(static_cast<unsigned>(div_up(ntiles, per_wg))), block(RR_BLOCK);
        if (narrow_starts || keys32)
            k_lf_reduce<uint32_t><<<grid, block, 0, st>>>(reinterpret_cast<const uint32_t *>(keys), count, 0, sym, 0, idx, zero_slot, agg, tiles, flags, narrow_starts,
                                                          static_cast<uint32_t>(ntiles), per_wg);
        else
            k_lf_reduce<uint64_t><<<grid, block, 0, st>>>(keys, count, cmp_shift, sym, sym_from_key, idx, zero_slot, agg, tiles, flags, nullptr,
                                                          static_cast<uint32_t>(ntiles), per_wg);
    }
    {
        LaunchScope ls(ctx, K_RERANK_SCAN, 64.0 * ntiles);
        k_lf_straddle<<<dim3(div_up(ntiles, 4)), dim3(256), 0, st>>>(tiles, agg, static_cast<uint32_t>(ntiles));
        if (ntiles <= 4 * RSC_CHUNK) {
            k_rerank_scan<<<dim3(1), dim3(1024), 0, st>>>(agg, ntiles, &ctx->d_mail->cls.rounds, gstart);
        } else {
            const size_t nchunks = div_up(ntiles, RSC_CHUNK);
            RerankAgg *chunk = ctx->ws_alloc<RerankAgg>(nchunks);
            if (!chunk) return DK_E_NOMEM;
            k_rerank_scan_a<<<dim3(nchunks), dim3(256), 0, st>>>(agg, ntiles, chunk);
            k_rerank_scan<<<dim3(1), dim3(1024), 0, st>>>(chunk, nchunks, &ctx->d_mail->cls.rounds, gstart);
            k_rerank_scan_c<<<dim3(nchunks), dim3(256), 0, st>>>(agg, ntiles, chunk);
        }
    }
    {
        LaunchScope ls(ctx, K_RERANK_APPLY, (pos_in ? 10.0 + 5.0 : 6.0 + 13.0) * count);
        k_lf_apply<<<dim3(ntiles), dim3(RR_BLOCK), 0, st>>>(flags, tiles, idx, pos_in, sym, count, agg, out_idx, out_pos, out_gid, out_sym, gstart, bwt, origin, dr);
    }
    DK_HIP(ctx, hipGetLastError());
    ctx->ws_release(mark);
    return DK_OK;
}

// ---- k_lf_finish: the live groups of at most LS_MAX members, to their end inside LDS ---------------------------------------------------------
// k_lf_finish<TILE, CAP, BLOCK>: a workgroup of BLOCK threads owns the groups whose head lies in its TILE list slots and refines those of up to CAP members
constexpr int LFS_BLOCK = 256;
constexpr int LFS_TILE = 512;               // (1e8 text block, k_lf_finish: 2048 slots 1.60 ms, 1024 1.14, 512 1.07)
constexpr int LFS_CAP = 256;                // largest group the rounds' instance refines (bigger ones go the global way): with 1024 the kernel held 64 KiB of
                                            // LDS, two workgroups per CU, and a step costs the latency of a random text gather -- 1e8 text 8.3 against 7.8 ms
// (Round 5, measured and removed: an instance <2048, 2048, 1024> for the rounds of a short big list -- the last eight of fourteen rounds on 50 MB of
//  real text are a dozen launches each for a few thousand slots.  Six rounds less, and slower: 12.2 against 10.9 ms; a member's place is found by
//  counting over its group, 2048 x 2048 per step.  profiles/NOTES.md)
constexpr int LF_SYMS = 7;                  // bytes of text per step (the key's low byte says how many of them exist)
constexpr int LF_STUCK = 2;                 // steps without a split after which a group leaves for the deep list (a long repeat) ...
constexpr int LF_STEPS = 6;                 // ... and steps after which whatever is still live does (DESIGN.md 4.1.10: a workgroup that goes on for the
                                            // sake of a few slowly splitting groups is a latency tail of the whole round -- measured on 50 MB of real text)
constexpr int LF_SHORT_STEPS = 1;           // ... one step where the round's list is short (at most LF_SHORT_SLOTS slots): such a launch is six steps of latency for a few
constexpr size_t LF_SHORT_SLOTS = 4u << 20; // hundred workgroups, and what one step does not split the pass over the arena orders anyway (50 MB of real text: 10.4 -> 9.7 ms;
                                            // lists up to 1 M 9.9, 2 M 9.8, 8 M 9.9, 16 M 10.2, all of them 11.25; the 1e8 text and word-like blocks do not care)
// A group on the deep list: members equal in their first `depth` symbols.  flags 0: the members stand in the ARENA at [start, start + size) -- copies
// (suffix, SA position, symbol in front) made by k_lf_finish when the group left its LDS; all such groups are ordered together when the rounds are over
// (k_lf_deep_wave: a wave per group of up to 64 members; k_lf_deep: a workgroup per bigger group).  LD_HANDED: a (sub)group the wave kernel gave up
// on (a common extension beyond what a lane measures): the workgroup kernel takes it.  LD_LIST: the members stand in the round's own list at slots
// [start, start + size) (groups of up to LS_MAX members that the big list let go after a stalled round): ordered before the round rewrites the list.
struct alignas(16) LfDeepGroup { uint32_t start, size, depth, flags; };
constexpr uint32_t LD_HANDED = 1, LD_LIST = 2, LD_DONE = 4;  // LD_DONE: a listed group that k_lf_medium has taken (what it left over is listed again, in the arena)
struct LfArena { uint32_t *idx, *pos; uint8_t *sym; uint32_t *used; uint32_t cap; };

// Key of the LF_SYMS bytes behind position p: the bytes big-endian above a low byte that counts how many of them exist (1 .. LF_SYMS), so
// that a suffix that ends inside the window sorts in front of one that goes on with zero bytes; 0 when the suffix ended before p (it is a
// proper prefix of every other member of its group: smallest).
// tokens of a round (next_break == nullptr: none): a member of a big group that follows the block's dominant short period through its group's depth
// -- the suffixes inside a run of one byte value, a stretch of one repeated word -- does not split on the next bytes of text, but where its stretch
// ends orders it at once (the period round of the suffix-array path, k_period_* in suffix_array.hip): its key takes (direction of the break, length
// to the break or its complement, the symbol at the break) in place of the text.  All members of a group agree on the test (it reads their first
// `depth` symbols only), so tokens meet tokens and text meets text.  next_break[i] = min { j >= i : j + period >= n or T[j] != T[j + period] }.
// bigper[dense index of a big group] = its members follow the period through the group's depth (all of them do or none: k_lf_periodic_groups asks the
// first one) -- so that only the members of such groups pay for the gather of their next break
struct LfTokens { const uint32_t *next_break; int period; int ebits; const uint8_t *bigper; };
__global__ __launch_bounds__(256) void k_lf_periodic_groups(const uint32_t *__restrict__ gstart, const uint32_t *__restrict__ gdepth, const uint32_t *__restrict__ act_idx,
                                                             const uint32_t *__restrict__ bigidx, size_t groups, uint32_t above, const uint32_t *__restrict__ next_break,
                                                             int period, uint32_t n, uint8_t *__restrict__ bigper) {
    const size_t g = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= groups) return;
    const uint32_t gs = gstart[g];
    if (gstart[g + 1] - gs <= above) return;
    const uint32_t x = act_idx[gs], h = gdepth[g];
    bigper[bigidx[g]] = static_cast<uint64_t>(x) + h <= n && next_break[x] - x + static_cast<uint32_t>(period) >= h ? 1 : 0;
}
__device__ __forceinline__ uint64_t lf_key(const uint8_t *__restrict__ t, size_t n, size_t p) {
    if (p >= n) return 0;
    const size_t avail = n - p;
    const uint64_t raw = text_key_raw(t, n, p);  // eight bytes, zero padded
    return (raw & ~0xFFull) | (avail >= static_cast<size_t>(LF_SYMS) ? static_cast<uint64_t>(LF_SYMS) : static_cast<uint64_t>(avail));
}

template <int LF_TILE, int LF_CAP, int LF_BLOCK>
__global__ __launch_bounds__(LF_BLOCK) void k_lf_finish(uint32_t *__restrict__ act_idx, const uint32_t *__restrict__ act_pos,
                                                         const uint32_t *__restrict__ act_gid, uint8_t *__restrict__ act_sym,
                                                         const uint32_t *__restrict__ gstart, const uint32_t *__restrict__ bigidx,
                                                         const uint32_t *__restrict__ bigoff, size_t count, const uint8_t *__restrict__ text,
                                                         uint32_t n, const uint32_t *__restrict__ gdepth, uint32_t *__restrict__ bigdepth, LfTokens tok, int kb,
                                                         uint32_t ls_max, uint32_t big_min, uint64_t *__restrict__ bkeys,
                                                         uint32_t *__restrict__ bidx,
                                                         uint32_t *__restrict__ bpos, uint8_t *__restrict__ bwt, uint32_t *__restrict__ origin,
                                                         LfDeepGroup *__restrict__ deep, uint32_t *__restrict__ deep_count, uint32_t deep_cap, LfArena arena,
                                                         uint32_t *__restrict__ fallback, int max_steps, int stuck_steps) {
    constexpr int LF_SPAN = LF_TILE + LF_CAP;   // slots it may touch: a group that begins in the tile ends at most LF_CAP - 1 slots behind it
    constexpr int LF_SPT = LF_SPAN / LF_BLOCK;  // slots per thread
    static_assert(LF_SPAN % LF_BLOCK == 0 && LF_SPAN < 65536 && LF_SPT <= 32, "16-bit group starts and sizes; one bit per slot of a thread");
    __shared__ uint64_t s_key[LF_SPAN];
    __shared__ uint32_t s_idx[LF_SPAN];
    __shared__ uint32_t s_base[LF_SPAN];  // depth of the slot's group when the round began (members move inside their group's slots only: it stays)
    __shared__ uint32_t s_aoff[LF_SPAN];  // a group that leaves for the deep list, at its head's slot: its number | its members' offset << 16 among this step's leavers
    __shared__ uint32_t s_leave[4];       // groups, members leaving in this step; then the workgroup's base in the list and in the arena
    __shared__ uint16_t s_gs[LF_SPAN], s_sz[LF_SPAN], s_dep[LF_SPAN];  // group start (relative to the tile) and size (0: not mine / done), depth behind h
    __shared__ uint8_t s_sym[LF_SPAN], s_nu[LF_SPAN], s_stuck[LF_SPAN];
    const int tid = threadIdx.x;
    const size_t b0 = static_cast<size_t>(blockIdx.x) * LF_TILE;
    uint32_t my_pos[LF_SPT];
    int alive = 0;
    if (tid < 2) s_leave[tid] = 0;
#pragma unroll
    for (int k = 0; k < LF_SPT; ++k) {
        const int s = k * LF_BLOCK + tid;
        const size_t a = b0 + s;
        s_sz[s] = 0;
        my_pos[k] = 0;
        if (a >= count) continue;
        const uint32_t g = act_gid[a];
        const uint32_t gs = gstart[g], size = gstart[g + 1] - gs, h = gdepth[g];
        if (size > ls_max && size <= big_min) {
            // a group too big for this kernel and not on the big list (the big groups have stopped splitting on text: runs of one byte,
            // periodic stretches): k_lf_deep orders it by what its members have in common with one of them
            if (s < LF_TILE && static_cast<uint32_t>(a) == gs) {
                const uint32_t at = atomicAdd(deep_count, 1u);
                if (at < deep_cap) deep[at] = LfDeepGroup{gs, size, h, LD_LIST};
                else *fallback = 1u;
            }
            continue;
        }
        if (size > ls_max) {
            if (s < LF_TILE) {  // a member of a big group: to the big list, keyed (dense index of the group) | (the next kb bits of text) | symbol in front
                const uint32_t suffix = act_idx[a];
                const uint32_t bj = bigidx[g];
                const uint32_t bo = bigoff[bj] + (static_cast<uint32_t>(a) - gs);
                if (static_cast<uint32_t>(a) == gs) bigdepth[bj] = h;
                uint64_t payload = text_key_raw(text, n, static_cast<size_t>(suffix) + h) >> (64 - kb);
                if (tok.next_break && tok.bigper[bj] && static_cast<uint64_t>(suffix) + h <= n) {  // (a suffix that ends before the depth keeps the text key: zero, it sorts first)
                    const uint32_t b = tok.next_break[suffix], e = b - suffix;  // T[suffix + k] == T[suffix + k + period] for k < e
                    {
                        const size_t brk = static_cast<size_t>(b) + tok.period;  // the first symbol that does not follow the period (<= n)
                        const bool down = brk >= n || text[brk] < text[b];
                        const uint64_t ev = down ? e : ((1u << tok.ebits) - 1u - e);
                        const uint64_t tk = (static_cast<uint64_t>(down ? 0u : 1u) << (tok.ebits + 8)) | (ev << 8) | (brk < n ? text[brk] : 0u);  // 1 + ebits + 8 bits
                        payload = tk << (kb - (1 + tok.ebits + 8));  // (the host hands tokens to a round only when they fit)
                    }
                }
                bkeys[bo] = ((((static_cast<uint64_t>(bj) << kb) | payload) << 8) | act_sym[a]);
                bidx[bo] = suffix;
                bpos[bo] = act_pos[a];
            }
            continue;
        }
        if (gs < b0 || gs >= b0 + LF_TILE) continue;  // the tile of the group's head owns the group
        s_idx[s] = act_idx[a];
        s_sym[s] = act_sym[a];
        s_gs[s] = static_cast<uint16_t>(gs - b0);
        s_sz[s] = static_cast<uint16_t>(size);
        s_base[s] = h;
        s_dep[s] = 0;
        s_stuck[s] = 0;
        my_pos[k] = act_pos[a];
        alive = 1;
    }
    for (int step = 1; __syncthreads_or(alive); ++step) {
        // (A) keys of the step
#pragma unroll
        for (int k = 0; k < LF_SPT; ++k) {
            const int s = k * LF_BLOCK + tid;
            s_nu[s] = 0;
            if (s_sz[s]) s_key[s] = lf_key(text, n, static_cast<size_t>(s_idx[s]) + s_base[s] + s_dep[s]);
        }
        __syncthreads();
        // (B) every member's place inside its group
        uint32_t m_idx[LF_SPT];
        uint16_t m_dest[LF_SPT], m_gs[LF_SPT], m_sz[LF_SPT], m_dep[LF_SPT];
        uint8_t m_sym[LF_SPT], m_stuck[LF_SPT];
#pragma unroll
        for (int k = 0; k < LF_SPT; ++k) {
            const int s = k * LF_BLOCK + tid;
            m_sz[k] = 0;
            const uint32_t sz = s_sz[s];
            if (!sz) continue;
            const uint32_t gs = s_gs[s];
            const uint64_t mine = s_key[s];
            const uint32_t me = s_idx[s];
            uint32_t less = 0, eq = 0, eqb = 0;
            if (mine != 0) {
                for (uint32_t b = gs; b < gs + sz; ++b) {
                    const uint64_t v = s_key[b];
                    less += v < mine;
                    eq += v == mine;
                    eqb += (v == mine) && b < static_cast<uint32_t>(s);
                }
            } else {  // my suffix ended in front of the window: so did every other member with key 0, and the shorter one is smaller
                eq = 1;
                for (uint32_t b = gs; b < gs + sz; ++b) less += s_key[b] == 0 && s_idx[b] > me;
            }
            m_idx[k] = me;
            m_sym[k] = s_sym[s];
            m_dest[k] = static_cast<uint16_t>(gs + less + eqb);
            m_gs[k] = static_cast<uint16_t>(gs + less);
            m_sz[k] = static_cast<uint16_t>(eq);
            m_dep[k] = static_cast<uint16_t>(s_dep[s] + LF_SYMS);
            m_stuck[k] = eq == sz ? static_cast<uint8_t>(s_stuck[s] + 1) : uint8_t(0);
        }
        __syncthreads();
        // (C) move
#pragma unroll
        for (int k = 0; k < LF_SPT; ++k) {
            if (!m_sz[k]) continue;
            const int d = m_dest[k];
            s_idx[d] = m_idx[k];
            s_sym[d] = m_sym[k];
            s_gs[d] = m_gs[k];
            s_sz[d] = m_sz[k];
            s_dep[d] = m_dep[k];
            s_stuck[d] = m_stuck[k];
        }
        __syncthreads();
        // (D) does a new group hold two symbols in front, or suffix 0?
#pragma unroll
        for (int k = 0; k < LF_SPT; ++k) {
            const int s = k * LF_BLOCK + tid;
            if (!s_sz[s]) continue;
            const int g0 = s_gs[s];
            if (s_sym[s] != s_sym[g0] || s_idx[s] == 0u) s_nu[g0] = 1;
        }
        __syncthreads();
        // (E) groups that are done write L; groups that do not move, and whatever is still live after max_steps steps, leave for the deep list --
        //     their members are copied to the arena (the list they stand in is rewritten by the round's rerank; the deep groups of ALL rounds are
        //     ordered together at the end); the rest goes on
        alive = 0;
        uint32_t leaving = 0;  // bit k: my slot k leaves for the arena
#pragma unroll
        for (int k = 0; k < LF_SPT; ++k) {
            const int s = k * LF_BLOCK + tid;
            const uint32_t sz = s_sz[s];
            if (!sz) continue;
            const int g0 = s_gs[s];
            if (sz == 1 || !s_nu[g0]) {
                bwt[my_pos[k]] = s_sym[s];
                if (s_idx[s] == 0u) *origin = my_pos[k];
                s_sz[s] = 0;
            } else if (static_cast<int>(s_stuck[s]) >= stuck_steps || step >= max_steps) {
                leaving |= 1u << k;
                // (places inside the workgroup's share of the list and of the arena: LDS counters; ONE pair of global atomics per workgroup and
                //  step below -- a pair per group was 0.7 ms of round 0 on 50 MB of real text, half a million groups on two addresses)
                if (s == g0) s_aoff[g0] = atomicAdd(&s_leave[0], 1u) | (atomicAdd(&s_leave[1], sz) << 16);
            } else {
                alive = 1;
            }
        }
        if (__syncthreads_or(leaving != 0u)) {
            if (tid == 0) {
                const uint32_t groups = s_leave[0], members = s_leave[1];
                const uint32_t at = atomicAdd(deep_count, groups), off = atomicAdd(arena.used, members);
                const bool fits = off + members <= arena.cap && at + groups <= deep_cap;  // (every suffix leaves at most once: the arena holds n members)
                if (!fits) *fallback = 1u;
                s_leave[2] = fits ? at : 0xFFFFFFFFu;
                s_leave[3] = off;
                s_leave[0] = s_leave[1] = 0;
            }
            __syncthreads();
            const uint32_t at0 = s_leave[2], off0 = s_leave[3];
#pragma unroll
            for (int k = 0; k < LF_SPT; ++k) {
                if (!((leaving >> k) & 1u)) continue;
                const int s = k * LF_BLOCK + tid, g0 = s_gs[s];
                if (at0 != 0xFFFFFFFFu) {
                    const uint32_t off = off0 + (s_aoff[g0] >> 16);
                    if (s == g0) deep[at0 + (s_aoff[g0] & 0xFFFFu)] = LfDeepGroup{off, s_sz[s], s_base[s] + s_dep[s], 0u};
                    const uint32_t at = off + static_cast<uint32_t>(s - g0);
                    arena.idx[at] = s_idx[s];
                    arena.sym[at] = s_sym[s];
                    arena.pos[at] = my_pos[k];  // the SA position of the slot: where the member that ends up (s - g0)-th in its group belongs
                }
                s_sz[s] = 0;
            }
        }
    }
}

// ---- the deep list: groups that stopped splitting (or were handed on for being slow) ------------------------------------------------------------
// The members of a listed group are equal in their first `depth` symbols: the first suffixes of long repeats and their copies, the suffixes inside a
// run of one byte or a periodic stretch, boilerplate.  They are ordered by what every member has in common with the FIRST member of its (sub)group,
// the pivot: how many bytes (LCE), and which of the two is smaller where they part (the end of the text counts: a proper prefix is smaller).  A member
// that parts from the pivot after c bytes parts there from every member that stays with the pivot longer, so the members SMALLER than the pivot come
// first, by c ascending, then the pivot and whoever stays with it for all that was measured, then the LARGER ones by c descending; members of one
// side with one c are equal in depth + c symbols and are the next subgroups.  One level settles a run (all c differ).  Subgroups that are singletons
// or have one symbol in front (and not suffix 0, whose place is the origin) write L and are done.
//   k_lf_deep_wave    a wave per group of up to 64 members, registers and cross-lane moves only
//   k_lf_deep_block   a workgroup per bigger group: ALL live subgroups of the group advance together, level by level (round 4's kernel took one
//                     subgroup at a time from a stack: 1.2 ms for the 4000 bigger groups of 50 MB of real text, each as long as its chain of levels)
//   k_lf_lce          a common extension beyond LD_MAX_STEPS KiB (copies of whole files): the whole grid measures it, the group comes back with the answers
constexpr int LD_MAX_STEPS = 64;  // wave steps of 1 KiB per member and level
struct LfGiantOut { LfDeepGroup *list; uint32_t *count; uint32_t cap; uint32_t *idx, *pos; uint8_t *sym; uint32_t *used; uint32_t arena_cap; };
constexpr int LDM_LIST = 0, LDM_ARENA = 1, LDM_ALL = 2;
constexpr uint32_t LW_MAX = 64;  // members of a group a wave orders by itself (k_lf_deep_wave)
constexpr uint32_t LD_TIE = 4;   // bytes from where a member parts from its pivot on that go into its key (the common extensions stay below 2^30)

// bytes the suffixes at x and y (x != y) have in common from there on, found by one wave: 16 bytes per lane and step = 1 KiB per step
__device__ __forceinline__ uint32_t wave_common_extension(const uint8_t *__restrict__ t, size_t n, size_t x, size_t y, int lane, bool *gave_up) {
    typedef uint64_t __attribute__((aligned(1))) unaligned_u64;
    typedef const unaligned_u64 __attribute__((address_space(1))) *gptr8;
    const size_t room = n - (x > y ? x : y);  // bytes the shorter of the two still has
    size_t off = 0;
    for (int step = 0; step < LD_MAX_STEPS; ++step, off += 1024) {
        const size_t o = off + 16 * static_cast<size_t>(lane);
        uint32_t mis = 16;  // first differing byte of my 16, 16 = none
        if (o + 16 <= room) {
            const uint64_t lo = *(gptr8)(t + x + o) ^ *(gptr8)(t + y + o), hi = *(gptr8)(t + x + o + 8) ^ *(gptr8)(t + y + o + 8);
            if (lo | hi) mis = lo ? static_cast<uint32_t>(__builtin_ctzll(lo)) >> 3 : 8u + (static_cast<uint32_t>(__builtin_ctzll(hi)) >> 3);
        } else {
            for (uint32_t j = 0; j < 16; ++j) {
                if (o + j >= room || t[x + o + j] != t[y + o + j]) { mis = j; break; }  // the end of the shorter suffix counts as a difference
            }
        }
        const uint64_t B = __ballot(mis < 16);
        if (B) {
            const int l = __builtin_ctzll(B);
            return static_cast<uint32_t>(off) + 16u * static_cast<uint32_t>(l) + static_cast<uint32_t>(__shfl(static_cast<int>(mis), l, kWave));
        }
    }
    *gave_up = true;
    return 0;
}

// mode LDM_LIST: the entries [begin, total) flagged LD_LIST (members in the round's list: act_* are the list's arrays); LDM_ARENA: the arena's entries
// of more than LW_MAX members, and those k_lf_deep_wave handed on (act_* are the arena's arrays); LDM_ALL: every entry.  Only groups of more than
// size_lo and at most CAP members are taken (one launch per size class).
// lce_known != nullptr (groups back from the grid-wide measure): what every member has in common with the group's first one, for the first level.
constexpr uint32_t LB_LANE_CAP = 256;  // bytes a lane compares by itself before a wave takes over (1 KiB per step)
constexpr uint64_t LB_PIVOT = 1ull << 62, LB_LONG = 3ull << 62;
template <int CAP, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_lf_deep_block(const uint32_t *__restrict__ act_idx, const uint32_t *__restrict__ act_pos, const uint8_t *__restrict__ act_sym,
                                                          const LfDeepGroup *__restrict__ deep, const uint32_t *__restrict__ end_ptr, uint32_t begin, uint32_t end,
                                                          uint32_t deep_cap, const uint8_t *__restrict__ text, uint32_t n, uint8_t *__restrict__ bwt, uint32_t *__restrict__ origin,
                                                          uint32_t *__restrict__ fallback, const uint32_t *__restrict__ lce_known, LfGiantOut giant, int mode, uint32_t size_lo) {
    typedef uint64_t __attribute__((aligned(1))) unaligned_u64;
    typedef const unaligned_u64 __attribute__((address_space(1))) *gptr8;
    typedef uint32_t __attribute__((aligned(1))) unaligned_u32;
    typedef const unaligned_u32 __attribute__((address_space(1))) *gptr4;
    constexpr int MPT = CAP / BLOCK, WAVES = BLOCK / 64;  // members per thread
    static_assert(CAP % BLOCK == 0 && CAP <= 65535, "16-bit subgroup starts and sizes");
    __shared__ uint64_t s_key[CAP];
    __shared__ uint32_t s_idx[CAP], s_grp[CAP], s_dep[CAP];  // s_grp: the slot's subgroup, start | size << 16 (size 0: done)
    __shared__ uint8_t s_sym[CAP], s_nu[CAP];
    __shared__ uint32_t s_long;  // a member of this level went beyond what a lane measures
    __shared__ uint32_t s_near;  // a member of this level ends within LD_TIE bytes of where it parts from its pivot: no tie bytes in this level's keys
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t total = end_ptr ? *end_ptr : end;  // the entries [begin, total) (end_ptr: a list whose length only the device knows)
    if (total > deep_cap) { if (blockIdx.x == 0 && tid == 0) *fallback = 1u; return; }
    for (uint32_t gi = begin + blockIdx.x; gi < total; gi += gridDim.x) {
        const LfDeepGroup grp = deep[gi];
        if (grp.size > static_cast<uint32_t>(CAP)) continue;
        if (mode == LDM_LIST && !(grp.flags & LD_LIST)) continue;
        if (mode == LDM_ARENA && (grp.flags & (LD_LIST | LD_DONE))) continue;
        if (mode == LDM_ARENA && (grp.flags & LD_HANDED) ? size_lo != 0u : (grp.size <= size_lo || (mode == LDM_ARENA && grp.size <= LW_MAX))) continue;
        __syncthreads();  // (the arrays of the group before this one are no longer read)
        for (uint32_t i = tid; i < grp.size; i += BLOCK) {
            s_idx[i] = act_idx[grp.start + i];
            s_sym[i] = act_sym[grp.start + i];
            s_grp[i] = grp.size << 16;
            s_dep[i] = grp.depth;
        }
        bool first_level = true;
        for (int level = 0;; ++level, first_level = false) {
            if (tid == 0) { s_long = 0; s_near = 0; }
            __syncthreads();
            // (1) every live member but the pivots against its subgroup's pivot.  A lane walks its own pair for LB_LANE_CAP bytes ...
            bool any = false;
            for (uint32_t i = tid; i < grp.size; i += BLOCK) {
                const uint32_t g = s_grp[i];
                if (!(g >> 16)) continue;
                any = true;
                const uint32_t g0 = g & 0xFFFFu;
                s_nu[i] = 0;
                if (i == g0) { s_key[i] = LB_PIVOT; continue; }
                const uint32_t depth = s_dep[i];
                const size_t ref = static_cast<size_t>(s_idx[g0]) + depth, other = static_cast<size_t>(s_idx[i]) + depth;
                uint32_t c = 0;
                bool long_one = false;
                if (first_level && lce_known) {
                    c = lce_known[grp.start + i];
                } else if (ref < n && other < n) {
                    const size_t room = n - (ref > other ? ref : other);
                    for (;;) {
                        if (c >= LB_LANE_CAP) { long_one = true; break; }
                        if (static_cast<size_t>(c) + 16 <= room) {
                            const uint64_t lo = *(gptr8)(text + ref + c) ^ *(gptr8)(text + other + c), hi = *(gptr8)(text + ref + c + 8) ^ *(gptr8)(text + other + c + 8);
                            if (lo | hi) { c += lo ? static_cast<uint32_t>(__builtin_ctzll(lo)) >> 3 : 8u + (static_cast<uint32_t>(__builtin_ctzll(hi)) >> 3); break; }
                            c += 16;
                        } else {
                            while (static_cast<size_t>(c) < room && text[ref + c] == text[other + c]) ++c;
                            break;
                        }
                    }
                }
                if (long_one) { s_key[i] = LB_LONG | c; s_long = 1u; continue; }
                const size_t pr = ref + c, po = other + c;
                const bool other_smaller = po >= n ? true : pr >= n ? false : text[po] < text[pr];
                uint32_t tie = 0;  // the LD_TIE bytes from where they part on (see k_lf_deep_wave)
                if (po + LD_TIE > n) s_near = 1u; else tie = __builtin_bswap32(*(gptr4)(text + po));
                s_key[i] = other_smaller ? ((static_cast<uint64_t>(c) << 32) | tie) : ((2ull << 62) | (static_cast<uint64_t>(0x3FFFFFFFu - c) << 32) | tie);
            }
            if (!__syncthreads_or(any)) break;
            if (level > 2 * CAP) { if (tid == 0) *fallback = 1u; break; }  // (cannot be: every level settles a pivot)
            // ... and a wave goes on for the members that are still equal there, a kilobyte per step
            bool gave_up = false;
            for (uint32_t i = wave; s_long != 0u && i < grp.size; i += WAVES) {
                const uint64_t k = s_key[i];  // (uniform over the wave)
                if ((k >> 62) != 3u || !(s_grp[i] >> 16)) continue;
                const uint32_t g0 = s_grp[i] & 0xFFFFu, depth = s_dep[i], c0 = static_cast<uint32_t>(k);
                const size_t ref = static_cast<size_t>(s_idx[g0]) + depth + c0, other = static_cast<size_t>(s_idx[i]) + depth + c0;
                bool long_one = false;
                const uint32_t c = c0 + wave_common_extension(text, n, ref, other, lane, &long_one);
                if (lane == 0) {
                    if (long_one) {
                        gave_up = true;
                        s_key[i] = LB_PIVOT;  // more than LD_MAX_STEPS KiB in common: stays with the pivot for now
                    } else {
                        const size_t pr = ref - c0 + c, po = other - c0 + c;
                        const bool other_smaller = po >= n ? true : pr >= n ? false : text[po] < text[pr];
                        uint32_t tie = 0;
                        if (po + LD_TIE > n) s_near = 1u; else tie = __builtin_bswap32(*(gptr4)(text + po));
                        s_key[i] = other_smaller ? ((static_cast<uint64_t>(c) << 32) | tie) : ((2ull << 62) | (static_cast<uint64_t>(0x3FFFFFFFu - c) << 32) | tie);
                    }
                }
            }
            const bool any_long = __syncthreads_or(gave_up) != 0;
            const uint64_t key_mask = s_near ? ~0xFFFFFFFFull : ~0ull;  // (a member near the text's end: this level's keys without their tie bytes)
            const uint32_t advance = s_near ? 0u : LD_TIE;
            // (2) every member's place inside its subgroup; members of one class keep their order
            uint32_t m_idx[MPT], m_dest[MPT], m_grp[MPT], m_depth[MPT];
            uint8_t m_sym[MPT], m_cls[MPT];
#pragma unroll
            for (int k = 0; k < MPT; ++k) {
                const uint32_t i = k * BLOCK + tid;
                m_grp[k] = 0;
                if (i >= grp.size) continue;
                const uint32_t g = s_grp[i], sz = g >> 16, g0 = g & 0xFFFFu;
                if (!sz) continue;
                const uint64_t mine = s_key[i] & key_mask;
                uint32_t less = 0, eq = 0, eqb = 0;
                for (uint32_t b = g0; b < g0 + sz; ++b) {
                    const uint64_t v = s_key[b] & key_mask;
                    less += v < mine;
                    eq += v == mine;
                    eqb += (v == mine) && b < i;
                }
                m_idx[k] = s_idx[i];
                m_sym[k] = s_sym[i];
                m_dest[k] = g0 + less + eqb;
                m_grp[k] = (g0 + less) | (eq << 16);
                m_cls[k] = static_cast<uint8_t>(mine >> 62);
                // what the class is known to share: depth + c (the pivot's class: nothing measured)
                const uint32_t c30 = static_cast<uint32_t>(mine >> 32) & 0x3FFFFFFFu;
                const uint32_t c = m_cls[k] == 0 ? c30 + advance : m_cls[k] == 2 ? 0x3FFFFFFFu - c30 + advance : 0u;
                m_depth[k] = s_dep[i] + c;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < MPT; ++k) {
                if (!(m_grp[k] >> 16)) continue;
                const uint32_t d = m_dest[k];
                s_idx[d] = m_idx[k];
                s_sym[d] = m_sym[k];
                s_grp[d] = m_grp[k];
                s_dep[d] = m_depth[k];
                s_key[d] = m_cls[k];  // (the class, for step 3)
            }
            __syncthreads();
            for (uint32_t i = tid; i < grp.size; i += BLOCK) {
                const uint32_t g = s_grp[i];
                if (!(g >> 16)) continue;
                const uint32_t g0 = g & 0xFFFFu;
                if (s_sym[i] != s_sym[g0] || s_idx[i] == 0u) s_nu[g0] = 1;
            }
            __syncthreads();
            // (3) subgroups that are done write L; a pivot's class that is still live holds a member with more in common with the pivot than a
            //     workgroup measures: to the giant list, members and all; the rest goes on
            for (uint32_t i = tid; i < grp.size; i += BLOCK) {
                const uint32_t g = s_grp[i], sz = g >> 16, g0 = g & 0xFFFFu;
                if (!sz) continue;
                if (sz == 1 || !s_nu[g0]) {
                    const uint32_t p = act_pos[grp.start + i];
                    bwt[p] = s_sym[i];
                    if (s_idx[i] == 0u) *origin = p;
                    s_grp[i] = g0;  // size 0: done
                } else if (i == g0 && s_key[i] == 1ull) {
                    uint32_t off = 0xFFFFFFFFu;
                    if (any_long) {
                        const uint32_t at = atomicAdd(giant.count, 1u), o = atomicAdd(giant.used, sz);
                        if (at < giant.cap && o + sz <= giant.arena_cap) { off = o; giant.list[at] = LfDeepGroup{o, sz, s_dep[i], 0u}; }
                    }
                    if (off == 0xFFFFFFFFu) *fallback = 1u;  // (a live pivot class without a long member cannot be; never spin on it)
                    s_dep[i] = off;  // (the class is leaving: its head's depth word carries the arena offset to its members)
                }
            }
            __syncthreads();
            for (uint32_t i = tid; i < grp.size; i += BLOCK) {
                const uint32_t g = s_grp[i], sz = g >> 16, g0 = g & 0xFFFFu;
                if (!sz || s_key[i] != 1ull) continue;
                const uint32_t off = s_dep[g0];
                if (off != 0xFFFFFFFFu) {
                    giant.idx[off + (i - g0)] = s_idx[i];
                    giant.sym[off + (i - g0)] = s_sym[i];
                    giant.pos[off + (i - g0)] = act_pos[grp.start + i];
                }
            }
            __syncthreads();
            for (uint32_t i = tid; i < grp.size; i += BLOCK)
                if ((s_grp[i] >> 16) && s_key[i] == 1ull) s_grp[i] &= 0xFFFFu;
        }
    }
}

// k_lf_deep_wave: the arena's groups of up to 64 members, a WAVE per group (lane = member, registers and cross-lane moves only: no LDS, no barrier).
// Real text leaves a hundred thousand such groups -- the first suffixes of copied passages and their copies, two to a few dozen members each -- and
// a workgroup per group (k_lf_deep) spends its time in barriers and dependent phases, not in measuring: 6.8 ms for the 120 K groups of 50 MB of
// real text, one launch per round, each as long as its slowest group.  Same method: per level every live subgroup measures its members against its
// first one (the pivot) -- here every lane walks its OWN pair of suffixes, 16 bytes per step -- and orders them by (smaller / larger than the pivot,
// bytes in common); all subgroups of the group advance together.  A lane that has LW_CAP bytes in common with its pivot hands its subgroup on to
// the workgroup kernel (which measures a kilobyte per wave step and knows the way to the grid-wide measure): the arena holds the members in their
// current order, the list gets an entry flagged LD_HANDED behind the `total0` entries this kernel reads.
constexpr uint32_t LW_CAP = 2048;
__device__ __forceinline__ uint32_t lane_move(uint32_t v, int dest) {  // forward permutation: my value goes to lane `dest`
    return static_cast<uint32_t>(__builtin_amdgcn_ds_permute(dest << 2, static_cast<int>(v)));
}
__global__ __launch_bounds__(256) void k_lf_deep_wave(uint32_t *__restrict__ a_idx, const uint32_t *__restrict__ a_pos, uint8_t *__restrict__ a_sym,
                                                       LfDeepGroup *__restrict__ deep, uint32_t *__restrict__ deep_count, uint32_t begin, uint32_t total0, uint32_t deep_cap,
                                                       const uint8_t *__restrict__ text, uint32_t n, uint8_t *__restrict__ bwt, uint32_t *__restrict__ origin,
                                                       uint32_t *__restrict__ fallback) {
    typedef uint64_t __attribute__((aligned(1))) unaligned_u64;
    typedef const unaligned_u64 __attribute__((address_space(1))) *gptr8;
    typedef uint32_t __attribute__((aligned(1))) unaligned_u32;
    typedef const unaligned_u32 __attribute__((address_space(1))) *gptr4;
    const int lane = threadIdx.x & 63;
    const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t gi = begin + ((blockIdx.x * blockDim.x + threadIdx.x) >> 6); gi < total0; gi += nwaves) {  // the entries [begin, total0)
        const LfDeepGroup grp = deep[gi];
        if (grp.size > LW_MAX || grp.flags != 0u) continue;  // (handed on, taken by k_lf_medium, or still in a round's list)
        const bool in = static_cast<uint32_t>(lane) < grp.size;
        uint32_t idx = in ? a_idx[grp.start + lane] : 0xFFFFFFFFu;
        uint32_t sym = in ? a_sym[grp.start + lane] : 0u;
        const uint32_t pos = in ? a_pos[grp.start + lane] : 0u;  // the SA position of this lane's PLACE in the group
        uint32_t sg0 = 0, sgn = grp.size, depth = grp.depth;     // my subgroup: lanes [sg0, sg0 + sgn), equal in `depth` symbols
        bool live = in;
        for (int level = 0; __ballot(live) != 0ull; ++level) {
            if (level > 2 * static_cast<int>(LW_MAX)) { if (lane == 0) *fallback = 1u; break; }  // (cannot be: every level settles a pivot)
            // (1) bytes in common with the pivot, and who is smaller where they part (the end of the text counts: a proper prefix is smaller)
            const uint32_t pidx = static_cast<uint32_t>(__shfl(static_cast<int>(idx), static_cast<int>(sg0), kWave));
            const bool measure = live && static_cast<uint32_t>(lane) != sg0;
            uint32_t c = 0;
            bool capped = false, other_smaller = false;
            const size_t ref = static_cast<size_t>(pidx) + depth, other = static_cast<size_t>(idx) + depth;
            if (measure) {
                if (ref < n && other < n) {
                    const size_t room = n - (ref > other ? ref : other);  // bytes the shorter of the two still has
                    for (;;) {
                        if (c >= LW_CAP) { capped = true; break; }
                        if (static_cast<size_t>(c) + 16 <= room) {
                            const uint64_t lo = *(gptr8)(text + ref + c) ^ *(gptr8)(text + other + c), hi = *(gptr8)(text + ref + c + 8) ^ *(gptr8)(text + other + c + 8);
                            if (lo | hi) { c += lo ? static_cast<uint32_t>(__builtin_ctzll(lo)) >> 3 : 8u + (static_cast<uint32_t>(__builtin_ctzll(hi)) >> 3); break; }
                            c += 16;
                        } else {
                            while (static_cast<size_t>(c) < room && text[ref + c] == text[other + c]) ++c;
                            break;
                        }
                    }
                }
            }
            // a lane at the cap: the whole wave goes on with its pair, a kilobyte per step (the first suffixes of copied files have tens of
            // kilobytes in common); only what is still equal after LD_MAX_STEPS of those is handed on
            for (uint64_t todo = __ballot(capped); todo; todo &= todo - 1) {
                const int t = __builtin_ctzll(todo);
                const size_t t_ref = static_cast<size_t>(static_cast<uint32_t>(__shfl(static_cast<int>(pidx), t, kWave))) +
                                     static_cast<uint32_t>(__shfl(static_cast<int>(depth), t, kWave)) + LW_CAP;
                const size_t t_other = static_cast<size_t>(static_cast<uint32_t>(__shfl(static_cast<int>(idx), t, kWave))) +
                                       static_cast<uint32_t>(__shfl(static_cast<int>(depth), t, kWave)) + LW_CAP;
                bool long_one = false;
                const uint32_t extra = wave_common_extension(text, n, t_ref, t_other, lane, &long_one);
                if (lane == t && !long_one) { c = LW_CAP + extra; capped = false; }
            }
            // ... and the LD_TIE bytes from where they part on: members of one side with one c are told apart by them at once (all members that differ
            // from the pivot in their first byte would otherwise be one class known no deeper than before: a group of pairwise different members
            // -- one that left k_lf_finish for its step limit, not for being stuck -- would lose only its pivot per level)
            uint32_t tie = 0;
            bool near_end = false;
            if (measure && !capped) {
                const size_t pr = ref + c, po = other + c;
                other_smaller = po >= n ? true : pr >= n ? false : text[po] < text[pr];
                near_end = po + LD_TIE > n;
                if (!near_end) tie = __builtin_bswap32(*(gptr4)(text + po));
            }
            // a lane still at the cap: its whole subgroup goes to the workgroup kernel, members in their current order
            const uint64_t mine = (sgn >= 64u ? ~0ull : ((1ull << sgn) - 1ull)) << sg0;
            const uint64_t capped_any = __ballot(capped);
            if (live && (capped_any & mine) != 0ull) {
                a_idx[grp.start + lane] = idx;
                a_sym[grp.start + lane] = static_cast<uint8_t>(sym);
                if (static_cast<uint32_t>(lane) == sg0) {
                    const uint32_t at = atomicAdd(deep_count, 1u);
                    if (at < deep_cap) deep[at] = LfDeepGroup{grp.start + sg0, sgn, depth, LD_HANDED};
                    else *fallback = 1u;
                }
                live = false;
            }
            // (2) my place inside my subgroup: smaller than the pivot by c ascending, the pivot, larger by c descending; one c on one side = the next subgroup
            // (a member that ends within the tie bytes -- the text's last suffixes -- switches them off for its whole subgroup: zero padding would tie
            //  it with a member that goes on with zero bytes)
            const bool ties = (__ballot(near_end) & mine) == 0ull;
            if (!ties) tie = 0;
            const uint64_t key = !measure ? (1ull << 62) : other_smaller ? ((static_cast<uint64_t>(c) << 32) | tie) : ((2ull << 62) | (static_cast<uint64_t>(0x3FFFFFFFu - c) << 32) | tie);
            const uint32_t k_lo = static_cast<uint32_t>(key), k_hi = static_cast<uint32_t>(key >> 32);
            uint32_t less = 0, eq = 0, eqb = 0;
            for (uint32_t t = 0; t < grp.size; ++t) {
                const uint64_t kt = (static_cast<uint64_t>(static_cast<uint32_t>(__shfl(static_cast<int>(k_hi), static_cast<int>(t), kWave))) << 32) |
                                    static_cast<uint32_t>(__shfl(static_cast<int>(k_lo), static_cast<int>(t), kWave));
                const bool inside = t - sg0 < sgn;  // (mod 2^32: t >= sg0 && t < sg0 + sgn)
                less += inside && kt < key ? 1u : 0u;
                eq += inside && kt == key ? 1u : 0u;
                eqb += inside && kt == key && t < static_cast<uint32_t>(lane) ? 1u : 0u;
            }
            const int dest = live ? static_cast<int>(sg0 + less + eqb) : lane;  // (a dead lane stays: the live subgroups permute among themselves)
            const uint32_t n_sg0 = sg0 + less, n_sgn = eq, n_depth = depth + (measure ? c + (ties ? LD_TIE : 0u) : 0u);
            idx = lane_move(idx, dest);
            sym = lane_move(sym, dest);
            sg0 = lane_move(live ? n_sg0 : sg0, dest);
            sgn = lane_move(live ? n_sgn : sgn, dest);
            depth = lane_move(live ? n_depth : depth, dest);
            live = lane_move(live ? 1u : 0u, dest) != 0u;
            // (3) a subgroup that is alone or has one symbol in front (and not suffix 0, whose place is the origin) is done
            const uint32_t fs = static_cast<uint32_t>(__shfl(static_cast<int>(sym), static_cast<int>(sg0), kWave));
            const uint64_t reasons = __ballot(live && (sym != fs || idx == 0u));
            const uint64_t mine2 = (sgn >= 64u ? ~0ull : ((1ull << sgn) - 1ull)) << sg0;
            if (live && (sgn == 1u || (reasons & mine2) == 0ull)) {
                bwt[pos] = static_cast<uint8_t>(sym);
                if (idx == 0u) *origin = pos;
                live = false;
            }
        }
    }
}

// k_lf_medium: the groups a round listed with their members still in the round's own list (LD_LIST, entries [begin, total): more members than
// k_lf_finish's LDS takes, at most BLOCK * 8) -- refined from the text to their END inside one workgroup's LDS, before the round's rerank rewrites
// the list.  Per step: five more bytes of text per live member, and ONE radix sort of the whole group inside LDS on (start of the member's
// subgroup | those bytes) -- k_sort_groups' loop; subgroups are stretches of positions and a member never leaves its own, so the subgroup's start
// above the text keeps everybody in place -- then heads where the key changes, a running maximum for every position's new subgroup, and the
// subgroups that are singletons or have one symbol in front write L and die.  (k_lf_finish finds a member's place by counting over its subgroup:
// s * s comparisons -- 4096 members: a millisecond per step on one CU, measured; the sort costs what the members cost, 40 us.)  Subgroups that do
// not split for `stuck_steps` steps, and what is left after `max_steps`, leave for the arena like k_lf_finish's.  Once the big list is short,
// every group of up to LF_DEEP_MAX members goes this way and the rounds that are left hold the few bigger ones (50 MB of real text: the last nine
// of fourteen rounds were a dozen launches each for fewer than 250 K slots).  Also the way of the groups of a stalled big list.
constexpr int LM_SYMS = 5;  // bytes of text per step: 13 bits of subgroup start | 40 bits of text | 3 bits "how many of them exist" | 8 bits symbol in front = 64
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_lf_medium(const uint32_t *__restrict__ l_idx, const uint32_t *__restrict__ l_pos, const uint8_t *__restrict__ l_sym,
                                                      LfDeepGroup *__restrict__ deep, uint32_t *__restrict__ deep_count, const uint32_t *__restrict__ deep_begin,
                                                      uint32_t deep_cap, const uint8_t *__restrict__ text, uint32_t n, uint8_t *__restrict__ bwt,
                                                      uint32_t *__restrict__ origin, LfArena arena, uint32_t *__restrict__ fallback, int max_steps, int stuck_steps) {
    constexpr int WAVES = BLOCK / 64, KPT = 8, CAP = BLOCK * KPT;
    static_assert(CAP <= 8192, "13 bits of subgroup start in the key");
    __shared__ uint64_t s_keys[CAP];
    __shared__ uint32_t s_vals[CAP];
    __shared__ uint16_t s_sg[CAP];                          // start of the position's subgroup
    __shared__ uint8_t s_dead[CAP], s_nu[CAP], s_chg[CAP], s_stuck[CAP];  // per position | per subgroup (at its start): reason to stay live, has split, steps without a split
    __shared__ uint32_t s_cnt[WAVES][256];
    __shared__ uint32_t s_start[256];
    __shared__ uint32_t s_tmp[WAVES + 1];
    __shared__ uint32_t s_wmax[WAVES];
    __shared__ uint32_t s_leave[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t total = *deep_count < deep_cap ? *deep_count : deep_cap;
    for (uint32_t gi = *deep_begin + blockIdx.x; gi < total; gi += gridDim.x) {
        const LfDeepGroup grp = deep[gi];
        if (!(grp.flags & LD_LIST) || grp.size > static_cast<uint32_t>(CAP)) continue;
        const uint32_t S = grp.size;
        const int kmax = static_cast<int>((S + BLOCK - 1) / BLOCK);  // members per thread this group needs: every loop below stops there
        const uint32_t wbase = static_cast<uint32_t>(wave) * (64u * static_cast<uint32_t>(kmax));  // wave w owns positions [w * 64 kmax, (w + 1) * 64 kmax), lane-striped
        const int sort_end = 51 + (S > 1u ? 32 - __builtin_clz(S - 1u) : 1);  // the key's sorted bits: [8, 51) text and count, above them the subgroup's start (< S)
        __syncthreads();  // (the arrays of the group before this one are no longer read)
        if (tid < 2) s_leave[tid] = 0;
        uint64_t key[KPT];
        uint32_t val[KPT];
#pragma unroll
        for (int k = 0; k < KPT; ++k) {
            if (k >= kmax) break;
            const uint32_t li = wbase + k * 64 + lane;
            val[k] = li < S ? l_idx[grp.start + li] : 0u;
            key[k] = li < S ? l_sym[grp.start + li] : 0u;  // (the symbol in front rides in the key's low byte)
            if (li < S) { s_sg[li] = 0; s_dead[li] = 0; s_stuck[li] = 0; }
        }
        for (int step = 1;; ++step) {
            const uint32_t depth = grp.depth + static_cast<uint32_t>(LM_SYMS) * static_cast<uint32_t>(step - 1);
            __syncthreads();
            // (A) keys of the step: subgroup start | the next LM_SYMS bytes (zero padded) | how many of them exist | symbol in front.  A suffix that
            //     ended in front of the window has zero there: it sorts first (a proper prefix of the others), and ties among such members are the
            //     deep list's business (they do not split).  Dead members keep their stretch (zero text).  Padding sorts last.
            int alive = 0;
#pragma unroll
            for (int k = 0; k < KPT; ++k) {
                if (k >= kmax) break;
                const uint32_t li = wbase + k * 64 + lane;
                if (li >= S) { key[k] = ~0ull; continue; }
                uint64_t field = 0;
                if (!s_dead[li]) {
                    alive = 1;
                    const size_t p = static_cast<size_t>(val[k]) + depth;
                    if (p < n) {
                        const size_t avail = n - p;
                        field = ((text_key_raw(text, n, p) >> 24) << 3) | (avail >= static_cast<size_t>(LM_SYMS) ? static_cast<uint64_t>(LM_SYMS) : static_cast<uint64_t>(avail));
                    }
                }
                key[k] = (static_cast<uint64_t>(s_sg[li]) << 51) | (field << 8) | (key[k] & 0xFFull);
                s_nu[li] = 0;
                s_chg[li] = 0;
            }
            if (!__syncthreads_or(alive)) break;
            // (B) one radix sort of the group on the key's bits [8, sort_end): k_sort_groups' loop
            for (int shift = 8; shift < sort_end; shift += 8) {
                for (int i = tid; i < WAVES * 256; i += BLOCK) (&s_cnt[0][0])[i] = 0;
                __syncthreads();
                uint32_t rnk[KPT];
#pragma unroll
                for (int k = 0; k < KPT; ++k) {
                    if (k >= kmax) break;
                    const uint32_t d = static_cast<uint32_t>(key[k] >> shift) & 0xFFu;
                    const LaneSet same = wave_match<8>(d, ~0ull);
                    const uint32_t before = same.before();
                    const uint32_t old = s_cnt[wave][d];
                    __builtin_amdgcn_wave_barrier();
                    if (before == 0) s_cnt[wave][d] = old + same.count();
                    __builtin_amdgcn_wave_barrier();
                    rnk[k] = old + before;
                }
                __syncthreads();
                {
                    const int d = tid & 255;
                    uint32_t run = 0;
                    if (tid < 256) {
#pragma unroll
                        for (int w = 0; w < WAVES; ++w) {
                            const uint32_t c = s_cnt[w][d];
                            s_cnt[w][d] = run;
                            run += c;
                        }
                    }
                    const uint32_t first = block_excl_sum<WAVES>(tid < 256 ? run : 0u, s_tmp, nullptr);
                    if (tid < 256) s_start[d] = first;
                }
                __syncthreads();
#pragma unroll
                for (int k = 0; k < KPT; ++k) {
                    if (k >= kmax) break;
                    const uint32_t d = static_cast<uint32_t>(key[k] >> shift) & 0xFFu;
                    const uint32_t p = s_start[d] + s_cnt[wave][d] + rnk[k];
                    s_keys[p] = key[k];
                    s_vals[p] = val[k];
                }
                __syncthreads();
#pragma unroll
                for (int k = 0; k < KPT; ++k) {
                    if (k >= kmax) break;
                    const uint32_t li = wbase + k * 64 + lane;
                    key[k] = s_keys[li];
                    val[k] = s_vals[li];
                }
                __syncthreads();
            }
            // (C) heads where the key changes (above the symbol in front); every position's new subgroup = the last head at or before it
            uint32_t nsg[KPT];
            bool head[KPT];
            {
                uint32_t running = 0;
#pragma unroll
                for (int k = 0; k < KPT; ++k) {
                    if (k >= kmax) break;
                    const uint32_t li = wbase + k * 64 + lane;
                    head[k] = li < S && (li == 0 || (s_keys[li - 1] >> 8) != (key[k] >> 8));
                    uint32_t v = wave_incl_max(head[k] ? li : 0u, lane);
                    v = v > running ? v : running;
                    nsg[k] = v;
                    running = static_cast<uint32_t>(__shfl(static_cast<int>(v), 63, kWave));
                }
                if (lane == 0) s_wmax[wave] = running;
            }
            __syncthreads();
            {
                uint32_t carry = 0;
                for (int w = 0; w < wave; ++w) carry = carry > s_wmax[w] ? carry : s_wmax[w];
#pragma unroll
                for (int k = 0; k < KPT; ++k) {
                    if (k >= kmax) break;
                    nsg[k] = nsg[k] > carry ? nsg[k] : carry;
                }
            }
            // (D) what the new subgroups hold: a reason to stay live (two symbols in front, suffix 0)?  has the old subgroup split?
#pragma unroll
            for (int k = 0; k < KPT; ++k) {
                if (k >= kmax) break;
                const uint32_t li = wbase + k * 64 + lane;
                if (li >= S || s_dead[li]) continue;
                if ((key[k] & 0xFFull) != (s_keys[nsg[k]] & 0xFFull) || val[k] == 0u) s_nu[nsg[k]] = 1;
                if (nsg[k] != s_sg[li]) s_chg[s_sg[li]] = 1;
            }
            __syncthreads();
            // (E) subgroups that are done write L; those that do not move, and what is still live after max_steps steps, leave for the arena
            uint32_t leaving = 0;  // bit k: my member k leaves
            bool dies[KPT];
#pragma unroll
            for (int k = 0; k < KPT; ++k) {
                dies[k] = false;
                if (k >= kmax) break;
                const uint32_t li = wbase + k * 64 + lane;
                if (li >= S || s_dead[li]) continue;
                const uint32_t g0 = nsg[k], old0 = s_sg[li];
                const bool single = head[k] && (li + 1 >= S || (s_keys[li + 1] >> 8) != (key[k] >> 8));
                const uint32_t stuck = s_chg[old0] ? 0u : static_cast<uint32_t>(s_stuck[old0]) + 1u;  // (an old subgroup that did not split is its own new one)
                if (single || !s_nu[g0]) {
                    const uint32_t p = l_pos[grp.start + li];
                    bwt[p] = static_cast<uint8_t>(key[k]);
                    if (val[k] == 0u) *origin = p;
                    dies[k] = true;
                } else if (static_cast<int>(stuck) >= stuck_steps || step >= max_steps) {
                    leaving |= 1u << k;
                    dies[k] = true;
                }
            }
            __syncthreads();  // (s_sg / s_stuck / s_chg of the old subgroups have been read)
            // the new heads' counts of steps without a split, parked beside the reason flags until every thread has read the old ones
#pragma unroll
            for (int k = 0; k < KPT; ++k) {
                if (k >= kmax) break;
                const uint32_t li = wbase + k * 64 + lane;
                if (li >= S) continue;
                if (!s_dead[li]) {
                    const uint32_t old0 = s_sg[li];
                    const uint8_t st = s_chg[old0] ? uint8_t(0) : static_cast<uint8_t>(s_stuck[old0] + 1);
                    if (head[k]) s_nu[li] = static_cast<uint8_t>(s_nu[li] | (st << 1));  // (parked: the new head's stuck count, written behind the barrier below)
                }
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < KPT; ++k) {
                if (k >= kmax) break;
                const uint32_t li = wbase + k * 64 + lane;
                if (li >= S || s_dead[li]) continue;
                s_sg[li] = static_cast<uint16_t>(nsg[k]);
                if (head[k]) s_stuck[li] = static_cast<uint8_t>(s_nu[li] >> 1);
                if (dies[k]) s_dead[li] = 1;
            }
            if (__syncthreads_or(leaving != 0u)) {
                // a leaving subgroup: its head reserves (group number, member offset) among the step's leavers; sizes by counting at the head
                for (int i = tid; i < CAP; i += BLOCK) s_vals[i] = 0;  // (s_vals: free until the next sort; here: members of the leaving subgroup at its head)
                __syncthreads();
#pragma unroll
                for (int k = 0; k < KPT; ++k)
                    if ((leaving >> k) & 1u) atomicAdd(&s_vals[nsg[k]], 1u);
                __syncthreads();
#pragma unroll
                for (int k = 0; k < KPT; ++k) {
                    if (!((leaving >> k) & 1u) || !head[k]) continue;
                    const uint32_t li = wbase + k * 64 + lane;
                    const uint32_t sz = s_vals[li];
                    s_keys[li] = atomicAdd(&s_leave[0], 1u) | (static_cast<uint64_t>(atomicAdd(&s_leave[1], sz)) << 32);  // (s_keys: free until the next sort)
                }
                __syncthreads();
                if (tid == 0) {
                    const uint32_t groups = s_leave[0], members = s_leave[1];
                    const uint32_t at = atomicAdd(deep_count, groups), off = atomicAdd(arena.used, members);
                    const bool fits = off + members <= arena.cap && at + groups <= deep_cap;
                    if (!fits) *fallback = 1u;
                    s_leave[2] = fits ? at : 0xFFFFFFFFu;
                    s_leave[3] = off;
                    s_leave[0] = s_leave[1] = 0;
                }
                __syncthreads();
                const uint32_t at0 = s_leave[2], off0 = s_leave[3];
#pragma unroll
                for (int k = 0; k < KPT; ++k) {
                    if (!((leaving >> k) & 1u) || at0 == 0xFFFFFFFFu) continue;
                    const uint32_t li = wbase + k * 64 + lane, g0 = nsg[k];
                    const uint32_t off = off0 + static_cast<uint32_t>(s_keys[g0] >> 32);
                    if (head[k]) deep[at0 + static_cast<uint32_t>(s_keys[g0])] = LfDeepGroup{off, s_vals[g0], depth + static_cast<uint32_t>(LM_SYMS), 0u};
                    const uint32_t at = off + (li - g0);
                    arena.idx[at] = val[k];
                    arena.sym[at] = static_cast<uint8_t>(key[k]);
                    arena.pos[at] = l_pos[grp.start + li];  // the SA position of the slot: where the member that ends up (li - g0)-th in its subgroup belongs
                }
            }
        }
        if (tid == 0) deep[gi].flags = LD_DONE;
    }
}

// k_lf_lce: the common extension of every member of every listed group with the group's first member, by the whole grid: a workgroup
// compares 4 KiB per step, the workgroups take the 4 KiB chunks of a pair in turn and stop at the first chunk behind the best answer so far
// (res[arena slot of the member], preset to ~0; the end of the shorter suffix counts as a difference).  Two copies of a 50 MB file: one pair,
// 100 MB read.  (Only classes that are still LIVE come here: the pairs (i, i + n/2) of two identical halves have one symbol in front.)
__global__ __launch_bounds__(256) void k_lf_lce(const uint32_t *__restrict__ g_idx, const LfDeepGroup *__restrict__ list, const uint32_t *__restrict__ count,
                                                 uint32_t cap, const uint8_t *__restrict__ t, uint32_t n, uint32_t *__restrict__ res) {
    typedef uint64_t __attribute__((aligned(1))) unaligned_u64;
    typedef const unaligned_u64 __attribute__((address_space(1))) *gptr8;
    __shared__ uint32_t s_mis, s_best;
    const int tid = threadIdx.x;
    const uint32_t total = *count < cap ? *count : cap;
    for (uint32_t g = 0; g < total; ++g) {
        const LfDeepGroup grp = list[g];
        const size_t x = static_cast<size_t>(g_idx[grp.start]) + grp.depth;
        for (uint32_t j = 1; j < grp.size; ++j) {
            const size_t y = static_cast<size_t>(g_idx[grp.start + j]) + grp.depth;
            uint32_t *r = res + grp.start + j;  // per member (arena slot)
            if (x >= n || y >= n) { if (blockIdx.x == 0 && tid == 0) *r = 0; continue; }
            const size_t room = n - (x > y ? x : y);
            for (size_t chunk = blockIdx.x;; chunk += gridDim.x) {
                const size_t off = chunk * 4096;
                __syncthreads();
                if (tid == 0) { s_best = __atomic_load_n(r, __ATOMIC_RELAXED); s_mis = 0xFFFFFFFFu; }
                __syncthreads();
                if (off >= room) { if (tid == 0) atomicMin(r, static_cast<uint32_t>(room)); break; }  // no difference up to the end of the shorter suffix
                if (off >= s_best) break;  // another workgroup has found a difference in front of this chunk
                const size_t o = off + 16 * static_cast<size_t>(tid);
                uint32_t mis = 16;
                if (o + 16 <= room) {
                    const uint64_t lo = *(gptr8)(t + x + o) ^ *(gptr8)(t + y + o), hi = *(gptr8)(t + x + o + 8) ^ *(gptr8)(t + y + o + 8);
                    if (lo | hi) mis = lo ? static_cast<uint32_t>(__builtin_ctzll(lo)) >> 3 : 8u + (static_cast<uint32_t>(__builtin_ctzll(hi)) >> 3);
                } else if (o < room) {
                    for (uint32_t q = 0; q < 16; ++q)
                        if (o + q >= room || t[x + o + q] != t[y + o + q]) { mis = q; break; }
                }
                if (mis < 16) atomicMin(&s_mis, static_cast<uint32_t>(o - off) + mis);
                __syncthreads();
                const uint32_t found = s_mis;
                if (found != 0xFFFFFFFFu) { if (tid == 0) atomicMin(r, static_cast<uint32_t>(off) + found); break; }
            }
            __syncthreads();
        }
    }
}

// ---- two size classes of big groups ---------------------------------------------------------------------------------------------------------------
// The big list of a round holds the members of every group above the LDS kernel's size, sorted by one global radix sort of (group, text) -- seven
// passes for five symbols.  Nearly half of its slots, round after round, sit in groups of at most 8192 members (word-like text: 69 M of 150 M
// slot-rounds), which ONE workgroup sorts inside LDS (sort_groups, radix_sort.hip) at a third of the price.  So the list gets two regions: the
// giant groups first (global sort, on their own few group bits), the medium ones behind (sorted group by group).  Same kernels as classify_and_read
// with a size range and the bases of the class: dense index and list offset go on from where the class before stopped.
//   Mail::Classes: rounds.big_slots / big_groups count the giant class, medium_slots / medium_groups the medium one
// (both classes in one pass: `part` holds (giant slots, giant groups, medium slots, medium groups) per workgroup)
__global__ __launch_bounds__(256) void k_cls_reduce(const uint32_t *__restrict__ gstart, const Mail::Classes *__restrict__ mail, uint4 *__restrict__ part, uint32_t lo,
                                                     uint32_t mid) {
    __shared__ uint32_t s_w[4][RR_WAVES];
    const size_t groups = mail->rounds.groups;
    size_t t0, t1;
    big_stretch(groups, &t0, &t1);
    uint32_t gs = 0, gc = 0, ms = 0, mc = 0;
    for (size_t t = t0; t < t1; ++t) {
        const size_t g0 = t * BG_TILE + static_cast<size_t>(threadIdx.x) * BG_IPT;
        if (g0 >= groups) continue;
        uint32_t prev = gstart[g0];
#pragma unroll
        for (int j = 0; j < BG_IPT && g0 + j < groups; ++j) {
            const uint32_t next = gstart[g0 + j + 1];
            const uint32_t sz = next - prev;
            prev = next;
            const bool giant = sz > mid, medium = sz > lo && sz <= mid;
            gs += giant ? sz : 0u;
            gc += giant ? 1u : 0u;
            ms += medium ? sz : 0u;
            mc += medium ? 1u : 0u;
        }
    }
    gs = wave_sum(gs);
    gc = wave_sum(gc);
    ms = wave_sum(ms);
    mc = wave_sum(mc);
    if ((threadIdx.x & 63) == 0) { s_w[0][threadIdx.x >> 6] = gs; s_w[1][threadIdx.x >> 6] = gc; s_w[2][threadIdx.x >> 6] = ms; s_w[3][threadIdx.x >> 6] = mc; }
    __syncthreads();
    if (threadIdx.x == 0)
        part[blockIdx.x] = make_uint4(s_w[0][0] + s_w[0][1] + s_w[0][2] + s_w[0][3], s_w[1][0] + s_w[1][1] + s_w[1][2] + s_w[1][3],
                                      s_w[2][0] + s_w[2][1] + s_w[2][2] + s_w[2][3], s_w[3][0] + s_w[3][1] + s_w[3][2] + s_w[3][3]);
}
// exclusive over the workgroups, the medium class behind the giant one; totals -> the mailbox; sentinel behind the last group
__global__ __launch_bounds__(BG_GRID) void k_cls_spine(uint4 *__restrict__ part, Mail::Classes *__restrict__ mail, uint32_t *__restrict__ bigoff) {
    __shared__ uint32_t s_tmp[16 + 1];
    const uint4 v = part[threadIdx.x];
    uint32_t tg, tgc, tm, tmc;
    const uint32_t rg = block_excl_sum<BG_GRID / 64>(v.x, s_tmp, &tg);
    const uint32_t rgc = block_excl_sum<BG_GRID / 64>(v.y, s_tmp, &tgc);
    const uint32_t rm = block_excl_sum<BG_GRID / 64>(v.z, s_tmp, &tm);
    const uint32_t rmc = block_excl_sum<BG_GRID / 64>(v.w, s_tmp, &tmc);
    part[threadIdx.x] = make_uint4(rg, rgc, tg + rm, tgc + rmc);
    if (threadIdx.x == 0) {
        mail->rounds.big_slots = tg;
        mail->rounds.big_groups = tgc;
        mail->medium_slots = tm;
        mail->medium_groups = tmc;
        bigoff[tgc + tmc] = tg + tm;
    }
}
__global__ __launch_bounds__(256) void k_cls_apply(const uint32_t *__restrict__ gstart, const Mail::Classes *__restrict__ mail, const uint4 *__restrict__ part,
                                                    uint32_t *__restrict__ bigidx, uint32_t *__restrict__ bigoff, uint32_t lo, uint32_t mid) {
    __shared__ uint32_t s_tmp[RR_WAVES + 1];
    const size_t groups = mail->rounds.groups;
    size_t t0, t1;
    big_stretch(groups, &t0, &t1);
    uint4 base = part[blockIdx.x];
    for (size_t t = t0; t < t1; ++t) {
        const size_t g0 = t * BG_TILE + static_cast<size_t>(threadIdx.x) * BG_IPT;
        uint32_t v[BG_IPT], gs = 0, gc = 0, ms = 0, mc = 0;
#pragma unroll
        for (int j = 0; j < BG_IPT; ++j) {
            uint32_t sz = 0;
            if (g0 + j < groups) sz = gstart[g0 + j + 1] - gstart[g0 + j];
            v[j] = sz > lo ? sz : 0u;
            const bool giant = sz > mid, medium = sz > lo && sz <= mid;
            gs += giant ? sz : 0u;
            gc += giant ? 1u : 0u;
            ms += medium ? sz : 0u;
            mc += medium ? 1u : 0u;
        }
        uint32_t t_gs, t_gc, t_ms, t_mc;
        uint32_t run_g = base.x + block_excl_sum<RR_WAVES>(gs, s_tmp, &t_gs);
        uint32_t idx_g = base.y + block_excl_sum<RR_WAVES>(gc, s_tmp, &t_gc);
        uint32_t run_m = base.z + block_excl_sum<RR_WAVES>(ms, s_tmp, &t_ms);
        uint32_t idx_m = base.w + block_excl_sum<RR_WAVES>(mc, s_tmp, &t_mc);
#pragma unroll
        for (int j = 0; j < BG_IPT; ++j) {
            if (g0 + j < groups && v[j]) {
                if (v[j] > mid) { bigidx[g0 + j] = idx_g; bigoff[idx_g] = run_g; ++idx_g; run_g += v[j]; }
                else { bigidx[g0 + j] = idx_m; bigoff[idx_m] = run_m; ++idx_m; run_m += v[j]; }
            }
        }
        base.x += t_gs;
        base.y += t_gc;
        base.z += t_ms;
        base.w += t_mc;
    }
}
constexpr uint32_t LF_MEDIUM_MAX = 8192;  // largest group sort_groups takes
// classification into (giant: above LF_MEDIUM_MAX | medium: above `lo`, at most LF_MEDIUM_MAX) and the read-back; the list offsets of both classes
// go to bigoff (giant groups first), a group's dense index over both classes to bigidx
int classify_two_and_read(dk_ctx *ctx, const uint32_t *gstart, uint32_t *bigidx, uint32_t *bigoff, uint32_t lo, GroupCounts *out) {
    hipStream_t st = ctx->stream;
    const size_t mark = ctx->ws_mark();
    uint4 *part = ctx->ws_alloc<uint4>(BG_GRID);
    if (!part) return DK_E_NOMEM;
    const uint32_t mid = std::max(lo, LF_MEDIUM_MAX);
    {
        LaunchScope ls(ctx, K_BIG_CLASSIFY, 0.0);
        k_cls_reduce<<<dim3(BG_GRID), dim3(256), 0, st>>>(gstart, &ctx->d_mail->cls, part, lo, mid);
        k_cls_spine<<<dim3(1), dim3(BG_GRID), 0, st>>>(part, &ctx->d_mail->cls, bigoff);
        k_cls_apply<<<dim3(BG_GRID), dim3(256), 0, st>>>(gstart, &ctx->d_mail->cls, part, bigidx, bigoff, lo, mid);
    }
    DK_HIP(ctx, hipGetLastError());
    const Mail::Classes &c = ctx->h_mail->cls;
    DK_TRY(ctx->mail_read(&ctx->h_mail->cls));
    *out = GroupCounts{};
    out->active = c.rounds.active, out->groups = c.rounds.groups;
    out->giant = c.rounds.big_slots, out->giant_groups = c.rounds.big_groups, out->medium = c.medium_slots, out->medium_groups = c.medium_groups;
    out->big = out->giant + out->medium, out->big_groups = out->giant_groups + out->medium_groups;
    ctx->ws_release(mark);
    return DK_OK;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------
struct LfBuffers {
    uint64_t *k0, *k1;                          // big list keys (ping-pong)
    uint32_t *v0, *v1;                          // big list suffixes (ping-pong)
    uint32_t *bpos;                             // SA position of every big-list place
    uint8_t *bsym;                              // symbol in front, big list (unpacked from the sorted keys)
    uint32_t *l_idx, *l_pos, *l_gid;            // the active list (rewritten in place by every rerank: the old list has been consumed by then)
    uint8_t *l_sym;
    uint32_t *gstart, *bigidx, *bigoff;
    uint32_t *a_idx, *a_pos;                    // the arena of the deep groups: n members (every suffix leaves its list at most once)
    uint8_t *a_sym;
    uint32_t *gdepth, *bigdepth;                // depth of every group of the list (beside gstart) / of every big group (beside bigoff)
    uint8_t *bigper;                            // per big group: periodic through its depth (a round with tokens)
};
constexpr int LF_MAX_ROUNDS = 24;       // global-sort rounds of the big groups before the path gives up (each adds four or five symbols)
constexpr uint32_t LF_DEEP_CAP = 1u << 20;
constexpr uint32_t LF_GIANT_CAP = 1u << 12, LF_GIANT_ARENA = 1u << 18;  // subgroups / members the giant list holds
constexpr int LF_GIANT_ROUNDS = 4;  // a subgroup comes back from k_lf_lce, splits, and a part of it may have another giant extension (copies of copies)
constexpr int LF_DEEP_MAX = 4096;       // members of the biggest group the deep list takes (k_lf_deep_block<LF_DEEP_MAX, 1024>)
constexpr int LF_TAIL_SLOTS = 0;         // a big list this short (slots) would let its groups of up to LF_DEEP_MAX members end inside LDS (k_lf_medium) while the rounds go on for
                                         // the bigger ones.  Off: measured on 50 MB of real text with 512 K slots, seven rounds instead of fourteen and the same 10.5 ms -- k_lf_medium runs
                                         // sixteen steps of 26 us for its slowest group where a round of a short list costs 150-350 us for everybody (profiles/NOTES.md)
constexpr uint32_t LF_AVG_BIG = 1u << 18;  // big groups of more than this many members on average: periodic / run-dominated input, not text
// A limit as the kernels and the host compare against it: the tuning build may lower it (test hooks, DK_KNOB), clamped to [0, hi]
inline uint32_t lf_limit(int knob, uint32_t hi) { return knob <= 0 ? 0u : std::min(static_cast<uint32_t>(knob), hi); }

// Where the path starts from.  Either behind the initial sort (list == nullptr): its sorted keys with the shift of their compared bits, the bucket
// starts when the keys are narrow, and the suffix array the sort's last pass wrote.  Or taking over in the middle of the suffix-array path: its
// active list (every group of more than one member, equal in its first h0 symbols) is filtered down to the live groups (keys = the list's group
// ids) instead of the first rerank
struct LfFrom {
    const uint64_t *init_keys = nullptr; int key_shift = 0; const uint32_t *narrow_starts = nullptr, *d_sa = nullptr;  // behind the initial sort
    const uint32_t *idx = nullptr, *pos = nullptr, *gid = nullptr; uint8_t *sym = nullptr; size_t count = 0;          // a list handed over (idx != nullptr)
    uint32_t h0 = 0;  // symbols every group is known to be equal in
};
// Tokens (LfTokens): once, when the block has a dominant short period (period > 0: the probe saw at least one 64-byte window of it) and the caller
// has room for the next-break positions (next_break: n words) -- in the first round when the probes saw runs or periodic windows worth it
// (tokens_early: real text with its indentation and rulers; the groups inside runs are the biggest and the slowest to split on text, 17 rounds
// instead of 9 on 50 MB of it), else in the round after the first stalled one.  A round with tokens is a text round for every group that is not periodic.
struct LfTokenPlan { int period = 0; uint32_t *next_break = nullptr; bool tokens_early = false; };

// One run of the path: what its rounds and the passes at the end share
struct LfRun {
    dk_ctx *ctx; hipStream_t st; const uint8_t *d_text; size_t n; uint8_t *d_bwt; uint32_t *d_origin; LfTokenPlan plan; bool trace;
    LfBuffers b;  // (k0 / k1, v0 / v1 are swapped by the big list's sorts)
    size_t mark;  // of the workspace, released on every way out but an error's
    // lf_setup: the limits past which the path gives up, the knobs of its kernels, and its lists.  ls_max: groups above go the global way
    uint32_t deep_cap, giant_cap, giant_arena, ls_max, refork_groups;
    int giant_rounds, max_rounds, max_steps, stuck_steps, short_steps, medium_steps;
    size_t short_slots, tail_slots, fork_slots;
    bool two_classes, by_wave;
    LfDeepGroup *deep;
    LfArena arena;
    LfGiantOut giant[2];  // giant list (subgroups whose common extension is longer than a workgroup measures): two sets, one being read, one being filled
    uint32_t *lce_res;    // per member of the listed subgroups
    // progress
    GroupCounts c;       // of the active list: big = above big_min
    uint32_t h;          // depth of the groups that were not periodic
    int stalled;         // global-sort rounds in a row that left nearly all of their slots in big groups (runs of one symbol, periodic stretches)
    uint32_t big_min;    // groups above this go through the global sort; after a stalled round, or once the big list is short: LF_DEEP_MAX, what the deep list takes
    int ebits;
    bool tokens_done, want_tokens;
    bool pristine;       // nothing the suffix-array path reads (sorted keys, SA, L, origin) has been written yet
    bool forked;         // a pass over the deep list is running on the side stream
    uint32_t deep_done;  // entries [0, deep_done) of the list have been given to the early pass

    Mail::LFirst *d_lf() const { return &ctx->d_mail->lf; }  // the path's counters (mailbox.hpp says who writes which of them from which stream)
    const Mail::LFirst &lf() const { return ctx->h_mail->lf; }  // (valid behind every mail_read of the group)
};

// The limits, the knobs and the lists.  Expects the call's fields of r; leaves the deep list zeroed, the counters cleared, the giant lists allocated.
int lf_setup(LfRun &r) {
    const size_t n = r.n;
    // The limits past which the path gives up.  Tuning build (test hooks, tests/test_gpu_fallbacks.py): DK_LF_DEEP_CAP, DK_LF_ARENA, DK_LF_GIANT_CAP,
    // DK_LF_GIANT_ARENA, DK_LF_GIANT_ROUNDS and DK_LF_ROUNDS lower them.  They lower only what the kernels and the host compare against: every buffer
    // keeps its full size, so a site that forgets its check still writes inside its buffer (and the parity tests see the wrong L).
    r.deep_cap = lf_limit(DK_KNOB("DK_LF_DEEP_CAP", static_cast<int>(LF_DEEP_CAP)), LF_DEEP_CAP);
    const uint32_t arena_cap = lf_limit(DK_KNOB("DK_LF_ARENA", 0x7FFFFFFF), static_cast<uint32_t>(n));  // (every suffix leaves its list at most once)
    r.giant_cap = lf_limit(DK_KNOB("DK_LF_GIANT_CAP", static_cast<int>(LF_GIANT_CAP)), LF_GIANT_CAP);
    r.giant_arena = lf_limit(DK_KNOB("DK_LF_GIANT_ARENA", static_cast<int>(LF_GIANT_ARENA)), LF_GIANT_ARENA);
    r.giant_rounds = static_cast<int>(lf_limit(DK_KNOB("DK_LF_GIANT_ROUNDS", LF_GIANT_ROUNDS), LF_GIANT_ROUNDS));
    r.max_rounds = static_cast<int>(lf_limit(DK_KNOB("DK_LF_ROUNDS", LF_MAX_ROUNDS), LF_MAX_ROUNDS));
    r.mark = r.ctx->ws_mark();
    r.deep = r.ctx->ws_alloc<LfDeepGroup>(LF_DEEP_CAP);
    if (!r.deep) return DK_E_NOMEM;
    // The list starts out as zeros (flags 0, size 0): k_lf_medium walks it up to the CURRENT count while a pass on the side stream may be handing groups
    // on, so it meets entries that are reserved and not written yet, or half written.  What keeps it safe: the flags dword alone decides whether it
    // takes an entry (LD_LIST), and what writes entries beside it -- k_lf_deep_wave on the side stream (LD_HANDED), k_lf_medium's own workgroups
    // (flags 0) -- never stores LD_LIST: an entry in flight reads as not listed whatever the order of its stores, and no LD_LIST bits of an earlier
    // call are left.  Nothing relies on an entry being one 16-byte store.  (16 bytes per entry, at most about n entries: a few microseconds.)
    DK_HIP(r.ctx, hipMemsetAsync(r.deep, 0, std::min<size_t>(LF_DEEP_CAP, n + 4096) * sizeof(LfDeepGroup), r.st));
    // the path's counters, cleared before its first kernel
    DK_TRY(r.ctx->mail_fill(r.d_lf(), 0));
    r.arena = LfArena{r.b.a_idx, r.b.a_pos, r.b.a_sym, &r.d_lf()->arena_used, arena_cap};
    // steps a group may take inside k_lf_finish, and steps without a split after which it leaves early (tuning build: DK_LF_STEPS, DK_LF_STUCK)
    r.max_steps = std::max(1, std::min(4096, DK_KNOB("DK_LF_STEPS", LF_STEPS))), r.stuck_steps = std::max(1, DK_KNOB("DK_LF_STUCK", LF_STUCK));
    // (short lists: LF_SHORT_STEPS steps for lists of at most LF_SHORT_SLOTS slots; tuning build: DK_LF_SHORT_STEPS, DK_LF_SHORT_SLOTS, 0 slots = the same everywhere)
    r.short_steps = std::max(1, std::min(4096, DK_KNOB("DK_LF_SHORT_STEPS", LF_SHORT_STEPS)));
    r.short_slots = static_cast<size_t>(DK_KNOB("DK_LF_SHORT_SLOTS", static_cast<int>(LF_SHORT_SLOTS)));
    for (int q = 0; q < 2; ++q) {
        LfGiantOut &g = r.giant[q];
        g.list = r.ctx->ws_alloc<LfDeepGroup>(LF_GIANT_CAP);
        g.count = &r.d_lf()->giant_count[q];
        g.cap = r.giant_cap;
        g.idx = r.ctx->ws_alloc<uint32_t>(LF_GIANT_ARENA);
        g.pos = r.ctx->ws_alloc<uint32_t>(LF_GIANT_ARENA);
        g.sym = r.ctx->ws_alloc<uint8_t>(LF_GIANT_ARENA);
        g.used = &r.d_lf()->giant_used[q];
        g.arena_cap = r.giant_arena;
        if (!g.list || !g.idx || !g.pos || !g.sym) return DK_E_NOMEM;
    }
    r.lce_res = r.ctx->ws_alloc<uint32_t>(LF_GIANT_ARENA);
    if (!r.lce_res) return DK_E_NOMEM;
    r.ls_max = static_cast<uint32_t>(std::min(LFS_CAP, std::max(32, DK_KNOB("DK_LF_MAX", LFS_CAP))));
    // DK_LF_MEDIUM (tuning build; default on): the big list in two regions -- giant groups through the global sort, groups of up to 8192 members sorted
    // group by group inside LDS (classify_two_and_read)
    r.two_classes = DK_KNOB("DK_LF_MEDIUM", 1) != 0;
    // a short big list lets every group of up to LF_DEEP_MAX members go to k_lf_medium (tuning build: DK_LF_TAIL = slots of the big list from which on; 0: never)
    r.tail_slots = static_cast<size_t>(DK_KNOB("DK_LF_TAIL", LF_TAIL_SLOTS));
    r.medium_steps = std::max(1, std::min(4096, DK_KNOB("DK_LF_MEDIUM_STEPS", 16)));
    r.by_wave = DK_KNOB("DK_LF_WAVE", 1) != 0;
    r.fork_slots = static_cast<size_t>(DK_KNOB("DK_LF_FORK", 4 << 20));  // big-list size from which on the early pass may start (0: never)
    r.refork_groups = static_cast<uint32_t>(std::max(1, DK_KNOB("DK_LF_REFORK", 4096)));  // new deep groups from which on another early pass starts
    return DK_OK;
}

// classify the list the last rerank left, with the line of the big groups at `lo`
int lf_classify(LfRun &r, uint32_t lo) {
    if (!r.two_classes) return classify_and_read(r.ctx, 0, r.b.gstart, r.b.bigidx, r.b.bigoff, &r.c, lo);
    return classify_two_and_read(r.ctx, r.b.gstart, r.b.bigidx, r.b.bigoff, lo, &r.c);
}

// the big groups do not split on text (a stalled round), or the big list is short: its groups of up to LF_DEEP_MAX members leave it (the next
// k_lf_finish lists them, k_lf_medium takes them), the classification is done again with that line
int lf_let_medium_groups_go(LfRun &r, bool stalled_now) {
    if (!(stalled_now || (r.tail_slots && r.c.big <= r.tail_slots)) || r.c.big == 0 || r.big_min == static_cast<uint32_t>(LF_DEEP_MAX)) return DK_OK;
    r.big_min = LF_DEEP_MAX;
    DK_TRY(lf_classify(r, r.big_min));
    if (r.trace) {  // (the deep list's length: the next round lists the groups that left behind it -- tests/test_gpu_fallbacks.py caps the list there)
        uint32_t listed = 0;
        DK_HIP(r.ctx, hipMemcpyAsync(&listed, &r.d_lf()->deep_count, sizeof listed, hipMemcpyDeviceToHost, r.st));
        DK_HIP(r.ctx, hipStreamSynchronize(r.st));
        fprintf(stderr, "[dk] L-first: %s, groups up to %d members end inside LDS: big=%zu in %zu groups, deep list at %u\n", stalled_now ? "stalled round" : "short big list",
                LF_DEEP_MAX, r.c.big, r.c.big_groups, listed);
    }
    return DK_OK;
}

// order the deep groups [begin, end) of the list from the arena, on stream `on`: a wave per group of up to 64 members, then a workgroup per bigger
// (or handed-on) group.
// (last: the pass at the end -- its workgroup kernels read the list's length on the device, behind the wave kernel that has just handed groups on)
int lf_order_deep(LfRun &r, hipStream_t on, uint32_t begin, uint32_t end, bool last) {
    const LfArena &arena = r.arena;
    const uint32_t n32 = static_cast<uint32_t>(r.n);
    uint32_t *d_deep_count = &r.d_lf()->deep_count, *d_fallback = &r.d_lf()->fallback;
    const uint32_t *end_ptr = last ? d_deep_count : nullptr;
    if (r.by_wave) {
        LaunchScope ls(r.ctx, K_CHAIN, 0.0, on);
        k_lf_deep_wave<<<dim3(static_cast<unsigned>(std::min<size_t>(div_up(end - begin, 4), 4096))), dim3(256), 0, on>>>(arena.idx, arena.pos, arena.sym, r.deep, d_deep_count, begin, end, r.deep_cap,
                                                                                                                       r.d_text, n32, r.d_bwt, r.d_origin, d_fallback);
    }
    {
        LaunchScope ls(r.ctx, K_CHAIN, 0.0, on);
        k_lf_deep_block<LS_MAX, 256><<<dim3(1024), dim3(256), 0, on>>>(arena.idx, arena.pos, arena.sym, r.deep, end_ptr, begin, end, r.deep_cap, r.d_text, n32, r.d_bwt,
                                                                       r.d_origin, d_fallback, nullptr, r.giant[0], r.by_wave ? LDM_ARENA : LDM_ALL, 0u);
        k_lf_deep_block<LF_DEEP_MAX, 1024><<<dim3(256), dim3(1024), 0, on>>>(arena.idx, arena.pos, arena.sym, r.deep, end_ptr, begin, end, r.deep_cap, r.d_text, n32,
                                                                             r.d_bwt, r.d_origin, d_fallback, nullptr, r.giant[0], r.by_wave ? LDM_ARENA : LDM_ALL, static_cast<uint32_t>(LS_MAX));
    }
    DK_HIP(r.ctx, hipGetLastError());
    return DK_OK;
}

// One round: k_lf_finish takes every group of the list up to ls_max members to its end inside LDS (or to the deep list) and moves the bigger ones
// to the big list; that is sorted on its next four or five symbols (or tokens), reranked into the next list and classified.
// Expects the list and its counts; leaves the next ones -- or, when the list had no big group, nothing active: the rounds are over.
int lf_round(LfRun &r, int round) {
    LfBuffers &b = r.b;
    const size_t n = r.n, active = r.c.active, nbig = r.c.big;
    const int period = r.plan.period;
    uint32_t *const next_break = r.plan.next_break;
    uint32_t *d_deep_count = &r.d_lf()->deep_count, *d_fallback = &r.d_lf()->fallback, *d_deep_begin = &r.d_lf()->deep_begin;
    const int bsbits = r.c.big_groups > 1 ? static_cast<int>(ceil_log2_u64(r.c.big_groups)) : 1;
    const int tsym_big = std::max(1, std::min(5, (55 - bsbits) / 8));
    const int kb = 8 * tsym_big;
    const bool token_round = r.want_tokens && !r.tokens_done && nbig > 0 && kb >= 1 + r.ebits + 8;
    if (token_round) {  // next break of every position (2 n bytes read, 4 n written)
        const size_t mark = r.ctx->ws_mark();
        uint32_t *tile_first = r.ctx->ws_alloc<uint32_t>(div_up(n, PB_TILE));
        if (!tile_first) return DK_E_NOMEM;
        DK_TRY(enqueue_next_breaks(r.ctx, r.d_text, n, period, tile_first, next_break));
        {
            LaunchScope ls(r.ctx, K_PERIOD, 16.0 * r.c.groups);
            k_lf_periodic_groups<<<dim3(div_up(r.c.groups, 256)), dim3(256), 0, r.st>>>(b.gstart, b.gdepth, b.l_idx, b.bigidx, r.c.groups, r.big_min, next_break, period, static_cast<uint32_t>(n), b.bigper);
        }
        DK_HIP(r.ctx, hipGetLastError());
        r.ctx->ws_release(mark);
        r.ctx->stats.sa_route |= DK_ROUTE_PERIOD_ROUND;
    }
    const LfTokens tok{token_round ? next_break : nullptr, period, r.ebits, b.bigper};
    {
        LaunchScope ls(r.ctx, K_LF_FINISH, 13.0 * active + 64.0 * active + 17.0 * nbig);
        k_lf_finish<LFS_TILE, LFS_CAP, LFS_BLOCK><<<dim3(div_up(active, LFS_TILE)), dim3(LFS_BLOCK), 0, r.st>>>(b.l_idx, b.l_pos, b.l_gid, b.l_sym, b.gstart, b.bigidx, b.bigoff, active, r.d_text,
                                                                            static_cast<uint32_t>(n), b.gdepth, b.bigdepth, tok, kb, r.ls_max, r.big_min, b.k0, b.v0, b.bpos, r.d_bwt,
                                                                            r.d_origin, r.deep, d_deep_count, r.deep_cap, r.arena, d_fallback, active <= r.short_slots ? r.short_steps : r.max_steps, r.stuck_steps);
    }
    if (r.big_min != r.ls_max) {  // the groups the big list let go stand in the round's list: refined to their end inside LDS before the list is rewritten
        LaunchScope ls(r.ctx, K_CHAIN, 0.0);
        k_lf_medium<LF_DEEP_MAX / 8><<<dim3(1024), dim3(LF_DEEP_MAX / 8), 0, r.st>>>(b.l_idx, b.l_pos, b.l_sym, r.deep, d_deep_count, d_deep_begin, r.deep_cap, r.d_text, static_cast<uint32_t>(n), r.d_bwt,
                                                                        r.d_origin, r.arena, d_fallback, r.medium_steps, r.stuck_steps);
    }
    DK_HIP(r.ctx, hipMemcpyAsync(d_deep_begin, d_deep_count, sizeof(uint32_t), hipMemcpyDeviceToDevice, r.st));  // the next round's groups start here
    if (r.fork_slots) DK_TRY(r.ctx->mail_fetch(&r.ctx->h_mail->deep_seen, d_deep_count));  // (read behind the round's classification)
    DK_HIP(r.ctx, hipGetLastError());
    r.ctx->stats.rounds += 1;
    if (nbig == 0) {
        r.c.active = 0;  // (k_lf_finish has taken every group of the list: no next one)
        return DK_OK;
    }
    r.ctx->stats.sa_route |= DK_ROUTE_LFIRST_BIG_ROUND;
    if (r.two_classes) {  // (short lists too: the word-like block's last five rounds, each below 2^19 slots, 17.2 against 17.5 ms; the text block pays 0.05 ms for the second classification)
        const uint64_t *k_src = b.k0;  // where k_lf_finish (and k_lf_tokens) left the list
        const uint32_t *v_src = b.v0;
        const int gbits = r.c.giant_groups > 1 ? static_cast<int>(ceil_log2_u64(r.c.giant_groups)) : 1;  // the giant groups have the lowest dense indices
        DK_TRY(sort_pairs(r.ctx, b.k0, b.k1, b.v0, b.v1, r.c.giant, 8, 8 + kb + gbits));
        DK_TRY(sort_groups(r.ctx, k_src, v_src, b.k0, b.v0, b.bigoff + r.c.giant_groups, r.c.medium_groups, r.c.medium, r.big_min, 8, 8 + kb));
    } else {
        DK_TRY(sort_pairs(r.ctx, b.k0, b.k1, b.v0, b.v1, nbig, 8, 8 + kb + bsbits));
    }
    const size_t big_count = nbig;
    const LfDepthRule rule{b.gdepth, 0u, b.k0, 8 + kb, b.bigdepth, static_cast<uint32_t>(tsym_big), token_round ? next_break : nullptr, period, static_cast<uint32_t>(n), b.bigper};
    DK_TRY(lf_rerank(r.ctx, b.k0, 8, nullptr, b.bsym, 1, b.v0, nullptr, b.bpos, big_count, b.l_idx, b.l_pos, b.l_gid, b.l_sym, b.gstart, r.d_bwt, r.d_origin, rule));
    DK_TRY(lf_classify(r, r.big_min));
    if (token_round) {
        r.tokens_done = true;
        r.want_tokens = false;
        if (r.trace) fprintf(stderr, "[dk] L-first round %d: periodic groups (period %d) keyed by the tokens of their stretches' ends\n", round, period);
    }
    r.h += static_cast<uint32_t>(tsym_big);
    // The deep groups listed so far can be ordered BESIDE the rounds that follow: they need nothing from them (their members stand in the arena, their
    // places in L are theirs alone), and the rounds of a short big list leave the GPU nearly idle -- 50 MB of real text: 1.3 ms of deep work behind
    // ten rounds of a few hundred microseconds each.  One early pass on the context's side stream once the big list is short; what is listed later
    // (and what the early pass's wave kernel hands on) takes the pass at the end.
    if (const uint32_t seen = r.ctx->h_mail->deep_seen; r.fork_slots && r.c.big > 0 && r.c.big <= r.fork_slots && seen <= r.deep_cap && seen >= r.deep_done + (r.forked ? r.refork_groups : 1024u)) {
        // (the count was read behind this round's k_lf_finish and k_lf_medium: every entry below it is complete -- those of the rounds by that read,
        //  those an earlier pass on the side stream handed on by the stream's order.  Again whenever enough new groups have arrived.)
        const uint32_t from_entry = r.deep_done;
        r.deep_done = seen;
        DK_HIP(r.ctx, hipEventRecord(r.ctx->ev_fork, r.st));
        DK_HIP(r.ctx, hipStreamWaitEvent(r.ctx->side_stream, r.ctx->ev_fork, 0));
        DK_TRY(lf_order_deep(r, r.ctx->side_stream, from_entry, r.deep_done, false));
        DK_HIP(r.ctx, hipEventRecord(r.ctx->ev_join, r.ctx->side_stream));
        r.forked = true;
        if (r.trace) fprintf(stderr, "[dk] L-first: deep groups %u .. %u ordered beside the rounds\n", from_entry, r.deep_done);
    }
    r.stalled = r.c.big * 16 > big_count * 15 ? r.stalled + 1 : 0;
    if (r.stalled && !r.tokens_done) r.want_tokens = true;
    const uint32_t line_before = r.big_min;
    // (a stalled round with tokens still to come: the tokens first -- a run of 3000 zeros is placed by one token round where the arena's kernels walk
    //  3000 bytes per member: 6.7 against 8.0 ms for the 1e8-byte block around it)
    DK_TRY(lf_let_medium_groups_go(r, r.stalled != 0 && !(r.want_tokens && !r.tokens_done)));
    if (r.big_min != line_before) r.stalled = 0;  // (the groups that have just left may have been the ones that did not split: count anew)
    if (r.trace)
        fprintf(stderr, "[dk] L-first round %d: big list %zu sorted on %d+%d bits -> depth %u (groups that were not periodic) live=%zu groups=%zu big=%zu in %zu groups\n", round, big_count, bsbits, kb, r.h,
                r.c.active, r.c.groups, r.c.big, r.c.big_groups);
    return DK_OK;
}

// The passes at the end.  Expects the rounds over (nothing active); leaves L complete (L_COMPLETE) or the verdict that the path gave up (START_OVER).
int lf_last_passes(LfRun &r) {
    const Mail::LFirst &lf = r.lf();
    uint32_t *d_fallback = &r.d_lf()->fallback;
    const uint32_t n32 = static_cast<uint32_t>(r.n);
    // the deep groups of all rounds, from the arena: a wave per group of up to 64 members, then a workgroup per bigger (or handed-on) group -- what an
    // early pass beside the rounds (lf_round) has not taken already
    if (r.forked) DK_HIP(r.ctx, hipStreamWaitEvent(r.st, r.ctx->ev_join, 0));
    r.forked = false;
    DK_TRY(r.ctx->mail_read(&r.ctx->h_mail->lf));
    if (lf.deep_count > r.deep_done && lf.deep_count <= r.deep_cap && lf.fallback == 0) {
        if (r.trace) fprintf(stderr, "[dk] L-first: %u deep groups (%u of them ordered beside the rounds), %u members in the arena\n", lf.deep_count, r.deep_done, lf.arena_used);
        DK_TRY(lf_order_deep(r, r.st, r.deep_done, lf.deep_count, true));
    }
    // giant common extensions: measured by the whole grid, then the subgroup goes through k_lf_deep again (and may hand on a part of itself)
    DK_TRY(r.ctx->mail_read(&r.ctx->h_mail->lf));
    const bool any_giant = lf.giant_count[0] != 0 && lf.fallback == 0 && lf.deep_count <= r.deep_cap;
    if (r.trace && any_giant) fprintf(stderr, "[dk] L-first: %u subgroups with giant common extensions go through the grid-wide measure\n", lf.giant_count[0]);
    for (int g = 0; any_giant && g < r.giant_rounds; ++g) {
        const LfGiantOut &in = r.giant[g & 1];
        LfGiantOut out = r.giant[(g + 1) & 1];
        if (g + 1 == r.giant_rounds) out.cap = 0;  // what is still giant after the last round makes the path give up
        if (r.trace) {
            uint32_t listed = 0;
            DK_HIP(r.ctx, hipMemcpyAsync(&listed, in.count, sizeof listed, hipMemcpyDeviceToHost, r.st));
            DK_HIP(r.ctx, hipStreamSynchronize(r.st));
            if (listed) fprintf(stderr, "[dk] L-first: giant round %d: %u subgroups\n", g, listed);
        }
        DK_HIP(r.ctx, hipMemsetAsync(r.lce_res, 0xFF, static_cast<size_t>(LF_GIANT_ARENA) * sizeof(uint32_t), r.st));
        DK_HIP(r.ctx, hipMemsetAsync(out.count, 0, sizeof(uint32_t), r.st));
        DK_HIP(r.ctx, hipMemsetAsync(out.used, 0, sizeof(uint32_t), r.st));
        {
            LaunchScope ls(r.ctx, K_CHAIN, 0.0);
            k_lf_lce<<<dim3(1024), dim3(256), 0, r.st>>>(in.idx, in.list, in.count, in.cap, r.d_text, n32, r.lce_res);
            k_lf_deep_block<LS_MAX, 256><<<dim3(256), dim3(256), 0, r.st>>>(in.idx, in.pos, in.sym, in.list, in.count, 0u, 0u, in.cap, r.d_text, n32, r.d_bwt, r.d_origin,
                                                                          d_fallback, r.lce_res, out, LDM_ALL, 0u);
            k_lf_deep_block<LF_DEEP_MAX, 1024><<<dim3(64), dim3(1024), 0, r.st>>>(in.idx, in.pos, in.sym, in.list, in.count, 0u, 0u, in.cap, r.d_text, n32, r.d_bwt, r.d_origin,
                                                                                d_fallback, r.lce_res, out, LDM_ALL, static_cast<uint32_t>(LS_MAX));
        }
    }
    DK_HIP(r.ctx, hipGetLastError());
    DK_TRY(r.ctx->mail_read(&r.ctx->h_mail->lf));
    const uint32_t deep_total = lf.deep_count;
    // Giving up: a kernel found a list full (deep list, arena, giant list or its arena) or a common extension still giant after the last giant round
    // (the fallback word) -- or the deep list's count went past its cap where no kernel said so (the host skipped the pass at the end above, and
    // every group listed since the early pass would stay unordered).  No giant round at all (tuning build) leaves the giant list unordered too.
    const bool gave_up = lf.fallback != 0 || deep_total > r.deep_cap || (any_giant && r.giant_rounds == 0);
    if (any_giant) r.ctx->stats.sa_route |= DK_ROUTE_LFIRST_GIANT;
    if (r.trace)
        fprintf(stderr, "[dk] L-first: %u groups went the deep way%s\n", deep_total,
                gave_up ? "; a list overflowed (deep groups, arena, giant list) or a common extension stayed giant: back to the suffix-array path" : "");
    r.ctx->ws_release(r.mark);
    if (deep_total) r.ctx->stats.sa_route |= DK_ROUTE_LFIRST_DEEP;
    return gave_up ? START_OVER : L_COMPLETE;
}

// whatever way the path is left, the side stream's work is over before the caller goes on (the suffix-array path reuses every buffer)
struct LfJoinSide {
    dk_ctx *c; const bool *forked;
    ~LfJoinSide() { if (*forked) (void)hipStreamSynchronize(c->side_stream); }
};

// The L-first path.  -> L_COMPLETE: L and the origin are complete.  Otherwise the caller takes the suffix-array path: WENT_ON: from where it stands
// (nothing it needs was touched but scratch buffers -- only when starting behind the initial sort); START_OVER: from the start (L and the origin
// word are rewritten by it).  Or an error.  force: go on even where the big groups hold most of the list (test hook; taking over a list)
int lfirst_path(dk_ctx *ctx, const uint8_t *d_text, size_t n, uint8_t *d_bwt, uint32_t *d_origin, const LfBuffers &buffers, const LfFrom &from, const LfTokenPlan &plan, bool trace,
                bool force) {
    LfRun r{};
    r.ctx = ctx, r.st = ctx->stream, r.d_text = d_text, r.n = n, r.d_bwt = d_bwt, r.d_origin = d_origin, r.b = buffers, r.plan = plan, r.trace = trace;
    const LfBuffers &b = r.b;
    const LfJoinSide join_side{ctx, &r.forked};
    DK_TRY(lf_setup(r));
    // first rerank: slot a is SA position a, L[a] is the symbol in front of the suffix standing there; every group is known to h0 symbols
    // (the table is filled below, once the path is sure to go on: it lies in the initial keys' buffer, which the suffix-array path reads again when it
    //  takes over from here -- "pristine")
    const uint32_t h0 = from.h0;
    const LfDepthRule first_rule{nullptr, h0, nullptr, 0, nullptr, 0u, nullptr, 0, static_cast<uint32_t>(n), nullptr};
    if (from.idx) {
        DK_TRY(lf_rerank(ctx, reinterpret_cast<const uint64_t *>(from.gid), 0, nullptr, from.sym, 0, from.idx, nullptr, from.pos, from.count, b.l_idx, b.l_pos, b.l_gid,
                         b.l_sym, b.gstart, d_bwt, d_origin, first_rule, true));
    } else {
        DK_TRY(lf_rerank(ctx, from.init_keys, from.key_shift, from.narrow_starts, d_bwt, 0, from.d_sa, d_origin, nullptr, n, b.l_idx, b.l_pos, b.l_gid, b.l_sym, b.gstart, d_bwt, d_origin, first_rule));
    }
    r.pristine = !from.idx;  // (taking over: finals of the filter have written L; the caller's group table has been rewritten)
    DK_TRY(lf_classify(r, r.ls_max));
    r.h = h0;
    if (trace)
        fprintf(stderr, "[dk] L-first: %s (%u symbols) live=%zu groups=%zu big=%zu in %zu groups\n", from.idx ? "taking over a list" : "after the initial sort", h0, r.c.active, r.c.groups,
                r.c.big, r.c.big_groups);
    // Big groups are refined four or five symbols per global sort where prefix doubling doubles.  Measured at 1e8 bytes (share of the live slots
    // in groups above 256 after the first rerank -> this way / the other): Markov text 0.5 % 6.4 / 10.0 ms; half Markov, half Zipf words 50 %
    // 13.2 / 16.6; Zipf words over 28 symbols 72 % 15.0 / 17.7; over 182 symbols, 2 M words 83 % 17.8 / 18.8; 200 K words 74 % (the most
    // frequent word 14 % of all) 20.5 / 20.7 -- never behind while the groups split on text at all.  Above 85 % the other way (nothing has
    // been written yet, the suffix-array path goes on from the same sorted keys).
    if (r.c.big * 100 > r.c.active * 85 && !force) {
        if (trace) fprintf(stderr, "[dk] L-first: %zu of %zu live slots in big groups: the suffix-array path goes on from here\n", r.c.big, r.c.active);
        ctx->ws_release(r.mark);
        return r.pristine ? WENT_ON : START_OVER;
    }
    r.pristine = false;
    DK_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(b.gdepth), static_cast<int>(h0), r.c.groups + 1, r.st));
    r.big_min = r.ls_max;
    r.ebits = static_cast<int>(ceil_log2_u64(static_cast<uint64_t>(n) + 1));
    r.tokens_done = plan.period <= 0 || !plan.next_break || static_cast<uint32_t>(plan.period) > h0;
    r.want_tokens = !r.tokens_done && plan.tokens_early;
    DK_TRY(lf_let_medium_groups_go(r, false));
    for (int round = 0; r.c.active > 0; ++round) {
        if (r.c.big > 0 && (round >= r.max_rounds || r.c.big / r.c.big_groups > LF_AVG_BIG || r.stalled >= 2)) {
            if (trace)
                fprintf(stderr, "[dk] L-first: %s (%zu slots in %zu groups, round %d): back to the suffix-array path\n",
                        round >= r.max_rounds ? "round limit" : r.stalled >= 2 ? "two stalled rounds" : "giant groups", r.c.big, r.c.big_groups, round);
            ctx->ws_release(r.mark);
            return START_OVER;
        }
        if (trace && DK_KNOB("DK_LF_SIZES", 0) != 0 && r.c.big > 0) {  // (debug: how the big list's slots spread over group sizes)
            GroupCounts above;
            for (uint32_t line : {1024u, 4096u, 8192u, 32768u, 1u << 20}) {
                DK_TRY(classify_and_read(ctx, 0, b.gstart, b.bigidx, b.bigoff, &above, line));
                fprintf(stderr, "[dk]    groups above %u members: %zu slots in %zu groups\n", line, above.big, above.big_groups);
            }
            DK_TRY(lf_classify(r, r.big_min));
        }
        DK_TRY(lf_round(r, round));
    }
    return lf_last_passes(r);
}
