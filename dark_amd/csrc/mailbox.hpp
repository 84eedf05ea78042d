// dk::Mail: the words through which the device stages report their small results to the host.  dk_ctx holds two of them, d_mail (device) and h_mail
// (pinned host); dk_ctx::mail_read / mail_fetch copy a member or a group of d_mail to its twin in h_mail, dk_ctx::mail_fill fills one of d_mail.
// THIS HEADER IS THE MAP: every word has one purpose and one place, and its comment says who writes it and who reads it.  Unless a comment says
// otherwise, the writers are kernels and fills on ctx->stream, and the host reads the twin in h_mail behind a copy and a synchronise on that stream.
// Two stages of one call never overlap (every API call runs its stages one after another on ctx->stream); what does run beside the main stream is the
// L-first path's early pass over the deep groups on ctx->side_stream, between ev_fork and ev_join: the words it touches say so.
// NO WORD LIVES FROM ONE CALL TO THE NEXT.  A word that a stage reads (on the device or on the host) has been stored by a kernel or filled on
// ctx->stream by that same stage in that same call: "cleared before" / "filled before" below is a mail_fill in the stage's host code, "k_x:" a
// plain store that the kernel makes on every launch.  dk_dbg_mail_fill therefore fills the whole struct, both twins, with any byte between two
// calls, and tests/test_gpu_poison_stages.py and tests/test_gpu_call_sequences.py run every stage behind such a fill (0x00, 0xA5, 0xFF).
#pragma once
#include <cstdint>

namespace dk {

constexpr int PP_MAX_CAND = 4;   // candidate prefix lengths of the prefix probe (k_prefix_probe)
constexpr int PS_SAMPLES = 32;   // sample positions of the long-period search (k_period_search)
constexpr int LIVE_RING = 8;     // in-place rounds in flight: live counters and their events (dk_ctx::round_ev); a power of two

struct Mail {
    // ---- suffix sort: what a rerank and the classification behind it leave, read back once per round -------------------------------------------
    struct Rounds {               // classify_and_read copies this group
        uint32_t active;          // k_rerank_scan (rerank, lf_rerank): slots of the new list; read on the device by k_rerank_apply_first
        uint32_t groups;          // k_rerank_scan: groups of the new list; read on the device by k_big_* / k_cls_* (the host does not know it yet)
        uint32_t big_slots;       // k_big_spine / k_cls_spine: slots in big groups (two classes: in giant groups); also read by k_big_apply
        uint32_t above_pl_slots;  // k_big_reduce (atomicAdd; classify_and_read clears it first): slots in groups of more than PL_MAX members
        uint32_t big_groups;      // k_big_spine / k_cls_spine: big groups (two classes: giant groups)
    };
    struct Classes {              // classify_two_and_read copies this group; k_cls_* take it
        Rounds rounds;
        alignas(8) uint32_t medium_slots;  // k_cls_spine: slots in groups of the medium class ...
        uint32_t medium_groups;            // ... and their number
    } cls;

    // ---- BWT origin ---------------------------------------------------------------------------------------------------------------------------
    // bwt_forward_device / bwt_gather_device fill it with 0xFF; the one kernel that places suffix 0 stores its slot: a sort's last pass, a rerank,
    // k_lf_finish / k_lf_medium / k_plateau_sort / k_chain_apply / k_bwt_gather on ctx->stream -- or k_lf_deep_wave / k_lf_deep_block, which also run
    // on side_stream (between ev_fork and ev_join; lfirst_path leaves only once the side stream has joined or drained).  The host reads it at the end.
    uint32_t origin;

    // ---- suffix sort: alphabet and probes -----------------------------------------------------------------------------------------------------
    struct Alphabet {             // suffix_array_impl clears and reads the group as one; the host keeps reading its twin for the whole sort
        uint32_t hist[256];       // k_sym_hist: occurrences of every byte value
        uint32_t run_probe[2];    // k_run_probe: [0] a run of 511 bytes exists, [1] 16-byte pieces inside runs
        uint32_t period_probe[8]; // k_period_probe: 64-byte windows that follow period q, at [q - 1]
    } alphabet;
    uint8_t code[256];            // device only: dense symbol codes, uploaded by suffix_array_impl from its own table; read by the text-key kernels
    uint8_t inv[256];             // code -> byte value, for the sorts that write L.  Host twin: the pinned staging the upload to the device twin reads
    uint32_t dups[PP_MAX_CAND];   // k_prefix_probe (cleared by the host before): equal pairs in the sample per candidate prefix length
    uint32_t found[PS_SAMPLES];   // k_period_search (filled with 0xFF before): the period every sample position found, 0xFFFFFFFF: none
    uint32_t found_windows;       // k_period_count (cleared before): 64-byte windows that follow the period most samples voted for
    uint32_t narrow_starts[256];  // device only: bucket starts of a narrow-key sort (SortFinalOut::bucket_starts), written by the sort's last pass,
                                  // read by the first rerank's reduce kernel (the host twin: only dk_dbg_dev_initial_sort fetches them)
    uint32_t chain_cnt[2];        // pair chains: k_chain_extract [0] records, [1] first reservation that did not fit (host: 0 / 0xFF fills before);
                                  // then k_plateau_scan [0]: slots still live behind the chains
    uint32_t live_ring[LIVE_RING];  // in-place rounds: round r clears and counts its live slots at [r % LIVE_RING] (k_plateau_sort) and the round behind
                                    // it reads that on the device; [0] also takes k_plateau_scan's count in compact().  The copy to the twin is
                                    // enqueued behind every round (mail_fetch) and read one round late, behind round_ev[r % LIVE_RING]

    // ---- L-first path (lfirst_path clears the group on ctx->stream before its first kernel; the side stream is idle then) -----------------------
    struct LFirst {               // read back as one group, on ctx->stream, only behind the join (hipStreamWaitEvent(stream, ev_join)) and a synchronise
        uint32_t deep_count;      // entries of the deep list.  atomicAdd by k_lf_finish / k_lf_medium (ctx->stream) and by k_lf_deep_wave handing a group
                                  // on (either stream; on side_stream between ev_fork and ev_join).  Read on the device by k_lf_medium (walks the list
                                  // up to the CURRENT count: see the list's fill in lfirst_path) and by the last pass's k_lf_deep_block (behind the join)
        uint32_t fallback;        // any kernel of the path, either stream: stores 1 when a list or an arena is full (never cleared inside a call: racing
                                  // stores all write 1).  Host: read at the end only
        uint32_t deep_begin;      // ctx->stream only: device-to-device copy of deep_count behind every round; k_lf_medium starts at it
        uint32_t giant_count[2];  // subgroups on the two giant lists.  [0]: atomicAdd by k_lf_deep_block of order_deep (either stream, as deep_count);
        uint32_t giant_used[2];   // members in their arenas.            [1] and the re-cleared [0]: the giant rounds at the end, ctx->stream only
        uint32_t arena_used;      // members in the deep groups' arena: atomicAdd by k_lf_finish / k_lf_medium, ctx->stream only
    } lf;
    // host only: deep_count as it stood behind a round's k_lf_finish / k_lf_medium.  The copy is enqueued on ctx->stream (mail_fetch) and valid after the
    // synchronise of the round's classification.  Every entry below it is complete for the early pass that takes [deep_done, deep_seen) on side_stream:
    // the rounds' entries by the copy's place in ctx->stream and ev_fork, those an earlier pass handed on by side_stream's own order.
    uint32_t deep_seen;

    // ---- inverse BWT --------------------------------------------------------------------------------------------------------------------------
    uint32_t ibwt_pending;        // k_ibwt_jump's last step (cleared before it; the earlier steps' stores are wiped by that fill): chains still unresolved, i.e. a cycle
    uint32_t ibwt_bad;            // k_ibwt_emit / k_ibwt_copy (cleared before): the walk did not cover the text once

    // ---- DC stage -----------------------------------------------------------------------------------------------------------------------------
    uint32_t dc_runs;             // k_dc_runscan: runs of L; read on the device by k_dc_main
    uint32_t dc_init[256];        // host only: landing area of the DC init table (the device table is workspace)

    // ---- packed paths (many small blocks in one pass) -----------------------------------------------------------------------------------------
    struct Packed {
        uint32_t live;            // k_pk_codes: symbols in use; then k_pk_spine, once per round: suffixes still live (plain stores, read back behind each)
        uint32_t dc_runs;         // host only: landing area of the pack's run count (d_rb[count], workspace)
        uint32_t ibwt_bad;        // k_pib_check, then k_pib_copy / k_pib_emit (filled with 0xFF before the first): lowest corrupt block, IB_END: none
        uint32_t ibwt_pending;    // device only: k_ibwt_jump's counter in the packed inverse and the FM structure builds (k_pib_check decides instead;
                                  // never cleared, and nobody reads it)
    } packed;

    // ---- LCP arrays (lcp.hip; lcp_device clears the group before its first kernel and reads it back as one, once per pass over the lists) -------
    struct Lcp {
        uint32_t bad_sa;          // k_lcp_phi: stores 1 for a suffix-array entry outside its block (racing stores all write 1).  Host: DK_E_ARG
        struct Lists {            // cleared again by lcp_device before every further pass
            uint32_t long_count;  // k_lcp_measure (atomicAdd): positions still equal at the lane's cap, listed or not (a full list: the excess says
                                  // "run again"); read on the device by k_lcp_wave, which walks min(long_count, capacity) entries
            uint32_t giant_count; // k_lcp_wave (atomicAdd): positions still equal at the wave's cap, as above; the host sizes k_lcp_giant's walk by it
        } lists;
    } lcp;

    // ---- FM-index find (fm_index.hip: fm_find_device) ---------------------------------------------------------------------------------------------
    struct FmFind {
        alignas(8) uint64_t total;  // k_fm_find_scan_b: the hits of all pairs together (a plain store on every launch); the host reads it behind the scan
        uint64_t near_cut;          // fm_near_device only: k_fm_find_scan_b over the pairs' cut flags (the same plain store, a launch of its own in
                                    // every call): the pairs that stopped at the node limit; the host reads it with `total`, as one group
    } fm_find;

    // ---- super-maximal matches on the suffix array (sa_query.hip: sa_smems_device) -------------------------------------------------------------------
    struct SaMatch {
        alignas(8) uint64_t total;  // k_sa_smem_scan_b: the flagged positions of all queries together (a plain store on every launch); the host reads
                                    // it behind the scan
    } sa_match;
};
static_assert(sizeof(Mail) <= 4096, "the mailbox is one page");
static_assert((LIVE_RING & (LIVE_RING - 1)) == 0, "rounds index the ring with a mask");

}  // namespace dk
