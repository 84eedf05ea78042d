"""The second mode of execution of every device stage: dk_set_profiling(ctx, 1).  Every quoted per-kernel number rests on it (bench.py --full,
tools/*_throughput.py, tools/kernel_breakdown.py, the kernel figures of DESIGN.md and profiles/), and it changes what runs: the LCP kernels
take a counter array and with it paths of their own (csrc/lcp.hip: wave_sum over the wave in k_lcp_measure, lcp_count in all three), lcp_device
takes 4 KiB more of the workspace, every launch is bracketed by a pair of pooled events (LaunchScope, prof_begin / prof_end / prof_collect in
csrc/context.cpp) and every entry and every dk_batch_push ends with one more wait.

  a  test_same_answers                every one of the twelve ops of test_gpu_call_sequences.build_ops gives its model's result with profiling on
  b  test_closed_accounting           per op: names of kernel_slot_name, finite times, and a second run adds exactly the first run's launches and bytes;
     test_profiling_off_counts_nothing
  c  test_launch_table_*              the launches per slot where the host driver fixes them: both inverses, the DC encode, one LCP call per route
  d  test_time_sanity                 no slot's time above the call's wall time, the sum at most streams x wall; the L-first route with its side stream
  e  test_no_carry_over*              behind every op, every refused call and every batch form, a small op reports what it reports on a fresh context
  f  test_batch_*                     batches under profiling: the single calls' streams, and the sums of their launches and bytes
  g  test_lcp_counters_*              the LCP array, the routes and the two counters of dk_stats against tests/lcp_count_model.py, every entry form;
     test_lcp_counters_tuning_build   lowered caps in a process of its own: a text of a few kilobytes through all three kernels' counting paths
  h  test_exact_capacity_*            contexts created for exactly their input, profiling on: the counters' 4 KiB must fit

All inputs are small; the models come from the CPU modules the other GPU tests use."""
import json
import math
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import dark_amd
import lcp_count_model as CM
from conftest import ROOT
from dark_amd import datagen
from dark_amd._lib import DK_E_ARG, NUM_KERNEL_SLOTS
from lcp_model import lcp_kasai
from test_gpu_call_sequences import build_ops, dev, error_of, host32, u8, words
from test_gpu_lcp import TIMEOUT, TUNING_LIB, Words, dev_text, gpu_sa, planted, run_pack

pytestmark = pytest.mark.gpu
CAP = 1 << 19


@pytest.fixture(scope="module")
def ops(orc):
    return build_ops(orc)


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    c.set_profiling(True)
    yield c
    c.close()


def profiled(n=CAP, **kw):
    c = dark_amd.Context(n, **kw)
    c.set_profiling(True)
    return c


def slot_names(ctx):
    return {ctx._lib.dk_kernel_name(i).decode() for i in range(NUM_KERNEL_SLOTS)}


def counts(kernels):
    """what must repeat from run to run: launches and algorithmic bytes per slot (the times do not)"""
    return {k: (v["launches"], v["bytes"]) for k, v in kernels.items()}


def launches(kernels):
    return {k: v["launches"] for k, v in kernels.items()}


def minus(after, before):
    out = {}
    for k, (n, b) in after.items():
        n0, b0 = before.get(k, (0, 0.0))
        if n != n0 or b != b0:
            out[k] = (n - n0, b - b0)
    return out


def ceil_log2(v):
    return (v - 1).bit_length()


# ---- a. same answers -------------------------------------------------------------------------------------------------------------------------------

def test_same_answers(ctx, ops):
    assert len(ops) == 12
    wrong = []
    for name in sorted(ops):
        call, want = ops[name]
        if call(ctx) != want:
            wrong.append(name)
        st = ctx.stats()
        assert 0 <= st["ws_peak_bytes"] <= st["ws_size_bytes"], (name, st)
    assert not wrong, "with profiling on these differ from their model: %s" % wrong
    ctx.set_profiling(False)
    try:
        assert all(call(ctx) == want for call, want in ops.values())  # (and the switch back: the same context, the same answers)
    finally:
        ctx.set_profiling(True)


# ---- b. closed accounting --------------------------------------------------------------------------------------------------------------------------

def test_closed_accounting(ctx, ops):
    """Per op: stats_reset, one run, read; a second run of the same input on top.  No stage's launch count may differ between two runs of one
    input: the suffix sort's rounds, the lists' lengths and the pass counts are functions of the input (atomics decide only the ORDER of list
    entries), so everything is asserted for all twelve."""
    names = slot_names(ctx)
    assert len(names) == NUM_KERNEL_SLOTS and ctx._lib.dk_kernel_name(NUM_KERNEL_SLOTS) is None
    for name in sorted(ops):
        call, want = ops[name]
        ctx.stats_reset()
        assert ctx.stats()["kernels"] == {}
        assert call(ctx) == want, name
        first = ctx.stats()["kernels"]
        assert first, name + ": nothing was bracketed"
        assert set(first) <= names, (name, sorted(set(first) - names))
        for slot, v in first.items():
            assert v["launches"] >= 1 and math.isfinite(v["ms"]) and v["ms"] >= 0 and math.isfinite(v["bytes"]) and v["bytes"] >= 0, (name, slot, v)
        assert call(ctx) == want, name
        second = ctx.stats()["kernels"]
        assert minus(counts(second), counts(first)) == counts(first), (name, counts(first), counts(second))
        for slot, v in second.items():
            assert math.isfinite(v["ms"]) and v["ms"] >= first[slot]["ms"], (name, slot, v, first[slot])


def test_profiling_off_counts_nothing(ops):
    with dark_amd.Context(CAP) as plain:
        for name in sorted(ops):
            call, want = ops[name]
            plain.stats_reset()
            assert call(plain) == want, name
            st = plain.stats()
            assert st["kernels"] == {} and st["lcp_measured"] == 0 and st["lcp_bytes_compared"] == 0, (name, st)
        # on, then off again: the LCP counters are the LAST pass's, so an unprofiled pass puts them back to 0
        plain.set_profiling(True)
        assert ops["lcp"][0](plain) == ops["lcp"][1]
        st = plain.stats()
        assert st["lcp_measured"] > 0 and st["lcp_bytes_compared"] > 0 and st["kernels"]
        plain.set_profiling(False)
        plain.stats_reset()
        assert ops["lcp"][0](plain) == ops["lcp"][1]
        st = plain.stats()
        assert st["kernels"] == {} and st["lcp_measured"] == 0 and st["lcp_bytes_compared"] == 0 and st["lcp_passes"] == 1, st


# ---- c. launch tables ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5000, 65535, 65536, 70001])
def test_launch_table_single_inverse(ctx, orc, n):
    """bwt_inverse_device: one bracket each for the table (k_ibwt_hist and its scans), k_ibwt_lf, k_ibwt_walk and the emit; pointer jumping takes
    ceil_log2(nsplit) + 1 brackets, nsplit = ceil(n / S) + (origin % S != 0), S = 8 below 2^16 and 64 from there on"""
    t = u8(datagen.wiki_like(n, seed=n))
    L, origin = orc.bwt_forward(t)
    S = 8 if n < (1 << 16) else 64
    nsplit = -(-n // S) + (1 if origin % S else 0)
    d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.stats_reset()
    ctx.dev_bwt_inverse(dev(L), n, origin, d_out)
    assert d_out.cpu().numpy().tobytes() == t.tobytes()
    assert launches(ctx.stats()["kernels"]) == {"k_ibwt_hist": 1, "k_ibwt_lf": 1, "k_ibwt_walk": 1, "k_ibwt_jump": ceil_log2(nsplit) + 1, "k_ibwt_emit": 1}
    ctx.stats_reset()
    assert ctx.bwt_inverse(L, origin).tobytes() == t.tobytes()  # the host form: the same driver
    assert launches(ctx.stats()["kernels"])["k_ibwt_jump"] == ceil_log2(nsplit) + 1


def test_launch_table_origin_on_a_splitter(ctx, orc):
    """the + 1 of nsplit decides the count at n = 4096, S = 8: 512 splitters and 10 jumps with the origin on a splitter, 513 and 11 off it"""
    n, found = 4096, {}
    for seed in range(200):
        t = u8(datagen.wiki_like(n, seed=seed))
        L, origin = orc.bwt_forward(t)
        found.setdefault(origin % 8 == 0, (t, L, origin))
        if len(found) == 2:
            break
    assert len(found) == 2
    d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    for on_splitter, (t, L, origin) in found.items():
        ctx.stats_reset()
        ctx.dev_bwt_inverse(dev(L), n, origin, d_out)
        assert d_out.cpu().numpy().tobytes() == t.tobytes()
        assert launches(ctx.stats()["kernels"])["k_ibwt_jump"] == (10 if on_splitter else 11), origin


def test_launch_table_packed_inverse(ctx, orc):
    """packed_ibwt_device: S = 64; the jumps follow the LARGEST block's splitter count, and k_pib_check's bracket is in the same slot"""
    rng = np.random.default_rng(3)
    for sizes in ([1, 2, 3, 17, 4097, 300, 9001], [64, 128], [1], [70001, 5]):
        blocks = [rng.integers(97, 101, size=k, dtype=np.uint8) for k in sizes]
        pairs = [orc.bwt_forward(b, orc.sa_naive(b) if len(b) < 64 else None) for b in blocks]
        origins = [int(p[1]) for p in pairs]
        max_split = max(-(-k // 64) + (1 if o % 64 else 0) for k, o in zip(sizes, origins))
        d_out = torch.empty(sum(sizes), dtype=torch.uint8, device="cuda")
        ctx.stats_reset()
        ctx.dev_bwt_inverse_packed(dev(np.concatenate([p[0] for p in pairs])), sizes, origins, d_out)
        assert d_out.cpu().numpy().tobytes() == np.concatenate(blocks).tobytes()
        assert launches(ctx.stats()["kernels"]) == {"k_ibwt_hist": 1, "k_ibwt_lf": 1, "k_ibwt_walk": 1, "k_ibwt_jump": ceil_log2(max_split) + 1 + 1,
                                                    "k_ibwt_emit": 1}, sizes


@pytest.mark.parametrize("n", [11, 4096, 100001])
def test_launch_table_dc_encode(ctx, orc, n):
    """dc_encode_device: four brackets whatever n -- the summary, the carries (k_dc_runscan and the three carry kernels in one), the main pass, init"""
    t = u8(datagen.wiki_like(n, seed=n))
    L, _ = orc.bwt_forward(t, orc.sa_naive(t) if n < 64 else None)
    want = orc.dc_encode(L)
    m = len(want["d"])
    d_dist, d_sym = words(n), torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.stats_reset()
    init, got_m = ctx.dev_dc_encode(dev(L), n, d_dist, d_sym)
    assert got_m == m and np.array_equal(host32(d_dist)[:m], np.asarray(want["d"], np.uint32)) and np.array_equal(init, np.asarray(want["init"], np.uint32))
    k = ctx.stats()["kernels"]
    assert launches(k) == {"k_dc_summary": 1, "k_dc_carry": 1, "k_dc_main": 1, "k_dc_init": 1}
    ntiles = round((k["k_dc_carry"]["bytes"]) / (3.0 * 2048.0))
    assert k["k_dc_summary"]["bytes"] == k["k_dc_main"]["bytes"] == 1.0 * n + 2048.0 * ntiles and k["k_dc_init"]["bytes"] == 2048.0


@pytest.mark.parametrize("length,giant", [(100, False), (300, False), (70000, True)])
def test_launch_table_lcp(ctx, length, giant):
    """lcp_device on a given suffix array, one pass: k_lcp_phi and k_lcp_gather in k_bwt_gather; k_lcp_measure and k_lcp_wave in k_chain (the wave
    kernel is launched whether or not anything was listed -- the count is on the device) and k_lcp_giant with them when something reached the
    grid; tile sums, spine and fill in the three rerank slots"""
    t = planted(length, seed=length)
    n = len(t)
    sa = gpu_sa(ctx, t)
    out = Words(n)
    ctx.stats_reset()
    ctx.dev_lcp(dev_text(t), n, sa.t, out.t)
    st = ctx.stats()
    assert np.array_equal(out.host(), lcp_kasai(t, sa.host())) and out.guards_intact()
    assert st["lcp_passes"] == 1 and ("lcp_giant" in st["routes"]) == giant and ("lcp_long" in st["routes"]) == (length >= CM.LANE_CAP)
    assert launches(st["kernels"]) == {"k_bwt_gather": 2, "k_chain": 3 if giant else 2, "k_rerank_reduce": 1, "k_rerank_scan": 1, "k_rerank_apply": 1}
    assert st["kernels"]["k_bwt_gather"]["bytes"] == 24.0 * n and st["kernels"]["k_chain"]["bytes"] == 10.0 * n


# ---- d. time sanity --------------------------------------------------------------------------------------------------------------------------------

def timed(ctx, call):
    ctx.stats_reset()
    t0 = time.perf_counter()
    got = call(ctx)
    wall_ms = 1e3 * (time.perf_counter() - t0)
    return got, wall_ms, ctx.stats()


def check_times(name, wall_ms, st, streams):
    k = st["kernels"]
    assert k, name
    for slot, v in k.items():
        assert math.isfinite(v["ms"]) and 0 <= v["ms"] <= wall_ms, "%s: %s took %.3f ms of a call of %.3f ms" % (name, slot, v["ms"], wall_ms)
    total = sum(v["ms"] for v in k.values())
    assert total <= streams * wall_ms, "%s: %.3f ms of kernels in a call of %.3f ms on %d stream(s)" % (name, total, wall_ms, streams)


def test_time_sanity(ctx, ops, orc):
    """A structural bound, no measurement: every entry returns synchronised while profiling, its brackets follow one another on their stream, so
    all of them lie inside the call.  A bracket closed with a stale event (csrc/context.cpp: the pool restarts at 0 behind every collect) ends
    in another call: its time is negative or as long as the time between the two calls.  Every op runs behind a DIFFERENT op here, so that the
    events of the pool were last recorded by other brackets.

    The L-first route (dev_bwt_forward of word-like text) orders its deep groups on side_stream beside the rounds once 1024 of them are listed
    while the big list is not yet empty (lfirst.inc, lf_round): twice the wall time bounds the sum then.  dk_stats does not say whether the
    early pass forked; the tuning build's DK_TRACE does, for these two texts: at 70 000 bytes 1011 deep groups, none ordered beside the
    rounds (no fork); at 2^20 bytes three forks, 17 836 of 18 180 deep groups ordered on the side stream.  Both run here, the second on a
    context of its own size."""
    for name in sorted(ops) + sorted(ops)[::-1]:
        call, want = ops[name]
        got, wall_ms, st = timed(ctx, call)
        assert got == want, name
        check_times(name, wall_ms, st, 1)
    for n in (70000, 1 << 20):
        t = u8(datagen.word_like(n, seed=3, vocab=2000))
        assert len(t) == n
        want = orc.bwt_forward(t)
        d_in, d_bwt = dev(t), torch.empty(n, dtype=torch.uint8, device="cuda")
        with profiled(n) as big:
            for again in range(2):  # (the second run finds every event of the pool recorded by the first)
                origin, wall_ms, st = timed(big, lambda c: c.dev_bwt_forward(d_in, n, d_bwt))
                assert {"lfirst", "lfirst_deep"} <= st["routes"], st["routes"]
                assert origin == int(want[1]) and d_bwt.cpu().numpy().tobytes() == want[0].tobytes()
                check_times("dev_bwt_forward of %d bytes, L-first" % n, wall_ms, st, 2)
                if again:
                    assert counts(st["kernels"]) == first, (n, first, counts(st["kernels"]))
                first = counts(st["kernels"])


# ---- e. no carry-over ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_op(ops):
    """op B (the DC encode of eleven bytes) and what a fresh context reports for it alone"""
    call, want = ops["dc_encode"]
    with profiled(CAP) as fresh:
        fresh.stats_reset()
        assert call(fresh) == want
        alone = counts(fresh.stats()["kernels"])
    assert {k: v[0] for k, v in alone.items()} == {"k_dc_summary": 1, "k_dc_carry": 1, "k_dc_main": 1, "k_dc_init": 1}
    return call, want, alone


def check_behind(ctx, small_op, what):
    call, want, alone = small_op
    ctx.stats_reset()
    got, wall_ms, st = timed(ctx, call)
    assert got == want, "the DC encode behind " + what
    assert counts(st["kernels"]) == alone, "behind %s the DC encode reports %s, alone %s" % (what, counts(st["kernels"]), alone)
    check_times("the DC encode behind " + what, wall_ms, st, 1)


def test_no_carry_over_behind_every_op(ctx, ops, small_op):
    for name in sorted(ops):
        call, want = ops[name]
        assert call(ctx) == want, name
        check_behind(ctx, small_op, name)


def test_no_carry_over_behind_refused_calls(ctx, ops, small_op):
    """one DK_E_ARG refusal per entry family, each behind an op that has left the pool's events recorded"""
    t = u8(datagen.wiki_like(3000, seed=1))
    n = len(t)
    d, d8, w = dev(t), torch.empty(n, dtype=torch.uint8, device="cuda"), words(n)
    pat = dev(u8(b"abc\0"))
    out = np.empty(2 * n + 4096, np.uint8)
    refused = {
        "dev_suffix_array": lambda: ctx.dev_suffix_array(d, CAP + 1, w),
        "dev_bwt_forward": lambda: ctx.dev_bwt_forward(d, 0, d8),
        "dev_bwt_inverse": lambda: ctx.dev_bwt_inverse(d, n, n, d8),
        "dev_dc_encode": lambda: ctx.dev_dc_encode(d, CAP + 1, w, d8),
        "dev_block_encode": lambda: ctx.dev_block_encode("dark", d, CAP + 1, out),
        "dev_bwt_forward_packed": lambda: ctx.dev_bwt_forward_packed(d, [300, 0], d8),
        "dev_bwt_inverse_packed": lambda: ctx.dev_bwt_inverse_packed(d, [300, 300], [0, 300], d8),
        "dev_batch_encode": lambda: ctx.dev_batch_encode("dark", [d, d], [n, CAP + 1]),
        "dev_packed_encode": lambda: ctx.dev_packed_encode("dark", d, [300, 0]),
        "dev_lcp": lambda: ctx.dev_lcp(d, CAP + 1, w, w),
        "dev_lcp_packed": lambda: ctx.dev_lcp_packed(d, [300, 0], w, w),
        "dev_sa_check": lambda: ctx.dev_sa_check(d, CAP + 1, w),
        "dev_sa_search": lambda: ctx.dev_sa_search(d, CAP + 1, w, pat, [3], words(1), words(1)),
        "dev_fm_build": lambda: ctx.dev_fm_build(d, CAP + 1, 0, torch.empty(1 << 16, dtype=torch.uint8, device="cuda")),
    }
    before = ops["packed_forward"]
    for name, call in refused.items():
        assert before[0](ctx) == before[1]
        assert error_of(call) == DK_E_ARG, name
        check_behind(ctx, small_op, "the refused " + name)


def five_blocks():
    rng = np.random.default_rng(77)
    blocks = [u8(datagen.wiki_like(30011, seed=4)), np.full(5000, 65, np.uint8), rng.integers(0, 256, size=12289, dtype=np.uint8),
              u8(datagen.word_like(70000, seed=9, vocab=500)), u8(b"abracadabra")]
    assert (blocks[2] == 0xFF).any() and not any((b == 0xFF).any() for k, b in enumerate(blocks) if k != 2)
    return blocks


def test_no_carry_over_behind_batches(ctx, small_op):
    blocks = five_blocks()
    d_blocks = [dev(b) for b in blocks]
    sizes = [len(b) for b in blocks]
    ctx.dev_batch_encode("dark+ff", d_blocks, sizes, host_threads=3)
    check_behind(ctx, small_op, "dev_batch_encode")
    with ctx.batch_begin("dark+ff", host_threads=2) as bt:
        bt.push(d_blocks[0], sizes[0])
        bt.push_packed(dev(np.concatenate(blocks[1:3])), sizes[1:3])
        bt.push(d_blocks[4], sizes[4])
        assert len(bt.finish()) == 4
    check_behind(ctx, small_op, "batch_begin / push / push_packed / push / finish")
    # a push that is refused in the middle of a batch (a block above the capacity): the batch closes, nothing stays pending
    with ctx.batch_begin("dark+ff", host_threads=2) as bt:
        bt.push(d_blocks[0], sizes[0])
        assert error_of(lambda: bt.push(d_blocks[0], CAP + 1)) == DK_E_ARG
    check_behind(ctx, small_op, "a batch with a refused push")


# ---- f. batches ------------------------------------------------------------------------------------------------------------------------------------

def add(total, part):
    for k, (n, b) in part.items():
        n0, b0 = total.get(k, (0, 0.0))
        total[k] = (n0 + n, b0 + b)


def test_batch_equals_the_single_calls(ctx):
    """five blocks of different sizes -- one of a single symbol, one holding 0xFF, model dark+ff -- through dev_batch_encode with three coding
    threads: four staging slots for five blocks, so one is reused"""
    blocks = five_blocks()
    d_blocks = [dev(b) for b in blocks]
    sizes = [len(b) for b in blocks]
    singles, want = {}, []
    for d, n in zip(d_blocks, sizes):
        ctx.stats_reset()
        want.append(ctx.dev_block_encode("dark+ff", d, n).tobytes())
        add(singles, counts(ctx.stats()["kernels"]))
    ctx.stats_reset()
    got = ctx.dev_batch_encode("dark+ff", d_blocks, sizes, host_threads=3)
    batch = counts(ctx.stats()["kernels"])
    assert [g.tobytes() for g in got] == want
    assert batch == singles
    # the streaming form, the same blocks: the same again
    ctx.stats_reset()
    with ctx.batch_begin("dark+ff", host_threads=3) as bt:
        for d, n in zip(d_blocks, sizes):
            bt.push(d, n)
        got = bt.finish()
    assert [g.tobytes() for g in got] == want and counts(ctx.stats()["kernels"]) == singles
    with profiled(CAP, purpose="decoder") as dec:  # (and the streams decode, under profiling, on a decoder context)
        for s, b in zip(want, blocks):
            d_out = torch.empty(len(b), dtype=torch.uint8, device="cuda")
            dec.dev_block_decode("dark+ff", s, len(b), d_out)
            assert d_out.cpu().numpy().tobytes() == b.tobytes()


def test_batch_push_packed_equals_packed_encode(ctx):
    """two packs pushed into one open batch against dev_packed_encode of each"""
    blocks = five_blocks()
    packs = [blocks[:2], blocks[2:]]
    d_packs = [dev(np.concatenate(p)) for p in packs]
    singles, want = {}, []
    for d, p in zip(d_packs, packs):
        ctx.stats_reset()
        streams, _ = ctx.dev_packed_encode("dark+ff", d, [len(b) for b in p], host_threads=3)
        want += [s.tobytes() for s in streams]
        add(singles, counts(ctx.stats()["kernels"]))
    for k, b in enumerate(blocks):  # (a pack's streams are the single calls')
        assert want[k] == ctx.dev_block_encode("dark+ff", dev(b), len(b)).tobytes(), k
    ctx.stats_reset()
    with ctx.batch_begin("dark+ff", host_threads=3) as bt:
        for d, p in zip(d_packs, packs):
            bt.push_packed(d, [len(b) for b in p])
        got = bt.finish()
    assert [g.tobytes() for g in got] == want
    assert counts(ctx.stats()["kernels"]) == singles


# ---- g. the LCP counters ---------------------------------------------------------------------------------------------------------------------------

def check_counters(st, model, routes, what):
    assert st["lcp_passes"] == 1, (what, st["lcp_passes"])
    if routes is not None:
        assert st["routes"] & {"lcp_long", "lcp_giant"} == routes, (what, st["routes"])
    assert (model["longs"] > 0) == ("lcp_long" in st["routes"]) and (model["giants"] > 0) == ("lcp_giant" in st["routes"]), (what, model, st["routes"])
    assert st["lcp_measured"] == model["measured"], "%s: lcp_measured = %d, model %d" % (what, st["lcp_measured"], model["measured"])
    assert model["bytes_lo"] <= st["lcp_bytes_compared"] <= model["bytes_hi"], \
        "%s: lcp_bytes_compared = %d, model [%d, %d]" % (what, st["lcp_bytes_compared"], model["bytes_lo"], model["bytes_hi"])
    if not model["giants"]:
        assert model["bytes_lo"] == model["bytes_hi"]  # (below the grid's kernel the model is exact)


@pytest.mark.parametrize("name", sorted(CM.single_cases()))
def test_lcp_counters_single(ctx, name):
    """dev_lcp on the suffix array dev_suffix_array gave, then the one-call forms: the same array, the same counters"""
    t, routes = CM.single_cases()[name]
    n = len(t)
    sa = gpu_sa(ctx, t)
    want = lcp_kasai(t, sa.host())
    model = CM.count_model([t], [sa.host()], lcps=[want])
    out = Words(n)
    ctx.dev_lcp(dev_text(t), n, sa.t, out.t)
    st = ctx.stats()
    assert out.guards_intact() and sa.guards_intact(), "a store left the outputs"
    assert np.array_equal(out.host(), want), name
    check_counters(st, model, routes, name + ", dev_lcp")
    d_sa, d_lcp = Words(n), Words(n)
    ctx.dev_suffix_array_lcp(dev_text(t), n, d_sa.t, d_lcp.t)
    st = ctx.stats()
    assert d_sa.guards_intact() and d_lcp.guards_intact()
    assert np.array_equal(d_sa.host(), sa.host()) and np.array_equal(d_lcp.host(), want)
    check_counters(st, model, routes, name + ", dev_suffix_array_lcp")
    out = Words(n)
    ctx.dev_lcp_packed(dev_text(t), [n], sa.t, out.t)  # a single block is a pack of one
    st = ctx.stats()
    assert out.guards_intact() and np.array_equal(out.host(), want)
    check_counters(st, model, routes, name + ", dev_lcp_packed of one block")
    if n < 10000:
        h_sa, h_lcp = ctx.suffix_array_lcp(t)
        assert np.array_equal(h_sa, sa.host()) and np.array_equal(h_lcp, want)
        check_counters(ctx.stats(), model, routes, name + ", suffix_array_lcp")


@pytest.mark.parametrize("one_call", [False, True])
@pytest.mark.parametrize("name", sorted(CM.pack_cases()))
def test_lcp_counters_pack(ctx, name, one_call):
    """dev_suffix_array_packed + dev_lcp_packed, and dev_suffix_array_packed_lcp (Phi from the sort's ranks); run_pack checks the guards"""
    blocks, routes = CM.pack_cases()[name]
    sas, lcps, _ = run_pack(ctx, blocks, one_call)
    st = ctx.stats()
    want = [lcp_kasai(b, sa) for b, sa in zip(blocks, sas)]
    for k, (g, w) in enumerate(zip(lcps, want)):
        assert np.array_equal(g, w), "%s: LCP array of block %d" % (name, k)
    check_counters(st, CM.count_model(blocks, sas, lcps=want), routes, "%s, one_call=%s" % (name, one_call))
    if name == "lane_and_wave" and not one_call:
        h = ctx.suffix_array_packed_lcp(blocks)
        assert all(np.array_equal(g[1], w) for g, w in zip(h, want))
        check_counters(ctx.stats(), CM.count_model(blocks, sas, lcps=want), routes, name + ", suffix_array_packed_lcp")


TUNED_LANE, TUNED_WAVE = 32, 128
WORKER = r"""
import json, os, sys
root = sys.argv[1]
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import dark_amd
from test_gpu_lcp import Words, dev_text, gpu_sa
from test_gpu_profiling import tuned_text
t = tuned_text()
with dark_amd.Context(1 << 16) as ctx:
    ctx.set_profiling(True)
    sa = gpu_sa(ctx, t)
    out = Words(len(t))
    ctx.dev_lcp(dev_text(t), len(t), sa.t, out.t)
    st = ctx.stats()
    assert out.guards_intact() and sa.guards_intact()
    print("RESULT " + json.dumps(dict(sa=sa.host().tolist(), lcp=out.host().tolist(), routes=sorted(st["routes"]), passes=int(st["lcp_passes"]),
                                      measured=int(st["lcp_measured"]), compared=int(st["lcp_bytes_compared"]))))
"""


def tuned_text():
    """common prefixes that end in the lane (random bytes), in the wave (100 bytes: between the lowered caps), in the grid's first chunk (300
    bytes) and in its second (5000 bytes: 4096 behind the wave's cap and on), and a^700 to the block's end"""
    return np.concatenate([planted(100, seed=1), planted(300, seed=2), planted(5000, seed=3), np.full(700, 97, np.uint8)])


def test_lcp_counters_tuning_build():
    assert os.path.exists(TUNING_LIB), "build the tuning library: python dark_amd/build.py --tuning"
    env = {k: v for k, v in os.environ.items() if not k.startswith("DK_")}
    env.update(DARK_AMD_LIB=TUNING_LIB, DK_LCP_LANE_CAP=str(TUNED_LANE), DK_LCP_WAVE_CAP=str(TUNED_WAVE))
    p = subprocess.run([sys.executable, "-c", WORKER, ROOT], env=env, capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0, "the worker failed (%d)\n%s%s" % (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    t = tuned_text()
    sa = np.array(r["sa"], np.int64)
    want = lcp_kasai(t, sa)
    assert np.array_equal(np.array(r["lcp"], np.uint32), want)
    model = CM.count_model([t], [sa], lane_cap=TUNED_LANE, wave_cap=TUNED_WAVE, lcps=[want])
    assert model["longs"] > model["giants"] >= 3 and model["bytes_lo"] < model["bytes_hi"], model  # every rule, the open interval too
    assert CM.count_model([t], [sa], lcps=[want]) != model  # (the default caps would count otherwise: the knobs are what is tested)
    st = dict(lcp_passes=r["passes"], routes=set(r["routes"]), lcp_measured=r["measured"], lcp_bytes_compared=r["compared"])
    check_counters(st, model, {"lcp_long", "lcp_giant"}, "lane cap 32, wave cap 128")


# ---- h. exact-capacity contexts --------------------------------------------------------------------------------------------------------------------

def exact_text(n):
    """word-like text with a passage of a third of it twice: the lists are in use whatever n"""
    t = u8(datagen.wiki_like(n, seed=n)).copy()
    k = n // 3
    t[n - k:] = t[:k]
    return t


@pytest.mark.parametrize("n", [4095, 4096, 4097, 65536, 70001])
def test_exact_capacity_lcp(n):
    t = exact_text(n)
    with profiled(n) as exact:
        assert exact.capacity() == n

        def ok(what):
            st = exact.stats()
            assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], (what, st)
            assert st["lcp_passes"] == 1 and st["lcp_measured"] > 0 and st["lcp_bytes_compared"] > 0 and "lcp_long" in st["routes"], (what, st)
            return st
        sa = gpu_sa(exact, t)
        want = lcp_kasai(t, sa.host())
        model = CM.count_model([t], [sa.host()], lcps=[want])
        out = Words(n)
        exact.dev_lcp(dev_text(t), n, sa.t, out.t)
        assert out.guards_intact() and np.array_equal(out.host(), want)
        check_counters(ok("dev_lcp"), model, None, "dev_lcp, context of exactly %d" % n)
        h_sa, h_lcp = exact.suffix_array_lcp(t)
        assert np.array_equal(h_sa, sa.host()) and np.array_equal(h_lcp, want)
        check_counters(ok("suffix_array_lcp"), model, None, "suffix_array_lcp, context of exactly %d" % n)
        sizes = [n // 3, 1, n - n // 3 - 1]
        ends = np.cumsum(sizes)
        blocks = [t[e - k:e] for k, e in zip(sizes, ends)]
        for one_call in (False, True):
            sas, lcps, _ = run_pack(exact, blocks, one_call)
            st = exact.stats()
            assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], st
            pw = [lcp_kasai(b, s) for b, s in zip(blocks, sas)]
            assert all(np.array_equal(g, w) for g, w in zip(lcps, pw))
            check_counters(st, CM.count_model(blocks, sas, lcps=pw), None, "a pack of exactly %d, one_call=%s" % (n, one_call))


@pytest.mark.parametrize("n", [4095, 4096, 4097, 70001])
def test_exact_capacity_decoder(ctx, orc, n):
    t = exact_text(n)
    L, origin = orc.bwt_forward(t)
    sizes = [n // 3, 1, n - n // 3 - 1]
    streams, _ = ctx.dev_packed_encode("dark", dev(t), sizes, host_threads=2)
    streams = [s.tobytes() for s in streams]
    with profiled(n, purpose="decoder", max_blocks=len(sizes)) as dec:
        dec.stats_reset()
        assert dec.bwt_inverse(L, origin).tobytes() == t.tobytes()
        st = dec.stats()
        assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"] and launches(st["kernels"])["k_ibwt_emit"] == 1, st
        d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
        dec.stats_reset()
        dec.dev_packed_decode("dark", streams, sizes, d_out, host_threads=2)
        st = dec.stats()
        assert d_out.cpu().numpy().tobytes() == t.tobytes()
        assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], st
        assert {k: v for k, v in launches(st["kernels"]).items() if k != "k_ibwt_jump"} == {"k_ibwt_hist": 1, "k_ibwt_lf": 1, "k_ibwt_walk": 1, "k_ibwt_emit": 1}
