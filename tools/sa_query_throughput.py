"""Suffix-array check and search on the GPU: time of the check against the suffix sort of the same input, and patterns per second of the search
(DESIGN.md section 4.12).

Check: the inputs of tools/lcp_throughput.py (six blocks, two packs of 64 MiB).  Every row records the median of --reps runs of dk_dev_suffix_array
(packs: dk_dev_suffix_array_packed) and of dk_dev_sa_check (dk_dev_sa_check_packed) on its result, which must be DK_SA_OK, and the time of the
check of the same array with two slots swapped, which must not be.
Search: enwik8_like_1e8 and its suffix array, 2^20 patterns of 8, 32 and 300 bytes cut from the text at random places, and as many patterns
of random bytes of the same lengths (which do not occur); then one 64 MiB pack of 1024 blocks with 2^20 patterns of 32 bytes, each cut from
the block it is searched in.  Before anything is timed a sample of the answers is checked on the GPU with torch: the suffixes at lo and hi - 1
start with the pattern, those at lo - 1 and hi do not.  The search's time is dk_stats.ms_total, the time inside the entry point (offsets built
and uploaded, kernels, synchronise).  From one profiled call each: the time of every kernel slot.

Every workload is a child process under its own time limit; the run ends at the first that fails.

    python tools/sa_query_throughput.py [--reps 3] [--only NAME[,NAME]] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lcp_throughput import BLOCKS, PACKS, child, make_block, median_ms  # noqa: E402

NPAT = 1 << 20
LENGTHS = (8, 32, 300)
SEARCH_PACK_BLOCK = 64 << 10  # 64 MiB in 1024 blocks
SAMPLE = 4096


def slots_of(st):
    return {k: dict(ms=round(v["ms"], 3), launches=v["launches"]) for k, v in sorted(st["kernels"].items())}


def profiled(ctx, fn):
    ctx.stats_reset()
    ctx.set_profiling(True)
    fn()
    st = ctx.stats()
    ctx.set_profiling(False)
    return slots_of(st)


def library_ms(ctx, fn, reps):
    """median of dk_stats.ms_total, the time inside the entry point: a call with 2^20 patterns spends longer in its Python wrapper, which turns
    the lengths into a C array, than in the library"""
    ts = []
    for _ in range(reps):
        fn()
        ts.append(ctx.stats()["ms_total"])
    return statistics.median(ts), [round(x, 3) for x in ts]


def run_check(name, reps):
    import torch
    import dark_amd
    data = make_block(name)
    n = len(data)
    packed = name.startswith("pack_")
    sizes = [min(dict(PACKS)[name], n - k) for k in range(0, n, dict(PACKS)[name])] if packed else [n]
    d_in = torch.from_numpy(data).cuda()
    d_sa = torch.empty(n, dtype=torch.int32, device="cuda")
    with dark_amd.Context(n) as ctx:
        sort = (lambda: ctx.dev_suffix_array_packed(d_in, sizes, d_sa)) if packed else (lambda: ctx.dev_suffix_array(d_in, n, d_sa))
        check = (lambda: ctx.dev_sa_check_packed(d_in, sizes, d_sa)) if packed else (lambda: [ctx.dev_sa_check(d_in, n, d_sa)])
        sort()
        if check() != [("ok", k) for k in sizes]:
            raise SystemExit("FAILED: %s: the sort's own array is not in order: %s" % (name, [r for r in check() if r[0] != "ok"][:3]))
        sort_ms, sort_all = median_ms(sort, reps)
        check_ms, check_all = median_ms(check, reps)
        slots = profiled(ctx, check)
        a, b = n // 3, n // 3 + 1  # two neighbours of one block (a pack's blocks have at least 64 KiB)
        pair = d_sa[[b, a]].clone()
        d_sa[[a, b]] = pair
        torch.cuda.synchronize()
        bad = [r for r in check() if r[0] != "ok"]
        if len(bad) != 1 or bad[0][0] != "bad_order":
            raise SystemExit("FAILED: %s: two swapped slots gave %s" % (name, bad[:3]))
        bad_ms, _ = median_ms(check, reps)
    print("ROW " + json.dumps(dict(name=name, kind="check", bytes=n, blocks=len(sizes), sort_ms=round(sort_ms, 3), sort_runs_ms=sort_all,
                                   check_ms=round(check_ms, 3), check_runs_ms=check_all, check_over_sort=round(check_ms / sort_ms, 3),
                                   check_GBps=round(n / 1e6 / check_ms, 3), swapped_ms=round(bad_ms, 3), swapped_answer=list(bad[0]), slots=slots)), flush=True)


def verify_sample(d_in, d_sa, base, block_len, d_pat, pat_off, lens, d_lo, d_hi, g):
    """SAMPLE patterns: the suffixes at lo and hi - 1 start with the pattern (where lo < hi), those at lo - 1 and hi do not"""
    import torch
    npat = len(lens)
    pick = torch.randint(0, npat, (SAMPLE,), device="cuda", generator=g)
    lens_t, off_t = torch.tensor(lens, device="cuda")[pick], torch.tensor(pat_off, device="cuda")[pick]
    lo, hi = d_lo[pick].long(), d_hi[pick].long()
    base, block_len = base[pick], block_len[pick]
    if bool(((lo > hi) | (hi > block_len)).any()):
        raise SystemExit("FAILED: lo <= hi <= n does not hold")

    def starts_with(slot, live):
        slot = torch.where(live, slot, torch.zeros_like(slot))
        v = d_sa[base + slot].long()
        ok = live & (v + lens_t <= block_len)
        for k in range(int(lens_t.max())):
            inside = ok & (k < lens_t)
            same = d_in[torch.where(inside, base + v + k, 0)] == d_pat[torch.where(inside, off_t + k, 0)]
            ok = ok & (same | ~inside)
        return ok

    some = lo < hi
    if bool((some & ~(starts_with(lo, some) & starts_with(hi - 1, some))).any()):
        raise SystemExit("FAILED: a suffix inside [lo, hi) does not start with its pattern")
    if bool(starts_with(lo - 1, lo > 0).any()) or bool(starts_with(hi, hi < block_len).any()):
        raise SystemExit("FAILED: a suffix outside [lo, hi) starts with its pattern")
    return int(some.sum())


def run_search(name, reps):
    import numpy as np
    import torch
    import dark_amd
    packed = name == "search_pack_64KiB"
    data = make_block("pack_64KiB" if packed else "enwik8_like_1e8")
    n = len(data)
    sizes = [min(SEARCH_PACK_BLOCK, n - k) for k in range(0, n, SEARCH_PACK_BLOCK)] if packed else [n]
    d_in = torch.from_numpy(data).cuda()
    d_sa = torch.empty(n, dtype=torch.int32, device="cuda")
    d_lo, d_hi = torch.empty(NPAT, dtype=torch.int32, device="cuda"), torch.empty(NPAT, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(1)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    rows = []
    with dark_amd.Context(n) as ctx:
        if packed:
            ctx.dev_suffix_array_packed(d_in, sizes, d_sa)
        else:
            ctx.dev_suffix_array(d_in, n, d_sa)
        for m in ((32,) if packed else LENGTHS):
            for occurring in (True, False):
                blocks = rng.integers(0, len(sizes), size=NPAT)
                starts = np.asarray(blocks, np.int64) * SEARCH_PACK_BLOCK
                lens_b = np.asarray(sizes, np.int64)[blocks]
                if occurring:
                    at = starts + (rng.random(NPAT) * (lens_b - m)).astype(np.int64)
                    d_pat = d_in[(torch.from_numpy(at).cuda()[:, None] + torch.arange(m, device="cuda")[None, :])].reshape(-1).contiguous()
                else:
                    d_pat = torch.from_numpy(rng.integers(0, 256, size=NPAT * m, dtype=np.uint8)).cuda()
                lens = [m] * NPAT
                if packed:
                    search = lambda: ctx.dev_sa_search_packed(d_in, sizes, d_sa, d_pat, lens, blocks.tolist(), d_lo, d_hi)  # noqa: E731
                else:
                    search = lambda: ctx.dev_sa_search(d_in, n, d_sa, d_pat, lens, d_lo, d_hi)  # noqa: E731
                search()
                found = verify_sample(d_in, d_sa, torch.from_numpy(starts).cuda(), torch.from_numpy(lens_b).cuda(), d_pat, list(range(0, NPAT * m, m)),
                                      lens, d_lo, d_hi, g)
                if occurring and found != SAMPLE:
                    raise SystemExit("FAILED: %d of %d sampled patterns cut from the text were not found" % (SAMPLE - found, SAMPLE))
                ms, runs = library_ms(ctx, search, reps)
                rows.append(dict(name=name, kind="search", bytes=n, blocks=len(sizes), patterns=NPAT, pattern_bytes=m, occurring=occurring,
                                 sampled_found=found, ms=round(ms, 3), runs_ms=runs, Mpatterns_per_s=round(NPAT / 1e3 / ms, 2), slots=profiled(ctx, search)))
    for row in rows:
        print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated workload names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_sa_query.json"))
    ap.add_argument("--step", help=argparse.SUPPRESS)
    args = ap.parse_args()
    searches = ("search_enwik8_like_1e8", "search_pack_64KiB")
    if args.step:
        (run_search if args.step in searches else run_check)(args.step, args.reps)
        return
    names = list(BLOCKS) + [p[0] for p in PACKS] + list(searches)
    if args.only:
        names = [x for x in args.only.split(",") if x in names]
    rows = []
    if os.path.exists(args.out) and args.only:  # a run of some workloads replaces their rows and keeps the others
        with open(args.out) as f:
            rows = [r for r in json.load(f)["rows"] if r["name"] not in names]
    for name in names:
        rows += child(name, args.reps, script=os.path.abspath(__file__))
        with open(args.out, "w") as f:  # (after every workload: a run that is cut short keeps what it has)
            json.dump(dict(tool="tools/sa_query_throughput.py", reps=args.reps, rows=rows), f, indent=1)
    print(args.out)


if __name__ == "__main__":
    main()
