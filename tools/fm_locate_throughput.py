"""FM-index locate on the GPU: time of the locate structure's build beside the inverse BWT and the index build of the same input, and positions
per second of dk_dev_fm_locate beside the 5 n route -- dk_dev_sa_search, then reading SA[lo, hi).

Inputs: enwik8_like_1e8, acgt_2p28, and a 64 MiB pack of 1024 blocks of 64 KiB (those of tools/fm_throughput.py).
Per input and sampling step: the median of --reps runs of dk_dev_fm_locate_build (_packed) beside dk_dev_bwt_inverse (_packed) and dk_dev_fm_build
(_packed) on the same L.  Then 2^20 patterns of 8 and 32 bytes cut from the text at random places, counted by dk_dev_fm_count and located with
max_hits 1 and 16.  EVERY position is compared with the suffix array's before anything is timed.  The times of the library's calls are
dk_stats.ms_total, the time inside the entry point; the gather of the 5 n route is a torch index over the suffix array, timed around a
synchronise.  Resident bytes per route are arithmetic.

Every input is a child process under its own time limit; the run ends at the first that fails.

    python tools/fm_locate_throughput.py [--reps 3] [--only NAME[,NAME]] [--steps 8,32,128] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lcp_throughput import child, make_block, median_ms  # noqa: E402
from sa_query_throughput import library_ms, profiled  # noqa: E402

NAMES = ("enwik8_like_1e8", "acgt_2p28", "pack_64KiB")
NPAT = 1 << 20
LENGTHS = (8, 32)
MAX_HITS = (1, 16)
PACK_BLOCK = 64 << 10
NO_HIT = -1  # DK_FM_NO_HIT seen through an int32 tensor


def run_one(spec, reps):
    import statistics
    import numpy as np
    import torch
    import dark_amd
    from dark_amd.context import fm_index_bytes, fm_locate_bytes
    name, _, steps = spec.partition("@")
    steps = [int(s) for s in steps.split(",")]
    data = make_block(name)
    n = len(data)
    packed = name.startswith("pack_")
    sizes = [min(PACK_BLOCK, n - k) for k in range(0, n, PACK_BLOCK)] if packed else [n]
    d_in = torch.from_numpy(data).cuda()
    d_bwt, d_out = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    d_sa = torch.empty(n, dtype=torch.int32, device="cuda")
    index_bytes = fm_index_bytes(n, len(sizes))
    d_index = torch.empty(index_bytes // 4, dtype=torch.int32, device="cuda")
    d_lo, d_hi, s_lo, s_hi = (torch.empty(NPAT, dtype=torch.int32, device="cuda") for _ in range(4))
    rng = np.random.default_rng(1)
    with dark_amd.Context(n) as ctx:
        if packed:
            origins = ctx.dev_suffix_array_packed(d_in, sizes, d_sa, d_bwt)
            inverse = lambda: ctx.dev_bwt_inverse_packed(d_bwt, sizes, origins, d_out)  # noqa: E731
            index = lambda: ctx.dev_fm_build_packed(d_bwt, sizes, origins, d_index)  # noqa: E731
        else:
            origins = [ctx.dev_bwt_forward(d_in, n, d_bwt)]
            ctx.dev_suffix_array(d_in, n, d_sa)
            inverse = lambda: ctx.dev_bwt_inverse(d_bwt, n, origins[0], d_out)  # noqa: E731
            index = lambda: ctx.dev_fm_build(d_bwt, n, origins[0], d_index)  # noqa: E731
        inverse()
        if not torch.equal(d_out, d_in):
            raise SystemExit("FAILED: %s: the inverse BWT does not give the text back" % name)
        inverse_ms, inverse_all = median_ms(inverse, reps)
        index()
        index_ms, index_all = median_ms(index, reps)
        # the patterns and their ranges, once for all steps
        batches = []
        for m in LENGTHS:
            blocks = rng.integers(0, len(sizes), size=NPAT)
            at = np.asarray(blocks, np.int64) * PACK_BLOCK + (rng.random(NPAT) * (np.asarray(sizes, np.int64)[blocks] - m)).astype(np.int64)
            d_pat = d_in[(torch.from_numpy(at).cuda()[:, None] + torch.arange(m, device="cuda")[None, :])].reshape(-1).contiguous()
            batches.append((m, blocks.tolist() if packed else None, torch.from_numpy(np.asarray(blocks, np.int64) * PACK_BLOCK).cuda(), d_pat))
        for step in steps:
            loc_bytes = fm_locate_bytes(n, len(sizes), step)
            d_loc = torch.empty(loc_bytes // 4, dtype=torch.int32, device="cuda")
            if packed:
                build = lambda: ctx.dev_fm_locate_build_packed(d_bwt, sizes, origins, step, d_loc)  # noqa: E731
            else:
                build = lambda: ctx.dev_fm_locate_build(d_bwt, n, origins[0], step, d_loc)  # noqa: E731
            build()
            build_ms, build_all = median_ms(build, reps)
            print("ROW " + json.dumps(dict(name=name, kind="build", step=step, bytes=n, blocks=len(sizes), locate_build_ms=round(build_ms, 3),
                                           locate_build_runs_ms=build_all, bwt_inverse_ms=round(inverse_ms, 3), bwt_inverse_runs_ms=inverse_all,
                                           fm_build_ms=round(index_ms, 3), fm_build_runs_ms=index_all, build_over_inverse=round(build_ms / inverse_ms, 3),
                                           locate_bytes=loc_bytes, index_bytes=index_bytes, resident_fm_locate_bytes=n + index_bytes + loc_bytes,
                                           resident_sa_bytes=5 * n, slots=profiled(ctx, build))), flush=True)
            for m, where, d_base, d_pat in batches:
                lens = [m] * NPAT
                if packed:
                    count = lambda: ctx.dev_fm_count_packed(d_bwt, sizes, d_index, d_pat, lens, where, d_lo, d_hi)  # noqa: E731
                    search = lambda: ctx.dev_sa_search_packed(d_in, sizes, d_sa, d_pat, lens, where, s_lo, s_hi)  # noqa: E731
                else:
                    count = lambda: ctx.dev_fm_count(d_bwt, n, d_index, d_pat, lens, d_lo, d_hi)  # noqa: E731
                    search = lambda: ctx.dev_sa_search(d_in, n, d_sa, d_pat, lens, s_lo, s_hi)  # noqa: E731
                count()
                search()
                if not (torch.equal(d_lo, s_lo) and torch.equal(d_hi, s_hi)):
                    raise SystemExit("FAILED: %s, %d bytes: the count's ranges differ from the suffix-array search's" % (name, m))
                sa_ms, sa_runs = library_ms(ctx, search, reps)
                for max_hits in MAX_HITS:
                    d_pos = torch.empty(NPAT * max_hits, dtype=torch.int32, device="cuda")
                    if packed:
                        locate = lambda: ctx.dev_fm_locate_packed(d_bwt, sizes, d_index, d_loc, step, d_lo, d_hi, where, max_hits, d_pos)  # noqa: E731
                    else:
                        locate = lambda: ctx.dev_fm_locate(d_bwt, n, d_index, d_loc, step, d_lo, d_hi, NPAT, max_hits, d_pos)  # noqa: E731

                    def gather():
                        j = torch.arange(max_hits, device="cuda")[None, :]
                        slot = s_lo.long()[:, None] + j
                        got = d_sa[(d_base[:, None] + slot).clamp_(max=n - 1)]
                        got[slot >= s_hi.long()[:, None]] = NO_HIT
                        torch.cuda.synchronize()
                        return got
                    locate()
                    want = gather()
                    if not torch.equal(d_pos.view(NPAT, max_hits), want):
                        bad = int((d_pos.view(NPAT, max_hits) != want).sum())
                        raise SystemExit("FAILED: %s step %d, %d bytes, max_hits %d: %d positions differ from the suffix array's" % (name, step, m, max_hits, bad))
                    positions = int((want != NO_HIT).sum())
                    fm_ms, fm_runs = library_ms(ctx, locate, reps)
                    ts = []
                    for _ in range(reps):
                        torch.cuda.synchronize()
                        t = time.perf_counter()
                        gather()
                        ts.append(1e3 * (time.perf_counter() - t))
                    gather_ms = statistics.median(ts)
                    print("ROW " + json.dumps(dict(name=name, kind="locate", step=step, bytes=n, blocks=len(sizes), patterns=NPAT, pattern_bytes=m,
                                                   max_hits=max_hits, positions=positions, answers_equal=True, fm_locate_ms=round(fm_ms, 3), fm_locate_runs_ms=fm_runs,
                                                   ms_per_step=round(fm_ms / step, 4), fm_Mpositions_per_s=round(positions / 1e3 / fm_ms, 2),
                                                   sa_search_ms=round(sa_ms, 3), sa_search_runs_ms=sa_runs, sa_gather_ms=round(gather_ms, 3),
                                                   sa_Mpositions_per_s=round(positions / 1e3 / (sa_ms + gather_ms), 2))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated input names (default: all)")
    ap.add_argument("--steps", default="8,32,128", help="comma-separated sampling steps, powers of two in [1, 4096]")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_fm_locate.json"))
    ap.add_argument("--step", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        run_one(args.step, args.reps)
        return
    names = [x for x in NAMES if not args.only or x in args.only.split(",")]
    rows = []
    if os.path.exists(args.out) and args.only:  # a run of some inputs replaces their rows and keeps the others
        with open(args.out) as f:
            rows = [r for r in json.load(f)["rows"] if r["name"] not in names]
    for name in names:
        rows += child(name + "@" + args.steps, args.reps, script=os.path.abspath(__file__))
        with open(args.out, "w") as f:  # (after every input: a run that is cut short keeps what it has)
            json.dump(dict(tool="tools/fm_locate_throughput.py", reps=args.reps, steps=args.steps, rows=rows), f, indent=1)
    print(args.out)


if __name__ == "__main__":
    main()
