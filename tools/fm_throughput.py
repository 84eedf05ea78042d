"""FM-index on the GPU: time of the build beside the forward BWT of the same input, and patterns per second of the backward search beside the
suffix-array search on the same patterns.

Inputs: enwik8_like_1e8, realtext_5e7 (where the host has the files it is made of), acgt_2p28, and a 64 MiB pack of 1024 blocks of 64 KiB.
Per input: the median of --reps runs of dk_dev_bwt_forward (the pack: dk_dev_bwt_forward_packed) and of dk_dev_fm_build (_packed) on its L; then
2^20 patterns of 4, 8, 32 and 300 bytes, cut from the text at random places and as many of random bytes, counted by dk_dev_fm_count (_packed) and
searched by dk_dev_sa_search (_packed) in the suffix array of the same text.  EVERY answer of the count is compared with the search's before
anything is timed.  The times of count and search are dk_stats.ms_total, the time inside the entry point (offsets built and uploaded, kernel,
synchronise).  Resident bytes: L and the index against text and suffix array.

Every input is a child process under its own time limit; the run ends at the first that fails.

    python tools/fm_throughput.py [--reps 3] [--only NAME[,NAME]] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lcp_throughput import child, make_block, median_ms  # noqa: E402
from sa_query_throughput import library_ms, profiled  # noqa: E402

NAMES = ("enwik8_like_1e8", "realtext_5e7", "acgt_2p28", "pack_64KiB")
NPAT = 1 << 20
LENGTHS = (4, 8, 32, 300)
PACK_BLOCK = 64 << 10


def run_one(name, reps):
    import numpy as np
    import torch
    import dark_amd
    from dark_amd.context import fm_index_bytes
    try:
        data = make_block(name)
    except Exception as e:  # realtext_5e7 on a host without its files
        print("ROW " + json.dumps(dict(name=name, kind="unavailable", why=repr(e)[:200])), flush=True)
        return
    n = len(data)
    packed = name.startswith("pack_")
    sizes = [min(PACK_BLOCK, n - k) for k in range(0, n, PACK_BLOCK)] if packed else [n]
    d_in = torch.from_numpy(data).cuda()
    d_bwt = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_sa = torch.empty(n, dtype=torch.int32, device="cuda")
    index_bytes = fm_index_bytes(n, len(sizes))
    d_index = torch.empty(index_bytes // 4, dtype=torch.int32, device="cuda")
    d_lo, d_hi = (torch.empty(NPAT, dtype=torch.int32, device="cuda") for _ in range(2))
    s_lo, s_hi = (torch.empty(NPAT, dtype=torch.int32, device="cuda") for _ in range(2))
    rng = np.random.default_rng(1)
    origins = []
    with dark_amd.Context(n) as ctx:
        def forward():
            origins[:] = ctx.dev_bwt_forward_packed(d_in, sizes, d_bwt) if packed else [ctx.dev_bwt_forward(d_in, n, d_bwt)]
        build = (lambda: ctx.dev_fm_build_packed(d_bwt, sizes, origins, d_index)) if packed else (lambda: ctx.dev_fm_build(d_bwt, n, origins[0], d_index))
        forward()
        routes = sorted(ctx.stats()["routes"])
        forward_ms, forward_all = median_ms(forward, reps)
        build()
        build_ms, build_all = median_ms(build, reps)
        print("ROW " + json.dumps(dict(name=name, kind="build", bytes=n, blocks=len(sizes), routes=routes, bwt_forward_ms=round(forward_ms, 3),
                                       bwt_forward_runs_ms=forward_all, fm_build_ms=round(build_ms, 3), fm_build_runs_ms=build_all,
                                       build_over_forward=round(build_ms / forward_ms, 4), build_GBps=round(n / 1e6 / build_ms, 2), index_bytes=index_bytes,
                                       resident_fm_bytes=n + index_bytes, resident_sa_bytes=5 * n, slots=profiled(ctx, build))), flush=True)
        if packed:
            ctx.dev_suffix_array_packed(d_in, sizes, d_sa)
        else:
            ctx.dev_suffix_array(d_in, n, d_sa)
        for m in LENGTHS:
            for occurring in (True, False):
                blocks = rng.integers(0, len(sizes), size=NPAT)
                starts = np.asarray(blocks, np.int64) * PACK_BLOCK
                lens_b = np.asarray(sizes, np.int64)[blocks]
                if occurring:
                    at = starts + (rng.random(NPAT) * (lens_b - m)).astype(np.int64)
                    d_pat = d_in[(torch.from_numpy(at).cuda()[:, None] + torch.arange(m, device="cuda")[None, :])].reshape(-1).contiguous()
                else:
                    d_pat = torch.from_numpy(rng.integers(0, 256, size=NPAT * m, dtype=np.uint8)).cuda()
                lens = [m] * NPAT
                if packed:
                    where = blocks.tolist()
                    count = lambda: ctx.dev_fm_count_packed(d_bwt, sizes, d_index, d_pat, lens, where, d_lo, d_hi)  # noqa: E731
                    search = lambda: ctx.dev_sa_search_packed(d_in, sizes, d_sa, d_pat, lens, where, s_lo, s_hi)  # noqa: E731
                else:
                    count = lambda: ctx.dev_fm_count(d_bwt, n, d_index, d_pat, lens, d_lo, d_hi)  # noqa: E731
                    search = lambda: ctx.dev_sa_search(d_in, n, d_sa, d_pat, lens, s_lo, s_hi)  # noqa: E731
                count()
                search()
                if not (torch.equal(d_lo, s_lo) and torch.equal(d_hi, s_hi)):
                    bad = int(((d_lo != s_lo) | (d_hi != s_hi)).sum())
                    raise SystemExit("FAILED: %s, %d bytes, occurring=%s: %d of %d answers differ from the suffix-array search's" % (name, m, occurring, bad, NPAT))
                found = int((d_hi > d_lo).sum())
                if occurring and found != NPAT:
                    raise SystemExit("FAILED: %d patterns cut from the text were not found" % (NPAT - found))
                fm_ms, fm_runs = library_ms(ctx, count, reps)
                sa_ms, sa_runs = library_ms(ctx, search, reps)
                print("ROW " + json.dumps(dict(name=name, kind="count", bytes=n, blocks=len(sizes), patterns=NPAT, pattern_bytes=m, occurring=occurring,
                                               found=found, answers_equal=True, fm_ms=round(fm_ms, 3), fm_runs_ms=fm_runs, sa_ms=round(sa_ms, 3),
                                               sa_runs_ms=sa_runs, fm_Mpatterns_per_s=round(NPAT / 1e3 / fm_ms, 2), sa_Mpatterns_per_s=round(NPAT / 1e3 / sa_ms, 2),
                                               fm_over_sa=round(fm_ms / sa_ms, 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated input names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_fm.json"))
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
        rows += child(name, args.reps, script=os.path.abspath(__file__))
        with open(args.out, "w") as f:  # (after every input: a run that is cut short keeps what it has)
            json.dump(dict(tool="tools/fm_throughput.py", reps=args.reps, fm_block=1024, rows=rows), f, indent=1)
    print(args.out)


if __name__ == "__main__":
    main()
