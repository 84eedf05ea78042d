"""LCP arrays on the GPU: time against the suffix sort of the same input, per-kernel-slot times and the pass's counters.

Blocks: enwik8_like_1e8, wordlike_1e8, realtext_5e7, acgt_2p28, two identical halves of 50 MB, a^n b at 1e8.  Packs: 64 MiB of wiki_like
in blocks of 64 KiB and of 1 MiB.  Every row records the median of --reps runs of dk_dev_suffix_array (packs: dk_dev_suffix_array_packed) and of
dk_dev_lcp (dk_dev_lcp_packed) on its result, their ratio, and from one profiled LCP call the time of every kernel slot, the route bits, the
positions measured, the bytes compared and the passes over the lists.

Every result is checked on the GPU with torch before it is timed: for every i >= 1 the bytes at SA[i-1] + LCP[i] and SA[i] + LCP[i] differ
or one of the two suffixes ends there (in a pack: at its block's end), LCP at a block's first slot is 0, and on 10^6 random i the common
prefix is equal at its first and last byte and at 32 random places between.  A wrong result ends the run as a failure, it is not a number.

Every workload is a child process under its own time limit; the run ends at the first that fails.

    python tools/lcp_throughput.py [--reps 3] [--only NAME[,NAME]] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCKS = ("enwik8_like_1e8", "wordlike_1e8", "realtext_5e7", "acgt_2p28", "two_halves_1e8", "a_n_b_1e8")
PACKS = (("pack_64KiB", 64 << 10), ("pack_1MiB", 1 << 20))
PACK_BYTES = 64 << 20
STEP_TIMEOUT = 540  # seconds per child: the host generates up to 2^28 bytes first
SAMPLES = 1_000_000


def make_block(name):
    import numpy as np
    from dark_amd import datagen
    if name == "two_halves_1e8":
        h = np.frombuffer(datagen.wiki_like(50_000_000, seed=2), np.uint8)
        return np.concatenate([h, h])
    if name == "a_n_b_1e8":
        t = np.full(100_000_000, ord("a"), np.uint8)
        t[-1] = ord("b")
        return t
    if name.startswith("pack_"):
        return np.ascontiguousarray(np.frombuffer(datagen.wiki_like(PACK_BYTES, seed=2), np.uint8))
    return np.ascontiguousarray(np.frombuffer(datagen.WORKLOADS[name](), np.uint8))


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()  # every entry point returns after a synchronise of the library's stream
        ts.append(1e3 * (time.perf_counter() - t))
    return statistics.median(ts), [round(x, 3) for x in ts]


def verify(d_in, d_sa, d_lcp, sizes):
    """the checks of the module's docstring; returns the number of slots, raises SystemExit on the first that fails"""
    import torch
    n = d_in.numel()
    ends = torch.cumsum(torch.tensor(sizes, dtype=torch.int64, device="cuda"), 0)
    starts = ends - torch.tensor(sizes, dtype=torch.int64, device="cuda")
    if len(sizes) == 1:
        base = torch.zeros(1, dtype=torch.int64, device="cuda")
        end = ends
    else:
        blk = torch.repeat_interleave(torch.arange(len(sizes), device="cuda"), torch.tensor(sizes, device="cuda"))
        base, end = starts[blk], ends[blk]
    if bool((d_lcp[starts] != 0).any()):
        raise SystemExit("FAILED: LCP at a block's first slot is not 0")
    first = torch.zeros(n, dtype=torch.bool, device="cuda")
    first[starts] = True
    CH = 1 << 26  # slots per step: the index arithmetic is 64-bit
    for lo in range(1, n, CH):
        hi = min(n, lo + CH)
        l = d_lcp[lo:hi].long()
        b0 = base if len(sizes) == 1 else base[lo:hi]
        e0 = end if len(sizes) == 1 else end[lo:hi]
        a = d_sa[lo - 1:hi - 1].long() + b0 + l
        b = d_sa[lo:hi].long() + b0 + l
        inside = (a < e0) & (b < e0)
        if bool(((a > e0) | (b > e0)).any()):
            raise SystemExit("FAILED: a common prefix runs past its block")
        ta = d_in[torch.where(inside, a, torch.zeros_like(a))]
        tb = d_in[torch.where(inside, b, torch.zeros_like(b))]
        if bool((inside & (ta == tb) & ~first[lo:hi]).any()):
            raise SystemExit("FAILED: a common prefix goes on behind LCP[i]")
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    i = torch.randint(1, max(n, 2), (SAMPLES,), device="cuda", generator=g).clamp(max=n - 1)
    i = i[~first[i]]
    l = d_lcp[i].long()
    b0 = base if len(sizes) == 1 else base[i]
    a, b = d_sa[i - 1].long() + b0, d_sa[i].long() + b0
    for k in range(34):
        if k == 0:
            o = torch.zeros_like(l)
        elif k == 1:
            o = (l - 1).clamp(min=0)
        else:
            o = (torch.rand(l.shape, device="cuda", generator=g) * l).long().clamp(max=(l - 1).clamp(min=0))
        live = l > 0
        if bool((live & (d_in[torch.where(live, a + o, 0)] != d_in[torch.where(live, b + o, 0)])).any()):
            raise SystemExit("FAILED: a sampled common prefix is not equal")
    return n


def run_one(name, reps):
    import numpy as np
    import torch
    import dark_amd
    data = make_block(name)
    n = len(data)
    packed = name.startswith("pack_")
    sizes = [min(dict(PACKS)[name], n - k) for k in range(0, n, dict(PACKS)[name])] if packed else [n]
    d_in = torch.from_numpy(data).cuda()
    d_sa = torch.empty(n, dtype=torch.int32, device="cuda")
    d_lcp = torch.empty(n, dtype=torch.int32, device="cuda")
    with dark_amd.Context(n) as ctx:
        sort = (lambda: ctx.dev_suffix_array_packed(d_in, sizes, d_sa)) if packed else (lambda: ctx.dev_suffix_array(d_in, n, d_sa))
        lcp = (lambda: ctx.dev_lcp_packed(d_in, sizes, d_sa, d_lcp)) if packed else (lambda: ctx.dev_lcp(d_in, n, d_sa, d_lcp))
        sort()
        lcp()
        verify(d_in, d_sa, d_lcp, sizes)
        sort_ms, sort_all = median_ms(sort, reps)
        lcp_ms, lcp_all = median_ms(lcp, reps)
        ctx.stats_reset()
        ctx.set_profiling(True)
        lcp()
        st = ctx.stats()
        ctx.set_profiling(False)
        row = dict(name=name, bytes=n, blocks=len(sizes), sort_ms=round(sort_ms, 3), sort_runs_ms=sort_all, lcp_ms=round(lcp_ms, 3), lcp_runs_ms=lcp_all,
                   lcp_over_sort=round(lcp_ms / sort_ms, 3), lcp_GBps=round(n / 1e6 / lcp_ms, 3), routes=sorted(r for r in st["routes"] if r.startswith("lcp")),
                   measured=int(st["lcp_measured"]), bytes_compared=int(st["lcp_bytes_compared"]), passes=int(st["lcp_passes"]),
                   slots={k: dict(ms=round(v["ms"], 3), launches=v["launches"], GBps=round(v["bytes"] / 1e6 / v["ms"], 1) if v["ms"] > 0 else None)
                          for k, v in sorted(st["kernels"].items())},
                   profiled_kernels_ms=round(sum(v["ms"] for v in st["kernels"].values()), 3), checked_slots=n)
        if packed:
            d_sa2, d_lcp2 = torch.empty_like(d_sa), torch.empty_like(d_lcp)
            one = lambda: ctx.dev_suffix_array_packed_lcp(d_in, sizes, d_sa2, d_lcp2)
            one()
            if not torch.equal(d_sa2, d_sa) or not torch.equal(d_lcp2, d_lcp):
                raise SystemExit("FAILED: %s: the one-call form differs from the two calls" % name)
            row["one_call_ms"] = round(median_ms(one, reps)[0], 3)
    print("ROW " + json.dumps(row), flush=True)


def child(name, reps, script=None):
    """one workload in a process of its own, under its own time limit -> its rows; the first failure ends the run (script: another tool's file)"""
    p = subprocess.Popen([sys.executable, script or os.path.abspath(__file__), "--step", name, "--reps", str(reps)], stdout=subprocess.PIPE, text=True)
    late = []
    timer = threading.Timer(STEP_TIMEOUT, lambda: (late.append(True), p.kill()))
    timer.start()
    lines = []
    try:
        for ln in p.stdout:
            sys.stdout.write(ln)
            sys.stdout.flush()
            lines.append(ln)
        rc = p.wait()
    finally:
        timer.cancel()
    if late:
        raise SystemExit("FAILED: %s was not done within %d s; nothing more is started" % (name, STEP_TIMEOUT))
    if rc != 0:
        raise SystemExit("FAILED: %s ended with status %d; nothing more is started" % (name, rc))
    return [json.loads(ln[4:]) for ln in lines if ln.startswith("ROW ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated workload names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_lcp.json"))
    ap.add_argument("--step", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        run_one(args.step, args.reps)
        return
    names = list(BLOCKS) + [p[0] for p in PACKS]
    if args.only:
        names = [x for x in args.only.split(",") if x in names]
    rows = []
    if os.path.exists(args.out) and args.only:  # a run of some workloads replaces their rows and keeps the others
        with open(args.out) as f:
            rows = [r for r in json.load(f)["rows"] if r["name"] not in names]
    for name in names:
        rows += child(name, args.reps)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/lcp_throughput.py", reps=args.reps, rows=rows), f, indent=1)
    print(args.out)


if __name__ == "__main__":
    main()
