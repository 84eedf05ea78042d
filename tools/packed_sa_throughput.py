"""Packed suffix arrays against the per-block loop, and the BWT-only packed pass against the parent commit's.

For wiki_like, english_like and random_bytes cut into blocks of 64 KiB, 256 KiB, 1 MiB and 4 MiB, packed to 64 MiB, every cell records ms and
GB/s (median of --reps) of
  packed_sa      dk_dev_suffix_array_packed without L          packed_sa_l   the same with L and the origins
  packed_bwt     dk_dev_bwt_forward_packed on the same pack    loop_sa       dk_dev_suffix_array block by block
and, from one profiled packed_sa call, the emit kernel's time (slot k_bwt_gather), all kernels' time, the radix scatters' time, the rounds
and whether the guard fired.  The packed suffix arrays (with and without L) must equal the loop's and L / origins must equal
dk_dev_bwt_forward_packed's: anything else ends the run as a failure, it is not a number.

The A/B leg loads this tree's library and the parent commit's (--parent-lib; build the parent in a worktree with `python dark_amd/build.py`
and copy its libdark_amd.so to tools/_ab/parent.so) side by side and lets their dk_dev_bwt_forward_packed take turns on the same packs:
three repeats each, alternating.  The medians must differ by no more than the spread (max - min) of the parent's own three repeats.

Every GPU step (one source's cells, the A/B leg) is a child process under its own time limit; the run ends at the first that fails.

    python tools/packed_sa_throughput.py [--mib 64] [--reps 3] [--parent-lib FILE] [--out FILE] [--quick]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOURCES = ("wiki_like", "english_like", "random_bytes")
BLOCKS = (64 << 10, 256 << 10, 1 << 20, 4 << 20)
STEP_TIMEOUT = 420  # seconds per child: data generation on the host, then about a hundred packs and four per-block loops
AB_CELLS = (("wiki_like", 64 << 10), ("wiki_like", 1 << 20))
# "All of the pack's radix scatters together": the scatter passes of the large lists and the one-workgroup sorts of the short lists, which
# scatter inside the kernel.  k_radix_scatter_text is not one of them: a pack brackets only k_pk_init_keys there (it builds the first keys
# and scatters nothing), recorded beside it as init_keys_ms.
SCATTER_SLOTS = ("k_radix_scatter", "k_radix_sort_small")
AB_CALLS = 5  # calls per repeat (a pack takes 15-20 ms: one repeat times about 0.1 s of work)


def make_source(name, total):
    import numpy as np
    from dark_amd import datagen
    gen = {"wiki_like": lambda n: datagen.wiki_like(n, seed=2), "english_like": lambda n: datagen.english_like(n, seed=1),
           "random_bytes": lambda n: datagen.random_bytes(n, seed=50)}[name]
    return np.ascontiguousarray(gen(total), dtype=np.uint8)


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()  # every entry point returns after a synchronise of the library's stream
        ts.append(1e3 * (time.perf_counter() - t))
    return statistics.median(ts)


def cut(total, bs):
    return [min(bs, total - k) for k in range(0, total, bs)]


def run_source(name, total, reps, blocks):
    import numpy as np
    import torch
    import dark_amd
    data = make_source(name, total)
    d_in = torch.from_numpy(data).cuda()
    rows = []
    with dark_amd.Context(total) as ctx:
        for bs in blocks:
            sizes = cut(total, bs)
            offs = np.concatenate([[0], np.cumsum(sizes)])
            d_sa = torch.empty(total, dtype=torch.int32, device="cuda")
            d_sa_l = torch.empty(total, dtype=torch.int32, device="cuda")
            d_sa_loop = torch.empty(total, dtype=torch.int32, device="cuda")
            d_bwt = torch.empty(total, dtype=torch.uint8, device="cuda")
            d_bwt_ref = torch.empty(total, dtype=torch.uint8, device="cuda")

            def loop_sa():
                for i in range(len(sizes)):
                    a, b = int(offs[i]), int(offs[i + 1])
                    ctx.dev_suffix_array(d_in[a:b], sizes[i], d_sa_loop[a:b])

            # warm-up of every shape, and the check: a wrong result is a failure, not a number
            ctx.dev_suffix_array_packed(d_in, sizes, d_sa)
            origins = ctx.dev_suffix_array_packed(d_in, sizes, d_sa_l, d_bwt)
            want_origins = ctx.dev_bwt_forward_packed(d_in, sizes, d_bwt_ref)
            loop_sa()
            torch.cuda.synchronize()
            if not torch.equal(d_sa, d_sa_loop) or not torch.equal(d_sa_l, d_sa_loop):
                raise SystemExit("FAILED: %s, blocks of %d: the packed suffix arrays are not the per-block loop's" % (name, bs))
            if origins != want_origins or not torch.equal(d_bwt, d_bwt_ref):
                raise SystemExit("FAILED: %s, blocks of %d: L / origins are not dk_dev_bwt_forward_packed's" % (name, bs))
            ms = dict(packed_sa=median_ms(lambda: ctx.dev_suffix_array_packed(d_in, sizes, d_sa), reps),
                      packed_sa_l=median_ms(lambda: ctx.dev_suffix_array_packed(d_in, sizes, d_sa_l, d_bwt), reps),
                      packed_bwt=median_ms(lambda: ctx.dev_bwt_forward_packed(d_in, sizes, d_bwt_ref), reps),
                      loop_sa=median_ms(loop_sa, reps))
            prof = {}
            for what, bwt in (("sa", None), ("sa_l", d_bwt)):
                ctx.stats_reset()
                ctx.set_profiling(True)
                ctx.dev_suffix_array_packed(d_in, sizes, d_sa, bwt)
                st = ctx.stats()
                ctx.set_profiling(False)
                k = st["kernels"]
                prof[what] = dict(emit_ms=round(k["k_bwt_gather"]["ms"], 3), emit_launches=k["k_bwt_gather"]["launches"],
                                  all_kernels_ms=round(sum(v["ms"] for v in k.values()), 3),
                                  radix_scatter_ms=round(sum(k.get(s, {}).get("ms", 0.0) for s in SCATTER_SLOTS), 3),
                                  init_keys_ms=round(k.get("k_radix_scatter_text", {}).get("ms", 0.0), 3),
                                  launches=sum(v["launches"] for v in k.values()), rounds=st["rounds"], guard="packed_guard" in st["routes"])
            row = dict(source=name, block_bytes=bs, blocks=len(sizes), pack_bytes=total)
            for key, v in ms.items():
                row[key + "_ms"] = round(v, 3)
                row[key + "_GBps"] = round(total / 1e6 / v, 3)
            row["speedup_over_loop"] = round(ms["loop_sa"] / ms["packed_sa"], 2)
            row["rounds"], row["guard"] = prof["sa"]["rounds"], prof["sa"]["guard"]
            row["emit_ms"], row["emit_with_l_ms"] = prof["sa"]["emit_ms"], prof["sa_l"]["emit_ms"]
            row["emit_share_of_kernels"] = round(prof["sa"]["emit_ms"] / prof["sa"]["all_kernels_ms"], 4)
            row["profile"] = prof
            print("ROW " + json.dumps(row), flush=True)
            rows.append(row)
    return rows


def run_ab(parent_lib, total, cells):
    import numpy as np
    import torch
    this_lib = os.environ.get("DARK_AMD_LIB") or os.path.join(ROOT, "dark_amd", "libdark_amd.so")
    libs = []
    for name, path in (("parent", parent_lib), ("this", this_lib)):
        lib = ctypes.CDLL(os.path.abspath(path), mode=ctypes.RTLD_LOCAL)
        lib.dk_ctx_create.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
        lib.dk_dev_bwt_forward_packed.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        lib.dk_ctx_destroy.argtypes = [ctypes.c_void_p]
        ctx = ctypes.c_void_p()
        rc = lib.dk_ctx_create(0, total, ctypes.byref(ctx))
        assert rc == 0, (name, rc)
        libs.append(dict(name=name, lib=lib, ctx=ctx))
    rows, cache = [], {}
    for src, bs in cells:
        if src not in cache:
            cache[src] = torch.from_numpy(make_source(src, total)).cuda()
        d_in = cache[src]
        sizes = cut(total, bs)
        ns = (ctypes.c_size_t * len(sizes))(*sizes)
        outs = {}
        for L in libs:
            L["d_bwt"] = torch.empty(total, dtype=torch.uint8, device="cuda")
            L["origin"] = np.zeros(len(sizes), dtype=np.uint32)
            L["ms"] = []
        torch.cuda.synchronize()

        def call(L):
            rc = L["lib"].dk_dev_bwt_forward_packed(L["ctx"], d_in.data_ptr(), len(sizes), ns, L["d_bwt"].data_ptr(), L["origin"].ctypes.data)
            assert rc == 0, (L["name"], rc)

        for L in libs:  # warm-up, and the same bytes from both
            call(L)
            outs[L["name"]] = (L["d_bwt"].clone(), L["origin"].copy())
        if not torch.equal(outs["parent"][0], outs["this"][0]) or not np.array_equal(outs["parent"][1], outs["this"][1]):
            raise SystemExit("FAILED: %s, blocks of %d: dk_dev_bwt_forward_packed differs from the parent's" % (src, bs))
        for _ in range(3):  # three repeats each, taking turns
            for L in libs:
                t = time.perf_counter()
                for _ in range(AB_CALLS):
                    call(L)
                L["ms"].append(1e3 * (time.perf_counter() - t) / AB_CALLS)
        parent, this = libs[0]["ms"], libs[1]["ms"]
        spread = max(parent) - min(parent)
        diff = statistics.median(this) - statistics.median(parent)
        row = dict(source=src, block_bytes=bs, pack_bytes=total, calls_per_repeat=AB_CALLS, parent_ms=[round(x, 3) for x in parent],
                   this_ms=[round(x, 3) for x in this], parent_median_ms=round(statistics.median(parent), 3),
                   this_median_ms=round(statistics.median(this), 3), parent_spread_ms=round(spread, 3), difference_ms=round(diff, 3),
                   within_parent_spread=bool(abs(diff) <= spread))
        print("ROW " + json.dumps(row), flush=True)
        rows.append(row)
    for L in libs:
        L["lib"].dk_ctx_destroy(L["ctx"])
    return rows


def child(args, what):
    """one GPU step in a process of its own, under its own time limit -> its rows; the first failure ends the run"""
    cmd = [sys.executable, os.path.abspath(__file__), "--step", what, "--mib", str(args.mib), "--reps", str(args.reps), "--parent-lib", args.parent_lib]
    if args.quick:
        cmd.append("--quick")
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
    late = []
    timer = threading.Timer(STEP_TIMEOUT, lambda: (late.append(True), p.kill()))
    timer.start()
    lines = []
    try:
        for ln in p.stdout:  # every row is shown as it arrives
            sys.stdout.write(ln)
            sys.stdout.flush()
            lines.append(ln)
        rc = p.wait()
    finally:
        timer.cancel()
    if late:
        raise SystemExit("FAILED: step %s was not done within %d s; nothing more is started" % (what, STEP_TIMEOUT))
    if rc != 0:
        raise SystemExit("FAILED: step %s ended with status %d; nothing more is started" % (what, rc))
    return [json.loads(ln[4:]) for ln in lines if ln.startswith("ROW ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="wiki_like only, blocks of 64 KiB and 1 MiB")
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "tools", "_ab", "parent.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_packed_sa.json"))
    ap.add_argument("--step", help=argparse.SUPPRESS)
    args = ap.parse_args()
    total = args.mib << 20
    blocks = (64 << 10, 1 << 20) if args.quick else BLOCKS
    if args.step == "ab":
        run_ab(args.parent_lib, total, AB_CELLS)
        return
    if args.step:
        run_source(args.step, total, args.reps, blocks)
        return
    if not os.path.exists(args.parent_lib):
        raise SystemExit("no parent library at %s: build the parent commit in a worktree and copy its libdark_amd.so there" % args.parent_lib)
    rows = []
    for name in SOURCES[:1] if args.quick else SOURCES:
        rows += child(args, name)
    ab = child(args, "ab")
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/packed_sa_throughput.py", reps=args.reps, pack_bytes=total, rows=rows, bwt_packed_parent_against_this=ab), f, indent=1)
    print(args.out)
    if not all(r["within_parent_spread"] for r in ab):
        raise SystemExit("FAILED: dk_dev_bwt_forward_packed's median moved by more than the spread of the parent's repeats (see %s)" % args.out)


if __name__ == "__main__":
    main()
