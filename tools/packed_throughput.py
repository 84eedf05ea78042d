"""Packed forward path against the per-block loop, in one process.

For wiki_like, english_like and random_bytes cut into blocks of 64 KiB, 256 KiB, 1 MiB and 4 MiB, packed to about 64 MiB:
  (a) device forward (BWT + DC), MB/s: dk_dev_bwt_forward_packed + dk_dev_dc_encode_packed against a loop of dk_dev_bwt_forward +
      dk_dev_dc_encode over the same blocks;
  (b) end-to-end encode, MB/s, models exp and dark: dk_dev_packed_encode against dk_dev_batch_encode, same host threads;
  launches per pack from one profiled packed forward.  Median of --reps runs.  Writes JSON (default profiles/r06_packed_throughput.json).

    python tools/packed_throughput.py [--mib 64] [--reps 5] [--threads 15] [--out FILE] [--quick]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import dark_amd  # noqa: E402
from dark_amd import datagen  # noqa: E402

SOURCES = {"wiki_like": lambda n: datagen.wiki_like(n, seed=2), "english_like": lambda n: datagen.english_like(n, seed=1),
           "random_bytes": lambda n: datagen.random_bytes(n, seed=50)}
BLOCKS = (64 << 10, 256 << 10, 1 << 20, 4 << 20)


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=15)
    ap.add_argument("--quick", action="store_true", help="one source, 1 MiB blocks only, no end-to-end leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_packed_throughput.json"))
    args = ap.parse_args()
    total = args.mib << 20
    rows = []
    with dark_amd.Context(total) as ctx:
        for src_name, gen in SOURCES.items():
            if args.quick and src_name != "wiki_like":
                continue
            data = np.ascontiguousarray(gen(total), dtype=np.uint8)
            if src_name != "random_bytes":
                data = np.where(data == 255, 254, data).astype(np.uint8)
            d_in = torch.from_numpy(data).cuda()
            for bs in BLOCKS:
                if args.quick and bs != (1 << 20):
                    continue
                sizes = [min(bs, total - k) for k in range(0, total, bs)]
                offs = np.concatenate([[0], np.cumsum(sizes)])
                views = [d_in[int(offs[i]):int(offs[i + 1])] for i in range(len(sizes))]
                d_bwt = torch.empty(total, dtype=torch.uint8, device="cuda")
                d_dist = torch.empty(total, dtype=torch.int32, device="cuda")
                d_sym = torch.empty(total, dtype=torch.uint8, device="cuda")

                def packed_fwd():
                    ctx.dev_bwt_forward_packed(d_in, sizes, d_bwt)
                    ctx.dev_dc_encode_packed(d_bwt, sizes, d_dist, d_sym)

                def loop_fwd():
                    for i, v in enumerate(views):
                        a, b = int(offs[i]), int(offs[i + 1])
                        ctx.dev_bwt_forward(v, sizes[i], d_bwt[a:b])
                        ctx.dev_dc_encode(d_bwt[a:b], sizes[i], d_dist[a:b], d_sym[a:b])

                packed_fwd()
                loop_fwd()
                ms_p, ms_l = median_ms(packed_fwd, args.reps), median_ms(loop_fwd, args.reps)
                ctx.stats_reset()
                ctx.set_profiling(True)
                ctx.dev_bwt_forward_packed(d_in, sizes, d_bwt)
                st_bwt = ctx.stats()
                ctx.dev_dc_encode_packed(d_bwt, sizes, d_dist, d_sym)
                st = ctx.stats()
                ctx.set_profiling(False)
                launches = sum(k["launches"] for k in st["kernels"].values())
                row = dict(source=src_name, block_bytes=bs, blocks=len(sizes), pack_bytes=total,
                           forward_packed_MBps=round(total / 1e3 / ms_p, 1), forward_loop_MBps=round(total / 1e3 / ms_l, 1),
                           forward_speedup=round(ms_l / ms_p, 2), launches_per_pack=launches, rounds=st_bwt["rounds"],
                           guard="packed_guard" in st_bwt["routes"],
                           kernels_ms={k: round(v["ms"], 3) for k, v in st["kernels"].items()})
                if not args.quick:
                    for model in ("exp", "dark"):
                        if src_name == "random_bytes" and model == "exp" and bs > (1 << 24):
                            continue
                        ms_pe = median_ms(lambda: ctx.dev_packed_encode(model, d_in, sizes, host_threads=args.threads), args.reps)
                        ms_be = median_ms(lambda: ctx.dev_batch_encode(model, views, sizes, host_threads=args.threads), args.reps)
                        row["encode_%s_packed_MBps" % model] = round(total / 1e3 / ms_pe, 1)
                        row["encode_%s_batch_MBps" % model] = round(total / 1e3 / ms_be, 1)
                print(json.dumps(row), flush=True)
                rows.append(row)
            del d_in
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/packed_throughput.py", reps=args.reps, host_threads=args.threads, rows=rows), f, indent=1)
    print(args.out)


if __name__ == "__main__":
    main()
