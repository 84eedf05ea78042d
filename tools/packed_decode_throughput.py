"""Packed inverse against the per-block loop, in one process; the decode twin of tools/packed_throughput.py.

For wiki_like, english_like and random_bytes (0xFF mapped to 0xFE: such blocks cannot be decoded) cut into blocks of 64 KiB, 256 KiB, 1 MiB and
4 MiB, packed to about 64 MiB:
  (a) device inverse, MB/s: dk_dev_bwt_inverse_packed against a loop of dk_dev_bwt_inverse over the same blocks, and against ONE
      dk_dev_bwt_inverse of the same bytes taken as a single block (what segmentation should cost nothing against);
  (b) end-to-end decode, MB/s, models exp and dark: dk_dev_packed_decode against dk_dev_batch_decode, same host threads;
  launches per pack from one profiled packed inverse.  Median of --reps runs.  Writes JSON (default profiles/r07_packed_decode.json).

    python tools/packed_decode_throughput.py [--mib 64] [--reps 3] [--threads 15] [--out FILE] [--quick] [--no-e2e]
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
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=15)
    ap.add_argument("--quick", action="store_true", help="wiki_like, 64 KiB blocks only")
    ap.add_argument("--no-e2e", action="store_true", help="device legs only")
    ap.add_argument("--one-pack", action="store_true", help="one packed forward and ONE packed inverse of a wiki_like pack of 64 KiB blocks, "
                    "nothing else (for a kernel trace: every k_ibwt_* / k_pib_* dispatch is the inverse's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_packed_decode.json"))
    args = ap.parse_args()
    total = args.mib << 20
    if args.one_pack:
        data = np.ascontiguousarray(SOURCES["wiki_like"](total), dtype=np.uint8)
        sizes = [min(64 << 10, total - k) for k in range(0, total, 64 << 10)]
        with dark_amd.Context(total) as ctx:
            d_in = torch.from_numpy(data).cuda()
            d_bwt = torch.empty(total, dtype=torch.uint8, device="cuda")
            origins = ctx.dev_bwt_forward_packed(d_in, sizes, d_bwt)
            d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
            ctx.dev_bwt_inverse_packed(d_bwt, sizes, origins, d_out)
            assert torch.equal(d_out, d_in)
        return
    rows = []
    with dark_amd.Context(total) as ctx:
        for src_name, gen in SOURCES.items():
            if args.quick and src_name != "wiki_like":
                continue
            data = np.ascontiguousarray(gen(total), dtype=np.uint8)
            data = np.where(data == 255, 254, data).astype(np.uint8)
            d_in = torch.from_numpy(data).cuda()
            # the same bytes as one block: the yardstick of the segmented pass
            d_one = torch.empty(total, dtype=torch.uint8, device="cuda")
            origin_one = ctx.dev_bwt_forward(d_in, total, d_one)
            d_back = torch.empty(total, dtype=torch.uint8, device="cuda")
            ms_one = median_ms(lambda: ctx.dev_bwt_inverse(d_one, total, origin_one, d_back), args.reps)
            assert torch.equal(d_back, d_in)
            for bs in BLOCKS:
                if args.quick and bs != (64 << 10):
                    continue
                sizes = [min(bs, total - k) for k in range(0, total, bs)]
                offs = np.concatenate([[0], np.cumsum(sizes)])
                d_bwt = torch.empty(total, dtype=torch.uint8, device="cuda")
                origins = ctx.dev_bwt_forward_packed(d_in, sizes, d_bwt)
                d_out = torch.empty(total, dtype=torch.uint8, device="cuda")

                def packed_inv():
                    ctx.dev_bwt_inverse_packed(d_bwt, sizes, origins, d_out)

                def loop_inv():
                    for i in range(len(sizes)):
                        a, b = int(offs[i]), int(offs[i + 1])
                        ctx.dev_bwt_inverse(d_bwt[a:b], sizes[i], origins[i], d_out[a:b])

                packed_inv()
                assert torch.equal(d_out, d_in)
                loop_inv()
                ms_p, ms_l = median_ms(packed_inv, args.reps), median_ms(loop_inv, args.reps)
                ctx.stats_reset()
                ctx.set_profiling(True)
                packed_inv()
                st = ctx.stats()
                ctx.set_profiling(False)
                launches = sum(k["launches"] for k in st["kernels"].values())
                row = dict(source=src_name, block_bytes=bs, blocks=len(sizes), pack_bytes=total,
                           inverse_packed_ms=round(ms_p, 3), inverse_loop_ms=round(ms_l, 3), inverse_one_block_ms=round(ms_one, 3),
                           inverse_packed_MBps=round(total / 1e3 / ms_p, 1), inverse_loop_MBps=round(total / 1e3 / ms_l, 1),
                           inverse_speedup=round(ms_l / ms_p, 2), packed_over_one_block=round(ms_p / ms_one, 2),
                           launches_per_pack=launches, kernels_ms={k: round(v["ms"], 3) for k, v in st["kernels"].items()})
                if not args.quick and not args.no_e2e:
                    views = [d_in[int(offs[i]):int(offs[i + 1])] for i in range(len(sizes))]
                    outs = [d_out[int(offs[i]):int(offs[i + 1])] for i in range(len(sizes))]
                    for model in ("exp", "dark"):
                        streams, _ = ctx.dev_packed_encode(model, d_in, sizes, host_threads=args.threads)
                        streams = [np.array(s) for s in streams]
                        ms_pd = median_ms(lambda: ctx.dev_packed_decode(model, streams, sizes, d_out, host_threads=args.threads), args.reps)
                        assert torch.equal(d_out, d_in)
                        ms_bd = median_ms(lambda: ctx.dev_batch_decode(model, streams, sizes, outs, host_threads=args.threads), args.reps)
                        assert torch.equal(d_out, d_in)
                        row["decode_%s_packed_MBps" % model] = round(total / 1e3 / ms_pd, 1)
                        row["decode_%s_batch_MBps" % model] = round(total / 1e3 / ms_bd, 1)
                    del views, outs
                print(json.dumps(row), flush=True)
                rows.append(row)
            del d_in
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/packed_decode_throughput.py", reps=args.reps, host_threads=args.threads, rows=rows), f, indent=1)
    print(args.out)


if __name__ == "__main__":
    main()
