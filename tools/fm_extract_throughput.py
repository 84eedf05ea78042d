"""FM-index extract on the GPU: time of the extract structure's build beside the inverse BWT and the locate structure's build of the same input,
and bytes per second of dk_dev_fm_extract beside a gather from the resident text.

Inputs: enwik8_like_1e8, acgt_2p28, and a 64 MiB pack of 1024 blocks of 64 KiB (those of tools/fm_locate_throughput.py).
Per input and anchor step: the median of --reps runs of dk_dev_fm_extract_build (_packed) beside dk_dev_bwt_inverse (_packed) and
dk_dev_fm_locate_build (_packed) on the same L.  Then 2^20 ranges of 16 and 256 bytes at random starts, beside a torch gather of the same
bytes from the text; then the whole block (every block of the pack) through one range each, beside the inverse.  EVERY extracted byte is
compared with the text before anything is timed.  The times of the library's calls are dk_stats.ms_total, the time inside the entry point;
the gather is timed around a synchronise.  Resident bytes per route are arithmetic.

Every input is a child process under its own time limit; the run ends at the first that fails.

    python tools/fm_extract_throughput.py [--reps 3] [--only NAME[,NAME]] [--steps 8,32,128] [--out FILE]
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
NRANGE = 1 << 20
LENGTHS = (16, 256)
PACK_BLOCK = 64 << 10


def run_one(spec, reps):
    import statistics
    import numpy as np
    import torch
    import dark_amd
    from dark_amd.context import fm_extract_bytes, fm_index_bytes, fm_locate_bytes
    name, _, steps = spec.partition("@")
    steps = [int(s) for s in steps.split(",")]
    data = make_block(name)
    n = len(data)
    packed = name.startswith("pack_")
    sizes = [min(PACK_BLOCK, n - k) for k in range(0, n, PACK_BLOCK)] if packed else [n]
    d_in = torch.from_numpy(data).cuda()
    d_bwt, d_out = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    index_bytes = fm_index_bytes(n, len(sizes))
    d_index = torch.empty(index_bytes // 4, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(1)
    with dark_amd.Context(n) as ctx:
        if packed:
            origins = ctx.dev_bwt_forward_packed(d_in, sizes, d_bwt)
            inverse = lambda: ctx.dev_bwt_inverse_packed(d_bwt, sizes, origins, d_out)  # noqa: E731
            ctx.dev_fm_build_packed(d_bwt, sizes, origins, d_index)
        else:
            origins = [ctx.dev_bwt_forward(d_in, n, d_bwt)]
            inverse = lambda: ctx.dev_bwt_inverse(d_bwt, n, origins[0], d_out)  # noqa: E731
            ctx.dev_fm_build(d_bwt, n, origins[0], d_index)
        inverse()
        if not torch.equal(d_out, d_in):
            raise SystemExit("FAILED: %s: the inverse BWT does not give the text back" % name)
        inverse_ms, inverse_all = median_ms(inverse, reps)
        # the ranges, once for all steps: block, start local to it, and the start in the pack for the gather
        batches = []
        for m in LENGTHS:
            blocks = rng.integers(0, len(sizes), size=NRANGE)
            local = (rng.random(NRANGE) * (np.asarray(sizes, np.int64)[blocks] - m)).astype(np.int64)
            batches.append((m, blocks.tolist() if packed else None, torch.from_numpy(local.astype(np.int32)).cuda(),
                            torch.from_numpy(np.asarray(blocks, np.int64) * PACK_BLOCK + local).cuda()))
        whole_len = max(sizes)
        d_zero = torch.zeros(len(sizes), dtype=torch.int32, device="cuda")
        for step in steps:
            ext_bytes, loc_bytes = fm_extract_bytes(n, len(sizes), step), fm_locate_bytes(n, len(sizes), step)
            d_ext = torch.empty(ext_bytes // 4, dtype=torch.int32, device="cuda")
            d_loc = torch.empty(loc_bytes // 4, dtype=torch.int32, device="cuda")
            if packed:
                build = lambda: ctx.dev_fm_extract_build_packed(d_bwt, sizes, origins, step, d_ext)  # noqa: E731
                locate_build = lambda: ctx.dev_fm_locate_build_packed(d_bwt, sizes, origins, step, d_loc)  # noqa: E731
            else:
                build = lambda: ctx.dev_fm_extract_build(d_bwt, n, origins[0], step, d_ext)  # noqa: E731
                locate_build = lambda: ctx.dev_fm_locate_build(d_bwt, n, origins[0], step, d_loc)  # noqa: E731
            locate_build()
            locate_ms, locate_all = median_ms(locate_build, reps)
            del d_loc
            build()
            build_ms, build_all = median_ms(build, reps)
            print("ROW " + json.dumps(dict(name=name, kind="build", step=step, bytes=n, blocks=len(sizes), extract_build_ms=round(build_ms, 3),
                                           extract_build_runs_ms=build_all, bwt_inverse_ms=round(inverse_ms, 3), bwt_inverse_runs_ms=inverse_all,
                                           locate_build_ms=round(locate_ms, 3), locate_build_runs_ms=locate_all,
                                           build_over_inverse=round(build_ms / inverse_ms, 3), build_over_locate_build=round(build_ms / locate_ms, 3),
                                           extract_bytes=ext_bytes, index_bytes=index_bytes, resident_fm_extract_bytes=n + index_bytes + ext_bytes,
                                           resident_text_sa_bytes=5 * n, slots=profiled(ctx, build))), flush=True)
            for m, where, d_local, d_global in batches:
                d_rows = torch.empty(NRANGE * m, dtype=torch.uint8, device="cuda")
                if packed:
                    extract = lambda: ctx.dev_fm_extract_packed(d_bwt, sizes, d_index, d_ext, step, d_local, None, where, m, d_rows)  # noqa: E731
                else:
                    extract = lambda: ctx.dev_fm_extract(d_bwt, n, d_index, d_ext, step, d_local, None, NRANGE, m, d_rows)  # noqa: E731

                def gather():
                    got = d_in[d_global[:, None] + torch.arange(m, device="cuda")[None, :]]
                    torch.cuda.synchronize()
                    return got
                extract()
                want = gather()
                if not torch.equal(d_rows.view(NRANGE, m), want):
                    bad = int((d_rows.view(NRANGE, m) != want).sum())
                    raise SystemExit("FAILED: %s step %d, ranges of %d bytes: %d bytes differ from the text's" % (name, step, m, bad))
                del want
                fm_ms, fm_runs = library_ms(ctx, extract, reps)
                ts = []
                for _ in range(reps):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    gather()
                    ts.append(1e3 * (time.perf_counter() - t))
                gather_ms = statistics.median(ts)
                print("ROW " + json.dumps(dict(name=name, kind="ranges", step=step, bytes=n, blocks=len(sizes), ranges=NRANGE, range_bytes=m,
                                               answers_equal=True, fm_extract_ms=round(fm_ms, 3), fm_extract_runs_ms=fm_runs,
                                               ns_per_range=round(1e6 * fm_ms / NRANGE, 2), ms_per_lf_step_unit=round(fm_ms / (m + step / 2), 4),
                                               fm_MB_per_s=round(NRANGE * m / 1e3 / fm_ms, 2), text_gather_ms=round(gather_ms, 3),
                                               text_gather_MB_per_s=round(NRANGE * m / 1e3 / gather_ms, 2))), flush=True)
                del d_rows
            # the whole block (every block of the pack) through one range each
            d_rows = torch.empty(len(sizes) * whole_len, dtype=torch.uint8, device="cuda")
            if packed:
                whole = lambda: ctx.dev_fm_extract_packed(d_bwt, sizes, d_index, d_ext, step, d_zero, None, list(range(len(sizes))), whole_len, d_rows)  # noqa: E731
            else:
                whole = lambda: ctx.dev_fm_extract(d_bwt, n, d_index, d_ext, step, d_zero, None, 1, whole_len, d_rows)  # noqa: E731
            whole()
            rows = d_rows.view(len(sizes), whole_len)
            for b in ([0] if not packed else range(len(sizes))):
                if not torch.equal(rows[b, :sizes[b]], d_in[b * PACK_BLOCK:b * PACK_BLOCK + sizes[b]]) or bool(rows[b, sizes[b]:].any()):
                    raise SystemExit("FAILED: %s step %d: block %d through one range is not its text" % (name, step, b))
            whole_ms, whole_runs = library_ms(ctx, whole, reps)
            print("ROW " + json.dumps(dict(name=name, kind="whole", step=step, bytes=n, blocks=len(sizes), answers_equal=True,
                                           fm_extract_ms=round(whole_ms, 3), fm_extract_runs_ms=whole_runs, fm_MB_per_s=round(n / 1e3 / whole_ms, 2),
                                           bwt_inverse_ms=round(inverse_ms, 3), extract_over_inverse=round(whole_ms / inverse_ms, 2))), flush=True)
            del d_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated input names (default: all)")
    ap.add_argument("--steps", default="8,32,128", help="comma-separated anchor steps, powers of two in [1, 4096]")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_fm_extract.json"))
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
            json.dump(dict(tool="tools/fm_extract_throughput.py", reps=args.reps, steps=args.steps, rows=rows), f, indent=1)
    print(args.out)


if __name__ == "__main__":
    main()
