"""FM-index find on the GPU beside the route the count and locate entries offer for the same question, and the archive search beside decoding the
archive and searching the output.  The numbers are RECORDED, NOT GATED.

device    pack_64KiB (64 MiB of wiki_like text as 1024 blocks of 64 KiB) with 1024 patterns of 8 bytes cut from the text: every pattern in every
          block, 2^20 pairs.  find: one dk_dev_fm_find_packed and the download of the records.  The other route: the patterns replicated per block
          through dk_dev_fm_count_packed (a pat_block word per query), dk_dev_fm_locate_packed at a fixed stride (the largest occurrence count, which
          that route learns from the ranges), the download of pairs x stride words and the host filter that drops DK_FM_NO_HIT.  EVERY answer of
          the two routes is compared before anything is timed.  Times are wall time around the calls (they synchronise) and, for the library's
          share, dk_stats.ms_total.
archive   --archive-mib MiB of the same text encoded with -b 65536 --packed; `--grep` with four patterns (grep_file: decode to (L, origin) on the
          host, upload, index and structures, find, context extraction) beside decode_file --packed plus bytes.find over the output.  The hit
          lists are compared (the search leaves out matches across block borders; the comparison does the same).

Each part is a child process under its own time limit; the run ends at the first that fails.

    python tools/fm_find_throughput.py [--reps 3] [--only device,archive] [--archive-mib 16] [--out FILE]
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lcp_throughput import child, make_block, median_ms  # noqa: E402
from sa_query_throughput import library_ms, profiled  # noqa: E402

PACK_BLOCK = 64 << 10
NPAT, PAT_BYTES = 1024, 8
STEP = 32


def run_device(reps):
    import numpy as np
    import torch
    import dark_amd
    from dark_amd._lib import FM_NO_HIT
    from dark_amd.context import FM_HIT_DTYPE, fm_index_bytes, fm_locate_bytes
    data = make_block("pack_64KiB")
    n = len(data)
    sizes = [min(PACK_BLOCK, n - k) for k in range(0, n, PACK_BLOCK)]
    count = len(sizes)
    rng = np.random.default_rng(1)
    starts = rng.integers(0, n - PAT_BYTES, size=NPAT)
    starts -= np.maximum((starts % PACK_BLOCK) + PAT_BYTES - PACK_BLOCK, 0)  # (inside one block each)
    pats = np.concatenate([data[a:a + PAT_BYTES] for a in starts])
    lens = [PAT_BYTES] * NPAT
    d_in = torch.from_numpy(data).cuda()
    d_bwt = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_pat = torch.from_numpy(pats).cuda()
    npairs = NPAT * count
    with dark_amd.Context(n) as ctx:
        origins = ctx.dev_bwt_forward_packed(d_in, sizes, d_bwt)
        d_index = torch.empty(fm_index_bytes(n, count) // 4, dtype=torch.int32, device="cuda")
        d_loc = torch.empty(fm_locate_bytes(n, count, STEP) // 4, dtype=torch.int32, device="cuda")
        ctx.dev_fm_build_packed(d_bwt, sizes, origins, d_index)
        ctx.dev_fm_locate_build_packed(d_bwt, sizes, origins, STEP, d_loc)
        # find: the total first (it sizes the records), then the list
        d_occ = torch.empty(npairs, dtype=torch.int32, device="cuda")
        total = ctx.dev_fm_find_packed(d_bwt, sizes, d_index, None, STEP, d_pat, lens, 0, None, d_occ)
        d_hits = torch.empty(4 * total, dtype=torch.int32, device="cuda")

        def find():
            got = ctx.dev_fm_find_packed(d_bwt, sizes, d_index, d_loc, STEP, d_pat, lens, total, d_hits, d_occ)
            return got, d_hits.cpu().numpy().view(FM_HIT_DTYPE)
        # the other route: the queries replicated, a fixed stride, the host filter
        rep_pat = d_pat.view(NPAT, PAT_BYTES).repeat_interleave(count, dim=0).contiguous().view(-1)
        rep_lens = [PAT_BYTES] * npairs
        rep_blocks = np.tile(np.arange(count, dtype=np.uint32), NPAT)
        d_lo = torch.empty(npairs, dtype=torch.int32, device="cuda")
        d_hi = torch.empty(npairs, dtype=torch.int32, device="cuda")
        inside = {}

        def other():
            ctx.dev_fm_count_packed(d_bwt, sizes, d_index, rep_pat, rep_lens, rep_blocks, d_lo, d_hi)
            inside["count"] = ctx.stats()["ms_total"]
            stride = int((d_hi - d_lo).max())
            d_pos = torch.empty(npairs * stride, dtype=torch.int32, device="cuda")
            ctx.dev_fm_locate_packed(d_bwt, sizes, d_index, d_loc, STEP, d_lo, d_hi, rep_blocks, stride, d_pos)
            inside["locate"] = ctx.stats()["ms_total"]
            rows = d_pos.cpu().numpy().view(np.uint32).reshape(npairs, stride)
            pair, j = np.nonzero(rows != FM_NO_HIT)
            return stride, pair, j, rows[pair, j]
        got_total, recs = find()
        stride, pair, j, pos = other()
        lo = d_lo.cpu().numpy().view(np.uint32)
        same = (got_total == total == len(pair) and np.array_equal(recs["pattern"], pair // count) and np.array_equal(recs["block"], pair % count) and
                np.array_equal(recs["position"], pos) and np.array_equal(recs["slot"], lo[pair] + j) and
                np.array_equal(d_occ.cpu().numpy(), (d_hi - d_lo).cpu().numpy()))
        if not same:
            raise SystemExit("FAILED: find and count + locate + filter differ (%d records, %d filtered)" % (len(recs), len(pair)))
        find_ms, find_runs = median_ms(find, reps)
        find_lib_ms, _ = library_ms(ctx, find, reps)
        other_ms, other_runs = median_ms(other, reps)
        print("ROW " + json.dumps(dict(name="pack_64KiB", kind="device", bytes=n, blocks=count, patterns=NPAT, pattern_bytes=PAT_BYTES, pairs=npairs,
                                       hits=total, step=STEP, answers_equal=True, find_ms=round(find_ms, 3), find_runs_ms=find_runs,
                                       find_library_ms=round(find_lib_ms, 3), find_record_bytes=16 * total,
                                       count_locate_filter_ms=round(other_ms, 3), count_locate_filter_runs_ms=other_runs,
                                       count_library_ms=round(inside["count"], 3), locate_library_ms=round(inside["locate"], 3), locate_stride=stride,
                                       locate_row_bytes=4 * npairs * stride, find_over_other=round(find_ms / other_ms, 3),
                                       slots=profiled(ctx, find))), flush=True)


def run_archive(reps, mib):
    import numpy as np
    from dark_amd import cli
    data = make_block("pack_64KiB")[:mib << 20]
    text = data.tobytes()
    rng = np.random.default_rng(2)
    patterns = [text[a:a + PAT_BYTES] for a in rng.integers(0, len(text) - PAT_BYTES, size=4).tolist()]
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as work:
        os.chdir(work)
        try:
            with open("corpus.txt", "wb") as f:
                f.write(text)
            t = time.perf_counter()
            cli.encode_file("corpus.txt", "exp", PACK_BLOCK, packed=True)
            encode_ms = 1e3 * (time.perf_counter() - t)

            def search():
                out = io.StringIO()
                cli.grep_file("corpus.dark", "exp", patterns, out=out)
                return out.getvalue().splitlines()

            def decode_and_find():
                cli.decode_file("corpus.dark", "exp", packed=True)
                with open("corpus.orig", "rb") as f:
                    back = f.read()
                hits = []
                for q, p in enumerate(patterns):
                    i = back.find(p)
                    while i >= 0:
                        hits.append((i, q))
                        i = back.find(p, i + 1)
                return back, sorted(hits)
            lines = search()
            back, hits = decode_and_find()
            inside = [(i, q) for i, q in hits if i // PACK_BLOCK == (i + PAT_BYTES - 1) // PACK_BLOCK]
            if back != text or [tuple(int(x) for x in ln.split(":")[:2]) for ln in lines] != inside:
                raise SystemExit("FAILED: the search lists %d hits, decode + bytes.find %d inside a block" % (len(lines), len(inside)))
            search_ms, search_runs = median_ms(search, reps)
            decode_ms, decode_runs = median_ms(decode_and_find, reps)
            st = {}
            cli.grep_file("corpus.dark", "exp", patterns, stats=st, out=io.StringIO())
            print("ROW " + json.dumps(dict(name="pack_64KiB[:%d MiB]" % mib, kind="archive", bytes=len(text), blocks=-(-len(text) // PACK_BLOCK),
                                           archive_bytes=os.path.getsize("corpus.dark"), patterns=len(patterns), hits=len(lines),
                                           hits_across_borders_not_found=len(hits) - len(inside), answers_equal=True, encode_ms=round(encode_ms, 1),
                                           search_ms=round(search_ms, 1), search_runs_ms=search_runs, decode_and_find_ms=round(decode_ms, 1),
                                           decode_and_find_runs_ms=decode_runs, search_over_decode=round(search_ms / decode_ms, 3),
                                           resident_bytes=st.get("resident_bytes", 0))), flush=True)
        finally:
            os.chdir(here)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated parts: device, archive (default: both)")
    ap.add_argument("--archive-mib", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_fm_find.json"))
    ap.add_argument("--step", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        part, _, mib = args.step.partition("@")
        return run_device(args.reps) if part == "device" else run_archive(args.reps, int(mib))
    rows = []
    for part in ("device", "archive"):
        if args.only and part not in args.only.split(","):
            continue
        rows += child("%s@%d" % (part, args.archive_mib), args.reps, script=os.path.abspath(__file__))
        with open(args.out, "w") as f:  # (after every part: a run that is cut short keeps what it has)
            json.dump(dict(tool="tools/fm_find_throughput.py", reps=args.reps, rows=rows), f, indent=1)
    print(args.out)


if __name__ == "__main__":
    main()
