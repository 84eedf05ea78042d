"""FM-index seams on the GPU beside find on the same pack and patterns, and the archive search with and without --across-blocks (DESIGN.md section
4.17).  The numbers are RECORDED, NOT GATED; find's times from the same run are the yardstick.

pack64k   pack_64KiB (64 MiB of wiki_like text as 1024 blocks of 64 KiB) with 1024 patterns of 8 bytes, half of them cut across a border: one
          dk_dev_fm_seams_packed with the download of its records beside one dk_dev_fm_find_packed with the download of its.
pack1k    the same text as 65536 blocks of 1 KiB and the same patterns: 2^26 pairs, four calls of 256 patterns each (DK_FM_FIND_MAX_PAIRS), about
          4.7e8 candidates in all; find in the same four calls.
          In both, EVERY seam record is compared with an enumeration on the host before anything is timed: the 14 bytes around every border,
          every `back`, looked up among the patterns.
archive   --archive-mib MiB of the same text encoded with -b 65536 --packed; grep_file with four patterns from inside blocks and two across a
          border, with and without across=True.  The lines with it are compared with bytes.find over the whole text, those without it with the
          occurrences inside a block.

Each part is a child process under its own time limit; the run ends at the first that fails.

    python tools/fm_seams_throughput.py [--reps 3] [--only pack64k,pack1k,archive] [--archive-mib 16] [--out FILE]
"""
import argparse
import io
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lcp_throughput import child, make_block, median_ms  # noqa: E402
from sa_query_throughput import profiled  # noqa: E402

NPAT, PAT_BYTES = 1024, 8
STEP = 32
PER_CALL = {64 << 10: 1024, 1 << 10: 256}  # patterns per call: npat x count <= DK_FM_FIND_MAX_PAIRS


def cut_patterns(data, block, rng):
    """NPAT different patterns of PAT_BYTES: the even ones from inside a block, the odd ones across a border"""
    import numpy as np
    seen, out = set(), []
    while len(out) < NPAT:
        a = int(rng.integers(0, len(data) - PAT_BYTES))
        if len(out) % 2:
            a = int(rng.integers(1, len(data) // block)) * block - int(rng.integers(1, PAT_BYTES))
        else:
            a -= max((a % block) + PAT_BYTES - block, 0)
        p = data[a:a + PAT_BYTES].tobytes()
        if p not in seen:
            seen.add(p)
            out.append(np.frombuffer(p, np.uint8))
    return out


def host_seams(data, block, pats):
    """every seam record of the pack by enumeration: (pattern, block, back) sorted as the device lists them"""
    import numpy as np
    keys = np.array([int.from_bytes(p.tobytes(), "little") for p in pats], dtype=np.uint64)
    order = np.argsort(keys)
    firsts = np.arange(block, len(data), block, dtype=np.int64)  # where the blocks 1 .. count - 1 start
    found = []
    for back in range(1, PAT_BYTES):
        at = firsts - back
        ok = at + PAT_BYTES <= len(data)  # (the last block may be short)
        win = np.stack([data[at[ok] + j] for j in range(PAT_BYTES)], axis=1).astype(np.uint64)
        key = (win << (8 * np.arange(PAT_BYTES, dtype=np.uint64))[None, :]).sum(axis=1, dtype=np.uint64)
        where = np.searchsorted(keys[order], key)
        hit = (where < len(keys)) & (keys[order][np.minimum(where, len(keys) - 1)] == key)
        # (the match must end inside block b: PAT_BYTES - back <= n_b holds for every block but perhaps the last)
        b = np.flatnonzero(ok)[hit] + 1
        fits = PAT_BYTES - back <= np.minimum(block, len(data) - b * block)
        found += [(int(q), int(bb), back) for q, bb in zip(order[where[hit]][fits], b[fits])]
    return sorted(found, key=lambda r: (r[0], r[1], -r[2]))


def run_pack(block, reps):
    import numpy as np
    import torch
    import dark_amd
    from dark_amd.context import FM_HIT_DTYPE, FM_SEAM_HIT_DTYPE, fm_extract_bytes, fm_index_bytes, fm_locate_bytes
    data = make_block("pack_64KiB")
    n = len(data)
    sizes = [min(block, n - k) for k in range(0, n, block)]
    count = len(sizes)
    pats = cut_patterns(data, block, np.random.default_rng(1))
    per = PER_CALL[block]
    calls = [(a, torch.from_numpy(np.concatenate(pats[a:a + per])).cuda()) for a in range(0, NPAT, per)]
    lens = [PAT_BYTES] * per
    d_in = torch.from_numpy(data).cuda()
    d_bwt = torch.empty(n, dtype=torch.uint8, device="cuda")
    with dark_amd.Context(n) as ctx:
        origins = ctx.dev_bwt_forward_packed(d_in, sizes, d_bwt)
        d_index = torch.empty(fm_index_bytes(n, count) // 4, dtype=torch.int32, device="cuda")
        d_loc = torch.empty(fm_locate_bytes(n, count, STEP) // 4, dtype=torch.int32, device="cuda")
        d_ext = torch.empty(fm_extract_bytes(n, count, STEP) // 4, dtype=torch.int32, device="cuda")
        ctx.dev_fm_build_packed(d_bwt, sizes, origins, d_index)
        ctx.dev_fm_locate_build_packed(d_bwt, sizes, origins, STEP, d_loc)
        ctx.dev_fm_extract_build_packed(d_bwt, sizes, origins, STEP, d_ext)
        d_occ = torch.empty(per * count, dtype=torch.int32, device="cuda")
        # the totals first (they size the records), then the lists
        seam_totals = [ctx.dev_fm_seams_packed(d_bwt, sizes, d_index, d_ext, STEP, None, d_pat, lens, 0, None, d_occ) for _, d_pat in calls]
        find_totals = [ctx.dev_fm_find_packed(d_bwt, sizes, d_index, None, STEP, d_pat, lens, 0, None, d_occ) for _, d_pat in calls]
        d_hits = torch.empty(4 * max(seam_totals + find_totals + [1]), dtype=torch.int32, device="cuda")
        inside = {}

        def seams():
            out, inside["seams"] = [], 0.0
            for (a, d_pat), total in zip(calls, seam_totals):
                got = ctx.dev_fm_seams_packed(d_bwt, sizes, d_index, d_ext, STEP, None, d_pat, lens, total, d_hits, d_occ)
                inside["seams"] += ctx.stats()["ms_total"]
                assert got == total
                recs = d_hits[:4 * total].cpu().numpy().view(FM_SEAM_HIT_DTYPE).copy()
                recs["pattern"] += a
                out.append(recs)
            return np.concatenate(out)

        def find():
            inside["find"] = 0.0
            for (a, d_pat), total in zip(calls, find_totals):
                ctx.dev_fm_find_packed(d_bwt, sizes, d_index, d_loc, STEP, d_pat, lens, total, d_hits, d_occ)
                inside["find"] += ctx.stats()["ms_total"]
                d_hits[:4 * total].cpu().numpy().view(FM_HIT_DTYPE)
        recs = seams()
        want = host_seams(data, block, pats)
        got = list(zip(recs["pattern"].tolist(), recs["block"].tolist(), recs["back"].tolist()))
        if got != want or recs["reserved"].any():
            raise SystemExit("FAILED: %d seam records, the enumeration on the host gives %d" % (len(got), len(want)))
        if len(want) < NPAT // 2:
            raise SystemExit("FAILED: the patterns cut across a border are not all found")
        seams_ms, seams_runs = median_ms(seams, reps)
        seams_lib = inside["seams"]
        find_ms, find_runs = median_ms(find, reps)
        slots = profiled(ctx, lambda: ctx.dev_fm_seams_packed(d_bwt, sizes, d_index, d_ext, STEP, None, calls[0][1], lens, seam_totals[0], d_hits, d_occ))
        print("ROW " + json.dumps(dict(name="pack_64KiB as blocks of %d" % block, kind="device", bytes=n, blocks=count, patterns=NPAT, pattern_bytes=PAT_BYTES,
                                       pairs=NPAT * count, calls=len(calls), candidates=NPAT * (count - 1) * (PAT_BYTES - 1), step=STEP,
                                       seam_hits=len(want), find_hits=sum(find_totals), answers_equal=True,
                                       strip_bytes=min(n, 2 * (PAT_BYTES - 1) * count), seams_ms=round(seams_ms, 3), seams_runs_ms=seams_runs,
                                       seams_library_ms=round(seams_lib, 3), find_ms=round(find_ms, 3), find_runs_ms=find_runs,
                                       find_library_ms=round(inside["find"], 3), seams_over_find=round(seams_ms / find_ms, 3),
                                       slots_first_call=slots)), flush=True)


def run_archive(reps, mib):
    import numpy as np
    from dark_amd import cli
    block = 64 << 10
    data = make_block("pack_64KiB")[:mib << 20]
    text = data.tobytes()
    rng = np.random.default_rng(2)
    patterns = [text[a:a + PAT_BYTES] for a in rng.integers(0, len(text) - PAT_BYTES, size=4).tolist()]
    patterns += [text[b * block - 3:b * block + 5] for b in (1, len(text) // block // 2)]
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as work:
        os.chdir(work)
        try:
            with open("corpus.txt", "wb") as f:
                f.write(text)
            cli.encode_file("corpus.txt", "exp", block, packed=True)

            def search(across):
                out = io.StringIO()
                cli.grep_file("corpus.dark", "exp", patterns, out=out, across=across)
                return [tuple(int(x) for x in ln.split(":")[:2]) for ln in out.getvalue().splitlines()]
            hits = []
            for q, p in enumerate(patterns):
                i = text.find(p)
                while i >= 0:
                    hits.append((i, q))
                    i = text.find(p, i + 1)
            hits.sort()
            inside = [(i, q) for i, q in hits if i // block == (i + PAT_BYTES - 1) // block]
            if search(True) != hits or search(False) != inside or len(hits) - len(inside) < 2:
                raise SystemExit("FAILED: the search lists other hits than bytes.find over the text (%d in all, %d inside a block)" % (len(hits), len(inside)))
            plain_ms, plain_runs = median_ms(lambda: search(False), reps)
            across_ms, across_runs = median_ms(lambda: search(True), reps)
            st, st_across = {}, {}
            cli.grep_file("corpus.dark", "exp", patterns, stats=st, out=io.StringIO())
            cli.grep_file("corpus.dark", "exp", patterns, stats=st_across, out=io.StringIO(), across=True)
            print("ROW " + json.dumps(dict(name="pack_64KiB[:%d MiB]" % mib, kind="archive", bytes=len(text), blocks=-(-len(text) // block),
                                           archive_bytes=os.path.getsize("corpus.dark"), patterns=len(patterns), hits=len(hits),
                                           hits_across_borders=len(hits) - len(inside), answers_equal=True, search_ms=round(plain_ms, 1),
                                           search_runs_ms=plain_runs, search_across_ms=round(across_ms, 1), search_across_runs_ms=across_runs,
                                           across_over_plain=round(across_ms / plain_ms, 3), resident_bytes=st.get("resident_bytes", 0),
                                           resident_bytes_across=st_across.get("resident_bytes", 0))), flush=True)
        finally:
            os.chdir(here)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated parts: pack64k, pack1k, archive (default: all)")
    ap.add_argument("--archive-mib", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_fm_seams.json"))
    ap.add_argument("--step", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        part, _, mib = args.step.partition("@")
        if part == "archive":
            return run_archive(args.reps, int(mib))
        return run_pack(64 << 10 if part == "pack64k" else 1 << 10, args.reps)
    rows = []
    for part in ("pack64k", "pack1k", "archive"):
        if args.only and part not in args.only.split(","):
            continue
        rows += child("%s@%d" % (part, args.archive_mib), args.reps, script=os.path.abspath(__file__))
        with open(args.out, "w") as f:  # (after every part: a run that is cut short keeps what it has)
            json.dump(dict(tool="tools/fm_seams_throughput.py", reps=args.reps, rows=rows), f, indent=1)
    print(args.out)


if __name__ == "__main__":
    main()
