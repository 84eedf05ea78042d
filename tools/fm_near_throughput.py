"""FM-index near on the GPU: the branching backward search beside find on the same patterns, with budgets of 1, 2 and
3 mismatches, with ignore-case classes, and one pattern of eight wildcards at the default node limit.  The numbers are RECORDED, NOT GATED.

pack      pack_64KiB (64 MiB of wiki_like text as 1024 blocks of 64 KiB): every pattern in every block.
single    the first 2^24 bytes of the same text as one block.
Both with 1024 patterns of 8 and of 24 bytes cut from the text (--patterns; --k3-patterns: fewer for k = 3, whose trees hold tens of thousands
of nodes per pair -- every row says how many patterns it ran).  Rows:
  k = 0 with one-bit classes beside dk_dev_fm_find(_packed) on the same patterns; the answers must agree, the ratio is written down
  k = 1, 2, 3
  ignore_case (k = 0, fm.classes(..., ignore_case=True))
  one pattern of eight wildcards at the default node limit: its time and `cut`
EVERY answer is checked before it is timed: k = 0 against find (the occurrence matrix and the set of (pattern, block, position)); every other
row record by record -- the cost of the text at the record's position against the classes is the record's cost and at most k -- and, for the
first --brute patterns, the occurrence counts against a brute-force count of the positions with cost <= k over the whole text (torch, on the
device).  Rows whose searches were cut at the node limit are checked record by record only; their counts are lower bounds.
Times are wall time around the calls (they synchronise) and, for the library's share, dk_stats.ms_total.

Each part is a child process under its own time limit; the run ends at the first that fails.

    python tools/fm_near_throughput.py [--reps 3] [--only pack,single] [--patterns 1024] [--k3-patterns 1024] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lcp_throughput import child, make_block, median_ms  # noqa: E402
from sa_query_throughput import library_ms  # noqa: E402

PACK_BLOCK = 64 << 10
SINGLE_BYTES = 1 << 24
STEP = 32
MAX_RECORDS = 1 << 24  # records listed per call (256 MiB); the counts are complete however many are listed


def run(part, reps, npat, npat_k3, nbrute):
    import numpy as np
    import torch
    import dark_amd
    from dark_amd import fm
    from dark_amd.context import FM_HIT_DTYPE, FM_NEAR_HIT_DTYPE, fm_index_bytes, fm_locate_bytes
    data = make_block("pack_64KiB")
    if part == "single":
        data = data[:SINGLE_BYTES]
    n = len(data)
    sizes = [min(PACK_BLOCK, n - a) for a in range(0, n, PACK_BLOCK)] if part == "pack" else [n]
    count, block = len(sizes), sizes[0]
    d_in = torch.from_numpy(data).cuda()
    d_bwt = torch.empty(n, dtype=torch.uint8, device="cuda")
    starts_of_blocks = torch.arange(count, device="cuda", dtype=torch.int64) * block
    with dark_amd.Context(n) as ctx:
        if count > 1:
            origins = ctx.dev_bwt_forward_packed(d_in, sizes, d_bwt)
        else:
            origins = [ctx.dev_bwt_forward(d_in, n, d_bwt)]
        d_index = torch.empty(fm_index_bytes(n, count) // 4, dtype=torch.int32, device="cuda")
        d_loc = torch.empty(fm_locate_bytes(n, count, STEP) // 4, dtype=torch.int32, device="cuda")
        if count > 1:
            ctx.dev_fm_build_packed(d_bwt, sizes, origins, d_index)
            ctx.dev_fm_locate_build_packed(d_bwt, sizes, origins, STEP, d_loc)
        else:
            ctx.dev_fm_build(d_bwt, n, origins[0], d_index)
            ctx.dev_fm_locate_build(d_bwt, n, origins[0], STEP, d_loc)

        def near(d_cls, lens, k, max_hits, d_hits, d_occ):
            if count > 1:
                return ctx.dev_fm_near_packed(d_bwt, sizes, d_index, d_loc, STEP, d_cls, lens, k, 0, max_hits, d_hits, d_occ)
            return ctx.dev_fm_near(d_bwt, n, d_index, d_loc, STEP, d_cls, lens, k, 0, max_hits, d_hits, d_occ)

        def find(d_pat, lens, max_hits, d_hits, d_occ):
            if count > 1:
                return ctx.dev_fm_find_packed(d_bwt, sizes, d_index, d_loc, STEP, d_pat, lens, max_hits, d_hits, d_occ)
            return ctx.dev_fm_find(d_bwt, n, d_index, d_loc, STEP, d_pat, lens, max_hits, d_hits, d_occ)

        def keys(r):
            return np.sort((r["pattern"].astype(np.int64) << 44) | (r["block"].astype(np.int64) << 32) | r["position"].astype(np.int64))

        def sound(recs, cls, m, k):
            """every record: the cost of the text at its position against the classes is its cost, and at most k"""
            at = torch.from_numpy(recs["block"].astype(np.int64) * block + recs["position"].astype(np.int64)).cuda()
            q = torch.from_numpy(recs["pattern"].astype(np.int64)).cuda()
            d_c = torch.from_numpy(cls.astype(np.int64)).cuda()  # npat x m x 32
            cost = torch.zeros(len(recs), dtype=torch.int64, device="cuda")
            for i in range(m):
                c = d_in[at + i].to(torch.int64)
                cost += 1 - ((d_c[q, i, c >> 3] >> (c & 7)) & 1)
            inside = torch.from_numpy(recs["position"].astype(np.int64) + m <= block).cuda()
            return bool(inside.all()) and bool((cost <= k).all()) and bool((cost.cpu() == torch.from_numpy(recs["cost"].astype(np.int64))).all())

        def brute_occ(cls_q, m, k):
            """the positions of every block whose text costs at most k against one pattern's classes, counted per block"""
            member = torch.from_numpy(np.unpackbits(cls_q, axis=1, bitorder="little").astype(np.int64)).cuda()  # m x 256
            cost = torch.zeros(n - m + 1, dtype=torch.int16, device="cuda")
            for i in range(m):
                cost += (1 - member[i][d_in[i:n - m + 1 + i].to(torch.int64)]).to(torch.int16)
            p = torch.nonzero(cost <= k).view(-1)
            p = p[(p % block) + m <= block]
            return torch.bincount(p // block, minlength=count).cpu().numpy()

        for m in (8, 24):
            rng = np.random.default_rng(m)
            starts = rng.integers(0, n - m, size=npat)
            starts -= np.maximum((starts % block) + m - block, 0)  # (inside one block each)
            pats = [data[a:a + m].tobytes() for a in starts]
            exact = np.stack([fm.classes(p) for p in pats])
            folded = np.stack([fm.classes(p, ignore_case=True) for p in pats])
            d_pat = torch.from_numpy(np.concatenate([np.frombuffer(p, np.uint8) for p in pats])).cuda()
            rows = [("k0", exact, 0, npat), ("k1", exact, 1, npat), ("k2", exact, 2, npat), ("k3", exact, 3, min(npat, npat_k3)), ("ignore_case", folded, 0, npat)]
            for name, cls, k, use in rows:
                cls, lens = cls[:use], [m] * use
                d_cls = torch.from_numpy(cls.reshape(-1)).cuda()
                d_occ = torch.empty(use * count, dtype=torch.int32, device="cuda")
                total, cut = near(d_cls, lens, k, 0, None, d_occ)
                listed = min(total, MAX_RECORDS)
                d_hits = torch.empty(4 * max(listed, 1), dtype=torch.int32, device="cuda")

                def call():
                    return near(d_cls, lens, k, listed, d_hits, d_occ)
                got = call()
                recs = d_hits[:4 * listed].cpu().numpy().view(FM_NEAR_HIT_DTYPE)
                occ = d_occ.cpu().numpy().view(np.uint32).reshape(use, count)
                if got != (total, cut) or int(occ.astype(np.int64).sum()) != total or not sound(recs, cls, m, k):
                    raise SystemExit("FAILED: %s %s m = %d: the records do not stand where they say" % (part, name, m))
                extra = {}
                if name == "k0":
                    f_occ = torch.empty(use * count, dtype=torch.int32, device="cuda")
                    f_hits = torch.empty(4 * max(listed, 1), dtype=torch.int32, device="cuda")

                    def find_call():
                        return find(d_pat[:use * m], lens, listed, f_hits, f_occ)
                    f_total = find_call()
                    f_recs = f_hits[:4 * listed].cpu().numpy().view(FM_HIT_DTYPE)
                    if f_total != total or cut or not torch.equal(f_occ, d_occ) or (listed == total and not np.array_equal(keys(recs), keys(f_recs))):
                        raise SystemExit("FAILED: %s m = %d: near at k = 0 and find differ (%d and %d hits)" % (part, m, total, f_total))
                    find_ms, find_runs = median_ms(find_call, reps)
                    extra = dict(answers_equal_find=True, find_ms=round(find_ms, 3), find_runs_ms=find_runs)
                if cut == 0:
                    for q in range(min(nbrute, use)):
                        if not np.array_equal(brute_occ(cls[q], m, k), occ[q]):
                            raise SystemExit("FAILED: %s %s m = %d: pattern %d's counts differ from the brute-force count" % (part, name, m, q))
                ms, runs = median_ms(call, reps)
                lib_ms, _ = library_ms(ctx, call, reps)
                if extra:
                    extra["near_over_find"] = round(ms / extra["find_ms"], 3)
                print("ROW " + json.dumps(dict(name=part, row=name, bytes=n, blocks=count, patterns=use, pattern_bytes=m, pairs=use * count, k=k, hits=total,
                                               listed=listed, cut_pairs=cut, checked="records, find" if extra else "records, brute-force counts of %d patterns" %
                                               min(nbrute, use) if cut == 0 else "records", near_ms=round(ms, 3), near_runs_ms=runs,
                                               near_library_ms=round(lib_ms, 3), **extra)), flush=True)
                del d_hits
        # eight wildcards: every string of eight bytes in a block is a leaf; the walk ends at the default node limit
        wild = fm.classes(b"????????", wildcard=ord("?"))
        d_cls = torch.from_numpy(wild.reshape(-1)).cuda()
        d_occ = torch.empty(count, dtype=torch.int32, device="cuda")
        total, cut = near(d_cls, [8], 0, 0, None, d_occ)
        occ = d_occ.cpu().numpy().view(np.uint32).astype(np.int64)
        if not ((occ <= block - 7).all() and (cut > 0 or (occ == np.array(sizes) - 7).all())):
            raise SystemExit("FAILED: %s, eight wildcards: %d hits, %d pairs cut" % (part, total, cut))
        ms, runs = median_ms(lambda: near(d_cls, [8], 0, 0, None, d_occ), reps)
        print("ROW " + json.dumps(dict(name=part, row="eight_wildcards", bytes=n, blocks=count, patterns=1, pattern_bytes=8, pairs=count, k=0, hits=total,
                                       positions=int(sum(sizes)) - 7 * count, cut_pairs=cut, node_limit=dark_amd.context.FM_NEAR_NODE_LIMIT,
                                       near_ms=round(ms, 3), near_runs_ms=runs)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated parts: pack, single (default: both)")
    ap.add_argument("--patterns", type=int, default=1024)
    ap.add_argument("--k3-patterns", type=int, default=1024, help="patterns of the k = 3 rows (their trees are the largest)")
    ap.add_argument("--brute", type=int, default=4, help="patterns per row whose counts are checked against a brute-force count")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_fm_near.json"))
    ap.add_argument("--step", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        part, npat, npat_k3, nbrute = args.step.split("@")
        return run(part, args.reps, int(npat), int(npat_k3), int(nbrute))
    rows = []
    for part in ("pack", "single"):
        if args.only and part not in args.only.split(","):
            continue
        rows += child("%s@%d@%d@%d" % (part, args.patterns, args.k3_patterns, args.brute), args.reps, script=os.path.abspath(__file__))
        with open(args.out, "w") as f:  # (after every part: a run that is cut short keeps what it has)
            json.dump(dict(tool="tools/fm_near_throughput.py", reps=args.reps, patterns=args.patterns, k3_patterns=args.k3_patterns, rows=rows), f, indent=1)
    print(args.out)


if __name__ == "__main__":
    main()
