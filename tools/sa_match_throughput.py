"""Matching statistics and super-maximal matches on the GPU: positions per second of dk_dev_sa_match and SMEMs per second of dk_dev_sa_smems
(DESIGN.md section 4.19), beside the time dk_dev_sa_search takes on the same windows, one pattern of max_len bytes (less at a read's end) per
position: one lower-bound search per position at the cost it had before this stage existed.

Two blocks: text_5e7 (datagen.wiki_like, 5e7 bytes) and acgt_2p26 (datagen.acgt, 2^26 bytes), each with its suffix array from
dk_dev_suffix_array.  Queries are reads cut from the block at random places with 2 % of their bytes replaced by random bytes of the block's
alphabet: 2048 reads of 150 bytes (max_len 150) and 128 reads of 2000 bytes (max_len 1000).  Before anything is timed, len of SAMPLE positions is
compared with a plain bisect over the cut suffixes on the host, and the SMEM list with the three conditions applied to the downloaded lengths.
Times are dk_stats.ms_total, the time inside the entry point (offsets built and uploaded, kernels, synchronise), the median of --reps calls
behind one warm-up call.  Recorded, not gated.

Every workload is a child process under its own time limit; the run ends at the first that fails.

    python tools/sa_match_throughput.py [--reps 3] [--only NAME[,NAME]] [--out FILE]
"""
import argparse
import bisect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lcp_throughput import child  # noqa: E402
from sa_query_throughput import library_ms, profiled  # noqa: E402

WORKLOADS = ("text_5e7", "acgt_2p26")
READS = ((150, 2048, 150), (2000, 128, 1000))  # read length, reads, max_len
SAMPLE = 256
MIN_LEN = 20


class Cut:
    def __init__(self, t, sa, m):
        self.t, self.sa, self.m = t, sa, m

    def __len__(self):
        return len(self.sa)

    def __getitem__(self, i):
        v = int(self.sa[i])
        return self.t[v:v + self.m]


def shared(a, b):
    k, m = 0, min(len(a), len(b))
    while k < m and a[k] == b[k]:
        k += 1
    return k


def plain_len(t, sa, window):
    slot = bisect.bisect_left(Cut(t, sa, len(window)), window)
    left = shared(window, t[int(sa[slot - 1]):int(sa[slot - 1]) + len(window)]) if slot else 0
    right = shared(window, t[int(sa[slot]):int(sa[slot]) + len(window)]) if slot < len(sa) else 0
    return max(left, right)


def run(name, reps):
    import numpy as np
    import torch
    import dark_amd
    from dark_amd import datagen
    data = np.ascontiguousarray(datagen.wiki_like(50_000_000, seed=11) if name == "text_5e7" else datagen.acgt(1 << 26, seed=11), dtype=np.uint8)
    n = len(data)
    text = data.tobytes()
    alphabet = np.unique(data[:1 << 20])
    rng = np.random.default_rng(3)
    d_in = torch.from_numpy(data.copy()).cuda()
    d_sa = torch.empty(n, dtype=torch.int32, device="cuda")
    with dark_amd.Context(n) as ctx:
        ctx.dev_suffix_array(d_in, n, d_sa)
        sa = d_sa.cpu().numpy().view(np.uint32)
        for read_len, nreads, max_len in READS:
            at = rng.integers(0, n - read_len, size=nreads)
            reads = data[at[:, None] + np.arange(read_len)[None, :]].copy()
            noise = rng.random(reads.shape) < 0.02
            reads[noise] = alphabet[rng.integers(0, len(alphabet), size=int(noise.sum()))]
            flat = reads.reshape(-1)
            Q, lens = flat.size, [read_len] * nreads
            d_q = torch.from_numpy(flat).cuda()
            d_len, d_lo, d_hi = (torch.empty(Q, dtype=torch.int32, device="cuda") for _ in range(3))
            match = lambda: ctx.dev_sa_match(d_in, n, d_sa, d_q, lens, max_len, d_len, d_lo, d_hi)  # noqa: E731
            match()
            got = d_len.cpu().numpy().view(np.uint32).astype(np.int64)
            raw = flat.tobytes()
            for g in rng.integers(0, Q, size=SAMPLE).tolist():
                m = min(max_len, read_len - g % read_len)
                want = plain_len(text, sa, raw[g:g + m])
                if got[g] != want:
                    raise SystemExit("FAILED: %s: len[%d] = %d, the plain bisect has %d" % (name, g, got[g], want))
            # the SMEMs from the downloaded lengths, by the three conditions
            l2 = got.reshape(nreads, read_len)
            prev = np.concatenate([np.zeros((nreads, 1), np.int64), l2[:, :-1]], axis=1)
            inner = np.arange(read_len)[None, :] > 0
            flags = (l2 >= MIN_LEN) & (prev <= l2) & ~(inner & (prev == max_len) & (l2 == max_len))
            want_at = np.flatnonzero(flags.reshape(-1))
            d_hits = torch.empty(4 * max(len(want_at), 1), dtype=torch.int32, device="cuda")
            smems = lambda: ctx.dev_sa_smems(d_in, n, d_sa, d_q, lens, MIN_LEN, max_len, len(want_at), d_hits)  # noqa: E731
            total = smems()
            recs = d_hits.cpu().numpy().view(np.uint32).reshape(-1, 4)[:len(want_at)]
            if total != len(want_at) or not np.array_equal(recs[:, 0], want_at) or not np.array_equal(recs[:, 1], got[want_at]):
                raise SystemExit("FAILED: %s: %d SMEMs, the three conditions on the lengths give %d" % (name, total, len(want_at)))
            match_ms, match_runs = library_ms(ctx, match, reps)
            smems_ms, smems_runs = library_ms(ctx, smems, reps)
            match_slots = profiled(ctx, match)
            # the same windows as patterns of dk_dev_sa_search: position g of a read has min(max_len, read_len - g) bytes
            wlen = np.minimum(max_len, read_len - np.arange(read_len))
            woff = np.concatenate([[0], np.cumsum(wlen)])
            idx = torch.from_numpy(np.concatenate([np.arange(g, g + int(wlen[g])) for g in range(read_len)])).cuda()
            d_pat = torch.cat([d_q[r * read_len + idx] for r in range(nreads)]).contiguous()
            plens = np.tile(wlen, nreads).tolist()
            s_lo, s_hi = (torch.empty(Q, dtype=torch.int32, device="cuda") for _ in range(2))
            search = lambda: ctx.dev_sa_search(d_in, n, d_sa, d_pat, plens, s_lo, s_hi)  # noqa: E731
            search()
            full = torch.from_numpy((got == np.tile(wlen, nreads))).cuda()  # a window that occurs whole: the search and the match give one range
            if not (torch.equal(s_lo[full], d_lo[full]) and torch.equal(s_hi[full], d_hi[full])):
                raise SystemExit("FAILED: %s: the ranges of the windows that occur whole differ from dk_dev_sa_search's" % name)
            search_ms, search_runs = library_ms(ctx, search, reps)
            print("ROW " + json.dumps(dict(
                name=name, bytes=n, read_bytes=read_len, reads=nreads, max_len=max_len, positions=Q, sampled=SAMPLE, mean_len=round(float(got.mean()), 2),
                through_the_cut=int((got > 256).sum()), match_ms=round(match_ms, 3), match_runs_ms=match_runs, Mpositions_per_s=round(Q / 1e3 / match_ms, 3),
                min_len=MIN_LEN, smems=int(total), smems_ms=round(smems_ms, 3), smems_runs_ms=smems_runs, Msmems_per_s=round(total / 1e3 / smems_ms, 4),
                search_pattern_bytes=int(woff[-1]) * nreads, sa_search_ms=round(search_ms, 3), sa_search_runs_ms=search_runs, match_slots=match_slots)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated workload names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_sa_match.json"))
    ap.add_argument("--step", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        run(args.step, args.reps)
        return
    names = [x for x in WORKLOADS if not args.only or x in args.only.split(",")]
    rows = []
    for name in names:
        rows += child(name, args.reps, script=os.path.abspath(__file__))
        with open(args.out, "w") as f:  # (after every workload: a run that is cut short keeps what it has)
            json.dump(dict(tool="tools/sa_match_throughput.py", reps=args.reps, rows=rows), f, indent=1)
    print(args.out)


if __name__ == "__main__":
    main()
