"""Matching statistics and super-maximal matches on a poisoned workspace behind a poisoned mailbox: the process tests/test_gpu_sa_match.py starts
once.

    python tests/sa_match_poison_worker.py sa_match BYTE      with DARK_AMD_LIB = dark_amd/libdark_amd_tuning.so and DK_POISON = BYTE in the environment

The context comes from tests/poison_worker.py's open_ctx (the tuning build, the poison live, dk_dbg_mail_fill(BYTE) in front of every call), the
calls from the helpers of tests/test_gpu_sa_match.py, and the answers are compared with tests/sa_match_model.py: the depths of the search at
their smallest sizes on both sides of the kernels' border, the pack, and the super-maximal matches with a list that is cut and one that is only
counted -- the total comes through the mailbox the fill has just poisoned."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison_worker as W  # noqa: E402  (reads the group's name and the byte from the command line)

import numpy as np  # noqa: E402

import test_gpu_sa_match as M  # noqa: E402
from test_gpu_lcp import Words, dev_text  # noqa: E402
from test_gpu_sa_search import gpu_sa  # noqa: E402


def run(ctx):
    for n in (1, 65):
        W.say("depth case n = %d" % n)
        t, queries = M.depth_case(n)
        sa = gpu_sa(ctx, t)
        for max_len in (3, 1000):
            M.check(ctx, t, queries, max_len, sa=sa)
        M.check_smems(ctx, t, queries, 1000, sa=sa, cuts=True)
    W.say("the pack")
    blocks, queries, where = M.pack_case()
    sizes = [len(b) for b in blocks]
    t = np.concatenate(blocks)
    d_sa = Words(len(t))
    ctx.dev_suffix_array_packed(dev_text(t), sizes, d_sa.t)
    want = M.pack_model(blocks, d_sa.host(), queries, where, 1000)
    got = np.stack(M.gpu_match(ctx, t, d_sa, queries, 1000, pack=(sizes, where)), axis=1)
    assert np.array_equal(got, want)
    rows = M.smem_rows(want, queries, 1, 1000)
    for max_hits in (len(rows) + 1, 9, 0):
        recs, total = M.gpu_smems(ctx, t, d_sa, queries, 1, 1000, max_hits, pack=(sizes, where))
        assert total == len(rows) and np.array_equal(recs, rows[:max_hits]), max_hits


if __name__ == "__main__":
    t0 = time.perf_counter()
    full = W.open_ctx(M.CAP)
    run(full)
    W.done_with(full)
    W.REPORT["seconds"] = round(time.perf_counter() - t0, 2)
    assert W.REPORT["contexts"] == 1 and W.REPORT["peeks"] >= 12 and W.REPORT["fills"] > 0, W.REPORT
    W.REPORT["routes"] = sorted(W.REPORT["routes"])
    print("RESULT " + json.dumps(W.REPORT))
