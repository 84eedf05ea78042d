"""The FM-index's near on a poisoned workspace behind a poisoned mailbox: the process tests/test_gpu_fm_near.py starts once.

    python tests/fm_near_poison_worker.py fm_near BYTE      with DARK_AMD_LIB = dark_amd/libdark_amd_tuning.so and DK_POISON = BYTE in the environment

The contexts come from tests/poison_worker.py's open_ctx (the tuning build, the poison live, dk_dbg_mail_fill(BYTE) in front of every call), the
calls from the helpers of tests/test_gpu_fm_near.py, and the answers are compared with tests/fm_near_model.py: a pack whose pairs fill more than
one row of the scan with budgets 0 and 2, a truncated list, a node limit that cuts some pairs, and the single-block entry, on a full context
and on a decoder context."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison_worker as W  # noqa: E402  (reads the group's name and the byte from the command line)

import numpy as np  # noqa: E402

from fm_near_model import exact_classes, near_model  # noqa: E402
from test_gpu_fm import words  # noqa: E402
from test_gpu_fm_near import gpu_near, make_pack, same_records  # noqa: E402


def run(ctx):
    texts = words(b"ab", range(1, 7)) + [b"abracadabra" * 40, b"a" * 1025]
    classes = [exact_classes(p) for p in words(b"abc", range(0, 3)) + [b"abra", b"a" * 128]]
    assert len(texts) * len(classes) > 256  # more than one row of the scan
    for step in (1, 32):
        d_bwt, idx, loc, sizes, _, _ = make_pack(ctx, texts, step)
        for k, limit in ((0, None), (2, None), (2, 5)):
            W.say("%s context, the pack, step %d, k = %d, limit %s" % (ctx.purpose, step, k, limit))
            want_occ, want, want_total, want_cut, _ = near_model(texts, classes, k, limit)
            assert (limit is None) == (want_cut == 0)
            for max_hits in (want_total + 1, 9, 0):
                occ, recs, total, cut = gpu_near(ctx, d_bwt, sizes, idx, loc if max_hits else None, step, classes, k, max_hits, limit or 0)
                assert total == want_total and cut == want_cut and np.array_equal(occ, want_occ.astype(np.int64)), (step, k, limit, max_hits)
                same_records(recs, want[:max_hits], "step %d k %d max_hits %d:" % (step, k, max_hits))
    W.say("%s context, one block" % ctx.purpose)
    t = texts[-2]
    one_occ, one, one_total, _, _ = near_model([t], classes, 1)
    d_bwt, idx, loc, sizes, _, _ = make_pack(ctx, [t], 8)
    occ, recs, total, cut = gpu_near(ctx, d_bwt, sizes, idx, loc, 8, classes, 1, one_total)
    assert total == one_total and cut == 0 and np.array_equal(occ, one_occ.astype(np.int64))
    same_records(recs, one)


if __name__ == "__main__":
    t0 = time.perf_counter()
    total = sum(m * 2 ** m for m in range(1, 7)) + 440 + 1025  # the pack of run()
    full = W.open_ctx(total)
    run(full)
    W.done_with(full)
    dec = W.open_ctx(total, "decoder", 128)
    run(dec)
    W.done_with(dec)
    W.REPORT["seconds"] = round(time.perf_counter() - t0, 2)
    assert W.REPORT["contexts"] == 2 and W.REPORT["peeks"] >= 12 * W.REPORT["contexts"] and W.REPORT["fills"] > 0, W.REPORT
    W.REPORT["routes"] = sorted(W.REPORT["routes"])
    print("RESULT " + json.dumps(W.REPORT))
