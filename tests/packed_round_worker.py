"""A short list of the cases of tests/test_gpu_packed_round.py in a process of its own on the tuning library (the parent sets the knobs and
DARK_AMD_LIB in the environment).  argv: the repository root and a JSON spec --
  first, rounds   names of tests/packed_round_cases.py, built here from their seeds
  poison          the byte of DK_POISON, proved to be in force first       mail_fill  a byte for dk_dbg_mail_fill before every call
Every case against the model, whole arrays.  Prints "RESULT " and {name: live}."""
import json
import os
import sys

root, spec = sys.argv[1], json.loads(sys.argv[2])
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import dark_amd  # noqa: E402
import packed_round_cases as K  # noqa: E402
import packed_round_model as M  # noqa: E402

out = {}
with dark_amd.Context(1 << 17) as ctx:
    assert (ctx.dbg_ws_peek(4096) == spec["poison"]).all(), "DK_POISON is not in force"  # the proof that the run is poisoned
    for name in spec["first"]:
        blocks = K.first_blocks(name)
        ctx.dbg_mail_fill(spec["mail_fill"])
        got = ctx.dbg_dev_packed_first(blocks, fill=0xC3, pad=K.PAD)
        K.check_first(name, got, M.first(blocks))
        out[name] = got["live"]
    for name in spec["rounds"]:
        c = K.ROUNDS[name]()
        ctx.dbg_mail_fill(spec["mail_fill"])
        got = K.call_round(ctx, c)
        K.check_round(name, got, M.round_(c.act, c.rank, c.off, c.h), c.guard)
        out[name] = got["live"]
print("RESULT " + json.dumps(out))
