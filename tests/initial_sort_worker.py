"""One setting of the tuning build's knobs for cases of tests/test_gpu_initial_sort.py, in a process of its own (the knobs are read once per
process; the parent sets them and DARK_AMD_LIB in the environment).  argv: the repository root and a JSON spec --
  cases        names of tests/initial_sort_cases.py, built here from their seeds     large   names of its LARGE cases, each on a context of its size
  packed_sort  false under DK_PACKED_SORT=0: the model then predicts plain pairs      wide    true: every case with 64-bit keys, whatever it is named
  poison       the byte of DK_POISON, proved to be in force first                     mail_fill  a byte for dk_dbg_mail_fill before every call, or null
Every case against the model: the same arrays under every setting, and the route the model predicts for it.  Prints "RESULT " and
{name: {"packed": the route bit, "passes": ...}}."""
import json
import os
import sys

root, spec = sys.argv[1], json.loads(sys.argv[2])
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import dark_amd  # noqa: E402
import initial_sort_cases as K  # noqa: E402
import initial_sort_model as M  # noqa: E402

packed_sort = spec.get("packed_sort", True)
out = {}


def run(ctx, c):
    if spec.get("mail_fill") is not None:
        ctx.dbg_mail_fill(spec["mail_fill"])
    narrow = False if spec.get("wide") else c.narrow
    m = K.expected(c, packed_sort=packed_sort, narrow=narrow, keep=False)
    got = K.call(ctx, c, narrow=narrow)
    K.check(c, got, m, want_packed=c.want_packed and packed_sort)
    out[c.name] = dict(packed=bool(got["route"] & M.ROUTE_PACKED_PAIRS), passes=got["passes"])


with dark_amd.Context(1 << 17) as ctx:
    if spec.get("poison") is not None:  # the proof that the run is poisoned
        assert (ctx.dbg_ws_peek(4096) == spec["poison"]).all(), "DK_POISON is not in force"
    for name in spec["cases"]:
        run(ctx, K.CASES[name]())
for name in spec.get("large", []):
    c = K.large(name)
    with dark_amd.Context(c.n) as ctx:
        run(ctx, c)
print("RESULT " + json.dumps(out))
