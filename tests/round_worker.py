"""One setting of the tuning build's knobs for cases of tests/test_gpu_round.py and one of tests/test_gpu_period.py, in a process of its own (the
knobs are read once per process; the parent sets them and DARK_AMD_LIB in the environment).  argv: the repository root and a JSON spec --
  cases      names of tests/round_cases.py, built here from their seeds     poison     the byte of DK_POISON, proved to be in force first
  mail_fill  a byte for dk_dbg_mail_fill before every call, or null
Every round case runs in both modes against the model, then tests/period_cases.py's POISON case: the same bytes as the plain run.  Prints
"RESULT " and {name: calls made}."""
import json
import os
import sys

root, spec = sys.argv[1], json.loads(sys.argv[2])
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import dark_amd  # noqa: E402
import period_cases as PK  # noqa: E402
import round_cases as K  # noqa: E402

out = {}
with dark_amd.Context(1 << 17) as ctx:
    if spec.get("poison") is not None:  # the proof that the run is poisoned
        assert (ctx.dbg_ws_peek(4096) == spec["poison"]).all(), "DK_POISON is not in force"

    def stale():
        if spec.get("mail_fill") is not None:
            ctx.dbg_mail_fill(spec["mail_fill"])

    for name in spec["cases"]:
        c = K.CASES[name]()
        out[name] = 0
        for mode in K.MODES:
            stale()
            K.check(c, mode, K.call(ctx, c, mode), K.expected(name, mode)[1])
            out[name] += 1
    stale()
    c = PK.CASES[PK.POISON]()
    PK.check(c, PK.call(ctx, c), PK.expected(c))
    out["period"] = 1
print("RESULT " + json.dumps(out))
