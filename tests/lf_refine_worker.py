"""One setting of the tuning build's knobs for the refinement cases of tests/test_gpu_lfirst_layer.py, in a process of its own (the knobs are read
once per process; the parent sets them and DARK_AMD_LIB in the environment).  argv: the repository root and a JSON spec --
  cases      names of tests/lf_refine_cases.py, built here from their seeds        labels    256 or 2 symbols in front
  mail_fill  a byte for dk_dbg_mail_fill before every call, or null                by_wave   is k_lf_deep_wave on (DK_LF_WAVE)
  gave_up    names whose verdict must be START_OVER with L untouched outside the listed places (the rest: L and the origin against the model)
  counters   {name: [deep_count, arena_used]} in place of the case's own
Prints "RESULT " and {name: the route and the counters}."""
import json
import os
import sys

root, spec = sys.argv[1], json.loads(sys.argv[2])
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np  # noqa: E402

import dark_amd  # noqa: E402
import lf_refine_cases as K  # noqa: E402
import lf_refine_model as M  # noqa: E402

out = {}
with dark_amd.Context(1 << 19) as ctx:
    if spec.get("poison") is not None:  # the proof that the run is poisoned
        assert (ctx.dbg_ws_peek(4096) == spec["poison"]).all(), "DK_POISON is not in force"
    for name in spec["cases"]:
        c = K.CASES[name](labels=spec.get("labels", 256))
        if spec.get("mail_fill") is not None:
            ctx.dbg_mail_fill(spec["mail_fill"])
        got = ctx.dbg_dev_lf_refine(c.text, c.idx, c.pos, c.gid, c.sym, c.h0, c.period, fill=K.FILL8, origin=K.FILL32)
        if name in spec.get("gave_up", ()):
            out[name] = K.check_gave_up(c, got)
        else:
            L, origin = M.lf_refine_model(c.text, c.idx, c.pos, c.gid, c.sym, np.full(len(c.text), K.FILL8, np.uint8), K.FILL32)
            out[name] = K.check_result(c, got, L, origin, by_wave=spec.get("by_wave", True), counters=spec.get("counters", {}).get(name))
print("RESULT " + json.dumps(out))
