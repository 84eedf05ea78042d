"""One setting of the tuning build's knobs for cases of tests/test_gpu_in_place.py, in a process of its own (the knobs are read once per process;
the parent sets them and DARK_AMD_LIB in the environment).  argv: the repository root and a JSON spec --
  cases      names of tests/in_place_cases.py, built here from their seeds     poison     the byte of DK_POISON, proved to be in force first
  mail_fill  a byte for dk_dbg_mail_fill before every call, or null
Every case runs in both modes under all six plans against the model (the soundness cases: chains only and to the end, against their own checks):
the same bytes as the plain run.  Prints "RESULT " and {name: calls made}."""
import json
import os
import sys

root, spec = sys.argv[1], json.loads(sys.argv[2])
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import dark_amd  # noqa: E402
import in_place_cases as K  # noqa: E402

out = {}
with dark_amd.Context(1 << 16) as ctx:
    if spec.get("poison") is not None:  # the proof that the run is poisoned
        assert (ctx.dbg_ws_peek(4096) == spec["poison"]).all(), "DK_POISON is not in force"
    for name in spec["cases"]:
        c = K.CASES[name]()
        out[name] = 0
        for mode in ("sa", "l"):
            for plan_id, plan in zip(K.PLAN_IDS, K.PLANS):
                if name in K.SOUND and plan_id not in ("chains_only", "to_the_end"):
                    continue
                if spec.get("mail_fill") is not None:
                    ctx.dbg_mail_fill(spec["mail_fill"])
                got = K.call(ctx, c, mode, **plan)
                if name not in K.SOUND:
                    K.check_exact(c, mode, got, K.expected(name, mode, plan_id))
                elif plan_id == "chains_only":
                    K.check_sound_chains(c, mode, got)
                if plan_id in ("to_the_end", "always_compact"):
                    K.check_complete(c, mode, got)
                out[name] += 1
print("RESULT " + json.dumps(out))
