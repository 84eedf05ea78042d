"""The six-stage host pipeline behind dev_block_encode (a prepare stage between the merger and the coder): a wiki-like block
of 5 MB -- 2.7 M distances, just above the 2^21 from which the pipeline codes a block -- in a fresh process with thread mode 5 (what bench.py plans on such a host).
The stream must be the oracle's, and the pass must have run on six threads where the host has an L3 group with six usable cores, on five
where it has not."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

N = 5_000_000
CHILD = r"""
import json, sys
import numpy as np, torch
import dark_amd
from dark_amd import datagen, entropy
n = int(sys.argv[1])
t = np.ascontiguousarray(datagen.wiki_like(n, 2))
d_in = torch.from_numpy(t).cuda()
entropy.set_threads(5)
with dark_amd.Context(n) as c:
    s = c.dev_block_encode("dark", d_in, n)
    threads = int(c.stats()["entropy_threads"])
    np.asarray(s).tofile(sys.argv[2])
print(json.dumps({"threads": threads, "last_info": entropy.last_info()[0], "groups6": entropy.l3_groups(6), "groups5": entropy.l3_groups(5)}))
"""


@pytest.mark.gpu
def test_six_stage_stream_equals_oracle(orc, tmp_path):
    from dark_amd import datagen
    want = orc.block_dc_encode("dark", np.ascontiguousarray(datagen.wiki_like(N, 2)))
    env = {k: v for k, v in os.environ.items() if k != "DK_ENTROPY_THREADS"}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    path = str(tmp_path / "stream.bin")
    out = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", CHILD, str(N), path], env=env, cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    info = json.loads(out.stdout.strip().splitlines()[-1])
    print(info)
    with open(path, "rb") as f:
        stream = f.read()
    assert stream == want, "stream of %d bytes, the oracle's has %d (%r)" % (len(stream), len(want), info)
    assert info["last_info"] == info["threads"], info
    if info["groups6"] >= 1:
        assert info["threads"] == 6, info
    elif info["groups5"] >= 1:
        assert info["threads"] == 5, info
    else:
        assert info["threads"] < 5, info
