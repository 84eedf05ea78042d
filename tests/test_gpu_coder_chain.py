"""The host pipeline behind dev_block_encode with the coder that takes its quotient from the previous one: a wiki-like
block just large enough for the automatic choice to take the pipeline (5 MB: 2.7 M distances, the pipeline starts at 2^21), with
DK_ENTROPY_THREADS unset and with 4, each in a fresh process (the variable is read when the library is loaded).  The stream must be the
oracle's, and the pass must have run in a form of at least four threads where the host has an L3 group with the cores."""
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
with dark_amd.Context(n) as c:
    s = c.dev_block_encode("dark", d_in, n)
    threads, group = entropy.last_info()
    np.asarray(s).tofile(sys.argv[2])
print(json.dumps({"threads": threads, "group": group, "groups4": entropy.l3_groups(4), "groups5": entropy.l3_groups(5)}))
"""


@pytest.fixture(scope="module")
def oracle_stream(orc):
    from dark_amd import datagen
    return orc.block_dc_encode("dark", np.ascontiguousarray(datagen.wiki_like(N, 2)))


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [None, "4"])
def test_pipeline_stream_equals_oracle(threads, oracle_stream, tmp_path):
    env = {k: v for k, v in os.environ.items() if k != "DK_ENTROPY_THREADS"}
    if threads is not None:
        env["DK_ENTROPY_THREADS"] = threads
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    path = str(tmp_path / "stream.bin")
    out = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", CHILD, str(N), path], env=env, cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    info = json.loads(out.stdout.strip().splitlines()[-1])
    print(info)
    with open(path, "rb") as f:
        stream = f.read()
    assert stream == oracle_stream, "stream of %d bytes, the oracle's has %d (%r)" % (len(stream), len(oracle_stream), info)
    if info["groups4"] < 1:
        pytest.skip("no L3 group with four usable cores on this host: the pass ran with %d thread(s)" % info["threads"])
    assert info["threads"] >= 4, info
