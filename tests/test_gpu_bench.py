"""A plain `python bench.py` run (no --full): it times exactly --steps steps, prints the headline keys alone, and --dump-outputs writes the
coded stream of its last timed step -- which must be the oracle's stream of the same seeded block."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(600)
def test_plain_run_and_dumped_stream(tmp_path, orc):
    from dark_amd import datagen
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "book1_like_768771",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    res = json.loads(lines[0])
    assert res["metric"] == "bwt_encode_MBps" and res["unit"] == "MB/s" and res["higher_is_better"] is True
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert abs(res["value"] - 768771 * 1e-3 / res["ms_per_step"]) <= 0.01 * res["value"]
    for key in ("kernel_ms_per_step", "host_input", "decode_MBps", "pipelined", "cpu_baseline", "gather_ms", "roofline"):
        assert key not in res, key  # legs of --full
    want = np.frombuffer(orc.block_dc_encode("dark", datagen.english_like(768771, 1)), dtype=np.uint8)
    assert res["compressed_bytes"] == len(want)
    assert np.load(out / "stream_length.npy").tolist() == [float(len(want))]
    got = np.load(out / "stream.npy")
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
