"""The suffix sort's give-ups, driven past each limit.  The L-first path (csrc/lfirst.inc) and the packed path (csrc/abi.cpp) give up when an
input goes past one of their fixed limits and take a slower path that must give the same answer.  The tuning build
(dark_amd/libdark_amd_tuning.so) lowers each limit through a knob, so that blocks of a few MB reach it:
  DK_LF_DEEP_CAP      entries of the deep list (LF_DEEP_CAP)          DK_LF_ARENA         members of the deep groups' arena (n)
  DK_LF_GIANT_CAP     subgroups of the giant list (LF_GIANT_CAP)      DK_LF_GIANT_ARENA   members of the giant list (LF_GIANT_ARENA)
  DK_LF_GIANT_ROUNDS  grid-wide measures of giant extensions          DK_LF_ROUNDS        global-sort rounds of the big groups (LF_MAX_ROUNDS)
  DK_PACKED_ROUNDS    rounds of the packed sort before its guard re-runs a block alone (PACKED_MAX_ROUNDS)
Knobs are read once per process: every setting runs in a fresh subprocess.  Below a limit the route must show the give-up (lfirst_fallback /
packed_guard); at or above it, the route equals the default run's.  Every run checks L and the origin against the oracle and the workspace
peak of a context sized exactly to its largest input; once per setting the inverse and the dark stream as well.  The limits are placed from a
default run's trace (DK_TRACE=1): how many groups went the deep way (N), how many big rounds ran (R), where the deep list stood when a round
stalled (the groups listed behind that point come from k_lf_finish's LD_LIST listing alone)."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

TUNING_LIB = os.path.join(ROOT, "dark_amd", "libdark_amd_tuning.so")
TIMEOUT = 240  # seconds per subprocess; the slowest (the packed checks) takes well under a minute
MODELS = ("dark", "exp", "ybs", "simple", "rawdc")

# One setting, in a fresh process on the tuning library: the inputs named in the spec, loaded from the parent's .npy files.
WORKER = r"""
import json, os, sys
root, spec = sys.argv[1], json.loads(sys.argv[2])
sys.path.insert(0, root)
import numpy as np
import dark_amd
d = spec["dir"]
def load(name):
    return np.load(os.path.join(d, name + ".npy"))
def ws_ok(ctx, what):
    st = ctx.stats()
    assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], (what, st["ws_peak_bytes"], st["ws_size_bytes"])
out = {}
if spec["mode"] == "single":
    texts = {k: load(k + ".text") for k in spec["inputs"]}
    with dark_amd.Context(max(len(t) for t in texts.values())) as ctx:
        for k, t in texts.items():
            sys.stderr.write("@@@ %s\n" % k)
            sys.stderr.flush()
            bwt, origin = ctx.bwt_forward(t)
            st = ctx.stats()
            out[k] = dict(routes=sorted(st["routes"]), rounds=int(st["rounds"]))
            assert origin == int(load(k + ".origin")), (k, "origin", origin)
            bad = np.flatnonzero(np.frombuffer(bwt, np.uint8) != load(k + ".bwt"))
            assert len(bad) == 0, (k, "L differs from the oracle's at %d places, first %d" % (len(bad), bad[0]), out[k]["routes"])
            ws_ok(ctx, k)
            if k == spec["full"]:
                back = ctx.bwt_inverse(bwt, origin)
                assert np.frombuffer(back, np.uint8).tobytes() == t.tobytes(), (k, "inverse")
                s = ctx.block_encode("dark", t)
                assert bytes(s) == load(k + ".dark").tobytes(), (k, "dark stream")
                out[k]["stream_routes"] = sorted(ctx.stats()["routes"])
else:  # a pack: every block as by the single-block calls, through every entry point that patches guarded origins
    sys.path.insert(0, os.path.join(root, "tests"))
    import torch
    from test_gpu_packed import check_pack, dev
    count = int(load("pack.count"))
    blocks = [load("pack.%d.text" % i) for i in range(count)]
    sizes = [len(b) for b in blocks]
    with dark_amd.Context(sum(sizes)) as ctx:
        d_in, _ = check_pack(ctx, blocks)  # L, origin, init, dist, sym, rank of every block against dev_bwt_forward / dev_dc_encode
        ws_ok(ctx, "pack")
        d_bwt = torch.empty(sum(sizes), dtype=torch.uint8, device="cuda")
        origins = ctx.dev_bwt_forward_packed(d_in, sizes, d_bwt)
        st = ctx.stats()
        out["pack"] = dict(routes=sorted(st["routes"]), rounds=int(st["rounds"]))
        bwt = d_bwt.cpu().numpy()
        off = np.concatenate([[0], np.cumsum(sizes)])
        for i in range(count):
            if sizes[i] <= (1 << 20):
                assert origins[i] == int(load("pack.%d.origin" % i)), ("origin of block", i)
                assert np.array_equal(bwt[off[i]:off[i + 1]], load("pack.%d.bwt" % i)), ("L of block", i)
        single = {}
        for model in spec["models"]:
            streams, flags = ctx.dev_packed_encode(model, d_in, sizes, host_threads=4)
            for i, b in enumerate(blocks):
                want = ctx.dev_block_encode(model, dev(b), len(b), out=np.empty(10 * len(b) + 4096, dtype=np.uint8))
                assert bytes(streams[i]) == bytes(want), (model, "stream of block", i)
                assert flags[i] == ctx.last_block_flags(), (model, "flags of block", i)
                if model == "dark":
                    single[i] = bytes(want)
        with ctx.batch_begin("dark", host_threads=3) as bt:  # pushes of single blocks and of packs, interleaved
            bt.push(dev(blocks[0]), sizes[0])
            bt.push_packed(dev(np.concatenate(blocks[1:9])), sizes[1:9])
            bt.push(dev(blocks[9]), sizes[9])
            bt.push_packed(dev(np.concatenate(blocks[10:])), sizes[10:])
            got = bt.finish()
        assert [bytes(g) for g in got] == [single[i] for i in range(count)], "Batch.push_packed"
        ws_ok(ctx, "pack encode")
    if spec.get("big"):  # the largest block a pack takes, re-run alone by the guard in a context of exactly its size
        t = load("big.text")
        n = len(t)
        with dark_amd.Context(n) as ctx:
            d = dev(t)
            streams, flags = ctx.dev_packed_encode("dark", d, [n], host_threads=4)
            st = ctx.stats()
            out["big"] = dict(routes=sorted(st["routes"]), rounds=int(st["rounds"]))
            ws_ok(ctx, "big")
            assert bytes(streams[0]) == bytes(ctx.dev_block_encode("dark", d, n)), "big block stream"
            assert flags[0] == ctx.last_block_flags(), "big block flags"
            ws_ok(ctx, "big, single")
print("RESULT " + json.dumps(out))
"""

_dead = []  # a subprocess that died by a signal or ran out of time: nothing more is started


def _env(knobs):
    e = {k: v for k, v in os.environ.items() if not k.startswith("DK_")}
    e.update({k: str(v) for k, v in knobs.items()})
    assert os.path.exists(TUNING_LIB), "build the tuning library: python dark_amd/build.py --tuning (__graft_entry__.build() does)"
    e["DARK_AMD_LIB"] = TUNING_LIB
    return e


def _call(cmd, env, what, cwd=None):
    if _dead:
        pytest.fail("not started: an earlier run of this module died (%s)" % _dead[0])
    try:
        p = subprocess.run(cmd, env=env, cwd=cwd, capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired:
        _dead.append("%s timed out" % what)
        pytest.fail("%s: no answer within %d s" % (what, TIMEOUT))
    if p.returncode < 0:
        _dead.append("%s: signal %d" % (what, -p.returncode))
        pytest.fail("%s died by signal %d\n%s" % (what, -p.returncode, p.stderr[-3000:]))
    assert p.returncode == 0, "%s failed\n%s%s" % (what, p.stdout[-2000:], p.stderr[-4000:])
    return p


def _run(data, knobs, inputs, full=None, mode="single", **extra):
    """one setting in a fresh process -> ({input: {"routes", "rounds"}}, stderr)"""
    spec = dict(mode=mode, dir=data["dir"], inputs=list(inputs), full=full if full is not None else (inputs[0] if inputs else None), **extra)
    what = " ".join("%s=%s" % kv for kv in sorted(knobs.items())) or "default"
    p = _call([sys.executable, "-c", WORKER, ROOT, json.dumps(spec)], _env(knobs), what)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout + p.stderr
    return json.loads(line[-1][7:]), p.stderr


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------

def _passages(base, count, copies, seed):
    """text with `count` passages of 200 .. 800 bytes, each written over it `copies` times: groups of a few hundred members that do not
    split on text.  The big list stalls on them, lets them go (groups up to LF_DEEP_MAX members) and k_lf_finish lists them (LD_LIST)."""
    rng = np.random.default_rng(seed)
    t = base[:2_000_000].copy()
    for _ in range(count):
        ln = int(rng.integers(200, 800))
        src = int(rng.integers(0, len(base) - ln))
        seg = base[src:src + ln].copy()
        for o in rng.integers(0, len(t) - ln, size=copies):
            t[o:o + ln] = seg
    return t


def _twice_giant(base):
    """Z A B A C A C: the three suffixes in front of the copies of A are one live group; measured against the first of them (A B ...) the
    other two part from it at the same place and stay together for all of C: a second grid-wide measure"""
    a, b, c = base[:300_000], base[400_000:600_000], base[700_000:1_000_000]
    assert b[-1] != c[-1]
    return np.concatenate([base[2_000_000:2_001_000], a, b, a, c, a, c])


def _inputs():
    from dark_amd import datagen
    base = datagen.wiki_like(3_000_000, 12)
    return {
        "passages_a": _passages(base, 40, 300, 1),        # deep groups and a stalled round (case a)
        "passages_b": _passages(base, 200, 300, 2),
        "halves": np.concatenate([base[:1_200_000]] * 2),  # one giant round (case c)
        "three": np.concatenate([base[:800_000]] * 3),     # giant subgroups again after the first measure
        "nested": np.concatenate([base[:700_000], base[100_000:700_000], base[:700_000]]),  # copies inside copies
        "twice": _twice_giant(base),
        "words": np.frombuffer(datagen.word_like(3_000_000, 5), np.uint8).copy(),  # five big rounds (case d)
    }


DEEP = ("passages_a", "passages_b")
GIANT = ("halves", "three", "nested", "twice")


@pytest.fixture(scope="module")
def data(tmp_path_factory, orc):
    d = tmp_path_factory.mktemp("fallbacks")
    texts = _inputs()
    for k, t in texts.items():
        t = np.ascontiguousarray(t, np.uint8)
        bwt, origin = orc.bwt_forward(t)
        np.save(d / (k + ".text.npy"), t)
        np.save(d / (k + ".bwt.npy"), np.asarray(bwt, np.uint8))
        np.save(d / (k + ".origin.npy"), np.array(origin, np.int64))
        np.save(d / (k + ".dark.npy"), np.frombuffer(orc.block_dc_encode("dark", t), np.uint8))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_packed import mixed_blocks
    blocks = mixed_blocks()
    np.save(d / "pack.count.npy", np.array(len(blocks), np.int64))
    for i, b in enumerate(blocks):
        b = np.ascontiguousarray(b, np.uint8)
        np.save(d / ("pack.%d.text.npy" % i), b)
        if len(b) <= (1 << 20):
            bwt, origin = orc.bwt_forward(b, orc.sa_naive(b) if len(b) < 64 else None)
            np.save(d / ("pack.%d.bwt.npy" % i), np.asarray(bwt, np.uint8))
            np.save(d / ("pack.%d.origin.npy" % i), np.array(origin, np.int64))
    from dark_amd import datagen
    from dark_amd._lib import DK_PACKED_MAX_BLOCK_BYTES
    np.save(d / "big.text.npy", np.ascontiguousarray(datagen.wiki_like(DK_PACKED_MAX_BLOCK_BYTES, 3), np.uint8))
    return dict(dir=str(d), names=list(texts))


def _trace_numbers(err):
    """per input of a DK_TRACE=1 run: N (groups that went the deep way), R (big rounds), the deep list's length at each stalled round"""
    out = {}
    for part in err.split("@@@ ")[1:]:
        name, body = part.split("\n", 1)
        deep = [int(x) for x in re.findall(r"L-first: (\d+) groups went the deep way", body)]
        out[name] = dict(N=deep[-1] if deep else 0, R=len(re.findall(r"L-first round \d+: big list", body)),
                         stalled_at=[int(x) for x in re.findall(r"stalled round, .* deep list at (\d+)", body)],
                         G=len(re.findall(r"L-first: giant round \d+: \d+ subgroups", body)))
    return out


@pytest.fixture(scope="module")
def default(data):
    res, err = _run(data, {"DK_TRACE": 1}, data["names"])
    nums = _trace_numbers(err)
    for k in data["names"]:
        res[k].update(nums[k])
        assert "lfirst_fallback" not in res[k]["routes"] and "lfirst" in res[k]["routes"], (k, res[k])
    return res


def _check_routes(res, default, want_fallback, setting):
    for k, fb in want_fallback.items():
        routes = res[k]["routes"]
        if fb:
            assert "lfirst_fallback" in routes, (setting, k, routes, default[k])
        else:
            assert routes == default[k]["routes"], (setting, k, routes, default[k]["routes"])


# ---- a. the deep list -----------------------------------------------------------------------------------------------------------------------

def test_deep_list_cap(data, default):
    """Caps 0, N/2, N - 1, N, N + 1 of every input's N, a few more just below N, and the deep list's length at the stalled round: from there on
    only the next round's LD_LIST listing (k_lf_finish) reserves entries before k_lf_medium.  A cap below N must give up, a cap of N or more
    must take the default route; L is the oracle's either way."""
    caps = {0}
    for k in DEEP:
        n, stalled_at = default[k]["N"], default[k]["stalled_at"]
        assert n > 100 and stalled_at, ("the input must have deep groups and a stalled round", k, default[k])
        assert "lfirst_deep" in default[k]["routes"] and "lfirst_big_round" in default[k]["routes"], (k, default[k])
        caps |= {n // 2, n - 1, n, n + 1} | set(stalled_at)
    n0 = default[DEEP[0]]["N"]
    caps |= {n0 - 2, n0 - 3, n0 - 5, n0 - 8}
    for cap in sorted(caps):
        res, _ = _run(data, {"DK_LF_DEEP_CAP": cap}, DEEP)
        _check_routes(res, default, {k: cap < default[k]["N"] for k in DEEP}, "DK_LF_DEEP_CAP=%d" % cap)
    res, _ = _run(data, {"DK_LF_DEEP_CAP": 0, "DK_POISON": 165}, DEEP)
    _check_routes(res, default, {k: True for k in DEEP}, "DK_LF_DEEP_CAP=0 DK_POISON=165")


# ---- b. the arena ----------------------------------------------------------------------------------------------------------------------------

def test_arena_cap(data, default):
    res, _ = _run(data, {"DK_LF_ARENA": 1}, DEEP)
    _check_routes(res, default, {k: True for k in DEEP}, "DK_LF_ARENA=1")


# ---- c. the giant list ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("knobs", [{"DK_LF_GIANT_CAP": 0}, {"DK_LF_GIANT_ARENA": 1}, {"DK_LF_GIANT_ROUNDS": 1}, {"DK_LF_GIANT_ROUNDS": 2}])
def test_giant_list_limits(data, default, knobs):
    """A full giant list or arena gives up wherever a giant common extension was measured.  G = the giant rounds an input needs (default
    trace): two identical halves, three copies and copies inside copies need one, Z A B A C A C two -- fewer rounds than G give up."""
    for k in GIANT:
        assert "lfirst_giant" in default[k]["routes"] and default[k]["G"] >= 1, (k, default[k])
    assert default["twice"]["G"] == 2, default["twice"]
    g = knobs.get("DK_LF_GIANT_ROUNDS")
    fallback = [k for k in GIANT if g is None or default[k]["G"] > g]
    res, _ = _run(data, knobs, GIANT, full=fallback[0] if fallback else GIANT[0])
    _check_routes(res, default, {k: k in fallback for k in GIANT}, knobs)


# ---- d. the round limit ---------------------------------------------------------------------------------------------------------------------

def test_round_limit(data, default):
    """R big rounds by the default trace: a limit of R - 1 gives up after L has been partly written, R does not.  Once more with an early pass
    on the side stream after every round (it has ordered deep groups when the path gives up), and once with the workspace poisoned."""
    r = default["words"]["R"]
    assert r >= 3, default["words"]
    res, _ = _run(data, {"DK_LF_ROUNDS": r - 1}, ["words"])
    _check_routes(res, default, {"words": True}, "DK_LF_ROUNDS=R-1")
    res, _ = _run(data, {"DK_LF_ROUNDS": r}, ["words"])
    _check_routes(res, default, {"words": False}, "DK_LF_ROUNDS=R")
    res, err = _run(data, {"DK_LF_ROUNDS": r - 1, "DK_LF_FORK": 100000000, "DK_LF_REFORK": 1, "DK_TRACE": 1}, ["words"])
    _check_routes(res, default, {"words": True}, "DK_LF_ROUNDS=R-1 with early passes")
    assert "ordered beside the rounds" in err and "round limit" in err, err[-3000:]
    res, _ = _run(data, {"DK_LF_ROUNDS": r - 1, "DK_POISON": 165}, ["words"])
    _check_routes(res, default, {"words": True}, "DK_LF_ROUNDS=R-1 DK_POISON=165")


# ---- e. the packed guard --------------------------------------------------------------------------------------------------------------------

def _cli_input(tmp_path):
    from dark_amd import datagen
    half = datagen.wiki_like(30000, seed=9)
    data = np.concatenate([half, half, datagen.wiki_like(1 << 20, seed=21), datagen.acgt(300000), datagen.english_like(400000)])
    src = tmp_path / "in.bin"
    np.ascontiguousarray(data, np.uint8).tofile(src)
    return src


def _cli(src, run_dir, knobs, packed):
    os.makedirs(run_dir, exist_ok=True)
    env = _env(knobs)
    env["PYTHONPATH"] = ROOT
    cmd = [sys.executable, "-m", "dark_amd.cli", "-b", "65536", "--host-threads", "4"] + (["--packed"] if packed else []) + [str(src)]
    _call(cmd, env, "cli %s%s" % (" ".join("%s=%s" % kv for kv in knobs.items()), " --packed" if packed else ""), cwd=str(run_dir))
    from dark_amd.cli import EXTENSION, output_name
    with open(os.path.join(run_dir, output_name(str(src), EXTENSION)), "rb") as f:  # (the CLI writes into its working directory)
        return f.read()


def test_packed_guard(data, tmp_path):
    """R = the rounds of a default packed forward over the mixed pack (it holds two identical halves and a 65 537-byte text block, so the
    single-block path behind the guard runs the L-first path).  At 0, 1, R - 1 and R rounds: every block's results equal the single-block
    calls', through dev_bwt_forward_packed, dev_packed_encode (all five models), Batch.push_packed and the CLI's --packed archive; the guard is
    taken exactly when rounds are cut short (or already in the default run).  At 0 rounds the largest block a pack takes is re-run alone in a
    context of exactly its size."""
    base, _ = _run(data, {}, [], mode="pack", models=["dark"])
    r, guarded = base["pack"]["rounds"], "packed_guard" in base["pack"]["routes"]
    assert r >= 3, base
    src = _cli_input(tmp_path)
    plain = _cli(src, tmp_path / "plain", {}, False)
    for rounds in sorted({0, 1, r - 1, r}):
        res, _ = _run(data, {"DK_PACKED_ROUNDS": rounds}, [], mode="pack", models=list(MODELS), big=rounds == 0)
        assert res["pack"]["rounds"] <= rounds, (rounds, res["pack"])
        assert ("packed_guard" in res["pack"]["routes"]) == (rounds < r or guarded), (rounds, r, res["pack"], base["pack"])
        if rounds == 0:
            assert res["big"]["routes"] == ["packed_guard"], res["big"]
        packed = _cli(src, tmp_path / ("packed%d" % rounds), {"DK_PACKED_ROUNDS": rounds}, True)
        assert packed == plain, "DK_PACKED_ROUNDS=%d: the --packed archive differs from the plain one" % rounds
        shutil.rmtree(tmp_path / ("packed%d" % rounds))
