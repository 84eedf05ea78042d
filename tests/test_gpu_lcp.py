"""LCP arrays on the GPU (dk_dev_lcp and its one-call and packed forms, csrc/lcp.hip).  Every result must equal the
plain model of tests/lcp_model.py (Kasai; pinned by tests/test_lcp_model.py) on the suffix array dev_suffix_array gives.  Every device output
has GUARD words of a known pattern in front of and behind it.  The routes (lane / wave / grid) are asserted from dk_stats.sa_route on inputs
built around the two caps; the tuning build lowers the caps, the lists' capacity and the packed sort's round limit in subprocesses."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dark_amd
from conftest import ROOT
from dark_amd import datagen
from dark_amd._lib import DK_E_ARG
from lcp_model import lcp_kasai

pytestmark = pytest.mark.gpu
CAP = 1 << 19
GUARD = 64
FILL = 0x5A5A5A5A
LANE_CAP, WAVE_CAP = 256, 65536  # csrc/lcp.hip: LCP_LANE_CAP, LCP_WAVE_CAP
TUNING_LIB = os.path.join(ROOT, "dark_amd", "libdark_amd_tuning.so")
TIMEOUT = 120
PACK_SIZES = [1, 2, 4097, 65536, 140000, 1, 3000, 3000]


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


def u8(x):
    return np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8)


class Words:
    """a uint32 device array of n words with GUARD words of FILL on each side; shift: elements the array starts off its natural place"""

    def __init__(self, n, shift=0):
        self.n, self.lo = n, GUARD + shift
        self.buf = torch.full((n + 2 * GUARD + shift,), FILL, dtype=torch.int32, device="cuda")
        self.t = self.buf[self.lo:self.lo + n]

    def host(self):
        return self.buf.cpu().numpy().view(np.uint32)[self.lo:self.lo + self.n].copy()

    def guards_intact(self):
        b = self.buf.cpu().numpy().view(np.uint32)
        return bool((b[:self.lo] == FILL).all() and (b[self.lo + self.n:] == FILL).all())

    def untouched(self):
        return bool((self.buf.cpu().numpy().view(np.uint32) == FILL).all())


def dev_text(t, shift=0):
    buf = torch.zeros(len(t) + shift, dtype=torch.uint8, device="cuda")
    buf[shift:] = torch.from_numpy(np.array(t, dtype=np.uint8))
    return buf[shift:]


def gpu_sa(ctx, t, shift=0):
    sa = Words(len(t), shift)
    ctx.dev_suffix_array(dev_text(t), len(t), sa.t)
    assert sa.guards_intact()
    return sa


def gpu_lcp(ctx, t, shifts=(0, 0, 0)):
    """-> (suffix array, LCP array, routes of the LCP call) through dev_suffix_array + dev_lcp"""
    sa = gpu_sa(ctx, t, shifts[1])
    out = Words(len(t), shifts[2])
    ctx.dev_lcp(dev_text(t, shifts[0]), len(t), sa.t, out.t)
    routes = ctx.stats()["routes"]
    assert out.guards_intact() and sa.guards_intact(), "a store left the outputs"
    return sa.host(), out.host(), routes


def check(ctx, t, shifts=(0, 0, 0)):
    t = u8(t)
    sa, lcp, routes = gpu_lcp(ctx, t, shifts)
    want = lcp_kasai(t, sa)
    bad = np.flatnonzero(lcp != want)
    assert bad.size == 0, "LCP[%d] = %d, model %d (n = %d, %d wrong)" % (bad[0], lcp[bad[0]], want[bad[0]], len(t), bad.size)
    return routes


def fibonacci_word(n):
    a, b = b"a", b"ab"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


def planted(length, seed):
    """a random passage of `length` bytes twice, different bytes in front of and behind the copies: one irreducible common prefix of exactly
    `length` between the copies, and nothing else of more than a few bytes (random bytes below 250; 251 .. 254 are the four fences)"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 250, size=length, dtype=np.uint8)
    fill = [rng.integers(0, 250, size=k, dtype=np.uint8) for k in (100, 37, 211)]
    return np.concatenate([fill[0], [251], p, [252], fill[1], [253], p, [254], fill[2]]).astype(np.uint8)


# ---- edges -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3])
def test_tiny(ctx, n):
    for t in (b"a" * n, b"ab"[:n] + b"a" * (n - min(n, 2)), bytes(range(n, 0, -1)), b"\xff" * n):
        check(ctx, t)


@pytest.mark.parametrize("n", [4095, 4096, 4097, 8193])
def test_one_symbol(ctx, n):
    """a^n: one measured position (suffix n-1 ... 0 in order, LCP[i] = i) and a reducible chain across the tile borders of the fill"""
    t = np.full(n, 97, np.uint8)
    routes = check(ctx, t)
    assert "lcp_long" in routes  # position 1 against position 0: n - 1 bytes in common
    _, lcp, _ = gpu_lcp(ctx, t)
    assert lcp.tolist() == list(range(n))


@pytest.mark.parametrize("name", ["abab", "fibonacci", "period1000"])
def test_periodic(ctx, name):
    rng = np.random.default_rng(5)
    t = {"abab": lambda: b"ab" * 5000 + b"a",
         "fibonacci": lambda: fibonacci_word(75025),
         "period1000": lambda: np.tile(rng.integers(0, 256, size=1000, dtype=np.uint8), 50)[:49999]}[name]()
    check(ctx, t)


# ---- ordinary inputs -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["random", "markov", "zero_and_ff"])
def test_ordinary(ctx, name):
    rng = np.random.default_rng(6)
    t = {"random": lambda: rng.integers(0, 256, size=65537, dtype=np.uint8),
         "markov": lambda: u8(datagen.wiki_like(300000, seed=3)),
         "zero_and_ff": lambda: rng.choice(np.array([0, 255, 1, 254], np.uint8), size=50001)}[name]()
    check(ctx, t)


# ---- the hand-offs: lane -> wave -> grid ------------------------------------------------------------------------------------------------------

HANDOFFS = [(cap + d, "lane" if cap == LANE_CAP else "wave") for cap in (LANE_CAP, WAVE_CAP) for d in (-1, 0, 1)]


def handoff_routes(length):
    """the routes a planted passage of `length` bytes must take at the default caps: a hand-off happens when the bytes are still equal AT the cap"""
    return ({"lcp_long"} if length >= LANE_CAP else set()) | ({"lcp_giant"} if length >= WAVE_CAP else set())


@pytest.mark.parametrize("length,which", HANDOFFS)
def test_handoff(ctx, length, which):
    routes = check(ctx, planted(length, seed=length))
    assert routes & {"lcp_long", "lcp_giant"} == handoff_routes(length), (length, which, routes)


def test_two_identical_halves(ctx):
    h = np.random.default_rng(8).integers(0, 256, size=70000, dtype=np.uint8)
    routes = check(ctx, np.concatenate([h, h]))
    assert {"lcp_long", "lcp_giant"} <= routes


# ---- pointers --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shifts", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)])
def test_pointers_off_their_alignment(ctx, shifts):
    check(ctx, planted(5000, seed=77), shifts)
    check(ctx, u8(datagen.wiki_like(20011, seed=5)), shifts)


# ---- one-call forms --------------------------------------------------------------------------------------------------------------------------

def test_one_call_forms(ctx):
    t = u8(datagen.wiki_like(40001, seed=11))
    sa, lcp, _ = gpu_lcp(ctx, t)
    d_sa, d_lcp = Words(len(t)), Words(len(t))
    ctx.dev_suffix_array_lcp(dev_text(t), len(t), d_sa.t, d_lcp.t)
    assert d_sa.guards_intact() and d_lcp.guards_intact()
    assert np.array_equal(d_sa.host(), sa) and np.array_equal(d_lcp.host(), lcp)
    h_sa, h_lcp = ctx.suffix_array_lcp(t)
    assert h_sa.dtype == np.uint32 and h_lcp.dtype == np.uint32 and np.array_equal(h_sa, sa) and np.array_equal(h_lcp, lcp)
    con = dark_amd.saca.Constructor(len(t))
    try:
        c_sa, c_lcp = con.compute_lcp(t)
        assert np.array_equal(c_sa, sa) and np.array_equal(c_lcp, lcp)
        with pytest.raises(ValueError):
            con.compute_lcp(t[:-1])
        blocks = [t[:1000], t[1000:1001], t[2000:9000]]
        got = con.compute_packed_lcp(blocks)
        for b, (g_sa, g_lcp) in zip(blocks, got):
            one_sa, one_lcp, _ = gpu_lcp(ctx, b)
            assert np.array_equal(g_sa, one_sa) and np.array_equal(g_lcp, one_lcp)
    finally:
        con.context().close()


def test_cpp_mirror_compute_lcp(tmp_path):
    exe = str(tmp_path / "cpp_lcp")
    lib_dir = os.path.join(ROOT, "dark_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_lcp.cpp"),
                           "-L", lib_dir, "-ldark_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=TIMEOUT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cpp lcp ok" in out.stdout


# ---- packs -----------------------------------------------------------------------------------------------------------------------------------

def the_pack():
    rng = np.random.default_rng(9)
    blocks = [rng.integers(0, 256, size=n, dtype=np.uint8) for n in PACK_SIZES]
    blocks[3] = u8(datagen.wiki_like(65536, seed=2))
    blocks[4] = np.concatenate([blocks[4][:70000], blocks[4][:70000]])  # two identical halves
    blocks[7] = blocks[6].copy()                                        # byte-identical neighbours
    assert [len(b) for b in blocks] == PACK_SIZES
    return blocks


def run_pack(ctx, blocks, one_call):
    """-> (suffix arrays, LCP arrays, routes); one_call: dev_suffix_array_packed_lcp, else dev_suffix_array_packed + dev_lcp_packed"""
    sizes = [len(b) for b in blocks]
    total = sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    d_in = dev_text(np.concatenate(blocks))
    d_sa, d_lcp = Words(total), Words(total)
    if one_call:
        ctx.dev_suffix_array_packed_lcp(d_in, sizes, d_sa.t, d_lcp.t)
        routes = ctx.stats()["routes"]
    else:
        ctx.dev_suffix_array_packed(d_in, sizes, d_sa.t)
        routes = ctx.stats()["routes"]
        ctx.dev_lcp_packed(d_in, sizes, d_sa.t, d_lcp.t)
        routes = routes | ctx.stats()["routes"]
    assert d_sa.guards_intact() and d_lcp.guards_intact(), "a store left the outputs"
    sa, lcp = d_sa.host(), d_lcp.host()
    return [sa[off[i]:off[i + 1]] for i in range(len(sizes))], [lcp[off[i]:off[i + 1]] for i in range(len(sizes))], routes


@pytest.fixture(scope="module")
def pack_want(ctx):
    """the single-block call's result for every block of the pack, checked against the model"""
    blocks = the_pack()
    want = []
    for b in blocks:
        sa, lcp, _ = gpu_lcp(ctx, b)
        assert np.array_equal(lcp, lcp_kasai(b, sa))
        want.append((sa, lcp))
    return dict(blocks=blocks, want=want)


@pytest.mark.parametrize("one_call", [False, True])
def test_pack(ctx, pack_want, one_call):
    sas, lcps, routes = run_pack(ctx, pack_want["blocks"], one_call)
    assert {"packed_guard", "lcp_long", "lcp_giant"} <= routes, routes  # the two halves: past the rounds, and 70 000 bytes in common
    for i, (sa, lcp) in enumerate(pack_want["want"]):
        assert np.array_equal(sas[i], sa), "suffix array of block %d" % i
        assert np.array_equal(lcps[i], lcp), "LCP array of block %d" % i
    assert lcps[7][0] == 0 and lcps[7].max() < 3000  # nothing runs on into the identical neighbour


def test_pack_fuzz(ctx):
    rng = np.random.default_rng(2025)
    for k in range(30):
        blocks = []
        for _ in range(int(rng.integers(1, 12))):
            n = int(rng.choice([rng.integers(1, 20), rng.integers(1, 600), rng.integers(1, 5000)]))
            sigma = int(rng.choice([1, 2, 4, 26, 256]))
            b = rng.integers(0, sigma, size=n, dtype=np.uint8)
            if rng.integers(0, 3) == 0:  # repeats, also across block borders
                b = np.tile(b[:max(1, n // 5)], 5)[:n]
            blocks.append(b)
            if rng.integers(0, 4) == 0:
                blocks.append(b.copy())
        sas, lcps, _ = run_pack(ctx, blocks, one_call=bool(k & 1))
        for i, b in enumerate(blocks):
            assert np.array_equal(lcps[i], lcp_kasai(b, sas[i])), "pack %d block %d (%d bytes)" % (k, i, len(b))


# ---- the tuning build: other caps, short lists, every block through the guard ------------------------------------------------------------------

WORKER = r"""
import json, os, sys
root, d = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import dark_amd
from test_gpu_lcp import CAP, gpu_lcp, run_pack
res = []
with dark_amd.Context(CAP) as ctx:
    for k in range(int(np.load(os.path.join(d, "count.npy")))):
        sizes = np.load(os.path.join(d, "%d.sizes.npy" % k)).tolist()
        text, want = np.load(os.path.join(d, "%d.text.npy" % k)), np.load(os.path.join(d, "%d.lcp.npy" % k))
        if len(sizes) == 1:
            _, lcp, routes = gpu_lcp(ctx, text)
        else:
            ends = np.cumsum(sizes)
            _, lcps, routes = run_pack(ctx, [text[e - n:e] for n, e in zip(sizes, ends)], one_call=True)
            lcp = np.concatenate(lcps)
        assert np.array_equal(lcp, want), ("LCP array of case", k)
        res.append(dict(routes=sorted(routes), passes=int(ctx.stats()["lcp_passes"]), rounds=int(ctx.stats()["rounds"])))
print("RESULT " + json.dumps(res))
"""

_dead = []  # a subprocess that died by a signal or ran out of time: nothing more is started


def three_plants():
    return np.concatenate([planted(300, seed=s) for s in (1, 2, 3)])


@pytest.fixture(scope="module")
def saved(tmp_path_factory, ctx, pack_want):
    """inputs and the default build's LCP arrays: the six hand-off texts, the two halves, three planted passages, the pack"""
    d = tmp_path_factory.mktemp("lcp")
    h = np.random.default_rng(8).integers(0, 256, size=70000, dtype=np.uint8)
    cases = [planted(length, seed=length) for length, _ in HANDOFFS] + [np.concatenate([h, h]), three_plants()]
    for k, t in enumerate(cases):
        np.save(d / ("%d.sizes.npy" % k), np.array([len(t)], np.int64))
        np.save(d / ("%d.text.npy" % k), t)
        np.save(d / ("%d.lcp.npy" % k), gpu_lcp(ctx, t)[1])
    k = len(cases)
    np.save(d / ("%d.sizes.npy" % k), np.array(PACK_SIZES, np.int64))
    np.save(d / ("%d.text.npy" % k), np.concatenate(pack_want["blocks"]))
    np.save(d / ("%d.lcp.npy" % k), np.concatenate([lcp for _, lcp in pack_want["want"]]))
    np.save(d / "count.npy", np.array(k + 1, np.int64))
    return str(d)


def run_tuned(saved, **knobs):
    if _dead:
        pytest.fail("not started: an earlier run of this module died (%s)" % _dead[0])
    assert os.path.exists(TUNING_LIB), "build the tuning library: python dark_amd/build.py --tuning"
    env = {k: v for k, v in os.environ.items() if not k.startswith("DK_")}
    env.update(DARK_AMD_LIB=TUNING_LIB, **{k: str(v) for k, v in knobs.items()})
    try:
        p = subprocess.run([sys.executable, "-c", WORKER, ROOT, saved], env=env, capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired:
        _dead.append("%s timed out" % knobs)
        pytest.fail("%s: no answer within %d s" % (knobs, TIMEOUT))
    if p.returncode < 0:
        _dead.append("%s: signal %d" % (knobs, -p.returncode))
        pytest.fail("%s died by signal %d\n%s" % (knobs, -p.returncode, p.stderr[-3000:]))
    assert p.returncode == 0, "%s failed\n%s%s" % (knobs, p.stdout[-2000:], p.stderr[-4000:])
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def test_lower_caps_take_the_other_routes(saved):
    """lane cap 32, wave cap 128: every planted passage (255 bytes and more) now ends in the grid's kernel, with the same arrays"""
    res = run_tuned(saved, DK_LCP_LANE_CAP=32, DK_LCP_WAVE_CAP=128)
    for r in res:
        assert {"lcp_long", "lcp_giant"} <= set(r["routes"]), res
    # and a lane cap above every passage but the halves: the small hand-off inputs stay with the lanes
    res = run_tuned(saved, DK_LCP_LANE_CAP=1024, DK_LCP_WAVE_CAP=1 << 20)
    for k in range(3):
        assert not set(res[k]["routes"]) & {"lcp_long", "lcp_giant"}, res[k]
    for k in range(3, 7):
        assert "lcp_long" in res[k]["routes"] and "lcp_giant" not in res[k]["routes"], res[k]


@pytest.mark.parametrize("cap,passes", [(2, 2), (1, 3)])
def test_short_lists_take_more_passes(saved, cap, passes):
    """three planted passages of 300 bytes are three listed positions: a list of two takes two passes over the remainder, a list of one three.
    With the lower caps of the second run the three go on to the grid's list, which is as short."""
    three = len(HANDOFFS) + 1
    res = run_tuned(saved, DK_LCP_LIST_CAP=cap)
    assert res[three]["passes"] == passes and "lcp_long" in res[three]["routes"], res[three]
    res = run_tuned(saved, DK_LCP_LIST_CAP=cap, DK_LCP_LANE_CAP=32, DK_LCP_WAVE_CAP=128)
    assert res[three]["passes"] == passes and "lcp_giant" in res[three]["routes"], res[three]


@pytest.mark.parametrize("rounds", [0, 1])
def test_pack_with_every_block_through_the_guard(saved, rounds):
    res = run_tuned(saved, DK_PACKED_ROUNDS=rounds)[-1]
    assert "packed_guard" in res["routes"] and res["rounds"] <= rounds, res


# ---- bad input -------------------------------------------------------------------------------------------------------------------------------

def test_entry_out_of_range(ctx):
    t = u8(datagen.wiki_like(10000, seed=21))
    sa = gpu_sa(ctx, t)
    good = sa.host()
    for where, value in ((0, len(t)), (5000, len(t) + 7), (len(t) - 1, 0xFFFFFFFF)):
        bad = good.copy()
        bad[where] = value
        sa.t.copy_(torch.from_numpy(bad.view(np.int32)))
        out = Words(len(t))
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.dev_lcp(dev_text(t), len(t), sa.t, out.t)
        assert e.value.code == DK_E_ARG and out.untouched()
    sizes = [4000, 6000]
    psa = Words(len(t))
    ctx.dev_suffix_array_packed(dev_text(t), sizes, psa.t)
    bad = psa.host()
    bad[100] = 4000  # in range for the whole text, not for its block
    psa.t.copy_(torch.from_numpy(bad.view(np.int32)))
    out = Words(len(t))
    with pytest.raises(dark_amd.DarkError) as e:
        ctx.dev_lcp_packed(dev_text(t), sizes, psa.t, out.t)
    assert e.value.code == DK_E_ARG and out.untouched()
    check(ctx, t)  # the context is usable afterwards


@pytest.mark.parametrize("damage", ["swapped", "duplicated", "all_zero", "reversed"])
def test_in_range_but_no_suffix_array(ctx, damage):
    """the values are unspecified; the call returns, the guards are intact and every value is at most n"""
    t = np.concatenate([planted(70000, seed=4), np.full(3000, 7, np.uint8)])
    n = len(t)
    sa = gpu_sa(ctx, t)
    v = sa.host()
    if damage == "swapped":
        v[[10, n - 10]] = v[[n - 10, 10]]
    elif damage == "duplicated":
        v[n // 2] = v[n // 2 - 1]
    elif damage == "all_zero":
        v[:] = 0
    else:
        v = v[::-1].copy()
    sa.t.copy_(torch.from_numpy(v.view(np.int32)))
    out = Words(n)
    ctx.dev_lcp(dev_text(t), n, sa.t, out.t)
    assert out.guards_intact() and sa.guards_intact()
    assert int(out.host().max()) <= n
    sizes = [n // 3, n - n // 3]
    v = np.minimum(v, sizes[0] - 1).astype(np.uint32)  # in range for both blocks
    sa.t.copy_(torch.from_numpy(v.view(np.int32)))
    out = Words(n)
    ctx.dev_lcp_packed(dev_text(t), sizes, sa.t, out.t)
    got = out.host()
    assert out.guards_intact() and int(got[:sizes[0]].max()) <= sizes[0] and int(got[sizes[0]:].max()) <= sizes[1]


def test_arguments(ctx):
    t = u8(b"banana" * 50)
    d_in, sa, out = dev_text(t), gpu_sa(ctx, t), Words(len(t))
    lib, h = ctx._lib, ctx._h
    p_in, p_sa, p_out = C.c_void_p(d_in.data_ptr()), C.c_void_p(sa.t.data_ptr()), C.c_void_p(out.t.data_ptr())
    ns = (C.c_size_t * 1)(len(t))
    host = np.zeros(len(t), np.uint32)
    p_host, p_text = host.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p)
    for n in (len(t), 0, CAP + 1):
        for args in ((None, n, p_sa, p_out), (p_in, n, None, p_out), (p_in, n, p_sa, None)) if n == len(t) else ((p_in, n, p_sa, p_out),):
            assert lib.dk_dev_lcp(h, *args) == DK_E_ARG
            assert lib.dk_dev_suffix_array_lcp(h, *args) == DK_E_ARG
    assert lib.dk_suffix_array_lcp(h, None, len(t), p_host, p_host) == DK_E_ARG
    assert lib.dk_suffix_array_lcp(h, p_text, len(t), None, p_host) == DK_E_ARG
    assert lib.dk_suffix_array_lcp(h, p_text, len(t), p_host, None) == DK_E_ARG
    assert lib.dk_suffix_array_lcp(h, p_text, 0, p_host, p_host) == DK_E_ARG
    for fn in (lib.dk_dev_lcp_packed, lib.dk_dev_suffix_array_packed_lcp):
        assert fn(h, None, 1, ns, p_sa, p_out) == DK_E_ARG
        assert fn(h, p_in, 1, None, p_sa, p_out) == DK_E_ARG
        assert fn(h, p_in, 1, ns, None, p_out) == DK_E_ARG
        assert fn(h, p_in, 1, ns, p_sa, None) == DK_E_ARG
        assert fn(h, p_in, 0, ns, p_sa, p_out) == DK_E_ARG
        assert fn(None, p_in, 1, ns, p_sa, p_out) == DK_E_ARG
    for args in ((None, 1, ns, p_host, p_host), (p_text, 1, None, p_host, p_host), (p_text, 1, ns, None, p_host), (p_text, 1, ns, p_host, None),
                 (p_text, 0, ns, p_host, p_host)):
        assert lib.dk_suffix_array_packed_lcp(h, *args) == DK_E_ARG
    for sizes in ([300, 0], [(1 << 24) + 1], [CAP, 1]):
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.dev_lcp_packed(d_in, sizes, sa.t, out.t)
        assert e.value.code == DK_E_ARG
    assert out.untouched()
    check(ctx, t)


def test_decoder_context_refuses():
    """every LCP entry of the header, by name: DK_E_ARG naming the entry, nothing allocated or written, and the context goes on serving the inverse"""
    import re
    header = open(os.path.join(ROOT, "include", "dark_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(dk_[a-z0-9_]*lcp[a-z0-9_]*)\s*\(", header))
    t = u8(b"banana" * 50)
    n = len(t)
    d_in = dev_text(t)
    d_sa, d_lcp = Words(n), Words(n)
    with dark_amd.Context(CAP) as full:
        L, origin = full.bwt_forward(t)
    with dark_amd.Context(n, purpose="decoder") as dec:
        assert np.array_equal(dec.bwt_inverse(L, origin), t)
        calls = {"dk_dev_lcp": lambda: dec.dev_lcp(d_in, n, d_sa.t, d_lcp.t),
                 "dk_dev_suffix_array_lcp": lambda: dec.dev_suffix_array_lcp(d_in, n, d_sa.t, d_lcp.t),
                 "dk_suffix_array_lcp": lambda: dec.suffix_array_lcp(t),
                 "dk_dev_lcp_packed": lambda: dec.dev_lcp_packed(d_in, [n], d_sa.t, d_lcp.t),
                 "dk_dev_suffix_array_packed_lcp": lambda: dec.dev_suffix_array_packed_lcp(d_in, [n], d_sa.t, d_lcp.t),
                 "dk_suffix_array_packed_lcp": lambda: dec.suffix_array_packed_lcp([t])}
        assert declared == set(calls), sorted(declared ^ set(calls))
        for name, call in calls.items():
            peak = dec.stats()["ws_peak_bytes"]
            with pytest.raises(dark_amd.DarkError) as e:
                call()
            msg = dec._lib.dk_last_error(dec._h).decode()
            assert e.value.code == DK_E_ARG and msg.startswith(name + ":") and "decoder context" in msg, msg
            assert dec.stats()["ws_peak_bytes"] == peak, name
            assert np.array_equal(dec.bwt_inverse(L, origin), t), "the inverse after the refused " + name
        assert d_sa.untouched() and d_lcp.untouched()


# ---- workspace -------------------------------------------------------------------------------------------------------------------------------

def test_workspace_of_exactly_sized_contexts(pack_want):
    t = u8(datagen.wiki_like(200000, seed=17))
    with dark_amd.Context(len(t)) as exact:
        d_sa, d_lcp = Words(len(t)), Words(len(t))
        exact.dev_suffix_array_lcp(dev_text(t), len(t), d_sa.t, d_lcp.t)
        st = exact.stats()
        assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], st
        sa, lcp = exact.suffix_array_lcp(t)
        st = exact.stats()
        assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], st
        assert np.array_equal(sa, d_sa.host()) and np.array_equal(lcp, d_lcp.host())
        assert np.array_equal(lcp, lcp_kasai(t, sa))
    blocks = pack_want["blocks"]
    with dark_amd.Context(sum(PACK_SIZES)) as exact:
        _, lcps, routes = run_pack(exact, blocks, one_call=True)
        st = exact.stats()
        assert "packed_guard" in routes and 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], st
        assert all(np.array_equal(g, w[1]) for g, w in zip(lcps, pack_want["want"]))
