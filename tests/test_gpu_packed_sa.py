"""Packed suffix arrays (dk_dev_suffix_array_packed / dk_suffix_array_packed, csrc/packed.hip k_pk_emit): the suffix array of every block of
a pack from one segmented device pass.  Every block's suffix array must equal the oracle's (oracle/dark_oracle.c, SA-IS) and what the
single-block entry point gives for the block alone; L and the origins written by the same pass must equal dev_bwt_forward_packed's.

The oracle's SA-IS takes no one-byte input (the reference's does not either); the suffix array of one byte comes from its direct sort."""
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

pytestmark = pytest.mark.gpu
CAP = 12 << 20
GUARD = 64             # guard words on each side of every device output
SA_FILL = 0x5A5A5A5A   # what the guard words (and untouched outputs) hold
L_FILL = 0xA5
TUNING_LIB = os.path.join(ROOT, "dark_amd", "libdark_amd_tuning.so")
TIMEOUT = 120  # seconds per subprocess; a setting takes a few


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()


def u8(x):
    return np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8)


def want_sa(orc, b):
    return orc.sa_sais(b) if len(b) > 1 else orc.sa_naive(b)


def mixed_blocks():
    rng = np.random.default_rng(7)
    blocks = [rng.integers(97, 100, size=k, dtype=np.uint8) for k in (1, 2, 3, 17, 255, 256, 257, 4095, 4096, 4097)]
    blocks.append(u8(datagen.wiki_like(65537, seed=4)))
    blocks.append(u8(datagen.english_like()))
    blocks.append(u8(datagen.acgt(1 << 20)))
    blocks.append(np.full(5000, ord("a"), np.uint8))                 # a^n
    blocks.append(u8(b"ab" * 3000))                                  # (ab)^n
    blocks.append(u8(b"abc" * 2000 + b"abd"))                        # (abc)^n, broken tail
    half = u8(datagen.wiki_like(30000, seed=9))
    # two identical halves.  Alone among text they would resolve inside the rounds; in this pack the random and 0xFF blocks make the pack's
    # alphabet 256 symbols, the first key holds (64 - 5) / 9 = 6 of them and twelve rounds reach 6 * 2^12 = 24 576 < 30 000: this one block
    # goes through the guard, in the middle of the pack
    blocks.append(np.concatenate([half, half]))
    blocks.append(np.full(777, 0x41, np.uint8))                      # one symbol
    blocks.append(u8(b"x\xffy\xff\xff" * 300))                       # contains 0xFF
    blocks.append(rng.integers(0, 256, size=100000, dtype=np.uint8))  # random bytes
    return blocks


class Outputs:
    """device outputs of one pack with GUARD words of a known pattern on each side"""

    def __init__(self, total, with_bwt):
        self.total = total
        self.sa_buf = torch.full((total + 2 * GUARD,), SA_FILL, dtype=torch.int32, device="cuda")
        self.sa = self.sa_buf[GUARD:GUARD + total]
        self.bwt_buf = torch.full((total + 8 * GUARD,), L_FILL, dtype=torch.uint8, device="cuda") if with_bwt else None
        self.bwt = self.bwt_buf[4 * GUARD:4 * GUARD + total] if with_bwt else None

    def guards_intact(self):
        sa = self.sa_buf.cpu().numpy().view(np.uint32)
        ok = (sa[:GUARD] == SA_FILL).all() and (sa[GUARD + self.total:] == SA_FILL).all()
        if self.bwt_buf is not None:
            b = self.bwt_buf.cpu().numpy()
            ok = ok and (b[:4 * GUARD] == L_FILL).all() and (b[4 * GUARD + self.total:] == L_FILL).all()
        return bool(ok)

    def untouched(self):
        ok = (self.sa_buf.cpu().numpy().view(np.uint32) == SA_FILL).all()
        return bool(ok and (self.bwt_buf is None or (self.bwt_buf.cpu().numpy() == L_FILL).all()))


def run_pack(ctx, blocks, with_bwt=True):
    """-> (list of suffix arrays, list of L or None, origins or None, routes of the call)"""
    sizes = [len(b) for b in blocks]
    total = sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    out = Outputs(total, with_bwt)
    origins = ctx.dev_suffix_array_packed(dev(np.concatenate(blocks)), sizes, out.sa, out.bwt)
    routes = ctx.stats()["routes"]
    assert out.guards_intact(), "a store left the outputs"
    sa = out.sa.cpu().numpy().view(np.uint32)
    sas = [sa[off[i]:off[i + 1]] for i in range(len(sizes))]
    if not with_bwt:
        assert origins is None
        return sas, None, None, routes
    bwt = out.bwt.cpu().numpy()
    return sas, [bwt[off[i]:off[i + 1]] for i in range(len(sizes))], origins, routes


def check_against_oracle(ctx, orc, blocks, with_bwt=False):
    sas, _, _, routes = run_pack(ctx, blocks, with_bwt)
    for i, b in enumerate(blocks):
        assert len(b) <= (1 << 20)
        assert np.array_equal(sas[i], want_sa(orc, b)), "suffix array of block %d (%d bytes)" % (i, len(b))
    return routes


@pytest.fixture(scope="module")
def mixed(orc):
    blocks = mixed_blocks()
    return dict(blocks=blocks, sa=[want_sa(orc, b) for b in blocks])


@pytest.fixture(scope="module")
def mixed_default(ctx, mixed):
    """the default build's results for the mixed pack, with L"""
    sas, bwts, origins, routes = run_pack(ctx, mixed["blocks"], with_bwt=True)
    return dict(sa=sas, bwt=bwts, origin=origins, routes=routes)


# ---- 1. mixed pack ---------------------------------------------------------------------------------------------------------------------------

def test_mixed_pack(ctx, mixed, mixed_default):
    blocks = mixed["blocks"]
    sizes = [len(b) for b in blocks]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    for i, b in enumerate(blocks):
        assert np.array_equal(mixed_default["sa"][i], mixed["sa"][i]), "suffix array of block %d (%d bytes) against the oracle" % (i, len(b))
        d_one = torch.empty(len(b), dtype=torch.int32, device="cuda")
        ctx.dev_suffix_array(dev(b), len(b), d_one)
        assert np.array_equal(d_one.cpu().numpy().view(np.uint32), mixed_default["sa"][i]), "block %d against dev_suffix_array" % i
    d_bwt = torch.empty(sum(sizes), dtype=torch.uint8, device="cuda")
    origins = ctx.dev_bwt_forward_packed(dev(np.concatenate(blocks)), sizes, d_bwt)
    bwt = d_bwt.cpu().numpy()
    assert origins == mixed_default["origin"]
    for i in range(len(blocks)):
        assert np.array_equal(bwt[off[i]:off[i + 1]], mixed_default["bwt"][i]), "L of block %d" % i
    sas, _, _, _ = run_pack(ctx, blocks, with_bwt=False)
    for i in range(len(blocks)):
        assert np.array_equal(sas[i], mixed["sa"][i]), "suffix array of block %d without L" % i


# ---- 2. heads and key widths -----------------------------------------------------------------------------------------------------------------

def _small_packs():
    rng = np.random.default_rng(11)
    text = u8(datagen.wiki_like(70000, seed=6))
    many = []
    for _ in range(3000):  # thousands of block heads per workgroup and per tile
        n = int(rng.integers(1, 41))
        sigma = int(rng.choice([1, 2, 4, 26, 256]))
        many.append(rng.integers(0, sigma, size=n, dtype=np.uint8))
    return {
        "one_block": [text[:5000]],
        "64_blocks": [text[100 * i:100 * i + 100] for i in range(64)],
        "65_blocks": [text[100 * i:100 * i + 100] for i in range(65)],  # the block id takes one more bit
        "3000_tiny": many,
        "not_a_multiple_of_256": [text[:1000], text[1000:1777], text[2000:2301]],  # 2078 bytes
    }


@pytest.mark.parametrize("name", ["one_block", "64_blocks", "65_blocks", "3000_tiny", "not_a_multiple_of_256"])
def test_heads_and_key_widths(ctx, orc, name):
    blocks = _small_packs()[name]
    if name == "not_a_multiple_of_256":
        assert sum(len(b) for b in blocks) % 256 != 0
    check_against_oracle(ctx, orc, blocks, with_bwt=(name == "3000_tiny"))


# ---- 3. guard --------------------------------------------------------------------------------------------------------------------------------

def test_guard(ctx, orc):
    """Twelve rounds resolve common prefixes of at most 9 * 2^12 = 36 864 symbols (a first key of at most (64 - blk_bits) / bits = 9 symbols with
    bits >= 7): two identical halves of 100 000 bytes stay unresolved and leave the pack.  The guarded block starts at an odd offset."""
    h = u8(datagen.wiki_like(100000, seed=13))
    blocks = [u8(b"xyz"), u8(datagen.english_like(100000)), np.concatenate([h, h]), u8(b"tail" * 100)]
    assert (len(blocks[0]) + len(blocks[1])) % 2 == 1
    sas, bwts, origins, routes = run_pack(ctx, blocks, with_bwt=True)
    assert "packed_guard" in routes
    for i, b in enumerate(blocks):
        assert np.array_equal(sas[i], want_sa(orc, b)), "suffix array of block %d" % i
        d_bwt = torch.empty(len(b), dtype=torch.uint8, device="cuda")
        origin = ctx.dev_bwt_forward(dev(b), len(b), d_bwt)
        assert origins[i] == origin, "origin of block %d" % i
        assert np.array_equal(bwts[i], d_bwt.cpu().numpy()), "L of block %d" % i
    sas, _, _, routes = run_pack(ctx, blocks, with_bwt=False)
    assert "packed_guard" in routes
    want = want_sa(orc, blocks[2])
    assert np.array_equal(sas[2], want), "the guarded block without L"
    # the guard's workspace: a pack that is one byte and the guarded block, from host memory, on a context of exactly its size
    pair = [u8(b"q"), blocks[2]]
    with dark_amd.Context(1 + len(blocks[2])) as exact:
        got = exact.suffix_array_packed(pair)
        st = exact.stats()
        assert "packed_guard" in st["routes"] and 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], st
        assert np.array_equal(got[0], [0]) and np.array_equal(got[1], want)


def test_long_repeat_resolves_inside_the_rounds(ctx, orc):
    """Two identical halves of 10 000 text bytes: suffixes 0 and 10 000 share 10 000 symbols.  A round at most doubles the depth compared, from
    a first key of at most 9 symbols, so ten rounds reach 9 * 2^10 = 9216 < 10 000: at least eleven are needed.  Twelve reach at least
    6 * 2^12 = 24 576 (the narrowest first key, 256 symbols in the pack) > 10 000: the block stays in the pack, and its suffix array is
    written by k_pk_emit after the rounds, not by the guard."""
    h = u8(datagen.wiki_like(10000, seed=9))
    blocks = [u8(b"xyz"), np.concatenate([h, h]), u8(b"tail" * 100)]
    assert 64 <= len(np.unique(np.concatenate(blocks))) < 128  # 7 bits per symbol: a first key of (64 - 2) / 7 = 8 symbols
    want = [want_sa(orc, b) for b in blocks]
    for with_bwt in (False, True):
        sas, bwts, origins, routes = run_pack(ctx, blocks, with_bwt)
        assert "packed_guard" not in routes
        assert 11 <= ctx.stats()["rounds"] <= 12
        for i in range(len(blocks)):
            assert np.array_equal(sas[i], want[i]), "suffix array of block %d" % i
    _, bwts, origins, _ = run_pack(ctx, blocks, with_bwt=True)
    d_bwt = torch.empty(len(blocks[1]), dtype=torch.uint8, device="cuda")
    assert ctx.dev_bwt_forward(dev(blocks[1]), len(blocks[1]), d_bwt) == origins[1]
    assert np.array_equal(bwts[1], d_bwt.cpu().numpy())


# ---- 4. every block through the guard --------------------------------------------------------------------------------------------------------

WORKER = r"""
import json, os, sys
root, d = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import dark_amd
from test_gpu_packed_sa import CAP, run_pack
count = int(np.load(os.path.join(d, "count.npy")))
blocks = [np.load(os.path.join(d, "%d.text.npy" % i)) for i in range(count)]
with dark_amd.Context(CAP) as ctx:
    sas, bwts, origins, routes = run_pack(ctx, blocks, with_bwt=True)
    rounds = int(ctx.stats()["rounds"])
for i in range(count):
    assert np.array_equal(sas[i], np.load(os.path.join(d, "%d.sa.npy" % i))), ("suffix array of block", i)
    assert np.array_equal(bwts[i], np.load(os.path.join(d, "%d.bwt.npy" % i))), ("L of block", i)
assert origins == [int(x) for x in np.load(os.path.join(d, "origins.npy"))], "origins"
print("RESULT " + json.dumps(dict(routes=sorted(routes), rounds=rounds)))
"""

_dead = []  # a subprocess that died by a signal or ran out of time: nothing more is started


@pytest.fixture(scope="module")
def saved_default(tmp_path_factory, mixed, mixed_default):
    d = tmp_path_factory.mktemp("packed_sa")
    np.save(d / "count.npy", np.array(len(mixed["blocks"]), np.int64))
    for i, b in enumerate(mixed["blocks"]):
        np.save(d / ("%d.text.npy" % i), np.ascontiguousarray(b, np.uint8))
        np.save(d / ("%d.sa.npy" % i), mixed_default["sa"][i])
        np.save(d / ("%d.bwt.npy" % i), mixed_default["bwt"][i])
    np.save(d / "origins.npy", np.array(mixed_default["origin"], np.int64))
    return str(d)


@pytest.mark.parametrize("rounds", [0, 1])
def test_every_block_through_the_guard(saved_default, rounds):
    if _dead:
        pytest.fail("not started: an earlier run of this module died (%s)" % _dead[0])
    assert os.path.exists(TUNING_LIB), "build the tuning library: python dark_amd/build.py --tuning"
    env = {k: v for k, v in os.environ.items() if not k.startswith("DK_")}
    env.update(DARK_AMD_LIB=TUNING_LIB, DK_PACKED_ROUNDS=str(rounds))
    try:
        p = subprocess.run([sys.executable, "-c", WORKER, ROOT, saved_default], env=env, capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired:
        _dead.append("DK_PACKED_ROUNDS=%d timed out" % rounds)
        pytest.fail("DK_PACKED_ROUNDS=%d: no answer within %d s" % (rounds, TIMEOUT))
    if p.returncode < 0:
        _dead.append("DK_PACKED_ROUNDS=%d: signal %d" % (rounds, -p.returncode))
        pytest.fail("DK_PACKED_ROUNDS=%d died by signal %d\n%s" % (rounds, -p.returncode, p.stderr[-3000:]))
    assert p.returncode == 0, "DK_PACKED_ROUNDS=%d failed\n%s%s" % (rounds, p.stdout[-2000:], p.stderr[-4000:])
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert "packed_guard" in res["routes"] and res["rounds"] <= rounds, res


# ---- 5. seeded fuzz --------------------------------------------------------------------------------------------------------------------------

def test_seeded_fuzz(ctx, orc):
    rng = np.random.default_rng(2024)
    for _ in range(12):
        count = int(rng.integers(1, 40))
        blocks = []
        for _ in range(count):
            n = int(rng.choice([rng.integers(1, 64), rng.integers(1, 5000), rng.integers(1, 70000)]))
            sigma = int(rng.choice([1, 2, 4, 26, 255, 256]))
            blocks.append(rng.integers(0, sigma, size=n, dtype=np.uint8) if sigma < 256 else rng.integers(0, 256, size=n, dtype=np.uint8))
            if rng.integers(0, 4) == 0:  # repeats
                blocks[-1] = np.tile(blocks[-1][:max(1, n // 7)], 7)[:n]
        check_against_oracle(ctx, orc, blocks)


# ---- 6. errors, then a correct call on the same context -------------------------------------------------------------------------------------

def test_errors_then_correct(ctx, orc):
    text = u8(b"banana" * 100)
    d_in = dev(text)
    out = Outputs(len(text), with_bwt=True)
    bad = [[], [1] * 65537, [300, 0, 300], [(1 << 24) + 1], [CAP // 2 + 1, CAP // 2 + 1]]
    for sizes in bad:
        for d_bwt in (None, out.bwt):
            with pytest.raises(dark_amd.DarkError) as e:
                ctx.dev_suffix_array_packed(d_in, sizes, out.sa, d_bwt)
            assert e.value.code == DK_E_ARG, sizes
    lib, h = ctx._lib, ctx._h
    ns = (C.c_size_t * 1)(len(text))
    p_in, p_sa, p_bwt = C.c_void_p(d_in.data_ptr()), C.c_void_p(out.sa.data_ptr()), C.c_void_p(out.bwt.data_ptr())
    origin = (C.c_uint32 * 1)(12345)
    call = lib.dk_dev_suffix_array_packed
    assert call(h, None, 1, ns, p_sa, None, None) == DK_E_ARG          # null input
    assert call(h, p_in, 1, None, p_sa, None, None) == DK_E_ARG        # null sizes
    assert call(h, p_in, 1, ns, None, None, None) == DK_E_ARG          # null output
    assert call(h, p_in, 1, ns, p_sa, p_bwt, None) == DK_E_ARG         # L without origins
    assert call(h, p_in, 1, ns, p_sa, None, origin) == DK_E_ARG        # origins without L
    assert call(None, p_in, 1, ns, p_sa, None, None) == DK_E_ARG       # null context
    host_sa = np.full(len(text), SA_FILL, np.uint32)
    p_host = text.ctypes.data_as(C.c_void_p)
    for args in ((None, 1, ns, host_sa.ctypes.data_as(C.c_void_p)), (p_host, 1, None, host_sa.ctypes.data_as(C.c_void_p)), (p_host, 1, ns, None),
                 (p_host, 0, ns, host_sa.ctypes.data_as(C.c_void_p))):
        assert lib.dk_suffix_array_packed(h, *args) == DK_E_ARG
    with ctx.batch_begin("exp", host_threads=1) as bt:  # an open batch owns the workspace
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.dev_suffix_array_packed(d_in, [len(text)], out.sa, out.bwt)
        assert e.value.code == DK_E_ARG
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.suffix_array_packed([text])
        assert e.value.code == DK_E_ARG
        bt.finish()
    assert out.untouched() and (host_sa == SA_FILL).all() and origin[0] == 12345
    check_against_oracle(ctx, orc, [text[:300], text[300:]], with_bwt=True)


# ---- 7. host layers -------------------------------------------------------------------------------------------------------------------------

def test_host_layers(ctx, mixed):
    rng = np.random.default_rng(3)
    blocks = [u8(b"banana"), u8(b"z"), rng.integers(0, 4, size=1000, dtype=np.uint8), u8(datagen.wiki_like(5000, seed=8)), u8(b"ab" * 50)]
    want = [ctx.suffix_array(b) for b in blocks]
    got = ctx.suffix_array_packed(blocks)
    assert len(got) == len(want) and all(g.dtype == np.uint32 and np.array_equal(g, w) for g, w in zip(got, want))
    total = sum(len(b) for b in blocks)
    con = dark_amd.saca.Constructor(total)
    try:
        got = con.compute_packed(blocks)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        with pytest.raises(ValueError):
            con.compute_packed(blocks + [u8(b"x")])
        with pytest.raises(ValueError):
            con.compute(blocks[0])  # compute keeps its exact-size assertion
    finally:
        con.context().close()
    # a context sized exactly to the pack: both entries stay inside the workspace
    blocks = mixed["blocks"]
    with dark_amd.Context(sum(len(b) for b in blocks)) as exact:
        sas, _, _, _ = run_pack(exact, blocks, with_bwt=True)
        st = exact.stats()
        assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], st
        assert all(np.array_equal(s, w) for s, w in zip(sas, mixed["sa"]))
        got = exact.suffix_array_packed(blocks)
        st = exact.stats()
        assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], st
        assert all(np.array_equal(g, w) for g, w in zip(got, mixed["sa"]))


def test_cpp_mirror_compute_packed(tmp_path):
    exe = str(tmp_path / "cpp_packed_sa")
    lib_dir = os.path.join(ROOT, "dark_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_packed_sa.cpp"),
                           "-L", lib_dir, "-ldark_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cpp packed sa ok" in out.stdout
