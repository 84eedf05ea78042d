"""tests/lcp_count_model.py checked without a GPU: its constants are those of csrc/lcp.hip, the vectorised model equals the per-position loop on
a few hundred small random texts and packs (at caps and a chunk small enough that texts of a few hundred bytes reach the lane's, the wave's
and the grid's rule, the grid's with several chunks and with fewer workgroups than chunks), and the cases of tests/test_gpu_profiling.py can
fail: each of the three wrong models of lcp_count_model.VARIANTS gives another number than the right one on a named case."""
import numpy as np
import pytest

import lcp_count_model as C
from lcp_model import lcp_brute, lcp_kasai


def sa_naive(t):
    b = bytes(t)
    return np.array(sorted(range(len(b)), key=lambda i: b[i:]), dtype=np.int64)


def test_constants():
    c = C.read_constants()
    assert c == dict(LCP_LANE_CAP=C.LANE_CAP, LCP_WAVE_CAP=C.WAVE_CAP, LCP_COUNTERS=C.COUNTERS, LCP_BLOCK=256, LCP_GIANT_CHUNK=C.GIANT_CHUNK,
                     LCP_GIANT_GRID=C.GIANT_GRID)
    with open(C.os.path.join(C.ROOT, "dark_amd", "csrc", "lcp.hip")) as f:
        src = f.read()
    # the rules the model restates, where the kernels have them
    assert "} else if (p > s && q > s && t[p - 1] == t[q - 1]) {" in src                   # reducible
    assert "if (i == s) { phi[s + v] = LCP_MARK; return; }" in src                         # the block's first slot: settled, never counted
    assert "if (l == lane_cap && room > lane_cap) {" in src                                # lane -> wave
    assert "const bool settled = differs || room <= wave_cap;" in src                      # wave -> grid
    assert "if (cnt) lcp_count(cnt, l - lane_cap, settled ? 1u : 0u);" in src              # the wave's part
    assert "lcp_count(cnt, room - o0 < LCP_GIANT_CHUNK ? room - o0 : LCP_GIANT_CHUNK, 0u);" in src  # whole chunks
    assert "if (o0 >= s_best) break;" in src and "if (cnt && blockIdx.x == 0 && tid == 0) lcp_count(cnt, 0u, 1u);" in src
    assert "ctx->ws_alloc<unsigned long long>(2 * LCP_COUNTERS)" in src                    # 4 KiB of workspace while profiling


def test_giant_interval():
    # L in the third chunk behind done = 100, room 1000, chunks of 64: 100, 164, 228 must be compared; 292 ... one each for other workgroups
    assert C.giant_interval(L=230, room=1000, done=100, chunk=64, grid=1024) == (192, 900)
    assert C.giant_interval(L=230, room=1000, done=100, chunk=64, grid=2) == (192, 192 + 128)
    assert C.giant_interval(L=228, room=1000, done=100, chunk=64, grid=1) == (192, 256)   # a difference at a chunk's first byte: that chunk too
    assert C.giant_interval(L=227, room=1000, done=100, chunk=64, grid=1) == (128, 192)
    assert C.giant_interval(L=1000, room=1000, done=100, chunk=64, grid=1024) == (900, 900)  # equal up to the end: every chunk, the last one short
    assert C.giant_interval(L=100, room=101, done=100, chunk=64, grid=1024) == (1, 1)


def random_blocks(rng):
    blocks = []
    for _ in range(int(rng.integers(1, 5))):
        n = int(rng.choice([rng.integers(1, 8), rng.integers(1, 80), rng.integers(80, 400)]))
        sigma = int(rng.choice([1, 2, 3, 26]))
        b = rng.integers(0, sigma, size=n, dtype=np.uint8)
        kind = int(rng.integers(0, 4))
        if kind == 0:  # periodic
            b = np.tile(b[:max(1, n // 7)], 8)[:n]
        elif kind == 1 and n > 40:  # a passage twice, other bytes around the copies: one long irreducible value
            k = (n - 6) // 2
            b = np.concatenate([[7], b[:k] % 5, [8, 9], b[:k] % 5, [10], b[:n - 2 * k - 4]]).astype(np.uint8)[:n]
        elif kind == 2 and n > 40:  # the same with one byte of the second copy changed: equal again behind the first difference
            k = (n - 6) // 2
            c = b[:k] % 5
            d = c.copy()
            d[int(rng.integers(0, k))] = 6
            b = np.concatenate([[7], c, [8, 9], d, [10], b[:n - 2 * k - 4]]).astype(np.uint8)[:n]
        blocks.append(np.ascontiguousarray(b, dtype=np.uint8))
    return blocks


def test_model_equals_the_per_position_loop():
    rng = np.random.default_rng(4011)
    seen = dict(longs=0, giants=0, open_interval=0, packs=0)
    for k in range(400):
        blocks = random_blocks(rng)
        sas = [sa_naive(b) for b in blocks]
        if k < 40:  # (the yardstick behind the model's LCP values, once more on these shapes)
            for b, sa in zip(blocks, sas):
                assert np.array_equal(lcp_kasai(b, sa), lcp_brute(b, sa))
        lane_cap, wave_cap = [(4, 16), (16, 16), (16, 48), (8, 100), (256, 65536)][k % 5]
        chunk, grid = [(8, 1024), (16, 2), (32, 1), (4096, 1024)][k % 4]
        got = C.count_model(blocks, sas, lane_cap, wave_cap, chunk, grid)
        want = C.count_loop(blocks, sas, lane_cap, wave_cap, chunk, grid)
        assert got == want, (k, [len(b) for b in blocks], lane_cap, wave_cap, chunk, grid)
        assert got["bytes_lo"] <= got["bytes_hi"] and (got["giants"] or got["bytes_lo"] == got["bytes_hi"])
        seen["longs"] += got["longs"] > 0
        seen["giants"] += got["giants"] > 0
        seen["open_interval"] += got["bytes_lo"] < got["bytes_hi"]
        seen["packs"] += len(blocks) > 1
    assert min(seen.values()) >= 20, seen  # every rule was reached, many times


# ---- the GPU cases can fail ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def counted(orc):
    """name -> (the right model's counts, {variant: its counts}) for every single case and every pack, on the oracle's suffix arrays"""
    lcps, out = {}, {}

    def one(blocks):
        sas = [np.asarray(orc.sa_sais(b) if len(b) > 1 else [0], dtype=np.int64) for b in blocks]
        for b, sa in zip(blocks, sas):
            if b.tobytes() not in lcps:
                lcps[b.tobytes()] = lcp_kasai(b, sa)
        ls = [lcps[b.tobytes()] for b in blocks]
        return C.count_model(blocks, sas, lcps=ls), {v: C.count_model(blocks, sas, variant=v, lcps=ls) for v in C.VARIANTS}
    for name, (t, _) in C.single_cases().items():
        out[name] = one([t])
    for name, (blocks, _) in C.pack_cases().items():
        out["pack:" + name] = one(blocks)
    return out


def test_cases_reach_the_routes_they_name(counted):
    for name, (_, routes) in list(C.single_cases().items()) + [("pack:" + k, v) for k, v in C.pack_cases().items()]:
        c = counted[name][0]
        if routes is not None:
            assert (c["longs"] > 0) == ("lcp_long" in routes) and (c["giants"] > 0) == ("lcp_giant" in routes), (name, c)
        assert c["bytes_hi"] - c["bytes_lo"] <= c["giants"] * C.GIANT_GRID * C.GIANT_CHUNK
    # the interval is open where bytes differ behind the passage, closed where the repeat runs to the block's end
    assert counted["planted90000"][0]["bytes_lo"] < counted["planted90000"][0]["bytes_hi"]
    for name in ("planted255", "planted256", "planted257", "planted65535", "a4097", "a70000", "two_halves"):
        assert counted[name][0]["bytes_lo"] == counted[name][0]["bytes_hi"], name
    assert counted["a70000"][0] == dict(measured=1, bytes_lo=69999, bytes_hi=69999, longs=1, giants=1)  # position 1 against position 0


@pytest.mark.parametrize("variant,where", [("reducible_too", ["a4097", "fibonacci", "pack:the_pack"]),
                                           ("no_wave", ["planted257", "planted65536", "pack:lane_and_wave"]),
                                           ("first_too", ["planted255", "a70000", "pack:giants"])])
def test_wrong_models_differ_on_named_cases(counted, variant, where):
    """what a kernel with that mistake would report lies outside what the right model allows"""
    for name in where:
        right, wrong = counted[name][0], counted[name][1][variant]
        outside = wrong["bytes_lo"] > right["bytes_hi"] or wrong["bytes_hi"] < right["bytes_lo"]
        assert wrong["measured"] != right["measured"] or outside, (variant, name, right, wrong)
    if variant == "no_wave":  # the bytes alone tell it: the positions are the same
        assert all(counted[n][1][variant]["measured"] == counted[n][0]["measured"] for n in where)
