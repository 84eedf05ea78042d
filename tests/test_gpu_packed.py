"""The packed forward path (include/dark_amd.h, csrc/packed.hip): many blocks back to back in one device buffer, one segmented pass.
Every block's results must equal the single-block entry points' (L / origin, the DC arrays, the coded streams and the flags)."""
import numpy as np
import pytest
import torch

import dark_amd
from dark_amd import datagen
from dark_amd._lib import DK_E_ARG, DK_E_MODEL, DK_FLAG_HAS_FF, DK_FLAG_SINGLE_SYMBOL

pytestmark = pytest.mark.gpu
CAP = 12 << 20
MODELS = ("dark", "exp", "ybs", "simple", "rawdc")


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()


def mixed_blocks():
    rng = np.random.default_rng(7)
    blocks = [rng.integers(97, 100, size=k, dtype=np.uint8) for k in (1, 2, 3, 17, 4095, 4096, 4097)]
    blocks.append(np.frombuffer(datagen.wiki_like(65537, seed=4), np.uint8))
    blocks.append(np.frombuffer(datagen.english_like(), np.uint8))
    blocks.append(np.frombuffer(datagen.acgt(1 << 20), np.uint8))
    blocks.append(np.full(5000, ord("a"), np.uint8))                                        # a^n
    blocks.append(np.frombuffer(b"ab" * 3000, np.uint8))                                    # (ab)^n
    blocks.append(np.frombuffer(b"abc" * 2000 + b"abd", np.uint8))                         # (abc)^n, broken tail
    half = np.frombuffer(datagen.wiki_like(30000, seed=9), np.uint8)
    blocks.append(np.concatenate([half, half]))                                             # two identical halves
    blocks.append(np.full(777, 0x41, np.uint8))                                             # single symbol
    blocks.append(np.frombuffer(b"x\xffy\xff\xff" * 300, np.uint8))                        # contains 0xFF
    blocks.append(rng.integers(0, 256, size=100000, dtype=np.uint8))                        # random bytes
    return blocks


def per_block_reference(ctx, blocks):
    out = []
    for b in blocks:
        n = len(b)
        d_in = dev(b)
        d_bwt = torch.empty(n, dtype=torch.uint8, device="cuda")
        origin = ctx.dev_bwt_forward(d_in, n, d_bwt)
        d_dist = torch.empty(n, dtype=torch.int32, device="cuda")
        d_sym = torch.empty(n, dtype=torch.uint8, device="cuda")
        d_rank = torch.empty(n, dtype=torch.uint8, device="cuda")
        init, m = ctx.dev_dc_encode(d_bwt, n, d_dist, d_sym, d_rank)
        out.append(dict(bwt=d_bwt.cpu().numpy(), origin=origin, init=init.copy(), m=m, dist=d_dist[:m].cpu().numpy().view(np.uint32),
                        sym=d_sym[:m].cpu().numpy(), rank=d_rank[:m].cpu().numpy()))
    return out


def check_pack(ctx, blocks, ref=None, orc=None):
    sizes = [len(b) for b in blocks]
    total = sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    d_in = dev(np.concatenate(blocks))
    d_bwt = torch.empty(total, dtype=torch.uint8, device="cuda")
    origins = ctx.dev_bwt_forward_packed(d_in, sizes, d_bwt)
    check_pack.routes = ctx.stats()["routes"]
    d_dist = torch.empty(total, dtype=torch.int32, device="cuda")
    d_sym = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_rank = torch.empty(total, dtype=torch.uint8, device="cuda")
    inits, ms = ctx.dev_dc_encode_packed(d_bwt, sizes, d_dist, d_sym, d_rank)
    bwt = d_bwt.cpu().numpy()
    dist, sym, rank = d_dist.cpu().numpy().view(np.uint32), d_sym.cpu().numpy(), d_rank.cpu().numpy()
    if ref is None:
        ref = per_block_reference(ctx, blocks)
    for i, r in enumerate(ref):
        a = off[i]
        assert np.array_equal(bwt[a:a + sizes[i]], r["bwt"]), "L of block %d (%d bytes)" % (i, sizes[i])
        assert origins[i] == r["origin"], "origin of block %d" % i
        if orc is not None and sizes[i] <= (1 << 20):
            want_bwt, want_origin = orc.bwt_forward(blocks[i], orc.sa_naive(blocks[i]) if sizes[i] < 64 else None)
            assert np.array_equal(r["bwt"], want_bwt) and r["origin"] == want_origin
        assert ms[i] == r["m"], "m of block %d" % i
        assert np.array_equal(inits[i], r["init"]), "init of block %d" % i
        m = ms[i]
        assert np.array_equal(dist[a:a + m], r["dist"]), "dist of block %d" % i
        assert np.array_equal(sym[a:a + m], r["sym"]), "sym of block %d" % i
        assert np.array_equal(rank[a:a + m], r["rank"]), "rank of block %d" % i
    return d_in, sizes


def test_mixed_pack_parity(ctx, orc):
    blocks = mixed_blocks()
    d_in, sizes = check_pack(ctx, blocks, orc=orc)
    for model in MODELS:
        streams, flags = ctx.dev_packed_encode(model, d_in, sizes, host_threads=4)
        for i, b in enumerate(blocks):
            want = ctx.dev_block_encode(model, dev(b), len(b), out=np.empty(10 * len(b) + 4096, dtype=np.uint8))
            assert bytes(streams[i]) == bytes(want), "%s stream of block %d" % (model, i)
            assert flags[i] == ctx.last_block_flags(), "%s flags of block %d" % (model, i)
            if model != "rawdc" and not flags[i] & DK_FLAG_HAS_FF:
                assert bytes(ctx.block_decode(model, streams[i], len(b))) == b.tobytes(), "%s round trip of block %d" % (model, i)
    _, flags = ctx.dev_packed_encode("exp", d_in, sizes)
    assert flags[-2] == DK_FLAG_HAS_FF and flags[-3] == DK_FLAG_SINGLE_SYMBOL and flags[0] == DK_FLAG_SINGLE_SYMBOL and flags[7] == 0


def test_guard_identical_halves(ctx):
    half = np.frombuffer(datagen.wiki_like(4 << 20, seed=11), np.uint8)
    blocks = [np.frombuffer(datagen.english_like(100000), np.uint8), np.concatenate([half, half]), np.frombuffer(b"tail" * 100, np.uint8)]
    check_pack(ctx, blocks)
    assert "packed_guard" in check_pack.routes


def test_seeded_fuzz(ctx):
    rng = np.random.default_rng(2024)
    for _ in range(12):
        count = int(rng.integers(1, 40))
        blocks = []
        for _ in range(count):
            n = int(rng.choice([rng.integers(1, 64), rng.integers(1, 5000), rng.integers(1, 70000)]))
            sigma = int(rng.choice([1, 2, 4, 26, 255, 256]))
            blocks.append(rng.integers(0, sigma, size=n, dtype=np.uint8) if sigma < 256 else rng.integers(0, 256, size=n, dtype=np.uint8))
            if rng.integers(0, 4) == 0:  # repeats
                blocks[-1] = np.tile(blocks[-1][:max(1, n // 7)], 7)[:n] if n > 0 else blocks[-1]
        check_pack(ctx, blocks)


def test_errors_then_correct(ctx):
    d_in = dev(np.frombuffer(b"banana" * 100, np.uint8))
    d_out = torch.empty(600, dtype=torch.uint8, device="cuda")
    bad = [[], [0], [300, 0, 300], [CAP + 1], [1 << 24 | 1], [1] * 65537, [CAP // 2 + 1, CAP // 2 + 1]]
    for sizes in bad:
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.dev_bwt_forward_packed(d_in, sizes, d_out)
        assert e.value.code == DK_E_ARG, sizes
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.dev_packed_encode("exp", d_in, sizes)
        assert e.value.code == DK_E_ARG, sizes
    with pytest.raises(dark_amd.DarkError) as e:
        ctx.dev_dc_encode_packed(d_in, [0], d_out, d_out)
    assert e.value.code == DK_E_ARG
    lib = ctx._lib
    import ctypes as C
    ns = (C.c_size_t * 1)(600)
    assert lib.dk_dev_bwt_forward_packed(ctx._h, None, 1, ns, C.c_void_p(d_out.data_ptr()), None) == DK_E_ARG
    with pytest.raises(dark_amd.DarkError) as e:
        ctx.dev_packed_encode(99, d_in, [600])
    assert e.value.code == DK_E_MODEL
    check_pack(ctx, [np.frombuffer(b"banana" * 50, np.uint8)] * 2)


def test_push_packed_mixed_with_pushes(ctx):
    rng = np.random.default_rng(5)
    blocks = [np.frombuffer(datagen.wiki_like(int(rng.integers(1000, 200000)), seed=s), np.uint8) for s in range(9)]
    want = [bytes(ctx.dev_block_encode("exp", dev(b), len(b))) for b in blocks]
    with ctx.batch_begin("exp", host_threads=3) as bt:
        bt.push(dev(blocks[0]), len(blocks[0]))
        bt.push_packed(dev(np.concatenate(blocks[1:5])), [len(b) for b in blocks[1:5]])
        bt.push(dev(blocks[5]), len(blocks[5]))
        bt.push_packed(dev(np.concatenate(blocks[6:9])), [len(b) for b in blocks[6:9]])
        got = bt.finish()
    assert [bytes(g) for g in got] == want


@pytest.mark.parametrize("block_size", [65536, 1000000])
def test_cli_packed_archive_identical(tmp_path, block_size):
    import os
    import shutil
    from dark_amd import cli
    rng = np.random.default_rng(3)
    data = np.concatenate([datagen.wiki_like(2 << 20, seed=21), datagen.acgt(1 << 20), datagen.english_like(900000),
                           rng.integers(0, 255, size=300000, dtype=np.uint8)])
    src = tmp_path / "in.bin"
    data.tofile(src)
    plain = cli.encode_file(str(src), "exp", block_size, host_threads=4)
    shutil.move(plain, str(tmp_path / "plain"))
    packed = cli.encode_file(str(src), "exp", block_size, host_threads=4, packed=True)
    assert open(packed, "rb").read() == open(tmp_path / "plain", "rb").read()
    os.remove(str(src))
    back = cli.decode_file(packed, "exp", host_threads=4)
    assert np.array_equal(np.fromfile(back, dtype=np.uint8), data)
