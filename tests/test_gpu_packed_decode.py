"""The packed inverse (include/dark_amd.h dk_dev_bwt_inverse_packed / dk_dev_packed_decode, csrc/bwt.hip k_pib_*):
many blocks back to back in one device buffer, inverted in one segmented pass.  Every block must equal its input and what the single-block
and batched entry points give."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest
import torch

import dark_amd
from dark_amd import datagen
from dark_amd._lib import DK_E_ARG, DK_E_MODEL, DK_E_STREAM, DK_PACKED_MAX_BLOCK_BYTES, DK_PACKED_MAX_BLOCKS

pytestmark = pytest.mark.gpu
CAP = 12 << 20
S = 64  # splitter spacing of the packed inverse


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()


def u8(b):
    return np.frombuffer(b, np.uint8)


def oracle_bwt(orc, b):
    return orc.bwt_forward(b, orc.sa_naive(b) if len(b) < 64 else None)


def block_with_origin(orc, rng, n, multiple):
    """random block of n bytes whose oracle origin is (multiple=True) or is not a multiple of S"""
    for _ in range(5000):
        b = rng.integers(97, 101, size=n, dtype=np.uint8)
        if (oracle_bwt(orc, b)[1] % S == 0) == multiple:
            return b
    raise AssertionError("no block of %d bytes with the wanted origin" % n)


def mixed_blocks(orc):
    rng = np.random.default_rng(11)
    blocks = [rng.integers(97, 100, size=k, dtype=np.uint8) for k in (1, 2, 3, 17)]
    blocks += [rng.integers(0, 256, size=k, dtype=np.uint8) for k in (4095, 4096, 4097)]
    blocks.append(block_with_origin(orc, rng, 200, True))                                  # origin a multiple of S
    blocks.append(block_with_origin(orc, rng, 200, False))
    blocks.append(block_with_origin(orc, rng, 50, False))                                  # shorter than S
    blocks.append(np.full(5000, ord("a"), np.uint8))                                       # a^n
    blocks.append(u8(b"ab" * 3000))                                                        # (ab)^n
    blocks.append(np.full(777, 0x00, np.uint8))                                            # single symbol
    blocks.append(u8(b"x\xffy\xff\xff" * 300))                                             # bytes 0xFF
    blocks.append(rng.integers(0, 256, size=100000, dtype=np.uint8))                       # random bytes
    half = u8(datagen.wiki_like(30000, seed=9))
    blocks.append(np.concatenate([half, half]))                                            # two identical halves
    total = sum(len(b) for b in blocks)
    blocks.append(rng.integers(97, 123, size=4096 - total % 4096, dtype=np.uint8))         # the next head on a tile boundary
    blocks.append(u8(datagen.wiki_like(65537, seed=4)))
    blocks.append(rng.integers(97, 99, size=333, dtype=np.uint8))
    return blocks


def pack_layout(blocks):
    sizes = [len(b) for b in blocks]
    return sizes, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def test_inverse_parity_with_oracle(ctx, orc):
    blocks = mixed_blocks(orc)
    sizes, off = pack_layout(blocks)
    assert any(o % 4096 == 0 for o in off[1:-1]) and any(o % 4096 for o in off[1:-1])  # heads on and off tile boundaries
    Ls, origins = [], []
    for b in blocks:
        L, o = oracle_bwt(orc, b)
        Ls.append(L)
        origins.append(o)
    assert any(o % S == 0 for o in origins) and any(o % S for o in origins)
    d_bwt = dev(np.concatenate(Ls))
    d_out = torch.empty(int(off[-1]), dtype=torch.uint8, device="cuda")
    ctx.dev_bwt_inverse_packed(d_bwt, sizes, origins, d_out)
    got = d_out.cpu().numpy()
    for i, b in enumerate(blocks):
        assert np.array_equal(got[off[i]:off[i + 1]], b), "block %d (%d bytes, origin %d)" % (i, sizes[i], origins[i])
        one = torch.empty(sizes[i], dtype=torch.uint8, device="cuda")
        ctx.dev_bwt_inverse(dev(Ls[i]), sizes[i], origins[i], one)
        assert np.array_equal(one.cpu().numpy(), got[off[i]:off[i + 1]]), "block %d against dk_dev_bwt_inverse" % i


def fuzz_block(rng, n):
    sigma = int(rng.choice([1, 2, 4, 16, 256]))
    t = rng.integers(0, sigma, size=n, dtype=np.uint8) if sigma < 256 else rng.integers(0, 256, size=n, dtype=np.uint8)
    if rng.integers(0, 5) == 0:  # long repeats, as seeded_inputs injects them
        seg = t[:max(1, n // 7)].copy()
        t = np.concatenate([t, seg, seg, t[:n // 3]])[:n]
    return np.ascontiguousarray(t)


def test_round_trip_with_forward_pack_fuzz(ctx):
    rng = np.random.default_rng(2025)
    for _ in range(50):
        want = int(rng.integers(1, 2001))
        blocks, total = [], 0
        while len(blocks) < want:
            n = int(np.exp(rng.uniform(0, np.log(300000))))
            if total + n > CAP:
                break
            blocks.append(fuzz_block(rng, n))
            total += n
        if not blocks:
            blocks = [fuzz_block(rng, 1)]
        sizes, off = pack_layout(blocks)
        d_in = dev(np.concatenate(blocks))
        d_bwt = torch.empty(int(off[-1]), dtype=torch.uint8, device="cuda")
        origins = ctx.dev_bwt_forward_packed(d_in, sizes, d_bwt)
        d_out = torch.empty_like(d_bwt)
        ctx.dev_bwt_inverse_packed(d_bwt, sizes, origins, d_out)
        assert torch.equal(d_out, d_in), "pack of %d blocks, %d bytes" % (len(blocks), int(off[-1]))


def test_limits_max_blocks_exact_context(ctx):
    rng = np.random.default_rng(8)
    sizes = [int(x) for x in rng.integers(1, 17, size=DK_PACKED_MAX_BLOCKS)]
    data = rng.integers(0, 4, size=sum(sizes), dtype=np.uint8)
    d_in = dev(data)
    d_bwt = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    origins = ctx.dev_bwt_forward_packed(d_in, sizes, d_bwt)
    with dark_amd.Context(len(data)) as small:
        d_out = torch.empty_like(d_bwt)
        small.dev_bwt_inverse_packed(d_bwt, sizes, origins, d_out)
        st = small.stats()
        assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"]
    assert torch.equal(d_out, d_in)


def test_limits_one_max_block():
    n = DK_PACKED_MAX_BLOCK_BYTES
    data = np.frombuffer(datagen.wiki_like(n, seed=5), np.uint8)
    with dark_amd.Context(n) as c:
        d_in = dev(data)
        d_bwt = torch.empty(n, dtype=torch.uint8, device="cuda")
        origin = c.dev_bwt_forward(d_in, n, d_bwt)
        d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
        c.dev_bwt_inverse_packed(d_bwt, [n], [origin], d_out)
        st = c.stats()
        assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"]
    assert torch.equal(d_out, d_in)


def test_errors(ctx):
    d_bwt = dev(u8(b"banana" * 100))
    d_out = torch.empty(600, dtype=torch.uint8, device="cuda")
    bad = [[], [0], [300, 0, 300], [CAP + 1], [DK_PACKED_MAX_BLOCK_BYTES + 1], [1] * (DK_PACKED_MAX_BLOCKS + 1), [CAP // 2 + 1, CAP // 2 + 1]]
    for sizes in bad:
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.dev_bwt_inverse_packed(d_bwt, sizes, [0] * len(sizes), d_out)
        assert e.value.code == DK_E_ARG, sizes
    for sizes, origins in (([600], [600]), ([300, 300], [0, 300]), ([1], [1])):
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.dev_bwt_inverse_packed(d_bwt, sizes, origins, d_out)
        assert e.value.code == DK_E_ARG, (sizes, origins)
    lib = ctx._lib
    ns = (C.c_size_t * 1)(600)
    org = np.zeros(1, np.uint32)
    assert lib.dk_dev_bwt_inverse_packed(ctx._h, None, 1, ns, C.c_void_p(org.ctypes.data), C.c_void_p(d_out.data_ptr())) == DK_E_ARG
    assert lib.dk_dev_bwt_inverse_packed(ctx._h, C.c_void_p(d_bwt.data_ptr()), 1, ns, None, C.c_void_p(d_out.data_ptr())) == DK_E_ARG
    assert lib.dk_dev_bwt_inverse_packed(ctx._h, C.c_void_p(d_bwt.data_ptr()), 1, None, C.c_void_p(org.ctypes.data), None) == DK_E_ARG


def test_corrupt_block_stays_inside(ctx, orc):
    """two victims, one pack each: two random unequal bytes of L swapped (a long leftover cycle, which holds a splitter) and a class-e input
    of tests/ibwt_model.py (adjacent bytes swapped: a short leftover cycle without one).  The model says which candidates are no text, and
    the single-block inverse must reject the first such candidate; only swaps that leave a text are passed over."""
    import ibwt_model as M
    rng = np.random.default_rng(21)
    blocks = [u8(datagen.wiki_like(int(n), seed=int(n))) for n in (5000, 70000, 300, 9000, 40000)]
    Ls, origins = zip(*[oracle_bwt(orc, b) for b in blocks])
    origins = list(origins)
    L = Ls[3]
    for _ in range(500):
        i, j = (int(x) for x in rng.integers(0, len(L), size=2))
        if L[i] == L[j]:
            continue
        cand = L.copy()
        cand[i], cand[j] = cand[j], cand[i]
        if M.invert(cand, origins[3]).text is None:
            break
    else:
        raise AssertionError("every swap left a text")
    short = M.adjacent_swaps(Ls[1], origins[1], orc.sa_sais(blocks[1]))[0]
    assert short.verdict.text is None and not short.verdict.cycle_has_splitter and short.origin == origins[1]
    sizes, off = pack_layout(blocks)
    total = int(off[-1])
    guard = 4096
    for victim, bad in ((3, cand), (1, short.L)):
        one = torch.empty(len(bad), dtype=torch.uint8, device="cuda")
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.dev_bwt_inverse(dev(bad), len(bad), origins[victim], one)
        assert e.value.code == DK_E_STREAM
        damaged = [L.copy() for L in Ls]
        damaged[victim] = bad
        buf = torch.full((total + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.dev_bwt_inverse_packed(dev(np.concatenate(damaged)), sizes, origins, buf[guard:guard + total])
        assert e.value.code == DK_E_STREAM
        assert "block %d " % victim in str(e.value), str(e.value)
        got = buf.cpu().numpy()
        assert (got == 0xA5).all(), "a rejected pack wrote to d_out or to the guard bytes around it"
        # the same context then inverts a correct pack
        d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
        ctx.dev_bwt_inverse_packed(dev(np.concatenate(Ls)), sizes, origins, d_out)
        assert np.array_equal(d_out.cpu().numpy(), np.concatenate(blocks))


def decode_blocks():
    rng = np.random.default_rng(13)
    blocks = [rng.integers(97, 100, size=k, dtype=np.uint8) for k in (1, 2, 3, 17, 4095, 4096, 4097)]
    blocks.append(u8(datagen.wiki_like(65537, seed=4)))
    blocks.append(u8(datagen.english_like(200000)))
    blocks.append(np.full(777, 0x41, np.uint8))                                            # single symbol
    blocks.append(u8(b"ab" * 3000))
    blocks.append(rng.integers(0, 255, size=100000, dtype=np.uint8))                       # random bytes (no 0xFF: decodable)
    half = u8(datagen.wiki_like(30000, seed=9))
    blocks.append(np.concatenate([half, half]))
    return blocks


@pytest.mark.parametrize("model", ["dark", "exp", "ybs", "simple"])
def test_packed_decode_models(ctx, model):
    blocks = decode_blocks()
    sizes, off = pack_layout(blocks)
    data = np.concatenate(blocks)
    streams, _ = ctx.dev_packed_encode(model, dev(data), sizes, host_threads=4)
    d_out = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    ctx.dev_packed_decode(model, streams, sizes, d_out, host_threads=4)
    got = d_out.cpu().numpy()
    assert np.array_equal(got, data)
    outs = [torch.empty(n, dtype=torch.uint8, device="cuda") for n in sizes]
    ctx.dev_batch_decode(model, streams, sizes, outs, host_threads=4)
    for i, o in enumerate(outs):
        assert np.array_equal(o.cpu().numpy(), got[off[i]:off[i + 1]]), "%s block %d against dk_dev_batch_decode" % (model, i)


def test_packed_decode_errors(ctx):
    blocks = decode_blocks()
    sizes, _ = pack_layout(blocks)
    data = np.concatenate(blocks)
    streams, _ = ctx.dev_packed_encode("exp", dev(data), sizes, host_threads=4)
    streams = [bytes(s) for s in streams]
    d_out = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    with pytest.raises(dark_amd.DarkError) as e:
        ctx.dev_packed_decode("rawdc", streams, sizes, d_out)
    assert e.value.code == DK_E_MODEL
    with pytest.raises(dark_amd.DarkError) as e:
        ctx.dev_packed_decode(99, streams, sizes, d_out)
    assert e.value.code == DK_E_MODEL
    victim = 8  # english_like, 200 000 bytes
    cut = list(streams)
    cut[victim] = cut[victim][:len(cut[victim]) // 2]
    with pytest.raises(dark_amd.DarkError) as e:
        ctx.dev_packed_decode("exp", cut, sizes, d_out, host_threads=4)
    assert e.value.code == DK_E_STREAM
    assert "block %d " % victim in str(e.value), str(e.value)
    with pytest.raises(dark_amd.DarkError) as e:
        ctx.dev_packed_decode("exp", streams, [0] + sizes[1:], d_out)
    assert e.value.code == DK_E_ARG
    ctx.dev_packed_decode("exp", streams, sizes, d_out, host_threads=4)
    assert np.array_equal(d_out.cpu().numpy(), data)


def cli_round_trip(tmp_path, data, block_size, model="exp"):
    from dark_amd import cli
    src = tmp_path / "in.bin"
    data.tofile(src)
    archive = cli.encode_file(str(src), model, block_size, host_threads=4)
    os.remove(str(src))
    plain = cli.decode_file(archive, model, host_threads=4)
    shutil.move(plain, str(tmp_path / "plain.orig"))
    packed = cli.decode_file(archive, model, host_threads=4, packed=True)
    got = open(packed, "rb").read()
    assert got == open(tmp_path / "plain.orig", "rb").read()
    assert got == data.tobytes()


@pytest.mark.parametrize("block_size", [65536, 1000000])
def test_cli_packed_decode_identical(tmp_path, monkeypatch, block_size):
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(3)
    data = np.concatenate([datagen.wiki_like(2 << 20, seed=21), datagen.acgt(1 << 20), datagen.english_like(900000),
                           rng.integers(0, 255, size=300017, dtype=np.uint8)])  # the last block is shorter
    assert len(data) % block_size
    cli_round_trip(tmp_path, data, block_size)


def test_cli_packed_decode_large_records(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    bs = (16 << 20) + 4096  # above DK_PACKED_MAX_BLOCK_BYTES: these records take the batched path, the short last one a pack
    rng = np.random.default_rng(4)
    data = np.concatenate([datagen.wiki_like(2 * bs, seed=7), rng.integers(0, 255, size=70000, dtype=np.uint8)])
    cli_round_trip(tmp_path, data, bs, model="dark")  # (exp codes blocks of at most 16 MiB)


def test_cli_packed_decode_refuses_gpus(tmp_path, monkeypatch):
    from dark_amd import cli
    monkeypatch.chdir(tmp_path)
    data = np.frombuffer(datagen.wiki_like(300000, seed=1), np.uint8)
    src = tmp_path / "in.bin"
    data.tofile(src)
    archive = cli.encode_file(str(src), "exp", 65536, host_threads=2)
    with pytest.raises(SystemExit):
        cli.decode_file(archive, "exp", gpus=2, packed=True)
    with pytest.raises(SystemExit):
        cli.main(["--packed", "--gpus", "2", archive])
