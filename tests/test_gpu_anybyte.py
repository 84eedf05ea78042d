"""DK_MODEL_ANYBYTE through every entry point that takes a model id (include/dark_amd.h): the stream is
[u32 LE init[255]][the stream of the same call without the flag], and with it blocks that hold byte 0xFF come back from every decoder."""
import os
import struct

import numpy as np
import pytest
import torch

import dark_amd
from dark_amd import _lib, datagen, entropy
from dark_amd._lib import DK_E_STREAM

pytestmark = pytest.mark.gpu
MODELS = ("dark", "exp", "ybs", "simple")
GUARD = 64
CAP = 3 << 20


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()


def u8(b):
    return np.frombuffer(b, np.uint8)


class Guarded:
    """a device output of n bytes with GUARD bytes of 0xA5 on both sides"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.out = self.buf[GUARD:GUARD + n]

    def check(self):
        got = self.buf.cpu().numpy()
        assert (got[:GUARD] == 0xA5).all() and (got[GUARD + self.n:] == 0xA5).all(), "guard bytes around a device output were written"
        return got[GUARD:GUARD + self.n]

    def untouched(self):
        return bool((self.buf.cpu().numpy() == 0xA5).all())


def blocks():
    rng = np.random.default_rng(41)
    return [np.full(50, 255, np.uint8), np.array([254, 255] * 20, np.uint8), np.arange(256, dtype=np.uint8),
            np.arange(255, -1, -1, dtype=np.uint8), u8(b"x\xffy\xff\xff" * 300), np.array([0] * 999 + [255], np.uint8),
            np.array([255] + [0] * 999, np.uint8), rng.integers(0, 256, size=70_000, dtype=np.uint8), datagen.wiki_like(20_000, seed=7),
            np.array([255], np.uint8), rng.integers(0, 256, size=4097, dtype=np.uint8)]


XFFY, RANDOM = 4, 7  # indices into blocks()


@pytest.fixture(scope="module")
def ref(orc):
    """per block: text, the oracle's init[255] and its stream for every model -- computed once"""
    out = []
    for t in blocks():
        t = np.ascontiguousarray(t, dtype=np.uint8)
        bwt, origin = orc.bwt_forward(t, orc.sa_naive(t) if len(t) < 64 else None)
        init = orc.dc_encode(bwt)["init"]
        out.append(dict(text=t, n=len(t), first_ff=int(init[255]), streams={m: orc.block_dc_encode_bwt(m, bwt, origin) for m in MODELS}))
    assert out[8]["first_ff"] == out[8]["n"] and sum(r["first_ff"] < r["n"] for r in out) == 10
    return out


def check_stream(r, m, flagged, plain, where):
    flagged, plain = bytes(flagged), bytes(plain)
    assert flagged[4:] == plain, "%s %s n=%d: bytes after the prefix differ from the call without the flag" % (where, m, r["n"])
    assert plain == r["streams"][m], "%s %s n=%d: not the oracle's stream" % (where, m, r["n"])
    assert flagged[:4] == struct.pack("<I", r["first_ff"]), "%s %s n=%d: prefix" % (where, m, r["n"])


@pytest.mark.parametrize("m", MODELS)
def test_block_entry_points(ctx, ref, m):
    for r in ref:
        t, n = r["text"], r["n"]
        plain = ctx.block_encode(m, t)
        flags0 = ctx.last_block_flags()
        s = ctx.block_encode(m + "+ff", t)
        assert ctx.last_block_flags() == flags0
        assert bool(flags0 & _lib.DK_FLAG_HAS_FF) == (r["first_ff"] < n) and bool(flags0 & _lib.DK_FLAG_SINGLE_SYMBOL) == (len(set(t.tolist())) == 1)
        check_stream(r, m, s, plain, "block_encode")
        assert ctx.block_decode(m + "+ff", s + b"\x5a" * 9, n) == t.tobytes()
        assert ctx.last_consumed() == len(s)
        d_in = dev(t)
        plain = bytes(ctx.dev_block_encode(m, d_in, n))
        flags0 = ctx.last_block_flags()
        s = bytes(ctx.dev_block_encode(m + "+ff", d_in, n))
        assert ctx.last_block_flags() == flags0
        check_stream(r, m, s, plain, "dev_block_encode")
        g = Guarded(n)
        ctx.dev_block_decode(m + "+ff", s, n, g.out)
        assert ctx.last_consumed() == len(s)
        assert np.array_equal(g.check(), t), "dev_block_decode %s n=%d" % (m, n)


@pytest.mark.parametrize("m", MODELS)
def test_batch_entry_points(ctx, ref, m):
    texts = [r["text"] for r in ref]
    sizes = [r["n"] for r in ref]
    d_blocks = [dev(t) for t in texts]
    plain = ctx.dev_batch_encode(m, d_blocks, sizes, host_threads=3)
    flagged = ctx.dev_batch_encode(m + "+ff", d_blocks, sizes, host_threads=3)
    for r, s, p in zip(ref, flagged, plain):
        check_stream(r, m, s, p, "dev_batch_encode")
    gs = [Guarded(n) for n in sizes]
    ctx.dev_batch_decode(m + "+ff", flagged, sizes, [g.out for g in gs], host_threads=3)
    for g, t in zip(gs, texts):
        assert np.array_equal(g.check(), t)
    with ctx.batch_begin(m + "+ff", 2) as b:
        for d, n in zip(d_blocks, sizes):
            b.push(d, n)
        pushed = b.finish()
    for s, f in zip(pushed, flagged):
        assert bytes(s) == bytes(f), "Batch.push"
    multi = dark_amd.multi_block_encode(m + "+ff", texts, devices=[0, 0], host_threads_per_gpu=2)
    back = dark_amd.multi_block_decode(m + "+ff", multi, sizes, devices=[0, 0], host_threads_per_gpu=2)
    for r, s, f, t, b2 in zip(ref, multi, flagged, texts, back):
        assert s == bytes(f), "multi_block_encode %s n=%d" % (m, r["n"])
        assert bytes(b2) == t.tobytes(), "multi_block_decode %s n=%d" % (m, r["n"])


@pytest.mark.parametrize("m", MODELS)
def test_packed_entry_points(ctx, ref, m):
    texts = [r["text"] for r in ref]
    sizes = [r["n"] for r in ref]
    d_in = dev(np.concatenate(texts))
    plain, flags0 = ctx.dev_packed_encode(m, d_in, sizes, host_threads=3)
    flagged, flags = ctx.dev_packed_encode(m + "+ff", d_in, sizes, host_threads=3)
    assert flags == flags0
    for r, s, p, fl in zip(ref, flagged, plain, flags):
        check_stream(r, m, s, p, "dev_packed_encode")
        assert bool(fl & _lib.DK_FLAG_HAS_FF) == (r["first_ff"] < r["n"])
    with ctx.batch_begin(m + "+ff", 2) as b:
        assert b.push_packed(d_in, sizes) == flags
        pushed = b.finish()
    for s, f in zip(pushed, flagged):
        assert bytes(s) == bytes(f), "Batch.push_packed"
    g = Guarded(sum(sizes))
    ctx.dev_packed_decode(m + "+ff", flagged, sizes, g.out, host_threads=3)
    assert np.array_equal(g.check(), np.concatenate(texts))


def test_flag_where_it_does_not_belong(ctx, ref):
    t = ref[XFFY]["text"]
    for bad in (_lib.MODEL_IDS["rawdc"] | 0x100, 5 | 0x100, 0x200):
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.block_encode(bad, t)
        assert e.value.code == _lib.DK_E_MODEL
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.block_decode(bad, b"\0" * 64, len(t))
        assert e.value.code == _lib.DK_E_MODEL
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.batch_begin(bad, 1)
        assert e.value.code == _lib.DK_E_MODEL
        with pytest.raises(dark_amd.DarkError) as e:
            ctx.dev_packed_decode(bad, [b"\0" * 64], [len(t)], torch.empty(len(t), dtype=torch.uint8, device="cuda"))
        assert e.value.code == _lib.DK_E_MODEL
    assert ctx.block_decode("exp+ff", ctx.block_encode("exp+ff", t), len(t)) == t.tobytes()


def test_large_single_block_every_thread_form(orc):
    """2 200 000 random bytes: at least 2^21 distances, so dev_block_encode hands the stream to the host coder while it still arrives"""
    n = 2_200_000
    t = np.random.default_rng(43).integers(0, 256, size=n, dtype=np.uint8)
    got = []
    with dark_amd.Context(n) as c:
        d_in = dev(t)
        try:
            for mode in (1, 2, 4, 5):
                entropy.set_threads(mode)
                got.append(bytes(c.dev_block_encode("dark+ff", d_in, n)))
                assert c.stats()["dc_runs"] >= 1 << 21
                assert c.last_block_flags() & _lib.DK_FLAG_HAS_FF
        finally:
            entropy.set_threads(0)
        plain = bytes(c.dev_block_encode("dark", d_in, n))
        for mode, s in zip((1, 2, 4, 5), got):
            assert s == got[0], "thread form %d" % mode
        assert got[0][4:] == plain
        bwt, _ = orc.bwt_forward(t)
        assert got[0][:4] == struct.pack("<I", int(np.flatnonzero(bwt == 255)[0]))
        g = Guarded(n)
        c.dev_block_decode("dark+ff", got[0], n, g.out)
        assert c.last_consumed() == len(got[0])
        assert np.array_equal(g.check(), t)


@pytest.mark.parametrize("victim", [XFFY, RANDOM])
def test_corrupt_prefix(ctx, ref, victim):
    """a damaged prefix is a corrupt input with a defined answer: DK_OK (some other block) or DK_E_STREAM, always DK_E_STREAM above n"""
    m = "exp"
    r = ref[victim]
    n, first_ff = r["n"], r["first_ff"]
    assert first_ff < n
    good = {i: struct.pack("<I", ref[i]["first_ff"]) + ref[i]["streams"][m] for i in (1, victim, 8)}
    pack = [1, victim, 8]  # the damaged block in the middle
    sizes = [ref[i]["n"] for i in pack]
    texts = np.concatenate([ref[i]["text"] for i in pack])
    for prefix in (0, (first_ff - 1) & 0xFFFFFFFF, first_ff + 1, n, n + 1, 0xFFFFFFFF):  # (first_ff may be 0: one below wraps)
        bad = struct.pack("<I", prefix) + r["streams"][m]
        must_fail = prefix > n
        # single block
        g = Guarded(n)
        try:
            ctx.dev_block_decode(m + "+ff", bad, n, g.out)
            code = 0
        except dark_amd.DarkError as e:
            code = e.code
        assert code in (0, DK_E_STREAM) and (code == DK_E_STREAM or not must_fail), (prefix, code)
        g.check()
        # batch
        gs = [Guarded(k) for k in sizes]
        try:
            ctx.dev_batch_decode(m + "+ff", [good[1], bad, good[8]], sizes, [x.out for x in gs], host_threads=2)
            code = 0
        except dark_amd.DarkError as e:
            code = e.code
        assert code in (0, DK_E_STREAM) and (code == DK_E_STREAM or not must_fail), (prefix, code)
        for x in gs:
            x.check()
        # pack
        g = Guarded(sum(sizes))
        try:
            ctx.dev_packed_decode(m + "+ff", [good[1], bad, good[8]], sizes, g.out, host_threads=2)
            code = 0
        except dark_amd.DarkError as e:
            code = e.code
            assert "block 1 " in str(e), str(e)
            assert g.untouched(), "a rejected pack wrote to d_out"
        assert code in (0, DK_E_STREAM) and (code == DK_E_STREAM or not must_fail), (prefix, code)
        g.check()
        # the context then decodes good blocks
        g = Guarded(sum(sizes))
        ctx.dev_packed_decode(m + "+ff", [good[i] for i in pack], sizes, g.out, host_threads=2)
        assert np.array_equal(g.check(), texts)
    g = Guarded(n)
    ctx.dev_block_decode(m + "+ff", good[victim], n, g.out)
    assert np.array_equal(g.check(), r["text"])


# ---- the command line -------------------------------------------------------------------------------------------------------------------
BLOCK = 65536
KINDS = {"single": dict(block_size=0), "blocks": dict(block_size=BLOCK), "packed": dict(block_size=BLOCK, packed=True),
         "gpus": dict(block_size=BLOCK, gpus=2, devices="0,0")}


def cli_input():
    rng = np.random.default_rng(5)
    data = np.concatenate([datagen.wiki_like(120_000, seed=3), rng.integers(0, 256, size=100_000, dtype=np.uint8), np.full(80_000, 255, np.uint8)])
    assert len(data) == 300_000 and not (data[:BLOCK] == 255).any()
    return data


@pytest.fixture(scope="module")
def archives(tmp_path_factory):
    """the 300 000-byte file encoded four ways with --any-byte, each once: kind -> archive bytes; the archives stay in `dir`"""
    from dark_amd import cli
    d = tmp_path_factory.mktemp("anybyte_cli")
    data = cli_input()
    data.tofile(d / "in.bin")
    here = os.getcwd()
    os.chdir(d)
    try:
        out = {}
        for kind, kw in KINDS.items():
            made = cli.encode_file(str(d / "in.bin"), "exp", host_threads=3, any_byte=True, **kw)
            os.replace(made, kind + ".dark")
            out[kind] = open(kind + ".dark", "rb").read()
    finally:
        os.chdir(here)
    return dict(dir=d, data=data, blobs=out)


def test_cli_archives(archives):
    from dark_amd import cli
    data, blobs = archives["data"], archives["blobs"]
    assert blobs["blocks"] == blobs["packed"] == blobs["gpus"]
    offsets, end = cli.read_footer(str(archives["dir"] / "blocks.dark"))
    assert len(offsets) == -(-len(data) // BLOCK)
    seen = set()
    for k, off in enumerate(offsets):  # bit 31 exactly on the records of blocks that contain 0xFF
        blk = data[k * BLOCK:(k + 1) * BLOCK]
        (word,) = struct.unpack("<I", blobs["blocks"][off:off + 4])
        has_ff = bool((blk == 255).any())
        assert word == len(blk) | (0x80000000 if has_ff else 0), k
        seen.add(has_ff)
    assert seen == {False, True}
    assert struct.unpack("<I", blobs["single"][:4])[0] == len(data) | 0x80000000 and cli.read_footer(str(archives["dir"] / "single.dark")) is None


@pytest.mark.parametrize("how", ["plain", "packed", "gpus"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_cli_decode(archives, monkeypatch, kind, how):
    from dark_amd import cli
    monkeypatch.chdir(archives["dir"])
    kw = dict(plain={}, packed=dict(packed=True), gpus=dict(gpus=2, devices="0,0"))[how]
    out = cli.decode_file(kind + ".dark", "exp", host_threads=3, **kw)
    assert out == kind + ".orig"
    assert open(out, "rb").read() == archives["data"].tobytes()
    os.remove(out)


def test_cli_text_file_gives_the_same_archive(tmp_path, monkeypatch):
    from dark_amd import cli
    monkeypatch.chdir(tmp_path)
    data = datagen.wiki_like(200_000, seed=8)
    assert not (data == 255).any()
    data.tofile(tmp_path / "text.txt")
    for kw in (dict(block_size=0), dict(block_size=BLOCK), dict(block_size=BLOCK, packed=True)):
        without = open(cli.encode_file(str(tmp_path / "text.txt"), "dark", host_threads=2, **kw), "rb").read()
        with_option = open(cli.encode_file(str(tmp_path / "text.txt"), "dark", host_threads=2, any_byte=True, **kw), "rb").read()
        assert with_option == without, kw
    assert open(cli.decode_file("text.dark", "dark", host_threads=2), "rb").read() == data.tobytes()


def test_cli_any_byte_and_force_exclude_each_other(tmp_path, monkeypatch):
    from dark_amd import cli
    monkeypatch.chdir(tmp_path)
    (tmp_path / "a.bin").write_bytes(b"x\xffy" * 100)
    (tmp_path / "a.dark").write_bytes(b"an archive that was here before")
    with pytest.raises(SystemExit):
        cli.main(["--any-byte", "--force", str(tmp_path / "a.bin")])
    with pytest.raises(SystemExit):
        cli.main(["--any-byte", "--force", "-b", "100", str(tmp_path / "a.bin")])
    for model in ("raw", "rawdc"):
        with pytest.raises(SystemExit):
            cli.main(["--any-byte", "-m", model, str(tmp_path / "a.bin")])
    assert (tmp_path / "a.dark").read_bytes() == b"an archive that was here before"
    assert sorted(os.listdir(tmp_path)) == ["a.bin", "a.dark"]  # no temporary file, no dump
    with pytest.raises(SystemExit):  # without the option: refused as ever
        cli.main([str(tmp_path / "a.bin")])
    cli.main(["--any-byte", "-m", "bbb", str(tmp_path / "a.bin")])  # a no-op for block::raw, which carries every byte value
    bbb = (tmp_path / "a.dark").read_bytes()
    cli.main(["-m", "bbb", str(tmp_path / "a.bin")])
    assert (tmp_path / "a.dark").read_bytes() == bbb
    cli.main(["--any-byte", str(tmp_path / "a.bin")])
    cli.main(["a.dark"])
    assert (tmp_path / "a.orig").read_bytes() == b"x\xffy" * 100
