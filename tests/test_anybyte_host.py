"""DK_MODEL_ANYBYTE on the host (no GPU): the stream is [u32 LE init[255]][the reference stream, unchanged], and with those four bytes every
block decodes -- blocks that hold byte 0xFF, which the reference's header cannot carry (src/block/dc.rs:57,60,73,127), included."""
import ctypes as C
import struct

import numpy as np
import pytest

import dark_amd
from dark_amd import _lib, datagen, model
from conftest import seeded_inputs

MODELS = ("dark", "exp", "ybs", "simple")
FLAG = 0x100


def fixed_blocks():
    rng = np.random.default_rng(41)
    return [np.full(50, 255, np.uint8), np.array([254, 255] * 20, np.uint8), np.arange(256, dtype=np.uint8),
            np.arange(255, -1, -1, dtype=np.uint8), np.frombuffer(b"x\xffy\xff\xff" * 300, np.uint8),
            np.array([0] * 999 + [255], np.uint8), np.array([255] + [0] * 999, np.uint8),
            rng.integers(0, 256, size=70_000, dtype=np.uint8), datagen.wiki_like(20_000, seed=7)]


@pytest.fixture(scope="module")
def cases(orc):
    """(text, L, origin, the oracle's DC arrays) of every input, computed once"""
    out = []
    for t in seeded_inputs(seed=23, count=40) + fixed_blocks():
        t = np.ascontiguousarray(t, dtype=np.uint8)
        bwt, origin = orc.bwt_forward(t, sa=orc.sa_naive(t) if len(t) == 1 else None)  # (the oracle's SA-IS takes no one-byte text)
        out.append((t, bwt, origin, orc.dc_encode(bwt)))
    assert not (out[-1][0] == 255).any() and sum(bool((c[0] == 255).any()) for c in out) >= 8
    return out


def test_model_names():
    for m in MODELS:
        assert _lib.MODEL_IDS[m + "+ff"] == _lib.MODEL_IDS[m] | FLAG
    assert "rawdc+ff" not in _lib.MODEL_IDS
    assert _lib.DK_MODEL_ANYBYTE == FLAG


@pytest.mark.parametrize("m", MODELS)
def test_prefix_plus_reference_stream_and_back(orc, cases, m):
    for t, bwt, origin, dc in cases:
        n = len(t)
        s = model.stream_encode(m + "+ff", n, dc["init"], dc["d"], dc["sym"], origin)
        assert s[4:] == orc.block_dc_encode_bwt(m, bwt, origin), n
        assert s[4:] == model.stream_encode(m, n, dc["init"], dc["d"], dc["sym"], origin)
        first_ff = int(dc["init"][255])
        assert first_ff == (int(np.flatnonzero(bwt == 255)[0]) if (bwt == 255).any() else n)
        assert s[:4] == struct.pack("<I", first_ff)
        b2, o2, single, used = model.stream_decode(m + "+ff", s + b"\x5a" * 9, n, with_consumed=True)  # trailing bytes = the next record
        assert used == len(s), (m, n, used, len(s))
        assert (b2 == bwt).all() and o2 == origin, (m, n)
        assert single == (len(set(t.tolist())) == 1)


def _gated(mid, n, init, dist, sym, origin, threads):
    lib = _lib.load()
    out = np.empty(8 * len(dist) + 8192 + 4, dtype=np.uint8)
    ln = C.c_size_t(0)
    ready = C.c_size_t(len(dist))  # the whole stream is there
    rc = lib.dk_dbg_stream_encode_gated(mid, n, init.ctypes.data, dist.ctypes.data, sym.ctypes.data, len(dist), origin, out.ctypes.data, len(out),
                                        C.byref(ln), C.addressof(ready), 5000, threads)
    return rc, out[:ln.value].tobytes()


def test_every_thread_form_writes_the_same_bytes(orc):
    """a block large enough for the pipelined forms of the host coder (at least 2^21 distances): 1, 2, 4 and 5 threads"""
    t = np.random.default_rng(43).integers(0, 256, size=2_200_000, dtype=np.uint8)
    bwt, origin = orc.bwt_forward(t)
    dc = orc.dc_encode(bwt)
    n, m = len(t), len(dc["d"])
    assert m >= 1 << 21
    init = np.ascontiguousarray(dc["init"], dtype=np.uint32)
    dist = np.ascontiguousarray(dc["d"], dtype=np.uint32)
    sym = np.ascontiguousarray(dc["sym"], dtype=np.uint8)
    assert init[255] < n
    rc, plain = _gated(_lib.MODEL_IDS["dark"], n, init, dist, sym, origin, 1)
    assert rc == 0
    want = struct.pack("<I", int(init[255])) + plain
    for threads in (1, 2, 4, 5):
        rc, got = _gated(_lib.MODEL_IDS["dark+ff"], n, init, dist, sym, origin, threads)
        assert rc == 0 and got == want, threads
    b2, o2, single, used = model.stream_decode("dark+ff", want, n, with_consumed=True)
    assert (b2 == bwt).all() and o2 == origin and not single and used == len(want)


def test_errors(orc, cases):
    t, bwt, origin, dc = next(c for c in cases if len(c[0]) == 1500 and c[0][0] == ord("x"))
    n = len(t)
    ends = np.flatnonzero(dc["sparse"] != n).astype(np.uint32)
    with pytest.raises(dark_amd.DarkError) as e:  # rawdc writes records, not a header the prefix could complete
        model.stream_encode(_lib.MODEL_IDS["rawdc"] | FLAG, n, dc["init"], dc["d"], dc["sym"], origin, rank=dc["rank"], run_end=ends)
    assert e.value.code == _lib.DK_E_MODEL
    for bad in (5 | FLAG, 0x200, 0x300, FLAG | 0x1000):
        with pytest.raises(dark_amd.DarkError) as e:
            model.stream_encode(bad, n, dc["init"], dc["d"], dc["sym"], origin)
        assert e.value.code == _lib.DK_E_MODEL
        with pytest.raises(dark_amd.DarkError) as e:
            model.stream_decode(bad, b"\0" * 40, n)
        assert e.value.code == _lib.DK_E_MODEL
    with pytest.raises(dark_amd.DarkError) as e:  # model level: no header there
        model.encode("dark+ff", [1, 2, 3], [1, 2, 3])
    assert e.value.code == _lib.DK_E_MODEL
    with pytest.raises(dark_amd.DarkError) as e:
        model.decode("dark+ff", model.encode("dark", [1, 2, 3], [1, 2, 3]), [1, 2, 3])
    assert e.value.code == _lib.DK_E_MODEL
    for m in MODELS:
        s = model.stream_encode(m + "+ff", n, dc["init"], dc["d"], dc["sym"], origin)
        for k in range(4):  # shorter than the prefix
            with pytest.raises(dark_amd.DarkError) as e:
                model.stream_decode(m + "+ff", s[:k] if k else np.zeros(0, np.uint8), n)
            assert e.value.code == _lib.DK_E_STREAM
        for prefix in (n + 1, n + 2, 0x7FFFFFFF, 0xFFFFFFFF):  # a first position past the end of the block
            with pytest.raises(dark_amd.DarkError) as e:
                model.stream_decode(m + "+ff", struct.pack("<I", prefix) + s[4:], n)
            assert e.value.code == _lib.DK_E_STREAM
        # "absent" where the block does hold 0xFF: the stream's distances of that symbol no longer fit -> an error or other bytes, never L
        try:
            b2, _, _ = model.stream_decode(m + "+ff", struct.pack("<I", n) + s[4:], n)
            assert not (b2 == bwt).all()
        except dark_amd.DarkError as e2:
            assert e2.code == _lib.DK_E_STREAM
        # without the flag the same bytes are what they always were: a stream that is lost
        try:
            b2, _, _ = model.stream_decode(m, s[4:], n)
            assert not (b2 == bwt).all()
        except dark_amd.DarkError as e2:
            assert e2.code == _lib.DK_E_STREAM


def test_output_capacity_counts_the_prefix(cases):
    """out_cap covers prefix + stream: a call with the flag and out_cap answers what the call without the flag answers to out_cap - 4"""
    t, bwt, origin, dc = cases[4]  # banana
    lib = _lib.load()
    init = np.ascontiguousarray(dc["init"], dtype=np.uint32)
    dist = np.ascontiguousarray(dc["d"], dtype=np.uint32)
    sym = np.ascontiguousarray(dc["sym"], dtype=np.uint8)
    want = model.stream_encode("exp+ff", len(t), init, dist, sym, origin)

    def call(mid, cap):
        out = np.full(len(want) + 64, 0xA5, dtype=np.uint8)
        ln = C.c_size_t(0)
        rc = lib.dk_stream_encode(mid, len(t), init.ctypes.data, dist.ctypes.data, sym.ctypes.data, None, None, len(dist), origin,
                                  out.ctypes.data, cap, C.byref(ln))
        assert (out[cap:] == 0xA5).all(), cap  # nothing past out_cap
        return rc, out[:ln.value].tobytes()

    for cap in range(0, len(want) + 32):
        rc, got = call(_lib.MODEL_IDS["exp+ff"], cap)
        if cap < 4:
            assert rc == _lib.DK_E_CAPACITY
            continue
        rc0, got0 = call(_lib.MODEL_IDS["exp"], cap - 4)
        assert rc == rc0 and rc in (0, _lib.DK_E_CAPACITY), cap
        if rc == 0:
            assert got == want and got[4:] == got0
    assert call(_lib.MODEL_IDS["exp+ff"], len(want) + 31)[0] == 0


def test_cli_record_forms(cases):
    """the container of --any-byte without a GPU: plain records for blocks without 0xFF (byte for byte what is written without the option),
    bit 31 of n and the prefix for the others; a batch with one flagged record runs with the flag, plain records prefixed with n"""
    from dark_amd import cli
    picked = [c for c in cases if len(c[0]) > 1][:12] + cases[-3:]
    ns, flagged, streams, want = [], [], [], []
    for t, bwt, origin, dc in picked:
        n = len(t)
        s = np.frombuffer(model.stream_encode("ybs+ff", n, dc["init"], dc["d"], dc["sym"], origin), np.uint8)
        head, body = cli._record_head(n, s, True)
        plain_head, plain_body = cli._record_head(n, np.frombuffer(model.stream_encode("ybs", n, dc["init"], dc["d"], dc["sym"], origin), np.uint8), False)
        has_ff = bool((t == 255).any())
        if has_ff:
            assert head == struct.pack("<I", n | 0x80000000) and bytes(body) == s.tobytes()
        else:
            assert head == plain_head == struct.pack("<I", n) and bytes(body) == bytes(plain_body)
        size, fl = cli._split_n(struct.unpack("<I", head)[0])
        assert (size, fl) == (n, has_ff)
        ns.append(size)
        flagged.append(fl)
        streams.append(np.frombuffer(bytes(body), np.uint8))
        want.append(bwt)
    assert any(flagged) and not all(flagged)
    call_model, uniform = cli._uniform_streams("ybs", ns, flagged, streams)
    assert call_model == "ybs+ff"
    for n, s, bwt in zip(ns, uniform, want):
        b2, _, _, used = model.stream_decode(call_model, s, n, with_consumed=True)
        assert (b2 == bwt).all() and used == len(s)
    none = [i for i, fl in enumerate(flagged) if not fl]
    call_model, same = cli._uniform_streams("ybs", [ns[i] for i in none], [False] * len(none), [streams[i] for i in none])
    assert call_model == "ybs" and all(a is b for a, b in zip(same, [streams[i] for i in none]))
