"""Decoder contexts (include/dark_amd.h dk_ctx_create_decoder): a context whose workspace holds the inverse path only.  Every decoder context
here is sized EXACTLY to its input -- max_n = the block (or the pack's sum), max_blocks = the pack's count -- so a term missing from
decoder_workspace_bytes (csrc/abi.cpp) shows as DK_E_NOMEM.  L, origins and streams come from a full context (or tests/golden), the texts
are the expected values; where an input is no BWT the expected answer is the full context's, labelled by tests/ibwt_model.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dark_amd
import ibwt_model as M
from conftest import GOLDEN, ROOT
from dark_amd import block, cli, datagen
from dark_amd import context as context_module
from dark_amd._lib import DK_E_ARG, DK_E_STREAM, DK_PACKED_MAX_BLOCKS
from dark_amd.context import _ptr, model_id, workspace_bytes

pytestmark = pytest.mark.gpu
FULL_CAP = 2 << 20
GUARD, FILL = 4096, 0xA5
MODELS = ("dark", "exp", "ybs", "simple")
SIZES = [1, 2, 63, 64, 65, 65535, 65536, 65537, 70000, (1 << 20) + 1]  # around the grid, around the S = 8 / S = 64 switch, many tiles
RECORD_OFF = os.environ.get("DK_IBWT_RECORD") == "0"  # the run test_record_off_fits_too starts: tuning library, no walk records


@pytest.fixture(scope="module")
def full():
    c = dark_amd.Context(FULL_CAP)
    yield c
    c.close()


def decoder(n, max_blocks=1):
    return dark_amd.Context(n, purpose="decoder", max_blocks=max_blocks)


def check_workspace(ctx, n, max_blocks=1):
    st = ctx.stats()
    assert ctx.purpose == "decoder" and ctx._lib.dk_ctx_purpose(ctx._h) == 1 and ctx.capacity() == n
    assert st["ws_size_bytes"] == workspace_bytes("decoder", n, max_blocks)
    assert 0 < st["ws_peak_bytes"] <= st["ws_size_bytes"], st
    return st


class Guarded:
    """n output bytes at `offset` past a 16-byte aligned address, guard bytes on both sides (device tensor, or host array with host=True)"""

    def __init__(self, n, offset=0, host=False):
        self.n, self.at = n, GUARD + offset
        size = n + 2 * GUARD + 16
        self.buf = np.full(size, FILL, np.uint8) if host else torch.full((size,), FILL, dtype=torch.uint8, device="cuda")
        self.view = self.buf[self.at:self.at + n]
        if not host:
            torch.cuda.synchronize()  # the library writes on a stream of its own: the fill must have landed before it does

    def read(self):
        got = self.buf if isinstance(self.buf, np.ndarray) else self.buf.cpu().numpy()
        assert (got[:self.at] == FILL).all() and (got[self.at + self.n:] == FILL).all(), "guard bytes written"
        return got[self.at:self.at + self.n]


def dev_at(a, offset=0):
    """device copy of `a` that starts `offset` bytes past a 16-byte aligned address"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    buf = torch.zeros(len(a) + 32, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + len(a)]
    view.copy_(torch.from_numpy(a.copy()))
    assert view.data_ptr() % 16 == offset % 16
    return view


def text_with_origin(n, k, seed):
    """A text whose origin is exactly k: the first byte 'b' occurs once, k bytes are 'a' and every other byte is larger, so exactly the k
    suffixes that start with 'a' sort in front of the whole text."""
    rng = np.random.default_rng(seed)
    t = rng.integers(99, 103, size=n, dtype=np.uint8)
    t[0] = 98
    if k:
        t[1 + rng.choice(n - 1, size=k, replace=False)] = 97
    return t


def origins_for(n):
    """an origin on the 64-grid (and on the 8-grid of the small blocks) and one off both; a block of one byte has origin 0 only"""
    on = 64 if n > 64 else 0
    return [on] if n == 1 else [on, 37 if n > 37 else 1]


# ---- single blocks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES, ids=["n%d" % n for n in SIZES])
def test_single_blocks_on_exact_contexts(full, n):
    with decoder(n) as dec:
        texts = []
        for k in origins_for(n):
            t = text_with_origin(n, k, seed=n + k)
            L, origin = full.bwt_forward(t)
            assert origin == k and (origin % 64 == 0) == (k in (0, 64))
            what = "n = %d, origin %d" % (n, origin)
            # dk_bwt_inverse
            out = Guarded(n, host=True)
            assert dec._lib.dk_bwt_inverse(dec._h, _ptr(L), n, origin, _ptr(out.view)) == 0, what
            assert np.array_equal(out.read(), t), what + ": dk_bwt_inverse"
            # dk_dev_bwt_inverse, neither buffer aligned
            out = Guarded(n, 5)
            dec.dev_bwt_inverse(dev_at(L, 3), n, origin, out.view)
            assert np.array_equal(out.read(), t), what + ": dk_dev_bwt_inverse"
            # the block decoders, four models
            streams = {m: full.block_encode(m, t) for m in MODELS}
            for m in MODELS:
                assert dec.block_decode(m, streams[m], n) == t.tobytes(), what + ": dk_block_decode " + m
                assert dec.last_consumed() == len(streams[m])
                out = Guarded(n, 1)
                dec.dev_block_decode(m, streams[m], n, out.view)
                assert np.array_equal(out.read(), t), what + ": dk_dev_block_decode " + m
            # block::raw with bbb
            assert dec.raw_block_decode(full.raw_block_encode(t, 1), n, 1) == t.tobytes(), what + ": dk_raw_block_decode"
            texts.append((t, streams))
        # dk_dev_batch_decode: both blocks (twice each, so that the slots are reused)
        m = MODELS[n % 4]
        outs = [Guarded(n, i) for i in range(2 * len(texts))]
        dec.dev_batch_decode(m, [s[m] for _, s in texts] * 2, [n] * len(outs), [o.view for o in outs], host_threads=2)
        for o, (t, _) in zip(outs, texts * 2):
            assert np.array_equal(o.read(), t), "n = %d: dk_dev_batch_decode %s" % (n, m)
        st = check_workspace(dec, n)
        peak_with_records = os.environ.get("DECODER_PEAK_WITH_RECORDS")
        if peak_with_records and n == 70000:  # (the record-off run only) the switch must be live: the peak drops by the records' 4 n
            assert RECORD_OFF and st["ws_peak_bytes"] < int(peak_with_records) - 2 * n


def test_one_symbol_block_and_block_with_ff(full):
    n = 70000
    with decoder(n) as dec:
        t = np.full(n, 0x61, np.uint8)
        assert np.array_equal(dec.bwt_inverse(t, n - 1), t)  # L = a^n with origin n - 1 is the one text
        for m in MODELS:
            assert dec.block_decode(m, full.block_encode(m, t), n) == t.tobytes(), m  # returned whole (reference quirks)
        t = text_with_origin(n, 37, seed=1)
        t[5::97] = 0xFF
        t[-1] = 0xFF
        stream = full.block_encode("dark+ff", t)
        assert dec.block_decode("dark+ff", stream, n) == t.tobytes()
        out = Guarded(n)
        dec.dev_block_decode("dark+ff", stream, n, out.view)
        assert np.array_equal(out.read(), t)
        # without the flag the reference format cannot carry the block: whatever a full context makes of such a stream, this one makes too
        plain = full.block_encode("dark", t)
        answers = []
        for ctx in (full, dec):
            out = np.zeros(n, np.uint8)
            rc = ctx._lib.dk_block_decode(ctx._h, model_id("dark"), _ptr(np.frombuffer(plain, np.uint8)), len(plain), n, _ptr(out))
            answers.append((rc, out.tobytes() if rc == 0 else b""))
        assert answers[0] == answers[1] and answers[0] != (0, t.tobytes())
        check_workspace(dec, n)


def one_inverse_peak():
    t = text_with_origin(70000, 37, seed=70037)
    with dark_amd.Context(70000) as c, decoder(70000) as dec:
        dec.bwt_inverse(*c.bwt_forward(t))
        return dec.stats()["ws_peak_bytes"]


def test_record_off_fits_too():
    """DK_IBWT_RECORD=0 (a switch of the tuning build): no walk records, k_ibwt_emit / k_pib_emit instead of the copy kernels.  The S = 64
    single-block case and the packs once more, in a process of their own: same results, within the same exact contexts"""
    tuning = os.path.join(ROOT, "dark_amd", "libdark_amd_tuning.so")
    assert os.path.exists(tuning), "build with tuning=True (__graft_entry__.build does)"
    env = dict(os.environ, DARK_AMD_LIB=tuning, DK_IBWT_RECORD="0", DECODER_PEAK_WITH_RECORDS=str(one_inverse_peak()))
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                          "n70000 or test_packs"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "\n4 passed" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


# ---- packs ------------------------------------------------------------------------------------------------------------------------------
def pack_of(name):
    rng = np.random.default_rng(31)
    if name == "one_byte_blocks":  # the densest splitters a pack can have (one per byte), no records
        return [rng.integers(0, 255, size=1, dtype=np.uint8) for _ in range(4096)]  # (no 0xFF: the streams are plain `dark`)
    if name == "mixed":  # 1 B ... 1 MiB, most blocks at odd offsets
        sizes = [1, 2, 3, 17, 255, 4097, 65537, 70001, 333, 1 << 20, 64, 5]
        return [text_with_origin(n, min(n - 1, 37 if i % 2 else 64), seed=i) if n > 1 else np.array([7], np.uint8) for i, n in enumerate(sizes)]
    return [np.ascontiguousarray(datagen.word_like(262144 + 77, seed=9, vocab=2000))]  # "one_block": one block that fills max_n


@pytest.mark.parametrize("name", ["one_byte_blocks", "mixed", "one_block"])
def test_packs_on_exact_contexts(full, name):
    blocks = pack_of(name)
    sizes = [len(b) for b in blocks]
    total, count = sum(sizes), len(blocks)
    off = np.concatenate([[0], np.cumsum(sizes)])
    if name == "mixed":
        assert sum(int(o) % 2 for o in off[1:-1]) >= 5 and max(sizes) == 1 << 20 and min(sizes) == 1
    text = np.concatenate(blocks)
    d_bwt = torch.empty(total, dtype=torch.uint8, device="cuda")
    origins = full.dev_bwt_forward_packed(torch.from_numpy(text).cuda(), sizes, d_bwt)
    if name == "mixed":
        assert any(o % 64 == 0 for o, n in zip(origins, sizes) if n > 64) and any(o % 64 for o in origins)
    streams, _ = full.dev_packed_encode("dark", torch.from_numpy(text).cuda(), sizes, host_threads=4)
    with decoder(total, count) as dec:
        out = Guarded(total, 3)
        dec.dev_bwt_inverse_packed(d_bwt, sizes, origins, out.view)
        assert np.array_equal(out.read(), text), name + ": dk_dev_bwt_inverse_packed"
        out = Guarded(total, 1)
        dec.dev_packed_decode("dark", streams, sizes, out.view, host_threads=4)
        assert np.array_equal(out.read(), text), name + ": dk_dev_packed_decode"
        check_workspace(dec, total, count)
        # one block more than the context was made for: same bytes, the last block cut in two (a one-byte block cannot be cut: one pack more)
        peak = dec.stats()["ws_peak_bytes"]
        more = sizes[:-1] + [sizes[-1] - 1, 1] if sizes[-1] > 1 else sizes + [1]
        out = Guarded(sum(more))
        with pytest.raises(dark_amd.DarkError) as e:
            dec.dev_bwt_inverse_packed(torch.zeros(sum(more), dtype=torch.uint8, device="cuda"), more, [0] * len(more), out.view)
        assert e.value.code == DK_E_ARG and "1 .. %d blocks, not %d" % (count, count + 1) in str(e.value), str(e.value)
        with pytest.raises(dark_amd.DarkError) as e:
            dec.dev_packed_decode("dark", list(streams) + [streams[-1]], more, out.view, host_threads=2)
        assert e.value.code == DK_E_ARG and (out.read() == FILL).all()
        assert dec.stats()["ws_peak_bytes"] == peak
        out = Guarded(total)
        dec.dev_bwt_inverse_packed(d_bwt, sizes, origins, out.view)  # ... and the context is as usable as before
        assert np.array_equal(out.read(), text)
    if name == "one_byte_blocks":  # a full context keeps its own rule: DK_PACKED_MAX_BLOCKS, whatever its size
        out = Guarded(total)
        full.dev_bwt_inverse_packed(d_bwt, sizes, origins, out.view)
        assert np.array_equal(out.read(), text) and count > 1 and DK_PACKED_MAX_BLOCKS >= count


# ---- inputs that are no BWT: the decoder context answers what the full context answers -----------------------------------------------------
def failing_cases(orc, n):
    """one changed byte, a wrong origin, and an adjacent swap that leaves a short cycle without a splitter -- each one the model calls "no text" """
    text = M.word_text(n)
    sa = orc.sa_sais(text)
    L, origin = orc.bwt_forward(text, sa)
    rng = np.random.default_rng(n)
    cases = []
    for _ in range(20):
        x = L.copy()
        i = int(rng.integers(0, n))
        x[i] = (int(x[i]) + int(rng.integers(1, 255))) % 255
        c = M.case("a", x, origin)
        if c.verdict.text is None:
            cases.append(c)
            break
    c = M.case("c", L, (origin + 1 + n // 3) % n)
    assert c.verdict.text is None
    cases.append(c)
    sa = np.asarray(sa, dtype=np.int64)
    near = np.flatnonzero((L[:-1] != L[1:]) & (np.abs(sa[:-1] - sa[1:]) <= 40))
    for i in near[np.argsort(np.abs(sa[near] - sa[near + 1]), kind="stable")].tolist()[:60]:  # the shortest cycles first
        x = L.copy()
        x[i], x[i + 1] = x[i + 1], x[i]
        c = M.case("e", x, origin)
        if c.verdict.text is None and not c.verdict.cycle_has_splitter:
            cases.append(c)
            break
    assert [c.kind for c in cases] == ["a", "c", "e"]
    return text, L, origin, cases


@pytest.mark.parametrize("n", [5000, 70000])
def test_failures_are_the_full_contexts(full, orc, n):
    text, good_L, good_origin, cases = failing_cases(orc, n)
    with decoder(n) as dec, decoder(3 * n, 3) as dec_pack:
        for c in cases:
            what = "class %s, n = %d" % (c.kind, n)
            s = np.frombuffer(orc.block_dc_encode_bwt("exp", c.L, c.origin), np.uint8)
            for ctx in (full, dec):
                out = Guarded(n, host=True)
                assert ctx._lib.dk_bwt_inverse(ctx._h, _ptr(c.L), n, c.origin, _ptr(out.view)) == DK_E_STREAM, what
                assert (out.read() == FILL).all(), what + ": dk_bwt_inverse leaves `out` untouched on DK_E_STREAM"
                out = Guarded(n, 7)
                with pytest.raises(dark_amd.DarkError) as e:
                    ctx.dev_bwt_inverse(dev_at(c.L, 9), n, c.origin, out.view)
                assert e.value.code == DK_E_STREAM, what
                out.read()
                out = Guarded(n, host=True)
                assert ctx._lib.dk_block_decode(ctx._h, model_id("exp"), _ptr(s), len(s), n, _ptr(out.view)) == DK_E_STREAM, what
                out.read()
                out = Guarded(n)
                with pytest.raises(dark_amd.DarkError) as e:
                    ctx.dev_batch_decode("exp", [s], [n], [out.view], host_threads=1)
                assert e.value.code == DK_E_STREAM, what
                out.read()
            errors = []
            for ctx in (full, dec_pack):  # the bad block between two good ones: the message names it and nothing is written
                out = Guarded(3 * n, 3)
                with pytest.raises(dark_amd.DarkError) as e:
                    ctx.dev_bwt_inverse_packed(dev_at(np.concatenate([good_L, c.L, good_L])), [n] * 3, [good_origin, c.origin, good_origin], out.view)
                assert e.value.code == DK_E_STREAM and (out.read() == FILL).all(), what
                errors.append(str(e.value))
            assert errors[0] == errors[1] and "block 1 " in errors[0]
            # ... and both decoder contexts go on with a good block
            assert np.array_equal(dec.bwt_inverse(good_L, good_origin), text), what
            out = Guarded(2 * n)
            dec_pack.dev_bwt_inverse_packed(dev_at(np.concatenate([good_L, good_L])), [n, n], [good_origin] * 2, out.view)
            assert np.array_equal(out.read(), np.concatenate([text, text])), what
        check_workspace(dec, n)
        check_workspace(dec_pack, 3 * n, 3)


# ---- what a decoder context refuses -------------------------------------------------------------------------------------------------------
def refused_calls(ctx, n):
    """(entry, call) for every entry point that needs the suffix sort's workspace.  The buffers are real and large enough for the call to run:
    a gate that let one through would produce a wrong return code, not a fault."""
    lib, h = ctx._lib, ctx._h
    host = np.zeros(16 * n + 4096, np.uint8)
    text = np.frombuffer(b"abracadabra" * (n // 11 + 1), np.uint8)[:n].copy()
    d_text = torch.from_numpy(text).cuda()
    d_a, d_b, d_c, d_d, d_e = (torch.zeros(8 * n + 64, dtype=torch.uint8, device="cuda") for _ in range(5))
    p = lambda x, at=0: C.c_void_p(_ptr(x).value + at)  # noqa: E731
    sz, u32 = C.c_size_t(0), C.c_uint32(0)
    one = (C.c_size_t * 1)(n)
    ptr1 = (C.c_void_p * 1)(p(host).value)
    dptr1 = (C.c_void_p * 1)(p(d_text).value)
    cap1 = (C.c_size_t * 1)(4 * n + 4096)
    len1 = (C.c_size_t * 1)()
    flags = (C.c_uint * 1)()
    init = np.zeros(256, np.uint32)
    starts = np.array([0, n], np.uint32)
    batch = C.c_void_p()
    mid = model_id("dark")
    torch.cuda.synchronize()
    return [
        ("dk_suffix_array", lambda: lib.dk_suffix_array(h, p(text), n, p(host))),
        ("dk_bwt_forward", lambda: lib.dk_bwt_forward(h, p(text), n, p(host), C.byref(u32))),
        ("dk_dc_encode", lambda: lib.dk_dc_encode(h, p(text), n, p(init), p(host), p(host, 4 * n), p(host, 5 * n), C.byref(sz))),
        ("dk_block_encode", lambda: lib.dk_block_encode(h, mid, p(text), n, p(host), len(host), C.byref(sz))),
        ("dk_raw_block_encode", lambda: lib.dk_raw_block_encode(h, 1, p(text), n, p(host), len(host), C.byref(sz), None, 0, None)),
        ("dk_dev_suffix_array", lambda: lib.dk_dev_suffix_array(h, p(d_text), n, p(d_a))),
        ("dk_dev_bwt_forward", lambda: lib.dk_dev_bwt_forward(h, p(d_text), n, p(d_a), C.byref(u32))),
        ("dk_dev_dc_encode", lambda: lib.dk_dev_dc_encode(h, p(d_text), n, p(init), p(d_a), p(d_b), p(d_c), C.byref(sz))),
        ("dk_dev_block_encode", lambda: lib.dk_dev_block_encode(h, mid, p(d_text), n, p(host), len(host), C.byref(sz))),
        ("dk_dev_batch_encode", lambda: lib.dk_dev_batch_encode(h, mid, 1, dptr1, one, ptr1, cap1, len1, 1)),
        ("dk_batch_begin", lambda: lib.dk_batch_begin(h, mid, 1, C.byref(batch))),
        ("dk_dev_bwt_forward_packed", lambda: lib.dk_dev_bwt_forward_packed(h, p(d_text), 1, one, p(d_a), C.byref(u32))),
        ("dk_dev_suffix_array_packed", lambda: lib.dk_dev_suffix_array_packed(h, p(d_text), 1, one, p(d_a), None, None)),
        ("dk_suffix_array_packed", lambda: lib.dk_suffix_array_packed(h, p(text), 1, one, p(host))),
        ("dk_dev_dc_encode_packed", lambda: lib.dk_dev_dc_encode_packed(h, p(d_text), 1, one, p(init), p(d_a), p(d_b), p(d_c), len1)),
        ("dk_dev_packed_encode", lambda: lib.dk_dev_packed_encode(h, mid, p(d_text), 1, one, ptr1, cap1, len1, flags, 1)),
        ("dk_dbg_sort_pairs", lambda: lib.dk_dbg_sort_pairs(h, p(host), p(host, 8 * n), n, 0, 64)),
        ("dk_dbg_dev_sort_pairs", lambda: lib.dk_dbg_dev_sort_pairs(h, p(d_a), p(d_b), n, 0, 64)),
        ("dk_dbg_dev_local_sort", lambda: lib.dk_dbg_dev_local_sort(h, p(d_a), p(d_b), n, 0, 64)),
        ("dk_dbg_dev_sort_groups", lambda: lib.dk_dbg_dev_sort_groups(h, p(d_a), p(d_b), p(d_c), p(d_d), p(starts), 1, n, 0, 0, 64)),
        ("dk_dbg_dev_rerank", lambda: lib.dk_dbg_dev_rerank(h, p(d_a), 8, None, p(d_b), None, None, 0, n, None, None, None, None, None, None, p(d_c), p(d_c, 4 * n),
                                                            p(d_d), p(d_d, 4 * n), p(d_b, 4 * n), p(d_b, 6 * n), 1024, p(host), 0, 0, -1)),
        ("dk_dbg_dev_lf_rerank", lambda: lib.dk_dbg_dev_lf_rerank(h, p(d_a), 8, None, 0, p(d_b), 0, p(d_b, 4 * n), None, None, n, p(d_c), p(d_c, 4 * n), p(d_d), p(d_d, 4 * n),
                                                                  p(d_d, 5 * n), None, None, None, 0, None, 0, 0, p(host), 0)),
        ("dk_dbg_dev_lf_refine", lambda: lib.dk_dbg_dev_lf_refine(h, p(d_text), n, p(d_a), p(d_a, 4 * n), p(d_b), p(d_b, 4 * n), n // 2, 4, 0, p(d_c), p(d_d), p(host))),
        ("dk_dbg_dev_in_place", lambda: lib.dk_dbg_dev_in_place(h, n, 4, n // 2, p(d_a), p(d_a, 4 * n), p(d_b), p(d_b, 4 * n), n // 4, p(d_c), p(d_c, 4 * n), None, None, None,
                                                                -1, 0, -1, 0, p(d_d), p(d_d, 2 * n), None, p(d_d, 4 * n), p(host))),
        ("dk_dbg_dev_round", lambda: lib.dk_dbg_dev_round(h, p(d_text), n, 4, n // 2, p(d_a), p(d_a, 4 * n), p(d_b), p(d_b, 4 * n), n // 4, p(d_c), 0, 0, None, p(d_c, 4 * n),
                                                          None, None, None, p(d_d), p(d_d, 4 * n), None, p(d_e), p(d_e, 2 * n), p(d_e, 4 * n), p(d_e, 6 * n), None, p(host))),
        ("dk_dbg_dev_period", lambda: lib.dk_dbg_dev_period(h, p(d_text), n, 1, p(d_a), p(host), p(host, 64), 3, p(host, 128), 0, None, 0, 0, None, 0, None)),
        ("dk_dbg_dev_initial_sort", lambda: lib.dk_dbg_dev_initial_sort(h, p(d_text), n, p(init), 8, 7, None, 0, p(d_a), p(d_b), None, None, None, p(host))),
        ("dk_dbg_dev_packed_first", lambda: lib.dk_dbg_dev_packed_first(h, p(d_text), 1, one, p(d_a), p(d_b), p(d_c), p(d_d), p(host), p(host, 1024))),
        ("dk_dbg_dev_packed_round", lambda: lib.dk_dbg_dev_packed_round(h, 1, one, 4, p(d_a), n // 2, p(d_b), p(d_c), p(d_d), p(d_e), None, p(host))),
        ("dk_dbg_dev_inverse_permutation", lambda: lib.dk_dbg_dev_inverse_permutation(h, p(d_a), n, p(d_b), None)),
    ], batch


def test_refusals(full):
    n = 1000
    t = text_with_origin(n, 37, seed=4)
    L, origin = full.bwt_forward(t)
    with decoder(n) as dec:
        assert np.array_equal(dec.bwt_inverse(L, origin), t)
        calls, batch = refused_calls(dec, n)
        names = [name for name, _ in calls]
        # every entry of the header that takes a context and is not on the served list is on this one (dk_batch_push* take a batch, which a
        # decoder context never hands out)
        served = {"dk_ctx_destroy", "dk_ctx_purpose", "dk_capacity", "dk_last_error", "dk_last_consumed", "dk_last_block_flags", "dk_bwt_inverse",
                  "dk_dev_bwt_inverse", "dk_block_decode", "dk_dev_block_decode", "dk_dev_batch_decode", "dk_dev_bwt_inverse_packed",
                  "dk_dev_packed_decode", "dk_raw_block_decode", "dk_dc_decode", "dk_set_profiling", "dk_stats_reset", "dk_get_stats"}
        header = open(os.path.join(ROOT, "include", "dark_amd.h")).read()
        import re
        takes_ctx = set(re.findall(r"\b(dk_[a-z0-9_]+)\s*\((?:const )?dk_ctx \*ctx", header))
        assert takes_ctx - served == set(names), sorted((takes_ctx - served) ^ set(names))
        for name, call in calls:
            peak = dec.stats()["ws_peak_bytes"]
            assert call() == DK_E_ARG, name
            msg = dec._lib.dk_last_error(dec._h).decode()
            assert msg.startswith(name + ":") and "decoder context" in msg, msg
            assert not batch.value
            assert dec.stats()["ws_peak_bytes"] == peak, name
            assert np.array_equal(dec.bwt_inverse(L, origin), t), "the inverse after the refused " + name
        check_workspace(dec, n)
    # on a full context the same calls are served (the gate looks at the purpose, not at the entry alone): one of them as a sample
    calls, _ = refused_calls(full, n)
    assert dict(calls)["dk_dev_bwt_forward"]() == 0


# ---- the layers above the ABI -------------------------------------------------------------------------------------------------------------
def test_python_decoders(full, vectors, license_bytes):
    n = len(license_bytes)
    for m in MODELS:  # streams from tests/golden: what the reference's encoder wrote
        d = block.dc.Decoder(n, m)
        assert d.purpose == "decoder" and d._ctx.stats()["ws_size_bytes"] == workspace_bytes("decoder", n)
        assert d.decode(bytes.fromhex(vectors["oracle"]["LICENSE"]["streams_hex"][m])) == license_bytes
        check_workspace(d._ctx, n)
    r = block.raw.Decoder(n, "bbb")
    assert r.purpose == "decoder"
    assert r.decode(block.raw.Encoder(n, "bbb", ctx=full).encode(license_bytes)) == license_bytes
    check_workspace(r._ctx, n)
    assert block.dc.Decoder(n, "dark", ctx=full).purpose == "full"  # a context that is handed in is taken as it is
    e = block.dc.Encoder(n, "dark")
    assert e._ctx.purpose == "full" and block.dc.Decoder(n, "dark").decode(e.encode(license_bytes)) == license_bytes


def test_cpp_mirror_decoders(tmp_path):
    exe = str(tmp_path / "cpp_decoder_ctx")
    lib_dir = os.path.join(ROOT, "dark_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_decoder_ctx.cpp"),
                           "-L", lib_dir, "-ldark_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe, os.path.join(GOLDEN, "LICENSE.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cpp decoder contexts ok" in out.stdout


def test_multi_block_decode_two_slots_on_one_gpu(full):
    blocks = [text_with_origin(n, 37, seed=n) for n in (70000, 1000, 65536)] + [np.frombuffer(b"aba", np.uint8)]
    streams = [full.block_encode("ybs", b) for b in blocks]
    got = context_module.multi_block_decode("ybs", streams, [len(b) for b in blocks], [0, 0], host_threads_per_gpu=2)
    assert got == [b.tobytes() for b in blocks]


# ---- command line -----------------------------------------------------------------------------------------------------------------------
def test_cli_decodes_on_decoder_contexts(tmp_path, monkeypatch, capsys):
    data = np.ascontiguousarray(datagen.word_like(300000, seed=12, vocab=3000)).tobytes()
    made = []

    class Spy(context_module.Context):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
            self.spied_size = self.stats()["ws_size_bytes"]

    monkeypatch.setattr(context_module, "Context", Spy)
    monkeypatch.chdir(tmp_path)
    archives = {}
    for name, flags in (("single", []), ("blocks", ["-b", "100000"]), ("packed", ["-b", "100000", "--packed"])):
        (tmp_path / (name + ".txt")).write_bytes(data)
        cli.main(["-m", "exp", "--host-threads", "2"] + flags + [name + ".txt"])
        archives[name] = (tmp_path / (name + ".dark")).read_bytes()
    assert archives["blocks"] == archives["packed"] and made and all(c.purpose == "full" for c in made)  # the encode side is as it was
    capsys.readouterr()
    for name, flags, capacity, max_blocks in (("single", [], 300000, 1), ("blocks", [], 100000, 1), ("packed", ["--packed"], 300000, 3)):
        del made[:]
        cli.STATS.pop("ws_size_bytes", None)
        cli.main(["-m", "exp", "--host-threads", "2", "--stats"] + flags + [name + ".dark"])
        assert (tmp_path / (name + ".orig")).read_bytes() == data, name
        assert made and all(c.purpose == "decoder" for c in made), [c.purpose for c in made]
        want = workspace_bytes("decoder", capacity, max_blocks)
        assert [c.spied_size for c in made] == [want], name
        stats = json.loads(capsys.readouterr().err.strip().splitlines()[-1])
        assert stats["ws_size_bytes"] == want and 4 * want <= workspace_bytes("full", capacity), stats


# ---- one shape where the constant is small -----------------------------------------------------------------------------------------------
def test_sixteen_mib_on_a_quarter_of_the_workspace():
    n = 1 << 24
    t = torch.from_numpy(np.ascontiguousarray(datagen.wiki_like(n, seed=2))).cuda()
    d_bwt = torch.empty_like(t)
    with dark_amd.Context(n) as c:
        origin = c.dev_bwt_forward(t, n, d_bwt)
        full_size = c.stats()["ws_size_bytes"]
    with decoder(n) as dec:
        out = Guarded(n)
        dec.dev_bwt_inverse(d_bwt, n, origin, out.view)
        assert torch.equal(out.buf[out.at:out.at + n], t)
        out.read()
        back = dec.bwt_inverse(d_bwt.cpu().numpy(), origin)  # the host call holds two more block-sized buffers
        assert np.array_equal(back, t.cpu().numpy())
        st = check_workspace(dec, n)
        print("n = 2^24: decoder context %d bytes (peak %d), full context %d bytes" % (st["ws_size_bytes"], st["ws_peak_bytes"], full_size))
        assert 4 * st["ws_size_bytes"] <= full_size
