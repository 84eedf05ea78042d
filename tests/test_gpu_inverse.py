"""The inverse BWT (csrc/bwt.hip k_ibwt_* and k_pib_*) against the plain model of tests/ibwt_model.py, on correct inputs and on inputs that
are no BWT.  It is the one device stage that takes untrusted data and the container has no checksum, so ONE invariant holds for every entry
point and every input: DK_OK implies the output equals the model's text; "no text" implies DK_E_STREAM.  Around
every output buffer lie guard bytes that must be untouched after every call, accepted or rejected, and after every rejection the same
context inverts a correct input correctly.

Order: correct inputs; classes a-d (random damage: a leftover cycle holds a splitter and the jump rounds never resolve it); classes e-g
(short leftover cycles without a splitter, which no kernel ever visits: the origin's chain is then shorter than n)."""
import ctypes as C
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import dark_amd
import ibwt_model as M
from conftest import ROOT
from dark_amd import datagen
from dark_amd._lib import DK_E_STREAM
from dark_amd.context import _ptr, model_id

pytestmark = pytest.mark.gpu
CAP = 1 << 20
GUARD, FILL = 4096, 0xA5
MODELS = ("dark", "exp", "ybs", "simple")
RECORD_OFF = os.environ.get("DK_IBWT_RECORD") == "0"  # the run test_record_off_same_results starts: tuning library, no walk records


@pytest.fixture(scope="module")
def ctx():
    peak_with_records = os.environ.get("IBWT_PEAK_WITH_RECORDS")
    if peak_with_records:  # (that run only) the switch must be live: without the 256-byte records the workspace peak drops by about 4 n
        assert RECORD_OFF and one_inverse_peak() < int(peak_with_records) - 2 * 70000
    c = dark_amd.Context(CAP)
    yield c
    c.close()


def one_inverse_peak():
    """workspace peak of a fresh context after one inverse of 70000 bytes"""
    L = np.frombuffer(b"ab" * 35000, np.uint8)
    with dark_amd.Context(len(L)) as c:
        c.bwt_inverse(*oracle_bwt(_orc(), L))
        return c.stats()["ws_peak_bytes"]


def _orc():
    from oracle import orc
    orc.lib()
    return orc


class Guarded:
    """n output bytes at `offset` past a 16-byte aligned address, guard bytes on both sides (device tensor, or host array with host=True)"""

    def __init__(self, n, offset=0, host=False):
        self.n, self.at = n, GUARD + offset
        size = n + 2 * GUARD + 16
        self.buf = np.full(size, FILL, np.uint8) if host else torch.full((size,), FILL, dtype=torch.uint8, device="cuda")
        if not host:
            assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.at:self.at + n]

    def read(self):
        """the n bytes; fails when a guard byte changed"""
        got = self.buf if isinstance(self.buf, np.ndarray) else self.buf.cpu().numpy()
        assert (got[:self.at] == FILL).all() and (got[self.at + self.n:] == FILL).all(), "guard bytes written"
        return got[self.at:self.at + self.n]


def dev_at(a, offset=0):
    """device copy of `a` that starts `offset` bytes past a 16-byte aligned address"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    buf = torch.zeros(len(a) + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + len(a)]
    view.copy_(torch.from_numpy(a.copy()))
    assert view.data_ptr() % 16 == offset % 16
    return view


def code_of(fn, *args, **kw):
    try:
        fn(*args, **kw)
        return 0, ""
    except dark_amd.DarkError as e:
        return e.code, str(e)


def judge(what, rc, out, verdict, want="model"):
    """the invariant; `want` overrides the model's text where a decoder has a rule of its own (one-symbol blocks)"""
    if isinstance(want, str):
        want = verdict.text
    if want is None:
        assert rc == DK_E_STREAM, "%s: no text (the path has %d of %d entries, the leftover cycles hold %s splitter, the longest has %d " \
            "entries) but the call returned %d" % (what, verdict.d, len(out), "a" if verdict.cycle_has_splitter else "no", verdict.longest_cycle, rc)
    else:
        assert rc == 0, "%s: a text, but the call returned %d" % (what, rc)
        diff = np.flatnonzero(np.asarray(out) != want)
        assert len(diff) == 0, "%s: DK_OK with a wrong text: %d bytes differ, the first at %d" % (what, len(diff), diff[0])


def oracle_bwt(orc, t):
    return orc.bwt_forward(t, orc.sa_naive(t) if len(t) < 64 else None)


def sample_text(n, seed=3, sigma=4):
    if n >= 4000:
        return np.ascontiguousarray(datagen.word_like(n, seed=seed, vocab=2000))
    return np.random.default_rng(seed).integers(97, 97 + sigma, size=n, dtype=np.uint8)


@pytest.fixture(scope="module")
def good(orc):
    """two correct blocks, with their streams: what a context must still decode after a rejection, and the neighbours of a bad block"""
    out = []
    for n, seed in ((3000, 7), (9001, 8)):
        t = sample_text(n, seed, 5)
        L, origin = oracle_bwt(orc, t)
        out.append(dict(text=t, L=L, origin=origin, streams={m: orc.block_dc_encode(m, t) for m in MODELS}))
    return out


def recovers(ctx, good):
    g = good[0]
    assert np.array_equal(ctx.bwt_inverse(g["L"], g["origin"]), g["text"]), "the context does not invert a correct input after a rejection"


# ---- the entry points, each returning (return code, the n output bytes with the guards checked, error text) ----------------------------------
def run_host(ctx, L, origin):
    L = np.ascontiguousarray(L)
    out = Guarded(len(L), host=True)
    rc = ctx._lib.dk_bwt_inverse(ctx._h, _ptr(L), len(L), int(origin), _ptr(out.view))
    return rc, out.read(), ""


def run_dev(ctx, L, origin, in_off=0, out_off=0):
    out = Guarded(len(L), out_off)
    rc, msg = code_of(ctx.dev_bwt_inverse, dev_at(L, in_off), len(L), origin, out.view)
    return rc, out.read(), msg


def run_packed(ctx, blocks, in_off=0, out_off=0):
    """blocks = [(L, origin), ...] -> (rc, list of the blocks' output ranges, error text)"""
    sizes = [len(L) for L, _ in blocks]
    out = Guarded(sum(sizes), out_off)
    rc, msg = code_of(ctx.dev_bwt_inverse_packed, dev_at(np.concatenate([L for L, _ in blocks]), in_off), sizes, [o for _, o in blocks], out.view)
    return rc, np.split(out.read(), np.cumsum(sizes)[:-1]), msg


def check_correct(ctx, orc, t, what):
    """a correct input through the host call, the device call and a pack of two; the class of the origin is the caller's business"""
    t = np.ascontiguousarray(t, dtype=np.uint8)
    L, origin = oracle_bwt(orc, t)
    v = M.invert(L, origin)
    assert v.text is not None and np.array_equal(v.text, t), "%s: the model does not give the text back" % what
    for name, (rc, out, _) in (("dk_bwt_inverse", run_host(ctx, L, origin)), ("dk_dev_bwt_inverse", run_dev(ctx, L, origin))):
        judge("%s, %s, origin %d" % (what, name, origin), rc, out, v)
    small = np.frombuffer(b"nnbaaa", np.uint8)  # banana, origin 3
    rc, outs, _ = run_packed(ctx, [(small, 3), (L, origin)])
    judge("%s, dk_dev_bwt_inverse_packed, origin %d" % (what, origin), rc, outs[1], v)
    assert outs[0].tobytes() == b"banana"
    return L, origin, v


# ---- correct inputs ---------------------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 7, 8, 9, 63, 64, 65, 4095, 4096, 4097, 65535, 65536, 65537, 262144 + 77]
EDGE_SIZES = [9, 4097, 65537]  # S = 8 with one and with many tiles, S = 64


@pytest.mark.parametrize("n", SIZES, ids=["n%d" % n for n in SIZES])
def test_correct_sizes(ctx, orc, n):
    """the sizes around the tile (4096), around the change of the splitter spacing (65536: S 8 -> 64, k_ibwt_emit -> k_ibwt_copy) and tiny ones"""
    check_correct(ctx, orc, sample_text(n, seed=n), "n = %d" % n)


@pytest.mark.parametrize("n", EDGE_SIZES, ids=["n%d" % n for n in EDGE_SIZES])
@pytest.mark.parametrize("where", ["first", "last", "multiple", "between"])
def test_correct_origin_classes(ctx, orc, n, where):
    """origin 0 (the first symbol is the text's only smallest one), n - 1 (its only largest one), a multiple of S and not a multiple of S
    (seeds searched); the class is asserted from the oracle's origin"""
    S = M.spacing(n)
    rng = np.random.default_rng(n)
    if where in ("first", "last"):
        t = rng.integers(98, 102, size=n, dtype=np.uint8)
        t[0] = 97 if where == "first" else 200
    else:
        for _ in range(5000):
            t = rng.integers(97, 101, size=n, dtype=np.uint8)
            o = oracle_bwt(orc, t)[1]
            if (o % S == 0) == (where == "multiple"):
                break
        else:
            raise AssertionError("no text of %d bytes with the wanted origin" % n)
    _, origin, _ = check_correct(ctx, orc, t, "n = %d, origin %s" % (n, where))
    assert {"first": origin == 0, "last": origin == n - 1, "multiple": origin % S == 0, "between": origin % S != 0}[where], origin


@pytest.mark.parametrize("n", EDGE_SIZES, ids=["n%d" % n for n in EDGE_SIZES])
@pytest.mark.parametrize("sigma", [1, 2, 4, 256])
def test_correct_alphabets(ctx, orc, n, sigma):
    """1, 2, 4 and 256 symbols, byte 0xFF among them (the inverse itself has no 0xFF quirk)"""
    alphabet = np.array({1: [0xFF], 2: [0x00, 0xFF], 4: [0x00, 0x01, 0xFE, 0xFF]}.get(sigma, range(256)), dtype=np.uint8)
    t = alphabet[np.random.default_rng(sigma).integers(0, sigma, size=n)]
    t[n // 2] = 0xFF
    if n >= 2 * sigma:
        t[n - sigma:] = alphabet  # every symbol at least once
        assert len(np.unique(t)) == sigma
    check_correct(ctx, orc, t, "n = %d, %d symbols" % (n, sigma))


GRID_SIZES = [4097, 65537, 300000]


@pytest.mark.parametrize("n", GRID_SIZES, ids=["n%d" % n for n in GRID_SIZES])
def test_correct_unaligned_buffers(ctx, orc, n):
    """d_bwt at byte offsets 0, 1, 8, 15 past a 16-byte boundary (k_ibwt_hist then leaves its 16-byte loads) and d_out at offsets 0, 1, 4, 7
    (the emit and copy kernels, single-block and packed, then store single bytes): slices of one allocation, all 16 combinations"""
    t = sample_text(n, seed=n + 1)
    L, origin = oracle_bwt(orc, t)
    v = M.invert(L, origin)
    assert np.array_equal(v.text, t)
    small = np.frombuffer(b"nnbaaa", np.uint8)
    for in_off in (0, 1, 8, 15):
        for out_off in (0, 1, 4, 7):
            what = "n = %d, d_bwt + %d, d_out + %d" % (n, in_off, out_off)
            rc, out, _ = run_dev(ctx, L, origin, in_off, out_off)
            judge(what + ", dk_dev_bwt_inverse", rc, out, v)
            rc, outs, _ = run_packed(ctx, [(small, 3), (L, origin)], in_off, out_off)
            judge(what + ", dk_dev_bwt_inverse_packed", rc, outs[1], v)
            assert outs[0].tobytes() == b"banana", what


# ---- inputs that are no BWT ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def damaged(orc):
    """n -> (text, L, origin, cases): classes a-f from a word-like text of n bytes; class g (one-symbol L, n = 10 and n = 70000) rides with the
    set of its splitter spacing"""
    out = {}
    for n in (5000, 70000):
        text, L, origin, cases = M.no_bwt_inputs(orc, n)
        out[n] = (text, L, origin, cases + [c for c in M.one_symbol() if M.spacing(len(c.L)) == M.spacing(n)])
    return out


@pytest.mark.parametrize("n", [70000], ids=["n70000"])
def test_correct_walk_longer_than_the_record(ctx, orc, damaged, n):
    """the resume branch of k_ibwt_copy / k_pib_copy: a walk between two splitters longer than IB_REC, asserted from the model's path"""
    text, L, origin, _ = damaged[n]
    assert M.invert(L, origin).longest_walk > M.IB_REC
    check_correct(ctx, orc, text, "n70000 word text")


def name_of(c, i):
    return "class %s input %d (n = %d, origin %d, n - d = %d)" % (c.kind, i, len(c.L), c.origin, len(c.L) - c.verdict.d)


def decoders_text(c):
    """what a block decoder owes for a stream made from (L, origin): the model's answer, except that a one-symbol block is returned whole
    whatever origin the stream carries (reference quirks)"""
    return c.L if int(c.L.min()) == int(c.L.max()) else c.verdict.text


def entry_host(ctx, orc, good, c, i):
    rc, out, _ = run_host(ctx, c.L, c.origin)
    judge(name_of(c, i) + ", dk_bwt_inverse", rc, out, c.verdict)
    if rc:
        recovers(ctx, good)


def entry_dev(ctx, orc, good, c, i):
    rc, out, _ = run_dev(ctx, c.L, c.origin)
    judge(name_of(c, i) + ", dk_dev_bwt_inverse", rc, out, c.verdict)
    if rc:
        recovers(ctx, good)


def entry_block_decode(model):
    def run(ctx, orc, good, c, i):
        s = np.frombuffer(orc.block_dc_encode_bwt(model, c.L, c.origin), np.uint8)
        out = Guarded(len(c.L), host=True)
        rc = ctx._lib.dk_block_decode(ctx._h, model_id(model), _ptr(s), len(s), len(c.L), _ptr(out.view))
        judge(name_of(c, i) + ", dk_block_decode " + model, rc, out.read(), c.verdict, decoders_text(c))
        if rc:
            recovers(ctx, good)
    return run


def entry_dev_block_decode(model):
    def run(ctx, orc, good, c, i):
        out = Guarded(len(c.L))
        rc, _ = code_of(ctx.dev_block_decode, model, orc.block_dc_encode_bwt(model, c.L, c.origin), len(c.L), out.view)
        judge(name_of(c, i) + ", dk_dev_block_decode " + model, rc, out.read(), c.verdict, decoders_text(c))
        if rc:
            recovers(ctx, good)
    return run


def entry_batch(ctx, orc, good, c, i):
    """one bad block between two good ones.  About the good blocks' buffers after a failure include/dark_amd.h promises nothing: only the
    guards are looked at, and the same context then decodes the good blocks"""
    model = MODELS[i % 4]
    streams = [good[0]["streams"][model], orc.block_dc_encode_bwt(model, c.L, c.origin), good[1]["streams"][model]]
    sizes = [len(good[0]["text"]), len(c.L), len(good[1]["text"])]
    outs = [Guarded(n) for n in sizes]
    rc, _ = code_of(ctx.dev_batch_decode, model, streams, sizes, [o.view for o in outs], host_threads=2)
    got = [o.read() for o in outs]
    judge(name_of(c, i) + ", dk_dev_batch_decode " + model, rc, got[1], c.verdict, decoders_text(c))
    if rc:
        outs = [Guarded(sizes[0]), Guarded(sizes[2])]
        ctx.dev_batch_decode(model, [streams[0], streams[2]], [sizes[0], sizes[2]], [o.view for o in outs], host_threads=2)
        got = [outs[0].read(), None, outs[1].read()]
    assert np.array_equal(got[0], good[0]["text"]) and np.array_equal(got[2], good[1]["text"]), name_of(c, i) + ": the good blocks"


def multi_decode(model, streams, sizes, outs):
    lib = dark_amd.load_library()
    keep = [np.frombuffer(bytes(s), np.uint8) for s in streams]
    count = len(keep)
    devs = (C.c_int * 2)(0, 0)  # two contexts on GPU 0
    ins = (C.c_void_p * count)(*[_ptr(s) for s in keep])
    lens = (C.c_size_t * count)(*[len(s) for s in keep])
    ns = (C.c_size_t * count)(*sizes)
    optrs = (C.c_void_p * count)(*[_ptr(o.view) for o in outs])
    err = C.create_string_buffer(512)
    return lib.dk_multi_block_decode(devs, 2, model_id(model), count, ins, lens, ns, optrs, 2, err, 512)


def entry_multi(ctx, orc, good, c, i):
    model = MODELS[(i + 1) % 4]
    streams = [good[0]["streams"][model], orc.block_dc_encode_bwt(model, c.L, c.origin), good[1]["streams"][model]]
    sizes = [len(good[0]["text"]), len(c.L), len(good[1]["text"])]
    outs = [Guarded(n, host=True) for n in sizes]
    rc = multi_decode(model, streams, sizes, outs)
    got = [o.read() for o in outs]
    judge(name_of(c, i) + ", dk_multi_block_decode " + model, rc, got[1], c.verdict, decoders_text(c))
    if rc:  # a fresh call decodes the good blocks
        outs = [Guarded(sizes[0], host=True), Guarded(sizes[2], host=True)]
        assert multi_decode(model, [streams[0], streams[2]], [sizes[0], sizes[2]], outs) == 0
        got = [outs[0].read(), None, outs[1].read()]
    assert np.array_equal(got[0], good[0]["text"]) and np.array_equal(got[2], good[1]["text"]), name_of(c, i) + ": the good blocks"


def packed_verdict(what, rc, msg, out, want, good, sizes):
    """the packed contract (include/dark_amd.h): DK_E_STREAM names the block and NOTHING is written"""
    whole = out.read()
    if want is None:
        assert rc == DK_E_STREAM, "%s: no text, but the call returned %d" % (what, rc)
        assert "block 1 " in msg, msg
        assert (whole == FILL).all(), what + ": a rejected pack wrote to d_out"
    else:
        assert rc == 0, "%s: a text, but the call returned %d (%s)" % (what, rc, msg)
        parts = np.split(whole, np.cumsum(sizes)[:-1])
        assert np.array_equal(parts[1], want), what + ": DK_OK with a wrong text"
        assert np.array_equal(parts[0], good[0]["text"]) and np.array_equal(parts[2], good[1]["text"]), what + ": the good blocks"


def entry_packed(ctx, orc, good, c, i):
    sizes = [len(good[0]["text"]), len(c.L), len(good[1]["text"])]
    out = Guarded(sum(sizes))
    rc, msg = code_of(ctx.dev_bwt_inverse_packed, dev_at(np.concatenate([good[0]["L"], c.L, good[1]["L"]])), sizes,
                      [good[0]["origin"], c.origin, good[1]["origin"]], out.view)
    packed_verdict(name_of(c, i) + ", dk_dev_bwt_inverse_packed", rc, msg, out, c.verdict.text, good, sizes)
    if rc:
        recovers(ctx, good)


def entry_packed_decode(ctx, orc, good, c, i):
    model = MODELS[(i + 2) % 4]
    streams = [good[0]["streams"][model], orc.block_dc_encode_bwt(model, c.L, c.origin), good[1]["streams"][model]]
    sizes = [len(good[0]["text"]), len(c.L), len(good[1]["text"])]
    out = Guarded(sum(sizes))
    rc, msg = code_of(ctx.dev_packed_decode, model, streams, sizes, out.view, host_threads=2)
    packed_verdict(name_of(c, i) + ", dk_dev_packed_decode " + model, rc, msg, out, decoders_text(c), good, sizes)
    if rc:
        recovers(ctx, good)


ENTRIES = dict([("bwt_inverse", entry_host), ("dev_bwt_inverse", entry_dev)] +
               [("block_decode_" + m, entry_block_decode(m)) for m in MODELS] +
               [("dev_block_decode_" + m, entry_dev_block_decode(m)) for m in MODELS] +
               [("dev_batch_decode", entry_batch), ("multi_block_decode", entry_multi), ("dev_bwt_inverse_packed", entry_packed),
                ("dev_packed_decode", entry_packed_decode)])
NO_BWT = [(kinds, n, entry) for kinds in ("abcd", "efg") for n in (5000, 70000) for entry in ENTRIES]  # a-d first, then e-g


@pytest.mark.parametrize("kinds,n,entry", NO_BWT, ids=["%s-n%d-%s" % p for p in NO_BWT])
def test_no_bwt(ctx, orc, good, damaged, kinds, n, entry):
    """Every input of the classes through one entry point.  Candidates the model calls a text (a swap can leave one) must decode to the
    model's text; nothing is dropped.  Classes e, f and g are the ones only the length of the origin's chain gives away: without that check
    every single-block entry point answers DK_OK and leaves the first n - d bytes of the output unwritten."""
    cases = [c for c in damaged[n][3] if c.kind in kinds]
    assert cases and {c.kind for c in cases} >= set(kinds) - set("f")  # (class f exists at S = 64 only: tests/test_ibwt_model.py)
    failures = []
    for i, c in enumerate(cases):  # every input is tried: a wrong answer is no fault, and the report names all of them
        try:
            ENTRIES[entry](ctx, orc, good, c, i)
        except AssertionError as e:
            failures.append(str(e).splitlines()[0])
    assert not failures, "%d of %d inputs:\n%s" % (len(failures), len(cases), "\n".join(failures))


def test_cli_refuses_a_record_that_is_no_bwt(tmp_path, orc, damaged):
    """an archive written by dark_amd.cli with one record's stream replaced by a class-e stream of the same block size: non-zero exit and
    no output file, partial or otherwise, batched and packed"""
    from dark_amd import cli
    text, _, _, cases = damaged[5000]
    bad = next(c for c in cases if c.kind == "e")
    data = np.concatenate([sample_text(5000, 21), text, sample_text(3333, 22)])
    (tmp_path / "words.txt").write_bytes(data.tobytes())
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))

    def run(*args):
        return subprocess.run([sys.executable, "-m", "dark_amd.cli", "-m", "exp", "--host-threads", "2"] + list(args), cwd=str(tmp_path), env=env,
                              capture_output=True, text=True, timeout=600)
    out = run("-b", "5000", "words.txt")
    assert out.returncode == 0, out.stderr[-2000:]
    archive = str(tmp_path / "words.dark")
    blob = open(archive, "rb").read()
    offsets, end = cli.read_footer(archive)
    assert len(offsets) == 3
    bounds = offsets + [end]
    records = [blob[bounds[k]:bounds[k + 1]] for k in range(3)]
    assert records[1] == struct.pack("<I", 5000) + orc.block_dc_encode("exp", text)
    for flags in ([], ["--packed"]):
        open(archive, "wb").write(blob)
        out = run(*(flags + ["words.dark"]))
        assert out.returncode == 0 and (tmp_path / "words.orig").read_bytes() == data.tobytes(), out.stderr[-2000:]
        os.remove(str(tmp_path / "words.orig"))
        records[1] = struct.pack("<I", 5000) + orc.block_dc_encode_bwt("exp", bad.L, bad.origin)
        f = io.BytesIO()
        f.write(b"".join(records))
        cli._write_footer(f, [0, len(records[0]), len(records[0]) + len(records[1])])
        open(archive, "wb").write(f.getvalue())
        out = run(*(flags + ["words.dark"]))
        assert out.returncode != 0, "the damaged archive decoded without complaint %s" % flags
        assert "DK_E_STREAM" in out.stderr, out.stderr[-2000:]
        assert sorted(os.listdir(str(tmp_path))) == ["words.dark", "words.txt"], os.listdir(str(tmp_path))
        records[1] = struct.pack("<I", 5000) + orc.block_dc_encode("exp", text)


LARGE = ["n%d" % n for n in SIZES + GRID_SIZES + [70000] if n >= 65536]


def test_record_off_same_results():
    """DK_IBWT_RECORD=0 (a switch of the tuning build): the single-block inverse then runs k_ibwt_emit at S = 64 and the packed one
    k_pib_emit on every pack.  The correct inputs of 65536 bytes and more and classes a-g at n = 70000, in a process of their own: the same
    tests, the same results"""
    tuning = os.path.join(ROOT, "dark_amd", "libdark_amd_tuning.so")
    assert os.path.exists(tuning), "build with tuning=True (__graft_entry__.build does)"
    env = dict(os.environ, DARK_AMD_LIB=tuning, DK_IBWT_RECORD="0", IBWT_PEAK_WITH_RECORDS=str(one_inverse_peak()))
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                          "not record_off and not cli and (%s)" % " or ".join(sorted(set(LARGE)))], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=1200)
    expected = sum(n >= 65536 for n in SIZES) + 4 + 4 + sum(n >= 65536 for n in GRID_SIZES) + 1 + 2 * len(ENTRIES)  # sizes, origin classes,
    assert out.returncode == 0 and "%d passed" % expected in out.stdout, out.stdout[-4000:] + out.stderr[-2000:]   # alphabets, grids, walk, a-g
