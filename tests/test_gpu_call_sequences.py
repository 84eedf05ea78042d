"""Every stage behind every other stage, on ONE context of the product library.  The mailbox (csrc/mailbox.hpp) and the workspace outlive a
call, and every test file feeds its own context near-identical calls: a stage that forgot to clear or write a word it reads gets away with
it until another stage has used that word.  Twelve ops, one per device stage, each with its expected result computed once from the CPU
models (oracle/orc.py, ibwt_model, lcp_model, sa_query_model, fm_model), sizes from a few bytes to 2^17; three of them end in an error or a
"no" (the inverse of a non-BWT, an LCP call with a bad suffix array, an sa_check with verdict bad_order).

  test_every_ordered_pair   one walk of 145 calls in which every ordered pair (A, then B) of the twelve occurs as neighbours (an Euler tour of the
                            complete directed graph with loops), every call checked against its model
  test_behind_a_filled_mailbox   every op once behind dk_dbg_mail_fill with 0x00, 0xA5 and 0xFF
  test_the_instruments_refuse_what_they_must   the argument checks of dk_dbg_mail_fill and dk_dbg_ws_peek, an open batch among them
tests/test_gpu_poison_stages.py runs the same stages on a poisoned workspace, in processes of their own."""
import numpy as np
import pytest
import torch

import dark_amd
import ibwt_model as M
from dark_amd import datagen, fm
from dark_amd._lib import DK_E_ARG, DK_E_HIP, DK_E_NOMEM, DK_E_STREAM
from dark_amd.context import _ptr
from fm_model import fm_model
from lcp_model import lcp_kasai
from sa_query_model import BAD_ORDER, check_model, search_model
from test_gpu_lcp import planted

pytestmark = pytest.mark.gpu
CAP = 1 << 17
FILL = 0xA5


def u8(x):
    return np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8)


def dev(a, dtype=np.uint8):
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.view({1: np.uint8, 4: np.int32}[a.dtype.itemsize]).copy()).cuda()


def words(n):
    return torch.full((max(n, 1),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")


def host32(t):
    return t.cpu().numpy().view(np.uint32)


def error_of(fn):
    try:
        fn()
    except dark_amd.DarkError as e:
        return e.code
    return 0


def build_ops(orc):
    """name -> (call(ctx) -> result, expected result); the results are plain Python values that compare with =="""
    rng = np.random.default_rng(5)

    def sa_of(t):
        return orc.sa_sais(t) if len(t) > 1 else orc.sa_naive(t)

    def bwt_of(t):
        return orc.bwt_forward(t, orc.sa_naive(t) if len(t) < 64 else None)

    ops = {}
    # 1. the single-block forward path: suffix sort, L, DC, the host coder (2^17 bytes)
    t_enc = u8(datagen.wiki_like(CAP, seed=31))
    ops["block_encode"] = (lambda ctx: ctx.block_encode("dark", t_enc), orc.block_dc_encode("dark", t_enc))
    # 2. the DC stage alone, eleven bytes
    L_small, _ = bwt_of(u8(b"abracadabra"))
    w = orc.dc_encode(L_small)

    def dc(ctx):
        got = ctx.dc_encode(L_small)
        return tuple(np.asarray(got[k]).tolist() for k in ("init", "d", "sym", "rank"))
    ops["dc_encode"] = (dc, tuple(np.asarray(w[k]).tolist() for k in ("init", "d", "sym", "rank")))
    # 3. the inverse, splitters every 64 positions with records
    t_inv = u8(datagen.word_like(70000, seed=3, vocab=2000))
    L_inv, o_inv = bwt_of(t_inv)
    ops["bwt_inverse"] = (lambda ctx: ctx.bwt_inverse(L_inv, o_inv).tobytes(), t_inv.tobytes())
    # 4. the inverse of bytes that are no BWT (class e: a short leftover cycle that no kernel visits)
    _, _, _, cases = M.no_bwt_inputs(orc, 5000)
    bad = next(c for c in cases if c.kind == "e" and c.verdict.text is None)

    bad_L = np.ascontiguousarray(bad.L)

    def no_bwt(ctx):  # (the host form: the one whose output is promised untouched, include/dark_amd.h)
        out = np.full(len(bad_L), FILL, np.uint8)
        rc = ctx._lib.dk_bwt_inverse(ctx._h, _ptr(bad_L), len(bad_L), int(bad.origin), _ptr(out))
        return rc, bool((out == FILL).all())
    ops["inverse_of_no_bwt"] = (no_bwt, (DK_E_STREAM, True))
    # 5. - 7. packs: forward, suffix arrays, inverse
    pack = [rng.integers(97, 100, size=k, dtype=np.uint8) for k in (1, 2, 3, 17, 4097)] + [u8(b"ab" * 150), u8(datagen.wiki_like(9001, seed=8))]
    sizes = [len(b) for b in pack]
    cat = np.concatenate(pack)
    pairs = [bwt_of(b) for b in pack]
    L_pack, o_pack = np.concatenate([p[0] for p in pairs]), [int(p[1]) for p in pairs]

    def packed_forward(ctx):
        d_bwt = torch.empty(len(cat), dtype=torch.uint8, device="cuda")
        origins = ctx.dev_bwt_forward_packed(dev(cat), sizes, d_bwt)
        return d_bwt.cpu().numpy().tobytes(), origins
    ops["packed_forward"] = (packed_forward, (L_pack.tobytes(), o_pack))

    def packed_sa(ctx):
        d_sa = words(len(cat))
        ctx.dev_suffix_array_packed(dev(cat), sizes, d_sa)
        return host32(d_sa).tobytes()
    ops["packed_sa"] = (packed_sa, np.concatenate([sa_of(b) for b in pack]).astype(np.uint32).tobytes())

    def packed_inverse(ctx):
        d_out = torch.empty(len(cat), dtype=torch.uint8, device="cuda")
        ctx.dev_bwt_inverse_packed(dev(L_pack), sizes, o_pack, d_out)
        return d_out.cpu().numpy().tobytes()
    ops["packed_inverse"] = (packed_inverse, cat.tobytes())
    # 8. LCP: a passage of 300 bytes twice (the long list), on the oracle's suffix array
    t_lcp = planted(300, seed=300)
    sa_lcp = sa_of(t_lcp)

    def lcp(ctx):
        d_lcp = words(len(t_lcp))
        ctx.dev_lcp(dev(t_lcp), len(t_lcp), dev(sa_lcp, np.uint32), d_lcp)
        return host32(d_lcp).tobytes(), "lcp_long" in ctx.stats()["routes"]
    ops["lcp"] = (lcp, (lcp_kasai(t_lcp, sa_lcp).astype(np.uint32).tobytes(), True))
    # 9. LCP with a suffix array that has an entry outside its block
    t_bad = u8(datagen.wiki_like(10000, seed=21))
    sa_bad = sa_of(t_bad).copy()
    sa_bad[5000] = len(t_bad) + 7

    def lcp_bad(ctx):
        d_lcp = words(len(t_bad))
        rc = error_of(lambda: ctx.dev_lcp(dev(t_bad), len(t_bad), dev(sa_bad, np.uint32), d_lcp))
        return rc, bool((host32(d_lcp) == 0x5A5A5A5A).all())
    ops["lcp_of_bad_sa"] = (lcp_bad, (DK_E_ARG, True))
    # 10. sa_check: two entries swapped
    t_chk = u8(datagen.wiki_like(20011, seed=6))
    sa_chk = sa_of(t_chk).copy()
    sa_chk[[5000, 5001]] = sa_chk[[5001, 5000]]
    want_chk = check_model(t_chk, sa_chk)
    assert want_chk[0] == BAD_ORDER
    ops["sa_check_bad_order"] = (lambda ctx: ctx.dev_sa_check(dev(t_chk), len(t_chk), dev(sa_chk, np.uint32)), want_chk)
    # 11. sa_search: patterns that occur and the same with their last byte changed, on both sides of the border between the two kernels
    t_q = t_inv
    sa_q = sa_of(t_q)
    pats = []
    for k, m in enumerate([1, 2, 5, 16, 17, 255, 256, 257, 1100] * 4):
        a = int(rng.integers(0, len(t_q) - m))
        p = t_q[a:a + m].copy()
        if k & 1:
            p[-1] ^= 1
        pats.append(p)
    pats.append(u8(b""))
    flat = np.concatenate(pats + [np.zeros(1, np.uint8)])

    def search(ctx):
        lo, hi = words(len(pats)), words(len(pats))
        ctx.dev_sa_search(dev(t_q), len(t_q), dev(sa_q, np.uint32), dev(flat), [len(p) for p in pats], lo, hi)
        return list(zip(host32(lo).tolist(), host32(hi).tolist()))
    ops["sa_search"] = (search, search_model(t_q, sa_q, pats))
    # 12. the FM-index: build, count, locate and extract structures, and the whole text back
    t_fm = u8(datagen.wiki_like(5000, seed=3))
    L_fm, o_fm = bwt_of(t_fm)
    sa_fm = sa_of(t_fm)
    fm_pats = [bytes(t_fm[a:a + m]) for a, m in ((0, 3), (100, 5), (4000, 9), (4990, 10), (17, 1))] + [b"\x00zz", b""]
    want_ranges = fm_model(L_fm, o_fm, fm_pats)

    def fm_index(ctx):
        index = fm.Index.from_bwt(ctx, L_fm, o_fm, locate_step=8, extract_step=32)
        lo, hi = index.count(fm_pats)
        return list(zip(lo.tolist(), hi.tolist())), [row.tolist() for row in index.locate(fm_pats, max_hits=4)], index.text()
    ops["fm_index"] = (fm_index, (want_ranges, [sa_fm[lo:min(hi, lo + 4)].tolist() for lo, hi in want_ranges], t_fm.tobytes()))
    return ops


@pytest.fixture(scope="module")
def ops(orc):
    return build_ops(orc)


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


def euler_tour(k):
    """nodes 0 .. k-1 in an order in which every ordered pair (a, b), a == b included, occurs once as neighbours: k * k + 1 entries"""
    unused = {a: list(range(k - 1, -1, -1)) for a in range(k)}
    stack, tour = [0], []
    while stack:  # Hierholzer: every node has as many edges in as out
        a = stack[-1]
        if unused[a]:
            stack.append(unused[a].pop())
        else:
            tour.append(stack.pop())
    return tour[::-1]


_dead = []  # a HIP error (a fault on the card): nothing more is started


def run(ctx, ops, name):
    if _dead:
        pytest.fail("not started: %s" % _dead[0])
    call, want = ops[name]
    try:
        got = call(ctx)
    except dark_amd.DarkError as e:
        if e.code == DK_E_HIP:
            _dead.append("%s: %s" % (name, e))
        raise
    st = ctx.stats()
    assert 0 <= st["ws_peak_bytes"] <= st["ws_size_bytes"], (name, st)
    return got == want


def test_every_ordered_pair(ctx, ops):
    names = sorted(ops)
    assert len(names) == 12
    tour = euler_tour(len(names))
    assert len(tour) == 145 and {(a, b) for a, b in zip(tour, tour[1:])} == {(a, b) for a in range(12) for b in range(12)}
    failures, before = [], None
    for k in tour:
        if not run(ctx, ops, names[k]):  # (a wrong answer is no fault: the walk goes on and the report names every pair)
            failures.append("%s behind %s" % (names[k], before))
        before = names[k]
    assert not failures, "%d of %d calls differ from their model:\n%s" % (len(failures), len(tour), "\n".join(failures))


@pytest.mark.parametrize("byte", [0x00, 0xA5, 0xFF])
def test_behind_a_filled_mailbox(ctx, ops, byte):
    failures = []
    for name in sorted(ops):
        ctx.dbg_mail_fill(byte)
        if not run(ctx, ops, name):
            failures.append(name)
    assert not failures, "behind a mailbox of 0x%02X: %s" % (byte, failures)


def test_the_instruments_refuse_what_they_must(ctx, ops):
    """dk_dbg_mail_fill: a byte only, and never while a batch is open; dk_dbg_ws_peek: something to read, and no more than the workspace holds"""
    for call in (lambda: ctx.dbg_mail_fill(256), lambda: ctx.dbg_mail_fill(-1), lambda: ctx.dbg_ws_peek(0)):
        assert error_of(call) == DK_E_ARG
    assert error_of(lambda: ctx.dbg_ws_peek(ctx.stats()["ws_size_bytes"] + 1)) == DK_E_NOMEM
    assert len(ctx.dbg_ws_peek(4097)) == 4097
    with ctx.batch_begin("dark", host_threads=1) as bt:
        assert error_of(lambda: ctx.dbg_mail_fill(0)) == DK_E_ARG and error_of(lambda: ctx.dbg_ws_peek(16)) == DK_E_ARG
        bt.finish()
    assert run(ctx, ops, "block_encode") and run(ctx, ops, "bwt_inverse")
