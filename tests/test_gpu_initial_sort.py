"""The initial sort of the suffix sort by itself, through dk_dbg_dev_initial_sort: ONE sort_pairs() with the text keys and the final destinations
initial_sort() builds -- text_fetch / text_stage / text_tile_keys (both staging paths, the zero padding, the byte in front of tile 0, the
sliding window), k_radix_hist<HS_TEXT> (its own digit, and its prefetch above 1024 tiles), k_radix_scatter's text pass in the plain and the packed
form, the passes behind it, and the last pass's stores to their final homes (SA, L, the origin, wide or narrow keys, the bucket starts) --
bit-exact against tests/initial_sort_model.py (tests/test_initial_sort_model.py pins the model and what every case is built for on the CPU).

End-to-end parity is a weak instrument here: a wrong word in the sorted keys only changes which neighbours the first rerank calls equal, and
later rounds heal most of that; a wrong carried byte shows only where a suffix is final after this sort.

Every device output holds 0xC3 before a call, with 64 guard entries in front and behind, and is compared WHOLE.  The alphabet is the test's: byte
values that are not contiguous, a code table that is a random permutation or not injective at all, and then any inv.  The (bits, spk, carry) grid is
exactly what choose_prefix can choose (tests/initial_sort_cases.py)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

import dark_amd
import initial_sort_cases as K
import rerank_model as R
from conftest import ROOT
from dark_amd._lib import DK_E_ARG
from test_gpu_fallbacks import _call, _env

pytestmark = pytest.mark.gpu
CAP = 1 << 17


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


@pytest.mark.parametrize("name", K.GRID_CASES)
def test_grid(ctx, name):
    """everything choose_prefix can choose, at three tiles and 85 bytes: narrow wherever the sort has at most 40 bits, wide keys as well"""
    c = K.CASES[name]()
    K.check(c, K.call(ctx, c), K.expected(c))


@pytest.mark.parametrize("offset", K.OFFSETS)
@pytest.mark.parametrize("point", sorted(K.POINTS))
def test_sizes_and_alignments(ctx, point, offset):
    """2 bytes to nine tiles, around every edge of a tile and of the staging paths (4175 / 4176, 8271 / 8272), the text 0, 1, 8 and 15 bytes behind
    an aligned address: offset 0 takes the 16-byte loads wherever a tile allows, every other offset goes byte by byte -- the same answer"""
    for n in K.SIZES:
        c = K.sized(point, n, offset)
        K.check(c, K.call(ctx, c), K.expected(c))


def run_large(name, keep=True):
    c = K.large(name)
    t0 = time.time()
    want = K.expected(c, keep=keep)
    t1 = time.time()
    with dark_amd.Context(c.n) as big:
        t2 = time.time()
        got = K.call(big, c)
        t3 = time.time()
    print("%s: n = %d, model %.2f s, context %.2f s, call with copies %.2f s" % (name, c.n, t1 - t0, t2 - t1, t3 - t2))
    K.check(c, got, want)
    return c


@pytest.mark.parametrize("name", ("plane_unpacked_7_passes", "plane_packed_4_passes"))
def test_the_digit_plane(name):
    """2^20 + 1 positions: every pass but the last leaves the next pass's digits in a byte plane, and the next histogram reads them -- behind plain
    pairs, and behind packed ones, whose digits stand at bit 32 and up"""
    c = run_large(name)
    assert c.want_packed == (name == "plane_packed_4_passes") and c.want_passes == (4 if c.want_packed else 7)


@pytest.mark.parametrize("name", ("two_tiles_b56_aligned", "two_tiles_b56_offset_1", "two_tiles_packed_aligned", "two_tiles_packed_offset_1",
                                  "two_tiles_fast_then_slow"))
def test_two_tiles_per_histogram_workgroup(name):
    """1028 tiles: a workgroup of the text histogram walks two, and asks for the second one's bytes before it counts the first -- the only place that
    prefetch runs.  Aligned (16-byte loads) and one byte off (none).  fast_then_slow: the size at which the last workgroup's first tile takes the
    16-byte loads and its second, the text's last 85 bytes, cannot"""
    run_large(name)


@pytest.mark.parametrize("name", ("edge_packed_2_24", "edge_unpacked_2_24_plus_1"))
def test_the_packed_words_last_bit(name):
    """bits = 8 with the carry: at 2^24 positions code and position fill the packed pair's low word to the last bit, at 2^24 + 1 the sort must take
    plain pairs -- the route says which; narrow keys both times"""
    c = run_large(name, keep=False)
    assert c.want_packed == (name == "edge_packed_2_24")


@pytest.mark.parametrize("name", K.HANDOFF)
def test_the_first_rerank_takes_what_the_sort_leaves(ctx, name):
    """the narrow words and the bucket starts handed to dk_dbg_dev_rerank as a first rerank give the list, the groups and the counts that
    tests/rerank_model.py finds from the model's WIDE keys above the carried byte"""
    c = K.CASES[name]()
    got = K.call(ctx, c)
    n, p = c.n, K.PAD
    words, sa, bwt = got["keys"][p:p + n], got["sa"][p:p + n], got["bwt"][p:p + n]
    res = ctx.dbg_dev_rerank(words, sa, bucket_starts=got["bucket_starts"], bwt=bwt)
    m = K.expected(c)
    want = R.rerank_model(m.wide_keys, m.sa, cmp_shift=8, bwt=m.bwt)
    assert res["counts"] == want.counts and want.active > 0 and want.groups > 1, (res["counts"], want.counts)
    for what in ("out_idx", "out_pos", "out_gid", "sym_out"):
        K.same(name, what, res[what][:want.active], getattr(want, what))
    K.same(name, "gstart", res["gstart"][:want.groups + 1], want.gstart)


def test_refusals_leave_every_array_untouched(ctx):
    lib, h = ctx._lib, ctx._h
    n = 5000
    filled = lambda nbytes: torch.full((nbytes,), 0xC3, dtype=torch.uint8, device="cuda")  # noqa: E731
    bufs = dict(keys=filled(8 * n), sa=filled(4 * n), bwt=filled(n), origin=filled(4))
    text = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    code, inv = np.full(256, 3, np.uint8), np.arange(256, dtype=np.uint8)
    starts, out = np.full(256, K.FILL32, np.uint32), np.full(4, K.FILL32, np.uint32)
    torch.cuda.synchronize()
    p = {k: C.c_void_p(v.data_ptr()) for k, v in bufs.items()}
    hp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    plain = dict(inv=None, bwt=None, origin=None)

    def call(ctx_h=h, text_p=C.c_void_p(text.data_ptr()), n=n, code_p=hp(code), bits=2, spk=8, narrow=0, starts_p=None, out_p=hp(out), **over):
        a = dict(dict(p, inv=hp(inv)), **over)
        return lib.dk_dbg_dev_initial_sort(ctx_h, text_p, n, code_p, bits, spk, a["inv"], narrow, a["keys"], a["sa"], a["bwt"], a["origin"], starts_p, out_p)

    wide_code = np.full(256, 3, np.uint8)
    wide_code[200] = 4
    refused = [("null context", dict(ctx_h=None)), ("null text", dict(text_p=None)), ("null code", dict(code_p=None)), ("null keys", dict(keys=None)),
               ("null sa", dict(sa=None)), ("null out", dict(out_p=None)), ("n = 0", dict(n=0)), ("n above the capacity", dict(n=CAP + 1)),
               ("n above 2^31 - 2", dict(n=(1 << 31) - 1)), ("bits 0", dict(bits=0)), ("bits 9", dict(bits=9, spk=1)), ("spk 0", dict(spk=0)),
               ("65 bits", dict(plain, bits=5, spk=13)), ("57 bits and the carry", dict(bits=3, spk=19)), ("64 bits and the carry", dict(bits=8, spk=8)),
               ("a code of three bits under bits = 2", dict(code_p=hp(wide_code))), ("a code of two bits under bits = 1", dict(bits=1)),
               ("inv alone", dict(bwt=None, origin=None)), ("no inv", dict(inv=None)), ("no d_bwt", dict(bwt=None)), ("no d_origin", dict(origin=None)),
               ("narrow 2", dict(narrow=2, starts_p=hp(starts))), ("narrow above 40 bits", dict(bits=2, spk=21, narrow=1, starts_p=hp(starts))),
               ("narrow without a place for the bucket starts", dict(narrow=1)), ("bucket starts without narrow", dict(starts_p=hp(starts)))]
    for name, over in refused:
        assert call(**over) == DK_E_ARG, name
    assert b"initial_sort" in lib.dk_last_error(h)
    with ctx.batch_begin("dark", host_threads=1):
        assert call() == DK_E_ARG, "an open batch"
    assert b"batch" in lib.dk_last_error(h)
    with dark_amd.Context(n, purpose="decoder") as dec:
        assert call(ctx_h=dec._h) == DK_E_ARG and b"decoder context" in lib.dk_last_error(dec._h)
    torch.cuda.synchronize()
    for name, t in bufs.items():
        assert bool((t == 0xC3).all()), "a refused call wrote to " + name
    assert (starts == K.FILL32).all() and (out == K.FILL32).all()
    assert call(**plain) == 0 and call() == 0 and call(narrow=1, starts_p=hp(starts)) == 0  # the same arguments, served: the refusals were the arguments'
    for name in ("grid_b2_k16_carry_narrow", "grid_b8_k7_carry_wide"):  # ... and the context serves the next calls
        c = K.CASES[name]()
        K.check(c, K.call(ctx, c), K.expected(c))


def test_a_context_of_exactly_n():
    """the four sort buffers and the sort's tables fit a context whose capacity is n"""
    c = K.CASES["grid_b8_k8_plain_wide"]()
    with dark_amd.Context(c.n) as small:
        K.check(c, K.call(small, c), K.expected(c))


SETTINGS = {
    "unpacked": (dict(DK_PACKED_SORT=0), dict(packed_sort=False)),             # the plain form of the sorts of at most 32 bits, at small n
    "packed_wide": (dict(DK_PACKED_SORT=1, DK_NARROW_KEYS=0), dict(wide=True)),  # (the knob acts in choose_prefix: the entry's caller asks for wide keys)
    "no_xcd": (dict(DK_XCD=0), {}),
    "no_plane": (dict(DK_DIGIT_PLANE=0), dict(large=["plane_unpacked_7_passes", "plane_packed_4_passes"])),
    "scatter_512": (dict(DK_SCATTER_BLOCK=512), {}),
    "poison": (dict(DK_POISON=165), dict(poison=165, mail_fill=165)),
}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_tuning_build(setting):
    """a short list of the cases in a process of its own on the tuning library, per setting of its knobs: the plain form of the packed sorts, wide
    keys behind packed pairs, no XCD tile order, no digit plane at 2^20 + 1, the scatter of 512 threads, and DK_POISON=165 (proved to be in
    force, every workspace allocation filled with 0xA5 first) behind dk_dbg_mail_fill(0xA5) -- the model's answer every time, with the route the
    model predicts for the setting"""
    knobs, spec = SETTINGS[setting]
    cmd = [sys.executable, os.path.join(ROOT, "tests", "initial_sort_worker.py"), ROOT, json.dumps(dict(spec, cases=list(K.WORKER)))]
    p = _call(cmd, _env(knobs), " ".join("%s=%s" % kv for kv in sorted(knobs.items())))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout + p.stderr
    res = json.loads(line[-1][7:])
    assert sorted(res) == sorted(list(K.WORKER) + spec.get("large", []))
    packed = [name for name, r in res.items() if r["packed"]]
    want = [] if setting == "unpacked" else [name for name in res if (K.CASES[name]() if name in K.CASES else K.large(name)).want_packed]
    assert sorted(packed) == sorted(want) and (setting == "unpacked" or len(want) >= 3), (setting, packed)
