"""The C ABI's boundary, as plain data: what every query entry (LCP, SA check / search, the FM-index family) and the packed stage entries answer
to a faulty argument -- (return code, dk_last_error text) -- and what one valid call of each takes from the workspace and writes.
tests/test_gpu_abi_boundary.py compares run() with tests/golden/abi_boundary.json, which this module wrote when run as a script:

    python tests/abi_boundary_cases.py tests/golden/abi_boundary.json

The table pins the order of the checks (the first one that fails decides code and text), the texts byte for byte, the order and rounding of the
workspace allocations (ws_peak_bytes on a fresh context per valid call) and the results (CRC-32 of every output buffer the call changed).
Everything goes through ctypes on the raw entry points: a refusal has to be provoked with arguments the Python methods would not build."""
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MAX_N, MAX_BLOCKS = 4096, 4
PACKED_MAX_BLOCKS = 65536        # DK_PACKED_MAX_BLOCKS: what a full context allows
FIND_MAX_PAIRS = 1 << 24         # DK_FM_FIND_MAX_PAIRS
SEAM_MAX_PATTERN = 4096          # DK_FM_SEAM_MAX_PATTERN
STEP = 4
BLOCKS = (b"t", b"he quit", (b"he lazy dog and the quick brown fox; the thin moth thaws the path." * 2)[:64])
SIZES = tuple(len(b) for b in BLOCKS)  # 1, 7, 64
PREV = b"mot"
PATTERNS = (b"", b"th")
PAT_BLOCKS = (1, 2)
RANGE_POS, RANGE_LEN = (0, 3), (5, 2)
BUF = 8192  # bytes of every output buffer: far more than any call here writes

DEFAULTS = dict(n=SIZES[2], count=3, ns=SIZES, origin=None, origins=None, index_off=0, aux_off=0, step=STEP, npat=len(PATTERNS),
                pat_len=tuple(len(p) for p in PATTERNS), pat_block=PAT_BLOCKS, cap=8, hits_off=0, prev_len=len(PREV))


def _sizes(xs):
    return None if xs is None else (C.c_size_t * max(len(xs), 1))(*xs)


def _u32(xs):
    return np.array(xs, dtype=np.uint32)


def _hp(a, off=0):
    """address of a host array"""
    return a.ctypes.data + off


class Bag:
    pass


def _kind(torch, ctx, full, blocks):
    """the inputs of one layout (a single block, or the pack): text, L, suffix arrays and the three structures, on the device and on the host"""
    k = Bag()
    k.sizes = [len(b) for b in blocks]
    k.h_text = np.frombuffer(b"".join(blocks), dtype=np.uint8).copy()
    fwd = [full.bwt_forward(b) for b in blocks]
    k.h_bwt = np.concatenate([f[0] for f in fwd])
    k.origins = [f[1] for f in fwd]
    k.h_sa = np.concatenate([full.suffix_array(b) for b in blocks]).astype(np.uint32)
    dev = lambda a: torch.from_numpy(np.array(a)).to("cuda:0")
    k.text, k.bwt, k.sa = dev(k.h_text), dev(k.h_bwt), dev(k.h_sa.view(np.int32))
    total, count = len(k.h_text), len(blocks)
    from dark_amd.context import fm_extract_bytes, fm_index_bytes, fm_locate_bytes
    k.index = torch.zeros(fm_index_bytes(total, count) + 256, dtype=torch.uint8, device="cuda:0")
    k.loc = torch.zeros(fm_locate_bytes(total, count, STEP) + 256, dtype=torch.uint8, device="cuda:0")
    k.ext = torch.zeros(fm_extract_bytes(total, count, STEP) + 256, dtype=torch.uint8, device="cuda:0")
    ctx.dev_fm_build_packed(k.bwt, k.sizes, k.origins, k.index)
    ctx.dev_fm_locate_build_packed(k.bwt, k.sizes, k.origins, STEP, k.loc)
    ctx.dev_fm_extract_build_packed(k.bwt, k.sizes, k.origins, STEP, k.ext)
    # the ranges dk_dev_fm_locate* reads: what the count of PATTERNS gives
    d_pat = dev(np.frombuffer(b"".join(PATTERNS), dtype=np.uint8))
    k.lo, k.hi = torch.zeros(64, dtype=torch.int32, device="cuda:0"), torch.zeros(64, dtype=torch.int32, device="cuda:0")
    blk = PAT_BLOCKS if count > 1 else (0, 0)
    ctx.dev_fm_count_packed(k.bwt, k.sizes, k.index, d_pat, [len(p) for p in PATTERNS], blk, k.lo, k.hi)
    k.epos, k.elen = dev(_u32(RANGE_POS).view(np.int32)), dev(_u32(RANGE_LEN).view(np.int32))
    torch.cuda.synchronize()
    return k


def _outputs(torch):
    """every buffer a call may write: zeroed before a valid call, and those that changed are what the call's record holds"""
    o = Bag()
    o.dev = {name: torch.zeros(BUF, dtype=torch.uint8, device="cuda:0") for name in ("a", "b", "pos", "rows", "hits", "occ", "idx_out", "loc_out",
                                                                                      "ext_out", "bwt_out")}
    o.host = {name: np.zeros(BUF, dtype=np.uint8) for name in ("h_a", "h_b", "h_pos", "h_rows", "h_hits", "h_occ", "total", "verdict", "where",
                                                              "h_origin", "h_m", "h_init")}
    o.pat = torch.from_numpy(np.frombuffer(b"".join(PATTERNS) + b"\0" * 14, dtype=np.uint8).copy()).to("cuda:0")
    o.h_pat = np.frombuffer(b"".join(PATTERNS) + b"\0" * 14, dtype=np.uint8).copy()
    o.prev = torch.from_numpy(np.frombuffer(PREV + b"\0" * (BUF - len(PREV)), dtype=np.uint8).copy()).to("cuda:0")
    o.h_epos, o.h_elen = _u32(RANGE_POS), _u32(RANGE_LEN)
    o.ranksym = torch.from_numpy(np.frombuffer(b"eh", dtype=np.uint8).copy()).to("cuda:0")
    return o


def _zero(o):
    for t in o.dev.values():
        t.zero_()
    for a in o.host.values():
        a[:] = 0


def _changed(torch, o):
    torch.cuda.synchronize()
    zero = zlib.crc32(bytes(BUF))
    out = {}
    for name, t in o.dev.items():
        out[name] = zlib.crc32(t.cpu().numpy().tobytes())
    for name, a in o.host.items():
        out[name] = zlib.crc32(a.tobytes())
    return {name: c for name, c in sorted(out.items()) if c != zero}


# entry -> (layout, features).  Features name the arguments an entry has AND checks: the faults below go to the entries that have all of theirs.
# "fwd": needs the suffix sort's workspace, so a decoder context refuses it whatever the arguments -- recorded there once, with valid arguments.
ENTRIES = {
    "dk_dev_lcp": ("single", {"fwd"}),
    "dk_dev_suffix_array_lcp": ("single", {"fwd"}),
    "dk_suffix_array_lcp": ("single", {"fwd"}),
    "dk_dev_lcp_packed": ("packed", {"fwd"}),
    "dk_dev_suffix_array_packed_lcp": ("packed", {"fwd"}),
    "dk_suffix_array_packed_lcp": ("packed", {"fwd"}),
    "dk_dev_sa_check": ("single", {"fwd"}),
    "dk_sa_check": ("single", {"fwd"}),
    "dk_dev_sa_check_packed": ("packed", {"fwd"}),
    "dk_dev_sa_search": ("single", {"fwd"}),
    "dk_sa_search": ("single", {"fwd"}),
    "dk_dev_sa_search_packed": ("packed", {"fwd", "pat_block"}),
    "dk_dev_fm_build": ("single", {"origin", "index"}),
    "dk_dev_fm_build_packed": ("packed", {"origin", "index"}),
    "dk_dev_fm_count": ("single", {"index"}),
    "dk_dev_fm_count_packed": ("packed", {"index", "pat_block"}),
    "dk_fm_count": ("single", {"origin"}),
    "dk_dev_fm_locate_build": ("single", {"origin", "step", "aux"}),
    "dk_dev_fm_locate_build_packed": ("packed", {"origin", "step", "aux"}),
    "dk_dev_fm_locate": ("single", {"index", "step", "aux", "cap"}),
    "dk_dev_fm_locate_packed": ("packed", {"index", "step", "aux", "cap", "pat_block"}),
    "dk_fm_locate": ("single", {"origin", "step", "cap"}),
    "dk_dev_fm_extract_build": ("single", {"origin", "step", "aux"}),
    "dk_dev_fm_extract_build_packed": ("packed", {"origin", "step", "aux"}),
    "dk_dev_fm_extract": ("single", {"index", "step", "aux", "cap"}),
    "dk_dev_fm_extract_packed": ("packed", {"index", "step", "aux", "cap", "pat_block"}),
    "dk_fm_extract": ("single", {"origin", "step", "cap"}),
    "dk_dev_fm_find": ("single", {"index", "step", "aux", "find", "hits"}),
    "dk_dev_fm_find_packed": ("packed", {"index", "step", "aux", "find", "hits"}),
    "dk_fm_find": ("single", {"origin", "step", "find", "hits"}),  # (host records of any alignment are served: that case records a success)
    "dk_dev_fm_seams": ("single", {"index", "step", "aux", "find", "hits", "seams"}),
    "dk_dev_fm_seams_packed": ("packed", {"index", "step", "aux", "find", "hits", "seams"}),
    "dk_dbg_dev_fm_rank": ("single", {"index"}),
    # the packed stage entries, which describe their blocks the same way
    "dk_dev_bwt_forward_packed": ("packed", {"fwd"}),
    "dk_dev_suffix_array_packed": ("packed", {"fwd"}),
    "dk_suffix_array_packed": ("packed", {"fwd"}),
    "dk_dev_dc_encode_packed": ("packed", {"fwd"}),
    "dk_dev_bwt_inverse_packed": ("packed", {"origin"}),
}


def faults(max_blocks):
    """(name, the layout and features an entry needs, the arguments that differ from a valid call).  The names joined by + violate two checks at
    once: which of the two texts comes back is the order of the checks."""
    over = (1,) * (max_blocks + 1)
    mid_origin = (0, SIZES[1], 0)  # block 1 of the pack: its origin = its size
    return [
        ("empty", {"single"}, dict(n=0)),
        ("over_max_n", {"single"}, dict(n=MAX_N + 1)),
        ("pack_over_max_n", {"packed"}, dict(ns=(64, MAX_N - 96, 64))),
        ("count_zero", {"packed"}, dict(count=0)),
        ("count_over", {"packed"}, dict(count=max_blocks + 1, ns=over)),
        ("null_n", {"packed"}, dict(ns=None)),
        ("empty_mid", {"packed"}, dict(ns=(1, 0, 64))),
        ("origin_eq_n", {"single", "origin"}, dict(origin=SIZES[2])),
        ("origin_eq_n", {"packed", "origin"}, dict(origins=mid_origin)),
        ("index_off1", {"index"}, dict(index_off=1)),
        ("aux_off1", {"aux"}, dict(aux_off=1)),
        ("step_0", {"step"}, dict(step=0)),
        ("step_3", {"step"}, dict(step=3)),
        ("step_8192", {"step"}, dict(step=8192)),
        ("pat_block_count", {"packed", "pat_block"}, dict(pat_block=(0, 3))),
        ("cap_zero", {"cap"}, dict(cap=0)),
        ("npat_over", {"find"}, dict(npat=FIND_MAX_PAIRS + 1)),
        ("hits_off8", {"hits"}, dict(hits_off=8)),
        ("prev_len_max", {"seams"}, dict(prev_len=SEAM_MAX_PATTERN)),
        ("empty+index_off1", {"single", "index"}, dict(n=0, index_off=1)),
        ("count_zero+index_off1", {"packed", "index"}, dict(count=0, index_off=1)),
        ("null_n+count_zero", {"packed"}, dict(ns=None, count=0)),
        ("step_3+origin_eq_n", {"single", "step", "origin"}, dict(step=3, origin=SIZES[2])),
        ("step_3+origin_eq_n", {"packed", "step", "origin"}, dict(step=3, origins=mid_origin)),
        ("empty_mid+origin_eq_n", {"packed", "origin"}, dict(ns=(1, 0, 64), origins=mid_origin)),
        ("step_0+aux_off1", {"step", "aux"}, dict(step=0, aux_off=1)),
        ("index_off1+aux_off1", {"index", "aux"}, dict(index_off=1, aux_off=1)),
        ("over_max_n+step_0", {"single", "step"}, dict(n=MAX_N + 1, step=0)),
        ("pack_over_max_n+step_0", {"packed", "step"}, dict(ns=(64, MAX_N - 96, 64), step=0)),
        ("cap_zero+step_3", {"cap", "step"}, dict(cap=0, step=3)),
        ("cap_zero+empty", {"single", "cap"}, dict(cap=0, n=0)),
        ("pat_block_count+cap_zero", {"packed", "pat_block", "cap"}, dict(pat_block=(0, 3), cap=0)),
        ("pat_block_count+empty_mid", {"packed", "pat_block"}, dict(pat_block=(0, 3), ns=(1, 0, 64))),
        ("npat_over+hits_off8", {"find", "hits"}, dict(npat=FIND_MAX_PAIRS + 1, hits_off=8)),
        ("npat_over+step_3", {"find", "step"}, dict(npat=FIND_MAX_PAIRS + 1, step=3)),
        ("hits_off8+aux_off1", {"hits", "aux"}, dict(hits_off=8, aux_off=1)),
        ("prev_len_max+npat_over", {"seams"}, dict(prev_len=SEAM_MAX_PATTERN, npat=FIND_MAX_PAIRS + 1)),
        ("prev_len_max+hits_off8", {"seams"}, dict(prev_len=SEAM_MAX_PATTERN, hits_off=8)),
    ]


def call(L, h, name, s, p, o, over):
    """one raw call of entry `name` with the valid arguments, `over` laid on top -> its return code"""
    a = dict(DEFAULTS, **over)
    k = s if ENTRIES[name][0] == "single" else p
    n, cnt, ns, step, npat, cap, prev_len = a["n"], a["count"], _sizes(a["ns"]), a["step"], a["npat"], a["cap"], a["prev_len"]
    org = k.origins[0] if a["origin"] is None else a["origin"]
    orgs = _u32(k.origins if a["origins"] is None else a["origins"])
    idx, loc, ext = k.index.data_ptr() + a["index_off"], k.loc.data_ptr() + a["aux_off"], k.ext.data_ptr() + a["aux_off"]
    lens, pblk = _sizes(a["pat_len"]), _u32(a["pat_block"])
    d = {key: t.data_ptr() for key, t in o.dev.items()}
    hh = {key: _hp(v) for key, v in o.host.items()}
    idx_out, loc_out, ext_out = d["idx_out"] + a["index_off"], d["loc_out"] + a["aux_off"], d["ext_out"] + a["aux_off"]
    text, bwt, sa, pat, prev = k.text.data_ptr(), k.bwt.data_ptr(), k.sa.data_ptr(), o.pat.data_ptr(), o.prev.data_ptr()
    h_text, h_bwt, h_sa, h_pat = _hp(k.h_text), _hp(k.h_bwt), _hp(k.h_sa), _hp(o.h_pat)
    lo, hi, epos, elen = k.lo.data_ptr(), k.hi.data_ptr(), k.epos.data_ptr(), k.elen.data_ptr()
    u32p = lambda key: C.cast(hh[key], C.POINTER(C.c_uint32))
    hits, h_hits = d["hits"] + a["hits_off"], hh["h_hits"] + a["hits_off"]
    f = getattr(L, name)
    table = {
        "dk_dev_lcp": lambda: f(h, text, n, sa, d["a"]),
        "dk_dev_suffix_array_lcp": lambda: f(h, text, n, d["a"], d["b"]),
        "dk_suffix_array_lcp": lambda: f(h, h_text, n, hh["h_a"], hh["h_b"]),
        "dk_dev_lcp_packed": lambda: f(h, text, cnt, ns, sa, d["a"]),
        "dk_dev_suffix_array_packed_lcp": lambda: f(h, text, cnt, ns, d["a"], d["b"]),
        "dk_suffix_array_packed_lcp": lambda: f(h, h_text, cnt, ns, hh["h_a"], hh["h_b"]),
        "dk_dev_sa_check": lambda: f(h, text, n, sa, u32p("verdict"), u32p("where")),
        "dk_sa_check": lambda: f(h, h_text, n, h_sa, u32p("verdict"), u32p("where")),
        "dk_dev_sa_check_packed": lambda: f(h, text, cnt, ns, sa, hh["verdict"], hh["where"]),
        "dk_dev_sa_search": lambda: f(h, text, n, sa, pat, npat, lens, d["a"], d["b"]),
        "dk_sa_search": lambda: f(h, h_text, n, h_sa, h_pat, npat, lens, hh["h_a"], hh["h_b"]),
        "dk_dev_sa_search_packed": lambda: f(h, text, cnt, ns, sa, pat, npat, lens, _hp(pblk), d["a"], d["b"]),
        "dk_dev_fm_build": lambda: f(h, bwt, n, org, idx_out),
        "dk_dev_fm_build_packed": lambda: f(h, bwt, cnt, ns, _hp(orgs), idx_out),
        "dk_dev_fm_count": lambda: f(h, bwt, n, idx, pat, npat, lens, d["a"], d["b"]),
        "dk_dev_fm_count_packed": lambda: f(h, bwt, cnt, ns, idx, pat, npat, lens, _hp(pblk), d["a"], d["b"]),
        "dk_fm_count": lambda: f(h, h_bwt, n, org, h_pat, npat, lens, hh["h_a"], hh["h_b"]),
        "dk_dev_fm_locate_build": lambda: f(h, bwt, n, org, step, loc_out),
        "dk_dev_fm_locate_build_packed": lambda: f(h, bwt, cnt, ns, _hp(orgs), step, loc_out),
        "dk_dev_fm_locate": lambda: f(h, bwt, n, idx, loc, step, lo, hi, npat, cap, d["pos"]),
        "dk_dev_fm_locate_packed": lambda: f(h, bwt, cnt, ns, idx, loc, step, lo, hi, npat, _hp(pblk), cap, d["pos"]),
        "dk_fm_locate": lambda: f(h, h_bwt, n, org, step, h_pat, npat, lens, cap, hh["h_a"], hh["h_b"], hh["h_pos"]),
        "dk_dev_fm_extract_build": lambda: f(h, bwt, n, org, step, ext_out),
        "dk_dev_fm_extract_build_packed": lambda: f(h, bwt, cnt, ns, _hp(orgs), step, ext_out),
        "dk_dev_fm_extract": lambda: f(h, bwt, n, idx, ext, step, epos, elen, npat, cap, d["rows"]),
        "dk_dev_fm_extract_packed": lambda: f(h, bwt, cnt, ns, idx, ext, step, epos, elen, npat, _hp(pblk), cap, d["rows"]),
        "dk_fm_extract": lambda: f(h, h_bwt, n, org, step, _hp(o.h_epos), _hp(o.h_elen), npat, cap, hh["h_rows"]),
        "dk_dev_fm_find": lambda: f(h, bwt, n, idx, loc, step, pat, npat, lens, cap, hits, d["occ"], hh["total"]),
        "dk_dev_fm_find_packed": lambda: f(h, bwt, cnt, ns, idx, loc, step, pat, npat, lens, cap, hits, d["occ"], hh["total"]),
        "dk_fm_find": lambda: f(h, h_bwt, n, org, step, h_pat, npat, lens, cap, h_hits, hh["h_occ"], hh["total"]),
        "dk_dev_fm_seams": lambda: f(h, bwt, n, idx, ext, step, prev, prev_len, pat, npat, lens, cap, hits, d["occ"], hh["total"]),
        "dk_dev_fm_seams_packed": lambda: f(h, bwt, cnt, ns, idx, ext, step, prev, prev_len, pat, npat, lens, cap, hits, d["occ"], hh["total"]),
        "dk_dbg_dev_fm_rank": lambda: f(h, bwt, n, idx, hi, o.ranksym.data_ptr(), 2, d["a"]),  # ranks at the two patterns' upper ends
        "dk_dev_bwt_forward_packed": lambda: f(h, text, cnt, ns, d["bwt_out"], u32p("h_origin")),
        "dk_dev_suffix_array_packed": lambda: f(h, text, cnt, ns, d["a"], d["bwt_out"], u32p("h_origin")),
        "dk_suffix_array_packed": lambda: f(h, h_text, cnt, ns, hh["h_a"]),
        "dk_dev_dc_encode_packed": lambda: f(h, bwt, cnt, ns, hh["h_init"], d["a"], d["rows"], d["pos"], C.cast(hh["h_m"], C.POINTER(C.c_size_t))),
        "dk_dev_bwt_inverse_packed": lambda: f(h, bwt, cnt, ns, _hp(orgs), d["rows"]),
    }
    return int(table[name]())


def run():
    """-> {"full": {"refusals": {"entry/fault": [rc, text]}, "valid": {entry: {"rc", "error", "ws_peak_bytes", "crc32": {buffer: value}}}}, "decoder": ...}"""
    import torch
    import dark_amd
    result = {}
    o = _outputs(torch)
    with dark_amd.Context(MAX_N) as full:
        for purpose in ("full", "decoder"):
            make = lambda: dark_amd.Context(MAX_N, purpose=purpose, max_blocks=MAX_BLOCKS)
            refusals, valid = {}, {}
            with make() as ctx:
                L, h = ctx._lib, ctx._h
                s, p = _kind(torch, ctx, full, BLOCKS[2:]), _kind(torch, ctx, full, BLOCKS)
                for name, (layout, feat) in ENTRIES.items():
                    if purpose == "decoder" and "fwd" in feat:
                        continue
                    for fault, need, over in faults(MAX_BLOCKS if purpose == "decoder" else PACKED_MAX_BLOCKS):
                        if need <= feat | {layout}:
                            rc = call(L, h, name, s, p, o, over)
                            refusals["%s/%s" % (name, fault)] = [rc, (L.dk_last_error(h) or b"").decode()]
            for name in ENTRIES:
                with make() as ctx:  # a fresh one: ws_peak_bytes is the context's running maximum
                    L, h = ctx._lib, ctx._h
                    _zero(o)
                    torch.cuda.synchronize()
                    ctx.stats_reset()
                    rc = call(L, h, name, s, p, o, {})
                    valid[name] = {"rc": rc, "error": (L.dk_last_error(h) or b"").decode() if rc else "",
                                   "ws_peak_bytes": int(ctx.stats()["ws_peak_bytes"]), "crc32": _changed(torch, o)}
            result[purpose] = {"refusals": refusals, "valid": valid}
    return result


if __name__ == "__main__":
    data = run()
    with open(sys.argv[1], "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%d refusals, %d valid calls" % (sum(len(v["refusals"]) for v in data.values()), sum(len(v["valid"]) for v in data.values())))
