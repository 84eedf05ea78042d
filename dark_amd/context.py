"""dk_ctx wrapper: one (host thread, GPU) pair owning the device workspace -- the role saca::Constructor's storage
(src/saca.rs:344-384) and block::dc::{Encoder,Decoder}'s buffers (src/block/dc.rs:21-26,96-102) play in the reference."""
import ctypes as C

import numpy as np

from . import _lib


class DarkError(RuntimeError):
    def __init__(self, code, text=""):
        self.code = code
        super().__init__("%s (%d)%s" % (_lib.ERROR_NAMES.get(code, "error"), code, (": " + text) if text else ""))


def _ptr(a):
    """host numpy array or device tensor / raw int -> void*"""
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(int(a))


def _inputs_ready(*tensors):
    """Stream contract of the dk_dev_ entry points (include/dark_amd.h): device inputs must be complete before the call -- the library
    runs on its own non-blocking stream and does not wait for the caller's.  For torch tensors: drain torch's current stream."""
    for t in tensors:
        if hasattr(t, "is_cuda") and t.is_cuda:
            import torch
            torch.cuda.current_stream(t.device).synchronize()
            return


def as_u8(x):
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x, dtype=np.uint8)
    return np.frombuffer(bytes(x), dtype=np.uint8)


def _pack_patterns(patterns):
    """a list of byte strings -> (the bytes back to back, their lengths as size_t[], how many)"""
    keep = [as_u8(p) for p in patterns]
    npat = len(keep)
    pat = np.concatenate(keep) if npat else np.zeros(0, dtype=np.uint8)
    if len(pat) == 0:
        pat = np.zeros(1, dtype=np.uint8)  # (never read: every pattern is empty)
    return pat, _sizes([len(p) for p in keep]), npat


def _sizes(xs):
    """lengths of blocks or patterns -> size_t[], of one element at least (an empty list still needs an address)"""
    return (C.c_size_t * max(len(xs), 1))(*[int(n) for n in xs])


def _u32s(xs):
    """origins or block numbers -> a uint32 array, of one element at least"""
    return np.array(xs, dtype=np.int64).astype(np.uint32) if len(xs) else np.zeros(1, np.uint32)


def _same_length(xs, what, count, of):
    """one of `xs` for every one of the `count` things they belong to"""
    if len(xs) != count:
        raise DarkError(_lib.DK_E_ARG, "%d %s for %d %s" % (len(xs), what, count, of))


def model_id(m):
    if isinstance(m, str):
        if m not in _lib.MODEL_IDS:
            raise DarkError(_lib.DK_E_MODEL, "unknown model %r" % m)
        return _lib.MODEL_IDS[m]
    return int(getattr(m, "MODEL_ID", m))


def _prefix(mid):
    """bytes the any-byte flag puts in front of a coded stream"""
    return 4 if mid & _lib.DK_MODEL_ANYBYTE else 0


def _stream_cap(mid, n):
    """output bound of one coded block: 10-byte records for rawdc, else 2 n + 4096, plus the any-byte prefix"""
    return (10 if mid == _lib.MODEL_IDS["rawdc"] else 2) * int(n) + 4096 + _prefix(mid)


def workspace_bytes(purpose, n, max_blocks=1):
    """dk_workspace_bytes: the device workspace a Context(n, purpose=purpose, max_blocks=max_blocks) allocates; needs no GPU.
    0 for arguments no context can be made with."""
    if purpose not in _lib.PURPOSES:
        return 0
    return int(_lib.load().dk_workspace_bytes(_lib.PURPOSES[purpose], int(n), int(max_blocks)))


def fm_index_bytes(total, count=1):
    """dk_fm_index_bytes: bytes of the FM-index of a pack of `count` blocks and `total` bytes; needs no GPU.  0 for what the pack checks refuse."""
    if total < 0 or count < 0:
        return 0
    return int(_lib.load().dk_fm_index_bytes(int(total), int(count)))


def fm_locate_bytes(total, count=1, step=32):
    """dk_fm_locate_bytes: bytes of the locate structure beside that index at sampling step `step`; needs no GPU.  0 for what fm_index_bytes
    refuses and for a step that is no power of two in [1, 4096]."""
    if total < 0 or count < 0 or not 0 <= step < 2 ** 32:
        return 0
    return int(_lib.load().dk_fm_locate_bytes(int(total), int(count), int(step)))


def fm_extract_bytes(total, count=1, step=32):
    """dk_fm_extract_bytes: bytes of the extract structure beside that index at anchor distance `step`; needs no GPU.  0 for what fm_index_bytes
    refuses and for a step that is no power of two in [1, 4096]."""
    if total < 0 or count < 0 or not 0 <= step < 2 ** 32:
        return 0
    return int(_lib.load().dk_fm_extract_bytes(int(total), int(count), int(step)))


# dk_fm_hit: a record of dk_dev_fm_find* (16 bytes)
FM_HIT_DTYPE = np.dtype([("pattern", np.uint32), ("block", np.uint32), ("position", np.uint32), ("slot", np.uint32)])
# dk_fm_seam_hit: a record of dk_dev_fm_seams* (16 bytes)
FM_SEAM_HIT_DTYPE = np.dtype([("pattern", np.uint32), ("block", np.uint32), ("back", np.uint32), ("reserved", np.uint32)])
# dk_fm_near_hit: a record of dk_dev_fm_near* (16 bytes)
FM_NEAR_HIT_DTYPE = np.dtype([("pattern", np.uint32), ("block", np.uint32), ("position", np.uint32), ("cost", np.uint32)])
# dk_sa_smem: a record of dk_dev_sa_smems* (16 bytes)
SA_SMEM_DTYPE = np.dtype([("at", np.uint32), ("len", np.uint32), ("lo", np.uint32), ("hi", np.uint32)])
FM_NEAR_MAX_PATTERN, FM_NEAR_MAX_K, FM_NEAR_NODE_LIMIT = _lib.FM_NEAR_MAX_PATTERN, _lib.FM_NEAR_MAX_K, _lib.FM_NEAR_NODE_LIMIT


class Context:
    def __init__(self, max_n, device=0, purpose="full", max_blocks=1):
        """purpose="decoder": a context for the inverse path only (dk_ctx_create_decoder), about a fifth of the workspace; max_blocks = most
        blocks one of its packed calls may hold.  A full context ignores max_blocks."""
        if purpose not in _lib.PURPOSES:
            raise DarkError(_lib.DK_E_ARG, "unknown context purpose %r" % (purpose,))
        self._lib = _lib.load()
        h = C.c_void_p()
        if purpose == "decoder":
            rc = self._lib.dk_ctx_create_decoder(int(device), int(max_n), int(max_blocks), C.byref(h))
            what = "dk_ctx_create_decoder(device=%d, max_n=%d, max_blocks=%d)" % (device, max_n, max_blocks)
        else:
            rc = self._lib.dk_ctx_create(int(device), int(max_n), C.byref(h))
            what = "dk_ctx_create(device=%d, max_n=%d)" % (device, max_n)
        if rc != 0:
            raise DarkError(rc, what)
        self._h = h
        self._batch = None  # the streaming Batch open on this context, if any
        self.device = device
        self.purpose = purpose

    def close(self):
        if getattr(self, "_h", None):
            b = getattr(self, "_batch", None)
            if b is not None:
                b.close()  # joins its coding threads before the staging memory goes (dk_ctx_destroy would do the same)
            self._lib.dk_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc):
        if rc != 0:
            raise DarkError(rc, (self._lib.dk_last_error(self._h) or b"").decode())

    def capacity(self):
        return int(self._lib.dk_capacity(self._h))

    def last_consumed(self):
        return int(self._lib.dk_last_consumed(self._h))

    def last_block_flags(self):
        """DK_FLAG_HAS_FF (1): the last block encode's input held byte 0xFF -> its stream cannot be decoded (reference format)"""
        return int(self._lib.dk_last_block_flags(self._h))

    # ---- host-pointer stage calls ----
    def suffix_array(self, data):
        t = as_u8(data)
        sa = np.empty(len(t), dtype=np.uint32)
        self._ck(self._lib.dk_suffix_array(self._h, _ptr(t), len(t), _ptr(sa)))
        return sa

    def suffix_array_packed(self, blocks):
        """the suffix array of every block (entries local to the block), all of them from one segmented device pass"""
        keep = [as_u8(b) for b in blocks]
        count = len(keep)
        ns = _sizes([len(b) for b in keep])
        t = np.concatenate(keep) if count else np.zeros(0, dtype=np.uint8)
        sa = np.empty(len(t), dtype=np.uint32)
        self._ck(self._lib.dk_suffix_array_packed(self._h, _ptr(t), count, ns, _ptr(sa)))
        ends = np.cumsum([len(b) for b in keep])
        return [sa[e - len(b):e] for b, e in zip(keep, ends)]

    def suffix_array_lcp(self, data):
        """(suffix array, LCP array): LCP[0] = 0, LCP[i] = leading bytes the suffixes SA[i-1] and SA[i] share (dk_suffix_array_lcp)"""
        t = as_u8(data)
        sa = np.empty(len(t), dtype=np.uint32)
        lcp = np.empty(len(t), dtype=np.uint32)
        self._ck(self._lib.dk_suffix_array_lcp(self._h, _ptr(t), len(t), _ptr(sa), _ptr(lcp)))
        return sa, lcp

    def suffix_array_packed_lcp(self, blocks):
        """(suffix array, LCP array) of every block, all of them from one segmented device pass (dk_suffix_array_packed_lcp)"""
        keep = [as_u8(b) for b in blocks]
        count = len(keep)
        ns = _sizes([len(b) for b in keep])
        t = np.concatenate(keep) if count else np.zeros(0, dtype=np.uint8)
        sa = np.empty(len(t), dtype=np.uint32)
        lcp = np.empty(len(t), dtype=np.uint32)
        self._ck(self._lib.dk_suffix_array_packed_lcp(self._h, _ptr(t), count, ns, _ptr(sa), _ptr(lcp)))
        ends = np.cumsum([len(b) for b in keep])
        return [(sa[e - len(b):e], lcp[e - len(b):e]) for b, e in zip(keep, ends)]

    def sa_check(self, data, sa):
        """is `sa` the suffix array of `data`?  -> (verdict, where): verdict one of _lib.SA_VERDICTS ("ok", "bad_range", "not_permutation",
        "bad_order"), where = the lowest slot / text position at fault (len(data) with "ok") (dk_sa_check)"""
        t = as_u8(data)
        sa = np.ascontiguousarray(sa, dtype=np.uint32)
        _same_length(sa, "entries", len(t), "bytes")
        verdict, where = C.c_uint32(0), C.c_uint32(0)
        self._ck(self._lib.dk_sa_check(self._h, _ptr(t), len(t), _ptr(sa), C.byref(verdict), C.byref(where)))
        return _lib.SA_VERDICTS[verdict.value], int(where.value)

    def sa_search(self, data, sa, patterns):
        """(lo, hi) per pattern, uint32 arrays: sa[lo[q]:hi[q]] are exactly the places patterns[q] occurs in `data`; lo == hi = the insertion
        slot of a pattern that does not occur (dk_sa_search).  The suffix array is trusted: sa_check verifies one."""
        t = as_u8(data)
        sa = np.ascontiguousarray(sa, dtype=np.uint32)
        _same_length(sa, "entries", len(t), "bytes")
        pat, lens, npat = _pack_patterns(patterns)
        lo, hi = np.zeros(npat, dtype=np.uint32), np.zeros(npat, dtype=np.uint32)
        self._ck(self._lib.dk_sa_search(self._h, _ptr(t), len(t), _ptr(sa), _ptr(pat), npat, lens, _ptr(lo), _ptr(hi)))
        return lo, hi

    def bwt_forward(self, data):
        t = as_u8(data)
        out = np.empty(len(t), dtype=np.uint8)
        origin = C.c_uint32(0)
        self._ck(self._lib.dk_bwt_forward(self._h, _ptr(t), len(t), _ptr(out), C.byref(origin)))
        return out, int(origin.value)

    def bwt_inverse(self, bwt, origin):
        b = as_u8(bwt)
        out = np.empty(len(b), dtype=np.uint8)
        self._ck(self._lib.dk_bwt_inverse(self._h, _ptr(b), len(b), int(origin), _ptr(out)))
        return out

    def dc_encode(self, bwt):
        b = as_u8(bwt)
        n = len(b)
        init = np.empty(256, dtype=np.uint32)
        d = np.empty(n, dtype=np.uint32)
        sym = np.empty(n, dtype=np.uint8)
        rank = np.empty(n, dtype=np.uint8)
        m = C.c_size_t(0)
        self._ck(self._lib.dk_dc_encode(self._h, _ptr(b), n, _ptr(init), _ptr(d), _ptr(sym), _ptr(rank), C.byref(m)))
        m = m.value
        return dict(init=init, d=d[:m].copy(), sym=sym[:m].copy(), rank=rank[:m].copy())

    def dc_decode(self, init, d, n):
        init = np.ascontiguousarray(init, dtype=np.uint32)
        d = np.ascontiguousarray(d, dtype=np.uint32)
        out = np.empty(n, dtype=np.uint8)
        used = C.c_size_t(0)
        self._ck(self._lib.dk_dc_decode(self._h, _ptr(init), _ptr(d), len(d), _ptr(out), n, C.byref(used)))
        return out, used.value

    def block_encode(self, model, data):
        t = as_u8(data)
        n = len(t)
        mid = model_id(model)
        cap = 10 * (n + 600) if mid == _lib.MODEL_IDS["rawdc"] else _stream_cap(mid, n)
        out = np.empty(cap, dtype=np.uint8)
        ln = C.c_size_t(0)
        self._ck(self._lib.dk_block_encode(self._h, mid, _ptr(t), n, _ptr(out), cap, C.byref(ln)))
        return out[:ln.value].tobytes()

    def block_encode_into(self, model, data, out):
        """dk_block_encode with a caller-owned output array (no copy of the stream): `data` is host memory -- pageable or pinned --
        and the H2D copy is part of the call (stats()["ms_h2d"]); returns a view of `out`"""
        t = as_u8(data)
        ln = C.c_size_t(0)
        self._ck(self._lib.dk_block_encode(self._h, model_id(model), _ptr(t), len(t), _ptr(out), len(out), C.byref(ln)))
        return out[:ln.value]

    def block_decode(self, model, stream, n):
        s = as_u8(stream)
        out = np.empty(n, dtype=np.uint8)
        self._ck(self._lib.dk_block_decode(self._h, model_id(model), _ptr(s), len(s), n, _ptr(out)))
        return out.tobytes()

    def raw_block_encode_dump(self, data, raw_model=0):
        """block::raw::Encoder with the dump model Out (src/block/raw.rs:35-59, src/model/raw.rs:46-76) -> what lands in ./out.raw"""
        t = as_u8(data)
        n = len(t)
        out = np.empty(8, dtype=np.uint8)
        dump = np.empty(n + 4, dtype=np.uint8)
        ln, dl = C.c_size_t(0), C.c_size_t(0)
        self._ck(self._lib.dk_raw_block_encode(self._h, int(raw_model), _ptr(t), n, _ptr(out), len(out), C.byref(ln), _ptr(dump), len(dump), C.byref(dl)))
        assert ln.value == 4 and not out[:4].any()
        return dump[:dl.value].tobytes()

    def raw_block_encode(self, data, raw_model=1):
        """block::raw::Encoder with a coding RawModel (1 = bbb) -> coded stream"""
        t = as_u8(data)
        n = len(t)
        out = np.empty(2 * n + 4096, dtype=np.uint8)
        ln, dl = C.c_size_t(0), C.c_size_t(0)
        self._ck(self._lib.dk_raw_block_encode(self._h, int(raw_model), _ptr(t), n, _ptr(out), len(out), C.byref(ln), None, 0, C.byref(dl)))
        return out[:ln.value].tobytes()

    def raw_block_decode(self, stream, n, raw_model=0):
        s = as_u8(stream)
        out = np.empty(n, dtype=np.uint8)
        self._ck(self._lib.dk_raw_block_decode(self._h, int(raw_model), _ptr(s), len(s), n, _ptr(out)))
        return out.tobytes()

    # ---- device-resident calls (torch tensors or raw device addresses) ----
    def dev_suffix_array(self, d_in, n, d_sa_out):
        _inputs_ready(d_in)
        self._ck(self._lib.dk_dev_suffix_array(self._h, _ptr(d_in), n, _ptr(d_sa_out)))

    def dev_bwt_forward(self, d_in, n, d_bwt_out):
        _inputs_ready(d_in)
        origin = C.c_uint32(0)
        self._ck(self._lib.dk_dev_bwt_forward(self._h, _ptr(d_in), n, _ptr(d_bwt_out), C.byref(origin)))
        return int(origin.value)

    def dev_bwt_inverse(self, d_bwt, n, origin, d_out):
        _inputs_ready(d_bwt)
        self._ck(self._lib.dk_dev_bwt_inverse(self._h, _ptr(d_bwt), n, int(origin), _ptr(d_out)))

    def dev_dc_encode(self, d_bwt, n, d_dist, d_sym, d_rank=None):
        _inputs_ready(d_bwt)
        init = np.empty(256, dtype=np.uint32)
        m = C.c_size_t(0)
        self._ck(self._lib.dk_dev_dc_encode(self._h, _ptr(d_bwt), n, _ptr(init), _ptr(d_dist), _ptr(d_sym),
                                            _ptr(d_rank) if d_rank is not None else None, C.byref(m)))
        return init, m.value

    # ---- packed forward path: blocks back to back in one uint8 device tensor, `sizes` = their lengths in order ----
    def dev_bwt_forward_packed(self, d_in, sizes, d_bwt_out):
        """L of every block into d_bwt_out (same layout as d_in); returns the list of origins"""
        _inputs_ready(d_in)
        count = len(sizes)
        ns = _sizes(sizes)
        origin = np.zeros(max(count, 1), dtype=np.uint32)
        self._ck(self._lib.dk_dev_bwt_forward_packed(self._h, _ptr(d_in), count, ns, _ptr(d_bwt_out),
                                                     origin.ctypes.data_as(C.POINTER(C.c_uint32))))
        return [int(o) for o in origin[:count]]

    def dev_suffix_array_packed(self, d_in, sizes, d_sa_out, d_bwt_out=None):
        """the suffix array of every block into d_sa_out (uint32, same layout as d_in, entries local to the block); with d_bwt_out also L
        of every block, from the same pass: returns the list of origins then, else None"""
        _inputs_ready(d_in)
        count = len(sizes)
        ns = _sizes(sizes)
        if d_bwt_out is None:
            self._ck(self._lib.dk_dev_suffix_array_packed(self._h, _ptr(d_in), count, ns, _ptr(d_sa_out), None, None))
            return None
        origin = np.zeros(max(count, 1), dtype=np.uint32)
        self._ck(self._lib.dk_dev_suffix_array_packed(self._h, _ptr(d_in), count, ns, _ptr(d_sa_out), _ptr(d_bwt_out),
                                                      origin.ctypes.data_as(C.POINTER(C.c_uint32))))
        return [int(o) for o in origin[:count]]

    # ---- LCP arrays (uint32 device tensors) ----
    def dev_lcp(self, d_in, n, d_sa, d_lcp_out):
        """d_lcp_out[i] = leading bytes the suffixes d_sa[i-1] and d_sa[i] of d_in[0, n) share, d_lcp_out[0] = 0"""
        _inputs_ready(d_in, d_sa)
        self._ck(self._lib.dk_dev_lcp(self._h, _ptr(d_in), n, _ptr(d_sa), _ptr(d_lcp_out)))

    def dev_suffix_array_lcp(self, d_in, n, d_sa_out, d_lcp_out):
        """dev_suffix_array, then dev_lcp on its result, in one call"""
        _inputs_ready(d_in)
        self._ck(self._lib.dk_dev_suffix_array_lcp(self._h, _ptr(d_in), n, _ptr(d_sa_out), _ptr(d_lcp_out)))

    def dev_lcp_packed(self, d_in, sizes, d_sa, d_lcp_out):
        """the LCP array of every block of a pack (layout of dev_suffix_array_packed: entries of d_sa local to their block) in one pass"""
        _inputs_ready(d_in, d_sa)
        count = len(sizes)
        ns = _sizes(sizes)
        self._ck(self._lib.dk_dev_lcp_packed(self._h, _ptr(d_in), count, ns, _ptr(d_sa), _ptr(d_lcp_out)))

    def dev_suffix_array_packed_lcp(self, d_in, sizes, d_sa_out, d_lcp_out):
        """dev_suffix_array_packed (without L), then the LCP arrays from the same sort's ranks, in one call"""
        _inputs_ready(d_in)
        count = len(sizes)
        ns = _sizes(sizes)
        self._ck(self._lib.dk_dev_suffix_array_packed_lcp(self._h, _ptr(d_in), count, ns, _ptr(d_sa_out), _ptr(d_lcp_out)))

    # ---- suffix-array check and search ----
    def dev_sa_check(self, d_in, n, d_sa):
        """is d_sa[0, n) the suffix array of d_in[0, n)?  -> (verdict, where) as from sa_check"""
        _inputs_ready(d_in, d_sa)
        verdict, where = C.c_uint32(0), C.c_uint32(0)
        self._ck(self._lib.dk_dev_sa_check(self._h, _ptr(d_in), n, _ptr(d_sa), C.byref(verdict), C.byref(where)))
        return _lib.SA_VERDICTS[verdict.value], int(where.value)

    def dev_sa_check_packed(self, d_in, sizes, d_sa):
        """every block of a pack (layout of dev_suffix_array_packed) in one pass -> a list of (verdict, where), where local to the block"""
        _inputs_ready(d_in, d_sa)
        count = len(sizes)
        ns = _sizes(sizes)
        verdict, where = np.zeros(max(count, 1), dtype=np.uint32), np.zeros(max(count, 1), dtype=np.uint32)
        self._ck(self._lib.dk_dev_sa_check_packed(self._h, _ptr(d_in), count, ns, _ptr(d_sa), _ptr(verdict), _ptr(where)))
        return [(_lib.SA_VERDICTS[int(v)], int(w)) for v, w in zip(verdict[:count], where[:count])]

    def dev_sa_search(self, d_in, n, d_sa, d_pat, pat_lens, d_lo, d_hi):
        """pattern q = the next pat_lens[q] bytes of the uint8 device tensor d_pat; d_lo[q] / d_hi[q] (uint32 device tensors): d_sa[lo:hi] are its
        occurrences in d_in[0, n)"""
        _inputs_ready(d_in, d_sa, d_pat)
        npat = len(pat_lens)
        lens = _sizes(pat_lens)
        self._ck(self._lib.dk_dev_sa_search(self._h, _ptr(d_in), n, _ptr(d_sa), _ptr(d_pat), npat, lens, _ptr(d_lo), _ptr(d_hi)))

    def dev_sa_search_packed(self, d_in, sizes, d_sa, d_pat, pat_lens, pat_blocks, d_lo, d_hi):
        """dev_sa_search in a pack: pattern q is searched in block pat_blocks[q], d_lo / d_hi are local to that block"""
        _inputs_ready(d_in, d_sa, d_pat)
        count, npat = len(sizes), len(pat_lens)
        _same_length(pat_blocks, "blocks", npat, "patterns")
        ns = _sizes(sizes)
        lens = _sizes(pat_lens)
        blocks = _u32s(pat_blocks)
        self._ck(self._lib.dk_dev_sa_search_packed(self._h, _ptr(d_in), count, ns, _ptr(d_sa), _ptr(d_pat), npat, lens, _ptr(blocks), _ptr(d_lo),
                                                   _ptr(d_hi)))

    # ---- matching statistics and super-maximal matches ----
    def dev_sa_match(self, d_in, n, d_sa, d_query, query_lens, max_len, d_len, d_lo=None, d_hi=None):
        """query j = the next query_lens[j] bytes of the uint8 device tensor d_query; for every position g of the queries, d_len[g] = the longest
        prefix of its window (at most max_len bytes, inside its query) that occurs in d_in[0, n), d_lo[g] / d_hi[g] (both or neither) = what
        dev_sa_search gives for that prefix (uint32 device tensors of sum(query_lens) entries)"""
        _inputs_ready(d_in, d_sa, d_query)
        self._ck(self._lib.dk_dev_sa_match(self._h, _ptr(d_in), n, _ptr(d_sa), _ptr(d_query), len(query_lens), _sizes(query_lens), int(max_len),
                                           _ptr(d_len), None if d_lo is None else _ptr(d_lo), None if d_hi is None else _ptr(d_hi)))

    def dev_sa_match_packed(self, d_in, sizes, d_sa, d_query, query_lens, query_blocks, max_len, d_len, d_lo=None, d_hi=None):
        """dev_sa_match in a pack: query j is matched against block query_blocks[j], d_lo / d_hi are local to that block"""
        _inputs_ready(d_in, d_sa, d_query)
        _same_length(query_blocks, "blocks", len(query_lens), "queries")
        blocks = _u32s(query_blocks)
        self._ck(self._lib.dk_dev_sa_match_packed(self._h, _ptr(d_in), len(sizes), _sizes(sizes), _ptr(d_sa), _ptr(d_query), len(query_lens),
                                                  _sizes(query_lens), _ptr(blocks), int(max_len), _ptr(d_len), None if d_lo is None else _ptr(d_lo),
                                                  None if d_hi is None else _ptr(d_hi)))

    def sa_match(self, data, sa, queries, max_len):
        """(len, lo, hi), uint32 arrays over the positions of the queries back to back, from host memory (dk_sa_match)"""
        t = as_u8(data)
        sa = np.ascontiguousarray(sa, dtype=np.uint32)
        _same_length(sa, "entries", len(t), "bytes")
        qry, lens, nq = _pack_patterns(queries)
        total = sum(int(x) for x in lens[:nq])
        out = [np.zeros(total, dtype=np.uint32) for _ in range(3)]
        self._ck(self._lib.dk_sa_match(self._h, _ptr(t), len(t), _ptr(sa), _ptr(qry), nq, lens, int(max_len), *[_ptr(x) for x in out]))
        return tuple(out)

    def dev_sa_smems(self, d_in, n, d_sa, d_query, query_lens, min_len, max_len, max_hits, d_hits):
        """the super-maximal matches of the queries in d_in[0, n): d_hits (a 16-byte aligned device tensor of max_hits records of four uint32
        words: at, len, lo, hi) receives the first min(total, max_hits) in rising order of at; returns the total.  max_hits == 0: d_hits may be None"""
        _inputs_ready(d_in, d_sa, d_query)
        total = C.c_uint64(0)
        self._ck(self._lib.dk_dev_sa_smems(self._h, _ptr(d_in), n, _ptr(d_sa), _ptr(d_query), len(query_lens), _sizes(query_lens), int(min_len),
                                           int(max_len), int(max_hits), None if d_hits is None else _ptr(d_hits), C.byref(total)))
        return int(total.value)

    def dev_sa_smems_packed(self, d_in, sizes, d_sa, d_query, query_lens, query_blocks, min_len, max_len, max_hits, d_hits):
        """dev_sa_smems in a pack: query j against block query_blocks[j]"""
        _inputs_ready(d_in, d_sa, d_query)
        _same_length(query_blocks, "blocks", len(query_lens), "queries")
        blocks = _u32s(query_blocks)
        total = C.c_uint64(0)
        self._ck(self._lib.dk_dev_sa_smems_packed(self._h, _ptr(d_in), len(sizes), _sizes(sizes), _ptr(d_sa), _ptr(d_query), len(query_lens),
                                                  _sizes(query_lens), _ptr(blocks), int(min_len), int(max_len), int(max_hits),
                                                  None if d_hits is None else _ptr(d_hits), C.byref(total)))
        return int(total.value)

    def sa_smems(self, data, sa, queries, min_len, max_len, max_hits=65536):
        """(records, total) from host memory: a structured array (SA_SMEM_DTYPE) of the first min(total, max_hits) super-maximal matches in
        rising order of at, and their number in all (dk_sa_smems)"""
        t = as_u8(data)
        sa = np.ascontiguousarray(sa, dtype=np.uint32)
        _same_length(sa, "entries", len(t), "bytes")
        qry, lens, nq = _pack_patterns(queries)
        hits = np.zeros(max(min(int(max_hits), sum(int(x) for x in lens[:nq])), 1), dtype=SA_SMEM_DTYPE)
        total = C.c_uint64(0)
        self._ck(self._lib.dk_sa_smems(self._h, _ptr(t), len(t), _ptr(sa), _ptr(qry), nq, lens, int(min_len), int(max_len), int(max_hits), _ptr(hits),
                                       C.byref(total)))
        return hits[:min(int(total.value), int(max_hits))], int(total.value)

    # ---- FM-index: count patterns in L, no text and no suffix array; served by decoder contexts too ----
    def dev_fm_build(self, d_bwt, n, origin, d_index):
        """the index of d_bwt[0, n) with its origin into d_index, a device tensor of fm_index_bytes(n) bytes"""
        _inputs_ready(d_bwt)
        self._ck(self._lib.dk_dev_fm_build(self._h, _ptr(d_bwt), n, int(origin), _ptr(d_index)))

    def dev_fm_build_packed(self, d_bwt, sizes, origins, d_index):
        """one index for every block of a packed L (layout of dev_bwt_forward_packed); d_index: fm_index_bytes(sum(sizes), len(sizes)) bytes"""
        _inputs_ready(d_bwt)
        count = len(sizes)
        _same_length(origins, "origins", count, "blocks")
        ns = _sizes(sizes)
        org = _u32s(origins)
        self._ck(self._lib.dk_dev_fm_build_packed(self._h, _ptr(d_bwt), count, ns, _ptr(org), _ptr(d_index)))

    def dev_fm_count(self, d_bwt, n, d_index, d_pat, pat_lens, d_lo, d_hi):
        """patterns as for dev_sa_search; d_lo[q] / d_hi[q] are what dev_sa_search gives for the text d_bwt is the BWT of: hi - lo occurrences"""
        _inputs_ready(d_bwt, d_index, d_pat)
        npat = len(pat_lens)
        lens = _sizes(pat_lens)
        self._ck(self._lib.dk_dev_fm_count(self._h, _ptr(d_bwt), n, _ptr(d_index), _ptr(d_pat), npat, lens, _ptr(d_lo), _ptr(d_hi)))

    def dev_fm_count_packed(self, d_bwt, sizes, d_index, d_pat, pat_lens, pat_blocks, d_lo, d_hi):
        """dev_fm_count in a pack: pattern q is counted in block pat_blocks[q], d_lo / d_hi are local to that block"""
        _inputs_ready(d_bwt, d_index, d_pat)
        count, npat = len(sizes), len(pat_lens)
        _same_length(pat_blocks, "blocks", npat, "patterns")
        ns = _sizes(sizes)
        lens = _sizes(pat_lens)
        blocks = _u32s(pat_blocks)
        self._ck(self._lib.dk_dev_fm_count_packed(self._h, _ptr(d_bwt), count, ns, _ptr(d_index), _ptr(d_pat), npat, lens, _ptr(blocks),
                                                  _ptr(d_lo), _ptr(d_hi)))

    def fm_count(self, bwt, origin, patterns):
        """(lo, hi) per pattern, uint32 arrays, from (L, origin) in host memory, e.g. as dk_stream_decode leaves them: what sa_search gives for
        the text, without the text (dk_fm_count)"""
        b = as_u8(bwt)
        pat, lens, npat = _pack_patterns(patterns)
        lo, hi = np.zeros(npat, dtype=np.uint32), np.zeros(npat, dtype=np.uint32)
        self._ck(self._lib.dk_fm_count(self._h, _ptr(b), len(b), int(origin), _ptr(pat), npat, lens, _ptr(lo), _ptr(hi)))
        return lo, hi

    # ---- FM-index locate: positions from a sampled suffix array beside the index; decoder contexts too ----
    def dev_fm_locate_build(self, d_bwt, n, origin, step, d_loc):
        """the locate structure of d_bwt[0, n) with its origin into d_loc, a device tensor of fm_locate_bytes(n, 1, step) bytes; needs no index"""
        _inputs_ready(d_bwt)
        self._ck(self._lib.dk_dev_fm_locate_build(self._h, _ptr(d_bwt), n, int(origin), int(step), _ptr(d_loc)))

    def dev_fm_locate_build_packed(self, d_bwt, sizes, origins, step, d_loc):
        """one structure for every block of a packed L; d_loc: fm_locate_bytes(sum(sizes), len(sizes), step) bytes"""
        _inputs_ready(d_bwt)
        count = len(sizes)
        _same_length(origins, "origins", count, "blocks")
        ns = _sizes(sizes)
        org = _u32s(origins)
        self._ck(self._lib.dk_dev_fm_locate_build_packed(self._h, _ptr(d_bwt), count, ns, _ptr(org), int(step), _ptr(d_loc)))

    def dev_fm_locate(self, d_bwt, n, d_index, d_loc, step, d_lo, d_hi, npat, max_hits, d_pos):
        """d_pos[q * max_hits + j] = the text position of slot d_lo[q] + j for j < min(d_hi[q] - d_lo[q], max_hits), FM_NO_HIT behind them;
        d_lo / d_hi as dev_fm_count wrote them, d_pos a uint32 device tensor of npat * max_hits words"""
        _inputs_ready(d_bwt, d_index, d_loc, d_lo, d_hi)
        self._ck(self._lib.dk_dev_fm_locate(self._h, _ptr(d_bwt), n, _ptr(d_index), _ptr(d_loc), int(step), _ptr(d_lo), _ptr(d_hi), int(npat),
                                            int(max_hits), _ptr(d_pos)))

    def dev_fm_locate_packed(self, d_bwt, sizes, d_index, d_loc, step, d_lo, d_hi, pat_blocks, max_hits, d_pos):
        """dev_fm_locate in a pack: row q holds positions local to block pat_blocks[q]"""
        _inputs_ready(d_bwt, d_index, d_loc, d_lo, d_hi)
        count, npat = len(sizes), len(pat_blocks)
        ns = _sizes(sizes)
        blocks = _u32s(pat_blocks)
        self._ck(self._lib.dk_dev_fm_locate_packed(self._h, _ptr(d_bwt), count, ns, _ptr(d_index), _ptr(d_loc), int(step), _ptr(d_lo), _ptr(d_hi),
                                                   npat, _ptr(blocks), int(max_hits), _ptr(d_pos)))

    def fm_locate(self, bwt, origin, patterns, max_hits=16, step=32):
        """(lo, hi, pos) from (L, origin) in host memory: lo / hi as fm_count gives them, pos a uint32 array of len(patterns) x max_hits whose
        row q starts with the first min(hi - lo, max_hits) text positions of pattern q in suffix-array order, FM_NO_HIT behind (dk_fm_locate)"""
        b = as_u8(bwt)
        pat, lens, npat = _pack_patterns(patterns)
        lo, hi = np.zeros(npat, dtype=np.uint32), np.zeros(npat, dtype=np.uint32)
        pos = np.zeros((npat, max(int(max_hits), 1)), dtype=np.uint32)
        self._ck(self._lib.dk_fm_locate(self._h, _ptr(b), len(b), int(origin), int(step), _ptr(pat), npat, lens, int(max_hits), _ptr(lo), _ptr(hi),
                                        _ptr(pos)))
        return lo, hi, pos

    # ---- FM-index extract: text ranges from L, the index and the anchors; decoder contexts too ----
    def dev_fm_extract_build(self, d_bwt, n, origin, step, d_ext):
        """the extract structure of d_bwt[0, n) with its origin into d_ext, a device tensor of fm_extract_bytes(n, 1, step) bytes; needs no index"""
        _inputs_ready(d_bwt)
        self._ck(self._lib.dk_dev_fm_extract_build(self._h, _ptr(d_bwt), n, int(origin), int(step), _ptr(d_ext)))

    def dev_fm_extract_build_packed(self, d_bwt, sizes, origins, step, d_ext):
        """one structure for every block of a packed L; d_ext: fm_extract_bytes(sum(sizes), len(sizes), step) bytes"""
        _inputs_ready(d_bwt)
        count = len(sizes)
        _same_length(origins, "origins", count, "blocks")
        ns = _sizes(sizes)
        org = _u32s(origins)
        self._ck(self._lib.dk_dev_fm_extract_build_packed(self._h, _ptr(d_bwt), count, ns, _ptr(org), int(step), _ptr(d_ext)))

    def dev_fm_extract(self, d_bwt, n, d_index, d_ext, step, d_pos, d_len, nrange, max_len, d_out):
        """row q of d_out (a uint8 device tensor of nrange * max_len bytes, any alignment) = the text at [d_pos[q], d_pos[q] + d_len[q]), cut to
        max_len and to the block's end, zeros behind; d_pos / d_len uint32 device tensors (d_len None: every range max_len long)"""
        _inputs_ready(d_bwt, d_index, d_ext, d_pos, *([] if d_len is None else [d_len]))
        self._ck(self._lib.dk_dev_fm_extract(self._h, _ptr(d_bwt), n, _ptr(d_index), _ptr(d_ext), int(step), _ptr(d_pos),
                                             None if d_len is None else _ptr(d_len), int(nrange), int(max_len), _ptr(d_out)))

    def dev_fm_extract_packed(self, d_bwt, sizes, d_index, d_ext, step, d_pos, d_len, range_blocks, max_len, d_out):
        """dev_fm_extract in a pack: range q lies in block range_blocks[q], its start is local to that block"""
        _inputs_ready(d_bwt, d_index, d_ext, d_pos, *([] if d_len is None else [d_len]))
        count, nrange = len(sizes), len(range_blocks)
        ns = _sizes(sizes)
        blocks = _u32s(range_blocks)
        self._ck(self._lib.dk_dev_fm_extract_packed(self._h, _ptr(d_bwt), count, ns, _ptr(d_index), _ptr(d_ext), int(step), _ptr(d_pos),
                                                    None if d_len is None else _ptr(d_len), nrange, _ptr(blocks), int(max_len), _ptr(d_out)))

    def fm_extract(self, bwt, origin, positions, lengths, max_len, step=32):
        """a uint8 array of len(positions) x max_len from (L, origin) in host memory: row q = the text at [positions[q], positions[q] +
        lengths[q]), cut to max_len and the text's end, zeros behind; lengths None: every range max_len long (dk_fm_extract)"""
        b = as_u8(bwt)
        pos = _u32s(positions)
        nrange = len(positions)
        lens = None if lengths is None else (np.array(lengths, dtype=np.int64).astype(np.uint32) if nrange else np.zeros(1, np.uint32))
        out = np.zeros((nrange, max(int(max_len), 1)), dtype=np.uint8)
        self._ck(self._lib.dk_fm_extract(self._h, _ptr(b), len(b), int(origin), int(step), _ptr(pos), None if lens is None else _ptr(lens), nrange,
                                         int(max_len), _ptr(out)))
        return out

    # ---- FM-index find: every pattern in every block, as a compact list of hit records; decoder contexts too ----
    def dev_fm_find(self, d_bwt, n, d_index, d_loc, step, d_pat, pat_lens, max_hits, d_hits, d_occ=None):
        """every pattern in d_bwt[0, n): d_occ[q] (a uint32 device tensor, or None) = its occurrences, the return value their sum; d_hits (a
        16-byte aligned device tensor of max_hits records of four uint32 words: pattern, block, position, slot) receives the first
        min(sum, max_hits) hits in the order (pattern, slot).  max_hits == 0: d_hits and d_loc may be None"""
        _inputs_ready(d_bwt, d_index, d_pat)
        npat = len(pat_lens)
        lens = _sizes(pat_lens)
        total = C.c_uint64(0)
        self._ck(self._lib.dk_dev_fm_find(self._h, _ptr(d_bwt), n, _ptr(d_index), None if d_loc is None else _ptr(d_loc), int(step), _ptr(d_pat),
                                          npat, lens, int(max_hits), None if d_hits is None else _ptr(d_hits),
                                          None if d_occ is None else _ptr(d_occ), C.byref(total)))
        return int(total.value)

    def dev_fm_find_packed(self, d_bwt, sizes, d_index, d_loc, step, d_pat, pat_lens, max_hits, d_hits, d_occ=None):
        """dev_fm_find over a pack: every pattern in every block.  d_occ[q * len(sizes) + b] = occurrences of pattern q in block b; the hits in
        the order (pattern, block, slot), positions and slots local to their block"""
        _inputs_ready(d_bwt, d_index, d_pat)
        count, npat = len(sizes), len(pat_lens)
        ns = _sizes(sizes)
        lens = _sizes(pat_lens)
        total = C.c_uint64(0)
        self._ck(self._lib.dk_dev_fm_find_packed(self._h, _ptr(d_bwt), count, ns, _ptr(d_index), None if d_loc is None else _ptr(d_loc), int(step),
                                                 _ptr(d_pat), npat, lens, int(max_hits), None if d_hits is None else _ptr(d_hits),
                                                 None if d_occ is None else _ptr(d_occ), C.byref(total)))
        return int(total.value)

    def fm_find(self, bwt, origin, patterns, max_hits=65536, step=32):
        """(occ, hits, total) from (L, origin) in host memory: occ a uint32 array per pattern, hits a structured array (FM_HIT_DTYPE) of the
        first min(total, max_hits) hits in the order (pattern, slot), total their number in all (dk_fm_find)"""
        b = as_u8(bwt)
        pat, lens, npat = _pack_patterns(patterns)
        occ = np.zeros(npat, dtype=np.uint32)
        hits = np.zeros(max(int(max_hits), 1), dtype=FM_HIT_DTYPE)
        total = C.c_uint64(0)
        self._ck(self._lib.dk_fm_find(self._h, _ptr(b), len(b), int(origin), int(step), _ptr(pat), npat, lens, int(max_hits), _ptr(hits), _ptr(occ),
                                      C.byref(total)))
        return occ, hits[:min(int(total.value), int(max_hits))], int(total.value)

    # ---- FM-index seams: the matches that straddle block borders; decoder contexts too ----
    def dev_fm_seams(self, d_bwt, n, d_index, d_ext, step, d_prev, d_pat, pat_lens, max_hits, d_hits, d_occ=None):
        """the occurrences of every pattern in (d_prev + the block's text) that start in d_prev (a uint8 device tensor, or None) and end in the
        block: d_occ[q] their number, the return value the sum; d_hits (16-byte aligned, max_hits records of four uint32 words: pattern, block,
        back, 0) receives the first min(sum, max_hits) in the order (pattern, back descending), back = the match's bytes in front of the block"""
        _inputs_ready(d_bwt, d_index, d_ext, d_pat)
        npat, prev_len = len(pat_lens), 0 if d_prev is None else int(d_prev.numel())
        lens = _sizes(pat_lens)
        total = C.c_uint64(0)
        self._ck(self._lib.dk_dev_fm_seams(self._h, _ptr(d_bwt), n, _ptr(d_index), _ptr(d_ext), int(step), _ptr(d_prev) if prev_len else None, prev_len,
                                           _ptr(d_pat), npat, lens, int(max_hits), None if d_hits is None else _ptr(d_hits),
                                           None if d_occ is None else _ptr(d_occ), C.byref(total)))
        return int(total.value)

    def dev_fm_seams_packed(self, d_bwt, sizes, d_index, d_ext, step, d_prev, d_pat, pat_lens, max_hits, d_hits, d_occ=None):
        """dev_fm_seams over a pack: d_prev and the blocks are the consecutive pieces of one text, and a seam hit -- first and last byte in
        different pieces -- belongs to the block of its last byte.  d_occ[q * len(sizes) + b]; the hits in the order (pattern, block, back
        descending)"""
        _inputs_ready(d_bwt, d_index, d_ext, d_pat)
        count, npat, prev_len = len(sizes), len(pat_lens), 0 if d_prev is None else int(d_prev.numel())
        ns = _sizes(sizes)
        lens = _sizes(pat_lens)
        total = C.c_uint64(0)
        self._ck(self._lib.dk_dev_fm_seams_packed(self._h, _ptr(d_bwt), count, ns, _ptr(d_index), _ptr(d_ext), int(step),
                                                  _ptr(d_prev) if prev_len else None, prev_len, _ptr(d_pat), npat, lens, int(max_hits),
                                                  None if d_hits is None else _ptr(d_hits), None if d_occ is None else _ptr(d_occ), C.byref(total)))
        return int(total.value)

    # ---- FM-index near: byte classes and a budget of mismatches; decoder contexts too ----
    def dev_fm_near(self, d_bwt, n, d_index, d_loc, step, d_cls, pat_lens, k, node_limit, max_hits, d_hits, d_occ=None):
        """every pattern in d_bwt[0, n) with at most k positions missed -> (total, cut).  d_cls (a uint8 device tensor): 32 bytes per pattern
        position, bit c & 7 of byte c >> 3 set where byte value c matches, the patterns back to back.  d_occ[q] (uint32 device tensor, or None) =
        the hits of pattern q; d_hits (16-byte aligned, max_hits records of four uint32 words: pattern, block, position, cost) receives the
        first min(total, max_hits) in the preorder of the search tree, of which node_limit nodes (0: FM_NEAR_NODE_LIMIT) are visited per pattern;
        cut = the patterns that stopped there.  max_hits == 0: d_hits and d_loc may be None"""
        _inputs_ready(d_bwt, d_index, d_cls)
        npat = len(pat_lens)
        lens = _sizes(pat_lens)
        total, cut = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._lib.dk_dev_fm_near(self._h, _ptr(d_bwt), n, _ptr(d_index), None if d_loc is None else _ptr(d_loc), int(step),
                                          None if d_cls is None else _ptr(d_cls), npat, lens, int(k), int(node_limit), int(max_hits),
                                          None if d_hits is None else _ptr(d_hits), None if d_occ is None else _ptr(d_occ), C.byref(total),
                                          C.byref(cut)))
        return int(total.value), int(cut.value)

    def dev_fm_near_packed(self, d_bwt, sizes, d_index, d_loc, step, d_cls, pat_lens, k, node_limit, max_hits, d_hits, d_occ=None):
        """dev_fm_near over a pack: every pattern in every block.  d_occ[q * len(sizes) + b]; the hits in the order (pattern, block, preorder of
        the pair's tree, slot), positions local to their block; cut = the (pattern, block) pairs that stopped at the node limit"""
        _inputs_ready(d_bwt, d_index, d_cls)
        count, npat = len(sizes), len(pat_lens)
        ns = _sizes(sizes)
        lens = _sizes(pat_lens)
        total, cut = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._lib.dk_dev_fm_near_packed(self._h, _ptr(d_bwt), count, ns, _ptr(d_index), None if d_loc is None else _ptr(d_loc), int(step),
                                                 None if d_cls is None else _ptr(d_cls), npat, lens, int(k), int(node_limit), int(max_hits),
                                                 None if d_hits is None else _ptr(d_hits), None if d_occ is None else _ptr(d_occ),
                                                 C.byref(total), C.byref(cut)))
        return int(total.value), int(cut.value)

    def dbg_dev_fm_rank(self, d_bwt, total, d_index, d_pos, d_sym, d_out):
        """d_out[q] = occurrences of d_sym[q] in d_bwt[0, d_pos[q]) by the count kernel's rank (uint32 / uint8 / uint32 device tensors)"""
        _inputs_ready(d_bwt, d_index, d_pos, d_sym)
        self._ck(self._lib.dk_dbg_dev_fm_rank(self._h, _ptr(d_bwt), total, _ptr(d_index), _ptr(d_pos), _ptr(d_sym), len(d_pos), _ptr(d_out)))

    def dev_dc_encode_packed(self, d_bwt, sizes, d_dist, d_sym, d_rank=None):
        """DC arrays of a packed L: block i's entries at [off_i, off_i + m_i); returns (list of init tables, list of m)"""
        _inputs_ready(d_bwt)
        count = len(sizes)
        ns = _sizes(sizes)
        init = np.zeros((max(count, 1), 256), dtype=np.uint32)
        m = (C.c_size_t * max(count, 1))()
        self._ck(self._lib.dk_dev_dc_encode_packed(self._h, _ptr(d_bwt), count, ns, _ptr(init), _ptr(d_dist), _ptr(d_sym),
                                                   _ptr(d_rank) if d_rank is not None else None, m))
        return [init[i] for i in range(count)], [int(m[i]) for i in range(count)]

    def dev_packed_encode(self, model, d_in, sizes, host_threads=8, outs=None):
        """every block of the pack coded as by dev_block_encode; returns (list of coded streams, list of DK_FLAG_* words)"""
        _inputs_ready(d_in)
        count = len(sizes)
        mid = model_id(model)
        if outs is None:  # (rawdc: one 10-byte record per distance)
            outs = [np.empty(_stream_cap(mid, n), dtype=np.uint8) for n in sizes]
        ns = _sizes(sizes)
        optrs = (C.c_void_p * count)(*[_ptr(o) for o in outs])
        caps = (C.c_size_t * count)(*[len(o) for o in outs])
        lens = (C.c_size_t * count)()
        flags = (C.c_uint * max(count, 1))()
        self._ck(self._lib.dk_dev_packed_encode(self._h, mid, _ptr(d_in), count, ns, optrs, caps, lens, flags,
                                                int(host_threads)))
        return [o[:lens[i]] for i, o in enumerate(outs)], [int(flags[i]) for i in range(count)]

    def dev_bwt_inverse_packed(self, d_bwt, sizes, origins, d_out):
        """inverse of dev_bwt_forward_packed: block i's text into d_out (same layout as d_bwt) from its L and origins[i]"""
        _inputs_ready(d_bwt)
        count = len(sizes)
        _same_length(origins, "origins", count, "blocks")
        ns = _sizes(sizes)
        org = _u32s(origins)
        self._ck(self._lib.dk_dev_bwt_inverse_packed(self._h, _ptr(d_bwt), count, ns, _ptr(org), _ptr(d_out)))

    def dev_packed_decode(self, model, streams, sizes, d_out, host_threads=8):
        """inverse of dev_packed_encode: every stream decoded, the blocks back to back into the device tensor d_out"""
        count = len(streams)
        keep = [as_u8(x) for x in streams]
        ins = (C.c_void_p * max(count, 1))(*[_ptr(x) for x in keep])
        lens = (C.c_size_t * max(count, 1))(*[len(x) for x in keep])
        ns = _sizes(sizes)
        self._ck(self._lib.dk_dev_packed_decode(self._h, model_id(model), count, ins, lens, ns, _ptr(d_out), int(host_threads)))

    def dev_block_encode(self, model, d_in, n, out=None):
        """out: optional preallocated host uint8 array; returns a view of the coded stream"""
        _inputs_ready(d_in)
        mid = model_id(model)
        if out is None:
            out = np.empty(2 * n + 4096 + _prefix(mid), dtype=np.uint8)
        ln = C.c_size_t(0)
        self._ck(self._lib.dk_dev_block_encode(self._h, mid, _ptr(d_in), n, _ptr(out), len(out), C.byref(ln)))
        return out[:ln.value]

    def dev_batch_encode(self, model, d_blocks, sizes, host_threads=8, outs=None):
        """d_blocks: device tensors / addresses; returns a list of coded streams (views of `outs` when given)"""
        _inputs_ready(*d_blocks[:1])
        count = len(d_blocks)
        mid = model_id(model)
        if outs is None:
            outs = [np.empty(2 * int(n) + 4096 + _prefix(mid), dtype=np.uint8) for n in sizes]
        ptrs = (C.c_void_p * count)(*[_ptr(b) for b in d_blocks])
        ns = _sizes(sizes)
        optrs = (C.c_void_p * count)(*[_ptr(o) for o in outs])
        caps = (C.c_size_t * count)(*[len(o) for o in outs])
        lens = (C.c_size_t * count)()
        self._ck(self._lib.dk_dev_batch_encode(self._h, mid, count, ptrs, ns, optrs, caps, lens, int(host_threads)))
        return [o[:lens[i]] for i, o in enumerate(outs)]

    def batch_begin(self, model, host_threads=8):
        """streaming form of dev_batch_encode: returns a Batch; push(d_in, n) per block as it arrives, then finish() -> list of streams"""
        return Batch(self, model, host_threads)

    def dev_batch_decode(self, model, streams, sizes, d_outs, host_threads=8):
        count = len(streams)
        keep = [as_u8(x) for x in streams]
        ins = (C.c_void_p * count)(*[_ptr(x) for x in keep])
        lens = (C.c_size_t * count)(*[len(x) for x in keep])
        ns = _sizes(sizes)
        outs = (C.c_void_p * count)(*[_ptr(o) for o in d_outs])
        self._ck(self._lib.dk_dev_batch_decode(self._h, model_id(model), count, ins, lens, ns, outs, int(host_threads)))

    def dev_block_decode(self, model, stream, n, d_out):
        s = as_u8(stream)
        self._ck(self._lib.dk_dev_block_decode(self._h, model_id(model), _ptr(s), len(s), n, _ptr(d_out)))

    # ---- measurement ----
    def set_profiling(self, enabled):
        self._ck(self._lib.dk_set_profiling(self._h, 1 if enabled else 0))

    def stats_reset(self):
        self._ck(self._lib.dk_stats_reset(self._h))

    def stats(self):
        st = _lib.Stats()
        self._ck(self._lib.dk_get_stats(self._h, C.byref(st)))
        out = {k: getattr(st, k) for k in ("ms_h2d", "ms_sa", "ms_bwt", "ms_dc", "ms_d2h", "ms_entropy", "ms_ibwt",
                                           "ms_total", "rounds", "sort_passes", "sorted_elements", "dc_runs",
                                           "entropy_threads", "entropy_l3_group", "entropy_l3_numa", "gpu_numa", "ws_peak_bytes", "ws_size_bytes",
                                           "lcp_measured", "lcp_bytes_compared", "lcp_passes")}
        kernels = {}
        for i in range(_lib.NUM_KERNEL_SLOTS):
            name = self._lib.dk_kernel_name(i)
            if name and st.kernel_launches[i]:
                kernels[name.decode()] = dict(launches=int(st.kernel_launches[i]), ms=float(st.kernel_ms[i]),
                                              bytes=float(st.kernel_bytes[i]))
        out["kernels"] = kernels
        out["routes"] = {name for name, bit in _lib.ROUTES.items() if st.sa_route & bit}  # which ways the last suffix sort took
        return out

    def dbg_mail_fill(self, byte):
        """dk_dbg_mail_fill: every word of the stages' mailbox (device page and host twin) = byte; between complete calls only"""
        self._ck(self._lib.dk_dbg_mail_fill(self._h, int(byte)))

    def dbg_ws_peek(self, nbytes):
        """dk_dbg_ws_peek: nbytes of a fresh workspace allocation as a stage would find them (tuning build, DK_POISON=b: all b) -> uint8 array"""
        out = np.empty(int(nbytes), dtype=np.uint8)
        self._ck(self._lib.dk_dbg_ws_peek(self._h, len(out), _ptr(out)))
        return out

    def dbg_sort_pairs(self, keys, vals, begin_bit=0, end_bit=64):
        keys = np.ascontiguousarray(keys, dtype=np.uint64).copy()
        vals = np.ascontiguousarray(vals, dtype=np.uint32).copy()
        self._ck(self._lib.dk_dbg_sort_pairs(self._h, _ptr(keys), _ptr(vals), len(keys), begin_bit, end_bit))
        return keys, vals

    # ---- the sort layer's device entry points (csrc/radix_sort.hip), numpy in and out; torch only holds the device buffers ----
    def _to_dev(self, a, dtype):
        import torch
        a = np.ascontiguousarray(a, dtype=dtype)
        signed = {4: np.int32, 8: np.int64}[a.dtype.itemsize]  # (torch has no arithmetic on unsigned words, and needs none here)
        return torch.from_numpy(a.view(signed).copy()).to("cuda:%d" % self.device)

    @staticmethod
    def _to_host(t, dtype):
        return t.cpu().numpy().view(dtype)

    def dbg_dev_sort_pairs(self, keys, vals, begin_bit=0, end_bit=64):
        """dk_dbg_dev_sort_pairs: the stable sort on bits [begin_bit, end_bit) of device arrays, in place -> (keys, vals)"""
        return self._dev_sort(self._lib.dk_dbg_dev_sort_pairs, keys, vals, begin_bit, end_bit)

    def dbg_dev_local_sort(self, keys, vals, begin_bit=0, end_bit=64):
        """dk_dbg_dev_local_sort: every 8192-pair tile sorted by itself -> (keys, vals)"""
        return self._dev_sort(self._lib.dk_dbg_dev_local_sort, keys, vals, begin_bit, end_bit)

    def _dev_sort(self, fn, keys, vals, begin_bit, end_bit):
        if len(keys) != len(vals):
            raise DarkError(_lib.DK_E_ARG, "%d keys, %d values" % (len(keys), len(vals)))
        d_k, d_v = self._to_dev(keys, np.uint64), self._to_dev(vals, np.uint32)
        _inputs_ready(d_k)
        self._ck(fn(self._h, _ptr(d_k), _ptr(d_v), len(keys), int(begin_bit), int(end_bit)))
        return self._to_host(d_k, np.uint64), self._to_host(d_v, np.uint32)

    def dbg_dev_sort_groups(self, kin, vin, starts, above, begin_bit, end_bit, kout=None, vout=None):
        """dk_dbg_dev_sort_groups: group g = the pairs [starts[g], starts[g + 1]).  kout / vout: what the output arrays hold before the call
        (both or neither); without them the sort is in place.  -> (kout, vout) after the call"""
        if (kout is None) != (vout is None):
            raise DarkError(_lib.DK_E_ARG, "kout and vout: both or neither")
        starts = np.ascontiguousarray(starts, dtype=np.uint32)
        d_ki, d_vi = self._to_dev(kin, np.uint64), self._to_dev(vin, np.uint32)
        d_ko, d_vo = (d_ki, d_vi) if kout is None else (self._to_dev(kout, np.uint64), self._to_dev(vout, np.uint32))
        if not (len(d_ki) == len(d_vi) == len(d_ko) == len(d_vo)):
            raise DarkError(_lib.DK_E_ARG, "arrays of different lengths")
        _inputs_ready(d_ki)
        self._ck(self._lib.dk_dbg_dev_sort_groups(self._h, _ptr(d_ki), _ptr(d_vi), _ptr(d_ko), _ptr(d_vo), _ptr(starts), len(starts) - 1, len(d_ki),
                                                  int(above), int(begin_bit), int(end_bit)))
        return self._to_host(d_ko, np.uint64), self._to_host(d_vo, np.uint32)

    def dbg_dev_rerank(self, keys, idx, pos_in=None, gid_in=None, bucket_starts=None, cmp_shift=0, rank=None, sa=None, bwt=None, sym_in=None,
                       origin=None, ls_max=1024, reduce_tiles_per_wg=0, first_tiles_per_wg=0, sparse_max=-1, shift=None, fill=0xC3, pad=64):
        """dk_dbg_dev_rerank: one regrouping and its classification.  keys: uint64, or uint32 with bucket_starts (256 words).  pos_in None: the
        first rerank.  rank / sa / bwt / origin: what those arrays hold before the call (None: a null pointer).  shift: {name: elements} by which
        the device view of keys / idx / gid_in / sym_in / bwt starts behind its allocation.  Every output array holds `fill` bytes before the
        call; gstart has count // 2 + 1 + pad words, bigidx and bigoff count // 2 + pad.  -> dict of the arrays after the call (whole, the
        untouched parts included; None for the null ones) and counts = (active, groups, big_slots, big_groups, above_pl_slots)"""
        import torch
        shift = shift or {}
        dev = "cuda:%d" % self.device

        def up(name, a, dtype):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            off = int(shift.get(name, 0))
            whole = np.concatenate([np.zeros(off, dtype), a]) if off else a.copy()
            return torch.from_numpy(whole.view({1: np.uint8, 4: np.int32, 8: np.int64}[whole.dtype.itemsize])).to(dev)[off:]

        def out(words, dtype):
            return torch.from_numpy(np.full(words * np.dtype(dtype).itemsize, fill, np.uint8)).to(dev)

        narrow = np.asarray(keys).dtype == np.uint32
        count = len(keys)
        d = dict(keys=up("keys", keys, np.uint32 if narrow else np.uint64), bucket_starts=up("bucket_starts", bucket_starts, np.uint32),
                 idx=up("idx", idx, np.uint32), pos_in=up("pos_in", pos_in, np.uint32), gid_in=up("gid_in", gid_in, np.uint32),
                 rank=up("rank", rank, np.uint32), sa=up("sa", sa, np.uint32), bwt=up("bwt", bwt, np.uint8), sym_in=up("sym_in", sym_in, np.uint8),
                 origin=up("origin", None if origin is None else [origin], np.uint32))
        for name in ("idx", "pos_in", "gid_in", "sym_in"):
            if d[name] is not None and len(d[name]) != count:
                raise DarkError(_lib.DK_E_ARG, "%d keys, %d entries of %s" % (count, len(d[name]), name))
        if pos_in is None and bwt is not None and len(d["bwt"]) != count:
            raise DarkError(_lib.DK_E_ARG, "the first rerank reads L[slot]: %d keys, %d bytes of bwt" % (count, len(d["bwt"])))
        outs = dict(out_idx=(count + pad, np.uint32), out_pos=(count + pad, np.uint32), out_gid=(count + pad, np.uint32),
                    sym_out=(count + pad, np.uint8), gstart=(count // 2 + 1 + pad, np.uint32), bigidx=(count // 2 + pad, np.uint32),
                    bigoff=(count // 2 + pad, np.uint32))
        if bwt is None:
            del outs["sym_out"]
        o = {name: out(words, dtype) for name, (words, dtype) in outs.items()}
        counts = np.zeros(5, np.uint32)
        p = lambda t: None if t is None else _ptr(t)  # noqa: E731
        _inputs_ready(d["keys"])
        self._ck(self._lib.dk_dbg_dev_rerank(self._h, p(d["keys"]), 4 if narrow else 8, p(d["bucket_starts"]), p(d["idx"]), p(d["pos_in"]), p(d["gid_in"]),
                                             int(cmp_shift), count, p(d["rank"]), p(d["sa"]), p(d["bwt"]), p(d["sym_in"]), p(o.get("sym_out")),
                                             p(d["origin"]), p(o["out_idx"]), p(o["out_pos"]), p(o["out_gid"]), p(o["gstart"]), p(o["bigidx"]),
                                             p(o["bigoff"]), int(ls_max), _ptr(counts), int(reduce_tiles_per_wg), int(first_tiles_per_wg),
                                             int(sparse_max)))
        res = {name: self._to_host(t, outs[name][1]) for name, t in o.items()}
        res.setdefault("sym_out", None)
        for name, dtype in (("rank", np.uint32), ("sa", np.uint32), ("bwt", np.uint8)):
            res[name] = None if d[name] is None else self._to_host(d[name], dtype)
        res["origin"] = None if d["origin"] is None else int(self._to_host(d["origin"], np.uint32)[0])
        res["counts"] = tuple(int(c) for c in counts)
        return res

    def dbg_dev_lf_rerank(self, keys, idx, sym=None, pos_in=None, bucket_starts=None, cmp_shift=0, sym_from_key=False, zero_slot=None, bwt=None,
                          origin=None, depth=None, bigdepth=None, key_shift=0, depth_add=0, reduce_tiles_per_wg=0, shift=None, fill=0xC3, pad=64):
        """dk_dbg_dev_lf_rerank: one rerank of the L-first path and its classification.  keys: uint64, or uint32 (with bucket_starts, 256 words:
        the narrow first rerank; without: group ids).  sym: the symbol in front of every slot (sym_from_key: what the array holds before the
        call; None: `fill` bytes).  pos_in None: the first rerank.  zero_slot: the word *d_zero_slot (None: a null pointer).  bwt / origin: what
        L and the origin word hold before the call (None: null pointers).  depth None: no d_gdepth_out; a number: every live group's; with
        bigdepth (words): the big-list rule bigdepth[key >> key_shift] + depth_add.  shift: {name: elements} by which the device view of keys /
        idx / sym / pos_in starts behind its allocation.  Every output array holds `fill` bytes before the call: the lists count + pad entries,
        gstart count // 2 + 1 + pad words, gdepth count // 2 + pad.  -> dict of the arrays after the call (whole, the untouched parts
        included; None for the null ones), sym, bwt, origin, and counts = (active, groups, big_slots, big_groups)"""
        import torch
        shift = shift or {}
        dev = "cuda:%d" % self.device

        def up(name, a, dtype):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            off = int(shift.get(name, 0))
            whole = np.concatenate([np.zeros(off, dtype), a]) if off else a.copy()
            return torch.from_numpy(whole.view({1: np.uint8, 4: np.int32, 8: np.int64}[whole.dtype.itemsize])).to(dev)[off:]

        def out(words, dtype):
            return torch.from_numpy(np.full(words * np.dtype(dtype).itemsize, fill, np.uint8)).to(dev)

        narrow = np.asarray(keys).dtype == np.uint32
        count = len(keys)
        if sym is None:
            sym = np.full(count, fill, np.uint8)
        d = dict(keys=up("keys", keys, np.uint32 if narrow else np.uint64), bucket_starts=up("bucket_starts", bucket_starts, np.uint32),
                 idx=up("idx", idx, np.uint32), sym=up("sym", sym, np.uint8), pos_in=up("pos_in", pos_in, np.uint32),
                 zero_slot=up("zero_slot", None if zero_slot is None else [zero_slot], np.uint32), bwt=up("bwt", bwt, np.uint8),
                 origin=up("origin", None if origin is None else [origin], np.uint32), bigdepth=up("bigdepth", bigdepth, np.uint32))
        for name in ("idx", "sym", "pos_in"):
            if d[name] is not None and len(d[name]) != count:
                raise DarkError(_lib.DK_E_ARG, "%d keys, %d entries of %s" % (count, len(d[name]), name))
        outs = dict(out_idx=(count + pad, np.uint32), out_pos=(count + pad, np.uint32), out_gid=(count + pad, np.uint32), out_sym=(count + pad, np.uint8),
                    gstart=(count // 2 + 1 + pad, np.uint32), gdepth=(count // 2 + pad, np.uint32))
        if depth is None and bigdepth is None:
            del outs["gdepth"]
        o = {name: out(words, dtype) for name, (words, dtype) in outs.items()}
        counts = np.zeros(4, np.uint32)
        p = lambda t: None if t is None else _ptr(t)  # noqa: E731
        _inputs_ready(d["keys"])
        self._ck(self._lib.dk_dbg_dev_lf_rerank(self._h, p(d["keys"]), 4 if narrow else 8, p(d["bucket_starts"]), int(cmp_shift), p(d["sym"]),
                                                int(bool(sym_from_key)), p(d["idx"]), p(d["zero_slot"]), p(d["pos_in"]), count, p(o["out_idx"]),
                                                p(o["out_pos"]), p(o["out_gid"]), p(o["out_sym"]), p(o["gstart"]), p(d["bwt"]), p(d["origin"]),
                                                p(o.get("gdepth")), int(depth or 0), p(d["bigdepth"]), int(key_shift), int(depth_add), _ptr(counts),
                                                int(reduce_tiles_per_wg)))
        res = {name: self._to_host(t, outs[name][1]) for name, t in o.items()}
        res.setdefault("gdepth", None)
        res["sym"] = self._to_host(d["sym"], np.uint8)
        res["bwt"] = None if d["bwt"] is None else self._to_host(d["bwt"], np.uint8)
        res["origin"] = None if d["origin"] is None else int(self._to_host(d["origin"], np.uint32)[0])
        res["counts"] = tuple(int(c) for c in counts)
        return res

    def dbg_dev_lf_refine(self, text, idx, pos, gid, sym, h0, period=0, fill=0xC3, origin=0xC3C3C3C3):
        """dk_dbg_dev_lf_refine: the L-first path from a list (suffix, place in L, group, symbol in front per slot; the members of a group equal in
        h0 symbols) to its end.  L holds `fill` bytes and the origin word `origin` before the call.  -> dict: bwt (n bytes), origin, verdict
        ("l_complete" / "start_over"), routes (names), and the counters rounds, deep_count, arena_used, giant_count, fallback, giant_count_1"""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        import torch
        dev = "cuda:%d" % self.device
        d_text = torch.from_numpy(text.copy()).to(dev)
        d_sym = torch.from_numpy(np.ascontiguousarray(sym, dtype=np.uint8).copy()).to(dev)
        d_idx, d_pos, d_gid = (self._to_dev(a, np.uint32) for a in (idx, pos, gid))
        if not (len(d_idx) == len(d_pos) == len(d_gid) == len(d_sym)):
            raise DarkError(_lib.DK_E_ARG, "list arrays of different lengths")
        d_bwt = torch.from_numpy(np.full(len(text), fill, np.uint8)).to(dev)
        d_origin = self._to_dev(np.array([origin], np.uint32), np.uint32)
        out = np.zeros(8, np.uint32)
        _inputs_ready(d_text)
        self._ck(self._lib.dk_dbg_dev_lf_refine(self._h, _ptr(d_text), len(text), _ptr(d_idx), _ptr(d_pos), _ptr(d_gid), _ptr(d_sym), len(d_idx), int(h0),
                                                int(period), _ptr(d_bwt), _ptr(d_origin), _ptr(out)))
        return dict(bwt=d_bwt.cpu().numpy(), origin=int(self._to_host(d_origin, np.uint32)[0]), verdict={1: "l_complete", 2: "start_over"}[int(out[0])],
                    routes={name for name, bit in _lib.ROUTES.items() if int(out[1]) & bit}, rounds=int(out[2]), deep_count=int(out[3]),
                    arena_used=int(out[4]), giant_count=int(out[5]), fallback=int(out[6]), giant_count_1=int(out[7]))

    def dbg_dev_in_place(self, n, h, idx, pos, gid, gstart, rank, sa=None, bwt=None, sym=None, origin=0xC3C3C3C3, chain_group=-1, record_cap=0,
                         max_rounds=-1, always_compact=False, fill=0xC3, pad=64):
        """dk_dbg_dev_in_place: the pair chains, the in-place rounds and the compaction on a list (suffix, SA position and group per slot, gstart
        with its end entry; rank for every suffix of the text).  sa (n words): the suffix-array mode; bwt (n bytes) with sym: the carried-L mode,
        the origin word holding `origin` before the call.  Every list output holds `fill` bytes before the call, count + pad entries.
        -> dict: idx, meta, pos, sym (whole, pad included; sym None in the sa mode), rank, sa or bwt, origin (None in the sa mode) and the
        counters slots, live, records, list_full, settled, rounds, compactions, routes (names)"""
        import torch
        dev = "cuda:%d" % self.device
        d_idx, d_pos, d_gid, d_gstart, d_rank = (self._to_dev(a, np.uint32) for a in (idx, pos, gid, gstart, rank))
        count = len(d_idx)
        if not (len(d_pos) == len(d_gid) == count) or len(d_rank) != n or (sa is None) == (bwt is None) or (bwt is None) != (sym is None):
            raise DarkError(_lib.DK_E_ARG, "list arrays of different lengths, %d ranks for n = %d, or not exactly one of sa and bwt + sym" % (len(d_rank), n))
        l_mode = sa is None
        if len(sa if not l_mode else bwt) != n or (l_mode and len(sym) != count):
            raise DarkError(_lib.DK_E_ARG, "sa / bwt of n entries, sym of one per slot")
        u8 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8).copy()).to(dev)  # noqa: E731
        d_sa = None if l_mode else self._to_dev(sa, np.uint32)
        d_bwt, d_sym = (u8(bwt), u8(sym)) if l_mode else (None, None)
        d_origin = self._to_dev(np.array([origin], np.uint32), np.uint32) if l_mode else None
        out_words = lambda: torch.from_numpy(np.full(4 * (count + pad), fill, np.uint8)).to(dev)  # noqa: E731
        o_idx, o_meta, o_pos = out_words(), out_words(), out_words()
        o_sym = u8(np.full(count + pad, fill, np.uint8)) if l_mode else None
        out = np.zeros(8, np.uint32)
        p = lambda t: None if t is None else _ptr(t)  # noqa: E731
        _inputs_ready(d_idx)
        self._ck(self._lib.dk_dbg_dev_in_place(self._h, int(n), int(h), count, _ptr(d_idx), _ptr(d_pos), _ptr(d_gid), _ptr(d_gstart), len(d_gstart) - 1, _ptr(d_rank),
                                               p(d_sa), p(d_bwt), p(d_sym), p(d_origin), int(chain_group), int(record_cap), int(max_rounds),
                                               int(bool(always_compact)), _ptr(o_idx), _ptr(o_meta), p(o_sym), _ptr(o_pos), _ptr(out)))
        return dict(idx=self._to_host(o_idx, np.uint32), meta=self._to_host(o_meta, np.uint32), pos=self._to_host(o_pos, np.uint32),
                    sym=None if o_sym is None else o_sym.cpu().numpy(), rank=self._to_host(d_rank, np.uint32),
                    sa=None if l_mode else self._to_host(d_sa, np.uint32), bwt=d_bwt.cpu().numpy() if l_mode else None,
                    origin=int(self._to_host(d_origin, np.uint32)[0]) if l_mode else None, slots=int(out[0]), live=int(out[1]), records=int(out[2]),
                    list_full=int(out[3]), settled=int(out[4]), rounds=int(out[5]), compactions=int(out[6]),
                    routes={name for name, bit in _lib.ROUTES.items() if int(out[7]) & bit})

    def _text_at(self, text, offset):
        """the text on the device `offset` bytes behind an aligned address -> (tensor that owns it, address of its first byte)"""
        import torch
        host = np.zeros(len(text) + offset, np.uint8)
        host[offset:] = np.asarray(text, dtype=np.uint8)
        t = torch.from_numpy(host).to("cuda:%d" % self.device)
        return t, t.data_ptr() + offset

    def dbg_dev_round(self, text, h, idx, pos, gid, gstart, rank=None, tsym=0, period=0, next_break=None, sa=None, bwt=None, sym=None, origin=0xC3C3C3C3,
                      text_offset=0, fill=0xC3, pad=64):
        """dk_dbg_dev_round: one general round on a list (suffix, SA position and group per slot, gstart with its end entry).  tsym 0: a doubling
        round on rank; above: a text round; period with next_break: a token round.  sa (n words): the suffix-array mode; bwt (n bytes) with sym: the
        carried-L mode, the origin word holding `origin` before the call.  text_offset: bytes between an aligned address and the text's first.
        Every list output holds `fill` bytes before the call, count + pad entries.
        -> dict: sorted_keys, sorted_idx, sorted_sym, idx, pos, gid, gstart, sym (whole, pad included; the syms None in the sa mode), rank (None
        without), sa or bwt, origin (None in the sa mode) and the counters active, groups, big_slots, big_groups, above_pl_slots, advanced,
        routes (names), kb"""
        import torch
        dev = "cuda:%d" % self.device
        n = len(text)
        d_idx, d_pos, d_gid, d_gstart = (self._to_dev(a, np.uint32) for a in (idx, pos, gid, gstart))
        count = len(d_idx)
        if not (len(d_pos) == len(d_gid) == count) or (sa is None) == (bwt is None) or (bwt is None) != (sym is None):
            raise DarkError(_lib.DK_E_ARG, "list arrays of different lengths, or not exactly one of sa and bwt + sym")
        l_mode = sa is None
        if len(sa if not l_mode else bwt) != n or (l_mode and len(sym) != count) or (rank is not None and len(rank) != n) or \
                (next_break is not None and len(next_break) != n):
            raise DarkError(_lib.DK_E_ARG, "sa / bwt / rank / next_break of n entries, sym of one per slot")
        u8 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8).copy()).to(dev)  # noqa: E731
        keep, d_text = self._text_at(text, text_offset)
        d_rank = None if rank is None else self._to_dev(rank, np.uint32)
        d_nb = None if next_break is None else self._to_dev(next_break, np.uint32)
        d_sa = None if l_mode else self._to_dev(sa, np.uint32)
        d_bwt, d_sym = (u8(bwt), u8(sym)) if l_mode else (None, None)
        d_origin = self._to_dev(np.array([origin], np.uint32), np.uint32) if l_mode else None
        filled = lambda width: torch.from_numpy(np.full(width * (count + pad), fill, np.uint8)).to(dev)  # noqa: E731
        o_skeys, o_sidx, o_idx, o_pos, o_gid, o_gstart = filled(8), filled(4), filled(4), filled(4), filled(4), filled(4)
        o_ssym, o_sym = (filled(1), filled(1)) if l_mode else (None, None)
        out = np.zeros(8, np.uint32)
        p = lambda t: None if t is None else _ptr(t)  # noqa: E731
        _inputs_ready(d_idx)
        self._ck(self._lib.dk_dbg_dev_round(self._h, d_text, n, int(h), count, _ptr(d_idx), _ptr(d_pos), _ptr(d_gid), _ptr(d_gstart), len(d_gstart) - 1, p(d_rank),
                                            int(tsym), int(period), p(d_nb), p(d_sa), p(d_bwt), p(d_sym), p(d_origin), _ptr(o_skeys), _ptr(o_sidx), p(o_ssym),
                                            _ptr(o_idx), _ptr(o_pos), _ptr(o_gid), _ptr(o_gstart), p(o_sym), _ptr(out)))
        del keep
        words = lambda t: self._to_host(t, np.uint32)  # noqa: E731
        return dict(sorted_keys=self._to_host(o_skeys, np.uint64), sorted_idx=words(o_sidx), sorted_sym=None if o_ssym is None else o_ssym.cpu().numpy(),
                    idx=words(o_idx), pos=words(o_pos), gid=words(o_gid), gstart=words(o_gstart), sym=None if o_sym is None else o_sym.cpu().numpy(),
                    rank=None if d_rank is None else words(d_rank), sa=None if l_mode else words(d_sa), bwt=d_bwt.cpu().numpy() if l_mode else None,
                    origin=int(words(d_origin)[0]) if l_mode else None, active=int(out[0]), groups=int(out[1]), big_slots=int(out[2]), big_groups=int(out[3]),
                    above_pl_slots=int(out[4]), advanced=int(out[5]), routes={name for name, bit in _lib.ROUTES.items() if int(out[6]) & bit}, kb=int(out[7]))

    def dbg_dev_period(self, text, period=0, run=False, probe=False, count_p=0, search_pmax=0, prefix=None, text_offset=0, fill=0xC3, pad=64):
        """dk_dbg_dev_period: the period kernels and the probes on a text `text_offset` bytes behind an aligned address.  period: the next-break
        array (n + pad words over `fill`); run / probe: k_run_probe's 2 and k_period_probe's 8 words; count_p: k_period_count's word; search_pmax:
        k_period_search's words; prefix = (m, span, lengths): k_prefix_probe's four.  -> dict of what was asked for: next_break, run, probe,
        count, found, dups"""
        import torch
        n = len(text)
        keep, d_text = self._text_at(text, text_offset)
        d_nb = torch.from_numpy(np.full(4 * (n + pad), fill, np.uint8)).to("cuda:%d" % self.device) if period else None
        host = lambda words, on: np.full(words, 0xC3C3C3C3, np.uint32) if on else None  # noqa: E731
        run_out, probe_out, count_out, found_out, dups_out = host(2, run), host(8, probe), host(1, count_p), host(32, search_pmax), host(4, prefix is not None)
        m, span, lengths = prefix if prefix is not None else (0, 0, None)
        cands = None if lengths is None else np.asarray(lengths, dtype=np.int32)
        p = lambda a: None if a is None else _ptr(a)  # noqa: E731
        _inputs_ready(keep)
        self._ck(self._lib.dk_dbg_dev_period(self._h, d_text, n, int(period), p(d_nb), p(run_out), p(probe_out), int(count_p), p(count_out), int(search_pmax),
                                             p(found_out), int(m), int(span), p(cands), 0 if cands is None else len(cands), p(dups_out)))
        del keep
        return dict(next_break=None if d_nb is None else self._to_host(d_nb, np.uint32), run=run_out, probe=probe_out,
                    count=None if count_out is None else int(count_out[0]), found=found_out, dups=dups_out)

    def dbg_dev_initial_sort(self, text, code, bits, spk, inv=None, narrow=False, text_offset=0, fill=0xC3, pad=64):
        """dk_dbg_dev_initial_sort: the suffix sort's initial sort by itself on a text `text_offset` bytes behind an aligned address, under the
        caller's code table (256 codes below 2^bits).  inv (256 bytes): the carry -- L and the origin word are written.  narrow: 32-bit keys and
        the 256 bucket starts.  Every device output holds `fill` bytes before the call and has `pad` guard entries in front and behind (the origin
        word: one each side).  -> dict of the whole arrays after the call, guards included: keys (uint64, or uint32 when narrow), sa, bwt and
        origin (3 words; both None without the carry), bucket_starts (None unless narrow), and route (DK_ROUTE_* bits), passes, sorted_elements,
        out (the four words)"""
        import torch
        n, kb, carry = len(text), 4 if narrow else 8, inv is not None
        keep, d_text = self._text_at(text, text_offset)
        code = np.ascontiguousarray(code, dtype=np.uint8)
        inv = None if inv is None else np.ascontiguousarray(inv, dtype=np.uint8)
        if len(code) != 256 or (carry and len(inv) != 256):
            raise DarkError(_lib.DK_E_ARG, "code and inv are tables of 256 bytes")
        filled = lambda nbytes: torch.from_numpy(np.full(nbytes, fill, np.uint8)).to("cuda:%d" % self.device)  # noqa: E731
        d_keys, d_sa = filled(kb * (n + 2 * pad)), filled(4 * (n + 2 * pad))
        d_bwt, d_origin = (filled(n + 2 * pad), filled(12)) if carry else (None, None)
        starts = np.full(256, 0xC3C3C3C3, np.uint32) if narrow else None
        out = np.full(4, 0xC3C3C3C3, np.uint32)
        at = lambda t, nbytes: None if t is None else C.c_void_p(t.data_ptr() + nbytes)  # noqa: E731
        _inputs_ready(keep)
        self._ck(self._lib.dk_dbg_dev_initial_sort(self._h, d_text, n, _ptr(code), int(bits), int(spk), None if inv is None else _ptr(inv), int(bool(narrow)),
                                                   at(d_keys, kb * pad), at(d_sa, 4 * pad), at(d_bwt, pad), at(d_origin, 4), None if starts is None else _ptr(starts),
                                                   _ptr(out)))
        del keep
        return dict(keys=self._to_host(d_keys, np.uint32 if narrow else np.uint64), sa=self._to_host(d_sa, np.uint32),
                    bwt=None if d_bwt is None else d_bwt.cpu().numpy(), origin=None if d_origin is None else self._to_host(d_origin, np.uint32),
                    bucket_starts=starts, route=int(out[0]), passes=int(out[1]), sorted_elements=int(out[2]), out=out)

    def dbg_dev_packed_first(self, blocks, fill=0xC3, pad=64):
        """dk_dbg_dev_packed_first: the first step of the segmented suffix sort on the pack `blocks` (byte arrays).  Every device output holds
        `fill` bytes before the call and has `pad` guard entries in front and behind.  -> dict of the whole arrays after the call, guards
        included: keys (uint64), vals, rank, act, and code (256 uint16, over `fill`), out (8 words, over `fill`), live"""
        import torch
        blocks = [np.ascontiguousarray(b, dtype=np.uint8) for b in blocks]
        total = sum(len(b) for b in blocks)
        d_text = torch.from_numpy(np.concatenate(blocks) if blocks else np.zeros(1, np.uint8)).to("cuda:%d" % self.device)
        filled = lambda width: torch.from_numpy(np.full(width * (total + 2 * pad), fill, np.uint8)).to("cuda:%d" % self.device)  # noqa: E731
        d_keys, d_vals, d_rank, d_act = filled(8), filled(4), filled(4), filled(4)
        code, out = np.full(512, fill, np.uint8).view(np.uint16), np.full(32, fill, np.uint8).view(np.uint32)
        at = lambda t, width: C.c_void_p(t.data_ptr() + width * pad)  # noqa: E731
        _inputs_ready(d_text)
        self._ck(self._lib.dk_dbg_dev_packed_first(self._h, _ptr(d_text), len(blocks), _sizes([len(b) for b in blocks]), at(d_keys, 8), at(d_vals, 4),
                                                   at(d_rank, 4), at(d_act, 4), _ptr(code), _ptr(out)))
        words = lambda t: self._to_host(t, np.uint32)  # noqa: E731
        return dict(keys=self._to_host(d_keys, np.uint64), vals=words(d_vals), rank=words(d_rank), act=words(d_act), code=code, out=out, live=int(out[4]))

    def dbg_dev_packed_round(self, sizes, h, act, rank, guard=True, fill=0xC3, pad=64):
        """dk_dbg_dev_packed_round: one round of the segmented suffix sort at depth h on the list `act` and the ranks `rank` (one word per byte of
        the pack of blocks of `sizes` bytes), and the guard words of the next list (guard=False: a null d_guard).  Every device output holds `fill`
        bytes before the call and has `pad` guard entries in front and behind; rank stands between such guards too.  -> dict of the whole
        arrays after the call, guards included: keys (uint64), vals, next_act, rank, guard (None without), and out (8 words, over `fill`), live"""
        import torch
        dev = "cuda:%d" % self.device
        act, rank = np.ascontiguousarray(act, dtype=np.uint32), np.ascontiguousarray(rank, dtype=np.uint32)
        if len(rank) != sum(int(n) for n in sizes):
            raise DarkError(_lib.DK_E_ARG, "rank holds one word per byte of the pack")
        c = len(act)
        guards = np.full(pad, fill * 0x01010101, np.uint32)
        d_act = self._to_dev(act if c else np.zeros(1, np.uint32), np.uint32)
        d_rank = self._to_dev(np.concatenate([guards, rank, guards]), np.uint32)
        filled = lambda width, entries: torch.from_numpy(np.full(width * (entries + 2 * pad), fill, np.uint8)).to(dev)  # noqa: E731
        d_keys, d_vals, d_next = filled(8, c), filled(4, c), filled(4, c)
        d_guard = filled(4, len(sizes)) if guard else None
        out = np.full(32, fill, np.uint8).view(np.uint32)
        at = lambda t, width: None if t is None else C.c_void_p(t.data_ptr() + width * pad)  # noqa: E731
        _inputs_ready(d_act)
        self._ck(self._lib.dk_dbg_dev_packed_round(self._h, len(sizes), _sizes(sizes), int(h), _ptr(d_act), c, at(d_rank, 4), at(d_keys, 8), at(d_vals, 4),
                                                   at(d_next, 4), at(d_guard, 4), _ptr(out)))
        words = lambda t: self._to_host(t, np.uint32)  # noqa: E731
        return dict(keys=self._to_host(d_keys, np.uint64), vals=words(d_vals), next_act=words(d_next), rank=words(d_rank),
                    guard=None if d_guard is None else words(d_guard), out=out, live=int(out[2]))

    def dbg_dev_inverse_permutation(self, sa, marked_val=None):
        """dk_dbg_dev_inverse_permutation: rank[sa[p] & 0x7FFFFFFF] = marked_val[p] if sa[p] has bit 31 set (and marked_val is given) else p"""
        d_sa = self._to_dev(sa, np.uint32)
        d_mv = None if marked_val is None else self._to_dev(marked_val, np.uint32)
        if d_mv is not None and len(d_mv) != len(d_sa):
            raise DarkError(_lib.DK_E_ARG, "%d entries, %d values for the marked ones" % (len(d_sa), len(d_mv)))
        d_rank = self._to_dev(np.full(len(d_sa), 0xFFFFFFFF, np.uint32), np.uint32)
        _inputs_ready(d_sa)
        self._ck(self._lib.dk_dbg_dev_inverse_permutation(self._h, _ptr(d_sa), len(d_sa), _ptr(d_rank), _ptr(d_mv) if d_mv is not None else None))
        return self._to_host(d_rank, np.uint32)


class _LenRef:
    """one entry of a packed push's length array, read like a c_size_t"""

    def __init__(self, arr, i):
        self._arr, self._i = arr, i

    @property
    def value(self):
        return self._arr[self._i]


class Batch:
    """dk_batch_begin / _push / _finish: the pipelined encoder fed one block at a time.

    The C coding threads write into this object's `out` buffers and length words until dk_batch_finish has joined them, so finish
    ALWAYS runs before those buffers or the context can go away: on a failed push (the error is raised after the batch is closed), at
    the end of a `with` block, from Context.close(), and as a last resort from __del__."""

    def __init__(self, ctx, model, host_threads):
        self._ctx = ctx
        self._h = C.c_void_p()
        self._outs, self._lens = [], []
        self._keep = []  # ctypes arrays the coding threads of packed pushes write into
        self._model = model_id(model)
        ctx._ck(ctx._lib.dk_batch_begin(ctx._h, model_id(model), int(host_threads), C.byref(self._h)))
        ctx._batch = self

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def push(self, d_in, n):
        """device stages of one block now (d_in may be reused when this returns), coding in the background"""
        if not self._h:
            raise DarkError(_lib.DK_E_ARG, "the batch is closed")
        _inputs_ready(d_in)
        out = np.empty(2 * int(n) + 4096 + _prefix(self._model), dtype=np.uint8)  # virtual until written: only the coded bytes become resident
        ln = C.c_size_t(0)
        self._outs.append(out)
        self._lens.append(ln)
        rc = self._ctx._lib.dk_batch_push(self._h, _ptr(d_in), int(n), _ptr(out), len(out), C.byref(ln))
        if rc != 0:
            text = (self._ctx._lib.dk_last_error(self._ctx._h) or b"").decode()
            self.close()  # joins the coders of the blocks already queued; only then may the buffers die with this object
            raise DarkError(rc, text)

    def push_packed(self, d_in, sizes):
        """device stages of a whole pack now (one segmented pass), every block queued as its own coding job; returns the blocks'
        DK_FLAG_* words.  Their streams come out of finish() in push order, with those of the other pushes."""
        if not self._h:
            raise DarkError(_lib.DK_E_ARG, "the batch is closed")
        _inputs_ready(d_in)
        count = len(sizes)
        outs = [np.empty(_stream_cap(self._model, n), dtype=np.uint8) for n in sizes]
        lens = (C.c_size_t * max(count, 1))()
        ns = _sizes(sizes)
        optrs = (C.c_void_p * count)(*[_ptr(o) for o in outs])
        caps = (C.c_size_t * count)(*[len(o) for o in outs])
        flags = (C.c_uint * max(count, 1))()
        self._outs.extend(outs)
        self._keep.append((lens, ns, optrs, caps))
        self._lens.extend(_LenRef(lens, i) for i in range(count))
        rc = self._ctx._lib.dk_batch_push_packed(self._h, _ptr(d_in), count, ns, optrs, caps, lens, flags)
        if rc != 0:
            text = (self._ctx._lib.dk_last_error(self._ctx._h) or b"").decode()
            self.close()
            raise DarkError(rc, text)
        return [int(flags[i]) for i in range(count)]

    def close(self):
        """dk_batch_finish without collecting anything (idempotent); returns its code"""
        h, self._h = self._h, None
        if not h:
            return 0
        if getattr(self._ctx, "_batch", None) is self:
            self._ctx._batch = None
        return self._ctx._lib.dk_batch_finish(h)

    def finish(self):
        if not self._h:
            raise DarkError(_lib.DK_E_ARG, "the batch is closed")
        self._ctx._ck(self.close())
        return [o[:ln.value] for o, ln in zip(self._outs, self._lens)]


def multi_block_encode(model, blocks, devices, host_threads_per_gpu=4):
    """dk_multi_block_encode: block i -> GPU devices[i mod len(devices)], one host thread + one context per listed device inside the call"""
    lib = _lib.load()
    keep = [as_u8(b) for b in blocks]
    count = len(keep)
    mid = model_id(model)
    outs = [np.empty(2 * len(b) + 4096 + _prefix(mid), dtype=np.uint8) for b in keep]
    devs = (C.c_int * len(devices))(*[int(d) for d in devices])
    ins = (C.c_void_p * count)(*[_ptr(b) for b in keep])
    ns = (C.c_size_t * count)(*[len(b) for b in keep])
    optrs = (C.c_void_p * count)(*[_ptr(o) for o in outs])
    caps = (C.c_size_t * count)(*[len(o) for o in outs])
    lens = (C.c_size_t * count)()
    err = C.create_string_buffer(512)
    rc = lib.dk_multi_block_encode(devs, len(devices), mid, count, ins, ns, optrs, caps, lens, int(host_threads_per_gpu), err, 512)
    if rc:
        raise DarkError(rc, err.value.decode())
    return [o[:lens[i]].tobytes() for i, o in enumerate(outs)]


def multi_block_decode(model, streams, sizes, devices, host_threads_per_gpu=4):
    lib = _lib.load()
    keep = [as_u8(s) for s in streams]
    count = len(keep)
    outs = [np.empty(int(n), dtype=np.uint8) for n in sizes]
    devs = (C.c_int * len(devices))(*[int(d) for d in devices])
    ins = (C.c_void_p * count)(*[_ptr(s) for s in keep])
    lens = (C.c_size_t * count)(*[len(s) for s in keep])
    ns = _sizes(sizes)
    optrs = (C.c_void_p * count)(*[_ptr(o) for o in outs])
    err = C.create_string_buffer(512)
    rc = lib.dk_multi_block_decode(devs, len(devices), model_id(model), count, ins, lens, ns, optrs, int(host_threads_per_gpu), err, 512)
    if rc:
        raise DarkError(rc, err.value.decode())
    return [o.tobytes() for o in outs]
