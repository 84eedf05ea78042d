"""FM-index over the library's BWT: count the occurrences of patterns without the text and without a suffix array,
say where they are from a sampled suffix array (section 4.14) and what the text says there from sampled inverse-suffix-array entries (section
4.15).  The reference has no counterpart.  L and the index stay on the GPU, about two bytes per text byte; the locate structure adds about
n / 8 + 4 n / locate_step, the extract structure 4 n / extract_step."""
import numpy as np

from .context import Context, DarkError, _pack_patterns, as_u8, fm_extract_bytes, fm_index_bytes, fm_locate_bytes
from . import _lib


def classes(pattern, ignore_case=False, wildcard=None):
    """the byte classes of a pattern for Index.near (section 4.18): an m x 32 uint8 array, row j the set of byte values position j matches, bit
    c & 7 of byte c >> 3 for byte value c.  Every position is the one-bit class of its byte; under ignore_case an ASCII letter gets the bits
    of both its cases; the byte value `wildcard`, if given, becomes the full class."""
    p = as_u8(pattern).astype(np.int64)
    out = np.zeros((len(p), 32), dtype=np.uint8)
    rows = np.arange(len(p))
    out[rows, p >> 3] = (1 << (p & 7)).astype(np.uint8)
    if ignore_case:
        letter = ((p | 0x20) >= 0x61) & ((p | 0x20) <= 0x7A)
        other = p ^ 0x20
        out[rows[letter], other[letter] >> 3] |= (1 << (other[letter] & 7)).astype(np.uint8)
    if wildcard is not None:
        out[p == int(wildcard)] = 0xFF
    return out


_classes = classes  # (Index.near has a keyword of that name)


class Index:
    """The index of one block, or of a pack of blocks (`sizes` their lengths, `origins` their origins).

    Index.from_text(ctx, data)          forward BWT on the GPU (a full context), then the index; the text is not kept
    Index.from_bwt(ctx, bwt, origin)    from (L, origin) in host memory or in a device tensor -- any context, a decoder context included
    Index.from_bwt_packed(ctx, d_bwt, sizes, origins)
    count(patterns[, blocks]) -> (lo, hi) uint32 arrays: the numbers Context.sa_search gives; occurrences(patterns[, blocks]) = hi - lo.
    locate_step (keyword of all four; None: no structure, count only): a power of two in [1, 4096], the distance of the sampled text positions.
    32 is a reasoned choice, not a measured one.
    locate(patterns[, blocks], max_hits=16) -> a list of uint32 arrays, the first max_hits positions of every pattern in suffix-array order.
    extract_step (keyword of all four; None: no structure): a power of two in [1, 4096], the distance of the anchored text positions (section 4.15).
    extract(positions, length[, blocks]) -> a list of bytes, the text at [position, position + length) cut at the block's end; text([block]) ->
    the whole block; snippets(patterns, before, after[, blocks], max_hits=16) -> per pattern a list of (position, bytes around the hit).
    find(patterns, max_hits=65536) -> (occ, hits, total): every pattern in EVERY block as one compact list of (pattern, block, position, slot)
    records (section 4.16); grep(patterns, before, after) -> (pattern, block, position, bytes around the hit) per record.
    seams(patterns, prev=b"", max_hits=65536) -> (occ, hits, total): the matches find cannot see, those that straddle a border between two
    blocks or between `prev` and the first block (section 4.17); tail(nbytes) -> the last bytes of the whole text, the `prev` of what follows.
    near(patterns, k=0, ignore_case=False, wildcard=None) -> (occ, hits, total, cut): find with byte classes at the pattern's positions and up
    to k of them missed (section 4.18), records (pattern, block, position, cost); near_grep(...) -> the same with the bytes around each hit."""

    def __init__(self, ctx, d_bwt, sizes, origins, locate_step=None, extract_step=None):
        import torch
        self._ctx = ctx
        self.sizes = [int(n) for n in sizes]
        self.origins = [int(o) for o in origins]
        self.total = sum(self.sizes)
        nbytes = fm_index_bytes(self.total, len(self.sizes))
        if nbytes == 0:
            raise DarkError(_lib.DK_E_ARG, "no index for %d blocks of %d bytes together" % (len(self.sizes), self.total))
        self.d_bwt = d_bwt
        self.d_index = torch.empty(nbytes // 4, dtype=torch.int32, device=d_bwt.device)
        if len(self.sizes) == 1:
            ctx.dev_fm_build(d_bwt, self.total, self.origins[0], self.d_index)
        else:
            ctx.dev_fm_build_packed(d_bwt, self.sizes, self.origins, self.d_index)
        self.locate_step = None if locate_step is None else int(locate_step)
        self.d_loc = None
        if locate_step is not None:
            nbytes = fm_locate_bytes(self.total, len(self.sizes), self.locate_step)
            if nbytes == 0:
                raise DarkError(_lib.DK_E_ARG, "locate_step %r is no power of two in [1, 4096]" % (locate_step,))
            self.d_loc = torch.empty(nbytes // 4, dtype=torch.int32, device=d_bwt.device)
            if len(self.sizes) == 1:
                ctx.dev_fm_locate_build(d_bwt, self.total, self.origins[0], self.locate_step, self.d_loc)
            else:
                ctx.dev_fm_locate_build_packed(d_bwt, self.sizes, self.origins, self.locate_step, self.d_loc)
        self.extract_step = None if extract_step is None else int(extract_step)
        self.d_ext = None
        if extract_step is not None:
            nbytes = fm_extract_bytes(self.total, len(self.sizes), self.extract_step)
            if nbytes == 0:
                raise DarkError(_lib.DK_E_ARG, "extract_step %r is no power of two in [1, 4096]" % (extract_step,))
            self.d_ext = torch.empty(nbytes // 4, dtype=torch.int32, device=d_bwt.device)
            if len(self.sizes) == 1:
                ctx.dev_fm_extract_build(d_bwt, self.total, self.origins[0], self.extract_step, self.d_ext)
            else:
                ctx.dev_fm_extract_build_packed(d_bwt, self.sizes, self.origins, self.extract_step, self.d_ext)

    @classmethod
    def from_text(cls, ctx, data, locate_step=None, extract_step=None):
        import torch
        t = as_u8(data)
        d_in = torch.from_numpy(t.copy()).to("cuda:%d" % ctx.device)
        d_bwt = torch.empty_like(d_in)
        origin = ctx.dev_bwt_forward(d_in, len(t), d_bwt)
        return cls(ctx, d_bwt, [len(t)], [origin], locate_step, extract_step)

    @classmethod
    def from_bwt(cls, ctx, bwt, origin, locate_step=None, extract_step=None):
        import torch
        if not hasattr(bwt, "data_ptr"):
            bwt = torch.from_numpy(as_u8(bwt).copy()).to("cuda:%d" % ctx.device)
        return cls(ctx, bwt, [bwt.numel()], [origin], locate_step, extract_step)

    @classmethod
    def from_bwt_packed(cls, ctx, d_bwt, sizes, origins, locate_step=None, extract_step=None):
        return cls(ctx, d_bwt, sizes, origins, locate_step, extract_step)

    def resident_bytes(self):
        """device bytes the index needs to answer: L and the index, and the locate and extract structures where they were built"""
        return self.total + self.d_index.numel() * 4 + sum(d.numel() * 4 for d in (self.d_loc, self.d_ext) if d is not None)

    def count(self, patterns, blocks=None):
        npat = len(patterns)
        if npat == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        d_lo, d_hi = self._count_dev(patterns, blocks)
        return d_lo.cpu().numpy().view(np.uint32), d_hi.cpu().numpy().view(np.uint32)

    def _count_dev(self, patterns, blocks):
        import torch
        pat, lens, npat = _pack_patterns(patterns)
        dev = self.d_bwt.device
        d_pat = torch.from_numpy(pat).to(dev)
        d_lo = torch.empty(npat, dtype=torch.int32, device=dev)
        d_hi = torch.empty(npat, dtype=torch.int32, device=dev)
        if len(self.sizes) == 1 and blocks is None:
            self._ctx.dev_fm_count(self.d_bwt, self.total, self.d_index, d_pat, list(lens)[:npat], d_lo, d_hi)
        else:
            if blocks is None:
                raise DarkError(_lib.DK_E_ARG, "an index over a pack needs the block of every pattern")
            self._ctx.dev_fm_count_packed(self.d_bwt, self.sizes, self.d_index, d_pat, list(lens)[:npat], blocks, d_lo, d_hi)
        return d_lo, d_hi

    def locate(self, patterns, blocks=None, max_hits=16):
        """per pattern a uint32 array of its first min(occurrences, max_hits) text positions (local to its block), in suffix-array order"""
        import torch
        if self.d_loc is None:
            raise DarkError(_lib.DK_E_ARG, "the index was built without a locate structure (locate_step=None)")
        npat = len(patterns)
        if npat == 0:
            return []
        pos = self._locate_dev(patterns, blocks, max_hits).cpu().numpy().view(np.uint32).reshape(npat, -1)
        return [row[row != _lib.FM_NO_HIT] for row in pos]

    def _locate_dev(self, patterns, blocks, max_hits):
        """count, then locate: the rows of dev_fm_locate as an int32 device tensor (FM_NO_HIT reads as -1)"""
        import torch
        npat = len(patterns)
        d_lo, d_hi = self._count_dev(patterns, blocks)
        d_pos = torch.empty(npat * max(int(max_hits), 1), dtype=torch.int32, device=self.d_bwt.device)
        if len(self.sizes) == 1 and blocks is None:
            self._ctx.dev_fm_locate(self.d_bwt, self.total, self.d_index, self.d_loc, self.locate_step, d_lo, d_hi, npat, max_hits, d_pos)
        else:
            self._ctx.dev_fm_locate_packed(self.d_bwt, self.sizes, self.d_index, self.d_loc, self.locate_step, d_lo, d_hi, blocks, max_hits, d_pos)
        return d_pos

    def _extract_dev(self, d_pos, d_len, nrange, blocks, max_len):
        """rows of dev_fm_extract(_packed) for int32 device tensors of starts and lengths (d_len None: max_len each)"""
        import torch
        if self.d_ext is None:
            raise DarkError(_lib.DK_E_ARG, "the index was built without an extract structure (extract_step=None)")
        d_out = torch.empty(nrange * max(int(max_len), 1), dtype=torch.uint8, device=self.d_bwt.device)
        if len(self.sizes) == 1 and blocks is None:
            self._ctx.dev_fm_extract(self.d_bwt, self.total, self.d_index, self.d_ext, self.extract_step, d_pos, d_len, nrange, max_len, d_out)
        else:
            if blocks is None:
                raise DarkError(_lib.DK_E_ARG, "an index over a pack needs the block of every range")
            self._ctx.dev_fm_extract_packed(self.d_bwt, self.sizes, self.d_index, self.d_ext, self.extract_step, d_pos, d_len, blocks, max_len, d_out)
        return d_out

    def extract(self, positions, length, blocks=None):
        """per position the text at [position, position + length) of its block as bytes, cut at the block's end (empty behind it)"""
        import torch
        nrange = len(positions)
        if self.d_ext is None:
            raise DarkError(_lib.DK_E_ARG, "the index was built without an extract structure (extract_step=None)")
        if nrange == 0:
            return []
        pos = np.array(positions, dtype=np.int64)
        d_pos = torch.from_numpy(pos.astype(np.uint32).view(np.int32)).to(self.d_bwt.device)
        rows = self._extract_dev(d_pos, None, nrange, blocks, length).cpu().numpy().reshape(nrange, -1)
        sizes = np.array(self.sizes, dtype=np.int64)[np.zeros(nrange, np.int64) if blocks is None else np.array(blocks, dtype=np.int64)]
        got = np.clip(np.minimum(int(length), sizes - pos), 0, None)
        return [bytes(rows[q, :got[q]]) for q in range(nrange)]

    def text(self, block=0):
        """the whole text of a block"""
        return self.extract([0], self.sizes[block], None if len(self.sizes) == 1 else [block])[0]

    def snippets(self, patterns, before, after, blocks=None, max_hits=16):
        """per pattern a list of (position, bytes): its first max_hits occurrences in suffix-array order, each with the text from `before` bytes
        in front of it to `after` bytes behind it, cut at the block's ends.  Count, locate and extract run back to back on the device; only the
        positions and the rows are read back."""
        import torch
        if self.d_loc is None or self.d_ext is None:
            raise DarkError(_lib.DK_E_ARG, "snippets need both structures (locate_step and extract_step)")
        npat, max_hits, before, after = len(patterns), max(int(max_hits), 1), int(before), int(after)
        if npat == 0:
            return []
        dev = self.d_bwt.device
        d_hit = self._locate_dev(patterns, blocks, max_hits)  # npat x max_hits positions, -1 where there is none
        plen = np.repeat(np.array([len(p) for p in patterns], dtype=np.int32), max_hits)
        found = d_hit >= 0
        d_start = torch.clamp(d_hit - before, min=0)
        d_len = torch.where(found, d_hit - d_start + torch.from_numpy(plen).to(dev) + after, torch.zeros_like(d_hit))
        d_start = torch.where(found, d_start, d_hit)
        max_len = before + int(plen.max()) + after
        where = None if blocks is None else [b for b in blocks for _ in range(max_hits)]
        rows = self._extract_dev(d_start, d_len, npat * max_hits, where, max_len).cpu().numpy().reshape(npat * max_hits, -1)
        hit = d_hit.cpu().numpy().astype(np.int64)
        sizes = np.array(self.sizes, dtype=np.int64)[np.zeros(len(hit), np.int64) if where is None else np.array(where, dtype=np.int64)]
        start = np.maximum(hit - before, 0)
        got = np.minimum(hit - start + plen + after, sizes - start)
        return [[(int(hit[i]), bytes(rows[i, :got[i]])) for i in range(q * max_hits, (q + 1) * max_hits) if hit[i] >= 0] for q in range(npat)]

    def find(self, patterns, max_hits=65536):
        """every pattern in every block (section 4.16) -> (occ, hits, total): occ a uint32 array of len(patterns) x blocks, hits a structured
        array (pattern, block, position, slot) of the first min(total, max_hits) hits in the order (pattern, block, suffix-array slot), total
        the number of hits in all.  max_hits=0 needs no locate structure.  The default 65536 (1 MiB of records) is a choice, not a measurement."""
        import torch
        from .context import FM_HIT_DTYPE
        npat, count, max_hits = len(patterns), len(self.sizes), int(max_hits)
        if max_hits and self.d_loc is None:
            raise DarkError(_lib.DK_E_ARG, "the index was built without a locate structure (locate_step=None): only max_hits=0 is served")
        if npat == 0:
            return np.zeros((0, count), np.uint32), np.zeros(0, FM_HIT_DTYPE), 0
        pat, lens, npat = _pack_patterns(patterns)
        dev = self.d_bwt.device
        d_pat = torch.from_numpy(pat).to(dev)
        d_occ = torch.empty(npat * count, dtype=torch.int32, device=dev)
        d_hits = torch.empty(4 * max_hits, dtype=torch.int32, device=dev) if max_hits else None  # (torch allocations are 256-byte aligned)
        step = self.locate_step if self.locate_step is not None else 32
        if count == 1:
            total = self._ctx.dev_fm_find(self.d_bwt, self.total, self.d_index, self.d_loc, step, d_pat, list(lens)[:npat], max_hits, d_hits, d_occ)
        else:
            total = self._ctx.dev_fm_find_packed(self.d_bwt, self.sizes, self.d_index, self.d_loc, step, d_pat, list(lens)[:npat], max_hits, d_hits,
                                                 d_occ)
        got = min(total, max_hits)
        hits = d_hits[:4 * got].cpu().numpy().view(FM_HIT_DTYPE) if got else np.zeros(0, FM_HIT_DTYPE)
        return d_occ.cpu().numpy().view(np.uint32).reshape(npat, count), hits, total

    def grep(self, patterns, before, after, max_hits=65536):
        """a list of (pattern, block, position, bytes) for the hits of find(patterns, max_hits), in its order: bytes is the text from `before`
        bytes in front of the hit to `after` bytes behind it, cut at the block's ends.  One find, the hits read back, one extract with a
        window per hit; the blocks come from the records.  Needs both structures, as snippets does."""
        import torch
        if self.d_loc is None or self.d_ext is None:
            raise DarkError(_lib.DK_E_ARG, "grep needs both structures (locate_step and extract_step)")
        before, after = int(before), int(after)
        _, hits, _ = self.find(patterns, max_hits)
        hits = hits[hits["position"] != _lib.FM_NO_HIT]
        if len(hits) == 0:
            return []
        plen = np.array([len(as_u8(p)) for p in patterns], dtype=np.int64)[hits["pattern"]]
        pos, blk = hits["position"].astype(np.int64), hits["block"].astype(np.int64)
        start = np.maximum(pos - before, 0)
        got = np.minimum(pos - start + plen + after, np.array(self.sizes, dtype=np.int64)[blk] - start)
        max_len = max(int(got.max()), 1)
        dev = self.d_bwt.device
        d_start = torch.from_numpy(start.astype(np.uint32).view(np.int32)).to(dev)
        d_len = torch.from_numpy(got.astype(np.uint32).view(np.int32)).to(dev)
        where = None if len(self.sizes) == 1 else [int(b) for b in blk]
        rows = self._extract_dev(d_start, d_len, len(hits), where, max_len).cpu().numpy().reshape(len(hits), -1)
        return [(int(hits["pattern"][i]), int(blk[i]), int(pos[i]), bytes(rows[i, :got[i]])) for i in range(len(hits))]

    def near(self, patterns, k=0, ignore_case=False, wildcard=None, classes=None, max_hits=65536, node_limit=0):
        """every pattern in every block with at most k positions missed (section 4.18) -> (occ, hits, total, cut): occ a uint32 array of
        patterns x blocks, hits a structured array (pattern, block, position, cost) of the first min(total, max_hits) hits in the order
        (pattern, block, preorder of the pair's search tree, suffix-array slot), total the hits in all, cut the (pattern, block) pairs that
        stopped at node_limit nodes (0: FM_NEAR_NODE_LIMIT) and whose occ is a lower bound.  A pattern's positions are byte classes: those of
        fm.classes(pattern, ignore_case, wildcard), or ready-made m x 32 arrays given as classes= in place of `patterns`.  max_hits=0 needs no
        locate structure."""
        import torch
        from .context import FM_NEAR_HIT_DTYPE
        made = [np.ascontiguousarray(c, dtype=np.uint8).reshape(-1, 32) for c in classes] if classes is not None else \
            [_classes(p, ignore_case, wildcard) for p in patterns]
        npat, count, max_hits = len(made), len(self.sizes), int(max_hits)
        if max_hits and self.d_loc is None:
            raise DarkError(_lib.DK_E_ARG, "the index was built without a locate structure (locate_step=None): only max_hits=0 is served")
        if npat == 0:
            return np.zeros((0, count), np.uint32), np.zeros(0, FM_NEAR_HIT_DTYPE), 0, 0
        lens = [len(c) for c in made]
        dev = self.d_bwt.device
        flat = np.concatenate(made).reshape(-1) if sum(lens) else np.zeros(32, np.uint8)  # (never read: every pattern is empty)
        d_cls = torch.from_numpy(flat).to(dev)
        d_occ = torch.empty(npat * count, dtype=torch.int32, device=dev)
        d_hits = torch.empty(4 * max_hits, dtype=torch.int32, device=dev) if max_hits else None  # (torch allocations are 256-byte aligned)
        step = self.locate_step if self.locate_step is not None else 32
        if count == 1:
            total, cut = self._ctx.dev_fm_near(self.d_bwt, self.total, self.d_index, self.d_loc, step, d_cls, lens, k, node_limit, max_hits, d_hits,
                                               d_occ)
        else:
            total, cut = self._ctx.dev_fm_near_packed(self.d_bwt, self.sizes, self.d_index, self.d_loc, step, d_cls, lens, k, node_limit, max_hits,
                                                      d_hits, d_occ)
        got = min(total, max_hits)
        hits = d_hits[:4 * got].cpu().numpy().view(FM_NEAR_HIT_DTYPE) if got else np.zeros(0, FM_NEAR_HIT_DTYPE)
        return d_occ.cpu().numpy().view(np.uint32).reshape(npat, count), hits, total, cut

    def near_grep(self, patterns, before, after, k=0, ignore_case=False, wildcard=None, classes=None, max_hits=65536, node_limit=0):
        """a list of (pattern, block, position, cost, bytes) for the hits of near(...), in its order: bytes is the text from `before` bytes in
        front of the hit to `after` bytes behind it, cut at the block's ends.  One near, the hits read back, one extract with a window per hit,
        as grep does.  Needs both structures."""
        if self.d_loc is None or self.d_ext is None:
            raise DarkError(_lib.DK_E_ARG, "near_grep needs both structures (locate_step and extract_step)")
        _, hits, _, _ = self.near(patterns, k, ignore_case, wildcard, classes, max_hits, node_limit)
        lens = [len(np.asarray(c).reshape(-1, 32)) for c in classes] if classes is not None else [len(as_u8(p)) for p in patterns]
        return self.near_windows(hits, lens, before, after)

    def near_windows(self, hits, lens, before, after):
        """near_grep's second half: the records of near(...) with the text around them; lens: the patterns' lengths.  One extract call."""
        import torch
        before, after = int(before), int(after)
        hits = hits[hits["position"] != _lib.FM_NO_HIT]
        if len(hits) == 0:
            return []
        plen = np.array(lens, dtype=np.int64)[hits["pattern"]]
        pos, blk = hits["position"].astype(np.int64), hits["block"].astype(np.int64)
        start = np.maximum(pos - before, 0)
        got = np.minimum(pos - start + plen + after, np.array(self.sizes, dtype=np.int64)[blk] - start)
        max_len = max(int(got.max()), 1)
        dev = self.d_bwt.device
        d_start = torch.from_numpy(start.astype(np.uint32).view(np.int32)).to(dev)
        d_len = torch.from_numpy(got.astype(np.uint32).view(np.int32)).to(dev)
        where = None if len(self.sizes) == 1 else [int(b) for b in blk]
        rows = self._extract_dev(d_start, d_len, len(hits), where, max_len).cpu().numpy().reshape(len(hits), -1)
        return [(int(hits["pattern"][i]), int(blk[i]), int(pos[i]), int(hits["cost"][i]), bytes(rows[i, :got[i]])) for i in range(len(hits))]

    def seams(self, patterns, prev=b"", max_hits=65536):
        """the matches that straddle block borders (section 4.17) -> (occ, hits, total).  `prev` and the blocks are the consecutive pieces of one
        text; a seam hit has its first and its last byte in different pieces and belongs to the block of its last byte.  occ: a uint32 array
        len(patterns) x blocks; hits: a structured array (pattern, block, back, reserved) of the first min(total, max_hits) in the order (pattern,
        block, back descending), back = the match's bytes in front of that block.  Only the last longest - 1 bytes of `prev` can matter and only
        they are uploaded.  find(...) and seams(...) together are every occurrence in prev + text that does not lie inside prev, each once."""
        import torch
        from .context import FM_SEAM_HIT_DTYPE
        if self.d_ext is None:
            raise DarkError(_lib.DK_E_ARG, "the index was built without an extract structure (extract_step=None)")
        npat, count, max_hits = len(patterns), len(self.sizes), int(max_hits)
        if npat == 0:
            return np.zeros((0, count), np.uint32), np.zeros(0, FM_SEAM_HIT_DTYPE), 0
        pat, lens, npat = _pack_patterns(patterns)
        dev = self.d_bwt.device
        keep = max(max(list(lens)[:npat]) - 1, 0)
        prev = as_u8(prev)
        prev = prev[len(prev) - min(len(prev), keep):]
        d_prev = torch.from_numpy(prev.copy()).to(dev) if len(prev) else None
        d_pat = torch.from_numpy(pat).to(dev)
        d_occ = torch.empty(npat * count, dtype=torch.int32, device=dev)
        d_hits = torch.empty(4 * max_hits, dtype=torch.int32, device=dev) if max_hits else None  # (torch allocations are 256-byte aligned)
        if count == 1:
            total = self._ctx.dev_fm_seams(self.d_bwt, self.total, self.d_index, self.d_ext, self.extract_step, d_prev, d_pat, list(lens)[:npat],
                                           max_hits, d_hits, d_occ)
        else:
            total = self._ctx.dev_fm_seams_packed(self.d_bwt, self.sizes, self.d_index, self.d_ext, self.extract_step, d_prev, d_pat,
                                                  list(lens)[:npat], max_hits, d_hits, d_occ)
        got = min(total, max_hits)
        hits = d_hits[:4 * got].cpu().numpy().view(FM_SEAM_HIT_DTYPE) if got else np.zeros(0, FM_SEAM_HIT_DTYPE)
        return d_occ.cpu().numpy().view(np.uint32).reshape(npat, count), hits, total

    def _pieces_before(self, block, nbytes):
        """(block, start, length) of the pieces that make the last min(nbytes, bytes in front) bytes in front of block `block`, in text order"""
        want, pieces = int(nbytes), []
        for b in range(block - 1, -1, -1):
            if want <= 0:
                break
            take = min(self.sizes[b], want)
            pieces.append((b, self.sizes[b] - take, take))
            want -= take
        return pieces[::-1]

    def _extract_pieces(self, groups):
        """the bytes of every group of (block, start, length) pieces, joined per group; ONE extract call for all of them"""
        import torch
        pieces = [p for g in groups for p in g]
        if not pieces:
            return [b"" for _ in groups]
        dev = self.d_bwt.device
        d_pos = torch.tensor([p for _, p, _ in pieces], dtype=torch.int64).to(torch.int32).to(dev)
        d_len = torch.tensor([n for _, _, n in pieces], dtype=torch.int64).to(torch.int32).to(dev)
        max_len = max(n for _, _, n in pieces)
        where = None if len(self.sizes) == 1 else [b for b, _, _ in pieces]
        rows = self._extract_dev(d_pos, d_len, len(pieces), where, max_len).cpu().numpy().reshape(len(pieces), -1)
        out, i = [], 0
        for g in groups:
            out.append(b"".join(bytes(rows[i + j, :g[j][2]]) for j in range(len(g))))
            i += len(g)
        return out

    def tail(self, nbytes):
        """the last min(nbytes, total) bytes of the pack's concatenated text, across block borders, in one extract call"""
        if self.d_ext is None:
            raise DarkError(_lib.DK_E_ARG, "the index was built without an extract structure (extract_step=None)")
        return self._extract_pieces([self._pieces_before(len(self.sizes), nbytes)])[0]

    def edges(self, blocks, nfront, nhead):
        """per block of `blocks` (front, head): the last min(nfront, bytes in front) bytes of the pack's text in front of the block, across block
        borders, and the block's first min(nhead, n_b) bytes -- the text around the border a seam hit crosses last.  One extract call."""
        if self.d_ext is None:
            raise DarkError(_lib.DK_E_ARG, "the index was built without an extract structure (extract_step=None)")
        groups = []
        for b in blocks:
            groups += [self._pieces_before(b, nfront), [(b, 0, min(self.sizes[b], int(nhead)))]]
        got = self._extract_pieces(groups)
        return [(got[2 * i], got[2 * i + 1]) for i in range(len(blocks))]

    def occurrences(self, patterns, blocks=None):
        lo, hi = self.count(patterns, blocks)
        return (hi - lo).astype(np.uint32)


__all__ = ["Index", "classes", "Context", "fm_index_bytes", "fm_locate_bytes", "fm_extract_bytes"]
