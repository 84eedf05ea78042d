"""FM-index over the library's BWT: count the occurrences of patterns without the text and without a suffix array,
and say where they are from a sampled suffix array (section 4.14).  The reference has no counterpart.  L and the index stay on the GPU, about two
bytes per text byte; the locate structure adds about n / 8 + 4 n / locate_step."""
import numpy as np

from .context import Context, DarkError, _pack_patterns, as_u8, fm_index_bytes, fm_locate_bytes
from . import _lib


class Index:
    """The index of one block, or of a pack of blocks (`sizes` their lengths, `origins` their origins).

    Index.from_text(ctx, data)          forward BWT on the GPU (a full context), then the index; the text is not kept
    Index.from_bwt(ctx, bwt, origin)    from (L, origin) in host memory or in a device tensor -- any context, a decoder context included
    Index.from_bwt_packed(ctx, d_bwt, sizes, origins)
    count(patterns[, blocks]) -> (lo, hi) uint32 arrays: the numbers Context.sa_search gives; occurrences(patterns[, blocks]) = hi - lo.
    locate_step (keyword of all four; None: no structure, count only): a power of two in [1, 4096], the distance of the sampled text positions.
    32 is a reasoned choice, not a measured one.
    locate(patterns[, blocks], max_hits=16) -> a list of uint32 arrays, the first max_hits positions of every pattern in suffix-array order."""

    def __init__(self, ctx, d_bwt, sizes, origins, locate_step=None):
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

    @classmethod
    def from_text(cls, ctx, data, locate_step=None):
        import torch
        t = as_u8(data)
        d_in = torch.from_numpy(t.copy()).to("cuda:%d" % ctx.device)
        d_bwt = torch.empty_like(d_in)
        origin = ctx.dev_bwt_forward(d_in, len(t), d_bwt)
        return cls(ctx, d_bwt, [len(t)], [origin], locate_step)

    @classmethod
    def from_bwt(cls, ctx, bwt, origin, locate_step=None):
        import torch
        if not hasattr(bwt, "data_ptr"):
            bwt = torch.from_numpy(as_u8(bwt).copy()).to("cuda:%d" % ctx.device)
        return cls(ctx, bwt, [bwt.numel()], [origin], locate_step)

    @classmethod
    def from_bwt_packed(cls, ctx, d_bwt, sizes, origins, locate_step=None):
        return cls(ctx, d_bwt, sizes, origins, locate_step)

    def resident_bytes(self):
        """device bytes the index needs to answer: L and the index, and the locate structure where it was built"""
        return self.total + self.d_index.numel() * 4 + (self.d_loc.numel() * 4 if self.d_loc is not None else 0)

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
        d_lo, d_hi = self._count_dev(patterns, blocks)
        d_pos = torch.empty(npat * max(int(max_hits), 1), dtype=torch.int32, device=self.d_bwt.device)
        if len(self.sizes) == 1 and blocks is None:
            self._ctx.dev_fm_locate(self.d_bwt, self.total, self.d_index, self.d_loc, self.locate_step, d_lo, d_hi, npat, max_hits, d_pos)
        else:
            self._ctx.dev_fm_locate_packed(self.d_bwt, self.sizes, self.d_index, self.d_loc, self.locate_step, d_lo, d_hi, blocks, max_hits, d_pos)
        pos = d_pos.cpu().numpy().view(np.uint32).reshape(npat, -1)
        return [row[row != _lib.FM_NO_HIT] for row in pos]

    def occurrences(self, patterns, blocks=None):
        lo, hi = self.count(patterns, blocks)
        return (hi - lo).astype(np.uint32)


__all__ = ["Index", "Context", "fm_index_bytes", "fm_locate_bytes"]
