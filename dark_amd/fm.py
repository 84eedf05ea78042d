"""FM-index over the library's BWT: count the occurrences of patterns without the text and without a suffix array.
The reference has no counterpart.  L and the index stay on the GPU, about two bytes per text byte."""
import numpy as np

from .context import Context, DarkError, _pack_patterns, as_u8, fm_index_bytes
from . import _lib


class Index:
    """The index of one block, or of a pack of blocks (`sizes` their lengths, `origins` their origins).

    Index.from_text(ctx, data)          forward BWT on the GPU (a full context), then the index; the text is not kept
    Index.from_bwt(ctx, bwt, origin)    from (L, origin) in host memory or in a device tensor -- any context, a decoder context included
    Index.from_bwt_packed(ctx, d_bwt, sizes, origins)
    count(patterns[, blocks]) -> (lo, hi) uint32 arrays: the numbers Context.sa_search gives; occurrences(patterns[, blocks]) = hi - lo."""

    def __init__(self, ctx, d_bwt, sizes, origins):
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

    @classmethod
    def from_text(cls, ctx, data):
        import torch
        t = as_u8(data)
        d_in = torch.from_numpy(t.copy()).to("cuda:%d" % ctx.device)
        d_bwt = torch.empty_like(d_in)
        origin = ctx.dev_bwt_forward(d_in, len(t), d_bwt)
        return cls(ctx, d_bwt, [len(t)], [origin])

    @classmethod
    def from_bwt(cls, ctx, bwt, origin):
        import torch
        if not hasattr(bwt, "data_ptr"):
            bwt = torch.from_numpy(as_u8(bwt).copy()).to("cuda:%d" % ctx.device)
        return cls(ctx, bwt, [bwt.numel()], [origin])

    @classmethod
    def from_bwt_packed(cls, ctx, d_bwt, sizes, origins):
        return cls(ctx, d_bwt, sizes, origins)

    def resident_bytes(self):
        """device bytes the index needs to answer: L and the index"""
        return self.total + self.d_index.numel() * 4

    def count(self, patterns, blocks=None):
        import torch
        pat, lens, npat = _pack_patterns(patterns)
        if npat == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
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
        return d_lo.cpu().numpy().view(np.uint32), d_hi.cpu().numpy().view(np.uint32)

    def occurrences(self, patterns, blocks=None):
        lo, hi = self.count(patterns, blocks)
        return (hi - lo).astype(np.uint32)


__all__ = ["Index", "Context", "fm_index_bytes"]
