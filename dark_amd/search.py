"""Search a .dark archive without inverting a block: every record is decoded only as far as (L, origin) by the host entropy
stage, a segment of records at a time is uploaded and indexed (dark_amd.fm.Index), and every pattern is looked for in every block of the segment by
one device call (Index.find / Index.grep).  Only one segment is resident at a time.

A block is searched on its own, as it was compressed on its own, so by default a match that straddles two blocks is NOT found.
across=True closes that gap: every pattern is also compared at every border of the segment (Index.seams), with the
last bytes of the text so far carried from segment to segment on the host, and those matches come back beside the others.

    plan(sizes)                 the segments _decode_records_packed (cli.py) would make of records of these sizes; needs no GPU
    search_archive(path, ...)   a generator over the segments: (hits, occ, records) per segment, with across=True (hits, occ, records, seams)
"""
import os
import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from ._lib import FM_NEAR_MAX_K, FM_SEAM_MAX_PATTERN
from .cli import (ANY_BYTE_SUFFIX, DUMP_MODELS, PACK_BYTES, PACKED_MAX_BLOCK_BYTES, PACKED_MAX_BLOCKS, RAW_CODING_MODELS, _host_threads, _split_n,
                  read_footer)

DEFAULT_MAX_HITS = 65536  # records per segment (1 MiB of them).  A choice, not a measurement.


def plan(sizes, pack_bytes=None):
    """-> a list of (kind, records, bytes): records of at most PACKED_MAX_BLOCK_BYTES go, in order, into packs ("pack") of at most PACK_BYTES and
    PACKED_MAX_BLOCKS records; every larger record is a segment ("big") of its own.  pack_bytes (default PACK_BYTES): another limit for the
    packs, for small memories and for tests; a record above it still gets a pack of its own."""
    pack_bytes = PACK_BYTES if pack_bytes is None else int(pack_bytes)
    segments = []
    for k, n in enumerate(sizes):
        n = int(n)
        if n > PACKED_MAX_BLOCK_BYTES:
            segments.append(["big", [k], n])
            continue
        last = segments[-1] if segments else None
        if last and last[0] == "pack" and last[2] + n <= pack_bytes and len(last[1]) < PACKED_MAX_BLOCKS:
            last[1].append(k)
            last[2] += n
        else:
            segments.append(["pack", [k], n])
    return [(kind, ks, nb) for kind, ks, nb in segments]


def _records(path, model):
    """-> (offsets of the records in the file, the offset where they end); a file without footer is walked by the bytes every record's decode
    consumes, as decode_file does"""
    from .model import raw_stream_decode, stream_decode
    footer = read_footer(path) if model not in RAW_CODING_MODELS else None
    if footer is not None:
        return footer
    size = os.path.getsize(path)
    blob = np.fromfile(path, dtype=np.uint8)
    offsets, pos = [], 0
    while pos < size:
        if pos + 4 > size:
            raise SystemExit("truncated record header at byte %d" % pos)
        (word,) = struct.unpack("<I", blob[pos:pos + 4].tobytes())
        offsets.append(pos)
        if model in RAW_CODING_MODELS:
            used = raw_stream_decode(blob[pos + 4:], word)[2]
        else:
            n, flagged = _split_n(word)
            used = stream_decode(model + ANY_BYTE_SUFFIX if flagged else model, blob[pos + 4:], n, with_consumed=True)[3]
        pos += 4 + used
    return offsets, size


def _decode_to_bwt(model, word, stream):
    """one record as far as (L, origin).  A one-symbol record's stream carries no usable origin (the decoders do not read it and
    copy L = c^n out, or invert it with origin n - 1): L = c^n, and origin n - 1 is what the conventions of section 4.4 give for c^n -- a suffix
    that is a proper prefix of another sorts first, so the suffixes of c^n stand in order of ascending length and suffix 0 takes the last slot."""
    from .model import raw_stream_decode, stream_decode
    if model in RAW_CODING_MODELS:
        bwt, origin, _ = raw_stream_decode(stream, word)
        return bwt, origin
    n, flagged = _split_n(word)
    bwt, origin, single = stream_decode(model + ANY_BYTE_SUFFIX if flagged else model, stream, n)
    return bwt, (n - 1 if single else origin)


def search_archive(path, model, patterns, device=0, before=0, after=0, max_hits=DEFAULT_MAX_HITS, host_threads=0, locate_step=32, extract_step=32,
                   count_only=False, stats=None, across=False, pack_bytes=None, mismatches=0, ignore_case=False):
    """A generator over the archive's segments.  Per segment it yields (hits, occ, records):
        hits     a list of (record, offset in the original file of the record's first byte, pattern, position in the record, bytes) for the first
                 max_hits hits of the segment in the order (pattern, record, suffix-array slot); bytes is the text from `before` bytes in front of
                 the hit to `after` bytes behind it, cut at the record's ends (before == after == 0: the pattern itself, and no extract structure)
        occ      a uint32 array len(patterns) x records of the segment: occurrences of every pattern in every record, however many hits were listed
        records  the segment's record numbers
    count_only: no hits are listed and no locate or extract structure is built.  stats (a dict, optional) receives resident_bytes of the largest
    segment.  Nothing is inverted; a match that straddles two records is not found unless across=True.
    across=True: 4-tuples (hits, occ, records, seams) with seams = (seam_hits, seam_occ) -- the matches whose first and last byte lie in different
    records; hits and occ are what across=False gives.
        seam_occ   a uint32 array len(patterns) x records of the segment: column j = the matches whose last crossed border is the one in front of
                   records[j] (zero for the archive's first record), however many were listed
        seam_hits  a list of (record holding the first byte, that record's offset in the original file, pattern, position in that record, bytes)
                   for the first max_hits of the segment in the order (pattern, record of the last byte, position); bytes runs from `before`
                   bytes in front of the match to `after` bytes behind it, cut at the start of the record holding the first byte and at the end
                   of the record holding the last byte
    The extract structure is then built even for count_only.  Patterns longer than DK_FM_SEAM_MAX_PATTERN are left out of the seam query and
    their indices listed in stats["seam_skipped"].  Between segments the last longest - 1 + before bytes of the text so far are kept on the host
    (Index.tail).  pack_bytes: see plan.
    mismatches=K (0 .. DK_FM_NEAR_MAX_K) and ignore_case=True search approximately (Index.near): a hit is a place whose text
    differs from the pattern in at most K bytes, ASCII letters compared without case under ignore_case.  With either option the hit tuples gain
    `cost`, the number of bytes that differ, as a sixth field, and `bytes` starts `before` bytes in front of the MATCHED TEXT -- which is not the
    pattern -- so the extract structure is built unless count_only.  stats["cut_pairs"] receives the (pattern, record) searches that stopped at
    the node limit; their occ is a lower bound.  With both at their defaults the generator runs the exact search and yields its tuples.
    across=True together with either option raises ValueError: near hits across record borders are not built."""
    near = bool(mismatches) or bool(ignore_case)
    if near and across:
        raise ValueError("across=True goes with the exact search only: near hits across block borders are not built")
    if not 0 <= int(mismatches) <= FM_NEAR_MAX_K:
        raise ValueError("mismatches = %r: 0 .. %d" % (mismatches, FM_NEAR_MAX_K))
    import torch
    from . import fm
    from .context import Context
    if model in DUMP_MODELS:
        raise SystemExit("model %s is dump-only: there is nothing to search" % model)
    torch.cuda.set_device(device)
    offsets, end = _records(path, model)
    bounds = list(offsets) + [end]
    with open(path, "rb") as f:
        words = []
        for k in range(len(offsets)):
            f.seek(offsets[k])
            words.append(struct.unpack("<I", f.read(4))[0])
        sizes = [w if model in RAW_CODING_MODELS else _split_n(w)[0] for w in words]
        starts = np.concatenate([[0], np.cumsum(np.array(sizes, dtype=np.int64))])  # where every record's text starts in the original file
        segments = plan(sizes, pack_bytes)
        if not segments:
            return
        served = [q for q, p in enumerate(patterns) if len(p) <= FM_SEAM_MAX_PATTERN] if across else []
        reach = max([len(patterns[q]) for q in served] + [1]) - 1  # W: the most bytes of a match in front of the last border it crosses
        seaming = across and reach > 0
        if across and stats is not None:
            stats["seam_skipped"] = [q for q in range(len(patterns)) if q not in served]
        carry = b""  # across: the last reach + before bytes of the text in front of the segment
        threads = host_threads or max(1, _host_threads() - 1)
        cap = max(nb for _, _, nb in segments)
        most = max(len(ks) for _, ks, _ in segments)
        want_text = not count_only and (before or after or near)
        if near and stats is not None:
            stats["cut_pairs"] = 0
        with Context(cap, device, purpose="decoder", max_blocks=min(most, PACKED_MAX_BLOCKS)) as ctx, ThreadPoolExecutor(threads) as pool:
            for kind, ks, nbytes in segments:
                streams = []
                for k in ks:
                    f.seek(offsets[k] + 4)
                    streams.append(np.fromfile(f, dtype=np.uint8, count=bounds[k + 1] - offsets[k] - 4))
                # (ctypes releases the GIL inside the entropy stage)
                decoded = list(pool.map(lambda a: _decode_to_bwt(model, *a), [(words[k], s) for k, s in zip(ks, streams)]))
                del streams
                ns = [sizes[k] for k in ks]
                d_bwt = torch.from_numpy(np.concatenate([b for b, _ in decoded])).to("cuda:%d" % device)
                origins = [o for _, o in decoded]
                del decoded
                lstep = None if count_only else locate_step
                estep = extract_step if want_text or seaming else None
                if kind == "pack" and len(ks) > 1:
                    index = fm.Index.from_bwt_packed(ctx, d_bwt, ns, origins, locate_step=lstep, extract_step=estep)
                else:
                    index = fm.Index.from_bwt(ctx, d_bwt, origins[0], locate_step=lstep, extract_step=estep)
                if stats is not None:
                    stats["resident_bytes"] = max(stats.get("resident_bytes", 0), index.resident_bytes())
                if near:
                    occ, recs, _, cut = index.near(patterns, int(mismatches), ignore_case, max_hits=0 if count_only else max_hits)
                    if stats is not None:
                        stats["cut_pairs"] += cut
                    found = index.near_windows(recs, [len(p) for p in patterns], before, after)
                    yield [(ks[b], int(starts[ks[b]]), q, p, text, cost) for q, b, p, cost, text in found], occ, list(ks)
                    del index, d_bwt
                    continue
                if count_only:
                    occ, _, _ = index.find(patterns, 0)
                    found = []
                elif want_text:
                    occ, _, _ = index.find(patterns, 0)
                    found = index.grep(patterns, before, after, max_hits)
                else:
                    occ, recs, _ = index.find(patterns, max_hits)
                    recs = recs[recs["position"] != 0xFFFFFFFF]
                    found = [(int(r["pattern"]), int(r["block"]), int(r["position"]), bytes(patterns[int(r["pattern"])])) for r in recs]
                hits = [(ks[b], int(starts[ks[b]]), q, p, text) for q, b, p, text in found]
                if not across:
                    yield hits, occ, list(ks)
                    del index, d_bwt
                    continue
                seam_occ = np.zeros((len(patterns), len(ks)), dtype=np.uint32)
                seam_hits = []
                if seaming:
                    part, recs, _ = index.seams([patterns[q] for q in served], carry, 0 if count_only else max_hits)
                    seam_occ[served] = part
                    seam_hits = _seam_windows(index, recs, [len(patterns[q]) for q in served], served, ks, starts, carry, reach, before, after)
                    carry = (carry + index.tail(reach + before))[-(reach + before):]
                yield hits, occ, list(ks), (seam_hits, seam_occ)
                del index, d_bwt


def _seam_windows(index, recs, lens, served, ks, starts, carry, reach, before, after):
    """the seam records of one segment as search_archive's seam_hits.  Per border with a listed hit, one window of text: the last reach + before
    bytes in front of the block (Index.edges; `carry` where the segment does not reach that far back) and the block's first reach + after."""
    if len(recs) == 0:
        return []
    borders = sorted(set(recs["block"].tolist()))
    edges = dict(zip(borders, index.edges(borders, reach + before, reach + after)))
    out = []
    for r in recs:
        b, back, m = int(r["block"]), int(r["back"]), lens[int(r["pattern"])]
        front, head = edges[b]
        front = (carry + front)[-(reach + before):] if len(front) < reach + before else front
        window, first = front + head, int(starts[ks[b]])  # window[len(front)] is the block's first byte, byte `first` of the file
        at = first - back
        rec = int(np.searchsorted(starts, at, side="right")) - 1  # the record holding the match's first byte
        lo, hi = max(at - before, int(starts[rec])), min(at + m + after, int(starts[ks[b] + 1]))
        out.append((rec, int(starts[rec]), served[int(r["pattern"])], at - int(starts[rec]), window[lo - first + len(front):hi - first + len(front)]))
    return out


__all__ = ["plan", "search_archive", "DEFAULT_MAX_HITS"]
