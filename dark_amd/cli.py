"""Command line front end with the reference's conventions (src/main.rs:34-116).

    python -m dark_amd.cli [-m dark|exp|ybs|simple|bbb|raw|rawdc] FILE       -> ./FILE with its extension replaced by .dark
    python -m dark_amd.cli [-m MODEL] FILE.dark                           -> ./FILE.orig

The default model is `exp`, as in src/main.rs:52.  Output names follow PathBuf::set_extension (src/main.rs:64-66,96-98):
book.txt -> book.dark, book -> book.dark, book.dark -> book.orig; the output lands in the current directory.  A file made here with
one block is byte-for-byte what the reference writes: [u32 LE n][coded stream] (to the extent DESIGN.md section 2 pins it).

Extensions beyond the reference (whole file = one block, read into memory, one thread):
  -b BYTES   cut the input into blocks; records [u32 LE n][stream] are concatenated, each byte-identical to a single-block run on that
             block, followed by an index footer (record offsets) so that decoding can be batched and spread over GPUs.  The reference
             reads such a file as its first block only.  Blocks are STREAMED: one block of input is in host memory at a time; each goes
             through dk_batch_push as soon as it is in HBM (file reading, upload, GPU stages and the host coding of earlier blocks overlap).
  --packed   with -b of at most 16 MiB on one GPU: consecutive blocks go to the GPU as packs of up to 64 MiB, each through ONE segmented
             device pass (dk_batch_push_packed); every block is still coded on its own, and the archive is byte-identical.  On decode
             (one GPU, indexed archives): records of at most 16 MiB are decoded in packs of up to 64 MiB, one upload and one segmented
             inverse BWT per pack (dk_dev_packed_decode); larger records take the batched path; the output is byte-identical.
  --gpus G   block b -> GPU b mod G, one worker process per GPU; the parent never touches a GPU and stitches the records in order.
  --force    encode blocks that contain byte 0xFF.  The reference's header cannot carry that symbol (src/block/dc.rs:57,60,73,127):
             it writes such an archive without complaint and can never decode it.  This front end refuses unless --force is given.
  --any-byte encode ANY file so that it decodes (DK_MODEL_ANYBYTE; not together with --force).  A block without byte 0xFF is
             written as the plain record [u32 n][stream], so a file without 0xFF gives the same archive with and without the option.  A
             block with 0xFF is written as [u32 n | 0x80000000][u32 first position of 0xFF in the BWT][stream]: the stream is still the
             reference's, the four bytes in front are what its header leaves out.  Decoding needs no option: bit 31 of a record's n says
             which kind it is.  The reference cannot read a record with bit 31 set.
  --grep TEXT / --grep-hex HEX (repeatable) FILE.dark
             search the archive instead of decoding it (dark_amd/search.py): the records are decoded as far as their BWT, a
             pack at a time is indexed on the GPU and every pattern is looked for in every block; no block is inverted, no file is written.
             One line per hit in file order, absolute_offset:pattern_index:enclosing line (--context-bytes, default 80, on either side, cut
             at the nearest newlines); --count-only: pattern_index:count per pattern; --max-hits bounds the hits listed per pack.  Exit status
             0 with hits, 1 without.  A match that straddles two blocks is NOT found, unless --across-blocks is given.
  --across-blocks (with --grep / --grep-hex)
             also find the matches that straddle block borders: every pattern is compared at every border of a pack on the
             GPU, with the last bytes of the text so far carried from pack to pack.  They are listed among the others in file order, in the
             same format; their line is cut at the start of the block holding the match's first byte and at the end of the block holding its
             last one.  --count-only adds them to the counts.  Patterns above 4096 bytes are searched inside the blocks only (a note says so).
  --mismatches K (0..3) / -i, --ignore-case (with --grep / --grep-hex, not with --across-blocks)
             approximate search: the places that differ from a pattern in at most K bytes, without insertions or deletions;
             -i: ASCII letters of every pattern, hexadecimal ones included, match either case.  Patterns hold at most 128 bytes.  With K > 0
             the lines are absolute_offset:pattern_index:cost:enclosing line; --count-only counts these hits.  A search is bounded: a note
             says how many (pattern, block) searches stopped at the node limit, whose counts are lower bounds.
"""
import argparse
import os
import time
import struct
import subprocess
import sys
import threading
import queue

import numpy as np

EXTENSION = "dark"
STATS = {}  # --stats: when the library and its context were ready (imports, workspace allocation done)
FOOTER_MAGIC = b"DKIX"
DUMP_MODELS = ("raw", "rawdc")
RAW_CODING_MODELS = ("bbb",)  # block::raw with a coding RawModel (src/main.rs:73,104): block after block through dk_raw_block_encode
ANY_BYTE_BIT = 0x80000000  # in a record's n: the stream starts with the any-byte prefix (n itself is at most 2^31 - 2, so the bit is free)
ANY_BYTE_SUFFIX = "+ff"    # _lib.MODEL_IDS: the model with DK_MODEL_ANYBYTE


def _record_head(n, stream, any_byte):
    """-> (the record's first four bytes, the rest of the record) for a block of n bytes coded as `stream`.  Under --any-byte the stream
    starts with the prefix the library wrote: prefix == n means "no 0xFF in this block", and the record is the plain one."""
    if not any_byte:
        return struct.pack("<I", n), memoryview(stream)
    (first_ff,) = struct.unpack("<I", bytes(stream[:4]))
    if first_ff == n:
        return struct.pack("<I", n), memoryview(stream)[4:]
    return struct.pack("<I", n | ANY_BYTE_BIT), memoryview(stream)


def _split_n(word):
    """a record's first word -> (n, the stream carries the any-byte prefix)"""
    return word & (ANY_BYTE_BIT - 1), bool(word & ANY_BYTE_BIT)


def _uniform_streams(model, ns, flagged, streams):
    """A batch or pack takes ONE model id.  With at least one flagged record in it, plain records get the prefix "absent" (= n) put in
    front -- a copy of compressed bytes only -- and the call runs with the flag; without any, everything is as it always was."""
    if not any(flagged):
        return model, streams
    return model + ANY_BYTE_SUFFIX, [s if fl else np.concatenate([np.frombuffer(struct.pack("<I", n), dtype=np.uint8), s])
                                     for n, fl, s in zip(ns, flagged, streams)]


def set_extension(name, ext):
    """std::path::PathBuf::set_extension on a bare file name: the part after the last '.' is replaced (a leading '.' alone does not start
    an extension); a name without extension gets one appended."""
    i = name.rfind(".")
    stem = name[:i] if i > 0 else name
    return stem + "." + ext


def output_name(path, ext):
    return set_extension(os.path.basename(path), ext)  # main.rs:96-98 / 64-66: file name only -> current directory


def has_extension(path, ext):
    name = os.path.basename(path)
    i = name.rfind(".")
    return i > 0 and name[i + 1:] == ext


class Refused(SystemExit):
    pass


class _AtomicOutput:
    """The archive is written to a temporary file next to its final name and renamed over it only when it is complete (records and
    footer written, file closed): a refusal, a GPU error or a failed worker leaves an existing archive of that name untouched and never
    leaves a truncated one behind -- a footer-less prefix of records would otherwise decode as a valid, shorter file.  Decoding writes the
    restored file the same way: a record that does not decode (DK_E_STREAM) leaves no output file, partial or otherwise."""

    def __init__(self, out_path):
        self.final = out_path
        self.tmp = os.path.join(os.path.dirname(out_path) or ".", ".%s.tmp%d" % (os.path.basename(out_path), os.getpid()))
        self.f = None

    def __enter__(self):
        self.f = open(self.tmp, "wb")
        return self.f

    def __exit__(self, exc_type, exc, tb):
        self.f.close()
        if exc_type is None:
            os.replace(self.tmp, self.final)
        else:
            try:
                os.remove(self.tmp)
            except OSError:
                pass
        return False


_NOTED = set()


def _note(key, text):
    """one line on stderr, once per run"""
    if key not in _NOTED:
        _NOTED.add(key)
        print("dark_amd: " + text, file=sys.stderr)


def _note_workspace(ctx):
    """--stats on decode: the largest device workspace a context of this run took"""
    STATS["ws_size_bytes"] = max(STATS.get("ws_size_bytes", 0), int(ctx.stats()["ws_size_bytes"]))


def _note_model(model):
    if model in RAW_CODING_MODELS:
        _note("bbb", "-m bbb is EXPERIMENTAL here: the model's gates restate compress::entropy::ari::apm from an in-repo analogue (parity "
                     "unpinned, DESIGN.md section 7); archives decode with this program, compatibility with the Rust crate's bytes is not claimed")


def _note_single_symbol(block, where):
    if len(block) and int(block.min()) == int(block.max()):
        _note("single", "%s holds one distinct byte value: this program decodes it, the reference's decoder mis-reads `origin` for such a "
                        "block and returns one byte (DESIGN.md, reference quirks)" % where)


def _check_ff(block, force, where):
    if not force and bool((block == 255).any()):
        raise Refused("%s contains byte 0xFF: the reference format cannot carry that symbol (src/block/dc.rs:57-73), the archive could "
                      "never be decoded.  Pass --force to write it anyway (bit-exact with what the reference writes)." % where)


# ---- single block: the reference's own behaviour ------------------------------------------------------------------------------------
def _encode_single(path, model, device, force, out_path, any_byte=False):
    from .context import Context
    data = np.fromfile(path, dtype=np.uint8)  # main.rs:87-95 reads the whole file: one block
    n = len(data)
    if n == 0:
        raise SystemExit("empty input: the reference panics on it (src/saca.rs:107)")
    if model not in DUMP_MODELS and model not in RAW_CODING_MODELS:
        _check_ff(data, force, "the block")               # before the output is touched
    _note_single_symbol(data, "the input")
    with Context(n, device) as ctx, _AtomicOutput(out_path) as out:
        if any_byte:
            head, body = _record_head(n, ctx.block_encode(model + ANY_BYTE_SUFFIX, data), True)
            out.write(head)
            out.write(body)
        else:
            out.write(struct.pack("<I", n))               # main.rs:102
            _write_block(ctx, model, data, out, True, force)
    return out_path


def _write_block(ctx, model, block, out, first, force):
    if model == "raw":
        # block::raw::Encoder with model::raw::Out (src/block/raw.rs:35-59, src/model/raw.rs:46-76): origin as four symbols, then every
        # BWT byte, go to ./out.raw; nothing reaches the coder, whose tail is four zero bytes
        with open("out.raw", "wb" if first else "ab") as dump:
            dump.write(ctx.raw_block_encode_dump(block))
        out.write(b"\0\0\0\0")
    elif model == "rawdc":
        # block::dc::Encoder with model::raw::DcOut (src/model/raw.rs:12-44): 10-byte records go to ./out-dc.raw
        with open("out-dc.raw", "wb" if first else "ab") as dump:
            dump.write(ctx.block_encode("rawdc", block))
        out.write(b"\0\0\0\0")
    elif model in RAW_CODING_MODELS:
        # block::raw::Encoder with model::bbb::Model (src/main.rs:104): every byte value can be carried, no 0xFF restriction
        out.write(ctx.raw_block_encode(block, 1))
    else:
        _check_ff(block, force, "the block")
        out.write(ctx.block_encode(model, block))         # main.rs:104-113


# ---- streamed, pipelined encode on one GPU ---------------------------------------------------------------------------------------------
def _reader(f, block_size, first_block, step, total_blocks, q, force, device):
    """reads blocks first_block, first_block+step, ... one at a time and uploads each to HBM; at most two are waiting to be pushed"""
    import torch
    try:
        for b in range(first_block, total_blocks, step):
            f.seek(b * block_size)
            block = np.fromfile(f, dtype=np.uint8, count=block_size)  # ONE block of input in host memory
            _check_ff(block, force, "block %d" % b)
            _note_single_symbol(block, "block %d" % b)
            q.put((b, len(block), torch.from_numpy(block).to("cuda:%d" % device)))
            del block
        q.put(None)
    except BaseException as e:  # noqa: BLE001 -- handed to the consumer, which re-raises
        q.put(e)


def _encode_blocks(path, model, block_size, device, first_block, step, total_blocks, out, index, force, host_threads, any_byte=False):
    """encode blocks first_block, first_block+step, ... of `path` in order into `out`; index gets (block number, record length).
    Every block goes through dk_batch_push as soon as it is in HBM: its device stages run at once, its coding on one of the host threads;
    file reading, upload, GPU stages and coding all overlap.  Records are written out every `flush_every` blocks."""
    import torch
    from .context import Context
    torch.cuda.set_device(device)
    flush_every = int(max(2 * host_threads, min(256, (1 << 32) // max(1, block_size))))  # at most about 4 GB of input between flushes
    q = queue.Queue(maxsize=2)
    with open(path, "rb") as f, Context(block_size, device) as ctx:
        STATS["t_ready"] = time.perf_counter()
        t = threading.Thread(target=_reader, args=(f, block_size, first_block, step, total_blocks, q, force, device), daemon=True)
        t.start()
        batch, pending = None, []

        def flush():
            nonlocal batch, pending
            if batch is None:
                return
            streams = batch.finish()
            for (b, n), s in zip(pending, streams):
                head, body = _record_head(n, s, any_byte)
                out.write(head)
                out.write(body)
                index.append((b, 4 + len(body)))
            batch, pending = None, []

        try:
            while True:
                item = q.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                b, n, d = item
                if batch is None:
                    batch = ctx.batch_begin(model + ANY_BYTE_SUFFIX if any_byte else model, host_threads)
                batch.push(d, n)  # a failed push closes the batch (joins the coders of the blocks before it) and raises
                pending.append((b, n))
                del d, item
                if len(pending) >= flush_every:
                    flush()
            flush()
        finally:
            if batch is not None:
                batch.close()  # error path: the coding threads are joined before their output buffers and the context go away
        t.join()


PACK_BYTES = 64 << 20
PACKED_MAX_BLOCKS = 65536  # DK_PACKED_MAX_BLOCKS
PACKED_MAX_BLOCK_BYTES = 1 << 24  # DK_PACKED_MAX_BLOCK_BYTES  # --packed: consecutive blocks grouped into packs of at most this many bytes


def _encode_blocks_packed(path, model, block_size, device, total_blocks, out, index, force, host_threads, any_byte=False):
    """--packed: consecutive blocks go to the GPU as one pack (dk_batch_push_packed: one segmented device pass per pack, every block still
    coded as its own job); the records are byte-identical to _encode_blocks'."""
    import torch
    from .context import Context
    torch.cuda.set_device(device)
    per_pack = max(1, PACK_BYTES // block_size)
    with open(path, "rb") as f, Context(per_pack * block_size, device) as ctx:
        STATS["t_ready"] = time.perf_counter()
        flush_every = int(max(2 * host_threads, min(256, (1 << 32) // max(1, block_size))))
        batch, pending = None, []

        def flush():
            nonlocal batch, pending
            if batch is None:
                return
            streams = batch.finish()
            for (b, n), s in zip(pending, streams):
                head, body = _record_head(n, s, any_byte)
                out.write(head)
                out.write(body)
                index.append((b, 4 + len(body)))
            batch, pending = None, []

        try:
            for b0 in range(0, total_blocks, per_pack):
                data = np.fromfile(f, dtype=np.uint8, count=per_pack * block_size)
                sizes = [min(block_size, len(data) - k) for k in range(0, len(data), block_size)]
                for j, k in enumerate(range(0, len(data), block_size)):
                    _check_ff(data[k:k + block_size], force, "block %d" % (b0 + j))
                    _note_single_symbol(data[k:k + block_size], "block %d" % (b0 + j))
                d = torch.from_numpy(data).to("cuda:%d" % device)
                if batch is None:
                    batch = ctx.batch_begin(model + ANY_BYTE_SUFFIX if any_byte else model, host_threads)
                batch.push_packed(d, sizes)
                pending.extend((b0 + j, n) for j, n in enumerate(sizes))
                del d, data
                if len(pending) >= flush_every:
                    flush()
            flush()
        finally:
            if batch is not None:
                batch.close()


def _write_footer(out, offsets):
    """index of a multi-record file: 'DKIX' u32 count, count x u64 record offsets, u64 offset of this footer, 'DKIX'"""
    start = out.tell()
    out.write(FOOTER_MAGIC + struct.pack("<I", len(offsets)))
    out.write(struct.pack("<%dQ" % len(offsets), *offsets))
    out.write(struct.pack("<Q", start) + FOOTER_MAGIC)


def read_footer(path):
    """-> list of record offsets + the offset where the records end, or None for a file without index (single block / legacy)"""
    size = os.path.getsize(path)
    if size < 24:
        return None
    with open(path, "rb") as f:
        f.seek(size - 12)
        tail = f.read(12)
        if tail[8:] != FOOTER_MAGIC:
            return None
        (start,) = struct.unpack("<Q", tail[:8])
        if start + 20 > size:
            return None
        f.seek(start)
        head = f.read(8)
        if head[:4] != FOOTER_MAGIC:
            return None
        (count,) = struct.unpack("<I", head[4:])
        if start + 8 + 8 * count + 12 != size:
            return None
        offs = list(struct.unpack("<%dQ" % count, f.read(8 * count)))
    return offs, start


def _host_threads():
    try:
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()
        cpus = max(1, int(q) // int(period)) if q != "max" else (os.cpu_count() or 1)
    except (OSError, ValueError):
        cpus = os.cpu_count() or 1
    return cpus


def _devices(device, gpus, devices):
    """GPU of worker r: --devices a,b,... (e.g. 0,0 rehearses two workers on a one-GPU box), else device + r"""
    if devices:
        ids = [int(x) for x in str(devices).split(",")]
        if len(ids) != gpus:
            raise SystemExit("--devices needs exactly --gpus entries")
        return ids
    return [device + r for r in range(gpus)]


def encode_file(path, model, block_size=0, device=0, gpus=1, force=False, host_threads=0, devices=None, packed=False, any_byte=False):
    out_path = output_name(path, EXTENSION)
    if any_byte:  # before any output is touched
        if force:
            raise SystemExit("--any-byte and --force exclude each other: one writes blocks with byte 0xFF so that they decode, the other so that they are lost")
        if model in DUMP_MODELS:
            raise SystemExit("--any-byte: model %s writes no stream the option could extend" % model)
        if model in RAW_CODING_MODELS:
            any_byte = False  # block::raw carries every byte value already
        else:
            force = True      # no host scan for 0xFF: whether a block holds one comes back from the library, in the prefix
    total = os.path.getsize(path)
    if total == 0:
        raise SystemExit("empty input: the reference panics on it (src/saca.rs:107)")
    _note_model(model)
    if not block_size or block_size >= total:
        return _encode_single(path, model, device, force, out_path, any_byte)
    nblocks = -(-total // block_size)
    if model in DUMP_MODELS or model in RAW_CODING_MODELS:  # block after block through the host entry points
        from .context import Context
        with open(path, "rb") as f, Context(block_size, device) as ctx, _AtomicOutput(out_path) as out:
            for b in range(nblocks):
                block = np.fromfile(f, dtype=np.uint8, count=block_size)
                _note_single_symbol(block, "block %d" % b)
                out.write(struct.pack("<I", len(block)))
                _write_block(ctx, model, block, out, b == 0, force)
        return out_path
    threads = host_threads or max(1, _host_threads() // max(1, gpus) - 1)
    if packed and (gpus > 1 or block_size > PACKED_MAX_BLOCK_BYTES):
        raise SystemExit("--packed: one GPU and -b at most %d" % PACKED_MAX_BLOCK_BYTES)
    if gpus <= 1:
        index = []
        with _AtomicOutput(out_path) as out:
            if packed:
                _encode_blocks_packed(path, model, block_size, device, nblocks, out, index, force, threads, any_byte)
            else:
                _encode_blocks(path, model, block_size, device, 0, 1, nblocks, out, index, force, threads, any_byte)
            offsets, pos = [], 0
            for _, ln in index:
                offsets.append(pos)
                pos += ln
            _write_footer(out, offsets)
        return out_path
    # one worker process per GPU (block b -> GPU b mod G); this parent has not touched and does not touch a GPU
    parts = ["%s.part%d" % (out_path, r) for r in range(gpus)]
    procs = []
    devs = _devices(device, gpus, devices)
    for r in range(gpus):
        cmd = [sys.executable, "-m", "dark_amd.cli", "--worker", "%d/%d" % (r, gpus), "--part", parts[r], "-m", model, "-b", str(block_size),
               "-d", str(devs[r]), "--host-threads", str(threads)] + (["--any-byte"] if any_byte else ["--force"] if force else []) + [path]
        procs.append(subprocess.Popen(cmd, env=dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.dirname(os.path.abspath(__file__)))] +
                                                                                               os.environ.get("PYTHONPATH", "").split(os.pathsep)))))
    rc = 0
    for p in procs:
        p.wait()
        rc = rc or p.returncode
    if rc:
        for part in parts:
            for name in (part, part + ".idx"):
                if os.path.exists(name):
                    os.remove(name)
        raise SystemExit("a GPU worker failed (exit code %d)" % rc)
    # stitch: records in block order, each worker's part holds its blocks in its own order
    lens = [[int(x) for x in open(part + ".idx").read().split()] for part in parts]
    files = [open(part, "rb") for part in parts]
    offsets, pos = [], 0
    with _AtomicOutput(out_path) as out:
        for b in range(nblocks):
            r, k = b % gpus, b // gpus
            ln = lens[r][k]
            offsets.append(pos)
            out.write(files[r].read(ln))
            pos += ln
        _write_footer(out, offsets)
    for fobj, part in zip(files, parts):
        fobj.close()
        os.remove(part)
        os.remove(part + ".idx")
    return out_path


def _worker_encode(args):
    r, g = (int(x) for x in args.worker.split("/"))
    total = os.path.getsize(args.file)
    nblocks = -(-total // args.block_size)
    index = []
    with open(args.part, "wb") as out:
        _encode_blocks(args.file, args.model, args.block_size, args.device, r, g, nblocks, out, index, args.force or args.any_byte,
                       args.host_threads or 1, args.any_byte)
    with open(args.part + ".idx", "w") as f:
        f.write(" ".join(str(ln) for _, ln in index))


# ---- decode -----------------------------------------------------------------------------------------------------------------------------
def _decode_records_batched(path, model, device, offsets, end, which, out_write, host_threads):
    """decode records `which` (indices into offsets) through dk_dev_batch_decode, in batches; out_write(k, bytes) receives them in order"""
    import torch
    from .context import Context
    torch.cuda.set_device(device)
    bounds = offsets + [end]
    with open(path, "rb") as f:
        sizes, flagged = [], []
        for k in which:
            f.seek(offsets[k])
            n, fl = _split_n(struct.unpack("<I", f.read(4))[0])
            sizes.append(n)
            flagged.append(fl)
        if not sizes:
            return
        batch = int(max(2, min(4 * host_threads, (1 << 30) // max(sizes))))  # two batches of outputs live in HBM at a time
        with Context(max(sizes), device, purpose="decoder") as ctx:
            STATS["t_ready"] = time.perf_counter()
            _note_workspace(ctx)
            # a writer thread downloads and writes the blocks of one batch while the next batch is being decoded
            wq = queue.Queue(maxsize=1)
            werr = []

            def writer():
                while True:
                    item = wq.get()
                    if item is None:
                        return
                    try:
                        if not werr:
                            for k, d in zip(*item):
                                out_write(k, d.cpu().numpy().tobytes())
                    except BaseException as e:  # noqa: BLE001 -- re-raised by the main thread
                        werr.append(e)

            wt = threading.Thread(target=writer, daemon=True)
            wt.start()
            try:
                for lo in range(0, len(which), batch):
                    ks = which[lo:lo + batch]
                    ns = sizes[lo:lo + batch]
                    streams = []
                    for k in ks:
                        f.seek(offsets[k] + 4)
                        streams.append(np.fromfile(f, dtype=np.uint8, count=bounds[k + 1] - offsets[k] - 4))
                    d_outs = [torch.empty(n, dtype=torch.uint8, device="cuda:%d" % device) for n in ns]
                    call_model, streams = _uniform_streams(model, ns, flagged[lo:lo + batch], streams)
                    ctx.dev_batch_decode(call_model, streams, ns, d_outs, host_threads)
                    wq.put((ks, d_outs))
                    del d_outs, streams
                    if werr:
                        break
            finally:
                wq.put(None)
                wt.join()
            if werr:
                raise werr[0]


def _decode_records_packed(path, model, device, offsets, end, out_write, host_threads):
    """--packed: runs of consecutive records of at most PACKED_MAX_BLOCK_BYTES go to the GPU as packs of up to PACK_BYTES through
    dk_dev_packed_decode (one upload and one segmented inverse BWT per pack); larger records go through _decode_records_batched, in order"""
    import torch
    from .context import Context
    torch.cuda.set_device(device)
    bounds = offsets + [end]
    with open(path, "rb") as f:
        sizes, flagged = [], []
        for k in range(len(offsets)):
            f.seek(offsets[k])
            n, fl = _split_n(struct.unpack("<I", f.read(4))[0])
            sizes.append(n)
            flagged.append(fl)
        # segments in record order: [kind, records, bytes], "pack" for small records (one pack each), "big" for a run of the others
        segments = []
        for k, n in enumerate(sizes):
            kind = "pack" if n <= PACKED_MAX_BLOCK_BYTES else "big"
            last = segments[-1] if segments else None
            if last and last[0] == kind and (kind == "big" or last[2] + n <= PACK_BYTES):
                last[1].append(k)
                last[2] += n
            else:
                segments.append([kind, [k], n])
        cap = max([nb for kind, _, nb in segments if kind == "pack"] or [0])
        most = max([len(ks) for kind, ks, _ in segments if kind == "pack"] or [0])  # the largest pack planned above decides max_blocks
        ctx = Context(cap, device, purpose="decoder", max_blocks=min(most, PACKED_MAX_BLOCKS)) if cap else None
        STATS["t_ready"] = time.perf_counter()
        if ctx is not None:
            _note_workspace(ctx)
        try:
            for kind, ks, _ in segments:
                if kind == "big":
                    _decode_records_batched(path, model, device, offsets, end, ks, out_write, host_threads)
                    continue
                streams = []
                for k in ks:
                    f.seek(offsets[k] + 4)
                    streams.append(np.fromfile(f, dtype=np.uint8, count=bounds[k + 1] - offsets[k] - 4))
                ns = [sizes[k] for k in ks]
                d_out = torch.empty(sum(ns), dtype=torch.uint8, device="cuda:%d" % device)
                call_model, streams = _uniform_streams(model, ns, [flagged[k] for k in ks], streams)
                ctx.dev_packed_decode(call_model, streams, ns, d_out, host_threads)
                data = d_out.cpu().numpy()
                pos = 0
                for k, n in zip(ks, ns):
                    out_write(k, data[pos:pos + n].tobytes())
                    pos += n
                del d_out, data, streams
        finally:
            if ctx is not None:
                ctx.close()


def decode_file(path, model, device=0, gpus=1, host_threads=0, devices=None, packed=False):
    from .context import Context
    out_path = output_name(path, "orig")                    # main.rs:64-66
    if model in DUMP_MODELS:
        raise SystemExit("model %s is dump-only: there is nothing to decode (src/model/raw.rs:39-43 panics)" % model)
    if packed and gpus > 1:
        raise SystemExit("--packed: one GPU")
    footer = read_footer(path) if model not in RAW_CODING_MODELS else None  # bbb archives carry no index: records are walked
    threads = host_threads or max(1, _host_threads() // max(1, gpus) - 1)
    if footer is None:
        # no index: the reference's single-block file (main.rs:70), or concatenated records walked by the bytes each decode consumed
        size = os.path.getsize(path)
        with open(path, "rb") as f, _AtomicOutput(out_path) as out:
            blob = np.fromfile(f, dtype=np.uint8)
            pos, ctx, records = 0, None, 0
            while pos < size:
                if pos + 4 > size:
                    raise SystemExit("truncated record header at byte %d" % pos)
                (n,) = struct.unpack("<I", blob[pos:pos + 4].tobytes())   # main.rs:70
                any_byte = False
                if model not in RAW_CODING_MODELS:
                    n, any_byte = _split_n(n)
                pos += 4
                if ctx is None or ctx.capacity() < n:
                    if ctx is not None:
                        ctx.close()
                    ctx = Context(n, device, purpose="decoder")
                    _note_workspace(ctx)
                if model in RAW_CODING_MODELS:
                    out.write(ctx.raw_block_decode(blob[pos:], n, 1))   # block::raw::Decoder, main.rs:73
                else:
                    out.write(ctx.block_decode(model + ANY_BYTE_SUFFIX if any_byte else model, blob[pos:], n))
                pos += ctx.last_consumed()
                records += 1
            if ctx is not None:
                ctx.close()
        if records > 1:
            _note("walked", "%d records without an index footer: every record decoded, but a file cut off at a record boundary cannot be "
                            "told from a complete one (archives written by -b carry a footer; bbb archives and plain concatenations do not)" % records)
        return out_path
    offsets, end = footer
    if gpus <= 1:
        with _AtomicOutput(out_path) as out:  # a record that does not decode leaves no output file, partial or otherwise
            if packed:
                _decode_records_packed(path, model, device, offsets, end, lambda k, data: out.write(data), threads)
            else:
                _decode_records_batched(path, model, device, offsets, end, list(range(len(offsets))), lambda k, data: out.write(data), threads)
        return out_path
    parts = ["%s.part%d" % (out_path, r) for r in range(gpus)]
    procs = []
    devs = _devices(device, gpus, devices)
    for r in range(gpus):
        cmd = [sys.executable, "-m", "dark_amd.cli", "--worker", "%d/%d" % (r, gpus), "--part", parts[r], "-m", model, "-d", str(devs[r]),
               "--host-threads", str(threads), path]
        procs.append(subprocess.Popen(cmd, env=dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.dirname(os.path.abspath(__file__)))] +
                                                                                               os.environ.get("PYTHONPATH", "").split(os.pathsep)))))
    rc = 0
    for p in procs:
        p.wait()
        rc = rc or p.returncode
    if rc:
        for part in parts:
            if os.path.exists(part):
                os.remove(part)
        raise SystemExit("a GPU worker failed (exit code %d)" % rc)
    files = [open(part, "rb") for part in parts]
    with open(path, "rb") as f, _AtomicOutput(out_path) as out:
        for k in range(len(offsets)):
            f.seek(offsets[k])
            n, _ = _split_n(struct.unpack("<I", f.read(4))[0])
            out.write(files[k % gpus].read(n))
    for fobj, part in zip(files, parts):
        fobj.close()
        os.remove(part)
    return out_path


def _worker_decode(args):
    r, g = (int(x) for x in args.worker.split("/"))
    offsets, end = read_footer(args.file)
    with open(args.part, "wb") as out:
        _decode_records_batched(args.file, args.model, args.device, offsets, end, list(range(r, len(offsets), g)), lambda k, data: out.write(data),
                                args.host_threads or 1)


# ---- search (--grep / --grep-hex: dark_amd/search.py) -----------------------------------------------------------------
def _escape(data):
    """bytes outside 0x20 .. 0x7E as \\xNN"""
    return "".join(chr(c) if 0x20 <= c <= 0x7E else "\\x%02x" % c for c in data)


def enclosing_line(window, at, length):
    """of a window of text around a hit (at: the hit's offset in it, length: the pattern's), the part between the nearest newlines on either side"""
    left = window.rfind(b"\n", 0, at) + 1
    right = window.find(b"\n", at + length)
    return window[left:right if right >= 0 else len(window)]


def grep_file(path, model, patterns, device=0, context_bytes=80, count_only=False, max_hits=None, host_threads=0, stats=None, out=None, across=False,
              mismatches=0, ignore_case=False):
    """search FILE.dark pack by pack without inverting a block; prints `absolute_offset:pattern_index:enclosing line` per hit in file order (or
    `pattern_index:count` per pattern) and returns the number of occurrences.  A match that straddles two blocks is found with across=True
    only (--across-blocks).  mismatches=K > 0: the places that differ from a pattern in at most K bytes, as
    `absolute_offset:pattern_index:cost:enclosing line`; ignore_case: ASCII letters without case (--mismatches, -i)."""
    from . import search
    out = out or sys.stdout
    max_hits = search.DEFAULT_MAX_HITS if max_hits is None else max_hits
    counts = np.zeros(len(patterns), dtype=np.int64)
    lines, listed = [], 0
    stats = {} if stats is None else stats
    for found in search.search_archive(path, model, patterns, device, context_bytes, context_bytes, max_hits, host_threads,
                                       count_only=count_only, stats=stats, across=across, mismatches=mismatches, ignore_case=ignore_case):
        hits, occ = found[0], found[1]
        counts += occ.astype(np.int64).sum(axis=1)
        if across:  # the same five fields, from the record that holds the match's first byte
            hits = hits + found[3][0]
            counts += found[3][1].astype(np.int64).sum(axis=1)
        listed += len(hits)
        for hit in hits:  # (a sixth field, the cost, with mismatches or ignore_case)
            _, start, q, pos, text = hit[:5]
            at = min(pos, context_bytes)
            lines.append((start + pos, q, enclosing_line(text, at, len(patterns[q]))) + tuple(hit[5:]))
    if stats.get("seam_skipped"):
        _note("seam_skipped", "pattern%s %s: longer than 4096 bytes, searched inside the blocks only" % (
            "s" if len(stats["seam_skipped"]) > 1 else "", ", ".join(str(q) for q in stats["seam_skipped"])))
    if stats.get("cut_pairs"):
        _note("cut_pairs", "%d (pattern, block) searches stopped at the node limit: their counts are lower bounds" % stats["cut_pairs"])
    if count_only:
        for q, c in enumerate(counts):
            print("%d:%d" % (q, c), file=out)
    else:
        for line in sorted(lines):  # file order: the device lists a segment's hits in the order (pattern, block, suffix-array slot)
            where, q, text = line[:3]
            if mismatches:
                print("%d:%d:%d:%s" % (where, q, line[3], _escape(text)), file=out)
            else:
                print("%d:%d:%s" % (where, q, _escape(text)), file=out)
        if listed < int(counts.sum()):
            _note("max_hits", "%d of %d hits listed: at most --max-hits %d per segment of the archive" % (listed, int(counts.sum()), max_hits))
    return int(counts.sum())


def main(argv=None):
    ap = argparse.ArgumentParser(prog="dark_amd.cli", description="Dark compressor usage: [options] input_file[.dark]")
    ap.add_argument("-m", "--model", default="exp", help="dark|exp|ybs|simple|bbb|raw|rawdc (default exp, like the reference; raw and rawdc are dump-only; bbb: DESIGN.md section 7)")
    ap.add_argument("-b", "--block-size", type=int, default=0, help="cut the input into blocks of this many bytes (extension; streamed and batched)")
    ap.add_argument("-d", "--device", type=int, default=0)
    ap.add_argument("--gpus", type=int, default=1, help="block b -> GPU b mod G, one worker process per GPU (needs -b / an indexed archive)")
    ap.add_argument("--force", action="store_true", help="write archives of blocks containing byte 0xFF (undecodable in the reference format)")
    ap.add_argument("--any-byte", action="store_true", help="encode any file so that it decodes: blocks with byte 0xFF get a flagged record with four "
                    "more bytes (extension, DESIGN.md 4.10); files without 0xFF give the same archive as without the option.  Not with --force")
    ap.add_argument("--host-threads", type=int, default=0, help="host coding threads per GPU (default: CPU quota / gpus - 1)")
    ap.add_argument("--devices", default="", help="GPU ids of the workers, comma separated (default: device, device+1, ...)")
    ap.add_argument("--stats", action="store_true", help="print a JSON line with the wall time of the work and the peak RSS to stderr")
    ap.add_argument("--packed", action="store_true", help="with -b (at most 16 MiB, one GPU): consecutive blocks share one segmented GPU pass "
                    "per 64 MiB pack; the archive is byte-identical to the one without.  On decode (one GPU): records of at most 16 MiB are "
                    "inverted in packs the same way; the output is byte-identical")
    ap.add_argument("--grep", action="append", default=[], metavar="TEXT", help="search FILE.dark for TEXT instead of decoding it (repeatable; one GPU; "
                    "-m as for decoding): the blocks are decoded as far as their BWT and searched there on the GPU, none is inverted and no file is "
                    "written.  Prints absolute_offset:pattern_index:enclosing line per hit in file order; exit status 0 with hits, 1 without.  A "
                    "match that straddles two blocks is NOT found unless --across-blocks is given")
    ap.add_argument("--across-blocks", action="store_true", help="--grep: also find the matches that straddle block borders, by one more GPU query "
                    "per pack over its borders; they are listed and counted among the others")
    ap.add_argument("--grep-hex", action="append", default=[], metavar="HEX", help="the same for a pattern given as hexadecimal bytes (repeatable; "
                    "pattern indices count the --grep patterns first)")
    ap.add_argument("--context-bytes", type=int, default=80, help="--grep: the enclosing line is cut from this many bytes on either side of a hit, "
                    "at the nearest newlines within them (default 80)")
    ap.add_argument("--count-only", action="store_true", help="--grep: print pattern_index:count per pattern only")
    ap.add_argument("--max-hits", type=int, default=None, help="--grep: list at most this many hits per segment of the archive (a pack of up to "
                    "64 MiB; default 65536); counts are always complete")
    ap.add_argument("--mismatches", type=int, default=None, metavar="K", help="--grep: also list the places that differ from a pattern in at most K "
                    "bytes (0..3; no insertions or deletions).  With K > 0 the lines are absolute_offset:pattern_index:cost:enclosing line.  Not "
                    "with --across-blocks")
    ap.add_argument("-i", "--ignore-case", action="store_true", help="--grep: ASCII letters of every pattern, hexadecimal ones included, match "
                    "either case.  Not with --across-blocks")
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    ap.add_argument("--part", default="", help=argparse.SUPPRESS)
    ap.add_argument("file")
    args = ap.parse_args(argv)
    decode = has_extension(args.file, EXTENSION)           # main.rs:56: direction by extension
    if args.worker:
        return _worker_decode(args) if decode else _worker_encode(args)
    t0 = time.perf_counter()
    if args.across_blocks and not (args.grep or args.grep_hex):
        ap.error("--across-blocks goes with --grep / --grep-hex")
    if (args.mismatches is not None or args.ignore_case) and not (args.grep or args.grep_hex):
        ap.error("--mismatches and -i / --ignore-case go with --grep / --grep-hex")
    if args.mismatches is not None and not 0 <= args.mismatches <= 3:
        ap.error("--mismatches: 0 .. 3")
    if (args.mismatches or args.ignore_case) and args.across_blocks:
        ap.error("--mismatches and -i / --ignore-case do not go with --across-blocks: near hits across block borders are not built")
    if args.grep or args.grep_hex:
        if not decode:
            ap.error("--grep searches a .%s archive" % EXTENSION)
        if args.gpus > 1:
            ap.error("--grep: one GPU")
        if args.context_bytes < 0 or (args.max_hits is not None and not 0 <= args.max_hits <= 1 << 31):
            ap.error("--context-bytes and --max-hits: not negative, --max-hits at most 2^31")
        patterns = [t.encode("utf-8", "surrogateescape") for t in args.grep]
        for h in args.grep_hex:
            try:
                patterns.append(bytes.fromhex(h))
            except ValueError:
                ap.error("--grep-hex %r: not hexadecimal bytes" % h)
        if any(len(p) == 0 for p in patterns):
            ap.error("--grep: an empty pattern")
        if (args.mismatches or args.ignore_case) and any(len(p) > 128 for p in patterns):
            ap.error("--mismatches and -i / --ignore-case: patterns of at most 128 bytes")
        st = {}
        found = grep_file(args.file, args.model, patterns, args.device, args.context_bytes, args.count_only, args.max_hits, args.host_threads, st,
                          across=args.across_blocks, mismatches=args.mismatches or 0, ignore_case=args.ignore_case)
        if args.stats:
            import json
            import resource
            print(json.dumps({"seconds": round(time.perf_counter() - t0, 3), "input_bytes": os.path.getsize(args.file), "hits": found,
                              "resident_bytes": st.get("resident_bytes", 0),
                              "peak_rss_bytes": resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024}), file=sys.stderr)
        return 0 if found else 1
    if decode:
        out = decode_file(args.file, args.model, args.device, args.gpus, args.host_threads, args.devices, args.packed)
    else:
        out = encode_file(args.file, args.model, args.block_size, args.device, args.gpus, args.force, args.host_threads, args.devices,
                          args.packed, args.any_byte)
    print(out)
    if args.stats:  # wall time of the work itself (interpreter start and imports of this front end excluded) and this process's peak RSS
        import json
        import resource
        t1 = time.perf_counter()
        line = {"seconds": round(t1 - t0, 3), "seconds_after_setup": round(t1 - STATS.get("t_ready", t0), 3), "input_bytes": os.path.getsize(args.file),
                "output_bytes": os.path.getsize(out), "peak_rss_bytes": resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024}
        if decode and "ws_size_bytes" in STATS:  # (one GPU: with --gpus the contexts live in the worker processes)
            line["ws_size_bytes"] = STATS["ws_size_bytes"]
        print(json.dumps(line), file=sys.stderr)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))  # (None from the coding directions: status 0; --grep: 0 with hits, 1 without)
