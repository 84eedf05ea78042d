"""Searching a .dark archive without inverting a block (dark_amd/search.py, dark_amd/cli.py --grep): search_archive and
the command line against an enumeration with bytes.find, block by block -- a match that straddles two blocks is not found, and the expectation
leaves it out by construction.  About 200 KB of word-like text with newlines, encoded by the front end in every way the search has a path for."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from dark_amd import cli, datagen, search

pytestmark = pytest.mark.gpu
N = 200_000
CONTEXT = 80
TIMEOUT = 240


def find_all(block, p):
    out, i = [], block.find(p)
    while i >= 0:
        out.append(i)
        i = block.find(p, i + 1)
    return out


def blocks_of(data, block_size):
    return [data[a:a + block_size] for a in range(0, len(data), block_size)] if block_size else [data]


def expected(data, block_size, patterns):
    """-> (sorted (record, record's offset, pattern, position) of every occurrence inside a block, occurrences per pattern and record)"""
    hits, occ = [], []
    blocks = blocks_of(data, block_size)
    for q, p in enumerate(patterns):
        occ.append([])
        for k, b in enumerate(blocks):
            at = find_all(b, p)
            occ[q].append(len(at))
            hits += [(k, k * (block_size or 0), q, i) for i in at]
    return sorted(hits), np.array(occ, dtype=np.int64)


def expected_lines(data, block_size, patterns):
    """the command line's output: per hit in file order `offset:pattern:` and the window of CONTEXT bytes on either side, cut at the nearest
    newlines within it and at the block's ends, bytes outside 0x20 .. 0x7E as \\xNN"""
    blocks = blocks_of(data, block_size)
    lines = []
    for k, start, q, pos in sorted(expected(data, block_size, patterns)[0], key=lambda h: (h[1] + h[3], h[2])):
        b, m = blocks[k], len(patterns[q])
        lo, hi = max(pos - CONTEXT, 0), min(pos + m + CONTEXT, len(b))
        left = b.rfind(b"\n", lo, pos) + 1 or lo
        right = b.find(b"\n", pos + m, hi)
        text = b[left:right if right >= 0 else hi]
        lines.append("%d:%d:%s" % (start + pos, q, "".join(chr(c) if 0x20 <= c <= 0x7E else "\\x%02x" % c for c in text)))
    return lines


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """the text, its variants and the archives, made once in a directory of their own (the front end writes into the current directory)"""
    work = tmp_path_factory.mktemp("archives")
    plain = bytes(datagen.word_like(N, seed=5, vocab=2000, alpha=26))
    assert plain.count(b"\n") > 1000 and b"\xff" not in plain
    with_ff = bytearray(plain)
    for at in (70000, 70500, 99990, 130000):  # all in the second block of 65536 bytes; the other blocks hold no 0xFF
        with_ff[at:at + 3] = b"\xff\xfe\xff"
    with_ff = bytes(with_ff)
    one_value = bytearray(plain)
    one_value[3 * 4096:4 * 4096] = b"z" * 4096  # record 3 of the -b 4096 archive is one byte value
    one_value = bytes(one_value)
    cases = {  # name: (text, model, block size, further options of the front end)
        "single": (plain, "exp", 0, {}),
        "b100000": (plain, "exp", 100000, {}),
        "packed4096": (plain, "exp", 4096, dict(packed=True)),
        "dark": (plain, "dark", 50000, {}),
        "anybyte": (with_ff, "exp", 65536, dict(any_byte=True)),
        "onevalue": (one_value, "exp", 4096, dict(packed=True)),
    }
    here = os.getcwd()
    os.chdir(str(work))
    try:
        for name, (data, model, block_size, opts) in cases.items():
            with open(name + ".txt", "wb") as f:
                f.write(data)
            assert cli.encode_file(name + ".txt", model, block_size, host_threads=2, **opts) == name + ".dark"
        # the records of an archive without its footer: walked by the bytes every record's decode consumes
        blob = open("b100000.dark", "rb").read()
        with open("walked.dark", "wb") as f:
            f.write(blob[:cli.read_footer("b100000.dark")[1]])
        cases["walked"] = cases["b100000"]
    finally:
        os.chdir(here)
    # a word, a frequent pair of letters with its space, an absent word, and six bytes across the border of the blocks of 100000 bytes
    word = next(plain[a:a + 7] for a in range(1000, 2000) if b"\n" not in plain[a:a + 7] and not plain[a:a + 1].isspace())
    patterns = [word, b"e t", b"QQQQ", plain[99997:100003], b"\n"]
    assert b"\n" not in patterns[3] and len(find_all(plain, patterns[3])) == 1  # found in one record, lost where the border cuts it
    assert find_all(plain, b"e t") and not find_all(plain, b"QQQQ")
    return dict(work=str(work), cases=cases, patterns=patterns)


def run_search(path, model, patterns, **kw):
    hits, occs, records = [], [], []
    for h, occ, ks in search.search_archive(path, model, patterns, host_threads=2, **kw):
        hits += h
        occs.append(occ.astype(np.int64))
        records += ks
    return hits, np.concatenate(occs, axis=1) if occs else np.zeros((len(patterns), 0), np.int64), records


@pytest.mark.parametrize("name", ["single", "b100000", "packed4096", "dark", "anybyte", "onevalue", "walked"])
def test_search_archive(corpus, name):
    data, model, block_size, _ = corpus["cases"][name]
    patterns = list(corpus["patterns"])
    if name == "anybyte":
        patterns += [b"\xfe\xff", b"\xff"]
    if name == "onevalue":
        patterns += [b"z" * 4096, b"zzzzz"]
    path = os.path.join(corpus["work"], name + ".dark")
    before = open(path, "rb").read()
    want, want_occ = expected(data, block_size, patterns)
    nrec = want_occ.shape[1]
    hits, occ, records = run_search(path, model, patterns)
    assert records == list(range(nrec)) and np.array_equal(occ, want_occ)
    assert sorted((k, start, q, pos) for k, start, q, pos, _ in hits) == want
    assert all(text == patterns[q] for _, _, q, _, text in hits)
    # with context: the window around every hit, cut at its record's ends
    blocks = blocks_of(data, block_size)
    hits, occ, _ = run_search(path, model, patterns, before=9, after=11)
    assert sorted((k, start, q, pos) for k, start, q, pos, _ in hits) == want and np.array_equal(occ, want_occ)
    for k, start, q, pos, text in hits:
        assert text == blocks[k][max(pos - 9, 0):pos + len(patterns[q]) + 11], (k, q, pos)
    # counting alone, and a list cut short: the counts stay complete
    hits, occ, _ = run_search(path, model, patterns, count_only=True)
    assert hits == [] and np.array_equal(occ, want_occ)
    hits, occ, _ = run_search(path, model, patterns, max_hits=3)
    assert np.array_equal(occ, want_occ) and set((k, start, q, pos) for k, start, q, pos, _ in hits) <= set(want)
    assert len(hits) == sum(min(3, int(want_occ[:, ks].sum())) for _, ks, _ in search.plan([len(b) for b in blocks]))
    if name == "single":
        assert want_occ[3].sum() == 1
    if name in ("b100000", "walked"):
        assert want_occ[3].sum() == 0  # the match across the border is not found
    if name == "anybyte":
        assert want_occ[-2].sum() == 4 and want_occ[-1, 1] == 8 and want_occ[-1].sum() == 8
    if name == "onevalue":
        assert want_occ[-2].tolist() == [1 if k == 3 else 0 for k in range(nrec)] and want_occ[-1, 3] == 4092
    assert open(path, "rb").read() == before and not any(f.endswith(".orig") for f in os.listdir(corpus["work"]))


def grep(corpus, capsys, *args):
    """the front end in this process -> (status, stdout lines, stderr)"""
    capsys.readouterr()
    here = os.getcwd()
    os.chdir(corpus["work"])
    try:
        status = cli.main(["--host-threads", "2"] + list(args))
    finally:
        os.chdir(here)
    out = capsys.readouterr()
    return status, out.out.splitlines(), out.err


@pytest.mark.parametrize("name", ["single", "b100000", "packed4096", "dark", "anybyte", "onevalue"])
def test_cli_lines(corpus, capsys, name):
    data, model, block_size, _ = corpus["cases"][name]
    text = [p for p in corpus["patterns"][:4]]
    hexed = [b"\n"] + ([b"\xfe\xff"] if name == "anybyte" else []) + ([b"z" * 5] if name == "onevalue" else [])
    patterns = text + hexed
    args = ["-m", model]
    for p in text:
        args += ["--grep", p.decode()]
    for p in hexed:
        args += ["--grep-hex", p.hex()]
    listing = sorted(os.listdir(corpus["work"]))
    status, lines, err = grep(corpus, capsys, *(args + [name + ".dark"]))
    assert status == 0 and lines == expected_lines(data, block_size, patterns), err
    status, lines, err = grep(corpus, capsys, *(args + ["--count-only", name + ".dark"]))
    want_occ = expected(data, block_size, patterns)[1]
    assert status == 0 and lines == ["%d:%d" % (q, want_occ[q].sum()) for q in range(len(patterns))], err
    status, lines, err = grep(corpus, capsys, "-m", model, "--grep", "QQQQ", "--grep-hex", "00ff00", name + ".dark")
    assert status == 1 and lines == [], err
    status, lines, err = grep(corpus, capsys, "-m", model, "--grep", "QQQQ", "--count-only", name + ".dark")
    assert status == 1 and lines == ["0:0"], err
    assert sorted(os.listdir(corpus["work"])) == listing  # nothing written: no .orig, no temporary file


def test_cli_context_and_stats(corpus, capsys):
    data, model, block_size, _ = corpus["cases"]["packed4096"]
    p = corpus["patterns"][0]
    status, lines, err = grep(corpus, capsys, "--grep", p.decode(), "--context-bytes", "0", "--stats", "packed4096.dark")
    want = expected(data, block_size, [p])[0]
    assert status == 0 and lines == ["%d:0:%s" % (start + pos, p.decode()) for _, start, _, pos in want]
    stats = json.loads(err.strip().splitlines()[-1])
    total = len(data)
    assert stats["hits"] == len(want) and total < stats["resident_bytes"] < 3 * total + (1 << 20), stats  # L, the index and one structure
    status, lines, err = grep(corpus, capsys, "--grep", "e t", "--max-hits", "2", "packed4096.dark")
    assert status == 0 and len(lines) == 2 and "--max-hits" in err


def test_cli_as_a_process(corpus):
    """the exit status of the program itself: 0 with hits, 1 without, 2 for arguments it refuses"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    data, model, block_size, _ = corpus["cases"]["b100000"]
    p = corpus["patterns"][0]

    def run(*args):
        return subprocess.run([sys.executable, "-m", "dark_amd.cli", "--host-threads", "2"] + list(args), cwd=corpus["work"], env=env,
                              capture_output=True, text=True, timeout=TIMEOUT)
    out = run("--grep", p.decode(), "b100000.dark")
    assert out.returncode == 0 and out.stdout.splitlines() == expected_lines(data, block_size, [p]), out.stderr[-2000:]
    out = run("--grep", "QQQQ", "b100000.dark")
    assert out.returncode == 1 and out.stdout == "", out.stderr[-2000:]
    out = run("--grep", "x", "b100000.txt")
    assert out.returncode == 2 and out.stdout == ""
