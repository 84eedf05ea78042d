"""Searching a .dark archive across its block borders (dark_amd/search.py across=True, dark_amd/cli.py --across-blocks):
search_archive and the command line against an enumeration with bytes.find over the WHOLE file, split by the records that hold a match's first
and last byte.  The matches inside one record are what tests/test_gpu_archive_search.py pins (and must stay what they are); the others are the
seam hits.  The corpus is that test's recipe (the helpers are copied, not imported): about 200 KB of word-like text with newlines."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from dark_amd import cli, datagen, search
from dark_amd._lib import FM_SEAM_MAX_PATTERN

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


def expected(data, block_size, patterns, before=0, after=0):
    """-> (inside, occ, seams, seam_occ): sorted (record, record's offset, pattern, position in the record, window) of every occurrence inside a
    record / of every occurrence whose first and last byte lie in different records (record = the one holding the FIRST byte; the window is cut
    at that record's start and at the end of the record holding the last byte); occurrences per pattern and record, the seam hits counted at
    the record holding their LAST byte"""
    bs = block_size or len(data)
    nrec = -(-len(data) // bs)
    inside, seams = [], []
    occ, seam_occ = np.zeros((len(patterns), nrec), np.int64), np.zeros((len(patterns), nrec), np.int64)
    for q, p in enumerate(patterns):
        m = len(p)
        for i in find_all(data, p):
            k, last = i // bs, (i + m - 1) // bs
            window = data[max(i - before, k * bs):min(i + m + after, (last + 1) * bs)]
            if k == last:
                occ[q, k] += 1
                inside.append((k, k * bs, q, i - k * bs, window))
            else:
                seam_occ[q, last] += 1
                seams.append((k, k * bs, q, i - k * bs, window))
    return sorted(inside), occ, sorted(seams), seam_occ


def expected_lines(data, block_size, patterns):
    """the command line's output with --across-blocks: per occurrence in file order `offset:pattern:` and the window of CONTEXT bytes on either
    side, cut at the nearest newlines within it and at the two record ends, bytes outside 0x20 .. 0x7E as \\xNN"""
    inside, _, seams, _ = expected(data, block_size, patterns, CONTEXT, CONTEXT)
    lines = []
    for k, start, q, pos, window in sorted(inside + seams, key=lambda h: (h[1] + h[3], h[2])):
        at, m = min(pos, CONTEXT), len(patterns[q])
        left = window.rfind(b"\n", 0, at) + 1
        right = window.find(b"\n", at + m)
        text = window[left:right if right >= 0 else len(window)]
        lines.append("%d:%d:%s" % (start + pos, q, "".join(chr(c) if 0x20 <= c <= 0x7E else "\\x%02x" % c for c in text)))
    return lines


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """the text, its variants and the archives, made once in a directory of their own (the front end writes into the current directory)"""
    work = tmp_path_factory.mktemp("archives_across")
    plain = bytes(datagen.word_like(N, seed=5, vocab=2000, alpha=26))
    assert plain.count(b"\n") > 1000 and b"\xff" not in plain
    with_ff = bytearray(plain)
    for at in (70000, 70500, 99990, 130000, 65535, 131071):  # the last two: 0xFF 0xFE 0xFF across the borders of the blocks of 65536 bytes
        with_ff[at:at + 3] = b"\xff\xfe\xff"
    with_ff = bytes(with_ff)
    one_value = bytearray(plain)
    one_value[3 * 4096:4 * 4096] = b"z" * 4096  # record 3 of the -b 4096 archive is one byte value
    one_value = bytes(one_value)
    small = plain[:6000]
    cases = {  # name: (text, model, block size, further options of the front end)
        "b100000": (plain, "exp", 100000, {}),
        "packed4096": (plain, "exp", 4096, dict(packed=True)),
        "dark": (plain, "dark", 50000, {}),
        "anybyte": (with_ff, "exp", 65536, dict(any_byte=True)),
        "onevalue": (one_value, "exp", 4096, dict(packed=True)),
        "b64": (small, "exp", 64, dict(packed=True)),  # (the front end takes blocks this small)
    }
    here = os.getcwd()
    os.chdir(str(work))
    try:
        for name, (data, model, block_size, opts) in cases.items():
            with open(name + ".txt", "wb") as f:
                f.write(data)
            assert cli.encode_file(name + ".txt", model, block_size, host_threads=2, **opts) == name + ".dark"
        blob = open("b100000.dark", "rb").read()
        with open("walked.dark", "wb") as f:  # the records of an archive without its footer
            f.write(blob[:cli.read_footer("b100000.dark")[1]])
        cases["walked"] = cases["b100000"]
    finally:
        os.chdir(here)
    # a word, a frequent pair of letters with its space, an absent word, six bytes across the border of the blocks of 100000 bytes, the newline
    word = next(plain[a:a + 7] for a in range(1000, 2000) if b"\n" not in plain[a:a + 7] and not plain[a:a + 1].isspace())
    patterns = [word, b"e t", b"QQQQ", plain[99997:100003], b"\n"]
    assert b"\n" not in patterns[3] and len(find_all(plain, patterns[3])) == 1
    return dict(work=str(work), cases=cases, patterns=patterns, listing=sorted(os.listdir(str(work))))


def patterns_of(corpus, name):
    data = corpus["cases"][name][0]
    patterns = list(corpus["patterns"])
    if name == "anybyte":
        patterns += [b"\xfe\xff", b"\xff", b"\xff\xfe\xff"]
    if name == "onevalue":  # the one-value record's two ends: three bytes of its neighbour and two of its own
        patterns += [b"z" * 4096, b"zzzzz", data[3 * 4096 - 3:3 * 4096 + 2], data[4 * 4096 - 2:4 * 4096 + 3]]
    if name == "packed4096":  # 200 bytes around a border, ten bytes around another, the two bytes at a third
        patterns += [data[4096 * 5 - 100:4096 * 5 + 100], data[4090:4100], data[8191:8193]]
    return patterns


def run_search(path, model, patterns, **kw):
    """-> (hits, occ, records, seam_hits, seam_occ) of the whole archive"""
    hits, occs, records, seam_hits, seam_occs = [], [], [], [], []
    for h, occ, ks, (sh, socc) in search.search_archive(path, model, patterns, host_threads=2, across=True, **kw):
        hits += h
        occs.append(occ.astype(np.int64))
        records += ks
        seam_hits += sh
        seam_occs.append(socc.astype(np.int64))
    return hits, np.concatenate(occs, axis=1), records, seam_hits, np.concatenate(seam_occs, axis=1)


@pytest.mark.parametrize("name", ["b100000", "packed4096", "dark", "anybyte", "onevalue", "walked"])
def test_search_archive_across(corpus, name):
    data, model, block_size, _ = corpus["cases"][name]
    patterns = patterns_of(corpus, name)
    path = os.path.join(corpus["work"], name + ".dark")
    archive = open(path, "rb").read()
    inside, want_occ, seams, want_seam_occ = expected(data, block_size, patterns, 9, 11)
    nrec = want_occ.shape[1]
    for p, total in zip(patterns, (want_occ + want_seam_occ).sum(axis=1)):
        assert total == len(find_all(data, p))  # every occurrence in the file, once
    assert want_seam_occ.sum() > 0 and not want_seam_occ[:, 0].any()
    # today's answer, then the same with across=True: the hits inside the records and their counts do not change
    today = [(h, occ.astype(np.int64), ks) for h, occ, ks in search.search_archive(path, model, patterns, host_threads=2, before=9, after=11)]
    hits, occ, records, seam_hits, seam_occ = run_search(path, model, patterns, before=9, after=11)
    assert hits == [h for part, _, _ in today for h in part] and sorted(hits) == inside
    assert np.array_equal(occ, np.concatenate([o for _, o, _ in today], axis=1)) and np.array_equal(occ, want_occ)
    assert records == list(range(nrec))
    assert np.array_equal(seam_occ, want_seam_occ), np.argwhere(seam_occ != want_seam_occ)[:5].tolist()
    assert sorted(seam_hits) == seams
    # without context the pattern itself; counting alone; a list cut short: the counts stay complete
    hits, occ, _, seam_hits, seam_occ = run_search(path, model, patterns)
    assert sorted(h[:4] for h in seam_hits) == [s[:4] for s in seams] and all(text == patterns[q] for _, _, q, _, text in seam_hits)
    assert np.array_equal(occ, want_occ) and np.array_equal(seam_occ, want_seam_occ)
    stats = {}
    hits, occ, _, seam_hits, seam_occ = run_search(path, model, patterns, count_only=True, stats=stats)
    assert hits == [] and seam_hits == [] and np.array_equal(occ, want_occ) and np.array_equal(seam_occ, want_seam_occ)
    assert stats["seam_skipped"] == [] and stats["resident_bytes"] > 2 * min(len(data), block_size)  # L, the index and the extract structure
    hits, occ, _, seam_hits, seam_occ = run_search(path, model, patterns, max_hits=2)
    assert np.array_equal(seam_occ, want_seam_occ) and set(h[:4] for h in seam_hits) <= set(s[:4] for s in seams)
    segments = search.plan([min(block_size, len(data) - a) for a in range(0, len(data), block_size)])
    assert len(seam_hits) == sum(min(2, int(want_seam_occ[:, ks].sum())) for _, ks, _ in segments)
    if name in ("b100000", "walked"):  # the six bytes at 99997 .. 100003 that the search inside the blocks loses
        assert want_occ[3].sum() == 0 and want_seam_occ[3].tolist() == [0, 1]
        assert [s for s in seams if s[2] == 3] == [(0, 0, 3, 99997, data[99988:100014])]
    if name == "anybyte":
        assert want_seam_occ[-1].tolist() == [0, 1, 1, 0] and want_occ[-1].tolist() == [0, 4, 0, 0]
    if name == "onevalue":
        assert want_occ[-4].tolist() == [1 if k == 3 else 0 for k in range(nrec)] and want_occ[-3, 3] == 4092  # zzzzz at both ends, as today
        assert want_seam_occ[-2, 3] == 1 and want_seam_occ[-1, 4] == 1
    if name == "packed4096":
        assert want_seam_occ[-3].tolist() == [1 if k == 5 else 0 for k in range(nrec)] and want_occ[-3].sum() == 0
    assert open(path, "rb").read() == archive and sorted(os.listdir(corpus["work"])) == corpus["listing"]  # nothing changed, nothing written


@pytest.mark.parametrize("pack_bytes,segments", [(16384, 13), (4096, 49)])
def test_pack_sizes_give_the_same_answer(corpus, pack_bytes, segments):
    """the carry between segments: four records per segment, then one"""
    data, model, block_size, _ = corpus["cases"]["packed4096"]
    patterns = patterns_of(corpus, "packed4096")
    path = os.path.join(corpus["work"], "packed4096.dark")
    assert len(search.plan([4096] * 48 + [N - 48 * 4096], pack_bytes)) == segments
    inside, want_occ, seams, want_seam_occ = expected(data, block_size, patterns, 9, 11)
    parts = list(search.search_archive(path, model, patterns, host_threads=2, across=True, before=9, after=11, pack_bytes=pack_bytes))
    assert len(parts) == segments
    hits, occ, records, seam_hits, seam_occ = run_search(path, model, patterns, before=9, after=11, pack_bytes=pack_bytes)
    assert records == list(range(49)) and sorted(hits) == inside and np.array_equal(occ, want_occ)
    assert np.array_equal(seam_occ, want_seam_occ) and sorted(seam_hits) == seams
    # without across the generator yields what it yields now, segment by segment
    plain = list(search.search_archive(path, model, patterns, host_threads=2, before=9, after=11, pack_bytes=pack_bytes))
    assert [(h, o.tolist(), ks) for h, o, ks in plain] == [(h, o.tolist(), ks) for h, o, ks, _ in parts]


@pytest.mark.parametrize("pack_bytes", [None, 128])
def test_matches_across_three_borders(corpus, pack_bytes):
    """6000 bytes in records of 64: a pattern of 150 bytes crosses two or three borders wherever it stands, and with two records per segment its
    front lies two segments back"""
    data, model, block_size, _ = corpus["cases"]["b64"]
    patterns = [data[a:a + 150] for a in (0, 1, 63, 64, 65, 1003, 3390, 5850)] + [data[100:229], b"e t", data[60:70]]
    path = os.path.join(corpus["work"], "b64.dark")
    inside, want_occ, seams, want_seam_occ = expected(data, block_size, patterns, 9, 11)
    assert all((s[1] + s[3] + len(patterns[s[2]]) - 1) // 64 - s[0] in (2, 3) for s in seams if len(patterns[s[2]]) == 150)
    assert sum((s[1] + s[3] + 149) // 64 - s[0] == 3 for s in seams if len(patterns[s[2]]) == 150) >= 3
    hits, occ, records, seam_hits, seam_occ = run_search(path, model, patterns, before=9, after=11, pack_bytes=pack_bytes)
    assert records == list(range(94)) and sorted(hits) == inside and np.array_equal(occ, want_occ)
    assert np.array_equal(seam_occ, want_seam_occ) and sorted(seam_hits) == seams


def test_a_pattern_above_the_bound_is_skipped(corpus):
    data, model, block_size, _ = corpus["cases"]["packed4096"]
    long_one = data[4000:4000 + FM_SEAM_MAX_PATTERN + 1]  # crosses a border wherever it stands, and is too long for the seam query
    patterns = [corpus["patterns"][0], long_one, data[4090:4100], data[8000:8000 + FM_SEAM_MAX_PATTERN]]
    path = os.path.join(corpus["work"], "packed4096.dark")
    _, want_occ, seams, want_seam_occ = expected(data, block_size, patterns)
    assert want_seam_occ[1].sum() == 1 and want_seam_occ[3].sum() == 1
    stats = {}
    hits, occ, _, seam_hits, seam_occ = run_search(path, model, patterns, stats=stats)
    assert stats["seam_skipped"] == [1]
    want_seam_occ[1] = 0  # left out of the seam query; the others are served, the longest pattern it takes among them
    assert np.array_equal(occ, want_occ) and np.array_equal(seam_occ, want_seam_occ)
    assert sorted(h[:4] for h in seam_hits) == [s[:4] for s in seams if s[2] != 1]


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


@pytest.mark.parametrize("name", ["b100000", "packed4096", "anybyte", "onevalue"])
def test_cli_lines(corpus, capsys, name):
    data, model, block_size, _ = corpus["cases"][name]
    patterns = patterns_of(corpus, name)
    text = patterns[:4]
    hexed = patterns[4:]
    args = ["-m", model, "--across-blocks"]
    for p in text:
        args += ["--grep", p.decode()]
    for p in hexed:
        args += ["--grep-hex", p.hex()]
    status, lines, err = grep(corpus, capsys, *(args + [name + ".dark"]))
    assert status == 0 and lines == expected_lines(data, block_size, patterns), err
    status, lines, err = grep(corpus, capsys, *(args + ["--count-only", name + ".dark"]))
    assert status == 0 and lines == ["%d:%d" % (q, len(find_all(data, p))) for q, p in enumerate(patterns)], err
    # a pattern that stands across a border only: status 1 without the option, 0 with it
    only = patterns[3] if name == "b100000" else patterns[-1]
    _, want_occ, _, want_seam_occ = expected(data, block_size, [only])
    if want_occ.sum() == 0:
        assert want_seam_occ.sum() > 0
        status, lines, err = grep(corpus, capsys, "-m", model, "--grep-hex", only.hex(), name + ".dark")
        assert status == 1 and lines == [], err
        status, lines, err = grep(corpus, capsys, "-m", model, "--grep-hex", only.hex(), "--across-blocks", name + ".dark")
        assert status == 0 and len(lines) == want_seam_occ.sum(), err
    status, lines, err = grep(corpus, capsys, "-m", model, "--grep", "QQQQ", "--across-blocks", name + ".dark")
    assert status == 1 and lines == [], err
    assert sorted(os.listdir(corpus["work"])) == corpus["listing"]  # nothing written: no .orig, no temporary file


def test_cli_as_a_process(corpus):
    """the exit status of the program itself: 0 with hits, 1 without, 2 for arguments it refuses; the note about a skipped pattern"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    data, model, block_size, _ = corpus["cases"]["b100000"]
    p = corpus["patterns"][3]

    def run(*args):
        return subprocess.run([sys.executable, "-m", "dark_amd.cli", "--host-threads", "2"] + list(args), cwd=corpus["work"], env=env,
                              capture_output=True, text=True, timeout=TIMEOUT)
    long_one = data[99000:99000 + FM_SEAM_MAX_PATTERN + 1]
    out = run("--across-blocks", "--grep", p.decode(), "--grep-hex", long_one.hex(), "b100000.dark")
    assert out.returncode == 0 and out.stdout.splitlines() == expected_lines(data, block_size, [p]), out.stderr[-2000:]
    assert "pattern 1" in out.stderr and "4096" in out.stderr
    out = run("--grep", p.decode(), "b100000.dark")
    assert out.returncode == 1 and out.stdout == "", out.stderr[-2000:]
    out = run("--across-blocks", "b100000.dark")
    assert out.returncode == 2 and out.stdout == "" and "--across-blocks" in out.stderr
    assert sorted(os.listdir(corpus["work"])) == corpus["listing"]
