"""Approximate search of a .dark archive (dark_amd/search.py mismatches= / ignore_case=, dark_amd/cli.py --mismatches / -i; DESIGN.md section
4.18): search_archive and the command line against a brute-force enumeration, block by block -- the Hamming cost of every pattern at every
position of every block, ASCII letters folded under ignore_case.  200 KB of word-like text with mixed case, as one record and as
-b 4096 --packed.  The archive is unchanged and nothing is written."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from dark_amd import cli, datagen, fm, search

pytestmark = pytest.mark.gpu
N = 200_000
CONTEXT = 80
TIMEOUT = 240


def fold(a):
    """ASCII letters to lower case, every other byte as it is"""
    a = np.asarray(a, dtype=np.uint8)
    return np.where((a >= 65) & (a <= 90), a + 32, a).astype(np.uint8)


def blocks_of(data, block_size):
    return [data[a:a + block_size] for a in range(0, len(data), block_size)] if block_size else [data]


def expected(data, block_size, patterns, k, ignore_case):
    """-> (sorted (record, record's offset, pattern, position, cost) of every near hit inside a block, hits per pattern and record)"""
    hits, occ = [], np.zeros((len(patterns), len(blocks_of(data, block_size))), dtype=np.int64)
    for r, b in enumerate(blocks_of(data, block_size)):
        text = np.frombuffer(b, np.uint8)
        text = fold(text) if ignore_case else text
        for q, p in enumerate(patterns):
            pat, m = np.frombuffer(p, np.uint8), len(p)
            pat = fold(pat) if ignore_case else pat
            if m > len(b):
                continue
            cost = np.zeros(len(b) - m + 1, dtype=np.int64)
            for i in range(m):
                cost += text[i:len(b) - m + 1 + i] != pat[i]
            at = np.flatnonzero(cost <= k)
            occ[q, r] = len(at)
            hits += [(r, r * (block_size or 0), q, int(i), int(cost[i])) for i in at]
    return sorted(hits), occ


def expected_lines(data, block_size, patterns, k, ignore_case):
    blocks = blocks_of(data, block_size)
    lines = []
    for r, start, q, pos, cost in sorted(expected(data, block_size, patterns, k, ignore_case)[0], key=lambda h: (h[1] + h[3], h[2])):
        b, m = blocks[r], len(patterns[q])
        lo, hi = max(pos - CONTEXT, 0), min(pos + m + CONTEXT, len(b))
        left = b.rfind(b"\n", lo, pos) + 1 or lo
        right = b.find(b"\n", pos + m, hi)
        text = "".join(chr(c) if 0x20 <= c <= 0x7E else "\\x%02x" % c for c in b[left:right if right >= 0 else hi])
        lines.append("%d:%d:%d:%s" % (start + pos, q, cost, text) if k else "%d:%d:%s" % (start + pos, q, text))
    return lines


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    work = tmp_path_factory.mktemp("near_archives")
    rng = np.random.default_rng(8)
    text = np.frombuffer(bytes(datagen.word_like(N, seed=5, vocab=2000, alpha=26)), np.uint8).copy()
    up = (rng.random(N) < 0.2) & (text >= 97) & (text <= 122)
    text[up] -= 32
    data = bytes(text)
    assert data != data.lower() and data.count(b"\n") > 1000
    cases = {"single": (data, "exp", 0, {}), "packed4096": (data, "exp", 4096, dict(packed=True))}
    here = os.getcwd()
    os.chdir(str(work))
    try:
        for name, (d, model, block_size, opts) in cases.items():
            with open(name + ".txt", "wb") as f:
                f.write(d)
            assert cli.encode_file(name + ".txt", model, block_size, host_threads=2, **opts) == name + ".dark"
    finally:
        os.chdir(here)
    low = data.lower()
    words = [low[a:a + m] for a, m in ((1203, 7), (50011, 5), (150007, 9)) ]
    patterns = [w.replace(b"\n", b" ") for w in words] + [b"QQQQQZZZ", low[4090:4100].replace(b"\n", b" ")]
    return dict(work=str(work), cases=cases, patterns=patterns)


def run_search(path, model, patterns, **kw):
    hits, occs, records = [], [], []
    for h, occ, ks in search.search_archive(path, model, patterns, host_threads=2, **kw):
        hits += h
        occs.append(occ.astype(np.int64))
        records += ks
    return hits, np.concatenate(occs, axis=1), records


@pytest.mark.parametrize("name", ["single", "packed4096"])
@pytest.mark.parametrize("k,ignore_case", [(1, False), (0, True), (1, True)])
def test_search_archive(corpus, name, k, ignore_case):
    data, model, block_size, _ = corpus["cases"][name]
    patterns = corpus["patterns"]
    path = os.path.join(corpus["work"], name + ".dark")
    before = open(path, "rb").read()
    want, want_occ = expected(data, block_size, patterns, k, ignore_case)
    assert want_occ[:3].sum() >= 3 and want_occ[3].sum() == 0
    blocks = blocks_of(data, block_size)
    stats = {}
    hits, occ, records = run_search(path, model, patterns, mismatches=k, ignore_case=ignore_case, stats=stats)
    assert records == list(range(len(blocks))) and np.array_equal(occ, want_occ) and stats["cut_pairs"] == 0
    assert sorted((r, start, q, pos, cost) for r, start, q, pos, _, cost in hits) == want
    for r, _, q, pos, text, _ in hits:  # the matched text, not the pattern
        assert text == blocks[r][pos:pos + len(patterns[q])]
    assert any(text != patterns[q] for _, _, q, _, text, _ in hits)
    hits, occ, _ = run_search(path, model, patterns, mismatches=k, ignore_case=ignore_case, before=9, after=11)
    assert sorted((r, start, q, pos, cost) for r, start, q, pos, _, cost in hits) == want and np.array_equal(occ, want_occ)
    for r, _, q, pos, text, _ in hits:
        assert text == blocks[r][max(pos - 9, 0):pos + len(patterns[q]) + 11], (r, q, pos)
    hits, occ, _ = run_search(path, model, patterns, mismatches=k, ignore_case=ignore_case, count_only=True)
    assert hits == [] and np.array_equal(occ, want_occ)
    hits, occ, _ = run_search(path, model, patterns, mismatches=k, ignore_case=ignore_case, max_hits=3)
    assert np.array_equal(occ, want_occ) and set((r, start, q, pos, cost) for r, start, q, pos, _, cost in hits) <= set(want)
    assert open(path, "rb").read() == before and not any(f.endswith(".orig") for f in os.listdir(corpus["work"]))


def test_without_the_options_nothing_changes(corpus):
    """the exact search's tuples, from a second call with the options at their defaults"""
    path = os.path.join(corpus["work"], "packed4096.dark")
    patterns = corpus["patterns"]
    for kw in (dict(), dict(before=5, after=5), dict(count_only=True)):
        plain = [(h, occ.tolist(), ks) for h, occ, ks in search.search_archive(path, "exp", patterns, host_threads=2, **kw)]
        again = [(h, occ.tolist(), ks) for h, occ, ks in search.search_archive(path, "exp", patterns, host_threads=2, mismatches=0, ignore_case=False, **kw)]
        assert plain == again and all(len(hit) == 5 for h, _, _ in plain for hit in h)
    stats = {}
    list(search.search_archive(path, "exp", patterns, host_threads=2, stats=stats))
    assert "cut_pairs" not in stats


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


@pytest.mark.parametrize("name", ["single", "packed4096"])
def test_cli_lines(corpus, capsys, name):
    data, model, block_size, _ = corpus["cases"][name]
    patterns = corpus["patterns"]
    args = []
    for p in patterns[:4]:
        args += ["--grep", p.decode()]
    args += ["--grep-hex", patterns[4].hex()]
    listing = sorted(os.listdir(corpus["work"]))
    for k, ignore_case, options in ((1, False, ["--mismatches", "1"]), (0, True, ["-i"]), (2, True, ["--mismatches", "2", "--ignore-case"]),
                                    (0, True, ["--mismatches", "0", "-i"])):
        status, lines, err = grep(corpus, capsys, *(args + options + [name + ".dark"]))
        assert status == 0 and lines == expected_lines(data, block_size, patterns, k, ignore_case), (options, err)
        assert "node limit" not in err
        status, lines, err = grep(corpus, capsys, *(args + options + ["--count-only", name + ".dark"]))
        want_occ = expected(data, block_size, patterns, k, ignore_case)[1]
        assert status == 0 and lines == ["%d:%d" % (q, want_occ[q].sum()) for q in range(len(patterns))], (options, err)
    status, lines, err = grep(corpus, capsys, "--grep", "QQQQQZZZ", "--mismatches", "1", "-i", name + ".dark")
    assert status == 1 and lines == [], err
    status, lines, err = grep(corpus, capsys, "--grep", "QQQQQZZZ", "--mismatches", "1", "--count-only", name + ".dark")
    assert status == 1 and lines == ["0:0"], err
    assert sorted(os.listdir(corpus["work"])) == listing  # nothing written


def test_cli_note_on_the_node_limit(corpus, capsys, monkeypatch):
    """searches that stop at the node limit: the counts are lower bounds and a note on stderr says how many stopped.  (The front end has no
    option for the limit and its default takes a tree of a million nodes: the limit is lowered here, in the call the search makes.)"""
    real = fm.Index.near
    monkeypatch.setattr(fm.Index, "near", lambda self, *a, **kw: real(self, *a, **dict(kw, node_limit=30)))
    monkeypatch.setattr(cli, "_NOTED", set())  # (a note is printed once per run of the front end)
    data, model, block_size, _ = corpus["cases"]["packed4096"]
    patterns = corpus["patterns"][:2]
    want_occ = expected(data, block_size, patterns, 1, False)[1]
    args = ["--grep", patterns[0].decode(), "--grep", patterns[1].decode(), "--mismatches", "1", "--count-only", "packed4096.dark"]
    status, lines, err = grep(corpus, capsys, *args)
    counts = [int(line.split(":")[1]) for line in lines]
    assert len(counts) == 2 and all(0 <= c <= want_occ[q].sum() for q, c in enumerate(counts)) and sum(counts) < want_occ.sum()
    assert status == (0 if sum(counts) else 1)
    note = [line for line in err.splitlines() if "node limit" in line]
    assert len(note) == 1 and "lower bounds" in note[0]
    cut = int(note[0].split("dark_amd: ")[1].split()[0])
    stats = {}
    run_search(os.path.join(corpus["work"], "packed4096.dark"), model, patterns, mismatches=1, count_only=True, stats=stats)
    assert 0 < cut == stats["cut_pairs"] <= want_occ.size


def test_cli_as_a_process(corpus):
    """the exit status of the program itself: 0 with hits, 1 without, 2 for arguments it refuses"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    data, model, block_size, _ = corpus["cases"]["packed4096"]
    p = corpus["patterns"][0]

    def run(*args):
        return subprocess.run([sys.executable, "-m", "dark_amd.cli", "--host-threads", "2"] + list(args), cwd=corpus["work"], env=env,
                              capture_output=True, text=True, timeout=TIMEOUT)
    out = run("--grep", p.decode(), "--mismatches", "1", "-i", "packed4096.dark")
    assert out.returncode == 0 and out.stdout.splitlines() == expected_lines(data, block_size, [p], 1, True), out.stderr[-2000:]
    out = run("--grep", "QQQQQZZZ", "--mismatches", "1", "packed4096.dark")
    assert out.returncode == 1 and out.stdout == "", out.stderr[-2000:]
    out = run("--grep", "x", "--mismatches", "4", "packed4096.dark")
    assert out.returncode == 2 and out.stdout == ""
    out = run("--grep", "x", "-i", "--across-blocks", "packed4096.dark")
    assert out.returncode == 2 and out.stdout == ""
