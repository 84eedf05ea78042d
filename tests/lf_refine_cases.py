"""TEST HELPER: the built texts and lists of the refinement half of tests/test_gpu_lfirst_layer.py, shared with its worker process
(tests/lf_refine_worker.py).  A case is a text of random bytes with planted strings, a list of groups over it -- the members of a group equal in
their first H0 symbols by construction, a RANDOM symbol in front of every member (256 values, or 2 to keep stretches of a group uniform), places
that are distinct random words below n -- and what the path's route and counters must show so that the case cannot pass through another kernel
than the one it is named for.

How the expectations are derived (the path's own rules, csrc/lfirst.inc; nothing is taken from a run):
  * a list this short gets ONE step of k_lf_finish (LF_SHORT_STEPS): a group of up to 256 members is split by the 7 bytes behind H0; a part that is
    still live (more than one member, and two labels or suffix 0) leaves for the deep list -- one entry and its members in the arena each
    (first_step_leavers).  Parts of up to 64 members are k_lf_deep_wave's, bigger ones k_lf_deep_block's.
  * a group of more than 256 members goes through a big round (lfirst_big_round): five more bytes.  If nearly nothing splits the round stalls, the
    line moves to 4096, the next k_lf_finish lists the groups (one entry each), k_lf_medium takes them and what is stuck for two of its 5-byte
    steps leaves for the arena (another entry each).
  * a pair with more than 2048 + 64 KiB in common is handed on by the wave kernel (one more entry) and ends on the giant list (lfirst_giant).
"""
from types import SimpleNamespace

import numpy as np

H0 = 4
FILL8, FILL32 = 0xC3, 0xC3C3C3C3


class Builder:
    """a text of n random bytes; put() plants strings from the front on, a free byte between them"""

    def __init__(self, seed, n, labels=256):
        self.rng = np.random.default_rng(seed)
        self.n, self.labels = n, labels
        self.t = self.rng.integers(0, 256, size=n, dtype=np.uint8)
        self.at = 16
        self.groups = []   # (members, labels or None)
        self.tail = n      # strings planted at the text's end begin here

    def bytes(self, k):
        return self.rng.integers(0, 256, size=k, dtype=np.uint8)

    def put(self, data, at=None):
        data = np.asarray(data, dtype=np.uint8)
        if at is None:
            at = self.at
            self.at += len(data) + 1
            assert self.at < self.tail - 8, "the text is too short for the case"
        self.t[at:at + len(data)] = data
        return at

    def put_tail(self, data):
        data = np.asarray(data, dtype=np.uint8)
        self.tail = self.n - len(data)
        assert self.tail > self.at + 8
        self.t[self.tail:] = data
        return self.tail

    def tags(self, m, taglen, avoid):
        """m distinct strings of taglen bytes whose first byte is none of `avoid`"""
        out, seen = [], set()
        while len(out) < m:
            for v in self.rng.integers(0, 256 ** taglen, size=2 * m + 16).tolist():
                b = v.to_bytes(taglen, "big")
                if b[0] not in avoid and v not in seen and len(out) < m:
                    seen.add(v)
                    out.append(np.frombuffer(b, np.uint8))
        return out

    def spine_group(self, ds, taglen=2, first_at=None, labels=None, shuffle=True):
        """members that follow one string (the spine) for H0 + ds[j] bytes and then leave it with a tag of their own: two members have
        H0 + min(d, d') bytes in common where their d differ, and H0 + d up to H0 + d + taglen - 1 where they are equal"""
        spine = self.bytes(H0 + max(ds) + 1)
        tags = self.tags(len(ds), taglen, {int(spine[H0 + d]) for d in set(ds)})
        members = [self.put(np.concatenate([spine[:H0 + d], tags[j]]), at=first_at if j == 0 else None) for j, d in enumerate(ds)]
        return self.group(members, labels, shuffle)

    def group(self, members, labels=None, shuffle=True):
        members = list(members)
        if shuffle:
            members = [members[i] for i in self.rng.permutation(len(members))]
        self.groups.append((members, labels))
        return members

    def case(self, name, period=0, **expect):
        idx = np.array([m for g, _ in self.groups for m in g], np.uint32)
        count = len(idx)
        assert len(set(idx.tolist())) == count and count <= self.n
        sizes = [len(g) for g, _ in self.groups]
        gid = np.repeat(np.arange(len(sizes), dtype=np.uint32) * 3 + 5, sizes)
        sym = self.rng.integers(0, self.labels, size=count).astype(np.uint8) * np.uint8(1 if self.labels > 2 else 131)
        for (g, lab), s in zip(self.groups, np.cumsum(sizes) - np.array(sizes)):
            if lab is not None:
                sym[s:s + len(g)] = lab
        pos = self.rng.permutation(self.n)[:count].astype(np.uint32)
        t = bytes(self.t)
        for g, _ in self.groups:  # the construction's promise
            assert all(t[m:m + H0] == t[g[0]:g[0] + H0] and m + H0 <= self.n for m in g), name
        c = SimpleNamespace(name=name, text=self.t, idx=idx, pos=pos, gid=gid, sym=sym, h0=H0, period=period, expect=expect)
        c.leavers = first_step_leavers(c)
        return c


def first_step_leavers(c):
    """(entries, members): the parts of the groups of 2 .. 256 members that one step of k_lf_finish (7 bytes behind h0) leaves live"""
    t, n = bytes(c.text), len(c.text)
    heads = np.flatnonzero(np.concatenate([[True], c.gid[1:] != c.gid[:-1]]))
    entries = members = 0
    for s, e in zip(heads.tolist(), np.append(heads[1:], len(c.gid)).tolist()):
        if not 2 <= e - s <= 256:
            continue
        if len(set(c.sym[s:e].tolist())) < 2 and 0 not in c.idx[s:e]:
            continue  # a final of the first filter
        parts = {}
        for a in range(s, e):
            p = int(c.idx[a]) + c.h0
            if p < n:  # (a suffix that ended in front of the window is alone: the shorter one is smaller)
                parts.setdefault(t[p:p + 7], []).append(a)
        for part in parts.values():
            if len(part) > 1 and (len(set(c.sym[part].tolist())) > 1 or 0 in c.idx[part]):
                entries, members = entries + 1, members + len(part)
    return entries, members


# ---- k_lf_finish -----------------------------------------------------------------------------------------------------------------------------------
def finish(seed=1, labels=256):
    """everything one step settles (the members of a group part inside the first 7 bytes): groups of 2, 255 and 256 members; a group of 256 whose
    head is the last slot of the first 512-slot tile and that ends 255 slots behind it; members that part at bytes 0 .. 5; a member whose suffix
    ends inside the 7-byte window beside one that goes on with zero bytes there, and one whose suffix ended before the window; suffix 0 in a
    group of equal labels"""
    b = Builder(seed, 96 * 1024, labels)
    small = lambda m: b.rng.integers(0, 5, size=m).tolist()  # noqa: E731
    for i in range(254):
        b.spine_group(small(2), labels=[7, 8 + i % 200])      # (two labels each: none of them is a final of the filter, the layout below holds)
    b.spine_group(small(3), labels=[1, 2, 3])
    g256 = b.spine_group(small(256))
    assert sum(len(g) for g, _ in b.groups[:-1]) == 511
    b.spine_group(small(255))
    b.spine_group(small(2))
    b.spine_group([0, 1, 2, 3, 4, 5, 5, 0], taglen=2)
    # the text's end: S x y S.  The member in front of "S x y S" ends inside the window (6 of 7 bytes exist), the last S ended before it
    S, xy = b.bytes(H0), b.bytes(2)
    tail = b.put_tail(np.concatenate([S, xy, S]))
    goes_on = b.put(np.concatenate([S, xy, S, [0, 0, 0, 0, 0, 0]]))   # ... and this one goes on with zero bytes where that one ends
    other = b.put(np.concatenate([S, xy, S[:2], [S[2] ^ 1]]))
    b.group([tail, b.n - H0, goes_on, other])
    # suffix 0: equal labels, so it is the group's only reason
    zero = b.spine_group([1, 0, 3, 2, 2], first_at=0, labels=[9] * 5)
    assert 0 in zero and len(g256) == 256
    return b.case("finish", verdict="l_complete", rounds=1, deep_count=0, arena_used=0, routes_out={"lfirst_big_round", "lfirst_deep", "lfirst_giant"},
                  origin_written=True)


def finish_steps(seed=2, labels=256):
    """members that part at bytes 0 .. 6, at 7 and 8, at 14 and 15 (twice), at 20 and 21: with the step limit of a short list the part that is
    equal in 7 bytes leaves for the deep list; with DK_LF_SHORT_SLOTS=0 (six steps) k_lf_finish takes it to its end -- every step splits it"""
    b = Builder(seed, 64 * 1024, labels)
    for turn in range(6):
        b.spine_group([0, 1, 2, 3, 4, 5, 6, 7, 8, 14, 15, 15, 20, 21], taglen=2)
    return b.case("finish_steps", verdict="l_complete", rounds=1, routes_out={"lfirst_big_round", "lfirst_giant"}, deep="leavers")


# ---- k_lf_deep_wave ---------------------------------------------------------------------------------------------------------------------------------
def tree(b, prefix, exts, fan):
    """copies of copies: `fan` children per level, a child = its parent's string + a byte of its own + exts[0] more bytes"""
    if not exts:
        return [b.put(prefix)]
    first = b.rng.permutation(256)[:fan]
    out = []
    for f in first.tolist():
        out += tree(b, np.concatenate([prefix, [f], b.bytes(exts[0])]), exts[1:], fan)
    return out


def wave(seed=3, labels=256):
    """groups that one step of k_lf_finish does not split, up to 64 members each: 2, 63 and 64 members; 65 (the workgroup kernel's); extensions of
    15, 16, 17, 2047, 2048 and 2049 bytes behind H0 (the lane's cap LW_CAP and the wave's steps behind it); 40 members pairwise different right
    behind the step; copies of copies (nested subgroups)"""
    b = Builder(seed, 160 * 1024, labels)
    for m in (2, 63, 64, 65):
        b.spine_group([10] * m)
    for ext in (15, 16, 17, 2047, 2048, 2049):
        b.spine_group([ext] * 3, taglen=1)
    b.spine_group([7] * 40)
    b.group(tree(b, b.bytes(H0 + 9), [30, 300, 12], 3))
    b.group(tree(b, b.bytes(H0 + 20), [2100, 40], 4))
    return b.case("wave", verdict="l_complete", rounds=1, routes_in={"lfirst_deep"}, routes_out={"lfirst_big_round", "lfirst_giant"}, deep="leavers")


def near_end(k, labels=256):
    """a member that ends k = 0 .. 4 bytes behind the point where it parts from the others (k < 4: the tie bytes are switched off for its
    subgroup), beside one that goes on with zero bytes where it ends"""
    b = Builder(40 + k, 64 * 1024, labels)
    common, extra = b.bytes(H0 + 12), np.array([1, 0, 0, 0], np.uint8)[:k]
    tail = b.put_tail(np.concatenate([common, extra]))
    members = [tail, b.put(np.concatenate([common, extra, [0, 0, 0, 0, 0]])), b.put(np.concatenate([common, [0, 0, 0, 0, 0, 0]])),
               b.put(np.concatenate([common, [1, 0, 0, 0, 0, 1]])), b.put(np.concatenate([common, [2]])), b.put(np.concatenate([common, [1, 1]]))]
    b.group(members)
    b.spine_group([9] * 5)
    return b.case("near_end_%d" % k, verdict="l_complete", rounds=1, routes_in={"lfirst_deep"}, routes_out={"lfirst_big_round", "lfirst_giant"}, deep="leavers")


def giant_pair(seed=5, labels=256):
    """two copies of 68,500 bytes: more than the wave kernel (2048 + 64 KiB) and the workgroup kernel (256 + 64 KiB) measure.  Handed on
    (LD_HANDED: one more entry), then the giant list and the grid-wide measure"""
    b = Builder(seed, 140 * 1024, labels)
    x = b.bytes(68500)
    b.group([b.put(np.concatenate([x, [1]])), b.put(np.concatenate([x, [2]]))], labels=[10, 20])
    b.spine_group([9] * 3)
    return b.case("giant_pair", verdict="l_complete", rounds=1, routes_in={"lfirst_deep", "lfirst_giant"}, routes_out={"lfirst_big_round"}, deep="leavers", handed=1)


def giant_triple(seed=6, labels=256):
    """Z A B A C A C: measured against the first member (A B ...) the other two part at the same place, |A| on, and stay together for all of
    C: a second grid-wide measure.  (With the pivot in front of "A C" one measure would tell all three apart: the list order is kept.)"""
    b = Builder(seed, 352 * 1024, labels)
    a, c = b.bytes(68500), b.bytes(68500)
    c[0] = 200
    m1 = b.put(np.concatenate([a, [100], b.bytes(50)]))
    m2 = b.put(np.concatenate([a, c]))
    m3 = b.put(np.concatenate([a, c, [3]]))
    b.group([m1, m3, m2], labels=[10, 20, 30], shuffle=False)
    return b.case("giant_triple", verdict="l_complete", rounds=1, routes_in={"lfirst_deep", "lfirst_giant"}, routes_out={"lfirst_big_round"}, deep="leavers", handed=1)


# ---- k_lf_deep_block --------------------------------------------------------------------------------------------------------------------------------
def block(seed=7, labels=256):
    """groups of more than 64 members out of k_lf_finish's step: 65 copies; 70 members that leave their spine around 256 (LB_LANE_CAP) and 1024
    bytes behind the step, every byte from 250 to 262 and from 1018 to 1030 among them"""
    b = Builder(seed, 64 * 1024, labels)
    b.spine_group([33] * 65)
    b.spine_group([7 + d for d in range(250, 263)] + [7 + d for d in range(1018, 1031)] + [10] * 44)
    return b.case("block", verdict="l_complete", rounds=1, routes_in={"lfirst_deep"}, routes_out={"lfirst_big_round", "lfirst_giant"}, deep="leavers")


def stall(seed=8, labels=256):
    """groups of 300, 1024, 1025 and 4096 members equal in 20 bytes behind H0: the big round does not split them and stalls, the line moves to
    LF_DEEP_MAX, k_lf_finish lists them (4 LD_LIST entries), k_lf_medium takes them and lets them go after two steps without a split (4 more
    entries, every member in the arena); k_lf_deep_block<1024, 256> orders the first two, <4096, 1024> the others"""
    b = Builder(seed, 256 * 1024, labels)
    for m in (300, 1024, 1025, 4096):
        b.spine_group([20] * m, taglen=3)
    return b.case("stall", verdict="l_complete", rounds=2, deep_count=8, arena_used=300 + 1024 + 1025 + 4096, routes_in={"lfirst_big_round", "lfirst_deep"},
                  routes_out={"lfirst_giant", "period_round"})


# ---- the big rounds -----------------------------------------------------------------------------------------------------------------------------------
def big_sizes(seed=9, labels=256):
    """groups of 257, 4096, 4097, 8192 and 8193 members that part within five bytes: one big round (the grouped sort up to 8192 members, the
    global sort above) settles them all"""
    b = Builder(seed, 256 * 1024, labels)
    for m in (257, 4096, 4097, 8192, 8193):
        b.spine_group(b.rng.integers(0, 3, size=m).tolist(), taglen=2)
    return b.case("big_sizes", verdict="l_complete", rounds=1, deep_count=0, arena_used=0, routes_in={"lfirst_big_round"},
                  routes_out={"lfirst_deep", "lfirst_giant", "period_round"})


def run_in_text(period, seed=10, labels=256):
    """a run of 3000 equal bytes inside text: the suffixes inside it are one group.  period 1: a token round places every member by where the
    run ends (period_round), in the first round.  period 0: the text round stalls, k_lf_medium peels five members per step and the deep list
    orders the rest"""
    b = Builder(seed, 64 * 1024, labels)
    r0 = b.put(np.concatenate([np.full(3000, 97), [98]]).astype(np.uint8))
    b.group(range(r0, r0 + 3000 - H0 + 1))
    b.spine_group([2, 3, 9, 9])
    if period:
        return b.case("run_tokens", period=period, verdict="l_complete", rounds=1, deep="leavers", routes_in={"period_round", "lfirst_big_round"},
                      routes_out={"lfirst_giant"})
    return b.case("run_text", verdict="l_complete", rounds=2, deep="leavers", listed=2, routes_in={"lfirst_big_round", "lfirst_deep"},
                  routes_out={"lfirst_giant", "period_round"})


CASES = dict(finish=finish, finish_steps=finish_steps, wave=wave, giant_pair=giant_pair, giant_triple=giant_triple, block=block, stall=stall,
             big_sizes=big_sizes, run_tokens=lambda **kw: run_in_text(1, **kw), run_text=lambda **kw: run_in_text(0, **kw),
             **{"near_end_%d" % k: (lambda k: lambda **kw: near_end(k, **kw))(k) for k in range(5)})
WAVE_CASES = ("wave", "giant_pair", "near_end_0", "near_end_1", "near_end_2", "near_end_3", "near_end_4")


def expected_counters(c, by_wave=True):
    """-> (deep_count, arena_used) or None where the case does not pin them"""
    e = c.expect
    if "deep_count" in e:
        return e["deep_count"], e["arena_used"]
    if e.get("deep") == "leavers":
        entries, members = c.leavers
        listed = e.get("listed", 0)  # (a group that the stalled big list let go: its LD_LIST entry, and the entry of what k_lf_medium left over)
        return entries + listed + (e.get("handed", 0) if by_wave else 0), None if listed else members
    return None


def check_gave_up(c, got):
    """the path gave up half way: START_OVER, and it has written to listed places of L only"""
    facts = {k: got[k] for k in ("verdict", "rounds", "deep_count", "arena_used", "giant_count", "fallback")}
    assert got["verdict"] == "start_over", (c.name, facts)
    unlisted = np.ones(len(c.text), bool)
    unlisted[c.pos] = False
    assert (got["bwt"][unlisted] == FILL8).all(), "%s: a give-up wrote to L outside the listed places" % c.name
    return facts


def check_result(c, got, want_L, want_origin, by_wave=True, counters=None):
    """the whole of L and the origin against the model, then the route and the counters the case is named for (counters: in place of the case's)"""
    e = c.expect
    bad = np.flatnonzero(got["bwt"] != want_L)
    assert len(bad) == 0, "%s: L differs from the model at %d of %d places, first at %d: got %#x want %#x (listed: %s)" % (
        c.name, len(bad), len(want_L), bad[0], got["bwt"][bad[0]], want_L[bad[0]], bool(np.isin(bad[0], c.pos)))
    assert got["origin"] == want_origin, "%s: origin %#x, model %#x" % (c.name, got["origin"], want_origin)
    assert (want_origin != FILL32) == bool(e.get("origin_written", False)), c.name
    facts = {k: got[k] for k in ("verdict", "rounds", "deep_count", "arena_used", "giant_count", "fallback")}
    facts["routes"] = sorted(got["routes"])
    assert got["verdict"] == e["verdict"] and got["fallback"] == 0, (c.name, facts)
    assert "lfirst" in got["routes"] and e.get("routes_in", set()) <= got["routes"] and not (e.get("routes_out", set()) & got["routes"]), (c.name, facts)
    assert got["rounds"] == e["rounds"], (c.name, facts)
    want = counters or expected_counters(c, by_wave)
    if want is not None:
        assert got["deep_count"] == want[0] and (want[1] is None or got["arena_used"] == want[1]), (c.name, facts, want)
    return facts
