"""Shared by tests/test_emu_columns_merge.py (CPU, emulator build) and tests/test_gpu_columns_merge.py (MI355X): the cases of the
columnar merge (dsrcgpu_columns_merge_device; dsrc_amd/csrc/k_columns_merge.h) and what they must give.

The reference has no counterpart, so the yardstick is the integer model written out here: merge_model() is the serial rule of
include/dsrc_gpu.h word for word, one pair and one position at a time in Python integers -- the five reasons in their order, the
consensus table, the twelve statistics.  COMP is built from the alphabet and the letter pairs, not copied from the kernel's table.
None of it comes from the library under test, and every comparison is exact equality.  Output arrays are filled with 0xA5 before a
call, so that "nothing written" can be asserted.  Before the library is compared on a crafted case the model alone is asked whether
the case is what it was built for.

How a pair is made.  perfect_pair() cuts both mates out of one insert: record 1 holds the insert positions 0 .. f1 + n1 - 1, record
2 the reverse complement's 0 .. f2 + n2 - 1, so insert position P is byte P of record 1 and byte I - 1 - P of record 2 -- a plant at
an insert position is two pokes.  The ranges are [f, f + n) of either record, the insert size is I.

Shapes.  The emulator pays a coroutine switch per wave exchange, so its pair-plan fuzz is 2 seeds x 120 pairs where the GPU runs 6 x
1200.  The judge's and the writer's grids hold at most 4096 workgroups of WG / 64 waves: with workgroups of 1024 threads a count above
65536 pairs takes the grid stride into a second round -- that count runs on the GPU only."""
from __future__ import annotations

import dataclasses

import numpy as np
import torch        # noqa: F401  before the first handle (see columns_cases)

from tests import columns_adapt_cases as ca
from tests import columns_enc_cases as ce
from tests import columns_pair_cases as cp
from tests import columns_sel_cases as cs
from tests._oracle import Config

E_ARG, E_INPUT, E_CAPACITY = cs.E_ARG, cs.E_INPUT, -4
NO_INSERT = 2 ** 64 - 1
SHAPES = cp.SHAPES
Arrays = ce.Arrays
Dev = cs.Dev
handle, staged, tensors = cp.handle, cp.staged, cp.tensors
MERGE_STATS = ("pairs_merged", "bases_written", "overlap_sum", "overlap_agree", "overlap_corrected", "overlap_one_sided", "overlap_neither",
               "not_kept", "no_insert", "bad_geometry", "short_overlap", "over_budget")
R_KEEP, R_INSERT, R_GEOMETRY, R_SHORT, R_BUDGET = 7, 8, 9, 10, 11

ALPHABET = "ACGTNRWSKMDVHBYXU.-"


def _comp_table():
    t = {ch: ch for ch in ALPHABET}
    for u, v in ("AT", "CG", "RY", "KM", "DH", "VB"):
        t[u], t[v] = v, u
    t["U"] = "A"
    return [ALPHABET.index(t[ch]) for ch in ALPHABET]


COMP = _comp_table()
comp = lambda c: COMP[c] if c <= 18 else c


# ---- the model -------------------------------------------------------------------------------------------------------------------
def rules_of(min_overlap=30, max_mm=5, rate=200, cap=41):
    return dict(min_overlap=min_overlap, max_mm=max_mm, rate=rate, cap=cap)


def consensus(c1, q1, c2, q2, cap):
    """One position that both reads cover -> (code, quality, statistic)."""
    if c1 < 4 and c2 < 4:
        if c1 == c2:
            return c1, min(q1 + q2, max(cap, q1, q2)), 3
        return (c1, q1 - q2, 4) if q1 >= q2 else (c2, q2 - q1, 4)
    if c1 < 4:
        return c1, q1, 5
    if c2 < 4:
        return c2, q2, 5
    return c1, min(q1, q2), 6


@dataclasses.dataclass
class Want:
    bases: np.ndarray
    quals: np.ndarray
    titles: object
    seq_offs: np.ndarray
    title_offs: object
    source: np.ndarray
    merged: np.ndarray
    totals: list
    stats: list
    why: list               # per pair: 0 = merged, else the statistic it counts in
    V: list                 # per pair: the overlap, None where the rule does not get that far

    def read(self, r):
        """The merged read of pair r -> (codes, qualities) as lists."""
        j = int(np.nonzero(self.source == r)[0][0])
        s, e = int(self.seq_offs[j]), int(self.seq_offs[j + 1])
        return self.bases[s:e].tolist(), self.quals[s:e].tolist()


def merge_model(a1: Arrays, a2: Arrays, rules, rg1=(None, None), rg2=(None, None), keep=None, insert=None, titles=True, first=0, n=None):
    """The rule of include/dsrc_gpu.h.  rg<s> = (begin, end) as positions in a<s>.bases of the pairs first .. first + n - 1."""
    assert a1.n_records == a2.n_records
    n = a1.n_records - first if n is None else n
    B1, Q1, B2, Q2 = a1.bases.tolist(), a1.quals.tolist(), a2.bases.tolist(), a2.quals.tolist()
    S1, S2 = [int(v) for v in a1.seq_offsets], [int(v) for v in a2.seq_offsets]
    T1 = [int(v) for v in a1.title_offsets]
    ob, oq, ot, so, to, src = [], [], [], [0], [0], []
    merged, why, Vs = np.zeros(n, np.uint8), [], []
    stats = [0] * 12
    for k in range(n):
        r = first + k
        b1, e1 = (S1[r], S1[r + 1]) if rg1[0] is None else (int(rg1[0][k]), int(rg1[1][k]))
        b2, e2 = (S2[r], S2[r + 1]) if rg2[0] is None else (int(rg2[0][k]), int(rg2[1][k]))
        assert S1[r] <= b1 <= e1 <= S1[r + 1] and S2[r] <= b2 <= e2 <= S2[r + 1]
        f1, n1, f2, n2 = b1 - S1[r], e1 - b1, b2 - S2[r], e2 - b2
        I = int(insert[k])
        V = None
        if keep is not None and int(keep[k]) == 0:
            y = R_KEEP
        elif I == NO_INSERT:
            y = R_INSERT
        elif I >= 2 ** 40 or n1 == 0 or n2 == 0 or I < f2 + n2 or f1 + n1 > I:
            y = R_GEOMETRY
        else:
            a1_, z1, a2_, z2 = f1, f1 + n1, I - f2 - n2, I - f2
            V = min(z1, z2) - max(a1_, a2_)
            y = 0
            if V < rules["min_overlap"]:
                y = R_SHORT
            else:
                at = lambda p: (B1[b1 + p - a1_], Q1[b1 + p - a1_], comp(B2[e2 - 1 - (p - a2_)]), Q2[e2 - 1 - (p - a2_)])
                mm = 0
                for p in range(max(a1_, a2_), min(z1, z2)):
                    c1, _, c2, _ = at(p)
                    if c1 != c2 or c1 >= 4 or c2 >= 4:
                        mm += 1
                if mm > rules["max_mm"] or mm * 1000 > V * rules["rate"]:
                    y = R_BUDGET
                else:
                    for p in range(min(a1_, a2_), max(z1, z2)):
                        in1, in2 = a1_ <= p < z1, a2_ <= p < z2
                        if in1 and in2:
                            c, q, st = consensus(*at(p), rules["cap"])
                            stats[st] += 1
                        elif in1:
                            c, q = B1[b1 + p - a1_], Q1[b1 + p - a1_]
                        else:
                            assert in2
                            c, q = comp(B2[e2 - 1 - (p - a2_)]), Q2[e2 - 1 - (p - a2_)]
                        ob.append(c); oq.append(q)
                    stats[0] += 1; stats[1] += max(z1, z2) - min(a1_, a2_); stats[2] += V
                    merged[k] = 1; src.append(k); so.append(len(ob))
                    if titles:
                        ot.extend(a1.titles[T1[r]: T1[r + 1]].tolist()); to.append(len(ot))
        if y:
            stats[y] += 1
        why.append(y); Vs.append(V)
    assert stats[3] + stats[4] + stats[5] + stats[6] == stats[2] and stats[0] + sum(stats[7:]) == n
    u8 = lambda v: np.array(v, np.uint8)
    return Want(u8(ob), u8(oq), u8(ot) if titles else None, np.array(so, np.uint64), np.array(to, np.uint64) if titles else None,
                np.array(src, np.uint64), merged, [len(src), len(ob), len(ot) if titles else 0], stats, why, Vs)


# ---- pairs -----------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Pair:
    x: np.ndarray           # record 1, its qualities, record 2, its qualities
    qx: np.ndarray
    z: np.ndarray
    qz: np.ndarray
    r1: tuple               # (f1, f1 + n1): the range in record 1
    r2: tuple
    I: int
    keep: int = 1

    def geo(self):
        """-> a1, z1, a2, z2."""
        return self.r1[0], self.r1[1], self.I - self.r2[1], self.I - self.r2[0]

    def overlap(self):
        a1, z1, a2, z2 = self.geo()
        return max(a1, a2), min(z1, z2)

    def plant(self, P, c1=None, q1=None, raw2=None, q2=None):
        """At insert position P: record 1's byte P, record 2's byte I - 1 - P."""
        if c1 is not None: self.x[P] = c1
        if q1 is not None: self.qx[P] = q1
        if raw2 is not None: self.z[self.I - 1 - P] = raw2
        if q2 is not None: self.qz[self.I - 1 - P] = q2


def perfect_pair(I, f1, n1, f2, n2, rng, tail1=0, tail2=0, keep=1):
    assert f1 + n1 <= I and f2 + n2 <= I
    ins = rng.integers(0, 4, I).astype(np.uint8)
    x = np.concatenate((ins[:f1 + n1], rng.integers(0, 4, tail1))).astype(np.uint8)
    z = np.concatenate((cp.revcomp(ins)[:f2 + n2], rng.integers(0, 4, tail2))).astype(np.uint8)
    q = lambda v: rng.integers(0, 42, len(v)).astype(np.uint8)
    return Pair(x, q(x), z, q(z), (f1, f1 + n1), (f2, f2 + n2), I, keep)


def raw_pair(len1, r1, len2, r2, I, rng, keep=1):
    """Random records with any ranges and any I: what the geometry must refuse, or what does not match."""
    x, z = rng.integers(0, 4, len1).astype(np.uint8), rng.integers(0, 4, len2).astype(np.uint8)
    return Pair(x, rng.integers(0, 42, len1).astype(np.uint8), z, rng.integers(0, 42, len2).astype(np.uint8), r1, r2, I, keep)


def build(pairs, title=lambda r: b"@p%d" % r + b"/" * (r % 7)):
    """-> arrays 1, arrays 2, ranges 1, ranges 2 (positions in the arrays), keep, insert."""
    prefix = lambda v: np.concatenate(([0], np.cumsum(np.asarray(v, np.int64)))).astype(np.uint64)
    cat = lambda v: np.concatenate(list(v) + [np.zeros(0, np.uint8)]).astype(np.uint8)
    titles = [title(r) for r in range(len(pairs))]
    T = np.frombuffer(b"".join(titles), np.uint8).copy()
    out = []
    for rec, ql in ((lambda p: p.x, lambda p: p.qx), (lambda p: p.z, lambda p: p.qz)):
        S = prefix([len(rec(p)) for p in pairs])
        out.append(Arrays(cat(rec(p) for p in pairs), cat(ql(p) for p in pairs), T, S, prefix([len(t) for t in titles]), [0, len(pairs)]))
    a1, a2 = out
    rg = lambda a, sel: ((a.seq_offsets[:-1] + np.array([sel(p)[0] for p in pairs], np.uint64)).astype(np.uint64),
                         (a.seq_offsets[:-1] + np.array([sel(p)[1] for p in pairs], np.uint64)).astype(np.uint64))
    return (a1, a2, rg(a1, lambda p: p.r1), rg(a2, lambda p: p.r2), np.array([p.keep for p in pairs], np.uint8),
            np.array([p.I for p in pairs], np.uint64))


# ---- one call ----------------------------------------------------------------------------------------------------------------------
def lib_rules(lib, rules, reserved=(0, 0, 0, 0)):
    return lib.MergeRules(rules["min_overlap"], rules["max_mm"], rules["rate"], rules["cap"], reserved)


class MergeCall:
    """One dsrcgpu_columns_merge_device on output arrays this test owns (0xA5-filled, allocated for K / S / T entries; the
    capacities told to the library may be smaller).  rg<s> / keep / insert: numpy arrays in the coordinates of the staged arrays."""

    def __init__(self, lib, h, cin1, cin2, n, mr, rg1, rg2, keep, insert, K, S, T, titles=True, caps=None, source=True, null=()):
        caps = caps or {}
        with Dev(h) as d:
            up = lambda v, dt: None if v is None else d.up(np.ascontiguousarray(v).astype(dt).tobytes())
            sizes = {"bases": S, "quals": S, "titles": T, "seq_offs": 8 * (K + 1), "title_offs": 8 * (K + 1), "source": 8 * K, "merged": n}
            ptr = {k: d.fill(v) for k, v in sizes.items()}
            out = lib.Columns(ptr["bases"], caps.get("bases_cap", S), ptr["quals"], caps.get("quals_cap", S),
                              ptr["titles"] if titles else None, caps.get("titles_cap", T) if titles else 0,
                              ptr["seq_offs"], ptr["title_offs"] if titles else None, caps.get("records_cap", K))
            self.error = self.totals = self.stats = None
            try:
                self.totals, self.stats = h.columns_merge_device(
                    cin1, cin2, mr, (up(rg1[0], np.uint64), up(rg1[1], np.uint64)), (up(rg2[0], np.uint64), up(rg2[1], np.uint64)),
                    up(keep, np.uint8), None if "insert" in null else up(insert, np.uint64), out, None if "merged" in null else ptr["merged"],
                    ptr["source"] if source else None)
            except lib.DsrcGpuError as e:
                self.error = e
            self.raw = {k: d.down(ptr[k], v) for k, v in sizes.items()}
        assert all(r[-8:] == b"\xA5" * 8 for r in self.raw.values()), "written behind the end of an output array"

    def untouched(self, *names):
        return all(self.raw[k] == b"\xA5" * len(self.raw[k]) for k in (names or self.raw))

    def array(self, name, count, dtype=np.uint8):
        return np.frombuffer(self.raw[name], dtype=dtype)[:count]

    def assert_equals(self, w: Want, titles=True, source=True, what=None):
        assert self.error is None, (what, self.error)
        K, S, T = w.totals
        assert self.stats == w.stats, (what, self.stats, w.stats)
        assert self.totals == w.totals, (what, self.totals, w.totals)
        n = len(w.merged)
        bad = np.nonzero(self.array("merged", n) != w.merged)[0]
        assert len(bad) == 0, (what, "d_merged, pair", int(bad[0]), len(bad))
        assert np.array_equal(self.array("seq_offs", K + 1, np.uint64), w.seq_offs), what
        for name, want in (("bases", w.bases), ("quals", w.quals)):
            bad = np.nonzero(self.array(name, S) != want)[0]
            if len(bad):
                j = int(np.searchsorted(w.seq_offs, bad[0], side="right")) - 1
                raise AssertionError((what, name, "output record", j, "pair", int(w.source[j]), "position", int(bad[0]) - int(w.seq_offs[j]),
                                      int(self.array(name, S)[bad[0]]), "want", int(want[bad[0]]), len(bad)))
        tail = lambda name, used: self.raw[name][used:] == b"\xA5" * (len(self.raw[name]) - used)
        assert tail("bases", S) and tail("quals", S) and tail("seq_offs", 8 * (K + 1)) and tail("merged", n), what
        if titles:
            assert np.array_equal(self.array("titles", T), w.titles), what
            assert np.array_equal(self.array("title_offs", K + 1, np.uint64), w.title_offs), what
            assert tail("titles", T) and tail("title_offs", 8 * (K + 1)), what
        else:
            assert self.untouched("titles", "title_offs"), what
        if source:
            assert np.array_equal(self.array("source", K, np.uint64), w.source) and tail("source", 8 * K), what
        else:
            assert self.untouched("source"), what


def padded(rg, pad):
    return tuple(None if v is None else np.asarray(v).astype(np.uint64) + np.uint64(pad) for v in rg)


def check_merge(lib, h, st1, st2, rules, rg1, rg2, keep, insert, pad=(0, 0), first=0, n=None, titles=True, what=None, model=None, source=True,
                titles_in2=True):
    """Arrays staged in st1 / st2, the ranges as positions in the UNPADDED arrays (the pads are added here) -> the call == the model."""
    n = st1.a.n_records - first if n is None else n
    w = model if model is not None else merge_model(st1.a, st2.a, rules, rg1, rg2, keep, insert, titles, first, n)
    K, S, T = w.totals
    cin1, cin2 = st1.cols_in(first, n), st2.cols_in(first, n)
    if not titles_in2:
        cin2 = lib.ColumnsIn(cin2.d_bases, cin2.bases_len, cin2.d_quals, None, 0, cin2.d_seq_offs, None, n)
    call = MergeCall(lib, h, cin1, cin2, n, lib_rules(lib, rules), padded(rg1, pad[0]), padded(rg2, pad[1]), keep, insert, K, S, T, titles, source=source)
    call.assert_equals(w, titles, source, what)
    return w


# ---- geometry --------------------------------------------------------------------------------------------------------------------
SIZES = [1, 63, 64, 65, 127, 128, 129]


def geometry_pairs(rng):
    """-> pairs, {name: index}."""
    pairs, at = [], {}

    def add(name, p):
        at[name] = len(pairs); pairs.append(p)
    for v in SIZES:
        add(("V", v), perfect_pair(v + 12, 0, v + 5, 0, v + 7, rng, tail1=3))          # staggered: a1 < a2, z1 < z2, V = v
        add(("V = n1 = n2", v), perfect_pair(v, 0, v, 0, v, rng))                        # V = L = v
        if v > 1:
            add(("L", v), perfect_pair(v, 0, v // 2 + 1, 0, v - v // 2, rng, tail2=2))   # V = 1, L = v
    add("1024", perfect_pair(1500, 0, 1024, 0, 1024, rng))
    add("a1 == a2", perfect_pair(100, 0, 80, 0, 100, rng, tail1=9))                      # a1 = a2 = 0, z1 < z2
    add("a1 > a2, z1 == z2", perfect_pair(100, 5, 95, 0, 100, rng, tail2=30))            # read-through, f1 > 0
    add("z1 > z2", perfect_pair(100, 0, 100, 7, 93, rng, tail1=30))                      # f2 > 0: z2 = 93, a2 = 0 = a1
    add("1 inside 2", perfect_pair(150, 20, 60, 10, 130, rng))                           # a2 = 10 < a1 = 20, z1 = 80 < z2 = 140
    add("2 inside 1", perfect_pair(150, 10, 130, 70, 60, rng))                           # a1 = 10 < a2 = 20, z2 = 80 < z1 = 140
    for f1 in (0, 1, 63, 64):
        for f2 in (0, 1, 63, 64):
            add(("f", f1, f2), perfect_pair(200, f1, 120, f2, 120, rng, tail1=f2 % 3, tail2=f1 % 3))
    add("after 1024", perfect_pair(90, 0, 70, 0, 60, rng))
    add("last", perfect_pair(200, 3, 150, 2, 150, rng))                                  # flush with bases_len on both sides
    return pairs, at


def run_geometry(lib, sh):
    rng = np.random.default_rng(4100)
    pairs, at = geometry_pairs(rng)
    a1, a2, rg1, rg2, keep, insert = build(pairs)
    assert int(a1.seq_offsets[-1]) == len(a1.bases) == int(rg1[1][-1]) and int(a2.seq_offsets[-1]) == len(a2.bases) == int(rg2[1][-1])
    rules = rules_of(1, 0, 0, 41)
    w = merge_model(a1, a2, rules, rg1, rg2, keep, insert)
    assert all(y == 0 for y in w.why), w.why                 # the model alone: every pair merges, with the overlap and the length it was built for
    L = lambda r: int(w.seq_offs[int(np.nonzero(w.source == r)[0][0]) + 1] - w.seq_offs[int(np.nonzero(w.source == r)[0][0])])
    for v in SIZES:
        assert w.V[at[("V", v)]] == v and L(at[("V", v)]) == v + 12
        assert w.V[at[("V = n1 = n2", v)]] == v == L(at[("V = n1 = n2", v)])
        if v > 1:
            assert w.V[at[("L", v)]] == 1 and L(at[("L", v)]) == v
    assert w.V[at["1024"]] == 548 and L(at["1024"]) == 1500
    geo = lambda name: pairs[at[name]].geo()
    assert geo("a1 == a2")[0] == geo("a1 == a2")[2] and geo("a1 > a2, z1 == z2") == (5, 100, 0, 100) and geo("z1 > z2") == (0, 100, 0, 93)
    assert geo("1 inside 2") == (20, 80, 10, 140) and geo("2 inside 1") == (10, 140, 20, 80)
    assert w.stats[3] == w.stats[2] and w.stats[4] == w.stats[5] == w.stats[6] == 0
    h = handle(lib)
    try:
        for pad in ((0, 0), (1, 3), (5, 1)):                 # the arrays start at odd addresses
            with staged(lib, h, a1, pad=pad[0]) as st1, staged(lib, h, a2, pad=pad[1]) as st2:
                check_merge(lib, h, st1, st2, rules, rg1, rg2, keep, insert, pad=pad, what=("geometry", pad), model=w)
                check_merge(lib, h, st1, st2, rules, rg1, rg2, None, insert, pad=pad, what=("no keep", pad), model=w, source=False)
                for first, cnt in ((at["1024"], None), (len(pairs) - 1, 1), (5, 9)):       # d_seq_offs + k
                    sl = slice(first, None if cnt is None else first + cnt)
                    cut = lambda rg: (rg[0][sl], rg[1][sl])
                    check_merge(lib, h, st1, st2, rules, cut(rg1), cut(rg2), keep[sl], insert[sl], pad=pad, first=first, n=cnt, what=("first", first, pad))
        # whole reads: records that ARE their ranges
        whole = [perfect_pair(I, 0, n1, 0, n2, rng) for I, n1, n2 in ((100, 100, 100), (180, 150, 150), (64, 33, 32), (90, 90, 20))]
        b1, b2, _, _, wk, wi = build(whole)
        with staged(lib, h, b1, pad=3) as st1, staged(lib, h, b2, pad=0) as st2:
            ww = check_merge(lib, h, st1, st2, rules, (None, None), (None, None), None, wi, pad=(3, 0), what="whole reads")
            assert ww.why == [0, 0, 0, 0]
    finally:
        h.close()


# ---- consensus ---------------------------------------------------------------------------------------------------------------------
def consensus_pairs(rng):
    """-> pairs, [(pair, insert position, what the merged read must hold there: (code, quality))] -- written down by hand."""
    pairs, expect = [], []
    new = lambda: perfect_pair(170, 0, 150, 0, 150, rng)     # overlap [20, 150): V = 130; the positions 0, 63, 64, V - 1 of it
    spots = [20, 83, 84, 149]
    for case in range(4):
        p = new()
        for P in spots:
            c = int(p.x[P])
            if case == 0:
                p.plant(P, q1=11, q2=12); expect.append((len(pairs), P, (c, 23)))
            elif case == 1:
                p.plant(P, q1=30, raw2=3 - (c + 1) % 4, q2=12); expect.append((len(pairs), P, (c, 18)))
            elif case == 2:
                p.plant(P, c1=4, q1=40, q2=7); expect.append((len(pairs), P, (c, 7)))
            else:
                p.plant(P, c1=5, q1=9, raw2=4, q2=8); expect.append((len(pairs), P, (5, 8)))
        pairs.append(p)
    p = new()
    plants = [(25, dict(q1=10, q2=20), 30), (26, dict(q1=20, q2=21), 41), (27, dict(q1=30, q2=30), 41),        # q1 + q2 below, at, above the cap
              (28, dict(q1=60, q2=5), 60), (29, dict(q1=5, q2=200), 200), (30, dict(q1=0, q2=0), 0),             # a quality above the cap stays
              (31, dict(q1=255, q2=255), 255), (32, dict(q1=0, q2=255), 255)]
    for P, kw, q in plants:
        p.plant(P, **kw); expect.append((len(pairs), P, (int(p.x[P]), q)))
    for P, q1, q2 in ((40, 30, 10), (41, 10, 30), (42, 17, 17), (43, 255, 0), (44, 0, 255)):                    # disagreement
        c = int(p.x[P]); other = (c + 2) % 4
        p.plant(P, q1=q1, raw2=3 - other, q2=q2)
        expect.append((len(pairs), P, (c, q1 - q2) if q1 >= q2 else (other, q2 - q1)))
    p.plant(50, c1=4, q1=40, q2=3); expect.append((len(pairs), 50, (int(3 - p.z[p.I - 1 - 50]), 3)))            # exactly one below 4: read 2's
    c = int(p.x[51]); p.plant(51, q1=2, raw2=14, q2=40); expect.append((len(pairs), 51, (c, 2)))                # ... read 1's (Y -> R is no base)
    for P, c1, raw2, want in ((60, 4, 4, 4), (61, 18, 18, 18), (62, 255, 255, 255), (63, 5, 255, 5), (64, 255, 6, 255), (65, 14, 5, 14)):
        p.plant(P, c1=c1, q1=20 + P % 3, raw2=raw2, q2=21); expect.append((len(pairs), P, (want, min(20 + P % 3, 21))))       # neither below 4
    # a code >= 4 whose low bits are the partner's code: no agreement, the proper base wins with its own quality
    c = int(p.x[70]); p.plant(70, c1=4 + c, q1=40, q2=6); expect.append((len(pairs), 70, (c, 6)))
    c = int(p.x[71]); p.plant(71, q1=6, raw2=[4, 14, 6, 7][c], q2=40); expect.append((len(pairs), 71, (c, 6)))      # N, Y -> R, W, S: 4 + c behind COMP
    # U in read 2 is an A: agreement with an A of read 1, disagreement with a C
    p.plant(75, c1=0, q1=10, raw2=16, q2=15); expect.append((len(pairs), 75, (0, 25)))
    p.plant(76, c1=1, q1=10, raw2=16, q2=15); expect.append((len(pairs), 76, (0, 5)))
    p.plant(77, c1=16, q1=30, raw2=3, q2=15); expect.append((len(pairs), 77, (0, 15)))                         # a U of read 1 stays a U: no base
    pairs.append(p)
    # every code in a position that read 2 alone covers: a2 = 0 < a1 = 30
    p = perfect_pair(160, 30, 120, 0, 160, rng)
    for k, raw in enumerate(list(range(19)) + [255]):
        p.plant(k, raw2=raw, q2=k); expect.append((len(pairs), k, (comp(raw), k)))
    pairs.append(p)
    # ... and read 1 alone: z2 = 100 < z1 = 130, the code as it is
    p = perfect_pair(130, 0, 130, 30, 100, rng)
    for k, c in enumerate((0, 3, 4, 16, 18, 255)):
        p.plant(105 + k, c1=c, q1=200 + k); expect.append((len(pairs), 105 + k, (c, 200 + k)))
    pairs.append(p)
    return pairs, expect


def run_consensus(lib, sh):
    rng = np.random.default_rng(4200)
    pairs, expect = consensus_pairs(rng)
    assert [COMP[c] for c in range(19)] == [ALPHABET.index(ch) for ch in "TGCANYWSMKHBDVRXA.-"] and comp(255) == 255 and comp(19) == 19
    a1, a2, rg1, rg2, keep, insert = build(pairs)
    h = handle(lib)
    try:
        with staged(lib, h, a1, pad=1) as st1, staged(lib, h, a2, pad=0) as st2:
            for cap in (41, 0, 255):
                rules = rules_of(30, 2000, 1000, cap)
                w = merge_model(a1, a2, rules, rg1, rg2, keep, insert)
                assert all(y == 0 for y in w.why) and all(v > 0 for v in w.stats[:7]), w.stats
                if cap == 41:                                # the model alone gives what was written down by hand
                    for r, P, (c, q) in expect:
                        bases, quals = w.read(r)
                        p = P - min(pairs[r].geo()[0], pairs[r].geo()[2])
                        assert (bases[p], quals[p]) == (c, q), (r, P, bases[p], quals[p], c, q)
                else:                                        # ... and the cap moves the sums only: 10 + 20 under a cap of 0 is 20, under 255 it is 30
                    p = 25 - 0
                    assert w.read(4)[1][p] == (20 if cap == 0 else 30) and w.read(4)[1][27] == (30 if cap == 0 else 60) and w.read(4)[1][31] == 255
                check_merge(lib, h, st1, st2, rules, rg1, rg2, keep, insert, pad=(1, 0), what=("consensus", cap), model=w)
    finally:
        h.close()


# ---- reasons -------------------------------------------------------------------------------------------------------------------------
def spoil(p, count):
    """`count` mismatches in the overlap: positions 0, V - 1, 63, 64 of it first, then from the middle."""
    lo, hi = p.overlap()
    for i in cp.mismatch_positions(hi - lo, count):
        p.plant(lo + i, raw2=3 - (int(p.x[lo + i]) + 1 + i % 3) % 4)
    return p


def reason_pairs(rng, min_overlap=30):
    """-> pairs, [the reason each must count in (0 = merged)]."""
    pairs, want = [], []

    def add(p, y):
        pairs.append(p); want.append(y)
    good = lambda keep=1: perfect_pair(170, 0, 150, 0, 150, rng, keep=keep)
    add(good(), 0)
    add(good(keep=0), R_KEEP)
    p = good(); p.I = NO_INSERT; add(p, R_INSERT)
    p = good(keep=0); p.I = NO_INSERT; add(p, R_KEEP)                                    # 1 before 2
    add(raw_pair(100, (0, 0), 100, (0, 100), 100, rng, keep=0), R_KEEP)                  # 1 before 3
    add(raw_pair(100, (0, 0), 100, (0, 100), NO_INSERT, rng), R_INSERT)                  # 2 before 3
    for I in (2 ** 40, 2 ** 63, 2 ** 64 - 2):
        add(raw_pair(100, (0, 100), 100, (0, 100), I, rng), R_GEOMETRY)
    add(raw_pair(100, (2, 100), 100, (5, 100), 99, rng), R_GEOMETRY)                     # I = f2 + n2 - 1 (and f1 + n1 - 1 as well)
    add(raw_pair(100, (3, 90), 120, (5, 120), 119, rng), R_GEOMETRY)                     # I = f2 + n2 - 1 alone
    add(raw_pair(120, (3, 120), 100, (5, 90), 119, rng), R_GEOMETRY)                     # I = f1 + n1 - 1 alone
    add(raw_pair(100, (40, 40), 100, (0, 100), 100, rng), R_GEOMETRY)                    # n1 = 0: fails 3 and 4, counts in 3
    add(raw_pair(100, (0, 100), 100, (100, 100), 100, rng), R_GEOMETRY)                  # n2 = 0
    add(perfect_pair(300, 0, 150, 0, 150, rng), R_SHORT)                                 # abutting: V = 0
    add(perfect_pair(400, 0, 150, 0, 150, rng), R_SHORT)                                 # a gap: V = -100
    add(perfect_pair(300 - min_overlap, 0, 150, 0, 150, rng), 0)                         # V == min_overlap
    add(perfect_pair(300 - min_overlap + 1, 0, 150, 0, 150, rng), R_SHORT)               # V == min_overlap - 1
    add(spoil(perfect_pair(300 - min_overlap + 1, 0, 150, 0, 150, rng), min_overlap - 1), R_SHORT)      # fails 4 and 5, counts in 4
    add(spoil(good(), 5), 0)                                 # V = 130 at 5 / 200: exactly the budget
    add(spoil(good(), 6), R_BUDGET)
    p = good(); p.plant(90, c1=4); p.plant(91, raw2=4); p.plant(92, c1=7, raw2=7); add(p, 0)        # one-sided and neither: three mismatches
    return pairs, want


def run_reasons(lib, sh):
    rng = np.random.default_rng(4300)
    pairs, want = reason_pairs(rng)
    a1, a2, rg1, rg2, keep, insert = build(pairs)
    rules = rules_of(30, 5, 200, 41)
    w = merge_model(a1, a2, rules, rg1, rg2, keep, insert)
    assert w.why == want, (w.why, want)                      # the model alone: every pair counts where it was built to count
    assert all(v > 0 for v in w.stats), w.stats              # all twelve statistics in one call
    assert w.stats[3] + w.stats[4] + w.stats[5] + w.stats[6] == w.stats[2] and w.stats[0] + sum(w.stats[7:]) == len(pairs)
    assert [w.V[k] for k in range(14, 19)] == [0, -100, 30, 29, 29]
    h = handle(lib)
    try:
        with staged(lib, h, a1, pad=3) as st1, staged(lib, h, a2, pad=5) as st2:
            check_merge(lib, h, st1, st2, rules, rg1, rg2, keep, insert, pad=(3, 5), what="reasons", model=w)
            wn = check_merge(lib, h, st1, st2, rules, rg1, rg2, None, insert, pad=(3, 5), what="reasons, every pair kept")
            assert wn.stats[R_KEEP] == 0 and wn.why[1] == 0 and wn.why[3] == R_INSERT and wn.why[4] == R_GEOMETRY
    finally:
        h.close()


BUDGET_RATES = [0, 200, 1000]


def run_budget(lib, sh, rate):
    """Exactly min(max_mismatches, floor(V * rate / 1000)) mismatches merge, one more does not."""
    rng = np.random.default_rng(4400 + rate)
    h = handle(lib)
    try:
        for max_mm in (0, 5, 2000):
            pairs, want = [], []
            for I, n1, n2 in ((170, 150, 150), (205, 140, 130), (101, 100, 100), (1500, 1024, 1024)):
                V = n1 + n2 - I
                k = min(max_mm, V * rate // 1000)
                for count in (k, k + 1):
                    if count <= V:
                        pairs.append(spoil(perfect_pair(I, 0, n1, 0, n2, rng), count)); want.append(0 if count <= k else R_BUDGET)
            a1, a2, rg1, rg2, keep, insert = build(pairs)
            rules = rules_of(30, max_mm, rate, 41)
            w = merge_model(a1, a2, rules, rg1, rg2, keep, insert)
            assert w.why == want and 0 in want and (R_BUDGET in want or (rate == 1000 and max_mm == 2000)), (rate, max_mm, w.why, want)
            with staged(lib, h, a1) as st1, staged(lib, h, a2) as st2:
                check_merge(lib, h, st1, st2, rules, rg1, rg2, keep, insert, what=("budget", rate, max_mm), model=w)
    finally:
        h.close()


# ---- with the pair plan --------------------------------------------------------------------------------------------------------------
def with_qualities(a: Arrays, rng):
    return dataclasses.replace(a, quals=rng.integers(0, 42, len(a.bases)).astype(np.uint8))


def run_with_pair_plan(lib, sh, seed):
    n_pairs = sh["pair_fuzz"][1]
    a1, a2, plan1, plan2, pr = cp.fuzz_pairs(seed, n_pairs)
    rng = np.random.default_rng(5000 + seed)
    a1, a2 = with_qualities(a1, rng), with_qualities(a2, rng)
    pm = cp.pair_model(a1, a2, pr, plan1, plan2)
    rules = rules_of(pr["min_overlap"], pr["max_mm"], pr["rate"], 41)
    out1, out2, pkeep, insert = (pm[0], pm[1]), (pm[2], pm[3]), pm[4], pm[5]
    # the model alone: behind the pair plan's own ranges and rules every kept pair with an insert merges
    w = merge_model(a1, a2, rules, out1, out2, pkeep, insert)
    found = (pkeep != 0) & (insert != np.uint64(NO_INSERT))
    print("merge fuzz", seed, "pairs", n_pairs, "merged", w.stats[0], "stats", w.stats)
    assert np.array_equal(w.merged != 0, found) and w.stats[R_GEOMETRY] == w.stats[R_SHORT] == w.stats[R_BUDGET] == 0, w.stats
    assert 4 * w.stats[0] >= n_pairs and 4 * (n_pairs - w.stats[0]) >= n_pairs, w.stats      # (holds for the emulator's 120 pairs as well)
    # ... and with the plans that went INTO the pair plan, every pair kept: the pairs it narrowed are those the geometry refuses
    in1, in2 = (plan1[0], plan1[1]), (plan2[0], plan2[1])
    wi = merge_model(a1, a2, rules, in1, in2, None, insert, titles=False)
    assert wi.stats[R_GEOMETRY] == pm[6][6] and wi.stats[R_INSERT] == n_pairs - pm[6][5], (wi.stats, pm[6])
    h = handle(lib)
    try:
        with staged(lib, h, a1, pad=3) as st1, staged(lib, h, a2, pad=1) as st2:
            check_merge(lib, h, st1, st2, rules, out1, out2, pkeep, insert, pad=(3, 1), what=("pair plan out", seed), model=w)
            check_merge(lib, h, st1, st2, rules, in1, in2, None, insert, pad=(3, 1), what=("pair plan in", seed), model=wi, titles=False)
    finally:
        h.close()


# ---- capacities ------------------------------------------------------------------------------------------------------------------------
def small_set(rng, n_pairs=40):
    pairs = []
    for r in range(n_pairs):
        I = int(rng.integers(60, 320))
        n1, n2 = int(rng.integers(50, 151)), int(rng.integers(50, 151))
        p = perfect_pair(max(I, n1, n2), 0, n1, 0, n2, rng, tail1=r % 4, tail2=r % 3, keep=int(r % 9 != 4))
        if r % 7 == 3:
            p.I = NO_INSERT
        pairs.append(spoil(p, r % 5) if p.overlap()[1] - p.overlap()[0] > 40 else p)
    return pairs


def run_capacity(lib, sh):
    rng = np.random.default_rng(4500)
    a1, a2, rg1, rg2, keep, insert = build(small_set(rng))
    n = a1.n_records
    rules = rules_of(30, 5, 200, 41)
    w = merge_model(a1, a2, rules, rg1, rg2, keep, insert)
    K, S, T = w.totals
    assert 5 <= K < n and w.stats[R_KEEP] and w.stats[R_INSERT] and w.stats[R_SHORT]
    h = handle(lib)
    try:
        with staged(lib, h, a1) as st1, staged(lib, h, a2) as st2:
            call = lambda **kw: MergeCall(lib, h, st1.cols_in(), st2.cols_in(), n, lib_rules(lib, rules), rg1, rg2, keep, insert, K, S, T, **kw)
            c = call(caps=dict(bases_cap=0, quals_cap=0, titles_cap=0, records_cap=0))            # a sizing call writes nothing
            assert c.error is not None and c.error.code == E_CAPACITY and c.error.need == w.totals and c.error.stats == w.stats and c.untouched()
            for name, full in (("bases_cap", S), ("quals_cap", S), ("titles_cap", T), ("records_cap", K)):
                c = call(caps={name: full - 1})
                assert c.error is not None and c.error.code == E_CAPACITY and c.error.need == w.totals and c.untouched(), (name, c.error)
            c = call(titles=False, caps=dict(bases_cap=0, quals_cap=0, records_cap=0))
            assert c.error is not None and c.error.code == E_CAPACITY and c.error.need == [K, S, 0] and c.untouched()
            call().assert_equals(w, what="exact capacities")
            call(source=False).assert_equals(w, source=False, what="no d_source")
            wt = merge_model(a1, a2, rules, rg1, rg2, keep, insert, titles=False)
            assert wt.totals == [K, S, 0]
            check_merge(lib, h, st1, st2, rules, rg1, rg2, keep, insert, titles=False, titles_in2=False, what="no titles, in2 without titles", model=wt)
            check_merge(lib, h, st1, st2, rules, rg1, rg2, keep, insert, titles_in2=False, what="titles, in2 without titles", model=w)
            # nothing merged: totals 0, offs[0] = 0, d_merged all 0 -- with capacities of 0 as well
            none = np.zeros(n, np.uint8)
            w0 = merge_model(a1, a2, rules, rg1, rg2, none, insert)
            assert w0.totals == [0, 0, 0] and w0.stats[R_KEEP] == n and list(w0.seq_offs) == [0] and list(w0.title_offs) == [0]
            check_merge(lib, h, st1, st2, rules, rg1, rg2, none, insert, what="nothing merged", model=w0)
            w0 = check_merge(lib, h, st1, st2, rules_of(2000, 5, 200, 41), rg1, rg2, keep, insert, what="nothing merged: min_overlap 2000")
            assert w0.totals == [0, 0, 0]
            c = MergeCall(lib, h, st1.cols_in(3, 0), st2.cols_in(7, 0), 0, lib_rules(lib, rules), (None, None), (None, None), None,
                          np.zeros(1, np.uint64), 0, 0, 0)                                    # no pairs
            assert c.error is None and c.totals == [0, 0, 0] and c.stats == [0] * 12
            assert c.array("seq_offs", 1, np.uint64)[0] == 0 and c.array("title_offs", 1, np.uint64)[0] == 0 and c.untouched("bases", "quals", "titles")
    finally:
        h.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def run_arg_refusals(lib, sh):
    rng = np.random.default_rng(4600)
    a1, a2, rg1, rg2, keep, insert = build(small_set(rng, 24))
    n = a1.n_records
    good = rules_of(30, 5, 200, 41)
    w = merge_model(a1, a2, good, rg1, rg2, keep, insert)
    K, S, T = w.totals
    C = lib.C
    h = handle(lib)
    try:
        with staged(lib, h, a1) as st1, staged(lib, h, a2) as st2:
            call = lambda mr=None, cin1=None, cin2=None, rg1_=rg1, rg2_=rg2, **kw: MergeCall(
                lib, h, cin1 or st1.cols_in(), cin2 or st2.cols_in(), n, mr or lib_rules(lib, good), rg1_, rg2_, keep, insert, K, S, T, **kw)
            no_quals = lambda c: lib.ColumnsIn(c.d_bases, c.bases_len, None, c.d_titles, c.titles_len, c.d_seq_offs, c.d_title_offs, c.n_records)
            bad = [("min_overlap 0", dict(mr=lib_rules(lib, dict(good, min_overlap=0)))), ("permille 1001", dict(mr=lib_rules(lib, dict(good, rate=1001)))),
                   ("quality_cap 256", dict(mr=lib_rules(lib, dict(good, cap=256))))] + \
                  [("reserved[%d]" % k, dict(mr=lib_rules(lib, good, tuple(int(i == k) for i in range(4))))) for k in range(4)] + \
                  [("fewer records of read 2", dict(cin2=st2.cols_in(0, n - 1))), ("fewer records of read 1", dict(cin1=st1.cols_in(1, n - 1))),
                   ("begin 1 alone", dict(rg1_=(rg1[0], None))), ("end 1 alone", dict(rg1_=(None, rg1[1]))),
                   ("begin 2 alone", dict(rg2_=(rg2[0], None))), ("end 2 alone", dict(rg2_=(None, rg2[1]))),
                   ("no d_insert", dict(null=("insert",))), ("no d_merged", dict(null=("merged",))),
                   ("no d_quals 1", dict(cin1=no_quals(st1.cols_in()))), ("no d_quals 2", dict(cin2=no_quals(st2.cols_in())))]
            for name, kw in bad:
                c = call(**kw)
                assert c.error is not None and c.error.code == E_ARG and c.untouched(), (name, c.error)
            assert len(bad) == 17
            # rules, totals, stats, out NULL: through the C ABI itself
            with Dev(h) as d:
                ins, mg = d.up(insert.tobytes()), d.fill(n)
                out = lib.Columns()
                tot, sta = (C.c_uint64 * 3)(), (C.c_uint64 * 12)()
                c1, c2, mr = st1.cols_in(), st2.cols_in(), lib_rules(lib, good)
                P = lambda v: C.c_void_p(v)
                for k in range(4):
                    args = [C.byref(mr), C.byref(out), tot, sta]
                    args[k] = None
                    rc = h.L.dsrcgpu_columns_merge_device(h.h, C.byref(c1), C.byref(c2), args[0], P(None), P(None), P(None), P(None), P(None), P(ins),
                                                          args[1], P(mg), P(None), args[2], args[3])
                    assert rc == E_ARG, (k, rc)
                    assert d.down(mg, n) == b"\xA5" * (n + 8)
            call().assert_equals(w, what="the same handle, clean")
            big = rules_of(0xFFFFFFFF, 0xFFFFFFFF, 1000, 255)                                 # the largest figures: nothing overlaps that far
            assert check_merge(lib, h, st1, st2, big, rg1, rg2, keep, insert, what="the largest figures").totals == [0, 0, 0]
    finally:
        h.close()
    hc = ce.handle(lib, dataclasses.replace(Config.from_levels(0, 0), color_space=True))
    try:
        with staged(lib, hc, a1) as st1, staged(lib, hc, a2) as st2:
            c = MergeCall(lib, hc, st1.cols_in(), st2.cols_in(), n, lib_rules(lib, good), rg1, rg2, keep, insert, K, S, T)
            assert c.error is not None and c.error.code == E_ARG and c.untouched()
    finally:
        hc.close()


def run_input_errors(lib, sh):
    """The pair plan's seven input plants on side 1, on side 2 and on both (side 1 is the one reported), in the first, a middle and
    the last pair, kept and dropped ones: code, side, record, outputs still 0xA5, and the same handle merges the clean arrays
    afterwards."""
    rng = np.random.default_rng(4650)
    a1, a2, rg1, rg2, keep, insert = build(small_set(rng, 41))
    n = a1.n_records
    keep[[0, 20]] = 0
    pads = (4, 6)
    rules = rules_of(30, 5, 200, 41)
    w = merge_model(a1, a2, rules, rg1, rg2, keep, insert)
    K, S, T = w.totals
    A = (a1, a2)
    S_ = lambda s, r: int(A[s].seq_offsets[r]) + pads[s]
    rgs = lambda: [list(padded(rg1, pads[0])), list(padded(rg2, pads[1]))]
    h = handle(lib)
    checked = 0
    try:
        with staged(lib, h, a1, pad=pads[0]) as st1, staged(lib, h, a2, pad=pads[1]) as st2:
            st = (st1, st2)

            def refused(p, side, r, word, name):
                c = MergeCall(lib, h, st1.cols_in(), st2.cols_in(), n, lib_rules(lib, rules), tuple(p[0]), tuple(p[1]), keep, insert, K, S, T)
                assert c.error is not None and c.error.code == E_INPUT and c.untouched(), (name, side, r, c.error)
                msg = str(c.error)
                assert "read %d" % (side + 1) in msg and "record %d:" % r in msg and word in msg, (name, side, r, msg)
            offs = [("order", lambda s, r: st[s].poke("seq_offs", r + 1, S_(s, r) - 1, np.uint64), "not non-decreasing"),
                    ("end", lambda s, r: st[s].poke("seq_offs", r + 1, len(A[s].bases) + pads[s] + 5, np.uint64), "above bases_len"),
                    ("wild", lambda s, r: st[s].poke("seq_offs", r + 1, 2 ** 64 - 1, np.uint64), "above bases_len")]
            for name, plant, word in offs:
                for r in (0, 20, 40):
                    for sides in ((0,), (1,), (0, 1)):
                        for s in sides:
                            plant(s, r if s == sides[0] else 0)      # on both: side 2's plant sits in pair 0, side 1 is reported all the same
                        refused(rgs(), sides[0], r, word, name)
                        refused([[None, None], [None, None]], sides[0], r, word, name)
                        st1.restore(); st2.restore()
                        checked += 1
            ranges = [("begin low", lambda s, r: dict(b=S_(s, r) - 1), "d_begin lies below"),
                      ("end high", lambda s, r: dict(e=S_(s, r + 1) + 1), "d_end lies above"),
                      ("end wild", lambda s, r: dict(e=2 ** 64 - 1), "d_end lies above"),
                      ("begin above end", lambda s, r: dict(b=S_(s, r + 1), e=S_(s, r + 1) - 1), "d_begin lies above d_end")]
            for name, how, word in ranges:
                for r in (0, 20, 40):
                    for sides in ((0,), (1,), (0, 1)):
                        p = rgs()
                        for s in sides:
                            rr = r if s == sides[0] else 0
                            for key, v in how(s, rr).items():
                                p[s][0 if key == "b" else 1][rr] = v
                        refused(p, sides[0], r, word, name)
                        checked += 1
                check_merge(lib, h, st1, st2, rules, rg1, rg2, keep, insert, pad=pads, what=("after", name), model=w)
            # with titles wanted, read 1's title offsets are checked as the select checks them
            st1.poke("title_offs", 8, len(a1.titles) + pads[0] + 9, np.uint64)
            c = MergeCall(lib, h, st1.cols_in(), st2.cols_in(), n, lib_rules(lib, rules), padded(rg1, pads[0]), padded(rg2, pads[1]), keep, insert, K, S, T)
            assert c.error is not None and c.error.code == E_INPUT and c.untouched() and "read 1" in str(c.error), c.error
            st1.restore()
            check_merge(lib, h, st1, st2, rules, rg1, rg2, keep, insert, pad=pads, what="after the title plant", model=w)
    finally:
        h.close()
    assert checked == 63


def run_codec_state(lib, sh):
    """The call touches nothing the codec carries, as run_codec_state of the pair cases checks it: the fields capacity stays, a
    pending record layout stays pending, and the text call that follows writes what it writes on a fresh handle seeded alike."""
    from tests import columns_cases as cc
    from tests.cases import TINY
    a1, a2, rg1, rg2, keep, insert = build(small_set(np.random.default_rng(4660), 30))
    chunks = [TINY, cc.wave_boundary_chunk()]
    cfg = Config.from_levels(0, 0)
    for layout in (False, True):
        h, fresh = ce.handle(lib, cfg), ce.handle(lib, cfg)
        try:
            for x in (h, fresh):
                x.set_fields_capacity(11)
                if layout:
                    x.set_record_layout([len(c) for c in chunks])
            with staged(lib, h, a1) as st1, staged(lib, h, a2) as st2:
                check_merge(lib, h, st1, st2, rules_of(), rg1, rg2, keep, insert)
                assert h.get_fields_capacity() == 11
            assert (h.compress_batch(chunks), h.get_fields_capacity()) == (fresh.compress_batch(chunks), fresh.get_fields_capacity()), layout
        finally:
            h.close(); fresh.close()


# ---- counts --------------------------------------------------------------------------------------------------------------------------
def repeated(w: Want, base, n_pairs, titles):
    """The model of `base` pairs -> the model of n_pairs pairs in which the same pairs repeat (the first n_pairs % base once more)."""
    reps, rest = divmod(n_pairs, base)
    K = w.totals[0]
    k_rest = int((w.source < rest).sum())                    # the merged ones among the first `rest` pairs, and where their output ends
    s_rest = int(w.seq_offs[k_rest]); t_rest = int(w.title_offs[k_rest]) if titles else 0
    cat = np.concatenate
    rep_offs = lambda offs, end_rest: cat([offs[:-1] + np.uint64(i) * offs[-1] for i in range(reps)] + [offs[:k_rest] + np.uint64(reps) * offs[-1],
                                          np.array([np.uint64(reps) * offs[-1] + np.uint64(end_rest)], np.uint64)])
    rep_data = lambda data, end_rest: cat([data] * reps + [data[:end_rest]])
    return Want(rep_data(w.bases, s_rest), rep_data(w.quals, s_rest), rep_data(w.titles, t_rest) if titles else None, rep_offs(w.seq_offs, s_rest),
                rep_offs(w.title_offs, t_rest) if titles else None,
                cat([w.source + np.uint64(i * base) for i in range(reps)] + [w.source[:k_rest] + np.uint64(reps * base)]),
                cat([w.merged] * reps + [w.merged[:rest]]), [reps * K + k_rest, reps * w.totals[1] + s_rest, reps * w.totals[2] + t_rest], None, None, None)


def run_count(lib, sh, n_pairs):
    """n_pairs pairs of 10 + 10 bases at min_overlap 3.  The model runs on the first 2049 pairs at the most; behind them the same pairs
    repeat, and so do their results."""
    base = min(n_pairs, 2049)
    rng = np.random.default_rng(4700 + n_pairs)
    pairs = []
    for r in range(base):
        I = int(rng.integers(10, 21))
        p = perfect_pair(I, 0, 10, 0, 10, rng, keep=int(rng.random() < 0.9))
        if rng.random() < 0.15: p.I = NO_INSERT
        if rng.random() < 0.3: p.plant(int(rng.integers(I - 10, 10)) if I < 20 else 0, c1=int(rng.integers(0, 5)))
        pairs.append(p)
    a1, a2, rg1, rg2, keep, insert = build(pairs, title=lambda r: b"@t%d" % (r % 10))
    rules = rules_of(3, 1, 200, 41)
    wb = merge_model(a1, a2, rules, rg1, rg2, keep, insert)
    if base >= 2049:
        assert all(wb.stats[k] > 0 for k in (0, 3, 7, 8, 10, 11)), wb.stats
    reps, rest = divmod(n_pairs, base)
    if reps == 1 and rest == 0:
        w, b1, b2 = wb, a1, a2
    else:
        w = repeated(wb, base, n_pairs, True)
        part = merge_model(a1, a2, rules, (rg1[0][:rest], rg1[1][:rest]), (rg2[0][:rest], rg2[1][:rest]), keep[:rest], insert[:rest], n=rest).stats
        w.stats = [reps * u + v for u, v in zip(wb.stats, part)]
        idx = np.concatenate([np.arange(base)] * reps + [np.arange(rest)]).astype(np.int64)
        big = lambda a: Arrays(a.bases.reshape(base, 10)[idx].reshape(-1), a.quals.reshape(base, 10)[idx].reshape(-1),
                               np.concatenate([a.titles] * reps + [a.titles[:int(a.title_offsets[rest])]]),
                               (10 * np.arange(n_pairs + 1)).astype(np.uint64),
                               np.concatenate([a.title_offsets[:-1] + np.uint64(i) * a.title_offsets[-1] for i in range(reps)] +
                                              [a.title_offsets[:rest + 1] + np.uint64(reps) * a.title_offsets[-1]]), [0, n_pairs])
        b1, b2 = big(a1), big(a2)
        keep, insert = keep[idx], insert[idx]
        rg1 = rg2 = (None, None)                             # whole reads: the ranges are the records
    h = handle(lib)
    try:
        with staged(lib, h, b1) as st1, staged(lib, h, b2) as st2:
            check_merge(lib, h, st1, st2, rules, rg1, rg2, keep, insert, what=n_pairs, model=w)
    finally:
        h.close()


def run_second_pair_of_a_wave(lib, sh):
    """One grid stride behind eight pairs of 1024 + 1024 bases the same waves get short pairs.  Between the two, pairs of 1 + 1 bases
    without an insert size.  The model runs on the sixteen pairs and one filler; the fillers add to one statistic."""
    stride = sh["wave_stride"]
    rng = np.random.default_rng(4800)
    heads = [perfect_pair(1500 + k, 0, 1024, 0, 1024, rng) for k in range(8)]
    tails = [spoil(perfect_pair(90 + k, 0, 70, 0, 60 + k, rng), k % 3) for k in range(8)]
    filler = raw_pair(1, (0, 1), 1, (0, 1), NO_INSERT, rng)
    small = heads + [filler] + tails
    title = lambda r: b"@w"
    sa1, sa2, _, _, skeep, sins = build(small, title)
    rules = rules_of(30, 5, 200, 41)
    sw = merge_model(sa1, sa2, rules, (None, None), (None, None), None, sins)
    assert sw.why == [0] * 8 + [R_INSERT] + [0] * 8
    n_fill = stride - 8
    n = stride + 8
    idx = np.concatenate((np.arange(8), np.full(n_fill, 8), np.arange(9, 17)))

    def big(sa, recs, quals):
        lens = (sa.seq_offsets[1:] - sa.seq_offsets[:-1]).astype(np.int64)[idx]
        S = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
        cat = lambda sel, fill: np.concatenate([sel(p) for p in heads] + [np.full(n_fill, fill, np.uint8)] + [sel(p) for p in tails])
        return Arrays(cat(recs, 0), cat(quals, 30), np.frombuffer(b"@w" * n, np.uint8).copy(), S, (2 * np.arange(n + 1)).astype(np.uint64), [0, n])
    a1 = big(sa1, lambda p: p.x, lambda p: p.qx)
    a2 = big(sa2, lambda p: p.z, lambda p: p.qz)
    stats = list(sw.stats); stats[R_INSERT] += n_fill - 1
    src = np.where(sw.source < 8, sw.source, sw.source + np.uint64(n_fill - 1)).astype(np.uint64)
    w = Want(sw.bases, sw.quals, sw.titles, sw.seq_offs, sw.title_offs, src, sw.merged[idx], sw.totals, stats, None, None)
    h = handle(lib)
    try:
        with staged(lib, h, a1) as st1, staged(lib, h, a2) as st2:
            check_merge(lib, h, st1, st2, rules, (None, None), (None, None), None, sins[idx], what="second pair of a wave", model=w)
    finally:
        h.close()


# ---- the Python layers -----------------------------------------------------------------------------------------------------------------
class Never:                                                 # ValueError comes before any library call
    def __getattr__(self, name):
        raise AssertionError("the library was called")


def raises_value_error(call, what):
    try:
        call()
    except ValueError:
        return
    raise AssertionError("no ValueError for %r" % (what,))


def run_python_layers(lib, sh, device):
    from dsrc_amd import columns
    a1, a2, plan1, plan2, pr = cp.fuzz_pairs(11, 100)
    rng = np.random.default_rng(5100)
    a1, a2 = with_qualities(a1, rng), with_qualities(a2, rng)
    pm = cp.pair_model(a1, a2, pr, plan1, plan2)
    rules = rules_of(pr["min_overlap"], pr["max_mm"], pr["rate"], 37)
    kw = dict(min_overlap=rules["min_overlap"], max_mismatches=rules["max_mm"], max_error_permille=rules["rate"], quality_cap=37)
    t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v).astype(dt)).to(device)
    h = handle(lib)
    try:
        assert tuple(lib.MERGE_STATS) == MERGE_STATS
        c1, c2 = tensors(a1, device), tensors(a2, device)
        rg = [t(v.astype(np.int64), np.int64) for v in pm[:4]]
        keep, insert = t(pm[4], np.uint8), t(pm[5].astype(np.int64), np.int64)       # (2^64 - 1 as int64 is -1: as pair_plan returns it)
        w = merge_model(a1, a2, rules, (pm[0], pm[1]), (pm[2], pm[3]), pm[4], pm[5])
        assert 10 < w.totals[0] < 90

        def same(got, w, titles=True):
            out, flag, stats = got[:3]
            assert list(stats) == list(MERGE_STATS) and list(stats.values()) == w.stats, (stats, w.stats)
            assert flag.dtype == torch.uint8 and np.array_equal(flag.cpu().numpy(), w.merged)
            assert out.n_records == w.totals[0] and out.block_records.tolist() == [0, w.totals[0]] and out.seq_offsets.dtype == torch.int64
            pairs_ = [(out.bases, w.bases), (out.quals, w.quals), (out.seq_offsets, w.seq_offs)]
            pairs_ += [(out.titles, w.titles), (out.title_offsets, w.title_offs)] if titles else []
            assert all(np.array_equal(g.cpu().numpy().astype(v.dtype), v) for g, v in pairs_)
            assert titles or (out.titles.numel() == 0 and out.title_offsets.numel() == 0)
            assert out.bases.device.type == torch.device(device).type
        got = columns.merge_pairs(h, c1, c2, rg[0], rg[1], rg[2], rg[3], keep, insert, return_source=True, **kw)
        assert len(got) == 4 and got[3].dtype == torch.int64 and np.array_equal(got[3].cpu().numpy().astype(np.uint64), w.source)
        same(got, w)
        got = columns.merge_pairs(h, c1, c2, rg[0], rg[1], rg[2], rg[3], keep, insert=insert, titles=False, **kw)
        assert len(got) == 3
        same(got, merge_model(a1, a2, rules, (pm[0], pm[1]), (pm[2], pm[3]), pm[4], pm[5], titles=False), titles=False)
        m2 = cp.pair_model(a1, a2, pr)                       # whole reads, every pair: only the pairs the plan did not narrow pass the geometry
        same(columns.merge_pairs(h, c1, c2, insert=t(m2[5].astype(np.int64), np.int64), **kw), merge_model(a1, a2, rules, insert=m2[5]))
        fewer = tensors(ca.arrays_from_bases([np.zeros(5, np.uint8)]), device)
        args = (rg[0], rg[1], rg[2], rg[3], keep, insert)
        bad = [dict(min_overlap=0), dict(min_overlap=2 ** 32), dict(min_overlap=3.0), dict(max_mismatches=-1), dict(max_mismatches=2 ** 32),
               dict(max_error_permille=1001), dict(max_error_permille=-1), dict(quality_cap=256), dict(quality_cap=-1), dict(quality_cap=True)]
        for b in bad:
            raises_value_error(lambda: columns.merge_pairs(Never(), c1, c2, *args, **b), b)
        calls = [("begin 1 alone", lambda: columns.merge_pairs(Never(), c1, c2, rg[0], None, rg[2], rg[3], keep, insert)),
                 ("end 2 alone", lambda: columns.merge_pairs(Never(), c1, c2, rg[0], rg[1], None, rg[3], keep, insert)),
                 ("short begin", lambda: columns.merge_pairs(Never(), c1, c2, rg[0][:5], rg[1][:5], rg[2], rg[3], keep, insert)),
                 ("short keep", lambda: columns.merge_pairs(Never(), c1, c2, *rg, keep[:7], insert)),
                 ("short insert", lambda: columns.merge_pairs(Never(), c1, c2, *rg, keep, insert[:99])),
                 ("no insert", lambda: columns.merge_pairs(Never(), c1, c2, *rg, keep)),
                 ("unequal counts", lambda: columns.merge_pairs(Never(), c1, fewer, insert=insert)),
                 ("merge without overlap", lambda: columns.filter_pairs(Never(), c1, c2, overlap=False, merge=True)),
                 ("merge_quality_cap", lambda: columns.filter_pairs(Never(), c1, c2, merge=True, merge_quality_cap=256))]
        if torch.device(device).type != "cpu":
            calls.append(("two devices", lambda: columns.merge_pairs(Never(), c1, tensors(a2, "cpu"), insert=insert)))
            calls.append(("insert elsewhere", lambda: columns.merge_pairs(Never(), c1, c2, *rg, keep, insert.cpu())))
        for what, call in calls:
            raises_value_error(call, what)
    finally:
        h.close()


def pipeline_model(a1, a2, trim, adapters, pair_rules, cap, adapter_min_overlap=3, adapter_rate=100):
    """model quality plan -> model adapter plan per side -> pair_model -> merge_model -> the three outputs of filter_pairs(merge=True)
    as select_model / Want, the joint keep of the unmerged pairs, the stats dict."""
    plans, stats = [], {}
    for name, a, ads in (("read1", a1, adapters[0]), ("read2", a2, adapters[1])):
        b, e, k, ts = cs.plan_model(a, trim)
        side = dict(zip(ca.TRIM_STATS, ts))
        if ads is not None:
            ar = ca.rules_of([ca.codes_of(s) for s in ads], adapter_min_overlap, adapter_rate, trim["min_length"])
            b, e, k, _, as_ = ca.adapter_model(a, ar, b, e, k)
            side["adapter"] = dict(zip(ca.ADAPTER_STATS, as_))
        plans.append((b, e, k)); stats[name] = side
    pr = dict(pair_rules, min_length=trim["min_length"])
    b1, e1, b2, e2, keep, insert, ps = cp.pair_model(a1, a2, pr, plans[0], plans[1])
    stats["pair"] = dict(zip(cp.PAIR_STATS, ps))
    w = merge_model(a1, a2, rules_of(pr["min_overlap"], pr["max_mm"], pr["rate"], cap), (b1, e1), (b2, e2), keep, insert)
    stats["merge"] = dict(zip(MERGE_STATS, w.stats))
    rest = (keep & (1 - w.merged)).astype(np.uint8)
    return cs.select_model(a1, b1, e1, rest), cs.select_model(a2, b2, e2, rest), w, rest, (b1, e1, b2, e2), stats


def run_filter_pairs(lib, sh, device):
    from dsrc_amd import columns
    (a1, _, _), (a2, _, _) = cp.paired_reads(160)
    trim = cs.rules_of(0, 20, min_length=30, max_n=2)
    pr = cp.rules_of(20, 4, 150)
    same = lambda sel, want: all(np.array_equal(g.cpu().numpy().astype(v.dtype), v) for g, v in
                                 zip((sel.bases, sel.quals, sel.titles, sel.seq_offsets, sel.title_offsets), want[:5]))
    h = handle(lib)
    try:
        c1, c2 = tensors(a1, device), tensors(a2, device)
        for ads in ((None, None), ([cp.ADAPTER_STR[0]], [cp.ADAPTER_STR[1]])):
            w1, w2, w, rest, _, wstats = pipeline_model(a1, a2, trim, ads, pr, 41)
            ms = wstats["merge"]
            assert ms["pairs_merged"] >= 20 and int(rest.sum()) >= 20 and ms["pairs_merged"] + int(rest.sum()) == wstats["pair"]["pairs_kept"], (ms, wstats["pair"])
            kw = dict(adapters1=ads[0], adapters2=ads[1], pair_min_overlap=20, pair_max_mismatches=4, pair_max_error_permille=150, **trim)
            got = columns.filter_pairs(h, c1, c2, merge=True, **kw)
            assert len(got) == 4
            o1, o2, merged, stats = got
            assert stats == wstats and list(stats) == ["read1", "read2", "pair", "merge"], (stats, wstats)
            assert same(o1, w1) and same(o2, w2) and o1.n_records == o2.n_records == int(rest.sum())
            assert same(merged, (w.bases, w.quals, w.titles, w.seq_offs, w.title_offs)) and merged.n_records == ms["pairs_merged"]
            assert merged.n_records + o1.n_records == stats["pair"]["pairs_kept"]
            # merge=False: what it returned before, as three values
            r1, r2, keep, pstats = cp.pairs_model(a1, a2, trim, ads, True, pr)
            got = columns.filter_pairs(h, c1, c2, **kw)
            assert len(got) == 3 and got[2] == pstats and "merge" not in got[2]
            assert same(got[0], cs.select_model(a1, r1[0], r1[1], keep)) and same(got[1], cs.select_model(a2, r2[0], r2[1], keep))
            assert len(columns.filter_pairs(h, c1, c2, merge=False, merge_quality_cap=7, **kw)) == 3
        # profile=True keeps its meaning for out1 / out2: "after" is the profile of what comes out
        o1, o2, merged, stats = columns.filter_pairs(h, c1, c2, merge=True, profile=True, pair_min_overlap=20, pair_max_mismatches=4,
                                                     pair_max_error_permille=150, **trim)
        for out, name in ((o1, "read1"), (o2, "read2")):
            after = stats[name]["profile_after"].summary()
            assert after["records"] == out.n_records and after["bases"] == out.bases.numel()
        o1, o2, merged, _ = columns.filter_pairs(h, c1, c2, merge=True, titles=False, merge_quality_cap=0, **trim)
        assert merged.titles.numel() == 0 and o1.titles.numel() == 0 and o1.n_records == o2.n_records
    finally:
        h.close()


def run_closed_loop(lib, sh, device):
    """300 pairs written here -> the oracle's blocks of both files -> decode_columns -> filter_pairs(merge=True) -> encode_columns of
    all three outputs == the oracle's blocks of the model's text, lossless -d3 -q2 with CRC."""
    from dsrc_amd import columns
    cfg = ce.BLOCK_CFG
    (a1, recs1, text1), (a2, recs2, text2) = cp.paired_reads(300, seed=23)
    trim = cs.rules_of(0, 20, min_length=35)
    _, _, w, rest, (b1, e1, b2, e2), wstats = pipeline_model(a1, a2, trim, (None, None), cp.rules_of(), 41)
    print("closed loop: model stats", wstats)
    assert wstats["merge"]["pairs_merged"] >= 40 and int(rest.sum()) >= 40 and wstats["merge"]["overlap_corrected"] > 0
    text_of = lambda recs: b"\n".join(t + b"\n" + s + b"\n+\n" + q for t, s, q in recs)
    wants = []
    for a, recs, b, e in ((a1, recs1, b1, e1), (a2, recs2, b2, e2)):
        S = a.seq_offsets.astype(np.int64)
        wants.append(text_of([(t, s[int(b[r] - S[r]): int(e[r] - S[r])], q[int(b[r] - S[r]): int(e[r] - S[r])])
                              for r, (t, s, q) in enumerate(recs) if rest[r]]))
    so = w.seq_offs.astype(np.int64)
    assert int(w.bases.max()) <= 4 and int(w.quals.max()) <= 41
    wants.append(text_of([(recs1[int(r)][0], bytes(b"ACGTN"[v] for v in w.bases[so[j]: so[j + 1]]), bytes((w.quals[so[j]: so[j + 1]].astype(np.int64) + 33).astype(np.uint8)))
                          for j, r in enumerate(w.source)]))
    blocks = []
    for text in wants:
        want = ce.oracle_blocks(cfg, [text])
        assert want is not None
        blocks.append(want[0][0])
    h = ce.handle(lib, cfg)
    try:
        cols = []
        for text, recs in ((text1, recs1), (text2, recs2)):
            src = ce.oracle_blocks(cfg, [text])
            assert src is not None
            d_blocks, offs = cs._stage_blocks([src[0][0]], device)
            rc = columns.decode_columns(h, d_blocks, offs, [len(src[0][0])], device)
            assert rc.n_records == len(recs)
            cols.append(rc)
        o1, o2, merged, stats = columns.filter_pairs(h, cols[0], cols[1], merge=True, **trim)
        assert stats == wstats and o1.n_records == o2.n_records == int(rest.sum()) and merged.n_records == w.totals[0]
        for out, want in zip((o1, o2, merged), blocks):
            h.set_fields_capacity(0)
            got, o_offs, o_sizes, _ = columns.encode_columns(h, out, block_records=out.block_records)
            host = got.cpu().numpy().tobytes()
            assert [host[o: o + s] for o, s in zip(o_offs, o_sizes)] == [want]       # byte for byte, the CRC field included
    finally:
        h.close()
