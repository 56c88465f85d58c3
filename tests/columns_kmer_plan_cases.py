"""Shared by tests/test_emu_columns_kmer_plan.py (CPU, emulator build) and tests/test_gpu_columns_kmer_plan.py (MI355X): the cases of
the columnar k-mer plan (dsrcgpu_columns_kmer_plan; dsrc_amd/csrc/k_columns_kmer_plan.h) and what they must give.

The reference has no counterpart, so the yardstick is the integer model written out here: plan_model_serial() is the serial rule of
include/dsrc_gpu.h, window by window, over a Python dict of counts that comes from kmer_model / kmer_model_serial of
tests/columns_kmer_cases.py -- never from the library's table.  plan_model() is the same rule with the keys of a record's windows
taken from whole numpy arrays, for the large batches; test_the_two_models_agree holds the two against each other.  Every
comparison is exact equality.  The tables are built by the library's dsrcgpu_columns_kmer_count from reads the test chooses (and
checked against the dict there), outputs are filled with 0xA5 before a call so that "untouched" and "not a byte beyond" can be
asserted, and the table is compared byte for byte before and after every call: it is only read.  Before the library is compared on
a crafted case the model alone is asked what that case is for.

Shapes.  The emulator pays a coroutine switch per wave exchange, so its fuzz is 2 seeds x 150 records where the GPU runs 6 x 2000,
and the record count that takes the wave-per-record grid stride into a second round (4096 * 16 + 1001) runs on the GPU only."""
from __future__ import annotations

import dataclasses

import numpy as np
import torch        # noqa: F401  before the first handle (see columns_cases)

from tests import columns_cases as cc
from tests import columns_enc_cases as ce
from tests import columns_kmer_cases as ck
from tests import columns_pair_cases as cp
from tests import columns_sel_cases as cs
from tests._oracle import Config
from tests.cases import TINY

E_ARG, E_INPUT = cs.E_ARG, cs.E_INPUT
CAP = 65535
NO_LIMIT = 0xFFFFFFFF
GRID_CAP = ck.GRID_CAP

SHAPES = {
    "gpu": dict(ck.SHAPES["gpu"], plan_fuzz=(6, 2000)),
    "emu": dict(ck.SHAPES["emu"], plan_fuzz=(2, 150)),
}
Dev = cs.Dev
staged = ck.staged
handle = ck.handle
tensors = ck.tensors
arrays = ck.arrays
whole = ck.whole
KS = ck.KS
PLAN_STATS = ("records_considered", "records_came_dropped", "records_no_window", "windows", "windows_good", "hits", "records_kept", "records_with_hit",
              "records_trimmed", "bases_cut", "dropped_hits", "dropped_hit_share", "dropped_median", "dropped_length", "bases_kept")
DEFAULT = dict(min_count=1, min_hits=0, max_hits=None, min_hit_permille=0, max_hit_permille=1000, min_median=0, max_median=None, trim=0, min_length=0,
               want_median=0)


def rules_of(**kw):
    assert set(kw) <= set(DEFAULT)
    return dict(DEFAULT, **kw)


def lib_rules(lib, r, reserved=(0, 0, 0, 0)):
    return lib.KmerPlanRules(r["min_count"], r["min_hits"], r["max_hits"], r["min_hit_permille"], r["max_hit_permille"], r["min_median"], r["max_median"],
                             r["trim"], r["min_length"], r["want_median"], reserved)


# ---- the model -------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Plan:
    begin: np.ndarray
    end: np.ndarray
    keep: np.ndarray
    good: np.ndarray
    hits: np.ndarray
    median: np.ndarray
    stats: list


def judge(r, b, e, k, W, flags, C, stats):
    """The second half of the rule for one considered record: flags[p] = window p hits, C = the capped counts of its good windows
    -> (e', keep, hits, median); stats are added to."""
    hits = sum(flags)
    first_hit = flags.index(True) if hits else W
    first_miss = flags.index(False) if hits < W else W
    good = len(C)
    median = sorted(C)[good // 2] if r["want_median"] and good > 0 else 0
    e2 = e
    if r["trim"] == 1 and first_miss < W:
        e2 = b + first_miss + k - 1
    if r["trim"] == 2 and first_hit < W:
        e2 = b + first_hit
    stats[3] += W; stats[4] += good; stats[5] += hits
    if hits > 0:
        stats[7] += 1
    if e2 < e:
        stats[8] += 1; stats[9] += e - e2
    if not (r["min_hits"] <= hits and (r["max_hits"] is None or hits <= r["max_hits"])):
        reason = 10
    elif not (W * r["min_hit_permille"] <= hits * 1000 <= W * r["max_hit_permille"]):
        reason = 11
    elif r["want_median"] and not (r["min_median"] <= median and (r["max_median"] is None or median <= r["max_median"])):
        reason = 12
    elif not e2 - b >= r["min_length"]:
        reason = 13
    else:
        reason = 0
    if reason:
        stats[reason] += 1
    else:
        stats[6] += 1; stats[14] += e2 - b
    return e2, int(reason == 0), hits, median


def _plan(a, counts, k, canonical, r, begin, end, keep, first, n, windows):
    n = a.n_records - first if n is None else n
    b, e = ck.plan_of(a, begin, end, first, n)
    out = Plan(b.copy(), e.copy(), np.zeros(n, np.uint8), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), [0] * 16)
    stats = out.stats
    for i in range(n):
        if keep is not None and keep[i] == 0:
            stats[1] += 1
            continue
        stats[0] += 1
        bi, ei = int(b[i]), int(e[i])
        W = ei - bi - k + 1 if ei - bi >= k else 0
        if W == 0:
            stats[2] += 1
        flags, C = [], []
        for key in windows(bi, W):                         # None: a broken window
            if key is None:
                flags.append(False)
            else:
                c = counts.get(key, 0)
                C.append(min(c, CAP)); flags.append(c >= r["min_count"])
        out.end[i], out.keep[i], out.hits[i], out.median[i] = judge(r, bi, ei, k, W, flags, C, stats)
        out.good[i] = len(C)
    assert stats[0] == stats[6] + sum(stats[10:14]) and stats[3] >= stats[4] >= stats[5] and stats[0] + stats[1] == n
    return out


def plan_model_serial(a, counts, k, canonical, r, begin=None, end=None, keep=None, first=0, n=None):
    """The serial rule, window by window: codes above 3 break a window, the key is packed base by base."""
    def windows(at, W):
        for p in range(at, at + W):
            w = a.bases[p: p + k]
            yield None if (w > 3).any() else ck.key_of(w, canonical)
    return _plan(a, counts, k, canonical, r, begin, end, keep, first, n, windows)


def plan_model(a, counts, k, canonical, r, begin=None, end=None, keep=None, first=0, n=None):
    """plan_model_serial with the key of the window at every position of the arrays taken at once (for the batches too large for a
    loop per base)."""
    keys, broken = ck.window_keys(a.bases, k, canonical)

    def windows(at, W):
        return [None if br else key for key, br in zip(keys[at: at + W].tolist(), broken[at: at + W].tolist())]
    return _plan(a, counts, k, canonical, r, begin, end, keep, first, n, windows)


def mixed_batch(seed, n, pool=12, lo=0, hi=90, other=0.01, keep_share=0.9, known=0.6):
    """n reads pieced together from a pool of sequences (`known` of the pool is the reference), their reverse complements and random
    stretches, a few codes that are no bases, poly-G tails -> (arrays, reference arrays, begin, end, keep): hits, misses and broken
    windows mix inside a read."""
    rng = np.random.default_rng(7000 + seed)
    seqs = [rng.integers(0, 4, int(rng.integers(40, 120))).astype(np.uint8) for _ in range(pool)]
    n_known = max(1, int(pool * known))
    ref = arrays(seqs[: n_known] + seqs[: (n_known + 1) // 2])      # half of the reference twice: counts of 1 and of 2
    codes = np.array([4, 4, 255, 7, 16], np.uint8)
    reads = []
    for _ in range(n):
        parts, L = [], int(rng.integers(lo, hi + 1))
        while sum(len(p) for p in parts) < L:
            u = rng.random()
            s = seqs[int(rng.integers(0, pool))]
            at = int(rng.integers(0, len(s)))
            piece = s[at: at + int(rng.integers(5, 70))]
            parts.append(piece if u < 0.5 else cp.revcomp(piece) if u < 0.7 else rng.integers(0, 4, int(rng.integers(1, 30))).astype(np.uint8))
        x = (np.concatenate(parts) if parts else np.zeros(0, np.uint8))[:L].copy()
        amb = rng.random(len(x)) < other
        x[amb] = codes[rng.integers(0, 5, int(amb.sum()))]
        if rng.random() < 0.1 and len(x) > 20:
            x[len(x) - int(rng.integers(1, 20)):] = 2
        reads.append(x)
    a = arrays(reads)
    S0, S1 = whole(a)
    lens = S1 - S0
    cut5 = np.minimum(np.where(rng.random(n) < 0.6, 0, rng.integers(0, 6, n)), lens)
    cut3 = np.minimum(np.where(rng.random(n) < 0.6, 0, rng.integers(0, 6, n)), lens - cut5)
    keep = (rng.random(n) < keep_share).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
    return a, ref, S0 + cut5, S1 - cut3, keep


def run_models_agree():
    for seed, k, canonical, r in ((0, 1, 1, rules_of(want_median=1, trim=1)), (1, 2, 0, rules_of(trim=2, min_hits=3)), (2, 15, 1, rules_of(want_median=1, min_median=1, trim=1)),
                                  (3, 16, 0, rules_of(min_count=2, max_hit_permille=500)), (4, 17, 1, rules_of(want_median=1, max_median=2, min_length=30, trim=2)),
                                  (5, 31, 1, rules_of(want_median=1, min_hit_permille=300, trim=1, min_length=40)), (6, 5, 1, rules_of(min_count=3, want_median=1, max_hits=20))):
        a, ref, b, e, keep = mixed_batch(seed, 60)
        counts = ck.kmer_model_serial(ref, k, canonical)[0]
        ms, mv = plan_model_serial(a, counts, k, canonical, r, b, e, keep), plan_model(a, counts, k, canonical, r, b, e, keep)
        for f in dataclasses.fields(Plan):
            assert np.array_equal(getattr(ms, f.name), getattr(mv, f.name)), (seed, f.name)
        assert ms.stats[1] > 0 and ms.stats[5] > 0 and (k < 5 or ms.stats[4] > ms.stats[5]) and ms.stats[3] > ms.stats[4], (seed, ms.stats)
    # the rule itself on a case small enough to do by hand: k = 2, forward, the table holds AC x 2, CG x 1
    a = arrays([np.array([0, 1, 2, 3, 0, 1], np.uint8)])       # ACGTAC: windows AC CG GT TA AC
    counts = {ck.pack([0, 1]): 2, ck.pack([1, 2]): 1}
    m = plan_model_serial(a, counts, 2, 0, rules_of(want_median=1, trim=1))
    assert (m.end[0], m.keep[0], m.good[0], m.hits[0], m.median[0]) == (3, 1, 5, 3, 1) and m.stats == [1, 0, 0, 5, 5, 3, 1, 1, 1, 3, 0, 0, 0, 0, 3, 0]
    m = plan_model_serial(a, counts, 2, 0, rules_of(min_count=2, trim=2, want_median=1, min_length=1))       # the first window hits: nothing is left
    assert (m.end[0], m.keep[0], m.hits[0], m.median[0]) == (0, 0, 2, 1) and m.stats[13] == 1 and m.stats[9] == 6
    m = plan_model_serial(a, counts, 2, 0, rules_of(min_count=3, trim=1))                                      # the first window misses: k - 1 bases
    assert (m.end[0], m.keep[0], m.hits[0], m.median[0]) == (1, 1, 0, 0)


# ---- a call ------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Got:
    error: object
    stats: object
    begin: np.ndarray
    end: np.ndarray
    keep: np.ndarray
    good: object
    hits: object
    median: object
    untouched: bool


def plan_call(lib, h, d, cin, n, r, table, begin=None, end=None, keep=None, inplace=False, annotations=(True, True, True), reserved=(0, 0, 0, 0),
              force_median_array=False):
    """One dsrcgpu_columns_kmer_plan.  begin / end / keep: numpy in the coordinates of the staged arrays, or None.  inplace: the outputs
    are the very arrays of the inputs (where there is an input).  table: a device address (or None)."""
    up = lambda v, dt: None if v is None else d.up(np.ascontiguousarray(v).astype(dt).tobytes())
    pbi, pei, pki = up(begin, np.uint64), up(end, np.uint64), up(keep, np.uint8)
    pb = pbi if inplace and pbi is not None else d.fill(8 * n)
    pe = pei if inplace and pei is not None else d.fill(8 * n)
    pk = pki if inplace and pki is not None else d.fill(n)
    want = [annotations[0], annotations[1], annotations[2] and (bool(r["want_median"]) or force_median_array)]
    pa = [d.fill(8 * n) if w else None for w in want]
    err = stats = None
    try:
        stats = h.columns_kmer_plan(cin, lib_rules(lib, r, reserved), table, pbi, pei, pki, pb, pe, pk, *pa)
    except lib.DsrcGpuError as e:
        err = e
    raw = [d.down(pb, 8 * n), d.down(pe, 8 * n), d.down(pk, n)] + [None if p is None else d.down(p, 8 * n) for p in pa]
    assert all(x is None or x[-8:] == b"\xA5" * 8 for x in raw), "written behind the end of an output array"
    given = [np.ascontiguousarray(v).astype(dt).tobytes() if v is not None and inplace else None for v, dt in ((begin, np.uint64), (end, np.uint64), (keep, np.uint8))]
    untouched = all(x is None or (x[:-8] == g if g is not None else x == b"\xA5" * len(x)) for x, g in zip(raw, given + [None] * 3))
    arr = lambda x, dt: None if x is None else np.frombuffer(x[:-8], dt)
    return Got(err, stats, arr(raw[0], np.uint64), arr(raw[1], np.uint64), arr(raw[2], np.uint8), arr(raw[3], np.uint64), arr(raw[4], np.uint64),
               arr(raw[5], np.uint64), untouched)


def build_table(lib, h, d, ref, k, canonical=1, hash_bits=0, M=None):
    """The library's own count of the reads `ref` (arrays) into a table this test owns -> (Table, the model's dict of counts)."""
    m = ck.kmer_model(ref, k, canonical)
    M = ck.need_of(m[1][3]) if M is None else M
    tab = ck.Table(lib, d, M)
    with staged(lib, h, ref) as sr:
        got = ck.kmer_call(lib, h, d, sr.cols_in(), ck.lib_rules(lib, k, canonical, 0, hash_bits, M), tab)
    assert got.error is None and got.stats == m[1] and got.stats[7] == 0, (got.error, got.stats, m[1])
    return tab, m[0]


def check_plan(lib, h, d, st, tab, counts, k, canonical, r, begin=None, end=None, keep=None, pad=0, first=0, n=None, inplace=False, what=None, fast=True,
               model=None, annotations=(True, True, True)):
    """One call on records first .. first + n - 1 of the staged arrays == the model."""
    n = st.a.n_records - first if n is None else n
    m = model if model is not None else (plan_model if fast else plan_model_serial)(st.a, counts, k, canonical, r, begin, end, keep, first, n)
    shift = lambda v: None if v is None else np.asarray(v).astype(np.uint64) + np.uint64(pad)
    before = tab.raw().tobytes()
    got = plan_call(lib, h, d, st.cols_in(first, n), n, r, tab.p, shift(begin), shift(end), keep, inplace, annotations)
    assert got.error is None, (what, got.error)
    assert tab.raw().tobytes() == before, (what, "the table has been written")
    bad = np.nonzero((got.begin != m.begin.astype(np.uint64) + np.uint64(pad)) | (got.end != m.end.astype(np.uint64) + np.uint64(pad)) | (got.keep != m.keep))[0]
    assert len(bad) == 0, (what, r, "record", int(bad[0]), int(got.begin[bad[0]]) - pad, int(got.end[bad[0]]) - pad, int(got.keep[bad[0]]), "want",
                           int(m.begin[bad[0]]), int(m.end[bad[0]]), int(m.keep[bad[0]]))
    for name, g, w in (("good", got.good, m.good), ("hits", got.hits, m.hits), ("median", got.median, m.median)):
        if g is not None:
            bad = np.nonzero(g != w.astype(np.uint64))[0]
            assert len(bad) == 0, (what, r, name, "record", int(bad[0]), int(g[bad[0]]), "want", int(w[bad[0]]))
    assert got.median is not None or not (r["want_median"] and annotations[2])
    assert got.stats == m.stats, (what, r, got.stats, m.stats)
    s = got.stats
    assert s[0] == s[6] + s[10] + s[11] + s[12] + s[13] and s[3] >= s[4] >= s[5] and s[15] == 0
    return m


TRIMS = (0, 1, 2)


# ---- geometry --------------------------------------------------------------------------------------------------------------------
def geometry_reads(rng, k):
    """Per range length in 0, k - 1, k, k + 1 and the lengths of 63, 64, 65, 127, 128, 129 windows, per offset 0 .. 7 of the range in its
    stored read.  Even records are reference material; an odd record starts as the even record in front of it and goes on at random."""
    reads, offs, lens = [], [], []
    pos = 0
    for L in (0, k - 1, k, k + 1, 62 + k, 63 + k, 64 + k, 126 + k, 127 + k, 128 + k):
        for off in range(8):
            x = rng.integers(0, 4, off + L + 2).astype(np.uint8)
            if len(reads) % 2 and L:
                y, yo = reads[-1], offs[-1] - (pos - len(reads[-1]))
                half = min(L, lens[-1]) // 2
                x[off: off + half] = y[yo: yo + half]
            reads.append(x); offs.append(pos + off); lens.append(L)
            pos += len(x)
    a = arrays(reads)
    b = np.array(offs, np.int64)
    e = b + np.array(lens, np.int64)
    ref = arrays([a.bases[int(b[i]): int(e[i])] for i in range(0, len(reads), 2) if lens[i]])
    return a, ref, b, e


def run_geometry(lib, sh, k):
    rng = np.random.default_rng(100 + k)
    a, ref, b, e = geometry_reads(rng, k)
    assert a.n_records == 80 and {int(v - s) for v, s in zip(b, a.seq_offsets[:-1].astype(np.int64))} == set(range(8))
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=3) as st, Dev(h) as d:
            for canonical in (1, 0):
                tab, counts = build_table(lib, h, d, ref, k, canonical)
                for trim in TRIMS:
                    r = rules_of(trim=trim, want_median=1, min_hits=1 if trim == 1 else 0)
                    m = plan_model(a, counts, k, canonical, r, b, e)
                    assert m.stats[2] == 16 and m.stats[3] == 8 * (1 + 2 + 63 + 64 + 65 + 127 + 128 + 129) and m.stats[4] == m.stats[3]
                    if k >= 15:
                        assert 0 < m.stats[5] < m.stats[3] and (trim == 0 or m.stats[8] > 30)
                    check_plan(lib, h, d, st, tab, counts, k, canonical, r, b, e, pad=3, model=m, what=("geometry", k, canonical, trim))
                check_plan(lib, h, d, st, tab, counts, k, canonical, rules_of(trim=1), pad=3, what=("geometry, whole reads", k, canonical))
    finally:
        h.close()


# ---- positions ---------------------------------------------------------------------------------------------------------------------
def run_positions(lib, sh):
    """The first miss -- and separately the first hit -- at window 0, 62, 63, 64, 65, the last one and nowhere, under each trim."""
    rng = np.random.default_rng(200)
    k, W = 11, 130
    L = W + k - 1
    source = rng.integers(0, 4, L + 40).astype(np.uint8)
    ref = arrays([source])
    places = (0, 62, 63, 64, 65, W - 1, None)
    reads = []
    for p in places:                                         # every window hits up to the one that holds a changed base first
        x = source[7: 7 + L].copy()
        if p is not None:
            x[p + k - 1] = (x[p + k - 1] + 1) % 4
        reads.append(x)
    for p in places:                                         # no window hits but the one planted at p
        x = rng.integers(0, 4, L).astype(np.uint8)
        if p is not None:
            x[p: p + k] = source[20: 20 + k]
            if p > 0:
                x[p - 1] = (source[19] + 1) % 4             # ... and its neighbours do not go on as the source does
            if p + k < L:
                x[p + k] = (source[20 + k] + 1) % 4
        reads.append(x)
    a = arrays(reads)
    S0, S1 = whole(a)
    h = handle(lib)
    try:
        with staged(lib, h, a) as st, Dev(h) as d:
            tab, counts = build_table(lib, h, d, ref, k, 1)
            for trim in TRIMS:
                for min_length in (0, k):
                    r = rules_of(trim=trim, min_length=min_length, want_median=1)
                    m = plan_model_serial(a, counts, k, 1, r)
                    for i, p in enumerate(places):           # the model alone: the plants sit where they should
                        first_miss, first_hit = (W if p is None else p), (W if p is None else p)
                        want_miss = S0[i] + first_miss + k - 1 if trim == 1 and p is not None else S1[i]
                        want_hit = S0[7 + i] + first_hit if trim == 2 and p is not None else S1[7 + i]
                        if trim == 2:
                            want_miss = S0[i] + (k if p == 0 else 0)       # the first window hits, unless the changed base is in it: then window k is the first
                        if trim == 1:
                            want_hit = S0[7 + i] + (k - 1 if p != 0 else k)      # the first window misses, unless it is the planted one
                        assert m.end[i] == want_miss and m.end[7 + i] == want_hit, (trim, p, int(m.end[i]) - int(S0[i]), int(m.end[7 + i]) - int(S0[7 + i]))
                        assert m.hits[7 + i] == (0 if p is None else 1) and m.hits[i] == (W if p is None else W - min(k, W - p))
                    if trim == 1:
                        assert m.end[0] - S0[0] == k - 1 and m.keep[0] == (0 if min_length else 1)      # first_miss == 0 leaves k - 1 bases
                    check_plan(lib, h, d, st, tab, counts, k, 1, r, model=m, what=("positions", trim, min_length))
    finally:
        h.close()


# ---- broken windows ------------------------------------------------------------------------------------------------------------------
def run_broken(lib, sh):
    """Codes that are no bases: their windows are misses for trim = 1, no hits for trim = 2, and absent from the median."""
    rng = np.random.default_rng(300)
    h = handle(lib)
    try:
        for k in (2, 16, 31):
            L = 130 + k
            clean, reads, broken = [], [], []

            def add(places, code=4):
                x = rng.integers(0, 4, L).astype(np.uint8)
                clean.append(x.copy())
                x[list(places)] = code
                reads.append(x)
                hit = np.zeros(L - k + 1, bool)
                for p in places:
                    hit[max(0, p - k + 1): p + 1] = True
                broken.append(hit)
            for p in (0, L - 1, 63, 64, 63 + k - 1, 64 + k - 1, 127, 128):
                add([p])
            add(range(0, L)); add(range(60, 60 + 2 * k + 5), 255)
            for code in (4, 16, 255, 5, 18, 19):
                add([33, 90], code)
            a, ref = arrays(reads), arrays(clean)
            with staged(lib, h, a, pad=5) as st, Dev(h) as d:
                for canonical in (1, 0):
                    tab, counts = build_table(lib, h, d, ref, k, canonical)
                    for trim in TRIMS:
                        r = rules_of(trim=trim, want_median=1)
                        m = plan_model_serial(a, counts, k, canonical, r)
                        S0, S1 = whole(a)
                        for i, hit in enumerate(broken):     # the model alone: every good window hits, the broken ones are what the plant says
                            W = L - k + 1
                            assert m.good[i] == m.hits[i] == W - int(hit.sum()), (k, i)
                            first_miss = int(np.argmax(hit)) if hit.any() else W
                            first_hit = int(np.argmin(hit)) if not hit.all() else W
                            want = S0[i] + first_miss + k - 1 if trim == 1 and first_miss < W else S0[i] + first_hit if trim == 2 and first_hit < W else S1[i]
                            assert m.end[i] == want and (m.median[i] > 0) == (m.good[i] > 0), (k, trim, i)
                        assert m.good[8] == 0 and m.median[8] == 0 and m.end[8] == (S0[8] + k - 1 if trim == 1 else S1[8])      # the read of all N
                        check_plan(lib, h, d, st, tab, counts, k, canonical, r, pad=5, model=m, what=("broken", k, canonical, trim))
    finally:
        h.close()


# ---- median ------------------------------------------------------------------------------------------------------------------------
def run_median(lib, sh):
    """good odd and even, ties, all counts equal, good == 0; the bounds on the median."""
    rng = np.random.default_rng(400)
    k = 4
    unit = rng.integers(0, 4, 40).astype(np.uint8)
    ref = arrays([unit[:40], unit[:30], unit[:30], unit[:20], unit[5:15], unit[5:15], unit[5:15], np.full(30, 1, np.uint8), rng.integers(0, 4, 50).astype(np.uint8)])
    reads = [unit[:k + g - 1] for g in (1, 2, 3, 4, 5, 6, 7, 8, 20, 37)]                                   # good = 1 .. 8, 20, 37: odd and even
    reads += [np.full(17, 1, np.uint8), np.full(16, 1, np.uint8)]                                            # all counts equal
    reads += [np.full(12, 4, np.uint8), unit[:k - 1], np.zeros(0, np.uint8)]                                 # good == 0: all N, too short, empty
    reads += [np.concatenate((unit[:12], [4], unit[20:33])), rng.integers(0, 4, 30).astype(np.uint8)]        # a broken stretch in the middle; mostly absent keys
    reads += [np.concatenate((unit[3:3 + k], unit[3:3 + k]))]                                                # two windows twice over and junctions
    a = arrays(reads)
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=1) as st, Dev(h) as d:
            tab, counts = build_table(lib, h, d, ref, k, 0)
            assert len(set(counts.values())) >= 5
            m = plan_model_serial(a, counts, k, 0, rules_of(want_median=1))
            assert m.good[:10].tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 20, 37] and m.good[12:15].tolist() == [0, 0, 0] and m.median[12:15].tolist() == [0, 0, 0]
            assert m.median[10] == m.median[11] == counts[ck.pack([1] * k)] >= 27
            C2 = sorted(counts[ck.pack(unit[p: p + k])] for p in range(2))
            assert m.median[1] == C2[1]                                                                      # of two, the upper one
            assert len(set(m.median.tolist())) >= 4
            check_plan(lib, h, d, st, tab, counts, k, 0, rules_of(want_median=1), pad=1, model=m, what="median")
            # without it: d_median is not asked for, the rest is the same
            m0 = check_plan(lib, h, d, st, tab, counts, k, 0, rules_of(), pad=1, what="no median")
            assert np.array_equal(m0.hits, m.hits) and not m0.median.any()
            check_plan(lib, h, d, st, tab, counts, k, 0, rules_of(want_median=1), pad=1, model=m, annotations=(False, False, True), what="median alone")
            check_plan(lib, h, d, st, tab, counts, k, 0, rules_of(want_median=1), pad=1, model=m, annotations=(True, False, False), what="good alone")
            lo, hi = sorted(set(m.median.tolist()))[1], sorted(set(m.median.tolist()))[-2]
            for r in (rules_of(want_median=1, min_median=lo + 1), rules_of(want_median=1, max_median=hi - 1), rules_of(want_median=1, min_median=lo, max_median=hi),
                      rules_of(want_median=1, max_median=0), rules_of(want_median=1, min_median=CAP), rules_of(want_median=1, min_median=1, trim=1, min_length=6)):
                mm = check_plan(lib, h, d, st, tab, counts, k, 0, r, pad=1, fast=False, what=("median bounds", r))
                assert mm.stats[12] > 0 and mm.stats[10] == mm.stats[11] == 0
    finally:
        h.close()


def run_count_cap(lib, sh):
    """One key counted more than 65535 times: a single record of 70 000 A's, counted once.  d_median shows the cap; min_count sees the
    raw count.  Its 69 996 windows are also far more than a wave keeps on chip."""
    k, L = 5, 70000
    a = arrays([np.zeros(L, np.uint8), np.zeros(40, np.uint8), np.array([0] * 10 + [1] * 10, np.uint8)])
    raw = L - k + 1
    h = handle(lib)
    try:
        with staged(lib, h, a) as st, Dev(h) as d:
            tab, counts = build_table(lib, h, d, arrays([a.bases[:L]]), k, 0)
            assert counts == {0: raw} and raw > CAP
            for min_count, hit in ((1, True), (L - k, True), (raw, True), (raw + 1, False), (2 ** 63, False)):
                r = rules_of(min_count=min_count, want_median=1, trim=1)
                m = plan_model(a, counts, k, 0, r)
                assert m.median.tolist() == [CAP, CAP, 0] and m.hits.tolist() == ([raw, 36, 6] if hit else [0, 0, 0]) and m.good.tolist() == [raw, 36, 16]
                check_plan(lib, h, d, st, tab, counts, k, 0, r, model=m, what=("count cap", min_count))
            for r in (rules_of(want_median=1, min_median=CAP), rules_of(want_median=1, max_median=CAP - 1)):
                m = check_plan(lib, h, d, st, tab, counts, k, 0, r, what=("count cap, bound", r))
                assert m.keep.tolist() == ([1, 1, 0] if r["min_median"] else [0, 0, 1])
    finally:
        h.close()


# ---- the LDS boundary ------------------------------------------------------------------------------------------------------------------
def run_lds_boundary(lib, sh):
    """Records of KMER_PLAN_LDS_WINDOWS - 1, exactly that, + 1 and three times as many windows in one batch with short ones: the counts
    kept on chip and those kept in scratch give the same median.  Then the short ones alone: no scratch at all."""
    rng = np.random.default_rng(500)
    LW = lib.KMER_PLAN_LDS_WINDOWS
    assert LW == 1024
    k = 7
    pool = [rng.integers(0, 4, 300).astype(np.uint8) for _ in range(6)]
    ref = arrays(pool[:4] + [pool[0][:200], pool[1][:100], pool[1][:100]])

    def read(W):
        L, parts = W + k - 1, []
        while sum(len(p) for p in parts) < L:
            s = pool[int(rng.integers(0, 6))]
            at = int(rng.integers(0, 250))
            parts.append(s[at: at + int(rng.integers(20, 200))])
        x = np.concatenate(parts)[:L].copy()
        x[rng.random(L) < 0.003] = 4
        return x
    Ws = [10, LW - 1, 50, LW, 3, LW + 1, 100, 3 * LW, 64, LW - 1, 3 * LW, 1]
    a = arrays([read(W) for W in Ws])
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=2) as st, Dev(h) as d:
            tab, counts = build_table(lib, h, d, ref, k, 1)
            for r in (rules_of(want_median=1), rules_of(want_median=1, trim=1, min_count=2, min_median=2), rules_of(trim=2)):
                m = plan_model(a, counts, k, 1, r)
                assert (m.good <= np.array(Ws)).all() and m.stats[3] == sum(Ws) and 0 < m.stats[5] < m.stats[4] < m.stats[3]
                assert not r["want_median"] or len(set(m.median.tolist())) >= 2
                check_plan(lib, h, d, st, tab, counts, k, 1, r, pad=2, model=m, what=("lds boundary", r))
                short = np.array([int(W <= LW) for W in Ws], np.uint8)                                    # the long ones dropped: nothing needs scratch
                check_plan(lib, h, d, st, tab, counts, k, 1, r, keep=short, pad=2, what=("lds boundary, short ones", r))
                S0, S1 = whole(a)
                check_plan(lib, h, d, st, tab, counts, k, 1, r, S0, np.minimum(S1, S0 + LW + k - 1), pad=2, what=("lds boundary, ranges cut to it", r))
    finally:
        h.close()


# ---- strands ---------------------------------------------------------------------------------------------------------------------
def run_strands(lib, sh):
    """A forward table and a canonical one: reverse-complemented reads hit the canonical table and miss the forward one; palindromes."""
    rng = np.random.default_rng(600)
    h = handle(lib)
    try:
        for k in (4, 16, 30, 15, 31):
            x = rng.integers(0, 4, k + 70).astype(np.uint8)
            pals = []
            if k % 2 == 0:
                half = rng.integers(0, 4, k // 2).astype(np.uint8)
                pals = [np.concatenate((half, cp.revcomp(half)))]
                assert ck.revcomp_word(ck.pack(pals[0]), k) == ck.pack(pals[0])
            ref = arrays([x] + pals)
            a = arrays([x, cp.revcomp(x)] + pals + [np.concatenate((rng.integers(0, 4, 9).astype(np.uint8), p, rng.integers(0, 4, 9).astype(np.uint8))) for p in pals]
                       + [rng.integers(0, 4, k + 70).astype(np.uint8)])
            with staged(lib, h, a) as st, Dev(h) as d:
                tc, cc_ = build_table(lib, h, d, ref, k, 1)
                tf, cf = build_table(lib, h, d, ref, k, 0)
                for trim in TRIMS:
                    r = rules_of(trim=trim, want_median=1)
                    mc, mf = plan_model_serial(a, cc_, k, 1, r), plan_model_serial(a, cf, k, 0, r)
                    assert mc.hits[0] == mc.hits[1] == 71 and mf.hits[0] == 71
                    if k >= 15:
                        assert mf.hits[1] == 0 and mc.hits[-1] == 0
                    if pals:
                        assert mc.hits[2] == mf.hits[2] == 1 and mc.hits[3] >= 1 and mf.hits[3] >= 1
                    check_plan(lib, h, d, st, tc, cc_, k, 1, r, model=mc, what=("strands, canonical", k, trim))
                    check_plan(lib, h, d, st, tf, cf, k, 0, r, model=mf, what=("strands, forward", k, trim))
    finally:
        h.close()


# ---- hash_bits ---------------------------------------------------------------------------------------------------------------------
def run_hash_bits(lib, sh):
    """A table built with hash_bits = 4 (sixteen homes, long walks) gives the plan of the full hash: the query walks as the inserts did."""
    a, ref, b, e, keep = mixed_batch(11, 60, hi=120)
    k = 12
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=2) as st, Dev(h) as d:
            plans = []
            for bits in (4, 0, 1, 63):
                tab, counts = build_table(lib, h, d, ref, k, 1, hash_bits=bits, M=2048)
                assert 300 <= len(counts) <= 1000
                r = rules_of(trim=1, want_median=1, min_hits=2)
                m = check_plan(lib, h, d, st, tab, counts, k, 1, r, b, e, keep, pad=2, what=("hash_bits", bits))
                plans.append(m)
                assert 0 < m.stats[5] < m.stats[4]
            assert all(np.array_equal(p.end, plans[0].end) and p.stats == plans[0].stats for p in plans)
    finally:
        h.close()


# ---- plans in ------------------------------------------------------------------------------------------------------------------------
def run_plans_in(lib, sh):
    """Dropped records pass their range through with zero annotations; empty ranges; slices; the outputs in place of the inputs."""
    a, ref, b, e, keep = mixed_batch(21, 70, lo=10, keep_share=0.8)
    n, k = a.n_records, 6
    S0, S1 = whole(a)
    b[[3, 30]] = e[[3, 30]]                                    # empty ranges
    b[0] = S1[0]; e[0] = S1[0]                                 # ... one at the record's end
    e[5] = b[5] + min(5, e[5] - b[5])
    h = handle(lib)
    try:
        for pad in (0, 9):
            with staged(lib, h, a, pad=pad) as st, Dev(h) as d:
                tab, counts = build_table(lib, h, d, ref, k, 1)
                for r in (rules_of(trim=1, want_median=1, min_length=8), rules_of(trim=2, min_hits=1), rules_of(max_hits=0)):
                    m = plan_model(a, counts, k, 1, r, b, e, keep)
                    dropped = keep == 0
                    assert m.stats[1] == dropped.sum() > 5 and m.stats[2] >= 3 and m.stats[6] > 0 and m.stats[6] < m.stats[0]
                    assert np.array_equal(m.end[dropped], e[dropped]) and not m.keep[dropped].any() and not m.good[dropped].any() and not m.hits[dropped].any()
                    for inplace in (False, True):
                        check_plan(lib, h, d, st, tab, counts, k, 1, r, b, e, keep, pad=pad, model=m, inplace=inplace, what=("plan in", r, inplace))
                    check_plan(lib, h, d, st, tab, counts, k, 1, r, b, e, None, pad=pad, inplace=True, what=("ranges in place, no keep", r))
                    check_plan(lib, h, d, st, tab, counts, k, 1, r, None, None, keep, pad=pad, inplace=True, what=("keep in place, whole reads", r))
                    for first, cnt in ((2, None), (n - 1, 1), (3, 6)):
                        sl = slice(first, None if cnt is None else first + cnt)
                        check_plan(lib, h, d, st, tab, counts, k, 1, r, b[sl], e[sl], keep[sl], pad=pad, first=first, n=cnt, what=("first", first))
                    mz = check_plan(lib, h, d, st, tab, counts, k, 1, r, keep=np.zeros(n, np.uint8), pad=pad, what="nothing considered")
                    assert mz.stats == [0, n] + [0] * 14
                    me = check_plan(lib, h, d, st, tab, counts, k, 1, r, S0, S0, pad=pad, what="every range empty")
                    assert me.stats[2] == n and me.stats[3] == 0
                got = plan_call(lib, h, d, st.cols_in(4, 0), 0, rules_of(), tab.p)
                assert got.error is None and got.stats == [0] * 16 and got.untouched
    finally:
        h.close()


# ---- reasons -------------------------------------------------------------------------------------------------------------------------
def run_reasons(lib, sh):
    """Each of the four reasons alone; a record that fails several is counted under the first."""
    a, ref, b, e, keep = mixed_batch(31, 90, lo=0, hi=110)
    k = 9
    h = handle(lib)
    try:
        with staged(lib, h, a) as st, Dev(h) as d:
            tab, counts = build_table(lib, h, d, ref, k, 1)
            alone = {10: [rules_of(min_hits=5), rules_of(max_hits=10), rules_of(max_hits=0)], 11: [rules_of(min_hit_permille=400), rules_of(max_hit_permille=600)],
                     12: [rules_of(want_median=1, min_median=1), rules_of(want_median=1, max_median=0)], 13: [rules_of(min_length=30, trim=1), rules_of(min_length=30, trim=2)]}
            fails = {}
            for reason, sets in alone.items():
                for r in sets:
                    m = check_plan(lib, h, d, st, tab, counts, k, 1, r, b, e, keep, what=("reason", reason, r))
                    assert m.stats[reason] > 3 and sum(m.stats[10:14]) == m.stats[reason] and m.stats[6] > 3, (reason, r, m.stats)
                    fails.setdefault(reason, (keep != 0) & (m.keep == 0))
            r = rules_of(min_hits=5, min_hit_permille=400, want_median=1, min_median=1, min_length=30, trim=1)
            m = check_plan(lib, h, d, st, tab, counts, k, 1, r, b, e, keep, what="all four")
            assert (fails[10] & fails[11] & fails[12] & fails[13]).sum() > 0                                  # records that fail everything ...
            assert m.stats[10] == fails[10].sum() and m.stats[11] == (fails[11] & ~fails[10]).sum()           # ... are counted under the first
            assert m.stats[12] == (fails[12] & ~fails[11] & ~fails[10]).sum() and m.stats[13] == (fails[13] & ~fails[12] & ~fails[11] & ~fails[10]).sum()
            assert m.stats[11] > 0 and m.stats[13] > 0
    finally:
        h.close()


# ---- record counts -----------------------------------------------------------------------------------------------------------------
def run_count(lib, sh, n_records):
    a, ref, b, e, keep = mixed_batch(700 + n_records, n_records, pool=max(2, min(40, n_records // 3)), hi=40)
    h = handle(lib)
    try:
        with staged(lib, h, a) as st, Dev(h) as d:
            tab, counts = build_table(lib, h, d, ref, 5, 1)
            m = check_plan(lib, h, d, st, tab, counts, 5, 1, rules_of(trim=1, want_median=1, min_hits=1), b, e, keep, what=n_records)
            tab, counts = build_table(lib, h, d, ref, 11, 0)
            check_plan(lib, h, d, st, tab, counts, 11, 0, rules_of(trim=2), what=(n_records, "every record, forward"))
            if n_records >= 2049:
                assert m.stats[3] > 20000 and m.stats[1] > 100 and 0 < m.stats[5] < m.stats[4] < m.stats[3] and m.stats[10] > 0
    finally:
        h.close()


def run_grid_stride(lib, sh):
    n = sh["stride_count"]
    a, ref, b, e, keep = mixed_batch(900, n, pool=60, lo=6, hi=20, keep_share=0.95)
    r = rules_of(trim=1, want_median=1, min_hits=1)
    counts = ck.kmer_model(ref, 6, 1)[0]
    m = plan_model(a, counts, 6, 1, r, b, e, keep)
    second = slice(GRID_CAP * 16, None)
    assert m.keep[second].sum() > 300 and m.hits[second].sum() > 3000 and m.stats[3] > 300000       # the records of the second round count
    h = handle(lib)
    try:
        with staged(lib, h, a) as st, Dev(h) as d:
            tab, counts2 = build_table(lib, h, d, ref, 6, 1)
            assert counts2 == counts
            check_plan(lib, h, d, st, tab, counts, 6, 1, r, b, e, keep, model=m, what="grid stride")
    finally:
        h.close()


# ---- fuzz ------------------------------------------------------------------------------------------------------------------------
def run_fuzz(lib, sh, seed):
    """The reads of the k-mer count's fuzz (copies and reverse complements of earlier reads, codes that are no bases, poly-G tails,
    ranges, a keep) screened against the table of every third of them."""
    n = sh["plan_fuzz"][1]
    k = KS[seed % len(KS)] if seed % 2 else [21, 31, 11][seed // 2 % 3]
    canonical = 0 if seed % 3 == 2 else 1
    a, begin, end, keep = ck.fuzz_batch(100 + seed, n, k)
    S = a.seq_offsets.astype(np.int64)
    ref = arrays([a.bases[S[i]: S[i + 1]] for i in range(0, n, 3)])
    r = rules_of(trim=seed % 3, min_count=1 + seed % 2, want_median=1, min_hits=seed % 4, max_hit_permille=1000 - 100 * (seed % 3), min_median=seed % 2,
                 min_length=(20, 25, 60)[seed % 3])
    counts = ck.kmer_model(ref, k, canonical)[0]
    m = plan_model(a, counts, k, canonical, r, begin, end, keep)
    print("kmer plan fuzz", seed, "records", n, "k", k, "canonical", canonical, "rules", r, "stats", m.stats)
    assert m.stats[1] > 0 and m.stats[5] > 0 and m.stats[3] > m.stats[4] and m.stats[6] < m.stats[0]
    assert k < 11 or (m.stats[4] > m.stats[5] and m.stats[2] > 0 and m.stats[6] > 0)      # the model alone: hits, misses, broken windows, both verdicts
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=3) as st, Dev(h) as d:
            tab, counts2 = build_table(lib, h, d, ref, k, canonical)
            assert counts2 == counts
            check_plan(lib, h, d, st, tab, counts, k, canonical, r, begin, end, keep, pad=3, model=m, what=("fuzz", seed))
            check_plan(lib, h, d, st, tab, counts, k, canonical, rules_of(trim=(seed + 1) % 3, max_hits=seed), pad=3, what=("fuzz, whole reads, no median", seed))
    finally:
        h.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def run_arg_refusals(lib, sh):
    a, ref, b, e, keep = mixed_batch(41, 40)
    n, k = a.n_records, 7
    S0, S1 = whole(a)
    u64 = lambda v: np.asarray(v).astype(np.uint64)
    h = handle(lib)
    try:
        with staged(lib, h, a) as st, Dev(h) as d:
            cin = st.cols_in()
            tab, counts = build_table(lib, h, d, ref, k, 1)
            before = tab.raw().tobytes()
            checked = 0

            def refused(got, name):
                assert got.error is not None and got.error.code == E_ARG and got.untouched, (name, got.error)
                assert tab.raw().tobytes() == before
                return 1
            for name, r in [("min_count 0", rules_of(min_count=0)), ("min permille 1001", rules_of(min_hit_permille=1001)), ("max permille 1001", rules_of(max_hit_permille=1001)),
                            ("trim 3", rules_of(trim=3)), ("want_median 2", rules_of(want_median=2)), ("min_median without want_median", rules_of(min_median=1)),
                            ("max_median without want_median", rules_of(max_median=5)), ("max_median 0 without want_median", rules_of(max_median=0))]:
                checked += refused(plan_call(lib, h, d, cin, n, r, tab.p), name)
            checked += refused(plan_call(lib, h, d, cin, n, rules_of(), tab.p, force_median_array=True), "d_median without want_median")
            for i in range(4):
                checked += refused(plan_call(lib, h, d, cin, n, rules_of(), tab.p, reserved=tuple(int(j == i) for j in range(4))), "reserved[%d]" % i)
            checked += refused(plan_call(lib, h, d, cin, n, rules_of(), tab.p, begin=u64(S0)), "begin alone")
            checked += refused(plan_call(lib, h, d, cin, n, rules_of(), tab.p, end=u64(S1)), "end alone")
            checked += refused(plan_call(lib, h, d, cin, n, rules_of(), None), "null table")
            raw = ck.Table(lib, d, 64)                            # 0xA5 all over: no table's header
            got = plan_call(lib, h, d, cin, n, rules_of(), raw.p)
            checked += refused(got, "no table")
            assert raw.untouched() and "not a k-mer table" in str(got.error)
            assert checked == 17
            # null outputs, rules, stats, in: straight through the C ABI
            C = lib.C
            stats = (C.c_uint64 * 16)()
            R = lib_rules(lib, rules_of())
            pb, pe, pk = d.fill(8 * n), d.fill(8 * n), d.fill(n)
            full = [C.byref(cin), C.byref(R), C.c_void_p(tab.p), None, None, None, C.c_void_p(pb), C.c_void_p(pe), C.c_void_p(pk), None, None, None, stats]
            for hole in (0, 1, 2, 6, 7, 8, 12):
                args = list(full); args[hole] = None
                assert h.L.dsrcgpu_columns_kmer_plan(h.h, *args) == E_ARG, hole
                assert all(d.down(p, sz) == b"\xA5" * (sz + 8) for p, sz in ((pb, 8 * n), (pe, 8 * n), (pk, n)))
            assert h.L.dsrcgpu_columns_kmer_plan(None, *full) == E_ARG
            assert h.L.dsrcgpu_columns_kmer_plan(h.h, *full) == 0 and list(stats)[0] == n      # the same arguments, whole: accepted
            # the limits themselves are accepted
            for r in (rules_of(min_hit_permille=1000, max_hit_permille=1000), rules_of(min_count=2 ** 64 - 1), rules_of(want_median=1, max_median=NO_LIMIT - 1),
                      rules_of(max_hits=NO_LIMIT - 1, min_hits=NO_LIMIT - 1, min_length=NO_LIMIT)):
                check_plan(lib, h, d, st, tab, counts, k, 1, r, what=("limits", r))
    finally:
        h.close()
    hc = ce.handle(lib, dataclasses.replace(Config.from_levels(0, 0), color_space=True))
    try:
        with staged(lib, hc, a) as st, Dev(hc) as d:
            tab = ck.Table(lib, d, 64)
            got = plan_call(lib, hc, d, st.cols_in(), n, rules_of(), tab.p)
            assert got.error is not None and got.error.code == E_ARG and got.untouched and "colour-space" in str(got.error)
    finally:
        hc.close()


def run_input_errors(lib, sh):
    """The plants of the adapter plan's input errors in the first, a middle and the last record, kept and dropped ones: code, the lowest
    record, the reason's text, outputs untouched, and the same handle plans the clean arrays afterwards."""
    a, ref, _, _, _ = mixed_batch(51, 41, lo=8)
    n, k, pad = a.n_records, 6, 4
    keep = np.ones(n, np.uint8); keep[[20, 40]] = 0
    S = lambda r: int(a.seq_offsets[r]) + pad
    S0, S1 = whole(a)
    hb, he = (S0 + pad).astype(np.uint64), (S1 + pad).astype(np.uint64)
    h = handle(lib)
    checked = 0
    try:
        with staged(lib, h, a, pad=pad) as st, Dev(h) as d:
            tab, counts = build_table(lib, h, d, ref, k, 1)
            before = tab.raw().tobytes()

            def refused(r, word, name, plan):
                for rules in (rules_of(trim=1), rules_of(want_median=1)):
                    for inplace in (False, True):
                        got = plan_call(lib, h, d, st.cols_in(), n, rules, tab.p, *plan, inplace=inplace)
                        assert got.error is not None and got.error.code == E_INPUT and got.untouched, (name, r, got.error)
                        assert "record %d:" % r in str(got.error) and word in str(got.error), (name, r, str(got.error))
                assert tab.raw().tobytes() == before
            offs = [("order", lambda r: st.poke("seq_offs", r + 1, S(r) - 1, np.uint64), "not non-decreasing"),
                    ("end", lambda r: st.poke("seq_offs", r + 1, len(a.bases) + pad + 5, np.uint64), "above bases_len"),
                    ("wild", lambda r: st.poke("seq_offs", r + 1, 2 ** 64 - 1, np.uint64), "above bases_len")]
            for name, plant, word in offs:
                for r in (0, 20, 40):
                    plant(r)
                    if r == 0:
                        plant(40)                            # two plants: the lowest record is the one named
                    for plan in ((None, None, None), (hb, he, keep)):
                        refused(r, word, name, plan)
                    st.restore()
                    checked += 1
                check_plan(lib, h, d, st, tab, counts, k, 1, rules_of(trim=1, want_median=1), keep=keep, pad=pad, what=("after", name))
            ranges = [("begin low", lambda r: dict(b=S(r) - 1), "d_begin lies below"),
                      ("end high", lambda r: dict(e=S(r + 1) + 1), "d_end lies above"),
                      ("end wild", lambda r: dict(e=2 ** 64 - 1), "d_end lies above"),
                      ("begin above end", lambda r: dict(b=S(r + 1), e=S(r + 1) - 1), "d_begin lies above d_end")]
            for name, how, word in ranges:
                for r in (0, 20, 40):
                    pb, pe = hb.copy(), he.copy()
                    for key, v in how(r).items():
                        (pb if key == "b" else pe)[r] = v
                    if r == 0:
                        pb[40] = S(40) - 1                   # a second plant further up
                    refused(r, word, name, (pb, pe, keep))
                    checked += 1
                check_plan(lib, h, d, st, tab, counts, k, 1, rules_of(trim=2), S0, S1, keep, pad=pad, what=("after", name))
    finally:
        h.close()
    assert checked == 21


def run_codec_state(lib, sh):
    """The call touches nothing the codec carries, as run_codec_state of the other planners: the fields capacity stays, a pending
    record layout stays pending, and the text call that follows writes what it writes on a fresh handle seeded alike."""
    a, ref, b, e, keep = mixed_batch(61, 60)
    chunks = [TINY, cc.wave_boundary_chunk()]
    cfg = Config.from_levels(0, 0)

    def text_blocks(h):
        return h.compress_batch(chunks), h.get_fields_capacity()
    for layout in (False, True):
        h, fresh = ce.handle(lib, cfg), ce.handle(lib, cfg)
        try:
            for x in (h, fresh):
                x.set_fields_capacity(11)
                if layout:
                    x.set_record_layout([len(c) for c in chunks])
            with staged(lib, h, a) as st, Dev(h) as d:
                tab, counts = build_table(lib, h, d, ref, 9, 1)
                check_plan(lib, h, d, st, tab, counts, 9, 1, rules_of(trim=1, want_median=1), b, e, keep)
                check_plan(lib, h, d, st, tab, counts, 9, 1, rules_of(max_hits=0))
                assert h.get_fields_capacity() == 11
            assert text_blocks(h) == text_blocks(fresh), layout
        finally:
            h.close(); fresh.close()


# ---- the Python layers and the closed loop ---------------------------------------------------------------------------------------------
CODES = "ACGTNRWSKMDVHBYXU.-"


def text_of(x):
    return "".join(CODES[v] if v < len(CODES) else "?" for v in x.tolist())


def lookup_hits(columns, h, tab, a, k, min_count, device):
    """What a user does today: every window unfolded and packed in torch, KmerTable.lookup, a reduction per read -> hits per record."""
    S = a.seq_offsets.astype(np.int64)
    bases = torch.from_numpy(a.bases.astype(np.int64)).to(device)
    wins, owner = [], []
    for r in range(a.n_records):
        if S[r + 1] - S[r] >= k:
            wins.append(bases[S[r]: S[r + 1]].unfold(0, k, 1))
            owner.append(torch.full((wins[-1].shape[0],), r, dtype=torch.int64, device=device))
    win, owner = torch.cat(wins), torch.cat(owner)
    ok = (win <= 3).all(1)
    words = (win * (4 ** torch.arange(k - 1, -1, -1, device=device, dtype=torch.int64))).sum(1)
    got = tab.lookup(h, torch.where(ok, words, torch.zeros_like(words)))
    hits = torch.zeros(a.n_records, dtype=torch.int64, device=device)
    hits.index_add_(0, owner, ((got >= min_count) & ok).to(torch.int64))
    return hits.tolist()


def run_python_layers(lib, sh, device):
    from dsrc_amd import columns
    a, ref, begin, end, keep = mixed_batch(71, 90, hi=120)
    n, k = a.n_records, 13
    t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v).astype(dt)).to(device)
    dev = torch.device(device).type
    S = ref.seq_offsets.astype(np.int64)
    h = handle(lib)
    try:
        assert tuple(lib.KMER_PLAN_STATS) == PLAN_STATS and lib.KMER_PLAN_TRIM == {"none": 0, "first_miss": 1, "first_hit": 2}
        assert lib.KMER_PLAN_LDS_WINDOWS == 1024 and lib.KMER_PLAN_COUNT_CAP == CAP
        # columns_from_sequences: either case, every letter of the alphabet, any other byte 255, empty strings, no strings
        seqs = [text_of(ref.bases[S[i]: S[i + 1]]) for i in range(ref.n_records)]
        rc = columns.columns_from_sequences([s.lower() if i % 2 else s for i, s in enumerate(seqs)], device)
        assert rc.bases.dtype == torch.uint8 and rc.bases.device.type == dev and np.array_equal(rc.bases.cpu().numpy(), ref.bases)
        assert np.array_equal(rc.seq_offsets.cpu().numpy(), S) and rc.seq_offsets.dtype == torch.int64 and rc.n_records == ref.n_records
        assert rc.quals.numel() == rc.bases.numel() and not rc.quals.any() and rc.titles.numel() == 0 and rc.title_offsets.numel() == 0 and rc.block_records.tolist() == [0, ref.n_records]
        odd = columns.columns_from_sequences([CODES, CODES.lower(), "", "A?z*\n", "€"], device)
        assert odd.bases.tolist() == list(range(19)) * 2 + [0, 255, 255, 255, 255, 255] and odd.seq_offsets.tolist() == [0, 19, 38, 38, 43, 44]
        none = columns.columns_from_sequences([], device)
        assert none.n_records == 0 and none.bases.numel() == 0 and none.seq_offsets.tolist() == [0]
        # the table of the reference, then the plan
        tab, _ = columns.count_kmers(h, rc, k)
        counts = ck.kmer_model(ref, k, 1)[0]
        assert ck.table_dict(tab) == counts
        before = tab.data.clone()
        c = tensors(a, device)
        tb, te, tk = t(begin, np.int64), t(end, np.int64), t(keep, np.uint8)
        got = columns.kmer_plan(h, c, tab, tb, te, tk, trim="first_miss", min_hits=1, min_length=20)
        m = plan_model(a, counts, k, 1, rules_of(trim=1, min_hits=1, min_length=20), begin, end, keep)
        assert len(got) == 4 and list(got[3]) == list(PLAN_STATS) and list(got[3].values()) == m.stats[:15]
        assert got[0].dtype == got[1].dtype == torch.int64 and got[2].dtype == torch.uint8 and all(x.device.type == dev for x in got[:3])
        assert got[0].tolist() == m.begin.tolist() and got[1].tolist() == m.end.tolist() and got[2].tolist() == m.keep.tolist()
        assert torch.equal(tk, t(keep, np.uint8)) and torch.equal(tb, t(begin, np.int64)) and torch.equal(te, t(end, np.int64))      # inputs as they were
        assert 0 < m.stats[6] < m.stats[0] and m.stats[8] > 0
        # the median only when asked for: by a bound, or by return_counts
        got = columns.kmer_plan(h, c, tab, trim="first_hit", max_median=0, return_counts=True)
        m = plan_model(a, counts, k, 1, rules_of(trim=2, want_median=1, max_median=0, min_length=1))
        assert len(got) == 7 and list(got[3].values()) == m.stats[:15] and all(x.dtype == torch.int64 and x.device.type == dev for x in got[4:])
        assert (got[1].tolist(), got[2].tolist(), got[4].tolist(), got[5].tolist(), got[6].tolist()) == (m.end.tolist(), m.keep.tolist(), m.good.tolist(), m.hits.tolist(), m.median.tolist())
        assert m.stats[12] > 0
        got = columns.kmer_plan(h, c, tab, min_median=1)
        assert list(got[3].values()) == plan_model(a, counts, k, 1, rules_of(want_median=1, min_median=1, min_length=1)).stats[:15]
        got = columns.kmer_plan(h, c, tab, max_hits=0, return_counts=True)
        m = plan_model(a, counts, k, 1, rules_of(max_hits=0, want_median=1, min_length=1))
        assert got[2].tolist() == m.keep.tolist() and got[5].tolist() == m.hits.tolist()
        # the cross-check through the existing API
        for min_count in (1, 2):
            hits = columns.kmer_plan(h, c, tab, min_count=min_count, return_counts=True)[5].tolist()
            assert hits == lookup_hits(columns, h, tab, a, k, min_count, device) and sum(hits) > 0, min_count
        assert torch.equal(tab.data, before)                 # the table is only read
        # no records
        e0 = columns.kmer_plan(h, none, tab, return_counts=True)
        assert all(x.numel() == 0 for x in e0[:3] + e0[4:]) and not any(e0[3].values())

        class Never:                                         # ValueError comes before any library call
            def __getattr__(self, name):
                raise AssertionError("the library was called")
        bad_calls = [dict(table=None), dict(table="table"), dict(table=tab.data), dict(begin=tb), dict(end=te), dict(begin=tb[:5], end=te[:5]), dict(keep=tk[:7]),
                     dict(min_count=0), dict(min_count=1.0), dict(min_count=True), dict(min_hits=-1), dict(max_hits=-1), dict(max_hits=2 ** 32), dict(min_hit_permille=1001),
                     dict(max_hit_permille=1001), dict(max_hit_permille=-1), dict(min_median=-1), dict(min_median=CAP + 1), dict(max_median=-1), dict(trim="left"), dict(trim=1),
                     dict(min_length=-1), dict(min_length=2 ** 32)]
        calls = [lambda bad=bad: columns.kmer_plan(Never(), c, **dict(dict(table=tab), **bad)) for bad in bad_calls]
        calls += [lambda: columns.columns_from_sequences("ACGT"), lambda: columns.columns_from_sequences([b"ACGT"]), lambda: columns.columns_from_sequences(5),
                  lambda: columns.filter_columns(Never(), c, screen=tab), lambda: columns.filter_columns(Never(), c, screen=dict(max_hits=0)),
                  lambda: columns.filter_columns(Never(), c, screen=dict(table=tab, hdist=1)), lambda: columns.filter_columns(Never(), c, screen=dict(table=tab, trim="x")),
                  lambda: columns.filter_pairs(Never(), c, c, screen=dict(table=tab, min_count=0)), lambda: columns.filter_pairs(Never(), c, c, screen=dict(table="t"))]
        if dev != "cpu":                                     # a table on another device
            calls.append(lambda: columns.kmer_plan(Never(), c, columns.KmerTable(tab.data.cpu(), k, True)))
        for i, call in enumerate(calls):
            try:
                call()
            except ValueError:
                pass
            else:
                raise AssertionError("no ValueError for call %d" % i)
    finally:
        h.close()


def same_tensors(x, y):
    return all(torch.equal(getattr(x, f.name), getattr(y, f.name)) for f in dataclasses.fields(x))


def run_filters(lib, sh, device):
    """filter_columns(screen=...) and filter_pairs(screen=...) against the same steps called by hand, and against the model.  The
    default leaves both functions as they are."""
    from dsrc_amd import columns
    from tests import columns_adapt_cases as ca
    from tests import columns_dedup_cases as cd
    (a1, _, _), (a2, _, _) = cd.duplicated_reads(120, 41, pairs=True)
    trim = cs.rules_of(0, 20, min_length=30, max_n=1)
    k = 15
    S = a1.seq_offsets.astype(np.int64)
    ref = arrays([a1.bases[S[i]: S[i] + 40] for i in range(0, 120, 7)])
    counts = ck.kmer_model(ref, k, 1)[0]
    h = handle(lib)
    try:
        c1, c2 = tensors(a1, device), tensors(a2, device)
        tab, _ = columns.count_kmers(h, columns.columns_from_sequences([text_of(ref.bases[int(s): int(e)]) for s, e in zip(*whole(ref))], device), k)
        assert ck.table_dict(tab) == counts
        plain, plain_stats = columns.filter_columns(h, c1, **trim)
        again, again_stats = columns.filter_columns(h, c1, screen=None, **trim)
        assert plain_stats == again_stats and same_tensors(plain, again)
        b, e, kp, ts = cs.plan_model(a1, trim)
        for screen, r in ((dict(max_hits=0), rules_of(max_hits=0, min_length=30)), (dict(trim="first_hit", min_length=10), rules_of(trim=2, min_length=10)),
                          (dict(trim="first_miss", min_median=1), rules_of(trim=1, want_median=1, min_median=1, min_length=30))):
            m = plan_model(a1, counts, k, 1, r, b, e, kp)
            assert 0 < m.stats[6] < m.stats[0] and m.stats[1] > 0, m.stats
            out, stats = columns.filter_columns(h, c1, screen=dict(screen, table=tab), **trim)
            assert stats == dict(dict(zip(ca.TRIM_STATS, ts)), screen=dict(zip(PLAN_STATS, m.stats))) and list(stats)[-1] == "screen"
            assert cd.same_columns(out, cs.select_model(a1, m.begin, m.end, m.keep)) and out.n_records == m.stats[6]
            pb, pe, pk, _ = columns.trim_plan(h, c1, **trim)
            pb, pe, pk, ps = columns.kmer_plan(h, c1, tab, pb, pe, pk, **dict(dict(min_length=30), **screen))
            assert ps == stats["screen"] and same_tensors(out, columns.select_columns(h, c1, pb, pe, pk))
            # dedup, profile and kmers see the narrowed plan
            out, stats = columns.filter_columns(h, c1, screen=dict(screen, table=tab), dedup=True, profile=True, kmers=9, **trim)
            md = cd.dedup_model(a1, r1=(m.begin, m.end), keep=m.keep)
            assert list(stats)[-5:-3] == ["screen", "dedup"] and list(stats["dedup"].values()) == md[3] and cd.same_columns(out, cs.select_model(a1, m.begin, m.end, md[0]))
            assert stats["profile_after"].summary()["records"] == out.n_records and stats["profile_after"].summary()["bases"] == out.bases.numel()
            assert ck.table_dict(stats["kmers_after"]) == ck.kmer_model(a1, 9, 1, m.begin, m.end, md[0])[0]
        # pairs: per side in front of the pair plan, which makes it a decision per pair
        kw = dict(pair_min_overlap=20, pair_max_mismatches=4, pair_max_error_permille=150)
        p1, p2, pstats = columns.filter_pairs(h, c1, c2, **kw, **trim)
        q1, q2, qstats = columns.filter_pairs(h, c1, c2, screen=None, **kw, **trim)
        assert pstats == qstats and same_tensors(p1, q1) and same_tensors(p2, q2)
        screen = dict(table=tab, max_hits=0)
        for overlap in (True, False):
            o1, o2, ostats = columns.filter_pairs(h, c1, c2, screen=screen, overlap=overlap, **(kw if overlap else {}), **trim)
            sides = []
            for a, c in ((a1, c1), (a2, c2)):
                sb, se, sk, _ = cs.plan_model(a, trim)
                m = plan_model(a, counts, k, 1, rules_of(max_hits=0, min_length=30), sb, se, sk)
                hb, he, hk, _ = columns.trim_plan(h, c, **trim)
                hb, he, hk, hs = columns.kmer_plan(h, c, tab, hb, he, hk, max_hits=0, min_length=30)
                assert list(hs.values()) == m.stats[:15] and hk.tolist() == m.keep.tolist() and hb.tolist() == m.begin.tolist() and he.tolist() == m.end.tolist()
                sides.append((m, (hb, he, hk), hs))
            assert ostats["read1"]["screen"] == sides[0][2] and ostats["read2"]["screen"] == sides[1][2]
            assert sides[0][0].stats[10] > 0 and sides[1][0].stats[10] > 0 and sides[0][0].keep.tolist() != sides[1][0].keep.tolist()
            if overlap:
                b1, e1, b2, e2, keep, ps = columns.pair_plan(h, c1, c2, sides[0][1], sides[1][1], 20, 4, 150, 30)
                assert ostats["pair"] == ps
            else:
                (b1, e1, k1), (b2, e2, k2) = sides[0][1], sides[1][1]
                keep = k1 & k2
                assert "pair" not in ostats
            assert same_tensors(o1, columns.select_columns(h, c1, b1, e1, keep)) and same_tensors(o2, columns.select_columns(h, c2, b2, e2, keep))
            assert o1.n_records == o2.n_records == int(keep.sum()) and 0 < o1.n_records < p1.n_records
            assert not (keep.cpu().numpy().astype(bool) & ~(sides[0][0].keep & sides[1][0].keep).astype(bool)).any()      # a pair goes if either mate is screened out
    finally:
        h.close()


def run_closed_loop(lib, sh, device):
    """Records written here -> the oracle's block -> decode_columns -> the table of a reference -> filter_columns(screen=...) ->
    encode_columns -> decode_columns: the records that come back are the model's."""
    from dsrc_amd import columns
    from tests import columns_dedup_cases as cd
    cfg = ce.BLOCK_CFG
    (a, recs, text), = cd.duplicated_reads(150, 61)
    k = 17
    S = a.seq_offsets.astype(np.int64)
    contaminant = [text_of(a.bases[S[i]: S[i + 1]]) for i in (3, 50, 77, 120) if (a.bases[S[i]: S[i + 1]] <= 3).all()]
    assert len(contaminant) >= 2
    ref = arrays([np.array([CODES.index(ch) for ch in s], np.uint8) for s in contaminant])
    counts = ck.kmer_model(ref, k, 1)[0]
    trim = cs.rules_of(0, 20, min_length=35)
    b, e, kp, _ = cs.plan_model(a, trim)
    m = plan_model(a, counts, k, 1, rules_of(max_hits=0, min_length=35), b, e, kp)
    print("closed loop: model stats", m.stats)
    assert m.stats[10] > 0 and 0 < m.stats[6] < m.stats[0] < 150
    want = cs.select_model(a, m.begin, m.end, m.keep)
    src = ce.oracle_blocks(cfg, [text])
    assert src is not None
    h = ce.handle(lib, cfg)
    try:
        d_blocks, offs = cs._stage_blocks([src[0][0]], device)
        rc = columns.decode_columns(h, d_blocks, offs, [len(src[0][0])], device)
        assert rc.n_records == 150
        tab, _ = columns.count_kmers(h, columns.columns_from_sequences(contaminant, device), k)
        out, stats = columns.filter_columns(h, rc, screen=dict(table=tab, max_hits=0), **trim)
        assert list(stats["screen"].values()) == m.stats[:15] and cd.same_columns(out, want)
        h.set_fields_capacity(0)
        blocks, o_offs, o_sizes, _ = columns.encode_columns(h, out, block_records=out.block_records)
    finally:
        h.close()
    h = ce.handle(lib, cfg)
    try:
        back = columns.decode_columns(h, blocks, o_offs, o_sizes, device)
        assert back.n_records == m.stats[6] and cd.same_columns(back, want)
    finally:
        h.close()
