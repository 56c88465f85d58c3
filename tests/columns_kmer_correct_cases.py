"""Shared by tests/test_emu_columns_kmer_correct.py (CPU, emulator build) and tests/test_gpu_columns_kmer_correct.py (MI355X): the cases
of the columnar k-mer correction (dsrcgpu_columns_kmer_correct; dsrc_amd/csrc/k_columns_kmer_correct.h) and what they must give.

The reference has no counterpart, so the yardstick is the integer model written out here: correct_model_serial() is the serial rule
of include/dsrc_gpu.h, window by window, over a Python dict of counts that comes from kmer_model / kmer_model_serial of
tests/columns_kmer_cases.py -- never from the library's table.  correct_model() is the same rule with the keys of the windows taken
from whole numpy arrays (the solid flags of the batch at once, the candidates' windows through window_keys), for the large batches;
test_the_two_models_agree holds the two against each other.  Every comparison is exact equality.  The tables are built by the
library's dsrcgpu_columns_kmer_count from reads the test chooses (and checked against the dict there), outputs are filled with 0xA5
before a call so that "untouched" and "not a byte before or behind the span" can be asserted, and the table is compared byte for byte
before and after every call: it is only read.  Before the library is compared on a crafted case the model alone is asked what that
case is for.

Shapes.  The emulator pays a coroutine switch per wave exchange, so its fuzz is 2 seeds x 150 records where the GPU runs 6 x 2000,
and the record count that takes the wave-per-record grid stride into a second round (4096 * 16 + 1001) runs on the GPU only."""
from __future__ import annotations

import dataclasses

import numpy as np
import torch        # noqa: F401  before the first handle (see columns_cases)

from tests import columns_cases as cc
from tests import columns_enc_cases as ce
from tests import columns_kmer_cases as ck
from tests import columns_kmer_plan_cases as kp
from tests import columns_pair_cases as cp
from tests import columns_sel_cases as cs
from tests._oracle import Config
from tests.cases import TINY

E_ARG, E_INPUT = cs.E_ARG, cs.E_INPUT
GRID_CAP = ck.GRID_CAP

SHAPES = {
    "gpu": dict(ck.SHAPES["gpu"], correct_fuzz=(6, 2000)),
    "emu": dict(ck.SHAPES["emu"], correct_fuzz=(2, 150)),
}
Dev = cs.Dev
staged = ck.staged
handle = ck.handle
tensors = ck.tensors
arrays = ck.arrays
whole = ck.whole
build_table = kp.build_table
KS = ck.KS
CORRECT_STATS = ("records_considered", "records_came_dropped", "records_no_window", "windows", "windows_solid", "runs", "bases_fixed", "bases_fixed_n",
                 "records_fixed", "runs_whole_range", "runs_long", "runs_short_interior", "runs_no_candidate", "runs_ambiguous", "runs_quality",
                 "records_all_solid")


def rules_of(min_count=1, max_quality=255):
    return dict(min_count=min_count, max_quality=max_quality)


def lib_rules(lib, r, reserved=(0, 0, 0, 0, 0)):
    return lib.KmerCorrectRules(r["min_count"], r["max_quality"], reserved)


def with_quals(a, quals):
    return ce.Arrays(a.bases, np.asarray(quals, np.uint8), a.titles, a.seq_offsets, a.title_offsets, a.block_records)


# ---- the model -------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Corrected:
    bases: np.ndarray          # all of a.bases, the records of the call repaired
    fixed: np.ndarray
    stats: list


def runs_of(solid):
    """The maximal runs [w0, w1] of False in a list of flags, in order."""
    out, w0 = [], None
    for w, s in enumerate(solid):
        if not s and w0 is None:
            w0 = w
        if s and w0 is not None:
            out.append((w0, w - 1)); w0 = None
    if w0 is not None:
        out.append((w0, len(solid) - 1))
    return out


def resolve(x, quals, W, w0, w1, k, r, all_solid, stats):
    """One run of the range x (codes as they came) -> (p, the one base) or None; stats are added to.  all_solid(codes): every window of k
    of them is solid."""
    stats[5] += 1
    ln = w1 - w0 + 1
    if w0 == 0 and w1 == W - 1:
        stats[9] += 1; return None
    if ln > k:
        stats[10] += 1; return None
    if w0 == 0:
        p = w1
    elif w1 == W - 1:
        p = w0 + k - 1
    elif ln == k:
        p = w1
    else:
        stats[11] += 1; return None
    assert w0 <= p <= w1 + k - 1 and max(0, p - k + 1) >= w0 and min(p, W - 1) <= w1       # every window that contains p lies inside the run
    if r["max_quality"] < 255 and quals[p] > r["max_quality"]:
        stats[14] += 1; return None
    A = []
    for cand in range(4):
        if cand == x[p]:
            continue
        y = x[w0: w1 + k].copy()
        y[p - w0] = cand
        if all_solid(y):
            A.append(cand)
    if len(A) == 0:
        stats[12] += 1; return None
    if len(A) >= 2:
        stats[13] += 1; return None
    stats[6] += 1
    if x[p] > 3:
        stats[7] += 1
    return p, A[0]


def _correct(a, k, r, begin, end, keep, first, n, solid_flags, all_solid):
    n = a.n_records - first if n is None else n
    b, e = ck.plan_of(a, begin, end, first, n)
    out = Corrected(a.bases.copy(), np.zeros(n, np.int64), [0] * 16)
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
        solid = solid_flags(bi, W)
        stats[3] += W; stats[4] += sum(solid)
        if W > 0 and all(solid):
            stats[15] += 1
        x = a.bases[bi: ei]
        for w0, w1 in runs_of(solid):
            got = resolve(x, a.quals[bi: ei], W, w0, w1, k, r, all_solid, stats)
            if got is not None:
                out.bases[bi + got[0]] = got[1]; out.fixed[i] += 1
        if out.fixed[i]:
            stats[8] += 1
    assert stats[5] == stats[6] + sum(stats[9:15]) and stats[3] >= stats[4] and stats[0] + stats[1] == n and stats[6] == out.fixed.sum() >= stats[7]
    return out


def correct_model_serial(a, counts, k, canonical, r, begin=None, end=None, keep=None, first=0, n=None):
    """The serial rule, window by window: codes above 3 break a window, the key is packed base by base."""
    def is_solid(w):
        return bool((w <= 3).all()) and counts.get(ck.key_of(w, canonical), 0) >= r["min_count"]
    return _correct(a, k, r, begin, end, keep, first, n, lambda at, W: [is_solid(a.bases[p: p + k]) for p in range(at, at + W)],
                    lambda y: all(is_solid(y[j: j + k]) for j in range(len(y) - k + 1)))


def correct_model(a, counts, k, canonical, r, begin=None, end=None, keep=None, first=0, n=None):
    """correct_model_serial with the solid flag of the window at every position of the arrays taken at once (a sorted key array and a
    binary search instead of the dict), and the candidates' windows keyed through window_keys."""
    uk = np.array(sorted(counts), np.uint64)
    uc = np.array([counts[x] for x in uk.tolist()], np.uint64)

    def solid_of(bases):
        keys, broken = ck.window_keys(bases, k, canonical)
        if len(keys) == 0 or len(uk) == 0:
            return np.zeros(len(keys), bool)
        at = np.minimum(np.searchsorted(uk, keys), len(uk) - 1)
        return ~broken & (uk[at] == keys) & (uc[at] >= np.uint64(r["min_count"]))
    flags = solid_of(a.bases)

    return _correct(a, k, r, begin, end, keep, first, n, lambda at, W: flags[at: at + W].tolist(), lambda y: bool(solid_of(y).all()))


def hand_cases():
    """k = 3, forward words, the table of the one read ACGTTGCA (and, for the last case, of ACGTCGCA as well), min_count = 1 ->
    (reads, reference reads of the first table, those of the second, per read what the first table must give: (text, stats index))."""
    cases = [("ACGTAGCA", "ACGTTGCA", 6), ("TCGTTGCA", "ACGTTGCA", 6), ("AGGTTGCA", "ACGTTGCA", 6), ("ACGTTGCC", "ACGTTGCA", 6), ("ACGTNGCA", "ACGTTGCA", 6),
             ("ACNTTGCA", "ACGTTGCA", 6), ("ACGAAGCA", "ACGAAGCA", 10), ("TTT", "TTT", 9), ("AC", "AC", None), ("ACG", "ACG", None)]
    code = lambda s: np.array(["ACGTN".index(ch) for ch in s], np.uint8)
    return arrays([code(c[0]) for c in cases]), arrays([code("ACGTTGCA")]), arrays([code("ACGTTGCA"), code("ACGTCGCA")]), [(code(c[1]), c[2]) for c in cases]


def check_hand_model(a, counts1, counts2, want):
    S0, S1 = whole(a)
    for i, (text, why) in enumerate(want):
        one = arrays([a.bases[S0[i]: S1[i]]])
        m = correct_model_serial(one, counts1, 3, 0, rules_of())
        assert np.array_equal(m.bases, text), i
        assert m.stats[5] == (0 if why is None else 1) and (why is None or m.stats[why] == 1) and m.fixed[0] == (1 if why == 6 else 0), (i, m.stats)
        assert m.stats[7] == (1 if 4 in one.bases and why == 6 else 0)
        assert np.array_equal(correct_model(one, counts1, 3, 0, rules_of()).bases, text)
    m = correct_model_serial(arrays([a.bases[S0[0]: S1[0]]]), counts2, 3, 0, rules_of())
    assert np.array_equal(m.bases, a.bases[S0[0]: S1[0]]) and m.stats[13] == 1 and m.stats[5] == 1 and m.stats[6] == 0


def run_models_agree():
    a, ref1, ref2, want = hand_cases()
    check_hand_model(a, ck.kmer_model_serial(ref1, 3, 0)[0], ck.kmer_model_serial(ref2, 3, 0)[0], want)
    seen = [0] * 16
    for seed, k, canonical, r in ((0, 1, 1, rules_of(1)), (1, 2, 0, rules_of(2)), (2, 15, 1, rules_of(1, 30)), (3, 16, 0, rules_of(1)), (4, 17, 1, rules_of(2)),
                                  (5, 31, 1, rules_of(1, 35)), (6, 5, 1, rules_of(3, 20))):
        a, ref, b, e, keep = kp.mixed_batch(seed, 60)
        a = with_quals(a, np.random.default_rng(seed).integers(0, 42, len(a.bases)))
        counts = ck.kmer_model_serial(ref, k, canonical)[0]
        ms, mv = correct_model_serial(a, counts, k, canonical, r, b, e, keep), correct_model(a, counts, k, canonical, r, b, e, keep)
        assert np.array_equal(ms.bases, mv.bases) and np.array_equal(ms.fixed, mv.fixed) and ms.stats == mv.stats, (seed, ms.stats, mv.stats)
        assert ms.stats[1] > 0 and ms.stats[4] > 0 and (k < 5 or ms.stats[5] > 0), (seed, ms.stats)
        seen = [x + y for x, y in zip(seen, ms.stats)]
    assert seen[6] > 0 and seen[9] > 0 and seen[10] > 0 and seen[11] > 0, seen


# ---- a call ------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Got:
    error: object
    stats: object
    out: np.ndarray            # the whole output array (in place: the staged bases), the spare bytes behind it cut off
    fixed: object
    untouched: bool


def correct_call(lib, h, d, st, cin, n, r, table, begin=None, end=None, keep=None, inplace=False, fixed=True, reserved=(0, 0, 0, 0, 0)):
    """One dsrcgpu_columns_kmer_correct on the staged arrays.  begin / end / keep: numpy in the coordinates of the staged arrays, or None.
    Out of place the output is an array of its own, 0xA5-filled; in place it is the staged bases, which are put back afterwards."""
    up = lambda v, dt: None if v is None else d.up(np.ascontiguousarray(v).astype(dt).tobytes())
    size = len(st.host["bases"])
    po = st.ptr["bases"] if inplace else d.fill(size)
    pf = d.fill(8 * n) if fixed else None
    err = stats = None
    try:
        stats = h.columns_kmer_correct(cin, lib_rules(lib, r, reserved), table, up(begin, np.uint64), up(end, np.uint64), up(keep, np.uint8), po, pf)
    except lib.DsrcGpuError as e:
        err = e
    raw = d.down(po, size)
    rf = None if pf is None else d.down(pf, 8 * n)
    assert raw[-8:] == b"\xA5" * 8 and (rf is None or rf[-8:] == b"\xA5" * 8), "written behind the end of an output array"
    untouched = (raw[:-8] == st.host["bases"] if inplace else raw == b"\xA5" * len(raw)) and (rf is None or rf == b"\xA5" * len(rf))
    for name in ("quals", "seq_offs"):
        assert st.h.dev_download(st.ptr[name], len(st.host[name])) == st.host[name], "an input array has been written"
    if inplace:
        st.restore()
    else:
        assert st.h.dev_download(st.ptr["bases"], size) == st.host["bases"], "the input bases have been written"
    return Got(err, stats, np.frombuffer(raw[:-8], np.uint8), None if rf is None else np.frombuffer(rf[:-8], np.uint64), untouched)


def check_correct(lib, h, d, st, tab, counts, k, canonical, r, begin=None, end=None, keep=None, pad=0, first=0, n=None, inplace=False, what=None, fast=True,
                  model=None, fixed=True):
    """One call on records first .. first + n - 1 of the staged arrays == the model."""
    a = st.a
    n = a.n_records - first if n is None else n
    m = model if model is not None else (correct_model if fast else correct_model_serial)(a, counts, k, canonical, r, begin, end, keep, first, n)
    shift = lambda v: None if v is None else np.asarray(v).astype(np.uint64) + np.uint64(pad)
    before = tab.raw().tobytes()
    got = correct_call(lib, h, d, st, st.cols_in(first, n), n, r, tab.p, shift(begin), shift(end), keep, inplace, fixed)
    assert got.error is None, (what, got.error)
    assert tab.raw().tobytes() == before, (what, "the table has been written")
    lo, hi = int(a.seq_offsets[first]), int(a.seq_offsets[first + n])
    span = got.out[pad + lo: pad + hi]
    bad = np.nonzero(span != m.bases[lo: hi])[0]
    assert len(bad) == 0, (what, r, "position", int(bad[0]) + lo, int(span[bad[0]]), "want", int(m.bases[lo + bad[0]]), "came", int(a.bases[lo + bad[0]]), len(bad))
    if inplace:                                              # only repaired positions were written: the other records are as they came
        assert np.array_equal(got.out[pad: pad + lo], a.bases[:lo]) and np.array_equal(got.out[pad + hi:], a.bases[hi:]) and not got.out[:pad].any(), what
    else:                                                    # not a byte before or behind the span
        assert (got.out[: pad + lo] == 0xA5).all() and (got.out[pad + hi:] == 0xA5).all(), (what, "written outside the span")
    if fixed:
        bad = np.nonzero(got.fixed != m.fixed.astype(np.uint64))[0]
        assert len(bad) == 0, (what, r, "fixed, record", int(bad[0]), int(got.fixed[bad[0]]), "want", int(m.fixed[bad[0]]))
    assert got.stats == m.stats, (what, r, got.stats, m.stats)
    s = got.stats
    assert s[5] == s[6] + s[9] + s[10] + s[11] + s[12] + s[13] + s[14] and s[3] >= s[4]
    return m


def both_ways(lib, h, d, st, tab, counts, k, canonical, r, *args, **kw):
    m = check_correct(lib, h, d, st, tab, counts, k, canonical, r, *args, **kw)
    kw = dict(kw, model=m, inplace=True)
    check_correct(lib, h, d, st, tab, counts, k, canonical, r, *args, **kw)
    return m


def sub(x, p, rng=None, to=None):
    """x with another base at position p."""
    y = x.copy()
    y[p] = to if to is not None else (int(x[p]) + 1 + (int(rng.integers(0, 3)) if rng is not None else 0)) % 4
    return y


# ---- hand cases ----------------------------------------------------------------------------------------------------------------------
def run_hand(lib, sh):
    a, ref1, ref2, want = hand_cases()
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=1) as st, Dev(h) as d:
            tab1, counts1 = build_table(lib, h, d, ref1, 3, 0)
            tab2, counts2 = build_table(lib, h, d, ref2, 3, 0)
            check_hand_model(a, counts1, counts2, want)
            m = both_ways(lib, h, d, st, tab1, counts1, 3, 0, rules_of(), pad=1, fast=False, what="hand cases")
            assert np.array_equal(m.bases, np.concatenate([w[0] for w in want])) and m.stats[5:16] == [8, 6, 2, 6, 1, 1, 0, 0, 0, 0, 1] and m.stats[2] == 1
            m = both_ways(lib, h, d, st, tab2, counts2, 3, 0, rules_of(), pad=1, fast=False, what="hand cases, two candidates")
            assert m.fixed[0] == 0 and m.stats[13] >= 1
    finally:
        h.close()


# ---- placement -----------------------------------------------------------------------------------------------------------------------
def placement_reads(rng, k):
    L = 2 * k + 70
    source = rng.integers(0, 4, L + 20).astype(np.uint8)
    x = source[5: 5 + L]
    mid = L // 2
    single = sorted({p for p in (0, 1, k - 2, k - 1, k, mid, L - k - 1, L - k, L - 2, L - 1) if 0 <= p < L})
    reads = [sub(x, p) for p in single]
    double = [(mid, mid + dlt) for dlt in (k - 1, k, k + 1)]
    reads += [sub(sub(x, p), q) for p, q in double]
    # an interior run of k - 1: the first altered window of a substitution is made solid in the table
    short = sub(x, mid + 3)
    reads.append(short)
    extra = short[mid + 3 - k + 1: mid + 4].copy()
    # ranges of exactly k, k + 1 and 2 k bases, an error at their first, a middle and their last position, the range 3 bases into the read
    begin, end = [0] * len(reads), [L] * len(reads)
    for Lr in (k, k + 1, 2 * k):
        for p in sorted({0, Lr // 2, Lr - 1}):
            reads.append(sub(x, 3 + p)); begin.append(3); end.append(3 + Lr)
    a = arrays(reads)
    S0, _ = whole(a)
    return a, arrays([source, extra]), S0 + np.array(begin), S0 + np.array(end), single, len(single)


def run_placement(lib, sh, k):
    rng = np.random.default_rng(1100 + k)
    a, ref, b, e, single, n_single = placement_reads(rng, k)
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=2) as st, Dev(h) as d:
            for canonical in (1, 0):
                tab, counts = build_table(lib, h, d, ref, k, canonical)
                m = correct_model_serial(a, counts, k, canonical, rules_of(), b, e)
                if k >= 15:                                      # the model alone: what the plants are for
                    assert m.fixed[:n_single].tolist() == [1] * n_single                                      # every placement and its borders
                    assert m.fixed[n_single: n_single + 4].tolist() == [0, 0, 2, 0] and m.stats[10] == 2 and m.stats[11] == 1
                    assert m.fixed[n_single + 4:].tolist() == [0, 0, 0, 1, 0, 1, 1, 1, 1] and m.stats[9] == 4   # W = 1: whole; W = 2: the ends only
                    assert m.stats[12] == m.stats[13] == 0
                both_ways(lib, h, d, st, tab, counts, k, canonical, rules_of(), b, e, pad=2, model=m, what=("placement", k, canonical))
            both_ways(lib, h, d, st, tab, counts, k, 0, rules_of(), pad=2, what=("placement, whole reads", k))
    finally:
        h.close()


# ---- step borders --------------------------------------------------------------------------------------------------------------------
def run_step_borders(lib, sh):
    """k = 11, W = 130: a run's first or last window at 62, 63, 64, 65, 127 and 128 -- runs that open in one step and close in the next, a 3'
    run in the partial last step; W = 64 and 128: a 3' run that ends with bit 63 of the last step."""
    rng = np.random.default_rng(1200)
    k = 11
    source = rng.integers(0, 4, 200).astype(np.uint8)
    reads, want = [], []
    for W in (130, 128, 64):
        L = W + k - 1
        x = source[9: 9 + L]
        places = sorted({q for X in (62, 63, 64, 65, 127, 128) for q in (X, X + k - 1) if q < L} | {L - 1, L - 2})
        for q in places:
            reads.append(sub(x, q)); want.append(1)
        reads.append(sub(sub(x, 3), L - 1)); want.append(2)
    a = arrays(reads)
    h = handle(lib)
    try:
        with staged(lib, h, a) as st, Dev(h) as d:
            tab, counts = build_table(lib, h, d, arrays([source]), k, 1)
            m = correct_model_serial(a, counts, k, 1, rules_of())
            S0, S1 = whole(a)
            assert m.fixed.tolist() == want and all(np.array_equal(m.bases[s: t], source[9: 9 + t - s]) for s, t in zip(S0, S1))
            both_ways(lib, h, d, st, tab, counts, k, 1, rules_of(), model=m, what="step borders")
    finally:
        h.close()


# ---- Ns ------------------------------------------------------------------------------------------------------------------------------
def run_ns(lib, sh):
    rng = np.random.default_rng(1300)
    h = handle(lib)
    try:
        for k in (2, 16, 31):
            L = 2 * k + 80
            source = rng.integers(0, 4, L).astype(np.uint8)
            reads = [sub(source, p, to=code) for code in (4, 255, 5, 18, 19) for p in (0, k - 1, L // 2, L - k, L - 1)]
            n_one = len(reads)
            two = source.copy(); two[[0, 2]] = 4; reads.append(two)                  # an N at p = 2 and a second one under the run: no candidate
            two = source.copy(); two[[L - 3, L - 1]] = 4; reads.append(two)          # the same at the 3' end
            two = source.copy(); two[[L // 2, L // 2 + 3]] = 4; reads.append(two)    # two N, 3 apart, inside: a run longer than k
            reads.append(np.full(L, 4, np.uint8))                                   # all N: the whole range
            a = arrays(reads)
            with staged(lib, h, a, pad=5) as st, Dev(h) as d:
                for canonical in (1, 0):
                    tab, counts = build_table(lib, h, d, arrays([source]), k, canonical)
                    m = correct_model_serial(a, counts, k, canonical, rules_of())
                    if k >= 16:
                        assert m.fixed.tolist() == [1] * n_one + [0] * 4 and m.stats[7] == n_one and m.stats[12] == 2 and m.stats[10] == 1 and m.stats[9] == 1
                        assert all(np.array_equal(m.bases[i * L: (i + 1) * L], source) for i in range(n_one))
                    both_ways(lib, h, d, st, tab, counts, k, canonical, rules_of(), pad=5, model=m, what=("Ns", k, canonical))
    finally:
        h.close()


# ---- ambiguity, none, quality, min_count ---------------------------------------------------------------------------------------------
def run_verdicts(lib, sh):
    rng = np.random.default_rng(1400)
    k, L, at = 15, 90, 40
    source = rng.integers(0, 4, L).astype(np.uint8)
    true, other, came = int(source[at]), (int(source[at]) + 1) % 4, (int(source[at]) + 2) % 4
    variant = sub(source, at, to=other)
    read = sub(source, at, to=came)
    a = arrays([read, sub(source, 0), sub(source, L - 1), source])
    quals = np.full(len(a.bases), 30, np.uint8)
    quals[at] = 20; quals[L] = 7; quals[3 * L - 1] = 41
    a = with_quals(a, quals)
    # windows that do not hold position `at` are counted twice, those that hold it once
    ref_single = arrays([source, source[:at], source[at + 1:]])
    ref_two = arrays([source, variant])
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=3) as st, Dev(h) as d:
            tab, counts = build_table(lib, h, d, ref_two, k, 1)
            m = both_ways(lib, h, d, st, tab, counts, k, 1, rules_of(), pad=3, fast=False, what="two candidates")
            assert m.stats[13] == 1 and m.fixed.tolist() == [0, 1, 1, 0] and m.stats[15] == 1
            tab, counts = build_table(lib, h, d, ref_single, k, 1)
            assert counts[ck.key_of(source[at: at + k], 1)] == 1 and counts[ck.key_of(source[at + 1: at + 1 + k], 1)] == 2
            m = both_ways(lib, h, d, st, tab, counts, k, 1, rules_of(1), pad=3, fast=False, what="min_count at the candidate's count")
            assert m.fixed.tolist() == [1, 1, 1, 0] and m.bases[at] == true
            m = both_ways(lib, h, d, st, tab, counts, k, 1, rules_of(2), pad=3, fast=False, what="min_count one above")
            assert m.fixed[0] == 0 and m.stats[12] >= 1
            for max_quality in (19, 20, 21, 6, 7, 40, 41, 0, 254):       # just below, at and above the quality at each p
                m = both_ways(lib, h, d, st, tab, counts, k, 1, rules_of(1, max_quality), pad=3, fast=False, what=("max_quality", max_quality))
                assert m.fixed.tolist() == [int(max_quality >= 20), int(max_quality >= 7), int(max_quality >= 41), 0] and m.stats[14] == int(max_quality < 20) + int(max_quality < 7) + int(max_quality < 41), (max_quality, m.stats)
            # max_quality = 255: the qualities are not read and need not be there
            cin = st.cols_in()
            cin.d_quals = None
            want = correct_model_serial(a, counts, k, 1, rules_of())
            for inplace in (False, True):
                got = correct_call(lib, h, d, st, cin, 4, rules_of(), tab.p, inplace=inplace)
                assert got.error is None and got.stats == want.stats and np.array_equal(got.out[3: 3 + len(a.bases)], want.bases)
    finally:
        h.close()


# ---- strands, hash_bits ----------------------------------------------------------------------------------------------------------------
def run_strands(lib, sh):
    rng = np.random.default_rng(1500)
    h = handle(lib)
    try:
        for k in (16, 15, 31):
            x = rng.integers(0, 4, k + 90).astype(np.uint8)
            if k % 2 == 0:
                half = rng.integers(0, 4, k // 2).astype(np.uint8)
                x[40: 40 + k] = np.concatenate((half, cp.revcomp(half)))
                assert ck.revcomp_word(ck.pack(x[40: 40 + k]), k) == ck.pack(x[40: 40 + k])
            y = cp.revcomp(x)
            a = arrays([sub(x, 45), sub(y, 45), sub(y, 0), sub(y, len(y) - 1), sub(x, 40 + k), y])
            with staged(lib, h, a) as st, Dev(h) as d:
                tc, cc_ = build_table(lib, h, d, arrays([x]), k, 1)
                tf, cf = build_table(lib, h, d, arrays([x]), k, 0)
                mc, mf = correct_model_serial(a, cc_, k, 1, rules_of()), correct_model_serial(a, cf, k, 0, rules_of())
                assert mc.fixed.tolist() == [1, 1, 1, 1, 1, 0] and mf.fixed.tolist() == [1, 0, 0, 0, 1, 0] and (k % 2 == 0 or mf.stats[9] == 4) and mc.stats[15] == 1
                both_ways(lib, h, d, st, tc, cc_, k, 1, rules_of(), model=mc, what=("strands, canonical", k))
                both_ways(lib, h, d, st, tf, cf, k, 0, rules_of(), model=mf, what=("strands, forward", k))
    finally:
        h.close()


def error_batch(seed, n, k, genome=400, lo=0, hi=90, rate=0.02, keep_share=0.9, other=0.01, g=None):
    """n reads drawn from a random genome, both strands, with substitutions planted at `rate` and a few codes that are no bases ->
    (arrays with random qualities, the clean reads as reference arrays, begin, end, keep)."""
    rng = np.random.default_rng(9000 + seed)
    g = rng.integers(0, 4, genome).astype(np.uint8) if g is None else g
    genome = len(g)
    codes = np.array([4, 4, 255, 7, 16], np.uint8)
    reads, clean = [], []
    for _ in range(n):
        L = int(rng.integers(lo, hi + 1))
        at = int(rng.integers(0, max(1, genome - L)))
        x = g[at: at + L].copy()
        if rng.random() < 0.5:
            x = cp.revcomp(x)
        clean.append(x.copy())
        err = rng.random(len(x)) < rate
        x[err] = (x[err] + rng.integers(1, 4, int(err.sum()))) % 4
        amb = rng.random(len(x)) < other
        x[amb] = codes[rng.integers(0, 5, int(amb.sum()))]
        reads.append(x)
    a = arrays(reads)
    a = with_quals(a, rng.integers(0, 42, len(a.bases)))
    S0, S1 = whole(a)
    lens = S1 - S0
    cut5 = np.minimum(np.where(rng.random(n) < 0.6, 0, rng.integers(0, 8, n)), lens)
    cut3 = np.minimum(np.where(rng.random(n) < 0.6, 0, rng.integers(0, 6, n)), lens - cut5)
    keep = (rng.random(n) < keep_share).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
    return a, arrays(clean), S0 + cut5, S1 - cut3, keep


def run_hash_bits(lib, sh):
    a, ref, b, e, keep = error_batch(11, 24, 12, hi=80)
    k = 12
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=2) as st, Dev(h) as d:
            outs = []
            for bits in (4, 0, 63):
                tab, counts = build_table(lib, h, d, ref, k, 1, hash_bits=bits, M=2048)
                m = check_correct(lib, h, d, st, tab, counts, k, 1, rules_of(1, 35), b, e, keep, pad=2, what=("hash_bits", bits))
                assert 300 <= len(counts) <= 1000
                assert m.stats[6] > 3
                outs.append(m)
            assert all(np.array_equal(o.bases, outs[0].bases) and o.stats == outs[0].stats for o in outs)
    finally:
        h.close()


# ---- plans in ------------------------------------------------------------------------------------------------------------------------
def run_plans_in(lib, sh):
    """Dropped records are copied and have d_fixed 0; empty ranges; ranges that start 0 .. 7 bases into the stored read; a repair at the
    range's first and last position with the bytes outside the range unchanged; slices; a pad in front of the arrays; d_fixed absent."""
    rng = np.random.default_rng(1600)
    k = 9
    g = rng.integers(0, 4, 300).astype(np.uint8)
    reads, begin, end = [], [], []
    for off in range(8):                                       # errors at the first and the last position of the range, and outside it
        x = g[20 + off: 20 + off + 70].copy()
        for p in (0, off, off + 39, 69):
            x = sub(x, p)
        if off:
            x[off - 1] = 4
        reads.append(x); begin.append(off); end.append(off + 40)
    a0, _, b0, e0, keep0 = error_batch(21, 60, k, lo=10, hi=80, keep_share=0.8, g=g)
    S = a0.seq_offsets.astype(np.int64)
    more = [a0.bases[S[i]: S[i + 1]] for i in range(60)]
    a = arrays(reads + more)
    a = with_quals(a, rng.integers(0, 42, len(a.bases)))
    S0, S1 = whole(a)
    b = np.concatenate((S0[:8] + np.array(begin), b0 - S[:-1] + S0[8:]))
    e = np.concatenate((S0[:8] + np.array(end), e0 - S[:-1] + S0[8:]))
    keep = np.concatenate((np.ones(8, np.uint8), keep0))
    b[[11, 30]] = e[[11, 30]]
    b[9] = e[9] = S1[9]
    keep[[9, 11, 30]] = 1
    n = a.n_records
    h = handle(lib)
    try:
        for pad in (0, 9):
            with staged(lib, h, a, pad=pad) as st, Dev(h) as d:
                tab, counts = build_table(lib, h, d, arrays([g]), k, 1)
                for r in (rules_of(), rules_of(1, 25)):
                    m = correct_model(a, counts, k, 1, r, b, e, keep)
                    dropped = keep == 0
                    assert m.stats[1] == dropped.sum() > 5 and m.stats[2] >= 3 and not m.fixed[dropped].any() and m.stats[6] > 10
                    if r["max_quality"] == 255:
                        assert m.fixed[:8].tolist() == [2] * 8
                        for i in range(8):                           # the bytes outside the range are as they came, errors included
                            assert np.array_equal(m.bases[S0[i]: b[i]], a.bases[S0[i]: b[i]]) and np.array_equal(m.bases[e[i]: S1[i]], a.bases[e[i]: S1[i]])
                            assert np.array_equal(m.bases[b[i]: e[i]], g[20 + 2 * i: 60 + 2 * i])
                    both_ways(lib, h, d, st, tab, counts, k, 1, r, b, e, keep, pad=pad, model=m, what=("plan in", r, pad))
                    check_correct(lib, h, d, st, tab, counts, k, 1, r, b, e, None, pad=pad, what=("ranges, no keep", r))
                    check_correct(lib, h, d, st, tab, counts, k, 1, r, None, None, keep, pad=pad, inplace=True, fixed=False, what=("keep, whole reads, no d_fixed", r))
                    check_correct(lib, h, d, st, tab, counts, k, 1, r, b, e, keep, pad=pad, fixed=False, what=("no d_fixed", r))
                    for first, cnt in ((2, None), (n - 1, 1), (3, 6)):
                        sl = slice(first, None if cnt is None else first + cnt)
                        both_ways(lib, h, d, st, tab, counts, k, 1, r, b[sl], e[sl], keep[sl], pad=pad, first=first, n=cnt, what=("first", first))
                    mz = both_ways(lib, h, d, st, tab, counts, k, 1, r, keep=np.zeros(n, np.uint8), pad=pad, what="nothing considered")
                    assert mz.stats == [0, n] + [0] * 14 and np.array_equal(mz.bases, a.bases)
                    me = both_ways(lib, h, d, st, tab, counts, k, 1, r, S0, S0, pad=pad, what="every range empty")
                    assert me.stats[2] == n and me.stats[3] == 0
                for inplace in (False, True):
                    got = correct_call(lib, h, d, st, st.cols_in(4, 0), 0, rules_of(), tab.p, inplace=inplace)
                    assert got.error is None and got.stats == [0] * 16 and got.untouched
    finally:
        h.close()


# ---- a long record ---------------------------------------------------------------------------------------------------------------------
def run_long_record(lib, sh):
    rng = np.random.default_rng(1700)
    k, L = 15, 70000
    g = rng.integers(0, 4, L).astype(np.uint8)
    x = g.copy()
    for p in (5, L // 2, L - 1):
        x = sub(x, p)
    x[20000] = 4
    a = arrays([g[100: 160], x, sub(g[3000: 3050], 20), g[:k - 1]])
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=1) as st, Dev(h) as d:
            tab, counts = build_table(lib, h, d, arrays([g]), k, 1)
            m = correct_model(a, counts, k, 1, rules_of())
            assert m.fixed.tolist() == [0, 4, 1, 0] and m.stats[7] == 1 and np.array_equal(m.bases[60: 60 + L], g)
            both_ways(lib, h, d, st, tab, counts, k, 1, rules_of(), pad=1, model=m, what="a long record")
    finally:
        h.close()


# ---- record counts -----------------------------------------------------------------------------------------------------------------
def run_count(lib, sh, n_records):
    a, ref, b, e, keep = error_batch(700 + n_records, n_records, 7, genome=max(60, min(3000, 3 * n_records)), hi=40, rate=0.03)
    h = handle(lib)
    try:
        with staged(lib, h, a) as st, Dev(h) as d:
            tab, counts = build_table(lib, h, d, ref, 7, 1)
            m = both_ways(lib, h, d, st, tab, counts, 7, 1, rules_of(2, 38), b, e, keep, what=n_records)
            tab, counts = build_table(lib, h, d, ref, 11, 0)
            check_correct(lib, h, d, st, tab, counts, 11, 0, rules_of(), what=(n_records, "every record, forward"))
            if n_records >= 2049:
                assert m.stats[3] > 15000 and m.stats[1] > 100 and m.stats[6] > 100 and m.stats[10] > 0 and m.stats[14] > 0, m.stats
    finally:
        h.close()


def run_grid_stride(lib, sh):
    n = sh["stride_count"]
    a, ref, b, e, keep = error_batch(900, n, 6, genome=3000, lo=6, hi=20, rate=0.03, keep_share=0.95)
    counts = ck.kmer_model(ref, 6, 1)[0]
    m = correct_model(a, counts, 6, 1, rules_of(2), b, e, keep)
    second = slice(GRID_CAP * 16, None)
    assert m.fixed[second].sum() > 10 and m.stats[3] > 300000 and m.stats[6] > 1000       # the records of the second round count
    h = handle(lib)
    try:
        with staged(lib, h, a) as st, Dev(h) as d:
            tab, counts2 = build_table(lib, h, d, ref, 6, 1)
            assert counts2 == counts
            both_ways(lib, h, d, st, tab, counts, 6, 1, rules_of(2), b, e, keep, model=m, what="grid stride")
    finally:
        h.close()


# ---- idempotence -------------------------------------------------------------------------------------------------------------------
def run_idempotent(lib, sh):
    h = handle(lib)
    try:
        for seed, k in ((31, 11), (32, 21), (33, 5)):
            a, ref, b, e, keep = error_batch(seed, 80, k, genome=600, lo=0, hi=120)
            r = rules_of(2 if k > 5 else 4, 36)
            with Dev(h) as d:
                with staged(lib, h, a) as st:
                    tab, counts = build_table(lib, h, d, ref, k, 1)
                    m1 = check_correct(lib, h, d, st, tab, counts, k, 1, r, b, e, keep, what=("first pass", k))
                a2 = ce.Arrays(m1.bases, a.quals, a.titles, a.seq_offsets, a.title_offsets, a.block_records)
                m2 = correct_model(a2, counts, k, 1, r, b, e, keep)
                assert m1.stats[6] > 5 and m2.stats[6] == 0 and m2.stats[5] == m1.stats[5] - m1.stats[6] and np.array_equal(m2.bases, m1.bases), (m1.stats, m2.stats)
                assert m2.stats[9:15] == m1.stats[9:15]
                with staged(lib, h, a2) as st2:
                    both_ways(lib, h, d, st2, tab, counts, k, 1, r, b, e, keep, model=m2, what=("second pass", k))
    finally:
        h.close()


# ---- fuzz ------------------------------------------------------------------------------------------------------------------------
FUZZ_KS = (5, 21, 11, 31, 15, 16)
_fuzz_cache = {}


def fuzz_case(n, seed):
    """The reads of the k-mer count's fuzz (copies and reverse complements of earlier reads, codes that are no bases, poly-G tails,
    ranges, a keep) with substitutions -- one in five of them an N -- planted at 2 % on top, against the table of every third read as it was
    before the plants, a one-base variant of every sixth among them.  Low k: the table is dense and min_count does the telling."""
    if (n, seed) in _fuzz_cache:
        return _fuzz_cache[(n, seed)]
    k = FUZZ_KS[seed % len(FUZZ_KS)]
    canonical = 0 if seed % 3 == 2 else 1
    clean, begin, end, keep = ck.fuzz_batch(300 + seed, n, k)
    rng = np.random.default_rng(9500 + seed)
    S = clean.seq_offsets.astype(np.int64)
    ref = [clean.bases[S[i]: S[i + 1]] for i in range(0, n, 3)]
    for i in range(0, len(ref), 2):
        if len(ref[i]) > 4 and (ref[i] <= 3).all():
            ref.append(sub(ref[i], int(rng.integers(0, len(ref[i]))), rng))
    ref = arrays(ref)
    bases = clean.bases.copy()
    err = rng.random(len(bases)) < 0.02
    plant = rng.integers(0, 5, int(err.sum())).astype(np.uint8)
    bases[err] = np.where(bases[err] == plant, (plant + 1) % 4, plant)
    a = ce.Arrays(bases, rng.integers(0, 42, len(bases)).astype(np.uint8), clean.titles, clean.seq_offsets, clean.title_offsets, clean.block_records)
    counts = ck.kmer_model(ref, k, canonical)[0]
    r = rules_of(1 if k > 5 else (3 if n <= 150 else n // 20), (255, 30, 38)[seed % 3])       # (k = 5: about the median count of a batch's table)
    m = correct_model(a, counts, k, canonical, r, begin, end, keep)
    _fuzz_cache[(n, seed)] = (a, ref, begin, end, keep, k, canonical, counts, r, m)
    return _fuzz_cache[(n, seed)]


def run_fuzz_covers(sh):
    """The model alone: the seeds taken together hit every verdict."""
    seeds, n = sh["correct_fuzz"]
    total = [0] * 16
    for seed in range(seeds):
        m = fuzz_case(n, seed)[-1]
        print("kmer correct fuzz", seed, "records", n, "k", FUZZ_KS[seed % len(FUZZ_KS)], "stats", m.stats)
        total = [x + y for x, y in zip(total, m.stats)]
    assert all(total[i] > 0 for i in (1, 2, 6, 7, 9, 10, 11, 12, 13, 14, 15)), total


def run_fuzz(lib, sh, seed):
    n = sh["correct_fuzz"][1]
    a, ref, begin, end, keep, k, canonical, counts, r, m = fuzz_case(n, seed)
    assert m.stats[1] > 0 and m.stats[5] > m.stats[6] > 0 and m.stats[3] > m.stats[4] > 0
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=3) as st, Dev(h) as d:
            tab, counts2 = build_table(lib, h, d, ref, k, canonical)
            assert counts2 == counts
            both_ways(lib, h, d, st, tab, counts, k, canonical, r, begin, end, keep, pad=3, model=m, what=("fuzz", seed))
            check_correct(lib, h, d, st, tab, counts, k, canonical, rules_of(1 + seed % 2), pad=3, what=("fuzz, whole reads, any quality", seed))
    finally:
        h.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def run_arg_refusals(lib, sh):
    a, ref, b, e, keep = error_batch(41, 40, 7)
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

            def refused(name, r=rules_of(), table=tab.p, word=None, cols=cin, **kw):
                for inplace in (False, True):
                    got = correct_call(lib, h, d, st, cols, n, r, table, inplace=inplace, **kw)
                    assert got.error is not None and got.error.code == E_ARG and got.untouched, (name, got.error)
                    assert word is None or word in str(got.error), (name, str(got.error))
                assert tab.raw().tobytes() == before
                return 1
            checked += refused("min_count 0", rules_of(0), word="kmer correct rules: min_count must be at least 1")
            checked += refused("max_quality 256", rules_of(1, 256), word="kmer correct rules: max_quality above 255")
            checked += refused("max_quality 2^32 - 1", rules_of(1, 2 ** 32 - 1), word="max_quality above 255")
            for i in range(5):
                checked += refused("reserved[%d]" % i, reserved=tuple(int(j == i) for j in range(5)), word="kmer correct rules: reserved fields must be 0")
            checked += refused("begin alone", begin=u64(S0), word="columns: d_begin and d_end go together")
            checked += refused("end alone", end=u64(S1), word="columns: d_begin and d_end go together")
            checked += refused("null table", table=None, word="null argument")
            raw = ck.Table(lib, d, 64)                            # 0xA5 all over: no table's header
            checked += refused("no table", table=raw.p, word="kmer correct: not a k-mer table")
            assert raw.untouched()
            noq = st.cols_in(); noq.d_quals = None
            checked += refused("null d_quals under max_quality < 255", rules_of(1, 254), cols=noq, word="columns: null array with a length")
            assert checked == 13
            # null in, rules, table, output, stats: straight through the C ABI
            C = lib.C
            stats = (C.c_uint64 * 16)()
            R = lib_rules(lib, rules_of())
            po, pf = d.fill(len(st.host["bases"])), d.fill(8 * n)
            full = [C.byref(cin), C.byref(R), C.c_void_p(tab.p), None, None, None, C.c_void_p(po), C.c_void_p(pf), stats]
            for hole in (0, 1, 2, 6, 8):
                args = list(full); args[hole] = None
                assert h.L.dsrcgpu_columns_kmer_correct(h.h, *args) == E_ARG, hole
                assert all(d.down(p, sz) == b"\xA5" * (sz + 8) for p, sz in ((po, len(st.host["bases"])), (pf, 8 * n)))
            assert h.L.dsrcgpu_columns_kmer_correct(None, *full) == E_ARG
            assert h.L.dsrcgpu_columns_kmer_correct(h.h, *full) == 0 and list(stats)[0] == n      # the same arguments, whole: accepted
            # the limits themselves are accepted
            for r in (rules_of(2 ** 64 - 1), rules_of(1, 0), rules_of(1, 254)):
                check_correct(lib, h, d, st, tab, counts, k, 1, r, what=("limits", r))
    finally:
        h.close()
    hc = ce.handle(lib, dataclasses.replace(Config.from_levels(0, 0), color_space=True))
    try:
        with staged(lib, hc, a) as st, Dev(hc) as d:
            tab = ck.Table(lib, d, 64)
            got = correct_call(lib, hc, d, st, st.cols_in(), n, rules_of(), tab.p)
            assert got.error is not None and got.error.code == E_ARG and got.untouched and "colour-space" in str(got.error)
    finally:
        hc.close()


def run_input_errors(lib, sh):
    """The five input errors planted in the first, a middle and the last record, kept and dropped ones, in place and out of place: code,
    the lowest record, the reason's text, not a byte of either output changed, and the same handle works on the clean arrays afterwards."""
    a, ref, _, _, _ = error_batch(51, 41, 6, lo=8)
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
                for rules in (rules_of(), rules_of(2, 30)):
                    for inplace in (False, True):
                        got = correct_call(lib, h, d, st, st.cols_in(), n, rules, tab.p, *plan, inplace=inplace)
                        assert got.error is not None and got.error.code == E_INPUT and got.untouched, (name, r, got.error)
                        assert "columns: record %d:" % r in str(got.error) and word in str(got.error), (name, r, str(got.error))
                assert tab.raw().tobytes() == before
            offs = [("order", lambda r: st.poke("seq_offs", r + 1, S(r) - 1, np.uint64), "d_seq_offs is not non-decreasing"),
                    ("end", lambda r: st.poke("seq_offs", r + 1, len(a.bases) + pad + 5, np.uint64), "d_seq_offs runs above bases_len"),
                    ("wild", lambda r: st.poke("seq_offs", r + 1, 2 ** 64 - 1, np.uint64), "d_seq_offs runs above bases_len")]
            for name, plant, word in offs:
                for r in (0, 20, 40):
                    plant(r)
                    if r == 0:
                        plant(40)                            # two plants: the lowest record is the one named
                    for plan in ((None, None, None), (hb, he, keep)):
                        refused_offsets(lib, h, d, st, n, tab, r, word, name, plan, before)
                    st.restore()
                    checked += 1
                check_correct(lib, h, d, st, tab, counts, k, 1, rules_of(), keep=keep, pad=pad, what=("after", name))
            ranges = [("begin low", lambda r: dict(b=S(r) - 1), "d_begin lies below the record's first base"),
                      ("end high", lambda r: dict(e=S(r + 1) + 1), "d_end lies above the record's last base"),
                      ("end wild", lambda r: dict(e=2 ** 64 - 1), "d_end lies above the record's last base"),
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
                both_ways(lib, h, d, st, tab, counts, k, 1, rules_of(), S0, S1, keep, pad=pad, what=("after", name))
    finally:
        h.close()
    assert checked == 21


def refused_offsets(lib, h, d, st, n, tab, r, word, name, plan, before):
    """A call on staged arrays whose offsets are spoilt: correct_call compares the inputs with the host's copy, which the plant has left
    behind, so the call is made here."""
    up = lambda v, dt: None if v is None else d.up(np.ascontiguousarray(v).astype(dt).tobytes())
    size = len(st.host["bases"])
    for rules in (rules_of(), rules_of(2, 30)):
        for inplace in (False, True):
            po = st.ptr["bases"] if inplace else d.fill(size)
            pf = d.fill(8 * n)
            try:
                h.columns_kmer_correct(st.cols_in(), lib_rules(lib, rules), tab.p, up(plan[0], np.uint64), up(plan[1], np.uint64), up(plan[2], np.uint8), po, pf)
            except lib.DsrcGpuError as e:
                assert e.code == E_INPUT and "columns: record %d:" % r in str(e) and word in str(e), (name, r, str(e))
            else:
                raise AssertionError("no error for %s in record %d" % (name, r))
            assert d.down(pf, 8 * n) == b"\xA5" * (8 * n + 8)
            assert d.down(po, size) == (st.host["bases"] + b"\xA5" * 8 if inplace else b"\xA5" * (size + 8)), (name, r, "an output has been written")
    assert tab.raw().tobytes() == before


def run_codec_state(lib, sh):
    """The call touches nothing the codec carries, as run_codec_state of the planners: the fields capacity stays, a pending record
    layout stays pending, and the text call that follows writes what it writes on a fresh handle seeded alike."""
    a, ref, b, e, keep = error_batch(61, 60, 9)
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
                both_ways(lib, h, d, st, tab, counts, 9, 1, rules_of(2, 30), b, e, keep)
                assert h.get_fields_capacity() == 11
            assert text_blocks(h) == text_blocks(fresh), layout
        finally:
            h.close(); fresh.close()


# ---- the Python layers and the closed loop ---------------------------------------------------------------------------------------------
text_of = kp.text_of
same_tensors = kp.same_tensors


def run_python_layers(lib, sh, device):
    from dsrc_amd import columns
    a, ref, begin, end, keep = error_batch(71, 90, 13, genome=500, hi=120)
    n, k = a.n_records, 13
    t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v).astype(dt)).to(device)
    dev = torch.device(device).type
    h = handle(lib)
    try:
        assert tuple(lib.KMER_CORRECT_STATS) == CORRECT_STATS and "dsrcgpu_columns_kmer_correct" in lib.EXPORTS
        tab, _ = columns.count_kmers(h, tensors(ref, device), k)
        counts = ck.kmer_model(ref, k, 1)[0]
        assert ck.table_dict(tab) == counts
        before = tab.data.clone()
        c = tensors(a, device)
        tb, te, tk = t(begin, np.int64), t(end, np.int64), t(keep, np.uint8)
        m = correct_model(a, counts, k, 1, rules_of(2), begin, end, keep)
        assert m.stats[6] > 10 and m.stats[1] > 0
        got = columns.correct_kmers(h, c, tab, tb, te, tk)                                  # min_count = 2 is the default
        assert len(got) == 2 and list(got[1]) == list(CORRECT_STATS) and list(got[1].values()) == m.stats
        out = got[0]
        assert out is not c and out.bases.dtype == torch.uint8 and out.bases.device.type == dev and np.array_equal(out.bases.cpu().numpy(), m.bases)
        assert all(getattr(out, f.name) is getattr(c, f.name) for f in dataclasses.fields(c) if f.name != "bases")
        assert np.array_equal(c.bases.cpu().numpy(), a.bases) and torch.equal(tk, t(keep, np.uint8)) and torch.equal(tb, t(begin, np.int64))      # inputs as they were
        m30 = correct_model(a, counts, k, 1, rules_of(1, 30))
        got = columns.correct_kmers(h, c, tab, min_count=1, max_quality=30, return_fixed=True)
        assert len(got) == 3 and list(got[1].values()) == m30.stats and got[2].dtype == torch.int64 and got[2].device.type == dev
        assert got[2].tolist() == m30.fixed.tolist() and np.array_equal(got[0].bases.cpu().numpy(), m30.bases) and m30.stats[14] > 0
        c2 = tensors(a, device)
        got = columns.correct_kmers(h, c2, tab, tb, te, tk, inplace=True, return_fixed=True)
        assert got[0] is c2 and np.array_equal(c2.bases.cpu().numpy(), m.bases) and list(got[1].values()) == m.stats and got[2].tolist() == m.fixed.tolist()
        assert torch.equal(tab.data, before)                 # the table is only read
        # no records
        none = columns.columns_from_sequences([], device)
        for inplace in (False, True):
            e0 = columns.correct_kmers(h, none, tab, inplace=inplace, return_fixed=True)
            assert e0[0].n_records == 0 and e0[0].bases.numel() == 0 and not any(e0[1].values()) and e0[2].numel() == 0

        class Never:                                         # ValueError comes before any library call
            def __getattr__(self, name):
                raise AssertionError("the library was called")
        bad_calls = [dict(table=None), dict(table="table"), dict(table=tab.data), dict(begin=tb), dict(end=te), dict(begin=tb[:5], end=te[:5]), dict(keep=tk[:7]),
                     dict(min_count=0), dict(min_count=1.0), dict(min_count=True), dict(max_quality=-1), dict(max_quality=256), dict(max_quality=3.5)]
        calls = [lambda bad=bad: columns.correct_kmers(Never(), c, **dict(dict(table=tab), **bad)) for bad in bad_calls]
        calls += [lambda: columns.filter_columns(Never(), c, correct=tab), lambda: columns.filter_columns(Never(), c, correct=dict(min_count=2)),
                  lambda: columns.filter_columns(Never(), c, correct=dict(table=tab, k=13)), lambda: columns.filter_columns(Never(), c, correct=dict(k=32)),
                  lambda: columns.filter_columns(Never(), c, correct=dict(table=tab, trim="x")), lambda: columns.filter_columns(Never(), c, correct=dict(k=13, min_count=0)),
                  lambda: columns.filter_pairs(Never(), c, c, correct=dict(table=tab, max_quality=256)), lambda: columns.filter_pairs(Never(), c, c, correct=dict(table="t")),
                  lambda: columns.correct_kmers(Never(), dataclasses.replace(c, bases=torch.stack((c.bases, c.bases), 1)[:, 0]), tab, inplace=True)]
        if dev != "cpu":                                     # a table on another device
            calls.append(lambda: columns.correct_kmers(Never(), c, columns.KmerTable(tab.data.cpu(), k, True)))
        for i, call in enumerate(calls):
            try:
                call()
            except ValueError:
                pass
            else:
                raise AssertionError("no ValueError for call %d" % i)
    finally:
        h.close()


def run_filters(lib, sh, device):
    """filter_columns(correct=...) and filter_pairs(correct=...) against the same steps called by hand, and against the model.  The default
    leaves both functions as they are."""
    from dsrc_amd import columns
    from tests import columns_adapt_cases as ca
    from tests import columns_dedup_cases as cd
    (a1, _, _), (a2, _, _) = cd.duplicated_reads(120, 41, pairs=True)
    rng = np.random.default_rng(1800)
    sides = []
    for a in (a1, a2):                                       # substitutions on top of the duplicated reads
        bases = a.bases.copy()
        err = (rng.random(len(bases)) < 0.01) & (bases <= 3)
        bases[err] = (bases[err] + rng.integers(1, 4, int(err.sum()))) % 4
        sides.append(ce.Arrays(bases, a.quals, a.titles, a.seq_offsets, a.title_offsets, a.block_records))
    e1, e2 = sides
    trim = cs.rules_of(0, 20, min_length=30, max_n=1)
    k = 15
    ref = arrays([a1.bases[s: t] for s, t in zip(*whole(a1)) if (a1.bases[s: t] <= 3).all()])
    counts = ck.kmer_model(ref, k, 1)[0]
    h = handle(lib)
    try:
        c1, c2 = tensors(e1, device), tensors(e2, device)
        tab, _ = columns.count_kmers(h, tensors(ref, device), k)
        plain, plain_stats = columns.filter_columns(h, c1, **trim)
        again, again_stats = columns.filter_columns(h, c1, correct=None, **trim)
        assert plain_stats == again_stats and same_tensors(plain, again)
        b, e, kp_, ts = cs.plan_model(e1, trim)
        m = correct_model(e1, counts, k, 1, rules_of(2), b, e, kp_)
        assert m.stats[6] > 5 and m.stats[1] > 0, m.stats
        fixed = ce.Arrays(m.bases, e1.quals, e1.titles, e1.seq_offsets, e1.title_offsets, e1.block_records)
        out, stats = columns.filter_columns(h, c1, correct=dict(table=tab), **trim)
        assert stats == dict(dict(zip(ca.TRIM_STATS, ts)), correct=dict(zip(CORRECT_STATS, m.stats))) and list(stats)[-1] == "correct"
        assert cd.same_columns(out, cs.select_model(fixed, b, e, kp_)) and np.array_equal(c1.bases.cpu().numpy(), e1.bases)
        # the screen, dedup, profile_after and kmers_after see the repaired bases; profile_before the bases as they came
        screen = dict(table=tab, trim="first_miss", min_count=2)
        out, stats = columns.filter_columns(h, c1, correct=dict(table=tab, min_count=2), screen=screen, dedup=True, profile=True, kmers=9, **trim)
        mp = kp.plan_model(fixed, counts, k, 1, kp.rules_of(trim=1, min_count=2, min_length=30), b, e, kp_)
        md = cd.dedup_model(fixed, r1=(mp.begin, mp.end), keep=mp.keep)
        assert list(stats)[-6:-3] == ["correct", "screen", "dedup"] and list(stats["screen"].values()) == mp.stats[:15] and list(stats["dedup"].values()) == md[3]
        assert cd.same_columns(out, cs.select_model(fixed, mp.begin, mp.end, md[0]))
        assert ck.table_dict(stats["kmers_after"]) == ck.kmer_model(fixed, 9, 1, mp.begin, mp.end, md[0])[0]
        assert stats["profile_before"].summary() == columns.profile_columns(h, c1).summary() and stats["profile_after"].summary()["bases"] == out.bases.numel()
        mp0 = kp.plan_model(e1, counts, k, 1, kp.rules_of(trim=1, min_count=2, min_length=30), b, e, kp_)
        assert mp0.stats != mp.stats                          # ... and that makes a difference
        # k=: the batch under the plan at that point is its own table
        own = ck.kmer_model(e1, k, 1, b, e, kp_)[0]
        mo = correct_model(e1, own, k, 1, rules_of(3), b, e, kp_)
        out, stats = columns.filter_columns(h, c1, correct=dict(k=k, min_count=3), **trim)
        assert list(stats["correct"].values()) == mo.stats and mo.stats[6] > 0
        assert cd.same_columns(out, cs.select_model(ce.Arrays(mo.bases, e1.quals, e1.titles, e1.seq_offsets, e1.title_offsets, e1.block_records), b, e, kp_))
        # pairs: per side in front of the pair plan; with k= one table of both mates
        kw = dict(pair_min_overlap=20, pair_max_mismatches=4, pair_max_error_permille=150)
        p1, p2, pstats = columns.filter_pairs(h, c1, c2, **kw, **trim)
        q1, q2, qstats = columns.filter_pairs(h, c1, c2, correct=None, **kw, **trim)
        assert pstats == qstats and same_tensors(p1, q1) and same_tensors(p2, q2)
        plans = [cs.plan_model(x, trim)[:3] for x in (e1, e2)]
        both = ck.kmer_model(e2, k, 1, *plans[1], table=ck.kmer_model(e1, k, 1, *plans[0])[0])[0]
        for correct, table in ((dict(k=k, min_count=3), both), (dict(table=tab, min_count=2, max_quality=35), counts)):
            o1, o2, ostats = columns.filter_pairs(h, c1, c2, correct=correct, **kw, **trim)
            r = rules_of(correct["min_count"], correct.get("max_quality", 255))
            ms = [correct_model(x, table, k, 1, r, *plan) for x, plan in zip((e1, e2), plans)]
            assert [list(ostats[s]["correct"].values()) for s in ("read1", "read2")] == [ms[0].stats, ms[1].stats] and ms[0].stats[6] > 0
            f1, f2 = (dataclasses.replace(c, bases=torch.from_numpy(mm.bases).to(device)) for c, mm in zip((c1, c2), ms))
            hp = [columns.trim_plan(h, c, **trim)[:3] for c in (c1, c2)]
            b1, x1, b2, x2, keep, ps = columns.pair_plan(h, f1, f2, hp[0], hp[1], 20, 4, 150, 30)
            assert ostats["pair"] == ps
            assert same_tensors(o1, columns.select_columns(h, f1, b1, x1, keep)) and same_tensors(o2, columns.select_columns(h, f2, b2, x2, keep))
    finally:
        h.close()


def run_closed_loop(lib, sh, device):
    """Records written here -> the oracle's block -> decode_columns -> count_kmers -> correct_kmers -> encode_columns -> decode_columns:
    the bases that come back are the model's, the qualities and the titles are untouched, and at least one N was repaired on the way."""
    from dsrc_amd import columns
    from tests import columns_dedup_cases as cd
    cfg = ce.BLOCK_CFG
    rng = np.random.default_rng(1900)
    g = rng.integers(0, 4, 400).astype(np.uint8)
    recs = []
    for r in range(150):
        at = int(rng.integers(0, 340))
        x = g[at: at + 60].copy()
        if rng.random() < 0.5:
            x = cp.revcomp(x)
        err = rng.random(60) < 0.01
        x[err] = (x[err] + rng.integers(1, 4, int(err.sum()))) % 4
        if rng.random() < 0.1:
            x[int(rng.integers(0, 60))] = 4
        recs.append((b"@loop.%d" % (r + 1), bytes(b"ACGTN"[v] for v in x), bytes((rng.integers(2, 41, 60) + 33).astype(np.uint8))))
    text = b"\n".join(t + b"\n" + sq + b"\n+\n" + q for t, sq, q in recs)
    a = ce.arrays_of([text])
    k = 17
    counts = ck.kmer_model(a, k, 1)[0]
    m = correct_model(a, counts, k, 1, rules_of(3))
    print("closed loop: model stats", m.stats)
    assert m.stats[6] > 20 and m.stats[7] > 0
    want = ce.Arrays(m.bases, a.quals, a.titles, a.seq_offsets, a.title_offsets, a.block_records)
    src = ce.oracle_blocks(cfg, [text])
    assert src is not None
    h = ce.handle(lib, cfg)
    try:
        d_blocks, offs = cs._stage_blocks([src[0][0]], device)
        rc = columns.decode_columns(h, d_blocks, offs, [len(src[0][0])], device)
        assert rc.n_records == 150
        tab, _ = columns.count_kmers(h, rc, k)
        out, stats = columns.correct_kmers(h, rc, tab, min_count=3)
        assert list(stats.values()) == m.stats
        h.set_fields_capacity(0)
        blocks, o_offs, o_sizes, _ = columns.encode_columns(h, out, block_records=out.block_records)
    finally:
        h.close()
    h = ce.handle(lib, cfg)
    try:
        back = columns.decode_columns(h, blocks, o_offs, o_sizes, device)
        got = (back.bases, back.quals, back.titles, back.seq_offsets, back.title_offsets)
        assert all(np.array_equal(x.cpu().numpy().astype(w.dtype), w) for x, w in zip(got, (want.bases, want.quals, want.titles, want.seq_offsets, want.title_offsets)))
    finally:
        h.close()


# ---- the rule's accuracy, model only -------------------------------------------------------------------------------------------------
def run_accuracy():
    """Reads of 100 bases at 30x from a genome of 20 000, both strands, 1 % substitutions, k = 21, canonical, min_count = 3, against the
    table of the reads themselves: at least half of the wrong bases are put right and no right base is made wrong."""
    rng = np.random.default_rng(2100)
    G, L, k = 20000, 100, 21
    g = rng.integers(0, 4, G).astype(np.uint8)
    n = 30 * G // L
    truth, reads = [], []
    for _ in range(n):
        at = int(rng.integers(0, G - L + 1))
        x = g[at: at + L].copy()
        if rng.random() < 0.5:
            x = cp.revcomp(x)
        truth.append(x.copy())
        err = rng.random(L) < 0.01
        x[err] = (x[err] + rng.integers(1, 4, int(err.sum()))) % 4
        reads.append(x)
    a, t = arrays(reads), np.concatenate(truth)
    counts = ck.kmer_model(a, k, 1)[0]
    m = correct_model(a, counts, k, 1, rules_of(3))
    wrong_before, wrong_after = int((a.bases != t).sum()), int((m.bases != t).sum())
    made_wrong = int(((a.bases == t) & (m.bases != t)).sum())
    print("accuracy: wrong before", wrong_before, "after", wrong_after, "right made wrong", made_wrong, "stats", m.stats)
    assert wrong_after * 2 <= wrong_before and made_wrong == 0
