"""Shared by tests/test_emu_columns_profile.py (CPU, emulator build) and tests/test_gpu_columns_profile.py (MI355X): the cases of the
columnar profile (dsrcgpu_columns_profile; dsrc_amd/csrc/k_columns_profile.h) and what they must give.

The reference has no counterpart, so the yardstick is the integer model written out here: profile_model() is the serial rule of
include/dsrc_gpu.h word for word, a record at a time (the loop over a record's positions is written with numpy index arithmetic: c =
min(i, C - 1), k = x < 4 ? x : 4, one add per position and table), in int64 throughout.  None of it comes from the library under
test, and every comparison is exact equality of all 11 C + 622 words.  d_profile is allocated with GUARD words on both sides and
filled with 0xA5 before a call, so that "overwritten", "untouched" and "not a word beyond" can be asserted.  Before the library is
compared on a crafted case the model alone is asked what that case is for.

Shapes.  The emulator pays a coroutine switch per wave exchange, so its fuzz is 2 seeds x 150 records where the GPU runs 6 x 2000.
The profile's grid holds at most 512 workgroups of WG / 64 waves up to 256 cycles and 256 workgroups above (prof_max_grid): with
workgroups of 1024 threads a count above 512 * 16 records takes the grid stride into a second round at 151 cycles, one above 256 * 16
at 1024 cycles -- those counts run on the GPU only (on the emulator, with workgroups of 256 threads, 2049 records are already above
512 * 4).  The record of 2^24 + 5 bases runs on the GPU only."""
from __future__ import annotations

import dataclasses

import numpy as np
import torch        # noqa: F401  before the first handle (see columns_cases)

from tests import columns_adapt_cases as ca
from tests import columns_cases as cc
from tests import columns_enc_cases as ce
from tests import columns_pair_cases as cp
from tests import columns_sel_cases as cs
from tests._oracle import Config
from tests.cases import TINY

E_ARG, E_INPUT = cs.E_ARG, cs.E_INPUT
MAX_CYCLES = 1024
GUARD = 16                                                   # words of 0xA5 on either side of d_profile
A5 = np.uint64(cs.A5_64)
TOTALS = ("records", "bases", "bases_q20", "bases_q30", "quality_sum", "gc_bases", "other_bases", "empty_records")


def max_grid(C):
    return 512 if C <= 256 else 256


SHAPES = {
    "gpu": dict(cc.SHAPES["gpu"], prof_fuzz=(6, 2000), counts=[1, 63, 64, 65, 2049], stride_counts=[(151, max_grid(151) * 16 + 1001), (1024, max_grid(1024) * 16 + 301)]),
    "emu": dict(cc.SHAPES["emu"], prof_fuzz=(2, 150), counts=[1, 63, 64, 65, 2049], stride_counts=[]),
}
Arrays = ce.Arrays
Dev = cs.Dev
CYCLES = [1, 2, 64, 151, 1024]
CODES = np.array([0, 1, 2, 3, 4, 18, 255], np.uint8)
QUALS = np.array([0, 19, 20, 29, 30, 255], np.uint8)


def words_of(C):
    return 11 * C + 622


# ---- the model -------------------------------------------------------------------------------------------------------------------
def tables(p, C):
    """The seven tables of a profile of C cycles as views: tot, base, qsum, qhist, len, gc, meanq."""
    p = np.asarray(p)
    assert len(p) == words_of(C)
    return (p[0:8], p[8: 8 + 5 * C].reshape(C, 5), p[8 + 5 * C: 8 + 10 * C].reshape(C, 5), p[8 + 10 * C: 264 + 10 * C],
            p[264 + 10 * C: 265 + 11 * C], p[265 + 11 * C: 366 + 11 * C], p[366 + 11 * C: 622 + 11 * C])


def profile_model(a: Arrays, C, begin=None, end=None, keep=None, first=0, n=None):
    """The serial rule on records first .. first + n - 1 under the plan (positions in a.bases) -> the profile, int64[11 C + 622]."""
    assert 1 <= C <= MAX_CYCLES
    S = [int(v) for v in a.seq_offsets]
    n = a.n_records - first if n is None else n
    p = np.zeros(words_of(C), np.int64)
    tot, base, qsum, qhist, length, gc, meanq = tables(p, C)
    for j in range(n):
        r = first + j
        b, e = (S[r], S[r + 1]) if begin is None else (int(begin[j]), int(end[j]))
        assert S[r] <= b <= e <= S[r + 1]
        if keep is not None and int(keep[j]) == 0:
            continue                                         # a record with a zero keep byte counts in nothing
        m = e - b
        x = a.bases[b:e].astype(np.int64); q = a.quals[b:e].astype(np.int64)
        k = np.where(x < 4, x, 4)                            # the class
        c = np.minimum(np.arange(m), C - 1)                  # the cycle: the position in the range, folded
        np.add.at(base, (c, k), 1); np.add.at(qsum, (c, k), q); np.add.at(qhist, q, 1)
        qs = int(q.sum()); g = int(((x == 1) | (x == 2)).sum()); acgt = int((x < 4).sum())
        tot[0] += 1; tot[1] += m; tot[2] += int((q >= 20).sum()); tot[3] += int((q >= 30).sum()); tot[4] += qs; tot[5] += g; tot[6] += m - acgt
        length[min(m, C)] += 1
        if acgt > 0:
            gc[100 * g // acgt] += 1
        if m > 0:
            meanq[qs // m] += 1
        else:
            tot[7] += 1
    return p


def invariants(p, C, what=None):
    tot, base, qsum, qhist, length, gc, meanq = tables(np.asarray(p).astype(np.int64), C)
    assert int(base.sum()) == int(tot[1]) and int(qsum.sum()) == int(tot[4]) and int(qhist.sum()) == int(tot[1]), what
    assert int(length.sum()) == int(tot[0]) and int(meanq.sum()) == int(tot[0]) - int(tot[7]) and int(gc.sum()) <= int(tot[0]), what
    assert int(tot[3]) <= int(tot[2]) <= int(tot[1]) and int(tot[5]) + int(tot[6]) <= int(tot[1]), what


# ---- records ---------------------------------------------------------------------------------------------------------------------
def arrays_from(reads):
    """Reads given as (codes, qualities) pairs; titles @r<i>."""
    a = ca.arrays_from_bases([x for x, _ in reads])
    a.quals = np.concatenate([np.asarray(q, np.uint8) for _, q in reads] + [np.zeros(0, np.uint8)]).astype(np.uint8)
    assert len(a.quals) == len(a.bases)
    return a


def random_read(n, rng, special=0.3):
    """n bases: A C G T and Phred 0 .. 41, `special` of the positions from CODES / QUALS."""
    x = rng.integers(0, 4, n).astype(np.uint8); q = rng.integers(0, 42, n).astype(np.uint8)
    sx, sq = rng.random(n) < special, rng.random(n) < special
    x[sx] = CODES[rng.integers(0, len(CODES), int(sx.sum()))]; q[sq] = QUALS[rng.integers(0, len(QUALS), int(sq.sum()))]
    return x, q


def handle(lib):
    return ce.handle(lib, Config.from_levels(0, 0))


def staged(lib, h, a, pad=0):
    return cs.staged(lib, h, a, pad)


# ---- one call ----------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Got:
    error: object
    totals: object
    profile: np.ndarray          # uint64, the words of d_profile after the call
    untouched: bool              # d_profile is what it was before the call


def prof_call(lib, h, cin, C, plan=(None, None, None), accumulate=0, prior=None, reserved=(0,) * 6, null_profile=False, n_words=None):
    """One dsrcgpu_columns_profile.  plan: begin / end / keep as numpy in the coordinates of the staged arrays, or None.  d_profile
    holds `prior` (0xA5 words if None) between GUARD words of 0xA5 on either side."""
    words = words_of(C) if n_words is None else n_words
    before = np.full(words, A5, np.uint64) if prior is None else np.asarray(prior).astype(np.uint64)
    assert len(before) == words
    with Dev(h) as d:
        pin = [None if v is None else d.up(np.ascontiguousarray(v).astype(dt).tobytes()) for v, dt in zip(plan, (np.uint64, np.uint64, np.uint8))]
        buf = d.up(b"\xA5" * (8 * GUARD) + before.tobytes() + b"\xA5" * (8 * GUARD))
        err = totals = None
        try:
            totals = h.columns_profile(cin, pin[0], pin[1], pin[2], lib.ProfileRules(C, accumulate, reserved), None if null_profile else buf + 8 * GUARD)
        except lib.DsrcGpuError as e:
            err = e
        raw = np.frombuffer(d.down(buf, 8 * (words + 2 * GUARD)), np.uint8)[: 8 * (words + 2 * GUARD)].view(np.uint64)
    assert (raw[:GUARD] == A5).all() and (raw[GUARD + words:] == A5).all(), "written outside d_profile"
    after = raw[GUARD: GUARD + words].copy()
    return Got(err, totals, after, bool((after == before).all()))


def check_profile(lib, h, st, C, begin=None, end=None, keep=None, pad=0, first=0, n=None, what=None, model=None):
    """Arrays staged in `st`, the plan as positions in the UNPADDED arrays (the pad is added here) -> the call over 0xA5 == the model."""
    n = st.a.n_records - first if n is None else n
    m = model if model is not None else profile_model(st.a, C, begin, end, keep, first, n)
    invariants(m, C, what)
    shift = lambda v: None if v is None else np.asarray(v).astype(np.uint64) + np.uint64(pad)
    got = prof_call(lib, h, st.cols_in(first, n), C, (shift(begin), shift(end), keep))
    assert got.error is None, (what, got.error)
    same(got.profile, m, C, what)
    assert got.totals == [int(v) for v in m[:8]], (what, got.totals, m[:8])
    return m


def same(p, m, C, what=None):
    bad = np.nonzero(np.asarray(p).astype(np.uint64) != np.asarray(m).astype(np.uint64))[0]
    if len(bad):
        w = int(bad[0])
        names = ("tot", "base", "qsum", "qhist", "len", "gc", "meanq")
        starts = (0, 8, 8 + 5 * C, 8 + 10 * C, 264 + 10 * C, 265 + 11 * C, 366 + 11 * C)
        t = max(i for i, s in enumerate(starts) if s <= w)
        raise AssertionError((what, "word", w, names[t], w - starts[t], "got", int(p[w]), "want", int(m[w]), len(bad), "words differ"))


# ---- geometry --------------------------------------------------------------------------------------------------------------------
def run_geometry(lib, sh, C):
    rng = np.random.default_rng(100 + C)
    lengths = sorted({0, 1, 63, 64, 65, 127, 128, 129, 150, C - 1, C, C + 1, 3 * C})
    reads = [random_read(n, rng) for n in lengths for _ in range(2)]
    a = arrays_from(reads)
    m = profile_model(a, C)
    tot, base, qsum, qhist, length, gc, meanq = tables(m, C)
    # the model alone: bases beyond C - 1 fold into the last cycle, the last length bin takes everything from C on
    beyond = sum(max(0, n - C) for n in lengths) * 2
    at_last = sum(1 for n in lengths if n >= C) * 2
    assert beyond > 0 and int(base[C - 1].sum()) == at_last + beyond, (C, beyond, at_last)
    assert int(length[C]) == at_last and int(length[0]) == 2 and int(tot[7]) == 2 and int(tot[0]) == len(reads)
    if C > 1:
        assert int(base[0].sum()) == sum(1 for n in lengths if n >= 1) * 2
    else:
        assert int(base[0].sum()) == int(tot[1])                # n_cycles = 1: every base on one cycle
    assert all(int(qhist[q]) > 0 for q in QUALS) and int(base[:, 4].sum()) > 0
    h = handle(lib)
    try:
        for pad in (0, 5):
            with staged(lib, h, a, pad=pad) as st:
                check_profile(lib, h, st, C, pad=pad, what=("geometry", C, pad), model=m)
    finally:
        h.close()


# ---- values ----------------------------------------------------------------------------------------------------------------------
def run_values(lib, sh):
    """One value throughout (the worst case for same-address atomics); a record without A C G T; GC bins 0, 50 and 100 hit exactly;
    100 g / a and qs / n where rounding up would differ; every code and quality of CODES / QUALS at a cycle of its own."""
    h = handle(lib)
    try:
        for x0, q0 in ((2, 37), (255, 255), (0, 0)):
            a = arrays_from([(np.full(n, x0, np.uint8), np.full(n, q0, np.uint8)) for n in (1, 64, 65, 150, 150, 400)])
            for C in (1, 64, 151):
                m = profile_model(a, C)
                tot, base, qsum, qhist, length, gc, meanq = tables(m, C)
                assert int(qhist[q0]) == 830 and int(meanq[q0]) == 6 and int(base[:, min(x0, 4)].sum()) == 830 and int(qsum.sum()) == 830 * q0
                assert int(gc.sum()) == (6 if x0 < 4 else 0) and (x0 >= 4 or int(gc[100 if x0 == 2 else 0]) == 6)
                with staged(lib, h, a) as st:
                    check_profile(lib, h, st, C, what=("one value", x0, q0, C), model=m)
        cases = [([4, 18, 255, 4], [10, 10, 10, 11]),        # 0: a == 0: no GC bin, meanq[10] (41 / 4)
                 ([0, 3, 0, 3], [30, 31, 30, 31]),           # 1: GC 0; qs / n = 122 / 4 = 30 (30.5 rounds up to 31)
                 ([1, 0, 2, 3], [29, 30, 30, 30]),           # 2: GC 50 exactly; 119 / 4 = 29 (29.75)
                 ([1, 2, 2, 1], [0, 0, 0, 1]),               # 3: GC 100; 1 / 4 = 0
                 ([1, 2, 0, 4, 255], [20, 20, 20, 20, 19]),  # 4: g = 2, a = 3: 66 (66.67 rounds up to 67), codes >= 4 are not in a
                 ([1, 0, 0], [255, 255, 254]),               # 5: g = 1, a = 3: 33; 764 / 3 = 254 (254.67)
                 ([2] + [0] * 198 + [1], [40] * 200),        # 6: g = 2, a = 200: bin 1 exactly
                 ([2] + [0] * 199 + [4] * 9, [40] * 209)]    # 7: g = 1, a = 200: bin 0 (0.5)
        a = arrays_from([(np.array(x, np.uint8), np.array(q, np.uint8)) for x, q in cases])
        for C in (2, 64):
            m = profile_model(a, C)
            tot, base, qsum, qhist, length, gc, meanq = tables(m, C)
            assert int(gc.sum()) == 7 and int(meanq.sum()) == 8 and [int(gc[v]) for v in (0, 1, 33, 50, 66, 67, 100)] == [2, 1, 1, 1, 1, 0, 1]
            assert [int(meanq[v]) for v in (0, 10, 20, 29, 30, 31, 40, 254, 255)] == [1, 1, 0, 1, 1, 0, 2, 1, 0] and int(meanq[19]) == 1
            assert int(tot[2]) == 4 + 4 + 4 + 3 + 209 + 200 and int(tot[3]) == 4 + 3 + 3 + 409 and int(tot[6]) == 4 + 2 + 9
            with staged(lib, h, a) as st:
                check_profile(lib, h, st, C, what=("rounding", C), model=m)
        # every code against every quality, one pair per cycle
        xs = np.repeat(CODES, len(QUALS)); qs = np.tile(QUALS, len(CODES))
        a = arrays_from([(xs, qs), (xs[::-1].copy(), qs)])
        m = profile_model(a, 64)
        tot, base, qsum, qhist, length, gc, meanq = tables(m, 64)
        assert [int(v) for v in base.sum(axis=0)] == [12, 12, 12, 12, 36] and int(qhist[255]) == 14 and int(tot[2]) == 56 and int(tot[3]) == 28
        with staged(lib, h, a) as st:
            check_profile(lib, h, st, 64, what="codes x qualities", model=m)
    finally:
        h.close()


# ---- plans in --------------------------------------------------------------------------------------------------------------------
def plan_records(rng, n_rec=60):
    """Reads of 0 .. 300 bases and a plan: 5' and 3' cuts, empty ranges at the start, in the middle and at the end of a read, keep
    bytes 0, 1, 7, 255."""
    a = arrays_from([random_read(int(rng.integers(0, 301)) if r % 7 else 150, rng) for r in range(n_rec)])
    S = a.seq_offsets.astype(np.int64)
    lens = S[1:] - S[:-1]
    cut5 = (rng.random(n_rec) * (lens + 1) * 0.3).astype(np.int64)
    cut3 = (rng.random(n_rec) * (lens - cut5 + 1) * 0.3).astype(np.int64)
    begin, end = S[:-1] + cut5, S[1:] - cut3
    begin[7], end[7] = S[7], S[7]                            # empty: at the start
    begin[14], end[14] = S[14] + 75, S[14] + 75              # in the middle
    begin[21], end[21] = S[22], S[22]                        # at the end
    keep = np.array([1, 7, 0, 255, 1, 1] * (n_rec // 6 + 1), np.uint8)[:n_rec]
    keep[[7, 14, 21]] = 1
    return a, begin.astype(np.uint64), end.astype(np.uint64), keep


def run_plans_in(lib, sh):
    rng = np.random.default_rng(400)
    a, begin, end, keep = plan_records(rng)
    n = a.n_records
    S = a.seq_offsets.astype(np.int64)
    C = 151
    whole, ranged, both = profile_model(a, C), profile_model(a, C, begin, end), profile_model(a, C, begin, end, keep)
    # the model alone: the cycle counts from `begin` (a record of 150 bases cut by 10 at the 5' end has nothing at cycle 140), what
    # lies beyond `end` is not counted, empty ranges count as records of length 0, dropped records count in nothing
    one = arrays_from([(np.arange(150) % 4, np.full(150, 30))])
    t = tables(profile_model(one, C, [10], [150]), C)
    assert int(t[1][139].sum()) == 1 and int(t[1][140:].sum()) == 0 and int(t[1][0, 10 % 4]) == 1 and int(t[4][140]) == 1
    assert int(tables(ranged, C)[0][1]) == int((end - begin).sum()) < int(tables(whole, C)[0][1]) == len(a.bases)
    assert int(tables(ranged, C)[0][7]) >= 3 and int(tables(ranged, C)[0][0]) == n and int(tables(both, C)[0][0]) == int((keep != 0).sum()) < n
    h = handle(lib)
    try:
        for pad in (0, 5):
            with staged(lib, h, a, pad=pad) as st:
                check_profile(lib, h, st, C, pad=pad, what=("whole reads", pad), model=whole)
                check_profile(lib, h, st, C, begin, end, pad=pad, what=("ranges", pad), model=ranged)
                check_profile(lib, h, st, C, begin, end, keep, pad=pad, what=("ranges, keep", pad), model=both)
                check_profile(lib, h, st, C, None, None, keep, pad=pad, what=("keep alone", pad))
                m = check_profile(lib, h, st, C, begin, end, np.zeros(n, np.uint8), pad=pad, what=("everything dropped", pad))
                assert not m.any()
                for first, cnt in ((5, None), (n - 1, 1), (17, 9)):          # d_seq_offs + k
                    sl = slice(first, None if cnt is None else first + cnt)
                    check_profile(lib, h, st, C, begin[sl], end[sl], keep[sl], pad=pad, first=first, n=cnt, what=("first", first, pad))
                    check_profile(lib, h, st, C, pad=pad, first=first, n=cnt, what=("first, whole", first, pad))
                # d_titles and d_title_offs are not read
                cin = st.cols_in()
                bare = lib.ColumnsIn(cin.d_bases, cin.bases_len, cin.d_quals, None, 0, cin.d_seq_offs, None, n)
                got = prof_call(lib, h, bare, C, (begin + np.uint64(pad), end + np.uint64(pad), keep))
                assert got.error is None
                same(got.profile, both, C, "no titles")
    finally:
        h.close()


# ---- accumulate ------------------------------------------------------------------------------------------------------------------
def run_accumulate(lib, sh):
    rng = np.random.default_rng(450)
    a, begin, end, keep = plan_records(rng, 48)
    n, half = a.n_records, 20
    C = 100
    whole = profile_model(a, C, begin, end, keep)
    parts = [profile_model(a, C, begin[:half], end[:half], keep[:half], 0, half), profile_model(a, C, begin[half:], end[half:], keep[half:], half, n - half)]
    assert (parts[0] + parts[1] == whole).all() and parts[0].any() and parts[1].any()
    h = handle(lib)
    try:
        with staged(lib, h, a) as st:
            acc = np.zeros(words_of(C), np.uint64)
            for k, (first, cnt) in enumerate(((0, half), (half, n - half))):
                sl = slice(first, first + cnt)
                got = prof_call(lib, h, st.cols_in(first, cnt), C, (begin[sl], end[sl], keep[sl]), accumulate=1, prior=acc)
                assert got.error is None and got.totals == [int(v) for v in parts[k][:8]], (k, got.totals)      # the call's own
                acc = got.profile
            same(acc, whole, C, "two halves")
            # onto a profile that holds something already, and large counts: 64-bit adds
            prior = rng.integers(0, 2 ** 62, words_of(C)).astype(np.uint64)
            got = prof_call(lib, h, st.cols_in(), C, (begin, end, keep), accumulate=1, prior=prior)
            assert got.error is None and got.totals == [int(v) for v in whole[:8]]
            same(got.profile, prior + whole.astype(np.uint64), C, "onto a prior")
            got = prof_call(lib, h, st.cols_in(), C, (begin, end, keep), accumulate=0, prior=prior)
            assert got.error is None and got.totals == [int(v) for v in whole[:8]]
            same(got.profile, whole, C, "accumulate = 0 overwrites")
            # no records: zeroed if accumulate == 0, untouched otherwise
            got = prof_call(lib, h, st.cols_in(3, 0), C)
            assert got.error is None and got.totals == [0] * 8 and not got.profile.any()
            got = prof_call(lib, h, st.cols_in(3, 0), C, accumulate=1, prior=prior)
            assert got.error is None and got.totals == [0] * 8 and got.untouched
    finally:
        h.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def run_arg_refusals(lib, sh):
    rng = np.random.default_rng(600)
    a, begin, end, keep = plan_records(rng, 24)
    n = a.n_records
    h = handle(lib)
    try:
        with staged(lib, h, a) as st:
            cin = st.cols_in()
            checked = 0
            for name, kw in [("n_cycles 0", dict(C=0, n_words=622)), ("n_cycles 1025", dict(C=1025)), ("accumulate 2", dict(C=64, accumulate=2))] + \
                            [("reserved[%d]" % k, dict(C=64, reserved=tuple(int(i == k) for i in range(6)))) for k in range(6)] + \
                            [("begin alone", dict(C=64, plan=(begin, None, None))), ("end alone", dict(C=64, plan=(None, end, keep)))]:
                got = prof_call(lib, h, cin, **kw)
                assert got.error is not None and got.error.code == E_ARG and got.untouched, (name, got.error)
                checked += 1
            got = prof_call(lib, h, cin, 64, null_profile=True)
            assert got.error is not None and got.error.code == E_ARG and got.untouched
            no_quals = lib.ColumnsIn(cin.d_bases, cin.bases_len, None, cin.d_titles, cin.titles_len, cin.d_seq_offs, cin.d_title_offs, n)
            got = prof_call(lib, h, no_quals, 64)
            assert got.error is not None and got.error.code == E_ARG and got.untouched
            L = lib.load()                                       # null rules, null totals
            buf = h.dev_alloc(8 * words_of(64))
            try:
                C_ = lib.C
                for rules, totals in ((None, (C_.c_uint64 * 8)()), (C_.byref(lib.ProfileRules(64)), None)):
                    rc = L.dsrcgpu_columns_profile(h.h, C_.byref(cin), None, None, None, rules, C_.c_void_p(buf), totals)
                    assert rc == E_ARG
                    checked += 1
            finally:
                h.dev_free(buf)
            assert checked == 13
            check_profile(lib, h, st, 64, begin, end, keep, what="the same handle, clean")
            check_profile(lib, h, st, MAX_CYCLES, begin, end, keep, what="the largest n_cycles")
    finally:
        h.close()
    hc = ce.handle(lib, dataclasses.replace(Config.from_levels(0, 0), color_space=True))
    try:
        with staged(lib, hc, a) as st:
            got = prof_call(lib, hc, st.cols_in(), 64)
            assert got.error is not None and got.error.code == E_ARG and got.untouched
    finally:
        hc.close()


def run_input_errors(lib, sh):
    """The plants of the adapter plan's input errors in the first, a middle and the last record, kept and dropped ones, with
    accumulate 0 and 1: code, the lowest record, d_profile as it was, and the same handle profiles the clean arrays afterwards."""
    rng = np.random.default_rng(650)
    a, begin, end, keep = plan_records(rng, 41)
    pad = 4
    n = a.n_records
    C = 151
    keep[0] = 1; keep[20] = 0; keep[40] = 0
    S = lambda r: int(a.seq_offsets[r]) + pad
    for r in (0, 20, 40):                                    # (the range plants need a base)
        assert S(r + 1) > S(r), "record %d has no bases: choose another seed" % r
    hb, he = begin + np.uint64(pad), end + np.uint64(pad)
    prior = rng.integers(0, 2 ** 40, words_of(C)).astype(np.uint64)
    h = handle(lib)
    checked = 0

    def refused(got, r, word, name):
        assert got.error is not None and got.error.code == E_INPUT and got.untouched, (name, r, got.error)
        assert "record %d:" % r in str(got.error) and word in str(got.error), (name, r, str(got.error))
    try:
        with staged(lib, h, a, pad=pad) as st:
            offs = [("order", lambda r: st.poke("seq_offs", r + 1, S(r) - 1, np.uint64), "not non-decreasing"),
                    ("end", lambda r: st.poke("seq_offs", r + 1, len(a.bases) + pad + 5, np.uint64), "above bases_len"),
                    ("wild", lambda r: st.poke("seq_offs", r + 1, 2 ** 64 - 1, np.uint64), "above bases_len")]
            for name, plant, word in offs:
                for r in (0, 20, 40):
                    plant(r)
                    if r == 0:
                        plant(40)                            # two plants: the lowest record is the one named
                    for plan in ((None, None, None), (hb, he, keep)):
                        refused(prof_call(lib, h, st.cols_in(), C, plan), r, word, name)
                        refused(prof_call(lib, h, st.cols_in(), C, plan, accumulate=1, prior=prior), r, word, name)
                    st.restore()
                    checked += 1
                check_profile(lib, h, st, C, begin, end, keep, pad=pad, what=("after", name))

            def ranged(r, b=None, e=None):
                pb, pe = hb.copy(), he.copy()
                if b is not None: pb[r] = b
                if e is not None: pe[r] = e
                return pb, pe
            ranges = [("begin low", lambda r: dict(b=S(r) - 1), "d_begin lies below"),
                      ("end high", lambda r: dict(e=S(r + 1) + 1), "d_end lies above"),
                      ("end wild", lambda r: dict(e=2 ** 64 - 1), "d_end lies above"),
                      ("begin above end", lambda r: dict(b=S(r + 1), e=S(r + 1) - 1), "d_begin lies above d_end")]
            for name, how, word in ranges:
                for r in (0, 20, 40):
                    pb, pe = ranged(r, **how(r))
                    if r == 0:
                        pb[40] = S(40) - 1                   # a second plant further up
                    for k in (keep, None):
                        refused(prof_call(lib, h, st.cols_in(), C, (pb, pe, k)), r, word, name)
                    refused(prof_call(lib, h, st.cols_in(), C, (pb, pe, keep), accumulate=1, prior=prior), r, word, name)
                    checked += 1
                check_profile(lib, h, st, C, begin, end, keep, pad=pad, what=("after", name))
    finally:
        h.close()
    assert checked == 21


def run_codec_state(lib, sh):
    """The call touches nothing the codec carries, as run_codec_state of the adapter cases: the fields capacity stays, a pending
    record layout stays pending, and the text call that follows writes what it writes on a fresh handle seeded alike."""
    a, begin, end, keep = plan_records(np.random.default_rng(660), 80)
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
            with staged(lib, h, a) as st:
                check_profile(lib, h, st, 151, begin, end, keep)
                check_profile(lib, h, st, MAX_CYCLES)
                assert h.get_fields_capacity() == 11
            assert text_blocks(h) == text_blocks(fresh), layout
        finally:
            h.close(); fresh.close()


# ---- record counts ---------------------------------------------------------------------------------------------------------------
def run_count(lib, sh, n_rec, C=8):
    """n_rec reads of 10 bases under a plan, n_cycles below the read length.  The model runs on the first 2049 records at the most;
    behind them the same records repeat under the same plan, and the profile is a sum."""
    base = min(n_rec, 2049)
    rng = np.random.default_rng(700 + n_rec)
    x = rng.integers(0, 4, (base, 10)).astype(np.uint8); x[rng.random((base, 10)) < 0.05] = 4
    q = rng.integers(0, 42, (base, 10)).astype(np.uint8)
    cut5, cut3 = rng.integers(0, 3, base).astype(np.uint64), rng.integers(0, 3, base).astype(np.uint64)
    keep0 = (rng.random(base) < 0.8).astype(np.uint8)
    mk = lambda xx, qq: Arrays(xx.reshape(-1), qq.reshape(-1), np.zeros(0, np.uint8), (10 * np.arange(len(xx) + 1)).astype(np.uint64),
                               np.zeros(len(xx) + 1, np.uint64), [0, len(xx)])
    S0 = (10 * np.arange(base + 1)).astype(np.uint64)
    full = profile_model(mk(x, q), C, S0[:-1] + cut5, S0[1:] - cut3, keep0)
    reps, rest = divmod(n_rec, base)
    part = profile_model(mk(x[:rest], q[:rest]), C, (S0[:-1] + cut5)[:rest], (S0[1:] - cut3)[:rest], keep0[:rest]) if rest else 0
    m = reps * full + part
    idx = np.concatenate([np.arange(base)] * reps + [np.arange(rest)]).astype(np.int64)
    S = (10 * np.arange(n_rec + 1)).astype(np.uint64)
    a = mk(x[idx], q[idx])
    begin, end, keep = S[:-1] + cut5[idx], S[1:] - cut3[idx], keep0[idx]
    assert int(m[0]) == int((keep != 0).sum()) and (n_rec < 63 or C >= 10 or int(tables(m, C)[1][C - 1].sum()) > int(m[0]) // 2)      # folded bases
    h = handle(lib)
    try:
        with staged(lib, h, a) as st:
            check_profile(lib, h, st, C, begin, end, keep, what=n_rec, model=m)
            if n_rec <= 2049:
                check_profile(lib, h, st, C, what=(n_rec, "whole reads"))
    finally:
        h.close()


def run_stride(lib, sh, C, n_rec):
    """A record count above the grid the kernel uses at C cycles (max_grid(C) workgroups of 16 waves): the stride's second round."""
    assert n_rec > max_grid(C) * 16
    run_count(lib, sh, n_rec, C=C)


def run_no_wrap(lib, sh):
    """One record of 2^24 + 5 bases, all of quality 255, n_cycles = 1: the case as the issue states it -- 34 MB of input, one launch,
    and a record above 2^24 bases, where the kernel sums and divides in 64 bits.  The issue gives its quality sum as above 2^32; it
    is not: 255 * (2^24 + 5) = 4 278 191 355 and 2^32 = 4 294 967 296.  So a second record of 2^24 + 2^17 bases follows, profiled by
    a launch of its own, whose sum in the one cycle is 4 311 613 440: that one a 32-bit partial could not hold."""
    lens = [2 ** 24 + 5, 2 ** 24 + 2 ** 17]
    assert 255 * lens[0] < 2 ** 32 < 255 * lens[1]
    total = sum(lens)
    a = Arrays(np.full(total, 1, np.uint8), np.full(total, 255, np.uint8), np.zeros(0, np.uint8), np.array([0, lens[0], total], np.uint64),
               np.zeros(3, np.uint64), [0, 2])

    def closed(n):                                           # the serial rule in closed form: every position gives the same adds
        m = np.zeros(words_of(1), np.int64)
        tot, base, qsum, qhist, length, gc, meanq = tables(m, 1)
        tot[:] = [1, n, n, n, 255 * n, n, 0, 0]
        base[0, 1] = n; qsum[0, 1] = 255 * n; qhist[255] = n; length[1] = 1; gc[100] = 1; meanq[255] = 1
        return m
    small = arrays_from([(np.full(70, 1, np.uint8), np.full(70, 255, np.uint8))])        # ... which the model confirms on 70 bases
    assert (profile_model(small, 1) == closed(70)).all()
    h = handle(lib)
    try:
        with staged(lib, h, a) as st:
            for k, n in enumerate(lens):
                check_profile(lib, h, st, 1, first=k, n=1, what=("no wrap", n), model=closed(n))
    finally:
        h.close()


# ---- fuzz ------------------------------------------------------------------------------------------------------------------------
def fuzz_case(seed, n_rec):
    """Lengths 0 .. 300 (a few up to 1500), random codes, qualities, plans, keep flags and n_cycles (some below the lengths)."""
    rng = np.random.default_rng(4000 + seed)
    reads = []
    for r in range(n_rec):
        n = int(rng.integers(0, 301)) if rng.random() < 0.97 else int(rng.integers(300, 1501))
        reads.append(random_read((0, 1400)[r] if r < 2 else n, rng, special=0.05))      # (the first two: no bases, and more than any n_cycles)
    a = arrays_from(reads)
    S = a.seq_offsets.astype(np.int64)
    lens = S[1:] - S[:-1]
    whole = rng.random(n_rec) < 0.5
    cut5 = np.where(whole, 0, (rng.random(n_rec) * (lens + 1) * 0.2).astype(np.int64))
    cut3 = np.where(whole, 0, (rng.random(n_rec) * (lens - cut5 + 1) * 0.2).astype(np.int64))
    keep = np.where(rng.random(n_rec) < 0.85, rng.integers(1, 256, n_rec), 0).astype(np.uint8)
    keep[:2] = 1
    C = [1, 37, 150, 151, 256, 257, 300, 1024][seed % 8]
    return a, (S[:-1] + cut5).astype(np.uint64), (S[1:] - cut3).astype(np.uint64), keep, C


def run_fuzz(lib, sh, seed):
    n_rec = sh["prof_fuzz"][1]
    a, begin, end, keep, C = fuzz_case(seed, n_rec)
    m = profile_model(a, C, begin, end, keep)
    lens = (end - begin)[keep != 0]
    print("profile fuzz", seed, "n_cycles", C, "records", n_rec, "totals", dict(zip(TOTALS, (int(v) for v in m[:8]))))
    assert (lens == 0).any() and (lens > C).any() and int(m[6]) > 0
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=3) as st:
            check_profile(lib, h, st, C, begin, end, keep, pad=3, what=("fuzz", seed), model=m)
            check_profile(lib, h, st, C, pad=3, what=("fuzz, whole reads", seed))
    finally:
        h.close()


# ---- the Python layers -------------------------------------------------------------------------------------------------------------
tensors = ca.tensors


def views_equal(prof, m, C):
    """The views of a ColumnsProfile against the tables of the model."""
    t = tables(m, C)
    got = (prof.totals, prof.base_by_cycle, prof.quality_sum_by_cycle, prof.quality_hist, prof.length_hist, prof.gc_hist, prof.mean_quality_hist)
    assert prof.n_cycles == C and prof.data.dtype == torch.int64 and prof.data.numel() == words_of(C)
    assert all(tuple(g.shape) == w.shape and np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, t)), "a view differs from the model"
    assert all(g.data_ptr() >= prof.data.data_ptr() and g.device == prof.data.device for g in got)       # views, not copies
    assert prof.summary() == dict(zip(TOTALS, (int(v) for v in t[0])))


def run_python_layers(lib, sh, device):
    from dsrc_amd import columns
    a, begin, end, keep, _ = fuzz_case(3, 120)
    S = a.seq_offsets.astype(np.int64)
    longest = int((S[1:] - S[:-1]).max())
    t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v).astype(dt)).to(device)
    h = handle(lib)
    try:
        assert tuple(lib.PROFILE_TOTALS) == TOTALS and lib.PROFILE_MAX_CYCLES == MAX_CYCLES and lib.profile_words(151) == words_of(151)
        c = tensors(a, device)
        tb, te, tk = t(begin, np.int64), t(end, np.int64), t(keep, np.uint8)
        p = columns.profile_columns(h, c)                    # n_cycles=None: the longest stored read, clipped
        assert p.data.device.type == torch.device(device).type
        views_equal(p, profile_model(a, min(longest, MAX_CYCLES)), min(longest, MAX_CYCLES))
        short = ca.arrays_from_bases([np.zeros(5, np.uint8), np.zeros(0, np.uint8)])
        assert columns.profile_columns(h, tensors(short, device)).n_cycles == 5
        assert columns.profile_columns(h, tensors(ca.arrays_from_bases([np.zeros(0, np.uint8)]), device)).n_cycles == 1
        for C in (1, 100, 1024):
            views_equal(columns.profile_columns(h, c, tb, te, tk, n_cycles=C), profile_model(a, C, begin, end, keep), C)
        views_equal(columns.profile_columns(h, c, keep=tk != 0, n_cycles=64), profile_model(a, 64, keep=keep), 64)      # a bool keep
        assert torch.equal(tb, t(begin, np.int64)) and torch.equal(tk, t(keep, np.uint8))                              # inputs as they were
        # into=: the two halves of the batch sum to the whole
        half = 50
        first = tensors(Arrays(a.bases, a.quals, a.titles, a.seq_offsets[: half + 1], a.title_offsets[: half + 1], [0, half]), device)
        rest = tensors(Arrays(a.bases, a.quals, a.titles, a.seq_offsets[half:], a.title_offsets[half:], [0, a.n_records - half]), device)
        p1 = columns.profile_columns(h, first, tb[:half], te[:half], tk[:half], n_cycles=100)
        ptr = p1.data.data_ptr()
        p2 = columns.profile_columns(h, rest, tb[half:], te[half:], tk[half:], into=p1)
        assert p2 is p1 and p1.data.data_ptr() == ptr
        views_equal(p1, profile_model(a, 100, begin, end, keep), 100)
        columns.profile_columns(h, rest, tb[half:], te[half:], tk[half:], n_cycles=100, into=p1)
        views_equal(p1, profile_model(a, 100, begin, end, keep) + profile_model(a, 100, begin[half:], end[half:], keep[half:], half), 100)

        class Never:                                         # ValueError comes before any library call
            def __getattr__(self, name):
                raise AssertionError("the library was called")
        p64 = columns.profile_columns(h, c, n_cycles=64)
        bad_calls = [dict(n_cycles=0), dict(n_cycles=1025), dict(n_cycles=64.0), dict(n_cycles=True), dict(begin=tb), dict(end=te), dict(begin=tb[:5], end=te[:5]),
                     dict(keep=tk[:7]), dict(into=p64, n_cycles=65), dict(into=p64.data), dict(into=columns.ColumnsProfile(p64.data[:-1], 64)),
                     dict(into=columns.ColumnsProfile(p64.data.to(torch.int32), 64))]
        if torch.device(device).type != "cpu":
            bad_calls += [dict(keep=tk.cpu()), dict(into=columns.ColumnsProfile(p64.data.cpu(), 64))]
        for bad in bad_calls:
            try:
                columns.profile_columns(Never(), c, **bad)
            except ValueError:
                pass
            else:
                raise AssertionError("no ValueError for %r" % (list(bad),))
    finally:
        h.close()


def run_plan_equals_selection(lib, sh, device):
    """With (begin, end, keep) from trim_plan: the profile of the plan on the columns == the profile of the selection, word for word."""
    from dsrc_amd import columns
    a, _, _ = ca.filter_reads(200)
    trim = cs.rules_of(15, 20, min_length=30, max_n=2, min_mean_quality=20)
    h = handle(lib)
    try:
        c = tensors(a, device)
        b, e, k, stats = columns.trim_plan(h, c, **trim)
        assert 0 < stats["records_kept"] < 200 and stats["bases_cut"] > 0
        sel = columns.select_columns(h, c, b, e, k)
        for C in (1, 90, 130):
            planned, selected = columns.profile_columns(h, c, b, e, k, n_cycles=C), columns.profile_columns(h, sel, n_cycles=C)
            assert torch.equal(planned.data, selected.data), C
            mb, me, mk, _ = cs.plan_model(a, trim)
            views_equal(planned, profile_model(a, C, mb, me, mk), C)
            assert planned.summary()["records"] == stats["records_kept"] and planned.summary()["bases"] == stats["bases_kept"]
    finally:
        h.close()


def selected_arrays(a, b, e, k):
    w = cs.select_model(a, b, e, k)
    return Arrays(w[0], w[1], w[2], w[3], w[4], [0, len(w[3]) - 1])


def run_filter_columns(lib, sh, device):
    """filter_columns(profile=True): before == the model on the input, after == the model on the OUTPUT records; without `profile`
    (and with profile=False) the function returns what it returned before it knew the word."""
    from dsrc_amd import columns
    a, _, _ = ca.filter_reads(200)
    trim = cs.rules_of(15, 20, min_length=30, max_n=2, min_mean_quality=20)
    S = a.seq_offsets.astype(np.int64)
    C = int((S[1:] - S[:-1]).max())
    same_cols = lambda sel, want: all(np.array_equal(g.cpu().numpy().astype(w.dtype), w) for g, w in
                                      zip((sel.bases, sel.quals, sel.titles, sel.seq_offsets, sel.title_offsets), want[:5]))
    h = handle(lib)
    try:
        c = tensors(a, device)
        for ads in (None, [ca.ADAPTER]):
            if ads is None:
                b, e, k, ts = cs.plan_model(a, trim)
                wstats = dict(zip(ca.TRIM_STATS, ts))
            else:
                b, e, k, wstats = ca.filter_model(a, trim, ads)
            want = cs.select_model(a, b, e, k)
            for kw in ({}, dict(profile=False)):
                sel, stats = columns.filter_columns(h, c, adapters=ads, **kw, **trim)
                assert stats == wstats and list(stats) == list(wstats) and same_cols(sel, want), (ads, kw)
            sel, stats = columns.filter_columns(h, c, adapters=ads, profile=True, **trim)
            assert same_cols(sel, want) and list(stats) == list(wstats) + ["profile_before", "profile_after"]
            assert {key: v for key, v in stats.items() if not key.startswith("profile_")} == wstats
            views_equal(stats["profile_before"], profile_model(a, C), C)
            out = selected_arrays(a, b, e, k)
            assert 0 < out.n_records < 200 and len(out.bases) < len(a.bases)
            views_equal(stats["profile_after"], profile_model(out, C), C)
    finally:
        h.close()


def run_filter_pairs(lib, sh, device):
    """filter_pairs(profile=True): per side, before == the model on that side's input, after == the model on that side's output
    records; without `profile` the function returns what it returned before."""
    from dsrc_amd import columns
    (a1, _, _), (a2, _, _) = cp.paired_reads(160)
    trim = cs.rules_of(0, 20, min_length=30, max_n=2)
    kw = dict(pair_min_overlap=20, pair_max_mismatches=4, pair_max_error_permille=150)
    same_cols = lambda sel, want: all(np.array_equal(g.cpu().numpy().astype(w.dtype), w) for g, w in
                                      zip((sel.bases, sel.quals, sel.titles, sel.seq_offsets, sel.title_offsets), want[:5]))
    h = handle(lib)
    try:
        c1, c2 = tensors(a1, device), tensors(a2, device)
        for overlap in (True, False):
            r1, r2, keep, wstats = cp.pairs_model(a1, a2, trim, (None, None), overlap, cp.rules_of(20, 4, 150))
            w1, w2 = cs.select_model(a1, r1[0], r1[1], keep), cs.select_model(a2, r2[0], r2[1], keep)
            for extra in ({}, dict(profile=False)):
                o1, o2, stats = columns.filter_pairs(h, c1, c2, overlap=overlap, **extra, **kw, **trim)
                assert stats == wstats and list(stats) == list(wstats) and same_cols(o1, w1) and same_cols(o2, w2), (overlap, extra)
            o1, o2, stats = columns.filter_pairs(h, c1, c2, overlap=overlap, profile=True, **kw, **trim)
            assert same_cols(o1, w1) and same_cols(o2, w2) and list(stats) == list(wstats)
            for name, a, (b, e) in (("read1", a1, r1), ("read2", a2, r2)):
                side = stats[name]
                assert {key: v for key, v in side.items() if not key.startswith("profile_")} == wstats[name]
                assert list(side)[-2:] == ["profile_before", "profile_after"]
                views_equal(side["profile_before"], profile_model(a, 100), 100)
                out = selected_arrays(a, b, e, keep)
                assert 0 < out.n_records < 160
                views_equal(side["profile_after"], profile_model(out, 100), 100)
            if overlap:
                assert stats["pair"] == wstats["pair"]
    finally:
        h.close()
