"""Shared by tests/test_emu_columns_pair.py (CPU, emulator build) and tests/test_gpu_columns_pair.py (MI355X): the cases of the
columnar pair plan (dsrcgpu_columns_pair_plan; dsrc_amd/csrc/k_columns_pair.h) and what they must give.

The reference has no counterpart, so the yardstick is the integer model written out here: pair_search() is the serial rule of
include/dsrc_gpu.h word for word (forward shifts first, then read-through shifts, a Hamming count under two budgets), pair_model()
applies it to two plans and counts the eleven statistics.  None of it comes from the library under test, and every comparison is
exact equality.  Output arrays are filled with 0xA5 before a call, so that "nothing written" can be asserted.  Before the library is
compared on a crafted case the model alone is asked what that case is for.

Two ways to make a pair.  insert_pair() is the natural one: an insert, read 1 reads it from the left and runs into an adapter, read 2
reads its reverse complement -- the true insert size is known and is what the plan must find.  crafted_xy() builds x and y (the
reverse complement of read 2) directly over disjoint alphabets, x over {A, G} and y over {C, T}, and copies x into y only where the
wanted candidate compares them: no other candidate in front of it can be accepted at rate 0, whatever min_overlap is, so the winner is
known exactly even for an overlap of one base.

Shapes.  The emulator pays a coroutine switch per wave exchange, so its fuzz is 2 seeds x 120 pairs where the GPU runs 6 x 1200.  The
planner's grid holds at most 4096 workgroups of WG / 64 waves: with workgroups of 1024 threads a count above 65536 pairs takes the
grid stride into a second round -- that count runs on the GPU only.  run_second_pair_of_a_wave needs one stride of pairs on either
build (the emulator's workgroups have 256 threads, so its stride is 16384 pairs); nearly all of them are one base long."""
from __future__ import annotations

import dataclasses

import numpy as np
import torch        # noqa: F401  before the first handle (see columns_cases)

from tests import columns_adapt_cases as ca
from tests import columns_cases as cc
from tests import columns_enc_cases as ce
from tests import columns_sel_cases as cs
from tests._oracle import Config
from tests.cases import TINY

E_ARG, E_INPUT = cs.E_ARG, cs.E_INPUT
NO_INSERT = 2 ** 64 - 1
MAX_BASES = 1024

SHAPES = {
    "gpu": dict(cc.SHAPES["gpu"], pair_fuzz=(6, 1200), counts=[1, 63, 64, 65, 2049], stride_count=4096 * 16 + 4001, wave_stride=4096 * 16),
    "emu": dict(cc.SHAPES["emu"], pair_fuzz=(2, 120), counts=[1, 63, 64, 65, 2049], stride_count=None, wave_stride=4096 * 4),
}
Arrays = ce.Arrays
Dev = cs.Dev
LENGTHS = [0, 1, 29, 30, 31, 63, 64, 65, 127, 128, 129, 150, 1023, 1024]
SHIFTS = [0, 1, -1, 62, -62, 63, -63, 64, -64, 65, -65]
PAIR_STATS = ("pairs_kept", "bases_kept_1", "bases_kept_2", "bases_cut_1", "bases_cut_2", "overlap_found", "overlap_narrowed", "dropped_mate",
              "dropped_length", "not_searched_long", "insert_sum")
arrays_from_bases = ca.arrays_from_bases


# ---- the model -------------------------------------------------------------------------------------------------------------------
def rules_of(min_overlap=30, max_mm=5, rate=200, min_length=1):
    return dict(min_overlap=min_overlap, max_mm=max_mm, rate=rate, min_length=min_length)


def _xy(x, z):
    """Read 1's range x and read 2's range z as stored -> x and y as integers in which a code >= 4 equals nothing."""
    x = np.asarray(x).astype(np.int64); zr = np.asarray(z)[::-1].astype(np.int64)
    return np.where(x < 4, x, -2), np.where(zr < 4, 3 - zr, -1)


def overlap_of(xx, y, d):
    """(L, mm) of the shift d."""
    n1, n2 = len(xx), len(y)
    if d >= 0:
        L = min(n1 - d, n2)
        return L, int(np.count_nonzero(xx[d: d + L] != y[:L]))
    L = min(n1, n2 + d)
    return L, int(np.count_nonzero(xx[:L] != y[-d: -d + L]))


def accepts(x, z, d, rules):
    xx, y = _xy(x, z)
    L, mm = overlap_of(xx, y, d)
    return L >= rules["min_overlap"] and mm <= rules["max_mm"] and mm * 1000 <= L * rules["rate"]


def pair_search(x, z, rules):
    """The serial rule on read 1's range x and read 2's range z (numpy uint8, as stored) -> the shift d found, or None."""
    xx, y = _xy(x, z)
    n1, n2 = len(xx), len(y)
    for d in list(range(n1)) + [-k for k in range(1, n2)]:           # the first accepted d wins
        L = min(n1 - d, n2) if d >= 0 else min(n1, n2 + d)
        if L < rules["min_overlap"]:
            continue
        mm = overlap_of(xx, y, d)[1]
        if mm <= rules["max_mm"] and mm * 1000 <= L * rules["rate"]:
            return d
    return None


def candidate_of(d, n1):
    """The place of shift d in the rule's order."""
    return d if d >= 0 else n1 - d - 1


def pair_model(a1: Arrays, a2: Arrays, rules, plan1=(None, None, None), plan2=(None, None, None), first=0, n=None):
    """Plans in (positions in a<s>.bases of records first .. first + n - 1) -> begin1, end1, begin2, end2, keep, insert, stats[11]."""
    assert a1.n_records == a2.n_records
    n = a1.n_records - first if n is None else n
    S = [[int(v) for v in a.seq_offsets] for a in (a1, a2)]
    out = [np.zeros(n, np.uint64) for _ in range(4)]
    ok, oi = np.zeros(n, np.uint8), np.full(n, NO_INSERT, np.uint64)
    stats = [0] * 11
    for k in range(n):
        r = first + k
        side = []
        for s, (a, (begin, end, keep)) in enumerate(((a1, plan1), (a2, plan2))):
            b, e = (S[s][r], S[s][r + 1]) if begin is None else (int(begin[k]), int(end[k]))
            assert S[s][r] <= b <= e <= S[s][r + 1]
            side.append((b, e, b - S[s][r], 1 if keep is None else int(keep[k] != 0)))
        (b1, e1, f1, k1), (b2, e2, f2, k2) = side
        n1, n2 = e1 - b1, e2 - b2
        m1, m2 = n1, n2
        if k1 and k2:
            if n1 > MAX_BASES or n2 > MAX_BASES:
                stats[9] += 1
            else:
                d = pair_search(a1.bases[b1:e1], a2.bases[b2:e2], rules)
                if d is not None:
                    I = d + n2 + f1 + f2
                    m1, m2 = min(n1, I - f1), min(n2, I - f2)
                    assert m1 >= 1 and m2 >= 1
                    oi[k] = I
                    stats[5] += 1; stats[10] += I
                    if m1 < n1 or m2 < n2:
                        stats[6] += 1
            if m1 >= rules["min_length"] and m2 >= rules["min_length"]:
                ok[k] = 1
                stats[0] += 1; stats[1] += m1; stats[2] += m2; stats[3] += n1 - m1; stats[4] += n2 - m2
            else:
                stats[8] += 1
        elif k1 != k2:
            stats[7] += 1
        out[0][k], out[1][k], out[2][k], out[3][k] = b1, b1 + m1, b2, b2 + m2
    return out[0], out[1], out[2], out[3], ok, oi, stats


# ---- pairs -----------------------------------------------------------------------------------------------------------------------
ADAPTER_1 = ca.codes_of("AGATCGGAAGAGCACACGTCTGAACTCCAGTCA")       # public Illumina TruSeq sequences: what read 1 / read 2 run into
ADAPTER_2 = ca.codes_of("AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT")


def revcomp(x):
    x = np.asarray(x, np.uint8)
    assert (x < 4).all()
    return (3 - x[::-1]).astype(np.uint8)


def insert_pair(insert, len1, len2, rng):
    """read 1 = insert + adapter 1 + random bases, read 2 = revcomp(insert) + adapter 2 + random bases, cut to len1 / len2."""
    tail = lambda: rng.integers(0, 4, 2048).astype(np.uint8)
    return (np.concatenate((insert, ADAPTER_1, tail()))[:len1].astype(np.uint8),
            np.concatenate((revcomp(insert), ADAPTER_2, tail()))[:len2].astype(np.uint8))


def crafted_xy(n1, n2, d, rng):
    """-> read 1, read 2 of n1 / n2 bases (n1, n2 >= 1, d a candidate) in which the shift d compares equal bases throughout and every
    candidate in front of it meets a mismatch: x over {A, G}, y over {C, T} but for the copy; forward: x[: d] = A and x[d] = G, so that
    an earlier forward shift compares an A with y[0] = G."""
    assert n1 >= 1 and n2 >= 1 and -(n2 - 1) <= d <= n1 - 1
    x = (2 * rng.integers(0, 2, n1)).astype(np.uint8)
    y = (1 + 2 * rng.integers(0, 2, n2)).astype(np.uint8)
    if d >= 0:
        x[:d] = 0; x[d] = 2
        L = min(n1 - d, n2)
        y[:L] = x[d: d + L]
    else:
        L = min(n1, n2 + d)
        y[-d: -d + L] = x[:L]
    return x, revcomp(y)


def y_index(n2, j):
    """Where in read 2 (as stored) position j of y lies."""
    return n2 - 1 - j


# ---- one call ----------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Got:
    error: object
    stats: object
    ranges: list            # begin1, end1, begin2, end2
    keep: np.ndarray
    insert: np.ndarray
    untouched: bool


def lib_rules(lib, rules, reserved=(0, 0, 0, 0)):
    return lib.PairRules(rules["min_overlap"], rules["max_mm"], rules["rate"], rules["min_length"], reserved)


def pair_call(lib, h, cin1, cin2, n, pr, plan1=(None, None, None), plan2=(None, None, None), inplace=False, keep_alias=None, insert=True,
              null_out=None):
    """One dsrcgpu_columns_pair_plan.  plan<s>: begin / end / keep as numpy in the coordinates of the staged arrays, or None.  Fresh
    outputs are 0xA5-filled; inplace: every range output that has an input counterpart IS that input; keep_alias 1 / 2: d_keep is that
    side's incoming keep; null_out: the index (0 .. 4) of an output passed as NULL."""
    with Dev(h) as d:
        up = lambda plan: [None if v is None else d.up(np.ascontiguousarray(v).astype(dt).tobytes()) for v, dt in zip(plan, (np.uint64, np.uint64, np.uint8))]
        p1, p2 = up(plan1), up(plan2)
        sizes = (8 * n, 8 * n, 8 * n, 8 * n, n)
        fresh = [d.fill(s) for s in sizes]
        ins = [p1[0], p1[1], p2[0], p2[1], {None: None, 1: p1[2], 2: p2[2]}[keep_alias]]
        use_in = [inplace and ins[i] is not None for i in range(4)] + [ins[4] is not None]
        out = [ins[i] if use_in[i] else fresh[i] for i in range(5)]
        pi = d.fill(8 * n)
        arg = [None if i == null_out else out[i] for i in range(5)]
        err = stats = None
        try:
            stats = h.columns_pair_plan(cin1, cin2, pr, tuple(p1), tuple(p2), arg[0], arg[1], arg[2], arg[3], arg[4], pi if insert else None)
        except lib.DsrcGpuError as e:
            err = e
        raw = [d.down(p, s) for p, s in zip(out, sizes)] + [d.down(pi, 8 * n)]
        raw_fresh = [d.down(p, s) for p, s in zip(fresh, sizes)] + [raw[5]]
        raw_plans = [[None if p is None else d.down(p, s)[:s] for p, s in zip(pl, (8 * n, 8 * n, n))] for pl in (p1, p2)]
    assert all(r[-8:] == b"\xA5" * 8 for r in raw + raw_fresh), "written behind the end of an output array"
    assert all(raw_fresh[i] == b"\xA5" * len(raw_fresh[i]) for i in range(5) if use_in[i]), "an output that was not given has been written"
    if not insert:
        assert raw[5] == b"\xA5" * len(raw[5]), "d_insert was not given"
    got = Got(err, stats, [np.frombuffer(raw[i], np.uint64)[:n] for i in range(4)], np.frombuffer(raw[4], np.uint8)[:n],
              np.frombuffer(raw[5], np.uint64)[:n], all(r == b"\xA5" * len(r) for r in raw_fresh))
    got.plans_after = raw_plans
    return got


def check_pair(lib, h, st1, st2, rules, plan1=(None, None, None), plan2=(None, None, None), pad=(0, 0), first=0, n=None, what=None, model=None,
               **how):
    """Arrays staged in st1 / st2, the plans as positions in the UNPADDED arrays (the pads are added here) -> the call == the model."""
    n = st1.a.n_records - first if n is None else n
    m = model if model is not None else pair_model(st1.a, st2.a, rules, plan1, plan2, first, n)
    shift = lambda plan, p: tuple(None if v is None else np.asarray(v).astype(np.uint64) + np.uint64(p) for v in plan[:2]) + (plan[2],)
    got = pair_call(lib, h, st1.cols_in(first, n), st2.cols_in(first, n), n, lib_rules(lib, rules), shift(plan1, pad[0]), shift(plan2, pad[1]), **how)
    assert got.error is None, (what, got.error)
    pads = (pad[0], pad[0], pad[1], pad[1])
    bad = got.keep != m[4]
    for i in range(4):
        bad = bad | (got.ranges[i] != m[i] + np.uint64(pads[i]))
    if how.get("insert", True):
        bad = bad | (got.insert != m[5])
    bad = np.nonzero(bad)[0]
    if len(bad):
        r = int(bad[0])
        raise AssertionError((what, "pair", r, [int(got.ranges[i][r]) - pads[i] for i in range(4)], int(got.keep[r]), int(got.insert[r]),
                              "want", [int(m[i][r]) for i in range(4)], int(m[4][r]), int(m[5][r]), len(bad)))
    assert got.stats == m[6], (what, got.stats, m[6])
    return m


def handle(lib):
    return ce.handle(lib, Config.from_levels(0, 0))


def staged(lib, h, a, pad=0):
    return cs.staged(lib, h, a, pad)


def found_d(a1, a2, m, r, plan1=None, plan2=None):
    """The shift the model found in pair r (whole reads unless the plans are given), None for none."""
    if int(m[5][r]) == NO_INSERT:
        return None
    f1 = int(m[0][r]) - int(a1.seq_offsets[r]); f2 = int(m[2][r]) - int(a2.seq_offsets[r])
    n2 = (int(plan2[1][r]) - int(plan2[0][r])) if plan2 is not None else int(a2.seq_offsets[r + 1]) - int(a2.seq_offsets[r])
    return int(m[5][r]) - n2 - f1 - f2


# ---- geometry --------------------------------------------------------------------------------------------------------------------
def length_pairs(k):
    """The k-th third of the length pairs: every length against itself, against 150 on the other side, and 150 against it."""
    return [[(n, n) for n in LENGTHS], [(n, 150) for n in LENGTHS] + [(1023, 1024)], [(150, n) for n in LENGTHS] + [(1024, 1023)]][k]


def geometry_pairs(pairs, min_overlap, rng):
    """Crafted pairs for the shifts of SHIFTS, the last shift of either branch at which L == min_overlap and the one beyond it, and the
    candidates 0, 63, 64, n1 - 1, n1, n1 + 1 -> reads 1, reads 2, [(n1, n2, d, L)]."""
    r1, r2, want = [], [], []
    for n1, n2 in pairs:
        if n1 == 0 or n2 == 0:
            r1.append(np.zeros(n1, np.uint8)); r2.append(np.full(n2, 3, np.uint8)); want.append((n1, n2, None, 0))
            continue
        cands = {c for c in (0, 63, 64, n1 - 1, n1, n1 + 1) if 0 <= c < n1 + n2 - 1}
        shifts = set(SHIFTS) | {n1 - min_overlap, n1 - min_overlap + 1, -(n2 - min_overlap), -(n2 - min_overlap + 1)}
        shifts |= {c if c < n1 else -(c - n1 + 1) for c in cands}
        for d in sorted(shifts):
            if not -(n2 - 1) <= d <= n1 - 1:
                continue
            x, z = crafted_xy(n1, n2, d, rng)
            r1.append(x); r2.append(z); want.append((n1, n2, d, min(n1 - d, n2) if d >= 0 else min(n1, n2 + d)))
    return r1, r2, want


def run_geometry(lib, sh, k):
    rng = np.random.default_rng(100 + k)
    h = handle(lib)
    try:
        for min_overlap in (30, 1):
            r1, r2, want = geometry_pairs(length_pairs(k), min_overlap, rng)
            a1, a2 = arrays_from_bases(r1), arrays_from_bases(r2)
            rules = rules_of(min_overlap, 0, 0, 0)
            m = pair_model(a1, a2, rules)
            n_found = n_short = 0
            for r, (n1, n2, d, L) in enumerate(want):        # the model alone: the wanted shift where its overlap suffices, else none
                got = found_d(a1, a2, m, r)
                if d is not None and L >= min_overlap:
                    assert got == d, (k, min_overlap, r, n1, n2, d, L, got)
                    assert int(m[5][r]) == d + n2 and int(m[1][r] - m[0][r]) == min(n1, d + n2) and int(m[3][r] - m[2][r]) == min(n2, d + n2)
                    n_found += 1
                else:
                    assert got is None, (k, min_overlap, r, n1, n2, d, L, got)
                    n_short += d is not None
            assert n_found > 50 and (min_overlap == 1 or n_short > 10), (n_found, n_short)
            if min_overlap == 30:                            # the last shift with L == min_overlap on both branches, and one beyond
                Ls = {(d >= 0, L) for _, _, d, L in want if d is not None}
                assert {(True, 30), (True, 29), (False, 30), (False, 29)} <= Ls
            with staged(lib, h, a1) as st1, staged(lib, h, a2) as st2:
                check_pair(lib, h, st1, st2, rules, what=("geometry", k, min_overlap), model=m)
    finally:
        h.close()


# ---- budget ------------------------------------------------------------------------------------------------------------------------
RATES = [0, 200, 334, 1000]
MAX_MMS = [0, 5, 2000]


def mismatch_positions(L, count):
    """`count` overlap positions to spoil: 0, 63, 64 and L - 1 first, then from the middle."""
    first = [v for v in (0, L - 1, 63, 64) if 0 <= v < L]
    order = list(dict.fromkeys(first + list(range(L // 2, L)) + list(range(L // 2))))
    return sorted(order[:count])


def spoiled_pair(n1, n2, d, positions, rng):
    """crafted_xy with mismatches at the given overlap positions (y gets the other base of its own alphabet there)."""
    x, z = crafted_xy(n1, n2, d, rng)
    for i in positions:
        j = i if d >= 0 else i - d
        z[y_index(n2, j)] = 3 - (1 + 2 * int(rng.integers(0, 2)))      # y[j] = C or T: x holds A or G
    return x, z


def run_budget(lib, sh, rate):
    rng = np.random.default_rng(200 + rate)
    h = handle(lib)
    try:
        for max_mm in MAX_MMS:
            rules = rules_of(30, max_mm, rate, 0)
            r1, r2, want = [], [], []
            for n1, n2, d in ((150, 150, 20), (150, 150, -40), (150, 140, 120), (200, 150, -86), (1024, 1024, 0)):
                L = min(n1 - d, n2) if d >= 0 else min(n1, n2 + d)
                k = min(max_mm, L * rate // 1000)
                for count in (k, k + 1):
                    if count > L:
                        continue
                    x, z = spoiled_pair(n1, n2, d, mismatch_positions(L, count), rng)
                    r1.append(x); r2.append(z); want.append((n1, d, L, count <= k))
            a1, a2 = arrays_from_bases(r1), arrays_from_bases(r2)
            m = pair_model(a1, a2, rules)
            for r, (n1, d, L, ok) in enumerate(want):        # exactly the budget: found there; one more: not there and nowhere in front
                got = found_d(a1, a2, m, r)
                if ok:
                    assert got is not None and candidate_of(got, n1) <= candidate_of(d, n1), (rate, max_mm, r, d, L, got)
                    assert got == d or (rate == 1000 and max_mm == 2000), (rate, max_mm, r, d, L, got)
                else:
                    assert got is None or candidate_of(got, n1) > candidate_of(d, n1), (rate, max_mm, r, d, L, got)
            assert any(ok for *_, ok in want) and (any(not ok for *_, ok in want) or (rate == 1000 and max_mm == 2000))
            with staged(lib, h, a1) as st1, staged(lib, h, a2) as st2:
                check_pair(lib, h, st1, st2, rules, what=("budget", rate, max_mm), model=m)
    finally:
        h.close()


def run_budget_edges(lib, sh):
    """One mismatch at the overlap positions 0, 63, 64, L - 1 each (counted) and at position L, just outside (not counted); the same
    code >= 4 at the same overlap position on both sides is one mismatch; a code >= 4 whose two low bits equal the partner's code is a
    mismatch on either side."""
    rng = np.random.default_rng(250)
    n1 = n2 = 150
    r1, r2, what = [], [], []
    for d in (20, -40):
        L = 130 if d >= 0 else 110
        for i in (0, 63, 64, L - 1):
            x, z = spoiled_pair(n1, n2, d, [i], rng)
            r1.append(x); r2.append(z); what.append((d, "mismatch at %d" % i, 1))
        x, z = crafted_xy(n1, n2, d, rng)                    # position L of the shifted side lies outside: a mismatch there is none
        if d >= 0:
            assert z[y_index(n2, L)] in (0, 2)               # y[L] is C or T already; beyond x's end there is nothing to compare with
        else:
            x[L] = 2 - x[L]
        r1.append(x); r2.append(z); what.append((d, "mismatch at L", 0))
        for code in (4, 18, 255):
            x, z = crafted_xy(n1, n2, d, rng)
            i = 64
            x[(d if d >= 0 else 0) + i] = code; z[y_index(n2, i if d >= 0 else i - d)] = code
            r1.append(x); r2.append(z); what.append((d, "code %d on both sides" % code, 1))
        for side in (1, 2):
            x, z = crafted_xy(n1, n2, d, rng)
            ix, iz = (d if d >= 0 else 0) + 5, y_index(n2, 5 if d >= 0 else 5 - d)
            if side == 1:
                x[ix] = 4 + (3 - z[iz])                      # low bits: the base that would match
            else:
                z[iz] = 16 + (3 - x[ix])                     # 17 or 19: the low bits of its complement are x's code
            r1.append(x); r2.append(z); what.append((d, "low bits match, side %d" % side, 1))
    a1, a2 = arrays_from_bases(r1), arrays_from_bases(r2)
    h = handle(lib)
    try:
        with staged(lib, h, a1) as st1, staged(lib, h, a2) as st2:
            strict, one = rules_of(30, 0, 0, 0), rules_of(30, 1, 1000, 0)
            ms, mo = pair_model(a1, a2, strict), pair_model(a1, a2, one)
            for r, (d, name, mm) in enumerate(what):
                assert found_d(a1, a2, mo, r) == d, (name, d)
                assert (found_d(a1, a2, ms, r) == d) == (mm == 0), (name, d)
                assert found_d(a1, a2, ms, r) in (None, d)
            check_pair(lib, h, st1, st2, strict, what="no mismatch allowed", model=ms)
            check_pair(lib, h, st1, st2, one, what="one mismatch allowed", model=mo)
    finally:
        h.close()


# ---- which candidate -----------------------------------------------------------------------------------------------------------------
def run_which_candidate(lib, sh):
    rng = np.random.default_rng(300)
    r1, r2 = [], []
    # 0: poly-A against poly-T: every candidate matches, d = 0 wins, nothing is cut
    r1.append(np.zeros(100, np.uint8)); r2.append(np.full(100, 3, np.uint8))
    # 1: y = A^100 with a C at 50, no mismatch allowed: forward d = 50 and read-through d = -51 are both acceptable
    y = np.zeros(100, np.uint8); y[50] = 1
    r1.append(np.zeros(100, np.uint8)); r2.append(revcomp(y))
    # 2: x = Q P P P, y = P P: d = 30 and d = 60 are both perfect, d = 0 is not
    P = rng.integers(0, 4, 30).astype(np.uint8); Q = (P + 1 + rng.integers(0, 3, 30)).astype(np.uint8) % 4
    r1.append(np.concatenate((Q, P, P, P))); r2.append(revcomp(np.concatenate((P, P))))
    # 3: x = P' P P P with two errors in P': d = 0 has 2 mismatches in 60 and comes before the perfect d = 30
    P2 = P.copy(); P2[[4, 17]] ^= 1
    r1.append(np.concatenate((P2, P, P, P))); r2.append(revcomp(np.concatenate((P, P))))
    a1, a2 = arrays_from_bases(r1), arrays_from_bases(r2)
    strict, loose = rules_of(30, 0, 0, 1), rules_of(30, 5, 200, 1)
    ms, ml = pair_model(a1, a2, strict), pair_model(a1, a2, loose)
    assert found_d(a1, a2, ms, 0) == 0 and int(ms[5][0]) == 100 and int(ms[1][0] - ms[0][0]) == 100 and int(ms[3][0] - ms[2][0]) == 100      # nothing cut
    assert accepts(r1[1], r2[1], 50, strict) and accepts(r1[1], r2[1], -51, strict) and not accepts(r1[1], r2[1], 49, strict)
    assert found_d(a1, a2, ms, 1) == 50
    assert accepts(r1[2], r2[2], 30, strict) and accepts(r1[2], r2[2], 60, strict) and found_d(a1, a2, ms, 2) == 30
    assert found_d(a1, a2, ms, 3) == 30 and found_d(a1, a2, ml, 3) == 0 and accepts(r1[3], r2[3], 30, loose)
    h = handle(lib)
    try:
        with staged(lib, h, a1) as st1, staged(lib, h, a2) as st2:
            check_pair(lib, h, st1, st2, strict, what="strict", model=ms)
            check_pair(lib, h, st1, st2, loose, what="loose", model=ml)
    finally:
        h.close()


# ---- plans in ------------------------------------------------------------------------------------------------------------------------
def run_plans_in(lib, sh):
    """Natural pairs of 150-base reads with 5' cuts of 0, 1, 63, 64 and 3' cuts on either side: the lengths that come out are min(n,
    I - f) for the insert the pair was BUILT from; plus empty ranges, the last record flush with bases_len, d_seq_offs + k and slack
    bytes in front of the arrays."""
    rng = np.random.default_rng(400)
    r1, r2, cuts, true_I = [], [], [], []

    def add(I, f1, c1, f2, c2, len1=150, len2=150):
        a, b = insert_pair(rng.integers(0, 4, I).astype(np.uint8), len1, len2, rng)
        r1.append(a); r2.append(b); cuts.append((f1, c1, f2, c2)); true_I.append(I)
    for I in (100, 140, 200, 260):
        for f1 in (0, 1, 63, 64):
            for f2 in (0, 1, 63, 64):
                add(I, f1, 0, f2, 0)
        for c1, c2 in ((5, 0), (0, 5), (40, 40)):
            add(I, 1, c1, 0, c2); add(I, 0, c1, 64, c2)
    narrowed_by_cut = len(r1)
    add(140, 0, 0, 0, 50)                                    # d = 40 >= 0: read 2 cut to 100 bases, read 1 narrowed from 150 to 140
    empty_from = len(r1)
    add(140, 0, 150, 0, 0); add(140, 0, 0, 150, 0); add(140, 75, 75, 75, 75)      # empty ranges: at the end, at the start, in the middle
    r1.append(np.zeros(0, np.uint8)); r2.append(np.zeros(0, np.uint8)); cuts.append((0, 0, 0, 0)); true_I.append(None)      # no bases at all
    # the next record of side 1 starts with the continuation of a match that is one base short of min_overlap
    ins = rng.integers(0, 4, 271).astype(np.uint8)
    short_at = len(r1)
    r1.append(ins[:150]); r2.append(revcomp(ins)[:150]); cuts.append((0, 0, 0, 0)); true_I.append(None)
    r1.append(ins[150:]); r2.append(rng.integers(0, 4, 121).astype(np.uint8)); cuts.append((0, 0, 0, 0)); true_I.append(None)
    add(200, 3, 0, 2, 0)                                     # the last record, flush with bases_len on both sides
    a1, a2 = arrays_from_bases(r1), arrays_from_bases(r2)
    S1, S2 = a1.seq_offsets.astype(np.int64), a2.seq_offsets.astype(np.int64)
    assert int(S1[-1]) == len(a1.bases) and int(S2[-1]) == len(a2.bases)
    c = np.array(cuts, np.int64)
    plan1 = (S1[:-1] + c[:, 0], S1[1:] - c[:, 1], None)
    plan2 = (S2[:-1] + c[:, 2], S2[1:] - c[:, 3], None)
    rules = rules_of(30, 5, 200, 0)
    m = pair_model(a1, a2, rules, plan1, plan2)
    n_found = 0
    for r, I in enumerate(true_I):
        if I is None:
            continue
        f1, c1, f2, c2 = cuts[r]
        n1, n2 = int(plan1[1][r] - plan1[0][r]), int(plan2[1][r] - plan2[0][r])
        both = min(I, f1 + n1, I - f2) - max(f1, I - f2 - n2, 0)           # the stretch of the insert that both ranges cover
        if both >= 30:
            assert int(m[5][r]) == I, (r, I, cuts[r], int(m[5][r]))
            assert int(m[1][r] - m[0][r]) == min(n1, I - f1) and int(m[3][r] - m[2][r]) == min(n2, I - f2), (r, I, cuts[r])
            n_found += 1
        else:
            assert int(m[5][r]) == NO_INSERT, (r, I, cuts[r])
    assert n_found >= 60 and m[6][6] >= 30
    r = narrowed_by_cut
    assert found_d(a1, a2, m, r, plan1, plan2) == 40 and int(m[1][r] - m[0][r]) == 140 and int(m[3][r] - m[2][r]) == 100
    assert all(int(m[5][r]) == NO_INSERT for r in range(empty_from, empty_from + 4))
    assert int(m[5][short_at]) == NO_INSERT and accepts(np.concatenate((r1[short_at], r1[short_at + 1][:1])), r2[short_at], 121, rules_of(30, 0, 0, 0))
    keep1 = np.ones(a1.n_records, np.uint8); keep1[[2, 9, 40]] = 0
    keep2 = np.ones(a1.n_records, np.uint8); keep2[[3, 9, 41]] = 0
    h = handle(lib)
    try:
        for pad in ((0, 0), (5, 3)):
            with staged(lib, h, a1, pad=pad[0]) as st1, staged(lib, h, a2, pad=pad[1]) as st2:
                check_pair(lib, h, st1, st2, rules, plan1, plan2, pad=pad, what=("plans", pad), model=m)
                check_pair(lib, h, st1, st2, rules, plan1[:2] + (keep1,), plan2[:2] + (keep2,), pad=pad, what=("plans, keep", pad))
                check_pair(lib, h, st1, st2, rules, pad=pad, what=("whole reads", pad))
                check_pair(lib, h, st1, st2, rules, plan1, (None, None, keep2), pad=pad, what=("ranges on side 1 only", pad))
                check_pair(lib, h, st1, st2, rules, (None, None, keep1), plan2, pad=pad, what=("ranges on side 2 only", pad))
                for first, cnt in ((5, None), (a1.n_records - 1, 1), (17, 9)):       # d_seq_offs + k
                    sl = slice(first, None if cnt is None else first + cnt)
                    cut = lambda plan, keep: (plan[0][sl], plan[1][sl], keep[sl])
                    check_pair(lib, h, st1, st2, rules, cut(plan1, keep1), cut(plan2, keep2), pad=pad, first=first, n=cnt, what=("first", first, pad))
                    check_pair(lib, h, st1, st2, rules, pad=pad, first=first, n=cnt, what=("first, whole", first, pad))
    finally:
        h.close()


# ---- keep, min_length, in place, d_insert, statistics, long ranges ---------------------------------------------------------------------
def keep_pairs(rng, n_pairs=72):
    """Natural pairs with inserts around the read length, all four combinations of the incoming flags with other non-zero bytes than
    1, three pairs each that leave min_length (40) exactly / one above / one below on read 1's and on read 2's side (inserts of 50,
    51, 49 bases of which the plan has cut 10 off that side's 5' end), and long ranges: 1025 and 4097 bases on one side (not
    searched) and a pair of 1024 + 1024 (searched)."""
    r1, r2 = [], []
    for _ in range(n_pairs):
        I = int(rng.integers(20, 300))
        a, b = insert_pair(rng.integers(0, 4, I).astype(np.uint8), int(rng.integers(100, 151)), int(rng.integers(100, 151)), rng)
        r1.append(a); r2.append(b)
    for k, I in enumerate((50, 51, 49, 50, 51, 49)):
        r1[3 + k], r2[3 + k] = insert_pair(rng.integers(0, 4, I).astype(np.uint8), 150, 150, rng)
    long_at = len(r1)
    ins = rng.integers(0, 4, 600).astype(np.uint8)
    for len1, len2 in ((1025, 150), (150, 4097), (1024, 1024), (1025, 30)):
        a, b = insert_pair(ins, len1, len2, rng)
        r1.append(a); r2.append(b)
    a1, a2 = arrays_from_bases(r1), arrays_from_bases(r2)
    n = a1.n_records
    S1, S2 = a1.seq_offsets.astype(np.int64), a2.seq_offsets.astype(np.int64)
    b1 = S1[:-1] + rng.integers(0, 5, n); e1 = S1[1:] - rng.integers(0, 3, n)
    b2 = S2[:-1] + rng.integers(0, 5, n); e2 = S2[1:] - rng.integers(0, 3, n)
    for arr, S in ((b1, S1[:-1]), (e1, S1[1:]), (b2, S2[:-1]), (e2, S2[1:])):
        arr[3:9] = S[3:9]; arr[long_at:] = S[long_at:]
    b1[3:6] += 10; b2[6:9] += 10
    k1 = np.array([1, 7, 0, 255, 0, 1] * (n // 6 + 1), np.uint8)[:n]
    k2 = np.array([1, 0, 0, 9, 1, 1, 255, 0, 1, 1, 1] * (n // 11 + 1), np.uint8)[:n]
    k1[3:9] = 1; k2[3:9] = 1; k1[long_at:] = 1; k2[long_at:] = 1
    return a1, a2, (b1, e1, k1), (b2, e2, k2), long_at


def run_keep_and_inplace(lib, sh):
    rng = np.random.default_rng(500)
    a1, a2, plan1, plan2, long_at = keep_pairs(rng)
    n = a1.n_records
    rules = rules_of(30, 5, 200, 40)
    m = pair_model(a1, a2, rules, plan1, plan2)
    k1, k2 = plan1[2] != 0, plan2[2] != 0
    assert all(((k1 == u) & (k2 == v)).sum() >= 3 for u in (False, True) for v in (False, True))
    # min_length exact, one above, one below: on read 1's side in pairs 3 .. 5, on read 2's side in pairs 6 .. 8
    assert [int(m[4][r]) for r in range(3, 9)] == [1, 1, 0, 1, 1, 0]
    assert [int(m[1][r] - m[0][r]) for r in range(3, 9)] == [40, 41, 39, 50, 51, 49] and [int(m[3][r] - m[2][r]) for r in range(3, 9)] == [50, 51, 49, 40, 41, 39]
    assert all(v > 0 for v in m[6]), m[6]                    # every statistic counts something
    assert m[6][7] == int((k1 != k2).sum()) and m[6][0] + m[6][8] == int((k1 & k2).sum()) and m[6][9] == 3
    assert [int(m[5][long_at + k]) for k in (0, 1, 3)] == [NO_INSERT] * 3 and int(m[5][long_at + 2]) == 600      # 1024 + 1024 is searched
    assert [int(m[4][long_at + k]) for k in range(4)] == [1, 1, 1, 0]      # ... and the keep rule applies to the untouched lengths (30 < 40)
    gone = ~(k1 & k2)
    assert (m[4][gone] == 0).all() and (m[5][gone] == NO_INSERT).all() and (m[1][gone] == plan1[1][gone].astype(np.uint64)).all()
    h = handle(lib)
    try:
        with staged(lib, h, a1) as st1, staged(lib, h, a2) as st2:
            for inplace in (False, True):
                for alias in (None, 1, 2):
                    check_pair(lib, h, st1, st2, rules, plan1, plan2, what=("all six", inplace, alias), inplace=inplace, keep_alias=alias, model=m)
                check_pair(lib, h, st1, st2, rules, plan1[:2] + (None,), plan2, what=("no keep 1", inplace), inplace=inplace, keep_alias=2)
                check_pair(lib, h, st1, st2, rules, (None, None, plan1[2]), plan2[:2] + (None,), what=("mixed", inplace), inplace=inplace, keep_alias=1)
            check_pair(lib, h, st1, st2, rules, plan1, plan2, what="no d_insert", insert=False, model=m)
            check_pair(lib, h, st1, st2, rules, plan1, plan2, what="no d_insert, in place", insert=False, inplace=True, keep_alias=1, model=m)
            check_pair(lib, h, st2, st1, rules, plan2, plan1, what="sides swapped")
            # d_quals, d_titles and d_title_offs are not read
            bare = lambda st: lib.ColumnsIn(st.cols_in().d_bases, st.cols_in().bases_len, None, None, 0, st.cols_in().d_seq_offs, None, n)
            u64 = lambda plan: (plan[0].astype(np.uint64), plan[1].astype(np.uint64), plan[2])
            got = pair_call(lib, h, bare(st1), bare(st2), n, lib_rules(lib, rules), u64(plan1), u64(plan2))
            assert got.error is None and got.stats == m[6] and np.array_equal(got.keep, m[4]) and np.array_equal(got.insert, m[5])
            assert all(np.array_equal(got.ranges[i], m[i]) for i in range(4))
    finally:
        h.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def run_arg_refusals(lib, sh):
    rng = np.random.default_rng(600)
    a1, a2, plan1, plan2, _ = keep_pairs(rng, 24)
    n = a1.n_records
    good = rules_of(30, 5, 200, 1)
    u64 = lambda v: np.asarray(v).astype(np.uint64)
    h = handle(lib)
    try:
        with staged(lib, h, a1) as st1, staged(lib, h, a2) as st2:
            checked = 0
            for name, pr in [("min_overlap 0", lib_rules(lib, dict(good, min_overlap=0))), ("min_overlap 1025", lib_rules(lib, dict(good, min_overlap=1025))),
                             ("permille 1001", lib_rules(lib, dict(good, rate=1001)))] + \
                            [("reserved[%d]" % k, lib_rules(lib, good, tuple(int(i == k) for i in range(4)))) for k in range(4)]:
                got = pair_call(lib, h, st1.cols_in(), st2.cols_in(), n, pr)
                assert got.error is not None and got.error.code == E_ARG and got.untouched, (name, got.error)
                checked += 1
            got = pair_call(lib, h, st1.cols_in(), st2.cols_in(0, n - 1), n, lib_rules(lib, good))
            assert got.error is not None and got.error.code == E_ARG and got.untouched, got.error
            got = pair_call(lib, h, st1.cols_in(1, n - 1), st2.cols_in(), n, lib_rules(lib, good))
            assert got.error is not None and got.error.code == E_ARG and got.untouched, got.error
            for name, p1, p2 in (("begin 1 alone", (u64(plan1[0]), None, None), (None,) * 3), ("end 1 alone", (None, u64(plan1[1]), None), (None,) * 3),
                                 ("begin 2 alone", (None,) * 3, (u64(plan2[0]), None, None)), ("end 2 alone", (None,) * 3, (None, u64(plan2[1]), None))):
                got = pair_call(lib, h, st1.cols_in(), st2.cols_in(), n, lib_rules(lib, good), p1, p2)
                assert got.error is not None and got.error.code == E_ARG and got.untouched, (name, got.error)
                checked += 1
            for k in range(5):
                got = pair_call(lib, h, st1.cols_in(), st2.cols_in(), n, lib_rules(lib, good), null_out=k)
                assert got.error is not None and got.error.code == E_ARG and got.untouched, ("null output", k, got.error)
                checked += 1
            assert checked == 16
            check_pair(lib, h, st1, st2, good, plan1, plan2, what="the same handle, clean")
            check_pair(lib, h, st1, st2, rules_of(1024, 0xFFFFFFFF, 1000, 0xFFFFFFFF), what="the largest figures")
            got = pair_call(lib, h, st1.cols_in(3, 0), st2.cols_in(5, 0), 0, lib_rules(lib, good))          # no records
            assert got.error is None and got.stats == [0] * 11 and got.untouched
    finally:
        h.close()
    hc = ce.handle(lib, dataclasses.replace(Config.from_levels(0, 0), color_space=True))
    try:
        with staged(lib, hc, a1) as st1, staged(lib, hc, a2) as st2:
            got = pair_call(lib, hc, st1.cols_in(), st2.cols_in(), n, lib_rules(lib, good))
            assert got.error is not None and got.error.code == E_ARG and got.untouched
    finally:
        hc.close()


def run_input_errors(lib, sh):
    """The adapter plan's input plants on side 1, on side 2 and on both (side 1 is the one reported), in the first, a middle and the
    last record, kept and dropped ones, fresh and in place: code, side, record, outputs still 0xA5 / the plans unchanged, and the
    same handle plans the clean arrays afterwards."""
    rng = np.random.default_rng(650)
    a1, a2, plan1, plan2, _ = keep_pairs(rng, 37)            # 41 pairs
    n = a1.n_records
    assert n == 41
    pads = (4, 6)
    rules = rules_of(30, 5, 200, 20)
    pr = lib_rules(lib, rules)
    A = (a1, a2)
    S = lambda s, r: int(A[s].seq_offsets[r]) + pads[s]
    padded = lambda s, plan: ((plan[0] + pads[s]).astype(np.uint64), (plan[1] + pads[s]).astype(np.uint64), plan[2].copy())
    hp = [padded(0, plan1), padded(1, plan2)]
    hp[0][2][[0, 20]] = 0; hp[1][2][[20, 40]] = 0            # plants hit kept and dropped records alike
    plans_of = lambda: [tuple(v.copy() for v in p) for p in hp]
    h = handle(lib)
    checked = 0

    def refused(got, side, r, word, name):
        assert got.error is not None and got.error.code == E_INPUT, (name, side, r, got.error)
        msg = str(got.error)
        assert "read %d" % (side + 1) in msg and "record %d:" % r in msg and word in msg, (name, side, r, msg)
    try:
        with staged(lib, h, a1, pad=pads[0]) as st1, staged(lib, h, a2, pad=pads[1]) as st2:
            st = (st1, st2)
            offs = [("order", lambda s, r: st[s].poke("seq_offs", r + 1, S(s, r) - 1, np.uint64), "not non-decreasing"),
                    ("end", lambda s, r: st[s].poke("seq_offs", r + 1, len(A[s].bases) + pads[s] + 5, np.uint64), "above bases_len"),
                    ("wild", lambda s, r: st[s].poke("seq_offs", r + 1, 2 ** 64 - 1, np.uint64), "above bases_len")]
            for name, plant, word in offs:
                for r in (0, 20, 40):
                    for sides in ((0,), (1,), (0, 1)):
                        for s in sides:
                            plant(s, r if s == sides[0] else 0)      # on both: side 2's plant sits in record 0, side 1 is reported all the same
                        for with_plans in (False, True):
                            p1, p2 = plans_of() if with_plans else ((None,) * 3, (None,) * 3)
                            got = pair_call(lib, h, st1.cols_in(), st2.cols_in(), n, pr, p1, p2)
                            refused(got, sides[0], r, word, name)
                            assert got.untouched
                        st1.restore(); st2.restore()
                        checked += 1
                check_pair(lib, h, st1, st2, rules, plan1, plan2, pad=pads, what=("after", name))

            def ranged(s, r, b=None, e=None):
                p = plans_of()
                if b is not None: p[s][0][r] = b
                if e is not None: p[s][1][r] = e
                return p
            ranges = [("begin low", lambda s, r: dict(b=S(s, r) - 1), "d_begin lies below"),
                      ("end high", lambda s, r: dict(e=S(s, r + 1) + 1), "d_end lies above"),
                      ("end wild", lambda s, r: dict(e=2 ** 64 - 1), "d_end lies above"),
                      ("begin above end", lambda s, r: dict(b=S(s, r + 1), e=S(s, r + 1) - 1), "d_begin lies above d_end")]
            for name, how, word in ranges:
                for r in (0, 20, 40):
                    for sides in ((0,), (1,), (0, 1)):
                        p = plans_of()
                        for s in sides:
                            rr = r if s == sides[0] else 0
                            for key, v in how(s, rr).items():
                                p[s][0 if key == "b" else 1][rr] = v
                        for inplace, alias in ((False, None), (True, 1), (True, 2)):
                            got = pair_call(lib, h, st1.cols_in(), st2.cols_in(), n, pr, p[0], p[1], inplace=inplace, keep_alias=alias)
                            refused(got, sides[0], r, word, name)
                            if inplace:                          # the plans themselves are what they were
                                for s in (0, 1):
                                    assert all(got.plans_after[s][i] == p[s][i].tobytes() for i in range(3)), (name, r, s)
                            else:
                                assert got.untouched, (name, r)
                        checked += 1
                check_pair(lib, h, st1, st2, rules, plan1, plan2, pad=pads, what=("after", name))
    finally:
        h.close()
    assert checked == 63


def run_codec_state(lib, sh):
    """The call touches nothing the codec carries, as run_codec_state of the adapter cases: the fields capacity stays, a pending
    record layout stays pending, and the text call that follows writes what it writes on a fresh handle seeded alike."""
    a1, a2, plan1, plan2, _ = keep_pairs(np.random.default_rng(660), 30)
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
            with staged(lib, h, a1) as st1, staged(lib, h, a2) as st2:
                check_pair(lib, h, st1, st2, rules_of(30, 5, 200, 20), plan1, plan2)
                assert h.get_fields_capacity() == 11
            assert text_blocks(h) == text_blocks(fresh), layout
        finally:
            h.close(); fresh.close()


# ---- pair counts -------------------------------------------------------------------------------------------------------------------
def run_count(lib, sh, n_pairs):
    """n_pairs pairs of 10 + 10 bases at min_overlap 3, plans in.  The model runs on the first 2049 pairs at the most; behind them the
    same pairs repeat, and so do their results."""
    base = min(n_pairs, 2049)
    rng = np.random.default_rng(700 + n_pairs)
    x = rng.integers(0, 4, (base, 10)).astype(np.uint8)
    z = rng.integers(0, 4, (base, 10)).astype(np.uint8)
    for r in np.nonzero(rng.random(base) < 0.6)[0]:          # an insert of 4 .. 16 bases
        I = int(rng.integers(4, 17))
        ins = rng.integers(0, 4, I).astype(np.uint8)
        x[r, :min(I, 10)] = ins[:10]; z[r, :min(I, 10)] = revcomp(ins)[:10]
    x[rng.random((base, 10)) < 0.02] = 4
    cut = lambda: rng.integers(0, 3, base).astype(np.uint64)
    cuts = [cut() for _ in range(4)]
    keeps = [(rng.random(base) < 0.85).astype(np.uint8) for _ in range(2)]
    S0 = (10 * np.arange(base + 1)).astype(np.uint64)
    mk = lambda b: Arrays(b.reshape(-1), np.full(b.size, 30, np.uint8), np.zeros(0, np.uint8), (10 * np.arange(len(b) + 1)).astype(np.uint64),
                          np.zeros(len(b) + 1, np.uint64), [0, len(b)])
    rules = rules_of(3, 1, 200, 4)
    mb = pair_model(mk(x), mk(z), rules, (S0[:-1] + cuts[0], S0[1:] - cuts[1], keeps[0]), (S0[:-1] + cuts[2], S0[1:] - cuts[3], keeps[1]))
    if base >= 2049:
        assert mb[6][5] > 0 and mb[6][6] > 0 and mb[6][7] > 0 and mb[6][8] > 0 and mb[6][0] > 0
    reps, rest = divmod(n_pairs, base)
    idx = np.concatenate([np.arange(base)] * reps + [np.arange(rest)]).astype(np.int64)
    S = (10 * np.arange(n_pairs + 1)).astype(np.uint64)
    a1, a2 = mk(x[idx]), mk(z[idx])
    plan1 = (S[:-1] + cuts[0][idx], S[1:] - cuts[1][idx], keeps[0][idx])
    plan2 = (S[:-1] + cuts[2][idx], S[1:] - cuts[3][idx], keeps[1][idx])
    move = S[:-1] - S0[:-1][idx]
    part = pair_model(mk(x[:rest]), mk(z[:rest]), rules, tuple(v[:rest] for v in (S0[:-1] + cuts[0], S0[1:] - cuts[1], keeps[0])),
                      tuple(v[:rest] for v in (S0[:-1] + cuts[2], S0[1:] - cuts[3], keeps[1])))[6] if rest else [0] * 11
    stats = [reps * u + v for u, v in zip(mb[6], part)]
    m = tuple(mb[i][idx] + move for i in range(4)) + (mb[4][idx], mb[5][idx], stats)
    h = handle(lib)
    try:
        with staged(lib, h, a1) as st1, staged(lib, h, a2) as st2:
            check_pair(lib, h, st1, st2, rules, plan1, plan2, what=n_pairs, model=m)
            check_pair(lib, h, st1, st2, rules, plan1, plan2, what=(n_pairs, "in place"), inplace=True, keep_alias=2, model=m)
    finally:
        h.close()


def run_second_pair_of_a_wave(lib, sh):
    """A wave's second pair finds the planes of its first one in LDS.  The first eight pairs are 1024 + 1024 bases long and set bits in
    every word of every plane; one grid stride further (4096 workgroups of WG / 64 waves), the same waves get pairs of 64 and 128
    bases with shifts whose windows reach into the word behind the range: that word must read as 0.  Between the two, pairs of 1 + 1
    bases that do not match.  The model runs on the sixteen pairs and one filler; the fillers' results are written down here."""
    stride = sh["wave_stride"]
    rng = np.random.default_rng(800)
    heads, tails = [], []
    for k in range(8):
        x = rng.integers(0, 4, 1024).astype(np.uint8); x[rng.random(1024) < 0.2] = 4
        z = rng.integers(0, 4, 1024).astype(np.uint8); z[rng.random(1024) < 0.2] = 4
        heads.append((x, z))
    for n1, n2, d in ((64, 64, 1), (64, 64, -1), (64, 64, 33), (64, 64, -33), (128, 128, 63), (128, 64, 64), (64, 128, -64), (128, 128, -65)):
        tails.append(crafted_xy(n1, n2, d, rng))
    filler = (np.zeros(1, np.uint8), np.zeros(1, np.uint8))          # A against comp(A) = T
    rules = rules_of(30, 0, 0, 0)
    small = heads + [filler] + tails
    sa1, sa2 = arrays_from_bases([p[0] for p in small]), arrays_from_bases([p[1] for p in small])
    sm = pair_model(sa1, sa2, rules)
    assert [found_d(sa1, sa2, sm, 9 + k) for k in range(8)] == [1, -1, 33, -33, 63, 64, -64, -65] and all(int(sm[5][k]) == NO_INSERT for k in range(9))
    n = stride + 8
    n_fill = stride - 8
    idx = np.concatenate((np.arange(8), np.full(n_fill, 8), np.arange(9, 17)))
    titles = np.zeros(0, np.uint8)

    def big(sa, col):
        lens = (sa.seq_offsets[1:] - sa.seq_offsets[:-1]).astype(np.int64)[idx]
        S = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
        bases = np.concatenate([p[col] for p in heads] + [np.zeros(n_fill, np.uint8)] + [p[col] for p in tails])
        return Arrays(bases, np.full(len(bases), 30, np.uint8), titles, S, np.zeros(n + 1, np.uint64), [0, n])
    a1, a2 = big(sa1, 0), big(sa2, 1)
    rel = lambda a, sa, i: (sm[i] - sa.seq_offsets[:-1])[idx] + a.seq_offsets[:-1]
    fill_stats = pair_model(arrays_from_bases([filler[0]]), arrays_from_bases([filler[1]]), rules)[6]
    stats = [u + (n_fill - 1) * v for u, v in zip(sm[6], fill_stats)]
    m = (rel(a1, sa1, 0), rel(a1, sa1, 1), rel(a2, sa2, 2), rel(a2, sa2, 3), sm[4][idx], sm[5][idx], stats)
    h = handle(lib)
    try:
        with staged(lib, h, a1) as st1, staged(lib, h, a2) as st2:
            check_pair(lib, h, st1, st2, rules, what="second pair of a wave", model=m)
    finally:
        h.close()


# ---- fuzz ------------------------------------------------------------------------------------------------------------------------
def fuzz_pairs(seed, n_pairs):
    """Random inserts of 20 .. 399 bases, reads of up to 150 bases, 1 % substitutions, a few codes >= 4, random plans and keep flags
    -> arrays 1, arrays 2, plan 1, plan 2, rules."""
    rng = np.random.default_rng(3000 + seed)
    other = np.concatenate([[4, 4, 255], np.arange(5, 19)]).astype(np.uint8)
    r1, r2 = [], []
    for _ in range(n_pairs):
        I = int(rng.integers(20, 400))
        reads = insert_pair(rng.integers(0, 4, I).astype(np.uint8), int(rng.integers(100, 151)), int(rng.integers(100, 151)), rng)
        for x in reads:
            sub = rng.random(len(x)) < 0.01
            x[sub] = (x[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
            amb = rng.random(len(x)) < 0.004
            x[amb] = other[rng.integers(0, len(other), int(amb.sum()))]
        r1.append(reads[0]); r2.append(reads[1])
    a1, a2 = arrays_from_bases(r1), arrays_from_bases(r2)
    plans = []
    for a in (a1, a2):
        S = a.seq_offsets.astype(np.int64)
        lens = S[1:] - S[:-1]
        whole = rng.random(n_pairs) < 0.5
        cut5 = np.where(whole, 0, (rng.random(n_pairs) * (lens + 1) * 0.15).astype(np.int64))
        cut3 = np.where(whole, 0, (rng.random(n_pairs) * (lens - cut5 + 1) * 0.15).astype(np.int64))
        plans.append(((S[:-1] + cut5).astype(np.uint64), (S[1:] - cut3).astype(np.uint64), (rng.random(n_pairs) < 0.92).astype(np.uint8)))
    return a1, a2, plans[0], plans[1], rules_of(int(rng.choice([20, 30])), 5, 200, int(rng.integers(0, 60)))


def run_fuzz(lib, sh, seed):
    n_pairs = sh["pair_fuzz"][1]
    a1, a2, plan1, plan2, rules = fuzz_pairs(seed, n_pairs)
    m = pair_model(a1, a2, rules, plan1, plan2)
    searched = int(((plan1[2] != 0) & (plan2[2] != 0)).sum())
    found = m[6][5]
    print("pair fuzz", seed, "pairs", n_pairs, "searched", searched, "found", found, "stats", m[6])
    assert 10 * found >= 3 * searched and 10 * (searched - found) >= 2 * searched      # the model alone: both outcomes are well represented
    h = handle(lib)
    try:
        with staged(lib, h, a1, pad=3) as st1, staged(lib, h, a2, pad=1) as st2:
            check_pair(lib, h, st1, st2, rules, plan1, plan2, pad=(3, 1), what=("fuzz", seed), model=m)
            check_pair(lib, h, st1, st2, rules, pad=(3, 1), what=("fuzz, whole reads", seed))
    finally:
        h.close()


# ---- the Python layers and the closed loop ---------------------------------------------------------------------------------------------
tensors = ca.tensors


def run_python_layers(lib, sh, device):
    from dsrc_amd import columns
    a1, a2, plan1, plan2, rules = fuzz_pairs(7, 100)
    kw = dict(min_overlap=rules["min_overlap"], max_mismatches=rules["max_mm"], max_error_permille=rules["rate"], min_length=rules["min_length"])
    t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v).astype(dt)).to(device)
    tp = lambda plan: (t(plan[0], np.int64), t(plan[1], np.int64), t(plan[2], np.uint8))
    h = handle(lib)
    try:
        assert tuple(lib.PAIR_STATS) == PAIR_STATS and lib.NO_INSERT == NO_INSERT
        c1, c2 = tensors(a1, device), tensors(a2, device)
        p1, p2 = tp(plan1), tp(plan2)
        m = pair_model(a1, a2, rules, plan1, plan2)
        got = columns.pair_plan(h, c1, c2, p1, p2, return_insert=True, **kw)
        assert len(got) == 7 and all(v.dtype == torch.int64 for v in got[:4]) and got[4].dtype == torch.uint8 and got[6].dtype == torch.int64
        assert got[4].device.type == torch.device(device).type
        assert got[0].data_ptr() != p1[0].data_ptr() and all(torch.equal(u, v) for u, v in zip(p1 + p2, tp(plan1) + tp(plan2)))      # fresh tensors, inputs as they were
        assert list(got[5]) == list(PAIR_STATS) and list(got[5].values()) == m[6]
        assert all(np.array_equal(got[i].cpu().numpy().astype(np.uint64), m[i]) for i in range(4)) and np.array_equal(got[4].cpu().numpy(), m[4])
        assert np.array_equal(got[6].cpu().numpy(), np.where(m[5] == NO_INSERT, -1, m[5].astype(np.int64)))
        m = pair_model(a1, a2, rules)
        got = columns.pair_plan(h, c1, c2, **kw)
        assert len(got) == 6 and list(got[5].values()) == m[6] and np.array_equal(got[3].cpu().numpy().astype(np.uint64), m[3])
        m = pair_model(a1, a2, rules, (None, None, plan1[2]), plan2)
        got = columns.pair_plan(h, c1, c2, (None, None, p1[2]), p2, **kw)
        assert list(got[5].values()) == m[6] and np.array_equal(got[4].cpu().numpy(), m[4])

        class Never:                                         # ValueError comes before any library call
            def __getattr__(self, name):
                raise AssertionError("the library was called")
        fewer = tensors(arrays_from_bases([np.zeros(5, np.uint8)]), device)
        bad_calls = [dict(min_overlap=0), dict(min_overlap=1025), dict(min_overlap=3.0), dict(max_mismatches=-1), dict(max_error_permille=1001),
                     dict(max_error_permille=-1), dict(min_length=-1), dict(min_length=2 ** 32), dict(plan1=(p1[0], None, None)),
                     dict(plan2=(None, p2[1], None)), dict(plan1=(p1[0][:5], p1[1][:5], None)), dict(plan2=(None, None, p2[2][:7]))]
        for bad in bad_calls:
            for call in (lambda: columns.pair_plan(Never(), c1, c2, **bad),):
                try:
                    call()
                except ValueError:
                    pass
                else:
                    raise AssertionError("no ValueError for %r" % (bad,))
        for call in (lambda: columns.pair_plan(Never(), c1, fewer), lambda: columns.filter_pairs(Never(), fewer, c2),
                     lambda: columns.filter_pairs(Never(), c1, c2, pair_min_overlap=0), lambda: columns.filter_pairs(Never(), c1, c2, adapters2=["ACGN"])):
            try:
                call()
            except ValueError:
                pass
            else:
                raise AssertionError("no ValueError")
        if torch.device(device).type != "cpu":               # column sets on different devices
            try:
                columns.pair_plan(Never(), c1, tensors(a2, "cpu"))
            except ValueError:
                pass
            else:
                raise AssertionError("no ValueError for two devices")
    finally:
        h.close()


ADAPTER_STR = ("AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT")


def paired_reads(n_pairs, seed=21):
    """Pairs with inserts of 25 .. 300 bases, reads of 100 bases that run into the adapters, qualities that fall off at the 3' end
    -> (arrays, records, text) per side."""
    rng = np.random.default_rng(seed)
    sides = ([], [])
    for r in range(n_pairs):
        I = 26 + r if r < 3 else int(rng.integers(25, 300))
        reads = insert_pair(rng.integers(0, 4, I).astype(np.uint8), 100, 100, rng)
        for s, x in enumerate(reads):
            sub = rng.random(100) < 0.01
            x[sub] = (x[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
            x[rng.random(100) < 0.005] = 4
            q = rng.integers(25, 41, 100)
            low = int(rng.integers(0, 15)) if rng.random() < 0.5 else 0
            if low: q[100 - low:] = rng.integers(2, 12, low)
            if rng.random() < 0.05: q[:] = rng.integers(2, 10, 100)      # a mate that the quality plan drops
            sides[s].append((b"@pair.%d/%d" % (r + 1, s + 1), bytes(b"ACGTN"[v] for v in x), bytes((q + 33).astype(np.uint8))))
    text = lambda recs: b"\n".join(t + b"\n" + s + b"\n+\n" + q for t, s, q in recs)
    return [(ce.arrays_of([text(recs)]), recs, text(recs)) for recs in sides]


def pairs_model(a1, a2, trim, adapters=(None, None), overlap=True, pair_rules=None, adapter_min_overlap=3, adapter_rate=100):
    """model quality plan -> model adapter plan per side -> pair_model (or keep1 & keep2) -> plans out, the stats dict of filter_pairs."""
    plans, stats = [], {}
    for name, a, ads in (("read1", a1, adapters[0]), ("read2", a2, adapters[1])):
        b, e, k, ts = cs.plan_model(a, trim)
        side = dict(zip(ca.TRIM_STATS, ts))
        if ads is not None:
            ar = ca.rules_of([ca.codes_of(s) for s in ads], adapter_min_overlap, adapter_rate, trim["min_length"])
            b, e, k, _, as_ = ca.adapter_model(a, ar, b, e, k)
            side["adapter"] = dict(zip(ca.ADAPTER_STATS, as_))
        plans.append((b, e, k)); stats[name] = side
    if overlap:
        pr = dict(pair_rules or rules_of(), min_length=trim["min_length"])
        b1, e1, b2, e2, keep, _, ps = pair_model(a1, a2, pr, plans[0], plans[1])
        stats["pair"] = dict(zip(PAIR_STATS, ps))
    else:
        (b1, e1, k1), (b2, e2, k2) = plans
        keep = ((k1 != 0) & (k2 != 0)).astype(np.uint8)
    return (b1, e1), (b2, e2), keep, stats


def run_filter_pairs(lib, sh, device):
    from dsrc_amd import columns
    (a1, _, _), (a2, _, _) = paired_reads(160)
    trim = cs.rules_of(0, 20, min_length=30, max_n=2)        # (inserts of 26 .. 28 bases are found at a min_overlap of 20 and dropped for length)
    same = lambda sel, want: all(np.array_equal(g.cpu().numpy().astype(w.dtype), w) for g, w in
                                 zip((sel.bases, sel.quals, sel.titles, sel.seq_offsets, sel.title_offsets), want[:5]))
    h = handle(lib)
    try:
        c1, c2 = tensors(a1, device), tensors(a2, device)
        for ads in ((None, None), ([ADAPTER_STR[0]], [ADAPTER_STR[1]]), (None, [ADAPTER_STR[1]])):
            for overlap in (True, False):
                r1, r2, keep, wstats = pairs_model(a1, a2, trim, ads, overlap, rules_of(20, 4, 150))
                if ads[1] is not None:                       # (what an adapter plan has cut already, the pair plan finds done)
                    assert wstats["read2"]["adapter"]["records_trimmed"] >= 20
                if overlap and ads == (None, None):
                    ps = wstats["pair"]
                    assert ps["overlap_narrowed"] >= 20 and ps["dropped_mate"] > 0 and ps["dropped_length"] > 0 and 0 < ps["pairs_kept"] < 160, ps
                w1, w2 = cs.select_model(a1, r1[0], r1[1], keep), cs.select_model(a2, r2[0], r2[1], keep)
                o1, o2, stats = columns.filter_pairs(h, c1, c2, adapters1=ads[0], adapters2=ads[1], overlap=overlap, pair_min_overlap=20,
                                                     pair_max_mismatches=4, pair_max_error_permille=150, **trim)
                assert stats == wstats and ("pair" in stats) == overlap and list(stats)[:2] == ["read1", "read2"], (stats, wstats)
                assert same(o1, w1) and same(o2, w2) and o1.n_records == o2.n_records == int(keep.sum()), (ads, overlap)
                _, s1 = columns.select_columns(h, c1, keep=torch.from_numpy(keep).to(device), return_source=True)
                _, s2 = columns.select_columns(h, c2, keep=torch.from_numpy(keep).to(device), return_source=True)
                assert torch.equal(s1, s2) and np.array_equal(s1.cpu().numpy(), np.nonzero(keep)[0])      # equal `source`: mate j is mate j
        o1, o2, _ = columns.filter_pairs(h, c1, c2, titles=False, **trim)
        assert o1.titles.numel() == 0 and o2.titles.numel() == 0 and o1.n_records == o2.n_records
    finally:
        h.close()


def run_closed_loop(lib, sh, device):
    """Pairs written here -> the oracle's blocks of both files -> decode_columns -> filter_pairs -> encode_columns == the oracle's
    blocks of the text of the model-filtered pairs, lossless -d3 -q2 with CRC."""
    from dsrc_amd import columns
    cfg = ce.BLOCK_CFG
    (a1, recs1, text1), (a2, recs2, text2) = paired_reads(300, seed=22)
    trim = cs.rules_of(0, 20, min_length=35)
    ads = (None, None)                                       # no adapter sequence is given: the read-through is found from the pairs
    r1, r2, keep, wstats = pairs_model(a1, a2, trim, ads)
    print("closed loop: model stats", wstats)
    assert wstats["pair"]["overlap_narrowed"] >= 40 and 0 < wstats["pair"]["pairs_kept"] < 300
    wants = []
    for a, recs, (b, e) in ((a1, recs1, r1), (a2, recs2, r2)):
        S = a.seq_offsets.astype(np.int64)
        kept = [(t, s[int(b[r] - S[r]): int(e[r] - S[r])], q[int(b[r] - S[r]): int(e[r] - S[r])]) for r, (t, s, q) in enumerate(recs) if keep[r]]
        want = ce.oracle_blocks(cfg, [b"\n".join(t + b"\n" + s + b"\n+\n" + q for t, s, q in kept)])
        assert want is not None
        wants.append(want[0][0])
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
        o1, o2, stats = columns.filter_pairs(h, cols[0], cols[1], adapters1=ads[0], adapters2=ads[1], **trim)
        assert stats == wstats and o1.n_records == o2.n_records == int(keep.sum())
        for out, want in ((o1, wants[0]), (o2, wants[1])):
            h.set_fields_capacity(0)
            blocks, o_offs, o_sizes, _ = columns.encode_columns(h, out, block_records=out.block_records)
            host = blocks.cpu().numpy().tobytes()
            assert [host[o: o + s] for o, s in zip(o_offs, o_sizes)] == [want]       # byte for byte, the CRC field included
    finally:
        h.close()
