"""Shared by tests/test_emu_columns_adapt.py (CPU, emulator build) and tests/test_gpu_columns_adapt.py (MI355X): the cases of the
columnar adapter trim (dsrcgpu_columns_adapter_plan; dsrc_amd/csrc/k_columns_adapt.h) and what they must give.

The reference has no counterpart, so the yardstick is the integer model written out here: adapter_search() is the serial rule of
include/dsrc_gpu.h word for word (every start position, every adapter, a Hamming count under an error budget), adapter_model()
applies it to a plan.  None of it comes from the library under test, and every comparison is exact equality.  Output arrays are
filled with 0xA5 before a call, so that "nothing written" can be asserted.  Before the library is compared on a crafted case the
model alone is asked what that case is for.

Shapes.  The emulator pays a coroutine switch per wave exchange, so its fuzz is 2 seeds x 150 records where the GPU runs 6 x 2000.
The planner's grid holds at most 4096 workgroups of WG / 64 waves: with workgroups of 1024 threads a count above 65536 records
takes the grid stride into a second round -- that count runs on the GPU only."""
from __future__ import annotations

import dataclasses

import numpy as np
import torch        # noqa: F401  before the first handle (see columns_cases)

from tests import columns_cases as cc
from tests import columns_enc_cases as ce
from tests import columns_sel_cases as cs
from tests._oracle import Config
from tests.cases import TINY

E_ARG, E_INPUT = cs.E_ARG, cs.E_INPUT
NONE = 0xFFFFFFFF

SHAPES = {
    "gpu": dict(cc.SHAPES["gpu"], adapt_fuzz=(6, 2000), counts=[1, 63, 64, 65, 2049], stride_count=4096 * 16 + 4001),
    "emu": dict(cc.SHAPES["emu"], adapt_fuzz=(2, 150), counts=[1, 63, 64, 65, 2049], stride_count=None),
}
Arrays = ce.Arrays
Dev = cs.Dev
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 200, 4097]
ADAPTER_LENGTHS = [1, 3, 13, 33, 63, 64]


# ---- the model -------------------------------------------------------------------------------------------------------------------
def adapter_search(x, adapters, min_overlap, rate):
    """The serial rule on the range x (numpy uint8) -> (p, a) of the hit, or (len(x), NONE)."""
    n = len(x)
    for p in range(n):                                       # leftmost start position wins
        for a, A in enumerate(adapters):                     # at the same p, the lowest adapter index wins
            L = min(len(A), n - p)                           # the adapter may hang over the 3' end of the range
            if L < min_overlap:
                continue
            mm = int(np.count_nonzero(x[p: p + L] != A[:L]))  # a read code >= 4 equals no adapter code (those are 0..3)
            if mm * 1000 <= L * rate:
                return p, a
    return n, NONE


def rules_of(adapters, min_overlap=3, rate=100, min_length=1):
    return dict(adapters=[np.asarray(a, np.uint8) for a in adapters], min_overlap=min_overlap, rate=rate, min_length=min_length)


def adapter_model(a: Arrays, rules, begin=None, end=None, keep=None, first=0, n=None):
    """-> begin, end (positions in a.bases), keep, which, stats[13] of records first .. first + n - 1."""
    S = [int(v) for v in a.seq_offsets]
    n = a.n_records - first if n is None else n
    ob, oe, ok, ow = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint8), np.full(n, NONE, np.uint32)
    stats = [0] * 13
    for k in range(n):
        r = first + k
        b, e = (S[r], S[r + 1]) if begin is None else (int(begin[k]), int(end[k]))
        assert S[r] <= b <= e <= S[r + 1]
        keep_in = 1 if keep is None else int(keep[k] != 0)
        ob[k], oe[k] = b, e
        if not keep_in:
            continue
        p, which = adapter_search(a.bases[b:e], rules["adapters"], rules["min_overlap"], rules["rate"])
        oe[k], ow[k] = b + p, which
        ok[k] = 1 if p >= rules["min_length"] else 0
        if which != NONE:
            stats[3] += 1; stats[5 + which] += 1
        if ok[k]:
            stats[0] += 1; stats[1] += p; stats[2] += e - b - p
        else:
            stats[4] += 1
    return ob, oe, ok, ow, stats


# ---- records ---------------------------------------------------------------------------------------------------------------------
def arrays_from_bases(reads):
    """Reads given by their base codes; qualities are 30 throughout, titles @r<i>."""
    lens = np.array([len(x) for x in reads], np.int64)
    titles = [b"@r%d" % i for i in range(len(reads))]
    prefix = lambda v: np.concatenate(([0], np.cumsum(np.asarray(v, np.int64)))).astype(np.uint64)
    bases = np.concatenate([np.asarray(x, np.uint8) for x in reads] + [np.zeros(0, np.uint8)]).astype(np.uint8)
    return Arrays(bases, np.full(len(bases), 30, np.uint8), np.frombuffer(b"".join(titles), np.uint8).copy(), prefix(lens),
                  prefix([len(t) for t in titles]), [0, len(reads)])


def adapter_of(length, rng):
    """C first and no A behind it: in a poly-A read nothing but a planted copy can match below an error rate of 1000."""
    return np.concatenate(([1], rng.integers(1, 4, length - 1))).astype(np.uint8)


def planted(n, A, p, fill=0):
    """A read of n bases `fill` with adapter A written from position p on, cut off at the read's end."""
    x = np.full(n, fill, np.uint8)
    L = max(0, min(len(A), n - p))
    x[p: p + L] = A[:L]
    return x


def mismatch_sets(L, count):
    """`count` positions below L to spoil: window bits 0, 62, 63 and the last compared bit L - 1 first, then from the middle."""
    want = [v for v in (L - 1, 0, 63, 62) if 0 <= v < L]
    order = list(dict.fromkeys(want + list(range(L // 2, L)) + list(range(L // 2))))
    return sorted(order[:count])


def spoil(x, p, A, positions):
    for j in positions:
        x[p + j] = A[j] ^ 1 if (A[j] ^ 1) != 0 else A[j] ^ 2          # another code of A C G T, and not the background's
    return x


# ---- one call ----------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Got:
    error: object
    stats: object
    begin: np.ndarray
    end: np.ndarray
    keep: np.ndarray
    which: np.ndarray
    untouched: bool


def lib_rules(lib, rules, reserved=(0, 0, 0)):
    return lib.AdapterRules([bytes(bytearray(int(v) for v in A)) for A in rules["adapters"]], rules["min_overlap"], rules["rate"], rules["min_length"],
                            reserved)


def adapt_call(lib, h, cin, n, ar, plan=(None, None, None), inplace=False, which=True):
    """One dsrcgpu_columns_adapter_plan.  plan: begin / end / keep as numpy in the coordinates of the staged arrays, or None.  Fresh
    outputs are 0xA5-filled; inplace: every output that has an input counterpart IS that input."""
    with Dev(h) as d:
        pin = [None if v is None else d.up(np.ascontiguousarray(v).astype(dt).tobytes()) for v, dt in zip(plan, (np.uint64, np.uint64, np.uint8))]
        sizes = (8 * n, 8 * n, n)
        fresh = [d.fill(s) for s in sizes]
        out = [pin[i] if inplace and pin[i] is not None else fresh[i] for i in range(3)]
        pw = d.fill(4 * n)
        err = stats = None
        try:
            stats = h.columns_adapter_plan(cin, ar, pin[0], pin[1], pin[2], out[0], out[1], out[2], pw if which else None)
        except lib.DsrcGpuError as e:
            err = e
        raw = [d.down(p, s) for p, s in zip(out, sizes)] + [d.down(pw, 4 * n)]
        raw_fresh = [d.down(p, s) for p, s in zip(fresh, sizes)] + [raw[3]]
    assert all(r[-8:] == b"\xA5" * 8 for r in raw + raw_fresh), "written behind the end of an output array"
    if inplace:                                              # what was not used as an output stayed as it was
        assert all(raw_fresh[i] == b"\xA5" * len(raw_fresh[i]) for i in range(3) if pin[i] is not None)
    if not which:
        assert raw[3] == b"\xA5" * len(raw[3]), "d_which was not given"
    untouched = all(r == b"\xA5" * len(r) for r in raw_fresh)
    return Got(err, stats, np.frombuffer(raw[0], np.uint64)[:n], np.frombuffer(raw[1], np.uint64)[:n], np.frombuffer(raw[2], np.uint8)[:n],
               np.frombuffer(raw[3], np.uint32)[:n], untouched)


def check_adapt(lib, h, st, rules, begin=None, end=None, keep=None, pad=0, first=0, n=None, what=None, inplace=False, which=True, model=None):
    """Arrays staged in `st`, the plan as positions in the UNPADDED arrays (the pad is added here) -> the call == the model."""
    a = st.a
    n = a.n_records - first if n is None else n
    wb, we, wk, ww, ws = model if model is not None else adapter_model(a, rules, begin, end, keep, first, n)
    shift = lambda v: None if v is None else np.asarray(v).astype(np.uint64) + np.uint64(pad)
    got = adapt_call(lib, h, st.cols_in(first, n), n, lib_rules(lib, rules), (shift(begin), shift(end), keep), inplace, which)
    assert got.error is None, (what, got.error)
    bad = np.nonzero((got.begin != wb + np.uint64(pad)) | (got.end != we + np.uint64(pad)) | (got.keep != wk) | ((got.which != ww) if which else False))[0]
    assert len(bad) == 0, (what, "record", int(bad[0]), int(got.begin[bad[0]]) - pad, int(got.end[bad[0]]) - pad, int(got.keep[bad[0]]),
                           int(got.which[bad[0]]), "want", int(wb[bad[0]]), int(we[bad[0]]), int(wk[bad[0]]), int(ww[bad[0]]), len(bad))
    assert got.stats == ws, (what, got.stats, ws)
    return wb, we, wk, ww, ws


def handle(lib):
    return ce.handle(lib, Config.from_levels(0, 0))


def staged(lib, h, a, pad=0):
    return cs.staged(lib, h, a, pad)


# ---- geometry --------------------------------------------------------------------------------------------------------------------
def geometry_reads(la, min_overlap, rng):
    """Adapter length la on every read length: planted at 0, 1, 62, 63, 64, 65, flush with the end, and hanging over the end by every
    amount (la <= 13) or by 1, 2, half, down to min_overlap and one below (longer ones) -> (adapter, reads, expected p or None)."""
    A = adapter_of(la, rng)
    reads, want = [], []
    for n in LENGTHS:
        reads.append(np.zeros(n, np.uint8)); want.append(None)                # nothing planted
        for p in (0, 1, 62, 63, 64, 65, n - la):
            if 0 <= p and p + la <= n:
                reads.append(planted(n, A, p)); want.append(p)
        overlaps = range(1, la) if la <= 13 else sorted({la - 1, la - 2, la // 2, min_overlap + 1, min_overlap, min_overlap - 1} & set(range(1, la)))
        for L in overlaps:
            if L <= n:
                reads.append(planted(n, A, n - L)); want.append(n - L if L >= min_overlap else None)
    return A, reads, want


def run_geometry(lib, sh, la):
    rng = np.random.default_rng(100 + la)
    h = handle(lib)
    try:
        for min_overlap in sorted({1, min(3, la)}):
            A, reads, want = geometry_reads(la, min_overlap, rng)
            a = arrays_from_bases(reads)
            rules = rules_of([A], min_overlap, 0, 0)
            model = adapter_model(a, rules)
            S = a.seq_offsets.astype(np.int64)
            for r, p in enumerate(want):                     # the model alone: every plant is found where it was put, and nothing else
                n = int(S[r + 1] - S[r])
                assert int(model[1][r]) - int(S[r]) == (n if p is None else p) and (model[3][r] == NONE) == (p is None), (la, min_overlap, r, n, p)
            if min_overlap == 1:                             # a read of 64 and of 128 bases (no next tile) with a hit at its last position
                lasts = [r for r, p in enumerate(want) if p is not None and int(S[r + 1] - S[r]) in (64, 128) and p == int(S[r + 1] - S[r]) - 1]
                assert len(lasts) >= 2 or la == 1, la
            assert sum(p is not None for p in want) > len(LENGTHS) and sum(p is None for p in want) >= len(LENGTHS)
            with staged(lib, h, a) as st:
                check_adapt(lib, h, st, rules, what=("geometry", la, min_overlap), model=model)
    finally:
        h.close()


# ---- error budget ------------------------------------------------------------------------------------------------------------------
RATES = [0, 100, 334, 1000]


def budget_reads(la, rate, rng):
    """Full and partial overlaps of one adapter with exactly floor(L * rate / 1000) mismatches (found) and one more (not found
    there), in a poly-A read of 150 bases.  -> adapter, reads, [(p, L, found?)]."""
    A = adapter_of(la, rng)
    reads, want = [], []
    n = 150
    for L in sorted({la, la - 1, la // 2 + 1, 3} & set(range(3, la + 1))):
        p = n - L if L < la else 70
        k = L * rate // 1000
        for count in (k, k + 1):
            if count > L:
                continue
            reads.append(spoil(planted(n, A, p), p, A, mismatch_sets(L, count))); want.append((p, L, count <= k))
    return A, reads, want


def run_budget(lib, sh, rate):
    rng = np.random.default_rng(200 + rate)
    h = handle(lib)
    try:
        for la in (13, 33, 64):
            A, reads, want = budget_reads(la, rate, rng)
            a = arrays_from_bases(reads)
            rules = rules_of([A], 3, rate, 0)
            model = adapter_model(a, rules)
            S = a.seq_offsets.astype(np.int64)
            for r, (p, L, found) in enumerate(want):
                at = int(model[1][r]) - int(S[r])
                if rate == 1000:
                    assert at == 0                           # anything matches at the first position
                elif found:
                    assert at == p, (rate, la, r, p, L, at)
                else:
                    assert at > p, (rate, la, r, p, L, at)   # one mismatch too many: not there (and nowhere in front of it)
            assert rate == 1000 or (any(f for _, _, f in want) and any(not f for _, _, f in want))
            with staged(lib, h, a) as st:
                check_adapt(lib, h, st, rules, what=("budget", rate, la), model=model)
    finally:
        h.close()


def run_budget_edges(lib, sh):
    """A mismatch just outside a partial overlap (bit L) does not count; read codes 4, 18 and 255 inside the adapter are mismatches
    although their two low bits equal the adapter's code there; rate 1000 matches at p = 0 on any non-empty read."""
    A = np.array([1, 0, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3], np.uint8)          # C A G T ...: an A, a G and a T at positions 1, 2, 3
    n, p = 100, 40
    reads = [planted(n, A, p)]
    for code, j in ((4, 1), (18, 2), (255, 3)):
        assert code & 3 == A[j]
        x = planted(n, A, p); x[p + j] = code
        reads.append(x)
    # records 4, 5: the adapter hangs over the end by 5 bases; the next record starts with what does NOT continue it / with what does
    L = 8
    reads += [planted(n, A, n - L), np.concatenate(([A[L] ^ 1], np.zeros(20, np.uint8))).astype(np.uint8),
              planted(n, A, n - L), np.concatenate((A[L:], np.zeros(20, np.uint8))).astype(np.uint8)]
    a = arrays_from_bases(reads)
    S = a.seq_offsets.astype(np.int64)
    at = lambda m, r: int(m[1][r]) - int(S[r])
    h = handle(lib)
    try:
        with staged(lib, h, a) as st:
            strict = rules_of([A], 3, 0, 0)
            m = adapter_model(a, strict)
            assert at(m, 0) == p and [at(m, r) for r in (1, 2, 3)] == [n] * 3 and at(m, 4) == n - L == at(m, 6)
            check_adapt(lib, h, st, strict, what="rate 0", model=m)
            one = rules_of([A], 3, 77, 0)                     # 13 * 77 = 1001: one mismatch in a full overlap, none in 8 bases
            m = adapter_model(a, one)
            assert [at(m, r) for r in (0, 1, 2, 3)] == [p] * 4 and at(m, 4) == n - L
            check_adapt(lib, h, st, one, what="rate 77", model=m)
            longer = rules_of([A], L + 1, 0, 0)               # the overlap is 8 bases whatever lies behind the read's end
            m = adapter_model(a, longer)
            assert at(m, 4) == n == at(m, 6) and m[3][6] == NONE
            check_adapt(lib, h, st, longer, what="min_overlap above the overlap", model=m)
            every = rules_of([A], 1, 1000, 1)
            m = adapter_model(a, every)
            assert all(at(m, r) == 0 for r in range(a.n_records)) and m[4][0] == 0 and m[4][4] == a.n_records
            check_adapt(lib, h, st, every, what="rate 1000", model=m)
        lens = arrays_from_bases([np.full(n_, 4, np.uint8) for n_ in LENGTHS])      # ... on every length, all N
        with staged(lib, h, lens) as st:
            m = adapter_model(lens, every)
            assert m[4][3] == len(LENGTHS) - 1 and m[4][0] == 0 and m[4][4] == len(LENGTHS)      # (the empty read has no position at all)
            check_adapt(lib, h, st, every, what="rate 1000, lengths", model=m)
    finally:
        h.close()


# ---- which hit ---------------------------------------------------------------------------------------------------------------------
def run_which_hit(lib, sh):
    rng = np.random.default_rng(300)
    A, B = adapter_of(20, rng), adapter_of(20, rng)
    B[1:] = (A[1:] % 3) + 1                                  # differs from A everywhere behind the first base
    assert (A[1:] != B[1:]).all()
    n = 200
    reads = []
    reads.append(planted(n, A, 110) | spoil(planted(n, A, 30), 30, A, [4, 11]))      # 0: two errors at 30, perfect at 110: the left one
    reads.append(planted(n, A, 50))                                                   # 1: found by adapters [A, A']: the lower index
    reads.append(planted(n, A, 120) | planted(n, B, 20))                              # 2: B at 20, A at 120: the leftmost, index 1
    reads.append(planted(n, B, 120) | planted(n, A, 20))                              # 3: ... index 0
    reads.append(np.zeros(n, np.uint8))                                               # 4: poly-A (for the poly-A adapter)
    reads.append(planted(n, B, 70) | planted(n, A, 100))                              # 5: different adapters in lanes 6 and 36 of tile 1
    reads.append(planted(n, A, 3) | planted(n, B, 40))                                # 6: ... lanes 3 and 40 of tile 0
    a = arrays_from_bases(reads)
    S = a.seq_offsets.astype(np.int64)
    at = lambda m, r: (int(m[1][r]) - int(S[r]), int(m[3][r]))
    h = handle(lib)
    try:
        with staged(lib, h, a) as st:
            r1 = rules_of([A, B], 3, 100, 1)
            m = adapter_model(a, r1)
            assert at(m, 0) == (30, 0) and at(m, 2) == (20, 1) and at(m, 3) == (20, 0) and at(m, 5) == (70, 1) and at(m, 6) == (3, 0)
            assert at(m, 4) == (n, NONE)
            check_adapt(lib, h, st, r1, what="A, B", model=m)
            m = check_adapt(lib, h, st, rules_of([B, A], 3, 100, 1), what="B, A")
            assert at(m, 2) == (20, 0) and at(m, 3) == (20, 1) and at(m, 5) == (70, 0)
            same = rules_of([A, A.copy(), A[:10]], 3, 100, 1)
            m = adapter_model(a, same)
            assert at(m, 1) == (50, 0) and m[4][5] > 0 and m[4][6] == 0 and m[4][7] == 0
            check_adapt(lib, h, st, same, what="the same adapter twice", model=m)
            m = adapter_model(a, rules_of([A[:10], A], 3, 100, 1))
            assert at(m, 1) == (50, 0)
            poly = rules_of([np.zeros(12, np.uint8)], 3, 0, 1)
            m = adapter_model(a, poly)
            assert at(m, 4) == (0, 0) and m[0][4] == m[1][4] and m[2][4] == 0 and m[4][4] >= 1       # an empty range, dropped for length
            check_adapt(lib, h, st, poly, what="poly-A", model=m)
    finally:
        h.close()


# ---- ranges in -----------------------------------------------------------------------------------------------------------------------
def run_ranges(lib, sh):
    rng = np.random.default_rng(400)
    A = adapter_of(16, rng)
    n = 260
    reads, begin, end, want = [], [], [], []

    def add(x, b, e, p, why):
        reads.append(x); begin.append(b); end.append(e); want.append((p, why))
    for shift in (1, 63, 64):                                # tiles count from b: the same plant at b + 0, 1, 62 .. 65
        for p in (0, 1, 62, 63, 64, 65):
            add(planted(n, A, shift + p), shift, n, p, "b = S + %d" % shift)
    add(planted(n, A, 10), 26, n, None, "wholly in front of b")
    add(planted(n, A, 11), 26, n, None, "in front of b but for its last base")
    add(planted(n, A, 200), 0, 200, None, "wholly behind e")
    add(planted(n, A, 190), 0, 200, 190, "10 of its bases in front of e")
    add(planted(n, A, 198), 0, 200, None, "2 of its bases in front of e: below min_overlap")
    add(planted(n, A, 100), 50, 50, None, "empty range")
    add(planted(n, A, 0), 0, 0, None, "empty range at the record's start")
    add(planted(n, A, n - 5), n, n, None, "empty range at the record's end")
    add(planted(n, A, n - 8), 0, n, n - 8, "hangs over the record's end")
    add(np.concatenate((A[8:], np.zeros(30, np.uint8))), 0, 38, None, "the continuation, first in the next record")
    add(np.zeros(0, np.uint8), 0, 0, None, "no bases")
    add(planted(n, A, n - 16), 3, n, n - 16 - 3, "the last record, flush with bases_len")
    a = arrays_from_bases(reads)
    S = a.seq_offsets.astype(np.int64)
    assert int(S[-1]) == len(a.bases)
    gb = S[:-1] + np.array(begin); ge = S[:-1] + np.array(end)
    rules = rules_of([A], 3, 0, 0)
    m = adapter_model(a, rules, gb, ge)
    for r, (p, why) in enumerate(want):
        assert int(m[0][r]) == gb[r] and int(m[1][r]) == (ge[r] if p is None else gb[r] + p), (why, r)
    keep = np.ones(a.n_records, np.uint8); keep[[2, 9, 20]] = 0
    h = handle(lib)
    try:
        for pad in (0, 5):
            with staged(lib, h, a, pad=pad) as st:
                check_adapt(lib, h, st, rules, gb, ge, pad=pad, what=("ranges", pad), model=m)
                check_adapt(lib, h, st, rules, gb, ge, keep, pad=pad, what=("ranges, keep", pad))
                check_adapt(lib, h, st, rules, pad=pad, what=("whole reads", pad))
                check_adapt(lib, h, st, rules, None, None, keep, pad=pad, what=("whole reads, keep", pad))
                for first, cnt in ((5, None), (a.n_records - 1, 1), (17, 9)):       # d_seq_offs + k
                    sl = slice(first, None if cnt is None else first + cnt)
                    check_adapt(lib, h, st, rules, gb[sl], ge[sl], keep[sl], pad=pad, first=first, n=cnt, what=("first", first, pad))
                    check_adapt(lib, h, st, rules, pad=pad, first=first, n=cnt, what=("first, whole", first, pad))
    finally:
        h.close()


# ---- keep, min_length, in place, d_which, statistics -----------------------------------------------------------------------------------
def run_keep_and_inplace(lib, sh):
    rng = np.random.default_rng(500)
    ads = [adapter_of(int(L), rng) for L in (12, 9, 20, 15, 10, 31, 8, 64)]
    n_rec = 90
    reads = []
    for r in range(n_rec):
        n = int(rng.integers(80, 140))
        x = planted(n, ads[r % 8], int(rng.integers(20, n - 4))) if r % 9 else np.zeros(n, np.uint8)
        reads.append(x)
    reads[3] = planted(100, ads[3], 40); reads[4] = planted(100, ads[4], 41); reads[5] = planted(100, ads[5], 39)
    a = arrays_from_bases(reads)
    S = a.seq_offsets.astype(np.int64)
    begin = S[:-1] + rng.integers(0, 5, n_rec); end = S[1:] - rng.integers(0, 3, n_rec)
    begin[3:6] = S[3:6]; end[3:6] = S[4:7]
    keep = (rng.random(n_rec) < 0.7).astype(np.uint8) * np.array([1, 7, 255] * 30, np.uint8)      # (any non-zero byte keeps)
    keep[3:6] = 1
    begin[7] = end[7] = S[7] + 9; keep[7] = 1                # an empty range that comes in kept: no search, dropped for length
    begin[8] = end[8] = S[9]; keep[8] = 0
    rules = rules_of(ads, 3, 0, 40)
    m = adapter_model(a, rules, begin, end, keep)
    assert [int(m[2][r]) for r in (3, 4, 5)] == [1, 1, 0] and [int(m[1][r] - m[0][r]) for r in (3, 4, 5)] == [40, 41, 39]      # min_length exact, one above, one below
    assert all(m[4][5 + k] > 0 for k in range(8)) and sum(m[4][5:]) == m[4][3] and m[4][4] > 0 and m[4][0] + m[4][4] == int((keep != 0).sum())
    dropped = np.nonzero(keep == 0)[0]
    assert len(dropped) > 5 and (m[2][dropped] == 0).all() and (m[3][dropped] == NONE).all() and (m[1][dropped] == end[dropped]).all()
    h = handle(lib)
    try:
        with staged(lib, h, a) as st:
            for inplace in (False, True):
                check_adapt(lib, h, st, rules, begin, end, keep, what=("all three", inplace), inplace=inplace, model=m)
                check_adapt(lib, h, st, rules, begin, end, None, what=("no keep", inplace), inplace=inplace)
                check_adapt(lib, h, st, rules, None, None, keep, what=("no range", inplace), inplace=inplace)
            check_adapt(lib, h, st, rules, begin, end, keep, what="no d_which", which=False, model=m)
            check_adapt(lib, h, st, rules, begin, end, keep, what="no d_which, in place", which=False, inplace=True, model=m)
            # d_quals, d_titles and d_title_offs are not read
            cin = st.cols_in()
            cin = lib.ColumnsIn(cin.d_bases, cin.bases_len, None, None, 0, cin.d_seq_offs, None, a.n_records)
            got = adapt_call(lib, h, cin, a.n_records, lib_rules(lib, rules), (begin.astype(np.uint64), end.astype(np.uint64), keep))
            assert got.error is None and got.stats == m[4] and np.array_equal(got.end, m[1]) and np.array_equal(got.keep, m[2]) and np.array_equal(got.which, m[3])
    finally:
        h.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def run_arg_refusals(lib, sh):
    rng = np.random.default_rng(600)
    A = adapter_of(12, rng)
    a = fuzz_arrays(0, 20)[0]
    good = rules_of([A, A[:7]], 3, 100, 1)
    h = handle(lib)

    def broken():
        mk = lambda **kw: lib_rules(lib, dict(good, **kw))
        yield "no adapters", mk(adapters=[])
        yield "nine adapters", mk(adapters=[A] * 9)
        ar = mk(); ar.adapter_len[1] = 0
        yield "a length of 0", ar
        yield "a length of 65", mk(adapters=[A, np.ones(65, np.uint8)])
        ar = mk(); ar.adapter_len[2] = 4
        yield "a length behind n_adapters", ar
        ar = mk(); ar.adapter_len[7] = 1
        yield "a length in the last slot", ar
        yield "code 4", mk(adapters=[A, np.array([1, 2, 4, 3], np.uint8)])
        yield "code 255 in the last position", mk(adapters=[np.concatenate((A, [255])).astype(np.uint8)])
        yield "min_overlap 0", mk(min_overlap=0)
        yield "min_overlap above the shortest", mk(min_overlap=8)
        yield "permille 1001", mk(rate=1001)
        for k in range(3):
            res = [0, 0, 0]; res[k] = 1
            yield "reserved[%d]" % k, lib_rules(lib, good, res)
    try:
        with staged(lib, h, a) as st:
            n = a.n_records
            S = a.seq_offsets
            checked = 0
            for name, ar in broken():
                got = adapt_call(lib, h, st.cols_in(), n, ar)
                assert got.error is not None and got.error.code == E_ARG and got.untouched, (name, got.error)
                checked += 1
            assert checked == 14
            for name, plan in (("begin alone", (S[:-1], None, None)), ("end alone", (None, S[1:], None))):
                got = adapt_call(lib, h, st.cols_in(), n, lib_rules(lib, good), plan)
                assert got.error is not None and got.error.code == E_ARG and got.untouched, (name, got.error)
            check_adapt(lib, h, st, good, what="the same handle, clean")
            check_adapt(lib, h, st, dict(good, min_overlap=7, rate=1000), what="the largest figures")
            got = adapt_call(lib, h, st.cols_in(3, 0), 0, lib_rules(lib, good))          # no records
            assert got.error is None and got.stats == [0] * 13 and got.untouched
    finally:
        h.close()
    hc = ce.handle(lib, dataclasses.replace(Config.from_levels(0, 0), color_space=True))
    try:
        with staged(lib, hc, a) as st:
            got = adapt_call(lib, hc, st.cols_in(), a.n_records, lib_rules(lib, good))
            assert got.error is not None and got.error.code == E_ARG and got.untouched
    finally:
        hc.close()


def run_input_errors(lib, sh):
    """The plants of the select's input errors in the first, a middle and the last record, kept and dropped ones: code, record,
    outputs still 0xA5, and the same handle plans the clean arrays afterwards."""
    a, begin, end, keep, rules = fuzz_arrays(1, 41)
    keep = np.ones(a.n_records, np.uint8); keep[20] = 0; keep[40] = 0
    pad = 4
    n = a.n_records
    S = lambda r: int(a.seq_offsets[r]) + pad
    for r in (0, 20, 40):                                    # (the range plants need a base)
        if S(r + 1) == S(r):
            raise AssertionError("record %d has no bases: choose another seed" % r)
    hb, he = begin + np.uint64(pad), end + np.uint64(pad)
    ar = lib_rules(lib, rules)
    h = handle(lib)
    checked = 0
    try:
        with staged(lib, h, a, pad=pad) as st:
            offs = [("order", lambda r: st.poke("seq_offs", r + 1, S(r) - 1, np.uint64), "not non-decreasing"),
                    ("end", lambda r: st.poke("seq_offs", r + 1, len(a.bases) + pad + 5, np.uint64), "above bases_len"),
                    ("wild", lambda r: st.poke("seq_offs", r + 1, 2 ** 64 - 1, np.uint64), "above bases_len")]
            for name, plant, word in offs:
                for r in (0, 20, 40):
                    plant(r)
                    for plan in ((None, None, None), (hb, he, keep)):
                        got = adapt_call(lib, h, st.cols_in(), n, ar, plan)
                        assert got.error is not None and got.error.code == E_INPUT and got.untouched, (name, r, got.error)
                        assert "record %d:" % r in str(got.error) and word in str(got.error), (name, r, str(got.error))
                    st.restore()
                    checked += 1
                check_adapt(lib, h, st, rules, begin, end, keep, pad=pad, what=("after", name))

            def ranged(r, b=None, e=None):
                pb, pe = hb.copy(), he.copy()
                if b is not None: pb[r] = b
                if e is not None: pe[r] = e
                return pb, pe, keep
            ranges = [("begin low", lambda r: ranged(r, b=S(r) - 1), "d_begin lies below"),
                      ("end high", lambda r: ranged(r, e=S(r + 1) + 1), "d_end lies above"),
                      ("end wild", lambda r: ranged(r, e=2 ** 64 - 1), "d_end lies above"),
                      ("begin above end", lambda r: ranged(r, b=S(r + 1), e=S(r + 1) - 1), "d_begin lies above d_end")]
            for name, plan_of, word in ranges:
                for r in (0, 20, 40):
                    for inplace in (False, True):
                        got = adapt_call(lib, h, st.cols_in(), n, ar, plan_of(r), inplace=inplace)
                        assert got.error is not None and got.error.code == E_INPUT, (name, r, got.error)
                        assert "record %d:" % r in str(got.error) and word in str(got.error), (name, r, str(got.error))
                        if inplace:                          # the plan itself is what it was
                            pb, pe, pk = plan_of(r)
                            assert np.array_equal(got.begin, pb) and np.array_equal(got.end, pe) and np.array_equal(got.keep, pk)
                        else:
                            assert got.untouched, (name, r)
                    checked += 1
                check_adapt(lib, h, st, rules, begin, end, keep, pad=pad, what=("after", name))
    finally:
        h.close()
    assert checked == 21


def run_codec_state(lib, sh):
    """The call touches nothing the codec carries: the fields capacity stays, a pending record layout stays pending, and the text
    call that follows writes what it writes on a fresh handle seeded alike."""
    a, begin, end, keep, rules = fuzz_arrays(2, 80)
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
                check_adapt(lib, h, st, rules, begin, end, keep)
                assert h.get_fields_capacity() == 11
            assert text_blocks(h) == text_blocks(fresh), layout
        finally:
            h.close(); fresh.close()


# ---- record counts -----------------------------------------------------------------------------------------------------------------
def run_count(lib, sh, n_rec):
    """n_rec reads of 10 bases, two adapters, a plan in."""
    rng = np.random.default_rng(700 + n_rec)
    ads = [np.array([1, 2, 3, 1], np.uint8), np.array([3, 3, 2, 1, 1], np.uint8)]
    bases = rng.integers(0, 4, (n_rec, 10)).astype(np.uint8)
    hit = rng.random(n_rec)
    at = rng.integers(0, 9, n_rec)
    for r in np.nonzero(hit < 0.5)[0]:
        A = ads[int(hit[r] < 0.2)]
        L = min(len(A), 10 - at[r])
        bases[r, at[r]: at[r] + L] = A[:L]
    bases[rng.random((n_rec, 10)) < 0.03] = 4
    S = (10 * np.arange(n_rec + 1)).astype(np.uint64)
    titles = np.empty(2 * n_rec, np.uint8); titles[0::2] = ord("@"); titles[1::2] = ord("t")
    a = Arrays(bases.reshape(-1), np.full(10 * n_rec, 30, np.uint8), titles, S, (2 * np.arange(n_rec + 1)).astype(np.uint64), [0, n_rec])
    begin = S[:-1] + rng.integers(0, 3, n_rec).astype(np.uint64)
    end = S[1:] - rng.integers(0, 3, n_rec).astype(np.uint64)
    keep = (rng.random(n_rec) < 0.8).astype(np.uint8)
    rules = rules_of(ads, 3, 0, 4)
    m = adapter_model(a, rules, begin, end, keep)
    if n_rec >= 63:
        assert m[4][5] > 0 and m[4][6] > 0 and m[4][4] > 0 and m[4][0] > 0
    h = handle(lib)
    try:
        with staged(lib, h, a) as st:
            check_adapt(lib, h, st, rules, begin, end, keep, what=n_rec, model=m)
            check_adapt(lib, h, st, rules, begin, end, keep, what=(n_rec, "in place"), inplace=True, model=m)
    finally:
        h.close()


# ---- fuzz ------------------------------------------------------------------------------------------------------------------------
def fuzz_arrays(seed, n_rec, max_len=300):
    """Lengths 0 .. max_len, 1 .. 4 adapters of mixed lengths, about 70 % of the reads with one of them planted at a random position
    (it may hang over the end) and about 8 % of its bases substituted, about 10 % of the read codes >= 4, random ranges and keep
    flags -> (arrays, begin, end, keep, rules)."""
    rng = np.random.default_rng(2000 + seed)
    k = 4 - seed % 4                                         # 4, 3, 2, 1, 4, ... adapters
    ads = [rng.integers(0, 4, int(rng.integers(8, 65))).astype(np.uint8) for _ in range(k)]
    other = np.concatenate([[4, 4, 255], np.arange(5, 19)]).astype(np.uint8)
    reads = []
    for _ in range(n_rec):
        n = int(rng.integers(0, max_len + 1))
        x = rng.integers(0, 4, n).astype(np.uint8)
        amb = rng.random(n) < 0.1
        x[amb] = other[rng.integers(0, len(other), int(amb.sum()))]
        if n and rng.random() < 0.7:                         # (planted over the read as drawn: the copy itself holds A C G T only)
            A = ads[int(rng.integers(0, k))].copy()
            sub = rng.random(len(A)) < 0.08
            A[sub] = (A[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
            p = int(rng.integers(0, n))
            L = min(len(A), n - p)
            x[p: p + L] = A[:L]
        reads.append(x)
    a = arrays_from_bases(reads)
    S = a.seq_offsets.astype(np.int64)
    lens = S[1:] - S[:-1]
    whole = rng.random(n_rec) < 0.5
    cut5 = np.where(whole, 0, (rng.random(n_rec) * (lens + 1) * 0.2).astype(np.int64))
    cut3 = np.where(whole, 0, (rng.random(n_rec) * (lens - cut5 + 1) * 0.2).astype(np.int64))
    begin = (S[:-1] + cut5).astype(np.uint64); end = (S[1:] - cut3).astype(np.uint64)
    keep = (rng.random(n_rec) < 0.85).astype(np.uint8)
    return a, begin, end, keep, rules_of(ads, int(rng.integers(3, 7)), int(rng.choice([100, 120, 200])), int(rng.integers(0, 60)))


def run_fuzz(lib, sh, seed):
    n_rec = sh["adapt_fuzz"][1]
    a, begin, end, keep, rules = fuzz_arrays(seed, n_rec)
    m = adapter_model(a, rules, begin, end, keep)
    found = int((m[3] != NONE).sum()); same = int(((m[1] == end) & (keep != 0)).sum())
    print("adapter fuzz", seed, "adapters", [len(A) for A in rules["adapters"]], "found in", found, "untouched", same, "of", n_rec, "stats", m[4])
    assert 3 * found >= n_rec and 10 * same >= n_rec
    assert int((a.bases >= 4).sum()) * 14 >= len(a.bases)
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=3) as st:
            check_adapt(lib, h, st, rules, begin, end, keep, pad=3, what=("fuzz", seed), model=m)
            check_adapt(lib, h, st, rules, pad=3, what=("fuzz, whole reads", seed))
    finally:
        h.close()


# ---- the Python layers and the closed loop ---------------------------------------------------------------------------------------------
ADAPTER = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"          # 33 bases (the read-1 adapter of Illumina's TruSeq kits, public)


def codes_of(s):
    return np.array(["ACGT".index(ch) for ch in s.upper()], np.uint8)


def tensors(a, device):
    from dsrc_amd import columns
    t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v).astype(dt)).to(device)
    return columns.RecordColumns(t(a.bases, np.uint8), t(a.quals, np.uint8), t(a.titles, np.uint8), t(a.seq_offsets, np.int64),
                                 t(a.title_offsets, np.int64), torch.tensor([0, a.n_records]))


def run_python_layers(lib, sh, device):
    from dsrc_amd import columns
    a, begin, end, keep, rules = fuzz_arrays(3, 120)
    strs = ["".join("ACGT"[v] for v in A) for A in rules["adapters"]]
    kw = dict(min_overlap=rules["min_overlap"], max_error_permille=rules["rate"], min_length=rules["min_length"])
    h = handle(lib)
    try:
        c = tensors(a, device)
        t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v).astype(dt)).to(device)
        tb, te, tk = t(begin, np.int64), t(end, np.int64), t(keep, np.uint8)
        for ads in (strs, [s.lower() for s in strs], [A.tolist() for A in rules["adapters"]], [bytes(A.tolist()) for A in rules["adapters"]]):
            m = adapter_model(a, rules, begin, end, keep)
            b, e, k, stats, which = columns.adapter_plan(h, c, ads, tb, te, tk, return_which=True, **kw)
            assert b.dtype == torch.int64 and k.dtype == torch.uint8 and which.dtype == torch.int64 and k.device.type == torch.device(device).type
            assert b.data_ptr() != tb.data_ptr() and torch.equal(tb, t(begin, np.int64)) and torch.equal(tk, t(keep, np.uint8))      # fresh tensors, inputs as they were
            assert list(stats) == list(lib.ADAPTER_STATS) and list(stats.values()) == m[4]
            assert np.array_equal(b.cpu().numpy().astype(np.uint64), m[0]) and np.array_equal(e.cpu().numpy().astype(np.uint64), m[1])
            assert np.array_equal(k.cpu().numpy(), m[2]) and np.array_equal(which.cpu().numpy(), np.where(m[3] == NONE, -1, m[3].astype(np.int64)))
        m = adapter_model(a, rules)
        got = columns.adapter_plan(h, c, strs, **kw)
        assert len(got) == 4 and list(got[3].values()) == m[4] and np.array_equal(got[1].cpu().numpy().astype(np.uint64), m[1])

        class Never:                                         # ValueError comes before any library call
            def __getattr__(self, name):
                raise AssertionError("the library was called")
        for bad in (["ACGN"], [], ["ACGT", ""], ["A" * 65], ["ACGT"] * 9, "ACGT", [[0, 1, 4]], [[0, -1]], [None], [b"\x00\x01\x09"]):
            for call in (lambda: columns.adapter_plan(Never(), c, bad), lambda: columns.filter_columns(Never(), c, adapters=bad, quality_3=20)):
                try:
                    call()
                except ValueError:
                    pass
                else:
                    raise AssertionError("no ValueError for adapters=%r" % (bad,))
        for bad_kw in (dict(min_overlap=0), dict(min_overlap=5), dict(max_error_permille=1001), dict(min_length=-1)):
            try:
                columns.adapter_plan(Never(), c, ["ACGT"], **bad_kw)
            except ValueError:
                pass
            else:
                raise AssertionError("no ValueError for %r" % (bad_kw,))
    finally:
        h.close()


def filter_reads(n_rec, seed=11):
    """Reads with qualities that fall off at the 3' end and, a third of them, an adapter tail -> (arrays, texts of the records)."""
    rng = np.random.default_rng(seed)
    A = codes_of(ADAPTER)
    records = []
    for r in range(n_rec):
        n = int(rng.integers(40, 120))
        x = rng.integers(0, 4, n).astype(np.uint8)
        if r % 3 == 0:
            p = int(rng.integers(5, n))
            L = min(len(A), n - p)
            x[p: p + L] = A[:L]
            if L > 12 and rng.random() < 0.5:
                x[p + int(rng.integers(0, L))] ^= 1
        x[rng.random(n) < 0.01] = 4
        q = rng.integers(25, 41, n)
        low = int(rng.integers(0, 12)) if rng.random() < 0.6 else 0
        if low: q[n - low:] = rng.integers(2, 12, low)
        lead = int(rng.integers(0, 6)) if rng.random() < 0.3 else 0
        if lead: q[:lead] = rng.integers(2, 12, lead)
        records.append((b"@read.%d len=%d" % (r + 1, n), bytes(b"ACGTN"[v] for v in x), bytes((q + 33).astype(np.uint8))))
    text = b"\n".join(t + b"\n" + s + b"\n+\n" + q for t, s, q in records)
    return ce.arrays_of([text]), records, text


def filter_model(a, trim_rules, adapters, min_overlap=3, rate=100):
    """model-quality-plan -> model-adapter-plan: begin, end, keep, the stats dict filter_columns returns."""
    b, e, k, ts = cs.plan_model(a, trim_rules)
    ar = rules_of([codes_of(s) for s in adapters], min_overlap, rate, trim_rules["min_length"])
    b2, e2, k2, _, as_ = adapter_model(a, ar, b, e, k)
    stats = dict(zip(TRIM_STATS, ts)); stats["adapter"] = dict(zip(ADAPTER_STATS, as_))
    return b2, e2, k2, stats


TRIM_STATS = ("records_kept", "bases_kept", "bases_cut", "dropped_length", "dropped_n", "dropped_mean_quality")
ADAPTER_STATS = ("records_kept", "bases_kept", "bases_cut", "records_trimmed", "dropped_length") + tuple("found_%d" % i for i in range(8))


def run_filter_columns(lib, sh, device):
    from dsrc_amd import columns
    a, _, _ = filter_reads(200)
    trim = cs.rules_of(15, 20, min_length=30, max_n=2, min_mean_quality=20)
    second = "ctgtctcttatacacatct"
    h = handle(lib)
    try:
        assert tuple(lib.ADAPTER_STATS) == ADAPTER_STATS and tuple(lib.TRIM_STATS) == TRIM_STATS
        c = tensors(a, device)
        # without adapters: today's result
        b, e, k, ts = cs.plan_model(a, trim)
        want = cs.select_model(a, b, e, k)
        sel, stats = columns.filter_columns(h, c, **trim)
        assert stats == dict(zip(TRIM_STATS, ts)) and "adapter" not in stats
        same = lambda sel, want: all(np.array_equal(g.cpu().numpy().astype(w.dtype), w) for g, w in
                                     zip((sel.bases, sel.quals, sel.titles, sel.seq_offsets, sel.title_offsets), want[:5]))
        assert same(sel, want) and sel.n_records == ts[0]
        sel, stats = columns.filter_columns(h, c, adapters=None, **trim)
        assert same(sel, want) and "adapter" not in stats
        # with adapters: quality first, adapter second, then the select
        for ads, mo, rate in (([ADAPTER], 3, 100), ([second, ADAPTER], 5, 0)):
            b2, e2, k2, wstats = filter_model(a, trim, ads, mo, rate)
            assert wstats["adapter"]["records_trimmed"] >= 20 and wstats["adapter"]["dropped_length"] > 0 and 0 < wstats["adapter"]["records_kept"] < ts[0]
            want2 = cs.select_model(a, b2, e2, k2)
            sel, stats = columns.filter_columns(h, c, adapters=ads, adapter_min_overlap=mo, adapter_max_error_permille=rate, **trim)
            assert stats == wstats and list(stats)[:6] == list(TRIM_STATS), (stats, wstats)
            assert same(sel, want2) and sel.n_records == wstats["adapter"]["records_kept"] and sel.block_records.tolist() == [0, sel.n_records]
            sel, _ = columns.filter_columns(h, c, titles=False, adapters=ads, adapter_min_overlap=mo, adapter_max_error_permille=rate, **trim)
            assert sel.titles.numel() == 0 and np.array_equal(sel.bases.cpu().numpy(), want2[0])
    finally:
        h.close()


def run_closed_loop(lib, sh, device):
    """Records written here -> the oracle's block -> decode_columns -> filter_columns(quality_3, adapters) -> encode_columns == the
    oracle's block of the text of the model-filtered records, lossless -d3 -q2 with CRC."""
    from dsrc_amd import columns
    cfg = ce.BLOCK_CFG
    a, records, text = filter_reads(300, seed=12)
    trim = cs.rules_of(0, 20, min_length=35)
    b, e, k, wstats = filter_model(a, trim, [ADAPTER])
    S = a.seq_offsets.astype(np.int64)
    kept = [(t, s[int(b[r] - S[r]): int(e[r] - S[r])], q[int(b[r] - S[r]): int(e[r] - S[r])]) for r, (t, s, q) in enumerate(records) if k[r]]
    print("closed loop: model stats", wstats)
    assert 60 <= wstats["adapter"]["records_trimmed"] and wstats["bases_cut"] > 0 and 0 < len(kept) < wstats["records_kept"] < len(records)
    src = ce.oracle_blocks(cfg, [text]); want = ce.oracle_blocks(cfg, [b"\n".join(t + b"\n" + s + b"\n+\n" + q for t, s, q in kept)])
    assert src is not None and want is not None
    d_blocks, offs = cs._stage_blocks([src[0][0]], device)
    h = ce.handle(lib, cfg)
    try:
        rc = columns.decode_columns(h, d_blocks, offs, [len(src[0][0])], device)
        assert rc.n_records == len(records)
        sel, stats = columns.filter_columns(h, rc, adapters=[ADAPTER], **trim)
        assert stats == wstats and sel.n_records == len(kept)
        h.set_fields_capacity(0)
        blocks, o_offs, o_sizes, _ = columns.encode_columns(h, sel, block_records=sel.block_records)
        host = blocks.cpu().numpy().tobytes()
        assert [host[o: o + s] for o, s in zip(o_offs, o_sizes)] == [want[0][0]]
    finally:
        h.close()
