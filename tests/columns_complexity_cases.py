"""Shared by tests/test_emu_columns_complexity.py (CPU, emulator build) and tests/test_gpu_columns_complexity.py (MI355X): the cases
of the columnar complexity plan (dsrcgpu_columns_complexity_plan; dsrc_amd/csrc/k_columns_complexity.h) and what they must give.

The reference has no counterpart, so the yardstick is the integer model written out here: poly_run_serial() is the serial rule of
include/dsrc_gpu.h word for word, poly_run() the same rule in numpy (the two are compared in test_model_forms_agree before
anything else relies on the fast one), dust_windows() and complexity_of() the two scores, complexity_model() applies them to a plan.
None of it comes from the library under test, and every comparison is exact equality.  Output arrays are filled with 0xA5 before a
call, so that "nothing written" can be asserted.  Before the library is compared on a crafted case the model alone is asked what
that case is for.

Shapes.  The emulator pays a coroutine switch per wave exchange, so its fuzz is 2 seeds x 150 records where the GPU runs 6 x 2000.
The planner's grid is the adapter plan's (the shared grid helper), so the count that takes the grid stride into a second round is
the adapter cases' stride_count -- it runs on the GPU only.

One case of the issue cannot be built as it is worded: a window of 64 positions holds 62 triplets, so the 64 triplet codes cannot
all be present in ONE window, let alone with distinct counts.  What stands in for it (run_dust_triplets): a de Bruijn sequence in
which every code occurs once, each code in a window where it is the only repeated one (the DUST sum is symmetric in the counts, so
only a mapping that merges or loses a code can show, and this shows it for every code), and windows with counts 1 .. 10 of ten
different codes."""
from __future__ import annotations

import dataclasses

import numpy as np
import torch        # noqa: F401  before the first handle (see columns_cases)

from tests import columns_adapt_cases as ca
from tests import columns_enc_cases as ce
from tests import columns_pair_cases as cp
from tests import columns_sel_cases as cs
from tests._oracle import Config
from tests.cases import TINY
from tests import columns_cases as cc

E_ARG, E_INPUT = cs.E_ARG, cs.E_INPUT
NONE = 255
OFF = 0xFFFFFFFF

SHAPES = {
    "gpu": dict(ca.SHAPES["gpu"], cplx_fuzz=(6, 2000)),
    "emu": dict(ca.SHAPES["emu"], cplx_fuzz=(2, 150)),
}
Arrays = ce.Arrays
Dev = cs.Dev
LENGTHS = [0, 1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 200, 4097]
DUST_LENGTHS = [2, 3, 4, 63, 64, 65, 95, 96, 97, 100, 128, 129, 200]
RATES = [0, 125, 334, 1000]
STATS = ("records_kept", "bases_kept", "bases_cut_5", "bases_cut_3", "records_head_cut", "records_tail_cut", "tail_A", "tail_C", "tail_G", "tail_T",
         "head_A", "head_C", "head_G", "head_T", "dropped_length", "dropped_complexity", "dropped_dust")
arrays_from_bases = ca.arrays_from_bases


# ---- the model -------------------------------------------------------------------------------------------------------------------
def poly_run_serial(x, X, rate, from_end=True):
    """The serial rule for one base at one end of the range x -> the run's length before poly_min_length is applied."""
    n = len(x)
    best, run, m, err = 0, 0, 0, 0
    for k in range(n):                                       # k: the distance from that end
        if int(x[n - 1 - k] if from_end else x[k]) == X:
            m += 1
        else:
            err += 1
        L = k + 1
        score = m - 2 * err
        if score > best and err * 1000 <= L * rate:
            best, run = score, L
    return run


def poly_run(x, X, rate, from_end=True):
    """The same in numpy: the highest score among the positions within the budget, if above 0, at the first position that has it."""
    n = len(x)
    if n == 0:
        return 0
    hit = (x[::-1] if from_end else x) == X
    m = np.cumsum(hit, dtype=np.int64)
    L = np.arange(1, n + 1, dtype=np.int64)
    err = L - m
    score = np.where(err * 1000 <= L * rate, m - 2 * err, -1)
    at = int(np.argmax(score))                               # (the first of equal maxima)
    return at + 1 if score[at] > 0 else 0


def poly_end(x, mask, min_run, rate, from_end):
    """-> (run length, base) of that end: the longest of the masks' runs of at least min_run positions, (0, NONE) for none."""
    got = (0, NONE)
    for X in range(4):
        if mask >> X & 1:
            t = poly_run(x, X, rate, from_end)
            if t >= min_run and t > got[0]:
                got = (t, X)
    return got


def complexity_of(x):
    """-> (d, cp) of fastp's measure on the codes as they are."""
    n = len(x)
    d = int(np.count_nonzero(x[:-1] != x[1:])) if n >= 2 else 0
    return d, (d * 1000 // (n - 1) if n >= 2 else 1000)


def window_starts(n):
    if n < 64:
        return [0]
    starts = list(range(0, n - 64 + 1, 32))
    if (n - 64) % 32:
        starts.append(n - 64)
    return starts


def dust_windows(x):
    """-> the DUST value of every window of x, in the order of window_starts."""
    n = len(x)
    out = []
    xi = x.astype(np.int64)
    for s in window_starts(n):
        wdw = xi[s: s + min(64, n)]
        if len(wdw) < 3:
            out.append(0); continue
        a, b, c = wdw[:-2], wdw[1:-1], wdw[2:]
        ok = (a < 4) & (b < 4) & (c < 4)
        counts = np.bincount((16 * a + 4 * b + c)[ok], minlength=64)
        l, S = int(counts.sum()), int((counts * (counts - 1) // 2).sum())
        out.append(10 * S // (l - 1) if l >= 2 else 0)
    return out


def rules_of(tail="", head="", poly_min=10, rate=125, min_length=1, min_cp=0, max_dust=None, max_windows=0):
    mask = lambda s: sum(1 << "ACGT".index(ch) for ch in s)
    return dict(tail=mask(tail), head=mask(head), poly_min=poly_min, rate=rate, min_length=min_length, min_cp=min_cp, max_dust=max_dust,
                max_windows=max_windows)


def read_model(x, R):
    """One range that came in kept -> (new begin, new end) relative to x, keep, info0, info1, the 20 statistics of this record."""
    n = len(x)
    t, tb = poly_end(x, R["tail"], R["poly_min"], R["rate"], True)
    hd, hb = poly_end(x, R["head"], R["poly_min"], R["rate"], False)
    nb, ne = (0, 0) if hd + t >= n else (hd, n - t)
    y = x[nb:ne]
    n2 = len(y)
    d, cpm = complexity_of(y)
    vs = dust_windows(y)
    dust = max(vs)
    over = 0 if R["max_dust"] is None else sum(v > R["max_dust"] for v in vs)
    why = 14 if n2 < R["min_length"] else 15 if n2 >= 2 and d * 1000 < R["min_cp"] * (n2 - 1) else 16 if over > R["max_windows"] else 0
    st = [0] * 20
    if why:
        st[why] = 1
    else:
        st[0], st[1], st[2], st[3] = 1, n2, nb, n - ne
    if hd:
        st[4] = 1; st[10 + hb] = 1
    if t:
        st[5] = 1; st[6 + tb] = 1
    return nb, ne, 0 if why else 1, hb | tb << 8, cpm | dust << 16, st


def complexity_model(a: Arrays, R, begin=None, end=None, keep=None, first=0, n=None):
    """-> begin, end (positions in a.bases), keep, info (n x 2), stats[20] of records first .. first + n - 1."""
    S = [int(v) for v in a.seq_offsets]
    n = a.n_records - first if n is None else n
    ob, oe, ok = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint8)
    info = np.zeros((n, 2), np.uint32)
    stats = [0] * 20
    for k in range(n):
        r = first + k
        b, e = (S[r], S[r + 1]) if begin is None else (int(begin[k]), int(end[k]))
        assert S[r] <= b <= e <= S[r + 1]
        ob[k], oe[k], info[k] = b, e, (0xFFFF, 0)
        if keep is not None and not keep[k]:
            continue
        nb, ne, kp, i0, i1, st = read_model(a.bases[b:e], R)
        ob[k], oe[k], ok[k], info[k] = b + nb, b + ne, kp, (i0, i1)
        stats = [u + v for u, v in zip(stats, st)]
    return ob, oe, ok, info, stats


def run_model_forms(lib, sh):
    """poly_run == poly_run_serial on random and planted reads, both ends, every rate; and the figures the issue quotes."""
    rng = np.random.default_rng(1)
    for _ in range(300):
        n = int(rng.integers(0, 200))
        x = rng.integers(0, 5, n).astype(np.uint8)
        if n and rng.random() < 0.6:
            k = int(rng.integers(1, n + 1)); X = int(rng.integers(0, 4))
            run = np.where(rng.random(k) < 0.1, rng.integers(0, 5, k), X).astype(np.uint8)
            if rng.random() < 0.5: x[n - k:] = run
            else: x[:k] = run
        for X in range(4):
            for rate in (0, 125, 200, 1000):
                for from_end in (True, False):
                    assert poly_run(x, X, rate, from_end) == poly_run_serial(x, X, rate, from_end), (x.tolist(), X, rate, from_end)
    rep = lambda unit, n=150: np.array(["ACGT".index(ch) for ch in (unit * n)[:n]], np.uint8)
    figures = {"A": (310, 0), "AC": (152, 1000), "ACG": (100, 1000), "ACGT": (73, 1000), "ACGTCA": (47, 838)}
    for unit, (dust, cpm) in figures.items():
        assert max(dust_windows(rep(unit))) == dust and complexity_of(rep(unit))[1] == cpm, unit
    assert window_starts(63) == [0] and window_starts(64) == [0] and window_starts(65) == [0, 1] and window_starts(96) == [0, 32]
    assert window_starts(97) == [0, 32, 33] and window_starts(200) == [0, 32, 64, 96, 128, 136]


# ---- one call ----------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Got:
    error: object
    stats: object
    begin: np.ndarray
    end: np.ndarray
    keep: np.ndarray
    info: np.ndarray
    untouched: bool


def lib_rules(lib, R, reserved=(0, 0, 0, 0), **over):
    f = dict(tail_bases=R["tail"], head_bases=R["head"], poly_min_length=R["poly_min"], poly_max_error_permille=R["rate"], min_length=R["min_length"],
             min_complexity_permille=R["min_cp"], max_dust=OFF if R["max_dust"] is None else R["max_dust"], max_dust_windows=R["max_windows"])
    f.update(over)
    return lib.ComplexityRules(reserved=reserved, **f)


def cplx_call(lib, h, cin, n, cr, plan=(None, None, None), inplace=False, info=True):
    """One dsrcgpu_columns_complexity_plan.  plan: begin / end / keep as numpy in the coordinates of the staged arrays, or None.  Fresh
    outputs are 0xA5-filled; inplace: every output that has an input counterpart IS that input."""
    with Dev(h) as d:
        pin = [None if v is None else d.up(np.ascontiguousarray(v).astype(dt).tobytes()) for v, dt in zip(plan, (np.uint64, np.uint64, np.uint8))]
        sizes = (8 * n, 8 * n, n)
        fresh = [d.fill(s) for s in sizes]
        out = [pin[i] if inplace and pin[i] is not None else fresh[i] for i in range(3)]
        pi = d.fill(8 * n)
        err = stats = None
        try:
            stats = h.columns_complexity_plan(cin, cr, pin[0], pin[1], pin[2], out[0], out[1], out[2], pi if info else None)
        except lib.DsrcGpuError as e:
            err = e
        raw = [d.down(p, s) for p, s in zip(out, sizes)] + [d.down(pi, 8 * n)]
        raw_fresh = [d.down(p, s) for p, s in zip(fresh, sizes)] + [raw[3]]
    assert all(r[-8:] == b"\xA5" * 8 for r in raw + raw_fresh), "written behind the end of an output array"
    if inplace:                                              # what was not used as an output stayed as it was
        assert all(raw_fresh[i] == b"\xA5" * len(raw_fresh[i]) for i in range(3) if pin[i] is not None)
    if not info:
        assert raw[3] == b"\xA5" * len(raw[3]), "d_info was not given"
    untouched = all(r == b"\xA5" * len(r) for r in raw_fresh)
    return Got(err, stats, np.frombuffer(raw[0], np.uint64)[:n], np.frombuffer(raw[1], np.uint64)[:n], np.frombuffer(raw[2], np.uint8)[:n],
               np.frombuffer(raw[3], np.uint32)[:2 * n].reshape(n, 2), untouched)


def check_cplx(lib, h, st, R, begin=None, end=None, keep=None, pad=0, first=0, n=None, what=None, inplace=False, info=True, model=None):
    """Arrays staged in `st`, the plan as positions in the UNPADDED arrays (the pad is added here) -> the call == the model."""
    a = st.a
    n = a.n_records - first if n is None else n
    wb, we, wk, wi, ws = model if model is not None else complexity_model(a, R, begin, end, keep, first, n)
    shift = lambda v: None if v is None else np.asarray(v).astype(np.uint64) + np.uint64(pad)
    got = cplx_call(lib, h, st.cols_in(first, n), n, lib_rules(lib, R), (shift(begin), shift(end), keep), inplace, info)
    assert got.error is None, (what, got.error)
    bad = np.nonzero((got.begin != wb + np.uint64(pad)) | (got.end != we + np.uint64(pad)) | (got.keep != wk) |
                     ((got.info != wi).any(axis=1) if info else False))[0]
    assert len(bad) == 0, (what, "record", int(bad[0]), int(got.begin[bad[0]]) - pad, int(got.end[bad[0]]) - pad, int(got.keep[bad[0]]),
                           [hex(v) for v in got.info[bad[0]]], "want", int(wb[bad[0]]), int(we[bad[0]]), int(wk[bad[0]]), [hex(v) for v in wi[bad[0]]], len(bad))
    assert got.stats == ws, (what, got.stats, ws)
    return wb, we, wk, wi, ws


def handle(lib):
    return ce.handle(lib, Config.from_levels(0, 0))


def staged(lib, h, a, pad=0):
    return cs.staged(lib, h, a, pad)


def run_cases(lib, reads, rule_sets, what, expect=None):
    """reads as whole records under every rule set; expect(R, model) asks the model alone first."""
    a = arrays_from_bases(reads)
    h = handle(lib)
    try:
        with staged(lib, h, a) as st:
            for R in rule_sets:
                m = complexity_model(a, R)
                if expect is not None:
                    expect(R, m)
                check_cplx(lib, h, st, R, what=(what, R), model=m)
    finally:
        h.close()
    return a


# ---- geometry of runs ------------------------------------------------------------------------------------------------------------
def filler(n, X, phase=0):
    """n positions of the two bases behind X in turn: no run of X, none of anything else above 1."""
    return ((X + 1 + (np.arange(n) + phase) % 2) % 4).astype(np.uint8)


def run_lengths(n, poly_min=10):
    return sorted({k for k in (0, 1, poly_min - 1, poly_min, poly_min + 1, 63, 64, 65, 128, n) if k <= n})


def run_geometry(lib, sh, X):
    """Runs of base X of every length at the 3' end, at the 5' end and at both, on every read length; rate 0."""
    other = (X + 2) % 4
    reads, want = [], []
    for n in LENGTHS:
        for k in run_lengths(n):
            x = filler(n, X); x[n - k:] = X
            reads.append(x); want.append((k if k == n else 0, k))
            x = filler(n, X); x[:k] = X
            reads.append(x); want.append((k, k if k == n else 0))
            if 2 * k <= n:
                x = filler(n, X); x[:k] = X; x[n - k:] = X
                reads.append(x); want.append((k, k))
        x = np.full(n, X, np.uint8)                          # both ends together eat the whole range
        reads.append(x); want.append((n, n))
        if n >= 22:                                          # ... but for one base in the middle
            x = x.copy(); x[n // 2] = other
            reads.append(x); want.append((n // 2, n - n // 2 - 1))
    both = rules_of("ACGT"[X], "ACGT"[X], rate=0, min_length=0)
    sets = [both, dict(both, head=0), dict(both, tail=0), rules_of("ACGT", "ACGT", rate=0, min_length=0), dict(both, poly_min=1)]
    S = np.concatenate(([0], np.cumsum([len(x) for x in reads])))

    def expect(R, m):
        if R is not both:
            return
        empty = 0
        for r, (hd, t) in enumerate(want):
            n = int(S[r + 1] - S[r])
            hd, t = (hd if hd >= 10 else 0), (t if t >= 10 else 0)
            wb, we = (0, 0) if hd + t >= n else (hd, n - t)
            assert (int(m[0][r] - S[r]), int(m[1][r] - S[r])) == (wb, we), (X, r, n, want[r])
            assert int(m[3][r][0]) == (X if hd else NONE) | (X if t else NONE) << 8
            empty += n > 0 and wb == we
        assert empty >= len(LENGTHS) - 4 and m[4][4] > 20 and m[4][5] > 20 and m[4][6 + X] == m[4][5] and m[4][10 + X] == m[4][4]
    run_cases(lib, reads, sets, ("geometry", X), expect)


# ---- error budget ------------------------------------------------------------------------------------------------------------------
def budget_reads(rate):
    """3' runs of G with exactly floor(L * rate / 1000) foreign positions and with one more: at distances 0 / 62 / 63 / 64 from the end
    (bits 0, 62, 63 of the first tile and bit 0 of the next: both sides of the seam), as the last position of the run, and in the
    middle; the foreign codes are A C T and 4, 18, 255 in turn."""
    foreign = [0, 4, 1, 18, 3, 255]
    reads, pairs = [], []
    for L in (10, 16, 63, 64, 65, 66, 130):
        k = L * rate // 1000
        for count in (k, k + 1):
            if count > L:
                continue
            for first in ([L - 1, 63, 64, 62, 0], [62, 63, 64], [L // 2]):
                spots = [p for p in dict.fromkeys(first + list(range(L // 3, L))) if p < L][:count]
                x = filler(200, 2); x[200 - L:] = 2
                for i, p in enumerate(spots):
                    x[199 - p] = foreign[i % len(foreign)]
                reads.append(x)
            pairs.append((len(reads) - 6, len(reads) - 3) if count == k + 1 else None)
    return reads, [p for p in pairs if p]


def run_budget(lib, sh, rate):
    reads, pairs = budget_reads(rate)
    R = rules_of("G", rate=rate, min_length=0)

    def expect(R_, m):
        if R_ is not R:
            return
        t = (m[1] - m[0]).astype(np.int64)
        if rate < 1000:                                      # one foreign position more: somewhere a shorter cut, or none
            assert any((t[lo: lo + 3] != t[hi: hi + 3]).any() for lo, hi in pairs), rate
        assert m[4][5] > 0
    run_cases(lib, reads, [R, dict(R, head=R["tail"], tail=0), dict(R, poly_min=1)], ("budget", rate), expect)
    # the mirror image: the same reads reversed under the head rule give the mirrored cuts
    a, ar = arrays_from_bases(reads), arrays_from_bases([x[::-1].copy() for x in reads])
    m, mr = complexity_model(a, R), complexity_model(ar, dict(R, head=R["tail"], tail=0))
    assert np.array_equal(m[1] - m[0], mr[1] - mr[0]) and m[4][5] == mr[4][4]


# ---- the score ---------------------------------------------------------------------------------------------------------------------
def run_score(lib, sh):
    G, A, T = 2, 0, 3
    body = filler(60, G)
    through = np.concatenate((body, [G] * 12, [A, 1, A], [G] * 30)).astype(np.uint8)          # 12 G, 3 others, 30 G
    two = np.concatenate(([T] * 20, filler(80, T, 1)[:78], [0, 1], [A] * 25)).astype(np.uint8)  # T wins at 5', A at 3'
    two[20] = 1
    ties = []
    for clean in (63, 64, 62, 127):                          # `clean` G, one foreign, then g more G: a tie at g = 2, the longer run at 3
        for g in (1, 2, 3):
            x = filler(300, G); x[300 - clean:] = G; x[300 - clean - 1] = A; x[300 - clean - 1 - g: 300 - clean - 1] = G
            ties.append(x)
    reads = [through, two] + ties
    gen, strict = rules_of("G", rate=200, min_length=0), rules_of("G", rate=0, min_length=0)
    mixed = rules_of("AT", "AT", rate=125, min_length=0)

    def expect(R, m):
        t = lambda r: int(m[1][r] - m[0][r])
        if R is gen:
            assert 105 - t(0) == 45
            for i, clean in enumerate((63, 64, 62, 127)):    # +1 -2 +1 +1: equal at g = 2 -- the shorter wins --, above at g = 3
                assert [300 - t(2 + 3 * i + j) for j in range(3)] == [clean, clean, clean + 4], (clean, [300 - t(2 + 3 * i + j) for j in range(3)])
        if R is strict:
            assert 105 - t(0) == 30
        if R is mixed:
            assert int(m[3][1][0]) == T | A << 8 and int(m[0][1] - 105) == 20 and t(1) == 125 - 20 - 25
    run_cases(lib, reads, [gen, strict, mixed, rules_of("ACGT", "ACGT", rate=200, min_length=0)], "score", expect)


# ---- complexity ----------------------------------------------------------------------------------------------------------------------
def run_complexity(lib, sh):
    rng = np.random.default_rng(40)
    rep = lambda unit, n: np.resize(np.asarray(unit, np.uint8), n)
    reads = [rep([0], 150), rep([0, 1], 150), rng.integers(0, 4, 150).astype(np.uint8)]                    # 0 .. 2
    reads += [np.zeros(0, np.uint8), rep([2], 1), rep([2], 2), rep([2, 3], 2)]                              # 3 .. 6: n' 0, 1, 2
    for n in (64, 65, 66, 128, 129):                                                                        # 7 .. 16: one differing pair, at the seam / next to it
        for at in (63, 64):
            x = rep([1], n)
            if at < n: x[at:] = 3
            reads.append(x)
    reads += [rep([4], 40), rep([4, 18], 40), rep([255], 40), rep([255, 4], 41), rep([0, 4], 40), rep([18], 70)]      # 17 .. 22: codes >= 4
    exact = rep([0], 101); exact[np.arange(1, 31) * 3] = 1                                                  # 23: 60 differing pairs of 100
    below = exact.copy(); below[3] = 0                                                                      # 24: 58
    reads += [exact, below]
    body = rng.integers(0, 4, 40).astype(np.uint8); body[-1] = 0
    reads.append(np.concatenate((body, rep([2], 110))).astype(np.uint8))                                     # 25: fails before the tail cut, passes after it
    reads.append(np.concatenate((rep([0], 20), rep([2, 2, 2, 1, 2, 2, 2, 3], 39)[::-1])).astype(np.uint8))   # 26: the reverse
    off = rules_of(min_length=0)
    at600, at601 = rules_of(min_cp=600, min_length=0), rules_of(min_cp=601, min_length=0)
    plain, cut = rules_of(min_cp=300), rules_of("G", rate=250, min_cp=300)

    def expect(R, m):
        cpm = lambda r: int(m[3][r][1]) & 0xFFFF
        if R is off:
            assert [cpm(r) for r in (0, 1, 3, 4, 5, 6)] == [0, 1000, 1000, 1000, 0, 1000] and 604 <= cpm(2) <= 900
            assert [cpm(r) for r in range(7, 17)] == [1000 // (n - 1) if at < n else 0 for n in (64, 65, 66, 128, 129) for at in (63, 64)]
            assert [cpm(r) for r in range(17, 23)] == [0, 1000, 0, 1000, 1000, 0]
            assert m[2].all()
        if R is at600: assert m[2][23] == 1 and m[2][24] == 0 and cpm(23) == 600 and cpm(24) == 580
        if R is at601: assert m[2][23] == 0
        if R is plain: assert m[2][25] == 0 and m[2][26] == 1 and m[2][4] == 1 and m[2][5] == 0 and m[4][15] > 5
        if R is cut:
            assert m[2][25] == 1 and m[2][26] == 0 and int(m[1][25] - m[0][25]) == 40 and int(m[1][26] - m[0][26]) == 20
    run_cases(lib, reads, [off, at600, at601, plain, cut, rules_of("ACGT", "ACGT", poly_min=5, min_cp=500, min_length=0)], "complexity", expect)


# ---- DUST --------------------------------------------------------------------------------------------------------------------------
def de_bruijn3():
    """66 bases in which every one of the 64 triplets starts exactly once."""
    seq, a = [], [0] * 12

    def db(t, p):
        if t > 3:
            if 3 % p == 0: seq.extend(a[1: p + 1])
        else:
            a[t] = a[t - p]; db(t + 1, p)
            for j in range(a[t - p] + 1, 4):
                a[t] = j; db(t + 1, t)
    db(1, 1)
    x = np.array(seq + seq[:2], np.uint8)
    codes = 16 * x[:-2].astype(int) + 4 * x[1:-1] + x[2:]
    assert len(x) == 66 and sorted(codes.tolist()) == list(range(64))
    return x


def run_dust_lengths(lib, sh):
    """Every branch of the window enumeration: random, poly-A and AC reads of the lengths at which it changes, whole and behind a cut."""
    rng = np.random.default_rng(50)
    reads = []
    for n in DUST_LENGTHS:
        reads += [rng.integers(0, 4, n).astype(np.uint8), np.zeros(n, np.uint8), np.resize(np.array([0, 1], np.uint8), n),
                  np.concatenate((np.resize(np.array([0, 1, 3], np.uint8), n), np.full(15, 2, np.uint8)))]
    on = rules_of(max_dust=20, min_length=0)
    cut = rules_of("G", max_dust=20, min_length=0)

    def expect(R, m):
        dust = (m[3][:, 1] >> 16).astype(int)
        if R is on:
            assert all(dust[4 * i + 1] == (310 if n >= 64 else 10 * ((n - 2) * (n - 3) // 2) // (n - 3) if n >= 4 else 0) for i, n in enumerate(DUST_LENGTHS))
            assert m[4][16] >= 2 * len(DUST_LENGTHS) and m[4][0] >= len(DUST_LENGTHS)
        if R is cut:
            assert m[4][5] == len(DUST_LENGTHS) and all(int(m[1][4 * i + 3] - m[0][4 * i + 3]) == n for i, n in enumerate(DUST_LENGTHS))
    run_cases(lib, reads, [on, cut, rules_of(max_dust=20, max_windows=1, min_length=0), rules_of(min_length=0)], "dust lengths", expect)


def run_dust_windows(lib, sh):
    """A low-complexity stretch that only the end-aligned window sees in full, the same stretch at starts 0 and 32; N codes down to
    l = 0, 1, 2; max_dust_windows exactly met and one more.  The thresholds come from the model's per-window values."""
    rng = np.random.default_rng(51)
    body = rng.integers(0, 4, 100).astype(np.uint8)
    ac = np.resize(np.array([0, 1], np.uint8), 30)
    at_end = body.copy(); at_end[70:] = ac
    v = dust_windows(at_end)
    assert window_starts(100) == [0, 32, 36] and v[2] > v[1] > v[0], v
    at0 = body.copy(); at0[:30] = ac
    at32 = body.copy(); at32[32:62] = ac
    v0, v32 = dust_windows(at0), dust_windows(at32)
    assert v0[0] > max(v0[1:]) and min(v32[0], v32[1]) > v32[2], (v0, v32)
    ns = lambda *keep: np.array([k if k is not None else 4 for k in keep], np.uint8)
    few = [np.full(70, 4, np.uint8), ns(None, 0, 0, 0, None, None), ns(0, 0, 0, 0, None, 18), ns(0, 0, 0, 255, 0, 1, 0), np.full(64, 255, np.uint8)]
    few.append(np.concatenate((np.zeros(64, np.uint8), [4])).astype(np.uint8))          # the N invalidates the last triplets of the end-aligned window only
    assert [max(dust_windows(x)) for x in few[:5]] == [0, 0, 10, 0, 0]                  # l = 0, 1, 2 (two equal triplets: S = 1), 2 (different ones, one each side of the N), 0
    poly = np.zeros(200, np.uint8)
    reads = [at_end, at0, at32, body] + few + [poly]
    only_end = rules_of(max_dust=v[1], min_length=0)
    sets = [only_end, rules_of(max_dust=v[2], min_length=0), rules_of(max_dust=v[0], max_windows=1, min_length=0),
            rules_of(max_dust=v[0], max_windows=2, min_length=0), rules_of(max_dust=309, max_windows=5, min_length=0),
            rules_of(max_dust=309, max_windows=6, min_length=0), rules_of(max_dust=310, min_length=0), rules_of(max_dust=0, min_length=0)]

    def expect(R, m):
        if R is only_end: assert m[2][0] == 0 and m[2][3] == 1
        if R is sets[1]: assert m[2][0] == 1
        if R is sets[2]: assert m[2][0] == 0                 # two windows above v[0], one allowed
        if R is sets[3]: assert m[2][0] == 1
        if R is sets[4]: assert m[2][10] == 0                # six windows of 310, five allowed
        if R is sets[5]: assert m[2][10] == 1
        if R is sets[6]: assert m[2].all()
    run_cases(lib, reads, sets, "dust windows", expect)


def run_dust_triplets(lib, sh):
    """What a wrong lane-to-triplet mapping would change (see the module's docstring)."""
    db = de_bruijn3()
    reads = [db, db[::-1].copy(), np.concatenate((db, db)).astype(np.uint8)]
    for t in range(64):                                      # code t eight times, each behind an N, then 30 triplets that all differ: one window
        trip = [t >> 4, (t >> 2) & 3, t & 3, 4]
        reads.append(np.concatenate((trip * 8, db[:32])).astype(np.uint8))
    rng = np.random.default_rng(52)
    for _ in range(12):                                      # skewed compositions: a few codes with large, different counts
        p = rng.dirichlet([0.4] * 4)
        reads.append(rng.choice(4, 64, p=p).astype(np.uint8))
    for k in range(4):                                       # counts 1 .. 10 of ten codes: runs of one base of the lengths 3 .. 12 would need 75 positions; 1 .. 7 fit
        x, codes = [], [(k + j) % 4 for j in range(7)]
        for j, base in enumerate(codes):
            x += [base] * (j + 3) + [4]
        reads.append(np.array(x[:64], np.uint8))
    R = rules_of(max_dust=5, min_length=0)

    def expect(R_, m):
        dust = (m[3][:, 1] >> 16).astype(int)
        assert dust[0] == 0 and dust[1] == 0 and set(dust[3:67]) <= {7, 9} and len(set(dust[67:])) >= 4
    run_cases(lib, reads, [R], "dust triplets", expect)


# ---- ranges in, keep in, in place, d_info -------------------------------------------------------------------------------------------
def run_ranges(lib, sh):
    """Ranges inside records whose bases outside the range are poly-G (and whose neighbours start and end with G): nothing outside
    [b, e) is seen.  With and without padding around the staged arrays, offsets into the record array, keep in, in place."""
    G = 2
    n = 260
    reads, begin, end, want = [], [], [], []

    def add(x, b, e, t, hd, why):
        reads.append(np.asarray(x, np.uint8)); begin.append(b); end.append(e); want.append((hd, t, why))
    for shift in (1, 63, 64, 65):
        x = filler(n, G); x[:shift] = G; x[200:] = G; x[180:200] = G
        add(x, shift, 200, 20, 0, "G in front of b and behind e; 20 G inside")
        x = filler(n, G); x[:shift] = G; x[200:] = G
        add(x, shift, 200, 0, 0, "G outside only")
        x = filler(n, G); x[shift: shift + 15] = G; x[:shift] = 0; x[195:] = G
        add(x, shift, 195, 0, 15, "a head run from b on")
    x = np.full(n, G, np.uint8)
    add(x, 100, 105, 0, 0, "5 G inside: below poly_min_length, although 260 stand around them")
    add(x, 100, 111, 11, 11, "11 G: both ends eat the range")
    add(x, 50, 50, 0, 0, "empty range")
    add(x, n, n, 0, 0, "empty range at the record's end")
    add(np.zeros(0, np.uint8), 0, 0, 0, 0, "no bases")
    x = filler(n, G); x[n - 12:] = G
    add(x, 3, n, 12, 0, "the last record, flush with bases_len")
    a = arrays_from_bases(reads)
    S = a.seq_offsets.astype(np.int64)
    gb = S[:-1] + np.array(begin); ge = S[:-1] + np.array(end)
    R = rules_of("G", "G", rate=0, min_length=0)
    m = complexity_model(a, R, gb, ge)
    for r, (hd, t, why) in enumerate(want):
        wb, we = (gb[r], gb[r]) if hd + t >= ge[r] - gb[r] else (gb[r] + hd, ge[r] - t)
        assert (int(m[0][r]), int(m[1][r])) == (wb, we), (why, r)
    keep = np.ones(a.n_records, np.uint8); keep[[1, 7, 13]] = 0
    full = rules_of("ACGT", "ACGT", rate=125, min_length=20, min_cp=300, max_dust=20)
    h = handle(lib)
    try:
        for pad in (0, 5):
            with staged(lib, h, a, pad=pad) as st:
                check_cplx(lib, h, st, R, gb, ge, pad=pad, what=("ranges", pad), model=m)
                for inplace in (False, True):
                    check_cplx(lib, h, st, R, gb, ge, keep, pad=pad, what=("ranges, keep", pad, inplace), inplace=inplace)
                    check_cplx(lib, h, st, full, gb, ge, keep, pad=pad, what=("every rule", pad, inplace), inplace=inplace)
                    check_cplx(lib, h, st, full, None, None, keep, pad=pad, what=("whole reads, keep", pad, inplace), inplace=inplace)
                    check_cplx(lib, h, st, full, gb, ge, None, pad=pad, what=("no keep", pad, inplace), inplace=inplace, info=False)
                check_cplx(lib, h, st, R, pad=pad, what=("whole reads", pad))
                for first, cnt in ((5, None), (a.n_records - 1, 1), (7, 6)):       # d_seq_offs + k
                    sl = slice(first, None if cnt is None else first + cnt)
                    check_cplx(lib, h, st, full, gb[sl], ge[sl], keep[sl], pad=pad, first=first, n=cnt, what=("first", first, pad))
                    check_cplx(lib, h, st, full, pad=pad, first=first, n=cnt, what=("first, whole", first, pad))
        with staged(lib, h, a) as st:                        # d_quals, d_titles and d_title_offs are not read
            cin = st.cols_in()
            cin = lib.ColumnsIn(cin.d_bases, cin.bases_len, None, None, 0, cin.d_seq_offs, None, a.n_records)
            mk = complexity_model(a, full, gb, ge, keep)
            got = cplx_call(lib, h, cin, a.n_records, lib_rules(lib, full), (gb.astype(np.uint64), ge.astype(np.uint64), keep))
            assert got.error is None and got.stats == mk[4] and np.array_equal(got.end, mk[1]) and np.array_equal(got.keep, mk[2]) and np.array_equal(got.info, mk[3])
            dropped = np.nonzero(keep == 0)[0]
            assert (mk[3][dropped] == (0xFFFF, 0)).all() and (mk[1][dropped] == ge[dropped]).all() and (mk[2][dropped] == 0).all()
    finally:
        h.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def run_arg_refusals(lib, sh):
    a = fuzz_arrays(0, 20)[0]
    good = rules_of("G", "T", max_dust=20, min_cp=300)
    h = handle(lib)
    broken = [("tail_bases", dict(tail_bases=16)), ("head_bases", dict(head_bases=16)), ("tail_bases", dict(tail_bases=OFF)),
              ("poly_min_length", dict(poly_min_length=0)), ("poly_min_length", dict(poly_min_length=0, tail_bases=0)),
              ("poly_max_error_permille", dict(poly_max_error_permille=1001)), ("min_complexity_permille", dict(min_complexity_permille=1001))]
    try:
        with staged(lib, h, a) as st:
            n = a.n_records
            S = a.seq_offsets
            for field, over in broken:
                got = cplx_call(lib, h, st.cols_in(), n, lib_rules(lib, good, **over))
                assert got.error is not None and got.error.code == E_ARG and got.untouched and field in str(got.error), (field, over, got.error)
            for k in range(4):
                res = [0, 0, 0, 0]; res[k] = 1
                got = cplx_call(lib, h, st.cols_in(), n, lib_rules(lib, good, tuple(res)))
                assert got.error is not None and got.error.code == E_ARG and got.untouched and "reserved" in str(got.error), (k, got.error)
            for name, plan in (("begin alone", (S[:-1], None, None)), ("end alone", (None, S[1:], None))):
                got = cplx_call(lib, h, st.cols_in(), n, lib_rules(lib, good), plan)
                assert got.error is not None and got.error.code == E_ARG and got.untouched and "go together" in str(got.error), (name, got.error)
            check_cplx(lib, h, st, good, what="the same handle, clean")
            check_cplx(lib, h, st, rules_of(min_length=40), what="no base, no filter: a length filter")      # poly_min_length 0 is legal without a mask
            got = cplx_call(lib, h, st.cols_in(), n, lib_rules(lib, rules_of(min_length=40), poly_min_length=0))
            assert got.error is None and got.stats == complexity_model(a, rules_of(min_length=40))[4] and got.stats[14] > 0
            check_cplx(lib, h, st, rules_of("ACGT", "ACGT", poly_min=OFF, rate=1000, min_length=OFF, min_cp=1000, max_dust=OFF - 1, max_windows=OFF),
                       what="the largest figures")
            got = cplx_call(lib, h, st.cols_in(3, 0), 0, lib_rules(lib, good))          # no records
            assert got.error is None and got.stats == [0] * 20 and got.untouched
    finally:
        h.close()
    hc = ce.handle(lib, dataclasses.replace(Config.from_levels(0, 0), color_space=True))
    try:
        with staged(lib, hc, a) as st:
            got = cplx_call(lib, hc, st.cols_in(), a.n_records, lib_rules(lib, good))
            assert got.error is not None and got.error.code == E_ARG and got.untouched
    finally:
        hc.close()


def run_input_errors(lib, sh):
    """The plants of the adapter plan's input errors in the first, a middle and the last record, kept and dropped ones: code, record,
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
    cr = lib_rules(lib, rules)
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
                        got = cplx_call(lib, h, st.cols_in(), n, cr, plan)
                        assert got.error is not None and got.error.code == E_INPUT and got.untouched, (name, r, got.error)
                        assert "record %d:" % r in str(got.error) and word in str(got.error), (name, r, str(got.error))
                    st.restore()
                    checked += 1
                check_cplx(lib, h, st, rules, begin, end, keep, pad=pad, what=("after", name))

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
                        got = cplx_call(lib, h, st.cols_in(), n, cr, plan_of(r), inplace=inplace)
                        assert got.error is not None and got.error.code == E_INPUT, (name, r, got.error)
                        assert "record %d:" % r in str(got.error) and word in str(got.error), (name, r, str(got.error))
                        if inplace:                          # the plan itself is what it was
                            pb, pe, pk = plan_of(r)
                            assert np.array_equal(got.begin, pb) and np.array_equal(got.end, pe) and np.array_equal(got.keep, pk)
                        else:
                            assert got.untouched, (name, r)
                    checked += 1
                check_cplx(lib, h, st, rules, begin, end, keep, pad=pad, what=("after", name))
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
                check_cplx(lib, h, st, rules, begin, end, keep)
                assert h.get_fields_capacity() == 11
            assert text_blocks(h) == text_blocks(fresh), layout
        finally:
            h.close(); fresh.close()


# ---- record counts -----------------------------------------------------------------------------------------------------------------
def run_count(lib, sh, n_rec):
    """n_rec reads of 12 bases drawn from 500 different ones (the model runs once per different read and plan), every rule on."""
    K = 500
    rng = np.random.default_rng(700)
    uniq = rng.integers(0, 4, (K, 12)).astype(np.uint8)
    for r in range(K):
        kind = r % 5
        if kind == 0: uniq[r, 12 - int(rng.integers(3, 10)):] = (r // 5) % 4
        if kind == 1: uniq[r, :int(rng.integers(3, 10))] = (r // 5) % 4
        if kind == 2: uniq[r] = np.resize(uniq[r, :int(rng.integers(1, 3))], 12)
    uniq[rng.random((K, 12)) < 0.03] = 4
    cb, ce_ = rng.integers(0, 3, K), rng.integers(0, 3, K)
    ukeep = (rng.random(K) < 0.8).astype(np.uint8)
    R = rules_of("ACGT", "ACGT", poly_min=3, rate=200, min_length=4, min_cp=400, max_dust=20)
    ua = Arrays(uniq.reshape(-1), np.full(12 * K, 30, np.uint8), np.zeros(0, np.uint8), (12 * np.arange(K + 1)).astype(np.uint64), np.zeros(K + 1, np.uint64), [0, K])
    ub = (12 * np.arange(K) + cb).astype(np.uint64); ue = (12 * np.arange(K) + 12 - ce_).astype(np.uint64)
    mb, me, mk, mi, _ = complexity_model(ua, R, ub, ue, ukeep)
    per = np.array([complexity_model(ua, R, ub[r: r + 1], ue[r: r + 1], ukeep[r: r + 1], first=r, n=1)[4] for r in range(K)], np.int64)
    idx = np.arange(n_rec) % K
    base = (12 * (np.arange(n_rec) - idx)).astype(np.uint64)
    bases = uniq[idx].reshape(-1)
    S = (12 * np.arange(n_rec + 1)).astype(np.uint64)
    titles = np.empty(2 * n_rec, np.uint8); titles[0::2] = ord("@"); titles[1::2] = ord("t")
    a = Arrays(bases, np.full(12 * n_rec, 30, np.uint8), titles, S, (2 * np.arange(n_rec + 1)).astype(np.uint64), [0, n_rec])
    begin, end, keep = ub[idx] + base, ue[idx] + base, ukeep[idx]
    stats = [int(v) for v in (np.bincount(idx, minlength=K)[:, None] * per).sum(axis=0)]
    m = (mb[idx] + base, me[idx] + base, mk[idx], mi[idx], stats)
    if n_rec <= 65:                                          # the expansion itself, against the model on the expanded arrays
        direct = complexity_model(a, R, begin, end, keep)
        assert all(np.array_equal(u, v) for u, v in zip(direct[:4], m[:4])) and direct[4] == stats
    if n_rec >= 500:
        assert all(stats[k] > 0 for k in range(17)), stats
    h = handle(lib)
    try:
        with staged(lib, h, a) as st:
            check_cplx(lib, h, st, R, begin, end, keep, what=n_rec, model=m)
            check_cplx(lib, h, st, R, begin, end, keep, what=(n_rec, "in place"), inplace=True, model=m)
    finally:
        h.close()


# ---- fuzz ------------------------------------------------------------------------------------------------------------------------
def fuzz_arrays(seed, n_rec, max_len=300):
    """Lengths 0 .. max_len; about a third of the reads with a planted run at either end (or both) with a few foreign positions,
    about a tenth low-complexity repeats of period 1 .. 6, about 5 % of the codes >= 4, random ranges and keep flags; the rules are
    drawn per seed -> (arrays, begin, end, keep, rules)."""
    rng = np.random.default_rng(3000 + seed)
    other = np.concatenate([[4, 4, 255], np.arange(5, 19)]).astype(np.uint8)
    reads = []
    for _ in range(n_rec):
        n = int(rng.integers(0, max_len + 1))
        x = rng.integers(0, 4, n).astype(np.uint8)
        u = rng.random()
        if u < 0.1 and n:
            x = np.resize(rng.integers(0, 4, int(rng.integers(1, 7))).astype(np.uint8), n)
        amb = rng.random(n) < 0.05
        x[amb] = other[rng.integers(0, len(other), int(amb.sum()))]
        if 0.1 <= u < 0.45 and n:
            for at_end in ((True,), (False,), (True, False))[int(rng.integers(0, 3))]:
                k = int(rng.integers(1, min(n, 90) + 1))
                run = np.full(k, int(rng.integers(0, 4)), np.uint8)
                bad = rng.random(k) < 0.06
                run[bad] = rng.integers(0, 5, int(bad.sum()))
                if at_end: x[n - k:] = run
                else: x[:k] = run
        reads.append(x)
    a = arrays_from_bases(reads)
    S = a.seq_offsets.astype(np.int64)
    lens = S[1:] - S[:-1]
    whole = rng.random(n_rec) < 0.6
    cut5 = np.where(whole, 0, (rng.random(n_rec) * (lens + 1) * 0.2).astype(np.int64))
    cut3 = np.where(whole, 0, (rng.random(n_rec) * (lens - cut5 + 1) * 0.2).astype(np.int64))
    begin = (S[:-1] + cut5).astype(np.uint64); end = (S[1:] - cut3).astype(np.uint64)
    keep = (rng.random(n_rec) < 0.85).astype(np.uint8)
    masks = ["G", "ACGT", "AT", "GT", "C", "ACG"]
    R = rules_of(masks[seed % 6], masks[(seed + 1) % 6], poly_min=int(rng.integers(3, 15)), rate=int(rng.choice([0, 100, 125, 200])),
                 min_length=int(rng.integers(0, 40)), min_cp=int(rng.choice([250, 300, 450])), max_dust=int(rng.choice([12, 20, 40])),
                 max_windows=int(rng.integers(0, 2)))
    return a, begin, end, keep, R


def run_fuzz(lib, sh, seed):
    n_rec = sh["cplx_fuzz"][1]
    a, begin, end, keep, R = fuzz_arrays(seed, n_rec)
    m = complexity_model(a, R, begin, end, keep)
    print("complexity fuzz", seed, "rules", R, "stats", m[4])
    assert m[4][4] + m[4][5] >= n_rec // 12 and m[4][0] >= n_rec // 4 and m[4][17:] == [0, 0, 0]
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=3) as st:
            check_cplx(lib, h, st, R, begin, end, keep, pad=3, what=("fuzz", seed), model=m)
            check_cplx(lib, h, st, R, pad=3, what=("fuzz, whole reads", seed))
    finally:
        h.close()


def run_fuzz_exercises_everything(lib, sh):
    """On the model alone: every one of the seventeen statistics is above 0 in at least one of the seeds the fuzz runs."""
    seeds, n_rec = sh["cplx_fuzz"]
    seen = [0] * 20
    for seed in range(seeds):
        a, begin, end, keep, R = fuzz_arrays(seed, n_rec)
        seen = [u + v for u, v in zip(seen, complexity_model(a, R, begin, end, keep)[4])]
    assert all(v > 0 for v in seen[:17]) and seen[17:] == [0, 0, 0], seen


# ---- the Python layers and the closed loop ---------------------------------------------------------------------------------------------
tensors = ca.tensors


def py_kw(R):
    s = lambda mask: "".join(ch for i, ch in enumerate("ACGT") if mask >> i & 1)
    return dict(tail=s(R["tail"]), head=s(R["head"]), poly_min_length=R["poly_min"], poly_max_error_permille=R["rate"], min_length=R["min_length"],
                min_complexity_permille=R["min_cp"], max_dust=R["max_dust"], max_dust_windows=R["max_windows"])


def run_python_layers(lib, sh, device):
    from dsrc_amd import columns
    a, begin, end, keep, R = fuzz_arrays(3, 120)
    h = handle(lib)
    try:
        assert tuple(lib.COMPLEXITY_STATS) == STATS and lib.COMPLEXITY_NONE == NONE
        c = tensors(a, device)
        t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v).astype(dt)).to(device)
        tb, te, tk = t(begin, np.int64), t(end, np.int64), t(keep, np.uint8)
        m = complexity_model(a, R, begin, end, keep)
        kw = py_kw(R)
        for kws in (kw, dict(kw, tail=kw["tail"].lower())):
            b, e, k, stats, hb, tbase, cpm, dust = columns.complexity_plan(h, c, tb, te, tk, return_info=True, **kws)
            assert b.dtype == torch.int64 and k.dtype == torch.uint8 and hb.dtype == torch.int64 and k.device.type == torch.device(device).type
            assert b.data_ptr() != tb.data_ptr() and torch.equal(tb, t(begin, np.int64)) and torch.equal(tk, t(keep, np.uint8))      # fresh tensors, inputs as they were
            assert list(stats) == list(STATS) and list(stats.values()) == m[4][:17]
            assert np.array_equal(b.cpu().numpy().astype(np.uint64), m[0]) and np.array_equal(e.cpu().numpy().astype(np.uint64), m[1])
            assert np.array_equal(k.cpu().numpy(), m[2])
            i0, i1 = m[3][:, 0].astype(np.int64), m[3][:, 1].astype(np.int64)
            gone = i0 == 0xFFFF
            unb = lambda v: np.where(v == NONE, -1, v)
            assert np.array_equal(hb.cpu().numpy(), unb(i0 & 255)) and np.array_equal(tbase.cpu().numpy(), unb(i0 >> 8 & 255))
            assert np.array_equal(cpm.cpu().numpy(), np.where(gone, -1, i1 & 0xFFFF)) and np.array_equal(dust.cpu().numpy(), np.where(gone, -1, i1 >> 16))
            assert gone.any() and (hb.cpu().numpy()[gone] == -1).all()
        m = complexity_model(a, rules_of())
        got = columns.complexity_plan(h, c)                  # the defaults: nothing searched, nothing judged but a length of 1
        assert len(got) == 4 and list(got[3].values()) == m[4][:17] and np.array_equal(got[1].cpu().numpy().astype(np.uint64), m[1])

        class Never:                                         # ValueError comes before any library call
            def __getattr__(self, name):
                raise AssertionError("the library was called")
        for bad in (dict(tail="N"), dict(tail="GG"), dict(head=4), dict(tail=None), dict(poly_min_length=0), dict(poly_max_error_permille=1001),
                    dict(min_length=-1), dict(min_complexity_permille=1001), dict(max_dust=-1), dict(max_dust=2 ** 32), dict(max_dust_windows=-1),
                    dict(max_dust=True), dict(poly_min_length=2.0)):
            for call in (lambda: columns.complexity_plan(Never(), c, **bad), lambda: columns.filter_columns(Never(), c, complexity=bad),
                         lambda: columns.filter_pairs(Never(), c, c, complexity=bad)):
                try:
                    call()
                except ValueError:
                    pass
                else:
                    raise AssertionError("no ValueError for %r" % (bad,))
        for bad in ("G", dict(tails="G"), []):
            try:
                columns.filter_columns(Never(), c, complexity=bad)
            except ValueError:
                pass
            else:
                raise AssertionError("no ValueError for complexity=%r" % (bad,))
    finally:
        h.close()


def filter_reads(n_rec, seed=31):
    """The adapter cases' reads (falling qualities, a third with an adapter tail), of which a third get a poly-G tail of 1 .. 60 bases
    with high qualities and a tenth are low-complexity repeats -> (arrays, records, text)."""
    rng = np.random.default_rng(seed)
    _, records, _ = ca.filter_reads(n_rec, seed)
    out = []
    for r, (t, s, q) in enumerate(records):
        s, q = bytearray(s), bytearray(q)
        if r % 3 == 1:
            k = min(len(s), int(rng.integers(1, 61)))
            s[len(s) - k:] = b"G" * k; q[len(q) - k:] = bytes([33 + 38]) * k
            if k > 12: s[len(s) - int(rng.integers(1, k))] = ord("A")
        if r % 10 == 5:
            unit = bytes(b"ACGT"[v] for v in rng.integers(0, 4, int(rng.integers(1, 4))))
            s[:] = (unit * len(s))[:len(s)]; q[:] = bytes([33 + 35]) * len(q)
        out.append((t, bytes(s), bytes(q)))
    text = b"\n".join(t + b"\n" + s + b"\n+\n" + q for t, s, q in out)
    return ce.arrays_of([text]), out, text


def filter_model(a, trim, adapters, complexity, min_overlap=3, rate=100):
    """model quality plan -> model adapter plan -> model complexity plan: begin, end, keep, the stats dict filter_columns returns."""
    if adapters is not None:
        b, e, k, stats = ca.filter_model(a, trim, adapters, min_overlap, rate)
    else:
        b, e, k, ts = cs.plan_model(a, trim)
        stats = dict(zip(ca.TRIM_STATS, ts))
    R = dict(dict(min_length=trim["min_length"]), **complexity)
    b, e, k, _, xs = complexity_model(a, R, b, e, k)
    stats["complexity"] = dict(zip(STATS, xs))
    return b, e, k, stats


def run_filter_columns(lib, sh, device):
    from dsrc_amd import columns
    a, _, _ = filter_reads(200)
    trim = cs.rules_of(15, 20, min_length=30, max_n=2, min_mean_quality=20)
    same = lambda sel, want: all(np.array_equal(g.cpu().numpy().astype(w.dtype), w) for g, w in
                                 zip((sel.bases, sel.quals, sel.titles, sel.seq_offsets, sel.title_offsets), want[:5]))
    h = handle(lib)
    try:
        c = tensors(a, device)
        # without complexity: what it returned before
        b, e, k, ts = cs.plan_model(a, trim)
        want = cs.select_model(a, b, e, k)
        for kw in ({}, dict(complexity=None)):
            sel, stats = columns.filter_columns(h, c, **kw, **trim)
            assert stats == dict(zip(ca.TRIM_STATS, ts)) and "complexity" not in stats and same(sel, want)
        b2, e2, k2, wstats = ca.filter_model(a, trim, [ca.ADAPTER])
        sel, stats = columns.filter_columns(h, c, adapters=[ca.ADAPTER], **trim)
        assert stats == wstats and same(sel, cs.select_model(a, b2, e2, k2))
        # with it: behind the adapter plan, with the filter's min_length unless the dict gives one
        for ads, R in ((None, rules_of("G", max_dust=20)), ([ca.ADAPTER], rules_of("G", "T", min_cp=300, max_dust=20)),
                       ([ca.ADAPTER], rules_of("ACGT", min_length=50))):
            kw = py_kw(R)
            if R["min_length"] == 1:
                del kw["min_length"]; R = {k_: v for k_, v in R.items() if k_ != "min_length"}
            b3, e3, k3, wstats = filter_model(a, trim, ads, dict(R))
            x = wstats["complexity"]
            assert x["records_tail_cut"] >= 30 and x["tail_G"] >= 30 and x["dropped_length"] > 0 and 0 < x["records_kept"] < ts[0], x
            if R.get("max_dust") is not None: assert x["dropped_dust"] + x["dropped_complexity"] > 0, x
            sel, stats = columns.filter_columns(h, c, adapters=ads, complexity=kw, **trim)
            assert stats == wstats and list(stats)[-1] == "complexity", (stats, wstats)
            assert same(sel, cs.select_model(a, b3, e3, k3)) and sel.n_records == x["records_kept"]
        # what stands behind it sees the narrowed plan
        R = rules_of("G", max_dust=20); kw = py_kw(R); del kw["min_length"]
        b3, e3, k3, wstats = filter_model(a, trim, None, {k_: v for k_, v in R.items() if k_ != "min_length"})
        _, stats = columns.filter_columns(h, c, complexity=kw, profile=True, **trim)
        assert stats["profile_after"].summary()["records"] == wstats["complexity"]["records_kept"]
        assert stats["profile_after"].summary()["bases"] == wstats["complexity"]["bases_kept"]
    finally:
        h.close()


def run_filter_pairs(lib, sh, device):
    """Per side the complexity plan stands behind the adapter plan and in front of the pair plan: the composed models."""
    from dsrc_amd import columns
    (a1, _, _), (a2, _, _) = cp.paired_reads(120)
    rng = np.random.default_rng(61)
    for a in (a1, a2):                                       # poly-G tails on a third of the mates, a few poly-A mates
        a.bases = a.bases.copy()
        S = a.seq_offsets.astype(np.int64)
        for r in range(a.n_records):
            if rng.random() < 0.33:
                a.bases[S[r + 1] - int(rng.integers(8, 50)): S[r + 1]] = 2
            elif rng.random() < 0.05:
                a.bases[S[r]: S[r + 1]] = 0
    trim = cs.rules_of(0, 20, min_length=30, max_n=2)
    R = rules_of("G", min_cp=300, max_dust=20)
    kw = py_kw(R); del kw["min_length"]
    same = lambda sel, want: all(np.array_equal(g.cpu().numpy().astype(w.dtype), w) for g, w in
                                 zip((sel.bases, sel.quals, sel.titles, sel.seq_offsets, sel.title_offsets), want[:5]))
    h = handle(lib)
    try:
        c1, c2 = tensors(a1, device), tensors(a2, device)
        for overlap in (True, False):
            plans, wstats = [], {}
            for name, a in (("read1", a1), ("read2", a2)):
                b, e, k, side = filter_model(a, trim, None, {k_: v for k_, v in R.items() if k_ != "min_length"})
                plans.append((b, e, k)); wstats[name] = side
            assert wstats["read1"]["complexity"]["tail_G"] >= 20 and wstats["read2"]["complexity"]["dropped_complexity"] + wstats["read2"]["complexity"]["dropped_dust"] > 0
            if overlap:
                pr = dict(cp.rules_of(20, 4, 150), min_length=trim["min_length"])
                b1, e1, b2, e2, keep, _, ps = cp.pair_model(a1, a2, pr, plans[0], plans[1])
                wstats["pair"] = dict(zip(cp.PAIR_STATS, ps))
            else:
                (b1, e1, k1), (b2, e2, k2) = plans
                keep = ((k1 != 0) & (k2 != 0)).astype(np.uint8)
            o1, o2, stats = columns.filter_pairs(h, c1, c2, overlap=overlap, pair_min_overlap=20, pair_max_mismatches=4, pair_max_error_permille=150,
                                                 complexity=kw, **trim)
            assert stats == wstats, (stats, wstats)
            assert same(o1, cs.select_model(a1, b1, e1, keep)) and same(o2, cs.select_model(a2, b2, e2, keep)) and o1.n_records == int(keep.sum())
        # without it: what filter_pairs returned before
        r1, r2, keep, wstats = cp.pairs_model(a1, a2, trim, (None, None), True, cp.rules_of(20, 4, 150))
        o1, o2, stats = columns.filter_pairs(h, c1, c2, pair_min_overlap=20, pair_max_mismatches=4, pair_max_error_permille=150, complexity=None, **trim)
        assert stats == wstats and same(o1, cs.select_model(a1, r1[0], r1[1], keep))
    finally:
        h.close()


def run_closed_loop(lib, sh, device):
    """Records written here -> the oracle's block -> decode_columns -> filter_columns(complexity=dict(tail="G", max_dust=20)) ->
    encode_columns == the oracle's block of the text of the model-filtered records, lossless -d3 -q2 with CRC."""
    from dsrc_amd import columns
    cfg = ce.BLOCK_CFG
    a, records, text = filter_reads(300, seed=32)
    trim = cs.rules_of(0, 20, min_length=35)
    b, e, k, wstats = filter_model(a, trim, None, {k_: v for k_, v in rules_of("G", max_dust=20).items() if k_ != "min_length"})
    S = a.seq_offsets.astype(np.int64)
    kept = [(t, s[int(b[r] - S[r]): int(e[r] - S[r])], q[int(b[r] - S[r]): int(e[r] - S[r])]) for r, (t, s, q) in enumerate(records) if k[r]]
    x = wstats["complexity"]
    print("closed loop: model stats", wstats)
    assert x["records_tail_cut"] >= 60 and x["dropped_dust"] >= 10 and x["bases_cut_3"] > 500 and 0 < len(kept) < wstats["records_kept"] < len(records)
    src = ce.oracle_blocks(cfg, [text]); want = ce.oracle_blocks(cfg, [b"\n".join(t + b"\n" + s + b"\n+\n" + q for t, s, q in kept)])
    assert src is not None and want is not None
    d_blocks, offs = cs._stage_blocks([src[0][0]], device)
    h = ce.handle(lib, cfg)
    try:
        rc = columns.decode_columns(h, d_blocks, offs, [len(src[0][0])], device)
        assert rc.n_records == len(records)
        sel, stats = columns.filter_columns(h, rc, complexity=dict(tail="G", max_dust=20), **trim)
        assert stats == wstats and sel.n_records == len(kept)
        h.set_fields_capacity(0)
        blocks, o_offs, o_sizes, _ = columns.encode_columns(h, sel, block_records=sel.block_records)
        host = blocks.cpu().numpy().tobytes()
        assert [host[o: o + s] for o, s in zip(o_offs, o_sizes)] == [want[0][0]]
    finally:
        h.close()
