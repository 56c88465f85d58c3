"""Shared by tests/test_emu_columns_demux.py (CPU, emulator build) and tests/test_gpu_columns_demux.py (MI355X): the cases of the
columnar demultiplex (dsrcgpu_columns_demux_plan and dsrcgpu_columns_partition_device; dsrc_amd/csrc/k_columns_demux.h) and what they
must give.

The reference has no counterpart, so the yardstick is the integer model written out here.  The planner's rule stands twice:
classify_serial() is the serial loop of include/dsrc_gpu.h word for word, classify_fast() the same rule as numpy array operations;
the two are compared in test_model_forms_agree before anything else relies on the fast one.  partition_model() is a stable sort by
class of the kept records.  None of it comes from the library under test, and every comparison is exact equality.  Output arrays are
filled with 0xA5 before a call, so that "nothing written" can be asserted.  Before the library is compared on a crafted case the
model alone is asked what that case is for.

Shapes.  The emulator pays a coroutine switch per wave exchange, so its fuzz is 2 seeds x 150 records where the GPU runs 6 x 2000.
The planner takes 64 records a wave and at most 512 workgroups, so the count that takes its grid stride into a second round is
512 workgroups of 1024 records and some more -- it runs on the GPU only.  `wg` is the build's workgroup size, which is the
partition's tile."""
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

E_ARG, E_CAPACITY, E_INPUT = cs.E_ARG, cs.E_CAPACITY, cs.E_INPUT
NO_LIMIT = 0xFFFFFFFF
DROPPED = 0xFFFFFFFF
SHORT, NO_MATCH, AMBIGUOUS = 1, 2, 3

SHAPES = {
    "gpu": dict(ca.SHAPES["gpu"], demux_fuzz=(6, 2000), wg=1024, stride_count=512 * 1024 + 4001),
    "emu": dict(ca.SHAPES["emu"], demux_fuzz=(2, 150), wg=256, stride_count=None),
}
Arrays = ce.Arrays
Dev = cs.Dev
BARCODE_LENGTHS = [1, 6, 8, 31, 32, 33, 63, 64]
OFFSETS = [0, 1, 63, 64, 65]
SAMPLE_COUNTS = [1, 2, 63, 64, 65, 1023]
WINNERS = [0, 63, 64, 65, 127, 128, 1022]
STATS = ("records_kept", "bases_kept", "bases_cut", "records_assigned", "assigned_perfect", "unassigned_short", "unassigned_no_match",
         "unassigned_ambiguous", "dropped_length")
arrays_from_bases = ca.arrays_from_bases


def codes_of(s):
    return np.array(["ACGT".index(ch) for ch in s.upper()], np.uint8)


# ---- the planner's model -----------------------------------------------------------------------------------------------------------
def rules_of(barcodes, slots=((0, 0),), max_mm=1, slot_max=None, min_delta=1, cut=1, keep_un=0, min_length=1):
    """barcodes: per sample a list with one uint8 array of codes per slot; slots: (source, offset) per slot; slot_max: None, or per
    slot an int or None."""
    barcodes = [[np.asarray(b, np.uint8) for b in sample] for sample in barcodes]
    return dict(barcodes=barcodes, slots=[tuple(s) for s in slots], max_mm=max_mm, slot_max=slot_max, min_delta=min_delta, cut=cut, keep_un=keep_un,
                min_length=min_length)


def slot_lens(R):
    return [len(b) for b in R["barcodes"][0]]


def windows(sets, R, b, e):
    """What every record holds at the barcode positions: per slot an n x len array, and `short` -- the records with a slot that does not
    fit its limit (their rows are not looked at).  sets[0] is read under the range b / e, sets[k] from the record's first base."""
    n = len(b)
    short = np.zeros(n, bool)
    Xs = []
    for s, (src, off) in enumerate(R["slots"]):
        L = slot_lens(R)[s]
        if src == 0:
            lo, limit = b + off, e
        else:
            Sk = sets[src].seq_offsets.astype(np.int64)
            lo, limit = Sk[:-1] + off, Sk[1:]
        sh = lo + L > limit
        short |= sh
        padded = np.concatenate((sets[src].bases, np.full(L, 255, np.uint8)))
        Xs.append(padded[np.where(sh, 0, lo)[:, None] + np.arange(L)[None, :]])
    return Xs, short


def classify_serial(Xs, short, R):
    """The rule of include/dsrc_gpu.h as it stands there -> class, best, second, reason per record."""
    n, A = len(short), len(R["barcodes"])
    out = np.zeros((n, 4), np.int64)
    for r in range(n):
        if short[r]:
            out[r] = (A, 255, 255, SHORT)
            continue
        D = []
        for a in range(A):
            total, within = 0, True
            for s, x in enumerate(Xs):
                bc = R["barcodes"][a][s]
                d = 0
                for j in range(len(bc)):
                    if int(x[r][j]) != int(bc[j]):
                        d += 1
                limit = None if R["slot_max"] is None else R["slot_max"][s]
                if limit is not None and d > limit:
                    within = False
                total += d
            D.append(total if within else 255)
        best = min(D)
        at = D.index(best)                                   # the lowest index that holds it
        second = min([D[a] for a in range(A) if a != at], default=255)
        assigned = best <= R["max_mm"] and second - best >= R["min_delta"]
        out[r] = (at if assigned else A, best, second, 0 if assigned else NO_MATCH if best > R["max_mm"] else AMBIGUOUS)
    return out[:, 0], out[:, 1], out[:, 2], out[:, 3]


def classify_fast(Xs, short, R):
    """The same in numpy: a distance matrix records x samples, its first minimum and the minimum of the rest."""
    n, A = len(short), len(R["barcodes"])
    D = np.zeros((n, A), np.int64)
    within = np.ones((n, A), bool)
    for s, X in enumerate(Xs):
        B = np.stack([R["barcodes"][a][s] for a in range(A)])
        L = B.shape[1]
        step = max(1, (1 << 24) // (A * L))
        d = np.concatenate([(X[i: i + step, None, :] != B[None, :, :]).sum(axis=2) for i in range(0, n, step)] + [np.zeros((0, A), np.int64)])
        limit = None if R["slot_max"] is None else R["slot_max"][s]
        if limit is not None:
            within &= d <= limit
        D += d
    D = np.where(within, D, 255)
    at = D.argmin(axis=1)                                    # (the first of equal minima)
    rows = np.arange(n)
    best = D[rows, at]
    rest = D.copy(); rest[rows, at] = 255
    second = rest.min(axis=1) if A > 1 else np.full(n, 255, np.int64)
    assigned = (best <= R["max_mm"]) & (second - best >= R["min_delta"])
    reason = np.where(assigned, 0, np.where(best > R["max_mm"], NO_MATCH, AMBIGUOUS))
    cls = np.where(assigned, at, A)
    cls, best, second, reason = (np.where(short, v, x) for v, x in ((A, cls), (255, best), (255, second), (SHORT, reason)))
    return cls, best, second, reason


def demux_model(sets, R, begin=None, end=None, keep=None, serial=False):
    """sets: [the reads, index set 1, index set 2] as Arrays -> begin, end (positions in sets[0].bases), keep, class, info, stats[9],
    class counts (n_samples + 1) of the call."""
    a = sets[0]
    n, A = a.n_records, len(R["barcodes"])
    S = a.seq_offsets.astype(np.int64)
    b = S[:-1].copy() if begin is None else np.asarray(begin).astype(np.int64)
    e = S[1:].copy() if end is None else np.asarray(end).astype(np.int64)
    assert np.all((S[:-1] <= b) & (b <= e) & (e <= S[1:]))
    came = np.ones(n, bool) if keep is None else np.asarray(keep) != 0
    Xs, short = windows(sets, R, b, e)
    cls, best, second, reason = (classify_serial if serial else classify_fast)(Xs, short, R)
    assigned = reason == 0
    cut_len = max([off + L for (src, off), L in zip(R["slots"], slot_lens(R)) if src == 0], default=0)
    ob = np.where(came & assigned & bool(R["cut"]), b + cut_len, b)
    flag = came & (assigned | bool(R["keep_un"]))
    ok = flag & (e - ob >= R["min_length"])
    info = np.where(came, best | second << 8 | reason << 16, DROPPED).astype(np.uint32)
    klass = np.where(came, cls, DROPPED).astype(np.uint32)
    stats = [int(ok.sum()), int((e - ob)[ok].sum()), int((ob - b)[ok].sum()), int((came & assigned).sum()), int((came & assigned & (best == 0)).sum()),
             int((came & (reason == SHORT)).sum()), int((came & (reason == NO_MATCH)).sum()), int((came & (reason == AMBIGUOUS)).sum()),
             int((flag & ~ok).sum())]
    counts = np.bincount(cls[came], minlength=A + 1).astype(np.uint64)
    return ob.astype(np.uint64), e.astype(np.uint64), ok.astype(np.uint8), klass, info, stats, counts


def random_barcodes(rng, A, lens):
    """A distinct samples; close neighbours on purpose (a few substitutions apart), so that ties and runners-up happen."""
    seen, out = set(), []
    base = [rng.integers(0, 4, L).astype(np.uint8) for L in lens]
    while len(out) < A:
        sample = []
        for s, L in enumerate(lens):
            x = base[s].copy() if rng.random() < 0.5 else rng.integers(0, 4, L).astype(np.uint8)
            for _ in range(int(rng.integers(0, 4))):
                x[int(rng.integers(0, L))] = rng.integers(0, 4)
            sample.append(x)
        key = tuple(x.tobytes() for x in sample)
        if key not in seen:
            seen.add(key); out.append(sample)
    return out


def run_model_forms(lib, sh):
    """classify_fast == classify_serial on random windows, and what the rule says in the cases the issue words."""
    rng = np.random.default_rng(1)
    for trial in range(60):
        lens = [int(rng.integers(3, 13)) for _ in range(int(rng.integers(1, 3)))]
        A = int(rng.integers(1, 9))
        bcs = random_barcodes(rng, A, lens)
        n = 40
        Xs = []
        for s, L in enumerate(lens):
            X = np.stack([bcs[int(rng.integers(0, A))][s] for _ in range(n)])
            X = np.where(rng.random(X.shape) < 0.15, rng.choice([0, 1, 2, 3, 4, 255], X.shape), X).astype(np.uint8)
            Xs.append(X)
        short = rng.random(n) < 0.1
        R = rules_of(bcs, [(0, 0)] * len(lens), int(rng.integers(0, 4)), None if rng.random() < 0.4 else [None if rng.random() < 0.3 else int(rng.integers(0, 3)) for _ in lens],
                     int(rng.integers(0, 3)))
        for u, v in zip(classify_fast(Xs, short, R), classify_serial(Xs, short, R)):
            assert np.array_equal(u, v), (trial, R)
    one = lambda x, bcs, **kw: [int(v[0]) for v in classify_serial([np.array([codes_of(x)])], np.zeros(1, bool), rules_of([[codes_of(b)] for b in bcs], **kw))]
    assert one("ACGT", ["ACGT", "TTTT"]) == [0, 0, 3, 0]
    assert one("ACGA", ["ACGT", "ACGC"], min_delta=0) == [0, 1, 1, 0] and one("ACGA", ["ACGT", "ACGC"], min_delta=1) == [2, 1, 1, AMBIGUOUS]
    assert one("AAAA", ["ACGT"]) == [1, 3, 255, NO_MATCH] and one("ACGT", ["ACGT"], min_delta=255) == [0, 0, 255, 0]
    assert one("ACGT", ["ACGA", "AGGA"], max_mm=1, min_delta=1) == [0, 1, 2, 0] and one("ACGT", ["ACGA", "AGGA"], max_mm=1, min_delta=2) == [2, 1, 2, AMBIGUOUS]


# ---- one planner call ----------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Got:
    error: object
    stats: object
    begin: np.ndarray
    end: np.ndarray
    keep: np.ndarray
    cls: np.ndarray
    info: np.ndarray
    counts: object
    untouched: bool


def lib_rules(lib, R, reserved=(0, 0, 0), **over):
    kw = dict(barcodes=[[b.tobytes() for b in sample] for sample in R["barcodes"]], slots=R["slots"], max_mismatches=R["max_mm"],
              slot_max_mismatches=None if R["slot_max"] is None else [NO_LIMIT if v is None else v for v in R["slot_max"]], min_delta=R["min_delta"],
              cut=R["cut"], keep_unassigned=R["keep_un"], min_length=R["min_length"])
    kw.update(over)
    return lib.DemuxRules(reserved=reserved, **kw)


def demux_call(lib, h, cins, n, dr, plan=(None, None, None), inplace=False, info=True, counts0=None, n_counts=None):
    """One dsrcgpu_columns_demux_plan.  cins: [the reads' ColumnsIn, the index sets' ...]; plan: begin / end / keep as numpy in the
    coordinates of the staged arrays, or None.  Fresh outputs are 0xA5-filled; inplace: every output that has an input counterpart IS
    that input.  counts0: None (d_class_counts NULL) or what the array holds before the call."""
    with Dev(h) as d:
        pin = [None if v is None else d.up(np.ascontiguousarray(v).astype(dt).tobytes()) for v, dt in zip(plan, (np.uint64, np.uint64, np.uint8))]
        sizes = (8 * n, 8 * n, n, 4 * n, 4 * n)
        fresh = [d.fill(s) for s in sizes]
        out = [pin[i] if inplace and pin[i] is not None else fresh[i] for i in range(3)] + fresh[3:]
        pc = None if counts0 is None else d.up(np.asarray(counts0, np.uint64).tobytes())
        err = stats = None
        try:
            stats = h.columns_demux_plan(cins[0], cins[1:], dr, pin[0], pin[1], pin[2], out[0], out[1], out[2], out[3], out[4] if info else None, pc)
        except lib.DsrcGpuError as e:
            err = e
        raw = [d.down(p, s) for p, s in zip(out, sizes)]
        raw_fresh = [d.down(p, s) for p, s in zip(fresh, sizes)]
        counts = None if pc is None else np.frombuffer(d.down(pc, 8 * len(counts0)), np.uint64)[:len(counts0)].copy()
        if pc is not None:
            assert d.down(pc, 8 * len(counts0))[-8:] == b"\xA5" * 8, "written behind the end of d_class_counts"
    assert all(r[-8:] == b"\xA5" * 8 for r in raw + raw_fresh), "written behind the end of an output array"
    if inplace:                                              # what was not used as an output stayed as it was
        assert all(raw_fresh[i] == b"\xA5" * len(raw_fresh[i]) for i in range(3) if pin[i] is not None)
    if not info:
        assert raw[4] == b"\xA5" * len(raw[4]), "d_info was not given"
    untouched = all(r == b"\xA5" * len(r) for r in raw_fresh) and (counts is None or np.array_equal(counts, np.asarray(counts0, np.uint64)))
    return Got(err, stats, np.frombuffer(raw[0], np.uint64)[:n], np.frombuffer(raw[1], np.uint64)[:n], np.frombuffer(raw[2], np.uint8)[:n],
               np.frombuffer(raw[3], np.uint32)[:n], np.frombuffer(raw[4], np.uint32)[:n], counts, untouched)


def check_demux(lib, h, sts, R, begin=None, end=None, keep=None, pad=0, what=None, inplace=False, info=True, counts0="zeros", model=None):
    """sts: the Staged reads and index sets; the plan as positions in the UNPADDED reads (the pad is added here) -> the call == the model."""
    sets = [st.a for st in sts]
    n, A = sets[0].n_records, len(R["barcodes"])
    wb, we, wk, wc, wi, ws, wn = model if model is not None else demux_model(sets, R, begin, end, keep)
    if isinstance(counts0, str):
        counts0 = np.zeros(A + 1, np.uint64)
    shift = lambda v: None if v is None else np.asarray(v).astype(np.uint64) + np.uint64(pad)
    got = demux_call(lib, h, [st.cols_in() for st in sts], n, lib_rules(lib, R), (shift(begin), shift(end), keep), inplace, info, counts0)
    assert got.error is None, (what, got.error)
    bad = np.nonzero((got.begin != wb + np.uint64(pad)) | (got.end != we + np.uint64(pad)) | (got.keep != wk) | (got.cls != wc) |
                     ((got.info != wi) if info else False))[0]
    assert len(bad) == 0, (what, "record", int(bad[0]), int(got.begin[bad[0]]) - pad, int(got.end[bad[0]]) - pad, int(got.keep[bad[0]]), int(got.cls[bad[0]]),
                           hex(int(got.info[bad[0]])), "want", int(wb[bad[0]]), int(we[bad[0]]), int(wk[bad[0]]), int(wc[bad[0]]), hex(int(wi[bad[0]])), len(bad))
    assert got.stats == ws, (what, got.stats, ws)
    if counts0 is not None:
        assert np.array_equal(got.counts, np.asarray(counts0, np.uint64) + wn), (what, got.counts, wn)
    return wb, we, wk, wc, wi, ws, wn


def handle(lib):
    return ce.handle(lib, Config.from_levels(0, 0))


class Sets:
    """The reads and the index sets of one case, staged on one handle."""

    def __init__(self, lib, h, sets, pad=0):
        self.sts = []
        try:
            for k, a in enumerate(sets):
                self.sts.append(cs.staged(lib, h, a, pad if k == 0 else 0))
        except Exception:
            self.free(); raise

    def free(self):
        for st in self.sts:
            st.free()

    def __enter__(self):
        return self.sts

    def __exit__(self, *exc):
        self.free()


def run_cases(lib, sets, cases, what):
    """cases: (rules, begin, end, keep, expect) tuples on one staged input; expect(model) asks the model alone first."""
    h = handle(lib)
    try:
        with Sets(lib, h, sets) as sts:
            for i, (R, begin, end, keep, expect) in enumerate(cases):
                m = demux_model(sets, R, begin, end, keep)
                if expect is not None:
                    expect(m)
                check_demux(lib, h, sts, R, begin, end, keep, what=(what, i), model=m)
    finally:
        h.close()


def must(cond):
    assert cond


def other_base(x, rng=None):
    return ((x.astype(np.int64) + (1 if rng is None else rng.integers(1, 4, x.shape))) % 4).astype(np.uint8)


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
def run_geometry(lib, sh, L):
    """A barcode of L bases at every offset: ending exactly at the range's end, one base beyond it, a range of 0 bases, and a range that
    ends inside a barcode that the array continues perfectly; inline and from an index set.  Record 0 has 7 bases, so that no later
    record starts at a multiple of 64."""
    rng = np.random.default_rng(100 + L)
    bc = [rng.integers(0, 4, L).astype(np.uint8) for _ in range(3)]
    bc[1] = bc[0].copy(); bc[1][L // 2] = (bc[1][L // 2] + 1) % 4
    bc[2] = ((bc[0].astype(np.int64) + 2) % 4).astype(np.uint8)
    samples = [[b] for b in bc]
    reads, begin, end, want = [np.zeros(7, np.uint8)], [0], [7], [(None, None)]          # want: (the offset the record was built for, its answer there)
    pos = 7
    for off in OFFSETS:
        for a in range(3):
            for tail in (0, 1, 40):                          # the barcode ends exactly at the range's end, and in front of it
                x = np.concatenate((rng.integers(0, 4, off), bc[a], rng.integers(0, 4, tail))).astype(np.uint8)
                reads.append(x); begin.append(pos); end.append(pos + len(x)); want.append((off, a)); pos += len(x)
            # the range ends one base inside the barcode; the array goes on with the rest of it
            x = np.concatenate((rng.integers(0, 4, off), bc[a], rng.integers(0, 4, 5))).astype(np.uint8)
            reads.append(x); begin.append(pos); end.append(pos + off + L - 1); want.append((off, "short")); pos += len(x)
            # a range of 0 bases in front of a perfect barcode
            x = np.concatenate((rng.integers(0, 4, off), bc[a], rng.integers(0, 4, 3))).astype(np.uint8)
            reads.append(x); begin.append(pos); end.append(pos); want.append((off, "short")); pos += len(x)
    a_in = arrays_from_bases(reads)
    begin, end = np.array(begin, np.uint64), np.array(end, np.uint64)
    assert any(int(s) % 64 for s in a_in.seq_offsets[1:-1])
    cases = []
    for off in OFFSETS:
        R = rules_of(samples, [(0, off)], max_mm=0, min_delta=1, min_length=0)

        def expect(m, off=off):
            seen = 0
            for r, (built_for, w) in enumerate(want):
                if int(end[r] - begin[r]) < off + L:
                    assert int(m[3][r]) == 3 and int(m[4][r]) == (255 | 255 << 8 | SHORT << 16), (L, off, r)
                if built_for != off:
                    continue
                if w == "short":
                    assert int(m[3][r]) == 3 and int(m[4][r]) >> 16 == SHORT, (L, off, r)
                else:
                    assert int(m[3][r]) == w and int(m[4][r]) & 255 == 0, (L, off, r, w)
                    seen += 1
            assert seen == 9, (L, off, seen)
        cases.append((R, begin, end, None, expect))
        cases.append((dict(R, cut=0, keep_un=1), begin, end, None, None))
    run_cases(lib, [a_in], cases, ("geometry inline", L))
    # the same barcodes as index reads: the record's first base counts, whatever the reads' ranges are
    idx = [np.zeros(0, np.uint8)]
    for off in OFFSETS:
        for a in range(3):
            for tail in (0, 1, 40):
                idx.append(np.concatenate((rng.integers(0, 4, off), bc[a], rng.integers(0, 4, tail))).astype(np.uint8))
            idx.append(np.concatenate((rng.integers(0, 4, off), bc[a][:L - 1])).astype(np.uint8))
            idx.append(np.zeros(0, np.uint8))
    a_idx = arrays_from_bases(idx)
    assert a_idx.n_records == a_in.n_records
    cases = []
    for off in OFFSETS:
        def expect(m, off=off):
            hit = sum(int(m[3][r]) < 3 for r in range(a_in.n_records))
            assert hit >= 9 and m[5][5] >= 10 and m[5][2] == 0, (L, off, hit, m[5])
        cases.append((rules_of(samples, [(1, off)], max_mm=0, min_delta=1, min_length=0), begin, end, None, expect))
    run_cases(lib, [a_in, a_idx], cases, ("geometry index", L))


# ---- distance ----------------------------------------------------------------------------------------------------------------------
def run_distance(lib, sh, L):
    """Exactly max_mismatches substitutions and one more, N and code 255 at a barcode position."""
    rng = np.random.default_rng(200 + L)
    bc = rng.integers(0, 4, L).astype(np.uint8)
    far = other_base(bc)
    reads, subs = [], []
    for k in range(0, min(L, 6) + 1):
        for _ in range(3):
            x = bc.copy()
            at = rng.choice(L, k, replace=False)
            x[at] = other_base(x[at], rng)
            reads.append(np.concatenate((x, rng.integers(0, 4, 6))).astype(np.uint8)); subs.append(k)
    for code in (4, 18, 255):
        x = bc.copy(); x[L - 1] = code
        reads.append(np.concatenate((x, [0, 1])).astype(np.uint8)); subs.append(1)
        x = bc.copy(); x[0] = code; x[L // 2] = code
        reads.append(np.concatenate((x, [0, 1])).astype(np.uint8)); subs.append(len({0, L // 2}))
    a = arrays_from_bases(reads)
    cases = []
    for mm in sorted({0, 1, 2, 3, min(L, 5)} & set(range(L + 1))):
        R = rules_of([[bc]], [(0, 0)], max_mm=mm, min_delta=0, min_length=0)

        def expect(m, mm=mm):
            for r, k in enumerate(subs):
                assert int(m[3][r]) == (0 if k <= mm else 1) and (int(m[4][r]) & 255) == k, (L, mm, r, k)
            assert any(k == mm for k in subs) and (mm == L or any(k == mm + 1 for k in subs))
        cases.append((R, None, None, None, expect))
        cases.append((dict(R, barcodes=[[bc], [far]], min_delta=1), None, None, None, None))
    run_cases(lib, [a], cases, ("distance", L))


def run_slot_budget(lib, sh):
    """Two slots of 8: (1, 1) assigns while (2, 0) at the same total does not under a per-slot budget of 1; NO_LIMIT lets both through."""
    rng = np.random.default_rng(300)
    b0, b1 = rng.integers(0, 4, 8).astype(np.uint8), rng.integers(0, 4, 8).astype(np.uint8)
    samples = [[b0, b1], [other_base(b0), other_base(b1)]]
    sub = lambda x, at: np.concatenate((x[:at], other_base(x[at: at + 1]), x[at + 1:])).astype(np.uint8)
    reads = [np.concatenate((sub(b0, 2), sub(b1, 5), [0, 1, 2])), np.concatenate((sub(sub(b0, 2), 6), b1, [0, 1, 2])),
             np.concatenate((b0, sub(sub(b1, 0), 7), [3]))]
    a = arrays_from_bases([x.astype(np.uint8) for x in reads])
    slots = [(0, 0), (0, 8)]

    def limited(m):
        assert [int(v) for v in m[3]] == [0, 2, 2] and [int(v) & 255 for v in m[4]] == [2, 255, 255]

    def free(m):
        assert [int(v) for v in m[3]] == [0, 0, 0] and [int(v) & 255 for v in m[4]] == [2, 2, 2]
    run_cases(lib, [a], [(rules_of(samples, slots, max_mm=2, slot_max=[1, 1], min_length=0), None, None, None, limited),
                         (rules_of(samples, slots, max_mm=2, slot_max=[None, None], min_length=0), None, None, None, free),
                         (rules_of(samples, slots, max_mm=2, slot_max=[2, None], min_length=0), None, None, None,
                          lambda m: must([int(v) for v in m[3]] == [0, 0, 0])),
                         (rules_of(samples, slots, max_mm=2, slot_max=None, min_length=0), None, None, None, free)], "slot budget")


# ---- choice ------------------------------------------------------------------------------------------------------------------------
def run_choice(lib, sh):
    """Ties and runners-up: two samples at equal distance under min_delta 0 and 1, a runner-up exactly min_delta above and one below,
    and one sample alone (second = 255)."""
    t = codes_of("ACGTACGT")
    s0, s1 = t.copy(), t.copy()
    s0[1] = 0; s1[6] = 0                                     # both one away from t, two from each other
    s2 = t.copy(); s2[0] = 3; s2[3] = 0; s2[4] = 2           # three away from t
    reads = [np.concatenate((x, [0, 1, 2, 3])).astype(np.uint8) for x in (t, s0, s1, s2)]
    a = arrays_from_bases(reads)

    def tie0(m):
        assert [int(v) for v in m[3]] == [0, 0, 1] + [2] and int(m[4][0]) == (1 | 1 << 8)

    def tie1(m):
        assert int(m[3][0]) == 3 and int(m[4][0]) == (1 | 1 << 8 | AMBIGUOUS << 16) and int(m[3][1]) == 0 and int(m[4][1]) == (0 | 2 << 8)

    def alone(m):
        assert [int(v) for v in m[3]] == [0, 0, 1, 1] and [int(v) for v in m[4]] == [1 | 255 << 8, 255 << 8, 2 | 255 << 8 | NO_MATCH << 16, 4 | 255 << 8 | NO_MATCH << 16]
    three = [[s0], [s1], [s2]]
    cases = [(rules_of(three, max_mm=1, min_delta=0, min_length=0), None, None, None, tie0),
             (rules_of(three, max_mm=1, min_delta=1, min_length=0), None, None, None, tie1),
             # read s0: best 0 at sample 0, runner-up 2 at sample 1: exactly min_delta = 2 above, and one below min_delta = 3
             (rules_of(three, max_mm=1, min_delta=2, min_length=0), None, None, None, lambda m: must(int(m[3][1]) == 0)),
             (rules_of(three, max_mm=1, min_delta=3, min_length=0), None, None, None, lambda m: must(int(m[3][1]) == 3)),
             (rules_of([[s0]], max_mm=1, min_delta=1, min_length=0), None, None, None, alone),
             (rules_of([[s0]], max_mm=1, min_delta=255, min_length=0), None, None, None, None)]
    run_cases(lib, [a], cases, "choice")


def run_sample_counts(lib, sh, A):
    """n_samples A: random barcodes of 10 bases, every sample planted once (with the winners of the issue among them when A allows),
    some with a substitution, some reads random."""
    rng = np.random.default_rng(400 + A)
    samples = random_barcodes(rng, A, [10])
    plant = sorted(set(range(min(A, 70))) | {w for w in WINNERS if w < A} | {A - 1})
    reads = []
    for s in plant:
        reads.append(np.concatenate((samples[s][0], rng.integers(0, 4, 5))).astype(np.uint8))
        x = samples[s][0].copy(); x[int(rng.integers(0, 10))] = rng.integers(0, 4)
        reads.append(np.concatenate((x, rng.integers(0, 4, 5))).astype(np.uint8))
    reads += [rng.integers(0, 4, 15).astype(np.uint8) for _ in range(10)]
    a = arrays_from_bases(reads)

    def expect(m):
        for i, s in enumerate(plant):
            assert int(m[3][2 * i]) == s and (int(m[4][2 * i]) & 255) == 0, (A, s)
        assert m[5][3] >= len(plant)
    run_cases(lib, [a], [(rules_of(samples, max_mm=1, min_delta=0, min_length=0), None, None, None, expect),
                         (rules_of(samples, max_mm=2, min_delta=1, min_length=0, keep_un=1), None, None, None, None)], ("samples", A))


# ---- the plan ----------------------------------------------------------------------------------------------------------------------
def plan_reads(rng, samples, n, off=0):
    """n reads with an inline barcode (most planted, some with substitutions, some short), random ranges and keep flags."""
    A, L = len(samples), len(samples[0][0])
    reads = []
    for _ in range(n):
        u = rng.random()
        if u < 0.08:
            reads.append(rng.integers(0, 4, int(rng.integers(0, off + L))).astype(np.uint8)); continue
        x = samples[int(rng.integers(0, A))][0].copy()
        for _ in range(int(rng.choice([0, 0, 0, 1, 1, 2, 3]))):
            x[int(rng.integers(0, L))] = rng.choice([0, 1, 2, 3, 4])
        reads.append(np.concatenate((rng.integers(0, 4, off), x, rng.integers(0, 4, int(rng.integers(0, 40))))).astype(np.uint8))
    a = arrays_from_bases(reads)
    S = a.seq_offsets.astype(np.int64)
    lens = S[1:] - S[:-1]
    cut3 = np.where(rng.random(n) < 0.5, 0, (rng.random(n) * (lens + 1) * 0.3).astype(np.int64))
    return a, S[:-1].astype(np.uint64), (S[1:] - cut3).astype(np.uint64), (rng.random(n) < 0.85).astype(np.uint8)


def run_plan(lib, sh):
    """Ranges in, keep in, in place, cut on and off, keep_unassigned on and off, min_length exactly met and one short, a dropped record
    passing through, d_info and d_class_counts given and NULL, d_class_counts summing over two calls."""
    rng = np.random.default_rng(500)
    samples = random_barcodes(rng, 5, [8])
    a, begin, end, keep = plan_reads(rng, samples, 150, off=2)
    # min_length exactly met, and one short: record 0 is assigned with 8 bases behind the barcode, record 1 with 7
    x = np.concatenate(([0, 0], samples[0][0], np.zeros(8, np.uint8))).astype(np.uint8)
    a = arrays_from_bases([x, x[:-1]] + [a.bases[int(a.seq_offsets[r]): int(a.seq_offsets[r + 1])] for r in range(a.n_records)])
    shift = np.uint64(len(x) + len(x) - 1)
    begin = np.concatenate(([0, len(x)], begin + shift)).astype(np.uint64)
    end = np.concatenate(([len(x), 2 * len(x) - 1], end + shift)).astype(np.uint64)
    keep = np.concatenate(([1, 1], keep)).astype(np.uint8)
    keep[5] = 0
    h = handle(lib)
    try:
        with Sets(lib, h, [a], pad=5) as sts:
            for cut in (1, 0):
                for keep_un in (0, 1):
                    R = rules_of(samples, [(0, 2)], max_mm=1, min_delta=1, cut=cut, keep_un=keep_un, min_length=8 if cut else 18)
                    m = demux_model([a], R, begin, end, keep)
                    assert (int(m[2][0]), int(m[2][1])) == (1, 0) and int(m[3][0]) == 0 and int(m[3][1]) == 0, (cut, keep_un)
                    assert int(m[3][5]) == DROPPED and int(m[4][5]) == DROPPED and int(m[2][5]) == 0 and (int(m[0][5]), int(m[1][5])) == (int(begin[5]), int(end[5]))
                    assert all(v > 0 for v in m[5][:2] + m[5][3:5]) and (m[5][2] > 0) == bool(cut) and m[5][8] > 0 and (int(m[0][0]) - int(begin[0])) == (10 if cut else 0)
                    assert int(m[6].sum()) == int(keep.sum())
                    for inplace in (False, True):
                        check_demux(lib, h, sts, R, begin, end, keep, pad=5, what=("plan", cut, keep_un, inplace), inplace=inplace, model=m)
                    check_demux(lib, h, sts, R, begin, end, None, pad=5, what=("no keep in", cut, keep_un))
                    check_demux(lib, h, sts, R, None, None, keep, pad=5, what=("no ranges in", cut, keep_un), inplace=True)
            R = rules_of(samples, [(0, 2)], max_mm=1, min_delta=1, min_length=3)
            m = demux_model([a], R, begin, end, keep)
            check_demux(lib, h, sts, R, begin, end, keep, pad=5, what="no info", info=False, model=m)
            check_demux(lib, h, sts, R, begin, end, keep, pad=5, what="no counts", counts0=None, model=m)
            check_demux(lib, h, sts, R, begin, end, keep, pad=5, what="neither", info=False, counts0=None, model=m, inplace=True)
            # the counts of two calls sum: the second call starts from what the first left, here from figures of this test's own
            start = (np.arange(6) * 1000 + 7).astype(np.uint64)
            check_demux(lib, h, sts, R, begin, end, keep, pad=5, what="counts are added to", counts0=start, model=m)
            check_demux(lib, h, sts, R, begin, end, keep, pad=5, what="counts are added to, again", counts0=start + m[6], model=m)
    finally:
        h.close()


# ---- index sets --------------------------------------------------------------------------------------------------------------------
def run_index_sets(lib, sh):
    """One and two index sets; an index record shorter than offset + length; dual barcodes where only the pair tells the samples apart."""
    rng = np.random.default_rng(600)
    AC, GT, TT = codes_of("AC"), codes_of("GT"), codes_of("TT")
    pair_samples = [[AC, GT], [AC, TT], [GT, GT]]
    n = 90
    which = rng.integers(0, 3, n)
    reads = [rng.integers(0, 4, int(rng.integers(0, 30))).astype(np.uint8) for _ in range(n)]
    i1 = [np.concatenate(([3], pair_samples[w][0], rng.integers(0, 4, int(rng.integers(0, 3))))).astype(np.uint8) for w in which]
    i2 = [np.concatenate((pair_samples[w][1], rng.integers(0, 4, int(rng.integers(0, 3))))).astype(np.uint8) for w in which]
    i1[7] = i1[7][:2]; i2[9] = i2[9][:1]; i1[11] = np.zeros(0, np.uint8)          # shorter than offset + length
    i2[13] = np.array([2, 4], np.uint8)                                         # G N: one away from GT, two from TT
    sets = [arrays_from_bases(reads), arrays_from_bases(i1), arrays_from_bases(i2)]
    keep = (rng.random(n) < 0.9).astype(np.uint8); keep[7] = keep[9] = keep[11] = keep[13] = 1

    def dual(m):
        for r in range(n):
            if r in (7, 9, 11):
                assert int(m[3][r]) == 3 and (int(m[4][r]) >> 16) == SHORT
            elif keep[r] and r != 13:
                assert int(m[3][r]) == which[r] and int(m[4][r]) & 255 == 0, r
        assert int(m[4][13]) & 255 == 1 and m[5][2] == 0
    R2 = rules_of(pair_samples, [(1, 1), (2, 0)], max_mm=1, min_delta=1, min_length=0)
    cases = [(R2, None, None, keep, dual), (dict(R2, slots=[(2, 0), (1, 1)], barcodes=[[s[1], s[0]] for s in pair_samples]), None, None, keep, None),
             (dict(R2, keep_un=1, max_mm=0), None, None, None, None)]
    run_cases(lib, sets, cases, "two index sets")
    one = [[np.concatenate((s[0], s[1]))] for s in pair_samples]
    joined = arrays_from_bases([np.concatenate((u[1:3], v[:2])) if len(u) >= 3 and len(v) >= 2 else np.zeros(0, np.uint8) for u, v in zip(i1, i2)])
    run_cases(lib, [sets[0], joined], [(rules_of(one, [(1, 0)], max_mm=0, min_length=0), None, None, keep,
                                        lambda m: must(all(int(m[3][r]) == which[r] for r in range(n) if keep[r] and r not in (7, 9, 11, 13))))], "one index set")
    # an inline slot and an index slot together: the cut moves behind the inline one only
    S = sets[0].seq_offsets.astype(np.int64)
    mixed = [np.concatenate((pair_samples[w][0], x)).astype(np.uint8) for w, x in zip(which, reads)]
    run_cases(lib, [arrays_from_bases(mixed), sets[2]], [(rules_of(pair_samples, [(0, 0), (1, 0)], max_mm=0, min_length=0), None, None, keep,
                                                          lambda m: must(m[5][2] == 2 * m[5][0] and m[5][0] > 20))], "inline and index")


# ---- record counts -----------------------------------------------------------------------------------------------------------------
def count_arrays(n_rec, rng, samples):
    """n_rec reads of 12 bases with an 8-base barcode in front, built as one array operation."""
    A = len(samples)
    B = np.stack([s[0] for s in samples])
    which = rng.integers(0, A, n_rec)
    bases = np.concatenate((B[which], rng.integers(0, 4, (n_rec, 4)).astype(np.uint8)), axis=1)
    noise = rng.random((n_rec, 12)) < 0.04
    bases[noise] = rng.integers(0, 5, int(noise.sum()))
    S = (12 * np.arange(n_rec + 1)).astype(np.uint64)
    titles = np.empty(2 * n_rec, np.uint8); titles[0::2] = ord("@"); titles[1::2] = ord("t")
    return Arrays(bases.reshape(-1).astype(np.uint8), np.full(12 * n_rec, 30, np.uint8), titles, S, (2 * np.arange(n_rec + 1)).astype(np.uint64), [0, n_rec])


def run_count(lib, sh, n_rec):
    rng = np.random.default_rng(700 + n_rec)
    samples = random_barcodes(rng, 7, [8])
    a = count_arrays(n_rec, rng, samples)
    S = a.seq_offsets
    begin = S[:-1].copy()
    end = S[1:] - rng.integers(0, 6, n_rec).astype(np.uint64)
    keep = (rng.random(n_rec) < 0.8).astype(np.uint8)
    R = rules_of(samples, max_mm=1, min_delta=1, min_length=2)
    h = handle(lib)
    try:
        with Sets(lib, h, [a]) as sts:
            if n_rec == 0:
                got = demux_call(lib, h, [sts[0].cols_in()], 0, lib_rules(lib, R), counts0=np.arange(8))
                assert got.error is None and got.stats == [0] * 9 and got.untouched
                return
            m = demux_model([a], R, begin, end, keep)
            if n_rec >= 63:
                assert all(v > 0 for v in m[5][:5]) and m[5][5] > 0
            check_demux(lib, h, sts, R, begin, end, keep, what=n_rec, model=m)
            check_demux(lib, h, sts, R, begin, end, keep, what=(n_rec, "in place"), inplace=True, model=m)
    finally:
        h.close()


# ---- fuzz ------------------------------------------------------------------------------------------------------------------------
def fuzz_case(seed, n_rec):
    """-> (sets, begin, end, keep, rules): seed % 3 = 0 a single inline barcode, 1 an inline and an index slot, 2 two index sets."""
    rng = np.random.default_rng(3000 + seed)
    kind = seed % 3
    A = [5, 64, 200, 1, 65, 2][seed % 6]
    lens = [int(rng.integers(4, 13))] if kind == 0 else [int(rng.integers(4, 10)), int(rng.integers(4, 10))]
    samples = random_barcodes(rng, A, lens)
    off = [int(rng.integers(0, 4)) for _ in lens]
    slots = [(0, off[0])] if kind == 0 else [(0, off[0]), (1, off[1])] if kind == 1 else [(1, off[0]), (2, off[1])]
    other = np.array([4, 4, 255, 7], np.uint8)

    def spoiled(s, w):
        x = samples[w][s].copy()
        for _ in range(int(rng.choice([0, 0, 0, 1, 1, 2, 3]))):
            x[int(rng.integers(0, len(x)))] = rng.choice([0, 1, 2, 3, 4, 255])
        return x
    per_src = {0: [], 1: [], 2: []}
    for _ in range(n_rec):
        w = int(rng.integers(0, A))
        body = rng.integers(0, 4, int(rng.integers(0, 100))).astype(np.uint8)
        amb = rng.random(len(body)) < 0.05
        body[amb] = other[rng.integers(0, 4, int(amb.sum()))]
        rec = {0: body, 1: rng.integers(0, 4, int(rng.integers(0, 4))).astype(np.uint8), 2: rng.integers(0, 4, int(rng.integers(0, 4))).astype(np.uint8)}
        for s, (src, o) in enumerate(slots):
            u = rng.random()
            if u < 0.06:
                x = rng.integers(0, 4, int(rng.integers(0, o + lens[s]))).astype(np.uint8)           # short
                rec[src] = x if src else np.concatenate((x, np.zeros(0, np.uint8)))
                continue
            x = spoiled(s, w) if u < 0.85 else rng.integers(0, 4, lens[s]).astype(np.uint8)
            rec[src] = np.concatenate((rng.integers(0, 4, o).astype(np.uint8), x, rec[src] if src == 0 else rng.integers(0, 4, int(rng.integers(0, 3))).astype(np.uint8)))
        for k in per_src:
            per_src[k].append(rec[k].astype(np.uint8))
    n_sets = 1 + max(src for src, _ in slots)
    sets = [arrays_from_bases(per_src[k]) for k in range(n_sets)]
    S = sets[0].seq_offsets.astype(np.int64)
    ln = S[1:] - S[:-1]
    whole = rng.random(n_rec) < 0.6
    cut5 = np.where(whole, 0, (rng.random(n_rec) * (ln + 1) * 0.1).astype(np.int64))
    cut3 = np.where(whole, 0, (rng.random(n_rec) * (ln - cut5 + 1) * 0.3).astype(np.int64))
    begin, end = (S[:-1] + cut5).astype(np.uint64), (S[1:] - cut3).astype(np.uint64)
    keep = (rng.random(n_rec) < 0.85).astype(np.uint8)
    R = rules_of(samples, slots, max_mm=int(rng.integers(0, 4)), slot_max=None if rng.random() < 0.5 else [None if rng.random() < 0.3 else int(rng.integers(0, 3)) for _ in lens],
                 min_delta=int(rng.integers(0, 3)), cut=1 if seed % 2 == 0 else int(rng.integers(0, 2)), keep_un=int(rng.integers(0, 2)), min_length=int(rng.integers(0, 50)))
    return sets, begin, end, keep, R


def run_fuzz(lib, sh, seed):
    n_rec = sh["demux_fuzz"][1]
    sets, begin, end, keep, R = fuzz_case(seed, n_rec)
    m = demux_model(sets, R, begin, end, keep)
    print("demux fuzz", seed, "samples", len(R["barcodes"]), "slots", R["slots"], "lens", slot_lens(R), "stats", m[5])
    assert min(m[5][3], m[5][6], m[5][0]) > n_rec // 40, m[5]
    h = handle(lib)
    try:
        with Sets(lib, h, sets, pad=3) as sts:
            check_demux(lib, h, sts, R, begin, end, keep, pad=3, what=("fuzz", seed), model=m)
            check_demux(lib, h, sts, R, pad=3, what=("fuzz, whole reads", seed), inplace=True)
    finally:
        h.close()


def run_fuzz_exercises_everything(lib, sh):
    """Over the seeds of the fuzz every statistic is above 0, and so is every reason and the unassigned class (the model alone)."""
    seeds, n_rec = sh["demux_fuzz"]
    total = np.zeros(9, np.int64)
    for seed in range(seeds):
        sets, begin, end, keep, R = fuzz_case(seed, n_rec)
        m = demux_model(sets, R, begin, end, keep)
        total += np.array(m[5])
        assert m[6][-1] > 0
    assert np.all(total > 0), total.tolist()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def run_arg_refusals(lib, sh):
    rng = np.random.default_rng(800)
    samples = random_barcodes(rng, 4, [8, 6])
    sets, begin, end, keep, _ = fuzz_case(1, 20)
    a, idx = sets[0], sets[1]
    good = rules_of(samples, [(0, 1), (1, 0)], max_mm=2, min_delta=1, min_length=1)
    h = handle(lib)

    def broken():
        mk = lambda **kw: lib_rules(lib, good, **kw)
        raw = [[b.tobytes() for b in s] for s in good["barcodes"]]
        yield "no samples", mk(barcodes=[])
        yield "1024 samples", lib_rules(lib, rules_of(random_barcodes(rng, 1024, [8, 6]), good["slots"]))
        dr = mk(); dr.n_slots = 0
        yield "no slots", dr
        dr = mk(); dr.n_slots = 3
        yield "three slots", dr
        yield "a source above n_index_sets", mk(slots=[(0, 1), (2, 0)])
        dr = mk(); dr.slot_len[1] = 0
        yield "a length of 0", dr
        yield "a length of 65", lib_rules(lib, rules_of([[np.zeros(65, np.uint8), s[1]] for s in samples[:1]], good["slots"]))
        dr = lib_rules(lib, rules_of([[s[0]] for s in samples], [(0, 1)])); dr.slot_len[1] = 4
        yield "a length behind n_slots", dr
        yield "code 4", mk(barcodes=raw[:3] + [[raw[3][0], b"\x01\x02\x04\x03\x00\x01"]])
        yield "code 255 in the last position", mk(barcodes=raw[:3] + [[raw[3][0][:7] + b"\xff", raw[3][1]]])
        yield "two samples alike", mk(barcodes=raw[:3] + [raw[1]])
        yield "max_mismatches above the summed lengths", mk(max_mismatches=15)
        yield "cut 2", mk(cut=2)
        for k in range(3):
            res = [0, 0, 0]; res[k] = 1
            yield "reserved[%d]" % k, lib_rules(lib, good, res)
    try:
        with Sets(lib, h, [a, idx]) as sts:
            n = a.n_records
            S = a.seq_offsets
            cins = [st.cols_in() for st in sts]
            zeros = np.zeros(5, np.uint64)
            checked = 0
            for name, dr in broken():
                got = demux_call(lib, h, cins, n, dr, counts0=zeros)
                assert got.error is not None and got.error.code == E_ARG and got.untouched, (name, got.error)
                checked += 1
            assert checked == 16
            for name, plan in (("begin alone", (S[:-1], None, None)), ("end alone", (None, S[1:], None))):
                got = demux_call(lib, h, cins, n, lib_rules(lib, good), plan, counts0=zeros)
                assert got.error is not None and got.error.code == E_ARG and got.untouched, (name, got.error)
                assert str(got.error).endswith("columns: d_begin_in and d_end_in go together"), str(got.error)      # (the shared helper's words)
            got = demux_call(lib, h, cins, n, lib_rules(lib, good, reserved=(0, 0, 9)), counts0=zeros)
            assert str(got.error).endswith("demux rules: reserved fields must be 0"), str(got.error)
            # an index set of another record count, and three of them
            got = demux_call(lib, h, [cins[0], sts[1].cols_in(0, n - 1)], n, lib_rules(lib, good), counts0=zeros)
            assert got.error is not None and got.error.code == E_ARG and got.untouched, got.error
            with Dev(h) as d:
                out = [d.fill(8 * n), d.fill(8 * n), d.fill(n), d.fill(4 * n)]
                for name, args in (("null d_class", out[:3] + [None]), ("null d_keep", out[:2] + [None, out[3]]), ("null d_begin", [None] + out[1:])):
                    try:
                        h.columns_demux_plan(cins[0], cins[1:], lib_rules(lib, good), None, None, None, *args)
                        raise AssertionError(name)
                    except lib.DsrcGpuError as e:
                        assert e.code == E_ARG and str(e).endswith("null argument"), (name, e)
                try:
                    h.columns_demux_plan(cins[0], [cins[1]] * 3, lib_rules(lib, good), None, None, None, *out)
                    raise AssertionError("three index sets")
                except lib.DsrcGpuError as e:
                    assert e.code == E_ARG
                assert all(d.down(p, s) == b"\xA5" * (s + 8) for p, s in zip(out, (8 * n, 8 * n, n, 4 * n)))
            check_demux(lib, h, sts, good, what="the same handle, clean")
            check_demux(lib, h, sts, dict(good, max_mm=14, min_delta=255), what="the largest figures")
            got = demux_call(lib, h, [sts[0].cols_in(3, 0), sts[1].cols_in(3, 0)], 0, lib_rules(lib, good), counts0=zeros)          # no records
            assert got.error is None and got.stats == [0] * 9 and got.untouched
    finally:
        h.close()
    hc = ce.handle(lib, dataclasses.replace(Config.from_levels(0, 0), color_space=True))
    try:
        with Sets(lib, hc, [a, idx]) as sts:
            got = demux_call(lib, hc, [st.cols_in() for st in sts], a.n_records, lib_rules(lib, good))
            assert got.error is not None and got.error.code == E_ARG and got.untouched
            assert "columns are defined for base space" in str(got.error)
    finally:
        hc.close()


def run_input_errors(lib, sh):
    """Offsets out of order or above bases_len through each of the three sides, bad ranges through the first: the code, the side,
    the record, outputs still 0xA5, and the same handle plans the clean arrays afterwards."""
    sets, begin, end, keep, R = fuzz_case(2, 41)                     # two index sets
    R = dict(R, slots=[(1, 0), (2, 0)])
    sets = [sets[0], sets[1], sets[2]]
    keep = np.ones(41, np.uint8); keep[20] = 0; keep[40] = 0
    n = 41
    h = handle(lib)
    dr = lib_rules(lib, R)
    checked = 0
    try:
        with Sets(lib, h, sets) as sts:
            cins = [st.cols_in() for st in sts]
            for side, st in enumerate(sts):
                a = st.a
                S = lambda r: int(a.seq_offsets[r])
                plants = [("order", lambda r: st.poke("seq_offs", r + 1, S(r + 2) + 1 if r + 2 <= n else S(r) - 1, np.uint64), "not non-decreasing"),
                          ("end", lambda r: st.poke("seq_offs", n, len(a.bases) + 5, np.uint64), "above bases_len"),
                          ("wild", lambda r: st.poke("seq_offs", n, 2 ** 64 - 1, np.uint64), "above bases_len")]
                for name, plant, word in plants:
                    for r in (0, 20, 40) if name == "order" else (40,):
                        if name == "order" and r == 40 and S(40) == 0:
                            continue
                        plant(r)
                        for plan in ((None, None, None), (begin, end, keep)) if side else ((None, None, None),):
                            got = demux_call(lib, h, cins, n, dr, plan, counts0=np.zeros(len(R["barcodes"]) + 1, np.uint64))
                            assert got.error is not None and got.error.code == E_INPUT and got.untouched, (side, name, r, got.error)
                            assert "dsrcgpu_columns_demux_plan, read %d: columns: record " % (side + 1) in str(got.error) and word in str(got.error), str(got.error)
                        st.restore()
                        checked += 1
                check_demux(lib, h, sts, R, begin, end, keep, what=("after side", side))
            S = sets[0].seq_offsets

            def ranged(r, b=None, e=None):
                pb, pe = begin.copy(), end.copy()
                if b is not None: pb[r] = b
                if e is not None: pe[r] = e
                return pb, pe, keep
            ranges = [("begin low", lambda r: ranged(r, b=int(S[r]) - 1), "d_begin lies below"), ("end high", lambda r: ranged(r, e=int(S[r + 1]) + 1), "d_end lies above"),
                      ("begin above end", lambda r: ranged(r, b=int(S[r + 1]), e=int(S[r + 1]) - 1), "d_begin lies above d_end")]
            for name, plan_of, word in ranges:
                for r in (1, 20, 40):
                    if int(S[r + 1]) == int(S[r]) or int(S[r]) == 0:
                        continue
                    for inplace in (False, True):
                        got = demux_call(lib, h, cins, n, dr, plan_of(r), inplace=inplace)
                        assert got.error is not None and got.error.code == E_INPUT, (name, r, got.error)
                        assert "demux_plan, read 1: columns: record %d:" % r in str(got.error) and word in str(got.error), str(got.error)
                        if not inplace:
                            assert got.untouched
                    checked += 1
            check_demux(lib, h, sts, R, begin, end, keep, what="after the ranges")
    finally:
        h.close()
    assert checked >= 15, checked


def run_codec_state(lib, sh):
    """Neither call touches what the codec carries (see columns_adapt_cases.run_codec_state)."""
    sets, begin, end, keep, R = fuzz_case(0, 80)
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
            with Sets(lib, h, sets) as sts:
                m = check_demux(lib, h, sts, R, begin, end, keep)
                check_partition(lib, h, sts[0], m[3], len(R["barcodes"]) + 1, m[0], m[1], m[2])
                assert h.get_fields_capacity() == 11
            assert text_blocks(h) == text_blocks(fresh), layout
        finally:
            h.close(); fresh.close()


# ---- the partition -----------------------------------------------------------------------------------------------------------------
def partition_model(a: Arrays, cls, n_classes, begin=None, end=None, keep=None, titles=True):
    """-> (bases, quals, titles, seq_offsets, title_offsets, source, totals[4], class_records): the kept records with a class below
    n_classes, sorted by class with a STABLE sort."""
    n = a.n_records
    S = a.seq_offsets.astype(np.int64)
    b = S[:-1] if begin is None else np.asarray(begin).astype(np.int64)
    e = S[1:] if end is None else np.asarray(end).astype(np.int64)
    k = np.ones(n, bool) if keep is None else np.asarray(keep) != 0
    cls = np.asarray(cls).astype(np.int64) & 0xFFFFFFFF
    inside = k & (cls < n_classes)
    idx = np.nonzero(inside)[0]
    source = idx[np.argsort(cls[idx], kind="stable")]
    crecs = np.concatenate(([0], np.cumsum(np.bincount(cls[idx], minlength=n_classes)))).tolist()
    bases, seq_offs = cs._ragged(a.bases, b[source], (e - b)[source])
    quals, _ = cs._ragged(a.quals, b[source], (e - b)[source])
    left = int((k & ~inside).sum())
    if not titles:
        return bases, quals, None, seq_offs, None, source.astype(np.uint64), [len(source), len(bases), 0, left], crecs
    T = a.title_offsets.astype(np.int64)
    tt, title_offs = cs._ragged(a.titles, T[:-1][source], (T[1:] - T[:-1])[source])
    return bases, quals, tt, seq_offs, title_offs, source.astype(np.uint64), [len(source), len(bases), len(tt), left], crecs


class PartCall(cs.SelCall):
    """One dsrcgpu_columns_partition_device on output arrays this test owns (as SelCall)."""

    def __init__(self, lib, h, cin, d_begin, d_end, d_keep, d_class, n_classes, R, S, T, titles=True, caps=None, source=True):
        caps = caps or {}
        with Dev(h) as d:
            sizes = {"bases": S, "quals": S, "titles": T, "seq_offs": 8 * (R + 1), "title_offs": 8 * (R + 1), "source": 8 * R}
            ptr = {k: d.fill(v) for k, v in sizes.items()}
            out = lib.Columns(ptr["bases"], caps.get("bases_cap", S), ptr["quals"], caps.get("quals_cap", S),
                              ptr["titles"] if titles else None, caps.get("titles_cap", T) if titles else 0,
                              ptr["seq_offs"], ptr["title_offs"] if titles else None, caps.get("records_cap", R))
            self.error = self.totals = self.all_totals = self.class_records = None
            try:
                self.all_totals, self.class_records = h.columns_partition_device(cin, d_begin, d_end, d_keep, d_class, n_classes, out, ptr["source"] if source else None)
                self.totals = self.all_totals[:3]
            except lib.DsrcGpuError as e:
                self.error = e
            self.raw = {k: d.down(ptr[k], v) for k, v in sizes.items()}


def check_partition(lib, h, st, cls, n_classes, begin=None, end=None, keep=None, pad=0, titles=True, what=None, source=True):
    """Arrays staged in `st`, begin / end as positions in the UNPADDED arrays -> the call == the model, twice over (the order is
    computed, so a second call gives the same bytes)."""
    a = st.a
    want = partition_model(a, cls, n_classes, begin, end, keep, titles)
    K, S, T, left = want[6]
    src = want[5].astype(np.int64)
    for c in range(n_classes):                              # the model itself: class-major, input order inside a class
        part = src[want[7][c]: want[7][c + 1]]
        assert np.all(np.diff(part) > 0) and np.all((np.asarray(cls).astype(np.int64)[part] & 0xFFFFFFFF) == c)
    with Dev(h) as d:
        up = lambda v, dt, add=0: None if v is None else d.up((np.asarray(v).astype(dt) + dt(add)).tobytes())
        pc = d.up(np.asarray(cls).astype(np.uint32).tobytes())
        args = (st.cols_in(), up(begin, np.uint64, pad), up(end, np.uint64, pad), up(keep, np.uint8), pc, n_classes)
        calls = [PartCall(lib, h, *args, K, S, T, titles, source=source) for _ in range(2)]
    for call in calls:
        call.assert_equals(want[:6] + ([K, S, T],), titles, source=source, what=what)
        assert call.all_totals == want[6] and call.class_records == want[7], (what, call.all_totals, want[6], call.class_records, want[7])
    return want


def part_arrays(n, seed=7):
    return cs.tiny_records(n, seed)


def run_part_tiles(lib, sh, n):
    """n records (around the tile size) in 5 classes, some beyond n_classes, with ranges and a keep."""
    a, begin, end, keep = part_arrays(n, 11)
    rng = np.random.default_rng(900 + n)
    cls = rng.integers(0, 7, n).astype(np.uint32)
    h = handle(lib)
    try:
        with cs.staged(lib, h, a, pad=2) as st:
            check_partition(lib, h, st, cls, 5, begin, end, keep, pad=2, what=("tiles", n))
            check_partition(lib, h, st, cls, 7, what=("tiles, whole", n), titles=False)
    finally:
        h.close()


def run_part_classes(lib, sh, n_classes):
    wg = sh["wg"]
    n = 2 * wg + 77
    a, begin, end, keep = part_arrays(n, 13)
    rng = np.random.default_rng(1000 + n_classes)
    cls = rng.integers(0, n_classes + 2, n).astype(np.uint32)
    cls[rng.random(n) < 0.02] = DROPPED
    h = handle(lib)
    try:
        with cs.staged(lib, h, a) as st:
            w = check_partition(lib, h, st, cls, n_classes, begin, end, keep, what=("classes", n_classes))
            assert w[6][3] > 0 and w[6][0] > 0
    finally:
        h.close()


def run_part_patterns(lib, sh):
    """All records in one class; every record in its own class (1024 records, 1024 classes); empty classes at the front, in the middle
    and at the end; only classes >= n_classes; classes alternating inside a wave and constant inside a wave; a class whose members are
    one per tile."""
    wg = sh["wg"]
    n = 1024
    a, begin, end, keep = part_arrays(n, 17)
    lane = np.arange(n)
    rng = np.random.default_rng(1100)
    patterns = [("one class", np.full(n, 3), 5), ("own class", lane, 1024), ("own class, reversed", lane[::-1].copy(), 1024),
                ("empties", np.where(lane % 3 == 0, 2, np.where(lane % 3 == 1, 3, 6)), 9), ("only beyond", np.full(n, 5), 5),
                ("alternating in a wave", lane % 2, 2), ("alternating by four", lane % 4, 4), ("constant in a wave", (lane // 64) % 5, 5),
                ("one member per tile", np.where(lane % wg == wg - 1, 0, 1 + lane % 3), 4), ("random of 1024", rng.integers(0, 1024, n), 1024)]
    h = handle(lib)
    try:
        with cs.staged(lib, h, a) as st:
            for name, cls, n_classes in patterns:
                for kp in (None, keep):
                    w = check_partition(lib, h, st, cls.astype(np.uint32), n_classes, begin, end, kp, what=name)
                if name == "only beyond":
                    assert w[6] == [0, 0, 0, int(keep.sum())] and w[7] == [0] * 6
                if name == "empties":
                    assert w[7][1] == 0 and w[7][2] == 0 and w[7][4] == w[7][5] == w[7][6] and w[7][7] == w[7][8] == w[7][9]
    finally:
        h.close()


def run_part_refusals(lib, sh):
    """E_ARG, the capacities and the sizing call, titles not wanted without titles in, and the input errors of the select."""
    a, begin, end, keep = part_arrays(300, 19)
    rng = np.random.default_rng(1200)
    cls = rng.integers(0, 4, 300).astype(np.uint32)
    want = partition_model(a, cls, 3, begin, end, keep)
    K, S, T, left = want[6]
    h = handle(lib)
    try:
        with cs.staged(lib, h, a) as st, Dev(h) as d:
            pb, pe, pk, pc = d.up(begin.tobytes()), d.up(end.tobytes()), d.up(keep.tobytes()), d.up(cls.tobytes())
            cin = st.cols_in()
            for name, args in (("n_classes 0", (pb, pe, pk, pc, 0)), ("n_classes 1025", (pb, pe, pk, pc, 1025)), ("null d_class", (pb, pe, pk, None, 3)),
                               ("begin alone", (pb, None, pk, pc, 3))):
                call = PartCall(lib, h, cin, *args, K, S, T)
                assert call.error is not None and call.error.code == E_ARG and call.untouched(), (name, call.error)
            sizing = PartCall(lib, h, cin, pb, pe, pk, pc, 3, K, S, T, caps=dict(bases_cap=0, quals_cap=0, titles_cap=0, records_cap=0))
            assert sizing.error is not None and sizing.error.code == E_CAPACITY and sizing.error.need == [K, S, T] and sizing.untouched()
            assert sizing.error.class_records == want[7] and sizing.error.totals[3] == left
            assert "%d records, %d bases, %d title bytes" % (K, S, T) in str(sizing.error) and "the caller's arrays hold 0, 0 / 0, 0" in str(sizing.error)
            for cap in ("bases_cap", "quals_cap", "titles_cap", "records_cap"):
                full = {"bases_cap": S, "quals_cap": S, "titles_cap": T, "records_cap": K}
                call = PartCall(lib, h, cin, pb, pe, pk, pc, 3, K, S, T, caps={cap: full[cap] - 1})
                assert call.error is not None and call.error.code == E_CAPACITY and call.untouched(), cap
            PartCall(lib, h, cin, pb, pe, pk, pc, 3, K, S, T).assert_equals(want[:6] + ([K, S, T],), what="exact capacities")
            bare = lib.ColumnsIn(cin.d_bases, cin.bases_len, cin.d_quals, None, 0, cin.d_seq_offs, None, 300)
            w2 = partition_model(a, cls, 3, begin, end, keep, titles=False)
            PartCall(lib, h, bare, pb, pe, pk, pc, 3, K, S, T, titles=False).assert_equals(w2[:6] + (w2[6][:3],), titles=False, what="no titles in")
            # input errors, for a kept and a dropped record
            Sx = a.seq_offsets
            for r in (int(np.nonzero(keep)[0][5]), int(np.nonzero(keep == 0)[0][3])):
                bad = begin.copy(); bad[r] = Sx[r + 1] + np.uint64(1)
                call = PartCall(lib, h, cin, d.up(bad.tobytes()), pe, pk, pc, 3, K, S, T)
                assert call.error is not None and call.error.code == E_INPUT and call.untouched() and "record %d:" % r in str(call.error), call.error
                st.poke("title_offs", r + 1, len(a.titles) + 9, np.uint64)
                call = PartCall(lib, h, cin, pb, pe, pk, pc, 3, K, S, T)
                assert call.error is not None and call.error.code == E_INPUT and call.untouched() and "d_title_offs" in str(call.error), call.error
                st.restore()
            check_partition(lib, h, st, cls, 3, begin, end, keep, what="the same handle, clean")
            none = PartCall(lib, h, st.cols_in(5, 0), None, None, None, pc, 3, 0, 0, 0)
            assert none.error is None and none.all_totals == [0, 0, 0, 0] and none.class_records == [0, 0, 0, 0]
            assert none.array("seq_offs", 1, np.uint64)[0] == 0 and none.array("title_offs", 1, np.uint64)[0] == 0
    finally:
        h.close()


# ---- the Python layers -----------------------------------------------------------------------------------------------------------------
def strings_of(samples):
    return ["+".join("".join("ACGT"[v] for v in b) for b in sample) for sample in samples]


def run_python_layers(lib, sh, device):
    """demux_plan, partition_columns, class_view and demux_columns through torch == the model; the ValueErrors."""
    from dsrc_amd import columns
    sets, begin, end, keep, R = fuzz_case(1, 120)            # an inline and an index slot
    A = len(R["barcodes"])
    kw = dict(index=[ca.tensors(sets[1], device)], slots=[("read", R["slots"][0][1]), ("index1", R["slots"][1][1])], max_mismatches=R["max_mm"],
              slot_max_mismatches=None if R["slot_max"] is None else [NO_LIMIT - 1 if v is None else v for v in R["slot_max"]],
              min_delta=R["min_delta"], cut=bool(R["cut"]), keep_unassigned=bool(R["keep_un"]), min_length=R["min_length"])
    if R["slot_max"] is not None:
        R = dict(R, slot_max=[NO_LIMIT - 1 if v is None else v for v in R["slot_max"]])
    m = demux_model(sets, R, begin, end, keep)
    t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v).astype(dt)).to(device)
    cols = ca.tensors(sets[0], device)
    h = handle(lib)
    try:
        names = strings_of(R["barcodes"])
        got = columns.demux_plan(h, cols, names, t(begin, np.int64), t(end, np.int64), t(keep, np.uint8), return_info=True, **kw)
        b, e, k, c, stats, best, second, reason = got
        assert np.array_equal(b.cpu().numpy().astype(np.uint64), m[0]) and np.array_equal(e.cpu().numpy().astype(np.uint64), m[1])
        assert np.array_equal(k.cpu().numpy(), m[2]) and np.array_equal(c.cpu().numpy().view(np.uint32), m[3])
        assert [stats[name] for name in STATS] == m[5] and tuple(lib.DEMUX_STATS) == STATS
        assert np.array_equal(stats["class_counts"].cpu().numpy().astype(np.uint64), m[6])
        came = keep != 0
        info = m[4].astype(np.int64)
        for tensor, want in ((best, info & 255), (second, (info >> 8) & 255), (reason, (info >> 16) & 255)):
            assert np.array_equal(tensor.cpu().numpy(), np.where(came, want, -1))
        # the counts of a second batch are added
        again = columns.demux_plan(h, cols, [tuple(s.split("+")) for s in names], t(begin, np.int64), t(end, np.int64), t(keep, np.uint8), counts=stats["class_counts"], **kw)
        assert again[4]["class_counts"] is stats["class_counts"] and np.array_equal(stats["class_counts"].cpu().numpy().astype(np.uint64), 2 * m[6])
        # partition_columns and class_view
        n_classes = A + 1
        parts, source = columns.partition_columns(h, cols, c, n_classes, b, e, k, return_source=True)
        w = partition_model(sets[0], m[3], n_classes, m[0], m[1], m[2])
        assert np.array_equal(parts.bases.cpu().numpy(), w[0]) and np.array_equal(parts.quals.cpu().numpy(), w[1]) and np.array_equal(parts.titles.cpu().numpy(), w[2])
        assert np.array_equal(parts.seq_offsets.cpu().numpy().astype(np.uint64), w[3]) and np.array_equal(parts.title_offsets.cpu().numpy().astype(np.uint64), w[4])
        assert np.array_equal(source.cpu().numpy().astype(np.uint64), w[5]) and parts.block_records.tolist() == w[7]
        for cl in range(n_classes):
            v = columns.class_view(parts, cl)
            only = partition_model(sets[0], np.where(m[3] == cl, 0, 9), 1, m[0], m[1], m[2])
            assert v.n_records == only[6][0] and v.bases.data_ptr() == parts.bases.data_ptr()
            lo, hi = int(v.seq_offsets[0]), int(v.seq_offsets[-1])
            assert np.array_equal(v.bases[lo:hi].cpu().numpy(), only[0]) and np.array_equal((v.seq_offsets - lo).cpu().numpy().astype(np.uint64), only[3])
        # demux_columns = the two in sequence
        parts2, stats2 = columns.demux_columns(h, cols, names, begin=t(begin, np.int64), end=t(end, np.int64), keep=t(keep, np.uint8), **kw)
        w2 = partition_model(sets[0], m[3], A + (1 if R["keep_un"] else 0), m[0], m[1], m[2])
        assert np.array_equal(parts2.bases.cpu().numpy(), w2[0]) and stats2["class_records"] == w2[7] and parts2.block_records.tolist() == w2[7]
        assert np.array_equal(parts2.title_offsets.cpu().numpy().astype(np.uint64), w2[4])
        # revcomp: the reverse complement of the barcodes given reverse-complemented is the barcodes
        rc = lambda s: "".join("TGCA"["ACGT".index(ch)] for ch in reversed(s))
        flipped = [s.split("+")[0] + "+" + rc(s.split("+")[1]) for s in names]
        again = columns.demux_plan(h, cols, flipped, t(begin, np.int64), t(end, np.int64), t(keep, np.uint8), revcomp=(False, True), **kw)
        assert np.array_equal(again[3].cpu().numpy().view(np.uint32), m[3])
        for bad in (["ACGT", "ACGT"], ["ACGN"], ["ACGT", "ACG"], [], "ACGT", ["ACGT", ("ACGT", "AC")], ["A" * 65], [5]):
            try:
                columns.demux_plan(h, cols, bad)
                raise AssertionError(bad)
            except ValueError:
                pass
        for bad_kw in (dict(max_mismatches=99), dict(slots=[("index1", 0)]), dict(slots=[(0, 0), (0, 4)]), dict(min_delta=-1), dict(index=[cols, cols, cols])):
            try:
                columns.demux_plan(h, cols, ["ACGT", "TTTT"], **bad_kw)
                raise AssertionError(bad_kw)
            except ValueError:
                pass
        for bad_args in ((c[:-1], 3), (c.to(torch.float32), 3), (c, 0), (c, 1025)):
            try:
                columns.partition_columns(h, cols, *bad_args)
                raise AssertionError(bad_args[1])
            except ValueError:
                pass
        # default slots: inline at offset 0; a dual inline barcode reads the second slot behind the first
        inline = columns.demux_plan(h, cols, ["ACGT+AA", "TTTT+CC"], max_mismatches=0, min_length=0)
        Rin = rules_of([[codes_of("ACGT"), codes_of("AA")], [codes_of("TTTT"), codes_of("CC")]], [(0, 0), (0, 4)], max_mm=0, min_length=0)
        assert np.array_equal(inline[3].cpu().numpy().view(np.uint32), demux_model(sets[:1], Rin)[3])
    finally:
        h.close()


def run_filter_columns(lib, sh, device):
    """filter_columns(demux=...) == the trim plan's model, the demux model on its plan, the partition model on that; the ValueErrors."""
    from dsrc_amd import columns
    sets, _, _, _, R = fuzz_case(0, 120)                     # a single inline barcode
    a = sets[0]
    R = dict(R, min_length=4, cut=1, keep_un=1)
    trim = cs.rules_of(quality_3=20, min_length=4, max_n=3)
    tb, te, tk, _ = cs.plan_model(a, trim)
    m = demux_model(sets, R, tb, te, tk)
    n_classes = len(R["barcodes"]) + 1
    w = partition_model(a, m[3], n_classes, m[0], m[1], m[2])
    assert w[6][0] > 30 and w[7][-1] > w[7][-2]
    dm = dict(barcodes=strings_of(R["barcodes"]), slots=[("read", R["slots"][0][1])], max_mismatches=R["max_mm"],
              slot_max_mismatches=None if R["slot_max"] is None else [NO_LIMIT - 1 if v is None else v for v in R["slot_max"]], min_delta=R["min_delta"],
              keep_unassigned=True)
    if R["slot_max"] is not None and R["slot_max"][0] is None:
        dm["slot_max_mismatches"] = None
    cols = ca.tensors(a, device)
    h = handle(lib)
    try:
        parts, stats = columns.filter_columns(h, cols, demux=dm, quality_3=20, min_length=4, max_n=3)
        assert np.array_equal(parts.bases.cpu().numpy(), w[0]) and np.array_equal(parts.quals.cpu().numpy(), w[1]) and np.array_equal(parts.titles.cpu().numpy(), w[2])
        assert np.array_equal(parts.seq_offsets.cpu().numpy().astype(np.uint64), w[3]) and parts.block_records.tolist() == w[7]
        assert [stats["demux"][name] for name in STATS] == m[5] and stats["demux"]["class_records"] == w[7]
        plain, plain_stats = columns.filter_columns(h, cols, quality_3=20, min_length=4, max_n=3)
        assert "demux" not in plain_stats and plain.block_records.tolist() == [0, plain.n_records]
        for bad in (dict(quality_5=20), dict(dedup=True)):
            try:
                columns.filter_columns(h, cols, demux=dm, **bad)
                raise AssertionError(bad)
            except ValueError:
                pass
        for bad in (dict(), dict(dm, nonsense=1), "ACGT"):
            try:
                columns.filter_columns(h, cols, demux=bad)
                raise AssertionError(bad)
            except ValueError:
                pass
    finally:
        h.close()


def run_filter_pairs(lib, sh, device):
    """filter_pairs(demux=...) with a slot on read 1 and one on read 2 == the models in sequence: the trim plans, the demux plan on read
    1 with read 2 as an index set, its keep on both sides, begin2 advanced behind read 2's barcode, a partition per side."""
    from dsrc_amd import columns
    rng = np.random.default_rng(1400)
    samples = random_barcodes(rng, 4, [6, 4])
    n = 120
    r1, r2 = [], []
    for _ in range(n):
        w = int(rng.integers(0, 4))
        x0, x1 = samples[w][0].copy(), samples[w][1].copy()
        if rng.random() < 0.3:
            x0[int(rng.integers(0, 6))] = rng.integers(0, 5)
        if rng.random() < 0.2:
            x1 = rng.integers(0, 4, 4).astype(np.uint8)
        r1.append(np.concatenate((x0, rng.integers(0, 4, int(rng.integers(0, 50))))).astype(np.uint8))
        r2.append(np.concatenate(([2], x1, rng.integers(0, 4, int(rng.integers(0, 50))))).astype(np.uint8) if rng.random() < 0.95 else np.array([1, 2], np.uint8))
    a1, a2 = arrays_from_bases(r1), arrays_from_bases(r2)
    trim = cs.rules_of(min_length=5)
    tb1, te1, tk1, _ = cs.plan_model(a1, trim)
    tb2, te2, tk2, _ = cs.plan_model(a2, trim)
    R = rules_of(samples, [(0, 0), (1, 1)], max_mm=1, min_delta=1, keep_un=1, min_length=5)
    m = demux_model([a1, a2], R, tb1, te1, tk1)
    assigned = (m[3] < 4)
    S2 = a2.seq_offsets[:-1]
    b2 = np.where(assigned, np.minimum(np.maximum(tb2, S2 + np.uint64(5)), te2), tb2)
    keep = m[2] & tk2
    w1 = partition_model(a1, m[3], 5, m[0], m[1], keep)
    w2 = partition_model(a2, m[3], 5, b2, te2, keep)
    assert w1[6][0] > 40 and w1[7] == w2[7] and w1[7][4] < w1[7][5]
    dm = dict(barcodes=strings_of(samples), slots=[("read1", 0), ("read2", 1)], max_mismatches=1, keep_unassigned=True)
    c1, c2 = ca.tensors(a1, device), ca.tensors(a2, device)
    h = handle(lib)
    try:
        o1, o2, stats = columns.filter_pairs(h, c1, c2, demux=dm, min_length=5, overlap=False)
        for o, w in ((o1, w1), (o2, w2)):
            assert np.array_equal(o.bases.cpu().numpy(), w[0]) and np.array_equal(o.titles.cpu().numpy(), w[2])
            assert np.array_equal(o.seq_offsets.cpu().numpy().astype(np.uint64), w[3]) and o.block_records.tolist() == w[7]
        assert [stats["demux"][name] for name in STATS] == m[5] and stats["demux"]["class_records"] == w1[7]
        o1, o2, merged, stats = columns.filter_pairs(h, c1, c2, demux=dm, min_length=5, merge=True, pair_min_overlap=8)
        assert o1.block_records.tolist() == o2.block_records.tolist() and merged.block_records.numel() == 6
        assert merged.n_records + o1.n_records == stats["pair"]["pairs_kept"] and merged.n_records == stats["merge"]["pairs_merged"]
        plain = columns.filter_pairs(h, c1, c2, min_length=5, overlap=False)
        assert "demux" not in plain[2] and plain[0].block_records.tolist() == [0, plain[0].n_records]
        for bad in (dict(quality_5=20), dict(dedup=True)):
            try:
                columns.filter_pairs(h, c1, c2, demux=dm, **bad)
                raise AssertionError(bad)
            except ValueError:
                pass
        try:
            columns.filter_pairs(h, c1, c2, demux=dict(dm, index=[c1, c2]))
            raise AssertionError("three sets")
        except ValueError:
            pass
    finally:
        h.close()


def run_closed_loop(lib, sh, device):
    """Blocks -> decode_columns -> demux_columns -> encode_columns of every class view -> decode: each sample's archive holds that
    sample's reads, cut behind the barcode, in input order."""
    from dsrc_amd import columns
    rng = np.random.default_rng(1300)
    names = ["ACGTAC", "TTGACC", "GGATTA"]
    recs, want = [], {0: [], 1: [], 2: []}
    for i in range(200):
        w = int(rng.integers(0, 4))
        body = "".join("ACGT"[v] for v in rng.integers(0, 4, int(rng.integers(20, 60))))
        bc = names[w] if w < 3 else "CCCCCC"
        if w < 3 and rng.random() < 0.3:
            bc = bc[:2] + "N" + bc[3:]
        seq = bc + body
        q = "".join(chr(33 + int(v)) for v in rng.integers(2, 41, len(seq)))
        recs.append(("@r%d" % i, seq, q))
        if w < 3:
            want[w].append(("@r%d" % i, body, q[6:]))
    text = "\n".join("%s\n%s\n+\n%s" % r for r in recs).encode()
    cfg = Config.from_levels(0, 0)
    h = ce.handle(lib, cfg)
    try:
        blocks = [b for b, _, _ in h.compress_batch([text])]
        d_blocks, offs = cs._stage_blocks(blocks, device)
        sizes = [len(b) for b in blocks]
        cols = columns.decode_columns(h, d_blocks, offs, sizes, device)
        parts, stats = columns.demux_columns(h, cols, names, max_mismatches=1)
        assert stats["class_records"] == [0] + list(np.cumsum([len(want[c]) for c in range(3)])) and stats["records_assigned"] == sum(len(v) for v in want.values())
        for c in range(3):
            view = columns.class_view(parts, c)
            out, o, s, _ = columns.encode_columns(h, view)
            back = columns.decode_columns(h, out, o, s, device)
            S, T = back.seq_offsets.tolist(), back.title_offsets.tolist()
            got = [(bytes(back.titles[T[r]: T[r + 1]].cpu().numpy()).decode(), "".join("ACGTN"[v] for v in back.bases[S[r]: S[r + 1]].cpu().numpy()),
                    "".join(chr(33 + int(v)) for v in back.quals[S[r]: S[r + 1]].cpu().numpy())) for r in range(back.n_records)]
            assert got == want[c], c
    finally:
        h.close()
