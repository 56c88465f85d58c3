"""Shared by tests/test_emu_columns_sel.py (CPU, emulator build) and tests/test_gpu_columns_sel.py (MI355X): the cases of the
columnar select (dsrcgpu_columns_trim_plan, dsrcgpu_columns_select_device; dsrc_amd/csrc/k_columns_sel.h) and what they must give.

The reference has no counterpart, so the yardstick is the integer model written out here: trim_range() is the serial running-sum
rule, plan_model() applies the keep rules in their order, select_model() is the compaction in numpy.  None of it comes from the
library under test, and every comparison is exact equality.  The closed loop ends at the ORACLE: its blocks of the text of the
model-filtered records.

Shapes.  As in columns_cases.SHAPES: the emulator pays a coroutine switch per wave exchange, so its fuzz is 2 seeds x 150 records
where the GPU runs 6 x 2000; everything else is the same on both builds.  A scan tile of k_sel_tiles is one workgroup of records
(256 on the emulator, 1024 on the GPU): 2049 records are above twice either; the second scan level (k_sel_scan_tiles) takes one
workgroup of TILES a round, so 1024 * 1024 + 5 records need a second round with a carry on the GPU -- that count runs there only."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest
import torch        # noqa: F401  before the first handle (see columns_cases)

from tests import columns_cases as cc
from tests import columns_enc_cases as ce
from tests._oracle import Config
from tests.cases import TINY

E_ARG, E_CAPACITY, E_INPUT = -1, -4, -5          # include/dsrc_gpu.h
NO_LIMIT = 0xFFFFFFFF
A5_64 = 0xA5A5A5A5A5A5A5A5

SHAPES = {
    "gpu": dict(cc.SHAPES["gpu"], sel_fuzz=(6, 2000), counts=[1, 63, 64, 65, 1023, 1024, 1025, 2049, 1024 * 1024 + 5]),
    "emu": dict(cc.SHAPES["emu"], sel_fuzz=(2, 150), counts=[1, 63, 64, 65, 1023, 1024, 1025, 2049]),
}
Arrays = ce.Arrays


# ---- the model -------------------------------------------------------------------------------------------------------------------
def trim_ends(q, c5, c3):
    """The two ends by themselves: (start, stop) before they are compared."""
    n = len(q); start, stop = 0, n
    if c5:
        s = best = 0
        for i in range(n):
            s += c5 - q[i]
            if s < 0: break
            if s > best: best, start = s, i + 1
    if c3:
        s = best = 0
        for i in range(n - 1, -1, -1):
            s += c3 - q[i]
            if s < 0: break
            if s > best: best, stop = s, i
    return start, stop


def trim_range(q, c5, c3):
    start, stop = trim_ends(q, c5, c3)
    return (0, 0) if start >= stop else (start, stop)


def rules_of(quality_5=0, quality_3=0, min_length=1, max_n=None, min_mean_quality=0):
    return dict(quality_5=quality_5, quality_3=quality_3, min_length=min_length, max_n=max_n, min_mean_quality=min_mean_quality)


def plan_model(a: Arrays, rules, first=0, n=None):
    """-> begin, end (positions in a.bases), keep, stats of records first .. first + n - 1."""
    S = [int(v) for v in a.seq_offsets]
    n = a.n_records - first if n is None else n
    begin, end, keep = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint8)
    stats = [0] * 6
    quals, bases = a.quals.tolist(), a.bases
    for k in range(n):
        r = first + k
        q = quals[S[r]: S[r + 1]]
        start, stop = trim_range(q, rules["quality_5"], rules["quality_3"])
        begin[k], end[k] = S[r] + start, S[r] + stop
        length = stop - start
        if length < rules["min_length"]:
            stats[3] += 1
        elif rules["max_n"] is not None and int((bases[S[r] + start: S[r] + stop] >= 4).sum()) > rules["max_n"]:
            stats[4] += 1
        elif rules["min_mean_quality"] and sum(q[start:stop]) < rules["min_mean_quality"] * length:
            stats[5] += 1
        else:
            keep[k] = 1
            stats[0] += 1; stats[1] += length; stats[2] += len(q) - length
    return begin, end, keep, stats


def _ragged(data, b, lens):
    """data[b[i] : b[i] + lens[i]] back to back, and the exclusive prefix of lens (len + 1 entries)."""
    offs = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    idx = np.repeat(b - offs[:-1], lens) + np.arange(int(offs[-1]), dtype=np.int64)
    return data[idx], offs.astype(np.uint64)


def select_model(a: Arrays, begin=None, end=None, keep=None, titles=True, first=0, n=None):
    """-> (bases, quals, titles, seq_offsets, title_offsets, source, totals) of the compaction; titles / title_offsets None when
    not wanted.  begin / end are positions in a.bases."""
    n = a.n_records - first if n is None else n
    S = a.seq_offsets.astype(np.int64)[first: first + n + 1]
    b = S[:-1] if begin is None else np.asarray(begin).astype(np.int64)
    e = S[1:] if end is None else np.asarray(end).astype(np.int64)
    k = np.ones(n, bool) if keep is None else np.asarray(keep) != 0
    source = np.nonzero(k)[0].astype(np.uint64)
    bases, seq_offs = _ragged(a.bases, b[k], (e - b)[k])
    quals, _ = _ragged(a.quals, b[k], (e - b)[k])
    if not titles:
        return bases, quals, None, seq_offs, None, source, [int(k.sum()), len(bases), 0]
    T = a.title_offsets.astype(np.int64)[first: first + n + 1]
    tt, title_offs = _ragged(a.titles, T[:-1][k], (T[1:] - T[:-1])[k])
    return bases, quals, tt, seq_offs, title_offs, source, [int(k.sum()), len(bases), len(tt)]


# ---- records ---------------------------------------------------------------------------------------------------------------------
def arrays_from_reads(quals, rng, titles=None, ambiguous=0.5):
    """Reads given by their quality lists; bases are drawn here: A C G T and, `ambiguous` of them, N, the codes 5 .. 18 and 255."""
    lens = np.array([len(q) for q in quals], np.int64)
    total = int(lens.sum())
    other = np.concatenate([[4, 4, 255], np.arange(5, 19)]).astype(np.uint8)
    bases = np.where(rng.random(total) < ambiguous, other[rng.integers(0, len(other), total)], rng.integers(0, 4, total)).astype(np.uint8)
    if titles is None:
        titles = [b"@r%d" % i + b"/" * int(rng.integers(0, 70)) for i in range(len(quals))]
    prefix = lambda v: np.concatenate(([0], np.cumsum(np.asarray(v, np.int64)))).astype(np.uint64)
    seq_offs, title_offs = prefix(lens), prefix([len(t) for t in titles])
    q = np.array([v for ql in quals for v in ql], np.uint8)
    return Arrays(bases, q, np.frombuffer(b"".join(titles), np.uint8).copy(), seq_offs, title_offs, [0, len(quals)])


def fuzz_reads(seed, n, max_len=300):
    """Lengths 0 .. max_len, Phred 0 .. 41, runs of low quality at either end."""
    rng = np.random.default_rng(1000 + seed)
    quals = []
    for _ in range(n):
        L = int(rng.integers(0, max_len + 1))
        q = rng.integers(0, 42, L)
        for at_end in (False, True):
            if L and rng.random() < 0.7:
                run = int(rng.integers(0, L + 1)) if rng.random() < 0.2 else int(rng.integers(0, min(L, 40) + 1))
                low = rng.integers(0, int(rng.integers(3, 25)), run)
                if at_end:
                    q[L - run:] = low
                else:
                    q[:run] = low
        quals.append(q.tolist())
    return arrays_from_reads(quals, rng, ambiguous=0.01)


LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 200, 4097]


def crafted_reads(c):
    """Named quality lists around the cutoff c (1 <= c <= 255) whose answers the serial rule decides in a particular way."""
    lo, hi = max(c - 10, 0), min(c + 10, 255)          # c - lo = d > 0 a base, hi - c = u: at c = 255 nothing lies above the cutoff
    d, u = c - lo, hi - c
    out = {}
    for L in LENGTHS:
        out["all at the cutoff %d" % L] = [c] * L
        out["all above %d" % L] = [hi] * L
        out["all below %d" % L] = [c - 1] * L
    if u:
        # the sum comes back to its maximum d: once inside the first tile, once in a later one; the first position met wins
        k = d // u if d % u == 0 else None
        if k:
            tie = [lo] + [hi] * k + [lo] + [c] * 70 + [hi] * k + [lo] + [hi] * (k + 1) + [hi]
            out["tie 5'"] = tie + [hi] * 30
            out["tie 3'"] = [hi] * 30 + tie[::-1]
        # a good stretch drives the sum below 0; behind it lies a region that would have given a larger maximum
        brk = [lo] * 3 + [hi] * (3 * d // u + 1) + [lo] * 50
        out["break 5'"] = brk + [hi] * 10
        out["break 3'"] = [hi] * 10 + brk[::-1]
    # the break exactly at position 63, 64, 65 counted from the end the pass starts at (needs c - 1 and c + B + 1 as qualities)
    for B in (63, 64, 65):
        if c >= 1 and c + B + 1 <= 255:
            walk = [c - 1] * B + [c + B + 1] + [lo] * 40
            out["break at %d 5'" % B] = walk + [hi] * 5
            out["break at %d 3'" % B] = [hi] * 5 + walk[::-1]
    # both ends eat the whole read: start >= stop
    out["crossing"] = [lo] * 6 + [min(c + 1, 255)] + [lo] * 6
    out["crossing long"] = [lo] * 100 + [min(c + 1, 255)] * 3 + [lo] * 100
    return out


def crafted_arrays(c):
    named = crafted_reads(c)
    rng = np.random.default_rng(c)
    for L in LENGTHS:                                   # ... and every length with qualities around the cutoff
        named["random %d" % L] = np.clip(rng.integers(c - 12, c + 13, L), 0, 255).tolist()
    return list(named), arrays_from_reads(list(named.values()), rng)


def tiny_records(n, seed=7):
    """n records of 0 .. 3 bases with 2-byte titles, sub-ranges and a random keep; all numpy."""
    rng = np.random.default_rng(seed + n)
    lens = rng.integers(0, 4, n)
    S = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    total = int(S[-1])
    titles = np.empty(2 * n, np.uint8); titles[0::2] = ord("@"); titles[1::2] = rng.integers(48, 123, n)
    a = Arrays(rng.integers(0, 19, total).astype(np.uint8), rng.integers(0, 42, total).astype(np.uint8), titles, S,
               (2 * np.arange(n + 1)).astype(np.uint64), [0, n])
    cut5 = rng.integers(0, 4, n); cut5 = np.minimum(cut5, lens)
    cut3 = np.minimum(rng.integers(0, 4, n), lens - cut5)
    begin = S[:-1] + cut5.astype(np.uint64); end = S[1:] - cut3.astype(np.uint64)
    return a, begin, end, (rng.random(n) < 0.6).astype(np.uint8)


# ---- device staging --------------------------------------------------------------------------------------------------------------
class Dev:
    """Device allocations of one test; every buffer has 8 spare bytes of 0xA5 behind it."""

    def __init__(self, h):
        self.h, self.held = h, []

    def up(self, data: bytes):
        p = self.h.dev_alloc(len(data) + 8); self.held.append(p)
        self.h.dev_upload(p, data + b"\xA5" * 8)
        return p

    def fill(self, nbytes):
        return self.up(b"\xA5" * nbytes)

    def down(self, p, nbytes):
        return self.h.dev_download(p, nbytes + 8)

    def free(self):
        for p in self.held:
            self.h.dev_free(p)
        self.held = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def staged(lib, h, a: Arrays, pad=0):
    return ce.Staged(lib, h, a, pad, out_cap=8)


def plan_call(lib, h, cin, rules, n, reserved=(0, 0, 0)):
    """One dsrcgpu_columns_trim_plan on 0xA5-filled outputs -> (error or None, stats, begin, end, keep, outputs untouched)."""
    with Dev(h) as d:
        pb, pe, pk = d.fill(8 * n), d.fill(8 * n), d.fill(n)
        tr = lib.TrimRules(rules["quality_5"], rules["quality_3"], rules["min_length"], NO_LIMIT if rules["max_n"] is None else rules["max_n"],
                           rules["min_mean_quality"], (lib.C.c_uint32 * 3)(*reserved))
        err = stats = None
        try:
            stats = h.columns_trim_plan(cin, tr, pb, pe, pk)
        except lib.DsrcGpuError as e:
            err = e
        raw = [d.down(pb, 8 * n), d.down(pe, 8 * n), d.down(pk, n)]
    untouched = all(r == b"\xA5" * len(r) for r in raw)
    tails = all(r[-8:] == b"\xA5" * 8 for r in raw)
    assert tails, "written behind the end of an output array"
    return (err, stats, np.frombuffer(raw[0], np.uint64)[:n], np.frombuffer(raw[1], np.uint64)[:n], np.frombuffer(raw[2], np.uint8)[:n], untouched)


def check_plan(lib, h, st, rules, pad=0, first=0, n=None, what=None):
    a = st.a
    n = a.n_records - first if n is None else n
    err, stats, begin, end, keep, _ = plan_call(lib, h, st.cols_in(first, n), rules, n)
    assert err is None, (what, err)
    wb, we, wk, ws = plan_model(a, rules, first, n)
    bad = np.nonzero((begin != wb + np.uint64(pad)) | (end != we + np.uint64(pad)) | (keep != wk))[0]
    assert len(bad) == 0, (what, rules, "record", int(bad[0]), int(begin[bad[0]]) - pad, int(end[bad[0]]) - pad, int(keep[bad[0]]),
                           "want", int(wb[bad[0]]), int(we[bad[0]]), int(wk[bad[0]]))
    assert stats == ws, (what, rules, stats, ws)
    return wb, we, wk, ws


class SelCall:
    """One dsrcgpu_columns_select_device on output arrays this test owns (0xA5-filled, allocated for R / S / T entries; the
    capacities told to the library may be smaller)."""

    def __init__(self, lib, h, cin, d_begin, d_end, d_keep, R, S, T, titles=True, caps=None, source=True):
        caps = caps or {}
        with Dev(h) as d:
            sizes = {"bases": S, "quals": S, "titles": T, "seq_offs": 8 * (R + 1), "title_offs": 8 * (R + 1), "source": 8 * R}
            ptr = {k: d.fill(v) for k, v in sizes.items()}
            out = lib.Columns(ptr["bases"], caps.get("bases_cap", S), ptr["quals"], caps.get("quals_cap", S),
                              ptr["titles"] if titles else None, caps.get("titles_cap", T) if titles else 0,
                              ptr["seq_offs"], ptr["title_offs"] if titles else None, caps.get("records_cap", R))
            self.error = self.totals = None
            try:
                self.totals = h.columns_select_device(cin, d_begin, d_end, d_keep, out, ptr["source"] if source else None)
            except lib.DsrcGpuError as e:
                self.error = e
            self.raw = {k: d.down(ptr[k], v) for k, v in sizes.items()}

    def untouched(self, *names):
        return all(self.raw[k] == b"\xA5" * len(self.raw[k]) for k in (names or self.raw))

    def array(self, name, count, dtype=np.uint8):
        return np.frombuffer(self.raw[name], dtype=dtype)[:count]

    def assert_equals(self, want, titles=True, source=True, what=None):
        assert self.error is None, (what, self.error)
        wb, wq, wt, wso, wto, wsrc, wtot = want
        K, S, T = wtot
        assert self.totals == wtot, (what, self.totals, wtot)
        assert np.array_equal(self.array("bases", S), wb), what
        assert np.array_equal(self.array("quals", S), wq), what
        assert np.array_equal(self.array("seq_offs", K + 1, np.uint64), wso), what
        tail = lambda name, used: self.raw[name][used:] == b"\xA5" * (len(self.raw[name]) - used)
        assert tail("bases", S) and tail("quals", S) and tail("seq_offs", 8 * (K + 1)), what      # nothing behind what was kept
        if titles:
            assert np.array_equal(self.array("titles", T), wt), what
            assert np.array_equal(self.array("title_offs", K + 1, np.uint64), wto), what
            assert tail("titles", T) and tail("title_offs", 8 * (K + 1)), what
        else:
            assert self.untouched("titles", "title_offs"), what
        if source:
            assert np.array_equal(self.array("source", K, np.uint64), wsrc) and tail("source", 8 * K), what
        else:
            assert self.untouched("source"), what


def check_select(lib, h, st, begin=None, end=None, keep=None, pad=0, first=0, n=None, titles=True, what=None, with_titles_in=True):
    """Arrays staged in `st`, begin / end as positions in the UNPADDED arrays (the pad is added here) -> the call == the model."""
    a = st.a
    n = a.n_records - first if n is None else n
    want = select_model(a, begin, end, keep, titles, first, n)
    K, S, T = want[6]
    with Dev(h) as d:
        up = lambda v, dt, add=0: None if v is None else d.up((np.asarray(v).astype(dt) + dt(add)).tobytes())
        cin = st.cols_in(first, n)
        if not with_titles_in:
            cin = lib.ColumnsIn(cin.d_bases, cin.bases_len, cin.d_quals, None, 0, cin.d_seq_offs, None, n)
        call = SelCall(lib, h, cin, up(begin, np.uint64, pad), up(end, np.uint64, pad), up(keep, np.uint8), K, S, T, titles)
    call.assert_equals(want, titles, what=what)
    return want


# ---- trim plan: the cases --------------------------------------------------------------------------------------------------------
MODES = [("off", 0, 0), ("5'", 1, 0), ("3'", 0, 1), ("both", 1, 1)]


def run_plan_crafted(lib, sh, c):
    """Every read length and every crafted quality pattern at cutoff c, with both ends off, 5' only, 3' only and both."""
    names, a = crafted_arrays(c)
    h = ce.handle(lib, Config.from_levels(0, 0))
    try:
        with staged(lib, h, a) as st:
            for mode, on5, on3 in MODES:
                rules = rules_of(c * on5, c * on3, min_length=0)
                wb, we, wk, ws = check_plan(lib, h, st, rules, what=(c, mode))
                assert wk.all() and ws[0] == len(names)
    finally:
        h.close()


def run_plan_model_says(lib, sh):
    """The crafted reads really are what their names say -- decided by the serial model alone -- and the library agrees (c = 20)."""
    c = 20
    reads = crafted_reads(c)
    n_of = lambda name: len(reads[name])
    for L in LENGTHS:
        assert trim_range(reads["all at the cutoff %d" % L], c, c) == (0, L) == trim_range(reads["all above %d" % L], c, c)
        assert trim_range(reads["all below %d" % L], c, c) == (0, 0)
    # ties: the first position the sum reaches its maximum at, not a later one (the same maximum comes back at 3 and, a tile later, at 75)
    q = reads["tie 5'"]
    assert trim_ends(q, c, 0)[0] == 1 and sum(c - v for v in q[:3]) == 10 == sum(c - v for v in q[:75]) == c - q[0]
    assert trim_ends(reads["tie 3'"], 0, c)[1] == n_of("tie 3'") - 1
    # the break: an argmax over the whole read would cut far more
    q = reads["break 5'"]
    sums = np.cumsum([c - v for v in q])
    assert trim_ends(q, c, 0)[0] == 3 and int(np.argmax(sums)) + 1 > 50
    assert trim_ends(reads["break 3'"], 0, c)[1] == n_of("break 3'") - 3
    for B in (63, 64, 65):
        assert trim_ends(reads["break at %d 5'" % B], c, 0)[0] == B
        assert trim_ends(reads["break at %d 3'" % B], 0, c)[1] == n_of("break at %d 3'" % B) - B
    for name in ("crossing", "crossing long"):
        start, stop = trim_ends(reads[name], c, c)
        assert start >= stop and start > 0 and stop < n_of(name) and trim_range(reads[name], c, c) == (0, 0)
    run_plan_crafted(lib, sh, c)


def run_plan_refusals(lib, sh):
    a = fuzz_reads(0, 20)
    h = ce.handle(lib, Config.from_levels(0, 0))
    try:
        with staged(lib, h, a) as st:
            cin = st.cols_in()
            for rules, reserved in ((rules_of(256, 0), (0, 0, 0)), (rules_of(0, 256), (0, 0, 0)), (rules_of(20, 20), (0, 0, 1)), (rules_of(20, 20), (1, 0, 0))):
                err, _, _, _, _, untouched = plan_call(lib, h, cin, rules, a.n_records, reserved)
                assert err is not None and err.code == E_ARG and untouched, (rules, reserved)
            check_plan(lib, h, st, rules_of(255, 255, min_length=0))       # the largest cutoff is taken
            # titles are not read: none given
            cin = lib.ColumnsIn(cin.d_bases, cin.bases_len, cin.d_quals, None, 0, cin.d_seq_offs, None, a.n_records)
            err, stats, begin, end, keep, _ = plan_call(lib, h, cin, rules_of(20, 20), a.n_records)
            wb, we, wk, ws = plan_model(a, rules_of(20, 20))
            assert err is None and stats == ws and np.array_equal(begin, wb) and np.array_equal(end, we) and np.array_equal(keep, wk)
            # no records
            err, stats, _, _, _, untouched = plan_call(lib, h, st.cols_in(3, 0), rules_of(20, 20), 0)
            assert err is None and stats == [0] * 6 and untouched
    finally:
        h.close()
    hc = ce.handle(lib, dataclasses.replace(Config.from_levels(0, 0), color_space=True))
    try:
        with staged(lib, hc, a) as st:
            err, _, _, _, _, untouched = plan_call(lib, hc, st.cols_in(), rules_of(20, 20), a.n_records)
            assert err is not None and err.code == E_ARG and untouched
            call = SelCall(lib, hc, st.cols_in(), None, None, None, a.n_records, len(a.bases), len(a.titles))
            assert call.error is not None and call.error.code == E_ARG and call.untouched()
    finally:
        hc.close()


def run_plan_filters(lib, sh):
    """min_length, max_n and min_mean_quality at the exact figure and one off it; a record that fails two rules counts under the first."""
    rng = np.random.default_rng(5)
    quals = [[5] * 4 + [30] * 20 + [5] * 6,            # record 0: trimmed to its 20 good bases at cutoff 20
             [30] * 40, [30] * 7, [25, 35] * 10, [30] * 12]
    a = arrays_from_reads(quals, rng)
    S = [int(v) for v in a.seq_offsets]
    a.bases[:] = rng.integers(0, 4, len(a.bases))
    a.bases[S[0] + 4: S[0] + 9] = [4, 255, 5, 18, 11]  # record 0: five ambiguous bases inside the kept range ...
    a.bases[S[0]: S[0] + 4] = 4; a.bases[S[0] + 24: S[1]] = 255      # (... and only ambiguous ones outside it: they do not count)
    a.bases[S[2]: S[3]] = 4                             # record 2: 7 bases, all N
    h = ce.handle(lib, Config.from_levels(0, 0))
    try:
        with staged(lib, h, a) as st:
            base = dict(quality_5=20, quality_3=20)
            assert trim_range(quals[0], 20, 20) == (4, 24)
            for rules, keep0, stat in ((rules_of(**base, min_length=20), 1, 0), (rules_of(**base, min_length=21), 0, 3),
                                       (rules_of(**base, max_n=5), 1, 0), (rules_of(**base, max_n=4), 0, 4), (rules_of(**base, max_n=0), 0, 4),
                                       (rules_of(**base, max_n=None), 1, 0),
                                       (rules_of(**base, min_mean_quality=30), 1, 0), (rules_of(**base, min_mean_quality=31), 0, 5)):
                wb, we, wk, ws = check_plan(lib, h, st, rules, what=rules)
                assert wk[0] == keep0 and (stat == 0 or ws[stat] >= 1), rules
            # record 3 has sum == 30 * len exactly
            _, _, wk, _ = check_plan(lib, h, st, rules_of(min_mean_quality=30))
            assert wk[3] == 1
            _, _, wk, _ = check_plan(lib, h, st, rules_of(min_mean_quality=31))
            assert wk[3] == 0
            # record 2 is too short AND all N: counted once, under length
            _, _, wk, ws = check_plan(lib, h, st, rules_of(**base, min_length=8, max_n=3))
            assert wk[2] == 0 and ws[3] == 1 and ws[4] == 1      # (record 2 under length, record 0 under N)
            _, _, wk, ws = check_plan(lib, h, st, rules_of(**base, min_length=0, max_n=3, min_mean_quality=40))
            assert ws[4] == 2 and ws[5] == 3 and ws[0] == 0
    finally:
        h.close()


RULE_SETS = [rules_of(0, 20, min_length=30), rules_of(20, 20, min_length=1, max_n=2, min_mean_quality=22), rules_of(30, 10, min_length=50, max_n=0, min_mean_quality=0)]


def run_plan_fuzz(lib, sh, seed):
    a = fuzz_reads(seed, sh["sel_fuzz"][1])
    h = ce.handle(lib, Config.from_levels(0, 0))
    try:
        with staged(lib, h, a, pad=3) as st:
            for rules in RULE_SETS:
                _, _, _, ws = check_plan(lib, h, st, rules, pad=3, what=(seed, rules))
                assert 0 < ws[0] < a.n_records and ws[1] > 0      # (the model's figures: the rules bite, and not everywhere)
    finally:
        h.close()


def run_plan_offset_and_errors(lib, sh):
    """d_seq_offs + k, and d_seq_offs out of order / above bases_len in the first, a middle and the last record: DSRCGPU_E_INPUT with
    the record, outputs still 0xA5, the same handle plans the clean arrays afterwards."""
    a = fuzz_reads(3, 60)
    rules = RULE_SETS[1]
    pad = 4
    h = ce.handle(lib, Config.from_levels(0, 0))
    try:
        with staged(lib, h, a, pad=pad) as st:
            for first, n in ((7, None), (59, 1), (20, 11)):
                check_plan(lib, h, st, rules, pad=pad, first=first, n=n, what=("first", first))
            S = lambda r: int(a.seq_offsets[r]) + pad
            plants = [("order", lambda r: st.poke("seq_offs", r + 1, S(r) - 1, np.uint64), "not non-decreasing"),
                      ("end", lambda r: st.poke("seq_offs", r + 1, len(a.bases) + pad + 5, np.uint64), "above bases_len"),
                      ("wild", lambda r: st.poke("seq_offs", r + 1, 2 ** 64 - 1, np.uint64), "above bases_len")]
            checked = 0
            for name, plant, word in plants:
                for r in (0, 30, 59):
                    plant(r)
                    err, _, _, _, _, untouched = plan_call(lib, h, st.cols_in(), rules, a.n_records)
                    assert err is not None and err.code == E_INPUT and untouched, (name, r, err)
                    assert "record %d:" % r in str(err) and word in str(err), (name, r, str(err))
                    st.restore()
                    checked += 1
                check_plan(lib, h, st, rules, pad=pad, what=("after", name))
            assert checked == 9
    finally:
        h.close()


# ---- select: the cases -----------------------------------------------------------------------------------------------------------
def keep_patterns(n, rng):
    first = np.zeros(n, np.uint8); first[0] = 1
    last = np.zeros(n, np.uint8); last[-1] = 7                 # (any non-zero byte keeps)
    alt = (np.arange(n) % 2).astype(np.uint8) * 255
    return [("all (null)", None), ("all", np.ones(n, np.uint8)), ("none", np.zeros(n, np.uint8)), ("alternating", alt),
            ("first", first), ("last", last), ("random", (rng.random(n) < 0.5).astype(np.uint8))]


def run_select_patterns(lib, sh):
    """Keep patterns x (whole reads, planned ranges that include empty ones)."""
    a = fuzz_reads(1, 200)
    begin, end, _, _ = plan_model(a, RULE_SETS[1])
    assert (begin == end).any() and (begin < end).any()
    rng = np.random.default_rng(11)
    h = ce.handle(lib, Config.from_levels(0, 0))
    try:
        with staged(lib, h, a) as st:
            for name, keep in keep_patterns(a.n_records, rng):
                for b, e in ((None, None), (begin, end)):
                    want = check_select(lib, h, st, b, e, keep, what=(name, b is None))
                    if name == "none":
                        assert want[6] == [0, 0, 0] and list(want[3]) == [0]
    finally:
        h.close()


def run_select_count(lib, sh, n):
    a, begin, end, keep = tiny_records(n)
    h = ce.handle(lib, Config.from_levels(0, 0))
    try:
        with staged(lib, h, a) as st:
            check_select(lib, h, st, begin, end, keep, what=n)
            if n <= 2049:
                check_select(lib, h, st, None, None, None, what=(n, "all"))
    finally:
        h.close()


def run_select_titles(lib, sh):
    a = fuzz_reads(2, 150)
    begin, end, keep, _ = plan_model(a, RULE_SETS[0])
    h = ce.handle(lib, Config.from_levels(0, 0))
    try:
        with staged(lib, h, a) as st:
            check_select(lib, h, st, begin, end, keep, titles=False, what="titles not wanted")
            check_select(lib, h, st, begin, end, keep, titles=False, with_titles_in=False, what="titles not given")
            check_select(lib, h, st, None, None, None, titles=False, with_titles_in=False, what="titles not given, all")
            # d_source not wanted
            with Dev(h) as d:
                want = select_model(a, begin, end, keep)
                call = SelCall(lib, h, st.cols_in(), d.up(begin.tobytes()), d.up(end.tobytes()), d.up(keep.tobytes()), *want[6], source=False)
            call.assert_equals(want, source=False)
            # the host convenience
            got, src = h.select_columns(a, begin, end, keep, return_source=True)
            assert got.totals == want[6] and got.block_records == [0, want[6][0]] and np.array_equal(src, want[5])
            for g, w in zip((got.bases, got.quals, got.titles, got.seq_offsets, got.title_offsets), want[:5]):
                assert np.array_equal(g, w)
            got = h.select_columns(a, keep=keep, titles=False)
            want = select_model(a, None, None, keep, titles=False)
            assert got.titles is None and got.title_offsets is None and got.totals == want[6]
            assert np.array_equal(got.bases, want[0]) and np.array_equal(got.quals, want[1]) and np.array_equal(got.seq_offsets, want[3])
    finally:
        h.close()


def run_select_capacity(lib, sh):
    a = fuzz_reads(4, 120)
    begin, end, keep, _ = plan_model(a, RULE_SETS[1])
    want = select_model(a, begin, end, keep)
    K, S, T = want[6]
    assert 0 < K < a.n_records
    h = ce.handle(lib, Config.from_levels(0, 0))
    try:
        with staged(lib, h, a) as st, Dev(h) as d:
            args = (st.cols_in(), d.up(begin.tobytes()), d.up(end.tobytes()), d.up(keep.tobytes()), K, S, T)
            zero = dict(bases_cap=0, quals_cap=0, titles_cap=0, records_cap=0)
            for caps in (zero, {"bases_cap": S - 1}, {"quals_cap": S - 1}, {"titles_cap": T - 1}, {"records_cap": K - 1}):
                call = SelCall(lib, h, *args, caps=caps)
                assert call.error is not None and call.error.code == E_CAPACITY, caps
                assert call.error.need == [K, S, T] and call.untouched(), caps
            SelCall(lib, h, *args).assert_equals(want)          # the same handle, exact capacities
    finally:
        h.close()


def run_select_offset(lib, sh):
    """d_seq_offs + k and d_title_offs + k, n_records reduced; arrays with slack in front (offsets that do not start at 0)."""
    a = fuzz_reads(5, 90)
    begin, end, keep, _ = plan_model(a, RULE_SETS[1])
    h = ce.handle(lib, Config.from_levels(0, 0))
    try:
        with staged(lib, h, a, pad=5) as st:
            for first, n in ((0, 90), (13, 77), (40, 17), (89, 1)):
                sl = slice(first, first + n)
                check_select(lib, h, st, begin[sl], end[sl], keep[sl], pad=5, first=first, n=n, what=first)
                check_select(lib, h, st, None, None, keep[sl], pad=5, first=first, n=n, what=(first, "whole"))
            with Dev(h) as d:                                    # no records
                call = SelCall(lib, h, st.cols_in(9, 0), None, None, None, 0, 0, 0)
            assert call.error is None and call.totals == [0, 0, 0]
            assert call.raw["seq_offs"] == bytes(8) + b"\xA5" * 8 == call.raw["title_offs"] and call.untouched("bases", "quals", "titles", "source")
    finally:
        h.close()


def run_select_input_errors(lib, sh):
    """The five refusals (and the two of the title offsets) planted in the first, a middle and the last record, kept and dropped
    ones: code, record index, outputs intact, clean input afterwards on the same handle."""
    a = fuzz_reads(6, 41)
    begin, end, _, _ = plan_model(a, rules_of(10, 10, min_length=0))
    keep = np.ones(a.n_records, np.uint8); keep[20] = 0; keep[40] = 0      # the middle and the last record are dropped ones
    pad = 4
    want = select_model(a, begin, end, keep)
    K, S, T = want[6]
    h = ce.handle(lib, Config.from_levels(0, 0))
    checked = 0
    try:
        with staged(lib, h, a, pad=pad) as st, Dev(h) as d:
            hb, he = (begin + np.uint64(pad)), (end + np.uint64(pad))
            pb, pe, pk = d.up(hb.tobytes()), d.up(he.tobytes()), d.up(keep.tobytes())
            So = lambda r: int(a.seq_offsets[r]) + pad
            To = lambda r: int(a.title_offsets[r]) + pad
            put = lambda p, r, v: h.dev_upload(p + 8 * r, np.array([v], np.uint64).tobytes())
            plants = [("seq order", lambda r: st.poke("seq_offs", r + 1, So(r) - 1, np.uint64), "d_seq_offs is not non-decreasing"),
                      ("seq end", lambda r: st.poke("seq_offs", r + 1, len(a.bases) + pad + 5, np.uint64), "above bases_len"),
                      ("title order", lambda r: st.poke("title_offs", r + 1, To(r) - 1, np.uint64), "d_title_offs is not non-decreasing"),
                      ("title end", lambda r: st.poke("title_offs", r + 1, 2 ** 64 - 1, np.uint64), "above titles_len"),
                      ("begin low", lambda r: put(pb, r, So(r) - 1), "d_begin lies below"),
                      ("end high", lambda r: put(pe, r, So(r + 1) + 1), "d_end lies above"),
                      ("begin above end", lambda r: (put(pb, r, So(r + 1)), put(pe, r, So(r + 1) - 1)), "d_begin lies above d_end")]
            for name, plant, word in plants:
                for r in (0, 20, 40):
                    if name == "begin above end":
                        assert So(r + 1) > So(r)               # (needs a base)
                    plant(r)
                    call = SelCall(lib, h, st.cols_in(), pb, pe, pk, K, S, T)
                    assert call.error is not None and call.error.code == E_INPUT, (name, r, call.error)
                    assert "record %d:" % r in str(call.error) and word in str(call.error), (name, r, str(call.error))
                    assert call.untouched(), (name, r)
                    st.restore(); h.dev_upload(pb, hb.tobytes()); h.dev_upload(pe, he.tobytes())
                    checked += 1
                SelCall(lib, h, st.cols_in(), pb, pe, pk, K, S, T).assert_equals(want, what=("after", name))
    finally:
        h.close()
    assert checked == 21


# ---- the closed loop, the codec state, mates -------------------------------------------------------------------------------------
def _stage_blocks(blocks, device):
    offs, pos = [], 0
    for b in blocks:
        offs.append(pos); pos += (len(b) + 63) // 64 * 64
    buf = bytearray(pos)
    for b, o in zip(blocks, offs):
        buf[o: o + len(b)] = b
    return torch.frombuffer(buf, dtype=torch.uint8).to(device), offs


def filtered_text(texts, rules, quality_offset=33):
    """The chunk text of the model-filtered records of decoded chunk texts, and the model's stats."""
    out, stats = [], [0] * 6
    for text in texts:
        lines = text.split(b"\n")
        for r in range((len(lines) - 1) // 4):
            t, s, _, q = lines[4 * r: 4 * r + 4]
            one = Arrays(cc.LUT[np.frombuffer(s, np.uint8)], (np.frombuffer(q, np.uint8).astype(np.int64) - quality_offset).astype(np.uint8),
                         np.zeros(0, np.uint8), np.array([0, len(s)], np.uint64), np.zeros(2, np.uint64), [0, 1])
            b, e, k, st = plan_model(one, rules)
            stats = [x + y for x, y in zip(stats, st)]
            if k[0]:
                out.append(t + b"\n" + s[int(b[0]): int(e[0])] + b"\n+\n" + q[int(b[0]): int(e[0])])
    return b"\n".join(out), stats


def run_closed_loop(lib, sh, device):
    """Oracle blocks -> decode_columns -> filter_columns -> encode_columns == the oracle's block of the text of the model-filtered
    records: lossless -d3 -q2 with CRC, and lossy -d2 -q1 on the Ion-Torrent-like reads."""
    from dsrc_amd import columns
    cases = [(ce.BLOCK_CFG, None, rules_of(10, 35, min_length=70, max_n=0, min_mean_quality=33)),
             (Config.from_levels(2, 1, True), [cc.iontorrent_chunk(sh["ion_lossy"])], rules_of(5, 25, min_length=40, max_n=5, min_mean_quality=5))]
    for cfg, chunks, rules in cases:
        exp = cc.five_blocks(sh) if chunks is None else cc.expected(cfg, chunks)
        assert exp is not None
        text, stats = filtered_text(exp.texts, rules)
        print("closed loop", cfg.dna_order, cfg.quality_order, "model stats", stats, "of", exp.totals[0])
        assert 0 < stats[0] < exp.totals[0] and stats[2] > 0
        want = ce.oracle_blocks(cfg, [text])
        assert want is not None
        d_blocks, offs = _stage_blocks(exp.blocks, device)
        h = ce.handle(lib, cfg)
        try:
            rc = columns.decode_columns(h, d_blocks, offs, [len(b) for b in exp.blocks], device)
            sel, got_stats = columns.filter_columns(h, rc, **rules)
            assert list(got_stats.values()) == stats and list(got_stats) == list(lib.TRIM_STATS)
            assert sel.block_records.tolist() == [0, stats[0]] and sel.n_records == stats[0]
            h.set_fields_capacity(0)
            blocks, o_offs, o_sizes, br = columns.encode_columns(h, sel, block_records=sel.block_records)
            host = blocks.cpu().numpy().tobytes()
            assert [host[o: o + s] for o, s in zip(o_offs, o_sizes)] == [want[0][0]], cfg
        finally:
            h.close()


def run_codec_state(lib, sh):
    """Neither call touches what the codec carries: the fields capacity stays, a pending record layout stays pending, and the text
    call that follows writes what it writes on a fresh handle seeded alike."""
    a = fuzz_reads(7, 80)
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
                wb, we, wk, _ = check_plan(lib, h, st, RULE_SETS[1])
                assert h.get_fields_capacity() == 11
                check_select(lib, h, st, wb, we, wk)
                assert h.get_fields_capacity() == 11
            assert text_blocks(h) == text_blocks(fresh), layout
        finally:
            h.close(); fresh.close()


def run_mates(lib, sh, device):
    """Two files of mates: plan both, combine the masks, select both with the one mask -- the pairs stay in step."""
    from dsrc_amd import columns
    a1, a2 = fuzz_reads(8, 300), fuzz_reads(9, 300)
    rules = RULE_SETS[1]
    h = ce.handle(lib, Config.from_levels(0, 0))

    def tensors(a):
        t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v).astype(dt)).to(device)
        return columns.RecordColumns(t(a.bases, np.uint8), t(a.quals, np.uint8), t(a.titles, np.uint8), t(a.seq_offsets, np.int64),
                                     t(a.title_offsets, np.int64), torch.tensor([0, a.n_records]))
    try:
        c1, c2 = tensors(a1), tensors(a2)
        b1, e1, k1, s1 = columns.trim_plan(h, c1, **rules)
        b2, e2, k2, s2 = columns.trim_plan(h, c2, **rules)
        m1, m2 = plan_model(a1, rules), plan_model(a2, rules)
        assert list(s1.values()) == m1[3] and list(s2.values()) == m2[3]
        assert b1.dtype == torch.int64 and k1.dtype == torch.uint8 and k1.device.type == torch.device(device).type
        keep = k1 & k2
        wk = m1[2] & m2[2]
        assert np.array_equal(keep.cpu().numpy(), wk) and 0 < wk.sum() < min(m1[2].sum(), m2[2].sum())
        o1, src1 = columns.select_columns(h, c1, b1, e1, keep, return_source=True)
        o2, src2 = columns.select_columns(h, c2, b2, e2, keep, return_source=True)
        assert torch.equal(src1, src2) and np.array_equal(src1.cpu().numpy().astype(np.uint64), np.nonzero(wk)[0].astype(np.uint64))
        for o, a, m in ((o1, a1, m1), (o2, a2, m2)):
            want = select_model(a, m[0], m[1], wk)
            for g, w in zip((o.bases, o.quals, o.titles, o.seq_offsets, o.title_offsets), want[:5]):
                assert np.array_equal(g.cpu().numpy().astype(w.dtype), w)
            assert o.block_records.tolist() == [0, int(wk.sum())]
        # titles=False through the wrapper, whole reads
        o = columns.select_columns(h, c1, keep=keep, titles=False)
        want = select_model(a1, None, None, wk, titles=False)
        assert o.titles.numel() == 0 and o.title_offsets.numel() == 0 and np.array_equal(o.bases.cpu().numpy(), want[0])
    finally:
        h.close()
