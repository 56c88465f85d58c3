"""Shared by tests/test_emu_columns_dedup.py (CPU, emulator build) and tests/test_gpu_columns_dedup.py (MI355X): the cases of the
columnar dedup plan (dsrcgpu_columns_dedup_plan; dsrc_amd/csrc/k_columns_dedup.h) and what they must give.

The reference has no counterpart, so the yardstick is the integer model written out here: dedup_model() is the serial rule of
include/dsrc_gpu.h with a Python dict keyed on the tuple (k_1, bytes, k_2, bytes).  None of it comes from the library under test, and
every comparison is exact equality of keep, dup_of, copies and all 24 statistics.  Output arrays are filled with 0xA5 before a call,
so that "nothing written" and "not a byte beyond" can be asserted.  Before the library is compared on a crafted case the model alone
is asked what that case is for.

Shapes.  The emulator pays a coroutine switch per wave exchange, so its fuzz is 2 seeds x 150 records where the GPU runs 6 x 2000.
The wave-per-record grid holds at most 4096 workgroups of WG / 64 waves: with workgroups of 1024 threads 4096 * 16 + 1001 records
take the grid stride into a second round -- that count, and the contention batch of 20 000 records of three sequences, run on the
GPU only.  hash_bits below 64 makes every probe chain long, so that batch stays below 300 records on either build."""
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
NONE = 2 ** 64 - 1
GRID_CAP = 4096                  # workgroups of the wave-per-record launches

SHAPES = {
    "gpu": dict(cc.SHAPES["gpu"], dedup_fuzz=(6, 2000), counts=[1, 63, 64, 65, 2049], stride_count=GRID_CAP * 16 + 1001, contention=20000),
    "emu": dict(cc.SHAPES["emu"], dedup_fuzz=(2, 150), counts=[1, 63, 64, 65, 2049], stride_count=None, contention=None),
}
Arrays = ce.Arrays
Dev = cs.Dev
staged = cp.staged
handle = cp.handle
tensors = ca.tensors
DEDUP_STATS = ("records_considered", "records_kept", "records_dropped", "classes_multiple", "largest_class", "came_in_dropped", "empty_keys",
               "representative_not_first", "level_1", "level_2", "level_3", "level_4", "level_5", "level_6", "level_7", "level_8", "level_9",
               "level_10_49", "level_50_99", "level_100_499", "level_500_999", "level_1000_4999", "level_5000_9999", "level_10000_up")
BIN_FLOORS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 50, 100, 500, 1000, 5000, 10000]


def arrays_of_reads(reads, quals=None):
    """Reads given by their base codes and, if wanted, their qualities (30 throughout otherwise); titles @r<i>."""
    a = ca.arrays_from_bases(reads)
    if quals is not None:
        a.quals = np.concatenate([np.asarray(q, np.uint8) for q in quals] + [np.zeros(0, np.uint8)]).astype(np.uint8)
        assert len(a.quals) == len(a.bases)
    return a


# ---- the model -------------------------------------------------------------------------------------------------------------------
def bin_of(size):
    return max(i for i, floor in enumerate(BIN_FLOORS) if size >= floor)


def dedup_model(a1: Arrays, a2=None, r1=(None, None), r2=(None, None), keep=None, key_bases=0, prefer=0, first=0, n=None):
    """The serial rule on records first .. first + n - 1 (ranges as positions in a<s>.bases, one entry per record of the call)
    -> keep (uint8), dup_of (uint64), copies (uint64), stats[24]; indices count from `first`."""
    n = a1.n_records - first if n is None else n
    sides = [(a1, r1)] + ([(a2, r2)] if a2 is not None else [])
    out_keep, dup_of, copies, stats = np.zeros(n, np.uint8), np.full(n, NONE, np.uint64), np.zeros(n, np.uint64), [0] * 24
    classes, rank = {}, {}
    for k in range(n):
        r = first + k
        if keep is not None and keep[k] == 0:
            stats[5] += 1
            continue
        stats[0] += 1
        key, q = [], 0
        for a, (begin, end) in sides:
            S = a.seq_offsets
            b, e = (int(S[r]), int(S[r + 1])) if begin is None else (int(begin[k]), int(end[k]))
            assert int(S[r]) <= b <= e <= int(S[r + 1])
            ks = min(e - b, key_bases) if key_bases else e - b
            key += [ks, a.bases[b: b + ks].tobytes()]
            q += int(a.quals[b: b + ks].astype(np.int64).sum())
        if sum(key[0::2]) == 0:
            stats[6] += 1
        rank[k] = (min(q, 2 ** 32 - 1) if prefer else 0, -k)
        classes.setdefault(tuple(key), []).append(k)
    for members in classes.values():
        rep = max(members, key=rank.get)
        out_keep[rep] = 1; copies[rep] = len(members)
        dup_of[members] = rep
        stats[1] += 1; stats[2] += len(members) - 1
        stats[3] += len(members) >= 2
        stats[4] = max(stats[4], len(members))
        stats[7] += rep != min(members)
        stats[8 + bin_of(len(members))] += 1
    assert stats[0] == stats[1] + stats[2] and sum(stats[8:]) == stats[1] and (prefer or stats[7] == 0)
    return out_keep, dup_of, copies, stats


# ---- one call ----------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Got:
    error: object
    stats: object
    keep: np.ndarray
    dup_of: np.ndarray
    copies: np.ndarray
    untouched: bool
    keep_in_after: object = None


def lib_rules(lib, key_bases=0, prefer=0, hash_bits=0, reserved=(0, 0, 0, 0, 0)):
    return lib.DedupRules(key_bases, prefer, hash_bits, reserved)


def dedup_call(lib, h, cin1, cin2, n, dr, r1=(None, None), r2=(None, None), keep=None, inplace=False, null_out=None):
    """One dsrcgpu_columns_dedup_plan.  r<s>: begin / end as numpy in the coordinates of the staged arrays, or None; keep: numpy or None.
    Outputs are 0xA5-filled; inplace: d_keep IS the incoming keep; null_out: "keep", "dup_of" or "copies" is passed as NULL."""
    with Dev(h) as d:
        up = lambda v, dt: None if v is None else d.up(np.ascontiguousarray(v).astype(dt).tobytes())
        p1, p2 = [up(v, np.uint64) for v in r1], [up(v, np.uint64) for v in r2]
        pk = up(keep, np.uint8)
        fresh = [d.fill(n), d.fill(8 * n), d.fill(8 * n)]
        sizes = (n, 8 * n, 8 * n)
        assert not inplace or pk is not None
        out = [pk if inplace else fresh[0], fresh[1], fresh[2]]
        arg = [None if name == null_out else p for name, p in zip(("keep", "dup_of", "copies"), out)]
        err = stats = None
        try:
            stats = h.columns_dedup_plan(cin1, cin2, dr, tuple(p1), tuple(p2), pk, arg[0], arg[1], arg[2])
        except lib.DsrcGpuError as e:
            err = e
        raw = [d.down(p, s) for p, s in zip(out, sizes)]
        raw_fresh = [d.down(p, s) for p, s in zip(fresh, sizes)]
        keep_after = None if pk is None else d.down(pk, n)[:n]
    assert all(r[-8:] == b"\xA5" * 8 for r in raw + raw_fresh), "written behind the end of an output array"
    if inplace:
        assert raw_fresh[0] == b"\xA5" * len(raw_fresh[0]), "an output that was not given has been written"
    for i, name in enumerate(("keep", "dup_of", "copies")):
        if name == null_out:
            assert raw_fresh[i] == b"\xA5" * len(raw_fresh[i]), "%s was not given" % name
    return Got(err, stats, np.frombuffer(raw[0], np.uint8)[:n], np.frombuffer(raw[1], np.uint64)[:n], np.frombuffer(raw[2], np.uint64)[:n],
               all(r == b"\xA5" * len(r) for r in raw_fresh), keep_after)


def check_dedup(lib, h, st1, st2=None, r1=(None, None), r2=(None, None), keep=None, key_bases=0, prefer=0, hash_bits=0, pad=(0, 0), first=0, n=None,
                what=None, model=None, **how):
    """Arrays staged in st1 / st2, the ranges as positions in the UNPADDED arrays (the pads are added here) -> the call == the model."""
    n = st1.a.n_records - first if n is None else n
    m = model if model is not None else dedup_model(st1.a, st2.a if st2 is not None else None, r1, r2, keep, key_bases, prefer, first, n)
    shift = lambda rr, p: tuple(None if v is None else np.asarray(v).astype(np.uint64) + np.uint64(p) for v in rr)
    got = dedup_call(lib, h, st1.cols_in(first, n), st2.cols_in(first, n) if st2 is not None else None, n, lib_rules(lib, key_bases, prefer, hash_bits),
                     shift(r1, pad[0]), shift(r2, pad[1]), keep, **how)
    assert got.error is None, (what, got.error)
    null = how.get("null_out")
    bad = np.zeros(n, bool)
    for name, g, w in (("keep", got.keep, m[0]), ("dup_of", got.dup_of, m[1]), ("copies", got.copies, m[2])):
        if name != null:
            bad |= g != w
    bad = np.nonzero(bad)[0]
    if len(bad):
        r = int(bad[0])
        raise AssertionError((what, "record", r, int(got.keep[r]), int(got.dup_of[r]), int(got.copies[r]), "want", int(m[0][r]), int(m[1][r]), int(m[2][r]),
                              len(bad)))
    assert got.stats == m[3], (what, got.stats, m[3])
    if how.get("inplace"):
        assert got.keep_in_after == got.keep.tobytes()
    elif keep is not None:
        assert got.keep_in_after == np.asarray(keep, np.uint8).tobytes(), "the incoming keep has been written"
    return m


def whole(a):
    S = a.seq_offsets.astype(np.int64)
    return S[:-1].copy(), S[1:].copy()


# ---- geometry --------------------------------------------------------------------------------------------------------------------
LENGTHS = [1, 15, 16, 17, 63, 64, 65, 1025]


def geometry_reads(rng):
    """Per length L: a read, its exact copy, a copy that differs in the last base only, a copy with code 4 and one with code 255 in the
    middle (each twice), and -- built from ONE sequence, so that each is a prefix of the next longer one -- nothing else.  Between them
    five empty reads.  -> reads, what[r] = (L, kind)"""
    master = rng.integers(0, 4, 1025).astype(np.uint8)
    reads, what = [], []

    def add(x, L, kind):
        reads.append(np.asarray(x, np.uint8)); what.append((L, kind))
    for L in LENGTHS:
        x = master[:L].copy()
        add(x, L, "first"); add(np.zeros(0, np.uint8), 0, "empty"); add(x, L, "copy")
        y = x.copy(); y[-1] = (y[-1] + 1) % 4
        add(y, L, "last base")
        for code in (4, 255):
            z = x.copy(); z[L // 2] = code
            add(z, L, "code %d" % code); add(z, L, "code %d again" % code)
    return reads, what


def run_geometry(lib, sh):
    rng = np.random.default_rng(100)
    reads, what = geometry_reads(rng)
    a = arrays_of_reads(reads)
    m = dedup_model(a)
    idx = lambda L, kind: what.index((L, kind))
    empties = [r for r, w in enumerate(what) if w[1] == "empty"]
    assert len(empties) == 8 and int(m[2][empties[0]]) == 8 and all(int(m[1][r]) == empties[0] for r in empties) and m[3][6] == 8
    for L in LENGTHS:
        assert int(m[1][idx(L, "copy")]) == idx(L, "first") and int(m[2][idx(L, "first")]) == 2                   # the exact copy, and nothing else
        assert int(m[0][idx(L, "last base")]) == 1 and int(m[2][idx(L, "last base")]) == 1                       # equal but for the last base
        for code in (4, 255):                                                                                     # a code equals itself
            assert int(m[1][idx(L, "code %d again" % code)]) == idx(L, "code %d" % code) and int(m[0][idx(L, "code %d" % code)]) == 1
    assert reads[idx(16, "first")].tobytes() == reads[idx(17, "first")][:16].tobytes() and int(m[0][idx(17, "first")]) == 1      # a prefix is no duplicate
    starts = {(int(a.seq_offsets[r]) + pad) % 16 for pad in (0, 1, 7) for r, w in enumerate(what) if w[0] >= 63}
    assert len(starts) >= 12, starts                          # the 16-byte path meets heads and tails of most sizes
    S0, S1 = whole(a)
    lens = S1 - S0
    cut5 = np.zeros(len(reads), np.int64)                     # ranges that begin at odd offsets: 1 .. 3 bases cut off, the same cut
    for r, w in enumerate(what):                              # for the members of a class, or they are no duplicates
        cut5[r] = min(w[0], 1 + LENGTHS.index(w[0]) % 3) if w[0] else 0
    assert (cut5 <= lens).all()
    rr = (S0 + cut5, S1)
    mr = dedup_model(a, r1=rr)
    assert int(mr[1][idx(65, "copy")]) == idx(65, "first") and mr[3][6] >= 8 + 5      # (the reads of one base have become empty)
    h = handle(lib)
    try:
        for pad in (0, 1, 7):
            with staged(lib, h, a, pad=pad) as st:
                check_dedup(lib, h, st, pad=(pad, 0), what=("geometry", pad), model=m)
                check_dedup(lib, h, st, r1=rr, pad=(pad, 0), what=("geometry, ranges", pad), model=mr)
                check_dedup(lib, h, st, r1=rr, prefer=1, pad=(pad, 0), what=("geometry, ranges, quality", pad))
    finally:
        h.close()


# ---- key_bases ---------------------------------------------------------------------------------------------------------------------
def run_key_bases(lib, sh):
    rng = np.random.default_rng(200)
    L = 40
    x = rng.integers(0, 4, L).astype(np.uint8)
    last = x.copy(); last[-1] ^= 1                           # differs at position L - 1 only
    first = x.copy(); first[0] ^= 1                          # differs at position 0 only
    longer = np.concatenate((x, [2]))                        # L + 1 bases, x in front
    short = x[:10].copy()                                    # a prefix of x, shorter than key_bases = 20
    tail = np.concatenate((x[:20], rng.integers(0, 4, 25))).astype(np.uint8)      # 45 bases, x's first 20 in front
    reads = [x, last, first, longer, short, tail, short.copy(), x.copy()]
    a = arrays_of_reads(reads)
    want = {1: [[0, 1, 3, 4, 5, 6, 7], [2]],                  # the first base alone: everything but `first`
            L - 1: [[0, 1, 3, 7], [2], [4, 6], [5]],          # `last` differs only behind the key; `longer` is cut to the same 39
            L: [[0, 3, 7], [1], [2], [4, 6], [5]],            # `longer`'s first 40 bases are x
            L + 1: [[0, 7], [1], [2], [3], [4, 6], [5]],      # `longer` keeps its 41: a read is no duplicate of its prefix
            20: [[0, 1, 3, 5, 7], [2], [4, 6]],               # short (10 < 20) stays apart from the longer reads with its prefix
            0: [[0, 7], [1], [2], [3], [4, 6], [5]]}
    models = {}
    for kb, classes in want.items():
        m = dedup_model(a, key_bases=kb)
        got = sorted(sorted(int(r) for r in np.nonzero(m[1] == rep)[0]) for rep in np.nonzero(m[0])[0])
        assert got == sorted(classes), (kb, got)
        models[kb] = m
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=3) as st:
            for kb, m in models.items():
                check_dedup(lib, h, st, key_bases=kb, pad=(3, 0), what=("key_bases", kb), model=m)
            check_dedup(lib, h, st, key_bases=0xFFFFFFFF, pad=(3, 0), what="the largest key_bases", model=models[0])
    finally:
        h.close()


# ---- prefer ------------------------------------------------------------------------------------------------------------------------
def run_prefer(lib, sh):
    rng = np.random.default_rng(300)
    x, y, z, w = (rng.integers(0, 4, 30).astype(np.uint8) for _ in range(4))
    q = lambda v, n=30: np.full(n, v, np.uint8)
    hot_tail = np.concatenate((q(10, 10), q(255, 20)))       # poor where key_bases = 10 looks, excellent behind
    reads = [x, y, x, z, x, y, z, w, z]
    quals = [q(20), q(30), q(35), q(25), q(35), q(30), hot_tail, q(2), q(25)]
    #        x: 2 wins (35, tie with 4: the lower index)     y: a tie, 1 wins     z: 3 / 6 / 8     w: alone
    a = arrays_of_reads(reads, quals)
    mf, mq, mk = dedup_model(a), dedup_model(a, prefer=1), dedup_model(a, prefer=1, key_bases=10)
    assert mf[0].tolist() == [1, 1, 0, 1, 0, 0, 0, 1, 0] and mf[3][7] == 0
    assert mq[0].tolist() == [0, 1, 1, 0, 0, 0, 1, 1, 0] and mq[3][7] == 2 and mq[1].tolist() == [2, 1, 2, 6, 2, 1, 6, 7, 6]      # z: the hot tail counts
    assert mk[0].tolist() == [0, 1, 1, 1, 0, 0, 0, 1, 0] and mk[3][7] == 1      # ... and does not where the key ends at 10: 3 (250) beats 6 (100)
    assert mq[2].tolist() == [0, 2, 3, 0, 0, 0, 3, 1, 0] and mq[3][3] == 3 and mq[3][4] == 3
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=1) as st:
            check_dedup(lib, h, st, pad=(1, 0), what="first", model=mf)
            check_dedup(lib, h, st, prefer=1, pad=(1, 0), what="quality", model=mq)
            check_dedup(lib, h, st, prefer=1, key_bases=10, pad=(1, 0), what="quality, key 10", model=mk)
            check_dedup(lib, h, st, st, prefer=1, pad=(1, 1), what="quality, both sides the same arrays")
            # under prefer = 0 the qualities are not read
            n = a.n_records
            bare = lib.ColumnsIn(st.cols_in().d_bases, st.cols_in().bases_len, None, None, 0, st.cols_in().d_seq_offs, None, n)
            got = dedup_call(lib, h, bare, None, n, lib_rules(lib))
            assert got.error is None and got.stats == mf[3] and np.array_equal(got.keep, mf[0]) and np.array_equal(got.dup_of, mf[1])
            got = dedup_call(lib, h, bare, None, n, lib_rules(lib, prefer=1))
            assert got.error is not None and got.error.code == E_ARG and got.untouched
    finally:
        h.close()


# ---- plans in ------------------------------------------------------------------------------------------------------------------------
def run_plans_in(lib, sh):
    rng = np.random.default_rng(400)
    core = rng.integers(0, 4, 50).astype(np.uint8)
    flank = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    f5 = [3, 0, 7, 1]
    reads = [np.concatenate((flank(f), core, flank(4))) for f in f5]          # 0 .. 3: different reads, one core
    reads += [core.copy(), core.copy(), core.copy()]                            # 4 .. 6: equal reads
    twin = rng.integers(0, 4, 33).astype(np.uint8)
    reads += [twin, twin.copy(), twin.copy(), twin.copy()]                       # 7 .. 10: dropped / kept / dropped / kept
    a = arrays_of_reads(reads, [rng.integers(2, 41, len(x)) for x in reads])
    n = a.n_records
    S0, S1 = whole(a)
    b, e = S0.copy(), S1.copy()
    for r, f in enumerate(f5):
        b[r] += f; e[r] -= 4                                   # the ranges are the core
    e[5] -= 1; b[6] += 1                                       # equal reads, different ranges
    keep = np.array([1, 7, 255, 1, 1, 1, 1, 0, 1, 0, 9], np.uint8)
    mw, mr, mk = dedup_model(a), dedup_model(a, r1=(b, e)), dedup_model(a, r1=(b, e), keep=keep)
    assert mw[0][:7].tolist() == [1, 1, 1, 1, 1, 0, 0]
    assert mr[1][:7].tolist() == [0, 0, 0, 0, 0, 5, 6] and int(mr[2][0]) == 5      # ranges make different reads equal and equal reads different
    assert mk[0][7:].tolist() == [0, 1, 0, 0] and mk[1][7:].tolist() == [NONE, 8, NONE, 8] and int(mk[2][8]) == 2 and mk[3][5] == 2
    h = handle(lib)
    try:
        for pad in (0, 5):
            with staged(lib, h, a, pad=pad) as st:
                kw = dict(pad=(pad, 0))
                check_dedup(lib, h, st, what="whole", model=mw, **kw)
                check_dedup(lib, h, st, r1=(b, e), what="ranges", model=mr, **kw)
                check_dedup(lib, h, st, r1=(b, e), keep=keep, what="ranges, keep", model=mk, **kw)
                check_dedup(lib, h, st, r1=(b, e), keep=keep, what="in place", model=mk, inplace=True, **kw)
                check_dedup(lib, h, st, r1=(b, e), keep=keep, prefer=1, what="in place, quality", inplace=True, **kw)
                check_dedup(lib, h, st, keep=keep, what="keep alone", **kw)
                for null in ("dup_of", "copies"):
                    check_dedup(lib, h, st, r1=(b, e), keep=keep, what=("null", null), model=mk, null_out=null, **kw)
                    check_dedup(lib, h, st, r1=(b, e), keep=keep, what=("null, in place", null), model=mk, null_out=null, inplace=True, **kw)
                for first, cnt in ((2, None), (n - 1, 1), (3, 6)):       # d_seq_offs + k: indices count from the call's first record
                    sl = slice(first, None if cnt is None else first + cnt)
                    check_dedup(lib, h, st, r1=(b[sl], e[sl]), keep=keep[sl], first=first, n=cnt, what=("first", first), **kw)
                    check_dedup(lib, h, st, first=first, n=cnt, what=("first, whole", first), **kw)
                check_dedup(lib, h, st, keep=np.zeros(n, np.uint8), what="nothing considered", **kw)
    finally:
        h.close()


# ---- pairs -------------------------------------------------------------------------------------------------------------------------
def run_pairs(lib, sh):
    rng = np.random.default_rng(500)
    A, B, C_, D = (rng.integers(0, 4, k).astype(np.uint8) for k in (40, 40, 35, 35))
    AC, G, A1, CG = np.array([0, 1], np.uint8), np.array([2], np.uint8), np.array([0], np.uint8), np.array([1, 2], np.uint8)
    E = np.zeros(0, np.uint8)
    #         0      1      2      3      4      5      6      7      8      9
    reads1 = [A,     A,     A,     B,     AC,    A1,    E,     E,     AC,    A]
    reads2 = [C_,    D,     C_,    C_,    G,     CG,    G,     E,     G,     C_]
    a1, a2 = arrays_of_reads(reads1, [rng.integers(2, 41, len(x)) for x in reads1]), arrays_of_reads(reads2, [rng.integers(2, 41, len(x)) for x in reads2])
    m = dedup_model(a1, a2)
    assert m[1].tolist() == [0, 1, 0, 3, 4, 5, 6, 7, 4, 0]      # mate 1 equal, mate 2 different: apart; both equal: together; AC|G is not A|CG
    assert m[3][6] == 1                                       # one pair with no base on either side
    m1 = dedup_model(a1)
    assert m1[1].tolist() == [0, 0, 0, 3, 4, 5, 6, 6, 4, 0]    # ... which read 1 alone would not tell
    S10, S11 = whole(a1); S20, S21 = whole(a2)
    e1 = S11.copy(); e1[[0, 1, 2, 9]] -= 3
    b2 = S20.copy(); b2[[0, 2, 3]] += 2; b2[9] += 1
    mr = dedup_model(a1, a2, (S10, e1), (b2, S21))
    assert mr[1].tolist() == [0, 1, 0, 3, 4, 5, 6, 7, 4, 9]
    keep = np.array([0, 1, 1, 1, 1, 1, 1, 1, 0, 1], np.uint8)
    h = handle(lib)
    try:
        for pad in ((0, 0), (3, 6)):
            with staged(lib, h, a1, pad=pad[0]) as st1, staged(lib, h, a2, pad=pad[1]) as st2:
                check_dedup(lib, h, st1, st2, pad=pad, what="pairs", model=m)
                check_dedup(lib, h, st1, pad=pad, what="read 1 alone", model=m1)
                check_dedup(lib, h, st1, st2, (S10, e1), (b2, S21), pad=pad, what="pairs, ranges", model=mr)
                check_dedup(lib, h, st1, st2, (S10, e1), pad=pad, what="pairs, ranges of side 1 only")
                check_dedup(lib, h, st1, st2, r2=(b2, S21), pad=pad, what="pairs, ranges of side 2 only")
                check_dedup(lib, h, st1, st2, (S10, e1), (b2, S21), keep, prefer=1, key_bases=30, pad=pad, what="pairs, everything", inplace=True)
                check_dedup(lib, h, st2, st1, pad=pad[::-1], what="sides swapped")
    finally:
        h.close()


# ---- records for the larger batches -------------------------------------------------------------------------------------------------
def pool_batch(rng, n, pool, lo=8, hi=20, keep_share=1.0, pairs=False):
    """n records drawn from `pool` sequences of lo .. hi bases (codes 0 .. 4), random qualities -> arrays (two with pairs: the mate is
    drawn from the pool on its own), keep (or None), pick"""
    seqs = [rng.integers(0, 5, int(rng.integers(lo, hi + 1))).astype(np.uint8) for _ in range(pool)]
    sides = []
    for _ in range(2 if pairs else 1):
        pick = rng.integers(0, pool, n)
        reads = [seqs[i] for i in pick]
        a = ca.arrays_from_bases(reads)
        a.quals = rng.integers(0, 42, len(a.bases)).astype(np.uint8)
        sides.append(a)
    keep = None if keep_share >= 1.0 else (rng.random(n) < keep_share).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
    return sides, keep


def run_hash_bits(lib, sh):
    """One batch, many classes; hash_bits 1, 2 and 4 send every key down the same few probe chains, where equal (cut) hashes meet
    different keys: outputs and statistics are those of the full hash."""
    rng = np.random.default_rng(600)
    (a,), keep = pool_batch(rng, 280, 90, keep_share=0.9)
    m, mq = dedup_model(a, keep=keep), dedup_model(a, keep=keep, prefer=1, key_bases=12)
    assert m[3][1] >= 60 and m[3][3] >= 40 and mq[3][7] >= 10, (m[3], mq[3])
    (p1, p2), _ = pool_batch(rng, 200, 12, pairs=True)
    mp = dedup_model(p1, p2)
    assert 60 <= mp[3][1] <= 144 and mp[3][3] >= 20
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=2) as st, staged(lib, h, p1) as s1, staged(lib, h, p2, pad=9) as s2:
            for bits in (1, 2, 4, 64):
                check_dedup(lib, h, st, keep=keep, hash_bits=bits, pad=(2, 0), what=("hash_bits", bits), model=m)
                check_dedup(lib, h, st, keep=keep, prefer=1, key_bases=12, hash_bits=bits, pad=(2, 0), what=("hash_bits, quality", bits), model=mq)
                check_dedup(lib, h, s1, s2, hash_bits=bits, pad=(0, 9), what=("hash_bits, pairs", bits), model=mp)
            check_dedup(lib, h, st, keep=keep, hash_bits=0, pad=(2, 0), what="hash_bits 0", model=m)
            check_dedup(lib, h, st, keep=keep, hash_bits=63, pad=(2, 0), what="hash_bits 63", model=m)
    finally:
        h.close()


def run_count(lib, sh, n_records):
    """n records of 8 .. 20 bases from a pool: 64 records fill a table of exactly 2 * 64 slots, 65 take the next power of two."""
    rng = np.random.default_rng(700 + n_records)
    (a,), keep = pool_batch(rng, n_records, max(1, n_records // 3), keep_share=0.9)
    m = dedup_model(a, keep=keep, prefer=1)
    if n_records >= 2049:
        assert m[3][3] > 100 and m[3][7] > 50 and m[3][5] > 100
    h = handle(lib)
    try:
        with staged(lib, h, a) as st:
            check_dedup(lib, h, st, keep=keep, prefer=1, what=n_records, model=m)
            check_dedup(lib, h, st, keep=keep, what=(n_records, "first, in place"), inplace=True)
            check_dedup(lib, h, st, what=(n_records, "every record"))
    finally:
        h.close()


def run_contention(lib, sh):
    """Every record hits one of three slots.  Run twice: the order in which the waves arrive changes nothing."""
    n = sh["contention"]
    rng = np.random.default_rng(800)
    (a,), _ = pool_batch(rng, n, 3)
    h = handle(lib)
    try:
        with staged(lib, h, a) as st:
            for prefer in (0, 1):
                m = dedup_model(a, prefer=prefer)
                assert m[3][1] == 3 and m[3][4] > n // 4 and sum(m[3][8:]) == 3 and m[3][8 + 14] + m[3][8 + 15] == 3, m[3]
                rounds = []
                for k in range(2):
                    check_dedup(lib, h, st, prefer=prefer, what=("contention", prefer, k), model=m)
                    got = dedup_call(lib, h, st.cols_in(), None, n, lib_rules(lib, 0, prefer))
                    rounds.append((got.stats, got.keep.tobytes(), got.dup_of.tobytes(), got.copies.tobytes()))
                assert rounds[0] == rounds[1]
    finally:
        h.close()


def run_grid_stride(lib, sh):
    n = sh["stride_count"]
    rng = np.random.default_rng(900)
    (a,), keep = pool_batch(rng, n, 500, keep_share=0.95)
    m = dedup_model(a, keep=keep)
    assert m[3][1] == 500 and m[3][8 + 10] + m[3][8 + 11] == 500 and m[3][8 + 11] > 400      # 500 classes of about 126 members
    h = handle(lib)
    try:
        with staged(lib, h, a) as st:
            check_dedup(lib, h, st, keep=keep, what="grid stride", model=m)
    finally:
        h.close()


# ---- fuzz ------------------------------------------------------------------------------------------------------------------------
def fuzz_batch(seed, n):
    """n records, each a copy of one of ~n / 7 pool reads of 0 .. 160 bases (pairs: of one pool pair) with a mutation (one base changed,
    dropped at the end or added, on one side) at probability 1/2, random ranges that cut up to 3 bases off some ends, a random keep; pairs on odd seeds."""
    rng = np.random.default_rng(4000 + seed)
    pairs = seed % 2 == 1
    pool = max(2, n // 7)
    other = np.array([4, 4, 255, 7], np.uint8)
    sides, ranges = [], []
    pick = rng.integers(0, pool, n)
    how, where = rng.random(n), rng.integers(0, 2 if pairs else 1, n)      # the mutation of a record, and the side it hits
    for s in range(2 if pairs else 1):
        seqs = []
        for _ in range(pool):
            x = rng.integers(0, 4, int(rng.integers(0, 161))).astype(np.uint8)
            amb = rng.random(len(x)) < 0.01
            x[amb] = other[rng.integers(0, 4, int(amb.sum()))]
            seqs.append(x)
        reads = []
        for r in range(n):
            x = seqs[pick[r]].copy()
            u = how[r] if where[r] == s else 1.0
            if u < 0.25 and len(x):
                x[int(rng.integers(0, len(x)))] ^= 1
            elif u < 0.375 and len(x):
                x = x[:-1]
            elif u < 0.5:
                x = np.concatenate((x, [rng.integers(0, 4)])).astype(np.uint8)
            reads.append(x)
        a = ca.arrays_from_bases(reads)
        a.quals = rng.integers(0, 42, len(a.bases)).astype(np.uint8)
        S0, S1 = whole(a)
        lens = S1 - S0
        if rng.random() < 0.7:
            cut5 = np.where(rng.random(n) < 0.85, 0, rng.integers(0, 4, n)); cut5 = np.minimum(cut5, lens)
            cut3 = np.minimum(np.where(rng.random(n) < 0.85, 0, rng.integers(0, 4, n)), lens - cut5)
            ranges.append((S0 + cut5, S1 - cut3))
        else:
            ranges.append((None, None))
        sides.append(a)
    keep = None if rng.random() < 0.25 else (rng.random(n) < 0.9).astype(np.uint8)
    rules = dict(key_bases=int(rng.choice([0, 0, 25, 150])), prefer=int(rng.integers(0, 2)))
    return sides, ranges, keep, rules


def run_fuzz(lib, sh, seed):
    n = sh["dedup_fuzz"][1]
    sides, ranges, keep, rules = fuzz_batch(seed, n)
    a1, a2 = sides[0], sides[1] if len(sides) == 2 else None
    r1, r2 = ranges[0], ranges[1] if len(sides) == 2 else (None, None)
    m = dedup_model(a1, a2, r1, r2, keep, **rules)
    print("dedup fuzz", seed, "records", n, "pairs", a2 is not None, rules, "stats", m[3])
    assert 10 * m[3][2] >= m[3][0] and 10 * m[3][1] >= 2 * m[3][0]      # the model alone: both outcomes are well represented
    h = handle(lib)
    try:
        with staged(lib, h, a1, pad=3) as st1:
            if a2 is None:
                check_dedup(lib, h, st1, None, r1, r2, keep, pad=(3, 0), what=("fuzz", seed), model=m, **rules)
                check_dedup(lib, h, st1, pad=(3, 0), what=("fuzz, whole reads", seed))
            else:
                with staged(lib, h, a2, pad=1) as st2:
                    check_dedup(lib, h, st1, st2, r1, r2, keep, pad=(3, 1), what=("fuzz", seed), model=m, **rules)
                    check_dedup(lib, h, st1, st2, pad=(3, 1), what=("fuzz, whole reads", seed))
    finally:
        h.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def run_arg_refusals(lib, sh):
    rng = np.random.default_rng(1000)
    (a1, a2), _ = pool_batch(rng, 40, 9, pairs=True)
    n = a1.n_records
    u64 = lambda v: np.asarray(v).astype(np.uint64)
    S10, S11 = whole(a1); S20, S21 = whole(a2)
    h = handle(lib)
    try:
        with staged(lib, h, a1) as st1, staged(lib, h, a2) as st2:
            c1, c2 = st1.cols_in(), st2.cols_in()
            checked = 0

            def refused(got, name):
                assert got.error is not None and got.error.code == E_ARG and got.untouched, (name, got.error)
                return 1
            checked += refused(dedup_call(lib, h, c1, st2.cols_in(0, n - 1), n, lib_rules(lib)), "fewer mates")
            checked += refused(dedup_call(lib, h, st1.cols_in(1, n - 1), c2, n, lib_rules(lib)), "fewer of read 1")
            for name, dr in [("prefer 2", lib_rules(lib, prefer=2)), ("hash_bits 65", lib_rules(lib, hash_bits=65))] + \
                            [("reserved[%d]" % k, lib_rules(lib, reserved=tuple(int(i == k) for i in range(5)))) for k in range(5)]:
                checked += refused(dedup_call(lib, h, c1, c2, n, dr), name)
                checked += refused(dedup_call(lib, h, c1, None, n, dr), name + ", single")
            for name, r1, r2 in (("begin 1 alone", (u64(S10), None), (None, None)), ("end 1 alone", (None, u64(S11)), (None, None)),
                                 ("begin 2 alone", (None, None), (u64(S20), None)), ("end 2 alone", (None, None), (None, u64(S21)))):
                checked += refused(dedup_call(lib, h, c1, c2, n, lib_rules(lib), r1, r2), name)
            checked += refused(dedup_call(lib, h, c1, None, n, lib_rules(lib), (None, None), (u64(S10), u64(S11))), "ranges of side 2 without in2")
            checked += refused(dedup_call(lib, h, c1, c2, n, lib_rules(lib), null_out="keep"), "null d_keep")
            checked += refused(dedup_call(lib, h, c1, None, n, lib_rules(lib), keep=np.ones(n, np.uint8), null_out="keep"), "null d_keep, single")
            # 2^31 + 1 records: refused before anything is read -- the arrays behind these pointers hold 40 records
            big = lib.ColumnsIn(c1.d_bases, c1.bases_len, c1.d_quals, None, 0, c1.d_seq_offs, None, 2 ** 31 + 1)
            checked += refused(dedup_call(lib, h, big, None, n, lib_rules(lib)), "2^31 + 1 records")
            big2 = lib.ColumnsIn(c2.d_bases, c2.bases_len, c2.d_quals, None, 0, c2.d_seq_offs, None, 2 ** 31 + 1)
            checked += refused(dedup_call(lib, h, big, big2, n, lib_rules(lib, prefer=1)), "2^31 + 1 pairs")
            assert checked == 2 + 14 + 4 + 3 + 2
            with Dev(h) as d:                                 # a null stats array
                pk = d.fill(n)
                rc = h.L.dsrcgpu_columns_dedup_plan(h.h, lib.C.byref(c1), None, lib.C.byref(lib_rules(lib)), None, None, None, None, None,
                                                    lib.C.c_void_p(pk), None, None, None)
                assert rc == E_ARG and d.down(pk, n) == b"\xA5" * (n + 8)
            check_dedup(lib, h, st1, st2, what="the same handle, clean")
            check_dedup(lib, h, st1, key_bases=0xFFFFFFFF, prefer=1, hash_bits=64, what="the largest figures")
            for cin2 in (None, st2.cols_in(5, 0)):                # no records
                got = dedup_call(lib, h, st1.cols_in(3, 0), cin2, 0, lib_rules(lib))
                assert got.error is None and got.stats == [0] * 24 and got.untouched
    finally:
        h.close()
    hc = ce.handle(lib, dataclasses.replace(Config.from_levels(0, 0), color_space=True))
    try:
        with staged(lib, hc, a1) as st1:
            got = dedup_call(lib, hc, st1.cols_in(), None, n, lib_rules(lib))
            assert got.error is not None and got.error.code == E_ARG and got.untouched
    finally:
        hc.close()


def run_input_errors(lib, sh):
    """The adapter plan's input plants on side 1, on side 2 and on both (side 1 is the one reported), in the first, a middle and the
    last record, considered and dropped ones, single-end and pairs, fresh and in place: code, side, record, outputs still 0xA5 / the
    incoming keep unchanged, and the same handle plans the clean arrays afterwards."""
    rng = np.random.default_rng(1100)
    (a1, a2), _ = pool_batch(rng, 41, 9, pairs=True)
    n = a1.n_records
    pads = (4, 6)
    A = (a1, a2)
    S = lambda s, r: int(A[s].seq_offsets[r]) + pads[s]
    R = [tuple((v + pads[s]).astype(np.uint64) for v in whole(A[s])) for s in (0, 1)]
    keep = np.ones(n, np.uint8); keep[[0, 20]] = 0            # plants hit considered and dropped records alike
    dr = lib_rules(lib, prefer=1)
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
                            r1, r2 = (R[0], R[1]) if with_plans else ((None, None), (None, None))
                            got = dedup_call(lib, h, st1.cols_in(), st2.cols_in(), n, dr, r1, r2, keep if with_plans else None)
                            refused(got, sides[0], r, word, name)
                            assert got.untouched
                        if sides == (0,):                        # single-end: the side is named all the same
                            got = dedup_call(lib, h, st1.cols_in(), None, n, dr)
                            refused(got, 0, r, word, name)
                            assert got.untouched
                        st1.restore(); st2.restore()
                        checked += 1
                check_dedup(lib, h, st1, st2, keep=keep, prefer=1, pad=pads, what=("after", name))
            ranges = [("begin low", lambda s, r: dict(b=S(s, r) - 1), "d_begin lies below"),
                      ("end high", lambda s, r: dict(e=S(s, r + 1) + 1), "d_end lies above"),
                      ("end wild", lambda s, r: dict(e=2 ** 64 - 1), "d_end lies above"),
                      ("begin above end", lambda s, r: dict(b=S(s, r + 1), e=S(s, r + 1) - 1), "d_begin lies above d_end")]
            for name, how, word in ranges:
                for r in (0, 20, 40):
                    for sides in ((0,), (1,), (0, 1)):
                        p = [[v.copy() for v in R[s]] for s in (0, 1)]
                        for s in sides:
                            rr = r if s == sides[0] else 0
                            for key, v in how(s, rr).items():
                                p[s][0 if key == "b" else 1][rr] = v
                        for inplace in (False, True):
                            got = dedup_call(lib, h, st1.cols_in(), st2.cols_in(), n, dr, tuple(p[0]), tuple(p[1]), keep, inplace=inplace)
                            refused(got, sides[0], r, word, name)
                            assert got.keep_in_after == keep.tobytes() and (inplace or got.untouched), (name, r)
                        if sides == (0,):
                            got = dedup_call(lib, h, st1.cols_in(), None, n, dr, tuple(p[0]))
                            refused(got, 0, r, word, name)
                            assert got.untouched
                        checked += 1
                check_dedup(lib, h, st1, st2, keep=keep, prefer=1, pad=pads, what=("after", name))
    finally:
        h.close()
    assert checked == 63


def run_codec_state(lib, sh):
    """The call touches nothing the codec carries, as run_codec_state of the other planners: the fields capacity stays, a pending
    record layout stays pending, and the text call that follows writes what it writes on a fresh handle seeded alike."""
    (a1, a2), keep = pool_batch(np.random.default_rng(1200), 60, 11, keep_share=0.9, pairs=True)
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
                check_dedup(lib, h, st1, st2, keep=keep, prefer=1)
                check_dedup(lib, h, st1, keep=keep)
                assert h.get_fields_capacity() == 11
            assert text_blocks(h) == text_blocks(fresh), layout
        finally:
            h.close(); fresh.close()


# ---- the Python layers and the closed loop ---------------------------------------------------------------------------------------------
def run_python_layers(lib, sh, device):
    from dsrc_amd import columns
    sides, ranges, keep, _ = fuzz_batch(1, 140)              # pairs
    (a1, a2), (r1, r2) = sides, ranges
    if r1[0] is None:
        r1 = whole(a1)
    if keep is None:
        keep = (np.arange(140) % 9 != 0).astype(np.uint8)
    t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v).astype(dt)).to(device)
    signed = lambda v: np.where(v == NONE, -1, v.astype(np.int64))
    h = handle(lib)
    try:
        assert tuple(lib.DEDUP_STATS) == DEDUP_STATS and lib.NO_DUP_OF == NONE and lib.DEDUP_PREFER == {"first": 0, "quality": 1}
        c1, c2 = tensors(a1, device), tensors(a2, device)
        tb, te, tk = t(r1[0], np.int64), t(r1[1], np.int64), t(keep, np.uint8)
        m = dedup_model(a1, a2, r1, (None, None), keep, 25, 1)
        got = columns.dedup_plan(h, c1, c2, tb, te, keep=tk, key_bases=25, prefer="quality", return_dup_of=True, return_copies=True)
        assert len(got) == 4 and got[0].dtype == torch.uint8 and got[2].dtype == torch.int64 and got[3].dtype == torch.int64
        assert got[0].device.type == torch.device(device).type and got[0].data_ptr() != tk.data_ptr()
        assert torch.equal(tk, t(keep, np.uint8)) and torch.equal(tb, t(r1[0], np.int64))      # fresh tensors, inputs as they were
        assert list(got[1]) == list(DEDUP_STATS) and list(got[1].values()) == m[3]
        assert np.array_equal(got[0].cpu().numpy(), m[0]) and np.array_equal(got[2].cpu().numpy(), signed(m[1])) and np.array_equal(got[3].cpu().numpy(), m[2].astype(np.int64))
        m = dedup_model(a1)
        got = columns.dedup_plan(h, c1)
        assert len(got) == 2 and list(got[1].values()) == m[3] and np.array_equal(got[0].cpu().numpy(), m[0])
        got = columns.dedup_plan(h, c1, return_copies=True)
        assert len(got) == 3 and np.array_equal(got[2].cpu().numpy(), m[2].astype(np.int64))
        got = columns.dedup_plan(h, c1, keep=tk.bool(), return_dup_of=True)
        m = dedup_model(a1, keep=keep)
        assert len(got) == 3 and np.array_equal(got[2].cpu().numpy(), signed(m[1])) and list(got[1].values()) == m[3]

        class Never:                                         # ValueError comes before any library call
            def __getattr__(self, name):
                raise AssertionError("the library was called")
        fewer = tensors(ca.arrays_from_bases([np.zeros(5, np.uint8)]), device)
        bad_calls = [dict(key_bases=-1), dict(key_bases=2 ** 32), dict(key_bases=3.0), dict(key_bases=True), dict(prefer="best"), dict(prefer=1),
                     dict(begin=tb), dict(end=te), dict(cols2=c2, begin2=tb), dict(begin2=tb, end2=te), dict(cols2=fewer), dict(begin=tb[:5], end=te[:5]),
                     dict(keep=tk[:7])]
        calls = [lambda bad=bad: columns.dedup_plan(Never(), c1, **bad) for bad in bad_calls]
        calls += [lambda: columns.filter_columns(Never(), c1, dedup=True, dedup_prefer="last"), lambda: columns.filter_columns(Never(), c1, dedup=True, dedup_key_bases=-2),
                  lambda: columns.filter_pairs(Never(), c1, c2, dedup=True, dedup_prefer=0), lambda: columns.filter_pairs(Never(), c1, c2, dedup=True, dedup_key_bases=2 ** 40)]
        if torch.device(device).type != "cpu":               # column sets on different devices
            calls.append(lambda: columns.dedup_plan(Never(), c1, tensors(a2, "cpu")))
        for k, call in enumerate(calls):
            try:
                call()
            except ValueError:
                pass
            else:
                raise AssertionError("no ValueError for call %d" % k)
    finally:
        h.close()


def duplicated_reads(n, seed, pairs=False):
    """n records (pairs) of 60-base reads drawn from n / 3 templates -- inserts of 70 .. 110 bases, read 1 from the left, read 2 the
    reverse complement from the right, so that most mates overlap --, qualities that fall off at the 3' end of some, a few N -> per
    side (arrays, records, text)."""
    rng = np.random.default_rng(seed)
    pool = max(2, n // 3)
    pick = rng.integers(0, pool, n)
    inserts = [rng.integers(0, 4, int(rng.integers(70, 111))).astype(np.uint8) for _ in range(pool)]
    out = []
    for s in range(2 if pairs else 1):
        seqs = [(x if s == 0 else cp.revcomp(x))[:60] for x in inserts]
        recs = []
        for r in range(n):
            x = seqs[pick[r]].copy()
            if rng.random() < 0.15:
                x[int(rng.integers(0, 60))] = 4
            q = rng.integers(25, 41, 60)
            low = int(rng.integers(0, 12)) if rng.random() < 0.4 else 0
            if low: q[60 - low:] = rng.integers(2, 10, low)
            if rng.random() < 0.05: q[:] = rng.integers(2, 8, 60)      # a read that the quality plan drops
            recs.append((b"@dup.%d/%d" % (r + 1, s + 1), bytes(b"ACGTN"[v] for v in x), bytes((q + 33).astype(np.uint8))))
        text = b"\n".join(t + b"\n" + sq + b"\n+\n" + q for t, sq, q in recs)
        out.append((ce.arrays_of([text]), recs, text))
    return out


def same_columns(sel, want):
    return all(np.array_equal(g.cpu().numpy().astype(w.dtype), w) for g, w in zip((sel.bases, sel.quals, sel.titles, sel.seq_offsets, sel.title_offsets), want[:5]))


def run_filter_columns(lib, sh, device):
    from dsrc_amd import columns
    (a, _, _), = duplicated_reads(240, 31)
    trim = cs.rules_of(0, 20, min_length=30, max_n=1)
    ads = [cp.ADAPTER_STR[0]]
    h = handle(lib)
    try:
        c = tensors(a, device)
        for adapters in (None, ads):
            for kb, prefer in ((0, "first"), (40, "quality")):
                b, e, k, ts = cs.plan_model(a, trim)
                want_stats = dict(zip(ca.TRIM_STATS, ts))
                if adapters is not None:
                    ar = ca.rules_of([ca.codes_of(s) for s in adapters], 3, 100, trim["min_length"])
                    b, e, k, _, as_ = ca.adapter_model(a, ar, b, e, k)
                    want_stats["adapter"] = dict(zip(ca.ADAPTER_STATS, as_))
                plain, plain_stats = columns.filter_columns(h, c, adapters=adapters, **trim)
                again, again_stats = columns.filter_columns(h, c, adapters=adapters, dedup=False, dedup_key_bases=kb, dedup_prefer=prefer, **trim)
                assert plain_stats == again_stats == want_stats and same_columns(again, cs.select_model(a, b, e, k))      # dedup=False changes nothing
                assert same_columns(plain, cs.select_model(a, b, e, k))
                m = dedup_model(a, r1=(b, e), keep=k, key_bases=kb, prefer=lib.DEDUP_PREFER[prefer])
                assert m[3][3] >= 15 and m[3][5] > 0 and (prefer == "first" or m[3][7] > 0), m[3]
                want_stats["dedup"] = dict(zip(DEDUP_STATS, m[3]))
                out, stats = columns.filter_columns(h, c, adapters=adapters, dedup=True, dedup_key_bases=kb, dedup_prefer=prefer, **trim)
                assert stats == want_stats and list(stats)[-1] == "dedup", (stats, want_stats)
                assert same_columns(out, cs.select_model(a, b, e, m[0])) and out.n_records == m[3][1]
        out, stats = columns.filter_columns(h, c, dedup=True, profile=True, **trim)
        b, e, k, _ = cs.plan_model(a, trim)
        m = dedup_model(a, r1=(b, e), keep=k)
        after = stats["profile_after"].summary()
        assert after["records"] == m[3][1] == out.n_records and after["bases"] == out.bases.numel()      # the profile reflects the dedup
        assert stats["profile_before"].summary()["records"] == a.n_records
    finally:
        h.close()


def run_filter_pairs(lib, sh, device):
    from dsrc_amd import columns
    (a1, _, _), (a2, _, _) = duplicated_reads(200, 41, pairs=True)
    trim = cs.rules_of(0, 20, min_length=30, max_n=2)
    h = handle(lib)
    try:
        c1, c2 = tensors(a1, device), tensors(a2, device)
        kw = dict(pair_min_overlap=20, pair_max_mismatches=4, pair_max_error_permille=150)
        for overlap in (True, False):
            r1, r2, keep, wstats = cp.pairs_model(a1, a2, trim, (None, None), overlap, cp.rules_of(20, 4, 150))
            p1, p2, pstats = columns.filter_pairs(h, c1, c2, overlap=overlap, **kw, **trim)
            q1, q2, qstats = columns.filter_pairs(h, c1, c2, overlap=overlap, dedup=False, dedup_key_bases=7, dedup_prefer="quality", **kw, **trim)
            assert pstats == qstats == wstats                  # dedup=False changes nothing
            for u, v, a, rr in ((p1, q1, a1, r1), (p2, q2, a2, r2)):
                w = cs.select_model(a, rr[0], rr[1], keep)
                assert same_columns(u, w) and same_columns(v, w)
            for kb, prefer in ((0, "first"), (45, "quality")):
                m = dedup_model(a1, a2, r1, r2, keep, kb, lib.DEDUP_PREFER[prefer])
                assert m[3][3] >= 10 and m[3][5] > 0, m[3]
                m1 = dedup_model(a1, None, r1, (None, None), keep, kb, lib.DEDUP_PREFER[prefer])
                assert m1[3] == m[3] or m1[3][1] <= m[3][1]      # (keyed on both mates: never fewer classes than on read 1 alone)
                o1, o2, stats = columns.filter_pairs(h, c1, c2, overlap=overlap, dedup=True, dedup_key_bases=kb, dedup_prefer=prefer, **kw, **trim)
                assert stats == dict(wstats, dedup=dict(zip(DEDUP_STATS, m[3]))), (overlap, kb, stats)
                assert same_columns(o1, cs.select_model(a1, r1[0], r1[1], m[0])) and same_columns(o2, cs.select_model(a2, r2[0], r2[1], m[0]))
                assert o1.n_records == o2.n_records == m[3][1]
        # merge=True: the dedup stands between the pair plan and the merge -- the merge gets the deduplicated keep
        r1, r2, keep, wstats = cp.pairs_model(a1, a2, trim, (None, None), True, cp.rules_of(20, 4, 150))
        m = dedup_model(a1, a2, r1, r2, keep)
        t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v).astype(dt)).to(device)
        b1, e1, b2, e2, pk, _, insert = columns.pair_plan(h, c1, c2, *[columns.trim_plan(h, c, **trim)[:3] for c in (c1, c2)], 20, 4, 150, trim["min_length"],
                                                          return_insert=True)
        assert np.array_equal(pk.cpu().numpy(), keep)
        wm, wflag, wms = columns.merge_pairs(h, c1, c2, b1, e1, b2, e2, t(m[0], np.uint8), insert, 20, 4, 150)
        o1, o2, merged, stats = columns.filter_pairs(h, c1, c2, merge=True, dedup=True, **kw, **trim)
        assert stats["dedup"] == dict(zip(DEDUP_STATS, m[3])) and stats["merge"] == wms and list(stats) == ["read1", "read2", "pair", "dedup", "merge"]
        assert merged.n_records + o1.n_records == m[3][1] and o1.n_records == o2.n_records and wms["pairs_merged"] > 0
        rest = m[0] & (wflag.cpu().numpy() ^ 1)
        assert same_columns(o1, cs.select_model(a1, r1[0], r1[1], rest)) and same_columns(o2, cs.select_model(a2, r2[0], r2[1], rest))
        assert torch.equal(merged.bases, wm.bases) and torch.equal(merged.seq_offsets, wm.seq_offsets) and torch.equal(merged.titles, wm.titles)
        x1, x2, xm, xstats = columns.filter_pairs(h, c1, c2, merge=True, **kw, **trim)
        y1, y2, ym, ystats = columns.filter_pairs(h, c1, c2, merge=True, dedup=False, dedup_prefer="quality", **kw, **trim)
        assert xstats == ystats and "dedup" not in xstats and torch.equal(xm.bases, ym.bases) and torch.equal(x1.bases, y1.bases) and torch.equal(x2.seq_offsets, y2.seq_offsets)
    finally:
        h.close()


def run_closed_loop(lib, sh, device):
    """Records written here -> the oracle's block -> decode_columns -> filter_columns(dedup=True) -> encode_columns -> decode_columns:
    the records that come back are the model's -- its trim, its keep, one record of every class."""
    from dsrc_amd import columns
    cfg = ce.BLOCK_CFG
    (a, recs, text), = duplicated_reads(180, 51)
    trim = cs.rules_of(0, 20, min_length=35)
    b, e, k, _ = cs.plan_model(a, trim)
    m = dedup_model(a, r1=(b, e), keep=k, prefer=1)
    print("closed loop: model stats", m[3])
    assert m[3][3] >= 12 and m[3][7] > 0 and 0 < m[3][1] < m[3][0] < 180
    want = cs.select_model(a, b, e, m[0])
    src = ce.oracle_blocks(cfg, [text])
    assert src is not None
    h = ce.handle(lib, cfg)
    try:
        d_blocks, offs = cs._stage_blocks([src[0][0]], device)
        rc = columns.decode_columns(h, d_blocks, offs, [len(src[0][0])], device)
        assert rc.n_records == 180
        out, stats = columns.filter_columns(h, rc, dedup=True, dedup_prefer="quality", **trim)
        assert list(stats["dedup"].values()) == m[3] and same_columns(out, want)
        h.set_fields_capacity(0)
        blocks, o_offs, o_sizes, _ = columns.encode_columns(h, out, block_records=out.block_records)
    finally:
        h.close()
    h = ce.handle(lib, cfg)
    try:
        back = columns.decode_columns(h, blocks, o_offs, o_sizes, device)
        assert back.n_records == m[3][1] and same_columns(back, want)
    finally:
        h.close()
