"""Shared by tests/test_emu_columns_kmer.py (CPU, emulator build) and tests/test_gpu_columns_kmer.py (MI355X): the cases of the
columnar k-mer count (dsrcgpu_columns_kmer_count, dsrcgpu_kmer_table_merge, dsrcgpu_kmer_spectrum, dsrcgpu_kmer_lookup;
dsrc_amd/csrc/k_columns_kmer.h) and what they must give.

The reference has no counterpart, so the yardstick is the integer model written out here: kmer_model_serial() is the serial rule of
include/dsrc_gpu.h with a Python dict keyed on the packed word.  kmer_model() is the same rule over whole numpy arrays for the
large batches; test_the_two_models_agree holds the two against each other.  None of it comes from the library under test, and
every comparison is exact equality.  A table is compared as its occupied slots SORTED BY KEY, plus the header, plus a lookup of
every model key and of some absent ones -- never by slot position, which depends on the order of arrival.  Tables and other outputs
are filled with 0xA5 before a call, so that "untouched" and "not a byte beyond" can be asserted.  Before the library is compared on a
crafted case the model alone is asked what that case is for.

Shapes.  The emulator pays a coroutine switch per wave exchange, so its fuzz is 2 seeds x 150 records where the GPU runs 6 x 2000.
The wave-per-record grid holds at most 4096 workgroups of WG / 64 waves: with workgroups of 1024 threads 4096 * 16 + 1001 records
take the grid stride into a second round -- that count, and the contention batch of 20 000 reads of three sequences, run on the GPU
only."""
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

E_ARG, E_INPUT, E_CAPACITY = cs.E_ARG, cs.E_INPUT, -4
EMPTY = 2 ** 64 - 1
GRID_CAP = 4096                  # workgroups of the wave-per-record launch
PROBE_LIMIT = 1024
MAGIC = 0x4B4D4552

SHAPES = {
    "gpu": dict(cc.SHAPES["gpu"], kmer_fuzz=(6, 2000), counts=[1, 63, 64, 65, 2049], stride_count=GRID_CAP * 16 + 1001, contention=20000),
    "emu": dict(cc.SHAPES["emu"], kmer_fuzz=(2, 150), counts=[1, 63, 64, 65, 2049], stride_count=None, contention=None),
}
Dev = cs.Dev
staged = cp.staged
handle = cp.handle
tensors = ca.tensors
arrays = ca.arrays_from_bases
KMER_STATS = ("records_considered", "records_came_dropped", "records_short", "windows", "kmers_counted", "windows_broken", "kmers_new", "overflow",
              "distinct_after", "total_after")
KS = [1, 2, 15, 16, 17, 31]


# ---- the model -------------------------------------------------------------------------------------------------------------------
def pack(codes):
    v = 0
    for c in codes:
        assert 0 <= int(c) <= 3
        v = (v << 2) | int(c)
    return v


def revcomp_word(v, k):
    out = 0
    for _ in range(k):
        out = (out << 2) | (3 - (v & 3))
        v >>= 2
    return out


def key_of(codes, canonical):
    f = pack(codes)
    return min(f, revcomp_word(f, len(codes))) if canonical else f


def header_word(k, canonical, hash_bits=0):
    return (MAGIC << 32) | ((hash_bits & 63) << 16) | (k << 8) | int(canonical)


def need_of(keys):
    need = 16
    while need < 2 * keys:
        need *= 2
    return need


def plan_of(a, begin, end, first, n):
    S = a.seq_offsets.astype(np.int64)
    b = S[first: first + n].copy() if begin is None else np.asarray(begin).astype(np.int64)
    e = S[first + 1: first + n + 1].copy() if end is None else np.asarray(end).astype(np.int64)
    assert (S[first: first + n] <= b).all() and (b <= e).all() and (e <= S[first + 1: first + n + 1]).all()
    return b, e


def kmer_model_serial(a, k, canonical=1, begin=None, end=None, keep=None, first=0, n=None, table=None):
    """The serial rule on records first .. first + n - 1 -> (table: dict key -> count, stats[16]).  `table`: the dict to add to
    (accumulate); stats[8], stats[9] are those of the dict that comes out."""
    n = a.n_records - first if n is None else n
    b, e = plan_of(a, begin, end, first, n)
    table = {} if table is None else dict(table)
    stats = [0] * 16
    before = len(table)
    for r in range(n):
        if keep is not None and keep[r] == 0:
            stats[1] += 1
            continue
        stats[0] += 1
        if e[r] - b[r] < k:
            stats[2] += 1
            continue
        for p in range(int(b[r]), int(e[r]) - k + 1):
            stats[3] += 1
            w = a.bases[p: p + k]
            if (w > 3).any():
                stats[5] += 1
                continue
            key = key_of(w, canonical)
            table[key] = table.get(key, 0) + 1
            stats[4] += 1
    stats[6] = len(table) - before
    stats[8], stats[9] = len(table), sum(table.values())
    assert stats[3] == stats[4] + stats[5]
    return table, stats


def window_keys(bases, k, canonical):
    """For every position p of `bases` with p + k <= len: the key of the window at p, and whether it is broken."""
    L = len(bases) - k + 1
    if L <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, bool)
    code = (bases & 3).astype(np.uint64)
    fwd, rc = np.zeros(L, np.uint64), np.zeros(L, np.uint64)
    for j in range(k):
        fwd = (fwd << np.uint64(2)) | code[j: j + L]
        rc |= (np.uint64(3) - code[j: j + L]) << np.uint64(2 * j)
    nb = np.concatenate(([0], np.cumsum(bases > 3)))
    return (np.minimum(fwd, rc) if canonical else fwd), (nb[k:] - nb[:-k])[:L] > 0


def kmer_model(a, k, canonical=1, begin=None, end=None, keep=None, first=0, n=None, table=None):
    """kmer_model_serial over whole arrays (for the batches too large for a Python loop per window)."""
    n = a.n_records - first if n is None else n
    b, e = plan_of(a, begin, end, first, n)
    cons = np.ones(n, bool) if keep is None else np.asarray(keep) != 0
    wins = np.where(cons, np.maximum(e - b - k + 1, 0), 0)
    stats = [0] * 16
    stats[0], stats[1], stats[2], stats[3] = int(cons.sum()), int((~cons).sum()), int((cons & (e - b < k)).sum()), int(wins.sum())
    keys, broken = window_keys(a.bases, k, canonical)
    at = np.repeat(b - (np.cumsum(wins) - wins), wins) + np.arange(int(wins.sum()))
    good = ~broken[at]
    stats[5] = int((~good).sum()); stats[4] = stats[3] - stats[5]
    uk, uc = np.unique(keys[at][good], return_counts=True)
    table = {} if table is None else dict(table)
    before = len(table)
    for key, c in zip(uk.tolist(), uc.tolist()):
        table[key] = table.get(key, 0) + c
    stats[6] = len(table) - before
    stats[8], stats[9] = len(table), sum(table.values())
    return table, stats


def run_models_agree():
    """The vectorised model against the serial one: k at both ends and in the middle, ranges, keep, every kind of code."""
    for seed, k, canonical in ((0, 1, 1), (1, 2, 0), (2, 15, 1), (3, 16, 0), (4, 17, 1), (5, 31, 1), (6, 31, 0), (7, 5, 1)):
        a, begin, end, keep = fuzz_batch(seed, 60, k)
        ms, mv = kmer_model_serial(a, k, canonical, begin, end, keep), kmer_model(a, k, canonical, begin, end, keep)
        assert ms == mv, (seed, k, ms[1], mv[1])
        assert ms[1][4] > 0 and ms[1][5] > 0 and ms[1][1] > 0
        half = a.n_records // 2
        m1 = kmer_model(a, k, canonical, begin[:half], end[:half], keep[:half], 0, half)
        m2 = kmer_model(a, k, canonical, begin[half:], end[half:], keep[half:], half, a.n_records - half, table=m1[0])
        assert m2[0] == ms[0] and m2[1][8:10] == ms[1][8:10]
    assert revcomp_word(pack([0, 1, 2, 3]), 4) == pack([0, 1, 2, 3]) and revcomp_word(pack([0, 0, 1]), 3) == pack([2, 3, 3])
    assert key_of([3, 3, 3], 1) == 0 and key_of([3, 3, 3], 0) == 63


# ---- a table in device memory, one call ------------------------------------------------------------------------------------------------
class Table:
    """kmer_words(M) uint64 words of device memory this test owns, 0xA5-filled, 8 spare bytes behind."""

    def __init__(self, lib, d, M):
        self.lib, self.d, self.M = lib, d, M
        self.nbytes = 8 * lib.kmer_words(M)
        self.p = d.fill(self.nbytes)

    def raw(self):
        got = self.d.down(self.p, self.nbytes)
        assert got[-8:] == b"\xA5" * 8, "written behind the end of the table"
        return np.frombuffer(got[:-8], np.uint64)

    def untouched(self):
        got = self.d.down(self.p, self.nbytes)
        return got == b"\xA5" * len(got)

    def items(self):
        w = self.raw()
        keys, counts = w[8: 8 + self.M], w[8 + self.M:]
        used = keys != np.uint64(EMPTY)
        assert (counts[~used] == 0).all(), "a count in a free slot"
        order = np.argsort(keys[used], kind="stable")
        return dict(zip(keys[used][order].tolist(), counts[used][order].tolist())), int(used.sum())


@dataclasses.dataclass
class Got:
    error: object
    stats: object


def lib_rules(lib, k, canonical=1, accumulate=0, hash_bits=0, capacity=16, reserved=(0, 0, 0, 0)):
    return lib.KmerRules(k, canonical, accumulate, hash_bits, capacity, reserved)


def kmer_call(lib, h, d, cin, kr, tab, begin=None, end=None, keep=None, null_table=False):
    """One dsrcgpu_columns_kmer_count into `tab`.  begin / end / keep: numpy in the coordinates of the staged arrays, or None."""
    up = lambda v, dt: None if v is None else d.up(np.ascontiguousarray(v).astype(dt).tobytes())
    try:
        return Got(None, h.columns_kmer_count(cin, up(begin, np.uint64), up(end, np.uint64), up(keep, np.uint8), kr, None if null_table else tab.p))
    except lib.DsrcGpuError as e:
        return Got(e, None)


def lookup(lib, h, d, tab, words):
    words = np.asarray(words, np.uint64)
    pq, po = d.up(words.tobytes()), d.fill(8 * len(words))
    invalid = h.kmer_lookup(tab.p, pq, len(words), po)
    got = d.down(po, 8 * len(words))
    assert got[-8:] == b"\xA5" * 8
    return np.frombuffer(got[:-8], np.uint64), invalid


def check_table(lib, h, d, tab, k, canonical, model, overflow=0, hash_bits=0, what=None, rng=None):
    """The table == the model's dict: pairs sorted by key, the header, and what the lookup says of every model key and of absent ones."""
    pairs, used = tab.items()
    assert used == len(pairs), (what, "a key sits in two slots")
    assert pairs == dict(sorted(model.items())), (what, len(pairs), len(model), [(x, pairs.get(x), model.get(x)) for x in list(set(pairs) ^ set(model))[:4]])
    hdr = tab.raw()[:8].tolist()
    assert hdr == [header_word(k, canonical, hash_bits), tab.M, len(model), sum(model.values()), overflow, 0, 0, 0], (what, hdr)
    rng = rng or np.random.default_rng(len(model))
    keys = list(model)
    absent = [int(v) for v in rng.integers(0, 4 ** k, 40) if key_of_word(int(v), k, canonical) not in model]
    got, invalid = lookup(lib, h, d, tab, keys + absent)
    assert invalid == 0 and got.tolist() == [model[x] for x in keys] + [0] * len(absent), what
    if canonical and keys:                                   # the other strand gives the same answer
        got, _ = lookup(lib, h, d, tab, [revcomp_word(x, k) for x in keys[:50]])
        assert got.tolist() == [model[x] for x in keys[:50]], what


def key_of_word(v, k, canonical):
    return min(v, revcomp_word(v, k)) if canonical else v


def check_count(lib, h, st, k, canonical=1, begin=None, end=None, keep=None, pad=0, first=0, n=None, M=None, hash_bits=0, model=None, what=None, fast=True):
    """A fresh table of M slots (None: what the 3/4 rule asks for) filled by one call == the model."""
    n = st.a.n_records - first if n is None else n
    m = model if model is not None else (kmer_model if fast else kmer_model_serial)(st.a, k, canonical, begin, end, keep, first, n)
    M = need_of(m[1][3]) if M is None else M
    shift = lambda v: None if v is None else np.asarray(v).astype(np.uint64) + np.uint64(pad)
    with Dev(h) as d:
        tab = Table(lib, d, M)
        got = kmer_call(lib, h, d, st.cols_in(first, n), lib_rules(lib, k, canonical, 0, hash_bits, M), tab, shift(begin), shift(end), keep)
        assert got.error is None, (what, got.error)
        assert got.stats == m[1], (what, got.stats, m[1])
        assert got.stats[3] == got.stats[4] + got.stats[5] + got.stats[7]
        check_table(lib, h, d, tab, k, canonical, m[0], hash_bits=hash_bits, what=what)
    return m


def whole(a):
    S = a.seq_offsets.astype(np.int64)
    return S[:-1].copy(), S[1:].copy()


# ---- geometry --------------------------------------------------------------------------------------------------------------------
def geometry_reads(rng, k):
    """Per range length in k - 1, k, k + 1, 63 + k, 64 + k, 65 + k, 128 + k and per alignment 0 .. 15 of the range's first byte: a
    stored read of random bases with the range somewhere inside -> arrays, begin, end."""
    reads, offs, lens = [], [], []
    pos = 0
    for L in (k - 1, k, k + 1, 63 + k, 64 + k, 65 + k, 128 + k):
        for align in range(16):
            lead = (align - pos) % 16
            reads.append(rng.integers(0, 4, lead + L + 2).astype(np.uint8))
            offs.append(pos + lead); lens.append(L)
            pos += lead + L + 2
    a = arrays(reads)
    b = np.array(offs, np.int64)
    return a, b, b + np.array(lens, np.int64)


def run_geometry(lib, sh, k):
    rng = np.random.default_rng(100 + k)
    a, b, e = geometry_reads(rng, k)
    assert {int(v) % 16 for v in b} == set(range(16)) and a.n_records == 7 * 16
    h = handle(lib)
    try:
        with staged(lib, h, a) as st:
            for canonical in (1, 0):
                m = kmer_model(a, k, canonical, b, e)
                assert m[1][2] == 16 and m[1][3] == 16 * (1 + 2 + 64 + 65 + 66 + 129) and m[1][5] == 0      # k - 1: no window; k: one
                check_count(lib, h, st, k, canonical, b, e, model=m, what=("geometry", k, canonical))
            check_count(lib, h, st, k, what=("geometry, whole reads", k))
    finally:
        h.close()


# ---- non-bases ---------------------------------------------------------------------------------------------------------------------
def run_non_bases(lib, sh):
    rng = np.random.default_rng(200)
    h = handle(lib)
    try:
        for k in (2, 16, 31):
            L = 130 + k
            reads, broken = [], []

            def add(places, code=4):
                x = rng.integers(0, 4, L).astype(np.uint8)
                x[list(places)] = code
                reads.append(x)
                hit = np.zeros(L - k + 1, bool)
                for p in places:
                    hit[max(0, p - k + 1): p + 1] = True     # the windows that hold position p
                broken.append(int(hit.sum()))
            # first and last base of the read, of a window in the middle; the positions round the 64-window step boundary and round
            # the end of the step's first / last window; runs longer than k; every kind of code that is not a base
            for p in (0, L - 1, 40, 62, 63, 64, 65, 63 + k - 1, 64 + k - 1, 127, 128):
                add([p])
            add(range(50, 50 + k + 3)); add(range(60, 60 + 2 * k + 5), 255); add(range(0, L))
            for code in (5, 15, 16, 18, 19, 255):
                add([33, 90], code)
            add([0, 1, 64, L - 1])
            a = arrays(reads)
            m = kmer_model_serial(a, k)
            for r, want in enumerate(broken):                   # the model alone: each read breaks what the plant says
                one = kmer_model_serial(a, k, first=r, n=1)
                assert one[1][5] == want and one[1][3] == L - k + 1, (k, r, one[1], want)
            assert broken[0] == 1 and broken[1] == 1 and broken[2] == min(k, 41) and broken[13] == L - k + 1
            with staged(lib, h, a, pad=5) as st:
                check_count(lib, h, st, k, model=m, what=("non-bases", k))
                check_count(lib, h, st, k, 0, what=("non-bases, forward", k))
    finally:
        h.close()


# ---- strands ---------------------------------------------------------------------------------------------------------------------
def run_strands(lib, sh):
    """Palindromic k-mers (even k, their own reverse complement), and a k-mer and its reverse complement in different reads."""
    rng = np.random.default_rng(300)
    h = handle(lib)
    try:
        for k in (2, 4, 16, 30):
            half = rng.integers(0, 4, k // 2).astype(np.uint8)
            pal = np.concatenate((half, cp.revcomp(half)))
            x = rng.integers(0, 4, k).astype(np.uint8)
            while pack(x) == revcomp_word(pack(x), k):
                x = rng.integers(0, 4, k).astype(np.uint8)
            a = arrays([pal, x, cp.revcomp(x), pal, x])
            assert revcomp_word(pack(pal), k) == pack(pal)
            mc, mf = kmer_model_serial(a, k, 1), kmer_model_serial(a, k, 0)
            assert mc[0] == {pack(pal): 2, min(pack(x), revcomp_word(pack(x), k)): 3}
            assert mf[0] == {pack(pal): 2, pack(x): 2, revcomp_word(pack(x), k): 1}
            with staged(lib, h, a) as st:
                check_count(lib, h, st, k, 1, model=mc, what=("strands, canonical", k))
                check_count(lib, h, st, k, 0, model=mf, what=("strands, forward", k))
        for k in (1, 15, 17, 31):                                # odd k: no k-mer is its own reverse complement
            x = rng.integers(0, 4, k + 40).astype(np.uint8)
            a = arrays([x, cp.revcomp(x)])
            mc, mf = kmer_model_serial(a, k, 1), kmer_model_serial(a, k, 0)
            assert all(c % 2 == 0 for c in mc[0].values()) and sum(mf[0].values()) == sum(mc[0].values()) and len(mf[0]) >= len(mc[0])
            with staged(lib, h, a) as st:
                check_count(lib, h, st, k, 1, model=mc, what=("two strands, canonical", k))
                check_count(lib, h, st, k, 0, model=mf, what=("two strands, forward", k))
    finally:
        h.close()


# ---- homopolymers ------------------------------------------------------------------------------------------------------------------
def run_homopolymers(lib, sh):
    """Runs of 1, 63, 64, 65 and 200 equal windows, at leads that put them across the step boundaries: the run aggregation."""
    rng = np.random.default_rng(400)
    h = handle(lib)
    try:
        for k in (1, 16, 31):
            reads, want_g = [], 0
            for base, runs in ((2, (1, 63, 64, 65, 200)), (0, (64, 200)), (3, (65,))):
                for run in runs:
                    for lead in (0, 1, 40, 63, 64):
                        # a lead and a tail that end / begin with another base, so that the run is exactly `run` windows
                        head = rng.integers(0, 4, lead).astype(np.uint8); tail = rng.integers(0, 4, 9).astype(np.uint8)
                        if lead: head[-1] = (base + 1) % 4
                        tail[0] = (base + 1) % 4
                        reads.append(np.concatenate((head, np.full(run + k - 1, base, np.uint8), tail)).astype(np.uint8))
            a = arrays(reads)
            mc, mf = kmer_model(a, k, 1), kmer_model(a, k, 0)
            g = pack([2] * k)
            assert mf[0][g] >= 5 * (1 + 63 + 64 + 65 + 200) and mf[0][pack([0] * k)] >= 5 * 264 and mf[0][pack([3] * k)] >= 5 * 65
            assert mc[0][pack([0] * k)] == mf[0][pack([0] * k)] + mf[0][pack([3] * k)] and mc[0][pack([1] * k)] >= mf[0][g]      # poly-T is poly-A, poly-G is poly-C
            with staged(lib, h, a, pad=3) as st:
                check_count(lib, h, st, k, 1, model=mc, what=("homopolymers", k))
                check_count(lib, h, st, k, 0, model=mf, what=("homopolymers, forward", k))
    finally:
        h.close()


# ---- plans in ------------------------------------------------------------------------------------------------------------------------
def pool_batch(rng, n, pool, lo=8, hi=40, keep_share=1.0, other=0.01):
    """n reads drawn from `pool` sequences of lo .. hi codes (a few not bases) -> arrays, keep (or None)"""
    seqs = []
    for _ in range(pool):
        x = rng.integers(0, 4, int(rng.integers(lo, hi + 1))).astype(np.uint8)
        x[rng.random(len(x)) < other] = 4
        seqs.append(x)
    a = arrays([seqs[i] for i in rng.integers(0, pool, n)])
    keep = None if keep_share >= 1.0 else (rng.random(n) < keep_share).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
    return a, keep


def run_plans_in(lib, sh):
    """Empty ranges, ranges shorter than k, records that came in dropped, a call on a slice of the records, nothing considered."""
    rng = np.random.default_rng(500)
    a, keep = pool_batch(rng, 70, 20, lo=12, keep_share=0.8)
    n = a.n_records
    S0, S1 = whole(a)
    b, e = S0 + rng.integers(0, 4, n), S1 - rng.integers(0, 4, n)
    b[[3, 30]] = e[[3, 30]]                                    # empty ranges
    b[0] = S1[0]; e[0] = S1[0]                                 # ... one at the record's end
    e[5] = b[5] + 4; e[6] = b[6] + 5; e[7] = b[7] + 6          # k = 6: too short, too short, one window
    k = 6
    m = kmer_model_serial(a, k, 1, b, e, keep)
    assert m[1][1] > 5 and m[1][2] >= 3 and m[1][5] > 0
    h = handle(lib)
    try:
        for pad in (0, 9):
            with staged(lib, h, a, pad=pad) as st:
                check_count(lib, h, st, k, 1, b, e, keep, pad=pad, model=m, what="ranges, keep")
                check_count(lib, h, st, k, 0, b, e, None, pad=pad, what="ranges")
                check_count(lib, h, st, k, 1, None, None, keep, pad=pad, what="keep alone")
                for first, cnt in ((2, None), (n - 1, 1), (3, 6)):
                    sl = slice(first, None if cnt is None else first + cnt)
                    check_count(lib, h, st, k, 1, b[sl], e[sl], keep[sl], pad=pad, first=first, n=cnt, what=("first", first))
                mz = check_count(lib, h, st, k, 1, keep=np.zeros(n, np.uint8), pad=pad, what="nothing considered")
                assert mz[0] == {} and mz[1][1] == n
                me = check_count(lib, h, st, k, 1, S0, S0, pad=pad, what="every range empty")
                assert me[0] == {} and me[1][2] == n
    finally:
        h.close()


def run_count(lib, sh, n_records):
    rng = np.random.default_rng(700 + n_records)
    a, keep = pool_batch(rng, n_records, max(1, n_records // 3), keep_share=0.9)
    h = handle(lib)
    try:
        with staged(lib, h, a) as st:
            m = check_count(lib, h, st, 5, 1, keep=keep, what=n_records)
            check_count(lib, h, st, 11, 0, what=(n_records, "every record, forward"))
            if n_records >= 2049:
                assert m[1][3] > 30000 and m[1][5] > 300 and m[1][1] > 100 and len(m[0]) == 512      # every canonical 5-mer
    finally:
        h.close()


def run_grid_stride(lib, sh):
    n = sh["stride_count"]
    rng = np.random.default_rng(900)
    a, keep = pool_batch(rng, n, 500, lo=8, hi=20, keep_share=0.95)
    m = kmer_model(a, 6, 1, keep=keep)
    second = kmer_model(a, 6, 1, keep=keep[GRID_CAP * 16:], first=GRID_CAP * 16, n=1001)
    assert second[1][0] > 900 and second[1][4] > 5000 and len(m[0]) > 1000 and m[1][3] > 400000      # the records of the second round count
    h = handle(lib)
    try:
        with staged(lib, h, a) as st:
            check_count(lib, h, st, 6, 1, keep=keep, model=m, what="grid stride")
    finally:
        h.close()


def run_contention(lib, sh):
    """20 000 reads of three sequences: every wave adds to the same few hundred slots.  Run twice: equal sorted tables."""
    n = sh["contention"]
    rng = np.random.default_rng(800)
    seqs = [rng.integers(0, 4, 60).astype(np.uint8), rng.integers(0, 4, 45).astype(np.uint8), np.full(50, 2, np.uint8)]
    a = arrays([seqs[i] for i in rng.integers(0, 3, n)])
    k = 15
    m = kmer_model(a, k, 1)
    assert len(m[0]) <= 46 + 31 + 1 and max(m[0].values()) > n // 4 * 36 and m[1][3] > 30 * n
    h = handle(lib)
    try:
        with staged(lib, h, a) as st, Dev(h) as d:
            M = need_of(m[1][3])
            rounds = []
            for _ in range(2):
                tab = Table(lib, d, M)
                got = kmer_call(lib, h, d, st.cols_in(), lib_rules(lib, k, 1, 0, 0, M), tab)
                assert got.error is None and got.stats == m[1], (got.error, got.stats, m[1])
                check_table(lib, h, d, tab, k, 1, m[0], what="contention")
                rounds.append((tab.items(), tab.raw()[:8].tolist()))
            assert rounds[0] == rounds[1]
    finally:
        h.close()


# ---- accumulate and merge --------------------------------------------------------------------------------------------------------
def merge_call(lib, h, src, dst):
    try:
        return Got(None, h.kmer_table_merge(src.p, dst.p))
    except lib.DsrcGpuError as e:
        return Got(e, None)


def run_accumulate_and_merge(lib, sh):
    rng = np.random.default_rng(1300)
    a, keep = pool_batch(rng, 120, 40, keep_share=0.9)
    n, k, half = a.n_records, 9, 50
    whole_m = kmer_model_serial(a, k, 1, keep=keep)
    m1 = kmer_model_serial(a, k, 1, keep=keep[:half], first=0, n=half)
    m2 = kmer_model_serial(a, k, 1, keep=keep[half:], first=half, n=n - half)
    m12 = kmer_model_serial(a, k, 1, keep=keep[half:], first=half, n=n - half, table=m1[0])
    assert m12[0] == whole_m[0] and 0 < m12[1][6] < len(m2[0])          # the second half brings new keys and meets old ones
    M = need_of(whole_m[1][3])
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=2) as st, Dev(h) as d:
            # two halves with accumulate == the whole
            tab = Table(lib, d, M)
            g1 = kmer_call(lib, h, d, st.cols_in(0, half), lib_rules(lib, k, 1, 0, 0, M), tab, keep=keep[:half])
            assert g1.error is None and g1.stats == m1[1]
            check_table(lib, h, d, tab, k, 1, m1[0], what="first half")
            g2 = kmer_call(lib, h, d, st.cols_in(half, n - half), lib_rules(lib, k, 1, 1, 0, M), tab, keep=keep[half:])
            assert g2.error is None and g2.stats == m12[1], (g2.error, g2.stats, m12[1])
            check_table(lib, h, d, tab, k, 1, whole_m[0], what="both halves")
            # accumulate = 0 on a table that holds something starts again
            g3 = kmer_call(lib, h, d, st.cols_in(half, n - half), lib_rules(lib, k, 1, 0, 0, M), tab, keep=keep[half:])
            assert g3.error is None and g3.stats == m2[1]
            check_table(lib, h, d, tab, k, 1, m2[0], what="started again")
            # no records: accumulate = 0 initialises, 1 only checks
            g4 = kmer_call(lib, h, d, st.cols_in(3, 0), lib_rules(lib, k, 1, 1, 0, M), tab)
            assert g4.error is None and g4.stats == [0] * 8 + [len(m2[0]), sum(m2[0].values())] + [0] * 6
            check_table(lib, h, d, tab, k, 1, m2[0], what="no records, accumulate")
            empty = Table(lib, d, 16)
            g5 = kmer_call(lib, h, d, st.cols_in(3, 0), lib_rules(lib, k, 1, 0, 0, 16), empty)
            assert g5.error is None and g5.stats == [0] * 16
            check_table(lib, h, d, empty, k, 1, {}, what="no records, fresh")
            # the merge of two tables == the table of the union: into an equal and into a larger capacity
            for M_dst in (M, 4 * M):
                t1, t2 = Table(lib, d, M), Table(lib, d, M_dst)
                assert kmer_call(lib, h, d, st.cols_in(0, half), lib_rules(lib, k, 1, 0, 0, M), t1, keep=keep[:half]).error is None
                assert kmer_call(lib, h, d, st.cols_in(half, n - half), lib_rules(lib, k, 1, 0, 0, M_dst), t2, keep=keep[half:]).error is None
                before = t1.raw().tobytes()
                got = merge_call(lib, h, t1, t2)
                both = len(set(m1[0]) & set(m2[0]))
                assert got.error is None and got.stats == [len(m1[0]), len(m1[0]) - both, sum(m1[0].values()), 0, len(whole_m[0]), sum(whole_m[0].values()), 0, 0], got
                check_table(lib, h, d, t2, k, 1, whole_m[0], what=("merged", M_dst))
                assert t1.raw().tobytes() == before, "the source of a merge has been written"
            # growing: every pair into an empty table of twice the slots; twice more doubles every count
            big = Table(lib, d, 2 * M)
            assert kmer_call(lib, h, d, st.cols_in(3, 0), lib_rules(lib, k, 1, 0, 0, 2 * M), big).error is None
            got = merge_call(lib, h, tab, big)
            assert got.error is None and got.stats[:4] == [len(m2[0]), len(m2[0]), sum(m2[0].values()), 0]
            check_table(lib, h, d, big, k, 1, m2[0], what="grown")
            got = merge_call(lib, h, tab, big)
            assert got.error is None and got.stats[:4] == [len(m2[0]), 0, sum(m2[0].values()), 0]
            check_table(lib, h, d, big, k, 1, {x: 2 * c for x, c in m2[0].items()}, what="merged twice")
            # refusals of the merge: other k, other strand rule, itself, no table, too small
            other_k, other_c, raw, small = Table(lib, d, M), Table(lib, d, M), Table(lib, d, M), Table(lib, d, 16)
            assert kmer_call(lib, h, d, st.cols_in(0, half), lib_rules(lib, k + 1, 1, 0, 0, M), other_k).error is None
            assert kmer_call(lib, h, d, st.cols_in(0, half), lib_rules(lib, k, 0, 0, 0, M), other_c).error is None
            assert kmer_call(lib, h, d, st.cols_in(3, 0), lib_rules(lib, k, 1, 0, 0, 16), small).error is None
            for name, s_, d_ in (("k", tab, other_k), ("canonical", tab, other_c), ("itself", tab, tab), ("source no table", raw, tab), ("destination no table", tab, raw)):
                before = d_.raw().tobytes()
                got = merge_call(lib, h, s_, d_)
                assert got.error is not None and got.error.code == E_ARG and d_.raw().tobytes() == before, (name, got.error)
            before = small.raw().tobytes()
            got = merge_call(lib, h, tab, small)
            assert got.error is not None and got.error.code == E_CAPACITY and got.error.need == need_of(len(m2[0])) and small.raw().tobytes() == before
    finally:
        h.close()


# ---- hash_bits -------------------------------------------------------------------------------------------------------------------
def run_hash_bits(lib, sh):
    """hash_bits 1, 2 and 4 send every key down the same few probe chains: no pair and no statistic changes."""
    rng = np.random.default_rng(600)
    a, keep = pool_batch(rng, 48, 30, hi=34, keep_share=0.9)
    k = 12
    m = kmer_model_serial(a, k, 1, keep=keep)
    assert 200 <= len(m[0]) <= 700 and m[1][3] <= 768 and m[1][6] < m[1][4]      # M = 1024: the 3/4 rule holds and a walk may cover the whole table
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=2) as st:
            for bits in (1, 2, 4, 63, 64, 0):
                check_count(lib, h, st, k, 1, keep=keep, M=1024, hash_bits=bits, model=m, what=("hash_bits", bits))
            check_count(lib, h, st, k, 0, keep=keep, M=1024, hash_bits=1, what="hash_bits 1, forward")
    finally:
        h.close()


def run_forced_overflow(lib, sh):
    """hash_bits = 1 and M = 4096: two homes, so every walk stays inside slots 0 .. 1024 and at most 1025 keys find a slot -- 2 500
    distinct k-mers cannot.  The 16 000 windows come in ten calls of 1 600 that accumulate, so that distinct_before + W stays under
    3 M / 4 = 3072 in every call (one call of 16 000 windows would be refused by that rule).  Which keys are dropped depends on the
    order of arrival; that a key is either there with its exact count or wholly absent does not."""
    rng = np.random.default_rng(1400)
    k, M = 15, 4096
    pool = [rng.integers(0, 4, 63 + k).astype(np.uint8) for _ in range(40)]
    a = arrays([pool[i] for i in np.concatenate((np.arange(40), rng.integers(0, 40, 210)))])
    n, per = a.n_records, 25
    m = kmer_model(a, k, 1)
    reachable = 2 + PROBE_LIMIT - 1
    assert m[1][3] == 16000 and m[1][5] == 0 and len(m[0]) >= 2500 and len(m[0]) > reachable      # overflow MUST occur
    assert reachable + 64 * per <= M // 4 * 3                                                        # ... and no call is refused
    h = handle(lib)
    try:
        with staged(lib, h, a) as st, Dev(h) as d:
            tab = Table(lib, d, M)
            total = [0] * 16
            for c in range(n // per):
                got = kmer_call(lib, h, d, st.cols_in(c * per, per), lib_rules(lib, k, 1, int(c > 0), 1, M), tab)
                assert got.error is None, got.error
                assert got.stats[3] == 64 * per == got.stats[4] + got.stats[5] + got.stats[7]
                for i in (0, 3, 4, 5, 6, 7):
                    total[i] += got.stats[i]
                pairs, _ = tab.items()
                assert got.stats[8] == len(pairs) == total[6] and got.stats[9] == sum(pairs.values()) == total[4]
            pairs, used = tab.items()
            assert used == len(pairs) <= reachable and total[7] > 0
            assert all(m[0][x] == c for x, c in pairs.items())                                     # present means exact
            assert total[7] == m[1][3] - m[1][5] - sum(pairs.values())
            assert total[7] == sum(c for x, c in m[0].items() if x not in pairs)                   # ... and absent means wholly absent
            assert tab.raw()[:8].tolist() == [header_word(k, 1, 1), M, len(pairs), sum(pairs.values()), total[7], 0, 0, 0]
            keys = list(m[0])
            got, invalid = lookup(lib, h, d, tab, keys)
            assert invalid == 0 and got.tolist() == [pairs.get(x, 0) for x in keys]
            # a merge carries the lost occurrences along
            big = Table(lib, d, 2 * M)
            assert kmer_call(lib, h, d, st.cols_in(0, 0), lib_rules(lib, k, 1, 0, 0, 2 * M), big).error is None
            got = merge_call(lib, h, tab, big)
            assert got.error is None and got.stats[3] == 0
            check_table(lib, h, d, big, k, 1, pairs, overflow=total[7], what="overflow carried by the merge")
    finally:
        h.close()


# ---- spectrum and lookup ---------------------------------------------------------------------------------------------------------
def spectrum_model(table, n_bins):
    hist = [0] * n_bins
    for c in table.values():
        hist[min(c, n_bins - 1)] += 1
    return hist, [len(table), sum(table.values()), sum(1 for c in table.values() if c == 1), max(table.values(), default=0)]


def run_spectrum(lib, sh):
    rng = np.random.default_rng(1500)
    a, _ = pool_batch(rng, 400, 12, lo=30, hi=60)
    extra = arrays([np.full(700, 1, np.uint8), rng.integers(0, 4, 60).astype(np.uint8)])      # one key counted 693 times: beyond the bins a workgroup keeps in LDS; and keys counted once
    k = 8
    m1 = kmer_model(a, k, 1)
    m = kmer_model(extra, k, 1, table=m1[0])
    counts = sorted(set(m[0].values()))
    assert counts[0] == 1 and counts[-1] > 600 and len(counts) > 10 and any(256 <= c for c in counts)
    M = need_of(m1[1][3] + m[1][3])
    h = handle(lib)
    try:
        with staged(lib, h, a) as st, staged(lib, h, extra) as sx, Dev(h) as d:
            tab = Table(lib, d, M)
            assert kmer_call(lib, h, d, st.cols_in(), lib_rules(lib, k, 1, 0, 0, M), tab).error is None
            assert kmer_call(lib, h, d, sx.cols_in(), lib_rules(lib, k, 1, 1, 0, M), tab).error is None
            for n_bins in (2, 3, 5, 256, 257, 1000, 65536):
                ph = d.fill(8 * n_bins)
                totals = h.kmer_spectrum(tab.p, n_bins, ph)
                raw = d.down(ph, 8 * n_bins)
                assert raw[-8:] == b"\xA5" * 8
                want_hist, want_totals = spectrum_model(m[0], n_bins)
                assert np.frombuffer(raw[:-8], np.uint64).tolist() == want_hist and totals == want_totals, (n_bins, totals, want_totals)
                assert want_hist[0] == 0 and sum(want_hist) == len(m[0])
            assert spectrum_model(m[0], 2)[0] == [0, len(m[0])]
            ph = d.fill(8 * 16)
            for bad_table, n_bins in ((tab.p, 1), (tab.p, 0), (tab.p, 65537), (Table(lib, d, 16).p, 16), (None, 16)):
                try:
                    h.kmer_spectrum(bad_table, n_bins, ph)
                except lib.DsrcGpuError as e:
                    assert e.code == E_ARG
                else:
                    raise AssertionError(("no refusal", n_bins))
                assert d.down(ph, 8 * 16) == b"\xA5" * (8 * 16 + 8)
            empty = Table(lib, d, 16)
            assert kmer_call(lib, h, d, st.cols_in(0, 0), lib_rules(lib, k, 1, 0, 0, 16), empty).error is None
            assert h.kmer_spectrum(empty.p, 4, ph) == [0, 0, 0, 0] and d.down(ph, 32)[:32] == bytes(32)
    finally:
        h.close()


def run_lookup(lib, sh):
    rng = np.random.default_rng(1600)
    a, _ = pool_batch(rng, 80, 30, other=0.0)
    h = handle(lib)
    try:
        with staged(lib, h, a) as st, Dev(h) as d:
            for k in (3, 16, 31):
                mc, mf = kmer_model_serial(a, k, 1), kmer_model_serial(a, k, 0)
                M = need_of(mc[1][3])
                tc, tf = Table(lib, d, M), Table(lib, d, M)
                assert kmer_call(lib, h, d, st.cols_in(), lib_rules(lib, k, 1, 0, 0, M), tc).error is None
                assert kmer_call(lib, h, d, st.cols_in(), lib_rules(lib, k, 0, 0, 0, M), tf).error is None
                fwd = list(mf[0])                                # forward words as the reads hold them: many are NOT the canonical form
                assert sum(1 for x in fwd if revcomp_word(x, k) < x) > len(fwd) // 4
                absent = [int(v) for v in rng.integers(0, 4 ** k, 60) if key_of_word(int(v), k, 1) not in mc[0]]
                assert k == 3 or len(absent) > 50
                bad = [4 ** k, 4 ** k + 5, 2 ** 64 - 1, 2 ** 63] + ([] if k == 31 else [2 ** 62])
                q = fwd + absent + bad
                got, invalid = lookup(lib, h, d, tc, q)
                assert invalid == len(bad) and got.tolist() == [mc[0][key_of_word(x, k, 1)] for x in fwd] + [0] * (len(absent) + len(bad))
                got, invalid = lookup(lib, h, d, tf, q + [revcomp_word(x, k) for x in fwd])
                assert invalid == len(bad)
                assert got.tolist() == [mf[0][x] for x in fwd] + [mf[0].get(x, 0) for x in absent] + [0] * len(bad) + [mf[0].get(revcomp_word(x, k), 0) for x in fwd]
            assert h.kmer_lookup(tc.p, None, 0, None) == 0       # no queries
            po = d.fill(8 * 4)
            pq = d.up(np.zeros(4, np.uint64).tobytes())
            for bad_args in ((Table(lib, d, 16).p, pq, 4, po), (None, pq, 4, po), (tc.p, None, 4, po), (tc.p, pq, 4, None)):
                try:
                    h.kmer_lookup(*bad_args)
                except lib.DsrcGpuError as e:
                    assert e.code == E_ARG
                else:
                    raise AssertionError("no refusal")
                assert d.down(po, 32) == b"\xA5" * 40
    finally:
        h.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def run_arg_refusals(lib, sh):
    rng = np.random.default_rng(1000)
    a, _ = pool_batch(rng, 40, 9)
    n, k = a.n_records, 7
    u64 = lambda v: np.asarray(v).astype(np.uint64)
    S0, S1 = whole(a)
    m = kmer_model_serial(a, k, 1)
    M = 2 * need_of(m[1][3])                                   # 3 M / 4 >= 3 W: the batch fits twice, whatever it holds
    h = handle(lib)
    try:
        with staged(lib, h, a) as st, Dev(h) as d:
            cin = st.cols_in()
            fresh = Table(lib, d, M)
            checked = 0

            def refused(got, name, tab=fresh, code=E_ARG):
                assert got.error is not None and got.error.code == code and tab.untouched(), (name, got.error)
                return 1
            R = lambda **kw: lib_rules(lib, **dict(dict(k=k, capacity=M), **kw))
            for name, kr in [("k 0", R(k=0)), ("k 32", R(k=32)), ("canonical 2", R(canonical=2)), ("accumulate 2", R(accumulate=2)), ("hash_bits 65", R(hash_bits=65)),
                             ("capacity 0", R(capacity=0)), ("capacity 8", R(capacity=8)), ("capacity 24", R(capacity=24)), ("capacity 2^41", R(capacity=2 ** 41)),
                             ("capacity 2^40 + 16", R(capacity=2 ** 40 + 16))] + [("reserved[%d]" % i, R(reserved=tuple(int(j == i) for j in range(4)))) for i in range(4)]:
                checked += refused(kmer_call(lib, h, d, cin, kr, fresh), name)
            checked += refused(kmer_call(lib, h, d, cin, R(), fresh, begin=u64(S0)), "begin alone")
            checked += refused(kmer_call(lib, h, d, cin, R(), fresh, end=u64(S1)), "end alone")
            checked += refused(kmer_call(lib, h, d, cin, R(), fresh, null_table=True), "null table")
            checked += refused(kmer_call(lib, h, d, cin, R(accumulate=1), fresh), "accumulate into memory that is no table")
            assert checked == 14 + 4
            C = lib.C
            stats, need = (C.c_uint64 * 16)(), (C.c_uint64 * 1)()
            for args in ((None, C.byref(R()), C.c_void_p(fresh.p), stats, need), (C.byref(cin), None, C.c_void_p(fresh.p), stats, need),
                         (C.byref(cin), C.byref(R()), C.c_void_p(fresh.p), None, need), (C.byref(cin), C.byref(R()), C.c_void_p(fresh.p), stats, None)):
                rc = h.L.dsrcgpu_columns_kmer_count(h.h, args[0], None, None, None, *args[1:])
                assert rc == E_ARG and fresh.untouched()
            assert h.L.dsrcgpu_kmer_table_merge(h.h, C.c_void_p(fresh.p), C.c_void_p(fresh.p), None, need) == E_ARG
            # accumulate: the header must match k, canonical, hash_bits and capacity -- the table stays as it is
            tab = Table(lib, d, M)
            assert kmer_call(lib, h, d, cin, R(), tab).error is None
            before = tab.raw().tobytes()
            for name, kr in (("k", R(k=k + 1, accumulate=1)), ("canonical", R(canonical=0, accumulate=1)), ("capacity", R(capacity=M // 2, accumulate=1)),
                             ("capacity up", R(capacity=2 * M, accumulate=1)), ("hash_bits", R(hash_bits=3, accumulate=1))):
                got = kmer_call(lib, h, d, cin, kr, tab)
                assert got.error is not None and got.error.code == E_ARG and tab.raw().tobytes() == before, (name, got.error)
            got = kmer_call(lib, h, d, cin, R(accumulate=1, hash_bits=64), tab)       # 64 and 0 are one and the same
            assert got.error is None
            check_table(lib, h, d, tab, k, 1, {x: 2 * c for x, c in m[0].items()}, what="the same handle, clean")
            # E_CAPACITY: need comes back, the table is still 0xA5; on a table in use it stays as it is
            W = m[1][3]
            small = need_of(W) // 4
            assert W > small // 4 * 3 and small >= 16
            got = kmer_call(lib, h, d, cin, R(capacity=small), fresh)
            refused(got, "capacity", code=E_CAPACITY)
            assert got.error.need == need_of(W)
            exact = Table(lib, d, need_of(W))
            assert kmer_call(lib, h, d, cin, R(capacity=need_of(W)), exact).error is None
            # the bound itself: M = 16 holds 12 windows, not 13; and what the table holds already counts
            one = arrays([np.arange(12 + k - 1, dtype=np.uint8) % 4, np.arange(13 + k - 1, dtype=np.uint8) % 4])
            distinct = len(kmer_model_serial(one, k, 1, first=0, n=1)[0])
            assert 1 <= distinct <= 4
            with staged(lib, h, one) as s1:
                t16 = Table(lib, d, 16)
                got = kmer_call(lib, h, d, s1.cols_in(1, 1), R(capacity=16), t16)
                assert got.error is not None and got.error.code == E_CAPACITY and got.error.need == 32 and t16.untouched()
                assert kmer_call(lib, h, d, s1.cols_in(0, 1), R(capacity=16), t16).error is None
                before = t16.raw().tobytes()
                got = kmer_call(lib, h, d, s1.cols_in(0, 1), R(capacity=16, accumulate=1), t16)
                assert got.error is not None and got.error.code == E_CAPACITY and got.error.need == need_of(distinct + 12) == 32 and t16.raw().tobytes() == before
    finally:
        h.close()
    hc = ce.handle(lib, dataclasses.replace(Config.from_levels(0, 0), color_space=True))
    try:
        with staged(lib, hc, a) as st, Dev(hc) as d:
            tab = Table(lib, d, M)
            got = kmer_call(lib, hc, d, st.cols_in(), lib_rules(lib, k, 1, 0, 0, M), tab)
            assert got.error is not None and got.error.code == E_ARG and tab.untouched()
    finally:
        hc.close()


def run_input_errors(lib, sh):
    """The plants of the profile's input errors in the first, a middle and the last record, considered and dropped ones, into a
    fresh table and into one in use: code, the lowest record, the table as it was, and the same handle counts the clean arrays."""
    rng = np.random.default_rng(1100)
    a, _ = pool_batch(rng, 41, 9)
    n, k, M, pad = a.n_records, 6, 4096, 4
    keep = np.ones(n, np.uint8); keep[[20, 40]] = 0
    S = lambda r: int(a.seq_offsets[r]) + pad
    S0, S1 = whole(a)
    hb, he = (S0 + pad).astype(np.uint64), (S1 + pad).astype(np.uint64)
    h = handle(lib)
    checked = 0
    try:
        with staged(lib, h, a, pad=pad) as st, Dev(h) as d:
            fresh, used = Table(lib, d, M), Table(lib, d, M)
            assert kmer_call(lib, h, d, st.cols_in(0, 10), lib_rules(lib, k, 1, 0, 0, M), used).error is None
            before = used.raw().tobytes()

            def refused(r, word, name, plan):
                for tab, acc in ((fresh, 0), (used, 1)):
                    got = kmer_call(lib, h, d, st.cols_in(), lib_rules(lib, k, 1, acc, 0, M), tab, *plan)
                    assert got.error is not None and got.error.code == E_INPUT, (name, r, got.error)
                    assert "record %d:" % r in str(got.error) and word in str(got.error), (name, r, str(got.error))
                assert fresh.untouched() and used.raw().tobytes() == before, (name, r)
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
                check_count(lib, h, st, k, 1, keep=keep, what=("after", name))
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
                check_count(lib, h, st, k, 1, S0, S1, keep, pad=pad, what=("after", name))
    finally:
        h.close()
    assert checked == 21


def run_codec_state(lib, sh):
    """The calls touch nothing the codec carries, as run_codec_state of the other planners: the fields capacity stays, a pending
    record layout stays pending, and the text call that follows writes what it writes on a fresh handle seeded alike."""
    a, keep = pool_batch(np.random.default_rng(1200), 60, 11, keep_share=0.9)
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
                m = check_count(lib, h, st, 9, 1, keep=keep)
                t1, t2 = Table(lib, d, 4096), Table(lib, d, 8192)
                for t in (t1, t2):
                    assert kmer_call(lib, h, d, st.cols_in(), lib_rules(lib, 9, 1, 0, 0, t.M), t, keep=keep).error is None
                assert merge_call(lib, h, t1, t2).error is None
                ph = d.fill(8 * 8)
                assert h.kmer_spectrum(t2.p, 8, ph)[:2] == [len(m[0]), 2 * sum(m[0].values())]
                lookup(lib, h, d, t2, list(m[0])[:5])
                assert h.get_fields_capacity() == 11
            assert text_blocks(h) == text_blocks(fresh), layout
        finally:
            h.close(); fresh.close()


# ---- fuzz ------------------------------------------------------------------------------------------------------------------------
def fuzz_batch(seed, n, k=None):
    """n reads of 0 .. 2 k + 170 codes, one in 60 not a base (N, IUPAC, U, 255), a third of them copies of an earlier read or of its
    reverse complement, poly-G tails on some; ranges that cut up to 5 bases off either end, a keep that drops one record in ten."""
    rng = np.random.default_rng(5000 + seed)
    other = np.array([4, 4, 255, 7, 16], np.uint8)
    reads = []
    for r in range(n):
        u = rng.random()
        if r and u < 0.2:
            x = reads[int(rng.integers(0, r))].copy()
        elif r and u < 0.33:
            y = reads[int(rng.integers(0, r))]
            x = np.where(y < 4, 3 - y, y)[::-1].astype(np.uint8)
        else:
            x = rng.integers(0, 4, int(rng.integers(0, 2 * (k or 21) + 171))).astype(np.uint8)
            amb = rng.random(len(x)) < 1 / 60
            x[amb] = other[rng.integers(0, 5, int(amb.sum()))]
            if rng.random() < 0.15 and len(x) > 30:
                x[len(x) - int(rng.integers(1, 90)):] = 2
        reads.append(x)
    a = arrays(reads)
    S0, S1 = whole(a)
    lens = S1 - S0
    cut5 = np.minimum(np.where(rng.random(n) < 0.6, 0, rng.integers(0, 6, n)), lens)
    cut3 = np.minimum(np.where(rng.random(n) < 0.6, 0, rng.integers(0, 6, n)), lens - cut5)
    keep = (rng.random(n) < 0.9).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
    return a, S0 + cut5, S1 - cut3, keep


def run_fuzz(lib, sh, seed):
    n = sh["kmer_fuzz"][1]
    k = KS[seed % len(KS)] if seed % 2 else [21, 31, 11][seed // 2 % 3]
    canonical = 0 if seed % 3 == 2 else 1
    a, begin, end, keep = fuzz_batch(seed, n, k)
    m = kmer_model(a, k, canonical, begin, end, keep)
    print("kmer fuzz", seed, "records", n, "k", k, "canonical", canonical, "stats", m[1][:10])
    assert m[1][4] > 20 * m[1][0] and m[1][5] > m[1][0] // 2 and m[1][1] > 0 and m[1][9] > len(m[0])      # the model alone: hits, broken windows, repeats
    h = handle(lib)
    try:
        with staged(lib, h, a, pad=3) as st:
            check_count(lib, h, st, k, canonical, begin, end, keep, pad=3, model=m, what=("fuzz", seed))
            check_count(lib, h, st, k, 1 - canonical, what=("fuzz, whole reads, the other strand rule", seed))
    finally:
        h.close()


# ---- the Python layers and the closed loop ---------------------------------------------------------------------------------------------
def table_dict(t):
    keys, counts = t.items()
    assert keys.dtype == torch.int64 and counts.dtype == torch.int64 and (keys[1:] > keys[:-1]).all()
    return dict(zip(keys.tolist(), counts.tolist()))


def run_python_layers(lib, sh, device):
    from dsrc_amd import columns
    a, begin, end, keep = fuzz_batch(3, 90, 21)
    n = a.n_records
    t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v).astype(dt)).to(device)
    dev = torch.device(device).type
    h = handle(lib)
    try:
        assert tuple(lib.KMER_STATS) == KMER_STATS and lib.KMER_PROBE_LIMIT == PROBE_LIMIT and lib.kmer_words(64) == 136 and lib.KMER_EMPTY == EMPTY
        c = tensors(a, device)
        tb, te, tk = t(begin, np.int64), t(end, np.int64), t(keep, np.uint8)
        # sizing
        m = kmer_model(a, 21, 1, begin, end, keep)
        tab, stats = columns.count_kmers(h, c, 21, tb, te, tk)
        assert list(stats) == list(KMER_STATS) and list(stats.values()) == m[1][:10]
        assert isinstance(tab, columns.KmerTable) and tab.data.dtype == torch.int64 and tab.data.device.type == dev and tab.capacity == need_of(m[1][3])
        assert (tab.k, tab.canonical) == (21, True) and tab.keys.numel() == tab.counts.numel() == tab.capacity
        assert table_dict(tab) == m[0]
        assert tab.summary() == dict(k=21, canonical=True, capacity=tab.capacity, distinct=len(m[0]), occurrences=sum(m[0].values()), overflow=0)
        assert torch.equal(tk, t(keep, np.uint8)) and torch.equal(tb, t(begin, np.int64))      # inputs as they were
        # a given capacity; one that is too small
        mf = kmer_model(a, 21, 0)
        tab_f, stats_f = columns.count_kmers(h, c, 21, canonical=False, capacity=2 * need_of(mf[1][3]))
        assert tab_f.capacity == 2 * need_of(mf[1][3]) and table_dict(tab_f) == mf[0] and list(stats_f.values()) == mf[1][:10]
        try:
            columns.count_kmers(h, c, 21, capacity=64)
        except lib.DsrcGpuError as e:
            assert e.code == E_CAPACITY and e.need == need_of(kmer_model(a, 21, 1)[1][3])
        else:
            raise AssertionError("no E_CAPACITY")
        # into, with automatic growth: a table sized for the first twenty records takes the rest
        first, _ = columns.count_kmers(h, tensors_slice(a, 0, 20, device), 21, tb[:20], te[:20], tk[:20])
        small = first.capacity
        m20 = kmer_model(a, 21, 1, begin[:20], end[:20], keep[:20], 0, 20)
        assert table_dict(first) == m20[0]
        rest = tensors_slice(a, 20, n - 20, device)
        shift = int(a.seq_offsets[20])
        again, stats2 = columns.count_kmers(h, rest, 21, tb[20:] - shift, te[20:] - shift, tk[20:], into=first)
        assert again is first and first.capacity > small and table_dict(first) == m[0]
        assert stats2["distinct_after"] == len(m[0]) and stats2["total_after"] == sum(m[0].values()) and stats2["overflow"] == 0
        assert first.capacity == need_of(len(m20[0]) + stats2["windows"])
        # items, top, spectrum, lookup, merged_into, grown
        order = sorted(m[0].items(), key=lambda kv: (-kv[1], kv[0]))
        for want in (0, 1, 7, len(order), len(order) + 5):
            top = tab.top(want)
            assert top == [(columns.unpack_kmer(x, 21), cnt) for x, cnt in order[:want]], want
        hist, totals = tab.spectrum(h, 6)
        assert hist.dtype == torch.int64 and hist.device.type == dev and (hist.tolist(), list(totals.values())) == spectrum_model(m[0], 6)
        assert tab.spectrum(h)[0].numel() == 256
        some = [x for x, _ in order[:5]]
        strs = [columns.unpack_kmer(x, 21) for x in some]
        assert columns.pack_kmers(strs, 21) == some and columns.pack_kmers(["acgtacgtacgtacgtacgta"], 21) == [pack([0, 1, 2, 3] * 5 + [0])]
        assert tab.lookup(h, strs).tolist() == [m[0][x] for x in some]
        rc_strs = [columns.unpack_kmer(revcomp_word(x, 21), 21) for x in some]
        assert tab.lookup(h, rc_strs).tolist() == [m[0][x] for x in some]
        got, invalid = tab.lookup(h, torch.tensor(some + [4 ** 21, -1], dtype=torch.int64, device=device), return_invalid=True)
        assert got.tolist() == [m[0][x] for x in some] + [0, 0] and invalid == 2
        assert tab.lookup(h, []).numel() == 0
        grown = tab.grown(h, 4 * tab.capacity)
        assert grown.capacity == 4 * tab.capacity and table_dict(grown) == m[0] and table_dict(tab) == m[0] and grown.summary()["distinct"] == len(m[0])
        tiny = columns.KmerTable.empty(h, 21, True, 16, device)
        assert tiny.summary()["distinct"] == 0 and tab.merged_into(h, tiny) is tiny and tiny.capacity == need_of(len(m[0])) and table_dict(tiny) == m[0]
        assert table_dict(tab.merged_into(h, tiny)) == {x: 2 * cnt for x, cnt in m[0].items()}

        class Never:                                         # ValueError comes before any library call
            def __getattr__(self, name):
                raise AssertionError("the library was called")
        bad_calls = [dict(k=0), dict(k=32), dict(k=21.0), dict(k=True), dict(k=21, begin=tb), dict(k=21, end=te), dict(k=21, begin=tb[:5], end=te[:5]),
                     dict(k=21, keep=tk[:7]), dict(k=21, capacity=24), dict(k=21, capacity=8), dict(k=21, capacity=2 ** 41), dict(k=21, into=tab_f),
                     dict(k=20, into=tab), dict(k=21, into=tab, capacity=2 * tab.capacity), dict(k=21, into="table")]
        calls = [lambda bad=bad: columns.count_kmers(Never(), c, **bad) for bad in bad_calls]
        calls += [lambda: columns.filter_columns(Never(), c, kmers=0), lambda: columns.filter_columns(Never(), c, kmers=32), lambda: columns.filter_columns(Never(), c, kmers="21"),
                  lambda: columns.filter_pairs(Never(), c, c, kmers=40), lambda: tab.spectrum(Never(), 1), lambda: tab.spectrum(Never(), 65537),
                  lambda: tab.lookup(Never(), ["ACGT"]), lambda: tab.lookup(Never(), ["ACGTNACGTACGTACGTACGT"]), lambda: tab.lookup(Never(), torch.zeros(3, dtype=torch.int32, device=device)),
                  lambda: tab.merged_into(Never(), tab), lambda: tab.merged_into(Never(), tab_f), lambda: tab.grown(Never(), 100), lambda: tab.top(-1)]
        if dev != "cpu":                                     # a table on another device
            calls.append(lambda: columns.count_kmers(Never(), c, 21, into=columns.KmerTable(tab.data.cpu(), 21, True)))
        for i, call in enumerate(calls):
            try:
                call()
            except ValueError:
                pass
            else:
                raise AssertionError("no ValueError for call %d" % i)
    finally:
        h.close()


def tensors_slice(a, first, n, device):
    """Records first .. first + n - 1 of `a` as columns of their own (offsets from 0)."""
    S, T = a.seq_offsets.astype(np.int64), a.title_offsets.astype(np.int64)
    sub = ce.Arrays(a.bases[S[first]: S[first + n]], a.quals[S[first]: S[first + n]], a.titles[T[first]: T[first + n]],
                    (S[first: first + n + 1] - S[first]).astype(np.uint64), (T[first: first + n + 1] - T[first]).astype(np.uint64), [0, n])
    return tensors(sub, device)


def run_filters(lib, sh, device):
    """filter_columns(kmers=21): the table of the final plan; filter_pairs(kmers=21): both sides in one table == the two-call form.
    The default leaves both functions as they are."""
    from dsrc_amd import columns
    from tests import columns_dedup_cases as cd
    (a1, _, _), (a2, _, _) = cd.duplicated_reads(120, 41, pairs=True)
    trim = cs.rules_of(0, 20, min_length=30, max_n=1)
    h = handle(lib)
    try:
        c1, c2 = tensors(a1, device), tensors(a2, device)
        b, e, k, ts = cs.plan_model(a1, trim)
        m = kmer_model(a1, 21, 1, b, e, k)
        plain, plain_stats = columns.filter_columns(h, c1, **trim)
        again, again_stats = columns.filter_columns(h, c1, kmers=None, **trim)
        assert plain_stats == again_stats == dict(zip(ca.TRIM_STATS, ts)) and cd.same_columns(again, cs.select_model(a1, b, e, k))
        out, stats = columns.filter_columns(h, c1, kmers=21, **trim)
        tab = stats.pop("kmers_after")
        assert stats == plain_stats and cd.same_columns(out, cs.select_model(a1, b, e, k))
        assert table_dict(tab) == m[0] and m[1][1] > 0 and m[1][5] > 0
        assert table_dict(columns.count_kmers(h, out, 21)[0]) == m[0]                   # the table of the plan IS the table of the records that come out
        out, stats = columns.filter_columns(h, c1, kmers=21, dedup=True, profile=True, **trim)
        md = cd.dedup_model(a1, r1=(b, e), keep=k)
        assert table_dict(stats["kmers_after"]) == kmer_model(a1, 21, 1, b, e, md[0])[0] and list(stats)[-1] == "kmers_after"
        # pairs
        kw = dict(pair_min_overlap=20, pair_max_mismatches=4, pair_max_error_permille=150)
        p1, p2, pstats = columns.filter_pairs(h, c1, c2, **kw, **trim)
        o1, o2, ostats = columns.filter_pairs(h, c1, c2, kmers=21, **kw, **trim)
        tab = ostats.pop("kmers_after")
        assert ostats == pstats and torch.equal(o1.bases, p1.bases) and torch.equal(o2.bases, p2.bases) and torch.equal(o1.seq_offsets, p1.seq_offsets)
        r1, r2, keep, _ = cp.pairs_model(a1, a2, trim, (None, None), True, cp.rules_of(20, 4, 150))
        ma = kmer_model(a1, 21, 1, r1[0], r1[1], keep)
        mb = kmer_model(a2, 21, 1, r2[0], r2[1], keep, table=ma[0])
        assert table_dict(tab) == mb[0] and len(mb[0]) > len(ma[0])
        two, _ = columns.count_kmers(h, o1, 21)
        two, _ = columns.count_kmers(h, o2, 21, into=two)
        assert table_dict(two) == mb[0] and two.summary()["occurrences"] == tab.summary()["occurrences"]
        assert any(c > ma[0].get(x, 0) > 0 for x, c in mb[0].items())                   # read-through pairs: the mates share k-mers, on opposite strands
    finally:
        h.close()


def run_closed_loop(lib, sh, device):
    """Records written here -> the oracle's block -> decode_columns -> count_kmers: the table is the model's on the arrays of that text."""
    from dsrc_amd import columns
    from tests import columns_dedup_cases as cd
    cfg = ce.BLOCK_CFG
    (a, recs, text), = cd.duplicated_reads(150, 61)
    m = kmer_model(a, 17, 1)
    assert m[1][5] > 0 and m[1][9] > 2 * len(m[0])
    src = ce.oracle_blocks(cfg, [text])
    assert src is not None
    h = ce.handle(lib, cfg)
    try:
        d_blocks, offs = cs._stage_blocks([src[0][0]], device)
        rc = columns.decode_columns(h, d_blocks, offs, [len(src[0][0])], device)
        assert rc.n_records == 150
        tab, stats = columns.count_kmers(h, rc, 17)
        assert list(stats.values()) == m[1][:10] and table_dict(tab) == m[0]
        hist, totals = tab.spectrum(h, 64)
        assert (hist.tolist(), list(totals.values())) == spectrum_model(m[0], 64)
    finally:
        h.close()
