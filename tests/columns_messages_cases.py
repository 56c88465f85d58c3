"""The exact text of dsrcgpu_last_error for the refusals of the columnar entry points (dsrc_amd/csrc/host_columns.h).

The per-feature cases check a refusal by its return code, by "nothing written" and here and there by a substring; what the message
says word for word is pinned here: every case is one small call (20 pairs of reads) through the helpers of the per-feature cases
files, its return code and message are compared for equality with tests/golden/columns_messages_golden.json, which
tests/golden/make_columns_messages_golden.py recorded from the library as it stood before the host layer was rewritten.  A case
runs once per entry point that can reach its message: parameter names and prefixes differ from call to call.  A variant that an
entry point does NOT refuse (titles or qualities it can do without) is recorded as [0, ""].

Covered: null `in`, a colour-space handle, lengths of 2^56, null offset arrays, null arrays with a length, one end of a range
without the other, every reserved field of every rules struct, null output arrays, the five device-found input errors through the
one-sided calls and through either side of the two-sided ones, the capacity refusals of select, merge and the k-mer count, and
"not a k-mer table".  Left out: "arena exhausted (...)" (needs a device without memory) and "batches of the queue form are still
in flight on this handle" (needs a batch of the queue form held in flight)."""
from __future__ import annotations

import contextlib
import dataclasses
import functools
import json
import os

import numpy as np
import torch        # noqa: F401  before the first handle (see columns_cases)

from tests import columns_adapt_cases as ca
from tests import columns_dedup_cases as cd
from tests import columns_enc_cases as ce
from tests import columns_kmer_cases as ck
from tests import columns_kmer_plan_cases as kp
from tests import columns_merge_cases as cm
from tests import columns_pair_cases as cp
from tests import columns_profile_cases as cf
from tests import columns_sel_cases as cs
from tests._oracle import Config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "columns_messages_golden.json")
N_PAIRS = 20
K = 5                                                        # the k of the k-mer calls
NO_PLAN = (None, None, None)


@functools.lru_cache(maxsize=None)
def scene():
    """20 pairs of reads with ranges, keep flags and insert sizes, and what the merge makes of them: shared by every case, never written."""
    a1, a2, rg1, rg2, keep, insert = cm.build(cm.small_set(np.random.default_rng(2000), N_PAIRS))
    merged = cm.merge_model(a1, a2, cm.rules_of(), rg1, rg2, keep, insert).totals
    assert merged[0] >= 2 and keep.sum() >= 2
    return a1, a2, rg1 + (keep,), rg2 + (keep,), insert, merged


@contextlib.contextmanager
def null_struct(lib, obj):
    """Within: the helpers pass NULL where they would pass the address of `obj` (they take a struct, never none at all)."""
    real = lib.C.byref
    lib.C.byref = lambda x, *more: None if x is obj else real(x, *more)
    try:
        yield
    finally:
        lib.C.byref = real


def cin_with(lib, c, **fields):
    return lib.ColumnsIn(**dict({name: getattr(c, name) for name, _ in c._fields_}, **fields))


def error_of(lib, call):
    try:
        call()
        return None
    except lib.DsrcGpuError as e:
        return e


@dataclasses.dataclass
class Entry:
    call: object            # (cin1, cin2, plan1, plan2, reserved) -> the DsrcGpuError or None
    sides: int = 1
    plans: int = 1          # sides that take a plan (d_begin / d_end / d_keep)
    reserved: int = 0       # reserved fields of the rules
    needs: tuple = ()       # of "titles", "quals": what the call cannot do without, side 1 (side 2 never needs titles)


class Calls:
    """The entry points on one handle, each as Entry.call over the helpers of the per-feature cases."""

    def __init__(self, lib, h, d, st1, st2, table):
        a1, a2, p1, p2, insert, merged = scene()
        n = a1.n_records
        S, T = len(a1.bases) + len(a2.bases), len(a1.titles)
        up = lambda v, dt: None if v is None else d.up(np.ascontiguousarray(v).astype(dt).tobytes())
        ups = lambda plan: (up(plan[0], np.uint64), up(plan[1], np.uint64), up(plan[2], np.uint8))
        res = lambda reserved, count: reserved or (0,) * count
        adapter = ca.rules_of([np.array([0, 1, 2, 3, 0, 1, 2, 3], np.uint8)])
        self.h, self.d, self.st = h, d, (st1, st2)

        def select(titles):
            return lambda c1, c2, q1, q2, r: cs.SelCall(lib, h, c1, *ups(q1), n, S, T, titles).error

        def dedup(prefer):
            return lambda c1, c2, q1, q2, r: cd.dedup_call(lib, h, c1, c2, n, cd.lib_rules(lib, 0, prefer, 0, res(r, 5)), q1[:2], q2[:2], q1[2]).error

        def merge(titles):
            return lambda c1, c2, q1, q2, r: cm.MergeCall(lib, h, c1, c2, n, cm.lib_rules(lib, cm.rules_of(), res(r, 4)), q1[:2], q2[:2], q1[2], insert,
                                                          merged[0], merged[1], merged[2], titles).error
        self.entries = {
            "compress_columns_device": Entry(lambda c1, c2, q1, q2, r: error_of(lib, lambda: h.compress_columns_device(c1, [0, n], st1.ptr["out"], st1.out_cap)),
                                             plans=0, needs=("titles", "quals")),
            "columns_cut": Entry(lambda c1, c2, q1, q2, r: error_of(lib, lambda: h.columns_cut(c1, 1 << 20, 4)), plans=0, needs=("titles", "quals")),
            "trim_plan": Entry(lambda c1, c2, q1, q2, r: cs.plan_call(lib, h, c1, cs.rules_of(20, 20), n, res(r, 3))[0], plans=0, reserved=3, needs=("quals",)),
            "select_device": Entry(select(True), needs=("titles", "quals")),
            "select_device, no titles": Entry(select(False), needs=("quals",)),
            "adapter_plan": Entry(lambda c1, c2, q1, q2, r: ca.adapt_call(lib, h, c1, n, ca.lib_rules(lib, adapter, res(r, 3)), q1).error, reserved=3),
            "pair_plan": Entry(lambda c1, c2, q1, q2, r: cp.pair_call(lib, h, c1, c2, n, cp.lib_rules(lib, cp.rules_of(), res(r, 4)), q1, q2).error,
                               sides=2, plans=2, reserved=4),
            "dedup_plan": Entry(dedup(0), sides=2, plans=2, reserved=5),
            "dedup_plan, one side, prefer quality": Entry(lambda c1, c2, q1, q2, r: dedup(1)(c1, None, q1, NO_PLAN, r), needs=("quals",)),
            "merge_device": Entry(merge(True), sides=2, plans=2, reserved=4, needs=("titles", "quals")),
            "merge_device, no titles": Entry(merge(False), sides=2, plans=2, needs=("quals",)),
            "profile": Entry(lambda c1, c2, q1, q2, r: cf.prof_call(lib, h, c1, 8, q1, reserved=res(r, 6)).error, reserved=6, needs=("quals",)),
            "kmer_count": Entry(lambda c1, c2, q1, q2, r: ck.kmer_call(lib, h, d, c1, ck.lib_rules(lib, K, capacity=table.M, reserved=res(r, 4)), table, *q1).error,
                                reserved=4),
            "kmer_plan": Entry(lambda c1, c2, q1, q2, r: kp.plan_call(lib, h, d, c1, n, kp.rules_of(), table.p, *q1, reserved=res(r, 4)).error, reserved=4),
        }

    def run(self, name, cin=(None, None), plan=None, reserved=None):
        """One call: the staged arrays and the scene's plans unless told otherwise."""
        st1, st2 = self.st
        plan = plan or scene()[2:4]
        return self.entries[name].call(cin[0] or st1.cols_in(), cin[1] or st2.cols_in(), plan[0], plan[1], reserved)


def collect(lib):
    """Every case -> {name: [return code, message]}."""
    a1, a2, p1, p2, insert, merged = scene()
    A, P = (a1, a2), (p1, p2)
    n = a1.n_records
    out = {}
    h = cp.handle(lib)

    def note(name, handle, err):
        assert name not in out, name
        out[name] = [0, ""] if err is None else [err.code, handle.L.dsrcgpu_last_error(handle.h).decode()]

    def two(side, value, other=None):
        return (value, other) if side == 0 else (other, value)
    try:
        with cp.staged(lib, h, a1) as st1, cp.staged(lib, h, a2) as st2, cs.Dev(h) as d:
            table = ck.Table(lib, d, 1 << 14)
            calls = Calls(lib, h, d, st1, st2, table)
            st = (st1, st2)
            error = calls.run("kmer_count")                  # (fills the table that kmer_plan reads)
            assert error is None, error
            for name, e in calls.entries.items():
                sides = range(e.sides)
                # ---- the arguments ----
                for s in sides:
                    cin = st[s].cols_in()
                    with null_struct(lib, cin):
                        note("%s: in%d null" % (name, s + 1), h, calls.run(name, cin=two(s, cin)))
                    # (what, the field, the array the field belongs to where a call may do without it: titles on side 1 only)
                    variants = [("n_records of 2^56", dict(n_records=1 << 56), None), ("bases_len of 2^56", dict(bases_len=1 << 56), None),
                                ("titles_len of 2^56", dict(titles_len=1 << 56), "titles"), ("d_seq_offs null", dict(d_seq_offs=None), None),
                                ("d_title_offs null", dict(d_title_offs=None), "titles"), ("d_bases null", dict(d_bases=None), None),
                                ("d_quals null", dict(d_quals=None), "quals"), ("d_titles null", dict(d_titles=None), "titles")]
                    for what, fields, array in variants:
                        err = calls.run(name, cin=two(s, cin_with(lib, cin, **fields)))
                        refused = array is None or (array in e.needs and (array == "quals" or s == 0))
                        assert (err is not None) == refused, (name, s, what, err)
                        note("%s: in%d %s" % (name, s + 1, what), h, err)
                for s in range(e.plans):
                    note("%s: begin of side %d alone" % (name, s + 1), h, calls.run(name, plan=two(s, (P[s][0], None, None), NO_PLAN)))
                    note("%s: end of side %d alone" % (name, s + 1), h, calls.run(name, plan=two(s, (None, P[s][1], None), NO_PLAN)))
                for k in range(e.reserved):
                    note("%s: reserved[%d]" % (name, k), h, calls.run(name, reserved=tuple(int(i == k) for i in range(e.reserved))))
                # ---- what the device finds: record 3 (the last record for an offset above bases_len) ----
                r = 3
                for s in sides:
                    S_ = [int(v) for v in A[s].seq_offsets]
                    offsets = [("seq_offs decrease", r + 1, S_[r] - 1), ("seq_offs above bases_len", n, len(A[s].bases) + 5)]
                    for what, index, value in offsets:
                        st[s].poke("seq_offs", index, value, np.uint64)
                        note("%s: side %d %s" % (name, s + 1, what), h, calls.run(name))
                        st[s].restore()
                    if s >= e.plans:
                        continue
                    ranges = [("begin low", dict(b=S_[r] - 1)), ("end high", dict(e=S_[r + 1] + 1)), ("begin above end", dict(b=S_[r + 1], e=S_[r + 1] - 1))]
                    for what, how in ranges:
                        b, e_, keep = P[s][0].copy(), P[s][1].copy(), np.ones(n, np.uint8)
                        b[r], e_[r] = how.get("b", b[r]), how.get("e", e_[r])
                        note("%s: side %d %s" % (name, s + 1, what), h, calls.run(name, plan=two(s, (b, e_, keep), P[1 - s])))

            # ---- capacities, null outputs ----
            pb, pe, pk = (d.up(p1[0].tobytes()), d.up(p1[1].tobytes()), d.up(p1[2].tobytes()))
            kept = int(p1[2].sum())
            sel = lambda **kw: cs.SelCall(lib, h, st1.cols_in(), pb, pe, pk, n, len(a1.bases), len(a1.titles), **kw).error
            note("select_device: capacities of 0", h, sel(caps=dict(bases_cap=0, quals_cap=0, titles_cap=0, records_cap=0)))
            note("select_device: records_cap one short", h, sel(caps=dict(records_cap=kept - 1)))
            note("select_device, no titles: capacities of 0", h, sel(titles=False, caps=dict(bases_cap=0, quals_cap=0, records_cap=0)))
            mrg = lambda **kw: cm.MergeCall(lib, h, st1.cols_in(), st2.cols_in(), n, cm.lib_rules(lib, cm.rules_of()), p1[:2], p2[:2], p1[2], insert, *merged, **kw).error
            note("merge_device: capacities of 0", h, mrg(caps=dict(bases_cap=0, quals_cap=0, titles_cap=0, records_cap=0)))
            note("merge_device: records_cap one short", h, mrg(caps=dict(records_cap=merged[0] - 1)))
            note("merge_device, no titles: capacities of 0", h, mrg(titles=False, caps=dict(bases_cap=0, quals_cap=0, records_cap=0)))
            small = ck.Table(lib, d, 16)
            note("kmer_count: capacity of 16", h, ck.kmer_call(lib, h, d, st1.cols_in(), ck.lib_rules(lib, K, capacity=16), small).error)
            assert small.untouched()
            buf = {k: d.fill(v) for k, v in dict(bases=merged[1] + len(a1.bases), quals=merged[1] + len(a1.bases), titles=len(a1.titles), seq_offs=8 * (n + 1),
                                                 title_offs=8 * (n + 1), merged=n).items()}
            empty = d.up(p1[0].tobytes())                    # begin = end: records are kept, no bases are
            for what in ("d_seq_offs", "d_title_offs", "d_bases", "d_quals"):
                cols = lambda: lib.Columns(buf["bases"], 1 << 20, buf["quals"], 1 << 20, buf["titles"], 1 << 20, buf["seq_offs"], buf["title_offs"], n)
                o = cols(); setattr(o, what, None)
                note("select_device: out %s null" % what, h, error_of(lib, lambda: h.columns_select_device(st1.cols_in(), pb, pe, pk, o)))
                if what in ("d_bases", "d_quals"):
                    o = cols(); setattr(o, what, None)
                    err = error_of(lib, lambda: h.columns_select_device(st1.cols_in(), empty, empty, pk, o))
                    assert err is None, err
                    note("select_device: out %s null, no bases kept" % what, h, err)
                o = cols(); setattr(o, what, None)
                note("merge_device: out %s null" % what, h, error_of(lib, lambda: h.columns_merge_device(
                    st1.cols_in(), st2.cols_in(), cm.lib_rules(lib, cm.rules_of()), (pb, pe), tuple(d.up(v.tobytes()) for v in p2[:2]), pk,
                    d.up(insert.tobytes()), o, buf["merged"])))

            # ---- not a k-mer table ----
            junk, hist = ck.Table(lib, d, 16), d.fill(8 * 4)
            note("kmer_plan: not a table", h, kp.plan_call(lib, h, d, st1.cols_in(), n, kp.rules_of(), junk.p).error)
            note("kmer_count: accumulate into what is not a table", h, ck.kmer_call(lib, h, d, st1.cols_in(), ck.lib_rules(lib, K, accumulate=1, capacity=16), junk).error)
            note("kmer_count: accumulate with another k", h, ck.kmer_call(lib, h, d, st1.cols_in(), ck.lib_rules(lib, K + 1, accumulate=1, capacity=table.M), table).error)
            note("kmer_lookup: not a table", h, error_of(lib, lambda: h.kmer_lookup(junk.p, hist, 4, hist)))
            note("kmer_spectrum: not a table", h, error_of(lib, lambda: h.kmer_spectrum(junk.p, 4, hist)))
            note("kmer_table_merge: the source is not a table", h, error_of(lib, lambda: h.kmer_table_merge(junk.p, table.p)))
            note("kmer_table_merge: the destination is not a table", h, error_of(lib, lambda: h.kmer_table_merge(table.p, junk.p)))
            assert junk.untouched()
    finally:
        h.close()

    # ---- a colour-space handle ----
    hc = ce.handle(lib, dataclasses.replace(Config.from_levels(0, 0), color_space=True))
    try:
        with cp.staged(lib, hc, a1) as st1, cp.staged(lib, hc, a2) as st2, cs.Dev(hc) as d:
            calls = Calls(lib, hc, d, st1, st2, ck.Table(lib, d, 16))
            for name in calls.entries:
                note("%s: colour space" % name, hc, calls.run(name))
    finally:
        hc.close()
    return out


def run_messages(lib):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = collect(lib)
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    wrong = {name: (got[name], want[name]) for name in want if got[name] != want[name]}
    assert not wrong, wrong
    refused = [v for v in want.values() if v[0]]
    assert len(refused) >= 250 and all(v[1] for v in refused)
