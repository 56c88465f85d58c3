#!/usr/bin/env python3
"""What the columnar k-mer plan costs: reads of one length made in HBM with torch ops (the legs of tools/columns_kmer_bench.py), in
three workloads --
  "screen"          a contaminant screen: the "pool" reads (30x of a random genome, either strand) with one read in a hundred cut out
                    of a small reference instead (5 386 bases, the size of PhiX), against the table of that reference alone;
                    trim none, max_hits = 0
  "abundance_trim"  the pool reads against the table of the batch itself; trim first_miss, min_count = 2 -- against the table as
                    count_kmers left it (sized for the windows of the call) and against the same pairs in a table sized for its keys
  "poly_g_tail"     random reads whose last 60 bases are G against their own table, trim first_miss, min_count = 2: what taking a
                    run's count from its head lane is for
each without and with the median (a bound that every record passes, so that the outputs are the same three arrays).  Timed on those
tensors: kmer_plan (dsrcgpu_columns_kmer_plan) of dsrc_amd/columns.py -- host wall time of the whole call, torch's allocation of the
outputs included --, and beside it two yardsticks that exist without it: count_kmers on the same batch (the same walk plus the atomics;
its table allocated outside the timed call) and what a user composes today with torch ops and KmerTable.lookup: the rolling forward
words by k shifted ORs over an int64 matrix (8 bytes a window), one lookup of all of them, then hits, the first miss and the cut per
read.  hits and the cut of the library must equal those of the torch ops.  One warm-up and --steps timed calls each, min / median / max.
A timing tool, not a gate.  With the emulator build of the library (DSRC_GPU_LIB, --device cpu) it runs end to end and the figures
mean nothing.  Results go to profiles/ (--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402  (before the first handle: dsrc_amd/columns.py)
from columns_adapter_bench import figures  # noqa: E402
from columns_filter_bench import timed  # noqa: E402
from columns_kmer_bench import as_columns, make_reads  # noqa: E402
from dsrc_amd import _lib, columns  # noqa: E402
from dsrc_amd.config import Config  # noqa: E402

REFERENCE_BASES = 5386


def pow2_at_least(v):
    c = 16
    while c < v:
        c *= 2
    return c


def torch_plan(h, table, matrix, k, min_count, trim):
    """hits and the new end of every read with torch ops and one KmerTable.lookup: what there is without the planner (reads without
    codes above 3 only)."""
    n, read_len = matrix.shape
    w = read_len - k + 1
    m = matrix.to(torch.int64)
    fwd = torch.zeros((n, w), dtype=torch.int64, device=matrix.device)
    for j in range(k):
        fwd = (fwd << 2) | m[:, j: j + w]
    hit = (table.lookup(h, fwd.reshape(-1)) >= min_count).view(n, w)
    hits = hit.sum(1)
    end = torch.full((n,), read_len, dtype=torch.int64, device=matrix.device)
    if trim == "first_miss":
        miss = ~hit
        end = torch.where(miss.any(1), miss.to(torch.uint8).argmax(1) + (k - 1), end)
    return hits, end


def run(n, read_len, k, coverage, steps, device, with_torch, torch_records):
    cfg = Config.from_levels(0, 0, False)
    h = _lib.Handle(cfg.dna_order, cfg.quality_order, cfg.lossy, cfg.crc)
    S = n * read_len
    windows = n * (read_len - k + 1)
    out = []
    try:
        pool = make_reads("pool", n, read_len, coverage, device)
        g = torch.Generator(device="cpu"); g.manual_seed(7)
        reference = torch.randint(0, 4, (REFERENCE_BASES,), generator=g, dtype=torch.uint8).to(device)
        spiked = pool.clone()
        where = torch.arange(0, n, 100, device=device)
        start = torch.randint(0, REFERENCE_BASES - read_len + 1, (where.numel(),), generator=g).to(device)
        spiked[where] = reference[start[:, None] + torch.arange(read_len, device=device)[None, :]]
        ref_cols = columns.RecordColumns(reference, torch.zeros_like(reference), torch.empty(0, dtype=torch.uint8, device=device),
                                         torch.tensor([0, REFERENCE_BASES], device=device), torch.empty(0, dtype=torch.int64, device=device), torch.tensor([0, 1]))
        ref_table, _ = columns.count_kmers(h, ref_cols, k)
        legs = [("screen", spiked, "reference", dict(max_hits=0)), ("abundance_trim", pool, "own", dict(trim="first_miss", min_count=2)),
                ("abundance_trim", pool, "own_shrunk", dict(trim="first_miss", min_count=2)),
                ("poly_g_tail", make_reads("poly_g_tail", n, read_len, coverage, device), "own", dict(trim="first_miss", min_count=2))]
        own = {}
        for name, matrix, which, kw in legs:
            c = as_columns(matrix)
            capacity = pow2_at_least(2 * windows)
            if which == "reference":
                table = ref_table
            elif (name, "own") in own:
                table = own[(name, "own")]
            else:
                table = own[(name, "own")] = columns.count_kmers(h, c, k, capacity=capacity)[0]
            if which == "own_shrunk":
                table = table.grown(h, pow2_at_least(2 * table.summary()["distinct"]))
            into = columns.KmerTable.empty(h, k, True, capacity, device)

            def count():
                # (a fresh count into the table allocated above: accumulate is off, the library empties the table first)
                return h.columns_kmer_count(columns._columns_in(c, False)[0], None, None, None, _lib.KmerRules(k, 1, 0, 0, capacity), into.data.data_ptr())
            count_s, _ = timed(device, steps, count)
            del into
            plain_s, plain = timed(device, steps, lambda: columns.kmer_plan(h, c, table, **kw))
            median_s, with_median = timed(device, steps, lambda: columns.kmer_plan(h, c, table, max_median=_lib.KMER_PLAN_COUNT_CAP, **kw))
            counts_s, with_counts = timed(device, steps, lambda: columns.kmer_plan(h, c, table, return_counts=True, **kw))
            stats = plain[3]
            least = S + 8 * (n + 1) + 17 * n                 # the bases and the offsets in, the plan out; the table is the call's own traffic
            res = {"workload": name, "table": which, "k": k, "windows": windows, "table_capacity": table.capacity, "table_MiB": round(16 * table.capacity / 2 ** 20, 1),
                   "table_distinct": table.summary()["distinct"], "stats": stats,
                   "kmer_plan": figures(least, plain_s), "kmer_plan_median": figures(least, median_s), "kmer_plan_median_and_counts": figures(least + 24 * n, counts_s),
                   "count_kmers_same_batch": figures(S + 8 * (n + 1), count_s),
                   "windows_per_us_median": round(windows / statistics.median(plain_s) / 1e6, 1),
                   "plan_ms_over_count_ms": round(statistics.median(plain_s) / statistics.median(count_s), 2),
                   "median_ms_over_plan_ms": round(statistics.median(median_s) / statistics.median(plain_s), 2),
                   "same_plan_with_median": all(bool(torch.equal(x, y)) for x, y in zip(plain[:3], with_median[:3]))}
            if with_torch:
                t_n = min(n, torch_records)
                sub = matrix[:t_n].contiguous()
                sub_c = as_columns(sub)
                sub_s, sub_plan = timed(device, steps, lambda: columns.kmer_plan(h, sub_c, table, return_counts=True, **kw))
                torch_s, (t_hits, t_end) = timed(device, steps, lambda: torch_plan(h, table, sub, k, kw.get("min_count", 1), kw.get("trim", "none")))
                res["torch_records"] = t_n
                res["torch_unfold_lookup_reduce"] = figures(t_n * read_len, torch_s)
                res["kmer_plan_on_those_records"] = figures(t_n * read_len + 8 * (t_n + 1) + 41 * t_n, sub_s)
                res["torch_ms_over_plan_ms"] = round(statistics.median(torch_s) / statistics.median(sub_s), 2)
                res["hits_equal_torch"] = bool(torch.equal(sub_plan[5], t_hits))
                res["ends_equal_torch"] = bool(torch.equal(sub_plan[1] - sub_plan[0], t_end))
                del t_hits, t_end, sub_plan
            out.append(res)
            print(json.dumps(res), file=sys.stderr, flush=True)
            del plain, with_median, with_counts
    finally:
        h.close()
    return {"case": "columnar k-mer plan, synthetic fixed-length reads, device-resident", "records": n, "read_length": read_len, "k": k, "coverage_of_pool": coverage,
            "steps": steps, "library": os.path.basename(_lib.lib_path()),
            "figures": "host wall time around the synchronous call of dsrc_amd/columns.py (torch's allocation of the outputs included); "
                       "bytes: the least the call must read plus write; GBps_median = bytes / median time; floor = bytes at 8 TB/s",
            "workloads": out}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--records", type=int, default=1 << 20, help="records (a few hundred with the emulator build)")
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--coverage", type=int, default=30, help="of the pool reads")
    ap.add_argument("--steps", type=int, default=5, help="timed calls (at least 5: the spread is min..max)")
    ap.add_argument("--device", default="cuda:0", help="torch device of the arrays (cpu with the emulator build)")
    ap.add_argument("--no-torch", action="store_true", help="leave the torch leg out")
    ap.add_argument("--torch-records", type=int, default=1 << 20, help="the torch leg takes the first this many records (8 bytes a window, several times over)")
    ap.add_argument("--out", default=None, help="also write the result to this file")
    a = ap.parse_args()
    res = run(a.records, a.read_length, a.k, a.coverage, max(a.steps, 5), torch.device(a.device), not a.no_torch, a.torch_records)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
