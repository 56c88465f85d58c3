#!/usr/bin/env python3
"""What the columnar k-mer correction costs and what it mends: reads of one length made in HBM with torch ops (the legs of
tools/columns_kmer_bench.py), in three workloads --
  "errors"       the "pool" reads (30x of a random genome, either strand) with substitutions planted at --error-permille (10 = 1 %), the
                 truth kept on the device, against the table of the batch itself, min_count = 3
  "error_free"   the pool reads as they are against their own table: no run exists, the cost should be the plan's
  "poly_g_tail"  random reads whose last 60 bases are G against their own table, min_count = 2: nothing but the tail is solid, every
                 read is one long run that is left alone
Timed on those tensors: correct_kmers (dsrcgpu_columns_kmer_correct) of dsrc_amd/columns.py out of place and in place -- host wall time of
the whole call, torch's allocation of the outputs included; in place the bases are put back as they came in front of every call,
outside the clock --, and beside it, from the same process on the same batch and table, kmer_plan(min_count, trim="first_miss") and
count_kmers (its table allocated outside the timed call).  Reported: wrong bases before and after against the truth, right bases made
wrong, and the statistics.  One warm-up and --steps timed calls each, min / median / max.  A timing tool, not a gate.  With the
emulator build of the library (DSRC_GPU_LIB, --device cpu) it runs end to end and the figures mean nothing.  Results go to profiles/
(--out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402  (before the first handle: dsrc_amd/columns.py)
from columns_adapter_bench import figures  # noqa: E402
from columns_filter_bench import timed  # noqa: E402
from columns_kmer_bench import as_columns, make_reads  # noqa: E402
from columns_kmer_plan_bench import pow2_at_least  # noqa: E402
from dsrc_amd import _lib, columns  # noqa: E402
from dsrc_amd.config import Config  # noqa: E402


def plant_errors(matrix, permille, seed=11):
    """-> the matrix with another base at about permille / 1000 of its positions (made on the device)."""
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    n, read_len = matrix.shape
    where = (torch.rand((n, read_len), generator=g) * 1000 < permille).to(matrix.device)
    shift = torch.randint(1, 4, (n, read_len), generator=g, dtype=torch.uint8).to(matrix.device)
    return torch.where(where, (matrix + shift) % 4, matrix).contiguous()


def timed_in_place(device, steps, cols, came, call):
    """timed() for a call that changes cols.bases: they are put back as they came in front of every call, outside the clock."""
    def once():
        cols.bases.copy_(came)
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        t = time.perf_counter()
        res = call()
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        return time.perf_counter() - t, res
    once()
    runs = [once() for _ in range(steps)]
    return [r[0] for r in runs], runs[-1][1]


def run(n, read_len, k, coverage, permille, steps, device):
    cfg = Config.from_levels(0, 0, False)
    h = _lib.Handle(cfg.dna_order, cfg.quality_order, cfg.lossy, cfg.crc)
    S = n * read_len
    windows = n * (read_len - k + 1)
    out = []
    try:
        pool = make_reads("pool", n, read_len, coverage, device)
        legs = [("errors", plant_errors(pool, permille), pool, 3), ("error_free", pool, pool, 3),
                ("poly_g_tail", make_reads("poly_g_tail", n, read_len, coverage, device), None, 2)]
        for name, matrix, truth, min_count in legs:
            c = as_columns(matrix.clone())                       # (in place writes into it; the truth may be the same tensor)
            came = c.bases.clone()
            capacity = pow2_at_least(2 * windows)
            table = columns.count_kmers(h, c, k, capacity=capacity)[0]
            into = columns.KmerTable.empty(h, k, True, capacity, device)

            def count():
                return h.columns_kmer_count(columns._columns_in(c, False)[0], None, None, None, _lib.KmerRules(k, 1, 0, 0, capacity), into.data.data_ptr())
            count_s, _ = timed(device, steps, count)
            del into
            plan_s, plan = timed(device, steps, lambda: columns.kmer_plan(h, c, table, min_count=min_count, trim="first_miss"))
            out_s, (fixed_cols, stats) = timed(device, steps, lambda: columns.correct_kmers(h, c, table, min_count=min_count))
            in_s, (_, in_stats) = timed_in_place(device, steps, c, came, lambda: columns.correct_kmers(h, c, table, min_count=min_count, inplace=True))
            same = bool(torch.equal(fixed_cols.bases, c.bases)) and stats == in_stats
            again = columns.correct_kmers(h, fixed_cols, table, min_count=min_count)
            least = S + 8 * (n + 1)                              # the bases and the offsets in; the table is the call's own traffic
            res = {"workload": name, "k": k, "min_count": min_count, "windows": windows, "table_capacity": table.capacity,
                   "table_MiB": round(16 * table.capacity / 2 ** 20, 1), "table_distinct": table.summary()["distinct"], "stats": stats,
                   "correct_kmers_out_of_place": figures(least + S, out_s), "correct_kmers_in_place": figures(least, in_s),
                   "kmer_plan_first_miss": figures(least + 17 * n, plan_s), "count_kmers_same_batch": figures(least, count_s),
                   "plan_stats": plan[3],
                   "out_of_place_ms_over_plan_ms": round(statistics.median(out_s) / statistics.median(plan_s), 2),
                   "in_place_ms_over_plan_ms": round(statistics.median(in_s) / statistics.median(plan_s), 2),
                   "in_place_equals_out_of_place": same,
                   "second_pass_fixes": again[1]["bases_fixed"], "second_pass_runs": again[1]["runs"],
                   "second_pass_changes_nothing": bool(torch.equal(again[0].bases, fixed_cols.bases))}
            if truth is not None:
                t = truth.reshape(-1)
                res["wrong_bases_before"] = int((came != t).sum())
                res["wrong_bases_after"] = int((fixed_cols.bases != t).sum())
                res["right_bases_made_wrong"] = int(((came == t) & (fixed_cols.bases != t)).sum())
            out.append(res)
            print(json.dumps(res), file=sys.stderr, flush=True)
            del table, fixed_cols, again, came, c
    finally:
        h.close()
    return {"case": "columnar k-mer correction, synthetic fixed-length reads, device-resident", "records": n, "read_length": read_len, "k": k,
            "coverage_of_pool": coverage, "error_permille": permille, "steps": steps, "library": os.path.basename(_lib.lib_path()),
            "figures": "host wall time around the synchronous call of dsrc_amd/columns.py (torch's allocation of the outputs included); "
                       "bytes: the least the call must read plus write; GBps_median = bytes / median time; floor = bytes at 8 TB/s",
            "workloads": out}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--records", type=int, default=1 << 20, help="records (a few hundred with the emulator build)")
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--coverage", type=int, default=30, help="of the pool reads")
    ap.add_argument("--error-permille", type=int, default=10, help="substitutions planted per thousand bases")
    ap.add_argument("--steps", type=int, default=5, help="timed calls (at least 5: the spread is min..max)")
    ap.add_argument("--device", default="cuda:0", help="torch device of the arrays (cpu with the emulator build)")
    ap.add_argument("--out", default=None, help="also write the result to this file")
    a = ap.parse_args()
    res = run(a.records, a.read_length, a.k, a.coverage, a.error_permille, max(a.steps, 5), torch.device(a.device))
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
