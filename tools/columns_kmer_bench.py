#!/usr/bin/env python3
"""What the columnar k-mer count costs: reads of one length made in HBM with torch ops, in four legs -- "distinct" (random reads:
nearly every window is a new key), "pool" (reads cut at random places out of a random genome of records * read_length / coverage
bases on either strand, 30x by default: most inserts are hits on a key that is there), "one_sequence" (one read repeated: every
wave on the same few slots) and "poly_g_tail" (random reads whose last 60 bases are G, the tails of a two-colour instrument: what
the run aggregation is for).  Timed on those tensors, for each k: count_kmers (dsrcgpu_columns_kmer_count) of dsrc_amd/columns.py
into a table of a given capacity -- host wall time of the whole call, torch's allocation of the table included --, and beside it two
yardsticks on the same columns: trim_plan (dsrcgpu_columns_trim_plan), existing code that reads the same bases once, and the same
table computed with torch ops, which only fixed-length reads allow: the rolling keys by k shifted ORs over an int64 matrix,
torch.minimum with the reverse-complement keys, then torch.unique(return_counts=True).  The sorted (key, count) pairs of the library
must equal those of the torch ops in every leg.  Also timed: KmerTable.spectrum and the merge of the full table into an empty one
of the same capacity.  One warm-up and --steps timed calls each, min / median / max.
With a build that has the test hooks (DSRC_GPU_LIB=dsrc_amd/csrc/libdsrc_gpu_hooks.so) --variants also times the count kernel
without the run aggregation and without the plain load in front of the CAS (DSRC_GPU_KMER_VARIANT=1 / 2).
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
from dsrc_amd import _lib, columns  # noqa: E402
from dsrc_amd.config import Config  # noqa: E402


def as_columns(matrix):
    n, read_len = matrix.shape
    device = matrix.device
    quals = torch.full((n * read_len,), 30, dtype=torch.uint8, device=device)
    S = torch.arange(n + 1, dtype=torch.int64, device=device) * read_len
    empty = torch.empty(0, dtype=torch.uint8, device=device)
    return columns.RecordColumns(matrix.reshape(-1).contiguous(), quals, empty, S, torch.empty(0, dtype=torch.int64, device=device), torch.tensor([0, n]))


def make_reads(leg, n, read_len, coverage, device, seed=1):
    """-> an n x read_len uint8 matrix of base codes on `device`."""
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    if leg == "distinct":
        return torch.randint(0, 4, (n, read_len), generator=g, dtype=torch.uint8).to(device)
    if leg == "poly_g_tail":
        reads = torch.randint(0, 4, (n, read_len), generator=g, dtype=torch.uint8)
        reads[:, max(0, read_len - 60):] = 2
        return reads.to(device)
    if leg == "one_sequence":
        return torch.randint(0, 4, (1, read_len), generator=g, dtype=torch.uint8).to(device).repeat(n, 1)
    genome_len = max(2 * read_len, n * read_len // coverage)
    genome = torch.randint(0, 4, (genome_len,), generator=g, dtype=torch.uint8).to(device)
    start = torch.randint(0, genome_len - read_len + 1, (n,), generator=g).to(device)
    reads = genome[start[:, None] + torch.arange(read_len, device=device)[None, :]]
    flip = torch.rand(n, generator=g).to(device) < 0.5
    return torch.where(flip[:, None], (3 - reads).flip(1), reads).contiguous()


def torch_table(matrix, k):
    """The sorted canonical (key, count) pairs with torch ops: the yardstick."""
    n, read_len = matrix.shape
    w = read_len - k + 1
    m = matrix.to(torch.int64)
    fwd = torch.zeros((n, w), dtype=torch.int64, device=matrix.device); rc = torch.zeros_like(fwd)
    for j in range(k):
        fwd = (fwd << 2) | m[:, j: j + w]
        rc |= (3 - m[:, j: j + w]) << (2 * j)
    return torch.unique(torch.minimum(fwd, rc), return_counts=True)


def run(n, read_len, ks, legs, coverage, steps, device, with_torch, variants):
    cfg = Config.from_levels(0, 0, False)
    h = _lib.Handle(cfg.dna_order, cfg.quality_order, cfg.lossy, cfg.crc)
    out = []
    try:
        for leg in legs:
            matrix = make_reads(leg, n, read_len, coverage, device)
            c = as_columns(matrix)
            S = n * read_len
            trim_s, _ = timed(device, steps, lambda: columns.trim_plan(h, c, quality_3=20))
            for k in ks:
                windows = n * (read_len - k + 1)
                capacity = 16
                while capacity < 2 * windows:
                    capacity *= 2
                count_s, (table, stats) = timed(device, steps, lambda: columns.count_kmers(h, c, k, capacity=capacity))
                spec_s, (hist, totals) = timed(device, steps, lambda: table.spectrum(h, 256))
                empty_s, empty = timed(device, steps, lambda: columns.KmerTable.empty(h, k, True, capacity, device))
                merge_s, _ = timed(device, 1, lambda: table.merged_into(h, columns.KmerTable.empty(h, k, True, capacity, device)))
                res = {"leg": leg, "k": k, "windows": windows, "capacity": capacity, "table_MiB": round(16 * capacity / 2 ** 20, 1), "distinct": stats["distinct_after"],
                       "overflow": stats["overflow"], "largest_count": totals["largest_count"], "singletons": totals["singletons"],
                       # the least the count has to move: the bases and the offsets in; the table is the call's own traffic
                       "count_kmers": figures(S + 8 * (n + 1), count_s), "windows_per_us_median": round(windows / statistics.median(count_s) / 1e6, 1),
                       "trim_plan": figures(2 * S + 8 * (n + 1) + 17 * n, trim_s), "spectrum_256": figures(8 * capacity, spec_s),
                       "empty_table": figures(16 * capacity, empty_s), "merge_into_empty_incl_empty_table": figures(32 * capacity, merge_s),
                       "count_ms_over_trim_ms": round(statistics.median(count_s) / statistics.median(trim_s), 2)}
                if variants:
                    for name, v in (("no_run_aggregation", "1"), ("no_plain_load", "2")):
                        os.environ["DSRC_GPU_KMER_VARIANT"] = v
                        try:
                            v_s, (v_table, _) = timed(device, steps, lambda: columns.count_kmers(h, c, k, capacity=capacity))
                        finally:
                            os.environ.pop("DSRC_GPU_KMER_VARIANT", None)
                        res["count_kmers_" + name] = figures(S + 8 * (n + 1), v_s)
                        res[name + "_same_pairs"] = all(bool(torch.equal(x, y)) for x, y in zip(v_table.items(), table.items()))
                if with_torch:
                    torch_s, (t_keys, t_counts) = timed(device, steps, lambda: torch_table(matrix, k))
                    keys, counts = table.items()
                    res["torch_shift_or_unique"] = figures(S, torch_s)
                    res["pairs_equal_torch"] = bool(torch.equal(keys, t_keys) and torch.equal(counts, t_counts))
                    res["torch_ms_over_count_ms"] = round(statistics.median(torch_s) / statistics.median(count_s), 2)
                    del t_keys, t_counts
                out.append(res)
                print(json.dumps(res), file=sys.stderr, flush=True)
                del table, empty, hist
    finally:
        h.close()
    return {"case": "columnar k-mer count, synthetic fixed-length reads, device-resident", "records": n, "read_length": read_len, "coverage_of_pool_leg": coverage,
            "steps": steps, "library": os.path.basename(_lib.lib_path()),
            "figures": "host wall time around the synchronous call of dsrc_amd/columns.py (torch's allocation of the table included); "
                       "bytes: the least the call must read plus write; GBps_median = bytes / median time; floor = bytes at 8 TB/s",
            "legs": out}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--records", type=int, default=1 << 20, help="records (a few hundred with the emulator build)")
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--k", default="21,31", help="k-mer lengths, comma-separated")
    ap.add_argument("--legs", default="distinct,pool,one_sequence,poly_g_tail")
    ap.add_argument("--coverage", type=int, default=30, help="of the pool leg")
    ap.add_argument("--steps", type=int, default=5, help="timed calls (at least 5: the spread is min..max)")
    ap.add_argument("--device", default="cuda:0", help="torch device of the arrays (cpu with the emulator build)")
    ap.add_argument("--no-torch", action="store_true", help="leave the torch leg out")
    ap.add_argument("--variants", action="store_true", help="also time the two measuring variants (needs a build with the test hooks)")
    ap.add_argument("--out", default=None, help="also write the result to this file")
    a = ap.parse_args()
    res = run(a.records, a.read_length, [int(s) for s in a.k.split(",")], a.legs.split(","), a.coverage, max(a.steps, 5), torch.device(a.device),
              not a.no_torch, a.variants)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
