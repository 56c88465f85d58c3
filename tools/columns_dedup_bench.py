#!/usr/bin/env python3
"""What the columnar dedup plan costs: reads of one length made in HBM with torch ops -- `unique` random templates, every record a copy
of one of them, shuffled --, at several duplicate shares (the share of the records that are copies of another one; 1.0 = one sequence
repeated, the worst case for the table: every record meets on one slot).  Timed on those tensors: dedup_plan
(dsrcgpu_columns_dedup_plan) of dsrc_amd/columns.py on whole reads with prefer="first" and prefer="quality", and beside it two
yardsticks on the same columns: trim_plan (dsrcgpu_columns_trim_plan), existing code that reads the same bases once, and the same keep
computed with torch ops -- torch.unique(dim=0, return_inverse=True) on the bases as a matrix (which only fixed-length reads allow) plus a
scatter-min of the record indices.  One warm-up and --steps timed calls each, host wall time around the synchronous call as min /
median / max, the bytes the call has to read and write at the least, the GB/s that follows and the time those bytes take at 8 TB/s
(the floor).  The keep of the library is compared with that of the torch ops.
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


def make_reads(n, read_len, share, device, seed=1):
    """-> columns of n reads of read_len bases of which about `share` are copies of another record, on `device`."""
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    unique = max(1, min(n, round(n * (1.0 - share))))
    templates = torch.randint(0, 4, (unique, read_len), generator=g, dtype=torch.uint8).to(device)
    pick = torch.cat((torch.arange(unique), torch.randint(0, unique, (n - unique,), generator=g)))[torch.randperm(n, generator=g)].to(device)
    bases = templates[pick].reshape(-1).contiguous()
    quals = torch.randint(2, 41, (n * read_len,), generator=g, dtype=torch.uint8).to(device)
    S = torch.arange(n + 1, dtype=torch.int64, device=device) * read_len
    empty = torch.empty(0, dtype=torch.uint8, device=device)
    return columns.RecordColumns(bases, quals, empty, S, torch.empty(0, dtype=torch.int64, device=device), torch.tensor([0, n]))


def torch_keep(cols, n, read_len):
    """The keep of prefer="first" with torch ops: the yardstick."""
    _, inverse = torch.unique(cols.bases.view(n, read_len), dim=0, return_inverse=True)
    index = torch.arange(n, device=inverse.device)
    first = torch.full((int(inverse.max()) + 1,), n, dtype=torch.int64, device=inverse.device).scatter_reduce_(0, inverse, index, "amin")
    return (first[inverse] == index).to(torch.uint8)


def run(n, read_len, shares, steps, device, with_torch=True):
    cfg = Config.from_levels(0, 0, False)
    h = _lib.Handle(cfg.dna_order, cfg.quality_order, cfg.lossy, cfg.crc)
    legs = []
    try:
        for share in shares:
            c = make_reads(n, read_len, share, device)
            S = n * read_len
            first_s, (keep, stats) = timed(device, steps, lambda: columns.dedup_plan(h, c))
            qual_s, (_, q_stats) = timed(device, steps, lambda: columns.dedup_plan(h, c, prefer="quality"))
            trim_s, _ = timed(device, steps, lambda: columns.trim_plan(h, c, quality_3=20))
            # the least a call has to move: the bases (prefer="quality": and the qualities) and the offsets in, a flag per record out; the
            # table and the per-record words in the arena are the call's own traffic and are not counted
            leg = {"duplicate_share": share, "records_kept": stats["records_kept"], "largest_class": stats["largest_class"],
                   "dedup_plan_first": figures(S + 8 * (n + 1) + n, first_s), "dedup_plan_quality": figures(2 * S + 8 * (n + 1) + n, qual_s),
                   "representative_not_first": q_stats["representative_not_first"],
                   "trim_plan": figures(2 * S + 8 * (n + 1) + 17 * n, trim_s),
                   "ns_per_record_median": round(statistics.median(first_s) * 1e9 / n, 2),
                   "dedup_first_ms_over_trim_ms": round(statistics.median(first_s) / statistics.median(trim_s), 3)}
            if with_torch:
                torch_s, t_keep = timed(device, steps, lambda: torch_keep(c, n, read_len))
                leg["torch_unique_scatter_min"] = figures(S + n, torch_s)
                leg["keep_equals_torch"] = bool(torch.equal(keep, t_keep))
                leg["torch_ms_over_dedup_first_ms"] = round(statistics.median(torch_s) / statistics.median(first_s), 2)
            legs.append(leg)
            print(json.dumps(leg), file=sys.stderr, flush=True)
    finally:
        h.close()
    return {"case": "columnar dedup plan, synthetic fixed-length reads, device-resident", "records": n, "read_length": read_len, "steps": steps,
            "figures": "host wall time around the synchronous call of dsrc_amd/columns.py (torch's allocation of the outputs included); "
                       "bytes: the least the call must read plus write; GBps_median = bytes / median time; floor = bytes at 8 TB/s",
            "legs": legs}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--records", type=int, default=1 << 20, help="records (a few hundred with the emulator build)")
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--shares", default="0,0.1,0.5,0.9,1", help="duplicate shares, comma-separated")
    ap.add_argument("--steps", type=int, default=5, help="timed calls (at least 5: the spread is min..max)")
    ap.add_argument("--device", default="cuda:0", help="torch device of the arrays (cpu with the emulator build)")
    ap.add_argument("--no-torch", action="store_true", help="leave the torch.unique leg out")
    ap.add_argument("--out", default=None, help="also write the result to this file")
    a = ap.parse_args()
    res = run(a.records, a.read_length, [float(s) for s in a.shares.split(",")], max(a.steps, 5), torch.device(a.device), not a.no_torch)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
