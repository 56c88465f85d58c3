#!/usr/bin/env python3
"""What the columnar pair plan costs: pairs made in HBM with torch ops -- a random "genome" tensor supplies the inserts, insert sizes
are drawn around the read length so that a good share of the pairs read through, read 1 is the insert from the left, read 2 its
reverse complement, each followed by its adapter and random bases, about 1 % of the bases substituted.  Timed on those tensors:
pair_plan (dsrcgpu_columns_pair_plan) of dsrc_amd/columns.py on whole reads, and beside it adapter_plan
(dsrcgpu_columns_adapter_plan) with one adapter on read 1 of the same tensors -- existing code that reads half the bases: the
yardstick.  One warm-up and --steps timed calls each, host wall time around the synchronous call as min / median / max, the bytes the
call has to read and write at the least, the GB/s that follows and the time those bytes take at 8 TB/s (the floor).  The insert sizes
the plan reports are compared with the ones the pairs were built from.
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
from columns_adapter_bench import ADAPTERS, figures  # noqa: E402
from columns_filter_bench import timed  # noqa: E402
from dsrc_amd import _lib, columns  # noqa: E402
from dsrc_amd.config import Config  # noqa: E402


def make_pairs(n_pairs, read_len, device, seed=1, genome=1 << 22, error=0.01):
    """-> (columns of read 1, columns of read 2, true insert sizes), all on `device`."""
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    rnd = lambda *shape: torch.rand(*shape, generator=g).to(device)
    codes = lambda *shape: torch.randint(0, 4, shape, generator=g, dtype=torch.uint8).to(device)
    G = codes(genome)
    insert = (read_len * (1.0 + 0.45 * torch.randn(n_pairs, generator=g))).long().clamp(20, 3 * read_len).to(device)
    start = (rnd(n_pairs) * (genome - 3 * read_len - 1)).long()
    j = torch.arange(read_len, device=device).unsqueeze(0)
    inside = j < insert.unsqueeze(1)
    reads = []
    for side, adapter in ((0, ADAPTERS[0]), (1, ADAPTERS[1])):
        a = torch.tensor(["ACGT".index(c) for c in adapter], dtype=torch.uint8, device=device)
        pos = start.unsqueeze(1) + (j if side == 0 else insert.unsqueeze(1) - 1 - j)
        from_insert = G[pos.clamp(0, genome - 1)]
        if side == 1:
            from_insert = 3 - from_insert
        behind = j - insert.unsqueeze(1)
        tail = torch.where((behind >= 0) & (behind < len(a)), a[behind.clamp(0, len(a) - 1)], codes(n_pairs, read_len))
        x = torch.where(inside, from_insert, tail)
        sub = rnd(n_pairs, read_len) < error
        x = torch.where(sub, (x + 1 + (rnd(n_pairs, read_len) * 3).to(torch.uint8)) % 4, x)
        S = torch.arange(n_pairs + 1, dtype=torch.int64, device=device) * read_len
        empty = torch.empty(0, dtype=torch.uint8, device=device)
        reads.append(columns.RecordColumns(x.reshape(-1).contiguous(), torch.full((n_pairs * read_len,), 30, dtype=torch.uint8, device=device), empty, S,
                                           torch.empty(0, dtype=torch.int64, device=device), torch.tensor([0, n_pairs])))
    return reads[0], reads[1], insert


def run(n_pairs, read_len, steps, device):
    cfg = Config.from_levels(0, 0, False)
    h = _lib.Handle(cfg.dna_order, cfg.quality_order, cfg.lossy, cfg.crc)
    try:
        c1, c2, true_insert = make_pairs(n_pairs, read_len, device)
        R, S = n_pairs, n_pairs * read_len
        pair_s, got = timed(device, steps, lambda: columns.pair_plan(h, c1, c2, return_insert=True))
        one_s, (_, _, _, one) = timed(device, steps, lambda: columns.adapter_plan(h, c1, ADAPTERS[:1]))
        stats, insert = got[5], got[6]
        found = insert >= 0
        right = int((insert[found] == true_insert[found]).sum())
        reachable = int((true_insert <= 2 * read_len - 30).sum())       # an overlap of min_overlap = 30 bases and more
    finally:
        h.close()
    # the least a call has to move: the pair plan reads both sets of bases and offsets and writes four positions, a flag and the insert
    # size per pair; the adapter plan reads one set of bases and offsets and writes 17 bytes a record
    pair_bytes = 2 * S + 2 * 8 * (R + 1) + 41 * R
    adapt_bytes = S + 8 * (R + 1) + 17 * R
    med = statistics.median
    return {"case": "columnar pair plan, synthetic pairs, device-resident", "pairs": R, "read_length": read_len, "steps": steps,
            "figures": "host wall time around the synchronous call of dsrc_amd/columns.py (torch's allocation of the outputs included); "
                       "bytes: the least the call must read plus write; GBps_median = bytes / median time; floor = bytes at 8 TB/s",
            "pairs_with_an_overlap_of_30_and_more": reachable, "overlap_found": stats["overlap_found"], "insert_equals_the_true_one": right,
            "pair_plan": dict(figures(pair_bytes, pair_s), stats=stats), "adapter_plan_1_read1": dict(figures(adapt_bytes, one_s), stats=one),
            "pair_ms_over_adapter_1_ms": round(med(pair_s) / med(one_s), 3) if min(one_s) > 0 else None,
            "ns_per_pair_median": round(med(pair_s) * 1e9 / R, 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=1 << 20, help="pairs (a few hundred with the emulator build)")
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--steps", type=int, default=5, help="timed calls (at least 5: the spread is min..max)")
    ap.add_argument("--device", default="cuda:0", help="torch device of the arrays (cpu with the emulator build)")
    ap.add_argument("--out", default=None, help="also write the result to this file")
    a = ap.parse_args()
    res = run(a.pairs, a.read_length, max(a.steps, 5), torch.device(a.device))
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
