#!/usr/bin/env python3
"""What the columnar merge costs: the pairs of tools/columns_pair_bench.py (made in HBM with torch ops, insert sizes drawn around the
read length, about 1 % of the bases substituted) go through pair_plan once, and on its output -- the narrowed ranges, the pair's keep
and the insert sizes -- merge_pairs (dsrcgpu_columns_merge_device) of dsrc_amd/columns.py is timed.  Beside it, as yardsticks in
the same run on the same pairs: pair_plan itself, and the two select_columns calls that would write the same pairs unmerged -- the
merge reads what those two selects read and writes about what one of them writes.  One warm-up and --steps timed calls each, host
wall time around the synchronous call as min / median / max, the bytes the call has to read and write at the least, the GB/s that
follows and the time those bytes take at 8 TB/s (the floor).  The pairs carry no titles.  The merged lengths are compared with the
insert sizes the pairs were built from.
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
from columns_pair_bench import make_pairs  # noqa: E402
from dsrc_amd import _lib, columns  # noqa: E402
from dsrc_amd.config import Config  # noqa: E402


def run(n_pairs, read_len, steps, device):
    cfg = Config.from_levels(0, 0, False)
    h = _lib.Handle(cfg.dna_order, cfg.quality_order, cfg.lossy, cfg.crc)
    try:
        c1, c2, true_insert = make_pairs(n_pairs, read_len, device)
        R, S = n_pairs, n_pairs * read_len
        pair_s, (b1, e1, b2, e2, keep, p_stats, insert) = timed(device, steps, lambda: columns.pair_plan(h, c1, c2, return_insert=True))
        merge_s, (merged, flag, m_stats) = timed(device, steps, lambda: columns.merge_pairs(h, c1, c2, b1, e1, b2, e2, keep, insert, titles=False))
        both = keep & flag                                   # the two selects of the pairs the merge takes: the same bytes read, both mates written
        sel_s, (s1, s2) = timed(device, steps, lambda: (columns.select_columns(h, c1, b1, e1, both, titles=False),
                                                        columns.select_columns(h, c2, b2, e2, both, titles=False)))
        lens = merged.seq_offsets[1:] - merged.seq_offsets[:-1]
        right = int((lens == true_insert[flag != 0]).sum())
        sel_bases = s1.bases.numel() + s2.bases.numel()
    finally:
        h.close()
    K, M = m_stats["pairs_merged"], m_stats["bases_written"]
    # the least a call has to move.  The merge: both sets of offsets, four range positions, the keep and the insert size per pair, bases
    # and qualities of the merged pairs' ranges, and out go bases and qualities of the merged reads, an offset each and a flag per pair.
    # The two selects: per side the offsets, two positions and the keep, and the kept ranges' bases and qualities in and out.
    merge_bytes = 2 * 8 * (R + 1) + 41 * R + 2 * sel_bases + 2 * M + 8 * (K + 1) + R
    sel_bytes = 2 * (8 * (R + 1) + 17 * R + 8 * (K + 1)) + 4 * sel_bases
    pair_bytes = 2 * S + 2 * 8 * (R + 1) + 41 * R
    med = statistics.median
    return {"case": "columnar merge behind the pair plan, synthetic pairs, device-resident", "pairs": R, "read_length": read_len, "steps": steps,
            "figures": "host wall time around the synchronous call(s) of dsrc_amd/columns.py (torch's allocation of the outputs and the sizing "
                       "call included); bytes: the least the call must read plus write; GBps_median = bytes / median time; floor = bytes at 8 TB/s",
            "pairs_merged": K, "merged_length_equals_the_true_insert": right,
            "merge_pairs": dict(figures(merge_bytes, merge_s), stats=m_stats), "pair_plan": dict(figures(pair_bytes, pair_s), stats=p_stats),
            "two_selects_of_the_merged_pairs": figures(sel_bytes, sel_s),
            "merge_ms_over_two_selects_ms": round(med(merge_s) / med(sel_s), 3) if min(sel_s) > 0 else None,
            "ns_per_pair_median": round(med(merge_s) * 1e9 / R, 2)}


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
