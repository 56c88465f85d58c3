#!/usr/bin/env python3
"""What the columnar profile costs: about a million Illumina-like reads of 150 bases generated in HBM (dsrcgpu_synth_fastq flavour 0),
compressed and decoded into arrays by decode_columns as in tools/columns_adapter_bench.py.  Timed on those tensors:
profile_columns (dsrcgpu_columns_profile) of dsrc_amd/columns.py on whole reads with n_cycles = the read length; beside it trim_plan
(dsrcgpu_columns_trim_plan) with both ends on -- existing code that reads one byte per base where the profile reads two: the first
yardstick; and the same tables computed with torch ops on the device (position indices materialised as int64, bincount and
scatter_add) -- what a user would otherwise run: the second.  The torch tables are compared with the library's, word for word.
One warm-up and --steps timed calls each, host wall time around the synchronous call as min / median / max, the bytes the call has to
read at the least, the GB/s that follows and the time those bytes take at 8 TB/s (the floor).  With --plan the profile is timed once
more under the quality plan ("after"); with --cycles 16,256,257,1024 once more per n_cycles given (below the read length most
positions fold into the last cycle; 256 and 257 do the same work in the small and in the large LDS table).
A timing tool, not a gate.  With the emulator build of the library (DSRC_GPU_LIB, --device cpu) it runs end to end and the figures
mean nothing.  Results go to profiles/."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402  (before the first handle: dsrc_amd/columns.py)
import bench  # noqa: E402
from columns_adapter_bench import figures  # noqa: E402
from columns_filter_bench import FLAVOURS, timed  # noqa: E402
from config_bench import record_offsets  # noqa: E402
from dsrc_amd import _lib, columns  # noqa: E402
from dsrc_amd.config import Config  # noqa: E402


def profile_torch(cols, C):
    """The tables of dsrcgpu_columns_profile on whole reads with torch ops -> one int64 tensor in the library's layout."""
    dev = cols.bases.device
    S = cols.seq_offsets
    R = cols.n_records
    lens = S[1:] - S[:-1]
    rec = torch.repeat_interleave(torch.arange(R, device=dev), lens)
    i = torch.arange(cols.bases.numel(), device=dev) - S[:-1][rec]
    x, q = cols.bases.long(), cols.quals.long()
    idx = torch.clamp(i, max=C - 1) * 5 + torch.clamp(x, max=4)
    zeros = lambda n: torch.zeros(n, dtype=torch.int64, device=dev)
    base = torch.bincount(idx, minlength=5 * C)
    qsum = zeros(5 * C).scatter_add_(0, idx, q)
    qhist = torch.bincount(q, minlength=256)
    length = torch.bincount(torch.clamp(lens, max=C), minlength=C + 1)
    gc_base, acgt_base = ((x == 1) | (x == 2)).long(), (x < 4).long()
    qs = zeros(R).scatter_add_(0, rec, q)
    g = zeros(R).scatter_add_(0, rec, gc_base)
    a = zeros(R).scatter_add_(0, rec, acgt_base)
    gc = torch.bincount((100 * g[a > 0]) // a[a > 0], minlength=101)
    meanq = torch.bincount(qs[lens > 0] // lens[lens > 0], minlength=256)
    tot = torch.stack([torch.tensor(R, device=dev), lens.sum(), (q >= 20).sum(), (q >= 30).sum(), q.sum(), gc_base.sum(), (x >= 4).sum(), (lens == 0).sum()])
    return torch.cat([tot, base, qsum, qhist, length, gc, meanq])


def run(blocks, steps, device, with_plan, cycles=(), torch_ops=True, first=1):
    name, synth_flavour, rec_bytes, levels, _ = FLAVOURS[0]
    cfg = Config.from_levels(*levels)
    h = _lib.Handle(cfg.dna_order, cfg.quality_order, cfg.lossy, cfg.crc)
    recs = int(blocks * bench.BUF / rec_bytes * 1.02) + 1000
    off = record_offsets(synth_flavour, first, recs)
    cap = int(off[-1])
    d_in = h.dev_alloc(cap); d_blk = h.dev_alloc(cap)
    try:
        assert h.synth_fastq(synth_flavour, first, recs, d_in, cap) == cap
        starts, sizes = bench.cut_blocks(off, blocks)
        b_offs, b_sizes, _, _ = h.compress_batch_device(d_in, starts, sizes, d_blk, cap)
        cols = columns.decode_columns(h, d_blk, b_offs, b_sizes, device, titles=False)
    finally:
        h.dev_free(d_in); h.dev_free(d_blk)
    try:
        h.release_memory()
        R, S = cols.n_records, cols.bases.numel()
        C = min(max(int(cols.seq_offsets.diff().max()), 1), _lib.PROFILE_MAX_CYCLES)
        quality = dict(quality_5=20, quality_3=20, min_length=1)
        prof_s, prof = timed(device, steps, lambda: columns.profile_columns(h, cols, n_cycles=C))
        trim_s, (begin, end, keep, trim_stats) = timed(device, steps, lambda: columns.trim_plan(h, cols, **quality))
        out = {"profile_columns": dict(figures(2 * S + 8 * (R + 1), prof_s), totals=prof.summary()),
               "trim_plan_both_ends": dict(figures(S + (trim_stats["bases_kept"] + trim_stats["bases_cut"]) + 8 * (R + 1) + 17 * R, trim_s), stats=trim_stats)}
        torch_s = None
        if torch_ops:
            torch_s, want = timed(device, steps, lambda: profile_torch(cols, C))
            assert torch.equal(prof.data, want), "the torch tables differ from the library's"
            out["torch_ops_same_tables"] = figures(2 * S + 8 * (R + 1), torch_s)
        for c in cycles:
            c_s, c_prof = timed(device, steps, lambda: columns.profile_columns(h, cols, n_cycles=c))
            assert c_prof.summary() == prof.summary()
            out["profile_columns_n_cycles_%d" % c] = figures(2 * S + 8 * (R + 1), c_s)
        if with_plan:
            after_s, after = timed(device, steps, lambda: columns.profile_columns(h, cols, begin, end, keep, n_cycles=C))
            out["profile_columns_under_the_quality_plan"] = dict(figures(2 * trim_stats["bases_kept"] + 8 * (R + 1) + 17 * R, after_s), totals=after.summary())
    finally:
        h.close()
    med = statistics.median
    print(json.dumps(dict({"case": f"columnar profile, flavour 0 ({name}), device-resident", "blocks": blocks, "steps": steps, "records": R, "bases": S,
                           "n_cycles": C,
                           "figures": "host wall time around the synchronous call of dsrc_amd/columns.py (torch's allocation of the outputs included); "
                                      "bytes: the least the call must read; GBps_median = bytes / median time; floor = bytes at 8 TB/s"}, **out,
                          profile_ms_over_trim_ms=round(med(prof_s) / med(trim_s), 3) if min(trim_s) > 0 else None,
                          torch_ms_over_profile_ms=round(med(torch_s) / med(prof_s), 3) if torch_s and min(prof_s) > 0 else None)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--blocks", type=int, default=45, help="8 MiB chunks of FASTQ text the records come from (45: a million reads of 150 bases)")
    ap.add_argument("--steps", type=int, default=5, help="timed calls (at least 5: the spread is min..max)")
    ap.add_argument("--chunk-mb", type=float, default=8.0, help="chunk size (smaller: toy runs)")
    ap.add_argument("--device", default="cuda:0", help="torch device of the arrays (cpu with the emulator build)")
    ap.add_argument("--plan", action="store_true", help="also time the profile under the quality plan")
    ap.add_argument("--cycles", default="", help="comma-separated n_cycles to time the profile at as well")
    ap.add_argument("--skip-torch", action="store_true", help="leave the torch-ops version out (under a profiler)")
    a = ap.parse_args()
    if a.chunk_mb != 8.0:
        bench.BUF = int(a.chunk_mb * (1 << 20)); bench.RECS_PER_BLOCK = max(8, int(bench.RECS_PER_BLOCK * a.chunk_mb / 8))
    run(a.blocks, max(a.steps, 5), torch.device(a.device), a.plan, [int(c) for c in a.cycles.split(",") if c], not a.skip_torch)


if __name__ == "__main__":
    main()
