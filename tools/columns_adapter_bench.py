#!/usr/bin/env python3
"""What the columnar adapter search costs: records generated in HBM (dsrcgpu_synth_fastq flavour 0, Illumina-like reads of one
length, and flavour 2, variable-length 454/Ion-Torrent-like reads), compressed and decoded into arrays by decode_columns as in
tools/columns_filter_bench.py; torch ops on the device then write the head of an adapter over the 3' end of about a third of the
reads.  Timed on those tensors: adapter_plan (dsrcgpu_columns_adapter_plan) of dsrc_amd/columns.py with 1 and with 4 adapters of 33
bases, and beside them trim_plan (dsrcgpu_columns_trim_plan) with both ends on -- existing code that reads the same arrays: the
yardstick.  One warm-up and --steps timed calls each, host wall time around the synchronous call as min / median / max, the bytes
the call has to read and write at the least, the GB/s that follows and the time those bytes take at 8 TB/s (the floor).
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
from columns_filter_bench import FLAVOURS, timed  # noqa: E402
from config_bench import record_offsets  # noqa: E402
from dsrc_amd import _lib, columns  # noqa: E402
from dsrc_amd.config import Config  # noqa: E402

# 33 bases each (public Illumina sequences: TruSeq read 1 and read 2, Nextera, small RNA 3'); the first one is planted
ADAPTERS = ["AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT", "CTGTCTCTTATACACATCTCCGAGCCCACGAGA", "TGGAATTCTCGGGTGCCAAGGAACTCCAGTCAC"]
HBM_BPS = 8e12


def plant(cols, adapter, seed=1):
    """The first k bases of `adapter` over the last k bases of about a third of the reads, k = 1 .. min(length, 2 * len(adapter)) drawn
    per read (beyond the adapter's length the read keeps what it had behind the adapter), with torch ops on the device of the arrays."""
    dev = cols.bases.device
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    S = cols.seq_offsets
    R = cols.n_records
    lens = S[1:] - S[:-1]
    chosen = (torch.rand(R, generator=g) < 1 / 3).to(dev) & (lens > 0)
    tail = (torch.rand(R, generator=g).to(dev) * torch.clamp(lens, max=2 * len(adapter)).double()).long() + 1
    tail = torch.minimum(tail, lens)
    start = torch.where(chosen, S[1:] - tail, S[1:])         # position in bases of the adapter's first base; S[r + 1]: none
    pos = torch.arange(cols.bases.numel(), device=dev)
    rec = torch.bucketize(pos, S[1:], right=True)
    rel = pos - start[rec]
    hit = (rel >= 0) & (rel < len(adapter))
    codes = torch.tensor(["ACGT".index(c) for c in adapter], dtype=torch.uint8, device=dev)
    cols.bases[hit] = codes[rel[hit]]
    return int(chosen.sum())


def figures(nbytes, secs):
    ms = sorted(s * 1e3 for s in secs)
    med = statistics.median(ms)
    return {"ms": {"min": round(ms[0], 3), "median": round(med, 3), "max": round(ms[-1], 3)}, "bytes": int(nbytes),
            "GBps_median": round(nbytes / med / 1e6, 1) if med > 0 else None, "floor_ms_at_8TBps": round(nbytes / HBM_BPS * 1e3, 4)}


def run(flavour, blocks, steps, device, first=1):
    name, synth_flavour, rec_bytes, levels, _ = FLAVOURS[flavour]
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
        n_planted = plant(cols, ADAPTERS[0])
        R, S = cols.n_records, cols.bases.numel()
        quality = dict(quality_5=20, quality_3=20, min_length=1)
        trim_s, (_, _, _, trim_stats) = timed(device, steps, lambda: columns.trim_plan(h, cols, **quality))
        one_s, (_, _, _, one) = timed(device, steps, lambda: columns.adapter_plan(h, cols, ADAPTERS[:1]))
        four_s, (_, _, _, four) = timed(device, steps, lambda: columns.adapter_plan(h, cols, ADAPTERS))
        assert one["records_trimmed"] >= n_planted * 0.7 and four["records_trimmed"] >= one["records_trimmed"]
    finally:
        h.close()
    # the least a call has to move: the adapter plan reads the bases and the offsets and writes 17 bytes a record; the quality plan
    # reads the qualities, the bases of the kept range and the offsets and writes the same 17 bytes
    adapt_bytes = S + 8 * (R + 1) + 17 * R
    trim_bytes = S + (trim_stats["bases_kept"] + trim_stats["bases_cut"]) + 8 * (R + 1) + 17 * R
    med = statistics.median
    print(json.dumps({"case": f"columnar adapter plan, flavour {flavour} ({name}), device-resident", "blocks": blocks, "steps": steps,
                      "records": R, "bases": S, "records_planted": n_planted, "adapter_bases": len(ADAPTERS[0]),
                      "figures": "host wall time around the synchronous call of dsrc_amd/columns.py (torch's allocation of the outputs included); "
                                 "bytes: the least the call must read plus write; GBps_median = bytes / median time; floor = bytes at 8 TB/s",
                      "adapter_plan_1": dict(figures(adapt_bytes, one_s), stats=one), "adapter_plan_4": dict(figures(adapt_bytes, four_s), stats=four),
                      "trim_plan_both_ends": dict(figures(trim_bytes, trim_s), stats=trim_stats),
                      "adapter_1_ms_over_trim_ms": round(med(one_s) / med(trim_s), 3) if min(trim_s) > 0 else None,
                      "adapter_4_ms_over_adapter_1_ms": round(med(four_s) / med(one_s), 3) if min(one_s) > 0 else None}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--blocks", type=int, default=24, help="8 MiB chunks of FASTQ text the records come from")
    ap.add_argument("--steps", type=int, default=5, help="timed calls (at least 5: the spread is min..max)")
    ap.add_argument("--chunk-mb", type=float, default=8.0, help="chunk size (smaller: toy runs)")
    ap.add_argument("--device", default="cuda:0", help="torch device of the arrays (cpu with the emulator build)")
    a = ap.parse_args()
    if a.chunk_mb != 8.0:
        bench.BUF = int(a.chunk_mb * (1 << 20)); bench.RECS_PER_BLOCK = max(8, int(bench.RECS_PER_BLOCK * a.chunk_mb / 8))
    for flavour in (0, 2):
        run(flavour, a.blocks, max(a.steps, 5), torch.device(a.device))


if __name__ == "__main__":
    main()
