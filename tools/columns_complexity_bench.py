#!/usr/bin/env python3
"""What the columnar complexity plan costs: records generated in HBM (dsrcgpu_synth_fastq flavour 0, Illumina-like reads of one
length, and flavour 2, variable-length 454/Ion-Torrent-like reads), compressed and decoded into arrays by decode_columns as in
tools/columns_adapter_bench.py; torch ops on the device then write a poly-G tail of 1 .. 60 bases over the 3' end of about a third of
the reads.  Timed on those tensors: complexity_plan (dsrcgpu_columns_complexity_plan) of dsrc_amd/columns.py with tail="G", with
tail="ACGT" and head="T", with the complexity filter on as well, and with DUST on as well; beside them the yardsticks trim_plan
(both ends) and adapter_plan (one adapter of 33 bases) -- existing code that reads the same arrays.  For the reads of one length the
same tail cut is also computed from torch ops (flip, cumsum, masked argmax): first the cuts are compared, then that is timed.
One warm-up and --steps timed calls each, host wall time around the synchronous call as min / median / max, the bytes the call has
to read and write at the least, the GB/s that follows and the time those bytes take at 8 TB/s (the floor).
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
from columns_adapter_bench import ADAPTERS, figures  # noqa: E402
from columns_filter_bench import FLAVOURS, timed  # noqa: E402
from config_bench import record_offsets  # noqa: E402
from dsrc_amd import _lib, columns  # noqa: E402
from dsrc_amd.config import Config  # noqa: E402

G = 2
POLY = dict(poly_min_length=10, poly_max_error_permille=125)


def plant(cols, seed=1):
    """A run of G over the last k bases of about a third of the reads, k = 1 .. min(length, 60) drawn per read, with torch ops on the
    device of the arrays."""
    dev = cols.bases.device
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    S = cols.seq_offsets
    R = cols.n_records
    lens = S[1:] - S[:-1]
    chosen = (torch.rand(R, generator=g) < 1 / 3).to(dev) & (lens > 0)
    tail = torch.minimum((torch.rand(R, generator=g).to(dev) * 60).long() + 1, lens)
    start = torch.where(chosen, S[1:] - tail, S[1:])         # position in bases of the tail's first base; S[r + 1]: none
    pos = torch.arange(cols.bases.numel(), device=dev)
    rec = torch.bucketize(pos, S[1:], right=True)
    cols.bases[pos >= start[rec]] = G
    return int(chosen.sum())


def torch_tail_cut(cols, length, base=G, min_run=POLY["poly_min_length"], permille=POLY["poly_max_error_permille"]):
    """The 3' rule of dsrcgpu_columns_complexity_plan for one base on reads of one length, from torch ops -> the new end of every record."""
    x = cols.bases.view(-1, length).flip(1)
    m = (x == base).long().cumsum(1)
    L = torch.arange(1, length + 1, device=x.device)
    err = L - m
    score = torch.where(err * 1000 <= L * permille, m - 2 * err, torch.full_like(m, -1))
    key = score * (length + 1) + (length - L)                # the highest score, the shortest run among equal ones
    at = key.argmax(1)
    run = torch.where(score.gather(1, at[:, None])[:, 0] > 0, at + 1, torch.zeros_like(at))
    run = torch.where(run >= min_run, run, torch.zeros_like(run))
    return cols.seq_offsets[1:] - run


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
    legs, extra = {}, {}
    try:
        h.release_memory()
        n_planted = plant(cols)
        R, S = cols.n_records, cols.bases.numel()
        trim_s, (_, _, _, trim_stats) = timed(device, steps, lambda: columns.trim_plan(h, cols, quality_5=20, quality_3=20, min_length=1))
        adapt_s, (_, _, _, adapt_stats) = timed(device, steps, lambda: columns.adapter_plan(h, cols, ADAPTERS[:1]))
        for leg, kw in (("complexity_plan_tail_G", dict(tail="G")), ("complexity_plan_tail_ACGT_head_T", dict(tail="ACGT", head="T")),
                        ("complexity_plan_tail_ACGT_head_T_complexity", dict(tail="ACGT", head="T", min_complexity_permille=300)),
                        ("complexity_plan_tail_ACGT_head_T_complexity_dust", dict(tail="ACGT", head="T", min_complexity_permille=300, max_dust=20))):
            secs, got = timed(device, steps, lambda: columns.complexity_plan(h, cols, **POLY, **kw))
            legs[leg] = (secs, got)
        _, end_g, _, stats_g = legs["complexity_plan_tail_G"][1]
        assert stats_g["records_tail_cut"] >= n_planted * 0.7 and stats_g["tail_G"] == stats_g["records_tail_cut"]
        lens = cols.seq_offsets[1:] - cols.seq_offsets[:-1]
        if R and int(lens.min()) == int(lens.max()) > 0:      # reads of one length: the same cut from torch ops
            length = int(lens[0])
            assert torch.equal(torch_tail_cut(cols, length), end_g), "the torch rule and the library disagree on a tail cut"
            torch_s, _ = timed(device, steps, lambda: torch_tail_cut(cols, length))
            extra["torch_tail_G"] = dict(figures(S + 8 * R, torch_s), note="flip, cumsum, masked argmax on a (records, length) view; the cuts equal the library's")
    finally:
        h.close()
    # the least a call has to move: the bases and the offsets are read, 17 bytes a record written (no d_info here); the quality plan
    # reads the qualities as well
    plan_bytes = S + 8 * (R + 1) + 17 * R
    trim_bytes = S + (trim_stats["bases_kept"] + trim_stats["bases_cut"]) + 8 * (R + 1) + 17 * R
    med = statistics.median
    out = {"case": f"columnar complexity plan, flavour {flavour} ({name}), device-resident", "blocks": blocks, "steps": steps,
           "records": R, "bases": S, "records_planted": n_planted, "poly": POLY,
           "figures": "host wall time around the synchronous call of dsrc_amd/columns.py (torch's allocation of the outputs included); "
                      "bytes: the least the call must read plus write; GBps_median = bytes / median time; floor = bytes at 8 TB/s",
           "trim_plan_both_ends": dict(figures(trim_bytes, trim_s), stats=trim_stats),
           "adapter_plan_1": dict(figures(plan_bytes, adapt_s), stats=adapt_stats)}
    for leg, (secs, got) in legs.items():
        out[leg] = dict(figures(plan_bytes, secs), stats=got[3], ms_over_adapter_plan_1_ms=round(med(secs) / med(adapt_s), 3) if min(adapt_s) > 0 else None)
    out.update(extra)
    print(json.dumps(out), flush=True)


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
