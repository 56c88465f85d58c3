#!/usr/bin/env python3
"""What the columnar select costs: records generated in HBM (dsrcgpu_synth_fastq flavour 0, Illumina-like reads of one length, and
flavour 2, variable-length 454/Ion-Torrent-like reads), compressed (-d0 -q0, the Ion-Torrent-like reads at -d2 -q1 lossy as in BASELINE's configuration 5) and decoded into arrays by decode_columns; then
trim_plan (dsrcgpu_columns_trim_plan) and select_columns (dsrcgpu_columns_select_device, sizing call + filling call) of
dsrc_amd/columns.py on those tensors: one warm-up and --steps timed calls each, host wall time around the synchronous call as
min / median / max, the bytes the call has to read and write at the least, and the GB/s that follows.  Beside it the same selection
done with torch ops on the same tensors (cumsum, repeat_interleave, index), checked to give the same arrays: the yardstick.
A timing tool, not a gate.  With the emulator build of the library (DSRC_GPU_LIB, --device cpu) it runs end to end and the figures mean
nothing.  Results go to profiles/."""
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
import bench  # noqa: E402
from config_bench import record_offsets  # noqa: E402
from dsrc_amd import _lib, columns  # noqa: E402
from dsrc_amd.config import Config  # noqa: E402

FLAVOURS = {0: ("illumina", _lib.SYNTH_ILLUMINA, 8 * (1 << 20) / bench.RECS_PER_BLOCK, (0, 0, False), dict(quality_3=25, min_length=60, max_n=1, min_mean_quality=28)),
            2: ("454/Ion-Torrent-like", _lib.SYNTH_IONTORRENT, 596.0, (2, 1, True), dict(quality_5=5, quality_3=25, min_length=40, max_n=5, min_mean_quality=5))}


def timed(device, steps, call):
    def once():
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        t = time.perf_counter()
        res = call()
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        return time.perf_counter() - t, res
    once()                                                   # warm-up: arena, kernels loaded, torch's allocator
    runs = [once() for _ in range(steps)]
    return [r[0] for r in runs], runs[-1][1]


def figures(nbytes, secs):
    ms = sorted(s * 1e3 for s in secs)
    med = statistics.median(ms)
    return {"ms": {"min": round(ms[0], 3), "median": round(med, 3), "max": round(ms[-1], 3)}, "bytes": int(nbytes),
            "GBps_median": round(nbytes / med / 1e6, 1) if med > 0 else None}


def torch_select(cols, begin, end, keep):
    """The same compaction with torch ops: the yardstick."""
    k = keep != 0
    b = begin[k]; lens = (end - begin)[k]
    offs = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=lens.device); torch.cumsum(lens, 0, out=offs[1:])
    idx = torch.repeat_interleave(b - offs[:-1], lens) + torch.arange(int(offs[-1]), device=lens.device)
    t0 = cols.title_offsets[:-1][k]; tl = (cols.title_offsets[1:] - cols.title_offsets[:-1])[k]
    toffs = torch.zeros(tl.numel() + 1, dtype=torch.int64, device=tl.device); torch.cumsum(tl, 0, out=toffs[1:])
    tidx = torch.repeat_interleave(t0 - toffs[:-1], tl) + torch.arange(int(toffs[-1]), device=tl.device)
    return cols.bases[idx], cols.quals[idx], cols.titles[tidx], offs, toffs


def run(flavour, blocks, steps, device, first=1):
    name, synth_flavour, rec_bytes, levels, rules = FLAVOURS[flavour]
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
        cols = columns.decode_columns(h, d_blk, b_offs, b_sizes, device)
    finally:
        h.dev_free(d_in); h.dev_free(d_blk)
    try:
        h.release_memory()
        R, S, T = cols.n_records, cols.bases.numel(), cols.titles.numel()
        plan_s, (begin, end, keep, stats) = timed(device, steps, lambda: columns.trim_plan(h, cols, **rules))
        sel_s, sel = timed(device, steps, lambda: columns.select_columns(h, cols, begin, end, keep))
        torch_s, ref = timed(device, steps, lambda: torch_select(cols, begin, end, keep))
        K, Sk, Tk = sel.n_records, sel.bases.numel(), sel.titles.numel()
        for mine, theirs in zip((sel.bases, sel.quals, sel.titles, sel.seq_offsets, sel.title_offsets), ref):
            assert torch.equal(mine, theirs), "the library's selection differs from the torch ops'"
        assert [K, Sk] == [stats["records_kept"], stats["bases_kept"]]
    finally:
        h.close()
    # the least a call has to move: the plan reads the qualities, the bases of the kept range and the offsets and writes 17 bytes a
    # record; the select reads offsets, ranges and flags, reads and writes the kept payload, writes the new offsets
    plan_bytes = S + (stats["bases_kept"] + stats["bases_cut"]) + 8 * (R + 1) + 17 * R
    sel_bytes = 16 * (R + 1) + 17 * R + 2 * (2 * Sk + Tk) + 16 * (K + 1)
    print(json.dumps({"case": f"columnar select, flavour {flavour} ({name}), device-resident", "blocks": blocks, "steps": steps,
                      "records": R, "bases": S, "title_bytes": T, "rules": rules, "stats": stats, "kept_title_bytes": Tk,
                      "figures": "host wall time around the synchronous call of dsrc_amd/columns.py (select_columns: sizing call + filling call + "
                                 "torch's allocations); bytes: the least the call must read plus write; GBps_median = bytes / median time",
                      "trim_plan": figures(plan_bytes, plan_s), "select_columns": figures(sel_bytes, sel_s),
                      "torch_select": figures(sel_bytes, torch_s),
                      "torch_ms_over_select_ms": round(statistics.median(torch_s) / statistics.median(sel_s), 3) if min(sel_s) > 0 else None}), flush=True)


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
