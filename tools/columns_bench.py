#!/usr/bin/env python3
"""What the columnar decode costs next to the text decode: Illumina records generated in HBM (dsrcgpu_synth_fastq flavour 0),
compressed on the device at -d3 -q2 and at -d0 -q0, then the SAME blocks decoded by dsrcgpu_decompress_batch_device (text) and
by dsrcgpu_decompress_batch_columns_device (bases, qualities, titles, offsets).  Per call: one warm-up, then --steps timed calls;
the figure is the HIP-event time of the call's stream work (dsrcgpu_last_timing: first launch to last kernel, the columns'
gather included), reported as raw FASTQ MB/s with min / median / max over the timed calls, and the host wall time beside it.
A timing tool, not a gate: the yardstick of the columns call is the text call of the same run.  Results go to profiles/."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from dsrc_amd import _lib  # noqa: E402
from dsrc_amd.config import Config  # noqa: E402


def timed(h, steps, call):
    call()                                                   # warm-up: arena, table region, kernels loaded
    ev, wall = [], []
    for _ in range(steps):
        t = time.perf_counter()
        call()
        wall.append(time.perf_counter() - t)
        ev.append(h.last_timing()[0] / 1e3)
    return ev, wall


def rates(nbytes, secs):
    if min(secs) <= 0:                                       # (the emulator build has no event clock)
        return None
    mb = sorted(nbytes / s / 1e6 for s in secs)
    return {"min": round(mb[0], 1), "median": round(statistics.median(mb), 1), "max": round(mb[-1], 1)}


def run(d, q, blocks, steps, first=1):
    cfg = Config.from_levels(d, q)
    h = _lib.Handle(cfg.dna_order, cfg.quality_order, cfg.lossy, cfg.crc)
    recs = int(blocks * bench.RECS_PER_BLOCK * 1.02) + 1000
    off = bench.record_offsets(first, recs)
    cap = int(off[-1])
    held = []

    def alloc(n):
        p = h.dev_alloc(max(n, 8)); held.append(p)
        return p
    try:
        d_in = alloc(cap); d_blk = alloc(cap // 2)
        assert h.synth_fastq(_lib.SYNTH_ILLUMINA, first, recs, d_in, cap) == cap
        starts, sizes = bench.cut_blocks(off, blocks)
        b_offs, b_sizes, _, _ = h.compress_batch_device(d_in, starts, sizes, d_blk, cap // 2)
        text_bytes = sum(sizes) + len(sizes)
        d_txt = alloc(text_bytes + 64)
        t_ev, t_wall = timed(h, steps, lambda: h.decompress_batch_device(d_blk, b_offs, b_sizes, d_txt, text_bytes + 64))
        try:
            h.decompress_columns_device(d_blk, b_offs, b_sizes, _lib.Columns())
            raise AssertionError("the sizing call must report DSRCGPU_E_CAPACITY")
        except _lib.DsrcGpuError as e:
            if e.code != _lib.E_CAPACITY:
                raise
            R, S, T = e.need
        cols = _lib.Columns(alloc(S), S, alloc(S), S, alloc(T), T, alloc(8 * (R + 1)), alloc(8 * (R + 1)), R)
        c_ev, c_wall = timed(h, steps, lambda: h.decompress_columns_device(d_blk, b_offs, b_sizes, cols))
        h.release_memory()
    finally:
        for p in held:
            h.dev_free(p)
        h.close()
    text, colm = rates(text_bytes, t_ev), rates(text_bytes, c_ev)
    print(json.dumps({"case": f"decode -d{d} -q{q}: text against columns (device-resident)", "blocks": blocks, "steps": steps,
                      "fastq_bytes": text_bytes,
                      "figures": "*_MBps: fastq_bytes over the HIP-event time of the call's stream work (dsrcgpu_last_timing: first launch to "
                                 "last kernel; for columns it spans the host's capacity check between k_col_sizes and k_col_gather); "
                                 "*_wall_MBps: fastq_bytes over the host wall time of the whole call; min / median / max over `steps` calls", "records": R, "bases": S, "title_bytes": T,
                      "text_MBps": text, "columns_MBps": colm, "columns_over_text": round(colm["median"] / text["median"], 3) if text and colm else None,
                      "text_wall_MBps": rates(text_bytes, t_wall), "columns_wall_MBps": rates(text_bytes, c_wall)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--blocks", type=int, default=96, help="8 MiB chunks per batch")
    ap.add_argument("--steps", type=int, default=5, help="timed calls per entry point (at least 5: the spread is min..max)")
    ap.add_argument("--chunk-mb", type=float, default=8.0, help="chunk size (8 = the reference's -b8; smaller: toy runs)")
    a = ap.parse_args()
    if a.chunk_mb != 8.0:
        bench.BUF = int(a.chunk_mb * (1 << 20)); bench.RECS_PER_BLOCK = max(8, int(bench.RECS_PER_BLOCK * a.chunk_mb / 8))
    for d, q in ((3, 2), (0, 0)):
        run(d, q, a.blocks, max(a.steps, 5))


if __name__ == "__main__":
    main()
