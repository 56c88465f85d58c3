#!/usr/bin/env python3
"""What the columnar encode costs next to the text encode: Illumina records generated in HBM (dsrcgpu_synth_fastq flavour 0),
compressed at -d3 -q2 and at -d0 -q0 by dsrcgpu_compress_batch_device (text), decoded once into arrays
(dsrcgpu_decompress_batch_columns_device), and the SAME records compressed again from those arrays by
dsrcgpu_compress_columns_device with the decoder's block_records -- the blocks must come out with the sizes of the text call's.
Per entry point: one warm-up, then --steps timed calls on one handle; the figure is the HIP-event time of the call's stream work
(dsrcgpu_last_timing; for the columns call it starts in front of the check pass and includes the scatter of the text), reported as
raw FASTQ MB/s with min / median / max over the timed calls, and the host wall time beside it.  dsrcgpu_columns_cut is timed on the
side (wall time, 8 MiB of text per block).  A timing tool, not a gate: the yardstick of the columns call is the text call of the
same run.  Results go to profiles/."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
from columns_bench import rates, timed  # noqa: E402
from dsrc_amd import _lib  # noqa: E402
from dsrc_amd.config import Config  # noqa: E402


def run(d, q, blocks, steps, first=1):
    cfg = Config.from_levels(d, q)
    h = _lib.Handle(cfg.dna_order, cfg.quality_order, cfg.lossy, cfg.crc)
    h.set_lanes(1)                                           # the columns call is never cut into sub-batches: neither is its yardstick
    recs = int(blocks * bench.RECS_PER_BLOCK * 1.02) + 1000
    off = bench.record_offsets(first, recs)
    cap = int(off[-1])
    held = []

    def alloc(n):
        p = h.dev_alloc(max(n, 8)); held.append(p)
        return p
    try:
        d_in = alloc(cap); d_blk = alloc(cap // 2); d_blk2 = alloc(cap // 2)
        assert h.synth_fastq(_lib.SYNTH_ILLUMINA, first, recs, d_in, cap) == cap
        starts, sizes = bench.cut_blocks(off, blocks)
        text_bytes = sum(sizes) + len(sizes)
        b_offs, b_sizes, _, _ = h.compress_batch_device(d_in, starts, sizes, d_blk, cap // 2)
        try:
            h.decompress_columns_device(d_blk, b_offs, b_sizes, _lib.Columns())
            raise AssertionError("the sizing call must report DSRCGPU_E_CAPACITY")
        except _lib.DsrcGpuError as e:
            if e.code != _lib.E_CAPACITY:
                raise
            R, S, T = e.need
        cols = _lib.Columns(alloc(S), S, alloc(S), S, alloc(T), T, alloc(8 * (R + 1)), alloc(8 * (R + 1)), R)
        block_records, _ = h.decompress_columns_device(d_blk, b_offs, b_sizes, cols)
        cin = _lib.ColumnsIn(cols.d_bases, S, cols.d_quals, cols.d_titles, T, cols.d_seq_offs, cols.d_title_offs, R)

        h.set_fields_capacity(0)
        t_ev, t_wall = timed(h, steps, lambda: h.compress_batch_device(d_in, starts, sizes, d_blk, cap // 2))
        h.set_fields_capacity(0)
        c_ev, c_wall = timed(h, steps, lambda: h.compress_columns_device(cin, block_records, d_blk2, cap // 2))
        # the same records, the same state at the start of the first call of each series: the last calls' blocks have the same sizes
        h.set_fields_capacity(0)
        want = h.compress_batch_device(d_in, starts, sizes, d_blk, cap // 2)[1]
        h.set_fields_capacity(0)
        got = h.compress_columns_device(cin, block_records, d_blk2, cap // 2)[1]
        assert got == want, "the columns call wrote blocks of other sizes than the text call"
        t = time.perf_counter()
        cut = h.columns_cut(cin, bench.BUF)
        cut_ms = (time.perf_counter() - t) * 1e3
        h.release_memory()
    finally:
        for p in held:
            h.dev_free(p)
        h.close()
    text, colm = rates(text_bytes, t_ev), rates(text_bytes, c_ev)
    print(json.dumps({"case": f"encode -d{d} -q{q}: text against columns (device-resident, one scheduler lane)", "blocks": blocks, "steps": steps,
                      "fastq_bytes": text_bytes, "records": R, "bases": S, "title_bytes": T,
                      "figures": "*_MBps: fastq_bytes over the HIP-event time of the call's stream work (dsrcgpu_last_timing; the columns call's "
                                 "starts in front of its check pass and spans the host's layout of the chunks and the scatter); *_wall_MBps: "
                                 "fastq_bytes over the host wall time of the whole call; min / median / max over `steps` calls",
                      "text_MBps": text, "columns_MBps": colm, "columns_over_text": round(colm["median"] / text["median"], 3) if text and colm else None,
                      "text_wall_MBps": rates(text_bytes, t_wall), "columns_wall_MBps": rates(text_bytes, c_wall),
                      "columns_cut_blocks": len(cut) - 1, "columns_cut_wall_ms": round(cut_ms, 3)}), flush=True)


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
