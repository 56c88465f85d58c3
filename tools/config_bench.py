#!/usr/bin/env python3
"""Device-resident throughput of the BASELINE configurations bench.py does not time: configuration 2 (Illumina records, -d0 -q0)
and configuration 5 (variable-length 454/Ion-Torrent-like records with IUPAC codes, -d2 -q1, lossy).  Per leg: the records are
generated in HBM (dsrcgpu_synth_fastq flavour 0 / 2), cut into chunks where the reference's reader would cut them, and pushed through
dsrcgpu_compress_batch_device on ONE handle: one warm-up call, then --steps timed calls; blocks stay in HBM.  Two blocks of the last
call are compared with the oracle when it is built.  Not the headline metric (bench.py); results go to profiles/."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from dsrc_amd import _lib, synth  # noqa: E402
from dsrc_amd.config import Config  # noqa: E402

ORACLE_LIB = os.path.join(ROOT, "oracle", "liboracle.so")

# name -> (case text, synthetic flavour, compression levels, mean record size in bytes for the first guess of the record count)
LEGS = {
    "config2": ("config2 illumina -d0 -q0 (device-resident)", _lib.SYNTH_ILLUMINA, (0, 0, False), 8 * (1 << 20) / bench.RECS_PER_BLOCK),
    "config5": ("config5 454/Ion-Torrent-like -d2 -q1 -l (device-resident)", _lib.SYNTH_IONTORRENT, (2, 1, True), 596.0),
}


def record_offsets(flavour, first, count):
    if flavour == _lib.SYNTH_IONTORRENT:
        off = np.zeros(count + 1, dtype=np.int64)
        np.cumsum(synth.iontorrent_record_sizes(first, count), out=off[1:])
        return off
    return bench.record_offsets(first, count)


def run(name, blocks, steps, first=1):
    case, flavour, (d, q, lossy), rec_bytes = LEGS[name]
    cfg = Config.from_levels(d, q, lossy)
    h = _lib.Handle(cfg.dna_order, cfg.quality_order, cfg.lossy, cfg.crc)
    recs = int(blocks * bench.BUF / rec_bytes * 1.02) + 1000
    off = record_offsets(flavour, first, recs)
    cap = int(off[-1])
    d_in = h.dev_alloc(cap); d_out = h.dev_alloc(cap // 2)
    try:
        h.synth_fastq(flavour, first, min(recs, 1024), d_in, cap)          # the generator's kernels are loaded before it is timed
        t = time.perf_counter()
        nbytes = h.synth_fastq(flavour, first, recs, d_in, cap)
        gen_s = time.perf_counter() - t
        assert nbytes == cap, (nbytes, cap)
        starts, sizes = bench.cut_blocks(off, blocks)
        assert len(starts) == blocks, f"{recs} records give {len(starts)} chunks, not {blocks}"
        sample = sorted({0, blocks - 1}) if os.path.exists(ORACLE_LIB) else []
        chunks = [h.dev_download(d_in + starts[i], sizes[i]) for i in sample]
        h.compress_batch_device(d_in, starts, sizes, d_out, cap // 2)
        fields_cap = h.get_fields_capacity()          # every title has the same number of fields: the block-to-block state stays here
        t = time.perf_counter()
        for _ in range(steps):
            o_offs, o_sizes, _, _ = h.compress_batch_device(d_in, starts, sizes, d_out, cap // 2)
        dt = (time.perf_counter() - t) / steps
        ms, rc_ms, _ = h.last_timing()
        if sample:
            from tests._oracle import Oracle
            assert h.get_fields_capacity() == fields_cap
            orc = Oracle()
            for i, chunk in zip(sample, chunks):
                want = orc.compress_blocks_state(cfg, [chunk], fields_cap)[0][0]
                assert h.dev_download(d_out + o_offs[i], o_sizes[i]) == want, f"{name}: block {i} differs from the oracle's"
    finally:
        h.dev_free(d_in); h.dev_free(d_out); h.close()
    nin = sum(sizes) + len(sizes); nout = sum(o_sizes)
    print(json.dumps({"case": case, "blocks": blocks, "in_bytes": nin, "out_bytes": nout, "ratio": round(nout / nin, 4),
                      "value_MBps": round(nin / dt / 1e6, 1), "gpu_batch_ms": round(ms, 1), "rc_ms": round(rc_ms, 1),
                      "oracle_checked": len(sample), "steps": steps, "synth_bytes": nbytes, "synth_MBps": round(nbytes / gen_s / 1e6, 1)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--blocks", type=int, default=450, help="chunks per call")
    ap.add_argument("--steps", type=int, default=3, help="timed calls per leg, after one warm-up call")
    ap.add_argument("--chunk-mb", type=int, default=8, help="chunk size in MiB (the reference's -b)")
    ap.add_argument("--legs", default="config2,config5", help="comma-separated: " + ", ".join(LEGS))
    a = ap.parse_args()
    legs = a.legs.split(",")
    for name in legs:
        if name not in LEGS:
            ap.error(f"unknown leg {name!r}")
    if a.blocks < 1 or a.steps < 1 or a.chunk_mb < 1:
        ap.error("--blocks, --steps and --chunk-mb are at least 1")
    bench.BUF = a.chunk_mb << 20          # what cut_blocks cuts by
    for name in legs:
        run(name, a.blocks, a.steps)


if __name__ == "__main__":
    main()
