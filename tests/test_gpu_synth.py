"""The device generators of dsrcgpu_synth_fastq on the MI355X: flavour 2 (variable-length 454/Ion-Torrent-like records, BASELINE
configuration 5) byte for byte against dsrc_amd/synth.py iontorrent_fastq, flavours 0 and 1 against illumina_fastq, the records
compressed where they were generated, and tools/config_bench.py end to end at a toy size."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from dsrc_amd import synth
from tests._oracle import Config

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_CAPACITY = -4          # include/dsrc_gpu.h


@pytest.fixture(scope="module")
def gpu():
    if not os.environ.get("DSRC_TEST_KEEP_GPU_LIB"):          # (set to run this suite on a variant build: tools/variant_bench.sh)
        os.environ.pop("DSRC_GPU_LIB", None)
    from dsrc_amd import _lib
    _lib._lib = None
    return _lib


def check_equal(gpu, flavour, first, count, want):
    h = gpu.Handle()
    cap = len(want) + 4096
    d = h.dev_alloc(cap)
    try:
        h.dev_upload(d, b"\xA5" * cap)
        n = h.synth_fastq(flavour, first, count, d, cap)
        buf = h.dev_download(d, cap)
    finally:
        h.dev_free(d); h.close()
    assert n == len(want)
    if buf[:n] != want:
        k = next(j for j in range(n) if buf[j] != want[j])
        lo = want.rfind(b"\n@", 0, k) + 1
        pytest.fail(f"first difference at byte {k}: want {want[lo: k + 40]!r}, got {buf[lo: k + 40]!r}")
    assert buf[n:] == b"\xA5" * (cap - n), "bytes written past the end of the last record"


@pytest.mark.parametrize("first,count", [(1, 1500), (999990, 1200), (9999999990, 40)])
def test_iontorrent_matches_host(gpu, first, count):
    """Two groups of 1024 records with every length class (40, 63..65, 127..129, 500); an id that grows a digit; ids beyond 2^32."""
    check_equal(gpu, gpu.SYNTH_IONTORRENT, first, count, synth.iontorrent_fastq(count, first=first))


def test_iontorrent_capacity(gpu):
    need = int(synth.iontorrent_record_sizes(1, 1500).sum())
    h = gpu.Handle()
    d = h.dev_alloc(need + 64)
    try:
        h.dev_upload(d, b"\xA5" * (need + 64))
        with pytest.raises(gpu.DsrcGpuError) as e:
            h.synth_fastq(gpu.SYNTH_IONTORRENT, 1, 1500, d, need - 1)
        assert e.value.code == E_CAPACITY
        assert h.dev_download(d, need + 64) == b"\xA5" * (need + 64), "the refused call wrote to the buffer"
    finally:
        h.dev_free(d); h.close()


@pytest.mark.parametrize("binned", [False, True])
def test_illumina_flavours_unchanged(gpu, binned):
    flavour = gpu.SYNTH_ILLUMINA_BINNED if binned else gpu.SYNTH_ILLUMINA
    check_equal(gpu, flavour, 999990, 1200, synth.illumina_fastq(1200, first=999990, binned=binned))


def test_generated_records_compress_on_the_device(gpu, oracle):
    """4000 flavour-2 records cut into two chunks at a record boundary and compressed where they lie, at -d2 -q1 -l."""
    cfg = Config.from_levels(2, 1, True)
    recs, cut = 4000, 2100
    off = np.concatenate(([0], np.cumsum(synth.iontorrent_record_sizes(1, recs))))
    cap = int(off[-1])
    starts = [0, int(off[cut])]; sizes = [int(off[cut]) - 1, cap - int(off[cut]) - 1]
    h = gpu.Handle(cfg.dna_order, cfg.quality_order, cfg.lossy, cfg.crc, cfg.quality_offset)
    d_in = h.dev_alloc(cap); d_out = h.dev_alloc(cap)
    try:
        assert h.synth_fastq(gpu.SYNTH_IONTORRENT, 1, recs, d_in, cap) == cap
        chunks = [h.dev_download(d_in + s, z) for s, z in zip(starts, sizes)]
        o_offs, o_sizes, raw, comp = h.compress_batch_device(d_in, starts, sizes, d_out, cap)
        got = [h.dev_download(d_out + o, z) for o, z in zip(o_offs, o_sizes)]
    finally:
        h.dev_free(d_in); h.dev_free(d_out); h.close()
    assert chunks[0].startswith(b"@GXYZ1234.1 ") and chunks[1].startswith(b"@GXYZ1234.%d " % (cut + 1))
    want = oracle.compress_blocks_state(cfg, chunks)
    for i in range(2):
        assert got[i] == want[i][0], f"chunk {i}: block bytes differ"
        assert raw[4 * i: 4 * i + 4] == want[i][1] and comp[4 * i: 4 * i + 4] == want[i][2], f"chunk {i}: stream sizes differ"


def test_config_bench_tool(gpu):
    """The tool in a process of its own, at a toy size: both legs, the keys of its JSON lines, the oracle spot check."""
    env = dict(os.environ)
    if not os.environ.get("DSRC_TEST_KEEP_GPU_LIB"):
        env.pop("DSRC_GPU_LIB", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "config_bench.py"), "--blocks", "2", "--steps", "1", "--chunk-mb", "1"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [json.loads(x) for x in p.stdout.decode().splitlines() if x.startswith("{")]
    assert len(lines) == 2
    assert lines[0]["case"].startswith("config2") and lines[1]["case"].startswith("config5")
    for r in lines:
        for key in ("case", "blocks", "in_bytes", "out_bytes", "ratio", "value_MBps", "gpu_batch_ms", "rc_ms", "oracle_checked"):
            assert key in r, key
        assert r["blocks"] == 2 and 1.9e6 < r["in_bytes"] < 2.2e6 and 0 < r["out_bytes"] < r["in_bytes"] and r["value_MBps"] > 0
        if os.path.exists(os.path.join(ROOT, "oracle", "liboracle.so")):
            assert r["oracle_checked"] >= 1
