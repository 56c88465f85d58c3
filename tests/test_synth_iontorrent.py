"""Flavour 2 of dsrcgpu_synth_fastq (variable-length 454/Ion-Torrent-like records, BASELINE configuration 5) on the CPU:
the kernel sources of dsrc_amd/csrc/k_synth.h compiled against the HIP emulator in tests/emu, driven through the C ABI
and compared byte for byte with its specification, dsrc_amd/synth.py iontorrent_fastq."""
import os
import re
import subprocess

import numpy as np
import pytest

from dsrc_amd import synth
from tests._oracle import Config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libdsrc_emu.so")

E_ARG, E_CAPACITY = -1, -4          # include/dsrc_gpu.h


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu")], stdout=subprocess.DEVNULL)
    old = os.environ.get("DSRC_GPU_LIB")
    os.environ["DSRC_GPU_LIB"] = EMU
    from dsrc_amd import _lib
    _lib._lib = None
    yield _lib
    _lib._lib = None
    if old is None:
        os.environ.pop("DSRC_GPU_LIB", None)
    else:
        os.environ["DSRC_GPU_LIB"] = old


_host = {}


def host_fastq(first, count):
    """The specification's bytes, generated once per case (a Python loop per record)."""
    if (first, count) not in _host:
        _host[first, count] = synth.iontorrent_fastq(count, first=first)
    return _host[first, count]


def device_fastq(lib, first, count):
    want = host_fastq(first, count)
    h = lib.Handle()
    cap = len(want) + 4096
    d = h.dev_alloc(cap)
    try:
        h.dev_upload(d, b"\xA5" * cap)
        n = h.synth_fastq(lib.SYNTH_IONTORRENT, first, count, d, cap)
        return n, h.dev_download(d, cap)
    finally:
        h.dev_free(d); h.close()


def check_equal(lib, first, count):
    want = host_fastq(first, count)
    n, buf = device_fastq(lib, first, count)
    assert n == len(want)
    if buf[:n] != want:
        k = next(j for j in range(n) if buf[j] != want[j])
        lo = want.rfind(b"\n@", 0, k) + 1
        pytest.fail(f"first difference at byte {k}: want {want[lo: k + 40]!r}, got {buf[lo: k + 40]!r}")
    assert buf[n:] == b"\xA5" * (len(buf) - n), "bytes written past the end of the last record"


@pytest.mark.parametrize("first,count", [(1, 1500), (999990, 1200), (9999999990, 1200)])
def test_record_sizes(first, count):
    data = host_fastq(first, count)
    lines = data.split(b"\n")
    assert lines[-1] == b"" and len(lines) == 4 * count + 1
    want = [sum(len(x) + 1 for x in lines[4 * k: 4 * k + 4]) for k in range(count)]
    got = synth.iontorrent_record_sizes(first, count)
    assert got.dtype == np.int64 and got.shape == (count,)
    assert got.tolist() == want


def test_emu_one_record(emu):
    check_equal(emu, 1, 1)


def test_emu_group_boundary_and_every_length_class(emu):
    """1500 records: two groups of SYNTH_CHUNK = 1024, the second one partial; reads shorter than a wave, of exactly one
    and two waves, one over, and the longest."""
    lens = {int(m) for m in re.findall(rb" length=(\d+) ", host_fastq(1, 1500))}
    for L in (40, 63, 64, 65, 128, 500):
        assert L in lens, f"no read of length {L} among records 1..1500"
    check_equal(emu, 1, 1500)


def test_emu_id_grows_a_digit(emu):
    assert b"@GXYZ1234.999999 " in host_fastq(999990, 1200) and b"@GXYZ1234.1000000 " in host_fastq(999990, 1200)
    check_equal(emu, 999990, 1200)


def test_emu_ids_beyond_32_bits(emu):
    assert b"@GXYZ1234.10000000000 " in host_fastq(9999999990, 40)
    check_equal(emu, 9999999990, 40)


def test_emu_no_records(emu):
    h = emu.Handle()
    d = h.dev_alloc(64)
    try:
        assert h.synth_fastq(emu.SYNTH_IONTORRENT, 1, 0, d, 64) == 0
    finally:
        h.dev_free(d); h.close()


def test_emu_capacity(emu):
    need = len(host_fastq(1, 1500))
    h = emu.Handle()
    d = h.dev_alloc(need + 64)
    try:
        h.dev_upload(d, b"\xA5" * (need + 64))
        with pytest.raises(emu.DsrcGpuError) as e:
            h.synth_fastq(emu.SYNTH_IONTORRENT, 1, 1500, d, need - 1)
        assert e.value.code == E_CAPACITY
        assert h.dev_download(d, need + 64) == b"\xA5" * (need + 64), "the refused call wrote to the buffer"
        assert h.synth_fastq(emu.SYNTH_IONTORRENT, 1, 1500, d, need) == need          # exactly enough is enough
    finally:
        h.dev_free(d); h.close()


def test_emu_unknown_flavour(emu):
    h = emu.Handle()
    d = h.dev_alloc(1 << 16)
    try:
        with pytest.raises(emu.DsrcGpuError) as e:
            h.synth_fastq(3, 1, 10, d, 1 << 16)
        assert e.value.code == E_ARG
    finally:
        h.dev_free(d); h.close()


def test_emu_generated_records_compress_like_the_host_ones(emu, oracle):
    """End to end: 600 device-generated records through compress_block at -d2 -q1 -l against the oracle on the host generator's."""
    want = synth.iontorrent_fastq(600)
    cfg = Config.from_levels(2, 1, True)
    h = emu.Handle(cfg.dna_order, cfg.quality_order, cfg.lossy, cfg.crc, cfg.quality_offset)
    d = h.dev_alloc(len(want))
    try:
        n = h.synth_fastq(emu.SYNTH_IONTORRENT, 1, 600, d, len(want))
        data = h.dev_download(d, n)
        assert data.endswith(b"\n")
        assert h.compress_block(data[:-1]) == oracle.compress_block(cfg, want[:-1])
    finally:
        h.dev_free(d); h.close()
