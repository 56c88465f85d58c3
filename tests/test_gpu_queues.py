"""Scheduler instances side by side: the range coder runs on a stream (and hardware queue) of its own and the front-end stream is
told on the HOST when the coder has finished (dsrc_gpu.hip: dsrcgpu_create, run_batch, the verifying pass of run_decode).

What would go wrong: k_meta_plan or a read-back enqueued before k_rcs has finished gives wrong sizes or bytes, whatever the batch size; a
verifying pass whose DNA chains are read before they are done gives a wrong verdict or text; streams that are not given back make a later
dsrcgpu_create fail.  Nothing here is timed: blocks are compared with the oracle's, texts with the input."""
import os
import threading

import pytest

from dsrc_amd import synth
from tests._oracle import Config

pytestmark = pytest.mark.gpu

N_SETS = 4          # one per concurrent handle
N_CHUNKS = 8
RECS = 700          # about 256 KiB of Illumina-like records per chunk
CALLS = 3


@pytest.fixture(scope="module")
def gpu():
    os.environ.pop("DSRC_GPU_LIB", None)
    from dsrc_amd import _lib
    _lib._lib = None
    return _lib


@pytest.fixture(scope="module")
def sets():
    """N_SETS x N_CHUNKS chunks of distinct records (no final newline, as the chunk reader cuts them)."""
    return [[synth.illumina_fastq(RECS, first=1 + (s * N_CHUNKS + k) * RECS)[:-1] for k in range(N_CHUNKS)] for s in range(N_SETS)]


@pytest.fixture(scope="module")
def want(sets, oracle):
    """The oracle's block of every chunk at -d3 -q2, computed once."""
    cfg = Config.from_levels(3, 2)
    return [[oracle.compress_block(cfg, c)[0] for c in chunks] for chunks in sets]


@pytest.fixture(scope="module")
def want_crc(sets, oracle):
    cfg = Config.from_levels(3, 2, False, True)
    return [[oracle.compress_block(cfg, c)[0] for c in chunks] for chunks in sets]


class DevChunks:
    """Chunks in device memory, one after the other (a newline between them), and an output buffer."""

    def __init__(self, h, chunks):
        self.h = h
        blob = b"\n".join(chunks) + b"\n"
        self.offs, self.sizes = [], []
        at = 0
        for c in chunks:
            self.offs.append(at); self.sizes.append(len(c)); at += len(c) + 1
        self.d_in = h.dev_alloc(len(blob) + 4096)
        h.dev_upload(self.d_in, blob)
        self.cap = len(blob) + len(chunks) * (1 << 16)
        self.d_out = h.dev_alloc(self.cap)

    def compress(self):
        o_offs, o_sizes, _, _ = self.h.compress_batch_device(self.d_in, self.offs, self.sizes, self.d_out, self.cap)
        return [self.h.dev_download(self.d_out + o, n) for o, n in zip(o_offs, o_sizes)]

    def free(self):
        self.h.dev_free(self.d_in); self.h.dev_free(self.d_out)


def _run_threads(work, n):
    errs = []

    def guarded(i):
        try:
            work(i)
        except BaseException as e:      # noqa: BLE001  (an assertion in a thread must fail the test)
            errs.append((i, e))
    ths = [threading.Thread(target=guarded, args=(i,)) for i in range(n)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    if errs:
        raise AssertionError(f"instance {errs[0][0]}: {errs[0][1]!r}") from errs[0][1]


def _concurrent_compress(gpu, sets, want, **kw):
    cfg = Config.from_levels(3, 2)
    hs = [gpu.Handle(cfg.dna_order, cfg.quality_order, quality_offset=33, **kw) for _ in range(N_SETS)]
    devs = [DevChunks(h, chunks) for h, chunks in zip(hs, sets)]
    got = [[None] * CALLS for _ in range(N_SETS)]
    try:
        def work(i):
            for k in range(CALLS):
                got[i][k] = devs[i].compress()
        _run_threads(work, N_SETS)
    finally:
        for d in devs:
            d.free()
        for h in hs:
            h.close()
    for i in range(N_SETS):
        for k in range(CALLS):
            assert len(got[i][k]) == N_CHUNKS
            for b in range(N_CHUNKS):
                assert got[i][k][b] == want[i][b], f"instance {i}, call {k}, block {b} differs from the oracle's"


def test_concurrent_handles(gpu, sets, want):
    """Four handles, four threads, three calls each: every block is the oracle's."""
    _concurrent_compress(gpu, sets, want)


def test_concurrent_verify_handles(gpu, sets, want_crc):
    """The same with -c handles: the verifying pass runs its DNA chains on the coder's stream.  A refused verification is an error
    of the call."""
    _concurrent_compress(gpu, sets, want_crc, crc=True, verify=True)


def test_decode_overlap(gpu, sets, want):
    """Two decoding handles at once, checksums verified: the text is the input."""
    cfg = Config.from_levels(3, 2)
    hs = [gpu.Handle(cfg.dna_order, cfg.quality_order, quality_offset=33) for _ in range(2)]
    res = [None, None]; bufs = []
    try:
        for i, h in enumerate(hs):
            blob = b"".join(want[i])
            offs, at = [], 0
            for b in want[i]:
                offs.append(at); at += len(b)
            d_blk = h.dev_alloc(len(blob) + 4096); h.dev_upload(d_blk, blob)
            cap = sum(len(c) + 1 for c in sets[i]) + 4096
            d_txt = h.dev_alloc(cap)
            bufs.append((h, d_blk, d_txt, offs, [len(b) for b in want[i]], cap))

        def work(i):
            h, d_blk, d_txt, offs, sizes, cap = bufs[i]
            for _ in range(CALLS):
                t_offs, t_sizes, ok = h.decompress_batch_device(d_blk, offs, sizes, d_txt, cap, verify=True)
                res[i] = (ok, [h.dev_download(d_txt + o, n) for o, n in zip(t_offs, t_sizes)])
        _run_threads(work, 2)
    finally:
        for h, d_blk, d_txt, *_ in bufs:
            h.dev_free(d_blk); h.dev_free(d_txt)
        for h in hs:
            h.close()
    for i in range(2):
        ok, texts = res[i]
        assert all(ok), f"instance {i}: verdicts {ok}"
        assert texts == [c + b"\n" for c in sets[i]], f"instance {i}: decoded text differs from the input"


def test_lanes_inside_one_handle(gpu, sets, want):
    """One handle that cuts its call into sub-batches of two chunks on four lanes (every lane a child with streams of its own):
    the blocks are those of the handle's own lane."""
    cfg = Config.from_levels(3, 2)
    got = {}
    for lanes in ((4, 2), (1, 0)):
        h = gpu.Handle(cfg.dna_order, cfg.quality_order, quality_offset=33)
        h.set_lanes(*lanes)
        d = DevChunks(h, sets[0])
        try:
            got[lanes] = d.compress()
        finally:
            d.free(); h.close()
    assert got[(4, 2)] == got[(1, 0)]
    assert got[(1, 0)] == want[0]


def test_queues_are_given_back(gpu, sets, want):
    """24 handles one after the other, then 8 at once: no call fails (a coder stream that kept its hardware queue after
    dsrcgpu_destroy would exhaust them), and the blocks are right."""
    cfg = Config.from_levels(3, 2)
    small = sets[0][0]
    for _ in range(24):
        h = gpu.Handle(cfg.dna_order, cfg.quality_order, quality_offset=33)
        try:
            assert h.compress_block(small)[0] == want[0][0]
        finally:
            h.close()
    hs = []
    try:
        for _ in range(8):
            hs.append(gpu.Handle(cfg.dna_order, cfg.quality_order, quality_offset=33))
        for h in hs:
            assert h.compress_block(small)[0] == want[0][0]
    finally:
        for h in hs:
            h.close()
