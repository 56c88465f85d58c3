"""Shared by tests/test_emu_columns.py (CPU, emulator build) and tests/test_gpu_columns.py (MI355X): the cases of the columnar
decode and what the ORACLE says they must give.  Blocks come from the oracle's encoder, the expected text from the oracle's
decoder; the expected arrays are derived from that text here, line by line -- never from the library under test.
Every comparison is exact equality."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import random

import numpy as np
import pytest
import torch        # before the first handle: a torch wheel that bundles its HIP runtime must be the one that brings it into the process

from dsrc_amd import synth
from tests._oracle import Config, Oracle
from tests.cases import LEVELS, TINY, fuzz_fastq, fuzz_solid        # noqa: F401  (re-exported to the two test files)

E_ARG, E_CAPACITY = -1, -4          # include/dsrc_gpu.h
LETTERS = b"ACGTNRWSKMDVHBYXU.-"
LUT = np.full(256, 255, np.uint8)
for _i, _c in enumerate(LETTERS):
    LUT[_c] = _i

FILTER_FLAGS = 0b110                # -f1,2: keep title fields 1 and 2

# Shapes per build: each of the two test files passes its own set (`sh`) to the run_* functions below.  The emulator runs the decoder's order-context chains at ~70 us a symbol (a coroutine switch per wave
# exchange), so a 7100-record batch at -d3 -q2 costs 80 s per decode there and milliseconds on the GPU.  What the shapes are for
# scales with the build: the emulator's workgroups have 256 threads, the GPU's 1024, and the tile carry of k_col_sizes needs one
# block with more records than that; everything else (blocks of 1 and 2 records between large ones, odd sizes, five blocks) is
# kept.  "one_pass": the large range-coded cases are decoded once, into arrays sized from the ORACLE's totals, instead of twice
# (Handle.decompress_columns sizes with a first decode); the two-pass path runs in every other case.
# Fuzz seeds were chosen on the CPU with the oracle alone (`python -m tests.columns_cases`): its encoder takes all 12 at every
# level and its decoder reads back everything it wrote.
SHAPES = {
    "gpu": dict(block_records=[3000, 1, 1500, 2, 2600], ion_lossy=2500, fuzz=[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11],
                plus_seed=0, filter_seed=12, one_pass=False),
    "emu": dict(block_records=[258, 1, 30, 2, 257], ion_lossy=300, fuzz=[1, 2, 3, 4, 7, 8, 9, 13, 14, 15, 16, 18],
                plus_seed=23, filter_seed=13, one_pass=True),
}


@functools.lru_cache(maxsize=1)
def oracle():
    return Oracle()


@dataclasses.dataclass
class Expected:
    bases: np.ndarray
    quals: np.ndarray
    titles: np.ndarray
    seq_offsets: np.ndarray
    title_offsets: np.ndarray
    block_records: list
    texts: list
    blocks: list
    crc_ok: list

    @property
    def totals(self):
        return [len(self.seq_offsets) - 1, len(self.bases), len(self.titles)]


def arrays_from_texts(texts, quality_offset):
    """Decoded chunk texts (every line ended by a newline) -> the expected arrays of the batch."""
    seqs, quals, titles, seq_offs, title_offs, block_records = [], [], [], [0], [0], [0]
    for text in texts:
        lines = text.split(b"\n")
        assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
        for r in range((len(lines) - 1) // 4):
            t, s, p, q = lines[4 * r: 4 * r + 4]
            assert t[:1] == b"@" and p[:1] == b"+" and len(s) == len(q)
            seqs.append(s); quals.append(q); titles.append(t)
            seq_offs.append(seq_offs[-1] + len(s)); title_offs.append(title_offs[-1] + len(t))
        block_records.append(len(seq_offs) - 1)
    s = np.frombuffer(b"".join(seqs), np.uint8); q = np.frombuffer(b"".join(quals), np.uint8)
    return (LUT[s], (q.astype(np.int64) - quality_offset).astype(np.uint8), np.frombuffer(b"".join(titles), np.uint8).copy(),
            np.array(seq_offs, np.uint64), np.array(title_offs, np.uint64), block_records)


def expected(cfg: Config, chunks):
    """None when the oracle's encoder refuses the input (rc = -2, the skip rule of tests/test_gpu_decode.py::check); else the
    oracle's blocks, texts and the arrays.  A block the oracle's decoder cannot read back raises: the cases here are chosen
    so that it can."""
    orc = oracle()
    try:
        blocks = [b for b, _, _ in orc.compress_blocks_state(cfg, chunks)]
    except RuntimeError as e:
        assert "rc=-2" in str(e)
        return None
    texts = [orc.decompress_block(cfg, b, 2 * len(c) + 4096) for b, c in zip(blocks, chunks)]
    crc_ok = [orc.verify_block(cfg, b, 2 * len(c) + 4096) if cfg.crc else 1 for b, c in zip(blocks, chunks)]
    return Expected(*arrays_from_texts(texts, cfg.quality_offset), texts, blocks, crc_ok)


def handle(lib, cfg: Config):
    return lib.Handle(cfg.dna_order, cfg.quality_order, cfg.lossy, cfg.crc, cfg.quality_offset,
                      plus_repetition=cfg.plus_repetition, color_space=cfg.color_space, tag_flags=cfg.tag_flags)


def assert_columns(got, exp: Expected, titles=True, what=None):
    assert got.totals == exp.totals, what
    assert got.block_records == exp.block_records, what
    assert got.bases.dtype == np.uint8 and np.array_equal(got.bases, exp.bases), what
    assert np.array_equal(got.quals, exp.quals), what
    assert np.array_equal(got.seq_offsets, exp.seq_offsets), what
    if titles:
        assert np.array_equal(got.titles, exp.titles), what
        assert np.array_equal(got.title_offsets, exp.title_offsets), what
    else:
        assert got.titles is None and got.title_offsets is None


def check(lib, cfg: Config, chunks, what=None, titles=True, one_pass=False):
    """Oracle blocks of `chunks` -> columns of the library == arrays derived from the oracle's text.  Returns the number of
    blocks compared (0: the oracle's encoder refuses the input)."""
    exp = expected(cfg, chunks)
    if exp is None:
        return 0
    h = handle(lib, cfg)
    try:
        if one_pass:
            call = RawCall(lib, h, exp.blocks, *exp.totals, titles=titles, verify=True)
            assert_raw(call, exp, titles)
            assert call.result[2] == exp.crc_ok, what
            return len(exp.blocks)
        # (a chunk with bare '+' lines decoded with plus_repetition is longer than the chunk size its block declares)
        caps = [len(t) for t in exp.texts] if cfg.plus_repetition else None
        got = h.decompress_columns(exp.blocks, titles=titles, text_caps=caps, verify=True)
        assert_columns(got, exp, titles, what)
        assert got.crc_ok == exp.crc_ok, what
    finally:
        h.close()
    return len(exp.blocks)


# ---- the cases ---------------------------------------------------------------------------------------------------------
def wave_boundary_chunk():
    """Read lengths around one and two waves (and 1000: many strides), titles of 2, 63, 64 and 65 bytes."""
    rng = random.Random(64)
    recs = []
    for i, L in enumerate([1, 2, 63, 64, 65, 127, 128, 129, 1000]):
        tl = [2, 63, 64, 65][i % 4]
        title = (b"@" + b"r%d." % i + b"t" * 80)[:tl] if tl > 2 else b"@a"
        seq = bytes(rng.choice(b"ACGTACGTACGTN") for _ in range(L))
        qual = bytes(33 + (rng.randrange(0, 7) if c == ord("N") else rng.randrange(8, 41)) for c in seq)
        recs.append(title + b"\n" + seq + b"\n+\n" + qual)
    return b"\n".join(recs)


@functools.lru_cache(maxsize=None)
def iontorrent_chunk(n=2500):
    return synth.iontorrent_fastq(n)[:-1]


BLOCK_CFG = Config.from_levels(3, 2, False, True)


@functools.lru_cache(maxsize=None)
def _five_blocks(counts):
    chunks, first = [], 1
    for n in counts:
        chunks.append(synth.illumina_fastq(n, first=first)[:-1]); first += n
    exp = expected(BLOCK_CFG, chunks)
    assert exp is not None and exp.block_records == [sum(counts[:k]) for k in range(6)]
    return exp


def five_blocks(sh):
    """Case "block bases": five blocks of very different record counts at -d3 -q2 with CRC; computed once, shared, never changed."""
    return _five_blocks(tuple(sh["block_records"]))


def offset64_chunk():
    rng = random.Random(6464)
    recs = []
    for i in range(300):
        L = 30 + i % 40
        seq = bytes(rng.choice(b"ACGTACGTACGTACGTN") for _ in range(L))
        qual = bytes(64 + (rng.randrange(0, 3) if c == ord("N") else rng.randrange(3, 41)) for c in seq)       # every character >= '@'
        recs.append(b"@o64.%d %d\n" % (i, L) + seq + b"\n+\n" + qual)
    return b"\n".join(recs)


class RawCall:
    """One call of the device entry point on arrays this test owns: every array is uploaded as 0xA5 bytes, the capacities told to
    the library may be smaller than what is allocated.  Gives back the exception (or None), totals and the arrays' bytes."""

    def __init__(self, lib, h, blocks, n_recs, n_bases, n_title, records_cap=None, bases_cap=None, quals_cap=None, titles_cap=None,
                 titles=True, verify=False):
        offs, pos = [], 0
        for b in blocks:
            offs.append(pos); pos += (len(b) + 63) // 64 * 64
        sizes = {"in": max(pos, 8), "bases": n_bases + 8, "quals": n_bases + 8, "titles": n_title + 8, "seq_offs": 8 * (n_recs + 2), "title_offs": 8 * (n_recs + 2)}
        ptr = {k: h.dev_alloc(v) for k, v in sizes.items()}
        try:
            for k, v in sizes.items():
                h.dev_upload(ptr[k], b"\xA5" * v)
            for b, o in zip(blocks, offs):
                h.dev_upload(ptr["in"] + o, b)
            pick = lambda v, d: d if v is None else v
            cols = lib.Columns(ptr["bases"], pick(bases_cap, n_bases), ptr["quals"], pick(quals_cap, n_bases),
                               ptr["titles"] if titles else None, pick(titles_cap, n_title) if titles else 0,
                               ptr["seq_offs"], ptr["title_offs"], pick(records_cap, n_recs))
            self.error = self.result = None
            try:
                self.result = h.decompress_columns_device(ptr["in"], offs, [len(b) for b in blocks], cols, verify=verify)
            except lib.DsrcGpuError as e:
                self.error = e
            self.raw = {k: h.dev_download(ptr[k], sizes[k]) for k in sizes if k != "in"}
        finally:
            for p in ptr.values():
                h.dev_free(p)

    def untouched(self, *names):
        return all(self.raw[k] == b"\xA5" * len(self.raw[k]) for k in (names or self.raw))

    def array(self, name, count, dtype=np.uint8):
        return np.frombuffer(self.raw[name], dtype=dtype)[:count]


def assert_raw(call: RawCall, exp: Expected, titles=True):
    assert call.error is None, call.error
    R, S, T = exp.totals
    assert call.result[0] == exp.block_records and call.result[1] == exp.totals
    assert np.array_equal(call.array("bases", S), exp.bases) and np.array_equal(call.array("quals", S), exp.quals)
    assert np.array_equal(call.array("seq_offs", R + 1, np.uint64), exp.seq_offsets)
    # nothing behind the arrays' ends
    assert call.raw["bases"][S:] == b"\xA5" * 8 and call.raw["quals"][S:] == b"\xA5" * 8 and call.raw["seq_offs"][8 * (R + 1):] == b"\xA5" * 8
    if titles:
        assert np.array_equal(call.array("titles", T), exp.titles)
        assert np.array_equal(call.array("title_offs", R + 1, np.uint64), exp.title_offsets)
        assert call.raw["titles"][T:] == b"\xA5" * 8 and call.raw["title_offs"][8 * (R + 1):] == b"\xA5" * 8
    else:
        assert call.untouched("titles", "title_offs")


# ---- the tests proper: the two files bind them to their library ------------------------------------------------------------
def run_tiny(lib, sh, d, q, lossy, crc):
    assert check(lib, Config.from_levels(d, q, lossy, crc), [TINY]) == 1


def run_wave_boundaries(lib, sh, d, q):
    assert check(lib, Config.from_levels(d, q), [wave_boundary_chunk()]) == 1


def run_scan_tiles(lib, sh, d, q, lossy):
    chunk = iontorrent_chunk(sh["ion_lossy"] if lossy else 2500)
    assert check(lib, Config.from_levels(d, q, lossy), [chunk], one_pass=sh["one_pass"] and lossy) == 1


def run_block_bases(lib, sh):
    exp = five_blocks(sh)
    h = handle(lib, BLOCK_CFG)
    try:
        if sh["one_pass"]:
            call = RawCall(lib, h, exp.blocks, *exp.totals, verify=True)
            assert_raw(call, exp)
            assert call.result[2] == [1] * 5 == exp.crc_ok
            return
        got = h.decompress_columns(exp.blocks, verify=True)
        assert got.block_records == exp.block_records and len(got.block_records) == 6
        assert_columns(got, exp)
        assert got.crc_ok == [1] * 5 == exp.crc_ok
    finally:
        h.close()


def run_empty_and_single(lib, sh):
    exp = five_blocks(sh)
    h = handle(lib, BLOCK_CFG)
    try:
        got = h.decompress_columns([])
        assert got.totals == [0, 0, 0] and got.block_records == [0]
        assert len(got.bases) == 0 and len(got.quals) == 0 and len(got.titles) == 0
        assert list(got.seq_offsets) == [0] and list(got.title_offsets) == [0]
        call = RawCall(lib, h, [], 0, 0, 0)
        assert call.error is None and call.result == ([0], [0, 0, 0])
        assert call.untouched("bases", "quals", "titles") and call.raw["seq_offs"] == bytes(8) + b"\xA5" * 8 == call.raw["title_offs"]
        one = h.decompress_columns(exp.blocks[1:2])                     # the block of one record, alone
        text = exp.texts[1]
        assert_columns(one, Expected(*arrays_from_texts([text], 33), [text], exp.blocks[1:2], [1]))
    finally:
        h.close()


def run_capacity(lib, sh):
    exp = five_blocks(sh)
    R, S, T = exp.totals
    h = handle(lib, BLOCK_CFG)
    try:
        for short in ({"bases_cap": S - 1}, {"quals_cap": S - 1}, {"titles_cap": T - 1}, {"records_cap": R - 1}):
            call = RawCall(lib, h, exp.blocks, R, S, T, **short)
            assert call.error is not None and call.error.code == E_CAPACITY, short
            assert call.error.need == [R, S, T], short
            assert call.untouched(), short
        assert_raw(RawCall(lib, h, exp.blocks, R, S, T, verify=True), exp)      # the same handle, exact capacities
    finally:
        h.close()


def run_titles_off(lib, sh):
    exp = five_blocks(sh)
    R, S, T = exp.totals
    h = handle(lib, BLOCK_CFG)
    try:
        assert_raw(RawCall(lib, h, exp.blocks, R, S, T, titles=False), exp, titles=False)
        text = exp.texts[3]                                              # ... and through the two-pass host path: the block of two records
        assert_columns(h.decompress_columns(exp.blocks[3:4], titles=False),
                       Expected(*arrays_from_texts([text], 33), [text], exp.blocks[3:4], [1]), titles=False)
    finally:
        h.close()


def run_dataset_flags(lib, sh):
    plus, _ = fuzz_fastq(sh["plus_seed"])
    filt, _ = fuzz_fastq(sh["filter_seed"])
    for d, q in ((3, 2), (0, 0)):
        base = Config.from_levels(d, q)
        assert check(lib, dataclasses.replace(base, plus_repetition=True), [plus], ("plus", d, q)) == 1
        assert check(lib, dataclasses.replace(base, tag_flags=FILTER_FLAGS), [filt], ("filter", d, q)) == 1
        assert check(lib, Config.from_levels(d, q, offset=64), [offset64_chunk()], ("offset 64", d, q)) == 1


def run_color_space(lib, sh):
    cfg = dataclasses.replace(Config.from_levels(0, 0), color_space=True)
    blocks = None
    for seed in range(24):
        try:
            blocks = [oracle().compress_block(cfg, fuzz_solid(seed)[0])[0]]
            break
        except RuntimeError:
            continue
    assert blocks
    h = handle(lib, cfg)
    try:
        call = RawCall(lib, h, blocks, 4096, 1 << 20, 1 << 18)
        assert call.error is not None and call.error.code == E_ARG
        assert call.untouched()
        with pytest.raises(lib.DsrcGpuError) as ei:
            h.decompress_columns(blocks)
        assert ei.value.code == E_ARG
    finally:
        h.close()


def run_fuzz(lib, sh, d, q, lossy, crc):
    compared = 0
    for seed in sh["fuzz"]:
        data, desc = fuzz_fastq(seed)
        compared += 1 if check(lib, Config.from_levels(d, q, lossy, crc), [data], (seed, desc, d, q, lossy, crc)) else 0
    assert compared >= 10


def run_text_path_unchanged(lib, sh):
    exp = five_blocks(sh)
    h = handle(lib, BLOCK_CFG)
    try:
        before = h.decompress_batch(exp.blocks)
        if sh["one_pass"]:
            assert_raw(RawCall(lib, h, exp.blocks, *exp.totals), exp)
        else:
            assert_columns(h.decompress_columns(exp.blocks), exp)
        after = h.decompress_batch(exp.blocks)
        assert before == after == exp.texts
    finally:
        h.close()


def run_torch_wrapper(lib, sh, device):
    """dsrc_amd.columns.decode_columns: blocks in a tensor on `device`, tensors out; against the arrays from the oracle's text and
    against the numpy path."""
    from dsrc_amd import columns
    exp = five_blocks(sh)
    offs, pos = [], 0
    for b in exp.blocks:
        offs.append(pos); pos += (len(b) + 63) // 64 * 64
    staged = bytearray(pos)
    for b, o in zip(exp.blocks, offs):
        staged[o: o + len(b)] = b
    d_blocks = torch.frombuffer(staged, dtype=torch.uint8).to(device)
    h = handle(lib, BLOCK_CFG)
    try:
        rc = columns.decode_columns(h, d_blocks, offs, [len(b) for b in exp.blocks], device)
        host = h.decompress_columns(exp.blocks)
        R, S, T = exp.totals
        for t, dt, n in ((rc.bases, torch.uint8, S), (rc.quals, torch.uint8, S), (rc.titles, torch.uint8, T), (rc.seq_offsets, torch.int64, R + 1),
                         (rc.title_offsets, torch.int64, R + 1), (rc.block_records, torch.int64, 6)):
            assert t.dtype == dt and tuple(t.shape) == (n,) and t.device.type == torch.device(device).type
        assert rc.n_records == R
        for name in ("bases", "quals", "titles", "seq_offsets", "title_offsets"):
            mine = getattr(rc, name).cpu().numpy()
            assert np.array_equal(mine.astype(np.uint64) if mine.dtype == np.int64 else mine, getattr(host, name)), name
            assert np.array_equal(mine.astype(np.uint64) if mine.dtype == np.int64 else mine, getattr(exp, name)), name
        assert rc.block_records.tolist() == exp.block_records
        # a middle record, sliced on the device
        i = R // 2
        lines = b"".join(exp.texts).split(b"\n")
        got = rc.bases[int(rc.seq_offsets[i]): int(rc.seq_offsets[i + 1])].cpu().numpy()
        assert np.array_equal(got, LUT[np.frombuffer(lines[4 * i + 1], np.uint8)])
        if sh["one_pass"]:
            return
        no_titles = columns.decode_columns(h, d_blocks, offs, [len(b) for b in exp.blocks], device, titles=False)
        assert no_titles.titles.numel() == 0 and no_titles.title_offsets.numel() == 0
        assert torch.equal(no_titles.bases, rc.bases) and torch.equal(no_titles.seq_offsets, rc.seq_offsets)
    finally:
        h.close()


if __name__ == "__main__":
    # how the seeds above were chosen: the oracle alone, on the CPU
    for seed in sorted({v for sh in SHAPES.values() for v in sh["fuzz"] + [sh["plus_seed"], sh["filter_seed"]]}):
        row = []
        for d, q, lossy, crc in LEVELS:
            try:
                row.append("ok" if expected(Config.from_levels(d, q, lossy, crc), [fuzz_fastq(seed)[0]]) else "--")
            except RuntimeError:
                row.append("DEC")
        print(seed, fuzz_fastq(seed)[1], " ".join(row))
