"""Shared by tests/test_emu_columns_enc.py (CPU, emulator build) and tests/test_gpu_columns_enc.py (MI355X): the cases of the
columnar encode (dsrcgpu_compress_columns_device, dsrcgpu_columns_cut) and what the ORACLE says they must give.

Chunks are FASTQ text; the expected blocks, raw_sizes and comp_sizes are oracle.compress_blocks_state(cfg, chunks); the input
arrays are derived from chunk + b"\\n" with columns_cases.arrays_from_texts -- never from the library under test.  Every comparison
is exact equality.  The one differential case (a read of length 0) compares with dsrcgpu_compress_batch_device of the same build on
the host-assembled text, as the entry point's contract says.

Line ends.  A record array has no carriage return, and the text the library assembles ends its lines with a newline alone, so the
chunks here are the LF form of the fuzz chunks (six of the seeds of columns_cases.SHAPES write CRLF).  The oracle's encoder takes
every one of those seeds in LF form at every entry of LEVELS, and the plus_repetition and -f1,2 chunks below at -d3 -q2 and -d0 -q0
(`python -m tests.columns_enc_cases` prints the table, with the oracle alone): no case is skipped, and the tests assert that the
number of compared cases equals the number listed.

plus_repetition.  With that dataset flag the assembled text repeats the title on the plus line, so the chunk given to the oracle
does as well (with_plus).

Shapes.  The same sets as columns_cases.SHAPES, for the same reason: the emulator runs the order-context coder and the verifying
decode of -d3 -q2 at tens of microseconds a symbol.  Its five blocks are 258 / 1 / 30 / 2 / 257 records (workgroups of 256 threads
there: with four waves a workgroup and gx = 1, a wave of k_col_scatter still strides over 60 and more records of the first and the
last block), the lossy Ion-Torrent case has 300 records.  Everything else is the same on both builds."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch        # noqa: F401  before the first handle (see columns_cases)

from dsrc_amd import synth
from tests import columns_cases as cc
from tests._oracle import Config
from tests.cases import LEVELS, TINY, fuzz_fastq

E_ARG, E_CAPACITY, E_INPUT = -1, -4, -5          # include/dsrc_gpu.h
SHAPES = cc.SHAPES
FILTER_FLAGS = cc.FILTER_FLAGS
BLOCK_CFG = cc.BLOCK_CFG


def lf(chunk: bytes) -> bytes:
    return chunk.replace(b"\r\n", b"\n")


def with_plus(chunk: bytes) -> bytes:
    lines = chunk.split(b"\n")
    for i in range(2, len(lines), 4):
        lines[i] = b"+" + lines[i - 2][1:]
    return b"\n".join(lines)


def records_of(chunk: bytes):
    lines = chunk.split(b"\n")
    assert len(lines) % 4 == 0
    return [b"\n".join(lines[i: i + 4]) for i in range(0, len(lines), 4)]


def chunks_of(records, block_records):
    return [b"\n".join(records[a:b]) for a, b in zip(block_records, block_records[1:])]


@dataclasses.dataclass
class Arrays:
    bases: np.ndarray
    quals: np.ndarray
    titles: np.ndarray
    seq_offsets: np.ndarray
    title_offsets: np.ndarray
    block_records: list

    @property
    def n_records(self):
        return len(self.seq_offsets) - 1


def arrays_of(chunks, quality_offset=33) -> Arrays:
    return Arrays(*cc.arrays_from_texts([c + b"\n" for c in chunks], quality_offset))


def oracle_blocks(cfg: Config, chunks, fields_cap=0):
    """[(block, raw, comp)] of one BlockCompressor fed in order, or None where the oracle's encoder refuses (rc = -2)."""
    try:
        return cc.oracle().compress_blocks_state(cfg, chunks, fields_cap)
    except RuntimeError as e:
        assert "rc=-2" in str(e)
        return None


def handle(lib, cfg: Config, verify=False):
    return lib.Handle(cfg.dna_order, cfg.quality_order, cfg.lossy, cfg.crc, cfg.quality_offset, plus_repetition=cfg.plus_repetition,
                      color_space=cfg.color_space, tag_flags=cfg.tag_flags, verify=verify)


class Staged:
    """Arrays in device memory this test owns, `pad` bytes / entries of slack in front of bases, quals and titles (the offsets are
    shifted by it: they need not start at 0), and an output buffer filled with 0xA5."""

    def __init__(self, lib, h, a: Arrays, pad=0, out_cap=None):
        self.lib, self.h, self.a, self.pad = lib, h, a, pad
        self.host = {"bases": bytes(pad) + a.bases.tobytes(), "quals": bytes(pad) + a.quals.tobytes(),
                     "titles": b"@" * pad + a.titles.tobytes(),
                     "seq_offs": (a.seq_offsets + np.uint64(pad)).astype(np.uint64).tobytes(),
                     "title_offs": (a.title_offsets + np.uint64(pad)).astype(np.uint64).tobytes()}
        self.out_cap = out_cap if out_cap is not None else 2 * len(a.bases) + 2 * len(a.titles) + 6 * a.n_records + (len(a.block_records) + 2) * (1 << 16)
        self.ptr = {}
        try:
            for k, v in self.host.items():
                self.ptr[k] = h.dev_alloc(len(v) + 8)
                h.dev_upload(self.ptr[k], v + b"\xA5" * 8)
            self.ptr["out"] = h.dev_alloc(self.out_cap)
            h.dev_upload(self.ptr["out"], b"\xA5" * self.out_cap)
        except Exception:
            self.free()
            raise

    def free(self):
        for p in self.ptr.values():
            self.h.dev_free(p)
        self.ptr = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def poke(self, name, index, value, dtype=np.uint8):
        """Overwrite one element of a staged array (index in elements of dtype, counted from the start of the allocation)."""
        self.h.dev_upload(self.ptr[name] + index * np.dtype(dtype).itemsize, np.array([value], dtype).tobytes())

    def restore(self):
        for k, v in self.host.items():
            self.h.dev_upload(self.ptr[k], v)

    def cols_in(self, first=0, n_records=None):
        a = self.a
        n = a.n_records - first if n_records is None else n_records
        return self.lib.ColumnsIn(self.ptr["bases"], len(self.host["bases"]), self.ptr["quals"], self.ptr["titles"], len(self.host["titles"]),
                                  self.ptr["seq_offs"] + 8 * first, self.ptr["title_offs"] + 8 * first, n)

    def compress(self, block_records=None, first=0, n_records=None):
        """-> [(block, raw, comp)] like Oracle.compress_blocks_state."""
        br = self.a.block_records if block_records is None else block_records
        offs, sizes, raw, comp = self.h.compress_columns_device(self.cols_in(first, n_records), br, self.ptr["out"], self.out_cap)
        out = self.h.dev_download(self.ptr["out"], self.out_cap)
        return [(out[o: o + s], raw[4 * i: 4 * i + 4], comp[4 * i: 4 * i + 4]) for i, (o, s) in enumerate(zip(offs, sizes))]

    def out_untouched(self):
        return self.h.dev_download(self.ptr["out"], self.out_cap) == b"\xA5" * self.out_cap


def check(lib, cfg: Config, chunks, what=None, verify=False, pad=0):
    """Arrays of `chunks` through the library == the oracle's blocks, sizes and block-to-block state.  Returns the number of blocks
    compared (0: the oracle's encoder refuses the input)."""
    want = oracle_blocks(cfg, chunks)
    if want is None:
        return 0
    h = handle(lib, cfg, verify)
    try:
        with Staged(lib, h, arrays_of(chunks, cfg.quality_offset), pad) as st:
            got = st.compress()
        assert len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            assert g[0] == w[0], (what, "block", i)
            assert g[1] == w[1] and g[2] == w[2], (what, "sizes", i)
        assert h.get_fields_capacity() == lib.fields_capacity_fold(chunks, cfg.tag_flags), what
    finally:
        h.close()
    return len(want)


# ---- the cases -------------------------------------------------------------------------------------------------------------
def run_tiny(lib, sh, d, q, lossy, crc):
    assert check(lib, Config.from_levels(d, q, lossy, crc), [TINY]) == 1


def run_wave_boundaries(lib, sh, d, q):
    assert check(lib, Config.from_levels(d, q), [cc.wave_boundary_chunk()], pad=3) == 1


def five_chunks(sh):
    chunks, first = [], 1
    for n in sh["block_records"]:
        chunks.append(synth.illumina_fastq(n, first=first)[:-1]); first += n
    return chunks


def run_block_bases(lib, sh):
    """3000 / 1 / 1500 / 2 / 2600 records at -d3 -q2 with CRC and verify_after_compress: block bases, one-record blocks between large ones."""
    assert check(lib, BLOCK_CFG, five_chunks(sh), verify=True) == 5


def run_iontorrent_lossy(lib, sh):
    assert check(lib, Config.from_levels(2, 1, True), [cc.iontorrent_chunk(sh["ion_lossy"])]) == 1


def run_dataset_flags(lib, sh):
    plus = with_plus(lf(fuzz_fastq(sh["plus_seed"])[0]))
    filt = lf(fuzz_fastq(sh["filter_seed"])[0])
    compared = 0
    for d, q in ((3, 2), (0, 0)):
        base = Config.from_levels(d, q)
        compared += check(lib, dataclasses.replace(base, plus_repetition=True), [plus], ("plus", d, q))
        compared += check(lib, dataclasses.replace(base, tag_flags=FILTER_FLAGS), [filt], ("filter", d, q))
        compared += check(lib, Config.from_levels(d, q, offset=64), [cc.offset64_chunk()], ("offset 64", d, q))
    assert compared == 6


def run_fuzz(lib, sh, d, q, lossy, crc):
    compared = 0
    for seed in sh["fuzz"]:
        data, desc = fuzz_fastq(seed)
        compared += check(lib, Config.from_levels(d, q, lossy, crc), [lf(data)], (seed, desc, d, q, lossy, crc))
    assert compared == len(sh["fuzz"])


def run_nonzero_start(lib, sh):
    """d_seq_offs + k and d_title_offs + k of a larger batch, n_records reduced: the blocks of those records alone."""
    recs = records_of(cc.wave_boundary_chunk()) + records_of(TINY)
    a = arrays_of([b"\n".join(recs)])
    compared = 0
    for d, q in ((0, 0), (3, 2)):
        cfg = Config.from_levels(d, q)
        for first, br in ((9, [0, 4]), (2, [0, 2, 5]), (12, [0, 1])):
            chunks = chunks_of(recs[first:], br)
            want = oracle_blocks(cfg, chunks)
            assert want is not None
            h = handle(lib, cfg)
            try:
                with Staged(lib, h, a, pad=5) as st:
                    got = st.compress(br, first=first, n_records=br[-1])
                assert got == want, (d, q, first)
                assert h.get_fields_capacity() == lib.fields_capacity_fold(chunks)
                compared += 1
            finally:
                h.close()
    assert compared == 6


def run_two_calls(lib, sh):
    """Two calls on one handle: the capacity of TagStats::fields is carried as by one BlockCompressor fed in order."""
    seeds = sh["fuzz"][:4]
    first = [lf(fuzz_fastq(s)[0]) for s in seeds[:2]]
    second = [lf(fuzz_fastq(s)[0]) for s in seeds[2:]] + [TINY]
    for d, q in ((0, 0), (3, 2)):
        cfg = Config.from_levels(d, q)
        want = oracle_blocks(cfg, first + second)
        assert want is not None
        h = handle(lib, cfg)
        try:
            with Staged(lib, h, arrays_of(first)) as st:
                assert st.compress() == want[:2]
            assert h.get_fields_capacity() == lib.fields_capacity_fold(first)
            with Staged(lib, h, arrays_of(second)) as st:
                assert st.compress() == want[2:]
            assert h.get_fields_capacity() == lib.fields_capacity_fold(first + second) == cc.oracle().last_fields_cap
        finally:
            h.close()


def run_empty_single_color(lib, sh):
    cfg = Config.from_levels(3, 2)
    h = handle(lib, cfg)
    try:
        empty = Arrays(np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(1, np.uint64), [0])
        with Staged(lib, h, empty, out_cap=64) as st:
            assert st.compress() == [] and st.out_untouched()
        assert h.compress_columns(lib.HostColumns(empty.bases, empty.quals, empty.titles, empty.seq_offsets, empty.title_offsets, [0], None, None)) == []
        one = records_of(TINY)[1]
        want = oracle_blocks(cfg, [one])
        with Staged(lib, h, arrays_of([one])) as st:
            assert st.compress() == want
        # ... and the host convenience, cutting by itself
        a = arrays_of([one])
        assert h.compress_columns(lib.HostColumns(a.bases, a.quals, a.titles, a.seq_offsets, a.title_offsets, None, None, None)) == [want[0][0]]
    finally:
        h.close()
    hc = handle(lib, dataclasses.replace(Config.from_levels(0, 0), color_space=True))
    try:
        with Staged(lib, hc, arrays_of([TINY])) as st:
            with pytest.raises(lib.DsrcGpuError) as ei:
                st.compress()
            assert ei.value.code == E_ARG and st.out_untouched()
            with pytest.raises(lib.DsrcGpuError) as ei:
                hc.columns_cut(st.cols_in(), 1 << 20)
            assert ei.value.code == E_ARG
    finally:
        hc.close()


def run_arg_errors(lib, sh):
    cfg = Config.from_levels(0, 0)
    recs = records_of(cc.wave_boundary_chunk())
    good = [0, 3, 6, 9]
    want = oracle_blocks(cfg, chunks_of(recs, good))
    h = handle(lib, cfg)
    try:
        with Staged(lib, h, arrays_of([b"\n".join(recs)])) as st:
            for br in ([0, 3, 3, 9], [0, 5, 3, 9], [0, 3, 6, 8], [0, 3, 6, 10], [1, 3, 6, 9]):
                with pytest.raises(lib.DsrcGpuError) as ei:
                    st.compress(br)
                assert ei.value.code == E_ARG and st.out_untouched(), br
            h.set_record_layout([100, 200, 300])                    # the archive API's layout has no meaning here
            with pytest.raises(lib.DsrcGpuError) as ei:
                st.compress(good)
            assert ei.value.code == E_ARG and st.out_untouched()
            assert st.compress(good) == want                        # (the layout was one-shot: gone with the refused call)
            with pytest.raises(lib.DsrcGpuError) as ei:
                h.columns_cut(st.cols_in(), 0)
            assert ei.value.code == E_ARG
    finally:
        h.close()


# what to plant in record r of a batch staged with pad >= 1 (so that offsets of record 0 can be lowered), and a word of the reason
def _plants(a: Arrays, pad: int):
    S = lambda r: int(a.seq_offsets[r]) + pad
    T = lambda r: int(a.title_offsets[r]) + pad
    n_b, n_t = len(a.bases) + pad, len(a.titles) + pad
    return [
        ("seq order", lambda st, r: st.poke("seq_offs", r + 1, S(r) - 1, np.uint64), "d_seq_offs is not non-decreasing"),
        ("seq end", lambda st, r: st.poke("seq_offs", r + 1, n_b + 5, np.uint64), "above bases_len"),
        ("title order", lambda st, r: st.poke("title_offs", r + 1, T(r) - 1, np.uint64), "d_title_offs is not non-decreasing"),
        ("title end", lambda st, r: st.poke("title_offs", r + 1, n_t + 5, np.uint64), "above titles_len"),
        ("base 19", lambda st, r: st.poke("bases", S(r + 1) - 1, 19), "base code"),
        ("base 255", lambda st, r: st.poke("bases", S(r), 255), "base code"),
        ("quality", lambda st, r: st.poke("quals", S(r + 1) - 1, 127 - 33), "quality"),
        ("empty title", lambda st, r: st.poke("title_offs", r + 1, T(r), np.uint64), "empty title"),
        ("no @", lambda st, r: st.poke("titles", T(r), ord("X")), "'@'"),
        ("newline", lambda st, r: st.poke("titles", T(r + 1) - 1, 10), "newline"),
    ]


def run_input_errors(lib, sh):
    """Each refusal of the check pass planted in the first, a middle and the last record of a 3-block batch: code, record index,
    output intact, and the same handle then compresses the clean arrays."""
    cfg = Config.from_levels(0, 0)
    recs = records_of(cc.wave_boundary_chunk())          # 9 records, reads of 1 .. 1000 bases, titles of 2 .. 65 bytes
    br = [0, 3, 6, 9]
    want = oracle_blocks(cfg, chunks_of(recs, br))
    a = arrays_of([b"\n".join(recs)])
    h = handle(lib, cfg)
    checked = 0
    try:
        with Staged(lib, h, a, pad=4) as st:
            for name, plant, word in _plants(a, 4):
                for r in (0, 4, 8):
                    plant(st, r)
                    with pytest.raises(lib.DsrcGpuError) as ei:
                        st.compress(br)
                    assert ei.value.code == E_INPUT, (name, r, str(ei.value))
                    assert "record %d:" % r in str(ei.value) and word in str(ei.value), (name, r, str(ei.value))
                    assert st.out_untouched(), (name, r)
                    if name in ("seq order", "seq end", "title order", "title end"):      # what dsrcgpu_columns_cut refuses as well
                        with pytest.raises(lib.DsrcGpuError) as ei:
                            h.columns_cut(st.cols_in(), 1 << 20)
                        assert ei.value.code == E_INPUT and "record %d:" % r in str(ei.value), (name, r, str(ei.value))
                    st.restore()
                    checked += 1
                assert st.compress(br) == want, name
                st.restore(); st.h.dev_upload(st.ptr["out"], b"\xA5" * st.out_cap)
    finally:
        h.close()
    assert checked == 30


def text_call(lib, cfg, chunks):
    """dsrcgpu_compress_batch_device on host-assembled text -> (code, [(block, raw, comp)])."""
    h = handle(lib, cfg)
    offs, pos = [], 0
    for c in chunks:
        offs.append(pos); pos += (len(c) + 255) // 256 * 256 + 256
    cap = pos + len(chunks) * (1 << 16)
    d_in, d_out = h.dev_alloc(pos), h.dev_alloc(cap)
    try:
        for c, o in zip(chunks, offs):
            h.dev_upload(d_in + o, c)
        try:
            o_offs, o_sizes, raw, comp = h.compress_batch_device(d_in, offs, [len(c) for c in chunks], d_out, cap)
        except lib.DsrcGpuError as e:
            return e.code, None
        out = h.dev_download(d_out, cap)
        return 0, [(out[o: o + s], raw[4 * i: 4 * i + 4], comp[4 * i: 4 * i + 4]) for i, (o, s) in enumerate(zip(o_offs, o_sizes))]
    finally:
        h.dev_free(d_in); h.dev_free(d_out); h.close()


def run_zero_length_read(lib, sh):
    """A read of length 0 goes through as empty lines: return code and blocks are those of the text call on the same build."""
    recs = records_of(TINY)
    title = recs[1].split(b"\n")[0]
    for where in (0, 1, 3):
        mine = list(recs); mine[where] = title + b"\n\n+\n"
        chunks = [b"\n".join(mine[:2]), b"\n".join(mine[2:])]
        a = arrays_of(chunks)
        assert int(a.seq_offsets[where]) == int(a.seq_offsets[where + 1])
        for d, q in ((0, 0), (3, 2)):
            cfg = Config.from_levels(d, q)
            code, want = text_call(lib, cfg, chunks)
            h = handle(lib, cfg)
            try:
                with Staged(lib, h, a) as st:
                    if code:
                        with pytest.raises(lib.DsrcGpuError) as ei:
                            st.compress()
                        assert ei.value.code == code, (where, d, q)
                    else:
                        assert st.compress() == want, (where, d, q)
            finally:
                h.close()


def greedy_cut(a: Arrays, chunk_bytes, plus_rep):
    """The contract of dsrcgpu_columns_cut in plain Python over the same offsets."""
    S, T = [int(v) for v in a.seq_offsets], [int(v) for v in a.title_offsets]
    size = lambda r: (T[r + 1] - T[r]) * (2 if plus_rep else 1) + 2 * (S[r + 1] - S[r]) + (4 if plus_rep else 5)      # with its newline
    cuts, r, R = [0], 0, a.n_records
    while r < R:
        text = size(r) - 1; r += 1
        while r < R and text + size(r) <= chunk_bytes:
            text += size(r); r += 1
        cuts.append(r)
    return cuts


def run_columns_cut(lib, sh):
    recs = records_of(cc.wave_boundary_chunk()) + records_of(cc.iontorrent_chunk(300)) + records_of(TINY)
    for plus_rep in (False, True):
        cfg = dataclasses.replace(Config.from_levels(0, 0), plus_repetition=plus_rep)
        text = b"\n".join(recs)
        if plus_rep:
            text = with_plus(text)
        a = arrays_of([text])
        texts = records_of(text)
        h = handle(lib, cfg)
        try:
            with Staged(lib, h, a, pad=2) as st:
                cin = st.cols_in()
                # below one record's text: one record per block
                assert h.columns_cut(cin, 1) == list(range(len(recs) + 1)) == greedy_cut(a, 1, plus_rep)
                # exactly the text of the first 40 records, and one byte less
                exact = len(b"\n".join(texts[:40]))
                assert h.columns_cut(cin, exact)[:2] == [0, 40] and h.columns_cut(cin, exact - 1)[:2] == [0, 39]
                for chunk_bytes in (exact, exact - 1, 700, 2100, 5000, 1 << 20, 1 << 40):
                    want = greedy_cut(a, chunk_bytes, plus_rep)
                    assert h.columns_cut(cin, chunk_bytes) == want, (plus_rep, chunk_bytes)
                    # (the blocks really keep to it, and the text sizes are the real ones)
                    for i, c in enumerate(chunks_of(texts, want)):
                        assert len(c) <= chunk_bytes or want[i + 1] - want[i] == 1
                # cap one short: the need comes back, nothing is written
                want = greedy_cut(a, 2100, plus_rep)
                n = len(want) - 1
                buf = (C.c_uint64 * (n + 1))(*([0xA5A5A5A5A5A5A5A5] * (n + 1))); got_n = C.c_uint32()
                rc = h.L.dsrcgpu_columns_cut(h.h, C.byref(cin), C.c_uint64(2100), buf, C.c_uint32(n), C.byref(got_n))
                assert rc == E_CAPACITY and got_n.value == n and list(buf) == [0xA5A5A5A5A5A5A5A5] * (n + 1)
                with pytest.raises(lib.DsrcGpuError) as ei:
                    h.columns_cut(cin, 2100, cap=n)
                assert ei.value.code == E_CAPACITY and ei.value.need == n
                assert h.columns_cut(cin, 2100, cap=n + 1) == want
                # a sub-range: offsets that do not start at 0
                sub = Arrays(a.bases, a.quals, a.titles, a.seq_offsets[7:], a.title_offsets[7:], [])
                assert h.columns_cut(st.cols_in(first=7), 2100) == greedy_cut(sub, 2100, plus_rep)
                # no records
                assert h.columns_cut(st.cols_in(first=3, n_records=0), 2100) == [0]
        finally:
            h.close()


def run_closed_loop(lib, sh, device):
    """Oracle blocks -> decode_columns -> encode_columns with the returned block_records == the oracle's blocks of the oracle's
    decoded text; one lossless case with CRC (five blocks) and one lossy one.  Also the torch wrapper's own cut."""
    from dsrc_amd import columns
    cases = [(BLOCK_CFG, None), (Config.from_levels(2, 1, True), [TINY, cc.iontorrent_chunk(300)])]
    for cfg, chunks in cases:
        exp = cc.five_blocks(sh) if chunks is None else cc.expected(cfg, chunks)      # (the five blocks: computed once, shared)
        assert exp is not None
        decoded = [t[:-1] for t in exp.texts]
        want = oracle_blocks(cfg, decoded)
        assert want is not None
        offs, pos = [], 0
        for b in exp.blocks:
            offs.append(pos); pos += (len(b) + 63) // 64 * 64
        staged = bytearray(pos)
        for b, o in zip(exp.blocks, offs):
            staged[o: o + len(b)] = b
        d_blocks = torch.frombuffer(staged, dtype=torch.uint8).to(device)
        h = handle(lib, cfg)
        try:
            rc = columns.decode_columns(h, d_blocks, offs, [len(b) for b in exp.blocks], device)
            h.set_fields_capacity(0)
            blocks, o_offs, o_sizes, br = columns.encode_columns(h, rc, block_records=rc.block_records)
            assert br == exp.block_records
            assert blocks.dtype == torch.uint8 and blocks.device.type == torch.device(device).type
            host = blocks.cpu().numpy().tobytes()
            assert [host[o: o + s] for o, s in zip(o_offs, o_sizes)] == [w[0] for w in want], cfg
            assert h.get_fields_capacity() == lib.fields_capacity_fold(decoded, cfg.tag_flags)
            if chunks is None:
                continue
            # the wrapper cutting by itself (the small case is enough for that): the whole batch fits one block of 8 MiB of text
            h.set_fields_capacity(0)
            blocks, o_offs, o_sizes, br = columns.encode_columns(h, rc)
            assert br == [0, rc.n_records]
            one = oracle_blocks(cfg, [b"\n".join(decoded)])
            host = blocks.cpu().numpy().tobytes()
            assert one is not None and [host[o: o + s] for o, s in zip(o_offs, o_sizes)] == [one[0][0]]
        finally:
            h.close()


if __name__ == "__main__":
    # what the docstring claims, with the oracle alone, on the CPU
    for seed in sorted({v for sh in SHAPES.values() for v in sh["fuzz"]}):
        print(seed, fuzz_fastq(seed)[1], " ".join("ok" if oracle_blocks(Config.from_levels(*lv), [lf(fuzz_fastq(seed)[0])]) else "--" for lv in LEVELS))
    for sh in SHAPES.values():
        for d, q in ((3, 2), (0, 0)):
            base = Config.from_levels(d, q)
            print("plus", sh["plus_seed"], d, q, bool(oracle_blocks(dataclasses.replace(base, plus_repetition=True), [with_plus(lf(fuzz_fastq(sh["plus_seed"])[0]))])))
            print("filter", sh["filter_seed"], d, q, bool(oracle_blocks(dataclasses.replace(base, tag_flags=FILTER_FLAGS), [lf(fuzz_fastq(sh["filter_seed"])[0])])))
