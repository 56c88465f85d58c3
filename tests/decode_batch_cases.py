"""Decode batches under a table budget, shared by the emulator tests (tests/test_emu_decode_rounds.py) and the GPU tests
(tests/test_gpu_decode_rounds.py): the rounds of run_decode (dsrc_amd/csrc/dsrc_gpu.hip), batches that mix quality alphabets and
DNA schemes, several passes on one handle, the other entry points and a refusal in the middle of a batch.

Blocks come from the ORACLE's encoder (compress_blocks_state), the expected text from its decoder, the verdicts from its
verify_block; every comparison is exact equality.  What the library did with its table region is read from the line it prints
with DSRC_GPU_DEBUG set and compared with a MODEL written here from the documented rule, fed with the region that line reports
(the allocation carries 1/16 + 4096 bytes of slack):

  * one table per block and stream.  4-symbol DNA: 2^(2 order) rows of 4 counters of 16 bits (-d1/-d2/-d3: 512 B, 32 KiB, 2 MiB);
    8-symbol DNA: 2^(3 min(order, 7)) rows of 8 (8 KiB, 4 MiB, 32 MiB); lossy quality: 8 symbols, order 3 q, rescale 8 (64 KiB,
    32 MiB); lossless quality: n = 16 << (scheme & 3), order (3, 2, 1, 1) at -q1 and (4, 3, 2, 1) at -q2, rescale 8 below scheme 4
    and n from it on; 2^(log2 n * order) * rescale * n / 2 words of 32 bits (q_table_words);
  * the scheme bytes by the reference's rules from the oracle's block statistics: the smallest alphabet that holds the block's
    quality values, + 4 at -q2 for reads of one length with raw / rle > 1.175; DNA 255 without any base in the stream, 0 with
    at most four symbols, else 1;
  * packing: tables aligned to 128 bytes, taken in block order, a round closed when the next table does not fit, at least one
    table per round; the 4-symbol DNA blocks first, then the 8-symbol ones, both planned in the region as the 8-symbol step left it.
"""
from __future__ import annotations

import random
import re

import pytest

from dsrc_amd import synth
from tests._oracle import Config
from tests.cases import TINY, alphabet_fastq

KIB, MIB = 1 << 10, 1 << 20
ALIGN = 128

# reads per block: the wave decoder costs the emulator 64 context switches per symbol
SHAPES = {
    "emu": dict(n_rec=36, illumina=60, hot="few"),
    "gpu": dict(n_rec=400, illumina=400, hot="hot"),
}


# ---- the model ---------------------------------------------------------------------------------------------------------------

def al(nbytes: int) -> int:
    return (nbytes + ALIGN - 1) // ALIGN * ALIGN


def slack(nbytes: int) -> int:
    """What ensure_dec_tables allocates for a region of nbytes."""
    return nbytes + nbytes // 16 + 4096


def q_scheme(cfg: Config, q_count: int, min_len: int, max_len: int, raw_len: int, rle_len: int) -> int:
    """QualityOrderModelerProxyLossless::SelectSchemeId."""
    sch = next(i for i in range(8) if (16 << i) >= q_count)
    if cfg.quality_order == 2 and min_len == max_len and rle_len and raw_len / rle_len > 1.175:
        sch += 4
    return sch


def q_table(cfg: Config, scheme: int):
    """(alphabet, table bytes) of a block's quality model; (0, 0) at -q0."""
    if cfg.quality_order == 0:
        return 0, 0
    if cfg.lossy:
        n, order, resc = 8, cfg.quality_order, 8
    else:
        sc = scheme & 3
        n = 16 << sc
        order = (3, 2, 1, 1)[sc] if cfg.quality_order == 1 else 4 - sc
        resc = 8 if scheme < 4 else n
    return n, 4 * ((1 << ((n.bit_length() - 1) * order)) * resc * n // 2)


def d_table(cfg: Config, scheme: int) -> int:
    """Table bytes of a block's DNA model (scheme 0: 4 symbols, 1: 8 symbols at order <= 7)."""
    if cfg.dna_order == 0 or scheme == 255:
        return 0
    return 4 * ((1 << (3 * min(cfg.dna_order, 7))) * 4 if scheme else (1 << (2 * cfg.dna_order)) * 2)


def describe(oracle, cfg: Config, chunks):
    """Per block, from the oracle's statistics: dict(n, q_bytes, d_scheme, d_bytes)."""
    out = []
    for c in chunks:
        d, q, _, _, _ = oracle.block_stats(cfg, c)
        sch = 0 if cfg.lossy or cfg.quality_order == 0 else q_scheme(cfg, q[0], q[1], q[2], q[3], q[5])
        n, qb = q_table(cfg, sch)
        ds = 255 if d[0] == 0 else (0 if d[0] <= 4 else 1)
        out.append(dict(n=n, q_bytes=qb, q_scheme=sch, d_scheme=ds, d_bytes=d_table(cfg, ds)))
    return out


def pack(sizes, region_bytes: int):
    """Rounds as lists of indices into `sizes`."""
    region = region_bytes // 4 * 4
    rounds, cur, top = [], [], 0
    for i, s in enumerate(sizes):
        w = al(s)
        if top + w > region and cur:
            rounds.append(cur)
            cur, top = [], 0
        cur.append(i)
        top += w
    if cur:
        rounds.append(cur)
    return rounds


def model(cfg: Config, info, region: int, final: int, par: bool = False):
    """What the debug line must say for blocks `info` with the quality rounds planned in `region` bytes and the DNA rounds in `final`."""
    m = dict(qrounds=0, r4=0, b4=0, r8=0, b8=0, plain=0)
    for k in (8, 16, 32, 64, 128):
        m["n%d" % k] = sum(1 for b in info if b["n"] == k)
    m["q_rounds_list"] = pack([b["q_bytes"] for b in info], region) if cfg.quality_order else []
    m["qrounds"] = len(m["q_rounds_list"])
    if cfg.dna_order:
        t4 = [b["d_bytes"] for b in info if b["d_scheme"] == 0]
        t8 = [b["d_bytes"] for b in info if b["d_scheme"] == 1]
        m["b4"], m["b8"] = len(t4), len(t8)
        m["plain"] = sum(1 for b in info if b["d_scheme"] == 255)
        if par:
            m["r4"], m["r8"] = int(bool(t4)), int(bool(t8))
        else:
            m["r4"], m["r8"] = len(pack(t4, final)), len(pack(t8, final))
    return m


LINE = re.compile(r"decode tables \((\d+) blocks\): budget (\d+), region (\d+), final (\d+) bytes; quality rounds (\d+), "
                  r"tables n8 (\d+) n16 (\d+) n32 (\d+) n64 (\d+) n128 (\d+); dna4 rounds (\d+) blocks (\d+); dna8 rounds (\d+) blocks (\d+); "
                  r"plain (\d+); par (\d)")
FIELDS = ("blocks", "budget", "region", "final", "qrounds", "n8", "n16", "n32", "n64", "n128", "r4", "b4", "r8", "b8", "plain", "par")


def debug_lines(err: str):
    return [dict(zip(FIELDS, map(int, m.groups()))) for m in LINE.finditer(err)]


def check_line(cfg: Config, info, line, budget=None, fresh=True):
    """The line against the model; on a handle whose region this pass allocated (`fresh`), the region against the budget."""
    assert line["blocks"] == len(info)
    m = model(cfg, info, line["region"], line["final"], par=bool(line["par"]))
    got = {k: line[k] for k in m if k != "q_rounds_list"}
    want = {k: v for k, v in m.items() if k != "q_rounds_list"}
    assert got == want, (line, m)
    if budget is not None:
        assert line["budget"] == budget
        if fresh:
            first = max([al(b["q_bytes"]) for b in info] + [al(d_table(cfg, 0))])
            every = max([first] + [al(b["d_bytes"]) for b in info])
            assert line["region"] <= slack(max(budget // 4 * 4, first)), line
            assert line["final"] <= slack(max(budget // 4 * 4, every)), line
    return m


# ---- inputs ------------------------------------------------------------------------------------------------------------------

def hot_block(kind: str) -> bytes:
    """A block hot enough to rescale: the `few` and `hot` recipes of tests/test_emu_decode.py."""
    rng = random.Random(11)
    if kind == "few":
        return b"\n".join(b"@h.%d\nACGT\n+\n%s" % (i, bytes(rng.choice(b"IIIIIIIH") for _ in range(4))) for i in range(2200))
    return b"\n".join([b"@r\nA\n+\n%c" % (73 if rng.random() < 0.97 else 60) for _ in range(42000)] + [b"@h\n%s\n+\n%s" % (b"A" * 100, b"I" * 100) for _ in range(40)])


def plain_block(n_rec: int = 20) -> bytes:
    """No base reaches the DNA stream (N below quality 7 travels in the quality stream; lossy: every N does): d_scheme 255."""
    return b"\n".join(b"@n.%d\n%s\n+\n%s" % (i, b"N" * (20 + i % 3), bytes(33 + (i + k) % 5 for k in range(20 + i % 3))) for i in range(n_rec))


def illumina(S, k: int = 0) -> bytes:
    return synth.illumina_fastq(S["illumina"], first=1 + 1000 * k)[:-1]


def mixed_alphabet_chunks(S, lossy: bool):
    if lossy:          # the lossy bin table has 64 entries; every block takes the 8-symbol model
        return [alphabet_fastq(n, n_rec=S["n_rec"], q_max=42) for n in (3, 12, 20)] + [illumina(S), TINY, hot_block(S["hot"])]
    return [alphabet_fastq(n, n_rec=S["n_rec"]) for n in (3, 12, 20, 40, 90)] + [illumina(S), TINY, hot_block(S["hot"])]


# ---- one pass, checked ---------------------------------------------------------------------------------------------------------

class Batch:
    """Blocks, expected texts and verdicts of `chunks` from the oracle, and the model's description of every block."""

    def __init__(self, oracle, cfg: Config, chunks):
        self.cfg, self.chunks = cfg, list(chunks)
        self.blocks = [b for b, _, _ in oracle.compress_blocks_state(cfg, self.chunks)]
        self.want = [oracle.decompress_block(cfg, b, 2 * len(c) + 4096) for b, c in zip(self.blocks, self.chunks)]
        self.ok = [oracle.verify_block(cfg, b, 2 * len(c) + 4096) if cfg.crc else 1 for b, c in zip(self.blocks, self.chunks)]
        self.info = describe(oracle, cfg, self.chunks)

    def reordered(self, order):
        other = object.__new__(Batch)
        other.cfg = self.cfg
        for name in ("chunks", "blocks", "want", "ok", "info"):
            setattr(other, name, [getattr(self, name)[i] for i in order])
        return other


def handle(lib, cfg: Config, verify=False):
    return lib.Handle(cfg.dna_order, cfg.quality_order, cfg.lossy, cfg.crc, cfg.quality_offset, verify=verify)


def one_pass(h, batch: Batch, capfd, budget=None, fresh=True):
    """decompress_batch of the whole batch on `h`: text and verdicts against the oracle, the debug line against the model."""
    capfd.readouterr()
    got, ok = h.decompress_batch(batch.blocks, verify=True)
    lines = debug_lines(capfd.readouterr().err)
    assert len(lines) == 1, lines
    m = check_line(batch.cfg, batch.info, lines[0], budget, fresh)
    assert got == batch.want
    assert ok == batch.ok
    return lines[0], m


def decode(lib, batch: Batch, capfd, budget=None):
    h = handle(lib, batch.cfg)
    try:
        if budget is not None:
            h.set_table_budget(budget)
        return one_pass(h, batch, capfd, budget)
    finally:
        h.close()


# ---- the cases -----------------------------------------------------------------------------------------------------------------

TRIPLES = [(9, 0, False, 1048576), (9, 1, False, 262144), (9, 3, True, 131072)]


def run_overflow_triple(lib, oracle, S, capfd, monkeypatch, dna_order, quality_order, lossy, budget):
    """A budget below the 4-symbol DNA table with no quality table that large: the region was smaller than the table placed in it."""
    monkeypatch.setenv("DSRC_GPU_DEBUG", "1")
    cfg = Config(dna_order=dna_order, quality_order=quality_order, lossy=lossy)
    n = S["n_rec"]
    batch = Batch(oracle, cfg, [alphabet_fastq(12, n_rec=n, q_max=42), alphabet_fastq(40 if not lossy else 20, n_rec=n + 7, q_max=42 if lossy else 93), illumina(S)])
    assert [b["d_scheme"] for b in batch.info] == [0, 0, 0] and d_table(cfg, 0) == 2 * MIB > budget
    assert max(b["q_bytes"] for b in batch.info) < 2 * MIB
    line, _ = decode(lib, batch, capfd, budget)
    assert line["region"] >= 2 * MIB and (line["r4"], line["b4"]) == (3, 3)


def run_rounds_lossy(lib, oracle, S, capfd, monkeypatch):
    """(2, 1, lossy), five blocks, 160 KiB: quality tables of 64 KiB two to a round, the five DNA tables of 32 KiB in one."""
    monkeypatch.setenv("DSRC_GPU_DEBUG", "1")
    cfg = Config.from_levels(2, 1, True)
    batch = Batch(oracle, cfg, [illumina(S, k) for k in range(4)] + [TINY])
    assert [b["q_bytes"] for b in batch.info] == [64 * KIB] * 5 and [b["d_bytes"] for b in batch.info] == [32 * KIB] * 5
    line, _ = decode(lib, batch, capfd, 160 * KIB)
    assert (line["qrounds"], line["n8"], line["r4"], line["b4"]) == (3, 5, 1, 5)
    rev, _ = decode(lib, batch.reordered([4, 3, 2, 1, 0]), capfd, 160 * KIB)
    assert (rev["qrounds"], rev["r4"]) == (3, 1)


def run_rounds_one_table(lib, oracle, S, capfd, monkeypatch):
    """(3, 2), four blocks of one scheme, a budget of exactly one quality table: one table per round."""
    monkeypatch.setenv("DSRC_GPU_DEBUG", "1")
    cfg = Config.from_levels(3, 2)
    batch = Batch(oracle, cfg, [illumina(S, k) for k in range(4)])
    sizes = {b["q_bytes"] for b in batch.info}
    assert len(sizes) == 1
    line, _ = decode(lib, batch, capfd, sizes.pop())
    assert line["qrounds"] == 4 and line["r4"] == 1


def run_rounds_mixed(lib, oracle, S, capfd, monkeypatch):
    """(2, 2): a budget that takes the first two of the batch's mixed tables; a budget above everything; the reversed batch."""
    monkeypatch.setenv("DSRC_GPU_DEBUG", "1")
    cfg = Config.from_levels(2, 2, False, True)
    n = S["n_rec"]
    batch = Batch(oracle, cfg, [alphabet_fastq(12, n_rec=n), alphabet_fastq(40, n_rec=n), illumina(S), alphabet_fastq(90, n_rec=n), TINY])
    sizes = [b["q_bytes"] for b in batch.info]
    assert len(set(sizes)) >= 3, sizes
    budget = al(sizes[0]) + al(sizes[1])
    line, m = decode(lib, batch, capfd, budget)
    assert 1 < line["qrounds"] < 5 and m["q_rounds_list"][0] == [0, 1]
    rev, _ = decode(lib, batch.reordered([4, 3, 2, 1, 0]), capfd, budget)
    assert rev["qrounds"] > 1
    big, _ = decode(lib, batch, capfd, 8 << 30)
    auto, _ = decode(lib, batch, capfd)
    for one in (big, auto):
        assert (one["qrounds"], one["r4"], one["r8"]) == (1, 1, 0)
    assert (big["region"], big["final"]) == (auto["region"], auto["final"])          # nothing at the automatic budget depends on it


def split_budget(cfg, info):
    """A budget (from the model alone) under which the batch takes several quality rounds and one of them holds two alphabet sizes."""
    sizes = [b["q_bytes"] for b in info]
    for k in range(len(sizes) - 1):
        for width in (2, 3):
            budget = sum(al(s) for s in sizes[k: k + width])
            rounds = pack(sizes, slack(max(budget, max(al(s) for s in sizes), al(d_table(cfg, 0)))))
            if len(rounds) > 1 and any(len({info[i]["n"] for i in r}) > 1 for r in rounds):
                return budget
    raise AssertionError("no budget splits this batch into a round of two alphabets")


MIXED_LEVELS = [(1, 1, False, True), (2, 2, False, True), (3, 2, False, True), (2, 1, True, False), (3, 2, True, False)]


def run_mixed_alphabets(lib, oracle, S, capfd, monkeypatch, d, q, lossy, crc):
    """Alphabets of 16, 16, 32, 64 and 128 symbols, illumina, TINY and a block hot enough to rescale in one batch: several k_dec_qrc<N>
    launches over one round, each wave leaving if its block has another alphabet; at the automatic budget and split into rounds."""
    monkeypatch.setenv("DSRC_GPU_DEBUG", "1")
    cfg = Config.from_levels(d, q, lossy, crc)
    batch = Batch(oracle, cfg, mixed_alphabet_chunks(S, lossy))
    ns = [b["n"] for b in batch.info]
    if lossy:
        assert ns == [8] * 6
        budget = 2 * al(batch.info[0]["q_bytes"])
    else:
        assert ns[:5] == [16, 16, 32, 64, 128] and set(ns[5:]) <= {16, 32, 64}, ns
        budget = split_budget(cfg, batch.info)
    auto, _ = decode(lib, batch, capfd)
    assert (auto["qrounds"], auto["r4"]) == (1, 1)
    line, m = decode(lib, batch, capfd, budget)
    assert line["qrounds"] > 1
    if not lossy:
        assert any(len({batch.info[i]["n"] for i in r}) > 1 for r in m["q_rounds_list"]), m


DNA_ORDERS = ("first", "last", "interleaved")


def run_mixed_dna(lib, oracle, S, capfd, monkeypatch, d, where):
    """4-symbol blocks, 8-symbol blocks and a block without a DNA stream in one batch, under a budget below one 8-symbol table:
    k_dec_dnarc<4>, then the region grown, then k_dec_dnarc<8> a table a round, and k_dec_dna0 beside them."""
    monkeypatch.setenv("DSRC_GPU_DEBUG", "1")
    cfg = Config.from_levels(d, 1, False, True)
    n = S["n_rec"]
    four = [illumina(S), alphabet_fastq(12, n_rec=n, seed=2), TINY]
    eight = [alphabet_fastq(20, n_rec=n, iupac=True), alphabet_fastq(12, n_rec=n + 5, iupac=True, seed=3)]
    plain = [plain_block()]
    chunks = {"first": eight + four + plain, "last": plain + four + eight,
              "interleaved": [four[0], eight[0], plain[0], four[1], eight[1], four[2]]}[where]
    batch = Batch(oracle, cfg, chunks)
    assert sorted(b["d_scheme"] for b in batch.info) == [0, 0, 0, 1, 1, 255]
    t8 = d_table(cfg, 1)
    budget = t8 // 4
    assert max(b["q_bytes"] for b in batch.info) < t8
    line, _ = decode(lib, batch, capfd, budget)
    assert (line["b4"], line["b8"], line["r8"], line["plain"]) == (3, 2, 2, 1)
    assert line["region"] < t8 <= line["final"]                      # grown between the quality rounds and the DNA rounds
    auto, _ = decode(lib, batch, capfd)
    assert (auto["r4"], auto["r8"], auto["plain"]) == (1, 1, 1)


def run_handle_passes(lib, oracle, S, capfd, monkeypatch):
    """One handle, several passes: the region does not shrink, comes back after release_memory, budget 0 is automatic again, and
    DSRC_GPU_DEC_TABLE_MB overrides the API's budget.  The texts are the oracle's throughout (one_pass)."""
    monkeypatch.setenv("DSRC_GPU_DEBUG", "1")
    cfg = Config.from_levels(3, 1, False, True)
    batch = Batch(oracle, cfg, [illumina(S, k) for k in range(3)])
    assert [b["d_bytes"] for b in batch.info] == [2 * MIB] * 3
    small, large = 1 * MIB, 1 << 30
    h = handle(lib, cfg)
    try:
        h.set_table_budget(large)
        a, _ = one_pass(h, batch, capfd, large)
        assert (a["qrounds"], a["r4"]) == (1, 1)
        h.set_table_budget(small)
        b, _ = one_pass(h, batch, capfd, small, fresh=False)
        assert (b["qrounds"], b["r4"], b["region"]) == (1, 1, a["region"])          # the region is kept
        h.release_memory()
        c, _ = one_pass(h, batch, capfd, small)
        assert c["r4"] == 3 and c["region"] < a["region"]
        h.release_memory()
        c2, _ = one_pass(h, batch, capfd, small)
        assert (c2["r4"], c2["region"]) == (3, c["region"])
        h.set_table_budget(0)
        e, _ = one_pass(h, batch, capfd)
        assert e["r4"] == 1 and e["budget"] > small
        h.release_memory()
        h.set_table_budget(large)
        monkeypatch.setenv("DSRC_GPU_DEC_TABLE_MB", "1")
        f, _ = one_pass(h, batch, capfd, 1 * MIB)
        assert f["r4"] == 3
        monkeypatch.delenv("DSRC_GPU_DEC_TABLE_MB")
    finally:
        h.close()


def _stage(h, blocks):
    offs, pos = [], 0
    for b in blocks:
        offs.append(pos)
        pos += (len(b) + 63) // 64 * 64
    d_in = h.dev_alloc(pos)
    for b, o in zip(blocks, offs):
        h.dev_upload(d_in + o, b)
    return d_in, offs, [len(b) for b in blocks]


def run_device_entry(lib, oracle, S, capfd, monkeypatch):
    """decompress_batch_device under a budget that forces rounds."""
    monkeypatch.setenv("DSRC_GPU_DEBUG", "1")
    cfg = Config.from_levels(2, 1, True, True)
    batch = Batch(oracle, cfg, [illumina(S, k) for k in range(4)] + [TINY])
    h = handle(lib, cfg)
    try:
        h.set_table_budget(160 * KIB)
        d_in, offs, sizes = _stage(h, batch.blocks)
        cap = sum(len(w) for w in batch.want) + 64
        d_out = h.dev_alloc(cap)
        capfd.readouterr()
        t_offs, t_sizes, ok = h.decompress_batch_device(d_in, offs, sizes, d_out, cap, verify=True)
        line = debug_lines(capfd.readouterr().err)[-1]
        check_line(cfg, batch.info, line, 160 * KIB)
        assert line["qrounds"] == 3
        assert [h.dev_download(d_out + o, s) for o, s in zip(t_offs, t_sizes)] == batch.want and ok == batch.ok
        h.dev_free(d_in); h.dev_free(d_out)
    finally:
        h.close()


def run_columns_entry(lib, oracle, S, capfd, monkeypatch):
    """decompress_columns(verify=True) under a round-forcing budget: the columns of the same call without a budget."""
    import numpy as np
    monkeypatch.setenv("DSRC_GPU_DEBUG", "1")
    cfg = Config.from_levels(3, 1, False, True)
    batch = Batch(oracle, cfg, [illumina(S, k) for k in range(3)] + [alphabet_fastq(40, n_rec=S["n_rec"])])
    res = []
    for budget in (None, 1 * MIB):
        h = handle(lib, cfg)
        try:
            if budget:
                h.set_table_budget(budget)
            capfd.readouterr()
            res.append(h.decompress_columns(batch.blocks, verify=True))
            lines = debug_lines(capfd.readouterr().err)
            assert lines
            for line in lines:                                     # (the sizing call and the decoding call)
                check_line(cfg, batch.info, line, budget, fresh=line is lines[0])
            assert lines[-1]["r4"] == (4 if budget else 1)
        finally:
            h.close()
    a, b = res
    for name in ("bases", "quals", "titles", "seq_offsets", "title_offsets"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert (a.block_records, a.totals, list(a.crc_ok)) == (b.block_records, b.totals, list(b.crc_ok))
    assert list(b.crc_ok) == batch.ok
    text = b"".join(batch.want)
    assert int(b.totals[0]) == text.count(b"\n") // 4


def run_verifying_compress(lib, oracle, S, capfd, monkeypatch):
    """Handle(crc, verify).compress_batch: the verifying pass (with hints) under a budget.  Its DNA chains run beside the quality
    chains (`par`) when the tables of both fit the budget together, and in rounds behind them when they do not."""
    monkeypatch.setenv("DSRC_GPU_DEBUG", "1")
    cfg = Config.from_levels(2, 1, True, True)
    chunks = [illumina(S, k) for k in range(4)] + [TINY]
    batch = Batch(oracle, cfg, chunks)
    total = sum(al(b["q_bytes"]) + al(b["d_bytes"]) for b in batch.info)
    assert total == 5 * (64 + 32) * KIB
    for budget, par in ((total, 1), (total - ALIGN, 0), (160 * KIB, 0)):
        h = handle(lib, cfg, verify=True)
        try:
            h.set_table_budget(budget)
            capfd.readouterr()
            got = h.compress_batch(chunks)
            lines = debug_lines(capfd.readouterr().err)
            assert len(lines) == 1, lines
            check_line(cfg, batch.info, lines[0], budget)
            assert lines[0]["par"] == par, lines[0]
            assert [g[0] for g in got] == batch.blocks
            if budget == 160 * KIB:
                assert lines[0]["qrounds"] == 3
        finally:
            h.close()


def run_refusal_in_a_batch(lib, oracle, S, capfd, monkeypatch):
    """One truncated block in the middle of a mixed batch under a budget is refused; the next call on the handle decodes the clean batch."""
    monkeypatch.setenv("DSRC_GPU_DEBUG", "1")
    cfg = Config.from_levels(2, 2, False, True)
    n = S["n_rec"]
    batch = Batch(oracle, cfg, [alphabet_fastq(12, n_rec=n), illumina(S), alphabet_fastq(40, n_rec=n), TINY])
    budget = al(batch.info[0]["q_bytes"]) + al(batch.info[1]["q_bytes"])
    bad = list(batch.blocks)
    bad[1] = bad[1][: len(bad[1]) // 2]                             # truncated, as in test_corrupt_and_mismatched_blocks
    h = handle(lib, cfg)
    try:
        h.set_table_budget(budget)
        with pytest.raises(lib.DsrcGpuError):
            h.decompress_batch(bad, verify=True)
        line, _ = one_pass(h, batch, capfd, budget, fresh=False)
        assert line["qrounds"] > 1
    finally:
        h.close()


def run_serial_decoder_sizes_itself(lib, oracle, S, capfd, monkeypatch):
    """Hooks / emulator builds only: the one-lane decoder (DSRC_GPU_DEC_SERIAL) takes a slot of the worst-case size whatever the budget."""
    monkeypatch.setenv("DSRC_GPU_DEC_SERIAL", "1")
    cfg = Config.from_levels(3, 1, False, True)
    batch = Batch(oracle, cfg, [illumina(S, k) for k in range(3)])
    h = handle(lib, cfg)
    try:
        h.set_table_budget(64 * KIB)                                 # below one slot (32 MiB: the 8-symbol DNA table)
        got, ok = h.decompress_batch(batch.blocks, verify=True)
        assert got == batch.want and ok == batch.ok
    finally:
        h.close()
