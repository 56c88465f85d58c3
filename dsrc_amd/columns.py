"""Records as torch tensors: decode_columns (dsrcgpu_decompress_batch_columns_device), the way back, encode_columns
(dsrcgpu_compress_columns_device), and what runs between the two: trim_plan (dsrcgpu_columns_trim_plan), adapter_plan
(dsrcgpu_columns_adapter_plan), kmer_plan (dsrcgpu_columns_kmer_plan, with columns_from_sequences for its reference), correct_kmers
(dsrcgpu_columns_kmer_correct), pair_plan
(dsrcgpu_columns_pair_plan), dedup_plan (dsrcgpu_columns_dedup_plan), merge_pairs (dsrcgpu_columns_merge_device), select_columns
(dsrcgpu_columns_select_device), filter_columns and, for paired-end data,
filter_pairs, demux_plan and partition_columns (dsrcgpu_columns_demux_plan, dsrcgpu_columns_partition_device) with class_view and
demux_columns, the report on either side of them, profile_columns (dsrcgpu_columns_profile), and the k-mer table of a plan, count_kmers
and KmerTable (dsrcgpu_columns_kmer_count, dsrcgpu_kmer_table_merge, dsrcgpu_kmer_spectrum, dsrcgpu_kmer_lookup), include/dsrc_gpu.h.

The blocks are already in device memory; the arrays are allocated by torch on the same device and filled by the library's
kernels -- no text, no host round trip of the payload.  With the emulator build of the library (tests/emu) device pointers
are host pointers, so CPU tensors work there.

Import this module (or torch) before the first Handle is created: a torch wheel that bundles its own HIP runtime finds no
device when another copy of the runtime -- the one libdsrc_gpu.so is linked to -- is already in the process; loaded after
torch, the library shares torch's copy (bench.py and dsrc_amd/dist.py work the same way).
"""
from __future__ import annotations

import dataclasses

import torch

from . import _lib


@dataclasses.dataclass
class RecordColumns:
    bases: torch.Tensor            # uint8, one code per base: index in "ACGTNRWSKMDVHBYXU.-", 255 = any other byte
    quals: torch.Tensor            # uint8, quality character - quality offset, same positions as bases
    titles: torch.Tensor           # uint8, title lines back to back ('@' included, no newline); empty when titles=False
    seq_offsets: torch.Tensor      # int64, records + 1: record r's bases and qualities are [seq_offsets[r], seq_offsets[r + 1])
    title_offsets: torch.Tensor    # int64, records + 1; empty when titles=False
    block_records: torch.Tensor    # int64, blocks + 1: exclusive prefix of the records per block

    @property
    def n_records(self) -> int:
        return self.seq_offsets.numel() - 1


def decode_columns(handle: _lib.Handle, d_blocks, offs, sizes, device, titles: bool = True) -> RecordColumns:
    """Decode the blocks d_blocks[offs[i] : offs[i] + sizes[i]] (a uint8 tensor on `device`, or a device address) into
    RecordColumns on `device`.  The first library call only sizes the arrays (capacities of zero), the second one decodes."""
    device = torch.device(device)
    d_in = d_blocks.data_ptr() if isinstance(d_blocks, torch.Tensor) else int(d_blocks)
    offs = [int(o) for o in offs]; sizes = [int(s) for s in sizes]

    def quiesce():
        # the library works on its own stream and returns only after synchronising it: memory the allocator has just handed
        # out again (and the blocks themselves) must not have work of torch's stream pending on it
        if device.type == "cuda":
            torch.cuda.current_stream(device).synchronize()

    need = [0, 0, 0]
    if offs:
        quiesce()
        try:
            handle.decompress_columns_device(d_in, offs, sizes, _lib.Columns())
        except _lib.DsrcGpuError as e:
            if e.code != _lib.E_CAPACITY or not any(e.need):      # (all zero: it is a block's text that does not fit)
                raise
            need = e.need
    n_recs, n_bases, n_title = need
    u8 = dict(dtype=torch.uint8, device=device); i64 = dict(dtype=torch.int64, device=device)
    bases = torch.empty(n_bases, **u8); quals = torch.empty(n_bases, **u8)
    seq_offsets = torch.empty(n_recs + 1, **i64)
    title_bytes = torch.empty(n_title if titles else 0, **u8)
    title_offsets = torch.empty(n_recs + 1 if titles else 0, **i64)
    # (data_ptr() of an empty tensor is null: one spare byte keeps "titles wanted, none there" apart from "not wanted")
    spare = torch.empty(8, **u8)
    ptr = lambda t: t.data_ptr() if t.numel() else spare.data_ptr()
    cols = _lib.Columns(ptr(bases), n_bases, ptr(quals), n_bases, ptr(title_bytes) if titles else None, n_title if titles else 0,
                        seq_offsets.data_ptr(), title_offsets.data_ptr() if titles else None, n_recs)
    quiesce()
    block_records, totals = handle.decompress_columns_device(d_in, offs, sizes, cols)
    assert totals == need
    return RecordColumns(bases, quals, title_bytes, seq_offsets, title_offsets, torch.tensor(block_records, **i64))


def encode_columns(handle: _lib.Handle, cols: RecordColumns, block_records=None, chunk_bytes: int = 8 << 20):
    """Compress the records of `cols` (tensors on one device, as decode_columns returns them) into DSRC blocks on that device:
    -> (blocks: uint8 tensor, offs, sizes, block_records); block i is blocks[offs[i] : offs[i] + sizes[i]] and holds records
    block_records[i] .. block_records[i + 1] - 1.  block_records=None: the greedy cut of dsrcgpu_columns_cut at chunk_bytes of
    chunk text per block.  No text is written by the caller and nothing of the payload crosses to the host."""
    device = cols.bases.device
    R = cols.n_records
    if cols.title_offsets.numel() != R + 1:
        raise ValueError("encode_columns needs the titles (decode_columns(..., titles=True))")

    def quiesce():       # as in decode_columns: the library works on its own stream
        if device.type == "cuda":
            torch.cuda.current_stream(device).synchronize()

    spare = torch.empty(8, dtype=torch.uint8, device=device)
    ptr = lambda t: t.data_ptr() if t.numel() else spare.data_ptr()
    held = [t.contiguous() for t in (cols.bases, cols.quals, cols.titles, cols.seq_offsets, cols.title_offsets)]
    bases, quals, titles, seq_offs, title_offs = held
    cin = _lib.ColumnsIn(ptr(bases), bases.numel(), ptr(quals), ptr(titles), titles.numel(), seq_offs.data_ptr(), title_offs.data_ptr(), R)
    if block_records is None:
        quiesce()
        block_records = handle.columns_cut(cin, chunk_bytes)
    block_records = [int(v) for v in (block_records.tolist() if isinstance(block_records, torch.Tensor) else block_records)]
    n = len(block_records) - 1
    # (the text: two bytes a base, the title at most twice, six more a record; a block is not larger than its text + 64 KiB)
    cap = 2 * bases.numel() + 2 * titles.numel() + 6 * R + n * (1 << 16) + 64
    blocks = torch.empty(cap, dtype=torch.uint8, device=device)
    quiesce()
    offs, sizes, _, _ = handle.compress_columns_device(cin, block_records, blocks.data_ptr(), cap)
    return blocks, offs, sizes, block_records


def _columns_in(cols: RecordColumns, titles: bool):
    """-> (_lib.ColumnsIn over the tensors of `cols`, the tensors to keep alive while it is in use)."""
    device = cols.bases.device
    spare = torch.empty(8, dtype=torch.uint8, device=device)
    ptr = lambda t: t.data_ptr() if t.numel() else spare.data_ptr()
    held = [t.contiguous() for t in (cols.bases, cols.quals, cols.titles, cols.seq_offsets, cols.title_offsets)] + [spare]
    bases, quals, title_bytes, seq_offs, title_offs = held[:5]
    R = cols.n_records
    if titles and title_offs.numel() != R + 1:
        raise ValueError("these columns have no titles (decode_columns(..., titles=False))")
    cin = _lib.ColumnsIn(ptr(bases), bases.numel(), ptr(quals), ptr(title_bytes) if titles else None, title_bytes.numel() if titles else 0,
                         seq_offs.data_ptr(), title_offs.data_ptr() if titles else None, R)
    return cin, held


def _quiesce(device):       # as in decode_columns: the library works on its own stream
    if device.type == "cuda":
        torch.cuda.current_stream(device).synchronize()


def _adr(t):
    """The device address of a tensor; None for no tensor and for an empty one."""
    return None if t is None or not t.numel() else t.data_ptr()


def _together(*ranges):
    if any((begin is None) != (end is None) for begin, end in ranges):
        raise ValueError("begin and end go together")


def _stage_plan(n, device, ranges, keep, insert=None):
    """A plan as the library takes it: `ranges` is a list of (begin, end) pairs, one per side, each both given or both None; `keep` and
    (merge_pairs) `insert` are tensors or None.  Checks that the ends go together, brings what is given to contiguous int64 / uint8 and
    checks that it has n entries on `device` -> (addresses, held): the device addresses in the order begin, end of every side[, insert],
    keep -- None for what is absent or empty --, and the tensors to keep alive while the addresses are in use."""
    _together(*ranges)
    held = [None if t is None else t.to(torch.int64).contiguous() for t in [t for r in ranges for t in r] + ([] if insert is None else [insert])]
    held.append(None if keep is None else keep.to(torch.uint8).contiguous())
    if any(t is not None and (t.numel() != n or t.device != device) for t in held):
        raise ValueError("begin, end, keep and insert have one entry per pair, on the device of the columns" if insert is not None else
                         "begin, end and keep have one entry per record, on the device of the columns")
    return [_adr(t) for t in held], held


def trim_plan(handle: _lib.Handle, cols: RecordColumns, quality_5: int = 0, quality_3: int = 0, min_length: int = 1, max_n=None,
              min_mean_quality: int = 0):
    """dsrcgpu_columns_trim_plan on the records of `cols`: -> (begin, end, keep, stats).  begin / end (int64) are the kept range of
    every record as positions in cols.bases, keep (uint8) is 1 for the records that pass the rules, stats is a dict with the keys
    of _lib.TRIM_STATS.  quality_5 / quality_3: Phred cutoffs of the running-sum trim, 0 = that end is left alone; max_n=None: no
    limit on bases other than A C G T.  Nothing of the payload crosses to the host."""
    device = cols.bases.device
    R = cols.n_records
    cin, held = _columns_in(cols, titles=False)
    begin = torch.empty(R, dtype=torch.int64, device=device); end = torch.empty(R, dtype=torch.int64, device=device)
    keep = torch.empty(R, dtype=torch.uint8, device=device)
    rules = _lib.TrimRules(quality_5, quality_3, min_length, 0xFFFFFFFF if max_n is None else max_n, min_mean_quality)
    _quiesce(device)
    stats = handle.columns_trim_plan(cin, rules, begin.data_ptr(), end.data_ptr(), keep.data_ptr())
    del held
    return begin, end, keep, dict(zip(_lib.TRIM_STATS, stats))


def select_columns(handle: _lib.Handle, cols: RecordColumns, begin=None, end=None, keep=None, titles: bool = True, return_source: bool = False):
    """dsrcgpu_columns_select_device: the records of `cols` with a non-zero `keep` entry (None: all), bases and qualities cut to
    [begin[r], end[r]) (None: whole reads), titles whole, compacted into new tensors on the same device -> RecordColumns with
    block_records = [0, kept]; return_source=True: -> (RecordColumns, source), source[j] = the index in `cols` of output record j.
    begin / end are int64 (or uint64-valued) tensors, keep a uint8 or bool tensor, as trim_plan returns them.  The first library call
    sizes the arrays, the second one fills them."""
    device = cols.bases.device
    _together((begin, end))                                  # (in front of the titles check of _columns_in)
    cin, held = _columns_in(cols, titles)
    plan, plan_held = _stage_plan(cols.n_records, device, [(begin, end)], keep)
    spare = held[-1]
    _quiesce(device)
    need = [0, 0, 0]
    try:
        handle.columns_select_device(cin, *plan, _lib.Columns(d_titles=spare.data_ptr() if titles else None))
    except _lib.DsrcGpuError as e:
        if e.code != _lib.E_CAPACITY:
            raise
        need = e.need
    K, S, T = need
    u8 = dict(dtype=torch.uint8, device=device); i64 = dict(dtype=torch.int64, device=device)
    bases = torch.empty(S, **u8); quals = torch.empty(S, **u8)
    seq_offsets = torch.empty(K + 1, **i64)
    title_bytes = torch.empty(T if titles else 0, **u8)
    title_offsets = torch.empty(K + 1 if titles else 0, **i64)
    source = torch.empty(K, **i64)
    ptr = lambda t: t.data_ptr() if t.numel() else spare.data_ptr()
    out = _lib.Columns(ptr(bases), S, ptr(quals), S, ptr(title_bytes) if titles else None, T if titles else 0,
                       seq_offsets.data_ptr(), title_offsets.data_ptr() if titles else None, K)
    _quiesce(device)
    totals = handle.columns_select_device(cin, *plan, out, _adr(source) if return_source else None)
    assert totals == need
    del held, plan_held
    got = RecordColumns(bases, quals, title_bytes, seq_offsets, title_offsets, torch.tensor([0, K], **i64))
    return (got, source) if return_source else got


_BASE_CODES = {"A": 0, "C": 1, "G": 2, "T": 3}


def _adapter_codes(adapters):
    """`adapters` (strs over ACGT in either case, or sequences of codes 0 .. 3) as a list of bytes; ValueError for anything else."""
    if isinstance(adapters, (str, bytes, bytearray)) or not hasattr(adapters, "__len__"):
        raise ValueError("adapters is a list of strings over ACGT or of sequences of base codes 0..3")
    if not 1 <= len(adapters) <= 8:
        raise ValueError("between 1 and 8 adapters are needed, %d given" % len(adapters))
    out = []
    for a in adapters:
        if isinstance(a, str):
            if any(ch not in _BASE_CODES for ch in a.upper()):
                raise ValueError("adapter %r: only A, C, G and T are allowed" % a)
            codes = [_BASE_CODES[ch] for ch in a.upper()]
        else:
            try:
                codes = [int(v) for v in a]
            except (TypeError, ValueError):
                raise ValueError("adapter %r is neither a string nor a sequence of base codes" % (a,)) from None
            if any(v < 0 or v > 3 for v in codes):
                raise ValueError("adapter %r: base codes are 0..3" % (a,))
        if not 1 <= len(codes) <= 64:
            raise ValueError("an adapter has 1 to 64 bases, %d given" % len(codes))
        out.append(bytes(codes))
    return out


def adapter_plan(handle: _lib.Handle, cols: RecordColumns, adapters, begin=None, end=None, keep=None, min_overlap: int = 3,
                 max_error_permille: int = 100, min_length: int = 1, return_which: bool = False):
    """dsrcgpu_columns_adapter_plan on the records of `cols`: the 3' adapter search on the plan begin / end / keep (None: whole
    reads, every record; as trim_plan returns them) -> (begin, end, keep, stats[, which]) in fresh tensors.  `adapters`: up to 8 strs
    over ACGT (either case) or sequences of codes 0 .. 3, 1 .. 64 bases each; anything else raises ValueError before the library is
    called.  The leftmost start position at which an adapter -- or its first min_overlap and more bases, at the end of the range
    -- matches with at most max_error_permille mismatches per 1000 compared bases becomes the new end; a record is kept iff it came
    in kept and at least min_length bases are left.  stats is a dict with the keys of _lib.ADAPTER_STATS; which (int64) is the index
    of the adapter found, -1 for none.  Nothing of the payload crosses to the host."""
    codes = _adapter_codes(adapters)
    for name, v, lo, hi in (("min_overlap", min_overlap, 1, min(len(c) for c in codes)), ("max_error_permille", max_error_permille, 0, 1000),
                            ("min_length", min_length, 0, 0xFFFFFFFF)):
        if not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError("%s must be an integer in %d..%d" % (name, lo, hi))
    device = cols.bases.device
    R = cols.n_records
    plan, plan_held = _stage_plan(R, device, [(begin, end)], keep)
    cin, held = _columns_in(cols, titles=False)
    out_begin = torch.empty(R, dtype=torch.int64, device=device); out_end = torch.empty(R, dtype=torch.int64, device=device)
    out_keep = torch.empty(R, dtype=torch.uint8, device=device)
    which = torch.empty(R, dtype=torch.int32, device=device) if return_which else None
    rules = _lib.AdapterRules(codes, min_overlap, max_error_permille, min_length)
    _quiesce(device)
    stats = handle.columns_adapter_plan(cin, rules, *plan, out_begin.data_ptr(), out_end.data_ptr(), out_keep.data_ptr(), _adr(which))
    del held, plan_held
    got = (out_begin, out_end, out_keep, dict(zip(_lib.ADAPTER_STATS, stats)))
    return got + (which.to(torch.int64),) if return_which else got


def _base_mask(name, bases):
    """`bases` (a str over ACGT in either case, each base at most once) as the mask of dsrcgpu_complexity_rules: A = 1, C = 2, G = 4, T = 8."""
    if not isinstance(bases, str) or any(ch not in _BASE_CODES for ch in bases.upper()) or len(set(bases.upper())) != len(bases):
        raise ValueError("%s is a string over ACGT, each base at most once, %r given" % (name, bases))
    return sum(1 << _BASE_CODES[ch] for ch in bases.upper())


def _check_complexity_args(tail="", head="", poly_min_length=10, poly_max_error_permille=125, min_length=1, min_complexity_permille=0,
                           max_dust=None, max_dust_windows=0):
    """The keywords of complexity_plan, checked -> _lib.ComplexityRules.  ValueError for anything out of range."""
    masks = _base_mask("tail", tail), _base_mask("head", head)
    _check_int("poly_min_length", poly_min_length, 1, 0xFFFFFFFF)
    _check_int("poly_max_error_permille", poly_max_error_permille, 0, 1000)
    _check_int("min_length", min_length, 0, 0xFFFFFFFF)
    _check_int("min_complexity_permille", min_complexity_permille, 0, 1000)
    if max_dust is not None:
        _check_int("max_dust", max_dust, 0, 0xFFFFFFFE)
    _check_int("max_dust_windows", max_dust_windows, 0, 0xFFFFFFFF)
    return _lib.ComplexityRules(masks[0], masks[1], poly_min_length, poly_max_error_permille, min_length, min_complexity_permille,
                                0xFFFFFFFF if max_dust is None else max_dust, max_dust_windows)


def _check_complexity(complexity):
    if not isinstance(complexity, dict):
        raise ValueError("complexity is a dict of complexity_plan keywords")
    try:
        _check_complexity_args(**complexity)
    except TypeError:
        raise ValueError("complexity holds keywords of complexity_plan (tail, head, poly_min_length, poly_max_error_permille, min_length, "
                         "min_complexity_permille, max_dust, max_dust_windows), %r given" % sorted(complexity)) from None


def complexity_plan(handle: _lib.Handle, cols: RecordColumns, begin=None, end=None, keep=None, tail: str = "", head: str = "",
                    poly_min_length: int = 10, poly_max_error_permille: int = 125, min_length: int = 1, min_complexity_permille: int = 0,
                    max_dust=None, max_dust_windows: int = 0, return_info: bool = False):
    """dsrcgpu_columns_complexity_plan on the records of `cols`: poly-X runs are cut off the ends of the plan begin / end / keep (None:
    whole reads, every record; as trim_plan returns them), then what is left is judged -> (begin, end, keep, stats[, head_base,
    tail_base, complexity_permille, dust]) in fresh tensors.  tail / head: the bases (a str over ACGT) whose runs are searched at the
    3' / 5' end -- fastp's poly-G is tail="G", its poly-X tail="ACGT", RNA-seq poly-A tails tail="A" and head="T"; a run is scored
    +1 per position that holds the base and -2 per other one (cutadapt's poly-A rule), may hold poly_max_error_permille other
    positions per 1000 and is cut if it spans at least poly_min_length.  A record is kept iff it came in kept, at least min_length
    bases are left, at least min_complexity_permille of 1000 neighbouring positions of the rest differ (fastp's 30 % is 300; 0 = off)
    and at most max_dust_windows of its 64-base windows score above max_dust (sdust's 20; None = off).  stats is a dict with the keys
    of _lib.COMPLEXITY_STATS; head_base / tail_base (int64) are the base code cut at that end, -1 for none, complexity_permille and dust
    (int64) the two scores of what is left; all four are -1 for a record that came in dropped.  Arguments out of range raise ValueError
    before the library is called.  Nothing of the payload crosses to the host."""
    rules = _check_complexity_args(tail, head, poly_min_length, poly_max_error_permille, min_length, min_complexity_permille, max_dust,
                                   max_dust_windows)
    device = cols.bases.device
    R = cols.n_records
    plan, plan_held = _stage_plan(R, device, [(begin, end)], keep)
    cin, held = _columns_in(cols, titles=False)
    out_begin = torch.empty(R, dtype=torch.int64, device=device); out_end = torch.empty(R, dtype=torch.int64, device=device)
    out_keep = torch.empty(R, dtype=torch.uint8, device=device)
    info = torch.empty((R, 2), dtype=torch.int32, device=device) if return_info else None
    _quiesce(device)
    stats = handle.columns_complexity_plan(cin, rules, *plan, out_begin.data_ptr(), out_end.data_ptr(), out_keep.data_ptr(), _adr(info))
    del held, plan_held
    got = (out_begin, out_end, out_keep, dict(zip(_lib.COMPLEXITY_STATS, stats)))
    if not return_info:
        return got
    word0, word1 = info[:, 0].to(torch.int64), info[:, 1].to(torch.int64)
    dropped = word0 == 0xFFFF
    base = lambda v: torch.where(v == _lib.COMPLEXITY_NONE, torch.full_like(v, -1), v)
    score = lambda v: torch.where(dropped, torch.full_like(v, -1), v)
    return got + (base(word0 & 255), base((word0 >> 8) & 255), score(word1 & 0xFFFF), score((word1 >> 16) & 0xFFFF))


@dataclasses.dataclass
class ColumnsProfile:
    """A profile of dsrcgpu_columns_profile: one int64 tensor of _lib.profile_words(n_cycles) counts on the device of the columns
    (layout: include/dsrc_gpu.h) and views of its tables.  Nothing is copied but by summary()."""
    data: torch.Tensor
    n_cycles: int

    def _table(self, offset, count):
        return self.data[offset: offset + count]

    @property
    def totals(self):                  # 8, named by _lib.PROFILE_TOTALS
        return self._table(0, 8)

    @property
    def base_by_cycle(self):           # n_cycles x 5: A, C, G, T, anything else
        return self._table(8, 5 * self.n_cycles).view(self.n_cycles, 5)

    @property
    def quality_sum_by_cycle(self):    # n_cycles x 5
        return self._table(8 + 5 * self.n_cycles, 5 * self.n_cycles).view(self.n_cycles, 5)

    @property
    def quality_hist(self):            # 256
        return self._table(8 + 10 * self.n_cycles, 256)

    @property
    def length_hist(self):             # n_cycles + 1: the last bin holds the ranges of n_cycles bases and more
        return self._table(264 + 10 * self.n_cycles, self.n_cycles + 1)

    @property
    def gc_hist(self):                 # 101: percent G or C among A C G T
        return self._table(265 + 11 * self.n_cycles, 101)

    @property
    def mean_quality_hist(self):       # 256
        return self._table(366 + 11 * self.n_cycles, 256)

    def summary(self) -> dict:
        """The eight totals as a dict of ints -- the only part that crosses to the host."""
        return dict(zip(_lib.PROFILE_TOTALS, self.totals.tolist()))


def profile_columns(handle: _lib.Handle, cols: RecordColumns, begin=None, end=None, keep=None, n_cycles=None, into=None) -> ColumnsProfile:
    """dsrcgpu_columns_profile on the records of `cols` under the plan begin / end / keep (None: whole reads, every record; as the
    planners return them) -> ColumnsProfile.  The cycle of a base is its position in the RANGE; positions from n_cycles - 1 on fold
    into the last cycle.  n_cycles=None: the longest stored read, clipped to 1 .. _lib.PROFILE_MAX_CYCLES (that of `into` if given).
    into: an earlier ColumnsProfile of the same n_cycles on the same device -- the counts are added to its tensor and it is returned,
    so that the batches of a file sum to the profile of the file.  The profile of a plan equals the profile of select_columns with that
    plan and needs no select.  Arguments out of range raise ValueError before the library is called.  Nothing of the payload crosses
    to the host."""
    device = cols.bases.device
    R = cols.n_records
    if into is not None:
        if not isinstance(into, ColumnsProfile) or n_cycles not in (None, into.n_cycles):
            raise ValueError("into is an earlier ColumnsProfile with the same n_cycles")
        n_cycles = into.n_cycles
    if n_cycles is None:
        n_cycles = min(max(int(cols.seq_offsets.diff().max()), 1), _lib.PROFILE_MAX_CYCLES) if R else 1
    _check_int("n_cycles", n_cycles, 1, _lib.PROFILE_MAX_CYCLES)
    words = _lib.profile_words(n_cycles)
    if into is not None and (into.data.dtype != torch.int64 or into.data.numel() != words or into.data.device != device or not into.data.is_contiguous()):
        raise ValueError("into holds %d int64 counts on the device of the columns" % words)
    plan, plan_held = _stage_plan(R, device, [(begin, end)], keep)
    cin, held = _columns_in(cols, titles=False)
    out = into if into is not None else ColumnsProfile(torch.empty(words, dtype=torch.int64, device=device), n_cycles)
    _quiesce(device)
    handle.columns_profile(cin, *plan, _lib.ProfileRules(n_cycles, 1 if into is not None else 0), out.data.data_ptr())
    del held, plan_held
    return out


def filter_columns(handle: _lib.Handle, cols: RecordColumns, titles: bool = True, adapters=None, adapter_min_overlap: int = 3,
                   adapter_max_error_permille: int = 100, profile: bool = False, dedup: bool = False, dedup_key_bases: int = 0,
                   dedup_prefer: str = "first", kmers=None, screen=None, correct=None, complexity=None, demux=None, **rules):
    """trim_plan(**rules) and select_columns with its plan in sequence: -> (RecordColumns of the trimmed, kept records, stats).
    adapters (see adapter_plan): between the two, adapter_plan narrows the trim plan -- the quality trim first, the adapter second,
    the order of cutadapt and fastp -- with the same min_length; stats is then the trim plan's dict plus a key "adapter" that holds
    the adapter plan's dict, and the number of records that come out is stats["adapter"]["records_kept"].  max_n and
    min_mean_quality were judged on the range before the adapter cut.
    profile=True: stats gets "profile_before", the ColumnsProfile of `cols` as they came, and "profile_after", that of the records
    that come out -- taken from the final plan on `cols`, with the same n_cycles.
    dedup=True: last among the plans, dedup_plan(key_bases=dedup_key_bases, prefer=dedup_prefer) on the final ranges and keep leaves one
    record of every set of exact duplicates; stats gets "dedup", its dict, the number of records that come out is
    stats["dedup"]["records_kept"], and "profile_after" reflects it.
    kmers=k (an int, 1 .. 31): stats gets "kmers_after", the KmerTable of count_kmers(k) under the final plan on `cols` -- the
    canonical k-mers of the records that come out, and it needs no select.
    screen (a dict of kmer_plan keywords, its `table` among them): behind the adapter plan and in front of dedup, kmer_plan narrows the
    plan against that table -- a contaminant screen (max_hits=0) or an abundance trim -- with the filter's min_length unless the dict
    gives one; stats gets "screen", its dict, and profile, kmers and the select see the narrowed plan.
    correct (a dict: min_count and max_quality of correct_kmers, and either table=a KmerTable or k=an int): behind the adapter plan and
    in front of the screen, correct_kmers repairs the bases on the ranges and keep at that point -- with k= against the table of
    count_kmers(k) of the batch under that very plan; stats gets "correct", its dict.  Everything behind it (screen, dedup,
    "profile_after", "kmers_after", the select) sees the repaired bases; `cols` stays as it is, and "profile_before", and max_n of
    the trim plan, saw the bases as they came.
    complexity (a dict of complexity_plan keywords): behind the adapter plan and in front of correct, complexity_plan cuts poly-X ends
    and drops low-complexity reads, with the filter's min_length unless the dict gives one; stats gets "complexity", its dict, and
    everything behind it sees the narrowed plan.
    demux (a dict of demux_plan keywords, its `barcodes` among them): directly behind the trim plan, demux_plan assigns every record its
    sample and cuts the inline barcode, with the filter's min_length unless the dict gives one, so that every later plan sees the
    cut; the filter then ends in partition_columns instead of select_columns: the records come out grouped by sample, block_records
    is the class prefix over n_samples (+ 1 with keep_unassigned) classes and class_view hands out a sample.  stats gets "demux", the
    plan's dict plus "class_records".  ValueError: an inline slot together with quality_5 (the 5' trim would eat the barcode), and
    dedup=True together with demux (duplicates are per sample: dedup the views)."""
    if demux is not None:
        demux = _check_demux(demux, cols, rules.get("quality_5", 0), dedup)
    if adapters is not None:
        codes = _adapter_codes(adapters)
    if complexity is not None:
        _check_complexity(complexity)
    if screen is not None:
        _check_screen(screen, cols)
    if correct is not None:
        _check_correct(correct, cols)
    if kmers is not None:
        _check_int("kmers", kmers, 1, _lib.KMER_MAX_K)
    if dedup:
        _check_dedup_args(dedup_key_bases, dedup_prefer)
    begin, end, keep, stats = trim_plan(handle, cols, **rules)
    classes = None
    if demux is not None:
        begin, end, keep, classes, m_stats = demux_plan(handle, cols, begin=begin, end=end, keep=keep,
                                                        **dict(dict(min_length=rules.get("min_length", 1)), **demux))
        stats = dict(stats, demux=m_stats)
    if adapters is not None:
        begin, end, keep, a_stats = adapter_plan(handle, cols, codes, begin, end, keep, adapter_min_overlap, adapter_max_error_permille,
                                                 rules.get("min_length", 1))
        stats = dict(stats, adapter=a_stats)
    if complexity is not None:
        begin, end, keep, x_stats = complexity_plan(handle, cols, begin, end, keep, **dict(dict(min_length=rules.get("min_length", 1)), **complexity))
        stats = dict(stats, complexity=x_stats)
    came = cols
    if correct is not None:
        cols, c_stats = _correct_step(handle, [(cols, begin, end, keep)], correct)[0]
        stats = dict(stats, correct=c_stats)
    if screen is not None:
        begin, end, keep, s_stats = kmer_plan(handle, cols, begin=begin, end=end, keep=keep,
                                              **dict(dict(min_length=rules.get("min_length", 1)), **screen))
        stats = dict(stats, screen=s_stats)
    if dedup:
        keep, d_stats = dedup_plan(handle, cols, begin=begin, end=end, keep=keep, key_bases=dedup_key_bases, prefer=dedup_prefer)
        stats = dict(stats, dedup=d_stats)
    if profile:
        before = profile_columns(handle, came)
        stats = dict(stats, profile_before=before, profile_after=profile_columns(handle, cols, begin, end, keep, n_cycles=before.n_cycles))
    if kmers is not None:
        stats = dict(stats, kmers_after=count_kmers(handle, cols, kmers, begin, end, keep)[0])
    if classes is not None:
        n_classes = stats["demux"]["class_counts"].numel() - (0 if demux.get("keep_unassigned", False) else 1)
        parts = partition_columns(handle, cols, classes, n_classes, begin, end, keep, titles=titles)
        return parts, dict(stats, demux=dict(stats["demux"], class_records=parts.block_records.tolist()))
    return select_columns(handle, cols, begin, end, keep, titles=titles), stats


def _check_int(name, v, lo, hi):
    if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
        raise ValueError("%s must be an integer in %d..%d" % (name, lo, hi))


def _check_pair_args(cols1, cols2, min_overlap, max_mismatches, max_error_permille, min_length):
    _check_int("min_overlap", min_overlap, 1, _lib.PAIR_MAX_BASES)
    _check_int("max_mismatches", max_mismatches, 0, 0xFFFFFFFF)
    _check_int("max_error_permille", max_error_permille, 0, 1000)
    _check_int("min_length", min_length, 0, 0xFFFFFFFF)
    if cols1.n_records != cols2.n_records:
        raise ValueError("the mates come in equal numbers: %d records of read 1, %d of read 2" % (cols1.n_records, cols2.n_records))
    if cols1.bases.device != cols2.bases.device:
        raise ValueError("both column sets live on one device")


def pair_plan(handle: _lib.Handle, cols1: RecordColumns, cols2: RecordColumns, plan1=None, plan2=None, min_overlap: int = 30,
              max_mismatches: int = 5, max_error_permille: int = 200, min_length: int = 1, return_insert: bool = False):
    """dsrcgpu_columns_pair_plan on the mates cols1 / cols2 (record r of one is the mate of record r of the other): the overlap of
    read 1 with the reverse complement of read 2 gives the insert size, each mate's 3' end is cut where the insert ends, and a pair is
    kept iff both mates came in kept and both are still min_length bases long -> (begin1, end1, begin2, end2, keep, stats[, insert])
    in fresh tensors.  plan1 / plan2: a (begin, end, keep) triple per side as trim_plan and adapter_plan return it (begin and end may
    both be None, keep may be None), or None: whole reads, every record.  An overlap is accepted with at least min_overlap compared
    bases, at most max_mismatches mismatches and at most max_error_permille of them per 1000 compared bases; forward shifts are tried
    first, then read-through shifts, the first accepted one wins.  stats is a dict with the keys of _lib.PAIR_STATS; insert (int64)
    is the insert size of the pair, -1 where no overlap was found.  Arguments out of range, and column sets of different record
    counts or devices, raise ValueError before the library is called.  Nothing of the payload crosses to the host."""
    _check_pair_args(cols1, cols2, min_overlap, max_mismatches, max_error_permille, min_length)
    device = cols1.bases.device
    R = cols1.n_records
    plans = []
    for plan in (plan1, plan2):
        begin, end, keep = (None, None, None) if plan is None else plan
        plans.append(_stage_plan(R, device, [(begin, end)], keep))
    cin1, held1 = _columns_in(cols1, titles=False)
    cin2, held2 = _columns_in(cols2, titles=False)
    i64 = dict(dtype=torch.int64, device=device)
    out = [torch.empty(R, **i64) for _ in range(4)]
    keep = torch.empty(R, dtype=torch.uint8, device=device)
    insert = torch.empty(R, **i64) if return_insert else None
    rules = _lib.PairRules(min_overlap, max_mismatches, max_error_permille, min_length)
    _quiesce(device)
    stats = handle.columns_pair_plan(cin1, cin2, rules, tuple(plans[0][0]), tuple(plans[1][0]),
                                     out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), keep.data_ptr(), _adr(insert))
    del held1, held2, plans
    got = (out[0], out[1], out[2], out[3], keep, dict(zip(_lib.PAIR_STATS, stats)))
    return got + (insert,) if return_insert else got          # (2^64 - 1 read as int64 is -1)


def _check_dedup_args(key_bases, prefer):
    _check_int("key_bases", key_bases, 0, 0xFFFFFFFF)
    if not isinstance(prefer, str) or prefer not in _lib.DEDUP_PREFER:
        raise ValueError("prefer must be one of %s" % ", ".join(repr(k) for k in _lib.DEDUP_PREFER))


def dedup_plan(handle: _lib.Handle, cols: RecordColumns, cols2=None, begin=None, end=None, begin2=None, end2=None, keep=None, key_bases: int = 0,
               prefer: str = "first", return_dup_of: bool = False, return_copies: bool = False):
    """dsrcgpu_columns_dedup_plan on the records of `cols`, or -- with cols2, record r of which is the mate of record r of `cols` -- on
    the pairs: of the considered records (keep non-zero, or keep None) whose keys are equal byte for byte exactly one survives ->
    (keep, stats[, dup_of][, copies]) in fresh tensors.  The key of a record is its range begin / end (None: the whole read), or its
    first key_bases bases (0: all of it), with its length; with cols2 the mate's range begin2 / end2 goes on behind it, and a pair is a
    duplicate only if both mates are.  prefer="first": the lowest index of a class survives; "quality": the member with the highest sum
    of qualities over the key positions, the lowest index on a tie.  keep (uint8) is 1 for the survivors; stats is a dict with the
    keys of _lib.DEDUP_STATS (counts, and the duplication-level histogram in FastQC's bins); dup_of (int64) is the survivor's index
    for every considered record, -1 for a record that came in dropped; copies (int64) is the class size at a survivor, 0 elsewhere.
    No reverse complement, no mismatches, nothing across calls.  Arguments out of range, half-given ranges, ranges of side 2
    without cols2, mis-sized tensors and column sets of different record counts or devices raise ValueError before the library is
    called.  Nothing of the payload crosses to the host."""
    _check_dedup_args(key_bases, prefer)
    device = cols.bases.device
    R = cols.n_records
    if cols2 is not None:
        if cols2.n_records != R:
            raise ValueError("the mates come in equal numbers: %d records of read 1, %d of read 2" % (R, cols2.n_records))
        if cols2.bases.device != device:
            raise ValueError("both column sets live on one device")
    elif begin2 is not None or end2 is not None:
        raise ValueError("begin2 and end2 need cols2")
    _together((begin, end), (begin2, end2))                  # (in front of the record count)
    if R > 1 << 31:
        raise ValueError("at most 2^31 records in one call")
    (b1, e1, b2, e2, keep_in), plan_held = _stage_plan(R, device, [(begin, end), (begin2, end2)], keep)
    cin1, held1 = _columns_in(cols, titles=False)
    cin2, held2 = _columns_in(cols2, titles=False) if cols2 is not None else (None, None)
    out_keep = torch.empty(R, dtype=torch.uint8, device=device)
    dup_of = torch.empty(R, dtype=torch.int64, device=device) if return_dup_of else None
    copies = torch.empty(R, dtype=torch.int64, device=device) if return_copies else None
    rules = _lib.DedupRules(key_bases, _lib.DEDUP_PREFER[prefer])
    _quiesce(device)
    stats = handle.columns_dedup_plan(cin1, cin2, rules, (b1, e1), (b2, e2), keep_in, _adr(out_keep), _adr(dup_of), _adr(copies))
    del held1, held2, plan_held
    got = (out_keep, dict(zip(_lib.DEDUP_STATS, stats)))
    if return_dup_of:
        got += (dup_of,)                                     # (2^64 - 1 read as int64 is -1)
    return got + (copies,) if return_copies else got


def merge_pairs(handle: _lib.Handle, cols1: RecordColumns, cols2: RecordColumns, begin1=None, end1=None, begin2=None, end2=None, keep=None,
                insert=None, min_overlap: int = 30, max_mismatches: int = 5, max_error_permille: int = 200, quality_cap: int = 41,
                titles: bool = True, return_source: bool = False):
    """dsrcgpu_columns_merge_device on the mates cols1 / cols2 with what pair_plan(return_insert=True) gave: the ranges begin<s> /
    end<s> (None: whole reads), the pair's keep (None: every pair) and `insert` (required; int64, -1 = no overlap found).  A kept pair
    whose ranges overlap, at the place its insert size says, by at least min_overlap positions with at most max_mismatches mismatches
    and at most max_error_permille of them per 1000 becomes ONE read: read 1, then the reverse complement of what read 2 adds, with a
    consensus in the overlap -- equal bases sum their qualities up to max(quality_cap, q1, q2), different ones leave the better base
    with the difference -- under read 1's title -> (RecordColumns of the merged reads, merged, stats[, source]): merged (uint8) is 1
    for the pairs that are in the output, stats a dict with the keys of _lib.MERGE_STATS, source[j] (int64) the pair of output record j.
    The unmerged mates are select_columns(..., keep=keep & ~merged) on either side.  The first library call sizes the arrays, the
    second one fills them.  Arguments out of range, half-given ranges, mis-sized tensors and column sets of different record counts or
    devices raise ValueError before the library is called.  Nothing of the payload crosses to the host."""
    _check_int("min_overlap", min_overlap, 1, 0xFFFFFFFF)
    _check_int("max_mismatches", max_mismatches, 0, 0xFFFFFFFF)
    _check_int("max_error_permille", max_error_permille, 0, 1000)
    _check_int("quality_cap", quality_cap, 0, 255)
    if cols1.n_records != cols2.n_records:
        raise ValueError("the mates come in equal numbers: %d records of read 1, %d of read 2" % (cols1.n_records, cols2.n_records))
    if cols1.bases.device != cols2.bases.device:
        raise ValueError("both column sets live on one device")
    if insert is None:
        raise ValueError("insert is needed: the insert sizes of pair_plan(..., return_insert=True)")
    device = cols1.bases.device
    R = cols1.n_records
    (b1, e1, b2, e2, d_insert, d_keep), plan_held = _stage_plan(R, device, [(begin1, end1), (begin2, end2)], keep, insert)
    cin1, held1 = _columns_in(cols1, titles)
    cin2, held2 = _columns_in(cols2, titles=False)
    spare = held1[-1]
    ptr = lambda t: t.data_ptr() if t.numel() else spare.data_ptr()
    u8 = dict(dtype=torch.uint8, device=device); i64 = dict(dtype=torch.int64, device=device)
    merged = torch.empty(R, **u8)
    rules = _lib.MergeRules(min_overlap, max_mismatches, max_error_permille, quality_cap)
    args = (cin1, cin2, rules, (b1, e1), (b2, e2), d_keep, d_insert or spare.data_ptr())      # (no pairs: d_insert is still an address)
    _quiesce(device)
    need = [0, 0, 0]
    try:
        handle.columns_merge_device(*args, _lib.Columns(d_titles=spare.data_ptr() if titles else None), ptr(merged))
    except _lib.DsrcGpuError as e:
        if e.code != _lib.E_CAPACITY:
            raise
        need = e.need
    K, S, T = need
    bases = torch.empty(S, **u8); quals = torch.empty(S, **u8)
    seq_offsets = torch.empty(K + 1, **i64)
    title_bytes = torch.empty(T if titles else 0, **u8)
    title_offsets = torch.empty(K + 1 if titles else 0, **i64)
    source = torch.empty(K, **i64)
    out = _lib.Columns(ptr(bases), S, ptr(quals), S, ptr(title_bytes) if titles else None, T if titles else 0,
                       seq_offsets.data_ptr(), title_offsets.data_ptr() if titles else None, K)
    _quiesce(device)
    totals, stats = handle.columns_merge_device(*args, out, ptr(merged), _adr(source) if return_source else None)
    assert totals == need
    del held1, held2, plan_held
    got = (RecordColumns(bases, quals, title_bytes, seq_offsets, title_offsets, torch.tensor([0, K], **i64)), merged, dict(zip(_lib.MERGE_STATS, stats)))
    return got + (source,) if return_source else got


def filter_pairs(handle: _lib.Handle, cols1: RecordColumns, cols2: RecordColumns, titles: bool = True, adapters1=None, adapters2=None,
                 overlap: bool = True, pair_min_overlap: int = 30, pair_max_mismatches: int = 5, pair_max_error_permille: int = 200,
                 adapter_min_overlap: int = 3, adapter_max_error_permille: int = 100, profile: bool = False, merge: bool = False,
                 merge_quality_cap: int = 41, dedup: bool = False, dedup_key_bases: int = 0, dedup_prefer: str = "first", kmers=None, screen=None,
                 correct=None, complexity=None, demux=None, **rules):
    """filter_columns for paired-end data: per side trim_plan(**rules) and, if adapters<s> is given, adapter_plan; then pair_plan with
    the same min_length, which cuts read-through found from the overlap of the mates and decides per PAIR; then one select_columns per
    side with that side's ranges and the joint keep -> (out1, out2, stats), out1.n_records == out2.n_records always and record j of
    one is the mate of record j of the other.  stats = {"read1": ..., "read2": ..., "pair": ...}: per side what filter_columns gives,
    and the pair plan's dict.  overlap=False: no search, the joint keep is keep1 & keep2, no min_length is applied again, and "pair"
    is absent.  profile=True: stats["read1"] and stats["read2"] get "profile_before" and "profile_after" as in filter_columns, the
    latter from that side's final ranges and the joint keep.
    merge=True (needs overlap=True): behind the pair plan, merge_pairs with the pair plan's ranges, keep and insert sizes, its
    min_overlap, max_mismatches and max_error_permille, and merge_quality_cap turns the kept pairs whose mates overlap into one read
    each; the two selects then take keep & ~merged -> (out1, out2, merged, stats): `merged` the RecordColumns of the merged reads,
    out1 / out2 the mates of the kept pairs that were not merged, stats["merge"] the dict of merge_pairs; merged.n_records +
    out1.n_records is the pair plan's pairs_kept, and "profile_after" is that of out1 / out2.
    dedup=True: behind the pair plan (overlap=False: on keep1 & keep2) and in front of the merge, dedup_plan(key_bases=dedup_key_bases,
    prefer=dedup_prefer) keyed on BOTH mates' final ranges leaves one pair of every set of exact duplicate pairs; stats["dedup"] is its
    dict, the pairs that come out -- merged ones included -- number stats["dedup"]["records_kept"], and "profile_after" reflects it.
    kmers=k (an int, 1 .. 31): stats gets "kmers_after", ONE KmerTable with the canonical k-mers of both sides under the final
    ranges and the final keep -- count_kmers(k) on read 1, then on read 2 into the same table; of the mates out1 / out2, so under
    merge=True without the merged reads.
    screen (a dict of kmer_plan keywords, its `table` among them): per side, behind that side's adapter plan and in front of the pair
    plan, kmer_plan narrows the side's plan against that table, with the filter's min_length unless the dict gives one; the pair plan
    (overlap=False: keep1 & keep2) then makes it a decision per PAIR -- a pair goes if either mate is screened out, as in BBDuk.
    stats["read1"]["screen"] and stats["read2"]["screen"] are its dicts.
    correct (as in filter_columns): per side, behind that side's adapter plan and in front of the screen and the pair plan, correct_kmers
    repairs the bases; with k= ONE table of both mates under their plans is counted first.  stats["read1"]["correct"] and
    stats["read2"]["correct"] are its dicts; everything behind it sees the repaired bases, "profile_before" the bases as they came.
    complexity (as in filter_columns): per side, behind that side's adapter plan and in front of correct, the screen and the pair plan --
    poly-G tails spoil the overlap search; stats["read1"]["complexity"] and stats["read2"]["complexity"] are its dicts.
    demux (a dict of demux_plan keywords, its `barcodes` among them): directly behind the two trim plans, demux_plan runs ONCE with read 1
    as its reads; slot sources are named "read1", "read2", "index1", "index2" (`index=` carries the index sets; a slot on read 2 makes
    read 2 one more index set, so at most one other beside it).  Its keep is ANDed into both sides, so every later plan sees it; with
    cut, a slot on read 2 advances begin2 of assigned pairs behind offset + length.  At the end out1, out2 and `merged` are each
    partitioned by the class of their source pair instead of selected: block_records is the class prefix of each.  stats["demux"]
    is the plan's dict plus "class_records", that of out1 and out2.  ValueError as in filter_columns."""
    if demux is not None:
        demux, read2_cut = _check_demux_pairs(demux, cols1, cols2, rules.get("quality_5", 0), dedup)
    if complexity is not None:
        _check_complexity(complexity)
    if dedup:
        _check_dedup_args(dedup_key_bases, dedup_prefer)
    if correct is not None:
        _check_correct(correct, cols1)
    if screen is not None:
        _check_screen(screen, cols1)
    if kmers is not None:
        _check_int("kmers", kmers, 1, _lib.KMER_MAX_K)
    _check_pair_args(cols1, cols2, pair_min_overlap, pair_max_mismatches, pair_max_error_permille, rules.get("min_length", 1))
    if merge:
        if not overlap:
            raise ValueError("merge=True needs overlap=True: the merge takes the insert sizes the overlap search finds")
        _check_int("merge_quality_cap", merge_quality_cap, 0, 255)
    plans, stats = [], {}
    codes1, codes2 = (_adapter_codes(a) if a is not None else None for a in (adapters1, adapters2))
    trimmed = [trim_plan(handle, cols, **rules) for cols in (cols1, cols2)]
    classes = None
    if demux is not None:
        (tb1, te1, tk1, side1), (tb2, te2, tk2, side2) = trimmed
        tb1, te1, tk1, classes, m_stats = demux_plan(handle, cols1, begin=tb1, end=te1, keep=tk1, **dict(dict(min_length=rules.get("min_length", 1)), **demux))
        n_classes = m_stats["class_counts"].numel() - (0 if demux.get("keep_unassigned", False) else 1)
        if read2_cut:                                        # (assigned: the barcode fits read 2 as it was stored)
            assigned = (classes >= 0) & (classes < m_stats["class_counts"].numel() - 1)
            tb2 = torch.where(assigned, torch.minimum(torch.maximum(tb2, cols2.seq_offsets[:-1] + read2_cut), te2), tb2)
        trimmed = [(tb1, te1, tk1, side1), (tb2, te2, tk2 & tk1, side2)]
        stats["demux"] = m_stats
    for (name, cols, codes), (begin, end, keep, side) in zip((("read1", cols1, codes1), ("read2", cols2, codes2)), trimmed):
        if codes is not None:
            begin, end, keep, a_stats = adapter_plan(handle, cols, codes, begin, end, keep, adapter_min_overlap, adapter_max_error_permille,
                                                     rules.get("min_length", 1))
            side = dict(side, adapter=a_stats)
        if complexity is not None:
            begin, end, keep, x_stats = complexity_plan(handle, cols, begin, end, keep,
                                                        **dict(dict(min_length=rules.get("min_length", 1)), **complexity))
            side = dict(side, complexity=x_stats)
        plans.append((begin, end, keep)); stats[name] = side
    came1, came2 = cols1, cols2
    if correct is not None:
        (cols1, c1_stats), (cols2, c2_stats) = _correct_step(handle, [(cols1,) + plans[0], (cols2,) + plans[1]], correct)
        stats["read1"] = dict(stats["read1"], correct=c1_stats); stats["read2"] = dict(stats["read2"], correct=c2_stats)
    if screen is not None:
        for i, (name, cols) in enumerate((("read1", cols1), ("read2", cols2))):
            begin, end, keep = plans[i]
            begin, end, keep, s_stats = kmer_plan(handle, cols, begin=begin, end=end, keep=keep,
                                                  **dict(dict(min_length=rules.get("min_length", 1)), **screen))
            plans[i] = (begin, end, keep); stats[name] = dict(stats[name], screen=s_stats)
    merged = None
    if merge:
        b1, e1, b2, e2, keep, p_stats, insert = pair_plan(handle, cols1, cols2, plans[0], plans[1], pair_min_overlap, pair_max_mismatches,
                                                          pair_max_error_permille, rules.get("min_length", 1), return_insert=True)
        stats["pair"] = p_stats
        if dedup:
            keep, stats["dedup"] = dedup_plan(handle, cols1, cols2, b1, e1, b2, e2, keep, dedup_key_bases, dedup_prefer)
        merged, flag, stats["merge"], m_source = merge_pairs(handle, cols1, cols2, b1, e1, b2, e2, keep, insert, pair_min_overlap, pair_max_mismatches,
                                                             pair_max_error_permille, merge_quality_cap, titles=titles, return_source=True)
        if classes is not None:
            merged = partition_columns(handle, merged, classes[m_source], n_classes, titles=titles)
        keep = keep & (flag ^ 1)                             # both hold 0 / 1
    elif overlap:
        b1, e1, b2, e2, keep, p_stats = pair_plan(handle, cols1, cols2, plans[0], plans[1], pair_min_overlap, pair_max_mismatches,
                                                  pair_max_error_permille, rules.get("min_length", 1))
        stats["pair"] = p_stats
    else:
        (b1, e1, k1), (b2, e2, k2) = plans
        keep = ((k1 != 0) & (k2 != 0)).to(torch.uint8)
    if dedup and not merge:
        keep, stats["dedup"] = dedup_plan(handle, cols1, cols2, b1, e1, b2, e2, keep, dedup_key_bases, dedup_prefer)
    if profile:
        for name, cols, came, b, e in (("read1", cols1, came1, b1, e1), ("read2", cols2, came2, b2, e2)):
            before = profile_columns(handle, came)
            stats[name] = dict(stats[name], profile_before=before, profile_after=profile_columns(handle, cols, b, e, keep, n_cycles=before.n_cycles))
    if kmers is not None:
        table, _ = count_kmers(handle, cols1, kmers, b1, e1, keep)
        stats["kmers_after"], _ = count_kmers(handle, cols2, kmers, b2, e2, keep, into=table)
    if classes is not None:
        out1 = partition_columns(handle, cols1, classes, n_classes, b1, e1, keep, titles=titles)
        out2 = partition_columns(handle, cols2, classes, n_classes, b2, e2, keep, titles=titles)
        stats["demux"] = dict(stats["demux"], class_records=out1.block_records.tolist())
    else:
        out1 = select_columns(handle, cols1, b1, e1, keep, titles=titles)
        out2 = select_columns(handle, cols2, b2, e2, keep, titles=titles)
    return (out1, out2, merged, stats) if merge else (out1, out2, stats)


# ---- k-mer count (dsrcgpu_columns_kmer_count and the three calls on its table) ---------------------------------------------------------
def _check_kmer_capacity(capacity):
    _check_int("capacity", capacity, 16, 1 << 40)
    if capacity & (capacity - 1):
        raise ValueError("capacity must be a power of two")


def pack_kmers(kmers, k: int):
    """Strings of k letters A C G T -> a list of packed forward words (first base most significant)."""
    out = []
    for s in kmers:
        if not isinstance(s, str) or len(s) != k or any(ch not in _BASE_CODES for ch in s.upper()):
            raise ValueError("a k-mer is a string of %d letters A C G T" % k)
        v = 0
        for ch in s.upper():
            v = (v << 2) | _BASE_CODES[ch]
        out.append(v)
    return out


def unpack_kmer(word: int, k: int) -> str:
    return "".join("ACGT"[(word >> (2 * (k - 1 - j))) & 3] for j in range(k))


@dataclasses.dataclass
class KmerTable:
    """A table of dsrcgpu_columns_kmer_count: one int64 tensor of _lib.kmer_words(capacity) words on the device of the columns
    (layout: include/dsrc_gpu.h; the EMPTY key reads as -1) and views of its parts.  Slot order is unspecified; items() is the
    table's content.  Nothing crosses to the host but by summary(), top() and the totals of spectrum()."""
    data: torch.Tensor
    k: int
    canonical: bool

    @property
    def capacity(self) -> int:
        return (self.data.numel() - 8) // 2

    @property
    def keys(self):
        return self.data[8: 8 + self.capacity]

    @property
    def counts(self):
        return self.data[8 + self.capacity:]

    @staticmethod
    def empty(handle: _lib.Handle, k: int, canonical: bool = True, capacity: int = 16, device="cpu") -> "KmerTable":
        """An initialised table without a key (a count over no records)."""
        _check_int("k", k, 1, _lib.KMER_MAX_K)
        _check_kmer_capacity(capacity)
        t = KmerTable(torch.empty(_lib.kmer_words(capacity), dtype=torch.int64, device=device), k, bool(canonical))
        _quiesce(t.data.device)
        handle.columns_kmer_count(_lib.ColumnsIn(), None, None, None, _lib.KmerRules(k, int(bool(canonical)), 0, 0, capacity), t.data.data_ptr())
        return t

    def summary(self) -> dict:
        """The header as a dict of ints -- the only part that crosses to the host."""
        h = self.data[:8].tolist()
        return dict(k=self.k, canonical=self.canonical, capacity=h[1], distinct=h[2], occurrences=h[3], overflow=h[4])

    def items(self):
        """-> (keys, counts) of the occupied slots, sorted by key: int64 tensors on the table's device."""
        keys, counts = self.keys, self.counts
        used = keys != -1
        keys, order = torch.sort(keys[used])
        return keys, counts[used][order]

    def top(self, n: int):
        """The n most frequent k-mers as a list of (string, count), the highest count first, equal counts by key."""
        _check_int("n", n, 0, 1 << 40)
        keys, counts = self.items()
        n = min(n, keys.numel())
        if n == 0:
            return []
        floor = torch.topk(counts, n).values[-1]
        cand = counts >= floor                               # every key that ties with the n-th is a candidate: the cut is by key, not by slot
        keys, counts = keys[cand], counts[cand]
        order = torch.sort(counts, descending=True, stable=True).indices[:n]
        return [(unpack_kmer(key, self.k), c) for key, c in zip(keys[order].tolist(), counts[order].tolist())]

    def spectrum(self, handle: _lib.Handle, n_bins: int = 256):
        """dsrcgpu_kmer_spectrum -> (hist, totals): hist[c] = the distinct keys counted c times (int64, n_bins, the last bin folds),
        totals a dict with the keys of _lib.KMER_SPECTRUM_TOTALS."""
        _check_int("n_bins", n_bins, 2, _lib.KMER_MAX_BINS)
        hist = torch.empty(n_bins, dtype=torch.int64, device=self.data.device)
        _quiesce(self.data.device)
        totals = handle.kmer_spectrum(self.data.data_ptr(), n_bins, hist.data_ptr())
        return hist, dict(zip(_lib.KMER_SPECTRUM_TOTALS, totals))

    def lookup(self, handle: _lib.Handle, kmers, return_invalid: bool = False):
        """dsrcgpu_kmer_lookup: the count of each k-mer -- strings of k letters, or an int64 tensor of packed forward words on the
        table's device -> int64 counts on that device, 0 for a key that is absent (with return_invalid: and the number of words of
        4^k and more).  Under a canonical table a k-mer and its reverse complement give the same count."""
        device = self.data.device
        if not isinstance(kmers, torch.Tensor):
            kmers = torch.tensor(pack_kmers(list(kmers), self.k), dtype=torch.int64, device=device)
        if kmers.dtype != torch.int64 or kmers.dim() != 1 or kmers.device != device:
            raise ValueError("kmers is a list of strings or a one-dimensional int64 tensor on the table's device")
        kmers = kmers.contiguous()
        out = torch.empty(kmers.numel(), dtype=torch.int64, device=device)
        _quiesce(device)
        invalid = handle.kmer_lookup(self.data.data_ptr(), kmers.data_ptr() if kmers.numel() else None, kmers.numel(),
                                     out.data_ptr() if kmers.numel() else None)
        return (out, invalid) if return_invalid else out

    def merged_into(self, handle: _lib.Handle, other: "KmerTable") -> "KmerTable":
        """dsrcgpu_kmer_table_merge: every (key, count) of this table is added into `other` (same k and canonical, any capacity),
        which is returned.  If `other` is too small it is grown first (its tensor is replaced)."""
        if not isinstance(other, KmerTable) or other.k != self.k or other.canonical != self.canonical or other.data.device != self.data.device:
            raise ValueError("both tables hold the same k and canonical on one device")
        if other.data.data_ptr() == self.data.data_ptr():
            raise ValueError("a table cannot be merged into itself")
        _quiesce(self.data.device)
        try:
            stats = handle.kmer_table_merge(self.data.data_ptr(), other.data.data_ptr())
        except _lib.DsrcGpuError as e:
            if e.code != _lib.E_CAPACITY:
                raise
            other.data = other.grown(handle, e.need).data
            stats = handle.kmer_table_merge(self.data.data_ptr(), other.data.data_ptr())
        if stats[3]:
            raise RuntimeError("k-mer merge: %d occurrences lost to overflow" % stats[3])
        return other

    def grown(self, handle: _lib.Handle, capacity: int) -> "KmerTable":
        """A new table of `capacity` slots with every (key, count) of this one."""
        new = KmerTable.empty(handle, self.k, self.canonical, capacity, self.data.device)
        return self.merged_into(handle, new)


def count_kmers(handle: _lib.Handle, cols: RecordColumns, k: int, begin=None, end=None, keep=None, canonical: bool = True, capacity=None,
                into=None):
    """dsrcgpu_columns_kmer_count on the records of `cols` under the plan begin / end / keep (None: whole reads, every record; as the
    planners return them) -> (KmerTable, stats), stats a dict with the keys of _lib.KMER_STATS.  Every window of k bases A C G T of a
    considered record's range counts once under its key: the lower of the forward word and its reverse complement (canonical=False:
    the forward word).  capacity=None: a first call sizes the table (a power of two of at least twice the windows); a capacity
    that is too small raises DsrcGpuError with .code == E_CAPACITY and .need.  into: an earlier KmerTable of the same k and
    canonical on the same device -- the counts are added to it and it is returned (the mates of a pair, the batches of a file); if
    it is too small it is grown to the size the library asks for (its tensor is replaced).  A non-zero overflow raises RuntimeError:
    with the full hash it is not expected.  Arguments out of range raise ValueError before the library is called.  Nothing of the
    payload crosses to the host."""
    device = cols.bases.device
    R = cols.n_records
    _check_int("k", k, 1, _lib.KMER_MAX_K)
    canonical = bool(canonical)
    if into is not None:
        if not isinstance(into, KmerTable) or into.k != k or into.canonical != canonical or capacity not in (None, into.capacity):
            raise ValueError("into is an earlier KmerTable with the same k and canonical")
        if into.data.dtype != torch.int64 or into.data.device != device or not into.data.is_contiguous() or into.data.numel() < _lib.kmer_words(16):
            raise ValueError("into holds int64 words on the device of the columns")
        capacity = into.capacity
    if capacity is not None:
        _check_kmer_capacity(capacity)
    plan, plan_held = _stage_plan(R, device, [(begin, end)], keep)
    cin, held = _columns_in(cols, titles=False)
    new_table = lambda M: KmerTable(torch.empty(_lib.kmer_words(M), dtype=torch.int64, device=device), k, canonical)
    sizing = into is None and capacity is None
    table = into if into is not None else new_table(16 if sizing else capacity)
    _quiesce(device)

    def call():
        return handle.columns_kmer_count(cin, *plan, _lib.KmerRules(k, int(canonical), 1 if into is not None else 0, 0, table.capacity),
                                         table.data.data_ptr())
    try:
        stats = call()
    except _lib.DsrcGpuError as e:
        if e.code != _lib.E_CAPACITY or not (sizing or into is not None):
            raise
        if into is not None:
            into.data = into.grown(handle, e.need).data
        else:
            table = new_table(e.need)
        stats = call()
    del held, plan_held
    stats = dict(zip(_lib.KMER_STATS, stats))
    if stats["overflow"]:
        raise RuntimeError("k-mer count: %d occurrences lost to overflow" % stats["overflow"])
    return table, stats


# ---- k-mer plan (dsrcgpu_columns_kmer_plan) --------------------------------------------------------------------------------------------
_CODE_ALPHABET = "ACGTNRWSKMDVHBYXU.-"


def columns_from_sequences(seqs, device="cpu") -> RecordColumns:
    """Strings over the code alphabet "ACGTNRWSKMDVHBYXU.-" (either case; any other byte becomes code 255) -> RecordColumns on `device`
    with zero qualities and no titles: a reference (adapters, PhiX, rRNA) that count_kmers takes without a FASTQ.  Pure torch."""
    if isinstance(seqs, (str, bytes, bytearray)) or not hasattr(seqs, "__iter__"):
        raise ValueError("seqs is a list of strings")
    seqs = list(seqs)
    if any(not isinstance(s, str) for s in seqs):
        raise ValueError("seqs is a list of strings")
    table = torch.full((256,), 255, dtype=torch.uint8)
    for code, ch in enumerate(_CODE_ALPHABET):
        table[ord(ch)] = code
        table[ord(ch.lower())] = code
    raw = [s.encode("latin-1", "replace") for s in seqs]
    text = torch.frombuffer(bytearray(b"".join(raw)), dtype=torch.uint8) if any(raw) else torch.empty(0, dtype=torch.uint8)
    bases = table[text.to(torch.int64)]
    offs = torch.zeros(len(raw) + 1, dtype=torch.int64)
    if raw:
        offs[1:] = torch.cumsum(torch.tensor([len(s) for s in raw], dtype=torch.int64), 0)
    device = torch.device(device)
    u8 = dict(dtype=torch.uint8, device=device); i64 = dict(dtype=torch.int64, device=device)
    return RecordColumns(bases.to(device), torch.zeros(bases.numel(), **u8), torch.empty(0, **u8), offs.to(device), torch.empty(0, **i64),
                         torch.tensor([0, len(raw)], **i64))


def _check_kmer_plan_args(min_count, min_hits, max_hits, min_hit_permille, max_hit_permille, min_median, max_median, trim, min_length):
    _check_int("min_count", min_count, 1, (1 << 64) - 1)
    _check_int("min_hits", min_hits, 0, 0xFFFFFFFE)
    _check_int("min_hit_permille", min_hit_permille, 0, 1000)
    _check_int("max_hit_permille", max_hit_permille, 0, 1000)
    _check_int("min_median", min_median, 0, _lib.KMER_PLAN_COUNT_CAP)
    _check_int("min_length", min_length, 0, 0xFFFFFFFF)
    if max_hits is not None:
        _check_int("max_hits", max_hits, 0, 0xFFFFFFFE)
    if max_median is not None:
        _check_int("max_median", max_median, 0, 0xFFFFFFFE)
    if not isinstance(trim, str) or trim not in _lib.KMER_PLAN_TRIM:
        raise ValueError("trim must be one of %s" % ", ".join(repr(k) for k in _lib.KMER_PLAN_TRIM))


def kmer_plan(handle: _lib.Handle, cols: RecordColumns, table, begin=None, end=None, keep=None, min_count: int = 1, min_hits: int = 0,
              max_hits=None, min_hit_permille: int = 0, max_hit_permille: int = 1000, min_median: int = 0, max_median=None, trim: str = "none",
              min_length: int = 1, return_counts: bool = False):
    """dsrcgpu_columns_kmer_plan on the records of `cols`: every window of k bases of a considered record's range (the plan begin / end
    / keep; None: whole reads, every record; as the planners return them) is looked up in `table`, a KmerTable of count_kmers on the
    device of the columns, which is only read -> (begin, end, keep, stats[, good, hits, median]) in fresh tensors.  A window HITS iff
    its k-mer's count is at least min_count; a window with a code other than A C G T never hits.  A record is kept iff it came in
    kept, min_hits <= hits <= max_hits, min_hit_permille <= 1000 * hits / windows <= max_hit_permille, min_median <= median <=
    max_median and at least min_length bases are left.  trim="first_miss": the range ends in front of the last base of the first
    window that does not hit (khmer's abundance trim, with the table of the batch itself and min_count=2, say); "first_hit": it ends in
    front of the first window that hits (BBDuk's ktrim=r against a table of adapters).  A contaminant screen is max_hits=0 against the
    table of count_kmers(columns_from_sequences(reference)).  The median (of the counts capped at 65535, the upper one of two) is taken
    only when a median bound or return_counts asks for it.  stats is a dict with the keys of _lib.KMER_PLAN_STATS; good, hits,
    median are int64, one per record.  Arguments out of range raise ValueError before the library is called.  Nothing of the payload
    crosses to the host."""
    _check_kmer_plan_args(min_count, min_hits, max_hits, min_hit_permille, max_hit_permille, min_median, max_median, trim, min_length)
    device = cols.bases.device
    R = cols.n_records
    if not isinstance(table, KmerTable) or table.data.dtype != torch.int64 or table.data.device != device or not table.data.is_contiguous() or \
            table.data.numel() < _lib.kmer_words(16):
        raise ValueError("table is a KmerTable on the device of the columns")
    plan, plan_held = _stage_plan(R, device, [(begin, end)], keep)
    want_median = bool(return_counts) or min_median != 0 or max_median is not None
    cin, held = _columns_in(cols, titles=False)
    i64 = dict(dtype=torch.int64, device=device)
    out_begin = torch.empty(R, **i64); out_end = torch.empty(R, **i64)
    out_keep = torch.empty(R, dtype=torch.uint8, device=device)
    good, hits, median = (torch.empty(R, **i64) for _ in range(3)) if return_counts else (None, None, None)
    rules = _lib.KmerPlanRules(min_count, min_hits, max_hits, min_hit_permille, max_hit_permille, min_median, max_median, _lib.KMER_PLAN_TRIM[trim],
                               min_length, int(want_median))
    _quiesce(device)
    stats = handle.columns_kmer_plan(cin, rules, table.data.data_ptr(), *plan, _adr(out_begin), _adr(out_end), _adr(out_keep),
                                     _adr(good), _adr(hits), _adr(median))
    del held, plan_held
    got = (out_begin, out_end, out_keep, dict(zip(_lib.KMER_PLAN_STATS, stats)))
    return got + (good, hits, median) if return_counts else got


def _check_screen(screen, cols):
    """The `screen` dict of filter_columns / filter_pairs: the keywords of kmer_plan, `table` among them."""
    allowed = ("table", "min_count", "min_hits", "max_hits", "min_hit_permille", "max_hit_permille", "min_median", "max_median", "trim", "min_length")
    if not isinstance(screen, dict) or "table" not in screen or any(key not in allowed for key in screen):
        raise ValueError("screen is a dict of kmer_plan keywords (%s) that holds a table" % ", ".join(allowed))
    table = screen["table"]
    if not isinstance(table, KmerTable) or table.data.device != cols.bases.device:
        raise ValueError("screen['table'] is a KmerTable on the device of the columns")
    kw = dict(min_count=1, min_hits=0, max_hits=None, min_hit_permille=0, max_hit_permille=1000, min_median=0, max_median=None, trim="none", min_length=1)
    kw.update({key: v for key, v in screen.items() if key != "table"})
    _check_kmer_plan_args(**kw)


# ---- k-mer correction (dsrcgpu_columns_kmer_correct) -----------------------------------------------------------------------------------
def _check_kmer_correct_args(min_count, max_quality):
    _check_int("min_count", min_count, 1, (1 << 64) - 1)
    if max_quality is not None:
        _check_int("max_quality", max_quality, 0, 255)


def correct_kmers(handle: _lib.Handle, cols: RecordColumns, table, begin=None, end=None, keep=None, min_count: int = 2, max_quality=None,
                  inplace: bool = False, return_fixed: bool = False):
    """dsrcgpu_columns_kmer_correct on the records of `cols`: isolated substitution errors, and codes other than A C G T, of a considered
    record's range (the plan begin / end / keep; None: whole reads, every record; as the planners return them) are repaired against
    `table`, a KmerTable of count_kmers on the device of the columns, which is only read -> (RecordColumns, stats[, fixed]).  A window
    of k bases is SOLID iff it holds A C G T only and its k-mer's count is at least min_count; an error shows as a run of up to k
    windows that are not solid, and the base they share is replaced where exactly ONE other base makes every one of them solid (the
    rule, and what it leaves alone: include/dsrc_gpu.h).  max_quality: a base of a higher quality is never replaced (None: any).
    The result shares every tensor of `cols` but bases; with inplace=True cols.bases itself is repaired and the result is `cols`.
    Qualities are not touched.  The usual table is that of the batch itself: count_kmers(handle, cols, 21), then min_count=3, say;
    the call is idempotent, and a second pass is count_kmers on the result and another call.  stats is a dict with the keys of
    _lib.KMER_CORRECT_STATS; fixed (int64) is the number of repairs per record.  Arguments out of range raise ValueError before the
    library is called.  Nothing of the payload crosses to the host."""
    _check_kmer_correct_args(min_count, max_quality)
    device = cols.bases.device
    R = cols.n_records
    if not isinstance(table, KmerTable) or table.data.dtype != torch.int64 or table.data.device != device or not table.data.is_contiguous() or \
            table.data.numel() < _lib.kmer_words(16):
        raise ValueError("table is a KmerTable on the device of the columns")
    if inplace and not cols.bases.is_contiguous():
        raise ValueError("inplace=True needs contiguous bases")
    plan, plan_held = _stage_plan(R, device, [(begin, end)], keep)
    cin, held = _columns_in(cols, titles=False)
    out = cols.bases if inplace else held[0].clone()         # (the bytes outside the records' span, if any, are the input's too)
    spare = torch.empty(8, dtype=torch.uint8, device=device)
    fixed = torch.empty(R, dtype=torch.int64, device=device) if return_fixed else None
    _quiesce(device)
    stats = handle.columns_kmer_correct(cin, _lib.KmerCorrectRules(min_count, max_quality), table.data.data_ptr(), *plan,
                                        cin.d_bases if inplace else out.data_ptr() if out.numel() else spare.data_ptr(), _adr(fixed))
    del held, plan_held
    got = (cols if inplace else dataclasses.replace(cols, bases=out), dict(zip(_lib.KMER_CORRECT_STATS, stats)))
    return got + (fixed,) if return_fixed else got


def _check_correct(correct, cols):
    """The `correct` dict of filter_columns / filter_pairs: the keywords min_count and max_quality of correct_kmers and either `table`
    or `k` (the batch is counted under the plan at that point first)."""
    allowed = ("table", "k", "min_count", "max_quality")
    if not isinstance(correct, dict) or ("table" in correct) == ("k" in correct) or any(key not in allowed for key in correct):
        raise ValueError("correct is a dict of correct_kmers keywords (%s) that holds a table or a k" % ", ".join(allowed))
    if "table" in correct:
        table = correct["table"]
        if not isinstance(table, KmerTable) or table.data.device != cols.bases.device:
            raise ValueError("correct['table'] is a KmerTable on the device of the columns")
    else:
        _check_int("k", correct["k"], 1, _lib.KMER_MAX_K)
    _check_kmer_correct_args(correct.get("min_count", 2), correct.get("max_quality"))


def _correct_step(handle, sides, correct):
    """The `correct` step of the filters: sides = [(cols, begin, end, keep)], one entry or the two mates -> [(repaired cols, stats)].
    With k= the sides are counted into ONE table under their plans first."""
    table = correct.get("table")
    if table is None:
        for cols, begin, end, keep in sides:
            table, _ = count_kmers(handle, cols, correct["k"], begin, end, keep, into=table)
    kw = {key: v for key, v in correct.items() if key in ("min_count", "max_quality")}
    return [correct_kmers(handle, cols, table, begin, end, keep, **kw) for cols, begin, end, keep in sides]


# ---- demultiplex (dsrcgpu_columns_demux_plan, dsrcgpu_columns_partition_device) --------------------------------------------------------
_COMPLEMENT = {0: 3, 1: 2, 2: 1, 3: 0}
_DEMUX_SOURCES = {"read": 0, "read1": 0, "index1": 1, "index2": 2}
_DEMUX_KEYS = ("barcodes", "index", "slots", "max_mismatches", "slot_max_mismatches", "min_delta", "cut", "keep_unassigned", "min_length", "revcomp",
               "counts")


def _demux_barcodes(barcodes, revcomp=None):
    """`barcodes` (one entry per sample: "ACGTAC", ("ACGTACGT", "TTGACCAA") or "ACGTACGT+TTGACCAA") -> a list of samples, each a list
    of one or two bytes of codes 0 .. 3.  ValueError for characters outside ACGT, ragged lengths within a slot, samples of different
    slot counts, duplicates and counts or lengths out of range."""
    if isinstance(barcodes, (str, bytes, bytearray)) or not hasattr(barcodes, "__len__"):
        raise ValueError("barcodes is a list with one barcode (a string over ACGT) or one pair of barcodes per sample")
    if not 1 <= len(barcodes) <= _lib.DEMUX_MAX_SAMPLES:
        raise ValueError("between 1 and %d samples are needed, %d given" % (_lib.DEMUX_MAX_SAMPLES, len(barcodes)))
    samples = []
    for entry in barcodes:
        parts = entry.split("+") if isinstance(entry, str) else list(entry) if isinstance(entry, (tuple, list)) else None
        if parts is None or not 1 <= len(parts) <= 2 or any(not isinstance(p, str) for p in parts):
            raise ValueError("barcode %r is neither a string over ACGT nor a pair of them" % (entry,))
        codes = []
        for p in parts:
            if any(ch not in _BASE_CODES for ch in p.upper()):
                raise ValueError("barcode %r: only A, C, G and T are allowed" % (entry,))
            if not 1 <= len(p) <= _lib.DEMUX_MAX_BARCODE:
                raise ValueError("a barcode has 1 to %d bases, %r has %d" % (_lib.DEMUX_MAX_BARCODE, entry, len(p)))
            codes.append([_BASE_CODES[ch] for ch in p.upper()])
        samples.append(codes)
    n_slots = len(samples[0])
    if any(len(s) != n_slots for s in samples):
        raise ValueError("every sample has the same number of barcodes")
    for s in range(n_slots):
        if any(len(sample[s]) != len(samples[0][s]) for sample in samples):
            raise ValueError("the barcodes of slot %d have different lengths" % s)
    if revcomp is not None:
        flags = [revcomp] * n_slots if isinstance(revcomp, bool) else list(revcomp)
        if len(flags) != n_slots or any(not isinstance(f, bool) for f in flags):
            raise ValueError("revcomp is a bool per slot")
        samples = [[[_COMPLEMENT[v] for v in reversed(b)] if f else b for b, f in zip(sample, flags)] for sample in samples]
    samples = [[bytes(b) for b in sample] for sample in samples]
    if len({tuple(sample) for sample in samples}) != len(samples):
        raise ValueError("two samples have the same barcodes")
    return samples


def _demux_slots(slots, n_slots, n_index, lens, names=_DEMUX_SOURCES):
    """`slots` (None, or per slot a (source, offset) pair; a source is 0 / "read", 1 / "index1", 2 / "index2") -> [(source, offset)]."""
    if slots is None:
        if n_index:
            if n_index != n_slots:
                raise ValueError("%d index read sets for barcodes of %d slots: say where each slot is read with slots=" % (n_index, n_slots))
            return [(k + 1, 0) for k in range(n_slots)]
        return [(0, sum(lens[:s])) for s in range(n_slots)]
    slots = list(slots)
    if len(slots) != n_slots:
        raise ValueError("slots has one (source, offset) pair per barcode slot: %d needed, %d given" % (n_slots, len(slots)))
    out = []
    for slot in slots:
        if not isinstance(slot, (tuple, list)) or len(slot) != 2:
            raise ValueError("a slot is a (source, offset) pair, %r given" % (slot,))
        source, offset = slot
        source = names.get(source, source) if isinstance(source, str) else source
        if not isinstance(source, int) or isinstance(source, bool) or not 0 <= source <= n_index:
            raise ValueError("slot source %r: 0 or 'read' for the reads, 1 .. %d or 'index1' .. for the index read sets given" % (slot[0], n_index))
        _check_int("slot offset", offset, 0, 0xFFFFFFFF - _lib.DEMUX_MAX_BARCODE)
        out.append((source, offset))
    return out


def _check_demux_args(cols, barcodes, index=(), slots=None, max_mismatches=1, slot_max_mismatches=None, min_delta=1, cut=True, keep_unassigned=False,
                      min_length=1, revcomp=None, counts=None):
    """The keywords of demux_plan, checked -> (_lib.DemuxRules, samples, slots).  ValueError for anything out of range."""
    samples = _demux_barcodes(barcodes, revcomp)
    index = list(index or ())
    if len(index) > 2 or any(not isinstance(x, RecordColumns) for x in index):
        raise ValueError("index is a list of at most two RecordColumns")
    if any(x.n_records != cols.n_records or x.bases.device != cols.bases.device for x in index):
        raise ValueError("an index read set has one record per read, on the device of the columns")
    lens = [len(b) for b in samples[0]]
    slots = _demux_slots(slots, len(lens), len(index), lens)
    _check_int("max_mismatches", max_mismatches, 0, sum(lens))
    if slot_max_mismatches is not None:
        slot_max_mismatches = list(slot_max_mismatches)
        if len(slot_max_mismatches) != len(lens):
            raise ValueError("slot_max_mismatches has one entry per barcode slot")
        for v in slot_max_mismatches:
            _check_int("slot_max_mismatches", v, 0, 0xFFFFFFFE)
    _check_int("min_delta", min_delta, 0, 255)
    _check_int("min_length", min_length, 0, 0xFFFFFFFF)
    if counts is not None and (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or counts.numel() != len(samples) + 1 or
                               counts.device != cols.bases.device or not counts.is_contiguous()):
        raise ValueError("counts holds %d int64 counts on the device of the columns" % (len(samples) + 1))
    rules = _lib.DemuxRules(samples, slots, max_mismatches, slot_max_mismatches, min_delta, int(bool(cut)), int(bool(keep_unassigned)), min_length)
    return rules, samples, slots


def demux_plan(handle: _lib.Handle, cols: RecordColumns, barcodes, begin=None, end=None, keep=None, index=(), slots=None, max_mismatches: int = 1,
               slot_max_mismatches=None, min_delta: int = 1, cut: bool = True, keep_unassigned: bool = False, min_length: int = 1,
               return_info: bool = False, counts=None, revcomp=None):
    """dsrcgpu_columns_demux_plan on the records of `cols`: every record that came in kept (the plan begin / end / keep; None: whole
    reads, every record) gets the sample whose barcodes lie nearest -> (begin, end, keep, classes, stats[, best, second, reason]) in
    fresh tensors.  `barcodes` has one entry per sample: "ACGTAC", a pair ("ACGTACGT", "TTGACCAA") or "ACGTACGT+TTGACCAA"; the
    barcodes of one slot have one length.  `slots` says where each slot is read, as (source, offset) pairs: source 0 / "read" = the
    record's own range, 1 / "index1" and 2 / "index2" = the RecordColumns in `index` (record r of which belongs to read r), offset = the
    bases in front of the barcode.  The default is inline at offset 0 (a second slot behind the first) when `index` is empty, else
    one slot per index set at offset 0.  revcomp=(False, True) reverse-complements the barcodes of a slot on the host (i5 on some
    instruments).  A record is assigned iff its best total distance is at most max_mismatches (and each slot's at most
    slot_max_mismatches[s], None: no limit per slot) and the runner-up lies at least min_delta above it; cut=True moves an assigned
    record's begin behind its inline barcodes; keep_unassigned=True keeps the others as class n_samples (bcl2fastq's
    "Undetermined").  classes (int32) is the sample, n_samples for unassigned, -1 for a record that came in dropped; stats is a
    dict with the keys of _lib.DEMUX_STATS plus "class_counts", the int64 tensor `counts` (n_samples + 1 entries, created as zeros
    when None, ADDED to, so that the batches of a file sum).  best, second (int64; 255 = none) and reason (int64: index into
    _lib.DEMUX_REASONS) are -1 for a record that came in dropped.  Duplicate barcodes, characters outside ACGT, ragged lengths within
    a slot and arguments out of range raise ValueError before the library is called.  Nothing of the payload crosses to the host."""
    rules, samples, _ = _check_demux_args(cols, barcodes, index, slots, max_mismatches, slot_max_mismatches, min_delta, cut, keep_unassigned,
                                          min_length, revcomp, counts)
    device = cols.bases.device
    R = cols.n_records
    plan, plan_held = _stage_plan(R, device, [(begin, end)], keep)
    cin, held = _columns_in(cols, titles=False)
    sets = [_columns_in(x, titles=False) for x in (index or ())]
    i64 = dict(dtype=torch.int64, device=device)
    out_begin = torch.empty(R, **i64); out_end = torch.empty(R, **i64)
    out_keep = torch.empty(R, dtype=torch.uint8, device=device)
    classes = torch.empty(R, dtype=torch.int32, device=device)
    info = torch.empty(R, dtype=torch.int32, device=device) if return_info else None
    if counts is None:
        counts = torch.zeros(len(samples) + 1, **i64)
    _quiesce(device)
    stats = handle.columns_demux_plan(cin, [s[0] for s in sets], rules, *plan, _adr(out_begin), _adr(out_end), _adr(out_keep), _adr(classes),
                                      _adr(info), counts.data_ptr())
    del held, plan_held, sets
    got = (out_begin, out_end, out_keep, classes, dict(dict(zip(_lib.DEMUX_STATS, stats)), class_counts=counts))
    if not return_info:
        return got
    word = info.to(torch.int64)
    dropped = word == -1
    field = lambda v: torch.where(dropped, torch.full_like(v, -1), v)
    return got + (field(word & 255), field((word >> 8) & 255), field((word >> 16) & 255))


def partition_columns(handle: _lib.Handle, cols: RecordColumns, classes, n_classes: int, begin=None, end=None, keep=None, titles: bool = True,
                      return_source: bool = False):
    """dsrcgpu_columns_partition_device: select_columns that groups -- the records of `cols` with a non-zero `keep` entry (None: all)
    and 0 <= classes[r] < n_classes come out class by class, in input order inside a class, cut to [begin[r], end[r]) (None: whole
    reads) -> RecordColumns whose block_records is the class prefix (n_classes + 1 entries): class c is records block_records[c] ..
    block_records[c + 1] - 1, class_view(parts, c) hands them out without a copy, and encode_columns(parts) writes one block per
    non-empty class when given block_records without the repeats.  classes is an integer tensor with one entry per record, as
    demux_plan returns it; return_source=True: -> (RecordColumns, source), source[j] = the index in `cols` of output record j.  The
    order is the same on every run."""
    _check_int("n_classes", n_classes, 1, _lib.PARTITION_MAX_CLASSES)
    device = cols.bases.device
    R = cols.n_records
    _together((begin, end))
    if not isinstance(classes, torch.Tensor) or classes.is_floating_point() or classes.numel() != R or classes.device != device:
        raise ValueError("classes is an integer tensor with one entry per record, on the device of the columns")
    classes = classes.to(torch.int32).contiguous()
    cin, held = _columns_in(cols, titles)
    plan, plan_held = _stage_plan(R, device, [(begin, end)], keep)
    spare = held[-1]
    d_class = classes.data_ptr() if R else spare.data_ptr()
    _quiesce(device)
    need = [0, 0, 0]
    try:
        handle.columns_partition_device(cin, *plan, d_class, n_classes, _lib.Columns(d_titles=spare.data_ptr() if titles else None))
    except _lib.DsrcGpuError as e:
        if e.code != _lib.E_CAPACITY:
            raise
        need = e.need
    K, S, T = need
    u8 = dict(dtype=torch.uint8, device=device); i64 = dict(dtype=torch.int64, device=device)
    bases = torch.empty(S, **u8); quals = torch.empty(S, **u8)
    seq_offsets = torch.empty(K + 1, **i64)
    title_bytes = torch.empty(T if titles else 0, **u8)
    title_offsets = torch.empty(K + 1 if titles else 0, **i64)
    source = torch.empty(K, **i64)
    ptr = lambda t: t.data_ptr() if t.numel() else spare.data_ptr()
    out = _lib.Columns(ptr(bases), S, ptr(quals), S, ptr(title_bytes) if titles else None, T if titles else 0,
                       seq_offsets.data_ptr(), title_offsets.data_ptr() if titles else None, K)
    _quiesce(device)
    totals, class_records = handle.columns_partition_device(cin, *plan, d_class, n_classes, out, _adr(source) if return_source else None)
    assert totals[:3] == need
    del held, plan_held
    got = RecordColumns(bases, quals, title_bytes, seq_offsets, title_offsets, torch.tensor(class_records, **i64))
    return (got, source) if return_source else got


def class_view(parts: RecordColumns, c: int) -> RecordColumns:
    """Class c of what partition_columns returned, without a copy: bases, quals and titles are shared, the two offset arrays are
    slices (they do not start at 0, which every call here and encode_columns accept), block_records = [0, the class's records]."""
    _check_int("c", c, 0, parts.block_records.numel() - 2)
    lo, hi = (int(v) for v in parts.block_records[c: c + 2].tolist())
    titled = parts.title_offsets.numel() == parts.n_records + 1
    return RecordColumns(parts.bases, parts.quals, parts.titles, parts.seq_offsets[lo: hi + 1],
                         parts.title_offsets[lo: hi + 1] if titled else parts.title_offsets,
                         torch.tensor([0, hi - lo], dtype=torch.int64, device=parts.seq_offsets.device))


def demux_columns(handle: _lib.Handle, cols: RecordColumns, barcodes, titles: bool = True, return_source: bool = False, **kw):
    """demux_plan(**kw), then partition_columns with its plan and classes: -> (parts, stats[, source]).  parts.block_records is the
    prefix over n_classes = n_samples + (1 if keep_unassigned else 0) classes, stats the plan's dict plus "class_records", that
    prefix as a list."""
    begin, end, keep, classes, stats = demux_plan(handle, cols, barcodes, **dict(kw, return_info=False))
    n_classes = stats["class_counts"].numel() - (0 if kw.get("keep_unassigned", False) else 1)
    got = partition_columns(handle, cols, classes, n_classes, begin, end, keep, titles=titles, return_source=return_source)
    parts = got[0] if return_source else got
    stats = dict(stats, class_records=parts.block_records.tolist())
    return (parts, stats, got[1]) if return_source else (parts, stats)


def _check_demux(demux, cols, quality_5, dedup, pairs=False):
    """The `demux` dict of filter_columns / filter_pairs: the keywords of demux_plan, `barcodes` among them."""
    if not isinstance(demux, dict) or "barcodes" not in demux or any(key not in _DEMUX_KEYS for key in demux):
        raise ValueError("demux is a dict of demux_plan keywords (%s) that holds barcodes" % ", ".join(_DEMUX_KEYS))
    if dedup:
        raise ValueError("dedup=True together with demux: duplicates are per sample -- dedup the class views")
    kw = dict(demux)
    if pairs:
        return kw
    _, _, slots = _check_demux_args(cols, **kw)
    if quality_5 and any(source == 0 for source, _ in slots):
        raise ValueError("an inline barcode slot together with quality_5: the 5' trim would eat the barcode")
    return kw


def _check_demux_pairs(demux, cols1, cols2, quality_5, dedup):
    """The `demux` dict of filter_pairs -> (the keywords for demux_plan on read 1, the advance of begin2 under cut or 0).  A slot on
    "read2" turns read 2 into one more index set."""
    kw = _check_demux(demux, cols1, quality_5, dedup, pairs=True)
    index = list(kw.get("index", None) or ())
    slots = kw.get("slots")
    read2, n_index = [], len(index)
    if slots is not None:
        slots = [tuple(s) if isinstance(s, (tuple, list)) else s for s in slots]
        if any(isinstance(s, tuple) and len(s) == 2 and s[0] == "read2" for s in slots):
            if len(index) >= 2:
                raise ValueError("a slot on read 2 takes the place of an index read set: at most one other beside it")
            index = index + [cols2]
            read2 = [i for i, s in enumerate(slots) if isinstance(s, tuple) and len(s) == 2 and s[0] == "read2"]
            slots = [(len(index), s[1]) if i in read2 else s for i, s in enumerate(slots)]
    kw = dict(kw, index=index, slots=slots)
    _, samples, checked = _check_demux_args(cols1, **kw)
    inline = any(source == 0 for source, _ in checked) or bool(read2)
    if quality_5 and inline:
        raise ValueError("an inline barcode slot together with quality_5: the 5' trim would eat the barcode")
    advance = max([checked[i][1] + len(samples[0][i]) for i in read2], default=0)
    return kw, advance if kw.get("cut", True) else 0
