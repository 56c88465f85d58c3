"""ctypes binding of libdsrc_gpu.so (include/dsrc_gpu.h).

The product path has exactly one implementation -- the HIP library.  If it has not been built, or
there is no GPU, loading / creating a handle fails loudly; nothing here falls back to a CPU codec.

``DSRC_GPU_LIB`` may point at another build of the same C ABI (the test-suite uses it to load the
emulator build under tests/emu for kernel-logic tests on GPU-less machines).
"""
from __future__ import annotations

import ctypes as C
import os
import typing

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "csrc", "libdsrc_gpu.so")

EXPORTS = [
    "dsrcgpu_create", "dsrcgpu_destroy", "dsrcgpu_last_error", "dsrcgpu_compress_block", "dsrcgpu_compress_batch",
    "dsrcgpu_compress_batch_device", "dsrcgpu_submit", "dsrcgpu_flush", "dsrcgpu_collect", "dsrcgpu_release",
    "dsrcgpu_last_timing", "dsrcgpu_synth_illumina", "dsrcgpu_dev_alloc", "dsrcgpu_dev_free", "dsrcgpu_dev_upload",
    "dsrcgpu_dev_download", "dsrcgpu_chain_create", "dsrcgpu_chain_destroy", "dsrcgpu_set_chain", "dsrcgpu_host_alloc",
    "dsrcgpu_host_free", "dsrcgpu_selftest", "dsrcgpu_set_record_layout",
    "dsrcgpu_decompress_block", "dsrcgpu_decompress_batch", "dsrcgpu_decompress_batch_device",
    "dsrcgpu_title_fields", "dsrcgpu_fields_capacity_after", "dsrcgpu_set_fields_capacity", "dsrcgpu_get_fields_capacity",
    "dsrcgpu_chain_seed", "dsrcgpu_last_stage_timing", "dsrcgpu_try_collect", "dsrcgpu_prepare", "dsrcgpu_set_table_budget", "dsrcgpu_device_memory", "dsrcgpu_release_memory",
    "dsrcgpu_synth_fastq", "dsrcgpu_reserve_memory", "dsrcgpu_set_lanes", "dsrcgpu_submit_pinned",
    "dsrcgpu_decompress_batch_columns_device", "dsrcgpu_compress_columns_device", "dsrcgpu_columns_cut",
    "dsrcgpu_columns_trim_plan", "dsrcgpu_columns_select_device", "dsrcgpu_columns_adapter_plan", "dsrcgpu_columns_pair_plan",
    "dsrcgpu_columns_profile", "dsrcgpu_columns_merge_device", "dsrcgpu_columns_dedup_plan",
    "dsrcgpu_columns_kmer_count", "dsrcgpu_kmer_table_merge", "dsrcgpu_kmer_spectrum", "dsrcgpu_kmer_lookup",
    "dsrcgpu_columns_kmer_plan", "dsrcgpu_columns_kmer_correct", "dsrcgpu_columns_complexity_plan",
    "dsrcgpu_columns_demux_plan", "dsrcgpu_columns_partition_device",
]

# error codes of include/dsrc_gpu.h that callers tell apart (DsrcGpuError.code)
E_ARG = -1
E_CAPACITY = -4
E_INPUT = -5


# flavours of dsrcgpu_synth_fastq (include/dsrc_gpu.h)
SYNTH_ILLUMINA = 0
SYNTH_ILLUMINA_BINNED = 1
SYNTH_IONTORRENT = 2


class Settings(C.Structure):
    _fields_ = [("dna_order", C.c_uint32), ("quality_order", C.c_uint32), ("tag_preserve_flags", C.c_uint64),
                ("lossy", C.c_uint8), ("calculate_crc32", C.c_uint8), ("verify_after_compress", C.c_uint8),
                ("reserved", C.c_uint8 * 5)]


class Dataset(C.Structure):
    _fields_ = [("quality_offset", C.c_uint32), ("plus_repetition", C.c_uint8), ("color_space", C.c_uint8),
                ("reserved", C.c_uint8 * 2)]


class Columns(C.Structure):
    """dsrcgpu_columns: the caller's device arrays of dsrcgpu_decompress_batch_columns_device."""
    _fields_ = [("d_bases", C.c_void_p), ("bases_cap", C.c_uint64), ("d_quals", C.c_void_p), ("quals_cap", C.c_uint64),
                ("d_titles", C.c_void_p), ("titles_cap", C.c_uint64), ("d_seq_offs", C.c_void_p), ("d_title_offs", C.c_void_p),
                ("records_cap", C.c_uint64)]


class ColumnsIn(C.Structure):
    """dsrcgpu_columns_in: the caller's device arrays of dsrcgpu_compress_columns_device / dsrcgpu_columns_cut (read only)."""
    _fields_ = [("d_bases", C.c_void_p), ("bases_len", C.c_uint64), ("d_quals", C.c_void_p), ("d_titles", C.c_void_p),
                ("titles_len", C.c_uint64), ("d_seq_offs", C.c_void_p), ("d_title_offs", C.c_void_p), ("n_records", C.c_uint64)]


class TrimRules(C.Structure):
    """dsrcgpu_trim_rules: cutoffs of the running-sum trim (0 = that end is not trimmed) and the keep rules of
    dsrcgpu_columns_trim_plan (max_n 0xFFFFFFFF = no limit, min_mean_quality 0 = off)."""
    _fields_ = [("quality_5", C.c_uint32), ("quality_3", C.c_uint32), ("min_length", C.c_uint32), ("max_n", C.c_uint32),
                ("min_mean_quality", C.c_uint32), ("reserved", C.c_uint32 * 3)]


TRIM_STATS = ("records_kept", "bases_kept", "bases_cut", "dropped_length", "dropped_n", "dropped_mean_quality")


class AdapterRules(C.Structure):
    """dsrcgpu_adapter_rules: up to 8 adapters of 1 .. 64 base codes 0 .. 3 and the figures of dsrcgpu_columns_adapter_plan.
    AdapterRules(adapters, min_overlap, max_error_permille, min_length): `adapters` is a list of bytes / sequences of codes.  Lists
    too long to fit are cut to what fits with their count and lengths kept, so that the library is the one that refuses them."""
    _fields_ = [("n_adapters", C.c_uint32), ("adapter_len", C.c_uint32 * 8), ("adapters", (C.c_uint8 * 64) * 8), ("min_overlap", C.c_uint32),
                ("max_error_permille", C.c_uint32), ("min_length", C.c_uint32), ("reserved", C.c_uint32 * 3)]

    def __init__(self, adapters=(), min_overlap=3, max_error_permille=100, min_length=1, reserved=(0, 0, 0)):
        super().__init__()
        adapters = [bytes(bytearray(a)) for a in adapters]
        self.n_adapters = len(adapters)
        for i, a in enumerate(adapters[:8]):
            self.adapter_len[i] = len(a)
            for j, code in enumerate(a[:64]):
                self.adapters[i][j] = code
        self.min_overlap, self.max_error_permille, self.min_length = min_overlap, max_error_permille, min_length
        self.reserved = (C.c_uint32 * 3)(*reserved)


ADAPTER_STATS = ("records_kept", "bases_kept", "bases_cut", "records_trimmed", "dropped_length") + tuple("found_%d" % a for a in range(8))
NO_ADAPTER = 0xFFFFFFFF          # d_which of a record in which none was found


class ComplexityRules(C.Structure):
    """dsrcgpu_complexity_rules: the figures of dsrcgpu_columns_complexity_plan.  ComplexityRules(tail_bases, head_bases,
    poly_min_length, poly_max_error_permille, min_length, min_complexity_permille, max_dust, max_dust_windows): the masks hold bit X
    for base X (A = 1, C = 2, G = 4, T = 8), max_dust 0xFFFFFFFF = off; the library is the one that refuses figures out of range."""
    _fields_ = [("tail_bases", C.c_uint32), ("head_bases", C.c_uint32), ("poly_min_length", C.c_uint32), ("poly_max_error_permille", C.c_uint32),
                ("min_length", C.c_uint32), ("min_complexity_permille", C.c_uint32), ("max_dust", C.c_uint32), ("max_dust_windows", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]

    def __init__(self, tail_bases=0, head_bases=0, poly_min_length=10, poly_max_error_permille=125, min_length=1, min_complexity_permille=0,
                 max_dust=0xFFFFFFFF, max_dust_windows=0, reserved=(0, 0, 0, 0)):
        super().__init__()
        self.tail_bases, self.head_bases, self.poly_min_length, self.poly_max_error_permille = tail_bases, head_bases, poly_min_length, poly_max_error_permille
        self.min_length, self.min_complexity_permille, self.max_dust, self.max_dust_windows = min_length, min_complexity_permille, max_dust, max_dust_windows
        self.reserved = (C.c_uint32 * 4)(*reserved)


COMPLEXITY_STATS = ("records_kept", "bases_kept", "bases_cut_5", "bases_cut_3", "records_head_cut", "records_tail_cut") + \
    tuple("tail_" + x for x in "ACGT") + tuple("head_" + x for x in "ACGT") + ("dropped_length", "dropped_complexity", "dropped_dust")
COMPLEXITY_NONE = 255            # DSRCGPU_COMPLEXITY_NONE: the head / tail base of a record without a cut at that end


class DemuxRules(C.Structure):
    """dsrcgpu_demux_rules: DemuxRules(barcodes, slots, max_mismatches, slot_max_mismatches, min_delta, cut, keep_unassigned,
    min_length).  `barcodes` is a list with one entry per sample, each a list of one or two barcodes (bytes / sequences of codes
    0 .. 3), one per slot; `slots` a list of (source, offset) pairs, one per slot: source 0 = the reads themselves, 1 / 2 = an index
    read set.  The slot lengths are those of sample 0; slot_max_mismatches None = no limit per slot.  The library is the one that
    refuses figures out of range (shorter barcodes of later samples are padded with code 255, which it refuses)."""
    _fields_ = [("n_samples", C.c_uint32), ("n_slots", C.c_uint32), ("slot_source", C.c_uint32 * 2), ("slot_offset", C.c_uint32 * 2),
                ("slot_len", C.c_uint32 * 2), ("slot_max_mismatches", C.c_uint32 * 2), ("max_mismatches", C.c_uint32), ("min_delta", C.c_uint32),
                ("cut", C.c_uint32), ("keep_unassigned", C.c_uint32), ("min_length", C.c_uint32), ("barcodes", C.c_void_p),
                ("reserved", C.c_uint32 * 3)]

    def __init__(self, barcodes=(), slots=((0, 0),), max_mismatches=1, slot_max_mismatches=None, min_delta=1, cut=1, keep_unassigned=0,
                 min_length=1, reserved=(0, 0, 0)):
        super().__init__()
        samples = [[bytes(bytearray(b)) for b in sample] for sample in barcodes]
        self.n_samples, self.n_slots = len(samples), len(slots)
        lens = [len(b) for b in samples[0][:2]] if samples else []
        for s, (source, offset) in enumerate(list(slots)[:2]):
            self.slot_source[s], self.slot_offset[s] = source, offset
            self.slot_len[s] = lens[s] if s < len(lens) else 0
            self.slot_max_mismatches[s] = DEMUX_NO_LIMIT if slot_max_mismatches is None else slot_max_mismatches[s]
        packed = bytearray()
        for sample in samples:
            for s, n in enumerate(lens):
                b = sample[s] if s < len(sample) else b""
                packed += (b + b"\xff" * n)[:n]
        self._codes = (C.c_uint8 * max(len(packed), 1))(*packed)          # (kept alive with the rules)
        self.barcodes = C.cast(self._codes, C.c_void_p)
        self.max_mismatches, self.min_delta, self.cut, self.keep_unassigned, self.min_length = max_mismatches, min_delta, cut, keep_unassigned, min_length
        self.reserved = (C.c_uint32 * 3)(*reserved)


DEMUX_MAX_SAMPLES = 1023         # DSRCGPU_DEMUX_MAX_SAMPLES
DEMUX_MAX_BARCODE = 64           # DSRCGPU_DEMUX_MAX_BARCODE
DEMUX_NO_LIMIT = 0xFFFFFFFF      # DSRCGPU_DEMUX_NO_LIMIT
DEMUX_STATS = ("records_kept", "bases_kept", "bases_cut", "records_assigned", "assigned_perfect", "unassigned_short", "unassigned_no_match",
               "unassigned_ambiguous", "dropped_length")
DEMUX_REASONS = ("assigned", "short", "no_match", "ambiguous")
PARTITION_MAX_CLASSES = 1024


class PairRules(C.Structure):
    """dsrcgpu_pair_rules: the figures of dsrcgpu_columns_pair_plan.  PairRules(min_overlap, max_mismatches, max_error_permille,
    min_length); the library is the one that refuses figures out of range."""
    _fields_ = [("min_overlap", C.c_uint32), ("max_mismatches", C.c_uint32), ("max_error_permille", C.c_uint32), ("min_length", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]

    def __init__(self, min_overlap=30, max_mismatches=5, max_error_permille=200, min_length=1, reserved=(0, 0, 0, 0)):
        super().__init__()
        self.min_overlap, self.max_mismatches, self.max_error_permille, self.min_length = min_overlap, max_mismatches, max_error_permille, min_length
        self.reserved = (C.c_uint32 * 4)(*reserved)


PAIR_MAX_BASES = 1024            # DSRCGPU_PAIR_MAX_BASES: a pair with a longer range is not searched
PAIR_STATS = ("pairs_kept", "bases_kept_1", "bases_kept_2", "bases_cut_1", "bases_cut_2", "overlap_found", "overlap_narrowed", "dropped_mate",
              "dropped_length", "not_searched_long", "insert_sum")
NO_INSERT = 0xFFFFFFFFFFFFFFFF   # d_insert of a pair in which no overlap was found


class MergeRules(C.Structure):
    """dsrcgpu_merge_rules: the figures of dsrcgpu_columns_merge_device.  MergeRules(min_overlap, max_mismatches, max_error_permille,
    quality_cap); the library is the one that refuses figures out of range."""
    _fields_ = [("min_overlap", C.c_uint32), ("max_mismatches", C.c_uint32), ("max_error_permille", C.c_uint32), ("quality_cap", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]

    def __init__(self, min_overlap=30, max_mismatches=5, max_error_permille=200, quality_cap=41, reserved=(0, 0, 0, 0)):
        super().__init__()
        self.min_overlap, self.max_mismatches, self.max_error_permille, self.quality_cap = min_overlap, max_mismatches, max_error_permille, quality_cap
        self.reserved = (C.c_uint32 * 4)(*reserved)


MERGE_STATS = ("pairs_merged", "bases_written", "overlap_sum", "overlap_agree", "overlap_corrected", "overlap_one_sided", "overlap_neither",
               "not_kept", "no_insert", "bad_geometry", "short_overlap", "over_budget")


class DedupRules(C.Structure):
    """dsrcgpu_dedup_rules: DedupRules(key_bases, prefer, hash_bits): key_bases 0 = the whole range; prefer 0 = the first record of a
    class survives, 1 = the one with the highest quality sum; hash_bits is a diagnostic (0 or 64: the full hash) on which no result
    depends.  The library is the one that refuses figures out of range."""
    _fields_ = [("key_bases", C.c_uint32), ("prefer", C.c_uint32), ("hash_bits", C.c_uint32), ("reserved", C.c_uint32 * 5)]

    def __init__(self, key_bases=0, prefer=0, hash_bits=0, reserved=(0, 0, 0, 0, 0)):
        super().__init__()
        self.key_bases, self.prefer, self.hash_bits = key_bases, prefer, hash_bits
        self.reserved = (C.c_uint32 * 5)(*reserved)


DEDUP_PREFER = {"first": 0, "quality": 1}
DEDUP_STATS = ("records_considered", "records_kept", "records_dropped", "classes_multiple", "largest_class", "came_in_dropped", "empty_keys",
               "representative_not_first") + tuple("level_" + b for b in ("1", "2", "3", "4", "5", "6", "7", "8", "9", "10_49", "50_99", "100_499", "500_999",
                                                                           "1000_4999", "5000_9999", "10000_up"))
NO_DUP_OF = 0xFFFFFFFFFFFFFFFF   # d_dup_of of a record that came in dropped


class ProfileRules(C.Structure):
    """dsrcgpu_profile_rules: ProfileRules(n_cycles, accumulate); the library is the one that refuses figures out of range."""
    _fields_ = [("n_cycles", C.c_uint32), ("accumulate", C.c_uint32), ("reserved", C.c_uint32 * 6)]

    def __init__(self, n_cycles=1, accumulate=0, reserved=(0, 0, 0, 0, 0, 0)):
        super().__init__()
        self.n_cycles, self.accumulate = n_cycles, accumulate
        self.reserved = (C.c_uint32 * 6)(*reserved)


PROFILE_MAX_CYCLES = 1024        # DSRCGPU_PROFILE_MAX_CYCLES
PROFILE_TOTALS = ("records", "bases", "bases_q20", "bases_q30", "quality_sum", "gc_bases", "other_bases", "empty_records")


def profile_words(n_cycles: int) -> int:
    """DSRCGPU_PROFILE_WORDS: the uint64 words of a profile of n_cycles cycles."""
    return 11 * n_cycles + 622


class KmerRules(C.Structure):
    """dsrcgpu_kmer_rules: KmerRules(k, canonical, accumulate, hash_bits, capacity); hash_bits is a diagnostic (0 or 64: the full
    hash).  The library is the one that refuses figures out of range."""
    _fields_ = [("k", C.c_uint32), ("canonical", C.c_uint32), ("accumulate", C.c_uint32), ("hash_bits", C.c_uint32), ("capacity", C.c_uint64),
                ("reserved", C.c_uint32 * 4)]

    def __init__(self, k=21, canonical=1, accumulate=0, hash_bits=0, capacity=16, reserved=(0, 0, 0, 0)):
        super().__init__()
        self.k, self.canonical, self.accumulate, self.hash_bits, self.capacity = k, canonical, accumulate, hash_bits, capacity
        self.reserved = (C.c_uint32 * 4)(*reserved)


KMER_MAX_K = 31                  # DSRCGPU_KMER_MAX_K
KMER_PROBE_LIMIT = 1024          # DSRCGPU_KMER_PROBE_LIMIT
KMER_MAX_BINS = 65536            # DSRCGPU_KMER_MAX_BINS
KMER_EMPTY = 0xFFFFFFFFFFFFFFFF  # the key word of a free slot
KMER_STATS = ("records_considered", "records_came_dropped", "records_short", "windows", "kmers_counted", "windows_broken", "kmers_new", "overflow",
              "distinct_after", "total_after")
KMER_MERGE_STATS = ("keys_merged", "keys_new", "occurrences_added", "overflow", "distinct_after", "total_after")
KMER_SPECTRUM_TOTALS = ("distinct", "occurrences", "singletons", "largest_count")


def kmer_words(capacity: int) -> int:
    """DSRCGPU_KMER_WORDS: the uint64 words of a k-mer table of `capacity` slots."""
    return 8 + 2 * capacity


class KmerPlanRules(C.Structure):
    """dsrcgpu_kmer_plan_rules: KmerPlanRules(min_count, min_hits, max_hits, min_hit_permille, max_hit_permille, min_median, max_median,
    trim, min_length, want_median); max_hits / max_median None = no upper limit.  The library is the one that refuses figures out of
    range."""
    _fields_ = [("min_count", C.c_uint64), ("min_hits", C.c_uint32), ("max_hits", C.c_uint32), ("min_hit_permille", C.c_uint32),
                ("max_hit_permille", C.c_uint32), ("min_median", C.c_uint32), ("max_median", C.c_uint32), ("trim", C.c_uint32),
                ("min_length", C.c_uint32), ("want_median", C.c_uint32), ("reserved", C.c_uint32 * 4)]

    def __init__(self, min_count=1, min_hits=0, max_hits=None, min_hit_permille=0, max_hit_permille=1000, min_median=0, max_median=None, trim=0,
                 min_length=1, want_median=0, reserved=(0, 0, 0, 0)):
        super().__init__()
        self.min_count, self.min_hits, self.max_hits = min_count, min_hits, KMER_PLAN_NO_LIMIT if max_hits is None else max_hits
        self.min_hit_permille, self.max_hit_permille = min_hit_permille, max_hit_permille
        self.min_median, self.max_median = min_median, KMER_PLAN_NO_LIMIT if max_median is None else max_median
        self.trim, self.min_length, self.want_median = trim, min_length, want_median
        self.reserved = (C.c_uint32 * 4)(*reserved)


KMER_PLAN_NO_LIMIT = 0xFFFFFFFF  # max_hits / max_median: no upper limit
KMER_PLAN_COUNT_CAP = 65535      # DSRCGPU_KMER_PLAN_COUNT_CAP: the median is that of the counts capped here
KMER_PLAN_LDS_WINDOWS = 1024     # DSRCGPU_KMER_PLAN_LDS_WINDOWS: longer ranges keep their counts in HBM scratch under want_median
KMER_PLAN_TRIM = {"none": 0, "first_miss": 1, "first_hit": 2}
KMER_PLAN_STATS = ("records_considered", "records_came_dropped", "records_no_window", "windows", "windows_good", "hits", "records_kept",
                   "records_with_hit", "records_trimmed", "bases_cut", "dropped_hits", "dropped_hit_share", "dropped_median", "dropped_length",
                   "bases_kept")


class KmerCorrectRules(C.Structure):
    """dsrcgpu_kmer_correct_rules: KmerCorrectRules(min_count, max_quality); max_quality None = 255 = a base of any quality may be
    replaced (the qualities are then not read).  The library is the one that refuses figures out of range."""
    _fields_ = [("min_count", C.c_uint64), ("max_quality", C.c_uint32), ("reserved", C.c_uint32 * 5)]

    def __init__(self, min_count=2, max_quality=None, reserved=(0, 0, 0, 0, 0)):
        super().__init__()
        self.min_count, self.max_quality = min_count, 255 if max_quality is None else max_quality
        self.reserved = (C.c_uint32 * 5)(*reserved)


KMER_CORRECT_STATS = ("records_considered", "records_came_dropped", "records_no_window", "windows", "windows_solid", "runs", "bases_fixed",
                      "bases_fixed_n", "records_fixed", "runs_whole_range", "runs_long", "runs_short_interior", "runs_no_candidate",
                      "runs_ambiguous", "runs_quality", "records_all_solid")


class HostColumns(typing.NamedTuple):
    """What Handle.decompress_columns returns: the five arrays as numpy (titles / title_offsets None when not wanted)."""
    bases: object
    quals: object
    titles: object
    seq_offsets: object
    title_offsets: object
    block_records: list
    totals: list
    crc_ok: object


class DsrcGpuError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"dsrc_gpu error {code}: {msg}")
        self.code = code


_lib = None


def lib_path() -> str:
    return os.environ.get("DSRC_GPU_LIB", DEFAULT_LIB)


def load():
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          f"(hipcc --offload-arch=gfx950). The DSRC GPU path has no CPU fallback.")
    L = C.CDLL(path)
    L.dsrcgpu_last_error.restype = C.c_char_p
    L.dsrcgpu_last_error.argtypes = [C.c_void_p]
    L.dsrcgpu_destroy.restype = None
    L.dsrcgpu_destroy.argtypes = [C.c_void_p]
    L.dsrcgpu_chain_destroy.restype = None
    L.dsrcgpu_chain_destroy.argtypes = [C.c_void_p]
    L.dsrcgpu_set_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.dsrcgpu_set_record_layout.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.dsrcgpu_title_fields.restype = C.c_uint32
    L.dsrcgpu_title_fields.argtypes = [C.c_char_p, C.c_uint32, C.c_uint64]
    L.dsrcgpu_fields_capacity_after.restype = C.c_uint32
    L.dsrcgpu_fields_capacity_after.argtypes = [C.c_uint32, C.c_uint32]
    L.dsrcgpu_chain_seed.argtypes = [C.c_void_p, C.c_uint32]
    _lib = L
    return L


def fields_capacity_fold(chunks, tag_flags: int = 0, cap: int = 0) -> int:
    """The block-to-block state (capacity of the reference's TagStats::fields) after `chunks` have been compressed in
    order, from the first title line of each chunk alone (include/dsrc_gpu.h: dsrcgpu_fields_capacity_after)."""
    L = load()
    for c in chunks:
        e = 0
        while e < len(c) and c[e] not in (10, 13):
            e += 1
        cap = L.dsrcgpu_fields_capacity_after(cap, L.dsrcgpu_title_fields(bytes(c[:e]), e, tag_flags))
    return cap


def host_alloc(nbytes: int) -> int:
    """Page-locked host memory (dsrcgpu_host_alloc); free with host_free."""
    p = C.c_void_p()
    rc = load().dsrcgpu_host_alloc(C.c_uint64(nbytes), C.byref(p))
    if rc:
        raise DsrcGpuError(rc, "dsrcgpu_host_alloc failed")
    return p.value


def host_free(ptr: int):
    load().dsrcgpu_host_free(C.c_void_p(ptr))


class Chain:
    """Hands DSRC's block-to-block state from batch seq to batch seq+1 across handles (include/dsrc_gpu.h)."""

    def __init__(self):
        self.L = load()
        self.c = C.c_void_p()
        rc = self.L.dsrcgpu_chain_create(C.byref(self.c))
        if rc != 0:
            raise DsrcGpuError(rc, "dsrcgpu_chain_create failed")

    def seed(self, fields_capacity: int):
        rc = self.L.dsrcgpu_chain_seed(self.c, fields_capacity)
        if rc != 0:
            raise DsrcGpuError(rc, "dsrcgpu_chain_seed: the chain has already started")

    def close(self):
        if getattr(self, "c", None):
            self.L.dsrcgpu_chain_destroy(self.c)
            self.c = None


class Handle:
    """One GPU block scheduler (replaces the reference's pool of BlockCompressor worker threads)."""

    def __init__(self, dna_order=0, quality_order=0, lossy=False, crc=False, quality_offset=33,
                 plus_repetition=False, color_space=False, tag_flags=0, device=0, arena_bytes=0, verify=False):
        self.L = load()
        self.h = C.c_void_p()
        self.device = device
        s = Settings(dna_order, quality_order, tag_flags, int(lossy), int(crc), int(verify))
        d = Dataset(quality_offset, int(plus_repetition), int(color_space))
        rc = self.L.dsrcgpu_create(C.byref(s), C.byref(d), device, C.c_uint64(arena_bytes), C.byref(self.h))
        if rc != 0:
            msg = self.L.dsrcgpu_last_error(self.h).decode() if self.h else "create failed"
            if self.h:
                self.L.dsrcgpu_destroy(self.h)
                self.h = None
            raise DsrcGpuError(rc, msg)

    def close(self):
        if getattr(self, "h", None):
            self.L.dsrcgpu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc < 0:
            raise DsrcGpuError(rc, self.L.dsrcgpu_last_error(self.h).decode())
        return rc

    def set_chain(self, chain, seq: int):
        """The next batch call on this handle is batch number `seq` of `chain` (None detaches)."""
        self._chk(self.L.dsrcgpu_set_chain(self.h, chain.c if chain is not None else None, C.c_uint64(seq)))

    def set_lanes(self, lanes: int = 0, sub_batch_chunks: int = 0):
        """Scheduler lanes inside the handle (include/dsrc_gpu.h): 0 = the defaults, lanes = 1: batches stay on the handle's own lane."""
        self._chk(self.L.dsrcgpu_set_lanes(self.h, C.c_uint32(lanes), C.c_uint32(sub_batch_chunks)))

    def set_fields_capacity(self, cap: int):
        """Seed the block-to-block state of a handle that starts in the middle of an archive (see fields_capacity_fold)."""
        self._chk(self.L.dsrcgpu_set_fields_capacity(self.h, C.c_uint32(cap)))

    def get_fields_capacity(self) -> int:
        v = C.c_uint32()
        self._chk(self.L.dsrcgpu_get_fields_capacity(self.h, C.byref(v)))
        return v.value

    def set_record_layout(self, chunk_sizes):
        """The next batch call compresses chunks assembled from records (reference: BlockCompressorExt);
        chunk_sizes[i] is block i's chunkSize word."""
        arr = (C.c_uint32 * len(chunk_sizes))(*[v & 0xFFFFFFFF for v in chunk_sizes])
        self._chk(self.L.dsrcgpu_set_record_layout(self.h, len(chunk_sizes), arr))

    def compress_block(self, data: bytes):
        cap = len(data) + (1 << 16)
        out = (C.c_uint8 * cap)()
        osz = C.c_uint64()
        raw = (C.c_uint64 * 4)(); comp = (C.c_uint64 * 4)()
        self._chk(self.L.dsrcgpu_compress_block(self.h, data, C.c_uint64(len(data)), out, C.c_uint64(cap), C.byref(osz), raw, comp))
        return bytes(out[: osz.value]), list(raw), list(comp)

    def compress_batch(self, chunks, cap=None):
        n = len(chunks)
        ptrs = (C.c_char_p * n)(*chunks)
        sizes = (C.c_uint64 * n)(*[len(c) for c in chunks])
        if cap is None:
            cap = sum(len(c) for c in chunks) + n * (1 << 16)
        out = (C.c_uint8 * cap)()
        offs = (C.c_uint64 * n)(); osz = (C.c_uint64 * n)()
        raw = (C.c_uint64 * (4 * n))(); comp = (C.c_uint64 * (4 * n))()
        self._chk(self.L.dsrcgpu_compress_batch(self.h, n, ptrs, sizes, out, C.c_uint64(cap), offs, osz, raw, comp))
        mv = memoryview(out)
        return [(bytes(mv[offs[i]: offs[i] + osz[i]]), list(raw[4 * i: 4 * i + 4]), list(comp[4 * i: 4 * i + 4])) for i in range(n)]

    def decompress_batch(self, blocks, cap=None, text_caps=None, verify=False):
        """BlockCompressor::Read for a batch of blocks -> list of chunk texts (each ends with a newline);
        with verify=True also the per-block VerifyChecksum verdicts."""
        n = len(blocks)
        ptrs = (C.c_char_p * n)(*blocks)
        sizes = (C.c_uint64 * n)(*[len(b) for b in blocks])
        if cap is None:
            cap = sum(text_caps) if text_caps else sum(int.from_bytes(b[12:16], "big") + 1 for b in blocks)
        out = (C.c_uint8 * max(cap, 1))()
        offs = (C.c_uint64 * n)(); osz = (C.c_uint64 * n)(); ok = (C.c_uint32 * n)()
        caps = (C.c_uint64 * n)(*text_caps) if text_caps else None
        self._chk(self.L.dsrcgpu_decompress_batch(self.h, n, ptrs, sizes, caps, out, C.c_uint64(cap), offs, osz, ok if verify else None))
        mv = memoryview(out)
        texts = [bytes(mv[offs[i]: offs[i] + osz[i]]) for i in range(n)]
        return (texts, list(ok)) if verify else texts

    def decompress_batch_device(self, d_in: int, offs, sizes, d_out: int, out_cap: int, verify=False):
        n = len(offs)
        a_offs = (C.c_uint64 * n)(*offs); a_sizes = (C.c_uint64 * n)(*sizes)
        o_offs = (C.c_uint64 * n)(); o_sizes = (C.c_uint64 * n)(); ok = (C.c_uint32 * n)()
        self._chk(self.L.dsrcgpu_decompress_batch_device(self.h, n, C.c_void_p(d_in), a_offs, a_sizes, None, C.c_void_p(d_out),
                                                         C.c_uint64(out_cap), o_offs, o_sizes, ok if verify else None))
        return (list(o_offs), list(o_sizes), list(ok)) if verify else (list(o_offs), list(o_sizes))

    def decompress_columns_device(self, d_in: int, offs, sizes, cols: Columns, text_caps=None, verify=False):
        """dsrcgpu_decompress_batch_columns_device: the records of the blocks as arrays in the caller's device memory (`cols`).
        Returns (block_records, totals[, crc_ok]); DsrcGpuError.code == E_CAPACITY when an array is too small -- `need` of the
        exception then holds the totals (records, bases, title bytes) to allocate for."""
        n = len(offs)
        a_offs = (C.c_uint64 * max(n, 1))(*offs); a_sizes = (C.c_uint64 * max(n, 1))(*sizes)
        caps = (C.c_uint64 * n)(*text_caps) if text_caps else None
        recs = (C.c_uint64 * (n + 1))(); totals = (C.c_uint64 * 3)(); ok = (C.c_uint32 * max(n, 1))()
        rc = self.L.dsrcgpu_decompress_batch_columns_device(self.h, C.c_uint32(n), C.c_void_p(d_in), a_offs, a_sizes, caps, C.byref(cols),
                                                            recs, totals, ok if verify else None)
        if rc < 0:
            e = DsrcGpuError(rc, self.L.dsrcgpu_last_error(self.h).decode())
            e.need = list(totals) if rc == E_CAPACITY else None
            raise e
        return (list(recs), list(totals), list(ok)[:n]) if verify else (list(recs), list(totals))

    def decompress_columns(self, blocks, titles=True, text_caps=None, verify=False) -> HostColumns:
        """Host convenience over decompress_columns_device: stages the blocks in HBM, sizes the arrays from a first call with
        capacities of zero, decodes, and brings the arrays back as numpy."""
        import numpy as np
        n = len(blocks)
        offs, pos = [], 0
        for b in blocks:
            offs.append(pos); pos += (len(b) + 63) // 64 * 64
        sizes = [len(b) for b in blocks]
        held = []

        def alloc(nbytes):
            p = self.dev_alloc(max(nbytes, 8)); held.append(p)
            return p

        def fetch(ptr, count, dtype):
            nbytes = count * np.dtype(dtype).itemsize
            return np.frombuffer(self.dev_download(ptr, nbytes), dtype=dtype).copy() if nbytes else np.zeros(0, dtype)
        try:
            d_in = alloc(pos)
            for b, o in zip(blocks, offs):
                self.dev_upload(d_in + o, b)
            need = [0, 0, 0]
            if n:
                try:
                    self.decompress_columns_device(d_in, offs, sizes, Columns(), text_caps=text_caps)
                except DsrcGpuError as e:
                    if e.code != E_CAPACITY or not any(e.need):      # (all zero: it is a block's TEXT that does not fit its text_caps)
                        raise
                    need = e.need
            R, S, T = need
            cols = Columns(alloc(S), S, alloc(S), S, alloc(T) if titles else None, T if titles else 0,
                           alloc(8 * (R + 1)), alloc(8 * (R + 1)) if titles else None, R)
            res = self.decompress_columns_device(d_in, offs, sizes, cols, text_caps=text_caps, verify=verify)
            return HostColumns(fetch(cols.d_bases, S, np.uint8), fetch(cols.d_quals, S, np.uint8),
                               fetch(cols.d_titles, T, np.uint8) if titles else None, fetch(cols.d_seq_offs, R + 1, np.uint64),
                               fetch(cols.d_title_offs, R + 1, np.uint64) if titles else None, res[0], res[1], res[2] if verify else None)
        finally:
            for p in held:
                self.dev_free(p)

    def compress_columns_device(self, cols_in: ColumnsIn, block_records, d_out: int, out_cap: int):
        """dsrcgpu_compress_columns_device: block i = records block_records[i] .. block_records[i + 1] - 1 of the device arrays
        `cols_in`, written back to back to d_out.  Returns (block_offs, block_sizes, raw_sizes, comp_sizes)."""
        n = len(block_records) - 1
        recs = (C.c_uint64 * (n + 1))(*block_records)
        o_offs = (C.c_uint64 * max(n, 1))(); o_sizes = (C.c_uint64 * max(n, 1))()
        raw = (C.c_uint64 * max(4 * n, 1))(); comp = (C.c_uint64 * max(4 * n, 1))()
        self._chk(self.L.dsrcgpu_compress_columns_device(self.h, C.c_uint32(n), C.byref(cols_in), recs, C.c_void_p(d_out),
                                                         C.c_uint64(out_cap), o_offs, o_sizes, raw, comp))
        return list(o_offs)[:n], list(o_sizes)[:n], list(raw)[:4 * n], list(comp)[:4 * n]

    def columns_cut(self, cols_in: ColumnsIn, chunk_bytes: int, cap: int | None = None):
        """dsrcgpu_columns_cut: the greedy cut of the records of `cols_in` into blocks of at most chunk_bytes of chunk text (at least
        one record each) -> block_records (blocks + 1 entries).  With `cap` (entries) given, a cut that needs more raises
        DsrcGpuError with .code == E_CAPACITY and .need = the number of blocks; without, the call is repeated with that many."""
        grow = cap is None
        if grow:
            cap = min(int(cols_in.n_records), 4096) + 1
        while True:
            recs = (C.c_uint64 * max(cap, 1))(); n = C.c_uint32()
            rc = self.L.dsrcgpu_columns_cut(self.h, C.byref(cols_in), C.c_uint64(chunk_bytes), recs, C.c_uint32(cap), C.byref(n))
            if rc == E_CAPACITY and grow:
                cap, grow = n.value + 1, False
                continue
            if rc < 0:
                e = DsrcGpuError(rc, self.L.dsrcgpu_last_error(self.h).decode())
                e.need = n.value if rc == E_CAPACITY else None
                raise e
            return list(recs)[: n.value + 1]

    def compress_columns(self, cols, block_records=None, chunk_bytes=8 << 20):
        """Host convenience over compress_columns_device: `cols` has numpy arrays bases, quals, titles, seq_offsets, title_offsets
        (a HostColumns, or anything shaped like it); they are staged in HBM, cut with columns_cut unless block_records is given,
        compressed, and the blocks come back as a list of bytes."""
        import numpy as np
        held = []

        def stage(a, dtype):
            data = np.ascontiguousarray(a, dtype=dtype).tobytes()
            p = self.dev_alloc(max(len(data), 8)); held.append(p)
            if data:
                self.dev_upload(p, data)
            return p
        try:
            R = len(cols.seq_offsets) - 1
            cin = ColumnsIn(stage(cols.bases, np.uint8), len(cols.bases), stage(cols.quals, np.uint8), stage(cols.titles, np.uint8),
                            len(cols.titles), stage(cols.seq_offsets, np.uint64), stage(cols.title_offsets, np.uint64), R)
            if block_records is None:
                block_records = self.columns_cut(cin, chunk_bytes)
            block_records = [int(v) for v in block_records]
            n = len(block_records) - 1
            # (the text: two bytes a base, the title at most twice, six more a record; a block is not larger than its text + 64 KiB)
            cap = 2 * len(cols.bases) + 2 * len(cols.titles) + 6 * R + n * (1 << 16) + 64
            d_out = self.dev_alloc(cap); held.append(d_out)
            offs, sizes, _, _ = self.compress_columns_device(cin, block_records, d_out, cap)
            return [self.dev_download(d_out + o, s) for o, s in zip(offs, sizes)]
        finally:
            for p in held:
                self.dev_free(p)

    def columns_trim_plan(self, cols_in: ColumnsIn, rules: TrimRules, d_begin: int, d_end: int, d_keep: int):
        """dsrcgpu_columns_trim_plan: the kept range of every record of `cols_in` into d_begin / d_end (uint64 each) and its keep
        flag into d_keep (uint8), all device memory of n_records entries.  Returns the six statistics (TRIM_STATS names them)."""
        stats = (C.c_uint64 * 6)()
        self._chk(self.L.dsrcgpu_columns_trim_plan(self.h, C.byref(cols_in), C.byref(rules), C.c_void_p(d_begin), C.c_void_p(d_end),
                                                   C.c_void_p(d_keep), stats))
        return list(stats)

    def columns_adapter_plan(self, cols_in: ColumnsIn, rules: AdapterRules, d_begin_in, d_end_in, d_keep_in, d_begin: int, d_end: int,
                             d_keep: int, d_which=None):
        """dsrcgpu_columns_adapter_plan: the 3' adapter search on the plan d_begin_in / d_end_in / d_keep_in (device addresses or None:
        whole reads, every record) into d_begin / d_end (uint64 each), d_keep (uint8) and, if wanted, d_which (uint32: the adapter
        found, NO_ADAPTER for none), all device memory of n_records entries; an output may be the very array of its input.  Returns
        the thirteen statistics (ADAPTER_STATS names them)."""
        stats = (C.c_uint64 * 13)()
        self._chk(self.L.dsrcgpu_columns_adapter_plan(self.h, C.byref(cols_in), C.byref(rules), C.c_void_p(d_begin_in), C.c_void_p(d_end_in),
                                                      C.c_void_p(d_keep_in), C.c_void_p(d_begin), C.c_void_p(d_end), C.c_void_p(d_keep),
                                                      C.c_void_p(d_which), stats))
        return list(stats)

    def columns_complexity_plan(self, cols_in: ColumnsIn, rules: ComplexityRules, d_begin_in, d_end_in, d_keep_in, d_begin: int, d_end: int,
                                d_keep: int, d_info=None):
        """dsrcgpu_columns_complexity_plan: poly-X ends, the complexity filter and the DUST filter on the plan d_begin_in / d_end_in /
        d_keep_in (device addresses or None: whole reads, every record) into d_begin / d_end (uint64 each), d_keep (uint8) and, if
        wanted, d_info (uint32, two per record: head base | tail base << 8, complexity permille | dust << 16), device memory of
        n_records entries; an output may be the very array of its input.  Returns the twenty statistics (COMPLEXITY_STATS names the
        first seventeen, the rest are 0)."""
        stats = (C.c_uint64 * 20)()
        self._chk(self.L.dsrcgpu_columns_complexity_plan(self.h, C.byref(cols_in), C.byref(rules), C.c_void_p(d_begin_in), C.c_void_p(d_end_in),
                                                         C.c_void_p(d_keep_in), C.c_void_p(d_begin), C.c_void_p(d_end), C.c_void_p(d_keep),
                                                         C.c_void_p(d_info), stats))
        return list(stats)

    def columns_demux_plan(self, cols_in: ColumnsIn, index_sets, rules: DemuxRules, d_begin_in, d_end_in, d_keep_in, d_begin: int, d_end: int,
                           d_keep: int, d_class: int, d_info=None, d_class_counts=None):
        """dsrcgpu_columns_demux_plan: every record of `cols_in` gets the sample whose barcodes lie nearest, read from the record under
        the plan d_begin_in / d_end_in / d_keep_in (device addresses or None: whole reads, every record) or from `index_sets` (a list
        of up to two ColumnsIn of equally many records).  Out: d_begin / d_end (uint64 each), d_keep (uint8), d_class (uint32: the
        sample, n_samples for unassigned, 0xFFFFFFFF for a record that came in dropped) and, if wanted, d_info (uint32: best | second
        << 8 | reason << 16) and d_class_counts (uint64, n_samples + 1, added to), device memory; an output may be the very array of
        its input.  Returns the nine statistics (DEMUX_STATS names them)."""
        stats = (C.c_uint64 * 9)()
        index_sets = list(index_sets or ())
        sets = (C.POINTER(ColumnsIn) * max(len(index_sets), 1))(*[C.pointer(s) for s in index_sets])
        self._chk(self.L.dsrcgpu_columns_demux_plan(self.h, C.byref(cols_in), sets if index_sets else None, C.c_uint32(len(index_sets)),
                                                    C.byref(rules), C.c_void_p(d_begin_in), C.c_void_p(d_end_in), C.c_void_p(d_keep_in),
                                                    C.c_void_p(d_begin), C.c_void_p(d_end), C.c_void_p(d_keep), C.c_void_p(d_class),
                                                    C.c_void_p(d_info), C.c_void_p(d_class_counts), stats))
        return list(stats)

    def columns_partition_device(self, cols_in: ColumnsIn, d_begin, d_end, d_keep, d_class, n_classes: int, out: Columns, d_source=None):
        """dsrcgpu_columns_partition_device: the kept records of `cols_in` with d_class[r] < n_classes, cut to [begin, end), grouped by
        class and in input order inside a class, into the device arrays `out`.  Returns (totals, class_records): totals = records,
        bases, title bytes that come out and the kept records left out for their class; class_records = the exclusive prefix of the
        records per class (n_classes + 1 entries).  DsrcGpuError.code == E_CAPACITY when an array is too small -- `need` of the
        exception then holds the first three totals, `class_records` the prefix."""
        totals = (C.c_uint64 * 4)()
        recs = (C.c_uint64 * (max(int(n_classes), 0) + 1))()
        rc = self.L.dsrcgpu_columns_partition_device(self.h, C.byref(cols_in), C.c_void_p(d_begin), C.c_void_p(d_end), C.c_void_p(d_keep),
                                                     C.c_void_p(d_class), C.c_uint32(n_classes), C.byref(out), C.c_void_p(d_source), recs, totals)
        if rc < 0:
            e = DsrcGpuError(rc, self.L.dsrcgpu_last_error(self.h).decode())
            e.need = list(totals)[:3] if rc == E_CAPACITY else None
            e.class_records = list(recs) if rc == E_CAPACITY else None
            e.totals = list(totals)
            raise e
        return list(totals), list(recs)

    def columns_pair_plan(self, cols_in1: ColumnsIn, cols_in2: ColumnsIn, rules: PairRules, plan1_in, plan2_in, d_begin1: int, d_end1: int,
                          d_begin2: int, d_end2: int, d_keep: int, d_insert=None):
        """dsrcgpu_columns_pair_plan: the overlap search and the joint keep on the mates cols_in1 / cols_in2.  plan<s>_in is the triple
        (d_begin_in, d_end_in, d_keep_in) of side s (device addresses or None: whole reads, every record); the ranges go out into
        d_begin<s> / d_end<s> (uint64 each), the pair's flag into d_keep (uint8) and, if wanted, the insert size into d_insert (uint64,
        NO_INSERT for none), all device memory of n_records entries; a range output may be the very array of its input, d_keep either
        incoming keep.  Returns the eleven statistics (PAIR_STATS names them)."""
        stats = (C.c_uint64 * 11)()
        (b1, e1, k1), (b2, e2, k2) = plan1_in, plan2_in
        self._chk(self.L.dsrcgpu_columns_pair_plan(self.h, C.byref(cols_in1), C.byref(cols_in2), C.byref(rules), C.c_void_p(b1), C.c_void_p(e1),
                                                   C.c_void_p(k1), C.c_void_p(b2), C.c_void_p(e2), C.c_void_p(k2), C.c_void_p(d_begin1),
                                                   C.c_void_p(d_end1), C.c_void_p(d_begin2), C.c_void_p(d_end2), C.c_void_p(d_keep),
                                                   C.c_void_p(d_insert), stats))
        return list(stats)

    def columns_dedup_plan(self, cols_in1: ColumnsIn, cols_in2, rules: DedupRules, ranges1, ranges2, d_keep_in, d_keep: int, d_dup_of=None,
                           d_copies=None):
        """dsrcgpu_columns_dedup_plan: exact duplicates among the records of cols_in1 (cols_in2 None) or among the pairs cols_in1 /
        cols_in2.  ranges<s> is the pair (d_begin, d_end) of side s (device addresses or None: whole reads), d_keep_in the incoming
        flag (or None: every record); d_keep (uint8) gets 1 for the one record of every class that survives -- it may be the very
        array d_keep_in --, d_dup_of (uint64, or None) the surviving record's index (NO_DUP_OF for a record that came in dropped),
        d_copies (uint64, or None) the class size at the survivor and 0 elsewhere, all device memory of n_records entries.  Returns
        the 24 statistics (DEDUP_STATS names them)."""
        stats = (C.c_uint64 * 24)()
        (b1, e1), (b2, e2) = ranges1, ranges2
        self._chk(self.L.dsrcgpu_columns_dedup_plan(self.h, C.byref(cols_in1), C.byref(cols_in2) if cols_in2 is not None else None, C.byref(rules),
                                                    C.c_void_p(b1), C.c_void_p(e1), C.c_void_p(b2), C.c_void_p(e2), C.c_void_p(d_keep_in),
                                                    C.c_void_p(d_keep), C.c_void_p(d_dup_of), C.c_void_p(d_copies), stats))
        return list(stats)

    def columns_merge_device(self, cols_in1: ColumnsIn, cols_in2: ColumnsIn, rules: MergeRules, ranges1, ranges2, d_keep, d_insert, out: Columns,
                             d_merged, d_source=None):
        """dsrcgpu_columns_merge_device: the mates cols_in1 / cols_in2 whose ranges overlap by the insert sizes d_insert (uint64, as
        columns_pair_plan wrote them) merged into one read each, compacted into the device arrays `out`.  ranges<s> is the pair
        (d_begin, d_end) of side s (device addresses or None: whole reads), d_keep the pair's flag (or None: every pair); d_merged
        (uint8, n_records) gets 1 for every pair that is in `out`, d_source (uint64, or None) the pair index of each output record.
        Returns (totals, stats): records, bases, title bytes of `out`, and the twelve statistics (MERGE_STATS names them);
        DsrcGpuError.code == E_CAPACITY when an array is too small -- `need` of the exception then holds the totals and `stats` the
        statistics."""
        totals, stats = (C.c_uint64 * 3)(), (C.c_uint64 * 12)()
        (b1, e1), (b2, e2) = ranges1, ranges2
        rc = self.L.dsrcgpu_columns_merge_device(self.h, C.byref(cols_in1), C.byref(cols_in2), C.byref(rules), C.c_void_p(b1), C.c_void_p(e1),
                                                 C.c_void_p(b2), C.c_void_p(e2), C.c_void_p(d_keep), C.c_void_p(d_insert), C.byref(out),
                                                 C.c_void_p(d_merged), C.c_void_p(d_source), totals, stats)
        if rc < 0:
            e = DsrcGpuError(rc, self.L.dsrcgpu_last_error(self.h).decode())
            e.need = list(totals) if rc == E_CAPACITY else None
            e.stats = list(stats) if rc == E_CAPACITY else None
            raise e
        return list(totals), list(stats)

    def columns_profile(self, cols_in: ColumnsIn, d_begin, d_end, d_keep, rules: ProfileRules, d_profile: int):
        """dsrcgpu_columns_profile: the per-cycle profile of the records of `cols_in` under the plan d_begin / d_end / d_keep (device
        addresses or None: whole reads, every record) into d_profile (device memory of profile_words(rules.n_cycles) uint64 words;
        overwritten, or added to with rules.accumulate = 1).  Returns this call's own eight totals (PROFILE_TOTALS names them)."""
        totals = (C.c_uint64 * 8)()
        self._chk(self.L.dsrcgpu_columns_profile(self.h, C.byref(cols_in), C.c_void_p(d_begin), C.c_void_p(d_end), C.c_void_p(d_keep),
                                                 C.byref(rules), C.c_void_p(d_profile), totals))
        return list(totals)

    def _chk_need(self, rc, need):
        if rc < 0:
            e = DsrcGpuError(rc, self.L.dsrcgpu_last_error(self.h).decode())
            e.need = int(need[0]) if rc == E_CAPACITY else None
            raise e

    def columns_kmer_count(self, cols_in: ColumnsIn, d_begin, d_end, d_keep, rules: KmerRules, d_table: int):
        """dsrcgpu_columns_kmer_count: the k-mers of the records of `cols_in` under the plan d_begin / d_end / d_keep (device
        addresses or None: whole reads, every record) into the table d_table (device memory of kmer_words(rules.capacity) uint64
        words; initialised first, or added to with rules.accumulate = 1).  Returns the sixteen statistics (KMER_STATS names the
        first ten); DsrcGpuError.code == E_CAPACITY when the table is too small for the call -- `need` of the exception then holds
        the capacity that would do, and the table is untouched."""
        stats, need = (C.c_uint64 * 16)(), (C.c_uint64 * 1)()
        self._chk_need(self.L.dsrcgpu_columns_kmer_count(self.h, C.byref(cols_in), C.c_void_p(d_begin), C.c_void_p(d_end), C.c_void_p(d_keep),
                                                         C.byref(rules), C.c_void_p(d_table), stats, need), need)
        return list(stats)

    def kmer_table_merge(self, d_src: int, d_dst: int):
        """dsrcgpu_kmer_table_merge: every (key, count) of the table at d_src is added into the table at d_dst (same k and
        canonical, any capacities).  Returns the eight statistics (KMER_MERGE_STATS names the first six); E_CAPACITY as
        columns_kmer_count."""
        stats, need = (C.c_uint64 * 8)(), (C.c_uint64 * 1)()
        self._chk_need(self.L.dsrcgpu_kmer_table_merge(self.h, C.c_void_p(d_src), C.c_void_p(d_dst), stats, need), need)
        return list(stats)

    def kmer_spectrum(self, d_table: int, n_bins: int, d_hist: int):
        """dsrcgpu_kmer_spectrum: d_hist[c] (device memory of n_bins uint64 words) = the distinct keys counted c times, the last bin
        folding.  Returns the four totals (KMER_SPECTRUM_TOTALS names them)."""
        totals = (C.c_uint64 * 4)()
        self._chk(self.L.dsrcgpu_kmer_spectrum(self.h, C.c_void_p(d_table), C.c_uint32(n_bins), C.c_void_p(d_hist), totals))
        return list(totals)

    def kmer_lookup(self, d_table: int, d_kmers, n: int, d_counts) -> int:
        """dsrcgpu_kmer_lookup: d_counts[i] = the count of the packed k-mer d_kmers[i] (device memory of n uint64 words each).
        Returns the number of query words of 4^k and more."""
        invalid = C.c_uint64()
        self._chk(self.L.dsrcgpu_kmer_lookup(self.h, C.c_void_p(d_table), C.c_void_p(d_kmers), C.c_uint64(n), C.c_void_p(d_counts), C.byref(invalid)))
        return invalid.value

    def columns_kmer_plan(self, cols_in: ColumnsIn, rules: KmerPlanRules, d_table, d_begin_in, d_end_in, d_keep_in, d_begin, d_end, d_keep,
                          d_good=None, d_hits=None, d_median=None):
        """dsrcgpu_columns_kmer_plan: every window of the records of `cols_in` under the plan d_begin_in / d_end_in / d_keep_in (device
        addresses or None: whole reads, every record) looked up in the table d_table (of columns_kmer_count; only read) -> the
        narrowed plan in d_begin / d_end (uint64 each), d_keep (uint8) and, if wanted, the good windows, the hits and the median count
        of every record in d_good / d_hits / d_median (uint64 each), all device memory of n_records entries; an output may be the very
        array of its input.  Returns the sixteen statistics (KMER_PLAN_STATS names the first fifteen)."""
        stats = (C.c_uint64 * 16)()
        self._chk(self.L.dsrcgpu_columns_kmer_plan(self.h, C.byref(cols_in), C.byref(rules), C.c_void_p(d_table), C.c_void_p(d_begin_in),
                                                   C.c_void_p(d_end_in), C.c_void_p(d_keep_in), C.c_void_p(d_begin), C.c_void_p(d_end),
                                                   C.c_void_p(d_keep), C.c_void_p(d_good), C.c_void_p(d_hits), C.c_void_p(d_median), stats))
        return list(stats)

    def columns_kmer_correct(self, cols_in: ColumnsIn, rules: KmerCorrectRules, d_table, d_begin, d_end, d_keep, d_bases_out, d_fixed=None):
        """dsrcgpu_columns_kmer_correct: the substitution errors of the records of `cols_in` under the plan d_begin / d_end / d_keep (device
        addresses or None: whole reads, every record) repaired against the table d_table (of columns_kmer_count; only read) into
        d_bases_out, device memory addressed like the bases of `cols_in` -- that very array (in place: only the repaired bytes are
        written) or another one (the span of the records is copied, with the repairs); d_fixed (uint64, n_records entries, or None)
        gets the repairs per record.  Returns the sixteen statistics (KMER_CORRECT_STATS names them)."""
        stats = (C.c_uint64 * 16)()
        self._chk(self.L.dsrcgpu_columns_kmer_correct(self.h, C.byref(cols_in), C.byref(rules), C.c_void_p(d_table), C.c_void_p(d_begin),
                                                      C.c_void_p(d_end), C.c_void_p(d_keep), C.c_void_p(d_bases_out), C.c_void_p(d_fixed), stats))
        return list(stats)

    def columns_select_device(self, cols_in: ColumnsIn, d_begin, d_end, d_keep, out: Columns, d_source=None):
        """dsrcgpu_columns_select_device: the kept records of `cols_in`, cut to [begin, end), compacted into the device arrays `out`
        (d_begin / d_end / d_keep / d_source: device addresses or None).  Returns totals (records, bases, title bytes kept);
        DsrcGpuError.code == E_CAPACITY when an array is too small -- `need` of the exception then holds the totals."""
        totals = (C.c_uint64 * 3)()
        rc = self.L.dsrcgpu_columns_select_device(self.h, C.byref(cols_in), C.c_void_p(d_begin), C.c_void_p(d_end), C.c_void_p(d_keep),
                                                  C.byref(out), C.c_void_p(d_source), totals)
        if rc < 0:
            e = DsrcGpuError(rc, self.L.dsrcgpu_last_error(self.h).decode())
            e.need = list(totals) if rc == E_CAPACITY else None
            raise e
        return list(totals)

    def select_columns(self, cols, begin=None, end=None, keep=None, titles=True, return_source=False):
        """Host convenience over columns_select_device: `cols` has numpy arrays bases, quals, titles, seq_offsets, title_offsets (a
        HostColumns, or anything shaped like it), begin / end / keep are numpy arrays or None; everything is staged in HBM, sized
        with a first call, selected, and the compacted arrays come back as a HostColumns (block_records = [0, kept], crc_ok None);
        return_source=True: -> (HostColumns, source), source[j] = the index in `cols` of output record j."""
        import numpy as np
        held = []

        def alloc(nbytes):
            p = self.dev_alloc(max(nbytes, 8)); held.append(p)
            return p

        def stage(a, dtype):
            if a is None:
                return None
            data = np.ascontiguousarray(a, dtype=dtype).tobytes()
            p = alloc(len(data))
            if data:
                self.dev_upload(p, data)
            return p

        def fetch(ptr, count, dtype):
            nbytes = count * np.dtype(dtype).itemsize
            return np.frombuffer(self.dev_download(ptr, nbytes), dtype=dtype).copy() if nbytes else np.zeros(0, dtype)
        try:
            R = len(cols.seq_offsets) - 1
            cin = ColumnsIn(stage(cols.bases, np.uint8), len(cols.bases), stage(cols.quals, np.uint8),
                            stage(cols.titles, np.uint8) if titles else None, len(cols.titles) if titles else 0,
                            stage(cols.seq_offsets, np.uint64), stage(cols.title_offsets, np.uint64) if titles else None, R)
            d_begin, d_end, d_keep = stage(begin, np.uint64), stage(end, np.uint64), stage(keep, np.uint8)
            spare = alloc(8)
            need = [0, 0, 0]
            try:
                self.columns_select_device(cin, d_begin, d_end, d_keep, Columns(d_titles=spare if titles else None))
            except DsrcGpuError as e:
                if e.code != E_CAPACITY:
                    raise
                need = e.need
            K, S, T = need
            out = Columns(alloc(S), S, alloc(S), S, alloc(T) if titles else None, T if titles else 0,
                          alloc(8 * (K + 1)), alloc(8 * (K + 1)) if titles else None, K)
            d_source = alloc(8 * K)
            totals = self.columns_select_device(cin, d_begin, d_end, d_keep, out, d_source)
            got = HostColumns(fetch(out.d_bases, S, np.uint8), fetch(out.d_quals, S, np.uint8),
                              fetch(out.d_titles, T, np.uint8) if titles else None, fetch(out.d_seq_offs, K + 1, np.uint64),
                              fetch(out.d_title_offs, K + 1, np.uint64) if titles else None, [0, K], totals, None)
            return (got, fetch(d_source, K, np.uint64)) if return_source else got
        finally:
            for p in held:
                self.dev_free(p)

    def compress_batch_device(self, d_in: int, offs, sizes, d_out: int, out_cap: int):
        n = len(offs)
        a_offs = (C.c_uint64 * n)(*offs); a_sizes = (C.c_uint64 * n)(*sizes)
        o_offs = (C.c_uint64 * n)(); o_sizes = (C.c_uint64 * n)()
        raw = (C.c_uint64 * (4 * n))(); comp = (C.c_uint64 * (4 * n))()
        self._chk(self.L.dsrcgpu_compress_batch_device(self.h, n, C.c_void_p(d_in), a_offs, a_sizes, C.c_void_p(d_out),
                                                       C.c_uint64(out_cap), o_offs, o_sizes, raw, comp))
        return list(o_offs), list(o_sizes), list(raw), list(comp)

    def submit_pinned(self, part_id: int, ptr: int, size: int) -> bool:
        """dsrcgpu_submit_pinned: the chunk at `ptr` (page-locked memory from host_alloc) is read in place; False = the ring is full."""
        rc = self.L.dsrcgpu_submit_pinned(self.h, C.c_int64(part_id), C.c_void_p(ptr), C.c_uint64(size))
        if rc == -8:
            return False
        self._chk(rc)
        return True

    def submit(self, part_id: int, data: bytes) -> bool:
        """False = all batches of the ring are in flight (DSRCGPU_E_BUSY): collect blocks, then submit again."""
        rc = self.L.dsrcgpu_submit(self.h, C.c_int64(part_id), data, C.c_uint64(len(data)))
        if rc == -8:
            return False
        self._chk(rc)
        return True

    def flush(self):
        self._chk(self.L.dsrcgpu_flush(self.h))

    def collect(self, wait: bool = True):
        pid = C.c_int64(); blk = C.POINTER(C.c_uint8)(); sz = C.c_uint64()
        raw = (C.c_uint64 * 4)(); comp = (C.c_uint64 * 4)()
        fn = self.L.dsrcgpu_collect if wait else self.L.dsrcgpu_try_collect
        rc = self._chk(fn(self.h, C.byref(pid), C.byref(blk), C.byref(sz), raw, comp))
        if rc == 0:
            return None
        data = bytes(C.cast(blk, C.POINTER(C.c_uint8 * sz.value)).contents) if sz.value else b""
        self.L.dsrcgpu_release(self.h, blk)
        return pid.value, data, list(raw), list(comp)

    def selftest(self) -> int:
        n = C.c_uint32(1)
        self._chk(self.L.dsrcgpu_selftest(self.h, C.byref(n)))
        return n.value

    def release_memory(self):
        """Hands the batch arena and the table region back to the device (they are allocated again on demand)."""
        self._chk(self.L.dsrcgpu_release_memory(self.h))

    def set_table_budget(self, nbytes: int):
        """HBM a decoding pass of this handle may take for model tables (dsrcgpu_set_table_budget; 0 = automatic again).  A pass
        whose tables do not fit runs in rounds; a budget below the largest table of a pass is raised to that table."""
        self._chk(self.L.dsrcgpu_set_table_budget(self.h, C.c_uint64(nbytes)))

    def reserve_memory(self, arena_bytes, table_bytes=0):
        """Grows the batch arena / the decoder's table region to at least these sizes now (nothing shrinks)."""
        self._chk(self.L.dsrcgpu_reserve_memory(self.h, C.c_uint64(arena_bytes), C.c_uint64(table_bytes)))

    def last_timing(self):
        ms = C.c_float(); rc_ms = C.c_float(); n = C.c_uint32()
        self.L.dsrcgpu_last_timing(self.h, C.byref(ms), C.byref(rc_ms), C.byref(n))
        return ms.value, rc_ms.value, n.value

    def last_stage_timing(self):
        a = C.c_float(); b = C.c_float()
        self.L.dsrcgpu_last_stage_timing(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    # device helpers -------------------------------------------------
    def dev_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._chk(self.L.dsrcgpu_dev_alloc(self.h, C.c_uint64(nbytes), C.byref(p)))
        return p.value

    def dev_free(self, ptr: int):
        self._chk(self.L.dsrcgpu_dev_free(self.h, C.c_void_p(ptr)))

    def dev_upload(self, d_dst: int, data: bytes):
        self._chk(self.L.dsrcgpu_dev_upload(self.h, C.c_void_p(d_dst), data, C.c_uint64(len(data))))

    def dev_download(self, d_src: int, nbytes: int) -> bytes:
        buf = (C.c_uint8 * nbytes)()
        self._chk(self.L.dsrcgpu_dev_download(self.h, buf, C.c_void_p(d_src), C.c_uint64(nbytes)))
        return bytes(buf)

    def synth_illumina(self, first: int, count: int, d_out: int, cap: int, binned: bool = False) -> int:
        n = C.c_uint64()
        self._chk(self.L.dsrcgpu_synth_fastq(self.h, C.c_uint32(1 if binned else 0), C.c_uint64(first), C.c_uint64(count), C.c_void_p(d_out), C.c_uint64(cap), C.byref(n)))
        return n.value

    def synth_fastq(self, flavour: int, first: int, count: int, d_out: int, cap: int) -> int:
        """Records first..first+count-1 of a SYNTH_* flavour written to d_out; returns the byte count (dsrc_amd/synth.py has the same bytes)."""
        n = C.c_uint64()
        self._chk(self.L.dsrcgpu_synth_fastq(self.h, C.c_uint32(flavour), C.c_uint64(first), C.c_uint64(count), C.c_void_p(d_out), C.c_uint64(cap), C.byref(n)))
        return n.value
