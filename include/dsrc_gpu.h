/*
 * dsrc_gpu.h -- C ABI of the MI355X-native DSRC block-compression path (libdsrc_gpu.so).
 *
 * This is the drop-in boundary: plain C, opaque handle, pointers and sizes only.  It replaces the
 * reference's CPU worker pool -- N threads each running
 *     BlockCompressor(datasetType, compSettings)                  (src/BlockCompressor.h:66)
 *     BlockCompressor::Store(BitMemoryWriter&, StreamsInfo& raw,
 *                            StreamsInfo& comp, const FastqDataChunk&)   (src/BlockCompressor.h:69)
 * inside DsrcCompressor::Process (src/DsrcWorker.cpp:30-73) -- by one GPU block scheduler.  Every
 * function returns 0 on success or a negative DSRCGPU_E_* code; dsrcgpu_last_error() gives the text.
 * Output blocks are bit-identical to what BlockCompressor::Store writes for the same chunk.
 *
 * INTEGRATION.md shows the binding a reference maintainer would add on top of this header.
 */
#ifndef DSRC_GPU_H
#define DSRC_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dsrcgpu_handle dsrcgpu_handle;

/* comp::CompressionSettings (src/Common.h:110-147).  Orders, not CLI levels:
 * dna_order = 3*level; quality_order = level (lossless) or 3*level (lossy) -- IDsrcOperator::GetCompressionSettings
 * (src/DsrcOperator.h:74-90). */
typedef struct dsrcgpu_settings
{
	uint32_t dna_order;
	uint32_t quality_order;
	uint64_t tag_preserve_flags;   /* -f mask (FastqParserExt, src/FastqParser.cpp:167-251): bit k set = keep title field k, k = 1..30;
	                                * 0 = titles as they are.  With a mask the chunk text is rewritten in place (device copy / the
	                                * caller's device buffer in the *_device entry point), as BlockCompressor::Store does to its input */
	uint8_t  lossy;
	uint8_t  calculate_crc32;
	uint8_t  verify_after_compress;/* with calculate_crc32: every compress call decodes the blocks it has written (on the device, nothing is
	                                * copied back) and fails with DSRCGPU_E_CRC "CRC32 checksums mismatch." unless the stored checksums match
	                                * -- the reference's worker does this whenever -c is given (src/DsrcWorker.cpp:53-62) */
	uint8_t  reserved[5];
} dsrcgpu_settings;

/* fq::FastqDatasetType (src/Common.h:56-80), decided once per file by FastqParser::Analyze on chunk 0. */
typedef struct dsrcgpu_dataset
{
	uint32_t quality_offset;       /* 33..64, already resolved (not 0/auto) */
	uint8_t  plus_repetition;
	uint8_t  color_space;          /* SOLiD colour space (primer base + colours); not together with tag_preserve_flags / record layout */
	uint8_t  reserved[2];
} dsrcgpu_dataset;

enum
{
	DSRCGPU_OK            =  0,
	DSRCGPU_E_ARG         = -1,   /* bad argument / unsupported setting */
	DSRCGPU_E_HIP         = -2,   /* HIP runtime failure (text in last_error) */
	DSRCGPU_E_NOMEM       = -3,
	DSRCGPU_E_CAPACITY    = -4,   /* caller's output buffer too small */
	DSRCGPU_E_INPUT       = -5,   /* a chunk could not be coded (no records, invalid bases, reference-UB input ...) */
	DSRCGPU_E_STATE       = -6,
	DSRCGPU_E_CRC         = -7,   /* verify_after_compress: a block did not decode back to the checksums stored in it */
	DSRCGPU_E_BUSY        = -8    /* dsrcgpu_submit: all batches of the ring are in flight -- collect and release blocks, then submit again */
};

/* Replaces: BlockCompressor::BlockCompressor (src/BlockCompressor.cpp:53-94) x worker threads.
 * device: HIP device ordinal.  arena_bytes: HBM to reserve for batch scratch, 0 = grow on demand. */
int dsrcgpu_create(const dsrcgpu_settings* settings, const dsrcgpu_dataset* dataset, int device,
				   uint64_t arena_bytes, dsrcgpu_handle** out);
void dsrcgpu_destroy(dsrcgpu_handle* h);
const char* dsrcgpu_last_error(const dsrcgpu_handle* h);

/* Replaces one call of BlockCompressor::Store (src/BlockCompressor.cpp:208-220) + bitMemory.Flush()
 * (src/DsrcWorker.cpp:48-51): chunk (host memory, size = FastqDataChunk::size, i.e. without the final newline)
 * -> block bytes.  raw_sizes/comp_sizes are fq::StreamsInfo::sizes in enum order Meta, Tag, Dna, Quality
 * (src/Common.h:82-105).  Synchronous. */
int dsrcgpu_compress_block(dsrcgpu_handle* h, const uint8_t* fastq, uint64_t size,
						   uint8_t* block, uint64_t block_cap, uint64_t* block_size,
						   uint64_t raw_sizes[4], uint64_t comp_sizes[4]);

/* The same for n chunks in one scheduler pass (this is what keeps the GPU full).  Blocks are written back to
 * back into `blocks` in chunk order; block_offs/block_sizes get n entries, raw_sizes/comp_sizes 4*n.
 * Compressor state that the reference carries from block to block inside one BlockCompressor (the capacity of
 * TagStats::fields) advances in chunk order, as with `dsrc c -t1`. */
int dsrcgpu_compress_batch(dsrcgpu_handle* h, uint32_t n, const uint8_t* const* fastq, const uint64_t* sizes,
						   uint8_t* blocks, uint64_t blocks_cap, uint64_t* block_offs, uint64_t* block_sizes,
						   uint64_t* raw_sizes, uint64_t* comp_sizes);

/* Device-resident variant: d_fastq is a HIP device pointer; chunk i is [offs[i], offs[i]+sizes[i]).
 * d_blocks (device, blocks_cap bytes) receives the blocks back to back.  No host<->device
 * payload copies happen inside this call; it is what bench.py times. */
int dsrcgpu_compress_batch_device(dsrcgpu_handle* h, uint32_t n, const void* d_fastq, const uint64_t* offs,
								  const uint64_t* sizes, void* d_blocks, uint64_t blocks_cap,
								  uint64_t* block_offs, uint64_t* block_sizes,
								  uint64_t* raw_sizes, uint64_t* comp_sizes);

/* Scheduler lanes inside a handle (round 6).  The reference needs one DsrcCompressorMT for a file (src/DsrcOperator.cpp:295-340);
 * a batch call on ONE handle now fills the GPU by itself: a batch of more than one sub-batch's worth of chunks is cut into
 * consecutive sub-batches (default: about 1.9 GB of chunks each) that run on up to `lanes` (default 4) scheduler lanes inside the
 * handle -- own arena and streams each, one host thread per lane for the duration of the call -- so that the serial range coder
 * of one sub-batch runs beside the front ends of the others.  The block-to-block state goes from sub-batch to sub-batch through an
 * internal chain: the blocks, their order and the state left behind are those of the same call on one lane.  HBM: an arena per
 * lane, sized for a sub-batch (about 7.5 x its chunks + 1.75 GiB), instead of one sized for the batch.
 * dsrcgpu_set_lanes(h, lanes, sub_batch_chunks): 0 = the default for either; lanes = 1 keeps a batch on the handle's own lane.
 * A handle that has been given a chain (dsrcgpu_set_chain) or a fixed arena (dsrcgpu_create's arena_bytes) is the caller's own
 * lane and is never cut; nor are the batches of the queue form's lanes. */
int dsrcgpu_set_lanes(dsrcgpu_handle* h, uint32_t lanes, uint32_t sub_batch_chunks);

/* ---- decompression -------------------------------------------------------------------------------------------------
 * Replaces one call of BlockCompressor::Read (src/BlockCompressor.cpp:262-297) inside DsrcDecompressor::Process
 * (src/DsrcWorker.cpp:75-104): block bytes -> the FASTQ text of the chunk, every line (also the last) ended by '\n'.
 * The handle's settings and dataset must be the archive's (DsrcFileFooter, src/DsrcFile.cpp:142-170); a block that does
 * not end exactly where its last stream ends is refused (DSRCGPU_E_INPUT), as are blocks the reference's own decoder
 * cannot read back deterministically (colour space without a constant primer; streams that run off the end of the block).
 * crc_ok (may be NULL): per block, 1 if the checksum words stored with calculate_crc32 equal the checksums of the
 * decoded records, 0 otherwise -- BlockCompressor::VerifyChecksum (src/BlockCompressor.cpp:576-594), which the
 * reference's compressing worker runs on every block it has just written (src/DsrcWorker.cpp:53-62); without
 * calculate_crc32 every entry is 1.
 * text_caps (may be NULL): text bytes to reserve per block instead of the chunkSize word + 1; needed for archives written
 * by the record-level API, whose chunkSize words are running totals (see dsrcgpu_set_record_layout).
 * n blocks in one scheduler pass; texts are laid out back to back in block order (text_offs / text_sizes). */
int dsrcgpu_decompress_block(dsrcgpu_handle* h, const uint8_t* block, uint64_t size,
							 uint8_t* text, uint64_t text_cap, uint64_t* text_size, uint32_t* crc_ok);
int dsrcgpu_decompress_batch(dsrcgpu_handle* h, uint32_t n, const uint8_t* const* blocks, const uint64_t* sizes,
							 const uint64_t* text_caps, uint8_t* text, uint64_t text_cap,
							 uint64_t* text_offs, uint64_t* text_sizes, uint32_t* crc_ok);
/* Device-resident variant (block i is d_blocks[offs[i] .. offs[i] + sizes[i])); no payload copies inside the call. */
int dsrcgpu_decompress_batch_device(dsrcgpu_handle* h, uint32_t n, const void* d_blocks, const uint64_t* offs,
									const uint64_t* sizes, const uint64_t* text_caps, void* d_text, uint64_t text_cap,
									uint64_t* text_offs, uint64_t* text_sizes, uint32_t* crc_ok);

/* Columnar decode: the records of the batch as arrays in HBM instead of text (no counterpart in the reference, whose readers get
 * text and look for the line ends again -- DsrcArchive::ReadNextRecord).  The blocks are decoded exactly as by
 * dsrcgpu_decompress_batch_device (the text lives in the handle's arena for the duration of the call); two more kernels then
 * gather bases, qualities and titles of all records, in block order and inside a block in record order, into the caller's arrays:
 *   d_seq_offs[r] .. d_seq_offs[r + 1]      record r's positions in d_bases and d_quals       (r = 0 .. totals[0] - 1)
 *   d_title_offs[r] .. d_title_offs[r + 1]  record r's title in d_titles
 * Offsets are 64-bit and global to the call: d_seq_offs[totals[0]] == totals[1], d_title_offs[totals[0]] == totals[2].
 * block_records (n + 1 entries, host): exclusive prefix of the records per block; totals (host): records, bases, title bytes.
 * Any capacity too small: DSRCGPU_E_CAPACITY, totals[] = what is needed, none of the caller's arrays is written (the check is made
 * on the host before the gathering kernel is launched) -- a call with capacities of 0 is the way to size the arrays.
 * n == 0: DSRCGPU_OK, totals 0, block_records[0] = 0.  text_caps, crc_ok and block errors: as dsrcgpu_decompress_batch_device.
 * Base space only: a handle whose dataset has color_space set gets DSRCGPU_E_ARG (a SOLiD line is a primer plus colours, not
 * bases; there is no column form of it). */
typedef struct dsrcgpu_columns      /* all pointers are device pointers owned by the caller */
{
	uint8_t*  d_bases;       uint64_t bases_cap;    /* one byte per base, records back to back: index of the character in
	                                                   "ACGTNRWSKMDVHBYXU.-" (A0 C1 G2 T3 N4 ... '-'18); 255 = any other byte */
	uint8_t*  d_quals;       uint64_t quals_cap;    /* one byte per base, same positions: quality character - quality_offset */
	uint8_t*  d_titles;      uint64_t titles_cap;   /* title lines back to back as decoded ('@' included, no newline); may be NULL
	                                                   with titles_cap 0 = titles not wanted, d_title_offs then ignored */
	uint64_t* d_seq_offs;                           /* records_cap + 1 entries: record r's bases/qualities are [offs[r], offs[r+1]) */
	uint64_t* d_title_offs;                         /* records_cap + 1 entries */
	uint64_t  records_cap;
} dsrcgpu_columns;

int dsrcgpu_decompress_batch_columns_device(dsrcgpu_handle* h, uint32_t n, const void* d_blocks, const uint64_t* offs,
		const uint64_t* sizes, const uint64_t* text_caps, const dsrcgpu_columns* out,
		uint64_t* block_records /* n + 1: exclusive prefix of records per block */,
		uint64_t totals[3]      /* records, bases, title bytes */, uint32_t* crc_ok);

/* Columnar encode: the way back -- record arrays in HBM become DSRC blocks without the caller writing FASTQ text (no counterpart in
 * the reference, whose writers take text or one record at a time: DsrcArchive::WriteNextRecord).  The arrays have the form
 * dsrcgpu_decompress_batch_columns_device leaves behind; they are only read.  Block i holds records block_records[i] ..
 * block_records[i + 1] - 1 and is bit-identical to the block dsrcgpu_compress_batch_device writes on the same handle for the chunk
 * text of those records:  title \n letters \n plus \n qualities+quality_offset,  records joined by \n, no newline after the last;
 * plus is "+", or "+" and the title without its '@' when the handle's dataset has plus_repetition.  That text is assembled in the
 * handle's arena and goes through the same scheduler pass: raw_sizes / comp_sizes, the block-to-block state, tag_preserve_flags,
 * calculate_crc32, verify_after_compress, chains and the codes for text the coder refuses are those of the text call (a read of
 * length 0 gives empty lines, and whatever the text call answers to them).
 * Offsets are relative to d_bases / d_titles as given and need not start at 0: d_seq_offs + k and d_title_offs + k of a decoded
 * batch, with n_records reduced, compress a sub-range without a copy.
 * A check pass on the device runs before any text is written and refuses, with DSRCGPU_E_INPUT, the lowest record index and the
 * reason in dsrcgpu_last_error and d_blocks untouched: offsets out of order, a closing entry above bases_len / titles_len, a base code
 * above 18, a quality q with q + quality_offset > 126, a title that is empty, does not start with '@' or contains '\n'.  No input
 * makes a kernel read or write outside the caller's arrays.
 * DSRCGPU_E_ARG: block_records not starting at 0, not strictly increasing (a block without records) or not ending at n_records; a
 * block whose text reaches 2^31 bytes; a colour-space handle; a pending dsrcgpu_set_record_layout (the archive API's: it has no
 * meaning here and is dropped by this call).  n == 0: DSRCGPU_OK.
 * The call stays on the handle's own scheduler lane: it is never cut into sub-batches (dsrcgpu_set_lanes does not apply).  HBM: the
 * arena of the text call for the same chunks plus the text itself. */
typedef struct dsrcgpu_columns_in   /* device pointers owned by the caller, read only */
{
	const uint8_t*  d_bases;   uint64_t bases_len;    /* codes 0..18 = index in "ACGTNRWSKMDVHBYXU.-" (as dsrcgpu_columns) */
	const uint8_t*  d_quals;                          /* quality character - quality_offset, same positions */
	const uint8_t*  d_titles;  uint64_t titles_len;   /* title lines back to back, '@' included, no newline */
	const uint64_t* d_seq_offs;                       /* n_records + 1 entries */
	const uint64_t* d_title_offs;                     /* n_records + 1 entries */
	uint64_t        n_records;
} dsrcgpu_columns_in;

int dsrcgpu_compress_columns_device(dsrcgpu_handle* h, uint32_t n, const dsrcgpu_columns_in* in,
		const uint64_t* block_records /* n + 1, host: exclusive prefix, [n] == in->n_records */,
		void* d_blocks, uint64_t blocks_cap, uint64_t* block_offs, uint64_t* block_sizes,
		uint64_t* raw_sizes, uint64_t* comp_sizes);

/* The cut a caller of the function above needs, because text sizes cannot be read off the arrays: greedily, each block takes as many
 * consecutive records as keep its chunk text at or below chunk_bytes, and at least one.  The offset arrays stay on the device (a
 * 64-way search per block).  block_records has room for `cap` entries; n blocks need n + 1 (the exclusive prefix, [n] ==
 * n_records).  Too few: DSRCGPU_E_CAPACITY, *n = the number of blocks, nothing written.  Offsets out of order or a closing entry above
 * bases_len / titles_len: DSRCGPU_E_INPUT.  chunk_bytes == 0 or a colour-space handle: DSRCGPU_E_ARG.  No records: *n = 0,
 * block_records[0] = 0.  d_bases, d_quals and d_titles are not read. */
int dsrcgpu_columns_cut(dsrcgpu_handle* h, const dsrcgpu_columns_in* in, uint64_t chunk_bytes,
		uint64_t* block_records, uint32_t cap /* entries */, uint32_t* n /* blocks */);

/* Columnar select: what runs between the two calls above -- a quality trim / read filter that plans, and a ragged compaction that
 * carries the plan (or any plan of the caller's) out, both in HBM (no counterpart in the reference, whose readers hand out text one
 * record at a time).  Both calls only read `in`; offsets are relative to the arrays as given and need not start at 0 (d_seq_offs + k
 * works as above).  Both run on the handle's own scheduler lane and stream, take their scratch (a few words per record) from the
 * handle's arena and synchronise before they return.  Neither reads, changes or consumes codec state: the fields capacity and a
 * pending dsrcgpu_set_record_layout are after the call what they were before it.  A colour-space handle: DSRCGPU_E_ARG.
 *
 * dsrcgpu_columns_trim_plan: per record the range [begin, end) of positions in d_bases / d_quals that survives trimming,
 * S[r] <= begin <= end <= S[r + 1] with S = d_seq_offs, and whether the record is kept.  d_titles and d_title_offs are not read and
 * may be NULL.  Trimming is the running-sum ("BWA") rule on d_quals (Phred values: the quality offset is already gone), each end
 * computed by itself on the whole read.  5' end with cutoff c: s = 0; for i = 0, 1, ...: s += c - q[i]; stop at the first s < 0; start
 * = i + 1 for the first i at which s reached its maximum above 0 (else 0).  3' end: the same from the last base backwards, stop = that
 * i (else the length).  start >= stop: the range is empty, begin = end = S[r].  A record is kept iff, in this order, it has at least
 * min_length bases in the range, at most max_n of them with a code >= 4, and a quality sum of at least min_mean_quality * length; the
 * first rule that fails is the one counted in stats.
 * stats (host): records kept, bases kept, bases cut off kept records, records dropped for length, for N, for mean quality.
 * n_records == 0: DSRCGPU_OK, stats 0.  d_seq_offs out of order or a closing entry above bases_len: DSRCGPU_E_INPUT, the lowest record
 * and the reason in dsrcgpu_last_error, nothing written.  A cutoff above 255 or a non-zero reserved field: DSRCGPU_E_ARG.  No input
 * makes a kernel read outside the caller's arrays. */
typedef struct dsrcgpu_trim_rules
{
	uint32_t quality_5, quality_3;   /* Phred cutoffs for the 5' / 3' end, 0 = that end is not trimmed; > 255: DSRCGPU_E_ARG */
	uint32_t min_length;             /* keep a record iff it has at least this many bases after trimming */
	uint32_t max_n;                  /* ... and at most this many bases with code >= 4 (anything but A C G T, 255 included) in the kept
	                                    range; 0xFFFFFFFF = no limit */
	uint32_t min_mean_quality;       /* ... and sum(q over the kept range) >= min_mean_quality * kept length; 0 = off */
	uint32_t reserved[3];            /* must be 0, else DSRCGPU_E_ARG */
} dsrcgpu_trim_rules;

int dsrcgpu_columns_trim_plan(dsrcgpu_handle* h, const dsrcgpu_columns_in* in, const dsrcgpu_trim_rules* rules,
		uint64_t* d_begin, uint64_t* d_end   /* device, n_records each */,
		uint8_t* d_keep                      /* device, n_records: 1 / 0 */,
		uint64_t stats[6]);

/* dsrcgpu_columns_select_device: the records with a non-zero d_keep byte (NULL = all), in input order, bases and qualities cut to
 * [d_begin[r], d_end[r]) (both NULL = whole reads), titles whole, compacted into `out` with offsets from 0: out->d_seq_offs and
 * out->d_title_offs get kept + 1 entries.  d_source (device, may be NULL) gets the index in `in` of each kept record.  totals (host):
 * records kept, bases kept, title bytes kept.
 * Capacities as in dsrcgpu_decompress_batch_columns_device: any too small: DSRCGPU_E_CAPACITY, totals = what is needed, none of the
 * caller's arrays written (the totals come home before the first writing kernel is launched); a call with capacities of 0 sizes the
 * arrays.  out->d_titles == NULL with titles_cap 0: titles are not wanted, totals[2] is 0, in->d_titles and in->d_title_offs may be NULL
 * (so a sizing call that wants the title total passes a non-null d_titles with titles_cap 0).
 * DSRCGPU_E_INPUT (lowest record and reason in dsrcgpu_last_error, outputs untouched), for kept and dropped records alike: offsets out of
 * order, a closing entry above bases_len / titles_len, d_begin[r] < S[r], d_end[r] > S[r + 1], d_begin[r] > d_end[r].
 * Nothing kept, or n_records == 0: DSRCGPU_OK, totals 0, offs[0] = 0.
 * The arrays of `in`, d_begin, d_end, d_keep on one side and the arrays of `out`, d_source on the other must not overlap; this is not
 * checked. */
int dsrcgpu_columns_select_device(dsrcgpu_handle* h, const dsrcgpu_columns_in* in,
		const uint64_t* d_begin, const uint64_t* d_end, const uint8_t* d_keep,
		const dsrcgpu_columns* out, uint64_t* d_source, uint64_t totals[3]);

/* dsrcgpu_columns_adapter_plan: the second planner -- a 3' adapter search that takes a plan in and gives a narrower plan out, for
 * dsrcgpu_columns_select_device to carry out.  Conventions as dsrcgpu_columns_trim_plan: the handle's own lane and stream, scratch
 * from the arena, synchronised before it returns, codec state (fields capacity, a pending record layout) left alone, a colour-space
 * handle: DSRCGPU_E_ARG.  Of `in` only d_bases and d_seq_offs are read; d_quals, d_titles and d_title_offs may be NULL.
 * The plan in: d_begin_in / d_end_in (both NULL = whole reads, one without the other: DSRCGPU_E_ARG) and d_keep_in (NULL = every
 * record; any non-zero byte keeps).  For record r with b = d_begin_in[r], e = d_end_in[r], n = e - b, x[i] = d_bases[b + i]:
 *   for p = 0 .. n - 1, for a = 0 .. n_adapters - 1:           (the leftmost start position wins, at one p the lowest adapter index)
 *     L = min(adapter_len[a], n - p)                           (the adapter may hang over the 3' end of the RANGE)
 *     if L < min_overlap: next a
 *     mm = the number of j < L with x[p + j] != adapters[a][j]  (a read code >= 4 -- N .. 255 -- matches nothing)
 *     if mm * 1000 <= L * max_error_permille: found (p, a), stop
 * Found: d_end[r] = b + p, d_which[r] = a; not found: d_end[r] = e, d_which[r] = 0xFFFFFFFF; d_begin[r] = b always; d_keep[r] = 1 iff
 * the record came in kept and d_end[r] - d_begin[r] >= min_length, else 0.  A record that came in dropped is not searched: its range
 * passes through, d_keep[r] = 0, d_which[r] = 0xFFFFFFFF, and it counts in no statistic.  Positions at or beyond e are outside the read
 * whatever the array holds there (the next record, or a tail an earlier plan has cut).  d_which may be NULL.
 * Not done here: indels, 5' and anchored adapters, IUPAC wildcards in the adapter, "best match" instead of leftmost.
 * (Poly-G tails and other poly-X ends: dsrcgpu_columns_complexity_plan.  Paired-end overlap detection: dsrcgpu_columns_pair_plan.  Both below.)
 * stats (host): [0] records kept, [1] bases kept, [2] bases this call cut off kept records, [3] records in which an adapter was found
 * (among those that came in kept), [4] records dropped for length, [5 + a] records in which adapter a was the one found.
 * n_records == 0: DSRCGPU_OK, stats 0.
 * DSRCGPU_E_ARG, nothing written: n_adapters 0 or above 8; a length of 0 or above 64, or a non-zero length behind n_adapters; an adapter
 * code above 3; min_overlap 0 or above the shortest adapter's length; max_error_permille above 1000; a non-zero reserved field.
 * DSRCGPU_E_INPUT (lowest record and reason in dsrcgpu_last_error, outputs untouched), for kept and dropped records alike: d_seq_offs
 * out of order, a closing entry above bases_len, d_begin_in[r] < S[r], d_end_in[r] > S[r + 1], d_begin_in[r] > d_end_in[r].  No input
 * makes a kernel read outside the caller's arrays.
 * In place: each output array may be the very same pointer as its input counterpart (d_begin == d_begin_in, d_end == d_end_in, d_keep
 * == d_keep_in): a record's three inputs are read before its outputs are written, and no other record's are touched.  In every other
 * way the outputs must not overlap the inputs or the arrays of `in`; this is not checked. */
typedef struct dsrcgpu_adapter_rules
{
	uint32_t n_adapters;            /* 1..8 */
	uint32_t adapter_len[8];        /* 1..64 for the first n_adapters, 0 for the rest */
	uint8_t  adapters[8][64];       /* host memory, base codes 0..3 (A C G T), 5' to 3' */
	uint32_t min_overlap;           /* 1 .. the shortest adapter's length */
	uint32_t max_error_permille;    /* 0..1000: mismatches allowed per 1000 compared bases */
	uint32_t min_length;            /* keep a record iff it has at least this many bases in front of the adapter */
	uint32_t reserved[3];           /* must be 0, else DSRCGPU_E_ARG */
} dsrcgpu_adapter_rules;

int dsrcgpu_columns_adapter_plan(dsrcgpu_handle* h, const dsrcgpu_columns_in* in, const dsrcgpu_adapter_rules* rules,
		const uint64_t* d_begin_in, const uint64_t* d_end_in, const uint8_t* d_keep_in   /* device, may be NULL */,
		uint64_t* d_begin, uint64_t* d_end, uint8_t* d_keep                              /* device, n_records each */,
		uint32_t* d_which                                                                /* device, n_records, may be NULL */,
		uint64_t stats[13]);

/* dsrcgpu_columns_complexity_plan: the sixth planner -- poly-X runs are cut off either end of the range (the poly-G tails of two-colour
 * instruments, poly-A / poly-T of RNA-seq), then what is left is judged for length, for complexity (fastp's measure) and for a windowed
 * DUST score.  Plan in, plan out, for dsrcgpu_columns_select_device to carry out.  Conventions as dsrcgpu_columns_adapter_plan: the
 * handle's own lane and stream, scratch from the arena, synchronised before it returns, codec state left alone, a colour-space handle:
 * DSRCGPU_E_ARG.  Of `in` only d_bases and d_seq_offs are read.  The plan in: d_begin_in / d_end_in (both NULL = whole reads, one
 * without the other: DSRCGPU_E_ARG) and d_keep_in (NULL = every record; any non-zero byte keeps).
 * For record r that came in kept, with b = d_begin_in[r], e = d_end_in[r], n = e - b, x[i] = d_bases[b + i]:
 * The 3' run of base X, for every X in tail_bases (the whole range is walked, there is no early break in the rule):
 *   best = 0, cut = n, m = 0, err = 0
 *   for i = n - 1 down to 0:
 *     if x[i] == X: m += 1  else: err += 1                       (a code >= 4 -- N .. 255 -- is never X)
 *     L = n - i;  score = m - 2 * err                            (signed; cutadapt's poly-A score with the error share a parameter)
 *     if score > best and err * 1000 <= L * poly_max_error_permille:  best = score, cut = i
 *   t_X = n - cut;  if t_X < poly_min_length: t_X = 0
 * Strict > : the shortest run that reaches the highest score wins.  t = the largest t_X (two bases cannot tie above 0: x[n - t] holds one
 * of them), the tail base is that X, DSRCGPU_COMPLEXITY_NONE if t = 0.  The 5' run is the mirror image for every X in head_bases (i from
 * 0 up, L = i + 1, cut = i + 1) and gives hd and the head base.  Each end is searched by itself on the range as it came.  If hd + t >= n
 * the range is empty, d_begin[r] = d_end[r] = b; otherwise d_begin[r] = b + hd, d_end[r] = e - t.  x', n' are what is left.
 * Complexity: d = the number of i < n' - 1 with x'[i] != x'[i + 1] (codes as they are: N equals N); cp = n' >= 2 ? floor(d * 1000 /
 * (n' - 1)) : 1000; the record fails iff n' >= 2 and d * 1000 < min_complexity_permille * (n' - 1).
 * DUST, windowed so that it does not grow with the read: windows of 64 positions start at 0, 32, 64, .. up to and including n' - 64, one
 * more at n' - 64 if that is no multiple of 32; n' < 64: the one window [0, n').  In a window [s, s + w) a triplet starts at i = s ..
 * s + w - 3 and is valid iff x'[i], x'[i + 1], x'[i + 2] are all < 4; its code is 16 x'[i] + 4 x'[i + 1] + x'[i + 2].  With c_t the count
 * of code t, l = sum c_t, S = sum c_t (c_t - 1) / 2:  v = l >= 2 ? floor(10 * S / (l - 1)) : 0  (at most 310).  The record fails iff more
 * than max_dust_windows windows have v > max_dust; dust = the largest v of the record.
 * d_keep[r] = 1 iff, in this order (the first rule that fails is the one counted): n' >= min_length, complexity, DUST.  Both filters judge
 * the range AFTER the cuts.  d_info (may be NULL): d_info[2r] = head base | tail base << 8, d_info[2r + 1] = cp | dust << 16, for every
 * record that came in kept, whichever filters are on.  A record that came in dropped is not examined: its range passes through,
 * d_keep[r] = 0, d_info = {0xFFFF, 0}, and it counts in no statistic.  Positions outside [b, e) are outside the read whatever the array
 * holds there.
 * Not done here: a quality-aware poly rule, masking of low-complexity stretches inside a read, an entropy score, weighted windows
 * (prinseq's mean over windows), a sliding-window quality cut.
 * stats (host): [0] records kept, [1] bases kept, [2] / [3] bases cut off the 5' / 3' ends of kept records (d_begin[r] - b and e -
 * d_end[r], so that [1] + [2] + [3] is what the kept records came with), [4] / [5] records with a head / tail cut among those that came
 * in kept, [6..9] tail cuts by base A C G T, [10..13] head cuts by base A C G T, [14] records dropped for length, [15] for complexity,
 * [16] for DUST, [17..19] 0.
 * n_records == 0: DSRCGPU_OK, stats 0.
 * DSRCGPU_E_ARG, nothing written: tail_bases or head_bases above 15; poly_min_length 0 with a base to search; poly_max_error_permille or
 * min_complexity_permille above 1000; a non-zero reserved field; a half-given range pair.  No base to search and both filters off is
 * legal: a pure length filter.
 * DSRCGPU_E_INPUT (lowest record and reason in dsrcgpu_last_error, outputs untouched), for kept and dropped records alike: the
 * conditions of dsrcgpu_columns_adapter_plan.  No input makes a kernel read outside the caller's arrays.
 * In place: as dsrcgpu_columns_adapter_plan (d_begin == d_begin_in, d_end == d_end_in, d_keep == d_keep_in). */
#define DSRCGPU_COMPLEXITY_NONE 255u
typedef struct dsrcgpu_complexity_rules
{
	uint32_t tail_bases;               /* bit X (A = 1, C = 2, G = 4, T = 8): a 3' run of base X is searched; 0: the 3' end is left alone; > 15: DSRCGPU_E_ARG */
	uint32_t head_bases;               /* the same for the 5' end */
	uint32_t poly_min_length;          /* a run is cut only if it spans at least this many positions; 0 with a mask set: DSRCGPU_E_ARG */
	uint32_t poly_max_error_permille;  /* 0..1000: positions of the run that may hold something else, per 1000 */
	uint32_t min_length;               /* keep a record iff this many bases are left */
	uint32_t min_complexity_permille;  /* 0 = off, ..1000 */
	uint32_t max_dust;                 /* 0xFFFFFFFF = off */
	uint32_t max_dust_windows;         /* a record may have this many windows above max_dust */
	uint32_t reserved[4];              /* must be 0, else DSRCGPU_E_ARG */
} dsrcgpu_complexity_rules;

int dsrcgpu_columns_complexity_plan(dsrcgpu_handle* h, const dsrcgpu_columns_in* in, const dsrcgpu_complexity_rules* rules,
		const uint64_t* d_begin_in, const uint64_t* d_end_in, const uint8_t* d_keep_in   /* device, may be NULL */,
		uint64_t* d_begin, uint64_t* d_end, uint8_t* d_keep                              /* device, n_records each */,
		uint32_t* d_info                                                                 /* device, 2 per record, may be NULL */,
		uint64_t stats[20]);

/* dsrcgpu_columns_demux_plan: the seventh planner -- a sequencing run is a pool of samples, and every record gets the sample whose
 * barcodes lie nearest (Hamming distance) to what the record holds at the barcode positions: inline at the front of the read, or in up
 * to two index read sets (i7 / i5) of equally many records.  Plan in, plan out, plus a class per record for
 * dsrcgpu_columns_partition_device to group by.  Conventions as dsrcgpu_columns_adapter_plan: the handle's own lane and stream, scratch
 * from the arena, synchronised before it returns, codec state left alone, a colour-space handle: DSRCGPU_E_ARG.  Of every set only
 * d_bases and d_seq_offs are read.  The plan in: d_begin_in / d_end_in (both NULL = whole reads, one without the other: DSRCGPU_E_ARG)
 * and d_keep_in (NULL = every record; any non-zero byte keeps).  sources[0] is `in` under the plan, sources[k] is index_sets[k - 1].
 * For record r that came in kept, with b = d_begin_in[r], e = d_end_in[r]:
 *   for slot s: src = slot_source[s]
 *     source 0:  lo = b + slot_offset[s],        limit = e
 *     source k:  lo = S_k[r] + slot_offset[s],   limit = S_k[r + 1]      (S_k = that index set's d_seq_offs)
 *     if lo + slot_len[s] > limit: SHORT                                  (the record is unassigned, reason "short"; no sample is compared)
 *     x_s[j] = bases_src[lo + j]
 *   for a = 0 .. n_samples - 1:
 *     d_s = the number of j < slot_len[s] with x_s[j] != barcode[a][s][j]   (a read code >= 4 -- N .. 255 -- matches nothing)
 *     D[a] = every d_s <= slot_max_mismatches[s] ? sum of d_s : 255
 *   best = min D, at a* = the LOWEST index that holds it;  second = min of D[a] over a != a* (255 if there is none)
 *   assigned iff best <= max_mismatches and second - best >= min_delta
 *   not assigned: reason NO_MATCH if best > max_mismatches, else AMBIGUOUS
 *   d_class[r] = assigned ? a* : n_samples
 *   d_info[r]  = best | second << 8 | reason << 16        (reason 0 assigned, 1 short, 2 no match, 3 ambiguous; short: best = second = 255)
 *   d_begin[r] = assigned && cut ? b + max over the source-0 slots of (slot_offset + slot_len) : b;     d_end[r] = e
 *   d_keep[r]  = (assigned || keep_unassigned) && d_end[r] - d_begin[r] >= min_length
 * A record that came in dropped is not compared: its range passes through, d_keep[r] = 0, d_class[r] = d_info[r] = 0xFFFFFFFF, and it
 * counts nowhere.  Positions at or beyond e are outside the read whatever the array holds there.  d_info may be NULL.
 * d_class_counts (device, n_samples + 1 entries, may be NULL): entry d_class[r] is incremented for every record that came in kept --
 * ADDED to what the array holds, so that the batches of a file sum.
 * Not done here: indels in the barcode, barcodes of different lengths within a slot, IUPAC wildcards, UMIs, quality-aware distances,
 * barcodes at the 3' end of the range, a search for the barcode at more than one offset.
 * stats (host): [0] records kept, [1] bases kept, [2] bases this call cut off kept records, [3] records assigned, [4] records assigned
 * with best == 0, [5] unassigned short, [6] unassigned no match, [7] unassigned ambiguous, [8] records dropped for length (the flag rule
 * passed, the length did not).
 * n_records == 0: DSRCGPU_OK, stats 0.
 * DSRCGPU_E_ARG, nothing written: n_samples 0 or above 1023; n_slots 0 or above 2; n_index_sets above 2; a slot source above
 * n_index_sets; a slot length of 0 or above 64; a non-zero figure of a slot behind n_slots; cut or keep_unassigned above 1; a barcode
 * code above 3; two samples whose barcodes are equal in every slot; max_mismatches above the summed lengths; a non-zero reserved
 * field; a null d_begin, d_end, d_keep or d_class; one range end without the other; an index set whose n_records differs.
 * DSRCGPU_E_INPUT ("dsrcgpu_columns_demux_plan, read N: columns: record ..." in dsrcgpu_last_error, N = 1: `in`, 2 / 3: an index set;
 * outputs untouched), for kept and dropped records alike: d_seq_offs out of order or a closing entry above bases_len in any set, and
 * for `in` d_begin_in[r] < S[r], d_end_in[r] > S[r + 1], d_begin_in[r] > d_end_in[r].  No input makes a kernel read outside the
 * caller's arrays.
 * In place: as dsrcgpu_columns_adapter_plan (d_begin == d_begin_in, d_end == d_end_in, d_keep == d_keep_in). */
#define DSRCGPU_DEMUX_MAX_SAMPLES 1023
#define DSRCGPU_DEMUX_MAX_BARCODE 64
#define DSRCGPU_DEMUX_NO_LIMIT    0xFFFFFFFFu
typedef struct dsrcgpu_demux_rules
{
	uint32_t n_samples;               /* 1 .. 1023 */
	uint32_t n_slots;                 /* 1 .. 2: single or dual barcode */
	uint32_t slot_source[2];          /* index into sources[]: 0 = `in` under the plan (inline barcode), 1.. = an index read set */
	uint32_t slot_offset[2];          /* bases in front of the barcode: from the RANGE's begin (source 0), from the record's first base (others) */
	uint32_t slot_len[2];             /* 1 .. 64 */
	uint32_t slot_max_mismatches[2];  /* per slot; DSRCGPU_DEMUX_NO_LIMIT = only the total counts */
	uint32_t max_mismatches;          /* of the total over the slots */
	uint32_t min_delta;               /* the runner-up's total must lie at least this far above the best; 0: ties go to the lowest index */
	uint32_t cut;                     /* 1: an ASSIGNED record's begin moves behind its inline barcodes */
	uint32_t keep_unassigned;         /* 1: unassigned records stay kept, as class n_samples (bcl2fastq's "Undetermined") */
	uint32_t min_length;
	const uint8_t* barcodes;          /* host: sample a, slot s at barcodes + a * (len0 + len1) + (s ? len0 : 0); codes 0..3 */
	uint32_t reserved[3];             /* must be 0 */
} dsrcgpu_demux_rules;

int dsrcgpu_columns_demux_plan(dsrcgpu_handle* h, const dsrcgpu_columns_in* in,
		const dsrcgpu_columns_in* const* index_sets, uint32_t n_index_sets   /* 0..2; sources 1, 2; same n_records as `in` */,
		const dsrcgpu_demux_rules* rules,
		const uint64_t* d_begin_in, const uint64_t* d_end_in, const uint8_t* d_keep_in   /* device, may be NULL */,
		uint64_t* d_begin, uint64_t* d_end, uint8_t* d_keep                              /* device, n_records each */,
		uint32_t* d_class          /* device, n_records */,
		uint32_t* d_info           /* device, n_records, may be NULL */,
		uint64_t* d_class_counts   /* device, n_samples + 1, may be NULL; ADDED to, so the batches of a file sum */,
		uint64_t stats[9]);

/* dsrcgpu_columns_partition_device: the select that groups.  The records with a non-zero d_keep byte (NULL = all) and d_class[r] <
 * n_classes come out CLASS-MAJOR -- class 0's records, then class 1's, and so on -- and inside a class in their input order; bases and
 * qualities cut to [d_begin[r], d_end[r]) (both NULL = whole reads), titles whole, offsets from 0, the closing entries of
 * out->d_seq_offs / out->d_title_offs written.  d_source (device, may be NULL): d_source[j] = the index in `in` of output record j.
 * class_records (host, n_classes + 1 entries): the exclusive prefix of the records per class -- class c's records are output records
 * class_records[c] .. class_records[c + 1] - 1, a slice of `out` (dsrcgpu_compress_columns_device takes d_seq_offs + k), so that
 * every sample's archive comes out of one compaction.  totals (host): records, bases, title bytes that come out, and [3] the kept
 * records left out because d_class[r] >= n_classes (a planner's unassigned class, when the caller does not want it).
 * The order is computed, not raced for: the same input gives the same output, byte for byte, on every run.
 * As dsrcgpu_columns_select_device: the capacities (any too small: DSRCGPU_E_CAPACITY, totals and class_records = what is needed, none
 * of the caller's arrays written; a call with capacities of 0 sizes the arrays), out->d_titles == NULL with titles_cap 0 for "titles
 * not wanted", DSRCGPU_E_INPUT for kept and dropped records alike, nothing kept or n_records == 0 (DSRCGPU_OK, totals 0, class_records
 * all 0, offs[0] = 0), and the no-overlap rule, which covers d_class as an input.
 * DSRCGPU_E_ARG: n_classes 0 or above 1024; a null d_class or class_records.
 * Scratch: 8 bytes per (class, tile of one workgroup's records) and 16 per record, from the arena.
 * Not done here: more than 1024 classes in one call (partition twice, by the high and the low half of the class). */
int dsrcgpu_columns_partition_device(dsrcgpu_handle* h, const dsrcgpu_columns_in* in,
		const uint64_t* d_begin, const uint64_t* d_end, const uint8_t* d_keep,
		const uint32_t* d_class, uint32_t n_classes   /* 1 .. 1024 */,
		const dsrcgpu_columns* out, uint64_t* d_source,
		uint64_t* class_records   /* host, n_classes + 1: exclusive prefix of the records per class */,
		uint64_t totals[4]        /* records, bases, title bytes that come out; kept records left out because d_class[r] >= n_classes */);

/* dsrcgpu_columns_pair_plan: the third planner, for paired-end data -- two column sets of equally many records, record r of `in2` is
 * the mate of record r of `in1`.  It takes a plan in per side and gives a narrower plan out per side and ONE keep flag per pair, so
 * that two dsrcgpu_columns_select_device calls with that flag keep the two outputs in step.  Read-through is found from the pair
 * itself: where the insert is shorter than the reads, the reverse complement of read 2 overlaps read 1 at a shift that gives the insert
 * size, and the 3' end of each mate is cut where the insert ends -- adapter remnants of any length, no adapter sequence needed.
 * Conventions as dsrcgpu_columns_adapter_plan: the handle's own lane and stream, a few words of the arena, synchronised before it
 * returns, codec state left alone, a colour-space handle: DSRCGPU_E_ARG.  Of each side only d_bases and d_seq_offs are read; d_quals,
 * d_titles and d_title_offs may be NULL.  The plans in: d_begin<s>_in / d_end<s>_in (both NULL = whole reads; one without the other:
 * DSRCGPU_E_ARG; the two sides are independent of each other) and d_keep<s>_in (NULL = every record; any non-zero byte keeps).
 * For pair r, side s in {1, 2}: [b_s, e_s) its range in its own d_bases, S_s its record start, f_s = b_s - S_s (what an earlier plan cut
 * off the 5' end), n_s = e_s - b_s; x[i] = bases1[b1 + i], y[j] = comp(bases2[e2 - 1 - j]) (the reverse complement of read 2's range),
 * comp(c) = 3 - c for codes 0..3 (A C G T); a code >= 4 on either side matches nothing, not even itself.
 *   for d in 0, 1, .., n1 - 1, then -1, -2, .., -(n2 - 1):               (the first accepted d wins; fastp's candidate order)
 *     d >= 0: L = min(n1 - d, n2), compare x[d + i] with y[i]     for i < L
 *     d <  0: L = min(n1, n2 + d), compare x[i]     with y[i - d] for i < L
 *     if L < min_overlap: next d
 *     mm = the number of i < L at which the two differ or either code is >= 4
 *     if mm <= max_mismatches and mm * 1000 <= L * max_error_permille: found d, stop
 * Found: the insert size is I = d + n2 + f1 + f2, the new lengths are n1' = min(n1, I - f1) and n2' = min(n2, I - f2) (d + n2 >= 1 always,
 * so both are at least 1): d_end<s>[r] = b_s + n_s'; d_begin<s>[r] = b_s always; d_insert[r] = I.  Not found: both ranges unchanged,
 * d_insert[r] = 2^64 - 1.  d_insert may be NULL.
 * A pair is searched iff both mates came in kept and n1, n2 <= DSRCGPU_PAIR_MAX_BASES; a pair with a longer range is not searched and
 * counted as such, its ranges pass through and the keep rule still applies to it.  d_keep[r] = 1 iff both mates came in kept and n1' >=
 * min_length and n2' >= min_length.  A pair that came in with a mate dropped passes its ranges through with d_keep[r] = 0; if exactly one
 * mate had been kept it counts in "dropped for the mate", if neither, in nothing.
 * Not done here: indels, a check that the mates' titles agree, interleaved input, the "best" overlap instead of the first accepted one.
 * (Base correction in the overlap and merging the mates into one read: dsrcgpu_columns_merge_device, below, which takes d_insert.)
 * stats (host): [0] pairs kept, [1] / [2] bases kept of read 1 / read 2, [3] / [4] bases this call cut off read 1 / read 2 of kept pairs,
 * [5] pairs in which an overlap was found, [6] of those, pairs in which either range became shorter, [7] pairs dropped for the mate,
 * [8] pairs dropped for length (both mates came in kept), [9] pairs not searched for a range above DSRCGPU_PAIR_MAX_BASES, [10] the sum
 * of I over the pairs of [5].
 * n_records == 0: DSRCGPU_OK, stats 0.
 * DSRCGPU_E_ARG, nothing written: in1->n_records != in2->n_records; min_overlap 0 or above DSRCGPU_PAIR_MAX_BASES; max_error_permille
 * above 1000; a non-zero reserved field; a half-given range pair; a null output other than d_insert.
 * DSRCGPU_E_INPUT (outputs untouched), for kept and dropped records alike: the conditions of dsrcgpu_columns_adapter_plan on either
 * side; dsrcgpu_last_error names the side (read 1 is reported first), the lowest record of that side and the reason.  No input makes a
 * kernel read outside the caller's arrays.
 * In place: each of the four range outputs may be the very pointer of its input counterpart, and d_keep may be d_keep1_in or
 * d_keep2_in: a pair's inputs are all read before any of its outputs are written, and no other pair's are touched.  In every other way
 * the outputs must not overlap the inputs or the arrays of `in1` / `in2`; this is not checked. */
#define DSRCGPU_PAIR_MAX_BASES 1024
typedef struct dsrcgpu_pair_rules
{
	uint32_t min_overlap;           /* 1 .. DSRCGPU_PAIR_MAX_BASES */
	uint32_t max_mismatches;
	uint32_t max_error_permille;    /* 0 .. 1000 */
	uint32_t min_length;
	uint32_t reserved[4];           /* must be 0 */
} dsrcgpu_pair_rules;

int dsrcgpu_columns_pair_plan(dsrcgpu_handle* h, const dsrcgpu_columns_in* in1, const dsrcgpu_columns_in* in2,
		const dsrcgpu_pair_rules* rules,
		const uint64_t* d_begin1_in, const uint64_t* d_end1_in, const uint8_t* d_keep1_in   /* device, may be NULL */,
		const uint64_t* d_begin2_in, const uint64_t* d_end2_in, const uint8_t* d_keep2_in,
		uint64_t* d_begin1, uint64_t* d_end1, uint64_t* d_begin2, uint64_t* d_end2          /* device, n_records each */,
		uint8_t* d_keep                                                                     /* device, n_records: the pair's flag */,
		uint64_t* d_insert                                                                  /* device, n_records, may be NULL */,
		uint64_t stats[11]);

/* dsrcgpu_columns_dedup_plan: the fourth planner -- exact duplicate reads, or exact duplicate pairs, are marked, and the keep flag
 * that comes out leaves one record of every set of equal ones.  It feeds dsrcgpu_columns_select_device, dsrcgpu_columns_profile,
 * dsrcgpu_columns_merge_device and the encoder like any other keep flag.  The first columnar call whose records talk to each other:
 * a device-wide hash table built with returning atomics (dsrc_amd/csrc/k_columns_dedup.h); the result does not depend on the order in
 * which the records reach the table.
 * Conventions as dsrcgpu_columns_pair_plan: the handle's own lane and stream, scratch from the arena (about 28 bytes a record and 16 to
 * 20 a table slot, 2 to 4 slots a record), synchronised before it returns, codec state left alone, a colour-space handle:
 * DSRCGPU_E_ARG.  in2 == NULL: single-end.  With in2, record r of `in2` is the mate of record r of `in1` and a pair is ONE record with
 * a key of two parts.  Of each side only d_bases, d_seq_offs and -- under prefer = 1 -- d_quals are read; d_titles and d_title_offs may
 * be NULL, and so may d_quals under prefer = 0.
 * The plan in: per side d_begin<s> / d_end<s> (both NULL = whole reads; one without the other: DSRCGPU_E_ARG; the two sides are
 * independent of each other) and ONE d_keep_in (NULL = every record; any non-zero byte keeps).  A record is CONSIDERED iff d_keep_in is
 * NULL or d_keep_in[r] != 0.
 * The key of record r: per side s, [b_s, e_s) its range, n_s = e_s - b_s, k_s = key_bases ? min(n_s, key_bases) : n_s; the key is the
 * tuple (k_1, bases1[b_1 .. b_1 + k_1)) and, with two sides, it goes on with (k_2, bases2[b_2 .. b_2 + k_2)).  Two records are
 * duplicates iff their keys are equal, compared as bytes: code 4 equals code 4 and 255 equals 255, the lengths are part of the key (a
 * read is no duplicate of its own prefix), there is no reverse complement and no mismatch tolerance.  A key is EMPTY when it holds no
 * base (k_1 + k_2 == 0); all considered records with an empty key are duplicates of each other.
 * The rank of record r is the pair (q, -r), compared q first: q = 0 under prefer = 0; under prefer = 1, q = min(2^32 - 1, the sum of the
 * qualities at the key positions of both sides).
 *   classes = {}                                                 (key -> the considered records that have it)
 *   for r = 0 .. n_records - 1:
 *     if not considered(r): d_keep[r] = 0, d_dup_of[r] = 2^64 - 1, d_copies[r] = 0, next r
 *     classes[key(r)] += r
 *   for every class C: rep = the member of highest rank       (prefer = 0: the lowest index; prefer = 1: the highest q, lowest index on a tie)
 *     for r in C: d_keep[r] = (r == rep), d_dup_of[r] = rep, d_copies[r] = (r == rep) ? |C| : 0
 * d_dup_of and d_copies may be NULL, each on its own.  d_keep may be the very pointer d_keep_in: a record's incoming flag is read
 * before its outgoing one is written, and no other record's is touched.  In every other way the outputs must not overlap the inputs
 * or the arrays of `in1` / `in2`; this is not checked.
 * Not done here: reverse-complement or mismatch-tolerant duplicates, optical or UMI duplicates, duplicates across calls (every call
 * starts with an empty table), any check of the titles.
 * stats (host): [0] records considered, [1] records kept = the number of classes, [2] records dropped as duplicates ([0] = [1] + [2]),
 * [3] classes of two and more members, [4] the size of the largest class, [5] records that came in dropped, [6] considered records whose
 * key is empty, [7] classes whose representative is not their lowest index (0 under prefer = 0), [8 .. 23] the duplication-level
 * histogram over classes in FastQC's bins: sizes 1, 2, .., 9, 10-49, 50-99, 100-499, 500-999, 1000-4999, 5000-9999, >= 10000; their
 * sum is [1].
 * n_records == 0: DSRCGPU_OK, stats 0.
 * DSRCGPU_E_ARG, nothing written: in2 with another record count than in1; n_records > 2^31 (refused before anything is read); prefer
 * above 1; hash_bits above 64; a non-zero reserved field; a half-given range pair; ranges of side 2 without in2; a null d_keep or stats.
 * DSRCGPU_E_INPUT (outputs untouched), for considered and dropped records alike: the conditions of dsrcgpu_columns_adapter_plan on either
 * side; dsrcgpu_last_error names the side (read 1 is reported first), the lowest record of that side and the reason.  No input makes a
 * kernel read outside the caller's arrays. */
typedef struct dsrcgpu_dedup_rules
{
	uint32_t key_bases;             /* 0 = the whole range, else at most this many leading bases of each side's range */
	uint32_t prefer;                /* 0 = the first record of a class is kept, 1 = the one with the highest quality sum */
	uint32_t hash_bits;             /* a diagnostic: 0 or 64 = the full hash, 1 .. 63 = only that many low bits of it are used.  The
	                                   results never depend on it; few bits make different keys meet in the table (long probes, slow) */
	uint32_t reserved[5];           /* must be 0 */
} dsrcgpu_dedup_rules;

int dsrcgpu_columns_dedup_plan(dsrcgpu_handle* h, const dsrcgpu_columns_in* in1, const dsrcgpu_columns_in* in2   /* may be NULL */,
		const dsrcgpu_dedup_rules* rules,
		const uint64_t* d_begin1, const uint64_t* d_end1, const uint64_t* d_begin2, const uint64_t* d_end2   /* device, may be NULL */,
		const uint8_t* d_keep_in                                                                             /* device, may be NULL */,
		uint8_t* d_keep                                                                                      /* device, n_records: 1 / 0 */,
		uint64_t* d_dup_of, uint64_t* d_copies                                                               /* device, n_records each, may be NULL */,
		uint64_t stats[24]);

/* dsrcgpu_columns_merge_device: what the insert size of the pair plan is for -- the two mates of a short insert become ONE read with
 * a consensus where they overlap (fastp --merge, PEAR, FLASH, BBMerge).  The first columnar call that writes new bases and qualities
 * instead of copying ranges.  It takes the pair plan's outputs -- the ranges, the pair's keep flag and d_insert -- and writes the merged
 * reads into `out` as dsrcgpu_columns_select_device writes its records: in pair order, offsets from 0.  d_merged[r] = 1 iff pair r is in
 * `out`; the caller selects the unmerged mates with keep & !merged.
 * Conventions as dsrcgpu_columns_select_device and dsrcgpu_columns_pair_plan: the handle's own lane and stream, scratch (a few words per
 * pair) from the arena, synchronised before it returns, codec state left alone, a colour-space handle: DSRCGPU_E_ARG.  d_bases, d_quals
 * and d_seq_offs of both sides are read; titles are taken from `in1` only, and only when out->d_titles is wanted: in2's titles may be NULL.
 * The ranges: d_begin<s> / d_end<s> (both NULL = whole reads; one without the other: DSRCGPU_E_ARG; the sides are independent); d_keep
 * (NULL = every pair; any non-zero byte keeps); d_insert is required and is caller data like any other: nothing about it is trusted.
 * For pair r, side s in {1, 2}: [b_s, e_s) its range in its own d_bases, S_s its record start, f_s = b_s - S_s, n_s = e_s - b_s,
 * I = d_insert[r].  In insert coordinates read 1's range lies at [a1, z1) = [f1, f1 + n1), the reverse complement of read 2's range at
 * [a2, z2) = [I - f2 - n2, I - f2).  At insert position p
 *   read 1 gives c1 = bases1[b1 + p - a1],               q1 = quals1[b1 + p - a1]                (a1 <= p < z1)
 *   read 2 gives c2 = COMP[bases2[e2 - 1 - (p - a2)]],   q2 = quals2[e2 - 1 - (p - a2)]          (a2 <= p < z2)
 * COMP over the code alphabet "ACGTNRWSKMDVHBYXU.-" (A<->T, C<->G, R<->Y, K<->M, D<->H, V<->B; N W S X . - themselves; U -> A), a code
 * above 18 is itself:
 *   code   0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15 16 17 18
 *          A  C  G  T  N  R  W  S  K  M  D  V  H  B  Y  X  U  .  -
 *   COMP   3  2  1  0  4 14  6  7  9  8 12 13 10 11  5 15  0 17 18
 * c2 is the code BEHIND the table everywhere below: a U of read 2 is an A, code 0, and counts as one of A C G T.
 *   if d_keep[r] == 0:                                         not merged, stats[7]
 *   else if I == 2^64 - 1:                                     not merged, stats[8]
 *   else if I >= 2^40 or n1 == 0 or n2 == 0 or I < f2 + n2 or f1 + n1 > I:
 *                                                              not merged, stats[9]  (I < f2 + n2: read 2 runs past the start of the
 *                                                              insert, the plan was not narrowed; f1 + n1 > I: read 1 past its end)
 *   else:
 *     V = min(z1, z2) - max(a1, a2)                            (signed: a gap between the ranges is negative)
 *     if V < min_overlap:                                      not merged, stats[10]
 *     else:
 *       mm = the number of p in [max(a1, a2), min(z1, z2)) with c1 != c2 or c1 >= 4 or c2 >= 4
 *       if mm > max_mismatches or mm * 1000 > V * max_error_permille:
 *                                                              not merged, stats[11]
 *       else merged: for p = min(a1, a2) .. max(z1, z2) - 1 the output read gets
 *         p in one range only:                 that read's (c, q)
 *         c1 < 4, c2 < 4, c1 == c2:            (c1, min(q1 + q2, max(quality_cap, q1, q2)))     stats[3]
 *         c1 < 4, c2 < 4, c1 != c2:            q1 >= q2 ? (c1, q1 - q2) : (c2, q2 - q1)         stats[4]  (read 1 wins a tie, quality 0)
 *         exactly one of c1, c2 < 4:           that one with its own quality                    stats[5]
 *         neither < 4:                         (c1, min(q1, q2))                                stats[6]
 *       stats[0] += 1; stats[1] += max(z1, z2) - min(a1, a2); stats[2] += V
 * The merged record's title is read 1's, whole.  d_source (may be NULL) gets the pair index of each output record.
 * stats (host): [0] pairs merged, [1] bases written, [2] the sum of V over merged pairs, [3] .. [6] the overlap positions of merged pairs
 * by case as above, [7] .. [11] pairs not merged by reason as above.  Sums of integers: the result does not depend on the order in which
 * the device takes the pairs.  [3] + [4] + [5] + [6] == [2] and [0] + [7] + .. + [11] == n_records.
 * totals (host): records, bases, title bytes of `out`.  Capacities exactly as in dsrcgpu_columns_select_device: any too small:
 * DSRCGPU_E_CAPACITY, totals = what is needed (stats are filled as well), none of the caller's arrays written, d_merged and d_source
 * included (the totals come home before the first writing kernel is launched); a call with capacities of 0 sizes the arrays.
 * out->d_titles == NULL with titles_cap 0: titles are not wanted, totals[2] is 0.
 * DSRCGPU_E_ARG, nothing written: in1->n_records != in2->n_records; min_overlap 0; max_error_permille above 1000; quality_cap above 255;
 * a non-zero reserved field; a half-given range pair; d_insert, d_merged, rules, totals, stats or out NULL; a NULL d_quals (or d_bases)
 * with bases_len > 0.
 * DSRCGPU_E_INPUT (outputs untouched), for kept and dropped pairs alike: the conditions of dsrcgpu_columns_pair_plan on either side;
 * dsrcgpu_last_error names the side (read 1 is reported first), the lowest record of that side and the reason.  With titles wanted,
 * in1's title offsets out of order or above titles_len as well, as in dsrcgpu_columns_select_device.
 * Nothing merged, or n_records == 0: DSRCGPU_OK, totals 0, offs[0] = 0, d_merged all 0.
 * The arrays of `in1` / `in2`, the ranges, d_keep and d_insert on one side and the arrays of `out`, d_merged and d_source on the other
 * must not overlap; this is not checked.  No input makes a kernel read or write outside the caller's arrays: a pair's offsets, ranges
 * and geometry are tested before a byte of it is read.
 * Not done here: indels, a new search (d_insert is taken as given), a title suffix such as fastp's merged_x_y, a check that the mates'
 * titles agree, writing the unmerged mates (two selects with keep & !merged), interleaved input. */
typedef struct dsrcgpu_merge_rules
{
	uint32_t min_overlap;           /* >= 1 */
	uint32_t max_mismatches;
	uint32_t max_error_permille;    /* 0 .. 1000 */
	uint32_t quality_cap;           /* 0 .. 255: ceiling of a summed quality */
	uint32_t reserved[4];           /* must be 0 */
} dsrcgpu_merge_rules;

int dsrcgpu_columns_merge_device(dsrcgpu_handle* h, const dsrcgpu_columns_in* in1, const dsrcgpu_columns_in* in2,
		const dsrcgpu_merge_rules* rules,
		const uint64_t* d_begin1, const uint64_t* d_end1   /* device, both NULL = whole reads */,
		const uint64_t* d_begin2, const uint64_t* d_end2,
		const uint8_t* d_keep                              /* device, NULL = every pair */,
		const uint64_t* d_insert                           /* device, required: as dsrcgpu_columns_pair_plan wrote it */,
		const dsrcgpu_columns* out                         /* merged reads, capacities as in dsrcgpu_columns_select_device */,
		uint8_t* d_merged                                  /* device, n_records: 1 = this pair is in `out`; required */,
		uint64_t* d_source                                 /* device, may be NULL: pair index of each output record */,
		uint64_t totals[3], uint64_t stats[12]);

/* dsrcgpu_columns_profile: the per-cycle quality report of the records of `in` under a plan -- what one reads to choose quality_3,
 * min_length and the adapters, and to see what a filter did: the profile with no plan is "before", the profile of the same columns
 * with the final plan is "after", and it needs no select.  Conventions as dsrcgpu_columns_adapter_plan: the handle's own lane and
 * stream, scratch (one profile) from the arena, synchronised before it returns, codec state (fields capacity, a pending record layout)
 * left alone, a colour-space handle: DSRCGPU_E_ARG.  Of `in`, d_bases, d_quals and d_seq_offs are read; d_titles and d_title_offs may
 * be NULL.  The plan, as the planners give it: d_begin / d_end (both NULL = whole reads, one without the other: DSRCGPU_E_ARG) and
 * d_keep (NULL = every record; any non-zero byte profiles the record; a record with a zero byte counts in nothing).
 * With C = n_cycles, for every profiled record r with b = d_begin[r], e = d_end[r]:
 *   n = e - b; qs = g = a = 0
 *   for i = 0 .. n - 1:
 *     x = d_bases[b + i]; q = d_quals[b + i]
 *     k = x < 4 ? x : 4                           (the class: A, C, G, T or anything else)
 *     c = min(i, C - 1)                           (the cycle is the position IN THE RANGE, not in the stored read; positions from C - 1
 *                                                  on fold into the last cycle, so that every sum is conserved)
 *     base[c][k] += 1; qsum[c][k] += q; qhist[q] += 1
 *     tot[1] += 1; if q >= 20: tot[2] += 1; if q >= 30: tot[3] += 1; tot[4] += q
 *     qs += q; if x == 1 or x == 2: g += 1, tot[5] += 1; if x < 4: a += 1, else tot[6] += 1
 *   tot[0] += 1; len[min(n, C)] += 1
 *   if a > 0: gc[100 * g / a] += 1                (integer division; a record without A C G T counts in no GC bin)
 *   if n > 0: meanq[qs / n] += 1, else tot[7] += 1
 * Positions at or beyond e are outside the read whatever the array holds there (the next record, or a tail a plan has cut).
 * d_profile, in uint64 words (DSRCGPU_PROFILE_WORDS(C) of them):
 *   0          tot[8]      [0] records profiled, [1] bases, [2] bases with q >= 20, [3] with q >= 30, [4] quality sum, [5] G or C bases,
 *                          [6] bases of class 4, [7] profiled records with n = 0
 *   8          base[C][5]
 *   8 + 5C     qsum[C][5]
 *   8 + 10C    qhist[256]
 *   264 + 10C  len[C + 1]
 *   265 + 11C  gc[101]
 *   366 + 11C  meanq[256]
 * accumulate == 0: d_profile is overwritten; 1: this call's counts are added to what it holds, so that the calls over the batches of a
 * file give what one call on all of it gives.  totals (host) is this call's own tot[8] either way.  Everything is an integer sum: the
 * result does not depend on the order in which the device takes the records and is bit-reproducible; no counter wraps below 2^64.
 * n_records == 0: DSRCGPU_OK, totals 0, d_profile zeroed if accumulate == 0 and untouched otherwise.
 * Not done here: k-mer counts and over-represented k-mers (dsrcgpu_columns_kmer_count below takes the same plan), a duplication
 * estimate (dsrcgpu_columns_dedup_plan has the duplication levels), over-represented
 * whole sequences, per-tile quality (nothing here reads the titles),
 * a per-cycle quality HISTOGRAM (per cycle there is the sum and the count, so the mean, not the quartiles).
 * On any error d_profile is untouched.  DSRCGPU_E_ARG: n_cycles 0 or above DSRCGPU_PROFILE_MAX_CYCLES; accumulate above 1; a non-zero
 * reserved field; a half-given range pair; a null d_profile, rules or totals; a null in->d_quals (or d_bases) with bases_len > 0.
 * DSRCGPU_E_INPUT (lowest record and reason in dsrcgpu_last_error), for kept and dropped records alike, exactly as
 * dsrcgpu_columns_adapter_plan: d_seq_offs out of order, a closing entry above bases_len, d_begin[r] < S[r], d_end[r] > S[r + 1],
 * d_begin[r] > d_end[r].  No input makes a kernel read outside the caller's arrays.  d_profile must not overlap the inputs. */
#define DSRCGPU_PROFILE_MAX_CYCLES 1024
#define DSRCGPU_PROFILE_WORDS(C) (11ull * (C) + 622)     /* uint64 words of a profile of C cycles */
typedef struct dsrcgpu_profile_rules
{
	uint32_t n_cycles;      /* C: 1 .. DSRCGPU_PROFILE_MAX_CYCLES */
	uint32_t accumulate;    /* 0: d_profile is overwritten; 1: this call's counts are ADDED to what d_profile holds */
	uint32_t reserved[6];   /* must be 0 */
} dsrcgpu_profile_rules;

int dsrcgpu_columns_profile(dsrcgpu_handle* h, const dsrcgpu_columns_in* in,
		const uint64_t* d_begin, const uint64_t* d_end, const uint8_t* d_keep   /* device, may be NULL: the plan, as the planners give it */,
		const dsrcgpu_profile_rules* rules,
		uint64_t* d_profile   /* device, DSRCGPU_PROFILE_WORDS(n_cycles) words */,
		uint64_t totals[8]    /* host: this call's own contribution, whatever accumulate is */);

/* dsrcgpu_columns_kmer_count: the canonical k-mer table of the records of `in` under a plan -- what the k-mer spectrum (genome size,
 * error rate), over-represented k-mers and contaminant screens are read from.  Conventions as dsrcgpu_columns_profile: the handle's
 * own lane and stream, a few words of scratch from the arena, synchronised before it returns, codec state left alone, a colour-space
 * handle: DSRCGPU_E_ARG.  Of `in`, d_bases and d_seq_offs are read; everything else may be NULL.  The plan, as the planners give it:
 * d_begin / d_end (both NULL = whole reads, one without the other: DSRCGPU_E_ARG) and d_keep (NULL = every record; any non-zero byte
 * considers the record).
 * Packing.  Base codes are those of dsrcgpu_columns_in: A C G T = 0 1 2 3; every other code (N, IUPAC, U = 16, 255) is NOT a base.  A
 * k-mer, k in 1 .. DSRCGPU_KMER_MAX_K, is the 2k-bit integer of k consecutive bases of a record's RANGE, first base most significant.
 * Its reverse complement reverses the order and takes 3 - code of each base.  canonical = 1: the key is the numeric minimum of the
 * two; canonical = 0: the forward value.  k <= 31 leaves the all-ones word free as the EMPTY mark.
 *   for r = 0 .. n_records - 1:
 *     if d_keep and d_keep[r] == 0: stats[1] += 1, next r
 *     stats[0] += 1; b = d_begin[r]; e = d_end[r]
 *     if e - b < k: stats[2] += 1, next r
 *     for p = b .. e - k:                                           (e - b - k + 1 windows)
 *       stats[3] += 1
 *       if any of d_bases[p .. p + k) is above 3: stats[5] += 1     (a BROKEN window adds nothing)
 *       else: key = canonical ? min(fwd, rc) : fwd; count[key] += 1
 * Records of the second mate are a second call with accumulate = 1; there is no pair rule.
 * The table is ONE caller-owned array of DSRCGPU_KMER_WORDS(M) = 8 + 2 M uint64 words in HBM, M = rules->capacity a power of two in
 * 16 .. 2^40:
 *   [0] 0x4B4D4552 << 32 | (hash_bits mod 64) << 16 | k << 8 | canonical   [1] M   [2] distinct keys   [3] occurrences counted
 *   [4] occurrences lost to overflow over the table's life   [5 .. 7] 0
 *   8       keys[M]     EMPTY = all ones
 *   8 + M   counts[M]
 * Slot order is unspecified: it depends on the order in which the device takes the windows.  The header and the SET of (key, count)
 * pairs do not, and they are what two runs, or a run and the loop above, agree on bit for bit.  The header is kept up to date on the
 * device by the library's kernels; a caller reads it and never writes it.
 * accumulate == 0: the table is initialised (empty) first; 1: the header must match k, canonical, hash_bits and capacity, else
 * DSRCGPU_E_ARG with nothing touched, and this call's counts are added.
 * The 3/4 rule: with W = stats[3], the windows of the call (summed by the check pass, before the table is written), a call with
 * distinct_before + W > 3 M / 4 returns DSRCGPU_E_CAPACITY with the table untouched and need[0] = the smallest power of two >= 2 *
 * (distinct_before + W), and at least 16.  So the load is at or under 3/4 at every moment of every call.
 * A probe walks at most min(M, DSRCGPU_KMER_PROBE_LIMIT) slots; an occurrence that meets neither its key nor an empty slot in that
 * walk is counted in overflow and dropped.  With the full hash and a load of 3/4 this does not happen; hash_bits can force it.
 * PRESENT MEANS EXACT: slots are never freed, so a key is either in the table with its exact count, or wholly absent with all its
 * occurrences in overflow.  overflow > 0 is no error code: it is a statistic, and header word 4 accumulates it.
 * stats (host), all independent of the order: [0] records considered, [1] records that came in dropped, [2] considered records
 * without a window, [3] windows, [4] k-mers counted, [5] broken windows, [6] keys new to the table, [7] overflow, [8] distinct keys
 * after the call, [9] occurrences in the table after the call, [10 .. 15] 0.  [3] == [4] + [5] + [7].
 * n_records == 0: DSRCGPU_OK; the table is initialised under accumulate = 0 and only checked under 1.
 * Not done here: k above 31, minimizers, per-read annotations (hits, median abundance, contaminant keep flags and the abundance trim
 * are dsrcgpu_columns_kmer_plan below, which reads this table), approximate counting (Bloom filters, count-min), tables that span several GPUs
 * (dsrcgpu_kmer_table_merge sums the tables of ranks), anything that reorders records.
 * On any error the table is untouched.  DSRCGPU_E_ARG: k 0 or above 31; canonical or accumulate above 1; hash_bits above 64; a
 * capacity that is no power of two in 16 .. 2^40; a non-zero reserved field; a half-given range pair; a null d_table, rules, stats
 * or need; under accumulate a header that is no table's or does not match the rules.  DSRCGPU_E_INPUT exactly as
 * dsrcgpu_columns_profile.  No input makes a kernel read outside the caller's arrays or write outside the DSRCGPU_KMER_WORDS(M) words
 * of d_table, which must not overlap the inputs. */
#define DSRCGPU_KMER_MAX_K 31
#define DSRCGPU_KMER_PROBE_LIMIT 1024
#define DSRCGPU_KMER_MAX_BINS 65536
#define DSRCGPU_KMER_WORDS(M) (8ull + 2ull * (M))        /* uint64 words of a table of M slots */
typedef struct dsrcgpu_kmer_rules
{
	uint32_t k;             /* 1 .. DSRCGPU_KMER_MAX_K */
	uint32_t canonical;     /* 1: a k-mer and its reverse complement are one key (the lower word); 0: the forward word */
	uint32_t accumulate;    /* 0: the table is initialised first; 1: this call's counts are ADDED to the table d_table holds */
	uint32_t hash_bits;     /* a diagnostic, as in dsrcgpu_dedup_rules: 0 or 64 = the full hash, 1 .. 63 = that many low bits.  It is part
	                           of the table's header (lookups must walk as the inserts did); no (key, count) pair depends on it unless
	                           it forces overflow */
	uint64_t capacity;      /* M: slots of the table, a power of two in 16 .. 2^40 */
	uint32_t reserved[4];   /* must be 0 */
} dsrcgpu_kmer_rules;

int dsrcgpu_columns_kmer_count(dsrcgpu_handle* h, const dsrcgpu_columns_in* in,
		const uint64_t* d_begin, const uint64_t* d_end, const uint8_t* d_keep   /* device, may be NULL: the plan, as the planners give it */,
		const dsrcgpu_kmer_rules* rules,
		uint64_t* d_table     /* device, DSRCGPU_KMER_WORDS(rules->capacity) words */,
		uint64_t stats[16]    /* host */,
		uint64_t need[1]      /* host: under DSRCGPU_E_CAPACITY the capacity that would do, else 0 */);

/* Every (key, count) of the table d_src is added into the table d_dst; d_src is only read.  The two must hold the same k and
 * canonical and may have any two capacities (and hash_bits): this grows a table (merge into an empty larger one), sums the tables of
 * batches, and sums the tables of ranks.  The 3/4 rule with W = the distinct keys of d_src: distinct(dst) + distinct(src) > 3 M(dst) /
 * 4: DSRCGPU_E_CAPACITY, d_dst untouched, need[0] as above.  Present means exact holds for d_dst as above; a key that cannot be
 * placed adds its whole count to overflow.  d_dst's header word 4 also takes over what d_src had lost.
 * stats (host): [0] keys of d_src, [1] of them new to d_dst, [2] occurrences added, [3] occurrences lost to overflow, [4] distinct
 * keys of d_dst afterwards, [5] its occurrences afterwards, [6 .. 7] 0.
 * DSRCGPU_E_ARG, nothing written: a null argument, d_src == d_dst, a header that is no table's, different k or canonical. */
int dsrcgpu_kmer_table_merge(dsrcgpu_handle* h, const uint64_t* d_src, uint64_t* d_dst, uint64_t stats[8], uint64_t need[1]);

/* The k-mer spectrum: d_hist[c] (device, n_bins uint64 words, overwritten) = the number of distinct keys counted c times; counts
 * >= n_bins - 1 fold into the last bin, d_hist[0] = 0.  totals (host): [0] distinct keys, [1] occurrences, [2] keys counted once,
 * [3] the largest count.  n_bins in 2 .. DSRCGPU_KMER_MAX_BINS, else DSRCGPU_E_ARG; a header that is no table's: DSRCGPU_E_ARG;
 * d_hist is untouched on any error. */
int dsrcgpu_kmer_spectrum(dsrcgpu_handle* h, const uint64_t* d_table, uint32_t n_bins, uint64_t* d_hist, uint64_t totals[4]);

/* d_counts[i] (device, n uint64 words) = the count of the packed k-mer d_kmers[i] (first base most significant), 0 for a key that
 * is not in the table.  Under a canonical table a query is canonicalised first: a k-mer and its reverse complement give the same
 * answer.  A word >= 4^k gets 0 and is counted in *invalid (host).  The walk is the insert's, without a write. */
int dsrcgpu_kmer_lookup(dsrcgpu_handle* h, const uint64_t* d_table, const uint64_t* d_kmers, uint64_t n, uint64_t* d_counts, uint64_t* invalid);

/* dsrcgpu_columns_kmer_plan: the fifth planner -- every window of every considered record is looked up in a table of
 * dsrcgpu_columns_kmer_count, and the record gets a narrowed plan and three annotations.  Two uses: a contaminant screen (count a
 * reference -- PhiX, rRNA, adapter dimers -- into a table, then drop or cut the reads that hit it: BBDuk), and an abundance trim (count
 * the batch itself, then cut every read at its first k-mer seen fewer than min_count times: khmer filter-abund / trim-low-abund).
 * Conventions as dsrcgpu_columns_adapter_plan: the handle's own lane and stream, scratch from the arena (a few words; under want_median
 * also 2 bytes per window of the longest range for every wave in flight, if a range has more than DSRCGPU_KMER_PLAN_LDS_WINDOWS windows),
 * synchronised before it returns, codec state left alone, a colour-space handle: DSRCGPU_E_ARG.  Of `in`, d_bases and d_seq_offs are
 * read; everything else may be NULL.  k and canonical are the table's (its header is read as dsrcgpu_kmer_lookup reads it; a header
 * that is no table's: DSRCGPU_E_ARG); windows, base codes, broken windows and keys are those of dsrcgpu_columns_kmer_count.  The table
 * is ONLY READ: not a word of it is written, no atomic touches it.  The plan in: d_begin_in / d_end_in (both NULL = whole reads, one
 * without the other: DSRCGPU_E_ARG), d_keep_in (NULL = every record; any non-zero byte considers the record).
 *   for r = 0 .. n_records - 1:
 *     b, e = the incoming range (whole read if NULL)
 *     if d_keep_in and d_keep_in[r] == 0:
 *       d_begin[r] = b; d_end[r] = e; d_keep[r] = 0; good = hits = median = 0; stats[1] += 1; next r
 *     stats[0] += 1; n = e - b; W = n >= k ? n - k + 1 : 0; if W == 0: stats[2] += 1
 *     good = hits = 0; first_miss = first_hit = W; C = []
 *     for p = 0 .. W - 1:
 *       if any of d_bases[b + p .. b + p + k) is above 3:      hit = false         (a BROKEN window: no hit, not in the median)
 *       else: good += 1; c = count of key (0 if absent); C += min(c, 65535); hit = c >= min_count
 *       if hit: hits += 1; first_hit = min(first_hit, p)   else: first_miss = min(first_miss, p)
 *     median = want_median and good > 0 ? sorted(C)[good / 2] : 0                   (khmer's median: the upper one of two)
 *     e' = e
 *     if trim == 1 and first_miss < W: e' = b + first_miss + k - 1                  (khmer: the bases in front of the first bad k-mer's last base)
 *     if trim == 2 and first_hit  < W: e' = b + first_hit                           (BBDuk ktrim=r: the k-mer and everything behind it go)
 *     stats[3] += W; stats[4] += good; stats[5] += hits; if hits > 0: stats[7] += 1
 *     if e' < e: stats[8] += 1; stats[9] += e - e'                                  (kept or not)
 *     reason = first that fails of:
 *       [10] min_hits <= hits <= max_hits
 *       [11] W * min_hit_permille <= hits * 1000 <= W * max_hit_permille
 *       [12] min_median <= median <= max_median           (only under want_median)
 *       [13] e' - b >= min_length
 *     d_begin[r] = b; d_end[r] = e'; d_keep[r] = no reason; stats[reason] += 1, or stats[6] += 1 and stats[14] += e' - b
 *     d_good[r] = good; d_hits[r] = hits; d_median[r] = median                      (each only if its array is given)
 * The keep rules judge the range as it CAME: hits, the share of ALL W windows (broken ones included) and the median are taken before the
 * cut; only min_length sees the cut.  A record without a window has 0 hits of 0 windows: it passes [11] whatever the bounds, fails [10]
 * under min_hits > 0 and has median 0.  Screening OUT is max_hits = 0 (or max_hit_permille); screening IN is min_hits.
 * The median is that of the counts CAPPED at DSRCGPU_KMER_PLAN_COUNT_CAP = 65535; min_count sees the raw 64-bit count.
 * A table with overflow (header word 4) reads a key it lost as absent, count 0: present means exact, absent means 0.
 * d_good, d_hits, d_median may be NULL, each on its own (d_median must be NULL under want_median = 0).  Aliasing as
 * dsrcgpu_columns_adapter_plan: a record's incoming plan is read before its outgoing one is written and no other record's is touched,
 * so d_begin may be d_begin_in, d_end d_end_in and d_keep d_keep_in; in every other way the outputs must not overlap the inputs, the
 * table or each other; this is not checked.
 * stats (host): [0] records considered, [1] records that came in dropped, [2] considered records without a window, [3] windows, [4] good
 * windows, [5] hits, [6] records kept, [7] considered records with at least one hit, [8] records trimmed, [9] bases cut, [10] .. [13]
 * records dropped, by reason as in the loop, [14] bases in the ranges of kept records, [15] 0.  [0] == [6] + [10] + [11] + [12] + [13]
 * and [3] >= [4] >= [5].  Sums of integers: the result does not depend on the order in which the device takes the records.
 * n_records == 0: DSRCGPU_OK, stats 0.
 * DSRCGPU_E_ARG, nothing written: min_count 0; a permille above 1000; trim above 2; want_median above 1, or 0 together with a median
 * bound (min_median != 0, max_median != 0xFFFFFFFF) or d_median; a non-zero reserved field; a half-given range pair; a null d_begin,
 * d_end, d_keep, d_table, rules or stats; a header that is no table's.
 * DSRCGPU_E_INPUT (outputs untouched; lowest record and reason in dsrcgpu_last_error), for kept and dropped records alike, exactly as
 * dsrcgpu_columns_adapter_plan: d_seq_offs out of order, a closing entry above bases_len, d_begin_in[r] < S[r], d_end_in[r] > S[r + 1],
 * d_begin_in[r] > d_end_in[r].  No input makes a kernel read outside the caller's arrays and the table's words, or write outside the
 * n_records entries of each output.
 * Not done here: digital normalisation (a read is judged against the counts of the reads kept before it: sequential by nature), a
 * left-side k-trim (ktrim=l), a mismatch-tolerant lookup (BBDuk's hdist / edist), masking (kmask), any pair rule (two calls; the pair
 * plan, or keep1 & keep2, joins the sides). */
#define DSRCGPU_KMER_PLAN_COUNT_CAP 65535
#define DSRCGPU_KMER_PLAN_LDS_WINDOWS 1024                /* ranges of up to this many windows keep their counts on chip under want_median */
typedef struct dsrcgpu_kmer_plan_rules
{
	uint64_t min_count;          /* >= 1: a window HITS iff the table's count of its key is >= min_count */
	uint32_t min_hits, max_hits; /* keep iff min_hits <= hits <= max_hits; 0xFFFFFFFF = no upper limit */
	uint32_t min_hit_permille, max_hit_permille;   /* 0 .. 1000, of ALL the record's windows */
	uint32_t min_median, max_median;               /* of the capped counts of the good windows; 0xFFFFFFFF = no upper limit */
	uint32_t trim;               /* 0 none, 1 at the first window that does not hit, 2 at the first window that hits */
	uint32_t min_length;
	uint32_t want_median;        /* 0: the median is not computed; d_median must be NULL, min_median 0, max_median 0xFFFFFFFF */
	uint32_t reserved[4];        /* must be 0 */
} dsrcgpu_kmer_plan_rules;

int dsrcgpu_columns_kmer_plan(dsrcgpu_handle* h, const dsrcgpu_columns_in* in,
		const dsrcgpu_kmer_plan_rules* rules,
		const uint64_t* d_table                        /* device: a table of dsrcgpu_columns_kmer_count, only read */,
		const uint64_t* d_begin_in, const uint64_t* d_end_in, const uint8_t* d_keep_in   /* device, may be NULL */,
		uint64_t* d_begin, uint64_t* d_end, uint8_t* d_keep                              /* device, n_records each */,
		uint64_t* d_good, uint64_t* d_hits, uint64_t* d_median                           /* device, n_records each, each may be NULL */,
		uint64_t stats[16]);

/* dsrcgpu_columns_kmer_correct: the third thing a k-mer toolkit does with a table -- the reads are REPAIRED against it (Tadpole,
 * Lighter, BFC, Musket, Quake).  A substitution error turns up to k consecutive windows of a read into k-mers the data set has hardly
 * seen; where exactly one replacement of the base those windows share makes every one of them solid, that base is put right.  The
 * second columnar call that writes new bases (dsrcgpu_columns_merge_device was the first) and the first that writes them from evidence
 * outside the record; it closes decode -> dsrcgpu_columns_kmer_count -> correct -> dsrcgpu_compress_columns_device on one device.
 * Conventions as dsrcgpu_columns_kmer_plan: the handle's own lane and stream, scratch from the arena (a few words), synchronised before
 * it returns, codec state left alone, a colour-space handle: DSRCGPU_E_ARG.  Of `in`, d_bases and d_seq_offs are read, and d_quals
 * under max_quality < 255; everything else may be NULL.  Windows, base codes, broken windows, keys, k and canonical are those of
 * dsrcgpu_columns_kmer_count and of the table's header, read as dsrcgpu_columns_kmer_plan reads it.  The table is ONLY READ.  The plan
 * in: d_begin / d_end (both NULL = whole reads, one without the other: DSRCGPU_E_ARG), d_keep (NULL = every record; any non-zero byte
 * considers the record).
 * A window is SOLID iff it holds no code above 3 and its key's count is at least min_count.  S = d_seq_offs, bases = in->d_bases,
 * out = d_bases_out, quals = in->d_quals:
 *   for r = 0 .. n_records - 1:
 *     b, e = the incoming range (whole read if NULL)
 *     out[S[r] .. S[r+1]) = bases[S[r] .. S[r+1])            (see "the output" below)
 *     if d_keep and d_keep[r] == 0: stats[1] += 1; d_fixed[r] = 0; next r
 *     stats[0] += 1; n = e - b; W = n >= k ? n - k + 1 : 0
 *     if W == 0: stats[2] += 1
 *     solid[w] for w = 0 .. W - 1, all taken from the bases AS THEY CAME
 *     stats[3] += W; stats[4] += number of solid windows
 *     if W > 0 and all solid: stats[15] += 1
 *     fixed = 0
 *     for every maximal run [w0, w1] of windows that are not solid, len = w1 - w0 + 1:
 *       stats[5] += 1
 *       if w0 == 0 and w1 == W - 1:   stats[9]  += 1; next run   (no solid window in the range)
 *       if len > k:                   stats[10] += 1; next run   (more than one error)
 *       if w0 == 0:           p = w1                             (the run touches the 5' end)
 *       else if w1 == W - 1:  p = w0 + k - 1                     (the run touches the 3' end)
 *       else if len == k:     p = w1                             (interior: == w0 + k - 1)
 *       else:                 stats[11] += 1; next run           (interior, shorter than k)
 *       if max_quality < 255 and quals[b + p] > max_quality: stats[14] += 1; next run
 *       A = { x in 0..3, x != bases[b + p] :
 *             every window w0 .. w1 is solid once position p reads x }
 *             (3 candidates for a base, 4 for a code above 3)
 *       if |A| == 0: stats[12] += 1; next run
 *       if |A| >= 2: stats[13] += 1; next run
 *       out[b + p] = the one x; fixed += 1; stats[6] += 1
 *       if bases[b + p] > 3: stats[7] += 1
 *     if fixed: stats[8] += 1
 *     d_fixed[r] = fixed                                         (only if the array is given)
 * - Every window that contains p lies inside the run, in all three placements.  So runs do not see each other's repairs, and the
 *   verdicts do not depend on the order of the runs.  A run needs only positions w0 .. w1 + k - 1 of the read, at most 2k - 1 <= 61.
 * - stats[5] == stats[6] + stats[9] + stats[10] + stats[11] + stats[12] + stats[13] + stats[14].
 * - Idempotent: a second call on the output with the same table and rules changes nothing, has stats[6] == 0 and finds stats[5]
 *   smaller by the first call's stats[6] (a repaired run is gone, every other run is as it was).
 * - Qualities are not touched.  A replaced N keeps its quality, and dsrcgpu_compress_columns_device takes that text as the text call
 *   does.
 * - A table with overflow (header word 4) reads a key it lost as absent.
 * Worked examples: k = 3, forward words, the table of the one read ACGTTGCA, min_count = 1.  ACGTAGCA, TCGTTGCA, AGGTTGCA, ACGTTGCC,
 * ACGTNGCA and ACNTTGCA each give ACGTTGCA, one run fixed.  ACGAAGCA is unchanged, counted in [10].  TTT is unchanged, counted in
 * [9].  AC and ACG have no run.  With ACGTCGCA counted into the table as well, ACGTAGCA is unchanged, counted in [13].
 * THE OUTPUT.  d_bases_out is addressed with the offsets of in->d_seq_offs, like in->d_bases.  Out of place: exactly the bytes
 * [S[0], S[n_records]) are written, a copy of the input with the repairs -- records that are dropped, out of range or without windows
 * included; nothing before or behind that span is written.  In place, d_bases_out == in->d_bases: only the repaired positions are
 * written.  Any other overlap with the inputs, the table or d_fixed is not allowed and not checked.  d_fixed (n_records, may be
 * NULL): the repairs of every record, 0 for a record that is not considered.
 * stats (host): [0] records considered, [1] records that came in dropped, [2] considered records without a window, [3] windows, [4]
 * solid windows, [5] runs, [6] bases repaired, [7] of these, codes above 3, [8] records with a repair, [9] .. [14] runs left alone, by
 * reason as in the loop, [15] considered records with windows that are all solid.  Sums of integers: the result does not depend on
 * the order in which the device takes the records.
 * n_records == 0: DSRCGPU_OK, stats 0, nothing written.
 * DSRCGPU_E_ARG, nothing written: min_count 0; max_quality above 255; a non-zero reserved field; a half-given range pair; a null in,
 * rules, d_table, d_bases_out or stats; a null d_quals under max_quality < 255; a header that is no table's.
 * DSRCGPU_E_INPUT (not a byte of d_bases_out or d_fixed changed; lowest record and reason in dsrcgpu_last_error), for kept and dropped
 * records alike, exactly as dsrcgpu_columns_kmer_plan: d_seq_offs out of order, a closing entry above bases_len, d_begin[r] < S[r],
 * d_end[r] > S[r + 1], d_begin[r] > d_end[r].  No input makes a kernel read outside the caller's arrays and the table's words, or
 * write outside [S[0], S[n_records]) of d_bases_out and the n_records entries of d_fixed.
 * Not done: two errors within k of each other, indels, a repair chosen by count among several candidates, more than one pass (the
 * caller can count again and call again), any pair rule, a new quality for a repaired base, masking instead of repairing. */
typedef struct dsrcgpu_kmer_correct_rules
{
	uint64_t min_count;          /* >= 1: a window is SOLID iff it is good and the table's count of its key is >= min_count */
	uint32_t max_quality;        /* 0 .. 255: a base above it is never replaced; 255 = any, and then in->d_quals is not read and may be NULL */
	uint32_t reserved[5];        /* must be 0 */
} dsrcgpu_kmer_correct_rules;

int dsrcgpu_columns_kmer_correct(dsrcgpu_handle* h, const dsrcgpu_columns_in* in, const dsrcgpu_kmer_correct_rules* rules,
		const uint64_t* d_table                        /* device: a table of dsrcgpu_columns_kmer_count, only read */,
		const uint64_t* d_begin, const uint64_t* d_end, const uint8_t* d_keep            /* device, the plan, each may be NULL */,
		uint8_t* d_bases_out                           /* device, addressed like in->d_bases; may be in->d_bases */,
		uint64_t* d_fixed                              /* device, n_records, may be NULL */,
		uint64_t stats[16]);

/* Queue form of DsrcCompressor::Process (src/DsrcWorker.cpp:39-70):
 *   fastqQueue.Pop(partId, chunk)            -> dsrcgpu_submit(partId, chunk)      (bytes are copied into page-locked staging)
 *   ... Store ... dsrcQueue.Push(partId, blk) -> dsrcgpu_collect(&partId, &blk, ...)
 *   dsrcPool.Release(blk)                    -> dsrcgpu_release(blk)
 * Asynchronous: dsrcgpu_flush hands everything submitted since the last flush to the handle's scheduler lanes as one
 * batch and returns; the ring holds as many batches as the handle has scheduler lanes, plus two: one being filled, the others running,
 * waiting or being collected.  When all are busy
 * dsrcgpu_submit returns DSRCGPU_E_BUSY without copying anything (it does not wait: the caller may be the thread that has
 * to collect): take blocks with dsrcgpu_collect, release them, submit again -- a slot is free once every block of the
 * oldest batch has been released.  Blocks come back in submission order:
 * dsrcgpu_collect returns 1 and a block (a pointer into page-locked memory owned by the handle, valid until
 * dsrcgpu_release), waits while a flushed batch is still running, and returns 0 when everything flushed has been
 * collected; dsrcgpu_try_collect never waits (0 = nothing ready right now).  A batch that failed makes the next call
 * return its error.  One submitter thread and one collector thread may use a handle concurrently; the batch calls above
 * must not be mixed in while batches are in flight.  Block-to-block state follows submission order (`dsrc c -t1`).
 * The batches that run at a time run on scheduler lanes inside the handle (round 4: two, round 6: DSRC_GPU_QUEUE_LANES, default 3,
 * at most 4) -- the handle and twins with their own arenas and streams, created at the first flush -- so that the range coder of one
 * batch (~0.08 s on a few CUs, whatever the batch's size) overlaps the copies and the front ends of the next ones; the block-to-block
 * state goes from lane to lane in flush order through an internal chain.  Every lane adds an arena (about 7.5 x a batch's chunks + 1.75
 * GiB) to the handle's HBM; the twins are left out when the caller has given the handle a chain of his own (dsrcgpu_set_chain) or with
 * DSRC_GPU_QUEUE_LANES=1.  dsrcgpu_set_fields_capacity counts before the first flush and between flushes once the queue has drained
 * (DSRCGPU_E_STATE while batches are in flight); dsrcgpu_set_record_layout belongs to whichever comes first, the next flush or the
 * next batch call, and travels with that batch: it may be set for the next flush while earlier batches are still running. */
int dsrcgpu_submit(dsrcgpu_handle* h, int64_t part_id, const uint8_t* fastq, uint64_t size);
/* The same without the copy (round 6): `fastq` is page-locked memory of the caller's (dsrcgpu_host_alloc) and stays as it is until
 * every block of its batch has been collected -- the batch's copy to the device reads it in place.  A submitter that copies 8 MiB chunks
 * into the ring moves ~10 GB/s; the reader threads of a host pipeline can fill page-locked buffers directly instead.  Both forms
 * may be mixed in one batch. */
int dsrcgpu_submit_pinned(dsrcgpu_handle* h, int64_t part_id, const uint8_t* fastq, uint64_t size);
int dsrcgpu_flush(dsrcgpu_handle* h);
int dsrcgpu_collect(dsrcgpu_handle* h, int64_t* part_id, uint8_t** block, uint64_t* block_size,
					uint64_t raw_sizes[4], uint64_t comp_sizes[4]);
int dsrcgpu_try_collect(dsrcgpu_handle* h, int64_t* part_id, uint8_t** block, uint64_t* block_size,
						uint64_t raw_sizes[4], uint64_t comp_sizes[4]);
int dsrcgpu_release(dsrcgpu_handle* h, uint8_t* block);

/* Several handles may compress consecutive batches of ONE archive at the same time (one host thread each); this is
 * what hides the serial range-coder stage.  The only state DSRC carries from block to block -- the capacity of
 * TagStats::fields inside one BlockCompressor (src/TagModeler.h:124) -- is then handed from
 * batch `seq` to batch `seq + 1` through a chain, so the blocks equal those of a single handle fed in order, i.e.
 * `dsrc c -t1`.  dsrcgpu_set_chain(h, chain, seq) declares that the NEXT batch call on h is batch number `seq`
 * (0, 1, 2, ... without gaps across all handles of the chain); that call waits, early in its course, for batch
 * seq - 1 to have published the state.  A batch that fails marks the chain failed and releases the waiters. */
typedef struct dsrcgpu_chain dsrcgpu_chain;
int dsrcgpu_chain_create(dsrcgpu_chain** out);
void dsrcgpu_chain_destroy(dsrcgpu_chain* c);
int dsrcgpu_set_chain(dsrcgpu_handle* h, dsrcgpu_chain* c, uint64_t seq);

/* Sharding one archive over several devices or processes.  Chunk ranges are independent except for the one
 * value above, which after a chunk is a pure function of the value before it and the number of fields in the title of
 * the chunk's first record:  cap' = dsrcgpu_fields_capacity_after(cap, dsrcgpu_title_fields(title, len, flags)).
 * So a shard that starts at chunk k needs only the fold of that function over the first titles of chunks 0..k-1 -- a
 * host-side pass over one line per chunk (or an exclusive scan of one uint32 across ranks, dsrc_amd/dist.py) -- to write
 * exactly the blocks `dsrc c -t1` writes: seed the first handle (or the chain) of the shard with it. */
uint32_t dsrcgpu_title_fields(const uint8_t* title, uint32_t len, uint64_t tag_preserve_flags);
uint32_t dsrcgpu_fields_capacity_after(uint32_t cap, uint32_t n_fields);
int dsrcgpu_set_fields_capacity(dsrcgpu_handle* h, uint32_t cap);
int dsrcgpu_get_fields_capacity(const dsrcgpu_handle* h, uint32_t* cap);
int dsrcgpu_chain_seed(dsrcgpu_chain* c, uint32_t fields_capacity);      /* before batch 0 of the chain has run */

/* Record-level API (reference: wrap::BlockCompressorExt::WriteNextRecord/Flush, src/BlockCompressorExt.cpp:20-46,65-127,
 * used by wrap::DsrcArchive, src/DsrcArchive.cpp:129-150,217-224).  The caller assembles each chunk as FASTQ text
 * (tag\nsequence\nplus\nquality, no newline after the last record) and declares, for the NEXT batch call on h
 * (n must equal that call's chunk count; one-shot), that the chunks come from records:
 *   - block i stores chunk_sizes[i] as chunkSize (the reference keeps a running total over the whole archive there,
 *     because BlockCompressor::Reset does not clear it);
 *   - the reference lays tag, sequence and quality out back to back, so its tag tokenizer takes the first sequence
 *     byte (already turned into a base index) as the separator after the last title field; reproduced.
 * Not combinable with tag_preserve_flags or calculate_crc32 (the reference's archive API drops both). */
int dsrcgpu_set_record_layout(dsrcgpu_handle* h, uint32_t n, const uint32_t* chunk_sizes);

/* Decoding the order-context levels keeps one adaptive model table per block in flight (up to 64 MiB at -q2, DESIGN.md
 * section 11); by default a pass takes 70 % of the HBM that is free when it starts.  Hosts that run several decoding
 * handles on one device give each its share: dsrcgpu_set_table_budget(h, bytes) (0 = automatic again).  A pass whose tables do
 * not fit the budget decodes in rounds (as many tables as fit at a time, at least one).  A budget below the largest single table
 * of a pass (2 MiB for a 4-symbol DNA table at -d3, 32 MiB for an 8-symbol one, up to 64 MiB for a quality table at -q2) is raised
 * to that table: the region is never smaller than one table plus the allocation's slack of 1/16 + 4 KiB, and a region an
 * earlier pass left larger is kept, not shrunk.  DSRC_GPU_DEBUG=1 prints the budget, the region and the rounds of every pass. */
int dsrcgpu_set_table_budget(dsrcgpu_handle* h, uint64_t bytes);
int dsrcgpu_device_memory(int device, uint64_t* free_bytes, uint64_t* total_bytes);
/* A handle keeps its batch arena and its table region between calls (tens of GB after a large pass).  A host that moves on to
 * another phase on the same device (other handles, other batch sizes) hands them back with dsrcgpu_release_memory; the next call
 * allocates again.  Not to be called while a call on this handle is in flight (queue form: after the last collect).  No
 * counterpart in the reference: its workers' buffers live as long as the workers. */
int dsrcgpu_release_memory(dsrcgpu_handle* h);
/* The opposite: a host that knows what its next call will need has the batch arena and / or the decoder's table region grown to at least
 * these sizes NOW (nothing shrinks; the table figure is capped by the table budget) -- on a side thread, or while it is still reading its
 * input.  Worth it where allocation is not free: HBM that another process has just released is wiped by the driver before it is handed
 * out again (~20-35 GB/s on the measured box, NOTES/round_5.md), and the first call would otherwise wait for that in the middle of its
 * course.  Not to be called while a call on this handle is in flight. */
int dsrcgpu_reserve_memory(dsrcgpu_handle* h, uint64_t arena_bytes, uint64_t table_bytes);

/* Optional: brings up the HIP runtime and the device context (the first HIP call of a process costs 0.3-1 s); call it on a
 * side thread while the host opens its files.  It is also the opt-in for a queue setting that helps several handles per device:
 * when the process has not set GPU_MAX_HW_QUEUES, the first call sets it to 24 -- effective only if this is the process's first
 * HIP call (the runtime reads the variable when it starts).  The library never touches the environment otherwise.  No handle
 * NEEDS the setting: every handle's range coder runs on a hardware queue that no front-end stream shares, whatever the variable
 * says, so handles overlap with the runtime's default of 4 queues as well (and in a process that started HIP earlier); with more
 * handles or lanes than queues only their data-parallel front ends take turns on a queue. */
int dsrcgpu_prepare(int device);

/* Page-locked host memory for chunk / block buffers: host<->device copies from it run at PCIe speed and
 * asynchronously to the other handles' kernels (the entry points accept any host pointer; pageable ones are slower). */
int dsrcgpu_host_alloc(uint64_t bytes, void** out);
int dsrcgpu_host_free(void* p);

/* Device arithmetic self-test: the exact-division identities the range-coder stage relies on (reciprocal of every
 * possible model total, quotients on a spread of numerators) are checked against the hardware integer division.
 * *mismatches must come back 0. */
int dsrcgpu_selftest(dsrcgpu_handle* h, uint32_t* mismatches);

/* Timing of the last batch measured with HIP events on the scheduler's stream: total ms of the batch's
 * kernels, ms of the range-coder kernel (k_rc), number of k_rc launches.  After dsrcgpu_compress_columns_device the batch figure starts
 * in front of the check pass: it includes the check, the host's layout of the chunks and the scatter of the text. */
int dsrcgpu_last_timing(const dsrcgpu_handle* h, float* batch_ms, float* rc_ms, uint32_t* rc_launches);

/* ... and of the two data-parallel stages that bound the throughput of the order-context levels: summed HIP-event time
 * of the k_sort launches (context sort) and of the k_replay_seams + k_replay launches (model replay) of the last batch. */
int dsrcgpu_last_stage_timing(const dsrcgpu_handle* h, float* sort_ms, float* replay_ms);

/* Counter-based synthetic Illumina-like FASTQ generated directly in HBM (bench input; same bytes as
 * dsrc_amd/synth.py illumina_fastq).  Writes records first..first+count-1, returns the byte count. */
int dsrcgpu_synth_illumina(dsrcgpu_handle* h, uint64_t first, uint64_t count, void* d_out, uint64_t cap, uint64_t* bytes);
/* ... with a flavour: 0 = the generator above (BASELINE's configurations); 1 = the same records with the qualities quantised to four
 * levels (Phred 2 / 12 / 23 / 37: what current instruments write) -- dsrc_amd/synth.py illumina_fastq(binned=True); bench.py's second line;
 * 2 = variable-length 454/Ion-Torrent-like reads (40..500 bases, 1 % IUPAC codes, zero qualities under most of them), the same bytes as
 * dsrc_amd/synth.py iontorrent_fastq: the input of BASELINE's configuration 5 (-d2 -q1, lossy), timed by tools/config_bench.py.
 * Any other flavour: DSRCGPU_E_ARG.  count == 0: *bytes = 0.  Output larger than cap: DSRCGPU_E_CAPACITY, *bytes = the size needed,
 * nothing written. */
int dsrcgpu_synth_fastq(dsrcgpu_handle* h, uint32_t flavour, uint64_t first, uint64_t count, void* d_out, uint64_t cap, uint64_t* bytes);

/* small HBM helpers so that non-HIP hosts (Python/ctypes, JNI ...) can stage device-resident batches */
int dsrcgpu_dev_alloc(dsrcgpu_handle* h, uint64_t bytes, void** d_ptr);
int dsrcgpu_dev_free(dsrcgpu_handle* h, void* d_ptr);
int dsrcgpu_dev_upload(dsrcgpu_handle* h, void* d_dst, const void* src, uint64_t bytes);
int dsrcgpu_dev_download(dsrcgpu_handle* h, void* dst, const void* d_src, uint64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* DSRC_GPU_H */
