// The host half of the columnar calls (the kernels: k_columns*.h).  Part of dsrc_gpu.hip, which includes it once, behind the decoder's
// entry points: the library stays one translation unit.
//
// Every call here is a scratch-only user of the handle's own lane: it takes its result words and a few words per record from the
// arena, runs on h->stream and synchronises before it returns; h->fields_cap, h->rec_pending and the chain are neither read nor
// written (dsrcgpu_compress_columns_device, which hands its text to run_batch, is the one exception).  An entry point reads top to
// bottom as: argument checks -> scratch -> launches -> results home -> report; what the calls share is in the helpers below.
#pragma once
#include <array>

namespace
{
// ---- refusals ------------------------------------------------------------------------------------------------------------------------
int queue_idle(dsrcgpu_handle* h)
{
	std::lock_guard<std::mutex> g(h->q_m);
	if (h->q_started && h->q_pending) return fail(h, DSRCGPU_E_STATE, "batches of the queue form are still in flight on this handle");
	return DSRCGPU_OK;
}

// The caller's arrays -> c.  need: the arrays this call cannot do without; titles it can do without are taken out of c.  The queue is
// looked at last (dsrcgpu_compress_columns_device comes here behind user_batch_begin, which has looked already).
enum : u32 { COL_TITLES = 1, COL_QUALS = 2 };
int col_in_args(dsrcgpu_handle* h, const dsrcgpu_columns_in* in, u32 need, ColIn& c)
{
	const bool titles = need & COL_TITLES, quals = need & COL_QUALS;
	if (!in) return fail(h, DSRCGPU_E_ARG, "null argument");
	if (h->ds.color_space) return fail(h, DSRCGPU_E_ARG, "columns are defined for base space: a colour-space line is a primer plus colours");
	if ((in->n_records | in->bases_len | (titles ? in->titles_len : 0)) >> 56) return fail(h, DSRCGPU_E_ARG, "columns: array lengths of 2^56 and more");
	if (in->n_records && (!in->d_seq_offs || (titles && !in->d_title_offs))) return fail(h, DSRCGPU_E_ARG, "columns: null offset array");
	if ((in->bases_len && (!in->d_bases || (quals && !in->d_quals))) || (titles && in->titles_len && !in->d_titles)) return fail(h, DSRCGPU_E_ARG, "columns: null array with a length");
	c = ColIn{in->d_bases, in->d_quals, titles ? in->d_titles : nullptr, in->d_seq_offs, titles ? in->d_title_offs : nullptr, in->n_records, in->bases_len,
	          titles ? in->titles_len : 0, h->ds.plus_repetition ? 1u : 0u, h->ds.quality_offset};
	return queue_idle(h);
}

// the two ends of a range array pair: both or neither
int together(dsrcgpu_handle* h, const void* d_begin, const void* d_end, const char* begin, const char* end)
{
	return !d_begin != !d_end ? fail(h, DSRCGPU_E_ARG, "columns: %s and %s go together", begin, end) : DSRCGPU_OK;
}

template <size_t N> int reserved_clear(dsrcgpu_handle* h, const char* rules, const uint32_t (&reserved)[N])
{
	for (size_t i = 0; i < N; ++i)
		if (reserved[i]) return fail(h, DSRCGPU_E_ARG, "%s: reserved fields must be 0", rules);
	return DSRCGPU_OK;
}

// an error word of the check passes: (record << 4) | reason
int col_input_error(dsrcgpu_handle* h, u64 word)
{
	static const char* const reason[] = {"d_seq_offs is not non-decreasing", "d_seq_offs runs above bases_len", "d_title_offs is not non-decreasing",
		"d_title_offs runs above titles_len", "empty title", "title does not start with '@'", "title contains a newline",
		"base code above 18", "quality + quality_offset above 126",
		"d_begin lies below the record's first base", "d_end lies above the record's last base", "d_begin lies above d_end"};
	static_assert(COLE_QUAL == 8 && COLS_BEGIN_LOW == 9 && COLS_RANGE_ORDER == 11, "reason[] is indexed by the kernels' reasons");
	const u32 why = (u32)(word & 15u);
	return fail(h, DSRCGPU_E_INPUT, "columns: record %llu: %s", (unsigned long long)(word >> 4), why < 12 ? reason[why] : "?");
}

// ---- result words ----------------------------------------------------------------------------------------------------------------------
// What a call brings home, in arena scratch: n_err error words (one per side; COLE_NONE = clean), n_zero counters that start at 0, n_plain
// words that a kernel writes whole.  res_alloc takes them from an arena the caller has sized (first, then the caller's other scratch);
// res_begin refuses when the arena did not hold all of it, else sets the words up; res_home brings the first `words` of them (all by
// default) into w with one copy and one synchronisation and reports the first dirty error word.
struct ResWords
{
	u64* d; u32 n_err, n_zero, n_plain;
	u64 w[32];
	u32 words() const { return n_err + n_zero + n_plain; }
	u64* counters() const { return d + n_err; }
	const u64* home() const { return w + n_err; }
};

ResWords res_alloc(dsrcgpu_handle* h, u32 n_err, u32 n_zero, u32 n_plain = 0)
{
	ResWords r{nullptr, n_err, n_zero, n_plain, {}};
	r.d = AP<u64>(h, h->arena.alloc((size_t)r.words() * 8));
	return r;
}

int res_begin(dsrcgpu_handle* h, const ResWords& r, const char* call)
{
	if (h->arena.failed) return fail(h, DSRCGPU_E_NOMEM, "arena exhausted (%s)", call);
	if (r.n_err) HIPCHK(hipMemsetAsync(r.d, 0xFF, (size_t)r.n_err * 8, h->stream));
	if (r.n_zero) HIPCHK(hipMemsetAsync(r.d + r.n_err, 0, (size_t)r.n_zero * 8, h->stream));
	return DSRCGPU_OK;
}

// sided: the call's name in a two-sided call ("<call>, read N: columns: record ..."), null in a one-sided one
int res_home(dsrcgpu_handle* h, ResWords& r, const char* sided = nullptr, u32 words = 0)
{
	if (!words) words = r.words();
	if (words > sizeof(r.w) / 8) return fail(h, DSRCGPU_E_HIP, "internal: %u result words", words);
	HIPCHK(hipMemcpyAsync(r.w, r.d, (size_t)words * 8, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	for (u32 side = 0; side < r.n_err; ++side)
		if (r.w[side] != COLE_NONE)
		{
			const int rc = col_input_error(h, r.w[side]);
			if (!sided) return rc;
			const std::string why = dsrcgpu_last_error(h);
			return fail(h, rc, "%s, read %u: %s", sided, side + 1, why.c_str());
		}
	return DSRCGPU_OK;
}

// ---- grids -----------------------------------------------------------------------------------------------------------------------------
dim3 grid_threads(u64 items, u64 cap = 1024) { return dim3((u32)std::max<u64>(1, std::min<u64>(cap, (items + WG - 1) / WG))); }      // a thread an item
dim3 grid_waves(u64 records, u64 cap = 4096) { return dim3((u32)std::max<u64>(1, std::min<u64>(cap, (records + WG / 64 - 1) / (WG / 64)))); }      // a wave a record

// ---- output placement (select, merge) --------------------------------------------------------------------------------------------------
// no record comes out: the offset arrays still get their first entry
int nothing_out(dsrcgpu_handle* h, const dsrcgpu_columns* out, bool titles)
{
	if (out->d_seq_offs) HIPCHK(hipMemsetAsync(out->d_seq_offs, 0, sizeof(u64), h->stream));
	if (titles && out->d_title_offs) HIPCHK(hipMemsetAsync(out->d_title_offs, 0, sizeof(u64), h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	return DSRCGPU_OK;
}

// tot: records, bases, title bytes that come out.  "<call>: ... <come out>; the caller's arrays hold ..."
int out_holds(dsrcgpu_handle* h, const dsrcgpu_columns* out, bool titles, const u64 tot[3], const char* call, const char* come_out)
{
	if (out->records_cap >= tot[0] && out->bases_cap >= tot[1] && out->quals_cap >= tot[1] && (!titles || out->titles_cap >= tot[2])) return DSRCGPU_OK;
	return fail(h, DSRCGPU_E_CAPACITY, "%s: %llu records, %llu bases, %llu title bytes %s; the caller's arrays hold %llu, %llu / %llu, %llu", call,
	            (unsigned long long)tot[0], (unsigned long long)tot[1], (unsigned long long)tot[2], come_out, (unsigned long long)out->records_cap,
	            (unsigned long long)out->bases_cap, (unsigned long long)out->quals_cap, (unsigned long long)out->titles_cap);
}

// bases: whether d_bases / d_quals are needed (the select does without them when no base is kept)
int out_arrays(dsrcgpu_handle* h, const dsrcgpu_columns* out, bool titles, bool bases, u64* d_source, const u64 tot[3], SelOut& o)
{
	if (!out->d_seq_offs || (titles && !out->d_title_offs) || (bases && (!out->d_bases || !out->d_quals))) return fail(h, DSRCGPU_E_ARG, "columns: null output array");
	o = SelOut{out->d_bases, out->d_quals, out->d_titles, out->d_seq_offs, out->d_title_offs, d_source, tot[0], tot[1], tot[2]};
	return DSRCGPU_OK;
}

// ---- k-mer tables (k_columns_kmer.h) ---------------------------------------------------------------------------------------------------
KmerTab kmer_tab(const uint64_t* d_table, u64 M, u32 hash_bits)
{
	u64* const keys = const_cast<u64*>(d_table) + KMER_HEADER;
	return KmerTab{keys, keys + M, M - 1, hash_bits == 0 || hash_bits == 64 ? ~0ull : (1ull << hash_bits) - 1ull, (u32)std::min<u64>(M, KMER_PROBE_LIMIT)};
}

// the 64-byte header of a caller's table, brought home and checked: the magic, k, canonical, M.  -> t (the table behind it), k, canonical
int kmer_table_home(dsrcgpu_handle* h, const uint64_t* d_table, const char* what, u64 hdr[8], KmerTab& t, u32& k, u32& canonical)
{
	HIPCHK(hipMemcpyAsync(hdr, d_table, 8 * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	k = (u32)((hdr[0] >> 8) & 255u); canonical = (u32)(hdr[0] & 255u);
	const u32 bits = (u32)((hdr[0] >> 16) & 255u);
	const u64 M = hdr[1];
	if (hdr[0] >> 32 != KMER_MAGIC || k < 1 || k > DSRCGPU_KMER_MAX_K || canonical > 1 || bits > 63 || hdr[0] != kmer_header_word(k, canonical, bits) || M < 16 ||
	    M > (1ull << 40) || (M & (M - 1)))
		return fail(h, DSRCGPU_E_ARG, "%s: not a k-mer table (header word %016llx, capacity %llu)", what, (unsigned long long)hdr[0], (unsigned long long)M);
	t = kmer_tab(d_table, M, bits);
	return DSRCGPU_OK;
}

u64 kmer_need(u64 keys)
{
	u64 need = 16;
	while (need < 2 * keys) need <<= 1;
	return need;
}
} // namespace

extern "C" {

// ---- columnar encode (k_columns_enc.h) -------------------------------------------------------------------------------------------
// The check pass and the cut points' text positions first (one synchronisation brings both home), then the text is laid out like the
// chunks of compress_batch_host, scattered into the arena and handed to run_batch as the library's own copy.
int dsrcgpu_compress_columns_device(dsrcgpu_handle* h, uint32_t n, const dsrcgpu_columns_in* in, const uint64_t* block_records,
									void* d_blocks, uint64_t blocks_cap, uint64_t* block_offs, uint64_t* block_sizes,
									uint64_t* raw_sizes, uint64_t* comp_sizes)
{
	if (!h) return DSRCGPU_E_ARG;
	if (h->ds.color_space) return fail(h, DSRCGPU_E_ARG, "columns are defined for base space: a colour-space line is a primer plus colours");
	{
		std::vector<u32> layout;
		if (const int rc = user_batch_begin(h, layout)) return rc;
		if (!layout.empty()) return fail(h, DSRCGPU_E_ARG, "columns: a record layout is pending (dsrcgpu_set_record_layout belongs to the text calls of the archive API); dropped");
	}
	if (n == 0) return DSRCGPU_OK;
	if (!block_records || !d_blocks || !block_offs || !block_sizes || !raw_sizes || !comp_sizes) return fail(h, DSRCGPU_E_ARG, "null argument");
	ColIn c;
	if (const int rc = col_in_args(h, in, COL_TITLES | COL_QUALS, c)) return rc;
	if (block_records[0] != 0 || block_records[n] != c.n_recs) return fail(h, DSRCGPU_E_ARG, "columns: block_records must run from 0 to n_records");
	u64 max_recs = 1;
	for (u32 i = 0; i < n; ++i)
	{
		if (block_records[i] >= block_records[i + 1]) return fail(h, DSRCGPU_E_ARG, "columns: block %u has no records (block_records must increase)", i);
		max_recs = std::max<u64>(max_recs, block_records[i + 1] - block_records[i]);
	}
	HIPCHK(hipSetDevice(h->device));
	hipStream_t s = h->stream;

	// ---- check pass (the arena as it stands is large enough for it, except on a handle's first call); unlike the calls below, every
	// failure from here on aborts the chain, and the result words (n + 2 of them) do not fit ResWords ----
	std::vector<u64> res((size_t)n + 2);                 // error word, P at the n + 1 cut points
	{
		const int rc = ensure_arena(h, (size_t)(2 * (size_t)n + 3) * 8 + 1024);
		if (rc) { chain_abort(h); return rc; }
		if (!h->col_ev) HIPCHK(hipEventCreate(&h->col_ev));
		HIPCHK(hipEventRecord(h->col_ev, s));
		const size_t o_cut = h->arena.alloc(((size_t)n + 1) * 8), o_res = h->arena.alloc(((size_t)n + 2) * 8);
		if (h->arena.failed) { chain_abort(h); return fail(h, DSRCGPU_E_NOMEM, "arena exhausted (columns check)"); }
		u64* d_cut = AP<u64>(h, o_cut); u64* d_res = AP<u64>(h, o_res);
		HIPCHK(hipMemcpyAsync(d_cut, block_records, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
		HIPCHK(hipMemsetAsync(d_res, 0xFF, 8, s));
		hipLaunchKernelGGL(k_col_check, grid_waves(c.n_recs), dim3(WG), 0, s, c, d_cut, n + 1, d_res + 1, d_res); KCHK();
		HIPCHK(hipMemcpyAsync(res.data(), d_res, ((size_t)n + 2) * 8, hipMemcpyDeviceToHost, s));
		HIPCHK(hipStreamSynchronize(s));
	}
	if (res[0] != COLE_NONE) { chain_abort(h); return col_input_error(h, res[0]); }

	// ---- the chunks: sizes from P, laid out as compress_batch_host lays out the chunks it uploads ----
	std::vector<u64> offs(n), sizes(n);
	std::vector<ColEncBlk> blk(n);
	size_t in_bytes = 0;
	for (u32 i = 0; i < n; ++i)
	{
		sizes[i] = res[i + 2] - res[i + 1] - 1;
		if (sizes[i] >= (1ull << 31)) { chain_abort(h); return fail(h, DSRCGPU_E_ARG, "columns: block %u: %llu bytes of text, the limit is 2^31 - 1; cut smaller blocks", i, (unsigned long long)sizes[i]); }
		offs[i] = in_bytes; in_bytes += al((size_t)sizes[i] + 16, 256);
		blk[i] = ColEncBlk{block_records[i], block_records[i + 1], res[i + 1], offs[i]};
	}
	const u32 gx = (u32)std::max<u64>(1, std::min<u64>(64, (max_recs + 4 * WAVES - 1) / (4 * WAVES)));
	float front = 0.f;              // HIP-event time from in front of the check pass to the start of run_batch
	const int rc_all = with_arena_retry(h, estimate_arena(h, n, sizes.data()) + in_bytes + (size_t)n * sizeof(ColEncBlk) + 1024, [&]() {
		const size_t o_in = h->arena.alloc(in_bytes + 256), o_blk = h->arena.alloc(sizeof(ColEncBlk) * n);
		if (h->arena.failed) return fail(h, DSRCGPU_E_NOMEM, "arena exhausted (text of the columns)");
		u8* d_in = h->arena.base + o_in;
		HIPCHK(hipMemcpyAsync(AP<ColEncBlk>(h, o_blk), blk.data(), sizeof(ColEncBlk) * n, hipMemcpyHostToDevice, s));
		hipLaunchKernelGGL(k_col_scatter, dim3(gx, n), dim3(WG), 0, s, c, AP<ColEncBlk>(h, o_blk), d_in); KCHK();
		BatchIO io{d_in, offs.data(), sizes.data(), n, (u8*)d_blocks, blocks_cap, nullptr, 0, block_offs, block_sizes, raw_sizes, comp_sizes, nullptr, false};
		const int rc = run_batch(h, io);
		if (rc == DSRCGPU_OK) hipEventElapsedTime(&front, h->col_ev, h->ev[0]);       // (before a verifying pass records ev[0] again)
		if (rc != DSRCGPU_OK || !h->set.verify_after_compress || !h->set.calculate_crc32) return rc;
		return verify_blocks(h, n, block_offs, block_sizes);
	});
	if (rc_all == DSRCGPU_OK)
	{	// dsrcgpu_last_timing: from the check pass to k_assemble (the host's layout of the chunks between the two kernels included)
		h->batch_ms += front;
		if (getenv("DSRC_GPU_DEBUG")) fprintf(stderr, "[dsrc_gpu] columns: check pass, layout and scatter of %llu records took %.3f ms of the batch's %.3f\n", (unsigned long long)c.n_recs, front, h->batch_ms);
	}
	return rc_all;
}

int dsrcgpu_columns_cut(dsrcgpu_handle* h, const dsrcgpu_columns_in* in, uint64_t chunk_bytes, uint64_t* block_records, uint32_t cap, uint32_t* n)
{
	if (!h) return DSRCGPU_E_ARG;
	if (!block_records || !n) return fail(h, DSRCGPU_E_ARG, "null argument");
	*n = 0;
	if (chunk_bytes == 0) return fail(h, DSRCGPU_E_ARG, "columns: chunk_bytes of 0");
	ColIn c;
	if (const int rc = col_in_args(h, in, COL_TITLES | COL_QUALS, c)) return rc;
	if (c.n_recs == 0)
	{
		if (cap < 1) return fail(h, DSRCGPU_E_CAPACITY, "columns: block_records needs 1 entry, caller gave 0");
		block_records[0] = 0;
		return DSRCGPU_OK;
	}
	HIPCHK(hipSetDevice(h->device));
	hipStream_t s = h->stream;
	const u64 out_cap = std::min<u64>(cap, c.n_recs + 1);       // (no more blocks than records)
	if (const int rc = ensure_arena(h, (size_t)(out_cap + 3) * 8 + 1024)) return rc;
	ResWords res = res_alloc(h, 1, 1);                    // error word, number of blocks
	u64* d_out = AP<u64>(h, h->arena.alloc((size_t)(out_cap + 1) * 8));
	if (const int rc = res_begin(h, res, "columns cut")) return rc;
	hipLaunchKernelGGL(k_col_mono, grid_threads(c.n_recs), dim3(WG), 0, s, c, res.d); KCHK();
	hipLaunchKernelGGL(k_col_cut, dim3(1), dim3(64), 0, s, c, std::min<u64>(chunk_bytes, 1ull << 62), d_out, out_cap, res.counters(), res.d); KCHK();
	if (const int rc = res_home(h, res)) return rc;
	const u64 blocks = res.home()[0];
	if (blocks >> 32) return fail(h, DSRCGPU_E_ARG, "columns: more than 2^32 - 1 blocks; raise chunk_bytes");
	*n = (u32)blocks;
	if (blocks + 1 > cap) return fail(h, DSRCGPU_E_CAPACITY, "columns: block_records needs %llu entries, caller gave %u", (unsigned long long)(blocks + 1), cap);
	HIPCHK(hipMemcpyAsync(block_records, d_out, (size_t)(blocks + 1) * 8, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	return DSRCGPU_OK;
}

// ---- columnar select (k_columns_sel.h) ---------------------------------------------------------------------------------------------
int dsrcgpu_columns_trim_plan(dsrcgpu_handle* h, const dsrcgpu_columns_in* in, const dsrcgpu_trim_rules* rules,
							  uint64_t* d_begin, uint64_t* d_end, uint8_t* d_keep, uint64_t stats[6])
{
	if (!h) return DSRCGPU_E_ARG;
	if (!rules || !stats) return fail(h, DSRCGPU_E_ARG, "null argument");
	for (u32 k = 0; k < 6; ++k) stats[k] = 0;
	ColIn c;
	if (const int rc = col_in_args(h, in, COL_QUALS, c)) return rc;
	if (rules->quality_5 > 255 || rules->quality_3 > 255) return fail(h, DSRCGPU_E_ARG, "trim rules: a quality cutoff above 255");
	if (const int rc = reserved_clear(h, "trim rules", rules->reserved)) return rc;
	if (c.n_recs == 0) return DSRCGPU_OK;
	if (!d_begin || !d_end || !d_keep) return fail(h, DSRCGPU_E_ARG, "null argument");
	HIPCHK(hipSetDevice(h->device));
	hipStream_t s = h->stream;
	if (const int rc = ensure_arena(h, 7 * 8 + 1024)) return rc;
	ResWords res = res_alloc(h, 1, 6);                    // error word, the six statistics
	if (const int rc = res_begin(h, res, "trim plan")) return rc;
	const TrimRules R{rules->quality_5, rules->quality_3, rules->min_length, rules->max_n, rules->min_mean_quality};
	hipLaunchKernelGGL(k_sel_seq_check, grid_threads(c.n_recs), dim3(WG), 0, s, c, res.d); KCHK();
	hipLaunchKernelGGL(k_sel_plan, grid_waves(c.n_recs), dim3(WG), 0, s, c, R, d_begin, d_end, d_keep, res.counters(), res.d); KCHK();
	if (const int rc = res_home(h, res)) return rc;
	for (u32 k = 0; k < 6; ++k) stats[k] = res.home()[k];
	return DSRCGPU_OK;
}

// tile sums and their scan first: error word and totals come home in one synchronisation, in front of the first kernel that writes the
// caller's arrays
int dsrcgpu_columns_select_device(dsrcgpu_handle* h, const dsrcgpu_columns_in* in, const uint64_t* d_begin, const uint64_t* d_end,
								  const uint8_t* d_keep, const dsrcgpu_columns* out, uint64_t* d_source, uint64_t totals[3])
{
	if (!h) return DSRCGPU_E_ARG;
	if (!out || !totals) return fail(h, DSRCGPU_E_ARG, "null argument");
	totals[0] = totals[1] = totals[2] = 0;
	if (const int rc = together(h, d_begin, d_end, "d_begin", "d_end")) return rc;
	if (!out->d_titles && out->titles_cap) return fail(h, DSRCGPU_E_ARG, "columns: titles_cap without d_titles");
	const bool titles = out->d_titles != nullptr;
	ColIn c;
	if (const int rc = col_in_args(h, in, COL_QUALS | (titles ? COL_TITLES : 0), c)) return rc;
	HIPCHK(hipSetDevice(h->device));
	hipStream_t s = h->stream;
	if (c.n_recs == 0) return nothing_out(h, out, titles);
	const u64 n_tiles = (c.n_recs + WG - 1) / WG;
	if (const int rc = ensure_arena(h, (size_t)(3 * n_tiles + c.n_recs + 4) * 8 + 4096)) return rc;
	ResWords res = res_alloc(h, 1, 0, 3);                 // error word, the three totals (the scan writes them)
	u64* d_tiles = AP<u64>(h, h->arena.alloc((size_t)n_tiles * 24));
	u64* d_pos = AP<u64>(h, h->arena.alloc((size_t)c.n_recs * 8));
	if (const int rc = res_begin(h, res, "columns select")) return rc;
	const SelWhat w{d_begin, d_end, d_keep, titles ? 1u : 0u};
	const u32 g_tiles = (u32)std::min<u64>(4096, n_tiles);
	hipLaunchKernelGGL(k_sel_tiles, dim3(g_tiles), dim3(WG), 0, s, c, w, n_tiles, d_tiles, res.d); KCHK();
	hipLaunchKernelGGL(k_sel_scan_tiles, dim3(1), dim3(WG), 0, s, n_tiles, d_tiles, res.counters()); KCHK();
	if (const int rc = res_home(h, res)) return rc;
	const u64* const tot = res.home();
	totals[0] = tot[0]; totals[1] = tot[1]; totals[2] = tot[2];
	if (const int rc = out_holds(h, out, titles, tot, "columns", "are kept")) return rc;
	if (tot[0] == 0) return nothing_out(h, out, titles);
	SelOut o;
	if (const int rc = out_arrays(h, out, titles, tot[1] != 0, d_source, tot, o)) return rc;
	hipLaunchKernelGGL(k_sel_apply, dim3(g_tiles), dim3(WG), 0, s, c, w, n_tiles, d_tiles, o, d_pos); KCHK();
	hipLaunchKernelGGL(k_sel_gather, grid_waves(c.n_recs), dim3(WG), 0, s, c, w, o, d_pos); KCHK();
	HIPCHK(hipStreamSynchronize(s));
	return DSRCGPU_OK;
}

// the adapter search (k_columns_adapt.h): the rules are checked and turned into bit planes here, then the check pass and the planner run
// back to back as in dsrcgpu_columns_trim_plan
int dsrcgpu_columns_adapter_plan(dsrcgpu_handle* h, const dsrcgpu_columns_in* in, const dsrcgpu_adapter_rules* rules,
								 const uint64_t* d_begin_in, const uint64_t* d_end_in, const uint8_t* d_keep_in,
								 uint64_t* d_begin, uint64_t* d_end, uint8_t* d_keep, uint32_t* d_which, uint64_t stats[13])
{
	if (!h) return DSRCGPU_E_ARG;
	if (!rules || !stats) return fail(h, DSRCGPU_E_ARG, "null argument");
	for (u32 k = 0; k < 13; ++k) stats[k] = 0;
	ColIn c;
	if (const int rc = col_in_args(h, in, 0, c)) return rc;
	if (rules->n_adapters < 1 || rules->n_adapters > ADAPT_MAX) return fail(h, DSRCGPU_E_ARG, "adapter rules: n_adapters must be 1 .. 8");
	AdaptRules R{};
	R.k = rules->n_adapters; R.min_overlap = rules->min_overlap; R.permille = rules->max_error_permille; R.min_len = rules->min_length;
	u32 shortest = 64;
	for (u32 a = 0; a < ADAPT_MAX; ++a)
	{
		const u32 len = rules->adapter_len[a];
		if (a >= R.k) { if (len) return fail(h, DSRCGPU_E_ARG, "adapter rules: a length behind n_adapters"); continue; }
		if (len < 1 || len > 64) return fail(h, DSRCGPU_E_ARG, "adapter rules: adapter %u: a length of 1 .. 64 is needed", a);
		shortest = std::min(shortest, len);
		R.len[a] = len;
		for (u32 j = 0; j < len; ++j)
		{
			const u32 code = rules->adapters[a][j];
			if (code > 3) return fail(h, DSRCGPU_E_ARG, "adapter rules: adapter %u: code %u at position %u (A C G T = 0 .. 3 only)", a, code, j);
			R.a0[a] |= (u64)(code & 1u) << j; R.a1[a] |= (u64)(code >> 1) << j;
		}
	}
	if (rules->min_overlap < 1 || rules->min_overlap > shortest) return fail(h, DSRCGPU_E_ARG, "adapter rules: min_overlap must be 1 .. the shortest adapter's length");
	if (rules->max_error_permille > 1000) return fail(h, DSRCGPU_E_ARG, "adapter rules: max_error_permille above 1000");
	if (const int rc = reserved_clear(h, "adapter rules", rules->reserved)) return rc;
	if (const int rc = together(h, d_begin_in, d_end_in, "d_begin_in", "d_end_in")) return rc;
	if (c.n_recs == 0) return DSRCGPU_OK;
	if (!d_begin || !d_end || !d_keep) return fail(h, DSRCGPU_E_ARG, "null argument");
	HIPCHK(hipSetDevice(h->device));
	hipStream_t s = h->stream;
	if (const int rc = ensure_arena(h, 14 * 8 + 1024)) return rc;
	ResWords res = res_alloc(h, 1, 13);                   // error word, the thirteen statistics
	if (const int rc = res_begin(h, res, "adapter plan")) return rc;
	const ColPlanIn w{d_begin_in, d_end_in, d_keep_in};
	hipLaunchKernelGGL(k_col_plan_check, grid_threads(c.n_recs), dim3(WG), 0, s, c, w, res.d); KCHK();
	hipLaunchKernelGGL(k_adapt_plan, grid_waves(c.n_recs), dim3(WG), 0, s, c, w, R, d_begin, d_end, d_keep, d_which, res.counters(), res.d); KCHK();
	if (const int rc = res_home(h, res)) return rc;
	for (u32 k = 0; k < 13; ++k) stats[k] = res.home()[k];
	return DSRCGPU_OK;
}

// the complexity plan (k_columns_complexity.h): the rules are checked here, then the check pass of the adapter plan and the planner
// run back to back as in dsrcgpu_columns_adapter_plan
int dsrcgpu_columns_complexity_plan(dsrcgpu_handle* h, const dsrcgpu_columns_in* in, const dsrcgpu_complexity_rules* rules,
									const uint64_t* d_begin_in, const uint64_t* d_end_in, const uint8_t* d_keep_in,
									uint64_t* d_begin, uint64_t* d_end, uint8_t* d_keep, uint32_t* d_info, uint64_t stats[20])
{
	if (!h) return DSRCGPU_E_ARG;
	if (!rules || !stats) return fail(h, DSRCGPU_E_ARG, "null argument");
	for (u32 k = 0; k < CPLX_STATS; ++k) stats[k] = 0;
	ColIn c;
	if (const int rc = col_in_args(h, in, 0, c)) return rc;
	if (rules->tail_bases > 15) return fail(h, DSRCGPU_E_ARG, "complexity rules: tail_bases above 15 (A = 1, C = 2, G = 4, T = 8)");
	if (rules->head_bases > 15) return fail(h, DSRCGPU_E_ARG, "complexity rules: head_bases above 15 (A = 1, C = 2, G = 4, T = 8)");
	if ((rules->tail_bases | rules->head_bases) && rules->poly_min_length == 0) return fail(h, DSRCGPU_E_ARG, "complexity rules: poly_min_length of 0 with a base to search");
	if (rules->poly_max_error_permille > 1000) return fail(h, DSRCGPU_E_ARG, "complexity rules: poly_max_error_permille above 1000");
	if (rules->min_complexity_permille > 1000) return fail(h, DSRCGPU_E_ARG, "complexity rules: min_complexity_permille above 1000");
	if (const int rc = reserved_clear(h, "complexity rules", rules->reserved)) return rc;
	if (const int rc = together(h, d_begin_in, d_end_in, "d_begin_in", "d_end_in")) return rc;
	if (c.n_recs == 0) return DSRCGPU_OK;
	if (!d_begin || !d_end || !d_keep) return fail(h, DSRCGPU_E_ARG, "null argument");
	HIPCHK(hipSetDevice(h->device));
	hipStream_t s = h->stream;
	if (const int rc = ensure_arena(h, (CPLX_STATS + 1) * 8 + 1024)) return rc;
	ResWords res = res_alloc(h, 1, CPLX_STATS);           // error word, the twenty statistics
	if (const int rc = res_begin(h, res, "complexity plan")) return rc;
	const ColPlanIn w{d_begin_in, d_end_in, d_keep_in};
	const CplxRules R{rules->tail_bases, rules->head_bases, rules->poly_min_length, rules->poly_max_error_permille, rules->min_length,
	                  rules->min_complexity_permille, rules->max_dust, rules->max_dust_windows};
	hipLaunchKernelGGL(k_col_plan_check, grid_threads(c.n_recs), dim3(WG), 0, s, c, w, res.d); KCHK();
	hipLaunchKernelGGL(k_cplx_plan, grid_waves(c.n_recs), dim3(WG), 0, s, c, w, R, d_begin, d_end, d_keep, d_info, res.counters(), res.d); KCHK();
	if (const int rc = res_home(h, res)) return rc;
	for (u32 k = 0; k < CPLX_STATS; ++k) stats[k] = res.home()[k];
	return DSRCGPU_OK;
}

// the pair plan (k_columns_pair.h): the check pass of the adapter plan once per side, each with an error word of its own (side 1 is
// reported first), then the planner; the error words and the statistics come home in one copy
int dsrcgpu_columns_pair_plan(dsrcgpu_handle* h, const dsrcgpu_columns_in* in1, const dsrcgpu_columns_in* in2, const dsrcgpu_pair_rules* rules,
							  const uint64_t* d_begin1_in, const uint64_t* d_end1_in, const uint8_t* d_keep1_in,
							  const uint64_t* d_begin2_in, const uint64_t* d_end2_in, const uint8_t* d_keep2_in,
							  uint64_t* d_begin1, uint64_t* d_end1, uint64_t* d_begin2, uint64_t* d_end2, uint8_t* d_keep, uint64_t* d_insert,
							  uint64_t stats[11])
{
	if (!h) return DSRCGPU_E_ARG;
	if (!rules || !stats) return fail(h, DSRCGPU_E_ARG, "null argument");
	for (u32 k = 0; k < PAIR_N_STATS; ++k) stats[k] = 0;
	ColIn c1, c2;
	if (const int rc = col_in_args(h, in1, 0, c1)) return rc;
	if (const int rc = col_in_args(h, in2, 0, c2)) return rc;
	if (c1.n_recs != c2.n_recs) return fail(h, DSRCGPU_E_ARG, "pair plan: %llu records of read 1, %llu of read 2", (unsigned long long)c1.n_recs, (unsigned long long)c2.n_recs);
	if (rules->min_overlap < 1 || rules->min_overlap > DSRCGPU_PAIR_MAX_BASES) return fail(h, DSRCGPU_E_ARG, "pair rules: min_overlap must be 1 .. %u", (u32)DSRCGPU_PAIR_MAX_BASES);
	if (rules->max_error_permille > 1000) return fail(h, DSRCGPU_E_ARG, "pair rules: max_error_permille above 1000");
	if (const int rc = reserved_clear(h, "pair rules", rules->reserved)) return rc;
	if (const int rc = together(h, d_begin1_in, d_end1_in, "d_begin1_in", "d_end1_in")) return rc;
	if (const int rc = together(h, d_begin2_in, d_end2_in, "d_begin2_in", "d_end2_in")) return rc;
	if (c1.n_recs == 0) return DSRCGPU_OK;
	if (!d_begin1 || !d_end1 || !d_begin2 || !d_end2 || !d_keep) return fail(h, DSRCGPU_E_ARG, "null argument");
	HIPCHK(hipSetDevice(h->device));
	hipStream_t s = h->stream;
	if (const int rc = ensure_arena(h, (2 + PAIR_N_STATS) * 8 + 1024)) return rc;
	ResWords res = res_alloc(h, 2, PAIR_N_STATS);         // an error word per side, the eleven statistics
	if (const int rc = res_begin(h, res, "pair plan")) return rc;
	const ColPlanIn w1{d_begin1_in, d_end1_in, d_keep1_in}, w2{d_begin2_in, d_end2_in, d_keep2_in};
	const PairRules R{rules->min_overlap, rules->max_mismatches, rules->max_error_permille, rules->min_length};
	const PairOut o{d_begin1, d_end1, d_begin2, d_end2, d_keep, d_insert};
	hipLaunchKernelGGL(k_col_plan_check, grid_threads(c1.n_recs), dim3(WG), 0, s, c1, w1, res.d); KCHK();
	hipLaunchKernelGGL(k_col_plan_check, grid_threads(c1.n_recs), dim3(WG), 0, s, c2, w2, res.d + 1); KCHK();
	hipLaunchKernelGGL(k_pair_plan, grid_waves(c1.n_recs), dim3(WG), 0, s, c1, c2, w1, w2, R, o, res.counters(), res.d); KCHK();
	if (const int rc = res_home(h, res, "pair plan")) return rc;
	for (u32 k = 0; k < PAIR_N_STATS; ++k) stats[k] = res.home()[k];
	return DSRCGPU_OK;
}

// the dedup plan (k_columns_dedup.h): the check pass per side as in the pair plan (one side: the second error word stays clean), the
// table filled by hipMemsetAsync, then the three launches; the error words and the statistics come home in one copy
int dsrcgpu_columns_dedup_plan(dsrcgpu_handle* h, const dsrcgpu_columns_in* in1, const dsrcgpu_columns_in* in2, const dsrcgpu_dedup_rules* rules,
							   const uint64_t* d_begin1, const uint64_t* d_end1, const uint64_t* d_begin2, const uint64_t* d_end2,
							   const uint8_t* d_keep_in, uint8_t* d_keep, uint64_t* d_dup_of, uint64_t* d_copies, uint64_t stats[24])
{
	if (!h) return DSRCGPU_E_ARG;
	if (!rules || !stats) return fail(h, DSRCGPU_E_ARG, "null argument");
	for (u32 k = 0; k < DEDUP_N_STATS; ++k) stats[k] = 0;
	const bool two = in2 != nullptr;
	const bool quals = rules->prefer == 1;               // the qualities are read for the rank of prefer = 1 only
	ColIn c1, c2{};
	if (const int rc = col_in_args(h, in1, quals ? COL_QUALS : 0, c1)) return rc;
	if (two) { if (const int rc = col_in_args(h, in2, quals ? COL_QUALS : 0, c2)) return rc; }
	if (two && c1.n_recs != c2.n_recs) return fail(h, DSRCGPU_E_ARG, "dedup plan: %llu records of read 1, %llu of read 2", (unsigned long long)c1.n_recs, (unsigned long long)c2.n_recs);
	if (c1.n_recs > (1ull << 31)) return fail(h, DSRCGPU_E_ARG, "dedup plan: more than 2^31 records in one call");
	if (rules->prefer > 1) return fail(h, DSRCGPU_E_ARG, "dedup rules: prefer must be 0 (first) or 1 (best quality)");
	if (rules->hash_bits > 64) return fail(h, DSRCGPU_E_ARG, "dedup rules: hash_bits above 64");
	if (const int rc = reserved_clear(h, "dedup rules", rules->reserved)) return rc;
	if (const int rc = together(h, d_begin1, d_end1, "d_begin1", "d_end1")) return rc;
	if (const int rc = together(h, d_begin2, d_end2, "d_begin2", "d_end2")) return rc;
	if (!two && d_begin2) return fail(h, DSRCGPU_E_ARG, "dedup plan: ranges of read 2 without in2");
	if (c1.n_recs == 0) return DSRCGPU_OK;
	if (!d_keep) return fail(h, DSRCGPU_E_ARG, "null argument");
	HIPCHK(hipSetDevice(h->device));
	hipStream_t s = h->stream;
	const u64 R = c1.n_recs;
	u64 M = 2;
	while (M < 2 * R) M <<= 1;                           // at most half the slots are ever claimed: a probe always ends
	const size_t n_res = 2 + DEDUP_N_STATS;
	const size_t slot_bytes = (size_t)(quals ? 20 : 16);     // occ 4, best 8, count 4, low 4 under prefer = 1
	if (const int rc = ensure_arena(h, n_res * 8 + (size_t)R * 20 + (size_t)M * slot_bytes + 8 * 256 + 1024)) return rc;
	ResWords res = res_alloc(h, 2, DEDUP_N_STATS);        // an error word per side, the 24 statistics
	const size_t o_hash = h->arena.alloc((size_t)R * 8), o_rank = h->arena.alloc((size_t)R * 8), o_slot = h->arena.alloc((size_t)R * 4),
	             o_occ = h->arena.alloc((size_t)M * 4), o_best = h->arena.alloc((size_t)M * 8), o_count = h->arena.alloc((size_t)M * 4),
	             o_low = quals ? h->arena.alloc((size_t)M * 4) : 0;
	if (const int rc = res_begin(h, res, "dedup plan")) return rc;
	const DedupTable t{AP<u32>(h, o_occ), AP<u64>(h, o_best), AP<u32>(h, o_count), quals ? AP<u32>(h, o_low) : nullptr, M - 1};
	HIPCHK(hipMemsetAsync(t.occ, 0xFF, (size_t)M * 4, s));
	HIPCHK(hipMemsetAsync(t.best, 0, (size_t)M * 8, s));
	HIPCHK(hipMemsetAsync(t.count, 0, (size_t)M * 4, s));
	if (quals) HIPCHK(hipMemsetAsync(t.low, 0xFF, (size_t)M * 4, s));
	const ColPlanIn w1{d_begin1, d_end1, nullptr}, w2{d_begin2, d_end2, nullptr};
	const u32 bits = rules->hash_bits;
	const DedupIn in{c1, c2, w1, w2, d_keep_in, rules->key_bases, bits == 0 || bits == 64 ? ~0ull : (1ull << bits) - 1ull, two ? 1u : 0u, rules->prefer};
	const dim3 g_check = grid_threads(R), g_wave = grid_waves(R);
	hipLaunchKernelGGL(k_col_plan_check, g_check, dim3(WG), 0, s, c1, w1, res.d); KCHK();
	if (two) { hipLaunchKernelGGL(k_col_plan_check, g_check, dim3(WG), 0, s, c2, w2, res.d + 1); KCHK(); }
	hipLaunchKernelGGL(k_dedup_key, g_wave, dim3(WG), 0, s, in, AP<u64>(h, o_hash), AP<u64>(h, o_rank), res.counters(), res.d); KCHK();
	hipLaunchKernelGGL(k_dedup_insert, g_wave, dim3(WG), 0, s, in, AP<u64>(h, o_hash), AP<u64>(h, o_rank), t, AP<u32>(h, o_slot), res.d); KCHK();
	hipLaunchKernelGGL(k_dedup_resolve, g_check, dim3(WG), 0, s, d_keep_in, R, t, AP<u32>(h, o_slot), rules->prefer, d_keep, d_dup_of, d_copies, res.counters(), res.d); KCHK();
	if (const int rc = res_home(h, res, "dedup plan")) return rc;
	for (u32 k = 0; k < DEDUP_N_STATS; ++k) stats[k] = res.home()[k];
	return DSRCGPU_OK;
}

// the merge (k_columns_merge.h): the check pass per side as in the pair plan, the judge, then the select's three-launch placement over
// the judge's verdicts; the error words, the statistics and the totals come home in one copy, in front of the first kernel that writes
// the caller's arrays
int dsrcgpu_columns_merge_device(dsrcgpu_handle* h, const dsrcgpu_columns_in* in1, const dsrcgpu_columns_in* in2, const dsrcgpu_merge_rules* rules,
								 const uint64_t* d_begin1, const uint64_t* d_end1, const uint64_t* d_begin2, const uint64_t* d_end2, const uint8_t* d_keep,
								 const uint64_t* d_insert, const dsrcgpu_columns* out, uint8_t* d_merged, uint64_t* d_source, uint64_t totals[3],
								 uint64_t stats[12])
{
	if (!h) return DSRCGPU_E_ARG;
	if (!rules || !totals || !stats || !out) return fail(h, DSRCGPU_E_ARG, "null argument");
	totals[0] = totals[1] = totals[2] = 0;
	for (u32 k = 0; k < MERGE_N_STATS; ++k) stats[k] = 0;
	if (!out->d_titles && out->titles_cap) return fail(h, DSRCGPU_E_ARG, "columns: titles_cap without d_titles");
	const bool titles = out->d_titles != nullptr;
	ColIn c1, c2;
	if (const int rc = col_in_args(h, in1, COL_QUALS | (titles ? COL_TITLES : 0), c1)) return rc;
	if (const int rc = col_in_args(h, in2, COL_QUALS, c2)) return rc;
	if (c1.n_recs != c2.n_recs) return fail(h, DSRCGPU_E_ARG, "merge: %llu records of read 1, %llu of read 2", (unsigned long long)c1.n_recs, (unsigned long long)c2.n_recs);
	if (rules->min_overlap < 1) return fail(h, DSRCGPU_E_ARG, "merge rules: min_overlap of 0");
	if (rules->max_error_permille > 1000) return fail(h, DSRCGPU_E_ARG, "merge rules: max_error_permille above 1000");
	if (rules->quality_cap > 255) return fail(h, DSRCGPU_E_ARG, "merge rules: quality_cap above 255");
	if (const int rc = reserved_clear(h, "merge rules", rules->reserved)) return rc;
	if (const int rc = together(h, d_begin1, d_end1, "d_begin1", "d_end1")) return rc;
	if (const int rc = together(h, d_begin2, d_end2, "d_begin2", "d_end2")) return rc;
	if (!d_insert || !d_merged) return fail(h, DSRCGPU_E_ARG, "null argument");
	HIPCHK(hipSetDevice(h->device));
	hipStream_t s = h->stream;
	const auto nothing_merged = [&]() -> int {
		if (c1.n_recs) HIPCHK(hipMemsetAsync(d_merged, 0, (size_t)c1.n_recs, s));
		return nothing_out(h, out, titles);
	};
	if (c1.n_recs == 0) return nothing_merged();
	const u64 n_tiles = (c1.n_recs + WG - 1) / WG;
	const u32 n_res = 2 + MERGE_N_STATS + 3;             // an error word per side, the twelve statistics, the three totals
	if (const int rc = ensure_arena(h, (size_t)(3 * n_tiles + 2 * c1.n_recs + n_res) * 8 + 4096)) return rc;
	ResWords res = res_alloc(h, 2, MERGE_N_STATS + 3);
	u64* d_tiles = AP<u64>(h, h->arena.alloc((size_t)n_tiles * 24));
	u64* d_len = AP<u64>(h, h->arena.alloc((size_t)c1.n_recs * 8));
	u64* d_pos = AP<u64>(h, h->arena.alloc((size_t)c1.n_recs * 8));
	if (const int rc = res_begin(h, res, "columns merge")) return rc;
	HIPCHK(hipMemsetAsync(d_len, 0xFF, (size_t)c1.n_recs * 8, s));      // MERGE_NOT: a pair the judge does not reach is not merged
	const MergeWhat w{ColPlanIn{d_begin1, d_end1, nullptr}, ColPlanIn{d_begin2, d_end2, nullptr}, d_keep, d_insert};
	const MergeRules R{rules->min_overlap, rules->max_mismatches, rules->max_error_permille, rules->quality_cap};
	const dim3 g_check = grid_threads(c1.n_recs), g_waves = grid_waves(c1.n_recs);
	const u32 g_tiles = (u32)std::min<u64>(4096, n_tiles);
	hipLaunchKernelGGL(k_col_plan_check, g_check, dim3(WG), 0, s, c1, w.w1, res.d); KCHK();
	hipLaunchKernelGGL(k_col_plan_check, g_check, dim3(WG), 0, s, c2, w.w2, res.d + 1); KCHK();
	hipLaunchKernelGGL(k_merge_judge, g_waves, dim3(WG), 0, s, c1, c2, w, R, d_len, res.counters(), res.d); KCHK();
	hipLaunchKernelGGL(k_merge_tiles, dim3(g_tiles), dim3(WG), 0, s, c1, d_len, titles ? 1u : 0u, n_tiles, d_tiles, res.d); KCHK();
	hipLaunchKernelGGL(k_sel_scan_tiles, dim3(1), dim3(WG), 0, s, n_tiles, d_tiles, res.counters() + MERGE_N_STATS); KCHK();
	if (const int rc = res_home(h, res, "merge")) return rc;
	for (u32 k = 0; k < MERGE_N_STATS; ++k) stats[k] = res.home()[k];
	const u64* const tot = res.home() + MERGE_N_STATS;
	totals[0] = tot[0]; totals[1] = tot[1]; totals[2] = tot[2];
	if (const int rc = out_holds(h, out, titles, tot, "merge", "come out")) return rc;
	if (tot[0] == 0) return nothing_merged();
	SelOut o;
	if (const int rc = out_arrays(h, out, titles, true, d_source, tot, o)) return rc;
	hipLaunchKernelGGL(k_merge_apply, dim3(g_tiles), dim3(WG), 0, s, c1, d_len, titles ? 1u : 0u, n_tiles, d_tiles, o, d_merged, d_pos); KCHK();
	hipLaunchKernelGGL(k_merge_write, g_waves, dim3(WG), 0, s, c1, c2, w, R, d_len, d_pos, o, titles ? 1u : 0u); KCHK();
	HIPCHK(hipStreamSynchronize(s));
	return DSRCGPU_OK;
}

// the profile (k_columns_profile.h): the check pass of the adapter plan, then this call's profile is built in zeroed arena scratch and a
// small kernel stores it into the caller's array or adds it there -- both do nothing unless the error word is clean, so d_profile is
// untouched on an input error; the error word and the totals (the first eight words of the scratch) come home in one copy
int dsrcgpu_columns_profile(dsrcgpu_handle* h, const dsrcgpu_columns_in* in, const uint64_t* d_begin, const uint64_t* d_end, const uint8_t* d_keep,
							const dsrcgpu_profile_rules* rules, uint64_t* d_profile, uint64_t totals[8])
{
	if (!h) return DSRCGPU_E_ARG;
	if (!rules || !totals || !d_profile) return fail(h, DSRCGPU_E_ARG, "null argument");
	for (u32 k = 0; k < PROF_N_TOTALS; ++k) totals[k] = 0;
	ColIn c;
	if (const int rc = col_in_args(h, in, COL_QUALS, c)) return rc;
	if (rules->n_cycles < 1 || rules->n_cycles > DSRCGPU_PROFILE_MAX_CYCLES) return fail(h, DSRCGPU_E_ARG, "profile rules: n_cycles must be 1 .. %u", (u32)DSRCGPU_PROFILE_MAX_CYCLES);
	if (rules->accumulate > 1) return fail(h, DSRCGPU_E_ARG, "profile rules: accumulate must be 0 or 1");
	if (const int rc = reserved_clear(h, "profile rules", rules->reserved)) return rc;
	if (const int rc = together(h, d_begin, d_end, "d_begin", "d_end")) return rc;
	const u32 C = rules->n_cycles, words = PROF_WORDS(C);
	HIPCHK(hipSetDevice(h->device));
	hipStream_t s = h->stream;
	if (c.n_recs == 0)
	{
		if (!rules->accumulate) { HIPCHK(hipMemsetAsync(d_profile, 0, (size_t)words * 8, s)); HIPCHK(hipStreamSynchronize(s)); }
		return DSRCGPU_OK;
	}
	if (const int rc = ensure_arena(h, (size_t)(words + 1) * 8 + 1024)) return rc;
	ResWords res = res_alloc(h, 1, words);                // error word, this call's profile
	if (const int rc = res_begin(h, res, "columns profile")) return rc;
	const ColPlanIn w{d_begin, d_end, d_keep};
	const dim3 grid = grid_waves(c.n_recs, prof_max_grid(C));
	hipLaunchKernelGGL(k_col_plan_check, grid_threads(c.n_recs), dim3(WG), 0, s, c, w, res.d); KCHK();
	if (C <= PROF_SMALL_CYCLES) { hipLaunchKernelGGL(k_prof<PROF_SMALL_CYCLES>, grid, dim3(WG), 0, s, c, w, C, res.counters(), res.d); KCHK(); }
	else { hipLaunchKernelGGL(k_prof<PROF_MAX_CYCLES>, grid, dim3(WG), 0, s, c, w, C, res.counters(), res.d); KCHK(); }
	hipLaunchKernelGGL(k_prof_store, dim3((words + WG - 1) / WG), dim3(WG), 0, s, res.counters(), d_profile, words, rules->accumulate, res.d); KCHK();
	if (const int rc = res_home(h, res, nullptr, 1 + PROF_N_TOTALS)) return rc;
	for (u32 k = 0; k < PROF_N_TOTALS; ++k) totals[k] = res.home()[k];
	return DSRCGPU_OK;
}

// ---- k-mer count (k_columns_kmer.h) --------------------------------------------------------------------------------------------------
// the k-mer count: the header comes home first under accumulate, then the check pass of the adapter plan and the window count; the
// error word and W come home BEFORE the first launch that writes the table, so that every refusal leaves it untouched
int dsrcgpu_columns_kmer_count(dsrcgpu_handle* h, const dsrcgpu_columns_in* in, const uint64_t* d_begin, const uint64_t* d_end, const uint8_t* d_keep,
							   const dsrcgpu_kmer_rules* rules, uint64_t* d_table, uint64_t stats[16], uint64_t need[1])
{
	if (!h) return DSRCGPU_E_ARG;
	if (!rules || !stats || !need || !d_table) return fail(h, DSRCGPU_E_ARG, "null argument");
	for (u32 i = 0; i < KMER_N_STATS; ++i) stats[i] = 0;
	need[0] = 0;
	ColIn c;
	if (const int rc = col_in_args(h, in, 0, c)) return rc;
	const u32 k = rules->k, bits = rules->hash_bits;
	const u64 M = rules->capacity;
	if (k < 1 || k > DSRCGPU_KMER_MAX_K) return fail(h, DSRCGPU_E_ARG, "kmer rules: k must be 1 .. %u", (u32)DSRCGPU_KMER_MAX_K);
	if (rules->canonical > 1) return fail(h, DSRCGPU_E_ARG, "kmer rules: canonical must be 0 or 1");
	if (rules->accumulate > 1) return fail(h, DSRCGPU_E_ARG, "kmer rules: accumulate must be 0 or 1");
	if (bits > 64) return fail(h, DSRCGPU_E_ARG, "kmer rules: hash_bits above 64");
	if (M < 16 || M > (1ull << 40) || (M & (M - 1))) return fail(h, DSRCGPU_E_ARG, "kmer rules: capacity must be a power of two, 16 .. 2^40");
	if (const int rc = reserved_clear(h, "kmer rules", rules->reserved)) return rc;
	if (const int rc = together(h, d_begin, d_end, "d_begin", "d_end")) return rc;
	HIPCHK(hipSetDevice(h->device));
	hipStream_t s = h->stream;
	u64 hdr[8] = {kmer_header_word(k, rules->canonical, bits), M, 0, 0, 0, 0, 0, 0};
	const KmerTab t = kmer_tab(d_table, M, bits);
	if (rules->accumulate)
	{
		u64 have[8]; KmerTab th; u32 hk, hc;
		if (const int rc = kmer_table_home(h, d_table, "kmer count, accumulate", have, th, hk, hc)) return rc;
		if (have[0] != hdr[0] || have[1] != M)
			return fail(h, DSRCGPU_E_ARG, "kmer count, accumulate: the table holds k = %u, canonical = %u, capacity %llu; the rules ask for %u, %u, %llu (or another hash_bits)",
			            hk, hc, (unsigned long long)have[1], k, rules->canonical, (unsigned long long)M);
		for (u32 i = 0; i < 8; ++i) hdr[i] = have[i];
	}
	const auto init = [&]() -> int {
		HIPCHK(hipMemsetAsync(t.keys, 0xFF, (size_t)M * 8, s));
		HIPCHK(hipMemsetAsync(t.counts, 0, (size_t)M * 8, s));
		HIPCHK(hipMemcpyAsync(d_table, hdr, sizeof(hdr), hipMemcpyHostToDevice, s));
		return DSRCGPU_OK;
	};
	if (c.n_recs == 0)
	{
		if (!rules->accumulate) { if (const int rc = init()) return rc; HIPCHK(hipStreamSynchronize(s)); }
		stats[KMER_DISTINCT_AFTER] = hdr[2]; stats[KMER_TOTAL_AFTER] = hdr[3];
		return DSRCGPU_OK;
	}
	if (const int rc = ensure_arena(h, (1 + KMER_N_STATS) * 8 + 1024)) return rc;
	ResWords res = res_alloc(h, 1, KMER_N_STATS);         // the error word, the sixteen statistics
	if (const int rc = res_begin(h, res, "kmer count")) return rc;
	u64* const st = res.counters();
	const ColPlanIn w{d_begin, d_end, d_keep};
	hipLaunchKernelGGL(k_col_plan_check, grid_threads(c.n_recs), dim3(WG), 0, s, c, w, res.d); KCHK();
	hipLaunchKernelGGL(k_kmer_windows, grid_threads(c.n_recs), dim3(WG), 0, s, c, w, k, st, res.d); KCHK();
	if (const int rc = res_home(h, res)) return rc;
	const u64 W = res.home()[KMER_WINDOWS];
	if (hdr[2] + W > M / 4 * 3)
	{
		need[0] = kmer_need(hdr[2] + W);
		return fail(h, DSRCGPU_E_CAPACITY, "kmer count: %llu keys in the table and %llu windows in this call; a capacity of %llu holds %llu, %llu would do",
		            (unsigned long long)hdr[2], (unsigned long long)W, (unsigned long long)M, (unsigned long long)(M / 4 * 3), (unsigned long long)need[0]);
	}
	if (!rules->accumulate) { if (const int rc = init()) return rc; }
	const dim3 g_count = grid_waves(c.n_recs);
	const long variant = hook_int("DSRC_GPU_KMER_VARIANT", 0);       // test hook: 1 = no run aggregation, 2 = no plain load in front of the CAS
	if (variant == 1) { hipLaunchKernelGGL((k_kmer_count<false, true>), g_count, dim3(WG), 0, s, c, w, k, rules->canonical, t, st, res.d); KCHK(); }
	else if (variant == 2) { hipLaunchKernelGGL((k_kmer_count<true, false>), g_count, dim3(WG), 0, s, c, w, k, rules->canonical, t, st, res.d); KCHK(); }
	else { hipLaunchKernelGGL((k_kmer_count<true, true>), g_count, dim3(WG), 0, s, c, w, k, rules->canonical, t, st, res.d); KCHK(); }
	hipLaunchKernelGGL(k_kmer_header, dim3(1), dim3(64), 0, s, d_table, st + KMER_NEW, st + KMER_COUNTED, st + KMER_OVERFLOW, 0ull,
	                   st + KMER_DISTINCT_AFTER, st + KMER_TOTAL_AFTER, res.d); KCHK();
	if (const int rc = res_home(h, res)) return rc;
	for (u32 i = 0; i < KMER_N_STATS; ++i) stats[i] = res.home()[i];
	return DSRCGPU_OK;
}

// both headers come home and are checked, the 3/4 rule is applied to what the destination may hold afterwards, then the merge
int dsrcgpu_kmer_table_merge(dsrcgpu_handle* h, const uint64_t* d_src, uint64_t* d_dst, uint64_t stats[8], uint64_t need[1])
{
	if (!h) return DSRCGPU_E_ARG;
	if (!d_src || !d_dst || !stats || !need) return fail(h, DSRCGPU_E_ARG, "null argument");
	for (u32 i = 0; i < KMERGE_N_STATS; ++i) stats[i] = 0;
	need[0] = 0;
	if (d_src == d_dst) return fail(h, DSRCGPU_E_ARG, "kmer merge: a table cannot be merged into itself");
	if (const int rc = queue_idle(h)) return rc;
	HIPCHK(hipSetDevice(h->device));
	hipStream_t s = h->stream;
	u64 hs[8], hd[8]; KmerTab ts, td; u32 ks, cs, kd, cd;
	if (const int rc = kmer_table_home(h, d_src, "kmer merge, source", hs, ts, ks, cs)) return rc;
	if (const int rc = kmer_table_home(h, d_dst, "kmer merge, destination", hd, td, kd, cd)) return rc;
	if (ks != kd || cs != cd) return fail(h, DSRCGPU_E_ARG, "kmer merge: the source holds k = %u, canonical = %u, the destination %u, %u", ks, cs, kd, cd);
	if (hd[2] + hs[2] > hd[1] / 4 * 3)
	{
		need[0] = kmer_need(hd[2] + hs[2]);
		return fail(h, DSRCGPU_E_CAPACITY, "kmer merge: %llu keys in the destination and %llu in the source; a capacity of %llu holds %llu, %llu would do",
		            (unsigned long long)hd[2], (unsigned long long)hs[2], (unsigned long long)hd[1], (unsigned long long)(hd[1] / 4 * 3), (unsigned long long)need[0]);
	}
	if (const int rc = ensure_arena(h, KMERGE_N_STATS * 8 + 1024)) return rc;
	ResWords res = res_alloc(h, 0, KMERGE_N_STATS);
	if (const int rc = res_begin(h, res, "kmer merge")) return rc;
	const u64 slots = hs[1];
	hipLaunchKernelGGL(k_kmer_merge, grid_threads(slots, 4096), dim3(WG), 0, s, ts.keys, ts.counts, slots, td, res.d); KCHK();
	hipLaunchKernelGGL(k_kmer_header, dim3(1), dim3(64), 0, s, d_dst, res.d + KMERGE_NEW, res.d + KMERGE_ADDED, res.d + KMERGE_OVERFLOW, hs[4],
	                   res.d + KMERGE_DISTINCT_AFTER, res.d + KMERGE_TOTAL_AFTER, (const u64*)nullptr); KCHK();
	if (const int rc = res_home(h, res)) return rc;
	for (u32 i = 0; i < KMERGE_N_STATS; ++i) stats[i] = res.home()[i];
	return DSRCGPU_OK;
}

int dsrcgpu_kmer_spectrum(dsrcgpu_handle* h, const uint64_t* d_table, uint32_t n_bins, uint64_t* d_hist, uint64_t totals[4])
{
	if (!h) return DSRCGPU_E_ARG;
	if (!d_table || !d_hist || !totals) return fail(h, DSRCGPU_E_ARG, "null argument");
	for (u32 i = 0; i < KSPEC_N_TOTALS; ++i) totals[i] = 0;
	if (n_bins < 2 || n_bins > DSRCGPU_KMER_MAX_BINS) return fail(h, DSRCGPU_E_ARG, "kmer spectrum: n_bins must be 2 .. %u", (u32)DSRCGPU_KMER_MAX_BINS);
	if (const int rc = queue_idle(h)) return rc;
	HIPCHK(hipSetDevice(h->device));
	hipStream_t s = h->stream;
	u64 hdr[8]; KmerTab t; u32 k, canonical;
	if (const int rc = kmer_table_home(h, d_table, "kmer spectrum", hdr, t, k, canonical)) return rc;
	if (const int rc = ensure_arena(h, KSPEC_N_TOTALS * 8 + 1024)) return rc;
	ResWords res = res_alloc(h, 0, KSPEC_N_TOTALS);
	if (const int rc = res_begin(h, res, "kmer spectrum")) return rc;
	HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)n_bins * 8, s));
	const u64 slots = hdr[1];
	// (every workgroup ends with a flush of its LDS bins: no more workgroups than the chip holds at a time)
	hipLaunchKernelGGL(k_kmer_spectrum, grid_threads(slots, 512), dim3(WG), 0, s, t.keys, t.counts, slots, n_bins, d_hist, res.d); KCHK();
	if (const int rc = res_home(h, res)) return rc;
	for (u32 i = 0; i < KSPEC_N_TOTALS; ++i) totals[i] = res.home()[i];
	return DSRCGPU_OK;
}

int dsrcgpu_kmer_lookup(dsrcgpu_handle* h, const uint64_t* d_table, const uint64_t* d_kmers, uint64_t n, uint64_t* d_counts, uint64_t* invalid)
{
	if (!h) return DSRCGPU_E_ARG;
	if (!d_table || !invalid) return fail(h, DSRCGPU_E_ARG, "null argument");
	*invalid = 0;
	if (n >> 56) return fail(h, DSRCGPU_E_ARG, "kmer lookup: 2^56 queries and more");
	if (n && (!d_kmers || !d_counts)) return fail(h, DSRCGPU_E_ARG, "null argument");
	if (const int rc = queue_idle(h)) return rc;
	HIPCHK(hipSetDevice(h->device));
	hipStream_t s = h->stream;
	u64 hdr[8]; KmerTab t; u32 k, canonical;
	if (const int rc = kmer_table_home(h, d_table, "kmer lookup", hdr, t, k, canonical)) return rc;
	if (n == 0) return DSRCGPU_OK;
	if (const int rc = ensure_arena(h, 8 + 1024)) return rc;
	ResWords res = res_alloc(h, 0, 1);                    // the queries that are no k-mers
	if (const int rc = res_begin(h, res, "kmer lookup")) return rc;
	hipLaunchKernelGGL(k_kmer_lookup, grid_threads(n, 4096), dim3(WG), 0, s, t, k, canonical, d_kmers, n, d_counts, res.d); KCHK();
	if (const int rc = res_home(h, res)) return rc;
	*invalid = res.home()[0];
	return DSRCGPU_OK;
}

// the k-mer plan (k_columns_kmer_plan.h): the table's header comes home as for a lookup, then the check pass of the adapter plan and
// the planner run back to back.  Under want_median the error word and the most windows of any considered record come home in
// between: records with more windows than a wave keeps in LDS get a slice of arena scratch per wave of the grid, and the grid is
// cut down so that the slices stay under KPLAN_SPILL_BYTES (fewer waves in flight, the same result).
int dsrcgpu_columns_kmer_plan(dsrcgpu_handle* h, const dsrcgpu_columns_in* in, const dsrcgpu_kmer_plan_rules* rules, const uint64_t* d_table,
							  const uint64_t* d_begin_in, const uint64_t* d_end_in, const uint8_t* d_keep_in,
							  uint64_t* d_begin, uint64_t* d_end, uint8_t* d_keep, uint64_t* d_good, uint64_t* d_hits, uint64_t* d_median,
							  uint64_t stats[16])
{
	if (!h) return DSRCGPU_E_ARG;
	if (!rules || !stats || !d_table) return fail(h, DSRCGPU_E_ARG, "null argument");
	static_assert(KMER_PLAN_LDS_WINDOWS == DSRCGPU_KMER_PLAN_LDS_WINDOWS && KMER_PLAN_COUNT_CAP == DSRCGPU_KMER_PLAN_COUNT_CAP, "the header's figures are the kernel's");
	for (u32 i = 0; i < KPLAN_N_STATS; ++i) stats[i] = 0;
	ColIn c;
	if (const int rc = col_in_args(h, in, 0, c)) return rc;
	if (rules->min_count < 1) return fail(h, DSRCGPU_E_ARG, "kmer plan rules: min_count must be at least 1");
	if (rules->min_hit_permille > 1000 || rules->max_hit_permille > 1000) return fail(h, DSRCGPU_E_ARG, "kmer plan rules: a permille above 1000");
	if (rules->trim > KPLAN_TRIM_FIRST_HIT) return fail(h, DSRCGPU_E_ARG, "kmer plan rules: trim must be 0, 1 or 2");
	if (rules->want_median > 1) return fail(h, DSRCGPU_E_ARG, "kmer plan rules: want_median must be 0 or 1");
	if (!rules->want_median && (rules->min_median != 0 || rules->max_median != KMER_PLAN_NO_LIMIT || d_median))
		return fail(h, DSRCGPU_E_ARG, "kmer plan rules: a median bound or d_median without want_median");
	if (const int rc = reserved_clear(h, "kmer plan rules", rules->reserved)) return rc;
	if (const int rc = together(h, d_begin_in, d_end_in, "d_begin_in", "d_end_in")) return rc;
	if (c.n_recs && (!d_begin || !d_end || !d_keep)) return fail(h, DSRCGPU_E_ARG, "null argument");
	HIPCHK(hipSetDevice(h->device));
	hipStream_t s = h->stream;
	u64 hdr[8]; KmerTab t; u32 k, canonical;
	if (const int rc = kmer_table_home(h, d_table, "kmer plan", hdr, t, k, canonical)) return rc;
	if (c.n_recs == 0) return DSRCGPU_OK;
	const bool median = rules->want_median != 0;
	const size_t res_bytes = (2 + KPLAN_N_STATS) * 8;     // the error word, the sixteen statistics, the most windows of a record
	if (const int rc = ensure_arena(h, res_bytes + 1024)) return rc;
	ResWords res = res_alloc(h, 1, KPLAN_N_STATS + 1);
	if (const int rc = res_begin(h, res, "kmer plan")) return rc;
	const ColPlanIn w{d_begin_in, d_end_in, d_keep_in};
	const u64 wpg = WG / 64;
	u64 gx = grid_waves(c.n_recs).x;
	hipLaunchKernelGGL(k_col_plan_check, grid_threads(c.n_recs), dim3(WG), 0, s, c, w, res.d); KCHK();
	u16* d_spill = nullptr;
	u64 stride = 0;
	if (median)
	{
		hipLaunchKernelGGL(k_kmer_plan_longest, grid_threads(c.n_recs), dim3(WG), 0, s, c, w, k, res.counters() + KPLAN_N_STATS, res.d); KCHK();
		if (const int rc = res_home(h, res)) return rc;
		const u64 longest = res.home()[KPLAN_N_STATS];
		if (longest > KMER_PLAN_LDS_WINDOWS)
		{
			stride = (longest + 63) & ~63ull;
			const u64 per_group = stride * 2 * wpg;
			gx = std::max<u64>(1, std::min<u64>(gx, KPLAN_SPILL_BYTES / per_group));
			// the arena starts again (it may move): the error word is known to be clean and is set up anew
			if (const int rc = ensure_arena(h, res_bytes + (size_t)(gx * per_group) + 1024)) return rc;
			res = res_alloc(h, 1, KPLAN_N_STATS + 1);
			d_spill = AP<u16>(h, h->arena.alloc((size_t)(gx * per_group)));
			if (const int rc = res_begin(h, res, "kmer plan")) return rc;
		}
	}
	const KmerPlanRules R{rules->min_count, rules->min_hits, rules->max_hits, rules->min_hit_permille, rules->max_hit_permille, rules->min_median,
	                      rules->max_median, rules->trim, rules->min_length};
	const KmerPlanOut o{d_begin, d_end, d_keep, d_good, d_hits, d_median};
	if (median) { hipLaunchKernelGGL(k_kmer_plan<true>, dim3((u32)gx), dim3(WG), 0, s, c, w, k, canonical, t, R, o, d_spill, stride, res.counters(), res.d); KCHK(); }
	else { hipLaunchKernelGGL(k_kmer_plan<false>, dim3((u32)gx), dim3(WG), 0, s, c, w, k, canonical, t, R, o, d_spill, stride, res.counters(), res.d); KCHK(); }
	if (const int rc = res_home(h, res, nullptr, 1 + KPLAN_N_STATS)) return rc;
	for (u32 i = 0; i < KPLAN_N_STATS; ++i) stats[i] = res.home()[i];
	return DSRCGPU_OK;
}

// the k-mer correction (k_columns_kmer_correct.h): the table's header comes home as for the plan, then the check pass of the adapter
// plan, out of place the copy of the span, and the corrector run back to back.  Both kernels behind the check pass look at its error
// word first, so that an input error leaves d_bases_out and d_fixed as they were.
int dsrcgpu_columns_kmer_correct(dsrcgpu_handle* h, const dsrcgpu_columns_in* in, const dsrcgpu_kmer_correct_rules* rules, const uint64_t* d_table,
								 const uint64_t* d_begin, const uint64_t* d_end, const uint8_t* d_keep, uint8_t* d_bases_out, uint64_t* d_fixed,
								 uint64_t stats[16])
{
	if (!h) return DSRCGPU_E_ARG;
	if (!rules || !stats || !d_table || !d_bases_out) return fail(h, DSRCGPU_E_ARG, "null argument");
	for (u32 i = 0; i < KCORR_N_STATS; ++i) stats[i] = 0;
	if (rules->max_quality > 255) return fail(h, DSRCGPU_E_ARG, "kmer correct rules: max_quality above 255");
	ColIn c;
	if (const int rc = col_in_args(h, in, rules->max_quality < 255 ? COL_QUALS : 0, c)) return rc;
	if (rules->min_count < 1) return fail(h, DSRCGPU_E_ARG, "kmer correct rules: min_count must be at least 1");
	if (const int rc = reserved_clear(h, "kmer correct rules", rules->reserved)) return rc;
	if (const int rc = together(h, d_begin, d_end, "d_begin", "d_end")) return rc;
	HIPCHK(hipSetDevice(h->device));
	hipStream_t s = h->stream;
	u64 hdr[8]; KmerTab t; u32 k, canonical;
	if (const int rc = kmer_table_home(h, d_table, "kmer correct", hdr, t, k, canonical)) return rc;
	if (c.n_recs == 0) return DSRCGPU_OK;
	if (const int rc = ensure_arena(h, (1 + KCORR_N_STATS) * 8 + 1024)) return rc;
	ResWords res = res_alloc(h, 1, KCORR_N_STATS);        // the error word, the sixteen statistics
	if (const int rc = res_begin(h, res, "kmer correct")) return rc;
	const ColPlanIn w{d_begin, d_end, d_keep};
	const KmerCorrectRules R{rules->min_count, rules->max_quality};
	hipLaunchKernelGGL(k_col_plan_check, grid_threads(c.n_recs), dim3(WG), 0, s, c, w, res.d); KCHK();
	if (d_bases_out != c.bases) { hipLaunchKernelGGL(k_kmer_correct_copy, grid_threads(c.bases_len / 8 + 1, 4096), dim3(WG), 0, s, c, d_bases_out, res.d); KCHK(); }
	hipLaunchKernelGGL(k_kmer_correct, grid_waves(c.n_recs), dim3(WG), 0, s, c, w, k, canonical, t, R, d_bases_out, d_fixed, res.counters(), res.d); KCHK();
	if (const int rc = res_home(h, res)) return rc;
	for (u32 i = 0; i < KCORR_N_STATS; ++i) stats[i] = res.home()[i];
	return DSRCGPU_OK;
}

// the demultiplex plan (k_columns_demux.h): the rules are checked and every sample's barcodes packed into bit planes here (four words a
// sample, uploaded to arena scratch), then the check pass of the adapter plan once per column set, each with an error word of its own
// (`in` is reported first), and the planner; the error words and the statistics come home in one copy
int dsrcgpu_columns_demux_plan(dsrcgpu_handle* h, const dsrcgpu_columns_in* in, const dsrcgpu_columns_in* const* index_sets, uint32_t n_index_sets,
							   const dsrcgpu_demux_rules* rules, const uint64_t* d_begin_in, const uint64_t* d_end_in, const uint8_t* d_keep_in,
							   uint64_t* d_begin, uint64_t* d_end, uint8_t* d_keep, uint32_t* d_class, uint32_t* d_info, uint64_t* d_class_counts,
							   uint64_t stats[9])
{
	if (!h) return DSRCGPU_E_ARG;
	if (!rules || !stats) return fail(h, DSRCGPU_E_ARG, "null argument");
	for (u32 k = 0; k < DMX_STATS; ++k) stats[k] = 0;
	ColIn c, ci[2] = {};
	if (const int rc = col_in_args(h, in, 0, c)) return rc;
	if (n_index_sets > 2) return fail(h, DSRCGPU_E_ARG, "demux: at most 2 index read sets");
	if (n_index_sets && !index_sets) return fail(h, DSRCGPU_E_ARG, "null argument");
	for (u32 k = 0; k < n_index_sets; ++k)
	{
		if (const int rc = col_in_args(h, index_sets[k], 0, ci[k])) return rc;
		if (ci[k].n_recs != c.n_recs) return fail(h, DSRCGPU_E_ARG, "demux: %llu records of the reads, %llu of index set %u", (unsigned long long)c.n_recs, (unsigned long long)ci[k].n_recs, k + 1);
	}
	if (rules->n_samples < 1 || rules->n_samples > DSRCGPU_DEMUX_MAX_SAMPLES) return fail(h, DSRCGPU_E_ARG, "demux rules: n_samples must be 1 .. %u", (u32)DSRCGPU_DEMUX_MAX_SAMPLES);
	if (rules->n_slots < 1 || rules->n_slots > 2) return fail(h, DSRCGPU_E_ARG, "demux rules: n_slots must be 1 or 2");
	if (rules->cut > 1 || rules->keep_unassigned > 1) return fail(h, DSRCGPU_E_ARG, "demux rules: cut and keep_unassigned must be 0 or 1");
	DemuxRules R{};
	R.n_samples = rules->n_samples; R.n_slots = rules->n_slots; R.max_total = rules->max_mismatches; R.min_delta = rules->min_delta;
	R.cut = rules->cut; R.keep_unassigned = rules->keep_unassigned; R.min_len = rules->min_length;
	u32 all_len = 0;
	for (u32 s = 0; s < 2; ++s)
	{
		if (s >= R.n_slots)
		{
			if (rules->slot_source[s] | rules->slot_offset[s] | rules->slot_len[s] | rules->slot_max_mismatches[s]) return fail(h, DSRCGPU_E_ARG, "demux rules: a figure of slot %u behind n_slots", s);
			continue;
		}
		if (rules->slot_source[s] > n_index_sets) return fail(h, DSRCGPU_E_ARG, "demux rules: slot %u reads source %u, %u index read sets were given", s, rules->slot_source[s], n_index_sets);
		if (rules->slot_len[s] < 1 || rules->slot_len[s] > DSRCGPU_DEMUX_MAX_BARCODE) return fail(h, DSRCGPU_E_ARG, "demux rules: slot %u: a length of 1 .. %u is needed", s, (u32)DSRCGPU_DEMUX_MAX_BARCODE);
		R.src[s] = rules->slot_source[s]; R.off[s] = rules->slot_offset[s]; R.len[s] = rules->slot_len[s]; R.max_mm[s] = rules->slot_max_mismatches[s];
		R.mask[s] = R.len[s] == 64 ? ~0ull : (1ull << R.len[s]) - 1ull;
		all_len += R.len[s];
		if (R.src[s] == 0)
		{
			if ((u64)R.off[s] + R.len[s] > 0xFFFFFFFFull) return fail(h, DSRCGPU_E_ARG, "demux rules: slot %u: offset + length above 2^32 - 1", s);
			R.cut_len = std::max(R.cut_len, R.off[s] + R.len[s]);
		}
	}
	if (rules->max_mismatches > all_len) return fail(h, DSRCGPU_E_ARG, "demux rules: max_mismatches above the summed barcode lengths");
	if (!rules->barcodes) return fail(h, DSRCGPU_E_ARG, "null argument");
	std::vector<u64> tab((size_t)4 * R.n_samples, 0);
	for (u32 a = 0; a < R.n_samples; ++a)
		for (u32 j = 0; j < all_len; ++j)
		{
			const u32 code = rules->barcodes[(size_t)a * all_len + j];
			if (code > 3) return fail(h, DSRCGPU_E_ARG, "demux rules: sample %u: code %u at position %u (A C G T = 0 .. 3 only)", a, code, j);
			const u32 s = j < R.len[0] ? 0 : 1, bit = s ? j - R.len[0] : j;
			tab[4 * a + 2 * s] |= (u64)(code & 1u) << bit; tab[4 * a + 2 * s + 1] |= (u64)(code >> 1) << bit;
		}
	{	// two samples with the same barcodes in every slot: sorted copies side by side
		std::vector<std::array<u64, 4>> keys(R.n_samples);
		for (u32 a = 0; a < R.n_samples; ++a) keys[a] = {tab[4 * a], tab[4 * a + 1], tab[4 * a + 2], tab[4 * a + 3]};
		std::sort(keys.begin(), keys.end());
		if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) return fail(h, DSRCGPU_E_ARG, "demux rules: two samples have the same barcodes");
	}
	if (const int rc = reserved_clear(h, "demux rules", rules->reserved)) return rc;
	if (const int rc = together(h, d_begin_in, d_end_in, "d_begin_in", "d_end_in")) return rc;
	if (c.n_recs == 0) return DSRCGPU_OK;
	if (!d_begin || !d_end || !d_keep || !d_class) return fail(h, DSRCGPU_E_ARG, "null argument");
	HIPCHK(hipSetDevice(h->device));
	hipStream_t s = h->stream;
	if (const int rc = ensure_arena(h, (3 + DMX_STATS) * 8 + tab.size() * 8 + 1024)) return rc;
	ResWords res = res_alloc(h, 3, DMX_STATS);            // an error word per column set, the nine statistics
	u64* d_tab = AP<u64>(h, h->arena.alloc(tab.size() * 8));
	if (const int rc = res_begin(h, res, "demux plan")) return rc;
	HIPCHK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
	const ColPlanIn w{d_begin_in, d_end_in, d_keep_in}, whole{nullptr, nullptr, nullptr};
	const DemuxSrc x1{ci[0].bases, ci[0].seq_offs, ci[0].bases_len}, x2{ci[1].bases, ci[1].seq_offs, ci[1].bases_len};
	hipLaunchKernelGGL(k_col_plan_check, grid_threads(c.n_recs), dim3(WG), 0, s, c, w, res.d); KCHK();
	for (u32 k = 0; k < n_index_sets; ++k) { hipLaunchKernelGGL(k_col_plan_check, grid_threads(c.n_recs), dim3(WG), 0, s, ci[k], whole, res.d + 1 + k); KCHK(); }
	hipLaunchKernelGGL(k_demux_plan, grid_threads(c.n_recs, DMX_GRID), dim3(WG), 0, s, c, w, x1, x2, R, d_tab, d_begin, d_end, d_keep, d_class, d_info, d_class_counts,
	                   res.counters(), res.d); KCHK();
	if (const int rc = res_home(h, res, "dsrcgpu_columns_demux_plan")) return rc;
	for (u32 k = 0; k < DMX_STATS; ++k) stats[k] = res.home()[k];
	return DSRCGPU_OK;
}

// the partition (k_columns_demux.h): the count pass and the scan of its (class, tile) counts first -- the error word, the four totals
// and the class prefix come home in one synchronisation, in front of the first kernel that writes the caller's arrays -- then the
// rank pass gives the output order, the select's placement runs over it, and k_sel_gather moves the bytes
int dsrcgpu_columns_partition_device(dsrcgpu_handle* h, const dsrcgpu_columns_in* in, const uint64_t* d_begin, const uint64_t* d_end, const uint8_t* d_keep,
									 const uint32_t* d_class, uint32_t n_classes, const dsrcgpu_columns* out, uint64_t* d_source,
									 uint64_t* class_records, uint64_t totals[4])
{
	if (!h) return DSRCGPU_E_ARG;
	if (!out || !totals) return fail(h, DSRCGPU_E_ARG, "null argument");
	totals[0] = totals[1] = totals[2] = totals[3] = 0;
	if (n_classes < 1 || n_classes > DMX_MAX_CLASSES) return fail(h, DSRCGPU_E_ARG, "partition: n_classes must be 1 .. %u", (u32)DMX_MAX_CLASSES);
	if (!class_records) return fail(h, DSRCGPU_E_ARG, "null argument");
	for (u32 k = 0; k <= n_classes; ++k) class_records[k] = 0;
	if (const int rc = together(h, d_begin, d_end, "d_begin", "d_end")) return rc;
	if (!out->d_titles && out->titles_cap) return fail(h, DSRCGPU_E_ARG, "columns: titles_cap without d_titles");
	const bool titles = out->d_titles != nullptr;
	ColIn c;
	if (const int rc = col_in_args(h, in, COL_QUALS | (titles ? COL_TITLES : 0), c)) return rc;
	if (c.n_recs && !d_class) return fail(h, DSRCGPU_E_ARG, "null argument");
	HIPCHK(hipSetDevice(h->device));
	hipStream_t s = h->stream;
	if (c.n_recs == 0) return nothing_out(h, out, titles);
	const u64 n_tiles = (c.n_recs + WG - 1) / WG, n_counts = (u64)n_classes * n_tiles, n_chunks = (n_counts + WG - 1) / WG;
	if (const int rc = ensure_arena(h, (size_t)(n_counts + n_chunks + n_classes + 3 * n_tiles + 2 * c.n_recs + 16) * 8 + 8 * 256 + 4096)) return rc;
	ResWords res = res_alloc(h, 1, PART_TOTALS, 4);       // error word, the four totals, the scan's total and the placement's three
	u64* d_counts = AP<u64>(h, h->arena.alloc((size_t)n_counts * 8));
	u64* d_chunks = AP<u64>(h, h->arena.alloc((size_t)n_chunks * 8));
	u64* d_crecs = AP<u64>(h, h->arena.alloc((size_t)(n_classes + 1) * 8));
	u64* d_tiles = AP<u64>(h, h->arena.alloc((size_t)n_tiles * 24));
	u64* d_order = AP<u64>(h, h->arena.alloc((size_t)c.n_recs * 8));
	u64* d_pos = AP<u64>(h, h->arena.alloc((size_t)c.n_recs * 8));
	if (const int rc = res_begin(h, res, "columns partition")) return rc;
	const PartWhat p{SelWhat{d_begin, d_end, d_keep, titles ? 1u : 0u}, d_class, n_classes};
	u64* const d_total = res.counters() + PART_TOTALS;
	const u32 g_tiles = (u32)std::min<u64>(4096, n_tiles), g_chunks = (u32)std::min<u64>(4096, n_chunks);
	hipLaunchKernelGGL(k_part_count, dim3(g_tiles), dim3(WG), 0, s, c, p, n_tiles, d_counts, res.counters(), res.d); KCHK();
	hipLaunchKernelGGL(k_part_scan_sums, dim3(g_chunks), dim3(WG), 0, s, n_counts, d_counts, n_chunks, d_chunks); KCHK();
	hipLaunchKernelGGL(k_part_scan_chunks, dim3(1), dim3(WG), 0, s, n_chunks, d_chunks, d_total); KCHK();
	hipLaunchKernelGGL(k_part_scan_apply, dim3(g_chunks), dim3(WG), 0, s, n_counts, d_counts, n_chunks, d_chunks); KCHK();
	hipLaunchKernelGGL(k_part_class_records, dim3(1), dim3(WG), 0, s, d_counts, n_tiles, n_classes, d_total, d_crecs); KCHK();
	std::vector<u64> crecs((size_t)n_classes + 1);
	HIPCHK(hipMemcpyAsync(crecs.data(), d_crecs, crecs.size() * 8, hipMemcpyDeviceToHost, s));
	if (const int rc = res_home(h, res, nullptr, 1 + PART_TOTALS)) return rc;
	const u64* const tot = res.home();
	for (u32 k = 0; k < PART_TOTALS; ++k) totals[k] = tot[k];
	for (u32 k = 0; k <= n_classes; ++k) class_records[k] = crecs[k];
	if (const int rc = out_holds(h, out, titles, tot, "partition", "come out")) return rc;
	if (tot[0] == 0) return nothing_out(h, out, titles);
	SelOut o;
	if (const int rc = out_arrays(h, out, titles, tot[1] != 0, d_source, tot, o)) return rc;
	const u64 n_out = tot[0], n_otiles = (n_out + WG - 1) / WG;
	const u32 g_otiles = (u32)std::min<u64>(4096, n_otiles);
	HIPCHK(hipMemsetAsync(d_order, 0xFF, (size_t)n_out * 8, s));          // (no record)
	HIPCHK(hipMemsetAsync(d_pos, 0xFF, (size_t)c.n_recs * 8, s));         // SEL_DROPPED
	hipLaunchKernelGGL(k_part_rank, dim3(g_tiles), dim3(WG), 0, s, c, p, n_tiles, d_counts, n_out, d_order); KCHK();
	hipLaunchKernelGGL(k_part_place_tiles, dim3(g_otiles), dim3(WG), 0, s, c, p, d_order, n_out, n_otiles, d_tiles); KCHK();
	hipLaunchKernelGGL(k_sel_scan_tiles, dim3(1), dim3(WG), 0, s, n_otiles, d_tiles, d_total + 1); KCHK();
	hipLaunchKernelGGL(k_part_place_apply, dim3(g_otiles), dim3(WG), 0, s, c, p, d_order, n_out, n_otiles, d_tiles, o, d_pos); KCHK();
	hipLaunchKernelGGL(k_sel_gather, grid_waves(c.n_recs), dim3(WG), 0, s, c, p.w, o, d_pos); KCHK();
	HIPCHK(hipStreamSynchronize(s));
	return DSRCGPU_OK;
}

} // extern "C"
