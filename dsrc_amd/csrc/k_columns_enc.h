// Columnar encode: the way back from k_columns.h -- record arrays in HBM become the chunk text that run_batch compresses
// (include/dsrc_gpu.h: dsrcgpu_compress_columns_device, dsrcgpu_columns_cut).  The kernels only READ the caller's arrays.  No
// counterpart in the reference, whose writers take text (or one record at a time: DsrcArchive::WriteNextRecord).
//
// Record r's line group is  title \n letters \n plus \n qualities+offset \n  with plus = "+" or "+" and the title without its '@'
// (plus_repetition), so with T = d_title_offs, S = d_seq_offs and pr = 0 / 1
//     P(r) = (1 + pr) * T[r] + 2 * S[r] + (5 - pr) * r
// grows by exactly the bytes of record r from r to r + 1: the text of records f .. e - 1 has P(e) - P(f) - 1 bytes (no newline after
// the last one) and record r of that chunk starts at P(r) - P(f).  Positions are closed-form in the two offset arrays: no prefix pass.
#pragma once
#include "k_common.h"
#include "k_columns_common.h"

// ---- the check pass ------------------------------------------------------------------------------------------------------
// grid (gx), a wave per record, lanes stride over the record's bytes.  A record's own four offsets are checked first (in order, closing
// entry inside the array), and only then are its bytes read: whatever the other records' offsets say, no lane reads outside the
// caller's arrays.  Nothing is written but the error word and -- by the first workgroup -- P at the n_cuts cut points (cut[] holds record
// indices <= n_recs, checked by the host, so the two offset arrays are read inside their n_recs + 1 entries).
__global__ void __launch_bounds__(WG) k_col_check(ColIn c, const u64* cut, u32 n_cuts, u64* cut_pos, u64* err)
{
	if (blockIdx.x == 0)
		for (u32 i = threadIdx.x; i < n_cuts; i += blockDim.x) { const u64 r = cut[i]; cut_pos[i] = col_pos(c, r, c.seq_offs[r], c.title_offs[r]); }
	const u32 lane = lane_id();
	const u64 wpg = blockDim.x >> 6;
	for (u64 r = blockIdx.x * wpg + wave_id(); r < c.n_recs; r += gridDim.x * wpg)
	{
		const u64 s0 = c.seq_offs[r], s1 = c.seq_offs[r + 1], t0 = c.title_offs[r], t1 = c.title_offs[r + 1];
		u32 bad = 0;                                       // (wave-uniform: every lane has read the same four words)
		if (s0 > s1) bad |= 1u << COLE_SEQ_ORDER; else if (s1 > c.bases_len) bad |= 1u << COLE_SEQ_END;
		if (t0 > t1) bad |= 1u << COLE_TITLE_ORDER; else if (t1 > c.titles_len) bad |= 1u << COLE_TITLE_END; else if (t0 == t1) bad |= 1u << COLE_TITLE_EMPTY;
		if (!(bad & 0x3u))
			for (u64 p = s0 + lane; p < s1; p += 64)
			{
				if (c.bases[p] > 18u) bad |= 1u << COLE_BASE;
				if ((u32)c.quals[p] + c.qoff > 126u) bad |= 1u << COLE_QUAL;
			}
		if (!(bad & 0x1Cu))
			for (u64 p = t0 + lane; p < t1; p += 64)
			{
				const u32 ch = c.titles[p];
				if (p == t0 && ch != '@') bad |= 1u << COLE_TITLE_AT;
				if (ch == '\n') bad |= 1u << COLE_TITLE_NL;
			}
		if (bad) col_err(err, r, (u32)__ffs((int)bad) - 1u);
	}
}

// ---- columns -> chunk text (the inverse of k_col_gather) -----------------------------------------------------------------------
// per block: first record and one past the last, P(first), where the chunk starts in the text buffer
struct ColEncBlk { u64 first, end, pos0, text_off; };

// grid (gx, B), a wave per record, a byte per lane: neighbouring lanes store neighbouring bytes.  code -> letter through a table in
// LDS (32 entries, the index masked: the check pass has refused codes above 18, the mask keeps a read inside the table regardless).
// Runs only behind a clean check pass: every offset is in order and inside its array, the host has sized the chunks from the same P.
__global__ void __launch_bounds__(WG) k_col_scatter(ColIn c, const ColEncBlk* blk, u8* text_all)
{
	__shared__ u8 s_let[32];
	const char* const letters = "ACGTNRWSKMDVHBYXU.-";
	if (threadIdx.x < 32) s_let[threadIdx.x] = threadIdx.x < 19 ? (u8)letters[threadIdx.x] : (u8)'N';
	__syncthreads();
	const ColEncBlk B = blk[blockIdx.y];
	u8* const text = text_all + B.text_off;
	const u32 lane = lane_id();
	const u64 wpg = blockDim.x >> 6;
	for (u64 r = B.first + blockIdx.x * wpg + wave_id(); r < B.end; r += gridDim.x * wpg)
	{
		const u64 s0 = c.seq_offs[r], sl = c.seq_offs[r + 1] - s0, t0 = c.title_offs[r], tl = c.title_offs[r + 1] - t0;
		u8* const d_title = text + (col_pos(c, r, s0, t0) - B.pos0);
		u8* const d_seq = d_title + tl + 1;
		u8* const d_plus = d_seq + sl + 1;
		u8* const d_qual = d_plus + (c.plus_rep ? tl : 1) + 1;
		for (u64 k = lane; k < tl; k += 64)
		{
			const u8 ch = c.titles[t0 + k];
			d_title[k] = ch;
			if (c.plus_rep && k) d_plus[k] = ch;
		}
		for (u64 p = lane; p < sl; p += 64)
		{
			d_seq[p] = s_let[c.bases[s0 + p] & 31u];
			d_qual[p] = (u8)(c.quals[s0 + p] + c.qoff);
		}
		if (lane == 0)
		{
			d_title[tl] = '\n'; d_seq[sl] = '\n'; d_plus[0] = '+'; d_qual[-1] = '\n';
			if (r + 1 != B.end) d_qual[sl] = '\n';              // (no newline after the chunk's last record)
		}
	}
}

// ---- dsrcgpu_columns_cut --------------------------------------------------------------------------------------------------
// stage 1, grid-stride over the records: both offset arrays in order, the closing entries inside the arrays (then P is strictly
// increasing and below 2^63: the host has refused array lengths of 2^56 and more)
__global__ void __launch_bounds__(WG) k_col_mono(ColIn c, u64* err)
{
	for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < c.n_recs; r += (u64)gridDim.x * blockDim.x)
	{
		const u64 s0 = c.seq_offs[r], s1 = c.seq_offs[r + 1], t0 = c.title_offs[r], t1 = c.title_offs[r + 1];
		if (s0 > s1) col_err(err, r, COLE_SEQ_ORDER); else if (s1 > c.bases_len) col_err(err, r, COLE_SEQ_END);
		if (t0 > t1) col_err(err, r, COLE_TITLE_ORDER); else if (t1 > c.titles_len) col_err(err, r, COLE_TITLE_END);
	}
}

// stage 2, ONE wave: block after block, the largest e with P(e) - P(f) - 1 <= chunk_bytes (at least f + 1), found by a 64-way search
// -- lane l probes the l + 1-th of 64 equidistant candidates, the ballot of "still fits" is a prefix of the wave because P grows.
// out[0 .. min(n, out_cap - 1)] gets the cuts, *n_out the number of blocks whatever out_cap is.  Indices stay inside [0, n_recs] and
// every round shrinks the range whatever the offsets hold; behind a failed stage 1 nothing is searched at all.
__global__ void __launch_bounds__(64) k_col_cut(ColIn c, u64 chunk_bytes, u64* out, u64 out_cap, u64* n_out, const u64* err)
{
	if (*err != COLE_NONE) return;
	const u32 lane = lane_id();
	u64 f = 0, n = 0;
	if (lane == 0 && out_cap) out[0] = 0;
	while (f < c.n_recs)
	{
		const u64 lim = col_pos(c, f, c.seq_offs[f], c.title_offs[f]) + 1 + chunk_bytes;      // (chunk_bytes < 2^62, checked by the host)
		u64 a = f + 1, b = c.n_recs + 1;                   // the answer is in [a, b): a is taken anyway, b does not exist
		while (b - a > 1)
		{
			const u64 step = (b - a - 1 + 63) / 64;
			const u64 idx = a + (lane + 1) * step;
			const bool fits = idx < b && col_pos(c, idx, c.seq_offs[idx], c.title_offs[idx]) <= lim;
			const u64 k = (u64)__popcll(__ballot(fits));
			const u64 a2 = a + k * step;
			b = b < a2 + step ? b : a2 + step;
			a = a2;
		}
		f = a; ++n;
		if (lane == 0 && n < out_cap) out[n] = f;
	}
	if (lane == 0) *n_out = n;
}
