// Columnar decode: the records of a decoded batch as arrays (include/dsrc_gpu.h: dsrcgpu_decompress_batch_columns_device).
// Both kernels run after k_dec_layout (and k_dec_crc) and only READ what the decoder has left: the laid-out text and the
// record index (RecPools).  No counterpart in the reference, whose only decoded form is text (DsrcArchive::ReadNextRecord
// looks for the line ends again on the host).
#pragma once
#include "k_common.h"
#include "k_parse.h"
#include "k_dec.h"

// Caller's arrays, passed by value (the pointers of dsrcgpu_columns; d_titles == nullptr: titles not wanted)
struct ColOut
{
	u8* bases; u8* quals; u8* titles;
	u64* seq_offs; u64* title_offs;
	u64 n_recs, n_bases, n_title;        // totals of the batch: the closing entries of the two offset arrays
};

// per block: first record, first base, first title byte of the block inside the batch's arrays (host scan over the blocks)
struct ColBase { u64 rec, seq, title; };

// ---- stage 1: block-local exclusive prefixes of the read lengths and of the title lengths ----------------------------------
// grid (B), one workgroup per block: tiles of blockDim.x records, block_excl_scan per tile, the tile totals carried in
// registers (every thread gets the same total back).  A block's text is below 2^31 bytes, so the sums fit 32 bits.
__global__ void __launch_bounds__(WG) k_col_sizes(const DecDesc* desc, const DecState* st, RecPools rp, u32* seq_pre, u32* title_pre, u64* block_tot)
{
	const u32 b = blockIdx.x;
	const DecState* S = &st[b];
	const DecDesc d = desc[b];
	const u32 n = S->err ? 0u : min_u32(S->n_recs, d.rec_cap);        // (workgroup-uniform)
	u32 carry_s = 0, carry_t = 0;
	for (u32 base_r = 0; base_r < n; base_r += blockDim.x)
	{
		const u32 r = base_r + threadIdx.x;
		const u64 g = (u64)d.rec_base + r;
		const u32 ls = r < n ? (u32)rp.len[g] : 0u, lt = r < n ? (u32)rp.title_len[g] : 0u;
		u32 tot_s, tot_t;
		const u32 ex_s = block_excl_scan(ls, &tot_s);
		__syncthreads();
		const u32 ex_t = block_excl_scan(lt, &tot_t);
		__syncthreads();
		if (r < n) { seq_pre[g] = carry_s + ex_s; title_pre[g] = carry_t + ex_t; }
		carry_s += tot_s; carry_t += tot_t;
	}
	if (threadIdx.x == 0) { block_tot[2 * b] = carry_s; block_tot[2 * b + 1] = carry_t; }
}

// ---- stage 2: text -> columns (wave per record, a byte per lane) -----------------------------------------------------------
// grid (gx, B) like k_dec_layout.  Base letters go through a 128-entry table in LDS built from "ACGTNRWSKMDVHBYXU.-" (the
// index of the letter; 255 for every other byte, also for bytes >= 128); qualities lose the dataset's offset.  The host has
// checked the capacities against the totals of k_col_sizes before this kernel is launched.
__global__ void __launch_bounds__(WG) k_col_gather(const DecDesc* desc, const DecState* st, RecPools rp, const u8* text_all, const u32* seq_pre,
                                                   const u32* title_pre, const ColBase* cbase, ColOut o, DecParams prm)
{
	__shared__ u8 s_map[128];
	const char* const letters = "ACGTNRWSKMDVHBYXU.-";
	for (u32 c = threadIdx.x; c < 128; c += blockDim.x)
	{
		u32 code = 255;
		for (u32 k = 0; k < 19; ++k) if ((u32)(u8)letters[k] == c) code = k;
		s_map[c] = (u8)code;
	}
	__syncthreads();
	const u32 b = blockIdx.y;
	const DecState* S = &st[b];
	if (S->err) return;
	const DecDesc d = desc[b];
	const ColBase cb = cbase[b];
	const u8* text = text_all + d.out_off;
	const u32 lane = lane_id();
	const u32 off = prm.quality_offset;
	const u32 wpg = blockDim.x >> 6;
	const u32 n = min_u32(S->n_recs, d.rec_cap);
	for (u32 r = blockIdx.x * wpg + wave_id(); r < n; r += gridDim.x * wpg)
	{
		const u64 g = (u64)d.rec_base + r;
		const u32 ql = rp.len[g], so = rp.seq_off[g], qo = rp.qual_off[g];
		const u64 sb = cb.seq + seq_pre[g], tb = cb.title + title_pre[g];
		for (u32 p = lane; p < ql; p += 64)
		{
			const u32 ch = text[so + p], q = text[qo + p];
			o.bases[sb + p] = ch < 128 ? s_map[ch] : (u8)255;
			o.quals[sb + p] = (u8)(q - off);
		}
		if (o.titles)
		{
			const u32 to = rp.title_off[g], tl = rp.title_len[g];
			for (u32 k = lane; k < tl; k += 64) o.titles[tb + k] = text[to + k];
		}
		if (lane == 0)
		{
			const u64 gr = cb.rec + r;
			o.seq_offs[gr] = sb;
			if (o.titles) o.title_offs[gr] = tb;
			if (gr + 1 == o.n_recs)
			{	// the batch's last record: the closing entries
				o.seq_offs[o.n_recs] = o.n_bases;
				if (o.titles) o.title_offs[o.n_recs] = o.n_title;
			}
		}
	}
}
