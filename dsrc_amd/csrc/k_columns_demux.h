// Columnar demultiplex: the seventh planner -- every record gets the sample whose barcodes lie nearest to what the record (or its index
// reads) holds at the barcode positions -- and the partition, a select whose output is grouped by class and stable inside a class
// (include/dsrc_gpu.h: dsrcgpu_columns_demux_plan, where the rule stands as a serial loop, and dsrcgpu_columns_partition_device).
// Plan in, plan out, as k_adapt_plan; the check pass is k_col_plan_check, once per column set.  The caller's input arrays are only read.
// No counterpart in the reference.
//
// THE PLANNER'S SHAPE: stage as a wave, compare as lanes.  A wave takes 64 records.  The barcode positions of each are read by the whole
// wave through col_planes (a lane a position, coalesced) and lane i keeps the planes of record i; then all 64 lanes walk the samples
// together.  The sample planes are wave-uniform loads through a const __restrict__ pointer, a distance is
// popcll(((p0 ^ s0) | (p1 ^ s1) | pn) & mask), and each lane keeps its own best, its index and the second best: no reduction, and the
// ALU work per record does not grow with the wave width.  (The other shape, a wave per record with the samples across the lanes and two
// wave minima per 64 samples, was not built.)
// THE CLASS COUNTS are a histogram in LDS per workgroup (64-bit, n_samples + 1 entries), flushed at the workgroup's end with one vector
// atomic add per non-zero class.  Atomics straight into the caller's array would give the same sums -- integer adds commute -- but
// with 8 samples a million records would queue on 8 addresses; in LDS the queue is per workgroup and the caller's array sees at most
// one add per class and workgroup.
// THE RANK of the partition is computed, never raced for: inside a wave the lanes of one class are found with one ballot per class bit
// and a lane's rank is the popcount of that mask below it; across the waves of a tile the waves are taken in turn over ONE array of
// running class counts in LDS (4 KiB at 1024 classes, a barrier per wave).  No kernel waits on another workgroup.
//
// Portable subset only (__syncthreads, __ballot, __shfl*, __popcll, __ffsll, vector atomics): tests/emu builds this file unchanged.
#pragma once
#include "k_common.h"
#include "k_columns_common.h"
#include "k_columns_sel.h"

#define DMX_MAX_CLASSES 1024u
#define DMX_GRID 512u           // the planner's workgroups at most: a histogram flush per workgroup, two of 1024 threads per CU
struct DemuxSrc { const u8* bases; const u64* offs; u64 bases_len; };       // an index read set: d_bases, d_seq_offs, bases_len
struct DemuxRules
{
	u32 n_samples, n_slots, src[2], off[2], len[2], max_mm[2], max_total, min_delta, cut, keep_unassigned, min_len;
	u32 cut_len;                // the largest offset + length over the slots of source 0
	u64 mask[2];                // the low len[s] bits
};
enum { DMX_KEPT = 0, DMX_BASES, DMX_CUT, DMX_ASSIGNED, DMX_PERFECT, DMX_SHORT, DMX_NO_MATCH, DMX_AMBIGUOUS, DMX_DROP_LEN, DMX_STATS = 9 };
enum { DMX_OK = 0, DMX_WHY_SHORT, DMX_WHY_NO_MATCH, DMX_WHY_AMBIGUOUS };

// grid (gx), a wave per 64 records with a grid stride, behind one k_col_plan_check per column set (err: three words, one per set; the
// words of sets that are not there stay clean).  tab: per sample four words -- bit 0 and bit 1 of the codes of slot 0, then of slot 1.
// A lane's record is re-checked through col_range, its index reads' offsets by hand, before a byte of either is read; a barcode is read
// only when it lies inside its limit, so a position at or behind the range's end is never looked at.
__global__ void __launch_bounds__(WG) k_demux_plan(ColIn c, ColPlanIn w, DemuxSrc x1, DemuxSrc x2, DemuxRules R, const u64* __restrict__ tab,
                                                   u64* begin, u64* end, u8* keep, u32* cls, u32* info, u64* class_counts, u64* stats, const u64* err)
{
	__shared__ unsigned long long s_hist[DMX_MAX_CLASSES];
	if (err[0] != COLE_NONE || err[1] != COLE_NONE || err[2] != COLE_NONE) return;
	const u32 lane = lane_id();
	const u64 wpg = blockDim.x >> 6;
	if (class_counts)
	{
		for (u32 i = threadIdx.x; i <= R.n_samples; i += blockDim.x) s_hist[i] = 0;
		__syncthreads();
	}
	u64 st[DMX_STATS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
	for (u64 first = (blockIdx.x * wpg + wave_id()) * 64; first < c.n_recs; first += gridDim.x * wpg * 64)
	{
		const u64 r = first + lane;
		u64 b = 0, e = 0;
		bool keep_in = false;
		bool ok = r < c.n_recs && col_range(c, w, r, b, e, keep_in);
		u64 lo[2] = {0, 0};
		bool is_short = false;
#pragma unroll
		for (u32 s = 0; s < 2; ++s)
			if (s < R.n_slots && ok)
			{
				u64 at = b, limit = e;
				if (R.src[s])
				{
					const DemuxSrc& x = R.src[s] == 1 ? x1 : x2;
					at = x.offs[r]; limit = x.offs[r + 1];
					if (at > limit || limit > x.bases_len) { ok = false; continue; }
				}
				if (limit - at < (u64)R.off[s] + R.len[s]) is_short = true; else lo[s] = at + R.off[s];
			}
		const bool search = ok && keep_in && !is_short;
		const u64 todo = __ballot(search);
		u64 p0[2] = {0, 0}, p1[2] = {0, 0}, pn[2] = {0, 0};
#pragma unroll
		for (u32 s = 0; s < 2; ++s)
			if (s < R.n_slots)
			{
				const u8* const xb = R.src[s] == 0 ? c.bases : R.src[s] == 1 ? x1.bases : x2.bases;
				for (u64 left = todo; left; left &= left - 1)
				{
					const u32 i = (u32)__ffsll((long long)left) - 1u;
					const u64 at = (u64)__shfl((unsigned long long)lo[s], (int)i);
					u64 a0, a1, an;
					col_planes(xb + at, R.len[s], 0, a0, a1, an);
					if (lane == i) { p0[s] = a0; p1[s] = a1; pn[s] = an; }
				}
			}
		u32 best = 256, second = 256, at_best = 0;
		if (todo)
		{
			if (R.n_slots == 2)
				for (u32 a = 0; a < R.n_samples; ++a)
				{
					const u64* const t = tab + 4 * (u64)a;
					const u32 d0 = (u32)__popcll(((p0[0] ^ t[0]) | (p1[0] ^ t[1]) | pn[0]) & R.mask[0]);
					const u32 d1 = (u32)__popcll(((p0[1] ^ t[2]) | (p1[1] ^ t[3]) | pn[1]) & R.mask[1]);
					const u32 D = d0 <= R.max_mm[0] && d1 <= R.max_mm[1] ? d0 + d1 : 255u;
					if (D < best) { second = best; best = D; at_best = a; } else if (D < second) second = D;
				}
			else
				for (u32 a = 0; a < R.n_samples; ++a)
				{
					const u64* const t = tab + 4 * (u64)a;
					const u32 d0 = (u32)__popcll(((p0[0] ^ t[0]) | (p1[0] ^ t[1]) | pn[0]) & R.mask[0]);
					const u32 D = d0 <= R.max_mm[0] ? d0 : 255u;
					if (D < best) { second = best; best = D; at_best = a; } else if (D < second) second = D;
				}
		}
		if (second > 255u) second = 255u;                    // (one sample: there is no runner-up)
		u64 ob = b;
		bool keep_out = false;
		u32 klass = 0xFFFFFFFFu, inf = 0xFFFFFFFFu;
		if (ok && keep_in)
		{
			u32 why;
			if (is_short) { best = second = 255u; why = DMX_WHY_SHORT; }
			else why = best > R.max_total ? DMX_WHY_NO_MATCH : second - best < R.min_delta ? DMX_WHY_AMBIGUOUS : DMX_OK;
			const bool assigned = why == DMX_OK;
			klass = assigned ? at_best : R.n_samples;
			inf = best | second << 8 | why << 16;
			if (assigned && R.cut) ob = b + R.cut_len;
			const bool flag = assigned || R.keep_unassigned;
			keep_out = flag && e - ob >= R.min_len;
			st[DMX_KEPT] += keep_out; st[DMX_BASES] += keep_out ? e - ob : 0; st[DMX_CUT] += keep_out ? ob - b : 0;
			st[DMX_ASSIGNED] += assigned; st[DMX_PERFECT] += assigned && best == 0;
			st[DMX_SHORT] += why == DMX_WHY_SHORT; st[DMX_NO_MATCH] += why == DMX_WHY_NO_MATCH; st[DMX_AMBIGUOUS] += why == DMX_WHY_AMBIGUOUS;
			st[DMX_DROP_LEN] += flag && !keep_out;
			if (class_counts) atomicAdd(&s_hist[klass], 1ull);
		}
		const u64 met = __ballot(1);                         // in place: k_columns_common.h (here a lane a record)
		if (met && ok)
		{
			begin[r] = ob; end[r] = e; keep[r] = keep_out ? 1 : 0; cls[r] = klass;
			if (info) info[r] = inf;
		}
	}
	u64 sum = 0;                                             // lane k adds up statistic k
#pragma unroll
	for (u32 k = 0; k < DMX_STATS; ++k)
	{
		const u64 t = wave_sum64(st[k]);
		if (lane == k) sum = t;
	}
	col_stats_flush(stats, DMX_STATS, sum);
	if (class_counts)
	{
		__syncthreads();
		for (u32 i = threadIdx.x; i <= R.n_samples; i += blockDim.x)
			if (s_hist[i]) atomicAdd((unsigned long long*)&class_counts[i], s_hist[i]);
	}
}

// ---- the partition -------------------------------------------------------------------------------------------------------------
// A tile = blockDim.x consecutive records, in every pass.  counts[class * n_tiles + tile], scanned in that order, gives every (class,
// tile) its first output record: class-major, inside a class tile after tile, inside a tile by rank -- the input order.
struct PartWhat { SelWhat w; const u32* cls; u32 n_classes; };
enum { PART_RECS = 0, PART_BASES, PART_TITLE, PART_LEFT, PART_TOTALS = 4 };

// pass 1, workgroups stride over the tiles: sel_record's checks, the tile's class histogram in LDS, and the four totals (integer sums:
// a wave sum and one vector atomic add per wave and total that is not 0)
__global__ void __launch_bounds__(WG) k_part_count(ColIn c, PartWhat p, u64 n_tiles, u64* counts, u64* totals, u64* err)
{
	__shared__ u32 s_hist[DMX_MAX_CLASSES];
	for (u32 i = threadIdx.x; i < p.n_classes; i += blockDim.x) s_hist[i] = 0;
	__syncthreads();
	u64 tot[PART_TOTALS] = {0, 0, 0, 0};
	for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
	{
		const u64 r = tile * blockDim.x + threadIdx.x;
		u64 v[3];
		sel_record(c, p.w, r, err, v);
		if (v[0])
		{
			const u32 k = p.cls[r];
			if (k < p.n_classes) { atomicAdd(&s_hist[k], 1u); tot[PART_RECS] += 1; tot[PART_BASES] += v[1]; tot[PART_TITLE] += v[2]; }
			else tot[PART_LEFT] += 1;
		}
		__syncthreads();
		for (u32 i = threadIdx.x; i < p.n_classes; i += blockDim.x) { counts[(u64)i * n_tiles + tile] = s_hist[i]; s_hist[i] = 0; }
		__syncthreads();
	}
	u64 sum = 0;
#pragma unroll
	for (u32 k = 0; k < PART_TOTALS; ++k)
	{
		const u64 t = wave_sum64(tot[k]);
		if (lane_id() == k) sum = t;
	}
	col_stats_flush(totals, PART_TOTALS, sum);
}

// exclusive scan of one 64-bit value over the workgroup (every thread calls it); tot = the sum
__device__ __forceinline__ u64 block_excl_scan1(u64 v, u64& tot)
{
	__shared__ u64 s_w[16];
	const u64 inc = wave_incl_scan64(v);
	if (lane_id() == 63) s_w[wave_id()] = inc;
	__syncthreads();
	u64 base = 0, t = 0;
	for (u32 i = 0; i < (blockDim.x >> 6); ++i)
	{
		const u64 x = s_w[i];
		if (i < wave_id()) base += x;
		t += x;
	}
	__syncthreads();
	tot = t;
	return base + inc - v;
}

// pass 2, the exclusive scan of vals[0 .. n) in three launches: the sums of chunks of blockDim.x values; ONE workgroup turns them into
// their exclusive prefix (with a carry from round to round) and writes the grand total; every value gets its chunk's base plus its
// place in the chunk
__global__ void __launch_bounds__(WG) k_part_scan_sums(u64 n, const u64* vals, u64 n_chunks, u64* chunk_sums)
{
	for (u64 ch = blockIdx.x; ch < n_chunks; ch += gridDim.x)
	{
		const u64 i = ch * blockDim.x + threadIdx.x;
		u64 tot;
		block_excl_scan1(i < n ? vals[i] : 0, tot);
		if (threadIdx.x == 0) chunk_sums[ch] = tot;
	}
}
__global__ void __launch_bounds__(WG) k_part_scan_chunks(u64 n_chunks, u64* chunk_sums, u64* total)
{
	u64 carry = 0;
	for (u64 first = 0; first < n_chunks; first += blockDim.x)
	{
		const u64 i = first + threadIdx.x;
		u64 tot;
		const u64 ex = block_excl_scan1(i < n_chunks ? chunk_sums[i] : 0, tot);
		if (i < n_chunks) chunk_sums[i] = carry + ex;
		carry += tot;
	}
	if (threadIdx.x == 0) *total = carry;
}
__global__ void __launch_bounds__(WG) k_part_scan_apply(u64 n, u64* vals, u64 n_chunks, const u64* chunk_sums)
{
	for (u64 ch = blockIdx.x; ch < n_chunks; ch += gridDim.x)
	{
		const u64 i = ch * blockDim.x + threadIdx.x;
		u64 tot;
		const u64 ex = block_excl_scan1(i < n ? vals[i] : 0, tot);
		if (i < n) vals[i] = chunk_sums[ch] + ex;
	}
}
// the class prefix out of the scanned counts: class_records[k] = the first output record of (k, tile 0), [n_classes] = the total
__global__ void __launch_bounds__(WG) k_part_class_records(const u64* first, u64 n_tiles, u32 n_classes, const u64* total, u64* class_records)
{
	for (u32 k = blockIdx.x * blockDim.x + threadIdx.x; k <= n_classes; k += gridDim.x * blockDim.x)
		class_records[k] = k < n_classes ? first[(u64)k * n_tiles] : *total;
}

// pass 3, tiles as in pass 1, behind a clean pass 1: order[first(class, tile) + rank] = r.  The rank among the earlier records of the
// class in the tile: in the wave by ballots (s_run is not involved), across the waves by taking them in turn over s_run.
__global__ void __launch_bounds__(WG) k_part_rank(ColIn c, PartWhat p, u64 n_tiles, const u64* first, u64 n_out, u64* order)
{
	__shared__ u32 s_run[DMX_MAX_CLASSES];
	const u32 lane = lane_id(), n_waves = blockDim.x >> 6;
	for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
	{
		for (u32 i = threadIdx.x; i < p.n_classes; i += blockDim.x) s_run[i] = 0;
		__syncthreads();
		const u64 r = tile * blockDim.x + threadIdx.x;
		u64 v[3];
		sel_record(c, p.w, r, nullptr, v);
		u32 k = v[0] ? p.cls[r] : 0xFFFFFFFFu;
		const bool part = k < p.n_classes;
		if (!part) k = 0;
		u64 same = __ballot(part);
#pragma unroll
		for (u32 bit = 0; bit < 10; ++bit)
		{
			const u64 set = __ballot(part && ((k >> bit) & 1u));
			same &= (k >> bit) & 1u ? set : ~set;
		}
		const u32 rank_w = (u32)__popcll(same & ((1ull << lane) - 1ull)), count_w = (u32)__popcll(same);
		u32 base_t = 0;
		for (u32 wv = 0; wv < n_waves; ++wv)
		{
			if (wave_id() == wv)
			{
				if (part) base_t = s_run[k];
				const u64 met = __ballot(1);                 // every lane of the class has read before its first lane writes
				if (met && part && rank_w == 0) s_run[k] = base_t + count_w;
			}
			__syncthreads();
		}
		if (part)
		{
			const u64 j = first[(u64)k * n_tiles + tile] + base_t + rank_w;
			if (j < n_out) order[j] = r;                     // (always, behind a clean pass 1 on unchanged arrays)
		}
	}
}

// pass 4, over OUTPUT records: the select's three-launch scan of (1, length, title length) of record order[j].  An entry of `order`
// that is no record (never, on unchanged arrays) counts as 0 / 0 / 0 and gets no place.
__device__ __forceinline__ void part_out_record(const ColIn& c, const PartWhat& p, const u64* order, u64 j, u64 n_out, u64& r, u64 v[3])
{
	r = j < n_out ? order[j] : ~0ull;
	const SelWhat w{p.w.begin, p.w.end, nullptr, p.w.titles};
	sel_record(c, w, r, nullptr, v);
}
__global__ void __launch_bounds__(WG) k_part_place_tiles(ColIn c, PartWhat p, const u64* order, u64 n_out, u64 n_tiles, u64* tile_sums)
{
	for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
	{
		u64 r, v[3], ex[3], tot[3];
		part_out_record(c, p, order, tile * blockDim.x + threadIdx.x, n_out, r, v);
		block_excl_scan3(v, ex, tot);
		if (threadIdx.x == 0) for (u32 k = 0; k < 3; ++k) tile_sums[3 * tile + k] = tot[k];
	}
}
// ... and behind k_sel_scan_tiles (the first kernel that writes the caller's arrays): output record j gets its two offsets and its
// source, pos[order[j]] = j is what k_sel_gather reads (pos comes in filled with SEL_DROPPED)
__global__ void __launch_bounds__(WG) k_part_place_apply(ColIn c, PartWhat p, const u64* order, u64 n_out, u64 n_tiles, const u64* tile_sums, SelOut o, u64* pos)
{
	if (blockIdx.x == 0 && threadIdx.x == 0)
	{
		o.seq_offs[o.kept] = o.n_bases;
		if (p.w.titles) o.title_offs[o.kept] = o.n_title;
	}
	for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
	{
		u64 r, v[3], ex[3], tot[3];
		part_out_record(c, p, order, tile * blockDim.x + threadIdx.x, n_out, r, v);
		block_excl_scan3(v, ex, tot);
		if (!v[0]) continue;
		const u64 j = tile_sums[3 * tile] + ex[0];
		if (j >= o.kept) continue;
		o.seq_offs[j] = tile_sums[3 * tile + 1] + ex[1];
		if (p.w.titles) o.title_offs[j] = tile_sums[3 * tile + 2] + ex[2];
		if (o.source) o.source[j] = r;
		pos[r] = j;
	}
}
