// Columnar select: what stands between k_columns.h and k_columns_enc.h -- a quality trim / read filter that PLANS (per record a kept
// range and a keep flag) and a ragged compaction that SELECTS (kept records, bases and qualities cut to their range, titles whole) into
// fresh arrays with offsets from 0 (include/dsrc_gpu.h: dsrcgpu_columns_trim_plan, dsrcgpu_columns_select_device).  The caller's input
// arrays are only read.  No counterpart in the reference, whose readers hand out text one record at a time.
//
// Portable subset only (__syncthreads, __ballot, __shfl*, vector atomics): tests/emu builds this file unchanged.  No kernel waits on
// another workgroup: the three prefix sums of the compaction are separate launches (tile sums, scan of the tile sums, apply).
#pragma once
#include "k_common.h"
#include "k_columns_common.h"

// ---- the trim plan ---------------------------------------------------------------------------------------------------------
struct TrimRules { u32 c5, c3, min_len, max_n, min_mq; };
enum { TRIM_KEPT = 0, TRIM_BASES, TRIM_CUT, TRIM_DROP_LEN, TRIM_DROP_N, TRIM_DROP_MQ };

// One end of the running-sum rule over a read of n bases at q: position j = 0, 1, ... counts from the 5' end (rev = 0) or from the 3'
// end (rev = 1).  s_j = sum over k <= j of (cut - q_k); the walk ends at the first s_j < 0; the answer is 1 + the FIRST j in front of
// that break at which s_j reaches its maximum, if that maximum is above 0, else 0.  64 positions a step: a wave inclusive scan of
// cut - q (at most 64 * 255 in size: 32 bits) on top of a 64-bit carry; the break is the lowest lane with a negative sum, the
// candidates are the lanes in front of it; a tile's maximum replaces the running best only when strictly greater, and inside a tile
// the lowest lane that holds the maximum wins -- the position the serial loop meets first.  After a break no further tile is read.
// Every branch is wave-uniform.
__device__ __forceinline__ u64 trim_end(const u8* q, u64 n, u32 cut, bool rev)
{
	const u32 lane = lane_id();
	i64 carry = 0, best = 0;
	u64 taken = 0;
	for (u64 base = 0; base < n; base += 64)
	{
		const u64 j = base + lane;
		const bool valid = j < n;
		const i32 v = valid ? (i32)cut - (i32)q[rev ? n - 1 - j : j] : 0;
		const i32 inc = (i32)wave_incl_scan((u32)v);
		const u64 neg = __ballot(valid && carry + inc < 0);
		const u32 first_neg = neg ? (u32)__ffsll((long long)neg) - 1u : 64u;
		const bool cand = valid && lane < first_neg;
		// (signed maximum through the unsigned wave_max: the sign bit flipped, 0 for lanes that are no candidates)
		const u32 top = wave_max(cand ? (u32)inc ^ 0x80000000u : 0u);
		if (top)
		{
			const i32 m = (i32)(top ^ 0x80000000u);
			const u64 at = __ballot(cand && inc == m);
			if (carry + m > best) { best = carry + m; taken = base + (u64)(__ffsll((long long)at) - 1) + 1; }
		}
		if (neg) break;
		carry += (i32)__shfl((u32)inc, 63);
	}
	return taken;
}

// grid (gx), a wave per record.  A record's own two offsets are checked before its bytes are read (the host launches this kernel behind
// k_sel_seq_check and it does nothing unless that pass was clean, so the test never fails: it is what keeps every read inside the
// caller's arrays whatever they hold).  The six statistics are sums: a wave adds up its records in registers and issues one vector
// atomic add per counter at its end, so the result does not depend on the order of the waves.
__global__ void __launch_bounds__(WG) k_sel_plan(ColIn c, TrimRules R, u64* begin, u64* end, u8* keep, u64* stats, const u64* err)
{
	if (*err != COLE_NONE) return;
	const u32 lane = lane_id();
	const u64 wpg = blockDim.x >> 6;
	u64 st[6] = {0, 0, 0, 0, 0, 0};
	for (u64 r = blockIdx.x * wpg + wave_id(); r < c.n_recs; r += gridDim.x * wpg)
	{
		const u64 s0 = c.seq_offs[r], s1 = c.seq_offs[r + 1];
		if (s0 > s1 || s1 > c.bases_len) continue;
		const u64 n = s1 - s0;
		const u8* const q = c.quals + s0;
		u64 start = R.c5 ? trim_end(q, n, R.c5, false) : 0;
		u64 stop = R.c3 ? n - trim_end(q, n, R.c3, true) : n;
		if (start >= stop) start = stop = 0;
		const u64 len = stop - start;
		u64 n_amb = 0, q_sum = 0;
		for (u64 p = start + lane; p < stop; p += 64)
		{
			n_amb += c.bases[s0 + p] >= 4u ? 1u : 0u;
			q_sum += q[p];
		}
		n_amb = wave_sum64(n_amb); q_sum = wave_sum64(q_sum);
		u32 why = TRIM_KEPT;
		if (len < R.min_len) why = TRIM_DROP_LEN;
		else if (R.max_n != 0xFFFFFFFFu && n_amb > R.max_n) why = TRIM_DROP_N;
		else if (R.min_mq && q_sum < (u64)R.min_mq * len) why = TRIM_DROP_MQ;
		st[TRIM_KEPT] += why == TRIM_KEPT; st[TRIM_DROP_LEN] += why == TRIM_DROP_LEN;
		st[TRIM_DROP_N] += why == TRIM_DROP_N; st[TRIM_DROP_MQ] += why == TRIM_DROP_MQ;
		if (why == TRIM_KEPT) { st[TRIM_BASES] += len; st[TRIM_CUT] += n - len; }
		if (lane == 0) { begin[r] = s0 + start; end[r] = s0 + stop; keep[r] = why == TRIM_KEPT ? 1 : 0; }
	}
	if (lane == 0)
		for (u32 k = 0; k < 6; ++k)
			if (st[k]) atomicAdd((unsigned long long*)&stats[k], (unsigned long long)st[k]);
}

// the plan's check pass, grid-stride over the records: d_seq_offs in order, its closing entries inside d_bases (k_col_mono without the
// titles, which the plan does not read)
__global__ void __launch_bounds__(WG) k_sel_seq_check(ColIn c, u64* err)
{
	for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < c.n_recs; r += (u64)gridDim.x * blockDim.x)
	{
		const u64 s0 = c.seq_offs[r], s1 = c.seq_offs[r + 1];
		if (s0 > s1) col_err(err, r, COLE_SEQ_ORDER); else if (s1 > c.bases_len) col_err(err, r, COLE_SEQ_END);
	}
}

// ---- select: the ragged compaction -------------------------------------------------------------------------------------------
// what to keep (all three may be null: whole reads, every record) and the caller's output arrays, by value
struct SelWhat { const u64* begin; const u64* end; const u8* keep; u32 titles; };
struct SelOut { u8* bases; u8* quals; u8* titles; u64* seq_offs; u64* title_offs; u64* source; u64 kept, n_bases, n_title; };
#define SEL_DROPPED (~0ull)

// Record r's contribution to the three sums -- kept flag, kept bases, kept title bytes -- behind the checks of k_col_mono and of the
// range: S[r] <= begin <= end <= S[r + 1].  The checks look at dropped records as well.  err == nullptr: the apply pass, which runs
// behind a clean first pass and reports nothing.  A record that fails a check counts as 0 / 0 / 0 (the host stops behind the first pass).
__device__ __forceinline__ void sel_record(const ColIn& c, const SelWhat& w, u64 r, u64* err, u64 v[3])
{
	v[0] = v[1] = v[2] = 0;
	if (r >= c.n_recs) return;
	const u64 s0 = c.seq_offs[r], s1 = c.seq_offs[r + 1];
	u32 bad = 0;
	if (s0 > s1) bad |= 1u << COLE_SEQ_ORDER; else if (s1 > c.bases_len) bad |= 1u << COLE_SEQ_END;
	u64 b = s0, e = s1, tl = 0;
	if (!bad && w.begin)
	{
		b = w.begin[r]; e = w.end[r];
		if (b < s0) bad |= 1u << COLS_BEGIN_LOW; else if (e > s1) bad |= 1u << COLS_END_HIGH; else if (b > e) bad |= 1u << COLS_RANGE_ORDER;
	}
	if (w.titles)
	{
		const u64 t0 = c.title_offs[r], t1 = c.title_offs[r + 1];
		if (t0 > t1) bad |= 1u << COLE_TITLE_ORDER; else if (t1 > c.titles_len) bad |= 1u << COLE_TITLE_END;
		tl = t1 - t0;
	}
	if (bad) { if (err) col_err(err, r, (u32)__ffs((int)bad) - 1u); return; }
	if (w.keep && !w.keep[r]) return;
	v[0] = 1; v[1] = e - b; v[2] = tl;
}

// exclusive scan of three 64-bit values over the workgroup (every thread calls it); tot[] = the sums
__device__ __forceinline__ void block_excl_scan3(const u64 v[3], u64 ex[3], u64 tot[3])
{
	__shared__ u64 s_w[3][16];
	u64 inc[3];
	for (u32 k = 0; k < 3; ++k) inc[k] = wave_incl_scan64(v[k]);
	if (lane_id() == 63) for (u32 k = 0; k < 3; ++k) s_w[k][wave_id()] = inc[k];
	__syncthreads();
	for (u32 k = 0; k < 3; ++k)
	{
		u64 base = 0, t = 0;
		for (u32 i = 0; i < (blockDim.x >> 6); ++i)
		{
			const u64 x = s_w[k][i];
			if (i < wave_id()) base += x;
			t += x;
		}
		ex[k] = base + inc[k] - v[k]; tot[k] = t;
	}
	__syncthreads();
}

// pass 1, a tile = blockDim.x records, a thread per record, workgroups stride over the tiles: the checks, and the tile's three sums
__global__ void __launch_bounds__(WG) k_sel_tiles(ColIn c, SelWhat w, u64 n_tiles, u64* tile_sums, u64* err)
{
	for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
	{
		u64 v[3], ex[3], tot[3];
		sel_record(c, w, tile * blockDim.x + threadIdx.x, err, v);
		block_excl_scan3(v, ex, tot);
		if (threadIdx.x == 0) for (u32 k = 0; k < 3; ++k) tile_sums[3 * tile + k] = tot[k];
	}
}

// pass 2, ONE workgroup: the tile sums become their exclusive prefix, blockDim.x tiles a round with a carry from round to round (the
// record count is not bounded by what one round holds); totals[] = records, bases, title bytes kept
__global__ void __launch_bounds__(WG) k_sel_scan_tiles(u64 n_tiles, u64* tile_sums, u64* totals)
{
	u64 carry[3] = {0, 0, 0};
	for (u64 first = 0; first < n_tiles; first += blockDim.x)
	{
		const u64 t = first + threadIdx.x;
		u64 v[3], ex[3], tot[3];
		for (u32 k = 0; k < 3; ++k) v[k] = t < n_tiles ? tile_sums[3 * t + k] : 0;
		block_excl_scan3(v, ex, tot);
		for (u32 k = 0; k < 3; ++k)
		{
			if (t < n_tiles) tile_sums[3 * t + k] = carry[k] + ex[k];
			carry[k] += tot[k];
		}
	}
	if (threadIdx.x == 0) for (u32 k = 0; k < 3; ++k) totals[k] = carry[k];
}

// pass 3, tiles as in pass 1 (behind the host's capacity check: the first kernel that writes the caller's arrays): kept record r
// becomes output record j = its place among the kept ones; the two output offset arrays and d_source get entry j, pos[r] = j or
// SEL_DROPPED is what the gather reads.  The first workgroup writes the closing entries (o.kept etc. are the totals of pass 2).
__global__ void __launch_bounds__(WG) k_sel_apply(ColIn c, SelWhat w, u64 n_tiles, const u64* tile_sums, SelOut o, u64* pos)
{
	if (blockIdx.x == 0 && threadIdx.x == 0)
	{
		o.seq_offs[o.kept] = o.n_bases;
		if (w.titles) o.title_offs[o.kept] = o.n_title;
	}
	for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
	{
		const u64 r = tile * blockDim.x + threadIdx.x;
		u64 v[3], ex[3], tot[3];
		sel_record(c, w, r, nullptr, v);
		block_excl_scan3(v, ex, tot);
		if (r >= c.n_recs) continue;
		if (!v[0]) { pos[r] = SEL_DROPPED; continue; }
		const u64 j = tile_sums[3 * tile] + ex[0];
		if (j >= o.kept) { pos[r] = SEL_DROPPED; continue; }       // (cannot happen behind a clean pass 1 on unchanged arrays)
		o.seq_offs[j] = tile_sums[3 * tile + 1] + ex[1];
		if (w.titles) o.title_offs[j] = tile_sums[3 * tile + 2] + ex[2];
		if (o.source) o.source[j] = r;
		pos[r] = j;
	}
}

// the gather, grid (gx), a wave per INPUT record, dropped records return at once; a byte per lane, neighbouring lanes move neighbouring
// bytes (k_col_scatter's shape).  Runs behind pass 3: the destinations are the output offsets that pass has written.
__global__ void __launch_bounds__(WG) k_sel_gather(ColIn c, SelWhat w, SelOut o, const u64* pos)
{
	const u32 lane = lane_id();
	const u64 wpg = blockDim.x >> 6;
	for (u64 r = blockIdx.x * wpg + wave_id(); r < c.n_recs; r += gridDim.x * wpg)
	{
		const u64 j = pos[r];
		if (j == SEL_DROPPED) continue;
		const u64 b = w.begin ? w.begin[r] : c.seq_offs[r], e = w.begin ? w.end[r] : c.seq_offs[r + 1];
		const u64 len = e - b, d = o.seq_offs[j];
		if (b > e || e > c.bases_len || d > o.n_bases || len > o.n_bases - d) continue;       // (as above: never behind a clean pass 1)
		for (u64 p = lane; p < len; p += 64)
		{
			o.bases[d + p] = c.bases[b + p];
			o.quals[d + p] = c.quals[b + p];
		}
		if (w.titles)
		{
			const u64 t0 = c.title_offs[r], t1 = c.title_offs[r + 1], dt = o.title_offs[j];
			if (t0 > t1 || t1 > c.titles_len || dt > o.n_title || t1 - t0 > o.n_title - dt) continue;
			for (u64 k = lane; k < t1 - t0; k += 64) o.titles[dt + k] = c.titles[t0 + k];
		}
	}
}
