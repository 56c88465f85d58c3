// Columnar adapter trim: the second planner beside k_sel_plan -- a 3' adapter search that takes a plan in (per record a range and a
// keep flag, or none: whole reads, every record) and gives a narrower plan out, which dsrcgpu_columns_select_device carries out
// (include/dsrc_gpu.h: dsrcgpu_columns_adapter_plan).  Hamming distance only, the leftmost start position wins, at one position the
// lowest adapter index; the adapter may hang over the 3' end of the range.  The caller's input arrays are only read.  No counterpart
// in the reference.
//
// Portable subset only (__ballot, __shfl*, __popcll, __ffsll, vector atomics): tests/emu builds this file unchanged.
#pragma once
#include "k_common.h"
#include "k_columns_common.h"

#define ADAPT_MAX 8
#define ADAPT_NONE 0xFFFFFFFFu
// by value in the kernel arguments; the kernel indexes len / a0 / a1 with compile-time constants only (unrolled loops of ADAPT_MAX
// rounds), so that the struct is never copied to scratch: once to put the table into LDS, from where the search reads it (40 scalar
// registers of table live across the tile loop were more than the wave has to spare)
struct AdaptRules
{
	u32 k, min_overlap, permille, min_len;
	u32 len[ADAPT_MAX];
	u64 a0[ADAPT_MAX], a1[ADAPT_MAX];      // bit j = bit 0 / bit 1 of the adapter's code at position j
};
enum { ADAPT_KEPT = 0, ADAPT_BASES, ADAPT_CUT, ADAPT_TRIMMED, ADAPT_DROP_LEN, ADAPT_FOUND };      // ADAPT_FOUND + a: found per adapter

// grid (gx), a wave per record, as k_sel_plan, behind k_col_plan_check (k_columns_common.h: the re-check, in place, the statistics).
// Lane l of a tile judges the start position p = base + l: its window of 64 positions is cut from the planes of this tile and the
// next one (col_funnel), and per adapter the mismatches are one popcount under the mask of the L = min(len, n - p) positions
// compared (L = 64: all ones, again no shift by 64).  A read code >= 4 is a mismatch whatever the adapter holds.  The leftmost lane
// with a hit of any adapter is p, the lowest adapter that hit in that lane is a (the adapters are tried from the last to the first,
// each lane keeps the last that matched); behind a tile with a hit no further tile is read.  Every branch is wave-uniform.
__global__ void __launch_bounds__(WG) k_adapt_plan(ColIn c, ColPlanIn w, AdaptRules R, u64* begin, u64* end, u8* keep, u32* which, u64* stats,
                                                   const u64* err)
{
	if (*err != COLE_NONE) return;
	__shared__ u64 s_a0[ADAPT_MAX], s_a1[ADAPT_MAX];
	__shared__ u32 s_len[ADAPT_MAX];
#pragma unroll
	for (u32 a = 0; a < ADAPT_MAX; ++a)
		if (threadIdx.x == a) { s_a0[a] = R.a0[a]; s_a1[a] = R.a1[a]; s_len[a] = R.len[a]; }
	__syncthreads();
	const u32 lane = lane_id();
	const u64 wpg = blockDim.x >> 6;
	u64 sum = 0;                                         // lane k adds up statistic k
	for (u64 r = blockIdx.x * wpg + wave_id(); r < c.n_recs; r += gridDim.x * wpg)
	{
		u64 b, e;
		bool keep_in;
		if (!col_range(c, w, r, b, e, keep_in)) continue;
		const u64 n = e - b;
		const u8* const x = c.bases + b;
		u64 cut_at = n;
		u32 found = ADAPT_NONE;
		if (keep_in && n)
		{
			u64 c0, c1, cn;
			col_planes(x, n, 0, c0, c1, cn);
			for (u64 base = 0; base < n; base += 64)
			{
				u64 n0 = 0, n1 = 0, nn = 0;
				if (n - base > 64) col_planes(x, n, base + 64, n0, n1, nn);
				const u64 w0 = col_funnel(c0, n0, lane), w1 = col_funnel(c1, n1, lane), wn = col_funnel(cn, nn, lane);
				const u64 p = base + lane;
				const bool valid = p < n;
				const u64 rem = valid ? n - p : 0;
				u32 mine = ADAPT_NONE;                           // the lowest adapter that matches at this lane's p
#pragma unroll
				for (u32 a = ADAPT_MAX; a-- > 0;)
					if (a < R.k)
					{
						const u32 la = s_len[a];
						const u32 L = rem < (u64)la ? (u32)rem : la;                  // 0 .. 64
						const u64 mask = L >= 64u ? ~0ull : (1ull << L) - 1ull;
						const u32 mm = (u32)__popcll(((w0 ^ s_a0[a]) | (w1 ^ s_a1[a]) | wn) & mask);
						if (L >= R.min_overlap && mm * 1000u <= L * R.permille) mine = a;
					}
				const u64 any = __ballot(mine != ADAPT_NONE);
				if (any)
				{
					const u32 at = (u32)__ffsll((long long)any) - 1u;
					cut_at = base + at;
					found = __shfl(mine, (int)at);
					break;
				}
				c0 = n0; c1 = n1; cn = nn;
			}
		}
		const u64 len = cut_at;
		const bool keep_out = keep_in && len >= R.min_len;
		if (keep_in)
		{
			const u64 mine = lane == ADAPT_KEPT ? (keep_out ? 1u : 0u) : lane == ADAPT_BASES ? (keep_out ? len : 0u) : lane == ADAPT_CUT ? (keep_out ? n - len : 0u)
			               : lane == ADAPT_TRIMMED ? (found != ADAPT_NONE ? 1u : 0u) : lane == ADAPT_DROP_LEN ? (keep_out ? 0u : 1u)
			               : (found != ADAPT_NONE && lane == ADAPT_FOUND + found ? 1u : 0u);
			sum += mine;
		}
		const u64 met = __ballot(1);                         // in place: k_columns_common.h
		if (lane == 0 && met)
		{
			begin[r] = b; end[r] = b + len; keep[r] = keep_out ? 1 : 0;
			if (which) which[r] = found;
		}
	}
	col_stats_flush(stats, ADAPT_FOUND + ADAPT_MAX, sum);
}
