// Columnar adapter trim: the second planner beside k_sel_plan -- a 3' adapter search that takes a plan in (per record a range and a
// keep flag, or none: whole reads, every record) and gives a narrower plan out, which dsrcgpu_columns_select_device carries out
// (include/dsrc_gpu.h: dsrcgpu_columns_adapter_plan).  Hamming distance only, the leftmost start position wins, at one position the
// lowest adapter index; the adapter may hang over the 3' end of the range.  The caller's input arrays are only read.  No counterpart
// in the reference.
//
// Portable subset only (__ballot, __shfl*, __popcll, __ffsll, vector atomics): tests/emu builds this file unchanged.
#pragma once
#include "k_common.h"
#include "k_columns_sel.h"

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
struct AdaptPlanIn { const u64* begin; const u64* end; const u8* keep; };
enum { ADAPT_KEPT = 0, ADAPT_BASES, ADAPT_CUT, ADAPT_TRIMMED, ADAPT_DROP_LEN, ADAPT_FOUND };      // ADAPT_FOUND + a: found per adapter

// the check pass, a thread per record with a grid stride: k_sel_seq_check plus the range checks of the select (sel_record), for kept
// and dropped records alike
__global__ void __launch_bounds__(WG) k_adapt_check(ColIn c, AdaptPlanIn w, u64* err)
{
	for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < c.n_recs; r += (u64)gridDim.x * blockDim.x)
	{
		const u64 s0 = c.seq_offs[r], s1 = c.seq_offs[r + 1];
		if (s0 > s1) { col_err(err, r, COLE_SEQ_ORDER); continue; }
		if (s1 > c.bases_len) { col_err(err, r, COLE_SEQ_END); continue; }
		if (!w.begin) continue;
		const u64 b = w.begin[r], e = w.end[r];
		if (b < s0) col_err(err, r, COLS_BEGIN_LOW); else if (e > s1) col_err(err, r, COLS_END_HIGH); else if (b > e) col_err(err, r, COLS_RANGE_ORDER);
	}
}

// 64 positions of the range x[0 .. n) from `base` on as three wave-uniform bit planes: bit 0 of the code, bit 1 of the code, code >= 4.
// A lane per position, each byte loaded once; positions at or beyond n give 0 in every plane.
__device__ __forceinline__ void adapt_planes(const u8* x, u64 n, u64 base, u64& p0, u64& p1, u64& pn)
{
	const u64 j = base + lane_id();
	const bool valid = j < n;
	const u32 code = valid ? x[j] : 0u;
	p0 = __ballot(valid && (code & 1u));
	p1 = __ballot(valid && (code & 2u));
	pn = __ballot(valid && code >= 4u);
}

// grid (gx), a wave per record, as k_sel_plan (and behind k_adapt_check in the same way: nothing happens unless that pass was clean,
// and a record's offsets and range are tested again before its bytes are read).  Lane l of a tile judges the start position p = base +
// l: its window of 64 positions is cut from the planes of this tile and the next one (lane 0 takes the current planes as they are: a
// shift by 64 is not a shift by 0), and per adapter the mismatches are one popcount under the mask of the L = min(len, n - p)
// positions compared (L = 64: all ones, again no shift by 64).  A read code >= 4 is a mismatch whatever the adapter holds.  The
// leftmost lane with a hit of any adapter is p, the lowest adapter that hit in that lane is a (the adapters are tried from the last to the
// first, each lane keeps the last that matched); behind a tile with a hit no further tile
// is read.  Every branch is wave-uniform.  A wave reads begin / end / keep of its record before lane 0 writes them (a ballot stands
// between the two), so each output array may be its input counterpart.  Statistics: sums as in k_sel_plan, here one to a lane (lane k adds up statistic k in a register and
// issues one vector atomic add at the wave's end if it is not 0), so the result does not depend on the order of the waves.
__global__ void __launch_bounds__(WG) k_adapt_plan(ColIn c, AdaptPlanIn w, AdaptRules R, u64* begin, u64* end, u8* keep, u32* which, u64* stats,
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
		const u64 s0 = c.seq_offs[r], s1 = c.seq_offs[r + 1];
		if (s0 > s1 || s1 > c.bases_len) continue;
		const u64 b = w.begin ? w.begin[r] : s0, e = w.begin ? w.end[r] : s1;
		const bool keep_in = w.keep ? w.keep[r] != 0 : true;
		if (b < s0 || e > s1 || b > e) continue;
		const u64 n = e - b;
		const u8* const x = c.bases + b;
		u64 cut_at = n;
		u32 found = ADAPT_NONE;
		if (keep_in && n)
		{
			u64 c0, c1, cn;
			adapt_planes(x, n, 0, c0, c1, cn);
			for (u64 base = 0; base < n; base += 64)
			{
				u64 n0 = 0, n1 = 0, nn = 0;
				if (n - base > 64) adapt_planes(x, n, base + 64, n0, n1, nn);
				const u32 up = (64u - lane) & 63u;
				const u64 w0 = (c0 >> lane) | (lane ? n0 << up : 0ull);
				const u64 w1 = (c1 >> lane) | (lane ? n1 << up : 0ull);
				const u64 wn = (cn >> lane) | (lane ? nn << up : 0ull);
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
		// in place: the wave meets once more, so that every lane has read begin / end / keep of this record before lane 0 overwrites them
		// (in lockstep that holds anyway; a record that was not searched has met nowhere else)
		const u64 met = __ballot(1);
		if (lane == 0 && met)
		{
			begin[r] = b; end[r] = b + len; keep[r] = keep_out ? 1 : 0;
			if (which) which[r] = found;
		}
	}
	if (lane < ADAPT_FOUND + ADAPT_MAX && sum) atomicAdd((unsigned long long*)&stats[lane], (unsigned long long)sum);
}
