// Columnar k-mer plan: the fifth planner -- every window of k bases of every considered record's range is looked up in a k-mer table
// (k_columns_kmer.h) that is ONLY READ, and the record gets a narrowed plan (a 3' cut at its first window that does not hit, or at
// its first that does, and a keep flag from the number and share of its hits, its median abundance and what is left) plus three
// annotations: good windows, hits, median count (include/dsrc_gpu.h: dsrcgpu_columns_kmer_plan has the rule as a serial loop).
// A contaminant screen (BBDuk) and an abundance trim (khmer) are the two uses.  The caller's input arrays and the table are only
// read.  No counterpart in the reference.
//
//   k_kmer_plan_longest  a lane per record, behind k_col_plan_check: the most windows any considered record has (the median's scratch)
//   k_kmer_plan          a wave per record, 64 windows a step: the plan and the annotations
//
// The walk is k_kmer_count's (kmer_step), and kmer_find walks as the inserts did (hash_mask included).  Equal neighbouring keys form
// a run whose head lane alone walks; the others take its count by shuffle (kmer_step_counts) -- a poly-G tail costs one walk per step.
// The table is never written and nothing here is an atomic on it: two calls, or a call and a lookup, may read one table at the same
// time.
// The median (MEDIAN = true only): the wave keeps min(count, 65535) of its record's good windows, compacted in window order, in
// KMER_PLAN_LDS_WINDOWS 16-bit words of LDS of its own; a record with more windows keeps them in the wave's slice of `spill` (HBM
// scratch the host sized from the longest range of the call).  The element of rank good / 2 comes from a 16-round radix select,
// most significant bit first: a round counts the stored values that agree with the bits chosen so far and have a 0 in the round's
// bit -- a ballot and a popcount per 64 values.  Both stores are read back by the wave that wrote them only, behind a wave fence.
// Statistics: wave-uniform sums, one to a lane (k_columns_common.h).  No lane waits for another wave: the loops are the bounded
// walk, the steps of a record and the select.
//
// Portable subset only (static __shared__, __ballot, __shfl*, __popcll, __ffsll, __clzll, the wave fence of k_common.h, vector
// atomics): tests/emu builds this file unchanged.
#pragma once
#include "k_common.h"
#include "k_columns_common.h"
#include "k_columns_kmer.h"

#define KMER_PLAN_LDS_WINDOWS 1024u                        // 16-bit counts a wave keeps in LDS: 32 KiB for a workgroup of 16 waves
#define KMER_PLAN_COUNT_CAP 65535u
#define KMER_PLAN_NO_LIMIT 0xFFFFFFFFu
#define KPLAN_SPILL_BYTES (256ull << 20)                   // the host keeps the waves' slices of HBM scratch under this by launching fewer waves
enum { KPLAN_CONSIDERED = 0, KPLAN_CAME_DROPPED, KPLAN_NO_WINDOW, KPLAN_WINDOWS, KPLAN_GOOD, KPLAN_HITS, KPLAN_KEPT, KPLAN_WITH_HIT, KPLAN_TRIMMED,
       KPLAN_CUT, KPLAN_DROP_HITS, KPLAN_DROP_SHARE, KPLAN_DROP_MEDIAN, KPLAN_DROP_LENGTH, KPLAN_BASES, KPLAN_N_STATS = 16 };
enum { KPLAN_TRIM_NONE = 0, KPLAN_TRIM_FIRST_MISS, KPLAN_TRIM_FIRST_HIT };

// by value in the kernel arguments
struct KmerPlanRules { u64 min_count; u32 min_hits, max_hits, min_permille, max_permille, min_median, max_median, trim, min_len; };
struct KmerPlanOut { u64* begin; u64* end; u8* keep; u64* good; u64* hits; u64* median; };

// grid (gx), a lane per record with a grid stride, behind k_col_plan_check: *longest = the most windows of a considered record
__global__ void __launch_bounds__(WG) k_kmer_plan_longest(ColIn c, ColPlanIn w, u32 k, u64* longest, const u64* err)
{
	if (*err != COLE_NONE) return;
	u64 most = 0;
	for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < c.n_recs; r += (u64)gridDim.x * blockDim.x)
	{
		u64 b, e;
		if (!col_range(c, w, r, b, e)) continue;
		if (w.keep && w.keep[r] == 0) continue;
		const u64 n = e - b;
		if (n >= k && n - k + 1 > most) most = n - k + 1;
	}
	most = wave_max64(most);
	if (lane_id() == 0 && most) atomicMax((unsigned long long*)longest, (unsigned long long)most);
}

// the value of rank `rank` (0 = the lowest) among cnt[0 .. n), n >= 1, rank < n; wave-uniform control flow, every lane gets the result
template <typename P> __device__ __forceinline__ u32 kplan_select(P cnt, u64 n, u64 rank)
{
	const u32 lane = lane_id();
	u32 prefix = 0;
	for (u32 bit = 16; bit-- > 0;)
	{
		u64 zeros = 0;
		for (u64 base = 0; base < n; base += 64)
		{
			const bool in = base + lane < n;
			const u32 v = in ? (u32)cnt[base + lane] : 0u;
			zeros += (u64)__popcll(__ballot(in && (v >> (bit + 1u)) == (prefix >> (bit + 1u)) && !((v >> bit) & 1u)));
		}
		if (rank >= zeros) { prefix |= 1u << bit; rank -= zeros; }
	}
	return prefix;
}

// grid (gx), a wave per record with a grid stride, 64 windows a step; lane i of a step has the window that starts at position base + i
// of the range (kmer_step).  Plan in, plan out, in place if the caller likes (k_columns_common.h).  Every branch around a ballot or
// a shuffle is wave-uniform; the walks of the head lanes are the only divergent code.
// spill: gridDim.x * (blockDim.x / 64) slices of spill_stride 16-bit words, one per wave (MEDIAN only, null if no record needs it).
template <bool MEDIAN>
__global__ void __launch_bounds__(WG) k_kmer_plan(ColIn c, ColPlanIn w, u32 k, u32 canonical, KmerTab t, KmerPlanRules R, KmerPlanOut o, u16* spill,
                                                  u64 spill_stride, u64* stats, const u64* err)
{
	if (*err != COLE_NONE) return;
	__shared__ u16 s_cnt[MEDIAN ? WG / 64 : 1][MEDIAN ? KMER_PLAN_LDS_WINDOWS : 1];
	const u32 lane = lane_id();
	const u64 wpg = blockDim.x >> 6;
	const u64 kmask = (1ull << k) - 1ull;
	u16* const my_lds = s_cnt[MEDIAN ? wave_id() : 0];
	u16* const my_spill = MEDIAN && spill ? spill + (blockIdx.x * wpg + wave_id()) * spill_stride : nullptr;
	u64 sum = 0;                                         // lane s adds up statistic s
	for (u64 r = blockIdx.x * wpg + wave_id(); r < c.n_recs; r += gridDim.x * wpg)
	{
		u64 b, e;
		bool keep_in;
		if (!col_range(c, w, r, b, e, keep_in)) continue;
		const u64 n = e - b;
		const u64 n_win = keep_in && n >= k ? n - k + 1 : 0;
		u64 good_n = 0, hits = 0, first_miss = n_win, first_hit = n_win;
		// (a record with more windows than the LDS holds, under a call whose host saw no such record: cannot be, and is not stored)
		const bool in_lds = n_win <= KMER_PLAN_LDS_WINDOWS;
		const bool stored = MEDIAN && (in_lds || (my_spill && n_win <= spill_stride));
		if (n_win)
		{
			const u8* const x = c.bases + b;
			u64 c0, c1, cn;
			col_planes(x, n, 0, c0, c1, cn);
			for (u64 base = 0; base < n_win; base += 64)
			{
				u64 n0 = 0, n1 = 0, nn = 0;
				if (base + 64 < n) col_planes(x, n, base + 64, n0, n1, nn);
				const KmerStep st = kmer_step(c0, c1, cn, n0, n1, nn, base, n_win, k, kmask, canonical);
				const u64 cnt = kmer_step_counts(t, st);
				const bool hit = st.good && cnt >= R.min_count;
				const u64 b_hit = __ballot(hit), b_miss = st.b_valid & ~b_hit;
				if (first_hit == n_win && b_hit) first_hit = base + (u64)__ffsll((long long)b_hit) - 1ull;
				if (first_miss == n_win && b_miss) first_miss = base + (u64)__ffsll((long long)b_miss) - 1ull;
				if (stored && st.good)
				{
					const u64 at = good_n + (u64)__popcll(st.b_good & lanemask_lt());
					const u16 v = (u16)(cnt < (u64)KMER_PLAN_COUNT_CAP ? cnt : (u64)KMER_PLAN_COUNT_CAP);
					if (in_lds) my_lds[at] = v; else my_spill[at] = v;
				}
				good_n += (u64)__popcll(st.b_good); hits += (u64)__popcll(b_hit);
				c0 = n0; c1 = n1; cn = nn;
			}
		}
		u32 median = 0;
		if (stored && good_n)
		{
			wave_fence();                                   // the counts are read by other lanes of this wave than wrote them
			median = in_lds ? kplan_select((const u16*)my_lds, good_n, good_n >> 1) : kplan_select((const u16*)my_spill, good_n, good_n >> 1);
			wave_fence();                                   // ... and the next record's stores stay behind these loads
		}
		u64 e_out = e;
		if (R.trim == KPLAN_TRIM_FIRST_MISS && first_miss < n_win) e_out = b + first_miss + k - 1;
		if (R.trim == KPLAN_TRIM_FIRST_HIT && first_hit < n_win) e_out = b + first_hit;
		u32 reason = 0;
		if (hits < (u64)R.min_hits || (R.max_hits != KMER_PLAN_NO_LIMIT && hits > (u64)R.max_hits)) reason = KPLAN_DROP_HITS;
		else if (n_win * R.min_permille > hits * 1000ull || hits * 1000ull > n_win * R.max_permille) reason = KPLAN_DROP_SHARE;
		else if (MEDIAN && (median < R.min_median || (R.max_median != KMER_PLAN_NO_LIMIT && median > R.max_median))) reason = KPLAN_DROP_MEDIAN;
		else if (e_out - b < (u64)R.min_len) reason = KPLAN_DROP_LENGTH;
		if (keep_in)
		{
			const u64 mine = lane == KPLAN_CONSIDERED ? 1u : lane == KPLAN_NO_WINDOW ? (n_win == 0 ? 1u : 0u) : lane == KPLAN_WINDOWS ? n_win : lane == KPLAN_GOOD ? good_n
			               : lane == KPLAN_HITS ? hits : lane == KPLAN_KEPT ? (reason == 0 ? 1u : 0u) : lane == KPLAN_WITH_HIT ? (hits ? 1u : 0u)
			               : lane == KPLAN_TRIMMED ? (e_out < e ? 1u : 0u) : lane == KPLAN_CUT ? e - e_out : lane == KPLAN_BASES ? (reason == 0 ? e_out - b : 0u)
			               : (reason != 0 && lane == reason ? 1u : 0u);
			sum += mine;
		}
		else if (lane == KPLAN_CAME_DROPPED) sum += 1;
		const u64 met = __ballot(1);                         // in place: k_columns_common.h
		if (lane == 0 && met)
		{
			o.begin[r] = b; o.end[r] = keep_in ? e_out : e; o.keep[r] = keep_in && reason == 0 ? 1 : 0;
			if (o.good) o.good[r] = good_n;
			if (o.hits) o.hits[r] = hits;
			if (o.median) o.median[r] = median;
		}
	}
	col_stats_flush(stats, KPLAN_N_STATS, sum);
}
