// Columnar k-mer correction: the second columnar call that writes new bases (the merge was the first), and the first that writes them
// from evidence outside the record -- every window of k bases of every considered record's range is looked up in a k-mer table
// (k_columns_kmer.h) that is ONLY READ; a sequencing error shows as a run of up to k consecutive windows that are not solid, and
// where exactly one replacement of the base that all of them share makes every one of them solid, that base is put right
// (include/dsrc_gpu.h: dsrcgpu_columns_kmer_correct has the rule as a serial loop).  Tadpole, Lighter, BFC, Musket and Quake do this;
// the rule here is the conservative core of theirs.  No counterpart in the reference.
//
//   k_kmer_correct_copy   a lane per 8 bytes, behind k_col_plan_check, out of place only: the bytes [S[0], S[n_records]) as they came
//   k_kmer_correct        a wave per record, 64 windows a step: the runs, their verdicts, the repaired bytes, d_fixed
//
// The pass over the windows is k_kmer_plan<false>'s (kmer_step, kmer_step_counts): the head lane of a run of equal neighbouring keys
// walks with kmer_find and the others take its count by shuffle.  New are the runs.  Per step the ballot of the valid windows that
// are not solid is scanned with wave-uniform bit operations (first set bit, first clear bit behind it); a run that reaches bit 63
// stays open and is carried into the next step, a run that is still open behind the last step ends at the last window.  Only a run's
// two ends are kept, so a read of 70 000 N is one run and costs nothing more than the plan's walk.
// A closed run [w0, w1] with a position p (the rule's three placements) is resolved by the whole wave: one col_planes(x, n, w0)
// gives every position the run's windows need -- w0 .. w1 + k - 1, at most 2 k - 1 <= 61 of them --, lane j of a half-wave takes window
// w0 + j with p's two plane bits replaced by a candidate; the two halves hold two candidates side by side, so four candidates are two
// rounds of at most 31 walks each, and the verdict per candidate is one ballot against the mask of the run's length.  A second code
// above 3 among the run's positions leaves no candidate and no walk.
// IN PLACE (out == c.bases) IS SOUND BECAUSE A WAVE NEVER LOADS A BYTE IT HAS CHANGED.  The staging of step `base` loads the positions
// base + 64 .. base + 127 in front of the runs that close in that step; such a run has w1 < base + 64, and p <= w1 unless the run
// touches the 3' end -- and then it is the record's last run and nothing is loaded behind it.  The resolution of a later run loads
// from its own w0 on, and every earlier repair sits at a p' <= w1' < w0: every window at or behind a later staging point starts behind
// p'.  No other wave reads the record.  Out of place the loads go to the input and the stores to the output, which the copy kernel
// has filled in an earlier launch.
// Every branch around a ballot or a shuffle is wave-uniform; the walks are the only divergent code.  No LDS, no scratch memory.
// Statistics: wave-uniform events, one to a lane (k_columns_common.h).  Atomics touch the statistics words only, the table is never
// written, and no lane waits for another wave.
//
// Portable subset only (__ballot, __shfl*, __popcll, __ffsll, __clzll, vector atomics): tests/emu builds this file unchanged.
#pragma once
#include "k_common.h"
#include "k_columns_common.h"
#include "k_columns_kmer.h"

enum { KCORR_CONSIDERED = 0, KCORR_CAME_DROPPED, KCORR_NO_WINDOW, KCORR_WINDOWS, KCORR_SOLID, KCORR_RUNS, KCORR_FIXED, KCORR_FIXED_N, KCORR_RECORDS_FIXED,
       KCORR_RUN_WHOLE, KCORR_RUN_LONG, KCORR_RUN_SHORT, KCORR_NO_CANDIDATE, KCORR_AMBIGUOUS, KCORR_QUALITY, KCORR_ALL_SOLID, KCORR_N_STATS = 16 };

// by value in the kernel arguments
struct KmerCorrectRules { u64 min_count; u32 max_quality; };

// grid (gx), a lane per 8 bytes with a grid stride, behind k_col_plan_check (nothing unless that pass was clean): out[S[0] .. S[n_recs]) =
// bases[S[0] .. S[n_recs]), not a byte before or behind.  Words of 8 bytes where the two arrays sit alike in their words (the head
// and the tail byte by byte), bytes throughout where they do not.
__global__ void __launch_bounds__(WG) k_kmer_correct_copy(ColIn c, u8* out, const u64* err)
{
	if (*err != COLE_NONE) return;
	const u64 lo = c.seq_offs[0], hi = c.seq_offs[c.n_recs];
	if (lo > hi || hi > c.bases_len) return;
	const u8* const src = c.bases + lo;
	u8* const dst = out + lo;
	const u64 n = hi - lo;
	const u64 tid = (u64)blockIdx.x * blockDim.x + threadIdx.x, step = (u64)gridDim.x * blockDim.x;
	u64 head = 0, words = 0;
	if ((((size_t)src ^ (size_t)dst) & 7u) == 0)
	{
		head = (u64)((8u - ((size_t)src & 7u)) & 7u);
		if (head > n) head = n;
		words = (n - head) >> 3;
	}
	for (u64 i = tid; i < head; i += step) dst[i] = src[i];
	const u64* const s8 = (const u64*)(src + head);
	u64* const d8 = (u64*)(dst + head);
	for (u64 i = tid; i < words; i += step) d8[i] = s8[i];
	for (u64 i = head + 8 * words + tid; i < n; i += step) dst[i] = src[i];
}

// One closed run [w0, w1] of the n_win windows of the range x[0 .. n), resolved by the whole wave (all arguments wave-uniform).
// -> what this lane adds to its statistic; `fixed` counts the repair.  q: the qualities of the range (read at p only, and only
// under max_quality < 255).  Lane 0 stores the one byte to out_x[p].
__device__ __forceinline__ u64 kcorr_run(const u8* x, const u8* q, u8* out_x, u64 n, u64 n_win, u64 w0, u64 w1, u32 k, u32 canonical, const KmerTab& t,
                                         const KmerCorrectRules& R, u64& fixed)
{
	const u32 lane = lane_id();
	const u64 add = lane == KCORR_RUNS ? 1u : 0u;
	const u64 len = w1 - w0 + 1;
	u32 why = 0;
	u64 p = 0;
	if (w0 == 0 && w1 == n_win - 1) why = KCORR_RUN_WHOLE;       // no solid window in the range
	else if (len > k) why = KCORR_RUN_LONG;                      // more than one error
	else if (w0 == 0) p = w1;                                    // the run touches the 5' end
	else if (w1 == n_win - 1) p = w0 + k - 1;                    // the run touches the 3' end
	else if (len == k) p = w1;                                   // interior
	else why = KCORR_RUN_SHORT;
	if (!why && R.max_quality < 255u && (u32)q[p] > R.max_quality) why = KCORR_QUALITY;
	if (why) return add + (lane == why ? 1u : 0u);
	// the positions w0 .. w0 + 63 of the range; the run's windows need w0 .. w1 + k - 1 <= w0 + 60, and p - w0 <= k - 1
	u64 r0, r1, rn;
	col_planes(x, n, w0, r0, r1, rn);
	const u32 at = (u32)(p - w0);
	const u64 bit = 1ull << at;
	const u32 orig = (rn & bit) ? 4u : (u32)((r0 >> at) & 1ull) | ((u32)((r1 >> at) & 1ull) << 1);
	const u64 span = (1ull << (len + k - 1)) - 1ull;
	u32 n_ok = 0, the_one = 0;
	if ((rn & ~bit & span) == 0)                                 // (else: another code above 3 under the run -- no candidate can mend it)
	{
		const u32 j = lane & 31u, half = lane >> 5;
		const u64 kmask = (1ull << k) - 1ull, all = (1ull << len) - 1ull;
		r0 &= ~bit; r1 &= ~bit;
		for (u32 round = 0; round < 2; ++round)
		{
			const u32 cand = 2u * round + half;
			const u64 m0 = r0 | ((u64)(cand & 1u) << at), m1 = r1 | ((u64)(cand >> 1) << at);
			const bool active = j < len && cand != orig;
			const u64 m = kmer_spread((u32)((m0 >> j) & kmask)) | (kmer_spread((u32)((m1 >> j) & kmask)) << 1);
			const u64 cnt = active ? kmer_find(t, kmer_key(m, k, canonical)) : 0ull;
			const u64 ok = __ballot(active && cnt >= R.min_count);
			if (2u * round != orig && (ok & all) == all) { ++n_ok; the_one = 2u * round; }
			if (2u * round + 1u != orig && ((ok >> 32) & all) == all) { ++n_ok; the_one = 2u * round + 1u; }
		}
	}
	if (n_ok != 1) return add + (lane == (n_ok ? KCORR_AMBIGUOUS : KCORR_NO_CANDIDATE) ? 1u : 0u);
	if (lane == 0) out_x[p] = (u8)the_one;
	fixed += 1;
	return add + (lane == KCORR_FIXED || (lane == KCORR_FIXED_N && orig > 3u) ? 1u : 0u);
}

// grid (gx), a wave per record with a grid stride, 64 windows a step; lane i of a step has the window that starts at position base +
// i of the range (kmer_step).  out: addressed like c.bases; c.bases itself (in place) or an array that k_kmer_correct_copy has
// filled.  See the head of this file for the runs and for why in place is sound.  fixed: n_recs entries or null; a record's entry is
// written whether or not it is considered.
__global__ void __launch_bounds__(WG) k_kmer_correct(ColIn c, ColPlanIn w, u32 k, u32 canonical, KmerTab t, KmerCorrectRules R, u8* out, u64* fixed_out,
                                                     u64* stats, const u64* err)
{
	if (*err != COLE_NONE) return;
	const u32 lane = lane_id();
	const u64 wpg = blockDim.x >> 6;
	const u64 kmask = (1ull << k) - 1ull;
	u64 sum = 0;                                         // lane s adds up statistic s
	for (u64 r = blockIdx.x * wpg + wave_id(); r < c.n_recs; r += gridDim.x * wpg)
	{
		u64 b, e;
		bool keep_in;
		if (!col_range(c, w, r, b, e, keep_in)) continue;
		const u64 n = e - b;
		const u64 n_win = keep_in && n >= k ? n - k + 1 : 0;
		u64 fixed = 0;
		if (n_win)
		{
			const u8* const x = c.bases + b;
			const u8* const q = c.quals ? c.quals + b : nullptr;
			u8* const out_x = out + b;
			u64 solid_n = 0, run_w0 = 0;
			bool open = false;                               // a run that began at run_w0 has not ended yet
			u64 c0, c1, cn;
			col_planes(x, n, 0, c0, c1, cn);
			for (u64 base = 0; base < n_win; base += 64)
			{
				u64 n0 = 0, n1 = 0, nn = 0;
				if (base + 64 < n) col_planes(x, n, base + 64, n0, n1, nn);
				const KmerStep st = kmer_step(c0, c1, cn, n0, n1, nn, base, n_win, k, kmask, canonical);
				const u64 cnt = kmer_step_counts(t, st);
				const u64 b_solid = __ballot(st.good && cnt >= R.min_count);
				const u64 bad = st.b_valid & ~b_solid;
				solid_n += (u64)__popcll(b_solid);
				// the runs of this step: `from` is the first bit that has not been looked at
				u32 from = 0;
				while (from < 64u)
				{
					const u64 ahead = ~0ull << from;
					if (!open)
					{
						const u64 first = bad & ahead;
						if (!first) break;
						from = (u32)__ffsll((long long)first) - 1u;
						run_w0 = base + from; open = true;
					}
					const u64 clear = ~bad & (~0ull << from);
					if (!clear) break;                              // up to bit 63: the run goes on in the next step (or ends with the range)
					from = (u32)__ffsll((long long)clear) - 1u;     // the first window behind the run
					sum += kcorr_run(x, q, out_x, n, n_win, run_w0, base + from - 1, k, canonical, t, R, fixed);
					open = false;
				}
				c0 = n0; c1 = n1; cn = nn;
			}
			if (open) sum += kcorr_run(x, q, out_x, n, n_win, run_w0, n_win - 1, k, canonical, t, R, fixed);
			sum += lane == KCORR_WINDOWS ? n_win : lane == KCORR_SOLID ? solid_n : lane == KCORR_ALL_SOLID ? (solid_n == n_win ? 1u : 0u)
			     : lane == KCORR_RECORDS_FIXED ? (fixed ? 1u : 0u) : 0u;
		}
		sum += keep_in ? (lane == KCORR_CONSIDERED || (lane == KCORR_NO_WINDOW && n_win == 0) ? 1u : 0u) : (lane == KCORR_CAME_DROPPED ? 1u : 0u);
		if (lane == 0 && fixed_out) fixed_out[r] = fixed;
	}
	col_stats_flush(stats, KCORR_N_STATS, sum);
}
