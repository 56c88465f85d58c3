// Columnar pair plan: the third planner, the first that reads two column sets -- record r of one is the mate of record r of the other.
// It takes a plan in per side (a range and a keep flag per record, or none) and gives a narrower plan out per side plus ONE keep flag for
// the pair: both mates survive or neither does.  The overlap of read 1 with the reverse complement of read 2 gives the insert size, and
// where the insert is shorter than a read the 3' end of that read is cut where the insert ends (include/dsrc_gpu.h:
// dsrcgpu_columns_pair_plan has the rule as a serial loop).  Hamming distance only, the first accepted shift wins: forward shifts d = 0,
// 1, .. first, then the read-through shifts d = -1, -2, ..  The caller's input arrays are only read.  No counterpart in the reference.
//
// Portable subset only (__ballot, __shfl*, __popcll, __ffsll, wave_fence, LDS, vector atomics): tests/emu builds this file unchanged.
#pragma once
#include "k_common.h"
#include "k_columns_common.h"

#define PAIR_MAX_BASES 1024u
#define PAIR_WORDS (PAIR_MAX_BASES / 64u)
#define PAIR_NO_INSERT (~0ull)
struct PairRules { u32 min_overlap, max_mm, permille, min_len; };
struct PairOut { u64* begin1; u64* end1; u64* begin2; u64* end2; u8* keep; u64* insert; };
enum { PAIR_KEPT = 0, PAIR_BASES_1, PAIR_BASES_2, PAIR_CUT_1, PAIR_CUT_2, PAIR_FOUND, PAIR_NARROWED, PAIR_DROP_MATE, PAIR_DROP_LEN, PAIR_LONG,
       PAIR_INSERT_SUM, PAIR_N_STATS };

// the range p[0 .. n), n <= PAIR_MAX_BASES, as three bit planes of PAIR_WORDS words each in the wave's LDS: bit 0 of the code, bit 1 of
// the code, code >= 4.  64 positions a step, a lane per position, each byte loaded once.  rev: position j is the complement of p[n - 1 -
// j] -- the lane loads from the back, so the reverse complement comes out in reading order and no bit is reversed.  Words at and beyond
// ceil(n / 64) are NOT written: the search never reads them (pair_word).  Bits at and beyond n in the last word are 0.
__device__ __forceinline__ void pair_lay(const u8* p, u32 n, bool rev, u64* pl)
{
	const u32 lane = lane_id();
	for (u32 base = 0; base < n; base += 64)
	{
		const u32 j = base + lane;
		const bool valid = j < n;
		u32 code = valid ? (u32)(rev ? p[n - 1u - j] : p[j]) : 0u;
		const bool amb = code >= 4u;
		if (rev) code ^= 3u;                             // comp(c) = 3 - c for c = 0 .. 3
		const bool acgt = valid && !amb;
		const u64 p0 = __ballot(acgt && (code & 1u)), p1 = __ballot(acgt && (code & 2u)), pn = __ballot(valid && amb);
		if (lane < 3) pl[lane * PAIR_WORDS + (base >> 6)] = lane == 0 ? p0 : lane == 1 ? p1 : pn;
	}
}

// word i of a plane of which nw words have been laid down; what lies behind them reads as 0, whatever the wave's previous pair left there
// (and index PAIR_WORDS is never touched)
__device__ __forceinline__ u64 pair_word(const u64* plane, u32 i, u32 nw) { return i < nw ? plane[i] : 0ull; }

// the compared length of candidate c: c < n1 is the forward shift d = c (x[d + i] against y[i]), otherwise the read-through shift d =
// -(c - n1 + 1) (x[i] against y[i - d])
__device__ __forceinline__ u32 pair_len(u32 c, u32 n1, u32 n2)
{
	if (c < n1) return min_u32(n1 - c, n2);
	return min_u32(n1, n2 - (c - n1 + 1u));
}

// grid (gx), a wave per pair with a grid stride, behind k_col_plan_check of either side (k_columns_common.h: the re-check -- here
// every figure of the pair is loaded before the first test --, in place, the statistics).  A pair that is searched -- both mates came
// in kept, both ranges at most PAIR_MAX_BASES long -- is laid down as bit planes (x = read 1's range, y = the reverse complement of
// read 2's), the wave meets, and the n1 + n2 - 1 candidates are judged 64 at a time in the rule's order: lane l of batch k has
// candidate c = 64 k + l.  One side of a candidate is shifted (x for d >= 0, y for d < 0) and one is not; per word of the overlap the
// lane cuts a 64-bit window of the shifted side out of two neighbouring LDS words (bit offset 0: the first word as it is -- a shift
// by 64 is not a shift by 0), compares it with the aligned word of the other side under the mask of the positions that are left of L
// (64 and more: all ones), and adds up the popcounts.  The word loop runs to the longest overlap of the batch, which is that of its
// first candidate or of its first read-through candidate -- wave-uniform, as every branch here; a batch whose longest overlap is
// below min_overlap is skipped.  A ballot and __ffsll give the first accepted candidate; behind a batch with a hit none is read.  In
// place: each output may be its input counterpart, and keep may be either incoming keep.
__global__ void __launch_bounds__(WG) k_pair_plan(ColIn c1, ColIn c2, ColPlanIn w1, ColPlanIn w2, PairRules R, PairOut o, u64* stats, const u64* err)
{
	if (err[0] != COLE_NONE || err[1] != COLE_NONE) return;
	__shared__ u64 s_planes[WG / 64][6 * PAIR_WORDS];
	u64* const pl = s_planes[wave_id()];
	const u32 lane = lane_id();
	const u64 wpg = blockDim.x >> 6;
	u64 sum = 0;                                         // lane k adds up statistic k
	for (u64 r = blockIdx.x * wpg + wave_id(); r < c1.n_recs; r += gridDim.x * wpg)
	{
		const u64 s1 = c1.seq_offs[r], t1 = c1.seq_offs[r + 1], s2 = c2.seq_offs[r], t2 = c2.seq_offs[r + 1];
		u64 b1, e1, b2, e2;
		col_range_load(w1, r, s1, t1, b1, e1);
		col_range_load(w2, r, s2, t2, b2, e2);
		const bool k1 = w1.keep ? w1.keep[r] != 0 : true, k2 = w2.keep ? w2.keep[r] != 0 : true;
		if (!col_range_ok(c1, s1, t1, b1, e1) || !col_range_ok(c2, s2, t2, b2, e2)) continue;
		const u64 n1 = e1 - b1, n2 = e2 - b2;
		const bool both = k1 && k2;
		const bool is_long = both && (n1 > PAIR_MAX_BASES || n2 > PAIR_MAX_BASES);
		u64 len1 = n1, len2 = n2, insert = PAIR_NO_INSERT;
		if (both && !is_long && n1 && n2)
		{
			const u32 m1 = (u32)n1, m2 = (u32)n2;
			const u32 nw1 = (m1 + 63u) >> 6, nw2 = (m2 + 63u) >> 6;
			pair_lay(c1.bases + b1, m1, false, pl);
			pair_lay(c2.bases + b2, m2, true, pl + 3 * PAIR_WORDS);
			wave_fence();                                    // the planes are read by other lanes than those that wrote them
			const u32 n_cand = m1 + m2 - 1u;
			u32 hit = n_cand;
			for (u32 cb = 0; cb < n_cand; cb += 64)
			{
				u32 l_max = pair_len(cb, m1, m2);
				if (cb < m1 && m1 - cb < 64u && m1 < n_cand)       // the switch to d < 0 falls into this batch: d = -1 has the longest overlap of those
				{
					const u32 l_rev = pair_len(m1, m1, m2);
					l_max = l_rev > l_max ? l_rev : l_max;
				}
				if (l_max < R.min_overlap) continue;
				const u32 cand = cb + lane;
				const bool valid = cand < n_cand;
				const bool fwd = cand < m1;
				const u32 shift = !valid ? 0u : fwd ? cand : cand - m1 + 1u;
				const u32 L = valid ? pair_len(cand, m1, m2) : 0u;
				const u64* const sh = pl + (fwd ? 0u : 3u * PAIR_WORDS);      // the shifted side's planes and the other side's
				const u64* const fx = pl + (fwd ? 3u * PAIR_WORDS : 0u);
				const u32 nw_sh = fwd ? nw1 : nw2;
				const u32 q = shift >> 6, off = shift & 63u, up = (64u - off) & 63u;
				const u32 n_words = (l_max + 63u) >> 6;          // <= ceil(min(m1, m2) / 64): word k of the unshifted side has been laid down
				u32 mm = 0;
				for (u32 k = 0; k < n_words; ++k)
				{
					const u32 done = k << 6;
					const u32 rem = L > done ? L - done : 0u;
					const u64 mask = rem >= 64u ? ~0ull : (1ull << rem) - 1ull;
					const u32 i = q + k;
					const u64 a0 = (pair_word(sh, i, nw_sh) >> off) | (off ? pair_word(sh, i + 1u, nw_sh) << up : 0ull);
					const u64 a1 = (pair_word(sh + PAIR_WORDS, i, nw_sh) >> off) | (off ? pair_word(sh + PAIR_WORDS, i + 1u, nw_sh) << up : 0ull);
					const u64 an = (pair_word(sh + 2 * PAIR_WORDS, i, nw_sh) >> off) | (off ? pair_word(sh + 2 * PAIR_WORDS, i + 1u, nw_sh) << up : 0ull);
					mm += (u32)__popcll(((a0 ^ fx[k]) | (a1 ^ fx[PAIR_WORDS + k]) | an | fx[2 * PAIR_WORDS + k]) & mask);
				}
				const bool ok = valid && L >= R.min_overlap && mm <= R.max_mm && mm * 1000u <= L * R.permille;
				const u64 any = __ballot(ok);
				if (any)
				{
					hit = cb + (u32)__ffsll((long long)any) - 1u;
					break;
				}
			}
			if (hit < n_cand)
			{
				// d + n2 >= 1 for every candidate, so neither length falls below 1
				const u64 dn2 = hit < m1 ? (u64)hit + n2 : n2 - (u64)(hit - m1 + 1u);
				const u64 f1 = b1 - s1, f2 = b2 - s2;
				insert = dn2 + f1 + f2;
				len1 = n1 < dn2 + f2 ? n1 : dn2 + f2;            // min(n1, I - f1)
				len2 = n2 < dn2 + f1 ? n2 : dn2 + f1;            // min(n2, I - f2)
			}
			wave_fence();                                    // every lane has read the planes before the wave's next pair overwrites them
		}
		const bool keep_out = both && len1 >= R.min_len && len2 >= R.min_len;
		const bool found = insert != PAIR_NO_INSERT;
		const u64 mine = lane == PAIR_KEPT ? (keep_out ? 1u : 0u) : lane == PAIR_BASES_1 ? (keep_out ? len1 : 0u) : lane == PAIR_BASES_2 ? (keep_out ? len2 : 0u)
		               : lane == PAIR_CUT_1 ? (keep_out ? n1 - len1 : 0u) : lane == PAIR_CUT_2 ? (keep_out ? n2 - len2 : 0u) : lane == PAIR_FOUND ? (found ? 1u : 0u)
		               : lane == PAIR_NARROWED ? (found && (len1 < n1 || len2 < n2) ? 1u : 0u) : lane == PAIR_DROP_MATE ? (k1 != k2 ? 1u : 0u)
		               : lane == PAIR_DROP_LEN ? (both && !keep_out ? 1u : 0u) : lane == PAIR_LONG ? (is_long ? 1u : 0u) : lane == PAIR_INSERT_SUM ? (found ? insert : 0u) : 0u;
		sum += mine;
		const u64 met = __ballot(1);                         // in place: k_columns_common.h
		if (lane == 0 && met)
		{
			o.begin1[r] = b1; o.end1[r] = b1 + len1; o.begin2[r] = b2; o.end2[r] = b2 + len2; o.keep[r] = keep_out ? 1 : 0;
			if (o.insert) o.insert[r] = insert;
		}
	}
	col_stats_flush(stats, PAIR_N_STATS, sum);
}
