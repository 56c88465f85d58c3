// Columnar merge: what stands behind the pair plan -- the two mates of a short insert become ONE read, with a consensus where they
// overlap (include/dsrc_gpu.h: dsrcgpu_columns_merge_device has the rule as a serial loop).  The first columnar call that writes new
// bases and qualities instead of copying ranges.  It searches nothing: the insert size of every pair is the caller's (as
// dsrcgpu_columns_pair_plan wrote it), and a pair's offsets, ranges and geometry are tested before a byte of it is read.  The caller's
// input arrays are only read.  No counterpart in the reference.
//
// Four launches of its own around k_sel_scan_tiles: the judge (a verdict and a merged length per pair, the twelve statistics), the
// tile sums, [the scan of the tile sums], the apply pass (behind the host's capacity check the first kernel that writes the caller's
// arrays) and the writer.  No kernel waits on another workgroup.
//
// Portable subset only (__ballot, __shfl*, __popcll, __syncthreads, LDS, vector atomics, plain vector stores): tests/emu
// builds this file unchanged.
#pragma once
#include "k_common.h"
#include "k_columns_common.h"
#include "k_columns_sel.h"
#include "k_columns_pair.h"

#define MERGE_NOT (~0ull)
#define MERGE_MAX_INSERT (1ull << 40)
#define MERGE_STEPS 4u                                   // steps of 64 overlap positions the judge loads at once
struct MergeRules { u32 min_overlap, max_mm, permille, qcap; };
struct MergeWhat { ColPlanIn w1, w2; const u8* keep; const u64* insert; };      // w<s>.keep is not used: ONE flag covers the pair
enum { MERGE_MERGED = 0, MERGE_BASES, MERGE_OVERLAP, MERGE_AGREE, MERGE_CORRECTED, MERGE_ONE_SIDED, MERGE_NEITHER, MERGE_NOT_KEPT, MERGE_NO_INSERT,
       MERGE_GEOMETRY, MERGE_SHORT, MERGE_BUDGET, MERGE_N_STATS };

// COMP over the code alphabet "ACGTNRWSKMDVHBYXU.-": 3 2 1 0 4 14 6 7 9 8 12 13 10 11 5 15 0 17 18, a byte per code in three
// registers; a code above 18 is its own complement
__device__ __forceinline__ u32 merge_comp(u32 c)
{
	const u64 t = c < 8u ? 0x07060E0400010203ull : c < 16u ? 0x0F050B0A0D0C0809ull : 0x0000000000121100ull;
	const u32 v = (u32)(t >> ((c & 7u) << 3)) & 255u;
	return c > 18u ? c : v;
}

// one pair's place in insert coordinates: read 1's range lies at [a1, z1), the reverse complement of read 2's at [a2, z2)
struct MergeGeo { u64 b1, e2, a1, z1, a2, z2; };

// The reasons 1 .. 4 for pair r, in the rule's order, behind the re-check of either side (k_columns_common.h): 0 = goes on to the budget,
// else the statistic the pair counts in; ~0u = an offset or range is out of order, the pair counts in nothing.  No base is read here.
__device__ __forceinline__ u32 merge_geometry(const ColIn& c1, const ColIn& c2, const MergeWhat& w, u32 min_overlap, u64 r, MergeGeo& g)
{
	// (every load of the pair's figures is issued before the first test: the arrays hold an entry per pair, so the addresses are good
	// whatever the entries are, and the wave waits for memory once instead of four times in a row)
	const u64 s1 = c1.seq_offs[r], t1 = c1.seq_offs[r + 1], s2 = c2.seq_offs[r], t2 = c2.seq_offs[r + 1];
	u64 b1, e1, b2, e2;
	col_range_load(w.w1, r, s1, t1, b1, e1);
	col_range_load(w.w2, r, s2, t2, b2, e2);
	const bool kept = w.keep ? w.keep[r] != 0 : true;
	const u64 I = w.insert[r];
	if (!col_range_ok(c1, s1, t1, b1, e1) || !col_range_ok(c2, s2, t2, b2, e2)) return ~0u;
	if (!kept) return MERGE_NOT_KEPT;
	if (I == PAIR_NO_INSERT) return MERGE_NO_INSERT;
	const u64 f1 = b1 - s1, n1 = e1 - b1, f2 = b2 - s2, n2 = e2 - b2;      // each below 2^56: no sum of two wraps
	if (I >= MERGE_MAX_INSERT || n1 == 0 || n2 == 0 || I < f2 + n2 || f1 + n1 > I) return MERGE_GEOMETRY;
	g.b1 = b1; g.e2 = e2; g.a1 = f1; g.z1 = f1 + n1; g.a2 = I - f2 - n2; g.z2 = I - f2;       // all at most I < 2^40
	const i64 V = (i64)(g.z1 < g.z2 ? g.z1 : g.z2) - (i64)(g.a1 > g.a2 ? g.a1 : g.a2);
	if (V < (i64)min_overlap) return MERGE_SHORT;
	return 0;
}

// grid (gx), a wave per pair with a grid stride, behind k_col_plan_check of either side (nothing happens unless both passes were clean).
// The reasons 1 .. 4 come from merge_geometry; for the budget the wave walks the overlap 64 positions a step, a lane per position,
// MERGE_STEPS steps to a round (a 150-base overlap is one round: one wait for memory) --
// read 1 forwards from b1 + (lo - a1), read 2 backwards from e2 - 1 - (lo - a2), both contiguous -- and three ballots and popcounts
// give the classes of the step: both codes below 4 and equal, both below 4 and different, exactly one below 4; the rest of the step's
// positions have neither below 4.  mm is what is not "equal".  Every branch is wave-uniform.  len[r] = the merged length or MERGE_NOT
// (arena scratch, which the host has filled with MERGE_NOT).  Statistics: lane k adds up statistic k in a register; at the end the
// waves of a workgroup meet once (every thread reaches that barrier: the test of the error words above is the same for all of them),
// and one vector atomic per statistic and workgroup goes out if it is not 0 -- sums, so the result does not depend on any order.
__global__ void __launch_bounds__(WG) k_merge_judge(ColIn c1, ColIn c2, MergeWhat w, MergeRules R, u64* len, u64* stats, const u64* err)
{
	if (err[0] != COLE_NONE || err[1] != COLE_NONE) return;
	const u32 lane = lane_id();
	const u64 wpg = blockDim.x >> 6;
	u64 sum = 0;                                         // lane k adds up statistic k
	for (u64 r = blockIdx.x * wpg + wave_id(); r < c1.n_recs; r += gridDim.x * wpg)
	{
		MergeGeo g;
		u32 why = merge_geometry(c1, c2, w, R.min_overlap, r, g);
		if (why == ~0u) continue;
		u64 V = 0, L = 0, eq = 0, diff = 0, one = 0;
		if (!why)
		{
			const u64 lo = g.a1 > g.a2 ? g.a1 : g.a2, hi = g.z1 < g.z2 ? g.z1 : g.z2;
			V = hi - lo;
			const u8* const x = c1.bases + g.b1 + (lo - g.a1);            // x[i], i < V: inside [b1, e1)
			const u8* const y = c2.bases + g.e2 - 1 - (lo - g.a2);        // y[-i], i < V: inside [b2, e2)
			for (u64 base = 0; base < V; base += 64 * MERGE_STEPS)
			{
				u32 k1[MERGE_STEPS], k2[MERGE_STEPS];            // the loads of MERGE_STEPS steps first, so that their latencies overlap
#pragma unroll
				for (u32 u = 0; u < MERGE_STEPS; ++u)
				{
					const u64 i = base + 64u * u + lane;
					const bool valid = i < V;                        // a position outside the overlap reads as "neither" and is in no ballot
					k1[u] = valid ? (u32)x[i] : 4u; k2[u] = valid ? (u32)*(y - i) : 4u;
				}
#pragma unroll
				for (u32 u = 0; u < MERGE_STEPS; ++u)
				{
					const u32 c2 = merge_comp(k2[u]);
					const bool l1 = k1[u] < 4u, l2 = c2 < 4u;
					eq += (u64)__popcll(__ballot(l1 && l2 && k1[u] == c2));
					diff += (u64)__popcll(__ballot(l1 && l2 && k1[u] != c2));
					one += (u64)__popcll(__ballot(l1 != l2));
				}
			}
			const u64 mm = V - eq;
			if (mm > R.max_mm || mm * 1000u > V * R.permille) why = MERGE_BUDGET;
			else L = (g.z1 > g.z2 ? g.z1 : g.z2) - (g.a1 < g.a2 ? g.a1 : g.a2);
		}
		const bool merged = !why;
		const u64 mine = !merged ? (lane == why ? 1u : 0u)
		               : lane == MERGE_MERGED ? 1u : lane == MERGE_BASES ? L : lane == MERGE_OVERLAP ? V : lane == MERGE_AGREE ? eq : lane == MERGE_CORRECTED ? diff
		               : lane == MERGE_ONE_SIDED ? one : lane == MERGE_NEITHER ? V - eq - diff - one : 0u;
		sum += mine;
		if (lane == 0) len[r] = merged ? L : MERGE_NOT;
	}
	// the waves of the workgroup add up in LDS first: twelve atomics a workgroup instead of twelve a wave on the same twelve words
	__shared__ u64 s_sum[WG / 64][MERGE_N_STATS];
	if (lane < MERGE_N_STATS) s_sum[wave_id()][lane] = sum;
	__syncthreads();
	if (threadIdx.x < MERGE_N_STATS)
	{
		u64 all = 0;
		for (u32 k = 0; k < (blockDim.x >> 6); ++k) all += s_sum[k][threadIdx.x];
		if (all) atomicAdd((unsigned long long*)&stats[threadIdx.x], (unsigned long long)all);
	}
}

// Pair r's contribution to the three sums -- merged flag, merged bases, title bytes of read 1 -- from the judge's scratch.  The title
// offsets of read 1 are checked here, for merged and unmerged pairs alike, as the select checks them (err == nullptr: the apply pass,
// which runs behind a clean first pass and reports nothing); a pair that fails counts as 0 / 0 / 0.
__device__ __forceinline__ void merge_record(const ColIn& c1, const u64* len, u32 titles, u64 r, u64* err, u64 v[3])
{
	v[0] = v[1] = v[2] = 0;
	if (r >= c1.n_recs) return;
	u64 tl = 0;
	if (titles)
	{
		const u64 t0 = c1.title_offs[r], t1 = c1.title_offs[r + 1];
		if (t0 > t1) { if (err) col_err(err, r, COLE_TITLE_ORDER); return; }
		if (t1 > c1.titles_len) { if (err) col_err(err, r, COLE_TITLE_END); return; }
		tl = t1 - t0;
	}
	const u64 L = len[r];
	if (L == MERGE_NOT) return;
	v[0] = 1; v[1] = L; v[2] = tl;
}

// pass 1 of the placement, as k_sel_tiles: a tile = blockDim.x pairs, a thread per pair, workgroups stride over the tiles.  The tile
// sums go through k_sel_scan_tiles as the select's do.
__global__ void __launch_bounds__(WG) k_merge_tiles(ColIn c1, const u64* len, u32 titles, u64 n_tiles, u64* tile_sums, u64* err)
{
	for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
	{
		u64 v[3], ex[3], tot[3];
		merge_record(c1, len, titles, tile * blockDim.x + threadIdx.x, err, v);
		block_excl_scan3(v, ex, tot);
		if (threadIdx.x == 0) for (u32 k = 0; k < 3; ++k) tile_sums[3 * tile + k] = tot[k];
	}
}

// pass 3, as k_sel_apply (behind the host's capacity check: the first kernel that writes the caller's arrays): merged pair r becomes
// output record j = its place among the merged ones; the output offsets and d_source get entry j, merged[r] = 1 / 0 for every pair,
// pos[r] = j or SEL_DROPPED is what the writer reads.  The first workgroup writes the closing entries.
__global__ void __launch_bounds__(WG) k_merge_apply(ColIn c1, const u64* len, u32 titles, u64 n_tiles, const u64* tile_sums, SelOut o, u8* merged, u64* pos)
{
	if (blockIdx.x == 0 && threadIdx.x == 0)
	{
		o.seq_offs[o.kept] = o.n_bases;
		if (titles) o.title_offs[o.kept] = o.n_title;
	}
	for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
	{
		const u64 r = tile * blockDim.x + threadIdx.x;
		u64 v[3], ex[3], tot[3];
		merge_record(c1, len, titles, r, nullptr, v);
		block_excl_scan3(v, ex, tot);
		if (r >= c1.n_recs) continue;
		const u64 j = tile_sums[3 * tile] + ex[0];
		if (!v[0] || j >= o.kept) { pos[r] = SEL_DROPPED; merged[r] = 0; continue; }      // (j >= kept: never behind a clean pass 1 on unchanged arrays)
		o.seq_offs[j] = tile_sums[3 * tile + 1] + ex[1];
		if (titles) o.title_offs[j] = tile_sums[3 * tile + 2] + ex[2];
		if (o.source) o.source[j] = r;
		pos[r] = j; merged[r] = 1;
	}
}

// the writer, grid (gx), a wave per INPUT pair, unmerged pairs go no further than their figures; a lane per output position, a byte of bases and a byte
// of qualities per lane and step (k_sel_gather's shape).  The geometry is taken from the inputs again and tested again, and the
// judge's length and the destination the apply pass wrote must agree with it and lie inside the output (never otherwise behind clean
// passes on unchanged arrays).  Output position p lies at P = min(a1, a2) + p of the insert: read 1's byte is at b1 + P - a1, read 2's
// at e2 - 1 - (P - a2); a position one read covers takes that read's code and quality, one that both cover the consensus -- selects
// only.  The title is read 1's, whole.
__global__ void __launch_bounds__(WG) k_merge_write(ColIn c1, ColIn c2, MergeWhat w, MergeRules R, const u64* len, const u64* pos, SelOut o, u32 titles)
{
	const u32 lane = lane_id();
	const u64 wpg = blockDim.x >> 6;
	for (u64 r = blockIdx.x * wpg + wave_id(); r < c1.n_recs; r += gridDim.x * wpg)
	{
		const u64 j = pos[r], len_r = len[r];                // (loaded beside the pair's figures: one wait, as in merge_geometry)
		MergeGeo g;
		const u32 why = merge_geometry(c1, c2, w, R.min_overlap, r, g);
		if (j == SEL_DROPPED || why != 0) continue;
		const u64 P0 = g.a1 < g.a2 ? g.a1 : g.a2, L = (g.z1 > g.z2 ? g.z1 : g.z2) - P0, d = o.seq_offs[j];
		if (L != len_r || d > o.n_bases || L > o.n_bases - d) continue;
		for (u64 p = lane; p < L; p += 64)
		{
			const u64 P = P0 + p;
			const bool in1 = P >= g.a1 && P < g.z1, in2 = P >= g.a2 && P < g.z2;
			const u64 i1 = g.b1 + (P - g.a1), i2 = g.e2 - 1 - (P - g.a2);
			const u32 k1 = in1 ? (u32)c1.bases[i1] : 0u, q1 = in1 ? (u32)c1.quals[i1] : 0u;
			const u32 k2 = in2 ? merge_comp(c2.bases[i2]) : 0u, q2 = in2 ? (u32)c2.quals[i2] : 0u;
			const bool l1 = k1 < 4u, l2 = k2 < 4u;
			const u32 qmax = q1 > q2 ? q1 : q2, top = R.qcap > qmax ? R.qcap : qmax;
			u32 code, q;
			if (l1 && l2 && k1 == k2) { code = k1; q = q1 + q2 < top ? q1 + q2 : top; }
			else if (l1 && l2) { code = q1 >= q2 ? k1 : k2; q = q1 >= q2 ? q1 - q2 : q2 - q1; }
			else if (l1 != l2) { code = l1 ? k1 : k2; q = l1 ? q1 : q2; }
			else { code = k1; q = q1 < q2 ? q1 : q2; }
			if (!in2) { code = k1; q = q1; }
			if (!in1) { code = k2; q = q2; }
			o.bases[d + p] = (u8)code;
			o.quals[d + p] = (u8)q;
		}
		if (titles)
		{
			const u64 t0 = c1.title_offs[r], t1 = c1.title_offs[r + 1], dt = o.title_offs[j];
			if (t0 > t1 || t1 > c1.titles_len || dt > o.n_title || t1 - t0 > o.n_title - dt) continue;
			for (u64 k = lane; k < t1 - t0; k += 64) o.titles[dt + k] = c1.titles[t0 + k];
		}
	}
}
