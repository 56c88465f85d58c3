// Columnar profile: the per-cycle quality report of a set of records under a plan (per record a range and a keep flag, or none: whole
// reads, every record) -- base composition and quality sum by cycle, the quality histogram, the length, GC and mean-quality
// distributions and eight totals, all as uint64 counts in one array (include/dsrc_gpu.h: dsrcgpu_columns_profile has the layout and
// the rule as a serial loop).  The caller's arrays are only read.  No counterpart in the reference.
//
// Portable subset only (static __shared__, __syncthreads, __ballot, __shfl*, __popcll, vector atomics): tests/emu builds this file
// unchanged; there __shared__ is a process-wide static, so the kernel zeroes its tables itself.
#pragma once
#include "k_common.h"
#include "k_columns_common.h"

#define PROF_MAX_CYCLES 1024u
#define PROF_SMALL_CYCLES 256u                           // the table capacity of the second instantiation
#define PROF_WORDS(C) (11u * (C) + 622u)
enum { PROF_RECORDS = 0, PROF_BASES, PROF_Q20, PROF_Q30, PROF_QSUM, PROF_GC, PROF_OTHER, PROF_EMPTY, PROF_N_TOTALS };
// the grid: at most this many workgroups, whatever the record count -- every workgroup ends with one pass of 64-bit atomics over
// its whole table, so more workgroups than the chip holds at a time only add flushes (the small table fits twice into a CU's LDS
// beside 2 x 16 waves, the large one once)
__host__ __device__ __forceinline__ u32 prof_max_grid(u32 n_cycles) { return n_cycles <= PROF_SMALL_CYCLES ? 512u : 256u; }

__device__ __forceinline__ void prof_add(u64* p, u64 v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }

// grid (gx), a wave per record with a grid stride, behind k_col_plan_check (k_columns_common.h: the re-check).  The workgroup keeps a
// whole profile of C cycles in LDS, in the layout of the result and in 64-bit words throughout: no partial can wrap, whatever a
// record's length (one record of 2^32 bases may fold into one cycle), and the flush at the end is one loop.  CAP is the capacity of
// that table in cycles; the host picks the instantiation.  The second launch bound asks for the registers of 8 waves per SIMD (64)
// where the table leaves room for two workgroups on a CU: left alone the compiler takes 65, which is 7 waves, which is one workgroup
// of 16.
// Per tile of 64 positions a lane has one base and one quality.  Positions below C go to their own cycle: 64 lanes, 64 different
// addresses of the two per-cycle tables.  Positions from C on all fold into cycle C - 1: they are counted per class with ballots
// (the quality sum from the eight bit planes of q: sum = sum_b 2^b popcount(class & plane b)) in wave-uniform registers and are
// added to the table once per record.  The quality histogram takes one add per lane, or one per tile where the whole tile has
// one quality (binned qualities, and the worst case of 64 lanes on one address).  Length, GC and mean-quality bins get one add per
// record from lane 0; the eight totals are summed one to a lane over the wave's records and added once per wave.
// Everything is an integer sum: the result does not depend on the order of the waves.
template <u32 CAP>
__global__ void __launch_bounds__(WG, CAP <= PROF_SMALL_CYCLES ? 8 : 4) k_prof(ColIn c, ColPlanIn w, u32 C, u64* prof, const u64* err)
{
	if (*err != COLE_NONE) return;
	__shared__ u64 s_p[PROF_WORDS(CAP)];
	const u32 words = PROF_WORDS(C);
	for (u32 i = threadIdx.x; i < words; i += blockDim.x) s_p[i] = 0;
	__syncthreads();
	u64* const s_base = s_p + 8; u64* const s_qsum = s_p + 8 + 5 * C; u64* const s_qhist = s_p + 8 + 10 * C;
	u64* const s_len = s_p + 264 + 10 * C; u64* const s_gc = s_p + 265 + 11 * C; u64* const s_meanq = s_p + 366 + 11 * C;
	const u32 lane = lane_id();
	const u64 wpg = blockDim.x >> 6;
	u64 sum = 0;                                         // lane k adds up total k
	const u64 wave = (u32)__builtin_amdgcn_readfirstlane((int)wave_id());      // (the compiler is told that a record's figures are wave-uniform)
	for (u64 r = blockIdx.x * wpg + wave; r < c.n_recs; r += gridDim.x * wpg)
	{
		u64 b, e;
		if (!col_range(c, w, r, b, e)) continue;
		if (w.keep && w.keep[r] == 0) continue;
		const u64 n = e - b;
		const u8* const x = c.bases + b; const u8* const qp = c.quals + b;
		u64 qs_lane = 0, acgt = 0, gc = 0, q20 = 0, q30 = 0;
		u64 fc[5] = {0, 0, 0, 0, 0}, fq[5] = {0, 0, 0, 0, 0};      // what folds into cycle C - 1: count and quality sum per class
		for (u64 base = 0; base < n; base += 64)
		{
			const u64 i = base + lane;
			const bool valid = i < n;
			const u32 code = valid ? x[i] : 0u, q = valid ? qp[i] : 0u;
			const u32 cls = code < 4u ? code : 4u;
			const bool fold = valid && i >= C;
			if (valid && !fold) { prof_add(&s_base[i * 5 + cls], 1); prof_add(&s_qsum[i * 5 + cls], q); }
			const u32 q_first = __shfl(q, 0);                  // (lane 0 of a tile is always inside the range)
			if (__ballot(valid && q != q_first) == 0)
			{
				if (lane == 0) prof_add(&s_qhist[q_first], n - base < 64 ? n - base : 64);
			}
			else if (valid) prof_add(&s_qhist[q], 1);
			acgt += (u64)__popcll(__ballot(valid && code < 4u));
			gc += (u64)__popcll(__ballot(valid && (code == 1u || code == 2u)));
			q20 += (u64)__popcll(__ballot(valid && q >= 20u));
			q30 += (u64)__popcll(__ballot(valid && q >= 30u));
			qs_lane += q;
			if (__ballot(fold))
			{
				u64 plane[8];
#pragma unroll
				for (u32 bit = 0; bit < 8; ++bit) plane[bit] = __ballot(fold && ((q >> bit) & 1u));
#pragma unroll
				for (u32 k = 0; k < 5; ++k)
				{
					const u64 m = __ballot(fold && cls == k);
					fc[k] += (u64)__popcll(m);
#pragma unroll
					for (u32 bit = 0; bit < 8; ++bit) fq[k] += (u64)__popcll(m & plane[bit]) << bit;
				}
			}
		}
		// a lane's share of the quality sum is below 2^32 while the record has at most 2^24 bases, and so is the sum of all of them
		const u64 qs = n <= (1u << 24) ? (u64)wave_sum((u32)qs_lane) : wave_sum64(qs_lane);
		if (n > C)
		{
			const u64 cnt = lane == 0 ? fc[0] : lane == 1 ? fc[1] : lane == 2 ? fc[2] : lane == 3 ? fc[3] : fc[4];
			const u64 qsm = lane == 0 ? fq[0] : lane == 1 ? fq[1] : lane == 2 ? fq[2] : lane == 3 ? fq[3] : fq[4];
			if (lane < 5 && cnt) { prof_add(&s_base[(u64)(C - 1) * 5 + lane], cnt); prof_add(&s_qsum[(u64)(C - 1) * 5 + lane], qsm); }
		}
		// 100 * gc / acgt and qs / n: in 32 bits where everything fits (a 64-bit division is a long routine)
		const bool narrow = n <= (1u << 24);
		const u32 gc_bin = acgt == 0 ? 0u : narrow ? 100u * (u32)gc / (u32)acgt : (u32)(100ull * gc / acgt);
		const u32 mq_bin = n == 0 ? 0u : narrow ? (u32)qs / (u32)n : (u32)(qs / n);
		if (lane == 0)
		{
			prof_add(&s_len[n < C ? n : C], 1);
			if (acgt) prof_add(&s_gc[gc_bin], 1);
			if (n) prof_add(&s_meanq[mq_bin], 1);
		}
		sum += lane == PROF_RECORDS ? 1u : lane == PROF_BASES ? n : lane == PROF_Q20 ? q20 : lane == PROF_Q30 ? q30 : lane == PROF_QSUM ? qs
		     : lane == PROF_GC ? gc : lane == PROF_OTHER ? n - acgt : lane == PROF_EMPTY ? (n == 0 ? 1u : 0u) : 0u;
	}
	if (lane < PROF_N_TOTALS && sum) prof_add(&s_p[lane], sum);
	__syncthreads();
	for (u32 i = threadIdx.x; i < words; i += blockDim.x)
	{
		const u64 v = s_p[i];
		if (v) prof_add(&prof[i], v);
	}
}

// this call's profile (arena scratch) into the caller's array: stored, or added to what is there; nothing unless the check pass was clean
__global__ void __launch_bounds__(WG) k_prof_store(const u64* mine, u64* out, u32 words, u32 accumulate, const u64* err)
{
	if (*err != COLE_NONE) return;
	for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < words; i += gridDim.x * blockDim.x) out[i] = accumulate ? out[i] + mine[i] : mine[i];
}
