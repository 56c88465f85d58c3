// What the columnar kernels share (k_columns_enc.h and every file behind it): the caller's arrays and a plan by value, the error
// word, and the few pieces of device text that every planner used to carry a copy of.  A new planner reaches for
//   ColIn, ColPlanIn, col_err        the arrays, the plan in, the error word          k_col_plan_check  the check pass in front of it
//   col_range                        record r's range, re-checked                    col_range_load / col_range_ok  the same in two halves
//   col_planes, col_funnel           64 positions as three bit planes; 64 positions from any bit of a tile pair
//   wave_sum64, wave_max64, wave_incl_scan64, col_stats_flush
// and for a walk over k-mer windows for kmer_step / kmer_step_counts (k_columns_kmer.h).  Four facts are stated here once:
//
// THE RE-CHECK.  A planner runs behind k_col_plan_check and does nothing unless that pass was clean, so col_range never fails.  It
// tests a record's offsets and range all the same before a byte of the record is read: that is what keeps every read inside the
// caller's arrays whatever they hold (they are the caller's, and may change between the two launches).
// A SHIFT BY 64 IS NOT A SHIFT BY 0.  A window of 64 positions that starts at bit 0 of a tile is the tile itself; col_funnel says so.
// LANE k ADDS UP STATISTIC k.  The statistics are integer sums: a lane keeps one in a register over the wave's records and
// col_stats_flush issues one vector atomic add per lane at the wave's end if it is not 0, so no order of the waves changes a bit.
// IN PLACE.  A planner's output arrays may be its input counterparts: a wave reads begin / end / keep of its record before lane 0
// writes them.  In lockstep that holds anyway; so that it is also SAID, the wave meets once more in front of the store -- the
// `const u64 met = __ballot(1); if (lane == 0 && met) { ... }` that stands spelled out at each planner's end (a record that was not
// searched has met nowhere else).  No other wave touches the record's entries.
//
// Portable subset only (__ballot, __shfl*, __popcll, vector atomics): tests/emu builds this file unchanged.
#pragma once
#include "k_common.h"

// the caller's arrays by value (the pointers of dsrcgpu_columns_in)
struct ColIn
{
	const u8* bases; const u8* quals; const u8* titles;
	const u64* seq_offs; const u64* title_offs;
	u64 n_recs, bases_len, titles_len;
	u32 plus_rep, qoff;
};
// a plan in, by value: per record a range of d_bases and a keep flag.  begin and end go together; null: whole reads, every record
struct ColPlanIn { const u64* begin; const u64* end; const u8* keep; };

// the error word is (record << 4) | reason, COLE_NONE when clean: atomicMin keeps the lowest record and of that record the lowest
// reason.  COLE_*: the arrays themselves (k_columns_enc.h); COLS_*: a range against its record.  col_input_error has the wordings.
enum { COLE_SEQ_ORDER = 0, COLE_SEQ_END, COLE_TITLE_ORDER, COLE_TITLE_END, COLE_TITLE_EMPTY, COLE_TITLE_AT, COLE_TITLE_NL, COLE_BASE, COLE_QUAL,
       COLS_BEGIN_LOW, COLS_END_HIGH, COLS_RANGE_ORDER };
#define COLE_NONE (~0ull)

__device__ __forceinline__ u64 col_pos(const ColIn& c, u64 r, u64 s, u64 t) { return (1 + c.plus_rep) * t + 2 * s + (5 - c.plus_rep) * r; }
__device__ __forceinline__ void col_err(u64* err, u64 r, u32 reason) { atomicMin((unsigned long long*)err, (unsigned long long)((r << 4) | reason)); }

// the check pass of every call that takes a plan, a thread per record with a grid stride: k_sel_seq_check plus the range checks of
// the select (sel_record), for kept and dropped records alike
__global__ void __launch_bounds__(WG) k_col_plan_check(ColIn c, ColPlanIn w, u64* err)
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

// ---- record r's range [b, e) of d_bases -------------------------------------------------------------------------------------
// S[r] <= b <= e <= S[r + 1] <= bases_len (the re-check, see above)
__device__ __forceinline__ bool col_range_ok(const ColIn& c, u64 s0, u64 s1, u64 b, u64 e) { return !(s0 > s1 || s1 > c.bases_len || b < s0 || e > s1 || b > e); }
// false: an offset or the range is out of order, and nothing of the record may be read.  The offsets are tested before the range is
// read.  (b = e = 0 with a false: nothing undefined is handed out -- k_prof<256> keeps its 64 registers only so)
__device__ __forceinline__ bool col_range(const ColIn& c, const ColPlanIn& w, u64 r, u64& b, u64& e)
{
	const u64 s0 = c.seq_offs[r], s1 = c.seq_offs[r + 1];
	b = e = 0;
	if (s0 > s1 || s1 > c.bases_len) return false;
	b = w.begin ? w.begin[r] : s0; e = w.begin ? w.end[r] : s1;
	return col_range_ok(c, s0, s1, b, e);
}
// ... with the record's incoming flag, for the planners, which need it whatever it says (they write a record that came in dropped
// as well).  keep_in is handed out, not acted on; it is read in front of the offsets' test (keep holds an entry per record, so
// the address is good whatever the offsets are).  A kernel that only skips dropped records reads the flag itself behind the
// re-check, as it always did.
__device__ __forceinline__ bool col_range(const ColIn& c, const ColPlanIn& w, u64 r, u64& b, u64& e, bool& keep_in)
{
	keep_in = w.keep ? w.keep[r] != 0 : true;
	return col_range(c, w, r, b, e);
}
// the same in two halves for the kernels that read two column sets, which issue every load of the pair's figures before the first
// test (the arrays hold an entry per record, so the addresses are good whatever the entries are, and the wave waits for memory
// once instead of four times in a row): the offsets of either side by hand, col_range_load per side (the range; a flag the
// kernel reads itself), then col_range_ok per side
__device__ __forceinline__ void col_range_load(const ColPlanIn& w, u64 r, u64 s0, u64 s1, u64& b, u64& e) { b = w.begin ? w.begin[r] : s0; e = w.begin ? w.end[r] : s1; }

// ---- bit planes -------------------------------------------------------------------------------------------------------------
// 64 positions of the range x[0 .. n) from `base` on as three wave-uniform bit planes: bit 0 of the code, bit 1 of the code, code >= 4.
// A lane per position, each byte loaded once; positions at or beyond n give 0 in every plane.  from_end: position j is x[n - 1 - j],
// the range read from its far end inwards.  -> this lane's code (0 beyond n).
__device__ __forceinline__ u32 col_planes(const u8* x, u64 n, u64 base, bool from_end, u64& p0, u64& p1, u64& pn)
{
	const u64 j = base + lane_id();
	const bool valid = j < n;
	const u32 code = valid ? x[from_end ? n - 1 - j : j] : 0u;
	p0 = __ballot(valid && (code & 1u));
	p1 = __ballot(valid && (code & 2u));
	pn = __ballot(valid && code >= 4u);
	return code;
}
__device__ __forceinline__ void col_planes(const u8* x, u64 n, u64 base, u64& p0, u64& p1, u64& pn) { col_planes(x, n, base, false, p0, p1, pn); }

// 64 positions from bit `sh` (0 .. 63) of the tile pair (cur, nxt)
__device__ __forceinline__ u64 col_funnel(u64 cur, u64 nxt, u32 sh) { return sh ? (cur >> sh) | (nxt << (64u - sh)) : cur; }

// ---- the wave in 64 bits ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 wave_incl_scan64(u64 v)
{
	const u32 l = lane_id();
	for (u32 d = 1; d < 64; d <<= 1)
	{
		const u64 t = (u64)__shfl_up((unsigned long long)v, d);
		if (l >= d) v += t;
	}
	return v;
}
__device__ __forceinline__ u64 wave_sum64(u64 v)
{
	for (u32 d = 32; d >= 1; d >>= 1) v += (u64)__shfl_xor((unsigned long long)v, (int)d);
	return v;
}
__device__ __forceinline__ u64 wave_max64(u64 v)
{
	for (u32 d = 32; d >= 1; d >>= 1) { const u64 o = (u64)__shfl_xor((unsigned long long)v, (int)d); v = v > o ? v : o; }
	return v;
}

// lane k adds up statistic k: the wave's end
__device__ __forceinline__ void col_stats_flush(u64* stats, u32 n_stats, u64 sum)
{
	const u32 lane = lane_id();
	if (lane < n_stats && sum) atomicAdd((unsigned long long*)&stats[lane], (unsigned long long)sum);
}
