// Columnar k-mer count: every window of k bases of every considered record's range is a key of a device-wide open-addressed table
// that the CALLER owns and that lives across calls (include/dsrc_gpu.h: dsrcgpu_columns_kmer_count has the rule as a serial loop and
// the table's layout).  The second user of what the dedup plan built (k_columns_dedup.h) -- but dedup keys a record, this keys
// every window of a record: two orders of magnitude more inserts, nearly all of them hits on a key that is already there.  The
// caller's input arrays are only read.  No counterpart in the reference.
//
//   k_kmer_windows   a lane per record, behind k_col_plan_check: W (the windows of the call) and the three record statistics
//   k_kmer_count     a wave per record, 64 windows a step: the table is filled
//   k_kmer_header    one lane: the table's header is brought up to date, distinct / total come home with the statistics
//   k_kmer_merge     a lane per slot of a source table: every (key, count) is added into another table
//   k_kmer_spectrum  a lane per slot: the histogram of the counts
//   k_kmer_lookup    a lane per query
//
// The table.  keys[M] (KMER_EMPTY = all ones; k <= 31 leaves that word free) and counts[M], M a power of two, linear probing from
// mix(key) & (M - 1), at most `limit` slots a walk.  Correctness rests on three facts:
//   1. A key word changes ONCE, from KMER_EMPTY to a key, and only by atomicCAS(keys + at, KMER_EMPTY, key).  A word that is not
//      KMER_EMPTY is final.  Slots are never freed.
//   2. A walk reads keys[at] with a PLAIN load first.  A plain load may be stale, but by (1) a stale value can only still say
//      KMER_EMPTY -- and then the lane issues the CAS and acts on what the CAS RETURNS, which is the truth.  A value that is not
//      KMER_EMPTY is final whether stale or not.  So the common case, a hit on a key that is there, costs a load and one
//      non-returning add, and the returning atomic is paid once per key and race, not once per occurrence.
//   3. Nothing else a lane decides depends on memory another wave of the same launch writes: counts[] is only added to (integer
//      sums, read by LATER launches), and the statistics are sums.
// Every occurrence of a key walks the same slots in the same order; the slots in front of the key's own hold other keys for good,
// so all occurrences stop at the same slot, whatever the arrival order.  PRESENT MEANS EXACT: if a walk of `limit` slots meets
// neither the key nor an empty slot, every one of them holds another key for good, so EVERY occurrence of that key, earlier or
// later, sees the same and is dropped into `overflow` -- a key is in the table with its exact count, or wholly absent.
// No lane waits for another wave: no lock, no spin, no retry; the one loop is the bounded walk.  All atomics are 64-bit vector
// atomics at device scope; nothing needs a fence inside a launch.
//
// Portable subset only (static __shared__, __syncthreads, __ballot, __shfl*, __popcll, __ffsll, vector atomics): tests/emu builds
// this file unchanged.
#pragma once
#include "k_common.h"
#include "k_columns_common.h"
#include "k_columns_dedup.h"

#define KMER_EMPTY (~0ull)
#define KMER_HEADER 8u
#define KMER_PROBE_LIMIT 1024u
#define KMER_MAGIC 0x4B4D4552ull                           // "KMER", the upper half of header word 0
#define KMER_SPEC_LDS 256u                                 // bins of the spectrum a workgroup counts in LDS
enum { KMER_CONSIDERED = 0, KMER_CAME_DROPPED, KMER_SHORT, KMER_WINDOWS, KMER_COUNTED, KMER_BROKEN, KMER_NEW, KMER_OVERFLOW, KMER_DISTINCT_AFTER,
       KMER_TOTAL_AFTER, KMER_N_STATS = 16 };
enum { KMERGE_KEYS = 0, KMERGE_NEW, KMERGE_ADDED, KMERGE_OVERFLOW, KMERGE_DISTINCT_AFTER, KMERGE_TOTAL_AFTER, KMERGE_N_STATS = 8 };
enum { KSPEC_DISTINCT = 0, KSPEC_TOTAL, KSPEC_SINGLE, KSPEC_LARGEST, KSPEC_N_TOTALS };

__host__ __device__ __forceinline__ u64 kmer_header_word(u32 k, u32 canonical, u32 hash_bits)
{
	return (KMER_MAGIC << 32) | ((u64)(hash_bits & 63u) << 16) | ((u64)k << 8) | (u64)canonical;      // (hash_bits 64 is stored as 0: the full hash)
}

// by value: the table behind its header.  mask = M - 1; hash_mask cuts the hash to the table's hash_bits; limit = min(M, KMER_PROBE_LIMIT)
struct KmerTab { u64* keys; u64* counts; u64 mask, hash_mask; u32 limit; };

// bit j of v to bit 2j
__device__ __forceinline__ u64 kmer_spread(u32 v)
{
	u64 x = v;
	x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
	x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
	x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
	x = (x | (x << 2)) & 0x3333333333333333ull;
	return (x | (x << 1)) & 0x5555555555555555ull;
}
__device__ __forceinline__ u32 kmer_rev32(u32 v)
{
	v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
	v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
	v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
	v = ((v >> 8) & 0x00FF00FFu) | ((v & 0x00FF00FFu) << 8);
	return (v >> 16) | (v << 16);
}
// the k two-bit groups of m (group j at bits 2j, 2j + 1) in reverse order: all 64 bits are reversed, the two bits of every group are
// put back in their order, and the 32 - k empty groups are shifted out
__device__ __forceinline__ u64 kmer_group_reverse(u64 m, u32 k)
{
	u64 r = ((u64)kmer_rev32((u32)m) << 32) | (u64)kmer_rev32((u32)(m >> 32));
	r = ((r >> 1) & 0x5555555555555555ull) | ((r & 0x5555555555555555ull) << 1);
	return r >> (64u - 2u * k);
}
// m holds the k bases with the FIRST base in the LOWEST group.  The forward word has the first base most significant: the groups
// reversed.  The reverse complement reverses the order once more and takes 3 - code: ~m under the mask of 2k bits.
__device__ __forceinline__ u64 kmer_key(u64 m, u32 k, u32 canonical)
{
	const u64 fwd = kmer_group_reverse(m, k);
	const u64 rc = ~m & ((1ull << (2u * k)) - 1ull);
	return canonical && rc < fwd ? rc : fwd;
}

// one walk: `add` occurrences of `key`.  true: counted (is_new: this lane's CAS claimed the slot); false: `limit` slots, all of other
// keys -- the occurrences are dropped.  See the head of this file for why the plain load is sound.  PLAIN = false (a measuring
// variant, tools/columns_kmer_bench.py) goes to the CAS at every slot without looking first.
template <bool PLAIN = true> __device__ __forceinline__ bool kmer_insert(const KmerTab& t, u64 key, u64 add, bool& is_new)
{
	u64 at = dedup_mix(key) & t.hash_mask & t.mask;
	is_new = false;
	for (u32 step = 0; step < t.limit; ++step, at = (at + 1) & t.mask)
	{
		u64 cur = PLAIN ? t.keys[at] : KMER_EMPTY;
		if (cur == KMER_EMPTY)
		{
			cur = (u64)atomicCAS((unsigned long long*)&t.keys[at], (unsigned long long)KMER_EMPTY, (unsigned long long)key);
			if (cur == KMER_EMPTY) { is_new = true; cur = key; }
		}
		if (cur == key)
		{
			atomicAdd((unsigned long long*)&t.counts[at], (unsigned long long)add);
			return true;
		}
	}
	return false;
}

// read only: the count of `key`, 0 when the walk ends at an empty slot or after `limit` slots
__device__ __forceinline__ u64 kmer_find(const KmerTab& t, u64 key)
{
	u64 at = dedup_mix(key) & t.hash_mask & t.mask;
	for (u32 step = 0; step < t.limit; ++step, at = (at + 1) & t.mask)
	{
		const u64 cur = t.keys[at];
		if (cur == key) return t.counts[at];
		if (cur == KMER_EMPTY) return 0;
	}
	return 0;
}

// ---- the window step ---------------------------------------------------------------------------------------------------------
// What k_kmer_plan and k_kmer_correct do per 64 windows (k_kmer_count does the same and keeps its own text, see there).  The wave
// holds 128 positions of the range as three wave-uniform bit planes each (col_planes): the step's own 64 (c0, c1, cn) and the 64
// behind them (n0, n1, nn), which the next step takes over as its own, so every byte of the range is loaded once.  Lane i has the
// window that starts at position base + i: it cuts 64 positions out of the planes (col_funnel) and no lane reads k bytes of its own
// from HBM.  valid: the window exists; good: and holds no code above 3; key: kmer_key of its k bases (of no meaning unless good).  A
// lane whose key equals the key of the good lane in front of it is not a head (head): equal neighbouring keys form a run, and only
// its head walks the table.  b_valid, b_good, b_head: the ballots of the three.
struct KmerStep { u64 key; bool valid, good, head; u64 b_valid, b_good, b_head; };

__device__ __forceinline__ KmerStep kmer_step(u64 c0, u64 c1, u64 cn, u64 n0, u64 n1, u64 nn, u64 base, u64 n_win, u32 k, u64 kmask, u32 canonical)
{
	const u32 lane = lane_id();
	KmerStep s;
	const u64 w0 = col_funnel(c0, n0, lane), w1 = col_funnel(c1, n1, lane), wn = col_funnel(cn, nn, lane);
	s.valid = base + lane < n_win;
	s.good = s.valid && (wn & kmask) == 0;
	const u64 m = kmer_spread((u32)(w0 & kmask)) | (kmer_spread((u32)(w1 & kmask)) << 1);
	s.key = kmer_key(m, k, canonical);
	const u64 prev = __shfl_up(s.key, 1);
	s.b_valid = __ballot(s.valid); s.b_good = __ballot(s.good);
	s.head = s.good && (lane == 0 || !((s.b_good >> (lane - 1u)) & 1ull) || prev != s.key);
	s.b_head = __ballot(s.head);
	return s;
}

// the count of every lane's key from a table that is only read: one kmer_find per head, and every lane takes the count of the head
// of its run -- the highest head at or below the lane (a lane that is not good takes what it gets; its caller drops it)
__device__ __forceinline__ u64 kmer_step_counts(const KmerTab& t, const KmerStep& s)
{
	const u32 lane = lane_id();
	const u64 cnt = s.head ? kmer_find(t, s.key) : 0ull;
	const u64 below = s.b_head & (lane == 63u ? ~0ull : (2ull << lane) - 1ull);
	const int src = below ? 63 - __clzll((long long)below) : (int)lane;
	return __shfl(cnt, src);
}

// grid (gx), a lane per record with a grid stride, behind k_col_plan_check.  stats[KMER_CONSIDERED .. KMER_WINDOWS]: lane s of a wave
// adds the wave's sum of statistic s.
__global__ void __launch_bounds__(WG) k_kmer_windows(ColIn c, ColPlanIn w, u32 k, u64* stats, const u64* err)
{
	if (*err != COLE_NONE) return;
	u64 cons = 0, dropped = 0, shrt = 0, win = 0;
	for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < c.n_recs; r += (u64)gridDim.x * blockDim.x)
	{
		u64 b, e;
		if (!col_range(c, w, r, b, e)) continue;
		if (w.keep && w.keep[r] == 0) { ++dropped; continue; }
		++cons;
		const u64 n = e - b;
		if (n < k) ++shrt; else win += n - k + 1;
	}
	cons = wave_sum64(cons); dropped = wave_sum64(dropped); shrt = wave_sum64(shrt); win = wave_sum64(win);
	const u32 lane = lane_id();
	const u64 mine = lane == KMER_CONSIDERED ? cons : lane == KMER_CAME_DROPPED ? dropped : lane == KMER_SHORT ? shrt : lane == KMER_WINDOWS ? win : 0ull;
	if (mine) atomicAdd((unsigned long long*)&stats[lane], (unsigned long long)mine);
}

// grid (gx), a wave per record with a grid stride, 64 windows a step.  The step is kmer_step's, spelled out here with the funnel in
// its earlier form: with the shared text the kernel was shorter, and one leg of its timing lay above what the parent's runs allow.
// Run aggregation: a head adds the length of its run (up to the next head or broken window, from two ballots) in ONE walk.  A
// homopolymer costs one atomic per step, not 64 on one word.
// Statistics: broken windows from ballots, counted / new / overflow per lane in registers; one wave sum each and one vector atomic
// per statistic and wave at the end.  Integer sums: the order of the waves changes no bit of the table's content or the statistics.
// AGG = false (every good window is a head of a run of one) and PLAIN = false are the measuring variants of a build with test hooks;
// they give the same table.
template <bool AGG, bool PLAIN>
__global__ void __launch_bounds__(WG) k_kmer_count(ColIn c, ColPlanIn w, u32 k, u32 canonical, KmerTab t, u64* stats, const u64* err)
{
	if (*err != COLE_NONE) return;
	const u32 lane = lane_id();
	const u64 wpg = blockDim.x >> 6;
	const u64 kmask = (1ull << k) - 1ull;
	u64 s_counted = 0, s_new = 0, s_over = 0, s_broken = 0;
	for (u64 r = blockIdx.x * wpg + wave_id(); r < c.n_recs; r += gridDim.x * wpg)
	{
		const u64 s0 = c.seq_offs[r], s1 = c.seq_offs[r + 1];
		if (s0 > s1 || s1 > c.bases_len) continue;
		const u64 b = w.begin ? w.begin[r] : s0, e = w.begin ? w.end[r] : s1;
		if (b < s0 || e > s1 || b > e) continue;
		if (w.keep && w.keep[r] == 0) continue;
		const u64 n = e - b;
		if (n < k) continue;
		const u64 n_win = n - k + 1;
		const u8* const x = c.bases + b;
		u64 c0, c1, cn;
		col_planes(x, n, 0, c0, c1, cn);
		for (u64 base = 0; base < n_win; base += 64)
		{
			u64 n0 = 0, n1 = 0, nn = 0;
			if (base + 64 < n) col_planes(x, n, base + 64, n0, n1, nn);
			// 64 positions from base + lane on (lane 0 takes the planes as they are: a shift by 64 is not a shift by 0)
			const u64 w0 = lane ? (c0 >> lane) | (n0 << (64u - lane)) : c0;
			const u64 w1 = lane ? (c1 >> lane) | (n1 << (64u - lane)) : c1;
			const u64 wn = lane ? (cn >> lane) | (nn << (64u - lane)) : cn;
			const bool valid = base + lane < n_win;
			const bool good = valid && (wn & kmask) == 0;
			s_broken += (u64)__popcll(__ballot(valid && !good));
			const u64 m = kmer_spread((u32)(w0 & kmask)) | (kmer_spread((u32)(w1 & kmask)) << 1);
			const u64 key = kmer_key(m, k, canonical);
			const u64 prev = __shfl_up(key, 1);
			const u64 b_good = __ballot(good);
			const bool head = good && (!AGG || lane == 0 || !((b_good >> (lane - 1u)) & 1ull) || prev != key);
			const u64 b_head = __ballot(head);
			if (head)
			{
				// the run ends in front of the next head or the next window that is not good
				const u64 above = lane == 63u ? 0ull : (b_head | ~b_good) & ~((2ull << lane) - 1ull);
				const u64 run = (above ? (u64)__ffsll((long long)above) - 1ull : 64ull) - lane;
				bool is_new;
				if (kmer_insert<PLAIN>(t, key, run, is_new)) { s_counted += run; s_new += is_new ? 1u : 0u; }
				else s_over += run;
			}
			c0 = n0; c1 = n1; cn = nn;
		}
	}
	s_counted = wave_sum64(s_counted); s_new = wave_sum64(s_new); s_over = wave_sum64(s_over);
	const u64 mine = lane == KMER_COUNTED ? s_counted : lane == KMER_BROKEN ? s_broken : lane == KMER_NEW ? s_new : lane == KMER_OVERFLOW ? s_over : 0ull;
	if (mine) atomicAdd((unsigned long long*)&stats[lane], (unsigned long long)mine);
}

// one lane, behind k_kmer_count or k_kmer_merge: distinct += n_new, total += added, overflow += over (and what the source table of a
// merge had lost itself); the two figures "after" go home with the statistics
__global__ void k_kmer_header(u64* header, const u64* n_new, const u64* added, const u64* over, u64 more_over, u64* distinct_after, u64* total_after, const u64* err)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	if (err && *err != COLE_NONE) return;
	header[2] += *n_new; header[3] += *added; header[4] += *over + more_over;
	*distinct_after = header[2]; *total_after = header[3];
}

// grid (gx), a lane per slot of the source table with a grid stride of whole workgroups
__global__ void __launch_bounds__(WG) k_kmer_merge(const u64* src_keys, const u64* src_counts, u64 src_slots, KmerTab t, u64* stats)
{
	u64 s_keys = 0, s_new = 0, s_added = 0, s_over = 0;
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < src_slots; i += (u64)gridDim.x * blockDim.x)
	{
		const u64 key = src_keys[i];
		if (key == KMER_EMPTY) continue;
		const u64 n = src_counts[i];
		++s_keys;
		bool is_new;
		if (kmer_insert(t, key, n, is_new)) { s_added += n; s_new += is_new ? 1u : 0u; }
		else s_over += n;
	}
	s_keys = wave_sum64(s_keys); s_new = wave_sum64(s_new); s_added = wave_sum64(s_added); s_over = wave_sum64(s_over);
	const u32 lane = lane_id();
	const u64 mine = lane == KMERGE_KEYS ? s_keys : lane == KMERGE_NEW ? s_new : lane == KMERGE_ADDED ? s_added : lane == KMERGE_OVERFLOW ? s_over : 0ull;
	if (mine) atomicAdd((unsigned long long*)&stats[lane], (unsigned long long)mine);
}

// grid (gx), a lane per slot with a grid stride.  hist[min(count, n_bins - 1)] += 1 for every occupied slot with a count (a slot
// holds a key only together with at least one occurrence once its launch has ended; a count of 0 adds nothing, so hist[0] stays 0).
// The bins below KMER_SPEC_LDS -- where nearly every key of a real spectrum falls -- are counted in LDS per workgroup and flushed
// once; the others go to HBM directly.  hist is zeroed by the host.
__global__ void __launch_bounds__(WG) k_kmer_spectrum(const u64* keys, const u64* counts, u64 slots, u32 n_bins, u64* hist, u64* totals)
{
	__shared__ u64 s_h[KMER_SPEC_LDS];
	for (u32 i = threadIdx.x; i < KMER_SPEC_LDS; i += blockDim.x) s_h[i] = 0;
	__syncthreads();
	u64 distinct = 0, total = 0, single = 0, largest = 0;
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (u64)gridDim.x * blockDim.x)
	{
		if (keys[i] == KMER_EMPTY) continue;
		const u64 n = counts[i];
		if (n == 0) continue;
		++distinct; total += n; single += n == 1 ? 1u : 0u;
		largest = largest > n ? largest : n;
		const u64 bin = n < (u64)(n_bins - 1u) ? n : (u64)(n_bins - 1u);
		if (bin < KMER_SPEC_LDS) atomicAdd((unsigned long long*)&s_h[bin], 1ull);
		else atomicAdd((unsigned long long*)&hist[bin], 1ull);
	}
	__syncthreads();
	for (u32 i = threadIdx.x; i < KMER_SPEC_LDS && i < n_bins; i += blockDim.x)
	{
		const u64 v = s_h[i];
		if (v) atomicAdd((unsigned long long*)&hist[i], (unsigned long long)v);
	}
	distinct = wave_sum64(distinct); total = wave_sum64(total); single = wave_sum64(single);
	for (u32 d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor(largest, (int)d); largest = largest > o ? largest : o; }
	const u32 lane = lane_id();
	if (lane == KSPEC_LARGEST) { if (largest) atomicMax((unsigned long long*)&totals[lane], (unsigned long long)largest); }
	else
	{
		const u64 mine = lane == KSPEC_DISTINCT ? distinct : lane == KSPEC_TOTAL ? total : lane == KSPEC_SINGLE ? single : 0ull;
		if (mine) atomicAdd((unsigned long long*)&totals[lane], (unsigned long long)mine);
	}
}

// grid (gx), a lane per query with a grid stride.  A query is a packed forward word (first base most significant); a word of 4^k
// and more gets 0 and counts in *invalid.  Under a canonical table the lower of the word and its reverse complement is looked up.
__global__ void __launch_bounds__(WG) k_kmer_lookup(KmerTab t, u32 k, u32 canonical, const u64* kmers, u64 n, u64* out, u64* invalid)
{
	u64 bad = 0;
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
	{
		const u64 q = kmers[i];
		if (q >> (2u * k)) { out[i] = 0; ++bad; continue; }
		const u64 key = kmer_key(kmer_group_reverse(q, k), k, canonical);
		out[i] = kmer_find(t, key);
	}
	bad = wave_sum64(bad);
	if (lane_id() == 0 && bad) atomicAdd((unsigned long long*)invalid, (unsigned long long)bad);
}
