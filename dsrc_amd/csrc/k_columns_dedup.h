// Columnar dedup plan: the fourth planner, and the first columnar call whose records talk to each other -- exact duplicate reads (or
// pairs) are marked through a device-wide hash table (include/dsrc_gpu.h: dsrcgpu_columns_dedup_plan has the rule as a serial loop).
// The key of a record is (k_1, its first k_1 bases of the range) and, with two column sets, (k_2, the mate's first k_2 bases); of
// the considered records with one key exactly one is kept, its class's member of highest rank.  The caller's input arrays are only
// read.  No counterpart in the reference.
//
// Three launches behind k_col_plan_check of either side; each does nothing unless both error words are clean.
//   k_dedup_key      a wave per record: hash[r] and rank[r] into the arena
//   k_dedup_insert   a wave per record: an open-addressed table of M = 2^m >= 2 * n_records slots, linear probing
//   k_dedup_resolve  a lane per record: d_keep, d_dup_of, d_copies and the statistics
//
// The table.  A slot is four words in four arrays: occ (u32: the record that claimed the slot, DEDUP_EMPTY = all ones), best (u64:
// the highest rank word among the slot's class), count (u32: the class size) and, under prefer = 1 only, low (u32: the lowest index
// of the class).  The host fills occ and low with 0xFF and best and count with 0 in front of the launches.  Correctness rests on two
// facts:
//   1. An occupant never changes once set: the only write to occ[] is atomicCAS(occ, DEDUP_EMPTY, r).
//   2. A key is compared only against caller input and against hash[] from the EARLIER launch -- nothing a wave decides depends on
//      memory another wave of the same launch writes, except through the value an atomic returns.
// A record walks from hash & (M - 1) and stops at the first slot that it claims or whose occupant has its key.  Slots in front of that
// one are held by other keys for good (1), so every member of a class walks past the same slots and stops at the same one, whatever
// the arrival order: the first member to arrive there claims it, the others find it.  best, count and low are atomicMax / atomicAdd /
// atomicMin of integers, whose results do not depend on the order either, and they are read in the NEXT launch only.  No lane ever
// waits for another wave: no lock, no spin on a flag, no retry; the one loop is a probe that advances a slot a step and ends after M
// steps at the latest (at most n_records <= M / 2 slots are ever claimed, so it ends earlier).  All atomics are 32- or 64-bit vector
// atomics at device scope; nothing needs a fence inside a launch.
//
// Portable subset only (__ballot, __shfl*, __popcll, vector atomics): tests/emu builds this file unchanged.
#pragma once
#include "k_common.h"
#include "k_columns_common.h"

#define DEDUP_EMPTY 0xFFFFFFFFu
#define DEDUP_NOT_CONSIDERED (~0ull)
enum { DEDUP_CONSIDERED = 0, DEDUP_KEPT, DEDUP_DROPPED, DEDUP_MULTI, DEDUP_LARGEST, DEDUP_CAME_DROPPED, DEDUP_EMPTY_KEY, DEDUP_NOT_FIRST, DEDUP_HIST,
       DEDUP_N_STATS = DEDUP_HIST + 16 };

// what the three kernels read, by value.  w<s>.keep is not used: ONE incoming flag covers both sides.  two = 0: c2 / w2 are not read.
struct DedupIn
{
	ColIn c1, c2;
	ColPlanIn w1, w2;
	const u8* keep;
	u64 key_bases, hash_mask;
	u32 two, prefer;
};
struct DedupTable { u32* occ; u64* best; u32* count; u32* low; u64 mask; };       // mask = M - 1

// the key range of record r on one side: x = c.bases + b, k bases.  false: offsets or range out of order (col_range)
__device__ __forceinline__ bool dedup_range(const ColIn& c, const ColPlanIn& w, u64 r, u64 key_bases, u64& b, u64& k)
{
	u64 e;
	if (!col_range(c, w, r, b, e)) return false;
	const u64 n = e - b;
	k = key_bases && n > key_bases ? key_bases : n;
	return true;
}

// splitmix64's finaliser
__device__ __forceinline__ u64 dedup_mix(u64 x)
{
	x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
	x ^= x >> 27; x *= 0x94D049BB133111EBull;
	return x ^ (x >> 31);
}

// what byte v at position i of side `seed` adds to the hash: position-dependent, and the terms are SUMMED, so the lanes may take the
// positions in any grouping and the wave's sum is that of the serial loop
__device__ __forceinline__ u64 dedup_term(u64 seed, u64 i, u32 v) { return dedup_mix(((i << 8) | v) * 0x9E3779B97F4A7C15ull + seed); }

// this lane's share of a fold over p[0 .. k): HASH: the sum of dedup_term, else the sum of the bytes.  The bytes in front of the first
// 16-byte boundary (lanes 0 .. 14) and behind the last one (lanes 0 .. 14 again) go a byte per lane, what lies between 16 bytes per
// lane and step.  Nothing outside p[0 .. k) is read.
template <bool HASH> __device__ __forceinline__ u64 dedup_fold(const u8* p, u64 k, u64 seed)
{
	const u32 lane = lane_id();
	const u64 to_boundary = (16u - ((u64)p & 15u)) & 15u;
	const u64 head = k < to_boundary ? k : to_boundary;
	const u64 n_body = (k - head) >> 4;
	const u64 tail = head + (n_body << 4);
	u64 acc = 0;
	if (lane < head) acc += HASH ? dedup_term(seed, lane, p[lane]) : (u64)p[lane];
	for (u64 c = lane; c < n_body; c += 64)
	{
		const u64 at = head + (c << 4);
		const uint4 w = *(const uint4*)(p + at);
		// four bytes at a time: all sixteen terms in flight at once cost more registers than a workgroup of 1024 has per lane
		u32 word = w.x;
#pragma unroll 1
		for (u32 k4 = 0; k4 < 16; k4 += 4)
		{
#pragma unroll
			for (u32 j = 0; j < 4; ++j)
			{
				const u32 v = (word >> (8u * j)) & 255u;
				acc += HASH ? dedup_term(seed, at + k4 + j, v) : (u64)v;
			}
			word = k4 == 0 ? w.y : k4 == 4 ? w.z : w.w;
		}
	}
	if (tail + lane < k) acc += HASH ? dedup_term(seed, tail + lane, p[tail + lane]) : (u64)p[tail + lane];
	return acc;
}

#define DEDUP_SEED_1 0x243F6A8885A308D3ull
#define DEDUP_SEED_2 0x13198A2E03707344ull

// grid (gx), a wave per record with a grid stride.  A considered record gets hash[r] (the sum of the terms of its key bytes, the two
// lengths mixed in, cut to the rules' hash_bits) and rank[r] = q << 32 | (0xFFFFFFFF - r), q = 0 or the clamped sum of the qualities at
// the key positions: a larger word is a higher rank, and no rank word is 0 (r < 2^31).  A record that came in dropped gets no entry.
// Lane DEDUP_EMPTY_KEY counts the considered records whose key holds no base.
__global__ void __launch_bounds__(WG) k_dedup_key(DedupIn in, u64* hash, u64* rank, u64* stats, const u64* err)
{
	if (err[0] != COLE_NONE || err[1] != COLE_NONE) return;
	const u32 lane = lane_id();
	const u64 wpg = blockDim.x >> 6;
	u64 empty = 0;
	for (u64 r = blockIdx.x * wpg + wave_id(); r < in.c1.n_recs; r += gridDim.x * wpg)
	{
		if (in.keep && !in.keep[r]) continue;
		u64 b1 = 0, k1 = 0, b2 = 0, k2 = 0;
		if (!dedup_range(in.c1, in.w1, r, in.key_bases, b1, k1)) continue;
		if (in.two && !dedup_range(in.c2, in.w2, r, in.key_bases, b2, k2)) continue;
		u64 hs = dedup_fold<true>(in.c1.bases + b1, k1, DEDUP_SEED_1);
		if (in.two) hs += dedup_fold<true>(in.c2.bases + b2, k2, DEDUP_SEED_2);
		u64 q = 0;
		if (in.prefer)
		{
			q = dedup_fold<false>(in.c1.quals + b1, k1, 0);
			if (in.two) q += dedup_fold<false>(in.c2.quals + b2, k2, 0);
			q = wave_sum64(q);
			if (q > 0xFFFFFFFFull) q = 0xFFFFFFFFull;
		}
		hs = wave_sum64(hs);
		if (lane == 0)
		{
			hash[r] = dedup_mix(hs + dedup_mix(k1 + DEDUP_SEED_1) + dedup_mix(k2 + DEDUP_SEED_2)) & in.hash_mask;
			rank[r] = (q << 32) | (u64)(0xFFFFFFFFu - (u32)r);
		}
		if (k1 + k2 == 0) ++empty;
	}
	if (lane == DEDUP_EMPTY_KEY && empty) atomicAdd((unsigned long long*)&stats[DEDUP_EMPTY_KEY], (unsigned long long)empty);
}

// this lane's share of the comparison of p[0 .. k) with o[0 .. k): true = a difference seen
__device__ __forceinline__ bool dedup_differ(const u8* p, const u8* o, u64 k)
{
	bool diff = false;
	for (u64 i = lane_id(); i < k; i += 64) diff |= p[i] != o[i];
	return diff;
}

// grid (gx), a wave per record with a grid stride, behind k_dedup_key (see the head of this file for why the arrival order changes
// nothing).  The probe is wave-uniform: lane 0 issues the atomic, its result is broadcast.  At an occupied slot hash[o] is compared
// first, then the lengths, then the wave compares the bytes and a ballot decides.  At its final slot the record raises best, counts
// itself and, under prefer = 1, lowers low; slot[r] keeps the slot for k_dedup_resolve.
__global__ void __launch_bounds__(WG) k_dedup_insert(DedupIn in, const u64* hash, const u64* rank, DedupTable t, u32* slot, const u64* err)
{
	if (err[0] != COLE_NONE || err[1] != COLE_NONE) return;
	const u32 lane = lane_id();
	const u64 wpg = blockDim.x >> 6;
	for (u64 r = blockIdx.x * wpg + wave_id(); r < in.c1.n_recs; r += gridDim.x * wpg)
	{
		if (in.keep && !in.keep[r]) continue;
		u64 b1 = 0, k1 = 0, b2 = 0, k2 = 0;
		if (!dedup_range(in.c1, in.w1, r, in.key_bases, b1, k1)) continue;
		if (in.two && !dedup_range(in.c2, in.w2, r, in.key_bases, b2, k2)) continue;
		const u64 h = hash[r];
		u64 at = h & t.mask;
		bool placed = false;
		for (u64 step = 0; step <= t.mask; ++step, at = (at + 1) & t.mask)
		{
			u32 o = 0;
			if (lane == 0) o = atomicCAS((unsigned int*)&t.occ[at], (unsigned int)DEDUP_EMPTY, (unsigned int)r);
			o = __shfl(o, 0);
			if (o == DEDUP_EMPTY) { placed = true; break; }      // claimed
			if (hash[o] != h) continue;
			u64 ob1 = 0, ok1 = 0, ob2 = 0, ok2 = 0;
			if (!dedup_range(in.c1, in.w1, o, in.key_bases, ob1, ok1)) continue;
			if (in.two && !dedup_range(in.c2, in.w2, o, in.key_bases, ob2, ok2)) continue;
			if (ok1 != k1 || ok2 != k2) continue;
			bool diff = dedup_differ(in.c1.bases + b1, in.c1.bases + ob1, k1);
			if (in.two) diff |= dedup_differ(in.c2.bases + b2, in.c2.bases + ob2, k2);
			if (__ballot(diff) == 0) { placed = true; break; }   // the occupant has this record's key
		}
		if (placed && lane == 0)
		{
			atomicMax((unsigned long long*)&t.best[at], (unsigned long long)rank[r]);
			atomicAdd((unsigned int*)&t.count[at], 1u);
			if (in.prefer) atomicMin((unsigned int*)&t.low[at], (unsigned int)r);
			slot[r] = (u32)at;
		}
	}
}

// the bin of a class of n >= 1 members in the duplication-level histogram: 1, 2, .., 9, 10-49, 50-99, 100-499, 500-999, 1000-4999,
// 5000-9999, >= 10000
__device__ __forceinline__ u32 dedup_bin(u32 n)
{
	return n < 10u ? n - 1u : n < 50u ? 9u : n < 100u ? 10u : n < 500u ? 11u : n < 1000u ? 12u : n < 5000u ? 13u : n < 10000u ? 14u : 15u;
}

// grid (gx), a lane per record with a grid stride of whole workgroups (every lane of a wave takes part in every ballot).  A record
// reads its incoming flag before it writes d_keep[r], and no other record's is touched: d_keep may be the incoming array.  The
// representative of a class is the record whose index the slot's best rank word holds; the class is counted there, once.  Lane k
// adds up statistic k from the ballots in a register, one vector atomic per lane and wave at the end if it is not 0 (DEDUP_LARGEST: a
// maximum).  All integer: the order of the waves cannot change a bit of the result.
__global__ void __launch_bounds__(WG) k_dedup_resolve(const u8* keep_in, u64 n_recs, DedupTable t, const u32* slot, u32 prefer, u8* keep, u64* dup_of, u64* copies,
                                                      u64* stats, const u64* err)
{
	if (err[0] != COLE_NONE || err[1] != COLE_NONE) return;
	const u32 lane = lane_id();
	u64 sum = 0;
	for (u64 base = (u64)blockIdx.x * blockDim.x; base < n_recs; base += (u64)gridDim.x * blockDim.x)
	{
		const u64 r = base + threadIdx.x;
		const bool valid = r < n_recs;
		const bool considered = valid && (keep_in ? keep_in[r] != 0 : true);
		u64 rep = DEDUP_NOT_CONSIDERED;
		u32 n = 0;
		bool not_first = false;
		if (considered)
		{
			const u64 at = slot[r] & t.mask;                 // (every considered record has been placed; the mask keeps any word inside the table)
			rep = (u64)(0xFFFFFFFFu - (u32)t.best[at]);
			if (rep == r)
			{
				n = t.count[at];
				not_first = prefer && t.low[at] != (u32)r;
			}
		}
		const bool is_rep = considered && rep == r;
		if (valid)
		{
			keep[r] = is_rep ? 1 : 0;
			if (dup_of) dup_of[r] = rep;
			if (copies) copies[r] = n;
		}
		const u32 bin = is_rep ? dedup_bin(n) : 0xFFFFFFFFu;
		const u64 b_cons = __ballot(considered), b_rep = __ballot(is_rep), b_multi = __ballot(is_rep && n >= 2u), b_in = __ballot(valid && !considered),
		          b_nf = __ballot(not_first);
		u64 mine = lane == DEDUP_CONSIDERED ? (u64)__popcll(b_cons) : lane == DEDUP_KEPT ? (u64)__popcll(b_rep) : lane == DEDUP_DROPPED ? (u64)__popcll(b_cons & ~b_rep)
		         : lane == DEDUP_MULTI ? (u64)__popcll(b_multi) : lane == DEDUP_CAME_DROPPED ? (u64)__popcll(b_in) : lane == DEDUP_NOT_FIRST ? (u64)__popcll(b_nf) : 0ull;
#pragma unroll
		for (u32 k = 0; k < 16; ++k)
		{
			const u64 b_bin = __ballot(bin == k);
			if (lane == DEDUP_HIST + k) mine = (u64)__popcll(b_bin);
		}
		const u32 largest = wave_max(n);
		if (lane == DEDUP_LARGEST) sum = sum > largest ? sum : (u64)largest; else sum += mine;
	}
	if (lane < DEDUP_N_STATS && lane != DEDUP_EMPTY_KEY && sum)
	{
		if (lane == DEDUP_LARGEST) atomicMax((unsigned long long*)&stats[lane], (unsigned long long)sum);
		else atomicAdd((unsigned long long*)&stats[lane], (unsigned long long)sum);
	}
}
