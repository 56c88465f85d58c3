// Columnar complexity plan: the sixth planner -- poly-X runs cut off either end of the range, then a complexity filter (fastp's share
// of positions that differ from their successor) and a windowed DUST score on what is left (include/dsrc_gpu.h:
// dsrcgpu_columns_complexity_plan, where the rule stands as a serial loop).  Plan in, plan out, as k_adapt_plan; the check pass is
// k_col_plan_check.  The caller's input arrays are only read.  No counterpart in the reference.
//
// Portable subset only (__ballot, __shfl*, __popcll, __ffsll, vector atomics): tests/emu builds this file unchanged.
#pragma once
#include "k_common.h"
#include "k_columns_common.h"

#define CPLX_NONE 255u
struct CplxRules { u32 tail, head, poly_min, poly_permille, min_len, min_cp, max_dust, max_dust_windows; };
enum { CPLX_KEPT = 0, CPLX_BASES, CPLX_CUT5, CPLX_CUT3, CPLX_HEAD_RECS, CPLX_TAIL_RECS, CPLX_TAIL_BASE = 6, CPLX_HEAD_BASE = 10, CPLX_DROP_LEN = 14,
       CPLX_DROP_CP, CPLX_DROP_DUST, CPLX_STATS = 20 };

// The poly-X run at one end of the range x[0 .. n): its length (0: none of at least min_run positions) and its base in `which`.
// Tiles of 64 positions are taken from that end inwards; lane l of a tile judges the position at distance k = base + l from the end
// (from_end: x[n - 1 - k], else x[k]), so both ends are one loop.  The tile is the three wave-uniform planes of col_planes; for base X
// the match plane is a combination of them, and a lane's m is the carry of the tiles before plus one popcount of the plane below and at
// its lane -- no scan.  The serial rule keeps the first position that reaches the highest score among those within the error budget:
// per tile that is the highest score among the lanes that beat the running best (a wave maximum over the score's offset from the
// tile's start, -128 .. 64), the lowest such lane, and it replaces the running best only when strictly greater.  Base X is given up,
// exactly, once its score at the tile's end plus every position still ahead cannot beat its best.  Every branch is wave-uniform.
__device__ __forceinline__ u64 cplx_poly_end(const u8* x, u64 n, u32 mask, bool from_end, u32 min_run, u32 permille, u32& which)
{
	const u32 lane = lane_id();
	i64 best[4] = {0, 0, 0, 0};
	u64 run[4] = {0, 0, 0, 0}, m_in[4] = {0, 0, 0, 0};
	u32 live = mask;
	for (u64 base = 0; base < n && live; base += 64)
	{
		const u64 k = base + lane;
		const bool valid = k < n;
		const u64 in = __ballot(valid);
		u64 p0, p1, pn;
		col_planes(x, n, base, from_end, p0, p1, pn);
		const u64 upto = (2ull << lane) - 1ull;                // lanes 0 .. lane (lane 63: 2 << 63 is 0, minus 1 all ones)
		const u64 L = k + 1;
		const u64 seen = n - base > 64 ? base + 64 : n;
#pragma unroll
		for (u32 X = 0; X < 4; ++X)
			if ((live >> X) & 1u)
			{
				const u64 mx = in & ~pn & ((X & 1u) ? p0 : ~p0) & ((X & 2u) ? p1 : ~p1);
				const u32 ml = (u32)__popcll(mx & upto);
				const u64 m = m_in[X] + ml, err = L - m;
				const i64 score = (i64)m - 2 * (i64)err;
				const bool ok = valid && score > best[X] && err * 1000ull <= L * (u64)permille;
				if (__ballot(ok))
				{
					const u32 key = ok ? 3u * ml + 127u - 2u * lane : 0u;      // 129 + ml - 2 * (lane + 1 - ml): 1 .. 193
					const u32 top = wave_max(key);
					const u32 at = (u32)__ffsll((long long)__ballot(ok && key == top)) - 1u;
					best[X] = (i64)m_in[X] - 2 * (i64)(base - m_in[X]) + (i64)top - 129;
					run[X] = base + at + 1;
				}
				m_in[X] += (u32)__popcll(mx);
				const i64 at_end = (i64)m_in[X] - 2 * (i64)(seen - m_in[X]);
				if (at_end + (i64)(n - seen) <= best[X]) live &= ~(1u << X);
			}
	}
	u64 len = 0;
	which = CPLX_NONE;
#pragma unroll
	for (u32 X = 0; X < 4; ++X)
		if (((mask >> X) & 1u) && run[X] >= min_run && run[X] > len) { len = run[X]; which = X; }
	return len;
}

// DUST of one window of w <= 64 positions given as planes (bit i = position i of the window): lane t counts triplet code t -- the AND,
// over the six planes of the code's bits (bit 1 and bit 0 of the window at shifts 0, 1, 2), of the plane or its complement according
// to t's bits, under the plane of valid triplet starts -- and c_t (c_t - 1) / 2 goes through a wave sum.
__device__ __forceinline__ u32 cplx_dust(u64 w0, u64 w1, u64 wn, u32 w)
{
	if (w < 3) return 0;
	const u64 valid = ~(wn | wn >> 1 | wn >> 2) & ((1ull << (w - 2)) - 1ull);       // w - 2 <= 62
	const u32 t = lane_id();
	u64 sel = valid;
	sel &= (t & 32u) ? w1 : ~w1;
	sel &= (t & 16u) ? w0 : ~w0;
	sel &= (t & 8u) ? w1 >> 1 : ~(w1 >> 1);
	sel &= (t & 4u) ? w0 >> 1 : ~(w0 >> 1);
	sel &= (t & 2u) ? w1 >> 2 : ~(w1 >> 2);
	sel &= (t & 1u) ? w0 >> 2 : ~(w0 >> 2);
	const u32 ct = (u32)__popcll(sel);
	const u32 S = wave_sum(ct * (ct - 1u) / 2u);                 // at most 62 * 61 / 2
	const u32 l = (u32)__popcll(valid);
	return l >= 2 ? 10u * S / (l - 1u) : 0u;
}

// grid (gx), a wave per record with a grid stride, behind k_col_plan_check (k_columns_common.h: the re-check, in place, the
// statistics).  The two ends are searched on the range as it came (cplx_poly_end, only when that end's mask is set), then ONE pass
// over what is left serves both filters: a lane per position holds the code itself, the next position's code comes by shuffle (lane
// 63: lane 0 of the next tile, which is loaded one tile ahead, so each byte is loaded once), and the codes are compared as they are
// -- N equals N, 4 differs from 18.  The same tile pair gives the DUST windows at bit offsets 0 and 32 and, once per record, the
// end-aligned one at a wave-uniform shift (col_funnel).
__global__ void __launch_bounds__(WG) k_cplx_plan(ColIn c, ColPlanIn w, CplxRules R, u64* begin, u64* end, u8* keep, u32* info, u64* stats,
                                                  const u64* err)
{
	if (*err != COLE_NONE) return;
	const u32 lane = lane_id();
	const u64 wpg = blockDim.x >> 6;
	const bool want_dust = info != nullptr || R.max_dust != 0xFFFFFFFFu;
	u64 sum = 0;                                         // lane k adds up statistic k
	for (u64 r = blockIdx.x * wpg + wave_id(); r < c.n_recs; r += gridDim.x * wpg)
	{
		u64 b, e;
		bool keep_in;
		if (!col_range(c, w, r, b, e, keep_in)) continue;
		const u64 n = e - b;
		u64 ob = b, oe = e;
		bool keep_out = false;
		u32 i0 = 0xFFFFu, i1 = 0;
		if (keep_in)
		{
			const u8* const x = c.bases + b;
			u32 hb = CPLX_NONE, tb = CPLX_NONE;
			const u64 t = R.tail && n ? cplx_poly_end(x, n, R.tail, true, R.poly_min, R.poly_permille, tb) : 0;
			const u64 hd = R.head && n ? cplx_poly_end(x, n, R.head, false, R.poly_min, R.poly_permille, hb) : 0;
			if (hd + t >= n) { ob = b; oe = b; } else { ob = b + hd; oe = e - t; }
			const u64 n2 = oe - ob;
			const u8* const y = c.bases + ob;
			u64 d = 0, over = 0;
			u32 dust = 0;
			if (n2)
			{
				u64 c0, c1, cn;
				u32 cc = col_planes(y, n2, 0, false, c0, c1, cn);
				const u64 s_end = n2 >= 64 ? n2 - 64 : 0;           // the start of the end-aligned window
				for (u64 base = 0; base < n2; base += 64)
				{
					u32 nc = 0;
					u64 n0 = 0, n1 = 0, nn = 0;
					if (n2 - base > 64) nc = col_planes(y, n2, base + 64, false, n0, n1, nn);
					const u32 down = __shfl_down(cc, 1), first = __shfl(nc, 0);
					const u32 nb = lane == 63 ? first : down;
					d += (u32)__popcll(__ballot(base + lane + 1 < n2 && cc != nb));
					if (want_dust)
					{
						u32 v = 0;
						if (n2 < 64) v = cplx_dust(c0, c1, cn, (u32)n2);
						else
						{
							if (base <= s_end) v = cplx_dust(c0, c1, cn, 64);
							if (base + 32 <= s_end)
							{
								const u32 v2 = cplx_dust(col_funnel(c0, n0, 32), col_funnel(c1, n1, 32), col_funnel(cn, nn, 32), 64);
								over += v2 > R.max_dust; dust = v2 > dust ? v2 : dust;
							}
							if ((s_end & 31u) && (s_end & ~63ull) == base)
							{
								const u32 sh = (u32)(s_end & 63u);
								const u32 v3 = cplx_dust(col_funnel(c0, n0, sh), col_funnel(c1, n1, sh), col_funnel(cn, nn, sh), 64);
								over += v3 > R.max_dust; dust = v3 > dust ? v3 : dust;
							}
						}
						over += v > R.max_dust; dust = v > dust ? v : dust;
					}
					cc = nc; c0 = n0; c1 = n1; cn = nn;
				}
			}
			const u64 cp = n2 >= 2 ? d * 1000ull / (n2 - 1) : 1000ull;
			const u32 why = n2 < R.min_len ? CPLX_DROP_LEN : n2 >= 2 && d * 1000ull < (u64)R.min_cp * (n2 - 1) ? CPLX_DROP_CP
			              : over > R.max_dust_windows ? CPLX_DROP_DUST : 0u;
			keep_out = why == 0;
			i0 = hb | tb << 8; i1 = (u32)cp | dust << 16;
			const u64 mine = lane == CPLX_KEPT ? (keep_out ? 1u : 0u) : lane == CPLX_BASES ? (keep_out ? n2 : 0u) : lane == CPLX_CUT5 ? (keep_out ? ob - b : 0u)
			               : lane == CPLX_CUT3 ? (keep_out ? e - oe : 0u) : lane == CPLX_HEAD_RECS ? (hd ? 1u : 0u) : lane == CPLX_TAIL_RECS ? (t ? 1u : 0u)
			               : lane >= CPLX_TAIL_BASE && lane < CPLX_HEAD_BASE ? (t && lane - CPLX_TAIL_BASE == tb ? 1u : 0u)
			               : lane >= CPLX_HEAD_BASE && lane < CPLX_DROP_LEN ? (hd && lane - CPLX_HEAD_BASE == hb ? 1u : 0u)
			               : (why && lane == why ? 1u : 0u);
			sum += mine;
		}
		const u64 met = __ballot(1);                         // in place: k_columns_common.h
		if (lane == 0 && met)
		{
			begin[r] = ob; end[r] = oe; keep[r] = keep_out ? 1 : 0;
			if (info) { info[2 * r] = i0; info[2 * r + 1] = i1; }
		}
	}
	col_stats_flush(stats, CPLX_STATS, sum);
}
