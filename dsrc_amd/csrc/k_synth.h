// Bench input: counter-based Illumina-like FASTQ generated directly in HBM (SURVEY 8d generator,
// integer-only so that it matches dsrc_amd/synth.py illumina_fastq byte for byte), and below it the
// variable-length 454/Ion-Torrent-like records of synth.py iontorrent_fastq (BASELINE configuration 5).
// Not part of the compression path.
#pragma once
#include "k_common.h"

#define SYNTH_READ_LEN 150u
#define SYNTH_CHUNK 1024u

__device__ __forceinline__ u64 synth_mix64(u64 x)
{
	x += 0x9E3779B97F4A7C15ull;
	x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
	x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
	return x ^ (x >> 31);
}

__device__ __forceinline__ u32 synth_digits(u64 v) { u32 d = 1; while (v >= 10) { v /= 10; ++d; } return d; }

__device__ __forceinline__ void synth_fields(u64 i, u32* lane, u32* tile, u32* x, u32* y)
{
	*lane = 1 + (u32)(((i - 1) / 250000) % 8);
	*tile = 1101 + (u32)(((i - 1) / 5000) % 96);
	*x = 1000 + (u32)((7 * i) % 20000);
	*y = 2000 + (u32)((13 * i) % 90000);
}

// "@SRRSYN.{i} HWI-ST1234:100:C0ABCACXX:{lane}:{tile}:{x}:{y} 1:N:0:ATCACG"
__device__ __forceinline__ u32 synth_title_len(u64 i)
{
	u32 lane, tile, x, y; synth_fields(i, &lane, &tile, &x, &y);
	return 8 + synth_digits(i) + 26 + 1 + 1 + 4 + 1 + synth_digits(x) + 1 + synth_digits(y) + 13;
}

__device__ __forceinline__ u32 synth_rec_size(u64 i) { return synth_title_len(i) + 1 + SYNTH_READ_LEN + 1 + 1 + 1 + SYNTH_READ_LEN + 1; }

__device__ __forceinline__ u8* synth_put_str(u8* p, const char* s) { while (*s) *p++ = (u8)*s++; return p; }
__device__ __forceinline__ u8* synth_put_num(u8* p, u64 v)
{
	const u32 d = synth_digits(v);
	for (u32 k = 0; k < d; ++k) { p[d - 1 - k] = (u8)('0' + v % 10); v /= 10; }
	return p + d;
}

__global__ void __launch_bounds__(256) k_synth_sizes(u64 first, u64 count, u64* chunk_tot)
{
	__shared__ u32 s_sum;
	if (threadIdx.x == 0) s_sum = 0;
	__syncthreads();
	u32 acc = 0;
	for (u32 k = threadIdx.x; k < SYNTH_CHUNK; k += blockDim.x)
	{
		const u64 r = (u64)blockIdx.x * SYNTH_CHUNK + k;
		if (r < count) acc += synth_rec_size(first + r);
	}
	atomicAdd(&s_sum, acc);
	__syncthreads();
	if (threadIdx.x == 0) chunk_tot[blockIdx.x] = s_sum;
}

__global__ void __launch_bounds__(256) k_synth_write(u64 first, u64 count, const u64* chunk_base, u8* out, u64 seed, u32 binned)
{
	__shared__ u32 s_off[SYNTH_CHUNK];
	// local exclusive scan of the record sizes of this chunk (serial per 256-thread stripe is enough here)
	for (u32 k = threadIdx.x; k < SYNTH_CHUNK; k += blockDim.x)
	{
		const u64 r = (u64)blockIdx.x * SYNTH_CHUNK + k;
		s_off[k] = r < count ? synth_rec_size(first + r) : 0;
	}
	__syncthreads();
	if (threadIdx.x == 0)
	{
		u32 run = 0;
		for (u32 k = 0; k < SYNTH_CHUNK; ++k) { const u32 v = s_off[k]; s_off[k] = run; run += v; }
	}
	__syncthreads();
	for (u32 k = threadIdx.x; k < SYNTH_CHUNK; k += blockDim.x)
	{
		const u64 r = (u64)blockIdx.x * SYNTH_CHUNK + k;
		if (r >= count) continue;
		const u64 i = first + r;
		u8* p = out + chunk_base[blockIdx.x] + s_off[k];
		u32 lane, tile, x, y; synth_fields(i, &lane, &tile, &x, &y);
		p = synth_put_str(p, "@SRRSYN."); p = synth_put_num(p, i);
		p = synth_put_str(p, " HWI-ST1234:100:C0ABCACXX:"); p = synth_put_num(p, lane); *p++ = ':';
		p = synth_put_num(p, tile); *p++ = ':'; p = synth_put_num(p, x); *p++ = ':'; p = synth_put_num(p, y);
		p = synth_put_str(p, " 1:N:0:ATCACG"); *p++ = '\n';
		u8* q = p + SYNTH_READ_LEN + 3;
		for (u32 pos = 0; pos < SYNTH_READ_LEN; ++pos)
		{
			const u64 h1 = synth_mix64(((i << 10) | pos) ^ seed);
			const u64 h2 = synth_mix64(h1);
			const bool is_n = ((h1 >> 2) % 500) == 0;
			i32 sum = 0;
			for (u32 b = 0; b < 8; ++b) sum += (i32)((h2 >> (8 * b)) & 0xFF);
			const i32 num = (sum - 1020) * 4 + 104;
			const i32 z4 = num >= 0 ? num / 209 : -((-num + 208) / 209);       // floor division
			i32 qv = 38 - (i32)((6 * pos) / 100) + z4;
			qv = qv < 2 ? 2 : (qv > 40 ? 40 : qv);
			if (binned) qv = qv < 3 ? 2 : qv < 18 ? 12 : qv < 30 ? 23 : 37;      // flavour 1 of dsrcgpu_synth_fastq: four-level (NovaSeq-like) qualities
			p[pos] = is_n ? (u8)'N' : (u8)"ACGT"[h1 & 3];
			q[pos] = (u8)(33 + (is_n ? 2 : qv));
		}
		p[SYNTH_READ_LEN] = '\n'; p[SYNTH_READ_LEN + 1] = '+'; p[SYNTH_READ_LEN + 2] = '\n';
		q[SYNTH_READ_LEN] = '\n';
	}
}

// host driver; returns non-zero if the data does not fit
// binned: the same records with the qualities quantised to four levels (2, 12, 23, 37: what current instruments write)
static inline int synth_illumina_device(hipStream_t s, u64 first, u64 count, u8* d_out, u64 cap, u64* bytes, u32 binned)
{
	const u32 n_chunks = (u32)((count + SYNTH_CHUNK - 1) / SYNTH_CHUNK);
	if (n_chunks == 0) { *bytes = 0; return 0; }
	u64* d_tot = nullptr;
	if (hipMalloc((void**)&d_tot, (size_t)n_chunks * 8) != hipSuccess) return 2;
	hipLaunchKernelGGL(k_synth_sizes, dim3(n_chunks), dim3(256), 0, s, first, count, d_tot);
	u64* tot = (u64*)malloc((size_t)n_chunks * 8);
	hipMemcpyAsync(tot, d_tot, (size_t)n_chunks * 8, hipMemcpyDeviceToHost, s);
	hipStreamSynchronize(s);
	u64 run = 0;
	for (u32 i = 0; i < n_chunks; ++i) { const u64 v = tot[i]; tot[i] = run; run += v; }
	*bytes = run;
	int rc = 0;
	if (run > cap) rc = 1;
	else
	{
		hipMemcpyAsync(d_tot, tot, (size_t)n_chunks * 8, hipMemcpyHostToDevice, s);
		hipLaunchKernelGGL(k_synth_write, dim3(n_chunks), dim3(256), 0, s, first, count, d_tot, d_out, (u64)0xD5C0FFEEull, binned);
		hipStreamSynchronize(s);
	}
	free(tot); hipFree(d_tot);
	return rc;
}

// ---- flavour 2 of dsrcgpu_synth_fastq: dsrc_amd/synth.py iontorrent_fastq, byte for byte --------------------------
// Reads of 40..500 bases with 1 % IUPAC codes.  One thread per record would diverge 12-fold inside a wave and put the
// byte stores of neighbouring lanes ~600 B apart, so the write kernel gives a whole wave to each record instead.
#define SYNTH_ION_SEED 0xD5C0FBBAull          // synth.SEED ^ 0x454

__device__ __forceinline__ u32 synth_ion_len(u64 i, u64 seed) { return 40u + (u32)(synth_mix64((i << 10) ^ seed ^ 0xABCDEFull) % 461u); }

// "@GXYZ1234.{i} length={L} xy={7i%10000:04d}_{13i%10000:04d} region={1+i%4}"
__device__ __forceinline__ u32 synth_ion_title_len(u64 i, u32 len) { return 10 + synth_digits(i) + 8 + (len >= 100 ? 3u : 2u) + 4 + 4 + 1 + 4 + 8 + 1; }

__device__ __forceinline__ u32 synth_ion_rec_size(u64 i, u64 seed)
{
	const u32 len = synth_ion_len(i, seed);
	return synth_ion_title_len(i, len) + 1 + len + 1 + 1 + 1 + len + 1;
}

// byte l of the title line of record i (l == title length: the newline); lanes beyond it get 0
__device__ __forceinline__ u8 synth_ion_title_byte(u32 l, u64 i, u32 len)
{
	const u32 e_id = 10 + synth_digits(i), e_len = e_id + 8 + (len >= 100 ? 3u : 2u);
	const u32 e_x = e_len + 4 + 4, e_y = e_x + 1 + 4, e_reg = e_y + 8 + 1;
	u8 c = 0; u64 v = 0; u32 shift = 0; bool digit = true;      // a digit is v / 10^shift % 10
	if (l < 10) { c = (u8)"@GXYZ1234."[l]; digit = false; }
	else if (l < e_id) { v = i; shift = e_id - 1 - l; }
	else if (l < e_id + 8) { c = (u8)" length="[l - e_id]; digit = false; }
	else if (l < e_len) { v = len; shift = e_len - 1 - l; }
	else if (l < e_len + 4) { c = (u8)" xy="[l - e_len]; digit = false; }
	else if (l < e_x) { v = (7 * i) % 10000; shift = e_x - 1 - l; }
	else if (l == e_x) { c = '_'; digit = false; }
	else if (l < e_y) { v = (13 * i) % 10000; shift = e_y - 1 - l; }
	else if (l < e_y + 8) { c = (u8)" region="[l - e_y]; digit = false; }
	else if (l < e_reg) { v = 1 + i % 4; }
	else { c = l == e_reg ? (u8)'\n' : (u8)0; digit = false; }
	for (; shift; --shift) v /= 10;
	return digit ? (u8)('0' + v % 10) : c;
}

__global__ void __launch_bounds__(256) k_synth_ion_sizes(u64 first, u64 count, u64* chunk_tot, u64 seed)
{
	__shared__ u32 s_sum;
	if (threadIdx.x == 0) s_sum = 0;
	__syncthreads();
	u32 acc = 0;
	for (u32 k = threadIdx.x; k < SYNTH_CHUNK; k += blockDim.x)
	{
		const u64 r = (u64)blockIdx.x * SYNTH_CHUNK + k;
		if (r < count) acc += synth_ion_rec_size(first + r, seed);
	}
	atomicAdd(&s_sum, acc);
	__syncthreads();
	if (threadIdx.x == 0) chunk_tot[blockIdx.x] = s_sum;
}

// one workgroup per group of SYNTH_CHUNK records; its waves take the records in turn, one wave per record
__global__ void __launch_bounds__(256) k_synth_ion_write(u64 first, u64 count, const u64* chunk_base, u8* out, u64 seed)
{
	constexpr u32 PER = SYNTH_CHUNK / 256;          // consecutive records whose sizes one thread sums for the scan
	__shared__ u32 s_off[SYNTH_CHUNK];
	const u64 r0 = (u64)blockIdx.x * SYNTH_CHUNK;
	u32 size[PER], mine = 0;
	for (u32 j = 0; j < PER; ++j)
	{
		const u64 r = r0 + threadIdx.x * PER + j;
		size[j] = r < count ? synth_ion_rec_size(first + r, seed) : 0;
		mine += size[j];
	}
	u32 total;
	u32 run = block_excl_scan(mine, &total);
	for (u32 j = 0; j < PER; ++j) { s_off[threadIdx.x * PER + j] = run; run += size[j]; }
	__syncthreads();

	const u32 lane = lane_id();
	u8* const base = out + chunk_base[blockIdx.x];
	for (u32 k = wave_id(); k < SYNTH_CHUNK; k += blockDim.x >> 6)
	{
		if (r0 + k >= count) break;                  // wave-uniform: the group's tail
		const u64 i = first + r0 + k;
		const u32 len = synth_ion_len(i, seed), tl = synth_ion_title_len(i, len);
		u8* const t = base + s_off[k];
		const u8 c = synth_ion_title_byte(lane, i, len);          // a title is at most 63 bytes (20-digit id): one lane per byte, newline included
		if (lane <= tl) t[lane] = c;
		u8* const sq = t + tl + 1;
		u8* const ql = sq + len + 3;
		for (u32 p0 = 0; p0 < len; p0 += 64)         // neighbouring lanes write neighbouring bytes of both lines
		{
			const u32 pos = p0 + lane;
			const u64 h1 = synth_mix64(((i << 10) | pos) ^ seed);
			const u64 h2 = synth_mix64(h1);
			const bool amb = ((h1 >> 2) % 100) == 0;
			i32 sum = 0;
			for (u32 b = 0; b < 8; ++b) sum += (i32)((h2 >> (8 * b)) & 0xFF);
			const i32 num = (sum - 1020) * 4 + 104;
			const i32 z4 = num >= 0 ? num / 209 : -((-num + 208) / 209);       // floor division
			i32 qv = 28 + 2 * z4;
			qv = qv < 0 ? 0 : (qv > 40 ? 40 : qv);
			u8 bs = (u8)"ACGT"[h1 & 3];
			if (amb)
			{
				bs = (u8)"NRYKMSWBDHV"[(h1 >> 16) % 11];
				if ((h1 >> 24) % 10 < 7) qv = 0;
			}
			if (pos < len) { sq[pos] = bs; ql[pos] = (u8)(33 + qv); }
		}
		if (lane == 0) { sq[len] = '\n'; sq[len + 1] = '+'; sq[len + 2] = '\n'; ql[len] = '\n'; }
	}
}

// host driver of flavour 2, the shape of synth_illumina_device: sizes, host scan of the group totals, capacity check, write
static inline int synth_iontorrent_device(hipStream_t s, u64 first, u64 count, u8* d_out, u64 cap, u64* bytes)
{
	const u32 n_chunks = (u32)((count + SYNTH_CHUNK - 1) / SYNTH_CHUNK);
	if (n_chunks == 0) { *bytes = 0; return 0; }
	u64* d_tot = nullptr;
	if (hipMalloc((void**)&d_tot, (size_t)n_chunks * 8) != hipSuccess) return 2;
	hipLaunchKernelGGL(k_synth_ion_sizes, dim3(n_chunks), dim3(256), 0, s, first, count, d_tot, (u64)SYNTH_ION_SEED);
	u64* tot = (u64*)malloc((size_t)n_chunks * 8);
	hipMemcpyAsync(tot, d_tot, (size_t)n_chunks * 8, hipMemcpyDeviceToHost, s);
	hipStreamSynchronize(s);
	u64 run = 0;
	for (u32 i = 0; i < n_chunks; ++i) { const u64 v = tot[i]; tot[i] = run; run += v; }
	*bytes = run;
	int rc = 0;
	if (run > cap) rc = 1;
	else
	{
		hipMemcpyAsync(d_tot, tot, (size_t)n_chunks * 8, hipMemcpyHostToDevice, s);
		hipLaunchKernelGGL(k_synth_ion_write, dim3(n_chunks), dim3(256), 0, s, first, count, d_tot, d_out, (u64)SYNTH_ION_SEED);
		hipStreamSynchronize(s);
	}
	free(tot); hipFree(d_tot);
	return rc;
}
