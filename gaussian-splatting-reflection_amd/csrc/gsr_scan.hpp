// The two-level scan of the mesh kernels (gsr_mesh.hip: the iso-surface; gsr_meshclean.hip: the clean-up), written once: a block of
// SCAN_BLOCK threads sums or scans its own values, ONE block scans the block sums with 64-bit carries, and every block adds its base.
// No atomics and no waiting between workgroups.  Two counts travel together, packed into one word: "vertices" in the low and
// "triangles" in the high 16 bits (a block's sum of either stays below 2^16 for both users).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace gsr {

#define SCAN_BLOCK 256

// Sum over the block of a value below 2^16 per thread in each half of `v`; valid in every thread.
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* lds) {
#pragma unroll
	for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s);
	if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
	__syncthreads();
	v = lds[0] + lds[1] + lds[2] + lds[3];
	__syncthreads();
	return v;
}

// Exclusive scan over the block (SCAN_BLOCK threads) of `v`.
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t* lds) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	uint32_t inc = v;
#pragma unroll
	for (int s = 1; s < 64; s <<= 1) {
		const uint32_t up = __shfl_up(inc, s);
		if (lane >= s) inc += up;
	}
	if (lane == 63) lds[wave] = inc;
	__syncthreads();
	uint32_t base = 0;
	for (int w = 0; w < wave; w++) base += lds[w];
	__syncthreads();
	return base + inc - v;
}

// One block: exclusive scan of the block sums, 1024 per round, with 64-bit carries; the totals go to counts[0..1].
// (static: each translation unit that launches it carries its own copy in its own code object)
static __global__ void __launch_bounds__(1024)
scan_spine_kernel(const uint32_t* __restrict__ part, uint32_t nblocks, uint32_t* __restrict__ vbase, uint32_t* __restrict__ tbase,
                  unsigned long long* __restrict__ counts) {
	__shared__ uint32_t wv[16], wt[16];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	unsigned long long carry_v = 0, carry_t = 0;
	for (uint32_t at = 0; at < nblocks; at += 1024) {
		const uint32_t b = at + threadIdx.x;
		const uint32_t p = b < nblocks ? part[b] : 0u;
		const uint32_t v = p & 0xffffu, t = p >> 16;
		uint32_t iv = v, it = t;                                    // (a round sums to at most 1024 * 3072)
#pragma unroll
		for (int s = 1; s < 64; s <<= 1) {
			const uint32_t uv = __shfl_up(iv, s), ut = __shfl_up(it, s);
			if (lane >= s) { iv += uv; it += ut; }
		}
		if (lane == 63) { wv[wave] = iv; wt[wave] = it; }
		__syncthreads();
		uint32_t bv = 0, bt = 0, round_v = 0, round_t = 0;
		for (int w = 0; w < 16; w++) {
			if (w < wave) { bv += wv[w]; bt += wt[w]; }
			round_v += wv[w];
			round_t += wt[w];
		}
		if (b < nblocks) {
			vbase[b] = (uint32_t)(carry_v + bv + iv - v);
			tbase[b] = (uint32_t)(carry_t + bt + it - t);
		}
		carry_v += round_v;
		carry_t += round_t;
		__syncthreads();
	}
	if (threadIdx.x == 0) { counts[0] = carry_v; counts[1] = carry_t; }
}

}  // namespace gsr
