// The float reductions of the streaming kernels, written once: a block of 256 threads adds a few floats per thread and leaves one
// partial per block (block_sums), and ONE workgroup adds the partials in double in a fixed order (sums_reduce_kernel).  No float
// atomics: the order of every addition is fixed by the code, so the sums are bitwise reproducible, and that order is part of the
// library's contract ("Block sums").  (Thousands of blocks adding into ONE address serialise at the memory side: measured
// 0.32 ms for the 1080p loss with atomics, see DESIGN.md.)
// (The grid of such a pass, stream_blocks, and the size of its partial buffer are gsr_host.hpp's.)
#pragma once
#include <hip/hip_runtime.h>

namespace gsr {

// ---- wave64 sums.  Classic GCN reduction: row_shr 1,2,4,8 inside each row of 16 lanes, then
// row_bcast:15 / row_bcast:31 across the four rows; the total lands in lane 63.  hipcc does not fuse
// __builtin_amdgcn_update_dpp into the add (it emits v_mov_b32_dpp + v_pk_add_f32 + a zeroing move), so the
// multi-value form below issues the fused `v_add_f32_dpp` directly: one VALU instruction per value per
// step.  Values are interleaved inside one asm statement so that consecutive DPP reads of a register are
// always >= 3 instructions after its last write (gfx9 VALU-write -> DPP-read hazard: 2 wait states; the
// compiler's hazard recogniser does not look inside asm, hence the leading s_nop).
#define GSR_DPP1(CTRL, i) "v_add_f32_dpp %" #i ", %" #i ", %" #i " " CTRL "\n\t"
#define GSR_DPP4(CTRL) GSR_DPP1(CTRL, 0) GSR_DPP1(CTRL, 1) GSR_DPP1(CTRL, 2) GSR_DPP1(CTRL, 3)
#define GSR_SHR1 "row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0"
#define GSR_SHR2 "row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:0"
#define GSR_SHR4 "row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:0"
#define GSR_SHR8 "row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:0"
#define GSR_BC15 "row_bcast:15 row_mask:0xa bank_mask:0xf"
#define GSR_BC31 "row_bcast:31 row_mask:0xc bank_mask:0xf"
// Sum 4 independent values across the wave; totals valid in lane 63 only.  Must be called with all 64 lanes active.
__device__ __forceinline__ void wave_sum4(float* v) {
	asm volatile("s_nop 1\n\t" GSR_DPP4(GSR_SHR1) GSR_DPP4(GSR_SHR2) GSR_DPP4(GSR_SHR4) GSR_DPP4(GSR_SHR8) GSR_DPP4(GSR_BC15) GSR_DPP4(GSR_BC31)
	             : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
}

// First stage: the sums over a block of 256 threads of N <= 4 values per thread.  Every thread calls it; it returns true in thread 0
// alone, where v then holds the block totals, each (w0 + w1) + (w2 + w3) of the four wave totals.
template <int N>
__device__ __forceinline__ bool block_sums(float (&v)[N]) {
	static_assert(N >= 1 && N <= 4, "block_sums: wave_sum4 carries four values");
	__shared__ float red[N][4];
	float r4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
	for (int k = 0; k < N; k++) r4[k] = v[k];
	wave_sum4(r4);
	if ((threadIdx.x & 63) == 63) {
#pragma unroll
		for (int k = 0; k < N; k++) red[k][threadIdx.x >> 6] = r4[k];
	}
	__syncthreads();
	if (threadIdx.x != 0) return false;
#pragma unroll
	for (int k = 0; k < N; k++) v[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
	return true;
}

// Second stage, one workgroup of 256: out[k] = the sum over the blocks of partials[STRIDE * block + k], k < N.  Thread t adds blocks
// t, t + 256, ... in double, then an LDS tree 128 -> 1.  No block at all gives zeros.  COUNT: out[N] = count, the number of elements
// the sums run over (the metric table's rows).
template <int N, int STRIDE, bool COUNT = false, class Out>
__global__ void __launch_bounds__(256) sums_reduce_kernel(const float* __restrict__ partials, size_t nblocks, Out* __restrict__ out, double count = 0.0) {
	static_assert(N <= STRIDE, "sums_reduce_kernel: a partial holds at least the N sums");
	__shared__ double red[N][256];
	double acc[N] = {};
	for (size_t i = threadIdx.x; i < nblocks; i += 256) {
#pragma unroll
		for (int k = 0; k < N; k++) acc[k] += (double)partials[STRIDE * i + k];
	}
#pragma unroll
	for (int k = 0; k < N; k++) red[k][threadIdx.x] = acc[k];
	__syncthreads();
	for (int s = 128; s > 0; s >>= 1) {
		if ((int)threadIdx.x < s) {
#pragma unroll
			for (int k = 0; k < N; k++) red[k][threadIdx.x] += red[k][threadIdx.x + s];
		}
		__syncthreads();
	}
	if (threadIdx.x < N) out[threadIdx.x] = (Out)red[threadIdx.x][0];
	if (COUNT && threadIdx.x == N) out[N] = (Out)count;
}

}  // namespace gsr
