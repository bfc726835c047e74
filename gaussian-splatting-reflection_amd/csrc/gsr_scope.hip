// Env-scope pass of the reference's iteration (train.py:56-63, 176-179): the bounded-scene sphere test of every Gaussian centre and the
// reflection-mask loss over the centres outside it,
//   outside = sum((xyz - centre)^2, -1) > radius^2;   loss += 0.4 * refl[outside].mean()
// six torch kernels, a nonzero and a host wait there; here one streaming pass each way (include/gsr_hip_scope.h).
//   * forward: 12 B of xyz (+ 4 B of refl) read and 2 mask bytes written per point, one point per lane per trip of a grid-stride loop;
//     each block leaves (sum of refl, count) over its outside points, sums_reduce_kernel adds the pairs in double in a fixed order.
//   * backward: 1 mask byte read and 4 B of gradient written per point (accumulate: read and written on outside rows only).
#include <cmath>
#include "gsr_host.hpp"
#include "../../include/gsr_hip_scope.h"
#include "gsr_reduce.hpp"

namespace gsr {

// The squared distance with the roundings of the torch expression: three subtractions, three squares, (a + b) + c; no fused multiply-add.
__device__ __forceinline__ float scope_d2(float x, float y, float z, float cx, float cy, float cz) {
#pragma clang fp contract(off)
	const float dx = x - cx, dy = y - cy, dz = z - cz;
	const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
	return (xx + yy) + zz;
}

// LOSS: refl, outside and partials are given; the block's pair goes to partials[2 * blockIdx.x ..].
// The two masks are two comparisons of the same d2: a point ON the sphere (d2 == radius2) and a point with a NaN coordinate fail both.
template <bool LOSS>
__global__ void __launch_bounds__(256)
env_scope_fwd_kernel(const float* __restrict__ means3D, const float* __restrict__ refl, size_t P, float cx, float cy, float cz, float radius2,
                     uint8_t* __restrict__ inside, uint8_t* __restrict__ outside, float* __restrict__ partials) {
	float acc = 0.f, cnt = 0.f;
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (size_t)gridDim.x * 256) {
		const float r = LOSS ? refl[i] : 0.f;      // (read whether or not the point is outside: both loads are in flight together)
		const float d2 = scope_d2(means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2], cx, cy, cz);
		const bool in = d2 < radius2, out = d2 > radius2;
		if (inside) inside[i] = in ? 1 : 0;
		if (outside) outside[i] = out ? 1 : 0;
		if (LOSS) {
			acc += out ? r : 0.f;
			cnt += out ? 1.f : 0.f;
		}
	}
	if (LOSS) {
		float sums[2] = {acc, cnt};
		if (block_sums(sums)) {
			partials[2 * blockIdx.x] = sums[0];
			partials[2 * blockIdx.x + 1] = sums[1];
		}
	}
}

// grad_refl[i] (+)= outside[i] ? g / count : 0.  One IEEE division per lane of the same two device floats: uniform over the grid.  count == 0
// (torch's mean over an empty selection: a NaN value, no gradient to any row) gives zeros, or with ACC no write at all.
template <bool ACC>
__global__ void __launch_bounds__(256)
env_scope_bwd_kernel(const uint8_t* __restrict__ outside, const float* __restrict__ sums, const float* __restrict__ g_loss, size_t P,
                     float* __restrict__ grad_refl) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= P) return;
	const float count = sums[1];
	const bool live = count > 0.f;
	const float v = live ? g_loss[0] / count : 0.f;
	const bool out = outside[i] != 0;
	if (ACC) {
		if (live && out) grad_refl[i] += v;
	} else {
		grad_refl[i] = out ? v : 0.f;
	}
}

}  // namespace gsr

using namespace gsr;

extern "C" size_t gsr_env_scope_scratch_floats(void) { return stream_partials(2); }

extern "C" int gsr_env_scope_forward(int P, const float* means3D, const float* refl, float cx, float cy, float cz, float radius2, uint8_t* inside,
                                     uint8_t* outside, float* sums, float* scratch, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (P < 0) { set_error("gsr_env_scope_forward: invalid size (P = %d)", P); return GSR_E_INVALID; }
	if (int rc = finite_check("gsr_env_scope_forward", "centre", cx, cy, cz)) return rc;
	// (not placement_check: a radius of zero is a scope, an empty one)
	if (!std::isfinite(radius2) || radius2 < 0.f) { set_error("gsr_env_scope_forward: radius2 must be finite and not negative"); return GSR_E_INVALID; }
	if (P == 0) {
		// nothing is read and no mask is written; a caller that asks for the sums gets (0, 0): the second stage over no block at all
		if (sums) {
			StageTimer st_(GSR_STAGE_LOSS_FWD, stream);
			sums_reduce_kernel<2, 2><<<1, 256, 0, stream>>>(scratch, (size_t)0, sums);
			GSR_LAUNCH_CHECK(0, stream);
		}
		return 0;
	}
	if (!means3D) { set_error("gsr_env_scope_forward: invalid argument (NULL means3D)"); return GSR_E_INVALID; }
	if (refl && (!outside || !sums || !scratch)) {
		set_error("gsr_env_scope_forward: refl is given, so outside, sums and scratch are required");
		return GSR_E_INVALID;
	}
	if (!refl && !inside && !outside) { set_error("gsr_env_scope_forward: nothing to do (no refl and both masks NULL)"); return GSR_E_INVALID; }
	const size_t n = (size_t)P;
	const unsigned blocks = stream_blocks(n);
	{
		StageTimer st_(GSR_STAGE_LOSS_FWD, stream);
		if (refl) {
			env_scope_fwd_kernel<true><<<blocks, 256, 0, stream>>>(means3D, refl, n, cx, cy, cz, radius2, inside, outside, scratch);
			sums_reduce_kernel<2, 2><<<1, 256, 0, stream>>>(scratch, (size_t)blocks, sums);      // sums[0] = sum of refl outside, sums[1] = their number
		} else {
			env_scope_fwd_kernel<false><<<blocks, 256, 0, stream>>>(means3D, nullptr, n, cx, cy, cz, radius2, inside, outside, nullptr);
		}
	}
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_env_scope_backward(int P, const uint8_t* outside, const float* sums, const float* g_loss, float* grad_refl, int accumulate,
                                      void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (P < 0) { set_error("gsr_env_scope_backward: invalid size (P = %d)", P); return GSR_E_INVALID; }
	if (!outside || !sums || !g_loss || !grad_refl) { set_error("gsr_env_scope_backward: invalid argument (NULL pointer)"); return GSR_E_INVALID; }
	if (accumulate != 0 && accumulate != 1) { set_error("gsr_env_scope_backward: accumulate must be 0 or 1 (got %d)", accumulate); return GSR_E_INVALID; }
	if (P == 0) return 0;
	const size_t n = (size_t)P;
	const unsigned blocks = blocks_of(n);
	{
		StageTimer st_(GSR_STAGE_LOSS_BWD, stream);
		if (accumulate) env_scope_bwd_kernel<true><<<blocks, 256, 0, stream>>>(outside, sums, g_loss, n, grad_refl);
		else env_scope_bwd_kernel<false><<<blocks, 256, 0, stream>>>(outside, sums, g_loss, n, grad_refl);
	}
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}
