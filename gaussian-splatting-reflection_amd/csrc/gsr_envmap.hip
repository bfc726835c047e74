// The two environment-map transforms of the reference's schedule (scene/gaussian_model.py:375-393): double_env_map's bicubic resize and
// filter_env_map's sharpening in sigmoid space, on the [6, C, L, L] texture as a run of `planes` contiguous L x L images
// (include/gsr_hip_envmap.h has the contracts).  Each runs once or a few times per training run: one thread per output texel, no LDS,
// no tuning.  Every index is formed in 64 bits from values the entries have bounded (planes * L * L < 2^31 for both resolutions).
#include <cmath>
#include <initializer_list>
#include "gsr_host.hpp"
#include "../../include/gsr_hip_envmap.h"

namespace gsr {

// Cubic convolution, A = -0.75 (torch's bicubic): the weight of a tap at distance x <= 1, and at distance 1 <= x <= 2, as Horner forms.
// Exactly 1 at x = 0 and exactly 0 at x = 1 and x = 2 (every intermediate is representable there), fused or not.
#define ENVMAP_CUBIC_A (-0.75f)
__device__ __forceinline__ float cubic_near(float x) { return ((ENVMAP_CUBIC_A + 2.f) * x - (ENVMAP_CUBIC_A + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cubic_far(float x) {
	return ((ENVMAP_CUBIC_A * x - 5.f * ENVMAP_CUBIC_A) * x + 8.f * ENVMAP_CUBIC_A) * x - 4.f * ENVMAP_CUBIC_A;
}

// Source node and fraction of output node d along one axis, from integers: the fraction carries one rounding (the division) and is exactly 0
// where the output node lies on a source node.  den = L_dst - 1 (0: the single output node reads source node 0).
__device__ __forceinline__ void source_coord(uint32_t d, uint32_t L_src, uint32_t den, int& i, float& t) {
	if (den == 0) { i = 0; t = 0.f; return; }
	const uint64_t n = (uint64_t)d * (L_src - 1);
	i = (int)(n / den);
	t = (float)(uint32_t)(n % den) / (float)den;
}

__device__ __forceinline__ void cubic_weights(float t, float w[4]) {
	w[0] = cubic_far(t + 1.f);
	w[1] = cubic_near(t);
	w[2] = cubic_near(1.f - t);
	w[3] = cubic_far(2.f - t);
}

__global__ void __launch_bounds__(256)
envmap_resize_kernel(const float* __restrict__ src, float* __restrict__ dst, uint32_t total, uint32_t L_src, uint32_t L_dst) {
	const uint32_t idx = blockIdx.x * 256u + threadIdx.x;      // (total < 2^31: the grid's last block stays below 2^32)
	if (idx >= total) return;
	const uint32_t per = L_dst * L_dst;
	const uint32_t plane = idx / per, rem = idx - plane * per;
	const uint32_t y = rem / L_dst, x = rem - y * L_dst;
	int ix, iy;
	float tx, ty, wx[4], wy[4];
	source_coord(x, L_src, L_dst - 1, ix, tx);
	source_coord(y, L_src, L_dst - 1, iy, ty);
	cubic_weights(tx, wx);
	cubic_weights(ty, wy);
	const float* __restrict__ img = src + (size_t)plane * L_src * L_src;
	const int hi = (int)L_src - 1;
	int cx[4];
#pragma unroll
	for (int k = 0; k < 4; k++) cx[k] = min(max(ix - 1 + k, 0), hi);
	float rows[4];
#pragma unroll
	for (int j = 0; j < 4; j++) {
		const float* __restrict__ row = img + (size_t)min(max(iy - 1 + j, 0), hi) * L_src;
		rows[j] = ((row[cx[0]] * wx[0] + row[cx[1]] * wx[1]) + row[cx[2]] * wx[2]) + row[cx[3]] * wx[3];      // along x first
	}
	dst[idx] = ((rows[0] * wy[0] + rows[1] * wy[1]) + rows[2] * wy[2]) + rows[3] * wy[3];                      // then along y
}

__device__ __forceinline__ float envmap_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }      // (a NaN stays one)

__global__ void __launch_bounds__(256)
envmap_sharpen_kernel(const float* __restrict__ src, float* __restrict__ dst, uint32_t total, uint32_t L, float factor, float lo, float hi) {
	const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
	if (idx >= total) return;
	const uint32_t per = L * L;
	const uint32_t rem = idx % per;
	const uint32_t y = rem / L, x = rem - y * L;
	const float s = envmap_sigmoid(src[idx]);
	float o = s;
	if (L > 2 && x > 0 && y > 0 && x < L - 1 && y < L - 1) {        // interior: the eight neighbours lie in the same plane
		const float* __restrict__ c = src + idx;
		float sum = 0.f;
#pragma unroll
		for (int dy = -1; dy <= 1; dy++)
#pragma unroll
			for (int dx = -1; dx <= 1; dx++)
				sum += (dx == 0 && dy == 0) ? s : envmap_sigmoid(c[(ptrdiff_t)dy * (ptrdiff_t)L + dx]);
		const float b = (sum + 4.f * s) / 13.f;
		o = clampf(factor * s + (1.f - factor) * b, 0.f, 1.f);
	}
	o = clampf(o, lo, hi);
	dst[idx] = logf(o / (1.f - o));
}

// What both entries check alike.  Returns 0 to go on.
static int envmap_check(const char* entry, const float* src, float* dst, int planes, int L_src, int L_dst) {
	if (!src || !dst) { set_error("%s: invalid argument (NULL pointer)", entry); return GSR_E_INVALID; }
	if (int rc = pointers_check(entry, {src, dst}, 4, "src and dst")) return rc;
	if (planes < 1 || L_src < 1 || L_dst < 1) {
		set_error("%s: invalid size (planes = %d, resolutions %d and %d)", entry, planes, L_src, L_dst);
		return GSR_E_INVALID;
	}
	for (int L : {L_src, L_dst})      // (L * L fits 64 bits; the product with planes is never formed)
		if ((uint64_t)L * (uint64_t)L > (LIMIT_2_31 - 1) / (uint64_t)planes) {
			set_error("%s: planes * L * L must be below 2^31 (planes = %d, L = %d)", entry, planes, L);
			return GSR_E_INVALID;
		}
	const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
	const uintptr_t s1 = s0 + (uintptr_t)planes * L_src * L_src * sizeof(float), d1 = d0 + (uintptr_t)planes * L_dst * L_dst * sizeof(float);
	if (s0 < d1 && d0 < s1) { set_error("%s: src and dst overlap (the transform does not work in place)", entry); return GSR_E_INVALID; }
	return 0;
}

}  // namespace gsr

using namespace gsr;

extern "C" int gsr_envmap_resize(const float* src, float* dst, int planes, int L_src, int L_dst, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (int rc = envmap_check("gsr_envmap_resize", src, dst, planes, L_src, L_dst)) return rc;
	const uint32_t total = (uint32_t)planes * (uint32_t)L_dst * (uint32_t)L_dst;
	envmap_resize_kernel<<<blocks_of(total), 256, 0, stream>>>(src, dst, total, (uint32_t)L_src, (uint32_t)L_dst);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_envmap_sharpen(const float* src, float* dst, int planes, int L, float factor, float lo, float hi, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (int rc = envmap_check("gsr_envmap_sharpen", src, dst, planes, L, L)) return rc;
	if (!std::isfinite(factor)) { set_error("gsr_envmap_sharpen: factor is not finite"); return GSR_E_INVALID; }
	if (!(0.f < lo && lo < hi && hi < 1.f)) {
		set_error("gsr_envmap_sharpen: the clamp must satisfy 0 < lo < hi < 1 (got %g, %g)", (double)lo, (double)hi);
		return GSR_E_INVALID;
	}
	const uint32_t total = (uint32_t)planes * (uint32_t)L * (uint32_t)L;
	envmap_sharpen_kernel<<<blocks_of(total), 256, 0, stream>>>(src, dst, total, (uint32_t)L, factor, lo, hi);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}
