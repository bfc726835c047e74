// Unbounded mesh extraction (include/gsr_hip_unbounded.h has the contracts): TSDF fusion of one rendered depth map into a lattice in
// contracted space, per-vertex colouring of world points from one view, and the map from contracted coordinates to the world.
//
// Each entry is one streaming kernel, one thread per element (node or point), 256 per block, plain loads and stores, no LDS.  In
// gsr_tsdf_integrate_contracted a wave holds 64 consecutive nodes along x, which project to neighbouring pixels: the four depth taps of
// the wave fall into a few cache lines, and the two plane accesses are one 256-byte line each.  Every skip rule is decided from
// registers and the gathered depth before a plane is touched, so a node beyond the shell or outside the view costs no plane traffic.
// The matrices and the scalars sit in the kernel arguments and in SGPRs.  Unlike gsr_tsdf_integrate the kernel hoists nothing along z:
// the contraction makes the world position a non-linear function of all three lattice coordinates.
// The view's matrix rows and dot products are gsr_view.hpp's (shared with gsr_mesh.hip); the entries' common checks are gsr_host.hpp's.
#include "gsr_host.hpp"
#include "gsr_view.hpp"
#include "../../include/gsr_hip_unbounded.h"

namespace gsr {

#define UNB_BLOCK 256

struct ViewArgs {             // what steps 2-4 need of a view
	const float* depth; const float* view; const float* proj;
	int W, H;
};

struct Taps {                 // the four pixels of a bilinear sample and their weights
	size_t i00, i01, i10, i11;
	float a, b;
	__device__ __forceinline__ float blend(const float* __restrict__ img) const {
		return (img[i00] * (1.f - a) + img[i01] * a) * (1.f - b) + (img[i10] * (1.f - a) + img[i11] * a) * b;
	}
};

// Steps 2-4 of the header for the world point (X, Y, Z): false when the point is skipped, else the taps and t.
__device__ __forceinline__ bool observe(const ViewArgs& a, const ViewRows& r, float X, float Y, float Z, float trunc, Taps& s, float& t) {
	const ViewDots xy = r.xy(X, Y);
	const float z = r.z(xy, Z), pw = r.w(xy, Z);
	if (!(z > 0.f && pw > 0.f)) return false;
	const float qx = r.x(xy, Z) / pw, qy = r.y(xy, Z) / pw;
	if (!(qx > -1.f && qx < 1.f && qy > -1.f && qy < 1.f)) return false;                  // (NaN: skipped)
	const float px = fminf(fmaxf(((qx + 1.f) * (float)a.W - 1.f) * 0.5f, 0.f), (float)(a.W - 1));
	const float py = fminf(fmaxf(((qy + 1.f) * (float)a.H - 1.f) * 0.5f, 0.f), (float)(a.H - 1));
	const float fx = floorf(px), fy = floorf(py);
	// 0 <= x0 <= W - 1 and 0 <= y0 <= H - 1 by the clamps, whatever float(W - 1) rounds to: the min with W - 1 below is on integers
	const int x0 = min((int)fx, a.W - 1), y0 = min((int)fy, a.H - 1);
	const int x1 = min(x0 + 1, a.W - 1), y1 = min(y0 + 1, a.H - 1);
	s.a = px - fx;
	s.b = py - fy;
	s.i00 = (size_t)y0 * a.W + x0;
	s.i01 = (size_t)y0 * a.W + x1;
	s.i10 = (size_t)y1 * a.W + x0;
	s.i11 = (size_t)y1 * a.W + x1;
	const float d00 = a.depth[s.i00], d01 = a.depth[s.i01], d10 = a.depth[s.i10], d11 = a.depth[s.i11];
	if (!(d00 > 0.f && d01 > 0.f && d10 > 0.f && d11 > 0.f)) return false;
	const float d = (d00 * (1.f - s.a) + d01 * s.a) * (1.f - s.b) + (d10 * (1.f - s.a) + d11 * s.a) * s.b;
	const float sdf = d - z;
	if (!(sdf > -trunc)) return false;
	t = fminf(1.f, fmaxf(-1.f, sdf / trunc));
	return true;
}

// x = y * uncontract_scale(m): the inverse of the contraction for m = |y| < 2
__device__ __forceinline__ float uncontract_scale(float m) { return m <= 1.f ? 1.f : 1.f / (m * (2.f - m)); }

struct ContractedArgs {
	float* tsdf; float* weight;
	ViewArgs v;
	int n;
	uint32_t N;               // n^3 < 2^31
	float lo, step, cx, cy, cz, radius, voxel;
};

__global__ void __launch_bounds__(UNB_BLOCK)
tsdf_integrate_contracted_kernel(const ContractedArgs a) {
	const uint32_t node = blockIdx.x * UNB_BLOCK + threadIdx.x;        // < 2^31 + 256
	if (node >= a.N) return;
	const uint32_t n = (uint32_t)a.n, row = node / n, k = row / n;
	const uint32_t i = node - row * n, j = row - k * n;
	const float yx = fmaf(a.step, (float)i, a.lo), yy = fmaf(a.step, (float)j, a.lo), yz = fmaf(a.step, (float)k, a.lo);
	const float m = sqrtf(fmaf(yx, yx, fmaf(yy, yy, yz * yz)));
	if (!(m < 2.f)) return;
	const float s = uncontract_scale(m) * a.radius;
	const float trunc = m <= 1.f ? 5.f * a.voxel : 5.f * a.voxel / (2.f - fminf(m, 1.9f));
	const ViewRows r(a.v.view, a.v.proj);
	Taps taps;
	float t;
	if (!observe(a.v, r, fmaf(s, yx, a.cx), fmaf(s, yy, a.cy), fmaf(s, yz, a.cz), trunc, taps, t)) return;
	const float w = a.weight[node], w1 = w + 1.f;
	a.tsdf[node] = (a.tsdf[node] * w + t) / w1;
	a.weight[node] = w1;
}

struct PointsArgs {
	const float* points; float* color; float* weight; const float* rgb;
	ViewArgs v;
	uint32_t n_points;        // < 2^31
	float sdf_trunc;
};

__global__ void __launch_bounds__(UNB_BLOCK)
points_fuse_view_kernel(const PointsArgs a) {
	const uint32_t p = blockIdx.x * UNB_BLOCK + threadIdx.x;
	if (p >= a.n_points) return;
	const size_t at = (size_t)p * 3;
	const ViewRows r(a.v.view, a.v.proj);
	Taps taps;
	float t;
	if (!observe(a.v, r, a.points[at], a.points[at + 1], a.points[at + 2], a.sdf_trunc, taps, t)) return;
	const size_t hw = (size_t)a.v.W * a.v.H;
	const float w = a.weight[p], w1 = w + 1.f;
#pragma unroll
	for (int c = 0; c < 3; c++) a.color[at + c] = (a.color[at + c] * w + taps.blend(a.rgb + c * hw)) / w1;
	a.weight[p] = w1;
}

__global__ void __launch_bounds__(UNB_BLOCK)
uncontract_points_kernel(const float* src, float* dst, uint32_t n_points, float cx, float cy, float cz, float radius, float max_range) {
	const uint32_t p = blockIdx.x * UNB_BLOCK + threadIdx.x;
	if (p >= n_points) return;
	const size_t at = (size_t)p * 3;
	const float yx = src[at], yy = src[at + 1], yz = src[at + 2];          // (read before the writes: dst may be src)
	float m = sqrtf(fmaf(yx, yx, fmaf(yy, yy, yz * yz)));
	if (!(m < 2.f)) m = 0x1.fffffep+0f;                                    // the largest float32 below 2: a finite scale
	const float s = uncontract_scale(m) * radius;
	dst[at] = fminf(fmaxf(fmaf(s, yx, cx), -max_range), max_range);
	dst[at + 1] = fminf(fmaxf(fmaf(s, yy, cy), -max_range), max_range);
	dst[at + 2] = fminf(fmaxf(fmaf(s, yz, cz), -max_range), max_range);
}

}  // namespace gsr

// ------------------------------------------------------------------------------------------------------------ host side
using namespace gsr;

extern "C" int gsr_tsdf_integrate_contracted(float* tsdf, float* weight, int n, float lo, float step, float cx, float cy, float cz, float radius,
                                             float voxel, const float* depth, int W, int H, const float* viewmatrix, const float* projmatrix,
                                             void* stream_) {
	const char* entry = "gsr_tsdf_integrate_contracted";
	hipStream_t stream = (hipStream_t)stream_;
	if (!tsdf || !weight || !depth || !viewmatrix || !projmatrix) { set_error("%s: invalid argument (NULL pointer)", entry); return GSR_E_INVALID; }
	if (int rc = pointers_check(entry, {tsdf, weight, depth, viewmatrix, projmatrix})) return rc;
	if (n < 2 || n > 2048 || (uint64_t)n * (uint64_t)n * (uint64_t)n >= LIMIT_2_31) {     // (the product of three factors up to 2^11 cannot wrap)
		set_error("%s: n must be at least 2 and n^3 below 2^31 (got %d)", entry, n);
		return GSR_E_INVALID;
	}
	if (!positive_finite(step) || !positive_finite(voxel)) {
		set_error("%s: step and voxel must be positive and finite (got %g, %g)", entry, (double)step, (double)voxel);
		return GSR_E_INVALID;
	}
	if (!std::isfinite(lo)) { set_error("%s: lo is not finite", entry); return GSR_E_INVALID; }
	if (int rc = placement_check(entry, "radius", radius, "centre", cx, cy, cz)) return rc;
	if (int rc = image_check(entry, W, H)) return rc;
	ContractedArgs a;
	a.tsdf = tsdf; a.weight = weight;
	a.v.depth = depth; a.v.view = viewmatrix; a.v.proj = projmatrix; a.v.W = W; a.v.H = H;
	a.n = n; a.N = (uint32_t)n * (uint32_t)n * (uint32_t)n;
	a.lo = lo; a.step = step; a.cx = cx; a.cy = cy; a.cz = cz; a.radius = radius; a.voxel = voxel;
	tsdf_integrate_contracted_kernel<<<(a.N + UNB_BLOCK - 1) / UNB_BLOCK, UNB_BLOCK, 0, stream>>>(a);      // at most 2^23 blocks
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_points_fuse_view(const float* points, uint64_t n_points, float* color, float* weight, const float* depth, const float* rgb,
                                    int W, int H, const float* viewmatrix, const float* projmatrix, float sdf_trunc, void* stream_) {
	const char* entry = "gsr_points_fuse_view";
	hipStream_t stream = (hipStream_t)stream_;
	if (!depth || !rgb || !viewmatrix || !projmatrix || (n_points > 0 && (!points || !color || !weight))) {
		set_error("%s: invalid argument (NULL pointer)", entry);
		return GSR_E_INVALID;
	}
	if (int rc = pointers_check(entry, {points, color, weight, depth, rgb, viewmatrix, projmatrix})) return rc;
	if (int rc = points_check(entry, n_points)) return rc;
	if (!positive_finite(sdf_trunc)) { set_error("%s: sdf_trunc must be positive and finite (got %g)", entry, (double)sdf_trunc); return GSR_E_INVALID; }
	if (int rc = image_check(entry, W, H)) return rc;
	if (n_points == 0) return 0;
	PointsArgs a;
	a.points = points; a.color = color; a.weight = weight; a.rgb = rgb;
	a.v.depth = depth; a.v.view = viewmatrix; a.v.proj = projmatrix; a.v.W = W; a.v.H = H;
	a.n_points = (uint32_t)n_points; a.sdf_trunc = sdf_trunc;
	points_fuse_view_kernel<<<(a.n_points + UNB_BLOCK - 1) / UNB_BLOCK, UNB_BLOCK, 0, stream>>>(a);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_uncontract_points(const float* src, float* dst, uint64_t n_points, float cx, float cy, float cz, float radius, float max_range,
                                     void* stream_) {
	const char* entry = "gsr_uncontract_points";
	hipStream_t stream = (hipStream_t)stream_;
	if (n_points > 0 && (!src || !dst)) { set_error("%s: invalid argument (NULL pointer)", entry); return GSR_E_INVALID; }
	if (int rc = pointers_check(entry, {src, dst})) return rc;
	if (int rc = points_check(entry, n_points)) return rc;
	if (int rc = placement_check(entry, "radius", radius, "centre", cx, cy, cz)) return rc;
	if (!positive_finite(max_range)) { set_error("%s: max_range must be positive and finite (got %g)", entry, (double)max_range); return GSR_E_INVALID; }
	if (n_points == 0) return 0;
	uncontract_points_kernel<<<((uint32_t)n_points + UNB_BLOCK - 1) / UNB_BLOCK, UNB_BLOCK, 0, stream>>>(src, dst, (uint32_t)n_points, cx, cy, cz,
	                                                                                                      radius, max_range);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}
