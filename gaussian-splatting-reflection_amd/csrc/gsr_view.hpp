// What the fusion kernels (gsr_mesh.hip, gsr_unbounded.hip) need of a view to project a world point: four rows of its two matrices and
// the four dot products with (X, Y, Z, 1), formed in two steps so that a kernel that walks along z keeps the first step out of its loop.
// The nesting of the fused multiply-adds is stated here once: fma(a, X, fma(b, Y, d)), then fma(c, Z, that).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace gsr {

struct ViewDots { float z, x, y, w; };   // view-space depth; clip-space x, y, w

// The rows of the two matrices (as the rasterizers take them: element [4 * c + r] multiplies coordinate c into output r): view z;
// projection x, y, w.  Wave-uniform: scalar loads.
struct ViewRows {
	float V[4], P[12];
	__device__ __forceinline__ ViewRows(const float* view, const float* proj) {
#pragma unroll
		for (int c = 0; c < 4; c++) {
			V[c] = view[4 * c + 2];
			P[c] = proj[4 * c];
			P[4 + c] = proj[4 * c + 1];
			P[8 + c] = proj[4 * c + 3];
		}
	}
	// the part of the four dot products that does not depend on Z
	__device__ __forceinline__ ViewDots xy(float X, float Y) const {
		return {fmaf(V[0], X, fmaf(V[1], Y, V[3])), fmaf(P[0], X, fmaf(P[1], Y, P[3])), fmaf(P[4], X, fmaf(P[5], Y, P[7])),
		        fmaf(P[8], X, fmaf(P[9], Y, P[11]))};
	}
	// each product completed with Z, one at a time: the kernels test z and w before they form x and y
	__device__ __forceinline__ float z(const ViewDots& xy, float Z) const { return fmaf(V[2], Z, xy.z); }
	__device__ __forceinline__ float x(const ViewDots& xy, float Z) const { return fmaf(P[2], Z, xy.x); }
	__device__ __forceinline__ float y(const ViewDots& xy, float Z) const { return fmaf(P[6], Z, xy.y); }
	__device__ __forceinline__ float w(const ViewDots& xy, float Z) const { return fmaf(P[10], Z, xy.w); }
};

}  // namespace gsr
