// simple_knn.distCUDA2 (the reference's scene/gaussian_model.py:20, 170): for every point of a cloud the mean of the squared
// distances to its 3 nearest OTHER points, used once per training run to initialise the surfel scales.  Exact search.
//
//   1. bounds:  one grid-stride reduction of the cloud's AABB into per-workgroup partials (knn_bounds_kernel);
//   2. order:   30-bit Morton keys quantised to the AABB (cubic cells), sorted with the index as value (gsr_sort.hpp or
//               rocprim::radix_sort_pairs, end_bit 30); the points are gathered into a sorted float4 array (w = original index);
//   3. boxes:   level 0 = the AABB of each run of 64 consecutive sorted points (one wavefront), levels 1 and 2 = unions of 64 children;
//   4. search:  one wavefront per leaf.  Each lane seeds its best-3 from its own leaf, then the wave walks the hierarchy from the top:
//               a child survives if its distance to the wave's own leaf box is not above the largest b2 of the lanes (one wave-uniform
//               test per child, children tested in parallel across lanes) AND at least one lane's own point-to-box distance is not
//               above that lane's b2 (a ballot).  A surviving leaf's 64 points are staged in LDS once and every lane updates its best-3.
//               The wave stops as soon as every lane has b2 == 0 (a cloud of identical points would otherwise scan everything).
//
// Exactness: a box-to-point (or box-to-box) distance is computed with the expression and operation order of the point-to-point
// distance, from per-axis gaps that are, by the monotonicity of rounding, never larger than the rounded coordinate differences of
// any pair of points the boxes contain.  So a box is pruned (strict >) only if none of its points can beat a current b2; ties do
// not change the multiset of the three smallest distances.  The result is (b0 + b1 + b2) / 3 of that multiset, summed in ascending
// order, and so does not depend on the input order bit for bit.  Missing neighbours (P < 4) stay at FLT_MAX.
// Host side: the caller's scratch is KnnLayout, typed pointers carved by knn_carve on Carver (a NULL base answers gsr_knn_scratch_bytes).
#include "gsr_host.hpp"
#include <algorithm>
#include <cfloat>
#include "gsr_sort.hpp"
#include <rocprim/iterator/counting_iterator.hpp>

namespace gsr {

#define KNN_LEAF 64                 // points per level-0 box = one wavefront
#define KNN_LEVELS 3                // levels of boxes; the top one is scanned in chunks of 64
#define KNN_BOUNDS_BLOCKS 256       // partial AABBs of the bounds pass (the Morton kernel reduces them again)
#define KNN_MORTON_BITS 30u
#define KNN_SORT_SHAPE 1024, 4, 8   // the depth sort's shape (gsr_common.hip): P keys, four 8-bit places
using KnnSortConfig = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 65536>;
using KnnSort = RadixSort<KNN_SORT_SHAPE, KnnSortConfig>;
static const size_t KNN_MAX_POINTS = (size_t)1 << 30;   // the C entries' range of P

// The squared distance of the contract: dx*dx + dy*dy + dz*dz in float32, in this order and without contraction, for points and
// for the lower bounds of boxes alike (see the exactness note above).
__device__ __forceinline__ float sq3(float dx, float dy, float dz) {
#pragma clang fp contract(off)
	return dx * dx + dy * dy + dz * dz;
}
// per-axis gap between [alo, ahi] and [blo, bhi] (0 where they overlap)
__device__ __forceinline__ float gap1(float alo, float ahi, float blo, float bhi) { return fmaxf(0.0f, fmaxf(blo - ahi, alo - bhi)); }

__device__ __forceinline__ float wave_min(float v) {
	for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
	return v;
}
__device__ __forceinline__ float wave_max(float v) {
	for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
	return v;
}

// Workgroup-wide min / max of lo / hi (256 threads); the result is valid in every thread.
__device__ __forceinline__ void block_minmax(float3& lo, float3& hi) {
	__shared__ float s[4][6];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	float v[6] = {wave_min(lo.x), wave_min(lo.y), wave_min(lo.z), wave_max(hi.x), wave_max(hi.y), wave_max(hi.z)};
	if (lane == 0)
		for (int k = 0; k < 6; k++) s[wave][k] = v[k];
	__syncthreads();
	for (int w = 0; w < 4; w++) {
		for (int k = 0; k < 3; k++) v[k] = fminf(v[k], s[w][k]);
		for (int k = 3; k < 6; k++) v[k] = fmaxf(v[k], s[w][k]);
	}
	lo = make_float3(v[0], v[1], v[2]);
	hi = make_float3(v[3], v[4], v[5]);
}

__global__ void __launch_bounds__(256) knn_bounds_kernel(int P, const float* __restrict__ points, float4* __restrict__ partial) {
	float3 lo = make_float3(FLT_MAX, FLT_MAX, FLT_MAX), hi = make_float3(-FLT_MAX, -FLT_MAX, -FLT_MAX);
	for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256) {
		const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
		lo = make_float3(fminf(lo.x, x), fminf(lo.y, y), fminf(lo.z, z));
		hi = make_float3(fmaxf(hi.x, x), fmaxf(hi.y, y), fmaxf(hi.z, z));
	}
	block_minmax(lo, hi);
	if (threadIdx.x == 0) {
		partial[2 * blockIdx.x] = make_float4(lo.x, lo.y, lo.z, 0.0f);
		partial[2 * blockIdx.x + 1] = make_float4(hi.x, hi.y, hi.z, 0.0f);
	}
}

// 10 bits -> every third bit of 30
__device__ __forceinline__ uint32_t spread3(uint32_t v) {
	v = (v * 0x00010001u) & 0xFF0000FFu;
	v = (v * 0x00000101u) & 0x0F00F00Fu;
	v = (v * 0x00000011u) & 0xC30C30C3u;
	v = (v * 0x00000005u) & 0x49249249u;
	return v;
}
__device__ __forceinline__ uint32_t quant10(float v, float lo, float scale) {
	return (uint32_t)fminf(fmaxf((v - lo) * scale, 0.0f), 1023.0f);   // (NaN -> 0: the key only orders, it never decides a result)
}

__global__ void __launch_bounds__(256) knn_morton_kernel(int P, int n_partial, const float* __restrict__ points, const float4* __restrict__ partial,
                                                          uint32_t* __restrict__ keys) {
	float3 lo = make_float3(FLT_MAX, FLT_MAX, FLT_MAX), hi = make_float3(-FLT_MAX, -FLT_MAX, -FLT_MAX);
	if ((int)threadIdx.x < n_partial) {
		const float4 a = partial[2 * threadIdx.x], b = partial[2 * threadIdx.x + 1];
		lo = make_float3(a.x, a.y, a.z);
		hi = make_float3(b.x, b.y, b.z);
	}
	block_minmax(lo, hi);
	const float ext = fmaxf(hi.x - lo.x, fmaxf(hi.y - lo.y, hi.z - lo.z));
	const float scale = (ext > 0.0f && ext <= FLT_MAX) ? 1024.0f / ext : 0.0f;     // cubic cells: boxes stay compact in flat clouds
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= P) return;
	const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
	keys[i] = (spread3(quant10(x, lo.x, scale)) << 2) | (spread3(quant10(y, lo.y, scale)) << 1) | spread3(quant10(z, lo.z, scale));
}

// The points in Morton order (w = original index) and the level-0 boxes: one wavefront per leaf.
__global__ void __launch_bounds__(256) knn_gather_leaves_kernel(int P, const float* __restrict__ points, const uint32_t* __restrict__ order,
                                                                 float4* __restrict__ sorted, float4* __restrict__ box_lo, float4* __restrict__ box_hi) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	float3 lo = make_float3(FLT_MAX, FLT_MAX, FLT_MAX), hi = make_float3(-FLT_MAX, -FLT_MAX, -FLT_MAX);
	if (i < P) {
		const uint32_t j = order[i];
		const float x = points[3 * (size_t)j], y = points[3 * (size_t)j + 1], z = points[3 * (size_t)j + 2];
		sorted[i] = make_float4(x, y, z, __uint_as_float(j));
		lo = hi = make_float3(x, y, z);
	}
	lo = make_float3(wave_min(lo.x), wave_min(lo.y), wave_min(lo.z));
	hi = make_float3(wave_max(hi.x), wave_max(hi.y), wave_max(hi.z));
	const int leaf = i / KNN_LEAF;
	if ((threadIdx.x & 63) == 0 && leaf * KNN_LEAF < P) {
		box_lo[leaf] = make_float4(lo.x, lo.y, lo.z, 0.0f);
		box_hi[leaf] = make_float4(hi.x, hi.y, hi.z, 0.0f);
	}
}

// One level up: the union of up to 64 consecutive children per parent, one wavefront per parent.
__global__ void __launch_bounds__(256) knn_parent_boxes_kernel(int n_child, const float4* __restrict__ child_lo, const float4* __restrict__ child_hi,
                                                                float4* __restrict__ lo_out, float4* __restrict__ hi_out) {
	const int c = blockIdx.x * 256 + threadIdx.x;
	float3 lo = make_float3(FLT_MAX, FLT_MAX, FLT_MAX), hi = make_float3(-FLT_MAX, -FLT_MAX, -FLT_MAX);
	if (c < n_child) {
		const float4 a = child_lo[c], b = child_hi[c];
		lo = make_float3(a.x, a.y, a.z);
		hi = make_float3(b.x, b.y, b.z);
	}
	lo = make_float3(wave_min(lo.x), wave_min(lo.y), wave_min(lo.z));
	hi = make_float3(wave_max(hi.x), wave_max(hi.y), wave_max(hi.z));
	const int parent = c / 64;
	if ((threadIdx.x & 63) == 0 && parent * 64 < n_child) {
		lo_out[parent] = make_float4(lo.x, lo.y, lo.z, 0.0f);
		hi_out[parent] = make_float4(hi.x, hi.y, hi.z, 0.0f);
	}
}

struct KnnTree {
	const float4* pts;                  // sorted points, w = original index
	const float4* lo[KNN_LEVELS];
	const float4* hi[KNN_LEVELS];
	int n[KNN_LEVELS];                  // boxes per level
	int P;
};

// State of one lane of a searching wavefront.  Lanes beyond P carry b = -1: never updated, never asking for a box, and not raising
// the wave's largest b2.
struct KnnLane {
	float qx, qy, qz;
	float b0, b1, b2;
	int lane, own_leaf;
	float4 wlo, whi;                    // the wave's own leaf box (uniform)
	float4* stage;                      // this wave's 64 LDS slots
};

// Stages leaf `leaf`'s points in LDS and lets every lane take them into its best-3.  SELF: the wave's own leaf (skip the lane's own point).
template <bool SELF>
__device__ __forceinline__ void knn_visit_leaf(const KnnTree& t, KnnLane& s, int leaf) {
	const int base = leaf * KNN_LEAF, n = min(KNN_LEAF, t.P - base);
	__builtin_amdgcn_wave_barrier();          // (every lane has read the previous leaf: LDS ops of a wave complete in order)
	if (s.lane < n) s.stage[s.lane] = t.pts[base + s.lane];
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	float b0 = s.b0, b1 = s.b1, b2 = s.b2;
#pragma unroll 8
	for (int j = 0; j < n; j++) {
		const float4 c = s.stage[j];
		float d = sq3(c.x - s.qx, c.y - s.qy, c.z - s.qz);
		if (SELF && j == s.lane) d = INFINITY;
		// sorted insertion into b0 <= b1 <= b2 (keeps the three smallest): min / med3 / med3 of the old values
		const float n0 = fminf(b0, d), n1 = __builtin_amdgcn_fmed3f(b0, d, b1), n2 = __builtin_amdgcn_fmed3f(b1, d, b2);
		b0 = n0;
		b1 = n1;
		b2 = n2;
	}
	s.b0 = b0;
	s.b1 = b1;
	s.b2 = b2;
}

// Children [first, first + count) (count <= 64) of level L.  Returns true once every lane has b2 == 0 (nothing can improve).
template <int L>
__device__ __forceinline__ bool knn_descend(const KnnTree& t, KnnLane& s, int first, int count) {
	const float mb2 = wave_max(s.b2);
	if (mb2 == 0.0f) return true;
	bool keep = false;
	if (s.lane < count) {
		const float4 lo = t.lo[L][first + s.lane], hi = t.hi[L][first + s.lane];
		const float g = sq3(gap1(lo.x, hi.x, s.wlo.x, s.whi.x), gap1(lo.y, hi.y, s.wlo.y, s.whi.y), gap1(lo.z, hi.z, s.wlo.z, s.whi.z));
		keep = !(g > mb2) && (L > 0 || first + s.lane != s.own_leaf);
	}
	unsigned long long m = __ballot(keep);
	while (m) {
		const int c = first + (int)__builtin_ctzll(m);
		m &= m - 1;
		const float4 lo = t.lo[L][c], hi = t.hi[L][c];
		const float g = sq3(gap1(lo.x, hi.x, s.qx, s.qx), gap1(lo.y, hi.y, s.qy, s.qy), gap1(lo.z, hi.z, s.qz, s.qz));
		if (__ballot(g <= s.b2) == 0ull) continue;
		if constexpr (L == 0) {
			knn_visit_leaf<false>(t, s, c);
			if (wave_max(s.b2) == 0.0f) return true;
		} else {
			const int cf = c * 64, cc = min(64, t.n[L - 1] - cf);
			if (knn_descend<L - 1>(t, s, cf, cc)) return true;
		}
	}
	return false;
}

__global__ void __launch_bounds__(256) knn_search_kernel(KnnTree t, float* __restrict__ mean_dist) {
	__shared__ float4 stage[4][KNN_LEAF];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int leaf = blockIdx.x * 4 + wave;
	if (leaf >= t.n[0]) return;                  // (wave-uniform; no workgroup barrier below)
	const int i = leaf * KNN_LEAF + lane;
	const bool valid = i < t.P;
	const float4 q = t.pts[valid ? i : leaf * KNN_LEAF];
	KnnLane s;
	s.qx = q.x;
	s.qy = q.y;
	s.qz = q.z;
	s.b0 = s.b1 = s.b2 = valid ? FLT_MAX : -1.0f;
	s.lane = lane;
	s.own_leaf = leaf;
	s.wlo = t.lo[0][leaf];
	s.whi = t.hi[0][leaf];
	s.stage = stage[wave];
	knn_visit_leaf<true>(t, s, leaf);
	const int top = KNN_LEVELS - 1;
	for (int first = 0; first < t.n[top]; first += 64)
		if (knn_descend<top>(t, s, first, min(64, t.n[top] - first))) break;
	if (valid) {
#pragma clang fp contract(off)
		mean_dist[__float_as_uint(q.w)] = (s.b0 + s.b1 + s.b2) / 3.0f;
	}
}

// ------------------------------------------------------------------ scratch layout (one caller-provided buffer)
struct KnnLayout {
	uint32_t *keys, *keys_sorted, *order;     // P each   Morton keys, the same sorted, the original index at each sorted position
	float4* sorted;                           // P        the points in Morton order, w = original index
	float4* partial;                          // 2 * KNN_BOUNDS_BLOCKS   partial AABBs: lo, hi
	float4 *lo[KNN_LEVELS], *hi[KNN_LEVELS];  // n[k]     boxes of level k
	char* sort_temp;                          // sort_bytes
	size_t sort_bytes, bytes;
	int n[KNN_LEVELS];                  // boxes per level
};
static KnnLayout knn_carve(void* base, size_t P) {
	Carver c(base);
	KnnLayout l;
	l.n[0] = (int)((P + KNN_LEAF - 1) / KNN_LEAF);
	for (int k = 1; k < KNN_LEVELS; k++) l.n[k] = (l.n[k - 1] + 63) / 64;
	l.keys = c.take<uint32_t>(P);
	l.keys_sorted = c.take<uint32_t>(P);
	l.order = c.take<uint32_t>(P);
	l.sorted = c.take<float4>(P);
	l.partial = c.take<float4>(2 * KNN_BOUNDS_BLOCKS);
	for (int k = 0; k < KNN_LEVELS; k++) {
		l.lo[k] = c.take<float4>(l.n[k]);
		l.hi[k] = c.take<float4>(l.n[k]);
	}
	l.sort_bytes = KnnSort::temp_bytes((const uint32_t*)nullptr, rocprim::counting_iterator<uint32_t>(0), (uint32_t*)nullptr, P, KNN_MORTON_BITS);
	l.sort_temp = c.take<char>(l.sort_bytes);
	l.bytes = c.size();
	return l;
}

}  // namespace gsr

using namespace gsr;

extern "C" size_t gsr_knn_scratch_bytes(int P) {
	if (P <= 0 || (size_t)P >= KNN_MAX_POINTS) return 0;
	return knn_carve(nullptr, (size_t)P).bytes;
}

extern "C" int gsr_knn_mean_dist(int P, const float* points, float* mean_dist, void* scratch, size_t scratch_bytes, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (P < 0 || (size_t)P >= KNN_MAX_POINTS) { set_error("gsr_knn_mean_dist: P = %d outside [0, 2^30)", P); return GSR_E_INVALID; }
	if (P == 0) return 0;
	if (!points || !mean_dist || !scratch) { set_error("gsr_knn_mean_dist: NULL buffer"); return GSR_E_INVALID; }
	const KnnLayout l = knn_carve(scratch, (size_t)P);
	if (scratch_bytes < l.bytes) {
		set_error("gsr_knn_mean_dist: scratch of %zu bytes, %zu needed (gsr_knn_scratch_bytes)", scratch_bytes, l.bytes);
		return GSR_E_INVALID;
	}
	if (int rc = aligned_check("gsr_knn_mean_dist", "scratch", scratch, 16)) return rc;   // (it is carved into float4 arrays)
	KnnTree t;
	t.pts = l.sorted;
	t.P = P;
	for (int k = 0; k < KNN_LEVELS; k++) {
		t.lo[k] = l.lo[k];
		t.hi[k] = l.hi[k];
		t.n[k] = l.n[k];
	}
	const int n_partial = (int)std::min<size_t>(KNN_BOUNDS_BLOCKS, ((size_t)P + 256 * 16 - 1) / (256 * 16));
	knn_bounds_kernel<<<n_partial, 256, 0, stream>>>(P, points, l.partial);
	GSR_LAUNCH_CHECK(0, stream);
	const unsigned blocks = blocks_of((size_t)P);
	knn_morton_kernel<<<blocks, 256, 0, stream>>>(P, n_partial, points, l.partial, l.keys);
	GSR_LAUNCH_CHECK(0, stream);
	GSR_HIP_CHECK(KnnSort::pairs(l.sort_temp, l.sort_bytes, l.keys, l.keys_sorted, rocprim::counting_iterator<uint32_t>(0), l.order, (size_t)P, KNN_MORTON_BITS, stream));
	knn_gather_leaves_kernel<<<blocks, 256, 0, stream>>>(P, points, l.order, l.sorted, l.lo[0], l.hi[0]);
	GSR_LAUNCH_CHECK(0, stream);
	for (int k = 1; k < KNN_LEVELS; k++) {
		knn_parent_boxes_kernel<<<blocks_of((size_t)l.n[k - 1]), 256, 0, stream>>>(l.n[k - 1], l.lo[k - 1], l.hi[k - 1], l.lo[k], l.hi[k]);
		GSR_LAUNCH_CHECK(0, stream);
	}
	knn_search_kernel<<<(unsigned)((l.n[0] + 3) / 4), 256, 0, stream>>>(t, mean_dist);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}
