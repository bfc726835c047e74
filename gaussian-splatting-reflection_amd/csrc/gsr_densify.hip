// Densification bookkeeping: the reference's adaptive density control (scene/gaussian_model.py:418-584,
// train.py:239-255).  The reference edits every parameter tensor and both Adam moment tensors of every group once per operation
// (prune -> clone -> split -> prune: ~80 boolean-index / cat passes per densification step).  Here ONE row map `new row -> old row`
// is composed per step and applied in ONE streaming gather per flat buffer.  The map is composed either by the host (gsr_densify.py,
// plan="torch": a few P-sized boolean vectors) or on the device by the plan entries at the end of this file
// (include/gsr_hip_densify.h: classify + rank per workgroup, a one-workgroup scan of the workgroup counts, emit); the only arithmetic
// besides the plan's tests is the per-view statistics update and the sampling of split children.
#include "gsr_host.hpp"
#include "../../include/gsr_hip_densify.h"

namespace gsr {

// add_densification_stats (scene/gaussian_model.py:578-584) for row i: `seen` is the reference's update_filter[i].
__device__ __forceinline__ void densify_stats_row(int i, bool seen, const float* __restrict__ grad_means2D, const float* __restrict__ weights,
                                                  float* __restrict__ xyz_gradient_accum, float* __restrict__ denom, float* __restrict__ accum_w,
                                                  float* __restrict__ denom_w) {
	if (seen) {
		const float gx = grad_means2D[3 * i], gy = grad_means2D[3 * i + 1], gz = grad_means2D[3 * i + 2];
		xyz_gradient_accum[i] += sqrtf(gx * gx + gy * gy + gz * gz);   // torch.norm(grad[update_filter], dim=-1)
		denom[i] += 1.0f;
	}
	const float w = weights[i];
	if (w > 0.0f) {
		accum_w[i] += w;
		denom_w[i] += 1.0f;
	}
}

// add_densification_stats + the max_radii2D update of train.py:243, one pass over P.
__global__ void __launch_bounds__(256)
densify_stats_kernel(int P, const float* __restrict__ grad_means2D, const int* __restrict__ radii, const float* __restrict__ weights,
                     float* __restrict__ xyz_gradient_accum, float* __restrict__ denom, float* __restrict__ accum_w, float* __restrict__ denom_w,
                     float* __restrict__ max_radii2D) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= P) return;
	const int r = radii[i];
	densify_stats_row(i, r > 0, grad_means2D, weights, xyz_gradient_accum, denom, accum_w, denom_w);   // visibility_filter = radii > 0
	if (r > 0) max_radii2D[i] = fmaxf(max_radii2D[i], (float)r);
}

// add_densification_stats as the reference calls it, under a boolean filter (torch.bool storage); max_radii2D is the caller's line.
__global__ void __launch_bounds__(256)
densify_stats_filter_kernel(int P, const float* __restrict__ grad_means2D, const uint8_t* __restrict__ update_filter, const float* __restrict__ weights,
                            float* __restrict__ xyz_gradient_accum, float* __restrict__ denom, float* __restrict__ accum_w,
                            float* __restrict__ denom_w) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= P) return;
	densify_stats_row(i, update_filter[i] != 0, grad_means2D, weights, xyz_gradient_accum, denom, accum_w, denom_w);
}

// Row gather over several row-major blocks that share one row map: dst_g[r, :] = map[r] >= 0 ? src_g[map[r], :] : 0.
#define GATHER_MAX_GROUPS 16
struct GatherGroups {
	int n;
	unsigned long long src_off[GATHER_MAX_GROUPS], dst_off[GATHER_MAX_GROUPS];   // float offsets of the blocks
	unsigned int width[GATHER_MAX_GROUPS];                                          // floats per row
	unsigned long long first[GATHER_MAX_GROUPS + 1];                                // prefix of n_rows * width (work items)
};
__global__ void __launch_bounds__(256)
gather_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, const int* __restrict__ row_map, GatherGroups g) {
	const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
	if (t >= g.first[g.n]) return;
	int k = 0;
	while (t >= g.first[k + 1]) k++;
	const unsigned long long e = t - g.first[k];
	const unsigned int w = g.width[k];
	const unsigned long long r = e / w, c = e - r * w;
	const int s = row_map[r];
	dst[g.dst_off[k] + e] = s >= 0 ? src[g.src_off[k] + (unsigned long long)s * w + c] : 0.0f;
}

// Children of densify_and_split (scene/gaussian_model.py:508-534): child j of selected surfel s gets
//   xyz = R(q_s) . (exp(scale_s) * noise_j, 0) + xyz_s,   scaling = log(exp(scale_s) / (0.8 N))
// R = build_rotation (utils/general_utils.py:78-99: quaternion normalised by its norm).  `noise` is standard normal,
// supplied by the caller (the reference draws torch.normal(0, stds) = stds * N(0,1)); S = 2 (surfel) or 3 scale components.
__global__ void __launch_bounds__(256)
split_children_kernel(int n_children, int S, int N, const int* __restrict__ parent, const float* __restrict__ xyz, const float* __restrict__ scaling,
                      const float* __restrict__ rotation, const float* __restrict__ noise, float* __restrict__ child_xyz,
                      float* __restrict__ child_scaling) {
	const int j = blockIdx.x * 256 + threadIdx.x;
	if (j >= n_children) return;
	const int p = parent[j];
	float s[3] = {0.f, 0.f, 0.f}, smp[3] = {0.f, 0.f, 0.f};
	for (int k = 0; k < S; k++) {
		s[k] = expf(scaling[(size_t)p * S + k]);
		smp[k] = s[k] * noise[(size_t)j * S + k];
		child_scaling[(size_t)j * S + k] = logf(s[k] / (0.8f * (float)N));
	}
	const float qr = rotation[4 * (size_t)p], qx = rotation[4 * (size_t)p + 1], qy = rotation[4 * (size_t)p + 2], qz = rotation[4 * (size_t)p + 3];
	const float nrm = sqrtf(qr * qr + qx * qx + qy * qy + qz * qz);
	const float r = qr / nrm, x = qx / nrm, y = qy / nrm, z = qz / nrm;
	const float R00 = 1 - 2 * (y * y + z * z), R01 = 2 * (x * y - r * z), R02 = 2 * (x * z + r * y);
	const float R10 = 2 * (x * y + r * z), R11 = 1 - 2 * (x * x + z * z), R12 = 2 * (y * z - r * x);
	const float R20 = 2 * (x * z - r * y), R21 = 2 * (y * z + r * x), R22 = 1 - 2 * (x * x + y * y);
	child_xyz[3 * (size_t)j] = R00 * smp[0] + R01 * smp[1] + R02 * smp[2] + xyz[3 * (size_t)p];
	child_xyz[3 * (size_t)j + 1] = R10 * smp[0] + R11 * smp[1] + R12 * smp[2] + xyz[3 * (size_t)p + 1];
	child_xyz[3 * (size_t)j + 2] = R20 * smp[0] + R21 * smp[1] + R22 * smp[2] + xyz[3 * (size_t)p + 2];
}

// dst rows that come from a second source: the gather above with `slot` in place of the map and rows with slot < 0 left alone.
__global__ void __launch_bounds__(256)
scatter_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, const int* __restrict__ slot, GatherGroups g) {
	const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
	if (t >= g.first[g.n]) return;
	int k = 0;
	while (t >= g.first[k + 1]) k++;
	const unsigned long long e = t - g.first[k];
	const unsigned int w = g.width[k];
	const unsigned long long r = e / w, c = e - r * w;
	const int s = slot[r];
	if (s >= 0) dst[g.dst_off[k] + e] = src[g.src_off[k] + (unsigned long long)s * w + c];
}

// ------------------------------------------------------------------ the densification plan (include/gsr_hip_densify.h)
// Three launches per pass: classify + rank inside workgroups of PLAN_B rows, a one-workgroup scan of the workgroup counts, emit.
// A rank is the number of rows in front of a row (in index order) that carry the same flag: a wave64 ballot and a popcount of the
// lanes below inside the wave, an LDS prefix over the four waves inside the workgroup, the scanned workgroup counts across
// workgroups.  No atomics, no waiting on another workgroup: positions are the index order, the same run to run.
#define PLAN_B 256
#define PLAN_WAVES (PLAN_B / 64)

// Every thread of the workgroup calls this (rows past the end with all flags false).  Returns the element's word: bits 0-2 the flags,
// bits 8-15 / 16-23 / 24-31 its rank (< 256) under flag 0 / 1 / 2 inside the workgroup; totals[c] = the workgroup's rows with flag c.
__device__ __forceinline__ uint32_t plan_rank(bool f0, bool f1, bool f2, int (*wave_counts)[PLAN_WAVES], int* totals) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const unsigned long long below = (1ull << lane) - 1ull;
	const unsigned long long m0 = __ballot(f0), m1 = __ballot(f1), m2 = __ballot(f2);
	if (lane == 0) {
		wave_counts[0][wave] = __popcll(m0);
		wave_counts[1][wave] = __popcll(m1);
		wave_counts[2][wave] = __popcll(m2);
	}
	__syncthreads();
	int r0 = __popcll(m0 & below), r1 = __popcll(m1 & below), r2 = __popcll(m2 & below);
	int t0 = 0, t1 = 0, t2 = 0;
#pragma unroll
	for (int w = 0; w < PLAN_WAVES; w++) {
		const int c0 = wave_counts[0][w], c1 = wave_counts[1][w], c2 = wave_counts[2][w];
		if (w < wave) { r0 += c0; r1 += c1; r2 += c2; }
		t0 += c0; t1 += c1; t2 += c2;
	}
	totals[0] = t0; totals[1] = t1; totals[2] = t2;
	return (f0 ? 1u : 0u) | (f1 ? 2u : 0u) | (f2 ? 4u : 0u) | ((uint32_t)r0 << 8) | ((uint32_t)r1 << 16) | ((uint32_t)r2 << 24);
}

// max_k expf(row[k]) as torch.exp(...).max(dim=1) gives it: NaN if any term is
__device__ __forceinline__ float plan_max_scale(const float* __restrict__ row, int S) {
	float m = expf(row[0]);
	for (int k = 1; k < S; k++) {
		const float e = expf(row[k]);
		m = (m != m || e != e) ? __int_as_float(0x7fc00000) : fmaxf(m, e);
	}
	return m;
}

// the last prune's test (scene/gaussian_model.py:566-571 without the screen-size term)
__device__ __forceinline__ bool plan_big(const gsr_densify_plan& p, const float* __restrict__ xyz, const float* __restrict__ scale_row) {
	const float m = plan_max_scale(scale_row, p.scale_dims);
	const float dx = xyz[0] - p.mean[0], dy = xyz[1] - p.mean[1], dz = xyz[2] - p.mean[2];
	const bool inside = dx * dx + dy * dy + dz * dz < p.extent2;
	return inside ? m > p.big_near : m > p.big_far;
}

// select, pass 1.  Flags: 0 = survives and is no parent (stays in place), 1 = is cloned, 2 = is a split parent.
__global__ void __launch_bounds__(PLAN_B)
plan_select_kernel(int P, gsr_densify_plan p, const float* __restrict__ grad_accum, const float* __restrict__ denom, const float* __restrict__ accum_w,
                   const float* __restrict__ denom_w, const float* __restrict__ scaling, uint32_t* __restrict__ words, int4* __restrict__ blocks) {
	__shared__ int wave_counts[3][PLAN_WAVES];
	const long long i = (long long)blockIdx.x * PLAN_B + threadIdx.x;
	bool stay = false, clone = false, parent = false;
	if (i < P) {
		const float dw = denom_w[i];
		const float w = dw == 0.0f ? 0.0f : accum_w[i] / dw;
		if (!(w < p.min_weight)) {
			float g = grad_accum[i] / denom[i];
			if (g != g) g = 0.0f;
			const float m = plan_max_scale(scaling + (size_t)i * p.scale_dims, p.scale_dims);
			clone = fabsf(g) >= p.max_grad && m <= p.dense_limit;
			parent = g >= p.max_grad && m > p.dense_limit;
			stay = !parent;
		}
	}
	int totals[3];
	const uint32_t word = plan_rank(stay, clone, parent, wave_counts, totals);
	if (i < P) words[i] = word;
	if (threadIdx.x == 0) blocks[blockIdx.x] = make_int4(totals[0], totals[1], totals[2], 0);
}

// One workgroup: blocks[b] (the counts of workgroup b) becomes their exclusive prefix, PLAN_B workgroups per turn; totals[0..2] = the
// sums.  counts (the entry's int32[4] output): select (`select` != 0): {survivors, clones, parents, 0}; otherwise {kept, dropped,
// kept under flag 2, 0} with dropped = length - kept and length = (sel_totals ? sel_totals[0] + sel_totals[1] : 0) + extra.
__global__ void __launch_bounds__(PLAN_B)
plan_scan_kernel(int nb, int4* __restrict__ blocks, int* __restrict__ totals, int* __restrict__ counts, int select, const int* __restrict__ sel_totals,
                 int extra) {
	__shared__ int wave_sums[3][PLAN_WAVES];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int carry0 = 0, carry1 = 0, carry2 = 0;
	for (int base = 0; base < nb; base += PLAN_B) {
		const int b = base + threadIdx.x;
		const int4 c = b < nb ? blocks[b] : make_int4(0, 0, 0, 0);
		int s0 = c.x, s1 = c.y, s2 = c.z;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const int u0 = __shfl_up(s0, d), u1 = __shfl_up(s1, d), u2 = __shfl_up(s2, d);
			if (lane >= d) { s0 += u0; s1 += u1; s2 += u2; }
		}
		if (lane == 63) { wave_sums[0][wave] = s0; wave_sums[1][wave] = s1; wave_sums[2][wave] = s2; }
		__syncthreads();
		int b0 = carry0, b1 = carry1, b2 = carry2;
#pragma unroll
		for (int w = 0; w < PLAN_WAVES; w++) {
			const int v0 = wave_sums[0][w], v1 = wave_sums[1][w], v2 = wave_sums[2][w];
			if (w < wave) { b0 += v0; b1 += v1; b2 += v2; }
			carry0 += v0; carry1 += v1; carry2 += v2;
		}
		if (b < nb) blocks[b] = make_int4(b0 + s0 - c.x, b1 + s1 - c.y, b2 + s2 - c.z, 0);
		__syncthreads();      // wave_sums is written again in the next turn
	}
	if (threadIdx.x == 0) {
		totals[0] = carry0; totals[1] = carry1; totals[2] = carry2; totals[3] = 0;
		if (select) {
			counts[0] = carry0 + carry2; counts[1] = carry1; counts[2] = carry2; counts[3] = 0;
		} else {
			const int kept = carry0 + carry1 + carry2;
			const int length = (sel_totals ? sel_totals[0] + sel_totals[1] : 0) + extra;
			counts[0] = kept; counts[1] = length - kept; counts[2] = carry2; counts[3] = 0;
		}
	}
}

__global__ void __launch_bounds__(PLAN_B)
plan_emit_parents_kernel(int P, const uint32_t* __restrict__ words, const int4* __restrict__ blocks, int* __restrict__ parents) {
	const long long i = (long long)blockIdx.x * PLAN_B + threadIdx.x;
	if (i >= P) return;
	const uint32_t w = words[i];
	if (w & 4u) parents[blocks[blockIdx.x].z + (int)(w >> 24)] = (int)i;
}

// rows, pass 1: the last prune.  Workgroups [0, nb_rows) take the old rows (an original and its clone are the same surfel: one test),
// the others the children.  Flags: 0 = kept original, 1 = kept clone, 2 = kept child.  Element index: row i, or P + child j.
__global__ void __launch_bounds__(PLAN_B)
plan_rows_kernel(int P, long long n_children, int nb_rows, gsr_densify_plan p, const uint32_t* __restrict__ sel_words, const float* __restrict__ xyz,
                 const float* __restrict__ scaling, const float* __restrict__ child_xyz, const float* __restrict__ child_scaling,
                 uint32_t* __restrict__ words, int4* __restrict__ blocks) {
	__shared__ int wave_counts[3][PLAN_WAVES];
	bool orig = false, clone = false, child = false;
	long long e = -1;
	if ((int)blockIdx.x < nb_rows) {
		const long long i = (long long)blockIdx.x * PLAN_B + threadIdx.x;
		if (i < P) {
			e = i;
			const uint32_t w = sel_words[i];
			if (w & 1u) {
				const bool big = p.size_prune && plan_big(p, xyz + 3 * (size_t)i, scaling + (size_t)i * p.scale_dims);
				orig = !big;
				clone = (w & 2u) && !big;
			}
		}
	} else {
		const long long j = (long long)((int)blockIdx.x - nb_rows) * PLAN_B + threadIdx.x;
		if (j < n_children) {
			e = P + j;
			child = !(p.size_prune && plan_big(p, child_xyz + 3 * (size_t)j, child_scaling + (size_t)j * p.scale_dims));
		}
	}
	int totals[3];
	const uint32_t word = plan_rank(orig, clone, child, wave_counts, totals);
	if (e >= 0) words[e] = word;
	if (threadIdx.x == 0) blocks[blockIdx.x] = make_int4(totals[0], totals[1], totals[2], 0);
}

__global__ void __launch_bounds__(PLAN_B)
plan_emit_rows_kernel(int P, long long n_children, int nb_rows, int k, const uint32_t* __restrict__ words, const int4* __restrict__ blocks,
                      const int* __restrict__ totals, const int* __restrict__ parents, int* __restrict__ map_param, int* __restrict__ map_moment,
                      int* __restrict__ child_of) {
	const int4 off = blocks[blockIdx.x];
	if ((int)blockIdx.x < nb_rows) {
		const long long i = (long long)blockIdx.x * PLAN_B + threadIdx.x;
		if (i >= P) return;
		const uint32_t w = words[i];
		if (w & 1u) {
			const int r = off.x + (int)((w >> 8) & 255u);
			map_param[r] = (int)i; map_moment[r] = (int)i; child_of[r] = -1;
		}
		if (w & 2u) {
			const int r = totals[0] + off.y + (int)((w >> 16) & 255u);
			map_param[r] = (int)i; map_moment[r] = -1; child_of[r] = -1;
		}
	} else {
		const long long j = (long long)((int)blockIdx.x - nb_rows) * PLAN_B + threadIdx.x;
		if (j >= n_children) return;
		const uint32_t w = words[P + j];
		if (w & 4u) {
			const int r = totals[0] + totals[1] + off.z + (int)(w >> 24);
			map_param[r] = parents[j % k]; map_moment[r] = -1; child_of[r] = (int)j;
		}
	}
}

// prune_points: flag 0 = the row stays
__global__ void __launch_bounds__(PLAN_B)
prune_rows_kernel(int P, const uint8_t* __restrict__ remove, uint32_t* __restrict__ words, int4* __restrict__ blocks) {
	__shared__ int wave_counts[3][PLAN_WAVES];
	const long long i = (long long)blockIdx.x * PLAN_B + threadIdx.x;
	const bool keep = i < P && remove[i] == 0;
	int totals[3];
	const uint32_t word = plan_rank(keep, false, false, wave_counts, totals);
	if (i < P) words[i] = word;
	if (threadIdx.x == 0) blocks[blockIdx.x] = make_int4(totals[0], 0, 0, 0);
}
__global__ void __launch_bounds__(PLAN_B)
prune_emit_kernel(int P, const uint32_t* __restrict__ words, const int4* __restrict__ blocks, int* __restrict__ row_map) {
	const long long i = (long long)blockIdx.x * PLAN_B + threadIdx.x;
	if (i >= P) return;
	const uint32_t w = words[i];
	if (w & 1u) row_map[blocks[blockIdx.x].x + (int)((w >> 8) & 255u)] = (int)i;
}

// The caller's scratch, sized for P parents: the select state (rows only reads it) and the state of the last prune.
struct PlanScratch {
	int* totals;          // [0..3] select: stay, clones, parents, 0;  [4..7] rows / prune_points: kept originals, clones, children, 0
	uint32_t* sel_words;  // P
	int4* sel_blocks;     // workgroups of P rows
	uint32_t* words;      // P + N P
	int4* blocks;         // workgroups of P rows + workgroups of N P children
	size_t bytes;
};
static inline size_t plan_blocks(size_t n) { return (n + PLAN_B - 1) / PLAN_B; }
static PlanScratch plan_carve(void* base, size_t P, size_t N) {
	Carver c(base);
	PlanScratch s;
	s.totals = c.take<int>(8);
	s.sel_words = c.take<uint32_t>(P);
	s.sel_blocks = c.take<int4>(plan_blocks(P));
	s.words = c.take<uint32_t>(P + N * P);
	s.blocks = c.take<int4>(plan_blocks(P) + plan_blocks(N * P));
	s.bytes = c.size();
	return s;
}
// (these entries refuse a misaligned scratch before one that is too small, so the alignment is asked first)
static int plan_scratch_check(const char* entry, const void* scratch, size_t scratch_bytes, size_t P, size_t N) {
	if (int rc = aligned_check(entry, "scratch", scratch, 16)) return rc;
	return scratch_check(entry, scratch, scratch_bytes, plan_carve(nullptr, P, N).bytes, "bytes", "gsr_densify_plan_scratch_bytes(P, N)", 16);
}
static inline bool plan_sizes_ok(int P, int N) { return P >= 0 && N >= 1 && (long long)P * ((long long)N + 1) < (1ll << 31); }

// What select and rows refuse alike.  0 to go on (P == 0 included: the caller writes its zero counts), GSR_E_INVALID otherwise.
static int plan_check(const char* entry, int P, const gsr_densify_plan* plan, const void* scratch, size_t scratch_bytes, const int* counts) {
	if (P < 0) { set_error("%s: P = %d", entry, P); return GSR_E_INVALID; }
	if (!plan) { set_error("%s: NULL plan", entry); return GSR_E_INVALID; }
	if (plan->N < 1) { set_error("%s: N = %d children per parent", entry, plan->N); return GSR_E_INVALID; }
	if (plan->scale_dims != 2 && plan->scale_dims != 3) { set_error("%s: scale_dims = %d, not 2 or 3", entry, plan->scale_dims); return GSR_E_INVALID; }
	if (!plan_sizes_ok(P, plan->N)) { set_error("%s: P * (N + 1) reaches 2^31 (P = %d, N = %d)", entry, P, plan->N); return GSR_E_INVALID; }
	if (!(plan->max_grad > 0.0f)) { set_error("%s: max_grad = %g must be positive (a clone enters the split test with gradient 0)", entry, (double)plan->max_grad); return GSR_E_INVALID; }
	if (!counts) { set_error("%s: NULL counts", entry); return GSR_E_INVALID; }
	if (P == 0) return 0;
	if (!scratch) { set_error("%s: NULL scratch", entry); return GSR_E_INVALID; }
	return plan_scratch_check(entry, scratch, scratch_bytes, (size_t)P, (size_t)plan->N);
}

static int fill_gather_groups(const char* entry, uint64_t n_rows, const gsr_gather_group* groups, int num_groups, GatherGroups* g) {
	g->n = num_groups;
	g->first[0] = 0;
	for (int k = 0; k < num_groups; k++) {
		if (groups[k].width == 0) { set_error("%s: zero-width group", entry); return GSR_E_INVALID; }
		g->src_off[k] = groups[k].src_offset; g->dst_off[k] = groups[k].dst_offset; g->width[k] = groups[k].width;
		g->first[k + 1] = g->first[k] + n_rows * (unsigned long long)groups[k].width;
	}
	return 0;
}

}  // namespace gsr

using namespace gsr;

extern "C" int gsr_densification_stats(int P, const float* grad_means2D, const int* radii, const float* gaussian_weights, float* xyz_gradient_accum,
                                       float* denom, float* accum_w, float* denom_w, float* max_radii2D, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (P < 0) { set_error("gsr_densification_stats: invalid argument"); return GSR_E_INVALID; }
	if (P == 0) return 0;
	if (!grad_means2D || !radii || !gaussian_weights || !xyz_gradient_accum || !denom || !accum_w || !denom_w || !max_radii2D) {
		set_error("gsr_densification_stats: NULL buffer");
		return GSR_E_INVALID;
	}
	densify_stats_kernel<<<(P + 255) / 256, 256, 0, stream>>>(P, grad_means2D, radii, gaussian_weights, xyz_gradient_accum, denom, accum_w, denom_w,
	                                                         max_radii2D);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_densification_stats_filter(int P, const float* grad_means2D, const uint8_t* update_filter, const float* gaussian_weights,
                                              float* xyz_gradient_accum, float* denom, float* accum_w, float* denom_w, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (P < 0) { set_error("gsr_densification_stats_filter: P = %d", P); return GSR_E_INVALID; }
	if (P == 0) return 0;
	if (!grad_means2D || !update_filter || !gaussian_weights || !xyz_gradient_accum || !denom || !accum_w || !denom_w) {
		set_error("gsr_densification_stats_filter: NULL buffer");
		return GSR_E_INVALID;
	}
	densify_stats_filter_kernel<<<(P + 255) / 256, 256, 0, stream>>>(P, grad_means2D, update_filter, gaussian_weights, xyz_gradient_accum, denom,
	                                                                accum_w, denom_w);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_gather_rows(const float* src, float* dst, const int* row_map, uint64_t n_rows, const gsr_gather_group* groups, int num_groups,
                               void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (num_groups < 0 || num_groups > GATHER_MAX_GROUPS) { set_error("gsr_gather_rows: at most 16 groups"); return GSR_E_INVALID; }
	if (n_rows == 0 || num_groups == 0) return 0;
	if (!src || !dst || !row_map || !groups) { set_error("gsr_gather_rows: NULL argument"); return GSR_E_INVALID; }
	GatherGroups g;
	if (int rc = fill_gather_groups("gsr_gather_rows", n_rows, groups, num_groups, &g)) return rc;
	const unsigned long long total = g.first[num_groups];
	gather_rows_kernel<<<blocks_of(total), 256, 0, stream>>>(src, dst, row_map, g);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_split_children(int n_children, int scale_dims, int N, const int* parent, const float* xyz, const float* scaling,
                                  const float* rotation, const float* noise, float* child_xyz, float* child_scaling, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (n_children < 0 || (scale_dims != 2 && scale_dims != 3) || N < 1) { set_error("gsr_split_children: invalid argument"); return GSR_E_INVALID; }
	if (n_children == 0) return 0;
	if (!parent || !xyz || !scaling || !rotation || !noise || !child_xyz || !child_scaling) { set_error("gsr_split_children: NULL buffer"); return GSR_E_INVALID; }
	split_children_kernel<<<(n_children + 255) / 256, 256, 0, stream>>>(n_children, scale_dims, N, parent, xyz, scaling, rotation, noise, child_xyz,
	                                                                   child_scaling);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_scatter_rows(const float* src, float* dst, const int* slot, uint64_t n_rows, const gsr_gather_group* groups, int num_groups,
                                void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (num_groups < 0 || num_groups > GATHER_MAX_GROUPS) { set_error("gsr_scatter_rows: at most 16 groups"); return GSR_E_INVALID; }
	if (n_rows == 0 || num_groups == 0) return 0;
	if (!src || !dst || !slot || !groups) { set_error("gsr_scatter_rows: NULL argument"); return GSR_E_INVALID; }
	GatherGroups g;
	if (int rc = fill_gather_groups("gsr_scatter_rows", n_rows, groups, num_groups, &g)) return rc;
	const unsigned long long total = g.first[num_groups];
	scatter_rows_kernel<<<blocks_of(total), 256, 0, stream>>>(src, dst, slot, g);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" size_t gsr_densify_plan_scratch_bytes(int P, int N) {
	return plan_sizes_ok(P, N) ? plan_carve(nullptr, (size_t)P, (size_t)N).bytes : 0;
}

extern "C" int gsr_densify_plan_select(int P, const gsr_densify_plan* plan, const float* xyz_gradient_accum, const float* denom, const float* accum_w,
                                       const float* denom_w, const float* scaling, void* scratch, size_t scratch_bytes, int* counts, int* parents,
                                       void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (int rc = plan_check("gsr_densify_plan_select", P, plan, scratch, scratch_bytes, counts)) return rc;
	if (P == 0) {
		GSR_HIP_CHECK(hipMemsetAsync(counts, 0, 4 * sizeof(int), stream));
		return 0;
	}
	if (!xyz_gradient_accum || !denom || !accum_w || !denom_w || !scaling || !parents) {
		set_error("gsr_densify_plan_select: NULL buffer");
		return GSR_E_INVALID;
	}
	const PlanScratch s = plan_carve(scratch, (size_t)P, (size_t)plan->N);
	const int nb = (int)plan_blocks((size_t)P);
	plan_select_kernel<<<nb, PLAN_B, 0, stream>>>(P, *plan, xyz_gradient_accum, denom, accum_w, denom_w, scaling, s.sel_words, s.sel_blocks);
	GSR_LAUNCH_CHECK(0, stream);
	plan_scan_kernel<<<1, PLAN_B, 0, stream>>>(nb, s.sel_blocks, s.totals, counts, 1, nullptr, 0);
	GSR_LAUNCH_CHECK(0, stream);
	plan_emit_parents_kernel<<<nb, PLAN_B, 0, stream>>>(P, s.sel_words, s.sel_blocks, parents);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_densify_plan_rows(int P, const gsr_densify_plan* plan, void* scratch, size_t scratch_bytes, const float* xyz, const float* scaling,
                                     const int* parents, const float* child_xyz, const float* child_scaling, int k, int* map_param, int* map_moment,
                                     int* child_of, int* counts, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (int rc = plan_check("gsr_densify_plan_rows", P, plan, scratch, scratch_bytes, counts)) return rc;
	if (k < 0 || k > P) { set_error("gsr_densify_plan_rows: k = %d parents of P = %d rows", k, P); return GSR_E_INVALID; }
	if (P == 0) {
		GSR_HIP_CHECK(hipMemsetAsync(counts, 0, 4 * sizeof(int), stream));
		return 0;
	}
	if (!xyz || !scaling || !map_param || !map_moment || !child_of) { set_error("gsr_densify_plan_rows: NULL buffer"); return GSR_E_INVALID; }
	if (k > 0 && (!parents || !child_xyz || !child_scaling)) { set_error("gsr_densify_plan_rows: k = %d with a NULL parents, child_xyz or child_scaling", k); return GSR_E_INVALID; }
	const PlanScratch s = plan_carve(scratch, (size_t)P, (size_t)plan->N);
	const long long n_children = (long long)plan->N * k;      // (<= N P < 2^31)
	const int nb_rows = (int)plan_blocks((size_t)P), nb = nb_rows + (int)plan_blocks((size_t)n_children);
	plan_rows_kernel<<<nb, PLAN_B, 0, stream>>>(P, n_children, nb_rows, *plan, s.sel_words, xyz, scaling, child_xyz, child_scaling, s.words, s.blocks);
	GSR_LAUNCH_CHECK(0, stream);
	plan_scan_kernel<<<1, PLAN_B, 0, stream>>>(nb, s.blocks, s.totals + 4, counts, 0, s.totals, (int)n_children);
	GSR_LAUNCH_CHECK(0, stream);
	plan_emit_rows_kernel<<<nb, PLAN_B, 0, stream>>>(P, n_children, nb_rows, k, s.words, s.blocks, s.totals + 4, parents, map_param, map_moment, child_of);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_prune_rows(int P, const uint8_t* remove, void* scratch, size_t scratch_bytes, int* row_map, int* counts, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (P < 0 || !plan_sizes_ok(P, 1)) { set_error("gsr_prune_rows: P = %d (0 <= P < 2^30)", P); return GSR_E_INVALID; }
	if (!counts) { set_error("gsr_prune_rows: NULL counts"); return GSR_E_INVALID; }
	if (P == 0) {
		GSR_HIP_CHECK(hipMemsetAsync(counts, 0, 4 * sizeof(int), stream));
		return 0;
	}
	if (!remove || !scratch || !row_map) { set_error("gsr_prune_rows: NULL buffer"); return GSR_E_INVALID; }
	if (int rc = plan_scratch_check("gsr_prune_rows", scratch, scratch_bytes, (size_t)P, 1)) return rc;
	const PlanScratch s = plan_carve(scratch, (size_t)P, 1);
	const int nb = (int)plan_blocks((size_t)P);
	prune_rows_kernel<<<nb, PLAN_B, 0, stream>>>(P, remove, s.words, s.blocks);
	GSR_LAUNCH_CHECK(0, stream);
	plan_scan_kernel<<<1, PLAN_B, 0, stream>>>(nb, s.blocks, s.totals + 4, counts, 0, nullptr, P);
	GSR_LAUNCH_CHECK(0, stream);
	prune_emit_kernel<<<nb, PLAN_B, 0, stream>>>(P, s.words, s.blocks, row_map);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}
