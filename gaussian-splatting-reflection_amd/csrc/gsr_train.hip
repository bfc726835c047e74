// Training-step kernels around the rasterizer: the Adam update of the reference's eight parameter groups
// (scene/gaussian_model.py:196-209, torch.optim.Adam(lr=0, eps=1e-15)) and the normal-consistency term of its loss.  (The
// photometric loss is gsr_loss.hip.)
//   * Adam: one float4 per lane over ONE flat parameter / gradient / moment buffer (28 B per parameter), learning rate
//     by segment table, so the 59 floats per Gaussian + cubemap update in a single launch.  A streaming, HBM-bound pass.
//   * Raw-parameter step: the same pass with a per-segment activation (sigmoid, exp, normalize): chain rule in, activated copy out.
#include <cstring>
#include "gsr_host.hpp"
#include "../../include/gsr_hip_train.h"   // the raw-parameter step's entries (added under ABI 102, declared apart from gsr_hip.h)
#include "gsr_reduce.hpp"

namespace gsr {

// ---------------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam, amsgrad = False, weight_decay = 0, maximize = False; torch/optim/adam.py _single_tensor_adam):
//   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// One kernel steps every caller.  The raw-parameter step (include/gsr_hip_train.h) has the activation's chain rule in front of adam_one
// and the activation behind it; gsr_adam_step[_range] is that step with every segment GSR_ACT_NONE.  The rasterizer left
// dL/d(activated) in the gradient slots of the activated segments; the activation is recomputed from raw in registers (8 of the
// 59 floats per surfel; the pass stays HBM-bound), the activated copy is only ever written.
// A NORMALIZE4 segment begins at a multiple of 4 and holds whole rows, so one lane's float4 IS one quaternion; an activated segment
// begins at a multiple of 4 in both buffers, so a float4 that lies inside one segment has one aligned float4 destination.
#define ADAM_MAX_SEG 16
#define ACT_KIND_MASK 0xFFu
struct AdamSegs {
	int n;
	unsigned long long end[ADAM_MAX_SEG];   // exclusive end offset of segment i (begin = end[i-1])
	float lr[ADAM_MAX_SEG], lr2[ADAM_MAX_SEG];
	unsigned int period[ADAM_MAX_SEG], split[ADAM_MAX_SEG];
	unsigned int kind[ADAM_MAX_SEG];
	unsigned long long act_begin[ADAM_MAX_SEG];
};
__device__ __forceinline__ int adam_seg(const AdamSegs& s, unsigned long long i) {
	int k = 0;
	while (k + 1 < s.n && i >= s.end[k]) k++;
	return k;
}
__device__ __forceinline__ float adam_lr(const AdamSegs& s, int k, unsigned long long i) {
	const unsigned long long begin = k ? s.end[k - 1] : 0ull;
	if (s.period[k] == 0u) return s.lr[k];
	return ((i - begin) % s.period[k]) < s.split[k] ? s.lr[k] : s.lr2[k];
}
__device__ __forceinline__ float act_value(unsigned int kind, float r) { return kind == GSR_ACT_SIGMOID ? 1.f / (1.f + expf(-r)) : expf(r); }
// dL/d raw of an elementwise activation from dL/d activated (torch's sigmoid_backward: g * (1 - y) * y; exp: g * y)
__device__ __forceinline__ float act_grad(unsigned int kind, float r, float g) {
	const float a = act_value(kind, r);
	return kind == GSR_ACT_SIGMOID ? g * a * (1.f - a) : g * a;
}
// The one definition of the update, and it fixes the roundings: the gradient's product is fused into each moment and the update into the
// parameter, every other operation rounds once.  Under -ffp-contract=fast the compiler would pick which product of `b1 * m + (1 - b1) * g`
// it fuses by the shape of the code around it, so an edit elsewhere in the kernel could move results by an ulp.
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float lr, float b1, float b2, float eps, float bc1,
                                         float sqrt_bc2) {
#pragma clang fp contract(off)
	m = fmaf(1.f - b1, g, b1 * m);
	v = fmaf(1.f - b2, g * g, b2 * v);
	const float denom = sqrtf(v) / sqrt_bc2 + eps;
	p = fmaf(-(lr / bc1), m / denom, p);
}
#define ACT_NORM_EPS 1e-12f     // eps of torch.nn.functional.normalize
__device__ __forceinline__ float4 normalize4(float4 q, float& norm) {
	norm = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
	const float d = fmaxf(norm, ACT_NORM_EPS);
	return make_float4(q.x / d, q.y / d, q.z / d, q.w / d);
}
// STEP: the whole step.  !STEP: act = act(raw) alone (grad and the moments are not touched and may be NULL; FROZEN is ignored).
template <bool STEP>
__global__ void __launch_bounds__(256)
adam_kernel(float* __restrict__ raw, const float* __restrict__ grad, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
            float* __restrict__ act, unsigned long long first, unsigned long long n, AdamSegs segs, float b1, float b2, float eps, float inv_bc1,
            float inv_sqrt_bc2) {
	// (inv_bc1, inv_sqrt_bc2 carry bc1 and sqrt(bc2) themselves: the divisions stay in the kernel, as in torch's addcdiv path)
	// elements [first, n) of the buffers (first is a multiple of 4): a rank that owns one shard of the flat buffer steps only that
	const unsigned long long i4 = first + ((unsigned long long)blockIdx.x * 256 + threadIdx.x) * 4ull;
	if (i4 >= n) return;
	const int k0 = adam_seg(segs, i4);
	if (i4 + 4 <= n && i4 + 4 <= segs.end[k0]) {
		// the float4 lies inside segment k0 (every float4 of a FlatParams layout does: its groups are padded to multiples of 4)
		const unsigned int kind = segs.kind[k0] & ACT_KIND_MASK;
		if (STEP ? (segs.kind[k0] & GSR_ACT_FROZEN) != 0 : kind == GSR_ACT_NONE) return;
		float4 p = *reinterpret_cast<const float4*>(raw + i4);
		if (STEP) {
			float4 g = *reinterpret_cast<const float4*>(grad + i4);
			float4 m = *reinterpret_cast<float4*>(exp_avg + i4), v = *reinterpret_cast<float4*>(exp_avg_sq + i4);
			if (kind == GSR_ACT_NORMALIZE4) {
				float norm;
				const float4 a = normalize4(p, norm);
				if (norm > ACT_NORM_EPS) {
					const float dot = a.x * g.x + a.y * g.y + a.z * g.z + a.w * g.w;
					g = make_float4((g.x - a.x * dot) / norm, (g.y - a.y * dot) / norm, (g.z - a.z * dot) / norm, (g.w - a.w * dot) / norm);
				} else {
					g = make_float4(g.x / ACT_NORM_EPS, g.y / ACT_NORM_EPS, g.z / ACT_NORM_EPS, g.w / ACT_NORM_EPS);
				}
			} else if (kind != GSR_ACT_NONE) {
				g = make_float4(act_grad(kind, p.x, g.x), act_grad(kind, p.y, g.y), act_grad(kind, p.z, g.z), act_grad(kind, p.w, g.w));
			}
			adam_one(p.x, g.x, m.x, v.x, adam_lr(segs, k0, i4), b1, b2, eps, inv_bc1, inv_sqrt_bc2);
			adam_one(p.y, g.y, m.y, v.y, adam_lr(segs, k0, i4 + 1), b1, b2, eps, inv_bc1, inv_sqrt_bc2);
			adam_one(p.z, g.z, m.z, v.z, adam_lr(segs, k0, i4 + 2), b1, b2, eps, inv_bc1, inv_sqrt_bc2);
			adam_one(p.w, g.w, m.w, v.w, adam_lr(segs, k0, i4 + 3), b1, b2, eps, inv_bc1, inv_sqrt_bc2);
			*reinterpret_cast<float4*>(raw + i4) = p;
			*reinterpret_cast<float4*>(exp_avg + i4) = m;
			*reinterpret_cast<float4*>(exp_avg_sq + i4) = v;
			if (kind == GSR_ACT_NONE) return;
		}
		const unsigned long long begin = k0 ? segs.end[k0 - 1] : 0ull;
		float norm;
		const float4 a = kind == GSR_ACT_NORMALIZE4 ? normalize4(p, norm)
		                                            : make_float4(act_value(kind, p.x), act_value(kind, p.y), act_value(kind, p.z), act_value(kind, p.w));
		*reinterpret_cast<float4*>(act + segs.act_begin[k0] + (i4 - begin)) = a;
		return;
	}
	// a float4 across a segment border (segments of a caller that does not pad) or the tail of the buffer: one element at a time.  No
	// element here belongs to a NORMALIZE4 segment: those begin and end at multiples of 4, and so does a range bound other than n.
	const unsigned long long stop = i4 + 4 < n ? i4 + 4 : n;
	for (unsigned long long i = i4; i < stop; i++) {
		const int k = adam_seg(segs, i);
		const unsigned int kind = segs.kind[k] & ACT_KIND_MASK;
		if (kind == GSR_ACT_NORMALIZE4 || (STEP ? (segs.kind[k] & GSR_ACT_FROZEN) != 0 : kind == GSR_ACT_NONE)) continue;
		float p = raw[i];
		if (STEP) {
			float g = grad[i], m = exp_avg[i], v = exp_avg_sq[i];
			if (kind != GSR_ACT_NONE) g = act_grad(kind, p, g);
			adam_one(p, g, m, v, adam_lr(segs, k, i), b1, b2, eps, inv_bc1, inv_sqrt_bc2);
			raw[i] = p; exp_avg[i] = m; exp_avg_sq[i] = v;
			if (kind == GSR_ACT_NONE) continue;
		}
		act[segs.act_begin[k] + (i - (k ? segs.end[k - 1] : 0ull))] = act_value(kind, p);
	}
}

// The checks of the segment table every entry shares, and the device-side table.  Returns 0 or GSR_E_INVALID (message set, naming `entry`).
static int adam_segments(const char* entry, const float* act, uint64_t n, uint64_t n_act, const gsr_act_segment* segments, int num_segments, AdamSegs& s) {
	if (!segments || num_segments < 1 || num_segments > ADAM_MAX_SEG) {
		set_error("%s: invalid argument (NULL segments, or not 1 to 16 of them)", entry);
		return GSR_E_INVALID;
	}
	memset(&s, 0, sizeof(s));
	s.n = num_segments;
	uint64_t prev = 0;
	for (int i = 0; i < num_segments; i++) {
		const gsr_act_segment& g = segments[i];
		if (g.begin != prev || g.end < g.begin || (g.period != 0 && g.split > g.period)) { set_error("%s: segments must tile [0, n) in order", entry); return GSR_E_INVALID; }
		prev = g.end;
		const uint32_t kind = g.kind & ACT_KIND_MASK;
		if ((g.kind & ~(ACT_KIND_MASK | (uint32_t)GSR_ACT_FROZEN)) != 0 || kind > GSR_ACT_NORMALIZE4) {
			set_error("%s: segment %d has an unknown activation kind or flag (%#x)", entry, i, g.kind);
			return GSR_E_INVALID;
		}
		if (kind != GSR_ACT_NONE) {
			const uint64_t len = g.end - g.begin;
			if (!act) { set_error("%s: act is NULL but segment %d is activated", entry, i); return GSR_E_INVALID; }
			if ((g.begin & 3u) != 0 || (g.act_begin & 3u) != 0) {
				set_error("%s: activated segment %d must begin at a multiple of 4 in both buffers", entry, i);
				return GSR_E_INVALID;
			}
			if (kind == GSR_ACT_NORMALIZE4 && (len & 3u) != 0) { set_error("%s: NORMALIZE4 segment %d does not hold whole rows of 4", entry, i); return GSR_E_INVALID; }
			if (g.act_begin > n_act || len > n_act - g.act_begin) { set_error("%s: segment %d does not fit into act (n_act = %llu)", entry, i, (unsigned long long)n_act); return GSR_E_INVALID; }
		}
		s.end[i] = g.end; s.lr[i] = g.lr; s.lr2[i] = g.lr2; s.period[i] = g.period; s.split[i] = g.split;
		s.kind[i] = g.kind; s.act_begin[i] = g.act_begin;
	}
	if (prev != n) { set_error("%s: segments must tile [0, n) in order", entry); return GSR_E_INVALID; }
	return aligned_check(entry, "act", act, 16);
}

// The host side of every Adam entry: all checks, the bias corrections, the one launch.  The buffers are device memory, and exp_avg /
// exp_avg_sq may point in front of their allocation (a caller that keeps moments for its range alone moves them back by range_begin
// elements): nothing is read from them here and the kernel touches [range_begin, range_end) only.
static int adam_step(const char* entry, float* raw, const float* grad, float* exp_avg, float* exp_avg_sq, float* act, uint64_t n, uint64_t n_act,
                     const gsr_act_segment* segments, int num_segments, float beta1, float beta2, float eps, int step, uint64_t range_begin,
                     uint64_t range_end, hipStream_t stream) {
	if (n == 0) return 0;
	if (range_begin > range_end || range_end > n || (range_begin & 3u) != 0 || (range_end != n && (range_end & 3u) != 0)) {
		set_error("%s: [range_begin, range_end) must lie inside [0, n) with multiples of 4 as bounds", entry);
		return GSR_E_INVALID;
	}
	if (!raw || !grad || !exp_avg || !exp_avg_sq || step < 1) { set_error("%s: invalid argument (NULL buffer or step < 1)", entry); return GSR_E_INVALID; }
	if (int rc = pointers_check(entry, {raw, grad, exp_avg, exp_avg_sq}, 16, "buffers")) return rc;
	AdamSegs s;
	if (int rc = adam_segments(entry, act, n, n_act, segments, num_segments, s)) return rc;
	// bias corrections in double on the host, as Python floats are in torch/optim/adam.py
	const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
	if (range_begin == range_end) return 0;
	const unsigned long long nvec = (range_end - range_begin + 3) / 4;
	{
		StageTimer st_(GSR_STAGE_ADAM, stream);
		adam_kernel<true><<<blocks_of(nvec), 256, 0, stream>>>(raw, grad, exp_avg, exp_avg_sq, act, range_begin, range_end, s, beta1, beta2, eps,
		                                                                      (float)bc1, (float)sqrt(bc2));
	}
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

}  // namespace gsr

using namespace gsr;

extern "C" int gsr_adam_act_step(float* raw, const float* grad, float* exp_avg, float* exp_avg_sq, float* act, uint64_t n, uint64_t n_act,
                                 const gsr_act_segment* segments, int num_segments, float beta1, float beta2, float eps, int step,
                                 uint64_t range_begin, uint64_t range_end, void* stream_) {
	return adam_step("gsr_adam_act_step", raw, grad, exp_avg, exp_avg_sq, act, n, n_act, segments, num_segments, beta1, beta2, eps, step, range_begin,
	                 range_end, (hipStream_t)stream_);
}

// gsr_adam_step[_range] (include/gsr_hip.h): the same step with no segment activated
extern "C" int gsr_adam_step_range(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, uint64_t n, const gsr_adam_segment* segments,
                                   int num_segments, float beta1, float beta2, float eps, int step, uint64_t range_begin, uint64_t range_end,
                                   void* stream_) {
	gsr_act_segment table[ADAM_MAX_SEG];
	const bool counted = segments && num_segments >= 1 && num_segments <= ADAM_MAX_SEG;      // (otherwise adam_step refuses the NULL table)
	for (int i = 0; counted && i < num_segments; i++) {
		const gsr_adam_segment& g = segments[i];
		table[i] = gsr_act_segment{g.begin, g.end, g.lr, g.lr2, g.period, g.split, GSR_ACT_NONE, 0};
	}
	return adam_step("gsr_adam_step", param, grad, exp_avg, exp_avg_sq, nullptr, n, 0, counted ? table : nullptr, num_segments, beta1, beta2, eps, step,
	                 range_begin, range_end, (hipStream_t)stream_);
}

extern "C" int gsr_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, uint64_t n, const gsr_adam_segment* segments,
                             int num_segments, float beta1, float beta2, float eps, int step, void* stream_) {
	return gsr_adam_step_range(param, grad, exp_avg, exp_avg_sq, n, segments, num_segments, beta1, beta2, eps, step, 0, n, stream_);
}

extern "C" int gsr_activate(const float* raw, float* act, uint64_t n, uint64_t n_act, const gsr_act_segment* segments, int num_segments, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (n == 0) return 0;
	if (!raw) { set_error("gsr_activate: invalid argument (NULL raw)"); return GSR_E_INVALID; }
	if (int rc = aligned_check("gsr_activate", "raw", raw, 16)) return rc;
	AdamSegs s;
	if (int rc = adam_segments("gsr_activate", act, n, n_act, segments, num_segments, s)) return rc;
	const unsigned long long nvec = (n + 3) / 4;
	{
		StageTimer st_(GSR_STAGE_ADAM, stream);
		adam_kernel<false><<<blocks_of(nvec), 256, 0, stream>>>(const_cast<float*>(raw), nullptr, nullptr, nullptr, act, 0ull, n, s, 0.f, 0.f,
		                                                                           0.f, 1.f, 1.f);
	}
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

// ---- normal-consistency term of the reference's training loss (train.py:182-189):
//   normal_error = (1 - sum_c rend_normal[c] * surf_normal[c]) [* env_scope_mask];  loss = lambda * mean(normal_error)
// five elementwise torch kernels each way at 1080p; here one pass each way.  The forward leaves sum(normal_error) (block
// partials added in a fixed order, in double: bitwise reproducible); the caller scales by lambda / HW.  The backward takes
// the upstream gradient of that SUM as a one-float device tensor (no host synchronisation) and writes both gradients fully.
__global__ void __launch_bounds__(256)
normal_loss_fwd_kernel(const float* __restrict__ rend, const float* __restrict__ surf, const float* __restrict__ mask, size_t HW, float* __restrict__ partials) {
	float acc = 0.f;
	for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < HW; p += (size_t)gridDim.x * 256) {
		float e = 1.0f - (rend[p] * surf[p] + rend[HW + p] * surf[HW + p] + rend[2 * HW + p] * surf[2 * HW + p]);
		if (mask) e *= mask[p];
		acc += e;
	}
	float sums[1] = {acc};
	if (block_sums(sums)) {
		partials[2 * blockIdx.x] = sums[0];
		partials[2 * blockIdx.x + 1] = 0.f;
	}
}
__global__ void __launch_bounds__(256)
normal_loss_bwd_kernel(const float* __restrict__ rend, const float* __restrict__ surf, const float* __restrict__ mask, size_t HW,
                       const float* __restrict__ g_sum, float* __restrict__ g_rend, float* __restrict__ g_surf) {
	const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (p >= HW) return;
	const float g = -g_sum[0] * (mask ? mask[p] : 1.0f);
#pragma unroll
	for (int c = 0; c < 3; c++) {
		const float r = rend[c * HW + p], s = surf[c * HW + p];
		g_rend[c * HW + p] = g * s;
		g_surf[c * HW + p] = g * r;
	}
}
// (both entries keep their own size test, not image_check: they accept H * W from 2^31 on; DESIGN.md, "Out of scope / next")
extern "C" size_t gsr_normal_loss_scratch_floats(void) { return stream_partials(2); }
extern "C" int gsr_normal_loss_forward(const float* rend_normal, const float* surf_normal, const float* mask, int H, int W, float* sum2,
                                       float* scratch, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (H <= 0 || W <= 0 || !rend_normal || !surf_normal || !sum2 || !scratch) { set_error("gsr_normal_loss_forward: invalid argument"); return GSR_E_INVALID; }
	const size_t HW = (size_t)H * W;
	const unsigned blocks = stream_blocks(HW);
	normal_loss_fwd_kernel<<<blocks, 256, 0, stream>>>(rend_normal, surf_normal, mask, HW, scratch);
	sums_reduce_kernel<2, 2><<<1, 256, 0, stream>>>(scratch, (size_t)blocks, sum2);         // sum2[0] = sum(normal_error), sum2[1] = 0
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}
extern "C" int gsr_normal_loss_backward(const float* rend_normal, const float* surf_normal, const float* mask, int H, int W, const float* g_sum,
                                        float* g_rend_normal, float* g_surf_normal, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (H <= 0 || W <= 0 || !rend_normal || !surf_normal || !g_sum || !g_rend_normal || !g_surf_normal) {
		set_error("gsr_normal_loss_backward: invalid argument");
		return GSR_E_INVALID;
	}
	const size_t HW = (size_t)H * W;
	normal_loss_bwd_kernel<<<blocks_of(HW), 256, 0, stream>>>(rend_normal, surf_normal, mask, HW, g_sum, g_rend_normal, g_surf_normal);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}
