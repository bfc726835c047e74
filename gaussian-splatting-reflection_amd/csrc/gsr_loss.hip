// The photometric loss of the reference's train loop (train.py:154-174: (1 - lambda) * L1 + lambda * (1 - SSIM),
// utils/loss_utils.py:40-97) and the per-pixel gradient of the SSIM map.  Streaming, HBM/LDS-bound passes: one 32x32 output tile
// per workgroup; the 42x42 halo of both images is staged in LDS once, the 11x11 Gaussian window (sigma 1.5, zero padding 5:
// F.conv2d(padding=5, groups=C)) is applied separably to the five moment planes x, y, x^2, y^2, xy from LDS, and the forward leaves
// only what a backward needs: the three partial-derivative planes of the SSIM map and two block-reduced sums.  The passes
// themselves are gsr_ssim.hpp's, shared with the evaluation metrics.
//   * loss_fwd_kernel<COMPOSITE>: gsr_ssim_l1_forward runs the plain instantiation, ~8 B read + 12 B written per pixel-channel.
//     When a view carries a gt_alpha_mask the reference composites the ground truth onto the background with the mask
//     (train.py:158) and the render with the rendered alpha (train.py:159), then takes l1_loss and ssim of the two composites:
//     gsr_photometric_forward with a plane runs the compositing instantiation, which forms both composites while the halo is
//     staged (as the evaluation metrics do, gsr_metrics.hip), and without one the plain instantiation.
//     Alpha is NOT clamped here (train.py:159 does not; render.py, and so the metrics entry, does).
//   * plane_bwd_kernel<PER_PIXEL>: dL/dimg1 per plane, under the two sums' scalar weights (gsr_ssim_l1_backward) or under a
//     per-pixel gradient of the SSIM map (gsr_ssim_map_backward: an arbitrary reduction of the map).
//   * photometric_bwd_kernel: the backward of the composites, dL/drgb = alpha dL/dv and dL/dalpha = sum_c (rgb[c] - background[c])
//     dL/dv[c] in one pass over the channels.  Global traffic per pixel, C = 3: forward 2 C + 2 reads and 3 C writes of 4 B (the
//     composed path adds ~10 plane passes of 3 x 4 B each way around the same kernels); backward 5 C + 2 reads, C + 1 writes.
// Host side: the SSIM grid's limits, the compositing triple and the derivative planes are checked by gsr_ssim.hpp.
#include "gsr_host.hpp"
#include "gsr_reduce.hpp"
#include "gsr_ssim.hpp"

namespace gsr {

// t * a + (1 - a) * bg.  At a == 1 the result is t itself and at a == 0 it is bg, with or without a fused multiply-add.
__device__ __forceinline__ float blend(float t, float a, float bg) { return t * a + (1.0f - a) * bg; }

// Forward: per-pixel SSIM and |x - y|, block-reduced into one partial pair per block (L1, SSIM); optionally the SSIM map and the
// three planes d ssim / d mu1, d ssim / d E[x^2], d ssim / d E[xy] for the backward.  Both separable passes are register-blocked: a
// work item produces SSIM_B neighbouring outputs from one sliding window of SSIM_B + 10 LDS reads (the kernel is LDS-read bound:
// 29 reads per output pixel instead of 90), every output still accumulating its eleven taps in the same order.
template <bool COMPOSITE>
__global__ void __launch_bounds__(256)
loss_fwd_kernel(const float* __restrict__ img1, const float* __restrict__ img2, int H, int W, SsimWindow win, float C1, float C2, Compositing cp,
                float* __restrict__ partials, float* __restrict__ ssim_map, float* __restrict__ dm_dmu1, float* __restrict__ dm_dsigma1_sq,
                float* __restrict__ dm_dsigma12) {
	__shared__ float ta[SSIM_HALO][SSIM_HALO + 1], tb[SSIM_HALO][SSIM_HALO + 1];
	__shared__ float hs[5][SSIM_HALO][SSIM_T + 1];
	const size_t plane = (size_t)blockIdx.z * H * W;
	const int x0 = blockIdx.x * SSIM_T, y0 = blockIdx.y * SSIM_T;
	{
		const float* const x = img1 + plane;
		const float* const y = img2 + plane;
		const float bg = COMPOSITE && cp.background ? cp.background[blockIdx.z] : 0.f;
		float (*const dst[2])[SSIM_HALO + 1] = {ta, tb};
		// the padding of the convolution surrounds the COMPOSITED images: outside the image both planes are zero, not the background
		ssim_stage_tiles<2>([&](bool in, size_t o, float (&t)[2]) {
			float v = 0.f, g = 0.f;
			if (in) {
				v = x[o]; g = y[o];
				if (COMPOSITE && cp.alpha) v = blend(v, cp.alpha[o], bg);
				if (COMPOSITE && cp.gt_mask) g = blend(g, cp.gt_mask[o], bg);
			}
			t[0] = v; t[1] = g;
		}, H, W, x0, y0, dst);
	}
	__syncthreads();
	ssim_moments_hpass(ta, tb, hs, win);
	__syncthreads();
	const int tx = threadIdx.x & 31, tq = threadIdx.x >> 5;
	const int gx = x0 + tx;
	float col[5][SSIM_B + 10];
	ssim_load_columns<5>(hs, tx, tq, col);
	float l1 = 0.f, ssim_sum = 0.f;
#pragma unroll
	for (int r = 0; r < SSIM_B; r++) {
		const int ty = tq * SSIM_B + r, gy = y0 + ty;
		if (gx < W && gy < H) {
			const SsimRow s = ssim_row(col, r, win, C1, C2);
			const size_t o = plane + (size_t)gy * W + gx;
			l1 += fabsf(ta[ty + SSIM_R][tx + SSIM_R] - tb[ty + SSIM_R][tx + SSIM_R]);
			ssim_sum += s.sv;
			if (ssim_map) ssim_map[o] = s.sv;
			if (dm_dmu1) {
				dm_dmu1[o] = s.dm_dmu1();
				dm_dsigma1_sq[o] = s.dm_dsigma1_sq();
				dm_dsigma12[o] = s.dm_dsigma12();
			}
		}
	}
	// one partial pair per block; sums_reduce_kernel adds them up in a fixed order
	float sums[2] = {l1, ssim_sum};
	if (block_sums(sums)) {
		const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
		partials[2 * blk] = sums[0];
		partials[2 * blk + 1] = sums[1];
	}
}

// Backward of one plane: dL/dimg1 = w_l1 * sign(x - y) + w_ssim * [ conv(p0) + 2 x conv(p1) + y conv(p2) ] with the three derivative
// planes p of the forward and upstream = the two weights {dL/d(sum |x-y|), dL/d(sum ssim)}; or, PER_PIXEL, upstream = G = dL/dmap
// per pixel, multiplied in while the halo is staged: dL/dimg1 = conv(G p0) + 2 x conv(G p1) + y conv(G p2).
template <bool PER_PIXEL>
__global__ void __launch_bounds__(256)
plane_bwd_kernel(const float* __restrict__ img1, const float* __restrict__ img2, int H, int W, SsimWindow win, const float* __restrict__ upstream,
                 const float* __restrict__ dm_dmu1, const float* __restrict__ dm_dsigma1_sq, const float* __restrict__ dm_dsigma12,
                 float* __restrict__ dL_dimg1) {
	__shared__ float t0[SSIM_HALO][SSIM_HALO + 1], t1[SSIM_HALO][SSIM_HALO + 1], t2[SSIM_HALO][SSIM_HALO + 1];
	__shared__ float hs[3][SSIM_HALO][SSIM_T + 1];
	const size_t plane = (size_t)blockIdx.z * H * W;
	const int x0 = blockIdx.x * SSIM_T, y0 = blockIdx.y * SSIM_T;
	{
		const float* const G = PER_PIXEL ? upstream + plane : nullptr;
		const float* const src[3] = {dm_dmu1 + plane, dm_dsigma1_sq + plane, dm_dsigma12 + plane};
		float (*const dst[3])[SSIM_HALO + 1] = {t0, t1, t2};
		ssim_stage_tiles<3>([&](bool in, size_t o, float (&t)[3]) {
			const float g = PER_PIXEL && in ? G[o] : 0.f;
#pragma unroll
			for (int p = 0; p < 3; p++) t[p] = !in ? 0.f : PER_PIXEL ? g * src[p][o] : src[p][o];
		}, H, W, x0, y0, dst);
	}
	__syncthreads();
	adjoint_hpass(t0, t1, t2, hs, win);
	__syncthreads();
	const int tx = threadIdx.x & 31, tq = threadIdx.x >> 5;
	const int gx = x0 + tx;
	if (gx >= W) return;
	float col[3][SSIM_B + 10];
	ssim_load_columns<3>(hs, tx, tq, col);
	const float w_l1 = PER_PIXEL ? 0.f : upstream[0], w_ssim = PER_PIXEL ? 1.f : upstream[1];
#pragma unroll
	for (int r = 0; r < SSIM_B; r++) {
		const int gy = y0 + tq * SSIM_B + r;
		if (gy >= H) break;
		const size_t o = plane + (size_t)gy * W + gx;
		const float x = img1[o], y = img2[o];
		const float adj = adjoint_value(col, r, win, x, y);
		if (PER_PIXEL) {
			dL_dimg1[o] = adj;
		} else {
			const float d = x - y;
			const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);   // torch.abs backward: sign(), 0 at 0
			dL_dimg1[o] = w_l1 * sgn + w_ssim * adj;
		}
	}
}

// One workgroup per tile, looping over the channels: dL/dalpha sums over them, so a thread keeps the sums of its four pixels in
// registers and stores them once (no atomics: the plane is bitwise reproducible).  v and g are recomputed at the pixel.
__global__ void __launch_bounds__(256)
photometric_bwd_kernel(const float* __restrict__ rgb, const float* __restrict__ gt, int C, int H, int W, SsimWindow win, Compositing cp,
                       const float* __restrict__ weights /* [2]: dL/d(sum |v-g|), dL/d(sum ssim) */, const float* __restrict__ dm_dmu1,
                       const float* __restrict__ dm_dsigma1_sq, const float* __restrict__ dm_dsigma12, float* __restrict__ dL_drgb,
                       float* __restrict__ dL_dalpha) {
	__shared__ float t0[SSIM_HALO][SSIM_HALO + 1], t1[SSIM_HALO][SSIM_HALO + 1], t2[SSIM_HALO][SSIM_HALO + 1];
	__shared__ float hs[3][SSIM_HALO][SSIM_T + 1];
	const size_t HW = (size_t)H * W;
	const int x0 = blockIdx.x * SSIM_T, y0 = blockIdx.y * SSIM_T;
	const int tx = threadIdx.x & 31, tq = threadIdx.x >> 5;
	const int gx = x0 + tx;
	const float w_l1 = weights[0], w_ssim = weights[1];
	bool live[SSIM_B];
	size_t px[SSIM_B];
	float a[SSIM_B], m[SSIM_B], acc[SSIM_B];
#pragma unroll
	for (int r = 0; r < SSIM_B; r++) {
		const int gy = y0 + tq * SSIM_B + r;
		live[r] = gx < W && gy < H;
		px[r] = live[r] ? (size_t)gy * W + gx : 0;
		a[r] = live[r] && cp.alpha ? cp.alpha[px[r]] : 1.f;
		m[r] = live[r] && cp.gt_mask ? cp.gt_mask[px[r]] : 1.f;
		acc[r] = 0.f;
	}
	for (int c = 0; c < C; c++) {
		const size_t plane = (size_t)c * HW;
		{
			const float* const src[3] = {dm_dmu1 + plane, dm_dsigma1_sq + plane, dm_dsigma12 + plane};
			float (*const dst[3])[SSIM_HALO + 1] = {t0, t1, t2};
			// (no barrier before restaging: the tiles were last read by the horizontal pass, which the barrier after it closed, and
			// hs, which the vertical pass below reads, is next written after the barrier that follows this staging)
			ssim_load_tiles<3>(src, H, W, x0, y0, dst);
		}
		__syncthreads();
		adjoint_hpass(t0, t1, t2, hs, win);
		__syncthreads();
		float col[3][SSIM_B + 10];
		ssim_load_columns<3>(hs, tx, tq, col);
		const float bg = cp.background ? cp.background[c] : 0.f;
#pragma unroll
		for (int r = 0; r < SSIM_B; r++) {
			if (!live[r]) continue;
			const size_t o = plane + px[r];
			const float x = rgb[o];
			float v = x, g = gt[o];
			if (cp.alpha) v = blend(v, a[r], bg);
			if (cp.gt_mask) g = blend(g, m[r], bg);
			const float d = v - g;
			const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);   // torch.abs backward: sign(), 0 at 0
			const float dv = w_l1 * sgn + w_ssim * adjoint_value(col, r, win, v, g);
			if (dL_drgb) dL_drgb[o] = cp.alpha ? a[r] * dv : dv;
			acc[r] += (x - bg) * dv;
		}
	}
	if (dL_dalpha) {
#pragma unroll
		for (int r = 0; r < SSIM_B; r++)
			if (live[r]) dL_dalpha[px[r]] = acc[r];
	}
}

}  // namespace gsr

using namespace gsr;

// the two forward entries' launches: the compositing instantiation only where there is a plane to composite with
static void launch_loss_forward(const float* img1, const float* img2, int C, int H, int W, float C1, float C2, const Compositing& cp, float* sums,
                                float* scratch, float* ssim_map, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, hipStream_t stream) {
	dim3 grid(ssim_tiles(W), ssim_tiles(H), C);
	StageTimer st_(GSR_STAGE_LOSS_FWD, stream);
	auto* const kernel = cp.alpha || cp.gt_mask ? loss_fwd_kernel<true> : loss_fwd_kernel<false>;
	kernel<<<grid, 256, 0, stream>>>(img1, img2, H, W, ssim_window(), C1, C2, cp, scratch, ssim_map, dm_dmu1, dm_dsigma1_sq, dm_dsigma12);
	sums_reduce_kernel<2, 2><<<1, 256, 0, stream>>>(scratch, (size_t)grid.x * grid.y * grid.z, sums);
}
template <bool PER_PIXEL>
static void launch_plane_backward(const float* img1, const float* img2, int planes, int H, int W, const float* upstream, const float* dm_dmu1,
                                  const float* dm_dsigma1_sq, const float* dm_dsigma12, float* dL_dimg1, hipStream_t stream) {
	dim3 grid(ssim_tiles(W), ssim_tiles(H), planes);
	StageTimer st_(GSR_STAGE_LOSS_BWD, stream);
	plane_bwd_kernel<PER_PIXEL><<<grid, 256, 0, stream>>>(img1, img2, H, W, ssim_window(), upstream, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_dimg1);
}

static size_t partial_pairs_floats(int C, int H, int W) {
	if (C <= 0 || H <= 0 || W <= 0) return 0;
	return 2 * (size_t)C * ssim_tiles(H) * ssim_tiles(W);
}
extern "C" size_t gsr_ssim_l1_scratch_floats(int C, int H, int W) { return partial_pairs_floats(C, H, W); }
extern "C" size_t gsr_photometric_scratch_floats(int C, int H, int W) { return partial_pairs_floats(C, H, W); }

extern "C" int gsr_ssim_l1_forward(const float* img1, const float* img2, int C, int H, int W, float C1, float C2, float* sums, float* scratch,
                                   float* ssim_map, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (C < 0 || H < 0 || W < 0 || !sums) { set_error("gsr_ssim_l1_forward: invalid argument"); return GSR_E_INVALID; }
	if (C == 0 || H == 0 || W == 0) { GSR_HIP_CHECK(hipMemsetAsync(sums, 0, 2 * sizeof(float), stream)); return 0; }
	if (!scratch) { set_error("gsr_ssim_l1_forward: scratch of gsr_ssim_l1_scratch_floats(C,H,W) floats is required"); return GSR_E_INVALID; }
	if (!img1 || !img2 || !derivative_planes_ok(dm_dmu1, dm_dsigma1_sq, dm_dsigma12, false)) {
		set_error("gsr_ssim_l1_forward: NULL image or partial set of derivative planes");
		return GSR_E_INVALID;
	}
	launch_loss_forward(img1, img2, C, H, W, C1, C2, Compositing{nullptr, nullptr, nullptr}, sums, scratch, ssim_map, dm_dmu1, dm_dsigma1_sq, dm_dsigma12,
	                    stream);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_ssim_l1_backward(const float* img1, const float* img2, int C, int H, int W, const float* weights, const float* dm_dmu1,
                                    const float* dm_dsigma1_sq, const float* dm_dsigma12, float* dL_dimg1, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (C < 0 || H < 0 || W < 0) { set_error("gsr_ssim_l1_backward: invalid argument"); return GSR_E_INVALID; }
	if (C == 0 || H == 0 || W == 0) return 0;
	if (!img1 || !img2 || !weights || !derivative_planes_ok(dm_dmu1, dm_dsigma1_sq, dm_dsigma12, true) || !dL_dimg1) {
		set_error("gsr_ssim_l1_backward: NULL argument");
		return GSR_E_INVALID;
	}
	launch_plane_backward<false>(img1, img2, C, H, W, weights, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_dimg1, stream);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_photometric_forward(const float* rgb, const float* alpha, const float* gt, const float* gt_mask, const float* background, int C,
                                       int H, int W, float C1, float C2, float* sums, float* scratch, float* dm_dmu1, float* dm_dsigma1_sq,
                                       float* dm_dsigma12, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	const Compositing cp = {alpha, gt_mask, background};
	if (int rc = ssim_planes_check("gsr_photometric_forward", "C", C, H, W)) return rc;
	if (!rgb || !gt || !sums || !scratch) { set_error("gsr_photometric_forward: NULL image, sums or scratch"); return GSR_E_INVALID; }
	if (int rc = compositing_check("gsr_photometric_forward", cp)) return rc;
	if (!derivative_planes_ok(dm_dmu1, dm_dsigma1_sq, dm_dsigma12, false)) {
		set_error("gsr_photometric_forward: partial set of derivative planes (all three or none)");
		return GSR_E_INVALID;
	}
	launch_loss_forward(rgb, gt, C, H, W, C1, C2, cp, sums, scratch, nullptr, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, stream);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_photometric_backward(const float* rgb, const float* alpha, const float* gt, const float* gt_mask, const float* background, int C,
                                        int H, int W, const float* weights, const float* dm_dmu1, const float* dm_dsigma1_sq,
                                        const float* dm_dsigma12, float* dL_drgb, float* dL_dalpha, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	const Compositing cp = {alpha, gt_mask, background};
	if (int rc = ssim_planes_check("gsr_photometric_backward", "C", C, H, W, false)) return rc;      // (the kernel loops over the channels)
	if (!rgb || !gt || !weights || !derivative_planes_ok(dm_dmu1, dm_dsigma1_sq, dm_dsigma12, true)) {
		set_error("gsr_photometric_backward: NULL image, weights or derivative plane");
		return GSR_E_INVALID;
	}
	if (int rc = compositing_check("gsr_photometric_backward", cp)) return rc;
	if (dL_dalpha && !alpha) { set_error("gsr_photometric_backward: dL_dalpha asked for without alpha"); return GSR_E_INVALID; }
	if (!dL_drgb && !dL_dalpha) return 0;
	dim3 grid(ssim_tiles(W), ssim_tiles(H), 1);
	{
		StageTimer st_(GSR_STAGE_LOSS_BWD, stream);
		photometric_bwd_kernel<<<grid, 256, 0, stream>>>(rgb, gt, C, H, W, ssim_window(), cp, weights, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_drgb, dL_dalpha);
	}
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_ssim_map_backward(const float* img1, const float* img2, int planes, int H, int W, const float* dL_dmap, const float* dm_dmu1,
                                     const float* dm_dsigma1_sq, const float* dm_dsigma12, float* dL_dimg1, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (int rc = ssim_planes_check("gsr_ssim_map_backward", "planes", planes, H, W)) return rc;
	if (!img1 || !img2 || !dL_dmap || !derivative_planes_ok(dm_dmu1, dm_dsigma1_sq, dm_dsigma12, true) || !dL_dimg1) {
		set_error("gsr_ssim_map_backward: NULL argument");
		return GSR_E_INVALID;
	}
	launch_plane_backward<true>(img1, img2, planes, H, W, dL_dmap, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_dimg1, stream);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}
