// Evaluation metrics on the device: what the reference computes after training to judge a model.
//   * image_metrics_kernel: metrics.py (PSNR = utils/image_utils.py:20-23, SSIM = utils/loss_utils.py:62-92) on the images as
//     render.py:48-62 presents them: clamp, alpha compositing onto the background, 8-bit quantisation (save_image + to_tensor).
//     Same 32x32 tile, 42x42 zero-padded halo and separable 11x11 window as the training loss (gsr_ssim.hpp), but the images
//     are presented while they are staged into LDS, nothing is kept for a backward, and a view leaves three sums:
//     sum (v - g)^2, sum |v - g| and sum ssim_map.  Global traffic: the reads alone, 8 B per pixel-channel (+ alpha / mask).
//   * normal_mae_kernel: eval_mae.py / utils/mae_utils.py:3-29, the angle between predicted and ground-truth normals.
// Block partials are added in a fixed order in double (block_sums and sums_reduce_kernel of gsr_reduce.hpp) and written to one row
// of a caller-owned table: a test set needs one read-back at its end, and every number is bitwise reproducible.
// Host side: sizes, the compositing triple, the table row and the scratch are checked by gsr_host.hpp and gsr_ssim.hpp.
#include "gsr_host.hpp"
#include "gsr_reduce.hpp"
#include "gsr_ssim.hpp"

namespace gsr {

// torchvision.utils.save_image followed by to_tensor: uint8(clamp(t * 255 + 0.5, 0, 255)) / 255 in float32, every operation
// rounded on its own.  hipcc contracts a * b + c into an FMA by default, which rounds once where torch rounds twice; the _rn
// intrinsics are never contracted, so the 8-bit images are torch's by construction and not by the luck of the inputs.
__device__ __forceinline__ float quantize8(float t) {
	const float s = fminf(fmaxf(__fadd_rn(__fmul_rn(t, 255.0f), 0.5f), 0.0f), 255.0f);
	return __fdiv_rn((float)(unsigned int)s, 255.0f);
}
// render.py:54-56: t * a + (1 - a) * bg, as the four separately rounded float32 operations of the torch expression
__device__ __forceinline__ float composite(float t, float a, float bg) {
	return __fadd_rn(__fmul_rn(t, a), __fmul_rn(__fsub_rn(1.0f, a), bg));
}

struct Presentation {
	Compositing cp;          // (the rendered image is composited with clamp(alpha, 0, 1))
	int clamp, quantize;
};

__global__ void __launch_bounds__(256)
image_metrics_kernel(const float* __restrict__ img, const float* __restrict__ gt, int H, int W, SsimWindow win, float C1, float C2, Presentation pr,
                     float4* __restrict__ partials, uint8_t* __restrict__ img_u8, uint8_t* __restrict__ gt_u8) {
	__shared__ float ta[SSIM_HALO][SSIM_HALO + 1], tb[SSIM_HALO][SSIM_HALO + 1];
	__shared__ float hs[5][SSIM_HALO][SSIM_T + 1];
	const size_t plane = (size_t)blockIdx.z * H * W;
	const int x0 = blockIdx.x * SSIM_T, y0 = blockIdx.y * SSIM_T;
	{
		const float* const x = img + plane;
		const float* const y = gt + plane;
		const float bg = pr.cp.background ? pr.cp.background[blockIdx.z] : 0.f;
		float (*const dst[2])[SSIM_HALO + 1] = {ta, tb};
		// the padding of the convolution surrounds the PRESENTED image: outside the image both planes stay zero
		ssim_stage_tiles<2>([&](bool in, size_t o, float (&t)[2]) {
			float v = 0.f, g = 0.f;
			if (in) {
				v = x[o]; g = y[o];
				if (pr.clamp) v = fminf(fmaxf(v, 0.f), 1.f);
				if (pr.cp.alpha) v = composite(v, fminf(fmaxf(pr.cp.alpha[o], 0.f), 1.f), bg);
				if (pr.cp.gt_mask) g = composite(g, pr.cp.gt_mask[o], bg);
				if (pr.quantize) { v = quantize8(v); g = quantize8(g); }
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
	float sse = 0.f, sad = 0.f, ssim_sum = 0.f;
#pragma unroll
	for (int r = 0; r < SSIM_B; r++) {
		const int ty = tq * SSIM_B + r, gy = y0 + ty;
		if (gx < W && gy < H) {
			const float v = ta[ty + SSIM_R][tx + SSIM_R], g = tb[ty + SSIM_R][tx + SSIM_R];
			const float d = v - g;
			sse += d * d;
			sad += fabsf(d);
			ssim_sum += ssim_row(col, r, win, C1, C2).sv;
			const size_t o = plane + (size_t)gy * W + gx;
			// a presented value is k / 255 rounded once: times 255 it is within 2^-15 of k, so the truncation gives k back
			if (img_u8) img_u8[o] = (uint8_t)(unsigned int)(v * 255.0f + 0.5f);
			if (gt_u8) gt_u8[o] = (uint8_t)(unsigned int)(g * 255.0f + 0.5f);
		}
	}
	float sums[3] = {sse, sad, ssim_sum};
	if (block_sums(sums)) {
		const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
		partials[blk] = make_float4(sums[0], sums[1], sums[2], 0.f);
	}
}

// utils/mae_utils.py:10-27 per pixel, in float32 as torch evaluates it.  A pixel is invalid where a norm is <= eps or the angle
// is NaN (a NaN input: the clamp below would turn a NaN cosine into -1, so the cosine is tested before it).
__global__ void __launch_bounds__(256)
normal_mae_kernel(const float* __restrict__ pred, const float* __restrict__ gt, size_t HW, float pred_div, float gt_div, float eps,
                  float4* __restrict__ partials, float* __restrict__ map) {
	float sum = 0.f, valid = 0.f, invalid = 0.f;
	for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < HW; p += (size_t)gridDim.x * 256) {
		float a[3], b[3];
#pragma unroll
		for (int c = 0; c < 3; c++) {
			a[c] = pred[c * HW + p]; b[c] = gt[c * HW + p];
			if (pred_div != 1.0f) a[c] = __fdiv_rn(a[c], pred_div);
			if (gt_div != 1.0f) b[c] = __fdiv_rn(b[c], gt_div);
		}
		const float dot = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
		const float na = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), nb = sqrtf(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
		const float cs = __fdiv_rn(dot, na * nb + eps);
		const float ang = acosf(fminf(fmaxf(cs, -1.0f), 1.0f)) * 57.29577951308232f;
		const bool bad = na <= eps || nb <= eps || cs != cs;
		if (bad) invalid += 1.f;
		else { valid += 1.f; sum += ang; }
		if (map) map[p] = bad ? __int_as_float(0x7fc00000) : ang;
	}
	// (the counts stay exact in float32: a block of the 1024 sees at most 2^31 / 1024 = 2^21 pixels)
	float sums[3] = {sum, valid, invalid};
	if (block_sums(sums)) partials[blockIdx.x] = make_float4(sums[0], sums[1], sums[2], 0.f);
}

}  // namespace gsr

using namespace gsr;

static size_t image_metrics_blocks(int C, int H, int W) { return (size_t)C * ssim_tiles(H) * ssim_tiles(W); }

extern "C" size_t gsr_image_metrics_scratch_floats(int C, int H, int W) {
	if (C <= 0 || H <= 0 || W <= 0) return 0;
	return 4 * image_metrics_blocks(C, H, W);
}

extern "C" int gsr_image_metrics(const float* img, const float* gt, int C, int H, int W, int flags, const float* alpha, const float* gt_mask,
                                 const float* background, double* row, float* scratch, size_t scratch_floats, uint8_t* img_u8, uint8_t* gt_u8,
                                 void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	const Presentation pr = {{alpha, gt_mask, background}, (flags & GSR_PRESENT_CLAMP) != 0, (flags & GSR_PRESENT_QUANT8) != 0};
	if (int rc = ssim_planes_check("gsr_image_metrics", "C", C, H, W)) return rc;
	if (!img || !gt || !row) { set_error("gsr_image_metrics: NULL image or table row"); return GSR_E_INVALID; }
	if (flags & ~(GSR_PRESENT_CLAMP | GSR_PRESENT_QUANT8)) { set_error("gsr_image_metrics: unknown presentation flags %d", flags); return GSR_E_INVALID; }
	if ((img_u8 || gt_u8) && !(flags & GSR_PRESENT_QUANT8)) {
		set_error("gsr_image_metrics: a uint8 output needs GSR_PRESENT_QUANT8 (it holds the quantised image)");
		return GSR_E_INVALID;
	}
	if (int rc = compositing_check("gsr_image_metrics", pr.cp)) return rc;
	if (int rc = aligned_check("gsr_image_metrics", "the table row", row, 8)) return rc;
	const size_t blocks = image_metrics_blocks(C, H, W);
	if (int rc = scratch_check("gsr_image_metrics", scratch, scratch_floats, 4 * blocks, "floats", "gsr_image_metrics_scratch_floats(C,H,W)", 16)) return rc;
	dim3 grid(ssim_tiles(W), ssim_tiles(H), C);
	image_metrics_kernel<<<grid, 256, 0, stream>>>(img, gt, H, W, ssim_window(), (float)(0.01 * 0.01), (float)(0.03 * 0.03), pr, (float4*)scratch, img_u8, gt_u8);
	sums_reduce_kernel<3, 4, true><<<1, 256, 0, stream>>>(scratch, blocks, row, (double)C * H * W);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" size_t gsr_normal_mae_scratch_floats(int H, int W) {
	if (H <= 0 || W <= 0) return 0;
	return 4 * (size_t)stream_blocks((size_t)H * W);
}

extern "C" int gsr_normal_mae(const float* pred, const float* gt, int H, int W, float pred_divisor, float gt_divisor, float eps, double* row,
                              float* scratch, size_t scratch_floats, float* error_map, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	// (not image_check and positive_finite: H * W from 2^31 on and an infinite divisor are accepted here)
	if (H <= 0 || W <= 0) { set_error("gsr_normal_mae: invalid size H = %d, W = %d", H, W); return GSR_E_INVALID; }
	if (!pred || !gt || !row) { set_error("gsr_normal_mae: NULL normals or table row"); return GSR_E_INVALID; }
	if (!(pred_divisor > 0.f) || !(gt_divisor > 0.f) || !(eps >= 0.f)) { set_error("gsr_normal_mae: divisors must be positive and eps non-negative"); return GSR_E_INVALID; }
	if (int rc = aligned_check("gsr_normal_mae", "the table row", row, 8)) return rc;
	const size_t HW = (size_t)H * W;
	const size_t blocks = stream_blocks(HW);
	if (int rc = scratch_check("gsr_normal_mae", scratch, scratch_floats, 4 * blocks, "floats", "gsr_normal_mae_scratch_floats(H,W)", 16)) return rc;
	normal_mae_kernel<<<(unsigned)blocks, 256, 0, stream>>>(pred, gt, HW, pred_divisor, gt_divisor, eps, (float4*)scratch, error_map);
	sums_reduce_kernel<3, 4, true><<<1, 256, 0, stream>>>(scratch, blocks, row, (double)HW);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}
