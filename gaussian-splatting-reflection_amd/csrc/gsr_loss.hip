// The loss front end of the reference's train loop (train.py:154-174) and the per-pixel gradient of the SSIM map.
//   * photometric_fwd_kernel / photometric_bwd_kernel: when a view carries a gt_alpha_mask the reference composites the ground
//     truth onto the background with the mask (train.py:158) and the render with the rendered alpha (train.py:159), then takes
//     l1_loss and ssim of the two composites.  Here both composites are formed while the 42x42 halo is staged into LDS (as the
//     evaluation metrics do, gsr_metrics.hip), the sums are those of gsr_ssim_l1_forward on the composites, and the backward
//     leaves dL/drgb = alpha dL/dv and dL/dalpha = sum_c (rgb[c] - background[c]) dL/dv[c] in one pass over the channels.
//     Alpha is NOT clamped here (train.py:159 does not; render.py, and so the metrics entry, does).
//     Global traffic per pixel, C = 3: forward 2 C + 2 reads and 3 C writes of 4 B (the composed path adds ~10 plane passes of
//     3 x 4 B each way around the same kernels); backward 5 C + 2 reads, C + 1 writes.
//   * ssim_map_bwd_kernel: dL/dimg1 of an arbitrary reduction of the SSIM map, conv(G p0) + 2 x conv(G p1) + y conv(G p2) with
//     G = dL/dmap: the backward of gsr_train.hip with the upstream gradient multiplied in while the halo is staged.
// Same tile, halo, window and pass structure as the training loss (gsr_ssim.hpp); those kernels are not touched.
#include "gsr_internal.hpp"
#include "gsr_ssim.hpp"

namespace gsr {

struct Compositing {
	const float* alpha;      // [H,W] or NULL: v = rgb * alpha + (1 - alpha) * background[c]
	const float* gt_mask;    // [H,W] or NULL: g = gt * gt_mask + (1 - gt_mask) * background[c]
	const float* background; // [C]
};
// t * a + (1 - a) * bg.  At a == 1 the result is t itself and at a == 0 it is bg, with or without a fused multiply-add.
__device__ __forceinline__ float blend(float t, float a, float bg) { return t * a + (1.0f - a) * bg; }

__global__ void __launch_bounds__(256)
photometric_fwd_kernel(const float* __restrict__ rgb, const float* __restrict__ gt, int H, int W, SsimWindow win, float C1, float C2, Compositing cp,
                       float* __restrict__ partials, float* __restrict__ dm_dmu1, float* __restrict__ dm_dsigma1_sq, float* __restrict__ dm_dsigma12) {
	__shared__ float ta[SSIM_HALO][SSIM_HALO + 1], tb[SSIM_HALO][SSIM_HALO + 1];
	__shared__ float hs[5][SSIM_HALO][SSIM_T + 1];
	__shared__ float red[2][4];
	const size_t plane = (size_t)blockIdx.z * H * W;
	const int x0 = blockIdx.x * SSIM_T, y0 = blockIdx.y * SSIM_T;
	{
		const float* const x = rgb + plane;
		const float* const y = gt + plane;
		const float bg = cp.background ? cp.background[blockIdx.z] : 0.f;
		float (*const dst[2])[SSIM_HALO + 1] = {ta, tb};
		// the padding of the convolution surrounds the COMPOSITED images: outside the image both planes are zero, not the background
		ssim_stage_tiles<2>([&](bool in, size_t o, float (&t)[2]) {
			float v = 0.f, g = 0.f;
			if (in) {
				v = x[o]; g = y[o];
				if (cp.alpha) v = blend(v, cp.alpha[o], bg);
				if (cp.gt_mask) g = blend(g, cp.gt_mask[o], bg);
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
			float mu1 = 0, mu2 = 0, e11 = 0, e22 = 0, e12 = 0;
#pragma unroll
			for (int k = 0; k < 11; k++) {
				const float w = win.g[k];
				mu1 += w * col[0][r + k]; mu2 += w * col[1][r + k];
				e11 += w * col[2][r + k]; e22 += w * col[3][r + k]; e12 += w * col[4][r + k];
			}
			const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
			const float sigma1_sq = e11 - mu1_sq, sigma2_sq = e22 - mu2_sq, sigma12 = e12 - mu12;
			const float A = 2.f * mu12 + C1, B = 2.f * sigma12 + C2, Cc = mu1_sq + mu2_sq + C1, D = sigma1_sq + sigma2_sq + C2;
			const float inv = 1.0f / (Cc * D);
			const float sv = A * B * inv;
			l1 += fabsf(ta[ty + SSIM_R][tx + SSIM_R] - tb[ty + SSIM_R][tx + SSIM_R]);
			ssim_sum += sv;
			if (dm_dmu1) {
				// as ssim_l1_fwd_kernel: mu1, E[v^2], E[vg] are the independent conv outputs of the composited render
				const size_t o = plane + (size_t)gy * W + gx;
				dm_dmu1[o] = 2.f * mu2 * (B - A) * inv - 2.f * mu1 * sv * (D - Cc) * inv;
				dm_dsigma1_sq[o] = -sv / D;
				dm_dsigma12[o] = 2.f * A * inv;
			}
		}
	}
	float r4[4] = {l1, ssim_sum, 0.f, 0.f};
	wave_sum4(r4);
	const int wave = threadIdx.x >> 6;
	if ((threadIdx.x & 63) == 63) { red[0][wave] = r4[0]; red[1][wave] = r4[1]; }
	__syncthreads();
	if (threadIdx.x < 2) {
		const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
		partials[2 * blk + threadIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
	}
}

// second stage: one workgroup adds the blocks' partial pairs in double, in a fixed order -> the sums are bitwise reproducible
__global__ void __launch_bounds__(256) photometric_reduce_kernel(const float* __restrict__ partials, size_t nblocks, float* __restrict__ sums) {
	__shared__ double red[2][256];
	double a = 0.0, b = 0.0;
	for (size_t i = threadIdx.x; i < nblocks; i += 256) { a += (double)partials[2 * i]; b += (double)partials[2 * i + 1]; }
	red[0][threadIdx.x] = a; red[1][threadIdx.x] = b;
	__syncthreads();
	for (int s = 128; s > 0; s >>= 1) {
		if ((int)threadIdx.x < s) { red[0][threadIdx.x] += red[0][threadIdx.x + s]; red[1][threadIdx.x] += red[1][threadIdx.x + s]; }
		__syncthreads();
	}
	if (threadIdx.x == 0) { sums[0] = (float)red[0][0]; sums[1] = (float)red[1][0]; }
}

// The adjoint convolutions both backward kernels run on three staged planes: the horizontal pass into hs ...
__device__ __forceinline__ void adjoint_hpass(const float (&t0)[SSIM_HALO][SSIM_HALO + 1], const float (&t1)[SSIM_HALO][SSIM_HALO + 1],
                                              const float (&t2)[SSIM_HALO][SSIM_HALO + 1], float (&hs)[3][SSIM_HALO][SSIM_T + 1], const SsimWindow& win) {
	for (int i = threadIdx.x; i < SSIM_HALO * (SSIM_T / SSIM_B); i += 256) {
		const int ly = i % SSIM_HALO, lx = (i / SSIM_HALO) * SSIM_B;   // lanes run down the rows: row pitch 43 / 33 words is odd, no bank conflicts
		float v0[SSIM_B + 10], v1[SSIM_B + 10], v2[SSIM_B + 10];
#pragma unroll
		for (int k = 0; k < SSIM_B + 10; k++) { v0[k] = t0[ly][lx + k]; v1[k] = t1[ly][lx + k]; v2[k] = t2[ly][lx + k]; }
#pragma unroll
		for (int c = 0; c < SSIM_B; c++) {
			float s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
			for (int k = 0; k < 11; k++) {
				const float w = win.g[k];
				s0 += w * v0[c + k]; s1 += w * v1[c + k]; s2 += w * v2[c + k];
			}
			hs[0][ly][lx + c] = s0; hs[1][ly][lx + c] = s1; hs[2][ly][lx + c] = s2;
		}
	}
}
// ... and the vertical pass of row r of a thread's column window, combined at the pixel: c0 + 2 x c1 + y c2
__device__ __forceinline__ float adjoint_value(const float (&col)[3][SSIM_B + 10], int r, const SsimWindow& win, float x, float y) {
	float c0 = 0, c1 = 0, c2 = 0;
#pragma unroll
	for (int k = 0; k < 11; k++) {
		const float w = win.g[k];
		c0 += w * col[0][r + k]; c1 += w * col[1][r + k]; c2 += w * col[2][r + k];
	}
	return c0 + 2.f * x * c1 + y * c2;
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

__global__ void __launch_bounds__(256)
ssim_map_bwd_kernel(const float* __restrict__ img1, const float* __restrict__ img2, int H, int W, SsimWindow win, const float* __restrict__ dL_dmap,
                    const float* __restrict__ dm_dmu1, const float* __restrict__ dm_dsigma1_sq, const float* __restrict__ dm_dsigma12,
                    float* __restrict__ dL_dimg1) {
	__shared__ float t0[SSIM_HALO][SSIM_HALO + 1], t1[SSIM_HALO][SSIM_HALO + 1], t2[SSIM_HALO][SSIM_HALO + 1];
	__shared__ float hs[3][SSIM_HALO][SSIM_T + 1];
	const size_t plane = (size_t)blockIdx.z * H * W;
	const int x0 = blockIdx.x * SSIM_T, y0 = blockIdx.y * SSIM_T;
	{
		const float* const G = dL_dmap + plane;
		const float* const p0 = dm_dmu1 + plane;
		const float* const p1 = dm_dsigma1_sq + plane;
		const float* const p2 = dm_dsigma12 + plane;
		float (*const dst[3])[SSIM_HALO + 1] = {t0, t1, t2};
		ssim_stage_tiles<3>([&](bool in, size_t o, float (&t)[3]) {
			const float g = in ? G[o] : 0.f;
			t[0] = in ? g * p0[o] : 0.f; t[1] = in ? g * p1[o] : 0.f; t[2] = in ? g * p2[o] : 0.f;
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
#pragma unroll
	for (int r = 0; r < SSIM_B; r++) {
		const int gy = y0 + tq * SSIM_B + r;
		if (gy >= H) break;
		const size_t o = plane + (size_t)gy * W + gx;
		dL_dimg1[o] = adjoint_value(col, r, win, img1[o], img2[o]);
	}
}

}  // namespace gsr

using namespace gsr;

static int tiles(int n) { return (n + SSIM_T - 1) / SSIM_T; }

extern "C" size_t gsr_photometric_scratch_floats(int C, int H, int W) {
	if (C <= 0 || H <= 0 || W <= 0) return 0;
	return 2 * (size_t)C * tiles(H) * tiles(W);
}

extern "C" int gsr_photometric_forward(const float* rgb, const float* alpha, const float* gt, const float* gt_mask, const float* background, int C,
                                       int H, int W, float C1, float C2, float* sums, float* scratch, float* dm_dmu1, float* dm_dsigma1_sq,
                                       float* dm_dsigma12, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (C <= 0 || H <= 0 || W <= 0) { set_error("gsr_photometric_forward: invalid size C = %d, H = %d, W = %d", C, H, W); return GSR_E_INVALID; }
	if (C > 65535 || tiles(H) > 65535) { set_error("gsr_photometric_forward: C and H / 32 are grid dimensions, at most 65535"); return GSR_E_INVALID; }
	if (!rgb || !gt || !sums || !scratch) { set_error("gsr_photometric_forward: NULL image, sums or scratch"); return GSR_E_INVALID; }
	if ((alpha || gt_mask) && !background) { set_error("gsr_photometric_forward: alpha or gt_mask given without a background"); return GSR_E_INVALID; }
	if (((dm_dmu1 != nullptr) != (dm_dsigma1_sq != nullptr)) || ((dm_dmu1 != nullptr) != (dm_dsigma12 != nullptr))) {
		set_error("gsr_photometric_forward: partial set of derivative planes (all three or none)");
		return GSR_E_INVALID;
	}
	static const SsimWindow win = make_window();
	const Compositing cp = {alpha, gt_mask, background};
	dim3 grid(tiles(W), tiles(H), C);
	{
		StageTimer st_(GSR_STAGE_LOSS_FWD, stream);
		photometric_fwd_kernel<<<grid, 256, 0, stream>>>(rgb, gt, H, W, win, C1, C2, cp, scratch, dm_dmu1, dm_dsigma1_sq, dm_dsigma12);
		photometric_reduce_kernel<<<1, 256, 0, stream>>>(scratch, (size_t)grid.x * grid.y * grid.z, sums);
	}
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_photometric_backward(const float* rgb, const float* alpha, const float* gt, const float* gt_mask, const float* background, int C,
                                        int H, int W, const float* weights, const float* dm_dmu1, const float* dm_dsigma1_sq,
                                        const float* dm_dsigma12, float* dL_drgb, float* dL_dalpha, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (C <= 0 || H <= 0 || W <= 0) { set_error("gsr_photometric_backward: invalid size C = %d, H = %d, W = %d", C, H, W); return GSR_E_INVALID; }
	if (tiles(H) > 65535) { set_error("gsr_photometric_backward: H / 32 is a grid dimension, at most 65535"); return GSR_E_INVALID; }
	if (!rgb || !gt || !weights || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12) {
		set_error("gsr_photometric_backward: NULL image, weights or derivative plane");
		return GSR_E_INVALID;
	}
	if ((alpha || gt_mask) && !background) { set_error("gsr_photometric_backward: alpha or gt_mask given without a background"); return GSR_E_INVALID; }
	if (dL_dalpha && !alpha) { set_error("gsr_photometric_backward: dL_dalpha asked for without alpha"); return GSR_E_INVALID; }
	if (!dL_drgb && !dL_dalpha) return 0;
	static const SsimWindow win = make_window();
	const Compositing cp = {alpha, gt_mask, background};
	dim3 grid(tiles(W), tiles(H), 1);
	{
		StageTimer st_(GSR_STAGE_LOSS_BWD, stream);
		photometric_bwd_kernel<<<grid, 256, 0, stream>>>(rgb, gt, C, H, W, win, cp, weights, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_drgb, dL_dalpha);
	}
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_ssim_map_backward(const float* img1, const float* img2, int planes, int H, int W, const float* dL_dmap, const float* dm_dmu1,
                                     const float* dm_dsigma1_sq, const float* dm_dsigma12, float* dL_dimg1, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	if (planes <= 0 || H <= 0 || W <= 0) { set_error("gsr_ssim_map_backward: invalid size planes = %d, H = %d, W = %d", planes, H, W); return GSR_E_INVALID; }
	if (planes > 65535 || tiles(H) > 65535) { set_error("gsr_ssim_map_backward: planes and H / 32 are grid dimensions, at most 65535"); return GSR_E_INVALID; }
	if (!img1 || !img2 || !dL_dmap || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || !dL_dimg1) {
		set_error("gsr_ssim_map_backward: NULL argument");
		return GSR_E_INVALID;
	}
	static const SsimWindow win = make_window();
	dim3 grid(tiles(W), tiles(H), planes);
	{
		StageTimer st_(GSR_STAGE_LOSS_BWD, stream);
		ssim_map_bwd_kernel<<<grid, 256, 0, stream>>>(img1, img2, H, W, win, dL_dmap, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_dimg1);
	}
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}
