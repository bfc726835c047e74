// The 11x11 Gaussian-window SSIM, written once for the loss kernels (gsr_loss.hip) and the evaluation metrics (gsr_metrics.hip):
// the window, the 32x32 output tile with its 42x42 zero-padded halo in LDS, the halo loader, the two register-blocked forward
// passes with the evaluation of one output row, and the two adjoint passes of the backwards.  Every device function is inlined
// into the kernel that calls it.  (The sums of the blocks' partials are gsr_reduce.hpp's.)
#pragma once
#include <cmath>
#include "gsr_internal.hpp"

namespace gsr {

#define SSIM_R 5
#define SSIM_T 32                          // output tile: 32 x 32 pixels per workgroup, four per thread
#define SSIM_HALO (SSIM_T + 2 * SSIM_R)   // 42
#define SSIM_B 4                           // outputs per work item along the filtered direction: 4 + 10 loads instead of 4 x 11

struct SsimWindow { float g[2 * SSIM_R + 1]; };

// utils/loss_utils.py:46-48: exp(-(x - 5)^2 / (2 sigma^2)) as float32, normalised by the float32 sum
static SsimWindow make_window() {
	SsimWindow w;
	float sum = 0.f;
	for (int i = 0; i < 11; i++) {
		w.g[i] = (float)exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
		sum += w.g[i];
	}
	for (int i = 0; i < 11; i++) w.g[i] /= sum;
	return w;
}
// the window, made once per process
inline const SsimWindow& ssim_window() {
	static const SsimWindow win = make_window();
	return win;
}
// tiles along an image side of n pixels
inline int ssim_tiles(int n) { return (n + SSIM_T - 1) / SSIM_T; }
// What an entry that launches a (ssim_tiles(W), ssim_tiles(H), planes) grid refuses first: an empty size, then a grid dimension past
// the limit.  `planes_name`: what the entry calls its planes ("C", "planes").  planes_in_grid = false: the kernel loops over them.
static inline int ssim_planes_check(const char* entry, const char* planes_name, int planes, int H, int W, bool planes_in_grid = true) {
	if (planes <= 0 || H <= 0 || W <= 0) { set_error("%s: invalid size %s = %d, H = %d, W = %d", entry, planes_name, planes, H, W); return GSR_E_INVALID; }
	const bool tall = ssim_tiles(H) > 65535;
	if (planes_in_grid && (planes > 65535 || tall)) { set_error("%s: %s and H / 32 are grid dimensions, at most 65535", entry, planes_name); return GSR_E_INVALID; }
	if (tall) { set_error("%s: H / 32 is a grid dimension, at most 65535", entry); return GSR_E_INVALID; }
	return 0;
}

// What the loss and the metrics composite with before they compare: v = rgb * alpha + (1 - alpha) * background[c], and the ground truth
// likewise with gt_mask.  A kernel argument (Presentation of gsr_metrics.hip begins with it).
struct Compositing {
	const float* alpha;      // [H,W] or NULL
	const float* gt_mask;    // [H,W] or NULL
	const float* background; // [C]
};
static inline int compositing_check(const char* entry, const Compositing& cp) {
	if ((cp.alpha || cp.gt_mask) && !cp.background) { set_error("%s: alpha or gt_mask given without a background", entry); return GSR_E_INVALID; }
	return 0;
}
// The three derivative planes of the SSIM map travel together: all three where a backward requires them, otherwise all three or none.
static inline bool derivative_planes_ok(const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12, bool required) {
	const int given = (dm_dmu1 != nullptr) + (dm_dsigma1_sq != nullptr) + (dm_dsigma12 != nullptr);
	return given == 3 || (!required && given == 0);
}

#ifdef __HIPCC__
// Stage the zero-padded halo tiles of NS planes into LDS.  `fetch(in, o, t)` gives the NS values of the pixel at offset o of
// its plane (in: inside the image; outside it must give zeros, the padding).  All of a thread's global loads are issued
// before the first LDS store (the loop is fully unrolled into registers): with three workgroups per CU a
// load-store-load-store sequence leaves the kernel waiting on seven dependent HBM round trips per tile.
#define SSIM_LOADS ((SSIM_HALO * SSIM_HALO + 255) / 256)
template <int NS, class Fetch>
__device__ __forceinline__ void ssim_stage_tiles(Fetch fetch, int H, int W, int x0, int y0, float (*const (&dst)[NS])[SSIM_HALO + 1]) {
	float v[NS][SSIM_LOADS];
#pragma unroll
	for (int j = 0; j < SSIM_LOADS; j++) {
		const int i = threadIdx.x + 256 * j;
		const int ly = i / SSIM_HALO, lx = i - ly * SSIM_HALO;
		const int gx = x0 + lx - SSIM_R, gy = y0 + ly - SSIM_R;
		const bool in = i < SSIM_HALO * SSIM_HALO && gx >= 0 && gx < W && gy >= 0 && gy < H;
		const size_t o = in ? (size_t)gy * W + gx : 0;
		float t[NS];
		fetch(in, o, t);
#pragma unroll
		for (int p = 0; p < NS; p++) v[p][j] = t[p];
	}
#pragma unroll
	for (int j = 0; j < SSIM_LOADS; j++) {
		const int i = threadIdx.x + 256 * j;
		const int ly = i / SSIM_HALO, lx = i - ly * SSIM_HALO;
		if (i < SSIM_HALO * SSIM_HALO) {
#pragma unroll
			for (int p = 0; p < NS; p++) dst[p][ly][lx] = v[p][j];
		}
	}
}
// the planes as they are in memory
template <int NP>
__device__ __forceinline__ void ssim_load_tiles(const float* const (&src)[NP], int H, int W, int x0, int y0, float (*const (&dst)[NP])[SSIM_HALO + 1]) {
	ssim_stage_tiles<NP>([&](bool in, size_t o, float (&t)[NP]) {
#pragma unroll
		for (int p = 0; p < NP; p++) t[p] = in ? src[p][o] : 0.f;
	}, H, W, x0, y0, dst);
}

// Horizontal pass of the five moments: 42 rows x (32 / 4) strips.  A work item produces SSIM_B neighbouring outputs from one
// sliding window of SSIM_B + 10 LDS reads, every output accumulating its eleven taps in the same order.
__device__ __forceinline__ void ssim_moments_hpass(const float (&ta)[SSIM_HALO][SSIM_HALO + 1], const float (&tb)[SSIM_HALO][SSIM_HALO + 1],
                                                   float (&hs)[5][SSIM_HALO][SSIM_T + 1], const SsimWindow& win) {
	for (int i = threadIdx.x; i < SSIM_HALO * (SSIM_T / SSIM_B); i += 256) {
		const int ly = i % SSIM_HALO, lx = (i / SSIM_HALO) * SSIM_B;   // lanes run down the rows: row pitch 43 / 33 words is odd, no bank conflicts
		float a[SSIM_B + 10], b[SSIM_B + 10], aa[SSIM_B + 10], bb[SSIM_B + 10], ab[SSIM_B + 10];
#pragma unroll
		for (int k = 0; k < SSIM_B + 10; k++) {
			a[k] = ta[ly][lx + k]; b[k] = tb[ly][lx + k];
			aa[k] = a[k] * a[k]; bb[k] = b[k] * b[k]; ab[k] = a[k] * b[k];   // once per window element, not once per tap
		}
#pragma unroll
		for (int c = 0; c < SSIM_B; c++) {
			float s1 = 0, s2 = 0, s11 = 0, s22 = 0, s12 = 0;
#pragma unroll
			for (int k = 0; k < 11; k++) {
				const float w = win.g[k];
				s1 += w * a[c + k]; s2 += w * b[c + k]; s11 += w * aa[c + k]; s22 += w * bb[c + k]; s12 += w * ab[c + k];
			}
			hs[0][ly][lx + c] = s1; hs[1][ly][lx + c] = s2; hs[2][ly][lx + c] = s11; hs[3][ly][lx + c] = s22; hs[4][ly][lx + c] = s12;
		}
	}
}
// Vertical pass: thread (tx, tq) owns the four rows 4 tq .. 4 tq + 3 of column tx; its sliding window of every moment
template <int NM>
__device__ __forceinline__ void ssim_load_columns(const float (&hs)[NM][SSIM_HALO][SSIM_T + 1], int tx, int tq, float (&col)[NM][SSIM_B + 10]) {
#pragma unroll
	for (int m = 0; m < NM; m++)
#pragma unroll
		for (int k = 0; k < SSIM_B + 10; k++) col[m][k] = hs[m][tq * SSIM_B + k][tx];
}
// ... and row r of it (utils/loss_utils.py:75-92): the eleven taps of every moment, then ssim = A B / (Cc D).  The three derivatives
// are those of the SSIM value with mu1, E[x^2], E[xy] as the independent conv outputs of image 1 (sigma1^2 = E[x^2] - mu1^2,
// sigma12 = E[xy] - mu1 mu2); a kernel that does not ask for them does not compute them.
struct SsimRow {
	float mu1, mu2, A, B, Cc, D, inv, sv;
	__device__ __forceinline__ float dm_dmu1() const { return 2.f * mu2 * (B - A) * inv - 2.f * mu1 * sv * (D - Cc) * inv; }
	__device__ __forceinline__ float dm_dsigma1_sq() const { return -sv / D; }
	__device__ __forceinline__ float dm_dsigma12() const { return 2.f * A * inv; }
};
__device__ __forceinline__ SsimRow ssim_row(const float (&col)[5][SSIM_B + 10], int r, const SsimWindow& win, float C1, float C2) {
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
	return {mu1, mu2, A, B, Cc, D, inv, A * B * inv};
}

// The adjoint convolutions of the backwards run on three staged planes (the window is symmetric, so the adjoint of the zero-padded
// correlation is the same correlation of the zero-padded planes): the horizontal pass into hs ...
__device__ __forceinline__ void adjoint_hpass(const float (&t0)[SSIM_HALO][SSIM_HALO + 1], const float (&t1)[SSIM_HALO][SSIM_HALO + 1],
                                              const float (&t2)[SSIM_HALO][SSIM_HALO + 1], float (&hs)[3][SSIM_HALO][SSIM_T + 1], const SsimWindow& win) {
	for (int i = threadIdx.x; i < SSIM_HALO * (SSIM_T / SSIM_B); i += 256) {
		const int ly = i % SSIM_HALO, lx = (i / SSIM_HALO) * SSIM_B;   // lanes run down the rows, as in ssim_moments_hpass
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

#endif

}  // namespace gsr
