// Viewer presentation on the device: what the reference does to a rendered map before it leaves the GPU for its interactive viewer
// (utils/image_utils.py:33-84 render_net_image / colormap / gradient_map, then train.py:334: clamp, times 255, to bytes, to [H,W,3]).
//   * minmax_kernel        pass 1 of a colour-mapped map: global min and max, one order-preserving integer atomic pair per block.
//   * sobel_kernel         gradient_map: both 3x3 Sobel filters from an LDS tile with a one-pixel halo (zero outside the image, after
//                          the affine).  With a colour map it is pass 1: it STORES the magnitude plane and takes its min and max;
//                          without one it presents the magnitude itself.
//   * present_kernel       the one pass of a mode without a colour map, pass 2 of one with: each lane presents four consecutive
//                          pixels of a row, 16-byte loads, 16-byte float stores, twelve bytes as three dwords.  The table lives in
//                          LDS beside its 8-bit form, both filled once per block.
// The colour index is the reference's float32 arithmetic bit for bit: subtract, IEEE divide, multiply, round half to even, each
// rounded on its own.  Contraction is switched off for the whole file (hipcc would turn a * b + c into one rounding).
#include "gsr_host.hpp"
#include <algorithm>

#pragma clang fp contract(off)

namespace gsr {

#define VIEW_MINMAX_BLOCKS 1024
#define VIEW_TILE_W 64          // sobel_kernel: 16 lanes x 4 pixels
#define VIEW_TILE_H 16
#define VIEW_TILE_PITCH (VIEW_TILE_W + 2 + 2)     // halo columns + 2 of padding: rows of 68 floats

// float bits -> unsigned key with the order of the floats (negative values reversed below the positive ones)
__device__ __forceinline__ uint32_t order_key(float v) {
	const uint32_t b = __float_as_uint(v);
	return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
	return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

__device__ __forceinline__ float view_affine(float v, int half) {
	return half ? (v + 1.0f) / 2.0f : v;
}

// min and max of the block's values into slots[0] (the complement of the min's key) and slots[1] (the max's key), both by an integer
// atomic max, so that zero is the identity of both and one memset prepares them; a NaN takes part in neither (fminf / fmaxf).
// Every thread of the 256 calls it.
__device__ __forceinline__ void block_minmax(float mn, float mx, uint32_t* __restrict__ slots) {
	__shared__ float red[2][4];
#pragma unroll
	for (int s = 32; s > 0; s >>= 1) {
		mn = fminf(mn, __shfl_xor(mn, s, 64));
		mx = fmaxf(mx, __shfl_xor(mx, s, 64));
	}
	const int wave = threadIdx.x >> 6;
	if ((threadIdx.x & 63) == 0) { red[0][wave] = mn; red[1][wave] = mx; }
	__syncthreads();
	if (threadIdx.x == 0) {
		mn = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
		mx = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
		atomicMax(&slots[0], ~order_key(mn));
		atomicMax(&slots[1], order_key(mx));
	}
}

__global__ void __launch_bounds__(256) minmax_kernel(const float* __restrict__ src, size_t n, int half, uint32_t* __restrict__ slots) {
	float mn = __int_as_float(0x7f800000), mx = __int_as_float(0xff800000);
	// scalars up to the first 16-byte boundary, float4 from there, scalars after the last whole float4
	const size_t head = std::min<size_t>(n, ((16u - (unsigned)(reinterpret_cast<uintptr_t>(src) & 15u)) & 15u) >> 2);
	const size_t n4 = (n - head) >> 2;
	const float4* const src4 = reinterpret_cast<const float4*>(src + head);
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
		const float4 v = src4[i];
		const float a = view_affine(v.x, half), b = view_affine(v.y, half), c = view_affine(v.z, half), d = view_affine(v.w, half);
		mn = fminf(mn, fminf(fminf(a, b), fminf(c, d)));
		mx = fmaxf(mx, fmaxf(fmaxf(a, b), fmaxf(c, d)));
	}
	if (blockIdx.x == 0) {
		const size_t tail0 = head + 4 * n4;
		const size_t rest = head + (n - tail0);          // at most 3 + 3 values
		if (threadIdx.x < rest) {
			const size_t i = threadIdx.x < head ? threadIdx.x : tail0 + (threadIdx.x - head);
			const float a = view_affine(src[i], half);
			mn = fminf(mn, a);
			mx = fmaxf(mx, a);
		}
	}
	block_minmax(mn, mx, slots);
}

// 8-bit form of one value: trunc(clamp(v, 0, 1) * 255).  fmaxf drops a NaN, so a NaN gives 0.
__device__ __forceinline__ uint32_t byte_of(float v) {
	return (uint32_t)(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f);
}

// n (1..4) pixels of a row starting at pixel p0 of the image: q[i] = r | g << 8 | b << 16
__device__ __forceinline__ void store_pixels_u8(uint8_t* __restrict__ u8, size_t p0, const uint32_t (&q)[4], int n) {
	uint8_t* const o = u8 + 3 * p0;
	if (n == 4 && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) {
		uint32_t* const w = reinterpret_cast<uint32_t*>(o);
		w[0] = q[0] | (q[1] << 24);
		w[1] = (q[1] >> 8) | (q[2] << 16);
		w[2] = (q[2] >> 16) | (q[3] << 8);
	} else {
		for (int i = 0; i < n; i++) {
			o[3 * i] = (uint8_t)q[i];
			o[3 * i + 1] = (uint8_t)(q[i] >> 8);
			o[3 * i + 2] = (uint8_t)(q[i] >> 16);
		}
	}
}
__device__ __forceinline__ void store_pixels_f32(float* __restrict__ o, const float (&v)[4], int n) {
	if (n == 4 && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
		*reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
	} else {
		for (int i = 0; i < n; i++) o[i] = v[i];
	}
}
__device__ __forceinline__ void load_pixels_f32(const float* __restrict__ s, float (&v)[4], int n) {
	if (n == 4 && (reinterpret_cast<uintptr_t>(s) & 15u) == 0) {
		const float4 t = *reinterpret_cast<const float4*>(s);
		v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
	} else {
#pragma unroll
		for (int i = 0; i < 4; i++) v[i] = i < n ? s[i] : 0.0f;
	}
}

// a one-channel result without a colour map: the float plane, and the byte repeated to three channels
__device__ __forceinline__ void present_gray(const float (&v)[4], int n, size_t p0, float* __restrict__ out_f32, uint8_t* __restrict__ out_u8) {
	if (out_f32) store_pixels_f32(out_f32 + p0, v, n);
	if (out_u8) {
		uint32_t q[4];
#pragma unroll
		for (int i = 0; i < 4; i++) q[i] = byte_of(v[i]) * 0x010101u;
		store_pixels_u8(out_u8, p0, q, n);
	}
}

// CIN: channels of src.  LUT: src is one channel (the map itself, or the plane sobel_kernel stored), looked up in the table with the
// min and max of `slots`.  Blocks of 64 x 4 lanes; lane (lx, ly) of block (bx, by) presents pixels 4 * (64 bx + lx) .. + 3 of row
// 4 by + ly.
template <int CIN, bool LUT>
__global__ void __launch_bounds__(256)
present_kernel(const float* __restrict__ src, int H, int W, int half, const float* __restrict__ table, const uint32_t* __restrict__ slots,
               float* __restrict__ out_f32, uint8_t* __restrict__ out_u8, int blocks_x) {
	__shared__ float lut_f[LUT ? 256 * 3 : 1];
	__shared__ uint32_t lut_8[LUT ? 256 : 1];
	if (LUT) {
		const float r = table[3 * threadIdx.x], g = table[3 * threadIdx.x + 1], b = table[3 * threadIdx.x + 2];
		lut_f[3 * threadIdx.x] = r; lut_f[3 * threadIdx.x + 1] = g; lut_f[3 * threadIdx.x + 2] = b;
		lut_8[threadIdx.x] = byte_of(r) | (byte_of(g) << 8) | (byte_of(b) << 16);
		__syncthreads();
	}
	const int bx = blockIdx.x % blocks_x, by = blockIdx.x / blocks_x;
	const int x0 = 4 * (64 * bx + (int)(threadIdx.x & 63)), y = 4 * by + (int)(threadIdx.x >> 6);
	if (x0 >= W || y >= H) return;
	const int n = min(4, W - x0);
	const size_t HW = (size_t)H * W, p0 = (size_t)y * W + x0;
	if (LUT) {
		float v[4];
		load_pixels_f32(src + p0, v, n);
		const float mn = key_value(~slots[0]), mx = key_value(slots[1]);
		const float range = mx - mn;
		const bool flat = !(range > 0.0f);        // max == min (the reference divides by zero), or nothing but NaN
		uint32_t q[4];
		float ch[3][4];
#pragma unroll
		for (int i = 0; i < 4; i++) {
			// colormap(): ((map - min) / (max - min) * 255).round().long(); f2i gives 0 for a NaN
			const float t = (view_affine(v[i], half) - mn) / range;
			const int idx = flat ? 0 : min(255, max(0, f2i(rintf(t * 255.0f))));
			q[i] = lut_8[idx];
			ch[0][i] = lut_f[3 * idx]; ch[1][i] = lut_f[3 * idx + 1]; ch[2][i] = lut_f[3 * idx + 2];
		}
		if (out_f32) {
#pragma unroll
			for (int c = 0; c < 3; c++) store_pixels_f32(out_f32 + c * HW + p0, ch[c], n);
		}
		if (out_u8) store_pixels_u8(out_u8, p0, q, n);
	} else if (CIN == 1) {
		float v[4];
		load_pixels_f32(src + p0, v, n);
#pragma unroll
		for (int i = 0; i < 4; i++) v[i] = view_affine(v[i], half);
		present_gray(v, n, p0, out_f32, out_u8);
	} else {
		uint32_t q[4] = {0, 0, 0, 0};
#pragma unroll
		for (int c = 0; c < 3; c++) {
			float v[4];
			load_pixels_f32(src + c * HW + p0, v, n);
#pragma unroll
			for (int i = 0; i < 4; i++) {
				v[i] = view_affine(v[i], half);
				q[i] |= byte_of(v[i]) << (8 * c);
			}
			if (out_f32) store_pixels_f32(out_f32 + c * HW + p0, v, n);
		}
		if (out_u8) store_pixels_u8(out_u8, p0, q, n);
	}
}

// gradient_map (utils/image_utils.py:33-42): per channel gx, gy = the 3x3 Sobel filters / 4 of the zero-padded image,
// sqrt(gx^2 + gy^2), then the L2 norm over the channels.  Tiles of 64 x 16 pixels, 16 x 16 lanes of four pixels each.
// plane != NULL (a colour map follows): the magnitudes go to `plane` and their min and max to `slots`; otherwise they are presented.
template <int CIN>
__global__ void __launch_bounds__(256)
sobel_kernel(const float* __restrict__ src, int H, int W, int half, float* __restrict__ plane, uint32_t* __restrict__ slots,
             float* __restrict__ out_f32, uint8_t* __restrict__ out_u8, int blocks_x) {
	__shared__ float tile[CIN][VIEW_TILE_H + 2][VIEW_TILE_PITCH];
	const int bx = blockIdx.x % blocks_x, by = blockIdx.x / blocks_x;
	const int tx0 = bx * VIEW_TILE_W, ty0 = by * VIEW_TILE_H;
	const size_t HW = (size_t)H * W;
	for (int e = threadIdx.x; e < (VIEW_TILE_H + 2) * (VIEW_TILE_W + 2); e += 256) {
		const int r = e / (VIEW_TILE_W + 2), c = e - r * (VIEW_TILE_W + 2);
		const int gy = ty0 + r - 1, gx = tx0 + c - 1;
		const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
#pragma unroll
		for (int k = 0; k < CIN; k++) tile[k][r][c] = in ? view_affine(src[k * HW + (size_t)gy * W + gx], half) : 0.0f;
	}
	__syncthreads();
	const int lx = 4 * (int)(threadIdx.x & 15), ly = (int)(threadIdx.x >> 4);
	const int x0 = tx0 + lx, y = ty0 + ly;
	const bool live = x0 < W && y < H;
	float mag[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
	for (int k = 0; k < CIN; k++) {
		float w[3][6];
#pragma unroll
		for (int r = 0; r < 3; r++)
#pragma unroll
			for (int c = 0; c < 6; c++) w[r][c] = tile[k][ly + r][lx + c];
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const float gx = ((w[0][i + 2] - w[0][i]) + 2.0f * (w[1][i + 2] - w[1][i]) + (w[2][i + 2] - w[2][i])) * 0.25f;
			const float gy = ((w[2][i] - w[0][i]) + 2.0f * (w[2][i + 1] - w[0][i + 1]) + (w[2][i + 2] - w[0][i + 2])) * 0.25f;
			const float m = sqrtf(gx * gx + gy * gy);
			mag[i] = CIN == 1 ? m : mag[i] + m * m;
		}
	}
	if (CIN != 1) {
#pragma unroll
		for (int i = 0; i < 4; i++) mag[i] = sqrtf(mag[i]);
	}
	const int n = live ? min(4, W - x0) : 0;
	const size_t p0 = (size_t)y * W + x0;
	if (plane) {
		float mn = __int_as_float(0x7f800000), mx = __int_as_float(0xff800000);
		if (live) {
			store_pixels_f32(plane + p0, mag, n);
#pragma unroll
			for (int i = 0; i < 4; i++) {
				if (i < n) { mn = fminf(mn, mag[i]); mx = fmaxf(mx, mag[i]); }
			}
		}
		block_minmax(mn, mx, slots);
	} else if (live) {
		present_gray(mag, n, p0, out_f32, out_u8);
	}
}

}  // namespace gsr

using namespace gsr;

#define VIEW_FLAGS (GSR_VIEW_HALF | GSR_VIEW_SOBEL | GSR_VIEW_COLORMAP)
#define VIEW_SLOT_FLOATS 4      // ~min key, max key, two words of padding: the stored plane behind them stays 16-byte aligned

extern "C" size_t gsr_present_view_scratch_floats(int C, int H, int W, int flags) {
	if (C <= 0 || H <= 0 || W <= 0 || !(flags & GSR_VIEW_COLORMAP)) return 0;
	return VIEW_SLOT_FLOATS + ((flags & GSR_VIEW_SOBEL) ? (size_t)H * W : 0);
}

extern "C" int gsr_present_view(const float* src, int C, int H, int W, int flags, const float* table, float* out_f32, uint8_t* out_u8,
                                float* scratch, size_t scratch_floats, void* stream_) {
	hipStream_t stream = (hipStream_t)stream_;
	// (its own size test: no SSIM grid here, and W has a limit of its own)
	if (C <= 0 || H <= 0 || W <= 0 || W > (1 << 30)) { set_error("gsr_present_view: invalid size C = %d, H = %d, W = %d", C, H, W); return GSR_E_INVALID; }
	if (C != 1 && C != 3) { set_error("gsr_present_view: C = %d channels, expected 1 or 3", C); return GSR_E_INVALID; }
	if (!src) { set_error("gsr_present_view: NULL src"); return GSR_E_INVALID; }
	if (!out_f32 && !out_u8) { set_error("gsr_present_view: both outputs are NULL"); return GSR_E_INVALID; }
	if (flags & ~VIEW_FLAGS) { set_error("gsr_present_view: unknown flags %d", flags); return GSR_E_INVALID; }
	const bool sobel = (flags & GSR_VIEW_SOBEL) != 0, lut = (flags & GSR_VIEW_COLORMAP) != 0;
	const int half = (flags & GSR_VIEW_HALF) != 0;
	if (lut && C != 1 && !sobel) {
		set_error("gsr_present_view: a colour map needs a one-channel result, got C = %d without GSR_VIEW_SOBEL", C);
		return GSR_E_INVALID;
	}
	if (lut && !table) { set_error("gsr_present_view: GSR_VIEW_COLORMAP without a colour table"); return GSR_E_INVALID; }
	const size_t HW = (size_t)H * W;
	const size_t need = gsr_present_view_scratch_floats(C, H, W, flags);
	if (lut)
		if (int rc = scratch_check("gsr_present_view", scratch, scratch_floats, need, "floats", "gsr_present_view_scratch_floats(C,H,W,flags)", 16)) return rc;
	const size_t bx = blocks_of((size_t)W), by = ((size_t)H + 3) / 4;
	const size_t sx = ((size_t)W + VIEW_TILE_W - 1) / VIEW_TILE_W, sy = ((size_t)H + VIEW_TILE_H - 1) / VIEW_TILE_H;
	if (bx * by > 0x7fffffffu || sx * sy > 0x7fffffffu) { set_error("gsr_present_view: invalid size H = %d, W = %d: more than 2^31 blocks", H, W); return GSR_E_INVALID; }
	uint32_t* const slots = (uint32_t*)scratch;
	float* const plane = (lut && sobel) ? scratch + VIEW_SLOT_FLOATS : nullptr;
	if (lut) GSR_HIP_CHECK(hipMemsetAsync(slots, 0, VIEW_SLOT_FLOATS * sizeof(uint32_t), stream));
	if (sobel) {
		if (C == 1) sobel_kernel<1><<<(unsigned)(sx * sy), 256, 0, stream>>>(src, H, W, half, plane, slots, out_f32, out_u8, (int)sx);
		else sobel_kernel<3><<<(unsigned)(sx * sy), 256, 0, stream>>>(src, H, W, half, plane, slots, out_f32, out_u8, (int)sx);
	} else if (lut) {
		const unsigned blocks = (unsigned)std::min<size_t>(VIEW_MINMAX_BLOCKS, (HW + 1023) / 1024);
		minmax_kernel<<<blocks, 256, 0, stream>>>(src, HW, half, slots);
	}
	const unsigned grid = (unsigned)(bx * by);
	if (lut) {
		// (the stored plane has the affine behind it)
		present_kernel<1, true><<<grid, 256, 0, stream>>>(plane ? plane : src, H, W, plane ? 0 : half, table, slots, out_f32, out_u8, (int)bx);
	} else if (!sobel) {
		if (C == 1) present_kernel<1, false><<<grid, 256, 0, stream>>>(src, H, W, half, nullptr, nullptr, out_f32, out_u8, (int)bx);
		else present_kernel<3, false><<<grid, 256, 0, stream>>>(src, H, W, half, nullptr, nullptr, out_f32, out_u8, (int)bx);
	}
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}
