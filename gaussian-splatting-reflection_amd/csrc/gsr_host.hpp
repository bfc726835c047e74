// Host-side argument checks and launch arithmetic shared by every translation unit with a C entry.  Host code only.
// Every check returns 0 to go on, or GSR_E_INVALID with the message set; `entry` names the caller in the message.  An entry calls them
// in the order in which its header lists the refusals: that order decides which message a doubly wrong call gets.
// (The checks that need the SSIM tile, and the compositing triple of the loss and the metrics, are gsr_ssim.hpp's.)
#pragma once
#include <algorithm>
#include <cmath>
#include <initializer_list>
#include "gsr_internal.hpp"

namespace gsr {

static const uint64_t LIMIT_2_31 = (uint64_t)1 << 31;   // element counts and 32-bit offsets stay below it
static inline bool misaligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) != 0; }
static inline bool positive_finite(float v) { return std::isfinite(v) && v > 0.f; }

// Blocks of 256 threads over n elements: one thread per element, or the at most `at_most` blocks of a grid-stride pass.
static inline unsigned blocks_of(size_t n, size_t at_most = SIZE_MAX) { return (unsigned)std::min(at_most, (n + 255) / 256); }
// A streaming pass that leaves one partial per block (gsr_reduce.hpp): its blocks fill the device and one block can add their partials.
// A partial buffer whose size query takes no argument holds `floats_per_block` for the largest such grid.
#define STREAM_BLOCKS_MAX 1024
static inline unsigned stream_blocks(size_t n) { return blocks_of(n, STREAM_BLOCKS_MAX); }
static inline size_t stream_partials(size_t floats_per_block) { return floats_per_block * STREAM_BLOCKS_MAX; }

// a list of arrays, float and int by default; NULL (an optional array that is absent) passes
static inline int pointers_check(const char* entry, std::initializer_list<const void*> ptrs, unsigned to = 4, const char* what = "pointers") {
	for (const void* p : ptrs)
		if (misaligned(p, to)) { set_error("%s: %s must be %u-byte aligned (got %p)", entry, what, to, p); return GSR_E_INVALID; }
	return 0;
}
// One named buffer: float4 arrays (16: the kernels' 128-bit accesses would fault or split sectors) or 64-bit counts and rows (8).  torch
// allocations are 256-byte aligned; VIEWS into a packed buffer (gradient sinks) need not be.  NULL passes.
static inline int aligned_check(const char* entry, const char* what, const void* p, unsigned to) { return pointers_check(entry, {p}, to, what); }
// The caller's scratch: `given` units ("floats", "bytes") at `scratch`, where `query` (the size query, spelt as the caller would call it)
// says `need`; then its alignment.  A NULL scratch holds nothing.
static inline int scratch_check(const char* entry, const void* scratch, size_t given, size_t need, const char* unit, const char* query, unsigned to) {
	if (!scratch) given = 0;
	if (given < need) { set_error("%s: scratch of %zu %s given, %s = %zu needed", entry, given, unit, query, need); return GSR_E_INVALID; }
	return aligned_check(entry, "scratch", scratch, to);
}
static inline int image_check(const char* entry, int W, int H) {
	if (W < 1 || H < 1 || (uint64_t)W * (uint64_t)H >= LIMIT_2_31) { set_error("%s: invalid image size %d x %d", entry, W, H); return GSR_E_INVALID; }
	return 0;
}
static inline int points_check(const char* entry, uint64_t n_points) {
	if (n_points >= LIMIT_2_31) { set_error("%s: n_points must be below 2^31 (got %llu)", entry, (unsigned long long)n_points); return GSR_E_INVALID; }
	return 0;
}
static inline int finite_check(const char* entry, const char* position_name, float x, float y, float z) {
	if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) { set_error("%s: the %s is not finite", entry, position_name); return GSR_E_INVALID; }
	return 0;
}
// A placement in the world: a positive finite length and a finite position, e.g. ("voxel", "origin") or ("radius", "centre").
static inline int placement_check(const char* entry, const char* length_name, float length, const char* position_name, float x, float y, float z) {
	if (!positive_finite(length)) { set_error("%s: %s must be positive and finite (got %g)", entry, length_name, (double)length); return GSR_E_INVALID; }
	return finite_check(entry, position_name, x, y, z);
}

// ------------------------------------------------------------------ the rasterizers' shared checks
// The check of the SH input every forward AND backward makes (through its variant's check_*_inputs): degree 0..3 with (D+1)^2 <= M
// coefficients per row, and rows of a multiple of 16 bytes 16-byte aligned (their float4 loads).  `entry` names the caller in the message.
static inline bool sh_rows_float4(int M, const float* shs) { return shs && ((M * 3) & 3) == 0; }
static inline int check_sh_input(const char* entry, int D, int M, const float* shs) {
	if (D < 0 || D > 3 || (shs && (D + 1) * (D + 1) > M)) { set_error("%s: SH degree %d not supported with M=%d", entry, D, M); return GSR_E_INVALID; }
	return sh_rows_float4(M, shs) ? aligned_check(entry, "shs (rows of a multiple of 16 bytes)", shs, 16) : 0;
}

// What both backward drivers do before their kernels, after the variant's check_*_inputs (the scene, camera and SH tests the forward makes
// too): size check, P == 0 (returns 0: nothing to do), the test of the pointers only the backward has (`missing_pointer`: the caller
// evaluates it, it only compares pointers), 16-byte alignment of what the per-Gaussian pass stores as float4 (`also_aligned`: one more
// such pointer of the variant, or NULL), the forward's buffers carved again, the accumulator zeroed.
// `entry` / `func` name the operation / the driver in the messages.  Returns 1 to go on, < 0 on error.
struct BackwardWorkspace { GeomState geom; ImageState img; BinningState bin; int tiles_x, ntiles; };
static inline int backward_prologue(const char* entry, const char* func, const WorkspaceLayout& layout, int P, int M, int R, int width, int height,
                                    bool missing_pointer, const float* shs, const float* dL_dsh, const float* dL_drot, const float* also_aligned,
                                    const char* also_what, void* geom_buffer, void* binning_buffer, void* image_buffer, hipStream_t stream,
                                    BackwardWorkspace* w) {
	if (P < 0 || R < 0 || width <= 0 || height <= 0) { set_error("%s: invalid size", entry); return GSR_E_INVALID; }
	if (P == 0) return 0;
	if (missing_pointer) { set_error("%s: missing required pointer", entry); return GSR_E_INVALID; }
	if (int rc = aligned_check(func, "dL_dsh", sh_rows_float4(M, shs) ? dL_dsh : nullptr, 16)) return rc;   // (shs itself: check_sh_input)
	if (int rc = aligned_check(func, "dL_drot", dL_drot, 16)) return rc;
	if (int rc = aligned_check(func, also_what, also_aligned, 16)) return rc;
	w->tiles_x = (width + 15) / 16;
	w->ntiles = w->tiles_x * ((height + 15) / 16);
	w->geom = carve_geom(geom_buffer, P, layout, nullptr);
	w->img = carve_image(image_buffer, (size_t)width * height, w->ntiles, layout, nullptr);
	w->bin = carve_binning(binning_buffer, R, w->ntiles, 0, nullptr);
	GSR_HIP_CHECK(hipMemsetAsync(w->geom.acc, 0, (size_t)P * layout.acc_floats * sizeof(float), stream));
	return 1;
}

}  // namespace gsr
