// Host-side argument checks shared by the extraction entries (gsr_mesh.hip, gsr_meshclean.hip, gsr_unbounded.hip).  Host code only.
// Every check returns 0 to go on, or GSR_E_INVALID with the message set; `entry` names the caller in the message.  An entry calls them
// in the order in which its header lists the refusals: that order decides which message a doubly wrong call gets.
#pragma once
#include <cmath>
#include <initializer_list>
#include "gsr_internal.hpp"

namespace gsr {

static const uint64_t LIMIT_2_31 = (uint64_t)1 << 31;   // element counts and 32-bit offsets stay below it
static inline bool misaligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) != 0; }
static inline bool positive_finite(float v) { return std::isfinite(v) && v > 0.f; }

// float and int arrays; NULL (an optional array that is absent) passes
static inline int pointers_check(const char* entry, std::initializer_list<const void*> ptrs) {
	for (const void* p : ptrs)
		if (misaligned(p, 4)) { set_error("%s: pointers must be 4-byte aligned (got %p)", entry, p); return GSR_E_INVALID; }
	return 0;
}
// one named buffer: the scratch (16) or the 64-bit counts (8)
static inline int aligned_check(const char* entry, const char* what, const void* p, unsigned to) {
	if (misaligned(p, to)) { set_error("%s: %s must be %u-byte aligned (got %p)", entry, what, to, p); return GSR_E_INVALID; }
	return 0;
}
static inline int image_check(const char* entry, int W, int H) {
	if (W < 1 || H < 1 || (uint64_t)W * (uint64_t)H >= LIMIT_2_31) { set_error("%s: invalid image size %d x %d", entry, W, H); return GSR_E_INVALID; }
	return 0;
}
static inline int points_check(const char* entry, uint64_t n_points) {
	if (n_points >= LIMIT_2_31) { set_error("%s: n_points must be below 2^31 (got %llu)", entry, (unsigned long long)n_points); return GSR_E_INVALID; }
	return 0;
}
// A placement in the world: a positive finite length and a finite position, e.g. ("voxel", "origin") or ("radius", "centre").
static inline int placement_check(const char* entry, const char* length_name, float length, const char* position_name, float x, float y, float z) {
	if (!positive_finite(length)) { set_error("%s: %s must be positive and finite (got %g)", entry, length_name, (double)length); return GSR_E_INVALID; }
	if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) { set_error("%s: the %s is not finite", entry, position_name); return GSR_E_INVALID; }
	return 0;
}

}  // namespace gsr
