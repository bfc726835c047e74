// What the wave-per-block tile kernels of both variants share (gsr_gauss.hip, gsr_surfel.hip; one wave owns an 8x8 pixel block of a
// tile and walks the tile's list in batches of WBATCH entries).  The kernels must compile to the instructions they had when each
// spelled these out: change a shape here only with tests/isa_digest.py at hand.
#ifndef GSR_TILE_WALK_HPP
#define GSR_TILE_WALK_HPP
#include "gsr_internal.hpp"

namespace gsr {

#define WBATCH 64         // list entries per batch: one per lane
#define CULL_PAD 0.05f    // the wave's pixel block is padded by this much in the footprint vote (each kernel says why that is enough for its cull record)

// Dispatch slot (xcd_slot) -> tile, quadrant and the block's origin in the image.  The two early returns (slot past the last tile,
// block outside the image) stay in the kernels: reported through this struct they move instructions in variant S.
struct TileBlock { uint32_t tile, quad; int bx0, by0; };
__device__ __forceinline__ TileBlock tile_block(const uint32_t* __restrict__ tile_order, uint32_t slot, int tiles_x) {
	const uint32_t tile = __builtin_amdgcn_readfirstlane(tile_order[slot >> 2]), quad = slot & 3u;   // (readfirstlane: the compiler cannot see that the loaded tile id is wave-uniform)
	const int tile_x = tile % tiles_x, tile_y = tile / tiles_x;
	return TileBlock{tile, quad, tile_x * 16 + (int)(quad & 1) * 8, tile_y * 16 + (int)(quad >> 1) * 8};
}

// Compaction of a batch's hits (mm = their ballot, nh > 0 their number) into the wave's work list: a hit lane parks its two payloads
// in LDS at its ordinal among the hits (kown); lane k < nh picks up those of hit k (0 beyond).  The barrier after the read-back, which
// keeps the next batch's stores behind it, is the caller's.  (Variant S's forward spells this out: see there.)
struct HitList { int kown; uint32_t a, b; };   // kown: meaningful in hit lanes only
__device__ __forceinline__ HitList compact_hits(bool hit, unsigned long long mm, int nh, int lane, uint32_t a, uint32_t b, uint32_t* s_a, uint32_t* s_b) {
	const int kown = __popcll(mm & ((1ull << lane) - 1ull));
	if (hit) {
		s_a[kown] = a;
		s_b[kown] = b;
	}
	__syncthreads();
	return HitList{kown, lane < nh ? s_a[lane] : 0u, lane < nh ? s_b[lane] : 0u};
}

// The record of hit k: wave-uniform, so it arrives through the scalar memory path into SGPRs.  The kernels keep two and ping-pong,
// so that the next record's load stays in flight while the current one is used.
template <int F4> struct TileRec { float4 f[F4]; };
template <int F4>
__device__ __forceinline__ TileRec<F4> fetch_rec(const float4* __restrict__ rec, uint32_t hid, int k) {
	const float4* q = rec + (size_t)__builtin_amdgcn_readlane(hid, k) * F4;
	TileRec<F4> r;
#pragma unroll
	for (int i = 0; i < F4; i++) r.f[i] = q[i];
	return r;
}

}  // namespace gsr
#endif
