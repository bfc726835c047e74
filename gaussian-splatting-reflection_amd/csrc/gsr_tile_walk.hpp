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

// The box the footprint vote tests an entry against: the bounding box of the centres of the block's pixels that have not retired, padded by
// CULL_PAD.  A retired pixel (and one outside the image: `done` from the start) never blends again, so an entry that reaches only such pixels is
// an empty pair whatever the vote says; the forward's outputs do not change, its evaluated pairs do (tests/vote_px_stats.py: 4.52 M -> 4.27 M at C3).
// The box is wave-uniform and only shrinks.  refresh() runs before a batch's vote and rebuilds it only if `done` has changed since it was
// built: the lane mask is folded to column bits and row bits of the block with scalar shifts and ORs (~20 scalar instructions, no cross-lane
// traffic) and the first and last set bit of each give the extent.  SUB4: lanes map to pixels by sub_px / sub_py (variant S: a 16-lane row is
// a 4x4 sub-block); otherwise row-major (px = lane & 7, py = lane >> 3; variant G).  Requires a live pixel (done != ~0: the kernels leave first).
template <bool SUB4>
struct LiveBox {
	lmask from;             // the `done` this box was built from
	float x0, x1, y0, y1;
	__device__ __forceinline__ LiveBox(float qx0, float qy0) : from(0ull), x0(qx0 - CULL_PAD), x1(qx0 + 7.0f + CULL_PAD), y0(qy0 - CULL_PAD), y1(qy0 + 7.0f + CULL_PAD) {}
	__device__ __forceinline__ void refresh(lmask done, float qx0, float qy0) {
		if (done == from) return;
		from = done;
		const lmask live = ~done;
		const uint32_t lo = (uint32_t)live, hi = (uint32_t)(live >> 32);
		uint32_t c = lo | hi, cols;
		int r0, r1;
		if (SUB4) {          // lane = py[2] px[2] py[1:0] px[1:0]
			const uint32_t rows = ((lo | (lo >> 16)) & 0xffffu) | ((hi | (hi >> 16)) << 16);   // bit 4 * py + (px & 3)
			r0 = __builtin_ctz(rows) >> 2;
			r1 = (31 - __builtin_clz(rows)) >> 2;
			c |= c >> 8;
			c |= c >> 4;     // bits 0..3: px 0..3, bits 16..19: px 4..7
			cols = (c & 0xfu) | ((c >> 12) & 0xf0u);
		} else {             // lane = py[2:0] px[2:0]: the first and the last live lane lie in the first and the last live row
			r0 = __builtin_ctzll(live) >> 3;
			r1 = (63 - __builtin_clzll(live)) >> 3;
			c |= c >> 16;
			c |= c >> 8;
			cols = c & 0xffu;
		}
		x0 = qx0 + (float)__builtin_ctz(cols) - CULL_PAD;
		x1 = qx0 + (float)(31 - __builtin_clz(cols)) + CULL_PAD;
		y0 = qy0 + (float)r0 - CULL_PAD;
		y1 = qy0 + (float)r1 + CULL_PAD;
	}
};

// Development counter of evaluated (wave, entry) pairs (dev option bit 2, gsr_internal.hpp): the COUNT instances of the forward tile kernels
// take the word's address as their last argument and add each wave's number to it with one atomic at exit; with dev bit 4 they also keep the
// vote's box at the whole block, which is the count the live box is compared with.  The production instances take the empty struct: no
// argument, no register, no instruction.
template <bool COUNT> struct PairCount { __device__ __forceinline__ bool whole_block() const { return false; } };
template <> struct PairCount<true> {
	unsigned long long* word;
	int block;
	__device__ __forceinline__ bool whole_block() const { return block != 0; }
};

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
