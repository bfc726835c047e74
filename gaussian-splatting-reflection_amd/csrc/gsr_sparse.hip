// The block-sparse TSDF volume (include/gsr_hip_sparse.h has the contracts): the dense volume of gsr_mesh.hip cut into blocks of 8 x 8 x 8
// nodes, of which only those near the surface get storage.  A direct table (one int32 per block of the box) names each block's slot in
// a pool of 2 KiB planes; nothing is hashed, nothing probes, and no kernel uses a global atomic or waits for another workgroup.
//
//   touch       one view: block -> -2 where a node within one node of the view's truncation band lies in it.  A workgroup takes one block
//               (four waves, two 8 x 8 slices each), ORs the 27-bit masks of its band nodes and stores -2 into the blocks the mask names.
//               A block whose box lies behind the camera or outside the image leaves before the node loop.
//   allocate    count (-2 entries per 256 table entries) -> spine (gsr_scan.hpp) -> assign (slot = allocated + exclusive rank, ascending
//               block index; writes the table and block_of_slot below capacity) -> finish (the two counts)
//   integrate   one view into the slots: a wave owns one slot and walks its eight slices, so every plane access is one 256-byte row;
//               the projection is tsdf_integrate_kernel's, call for call
//   extract     the five passes of gsr_mesh.hip over the POOL in slot order, 256 pool nodes (half a slot) per workgroup; the neighbours
//               of a node that lie in another block are found through the table, whose 27 (count) or 8 (emit) entries around the block
//               go to LDS once per workgroup
// The case table, the tetrahedra and the edge numbering are those of gsr_mesh.hip (include/gsr_hip_mesh.h states them), restated here
// because the dense translation unit is not to change; tests hold both to tests/mesh_ref.py.
#include "gsr_host.hpp"
#include "gsr_scan.hpp"
#include "gsr_view.hpp"
#include "../../include/gsr_hip_sparse.h"

namespace gsr {

#define SP_BLOCK_NODES 512u       // 8 x 8 x 8
#define SP_MAX_GRID 65536u        // workgroups per launch of touch and integrate; the kernels stride over the rest
#define SP_UNTOUCHED (-1)
#define SP_WAITING (-2)

// the block grid of a volume
struct BlockGrid {
	int nx, ny, nz;
	uint32_t gx, gy, gz, G;
};
__device__ __forceinline__ void block_ijk(uint32_t b, const BlockGrid& g, int& bi, int& bj, int& bk) {
	const uint32_t row = b / g.gx;
	bi = (int)(b - row * g.gx);
	bk = (int)(row / g.gy);
	bj = (int)(row - (uint32_t)bk * g.gy);
}

// ------------------------------------------------------------------------------------------------------------ touch
struct TouchArgs {
	int32_t* table;
	const float* depth; const float* alpha;
	const float* view; const float* proj;
	BlockGrid g;
	int W, H;
	float ox, oy, oz, voxel, alpha_min, sdf_trunc, depth_trunc;
};

// The largest value a linear form c . (X, Y, Z, 1) takes over the box of half-side `h` about `p`, plus a margin of 1e-4 of the sum of
// its terms' magnitudes: three orders above what float32 loses in the four fused multiply-adds, so a block is only given up when every
// node of it fails the test by far.
__device__ __forceinline__ float form_max(float c0, float c1, float c2, float c3, const float* p, float h) {
	const float at = fmaf(c0, p[0], fmaf(c1, p[1], fmaf(c2, p[2], c3)));
	const float spread = h * (fabsf(c0) + fabsf(c1) + fabsf(c2));
	const float mag = fabsf(c0 * p[0]) + fabsf(c1 * p[1]) + fabsf(c2 * p[2]) + fabsf(c3) + spread;
	return at + spread + 1e-4f * mag;
}

// true when no node of the block about `p` can pass steps 1-2: z <= 0 or p.w <= 0 everywhere, or the whole box projects off one side
// of the image (for p.w > 0: u < 0 <=> p.x + p.w < 0, u >= W <=> p.w - p.x <= 0, and likewise v).  NaN compares false: no skip.
__device__ __forceinline__ bool block_unseen(const ViewRows& r, const float* p, float h) {
	if (form_max(r.V[0], r.V[1], r.V[2], r.V[3], p, h) < 0.f) return true;
	if (form_max(r.P[8], r.P[9], r.P[10], r.P[11], p, h) < 0.f) return true;
#pragma unroll
	for (int a = 0; a < 2; a++) {
		const float* q = r.P + 4 * a;
		if (form_max(q[0] + r.P[8], q[1] + r.P[9], q[2] + r.P[10], q[3] + r.P[11], p, h) < 0.f) return true;
		if (form_max(r.P[8] - q[0], r.P[9] - q[1], r.P[10] - q[2], r.P[11] - q[3], p, h) < 0.f) return true;
	}
	return false;
}

__global__ void __launch_bounds__(256)
sparse_touch_kernel(const TouchArgs a) {
	__shared__ uint32_t lds[4];
	const ViewRows r(a.view, a.proj);
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int li = lane & 7, lj = lane >> 3;
	for (uint32_t b = blockIdx.x; b < a.g.G; b += gridDim.x) {
		int bi, bj, bk;
		block_ijk(b, a.g, bi, bj, bk);
		const float centre[3] = {fmaf(a.voxel, 8.f * (float)bi + 3.5f, a.ox), fmaf(a.voxel, 8.f * (float)bj + 3.5f, a.oy),
		                         fmaf(a.voxel, 8.f * (float)bk + 3.5f, a.oz)};
		if (block_unseen(r, centre, 3.51f * a.voxel)) continue;               // (the same for every thread of the workgroup)
		const int i = bi * 8 + li, j = bj * 8 + lj;
		uint32_t mask = 0;          // bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1): the block at that offset holds a node next to a band node
		if (i < a.g.nx && j < a.g.ny) {
			const float X = fmaf(a.voxel, (float)i, a.ox), Y = fmaf(a.voxel, (float)j, a.oy);
			const ViewDots xy = r.xy(X, Y);
			// the blocks along x and y that hold an existing node within one node: bit 0 = the one below, 1 = this, 2 = the one above
			const uint32_t mx = 2u | (li == 0 && i > 0 ? 1u : 0u) | (li == 7 && i + 1 < a.g.nx ? 4u : 0u);
			const uint32_t my = 2u | (lj == 0 && j > 0 ? 1u : 0u) | (lj == 7 && j + 1 < a.g.ny ? 4u : 0u);
			const uint32_t plane = ((my & 1u) ? mx : 0u) | (mx << 3) | ((my & 4u) ? mx << 6 : 0u);
#pragma unroll
			for (int s = 0; s < 2; s++) {
				const int lk = wave + 4 * s, k = bk * 8 + lk;
				if (k >= a.g.nz) continue;
				const float Z = fmaf(a.voxel, (float)k, a.oz);
				const float z = r.z(xy, Z), pw = r.w(xy, Z);
				if (!(z > 0.f && pw > 0.f)) continue;
				const float fx = ((r.x(xy, Z) / pw + 1.f) * (float)a.W - 1.f) * 0.5f;
				const float fy = ((r.y(xy, Z) / pw + 1.f) * (float)a.H - 1.f) * 0.5f;
				const float ru = rintf(fx), rv = rintf(fy);
				if (!(ru >= 0.f && ru < (float)a.W && rv >= 0.f && rv < (float)a.H)) continue;
				const size_t pix = (size_t)(int)rv * a.W + (int)ru;
				const float d = a.depth[pix];
				if (!(d > 0.f && d <= a.depth_trunc)) continue;
				if (a.alpha && !(a.alpha[pix] >= a.alpha_min)) continue;
				const float sdf = d - z;
				if (!(sdf >= -a.sdf_trunc && sdf < a.sdf_trunc)) continue;
				mask |= (lk == 0 && k > 0 ? plane : 0u) | (plane << 9) | (lk == 7 && k + 1 < a.g.nz ? plane << 18 : 0u);
			}
		}
#pragma unroll
		for (int s = 1; s < 64; s <<= 1) mask |= __shfl_xor(mask, s);
		if (lane == 0) lds[wave] = mask;
		__syncthreads();
		mask = lds[0] | lds[1] | lds[2] | lds[3];
		__syncthreads();
		if (threadIdx.x < 27 && ((mask >> threadIdx.x) & 1u)) {
			// (in the grid: the bit was set for a node that exists)
			const int dx = (int)(threadIdx.x % 3u) - 1, dy = (int)((threadIdx.x / 3u) % 3u) - 1, dz = (int)(threadIdx.x / 9u) - 1;
			const uint32_t nb = (uint32_t)(((bk + dz) * (int)a.g.gy + (bj + dy)) * (long long)a.g.gx + (bi + dx));
			if (a.table[nb] == SP_UNTOUCHED) a.table[nb] = SP_WAITING;
		}
	}
}

// ------------------------------------------------------------------------------------------------------------ allocate
struct AllocScratch {
	uint32_t* part;        // nblocks  waiting entries per 256 table entries
	uint32_t* vbase;       // nblocks  waiting entries in front of the block
	uint32_t* tbase;       // nblocks  (the spine's second count: not used)
	unsigned long long* total;   // 2  the spine's totals
	size_t bytes;
	uint32_t nblocks;
};
static AllocScratch alloc_carve(void* base, uint64_t G) {
	Carver c(base);
	AllocScratch s;
	s.nblocks = (uint32_t)((G + SCAN_BLOCK - 1) / SCAN_BLOCK);
	s.part = c.take<uint32_t>(s.nblocks);
	s.vbase = c.take<uint32_t>(s.nblocks);
	s.tbase = c.take<uint32_t>(s.nblocks);
	s.total = c.take<unsigned long long>(2);
	s.bytes = c.size();
	return s;
}

__global__ void __launch_bounds__(SCAN_BLOCK)
alloc_count_kernel(const int32_t* __restrict__ table, uint32_t G, uint32_t* __restrict__ part) {
	__shared__ uint32_t lds[4];
	const uint32_t n = blockIdx.x * SCAN_BLOCK + threadIdx.x;
	const uint32_t sum = block_sum(n < G && table[n] == SP_WAITING ? 1u : 0u, lds);
	if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(SCAN_BLOCK)
alloc_assign_kernel(int32_t* __restrict__ table, uint32_t G, const uint32_t* __restrict__ vbase, const unsigned long long* __restrict__ counts,
                    unsigned long long capacity, int32_t* __restrict__ block_of_slot) {
	__shared__ uint32_t lds[4];
	const uint32_t n = blockIdx.x * SCAN_BLOCK + threadIdx.x;
	const bool waiting = n < G && table[n] == SP_WAITING;
	const uint32_t ex = block_exclusive(waiting ? 1u : 0u, lds);
	if (!waiting) return;
	const unsigned long long slot = counts[0] + vbase[blockIdx.x] + ex;
	if (slot < capacity) {
		table[n] = (int32_t)slot;
		block_of_slot[slot] = (int32_t)n;
	}
}

__global__ void alloc_finish_kernel(const unsigned long long* __restrict__ total, unsigned long long capacity, unsigned long long* __restrict__ counts) {
	const unsigned long long wanted = counts[0] + total[0];
	counts[0] = wanted < capacity ? wanted : capacity;
	counts[1] = wanted;
}

// ------------------------------------------------------------------------------------------------------------ integrate
struct SparseTsdfArgs {
	const int32_t* block_of_slot;
	float* tsdf; float* weight; float* color;
	const float* depth; const float* rgb; const float* alpha;
	const float* view; const float* proj;
	BlockGrid g;
	int W, H;
	float ox, oy, oz, voxel, alpha_min, sdf_trunc, depth_trunc;
	uint32_t n_slots;
};

__global__ void __launch_bounds__(256)
sparse_integrate_kernel(const SparseTsdfArgs a) {
	const ViewRows r(a.view, a.proj);
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int li = lane & 7, lj = lane >> 3;
	for (uint32_t s = blockIdx.x * 4u + (uint32_t)wave; s < a.n_slots; s += gridDim.x * 4u) {
		const uint32_t b = (uint32_t)a.block_of_slot[s];
		if (b >= a.g.G) continue;                                      // (not a block of this volume: nothing of the slot is touched)
		int bi, bj, bk;
		block_ijk(b, a.g, bi, bj, bk);
		const int i = bi * 8 + li, j = bj * 8 + lj;
		if (i >= a.g.nx || j >= a.g.ny) continue;                      // a node of an edge block that does not exist
		const int k0 = bk * 8, k1 = min(k0 + 8, a.g.nz);
		const float X = fmaf(a.voxel, (float)i, a.ox), Y = fmaf(a.voxel, (float)j, a.oy);
		const ViewDots xy = r.xy(X, Y);
		const size_t slot0 = (size_t)s * SP_BLOCK_NODES;               // < 2^31
		uint32_t local = (uint32_t)lane;
#pragma unroll 2
		for (int k = k0; k < k1; k++, local += 64u) {
			const float Z = fmaf(a.voxel, (float)k, a.oz);
			const float z = r.z(xy, Z), pw = r.w(xy, Z);
			if (!(z > 0.f && pw > 0.f)) continue;
			const float fx = ((r.x(xy, Z) / pw + 1.f) * (float)a.W - 1.f) * 0.5f;
			const float fy = ((r.y(xy, Z) / pw + 1.f) * (float)a.H - 1.f) * 0.5f;
			const float ru = rintf(fx), rv = rintf(fy);
			if (!(ru >= 0.f && ru < (float)a.W && rv >= 0.f && rv < (float)a.H)) continue;      // (NaN: skipped)
			const size_t pix = (size_t)(int)rv * a.W + (int)ru;
			const float d = a.depth[pix];
			if (!(d > 0.f && d <= a.depth_trunc)) continue;
			if (a.alpha && !(a.alpha[pix] >= a.alpha_min)) continue;
			const float sdf = d - z;
			if (sdf < -a.sdf_trunc) continue;
			const float t = fminf(1.f, sdf / a.sdf_trunc);
			const size_t node = slot0 + local;
			const float w = a.weight[node], w1 = w + 1.f;
			a.tsdf[node] = (a.tsdf[node] * w + t) / w1;
			if (a.color) {
				const size_t hw = (size_t)a.W * a.H;
				float* col = a.color + 3 * slot0 + local;                  // color [capacity, 3, 512]
#pragma unroll
				for (int c = 0; c < 3; c++) col[c * SP_BLOCK_NODES] = (col[c * SP_BLOCK_NODES] * w + a.rgb[c * hw + pix]) / w1;
			}
			a.weight[node] = w1;
		}
	}
}

// ------------------------------------------------------------------------------------------------------------ the iso-surface over the pool
#define NODE_VALID 1u
#define NODE_INSIDE 2u
#define CELL_VALID 0x80u          // bit 7 of a node's vertex mask: the cell whose low corner it is is valid

// scratch of gsr_sparse_mesh_count, shared with gsr_sparse_mesh_emit (which only reads it): N = 512 n_slots pool nodes in N / 256 blocks
struct PoolScratch {
	uint8_t* cls;          // N        node class (0 for a node that does not exist)
	uint8_t* vmask;        // N        vertex mask | CELL_VALID
	uint8_t* tcnt;         // N        triangles of the node's cell (0..12)
	uint32_t* vert_off;    // N        exclusive vertex offset of the node
	uint32_t* tri_off;     // N        exclusive triangle offset of the node's cell
	uint32_t* part;        // nblocks  block sums: vertices | triangles << 16
	uint32_t* vbase;       // nblocks
	uint32_t* tbase;       // nblocks
	size_t bytes;
	uint32_t nblocks;
};
static PoolScratch pool_carve(void* base, uint64_t n_slots) {
	Carver c(base);
	PoolScratch s;
	const uint64_t N = n_slots * SP_BLOCK_NODES;
	s.nblocks = (uint32_t)(N / SCAN_BLOCK);
	s.cls = c.take<uint8_t>(N);
	s.vmask = c.take<uint8_t>(N);
	s.tcnt = c.take<uint8_t>(N);
	s.vert_off = c.take<uint32_t>(N);
	s.tri_off = c.take<uint32_t>(N);
	s.part = c.take<uint32_t>(s.nblocks);
	s.vbase = c.take<uint32_t>(s.nblocks);
	s.tbase = c.take<uint32_t>(s.nblocks);
	s.bytes = c.size();
	return s;
}

// (gsr_mesh.hip's tables: the case table of a positively oriented tetrahedron, the ends of edge 0..5, the direction of a corner difference)
__constant__ uint32_t SP_TET_CASES[16] = {0x00000u, 0x00221u, 0x00381u, 0x70c46u, 0x00565u, 0xad30au, 0x34582u, 0x00589u,
                                          0x004a9u, 0x94522u, 0xa9a0eu, 0x003a5u, 0x50c66u, 0x00461u, 0x00141u, 0x00000u};
#define EDGE_ENDS(e) ((0xed9c84u >> (4 * (e))) & 15u)
#define DIR_OF_BITS(m) ((0x65423100u >> (4 * (m))) & 7u)
// direction 0..6 as corner bits (x = 1, y = 2, z = 4)
__device__ __forceinline__ int dir_bits(int e) { return (e < 3) ? (1 << e) : (e == 3) ? 3 : (e == 4) ? 5 : (e == 5) ? 6 : 7; }
// corner offsets of p0..p3 of tetrahedron t, one nibble each
__device__ __forceinline__ uint32_t tet_corner_bits(int t) {
	const int a = t >> 1;
	const int b2 = (a == 0) ? 1 + (t & 1) : (a == 1) ? 2 * (t & 1) : (t & 1);
	const uint32_t p1 = 1u << a, p2 = p1 | (1u << b2);
	return (p1 << 4) | (p2 << 8) | (7u << 12);
}
// the inside mask over (p0..p3) of tetrahedron `p` from the cell's corner bits
__device__ __forceinline__ uint32_t tet_mask(uint32_t corner, uint32_t p) {
	return (corner & 1u) | (((corner >> ((p >> 4) & 7u)) & 1u) << 1) | (((corner >> ((p >> 8) & 7u)) & 1u) << 2) | (((corner >> 7) & 1u) << 3);
}

struct PoolArgs {
	const int32_t* table; const int32_t* block_of_slot;
	const float* tsdf; const float* weight; const float* color;
	const uint8_t* cls; const uint8_t* vmask; const uint32_t* vert_off; const uint32_t* tri_off;
	float* verts; float* vcolor; int* faces;
	BlockGrid g;
	uint32_t n_slots, nV, nT;
	float ox, oy, oz, voxel, min_weight;
};

// The slots of the blocks around block b into LDS, `span` per axis from offset `low` (3 from -1: the 27 of the count; 2 from 0: the 8 of
// the emit); -1 for a block outside the grid, without a slot, or with one at or beyond n_slots.  Ends with a barrier.
__device__ __forceinline__ void neighbour_slots(const PoolArgs& a, uint32_t b, int span, int low, int* slots) {
	if ((int)threadIdx.x < span * span * span) {
		int bi, bj, bk;
		block_ijk(b, a.g, bi, bj, bk);
		const int t = (int)threadIdx.x;
		const int x = bi + t % span + low, y = bj + (t / span) % span + low, z = bk + t / (span * span) + low;
		int slot = -1;
		if (b < a.g.G && x >= 0 && y >= 0 && z >= 0 && x < (int)a.g.gx && y < (int)a.g.gy && z < (int)a.g.gz) {
			slot = a.table[((size_t)z * a.g.gy + y) * a.g.gx + x];
			if (slot < 0 || (uint32_t)slot >= a.n_slots) slot = -1;
		}
		slots[t] = slot;
	}
	__syncthreads();
}

__global__ void __launch_bounds__(SCAN_BLOCK)
pool_classify_kernel(const PoolArgs a, uint8_t* __restrict__ cls) {
	const uint32_t n = blockIdx.x * SCAN_BLOCK + threadIdx.x, slot = n >> 9, local = n & 511u;
	const uint32_t b = (uint32_t)a.block_of_slot[slot];
	uint32_t c = 0;
	if (b < a.g.G) {
		int bi, bj, bk;
		block_ijk(b, a.g, bi, bj, bk);
		// a node that does not exist is invalid, and its planes are not read
		if (bi * 8 + (int)(local & 7u) < a.g.nx && bj * 8 + (int)((local >> 3) & 7u) < a.g.ny && bk * 8 + (int)(local >> 6) < a.g.nz)
			c = (a.weight[n] >= a.min_weight ? NODE_VALID : 0u) | (a.tsdf[n] < 0.f ? NODE_INSIDE : 0u);
	}
	cls[n] = (uint8_t)c;
}

__global__ void __launch_bounds__(SCAN_BLOCK)
pool_count_kernel(const PoolArgs a, uint8_t* __restrict__ vmask, uint8_t* __restrict__ tcnt, uint32_t* __restrict__ part) {
	__shared__ uint32_t lds[4];
	__shared__ int slots[27];
	const uint32_t n = blockIdx.x * SCAN_BLOCK + threadIdx.x, slot = n >> 9, local = n & 511u;
	neighbour_slots(a, (uint32_t)a.block_of_slot[slot], 3, -1, slots);
	uint32_t vm = 0, nt = 0;
	if (a.cls[n] & NODE_VALID) {
		const int li = (int)(local & 7u), lj = (int)((local >> 3) & 7u), lk = (int)(local >> 6);
		// valid and inside bits of the 27 nodes around n, bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); no slot, or no such node: invalid
		uint32_t valid = 0, inside = 0;
#pragma unroll
		for (int dz = -1; dz <= 1; dz++)
#pragma unroll
			for (int dy = -1; dy <= 1; dy++)
#pragma unroll
				for (int dx = -1; dx <= 1; dx++) {
					const int x = li + dx, y = lj + dy, z = lk + dz;
					const int s = slots[((z >> 3) + 1) * 9 + ((y >> 3) + 1) * 3 + (x >> 3) + 1];      // (-1 >> 3 = -1, 8 >> 3 = 1)
					if (s < 0) continue;
					const uint32_t c = a.cls[(size_t)s * SP_BLOCK_NODES + (uint32_t)(((z & 7) * 8 + (y & 7)) * 8 + (x & 7))];
					const int bit = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1);
					valid |= (c & NODE_VALID) << bit;
					inside |= ((c & NODE_INSIDE) >> 1) << bit;
				}
		const uint32_t CELL = 1u | 2u | 8u | 16u | 512u | 1024u | 4096u | 8192u;
		// cell_ok bit (cz * 4 + cy * 2 + cx) for the cell with low corner n - (1,1,1) + (cx, cy, cz)
		uint32_t cell_ok = 0;
#pragma unroll
		for (int c = 0; c < 8; c++) {
			const int low = (c >> 2) * 9 + ((c >> 1) & 1) * 3 + (c & 1);
			if (((valid >> low) & CELL) == CELL) cell_ok |= 1u << c;
		}
		const uint32_t centre = 13;
		const uint32_t in0 = (inside >> centre) & 1u;
#pragma unroll
		for (int e = 0; e < 7; e++) {
			const int db = dir_bits(e);
			const int far = centre + (db & 1) + ((db >> 1) & 1) * 3 + (db >> 2) * 9;
			if (!((valid >> centre) & (valid >> far) & 1u) || ((inside >> far) & 1u) == in0) continue;
			uint32_t held = 0;          // the cells that hold the edge: low corner n on the axes of the edge, n or n - 1 on the others
#pragma unroll
			for (int c = 0; c < 8; c++)
				if ((c & db) == db) held |= (cell_ok >> c) & 1u;
			if (held) vm |= 1u << e;
		}
		if ((cell_ok >> 7) & 1u) {           // the node's own cell
			vm |= CELL_VALID;
			uint32_t corner = 0;
#pragma unroll
			for (int c = 0; c < 8; c++) corner |= ((inside >> (centre + (c & 1) + ((c >> 1) & 1) * 3 + (c >> 2) * 9)) & 1u) << c;
#pragma unroll
			for (int t = 0; t < 6; t++) nt += SP_TET_CASES[tet_mask(corner, tet_corner_bits(t))] & 3u;
		}
	}
	vmask[n] = (uint8_t)vm;
	tcnt[n] = (uint8_t)nt;
	const uint32_t sum = block_sum(__popc(vm & 0x7fu) | (nt << 16), lds);
	if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(SCAN_BLOCK)
pool_offsets_kernel(const uint8_t* __restrict__ vmask, const uint8_t* __restrict__ tcnt, const uint32_t* __restrict__ vbase,
                    const uint32_t* __restrict__ tbase, uint32_t* __restrict__ vert_off, uint32_t* __restrict__ tri_off) {
	__shared__ uint32_t lds[4];
	const uint32_t n = blockIdx.x * SCAN_BLOCK + threadIdx.x;                 // (the pool is whole blocks)
	const uint32_t ex = block_exclusive((uint32_t)__popc(vmask[n] & 0x7fu) | ((uint32_t)tcnt[n] << 16), lds);
	vert_off[n] = vbase[blockIdx.x] + (ex & 0xffffu);
	tri_off[n] = tbase[blockIdx.x] + (ex >> 16);
}

__global__ void __launch_bounds__(SCAN_BLOCK)
pool_emit_kernel(const PoolArgs a) {
	__shared__ int slots[8];
	const uint32_t n = blockIdx.x * SCAN_BLOCK + threadIdx.x, slot = n >> 9, local = n & 511u;
	const uint32_t b = (uint32_t)a.block_of_slot[slot];
	neighbour_slots(a, b, 2, 0, slots);
	const uint32_t vm = a.vmask[n];
	if (vm == 0) return;
	int bi, bj, bk;
	block_ijk(b, a.g, bi, bj, bk);
	const int li = (int)(local & 7u), lj = (int)((local >> 3) & 7u), lk = (int)(local >> 6);
	const int i = bi * 8 + li, j = bj * 8 + lj, k = bk * 8 + lk;
	// pool index of the node at corner `c` (bit x + 2y + 4z) of n's cell: allocated wherever the count kernel set a bit that leads here
	auto corner_node = [&](int c) -> size_t {
		const int x = li + (c & 1), y = lj + ((c >> 1) & 1), z = lk + (c >> 2);
		const int s = slots[(z >> 3) * 4 + (y >> 3) * 2 + (x >> 3)];
		return (size_t)(s < 0 ? (int)slot : s) * SP_BLOCK_NODES + (uint32_t)(((z & 7) * 8 + (y & 7)) * 8 + (x & 7));
	};
	auto plane = [&](size_t node, int c) -> size_t { return (node >> 9) * (3 * SP_BLOCK_NODES) + c * SP_BLOCK_NODES + (node & 511u); };
	if (vm & 0x7fu) {
		const float ta = a.tsdf[n];
		const float ax = fmaf(a.voxel, (float)i, a.ox), ay = fmaf(a.voxel, (float)j, a.oy), az = fmaf(a.voxel, (float)k, a.oz);
		uint32_t at = a.vert_off[n];
		for (int e = 0; e < 7; e++) {
			if (!((vm >> e) & 1u)) continue;
			const int db = dir_bits(e);
			const int dx = db & 1, dy = (db >> 1) & 1, dz = db >> 2;
			const size_t m = corner_node(db);
			const float tb = a.tsdf[m];
			const float f = ta / (ta - tb);
			const uint32_t vi = at++;
			if (vi >= a.nV) continue;                                      // (never with the counts of this scratch: no row beyond nV)
			const float bx = fmaf(a.voxel, (float)(i + dx), a.ox), by = fmaf(a.voxel, (float)(j + dy), a.oy), bz = fmaf(a.voxel, (float)(k + dz), a.oz);
			float* o = a.verts + 3 * (size_t)vi;
			o[0] = ax + (bx - ax) * f;
			o[1] = ay + (by - ay) * f;
			o[2] = az + (bz - az) * f;
			if (a.vcolor) {
#pragma unroll
				for (int c = 0; c < 3; c++) {
					const float ca = a.color[plane(n, c)], cb = a.color[plane(m, c)];
					a.vcolor[3 * (size_t)vi + c] = ca + (cb - ca) * f;
				}
			}
		}
	}
	if (vm & CELL_VALID) {
		// the cell's corners: inside bits, and for the seven that start an edge their vertex masks and offsets
		uint32_t corner = 0, cmask[8], coff[8];
#pragma unroll
		for (int c = 0; c < 8; c++) {
			const size_t m = corner_node(c);
			corner |= (((uint32_t)a.cls[m] >> 1) & 1u) << c;
			cmask[c] = c < 7 ? (uint32_t)a.vmask[m] : 0u;
			coff[c] = c < 7 ? a.vert_off[m] : 0u;
		}
		uint32_t at = a.tri_off[n];
		for (int t = 0; t < 6; t++) {
			const uint32_t p = tet_corner_bits(t);
			uint32_t code = SP_TET_CASES[tet_mask(corner, p)];
			const uint32_t ntri = code & 3u;
			code >>= 2;
			const bool positive = (t == 0 || t == 3 || t == 4);
			for (uint32_t r = 0; r < ntri; r++) {
				int id[3];
#pragma unroll
				for (int q = 0; q < 3; q++, code >>= 3) {
					const uint32_t ends = EDGE_ENDS(code & 7u);
					const uint32_t lo = (p >> (4 * (ends & 3u))) & 7u, hi = (p >> (4 * (ends >> 2))) & 7u;
					const uint32_t dir = DIR_OF_BITS(hi ^ lo);
					uint32_t cm = 0, co = 0;          // (selects: a dynamic index would send cmask and coff to scratch memory)
#pragma unroll
					for (int c = 0; c < 7; c++)
						if (lo == (uint32_t)c) { cm = cmask[c]; co = coff[c]; }
					id[q] = (int)(co + __popc(cm & ((1u << dir) - 1u)));
				}
				const uint32_t ti = at++;
				if (ti >= a.nT) continue;                                  // (never with the counts of this scratch)
				int* o = a.faces + 3 * (size_t)ti;
				o[0] = id[0];
				o[1] = positive ? id[1] : id[2];
				o[2] = positive ? id[2] : id[1];
			}
		}
	}
}

// ------------------------------------------------------------------------------------------------------------ host side
// The block grid of a volume the entries take (every dimension at least 2, fewer than 2^31 blocks); G = 0 otherwise.
static BlockGrid block_grid(int nx, int ny, int nz) {
	BlockGrid g;
	g.nx = nx; g.ny = ny; g.nz = nz;
	g.gx = g.gy = g.gz = g.G = 0;
	if (nx < 2 || ny < 2 || nz < 2) return g;
	g.gx = ((uint32_t)nx + 7u) / 8u; g.gy = ((uint32_t)ny + 7u) / 8u; g.gz = ((uint32_t)nz + 7u) / 8u;
	const uint64_t G = (uint64_t)g.gx * g.gy * g.gz;                  // < 2^87 / 2^9: no overflow
	g.G = G < LIMIT_2_31 ? (uint32_t)G : 0u;
	return g;
}
static int grid_check(const char* entry, int nx, int ny, int nz, BlockGrid* g) {
	*g = block_grid(nx, ny, nz);
	if (g->G) return 0;
	if (nx < 2 || ny < 2 || nz < 2) set_error("%s: every dimension of the volume must be at least 2 (got %d x %d x %d)", entry, nx, ny, nz);
	else set_error("%s: the volume must have fewer than 2^31 blocks of 8 x 8 x 8 nodes (got %d x %d x %d nodes)", entry, nx, ny, nz);
	return GSR_E_INVALID;
}
// `capacity` slots, of which the first n_slots are in use
static int pool_check(const char* entry, uint64_t n_slots, uint64_t capacity) {
	if (capacity >= LIMIT_2_31 / SP_BLOCK_NODES) {
		set_error("%s: capacity * 512 must be below 2^31 (got %llu slots)", entry, (unsigned long long)capacity);
		return GSR_E_INVALID;
	}
	if (n_slots > capacity) {
		set_error("%s: n_slots beyond the capacity (%llu of %llu)", entry, (unsigned long long)n_slots, (unsigned long long)capacity);
		return GSR_E_INVALID;
	}
	return 0;
}
// what touch and integrate take of a view
static int view_check(const char* entry, int W, int H, float sdf_trunc, float depth_trunc, float alpha_min) {
	if (int rc = image_check(entry, W, H)) return rc;
	if (!positive_finite(sdf_trunc) || !positive_finite(depth_trunc)) {
		set_error("%s: sdf_trunc and depth_trunc must be positive and finite (got %g, %g)", entry, (double)sdf_trunc, (double)depth_trunc);
		return GSR_E_INVALID;
	}
	if (!std::isfinite(alpha_min)) { set_error("%s: alpha_min is not finite", entry); return GSR_E_INVALID; }
	return 0;
}

}  // namespace gsr

using namespace gsr;

extern "C" int gsr_sparse_tsdf_touch(int32_t* table, int nx, int ny, int nz, float ox, float oy, float oz, float voxel, const float* depth,
                                     const float* alpha, float alpha_min, int W, int H, const float* viewmatrix, const float* projmatrix,
                                     float sdf_trunc, float depth_trunc, void* stream_) {
	const char* entry = "gsr_sparse_tsdf_touch";
	hipStream_t stream = (hipStream_t)stream_;
	if (!table || !depth || !viewmatrix || !projmatrix) { set_error("%s: invalid argument (NULL pointer)", entry); return GSR_E_INVALID; }
	if (int rc = pointers_check(entry, {table, depth, alpha, viewmatrix, projmatrix})) return rc;
	TouchArgs a;
	if (int rc = grid_check(entry, nx, ny, nz, &a.g)) return rc;
	if (int rc = placement_check(entry, "voxel", voxel, "origin", ox, oy, oz)) return rc;
	if (int rc = view_check(entry, W, H, sdf_trunc, depth_trunc, alpha_min)) return rc;
	a.table = table; a.depth = depth; a.alpha = alpha; a.view = viewmatrix; a.proj = projmatrix;
	a.W = W; a.H = H;
	a.ox = ox; a.oy = oy; a.oz = oz; a.voxel = voxel; a.alpha_min = alpha_min; a.sdf_trunc = sdf_trunc; a.depth_trunc = depth_trunc;
	sparse_touch_kernel<<<a.g.G < SP_MAX_GRID ? a.g.G : SP_MAX_GRID, 256, 0, stream>>>(a);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" size_t gsr_sparse_tsdf_allocate_scratch_bytes(int nx, int ny, int nz) {
	const BlockGrid g = block_grid(nx, ny, nz);
	return g.G ? alloc_carve(nullptr, g.G).bytes : 0;
}

extern "C" int gsr_sparse_tsdf_allocate(int32_t* table, int nx, int ny, int nz, int32_t* block_of_slot, uint64_t capacity, uint64_t* counts,
                                        void* scratch, size_t scratch_bytes, void* stream_) {
	const char* entry = "gsr_sparse_tsdf_allocate";
	hipStream_t stream = (hipStream_t)stream_;
	if (!table || !counts || (capacity > 0 && !block_of_slot)) { set_error("%s: invalid argument (NULL pointer)", entry); return GSR_E_INVALID; }
	if (int rc = pointers_check(entry, {table, block_of_slot})) return rc;
	if (int rc = aligned_check(entry, "counts", counts, 8)) return rc;
	BlockGrid g;
	if (int rc = grid_check(entry, nx, ny, nz, &g)) return rc;
	if (int rc = pool_check(entry, 0, capacity)) return rc;
	const AllocScratch s = alloc_carve(scratch, g.G);
	if (int rc = scratch_check(entry, scratch, scratch_bytes, s.bytes, "bytes", "gsr_sparse_tsdf_allocate_scratch_bytes(nx, ny, nz)", 16)) return rc;
	alloc_count_kernel<<<s.nblocks, SCAN_BLOCK, 0, stream>>>(table, g.G, s.part);
	GSR_LAUNCH_CHECK(0, stream);
	scan_spine_kernel<<<1, 1024, 0, stream>>>(s.part, s.nblocks, s.vbase, s.tbase, s.total);
	GSR_LAUNCH_CHECK(0, stream);
	alloc_assign_kernel<<<s.nblocks, SCAN_BLOCK, 0, stream>>>(table, g.G, s.vbase, (const unsigned long long*)counts, capacity, block_of_slot);
	GSR_LAUNCH_CHECK(0, stream);
	alloc_finish_kernel<<<1, 1, 0, stream>>>(s.total, capacity, (unsigned long long*)counts);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_sparse_tsdf_integrate(const int32_t* block_of_slot, uint64_t n_slots, uint64_t capacity, float* tsdf, float* weight, float* color,
                                         int nx, int ny, int nz, float ox, float oy, float oz, float voxel, const float* depth, const float* rgb,
                                         const float* alpha, float alpha_min, int W, int H, const float* viewmatrix, const float* projmatrix,
                                         float sdf_trunc, float depth_trunc, void* stream_) {
	const char* entry = "gsr_sparse_tsdf_integrate";
	hipStream_t stream = (hipStream_t)stream_;
	if (!depth || !viewmatrix || !projmatrix || (n_slots > 0 && (!block_of_slot || !tsdf || !weight))) {
		set_error("%s: invalid argument (NULL pointer)", entry);
		return GSR_E_INVALID;
	}
	if ((color != nullptr) != (rgb != nullptr)) { set_error("%s: color and rgb must both be given or both be NULL", entry); return GSR_E_INVALID; }
	if (int rc = pointers_check(entry, {block_of_slot, tsdf, weight, color, depth, rgb, alpha, viewmatrix, projmatrix})) return rc;
	SparseTsdfArgs a;
	if (int rc = grid_check(entry, nx, ny, nz, &a.g)) return rc;
	if (int rc = pool_check(entry, n_slots, capacity)) return rc;
	if (int rc = placement_check(entry, "voxel", voxel, "origin", ox, oy, oz)) return rc;
	if (int rc = view_check(entry, W, H, sdf_trunc, depth_trunc, alpha_min)) return rc;
	if (n_slots == 0) return 0;
	a.block_of_slot = block_of_slot; a.tsdf = tsdf; a.weight = weight; a.color = color;
	a.depth = depth; a.rgb = rgb; a.alpha = alpha; a.view = viewmatrix; a.proj = projmatrix;
	a.W = W; a.H = H;
	a.ox = ox; a.oy = oy; a.oz = oz; a.voxel = voxel; a.alpha_min = alpha_min; a.sdf_trunc = sdf_trunc; a.depth_trunc = depth_trunc;
	a.n_slots = (uint32_t)n_slots;
	const uint32_t wgs = (a.n_slots + 3u) / 4u;                         // a wave per slot
	sparse_integrate_kernel<<<wgs < SP_MAX_GRID ? wgs : SP_MAX_GRID, 256, 0, stream>>>(a);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" size_t gsr_sparse_mesh_scratch_bytes(uint64_t n_slots) {
	return n_slots > 0 && n_slots < LIMIT_2_31 / SP_BLOCK_NODES ? pool_carve(nullptr, n_slots).bytes : 0;
}

extern "C" int gsr_sparse_mesh_count(const int32_t* table, const int32_t* block_of_slot, uint64_t n_slots, uint64_t capacity, const float* tsdf,
                                     const float* weight, int nx, int ny, int nz, float min_weight, void* scratch, size_t scratch_bytes,
                                     uint64_t* counts, void* stream_) {
	const char* entry = "gsr_sparse_mesh_count";
	hipStream_t stream = (hipStream_t)stream_;
	if (!table || !counts || (n_slots > 0 && (!block_of_slot || !tsdf || !weight || !scratch))) {
		set_error("%s: invalid argument (NULL pointer)", entry);
		return GSR_E_INVALID;
	}
	if (int rc = pointers_check(entry, {table, block_of_slot, tsdf, weight})) return rc;
	if (int rc = aligned_check(entry, "counts", counts, 8)) return rc;
	PoolArgs a;
	if (int rc = grid_check(entry, nx, ny, nz, &a.g)) return rc;
	if (int rc = pool_check(entry, n_slots, capacity)) return rc;
	if (std::isnan(min_weight)) { set_error("%s: min_weight is NaN", entry); return GSR_E_INVALID; }
	if (n_slots == 0) {                                                 // nothing is allocated: an empty surface
		GSR_HIP_CHECK(hipMemsetAsync(counts, 0, 2 * sizeof(uint64_t), stream));
		return 0;
	}
	const PoolScratch s = pool_carve(scratch, n_slots);
	if (int rc = scratch_check(entry, scratch, scratch_bytes, s.bytes, "bytes", "gsr_sparse_mesh_scratch_bytes(n_slots)", 16)) return rc;
	a.table = table; a.block_of_slot = block_of_slot; a.tsdf = tsdf; a.weight = weight; a.color = nullptr;
	a.cls = s.cls; a.vmask = s.vmask; a.vert_off = s.vert_off; a.tri_off = s.tri_off;
	a.verts = nullptr; a.vcolor = nullptr; a.faces = nullptr;
	a.n_slots = (uint32_t)n_slots; a.nV = a.nT = 0;
	a.ox = a.oy = a.oz = 0.f; a.voxel = 1.f; a.min_weight = min_weight;
	pool_classify_kernel<<<s.nblocks, SCAN_BLOCK, 0, stream>>>(a, s.cls);
	GSR_LAUNCH_CHECK(0, stream);
	pool_count_kernel<<<s.nblocks, SCAN_BLOCK, 0, stream>>>(a, s.vmask, s.tcnt, s.part);
	GSR_LAUNCH_CHECK(0, stream);
	scan_spine_kernel<<<1, 1024, 0, stream>>>(s.part, s.nblocks, s.vbase, s.tbase, (unsigned long long*)counts);
	GSR_LAUNCH_CHECK(0, stream);
	pool_offsets_kernel<<<s.nblocks, SCAN_BLOCK, 0, stream>>>(s.vmask, s.tcnt, s.vbase, s.tbase, s.vert_off, s.tri_off);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_sparse_mesh_emit(const int32_t* table, const int32_t* block_of_slot, uint64_t n_slots, uint64_t capacity, const float* tsdf,
                                    const float* weight, const float* color, int nx, int ny, int nz, float ox, float oy, float oz, float voxel,
                                    float min_weight, const void* scratch, float* verts, float* vcolor, int* faces, uint64_t nV, uint64_t nT,
                                    void* stream_) {
	const char* entry = "gsr_sparse_mesh_emit";
	hipStream_t stream = (hipStream_t)stream_;
	(void)min_weight;             // the classification is the one gsr_sparse_mesh_count left in the scratch
	if (!table || (n_slots > 0 && (!block_of_slot || !tsdf || !weight || !scratch))) {
		set_error("%s: invalid argument (NULL pointer)", entry);
		return GSR_E_INVALID;
	}
	if (int rc = pointers_check(entry, {table, block_of_slot, tsdf, weight, color, verts, vcolor, faces})) return rc;
	if (int rc = aligned_check(entry, "scratch", scratch, 16)) return rc;
	PoolArgs a;
	if (int rc = grid_check(entry, nx, ny, nz, &a.g)) return rc;
	if (int rc = pool_check(entry, n_slots, capacity)) return rc;
	if (int rc = placement_check(entry, "voxel", voxel, "origin", ox, oy, oz)) return rc;
	if (nV >= LIMIT_2_31 || nT >= LIMIT_2_31 || 3 * nT >= LIMIT_2_31) {
		set_error("%s: nV and 3 * nT must be below 2^31 (got %llu vertices, %llu triangles)", entry, (unsigned long long)nV, (unsigned long long)nT);
		return GSR_E_INVALID;
	}
	if (nV == 0 || n_slots == 0) return 0;
	if (!verts || (nT > 0 && !faces)) { set_error("%s: invalid argument (NULL verts or faces)", entry); return GSR_E_INVALID; }
	if ((color != nullptr) != (vcolor != nullptr)) { set_error("%s: color and vcolor must both be given or both be NULL", entry); return GSR_E_INVALID; }
	const PoolScratch s = pool_carve(const_cast<void*>(scratch), n_slots);      // (read only)
	a.table = table; a.block_of_slot = block_of_slot; a.tsdf = tsdf; a.weight = weight; a.color = color;
	a.cls = s.cls; a.vmask = s.vmask; a.vert_off = s.vert_off; a.tri_off = s.tri_off;
	a.verts = verts; a.vcolor = vcolor; a.faces = faces;
	a.n_slots = (uint32_t)n_slots; a.nV = (uint32_t)nV; a.nT = (uint32_t)nT;
	a.ox = ox; a.oy = oy; a.oz = oz; a.voxel = voxel; a.min_weight = min_weight;
	pool_emit_kernel<<<s.nblocks, SCAN_BLOCK, 0, stream>>>(a);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}
