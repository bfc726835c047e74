// Mesh extraction (include/gsr_hip_mesh.h has the contracts): TSDF fusion of one rendered depth map into a dense voxel grid, and the
// iso-surface of the grid as an indexed mesh by marching tetrahedra on the Kuhn split.
//
// gsr_tsdf_integrate is a streaming pass: per node ~40 flops, one gathered depth read and two to five plane reads and writes.  A
// workgroup is four waves; a wave owns a run of 64 nodes along x (one 256-byte line per plane and instruction) and walks TSDF_KZ slices of
// z with it, the parts of the dot products that do not depend on z hoisted.  Every skip rule is decided from registers and the gathered
// depth before a plane is touched, so a node outside the view costs a dozen instructions and no traffic.  (A per-wave test of the wave's
// box against the frustum, leaving before the node loop, was built and measured: 0.217 ms with it, 0.215 ms without, for a 1080p view
// into 512^3 from a face of the box — it costs as much as the eight skips it saves, and is gone.  DESIGN.md, "Mesh extraction".)
//
// The extraction is five kernels over the nodes in linear order, 256 per block, no atomics and no waiting between workgroups:
//   classify    node -> valid | inside << 1                                                           (reads tsdf and weight once)
//   count       node -> the 7-bit mask of the lattice edges leaving it that carry a vertex, bit 7 = its cell is valid, and the cell's
//               triangle count, from the 27 classes around it; block sums of both counts
//   spine       ONE block scans the block sums (64-bit carries: the totals are exact) and writes counts[0..1]
//   offsets     node -> exclusive vertex and triangle offsets (block scan + the block's base)
//   emit        node -> its vertices, and its cell's triangles with the vertex indices looked up at the cell's corners
// Offsets are 32-bit: they are exact whenever the totals are below 2^31, and gsr_mesh_emit refuses larger ones.
// Host side: the checks that are not specific to an entry are gsr_host.hpp's; the scratch is MeshScratch, typed pointers carved by
// mesh_carve (a NULL base answers gsr_mesh_scratch_bytes).  The view's matrix rows and dot products are gsr_view.hpp's.
#include "gsr_host.hpp"
#include "gsr_scan.hpp"
#include "gsr_view.hpp"
#include "../../include/gsr_hip_mesh.h"

namespace gsr {

#define TSDF_KZ 8                 // z slices a wave walks
#define TSDF_ROWS 4               // waves (rows of y) per block
#define TSDF_MAX_GRID 65536u      // blocks per launch; the kernel strides over the rest

struct TsdfArgs {
	float* tsdf; float* weight; float* color;
	const float* depth; const float* rgb; const float* alpha;
	const float* view; const float* proj;
	int nx, ny, nz, W, H;
	float ox, oy, oz, voxel, alpha_min, sdf_trunc, depth_trunc;
	uint32_t bx, bxy, nblocks;    // blocks along x, in one slab of TSDF_KZ slices, in all (< 2^28, see gsr_tsdf_integrate)
};

__global__ void __launch_bounds__(64 * TSDF_ROWS)
tsdf_integrate_kernel(const TsdfArgs a) {
	const ViewRows r(a.view, a.proj);
	const int lane = threadIdx.x & 63, row = threadIdx.x >> 6;
	const size_t plane = (size_t)a.nx * a.ny, vol = plane * a.nz;
	for (uint32_t b = blockIdx.x; b < a.nblocks; b += gridDim.x) {
		const uint32_t slab = b / a.bxy, bxy = b - slab * a.bxy, brow = bxy / a.bx;
		const int k0 = (int)slab * TSDF_KZ;
		const int i0 = (int)(bxy - brow * a.bx) * 64, j = (int)brow * TSDF_ROWS + row;
		if (j >= a.ny) continue;                                   // (the whole wave: no lane of it has a node)
		const int i = i0 + lane;
		const int k1 = min(k0 + TSDF_KZ, a.nz);
		if (i >= a.nx) continue;
		const float X = fmaf(a.voxel, (float)i, a.ox), Y = fmaf(a.voxel, (float)j, a.oy);
		const ViewDots xy = r.xy(X, Y);                                // the part of the four dot products that does not change along z
		size_t node = (size_t)k0 * plane + (size_t)j * a.nx + i;       // < 2^31
#pragma unroll 2
		for (int k = k0; k < k1; k++, node += plane) {
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
			const float w = a.weight[node], w1 = w + 1.f;
			a.tsdf[node] = (a.tsdf[node] * w + t) / w1;
			if (a.color) {
				const size_t hw = (size_t)a.W * a.H;
#pragma unroll
				for (int c = 0; c < 3; c++) a.color[c * vol + node] = (a.color[c * vol + node] * w + a.rgb[c * hw + pix]) / w1;
			}
			a.weight[node] = w1;
		}
	}
}

// ------------------------------------------------------------------------------------------------------------ the iso-surface
#define MESH_BLOCK SCAN_BLOCK      // the block of the two-level scan (gsr_scan.hpp: block_sum, block_exclusive, scan_spine_kernel)
#define NODE_VALID 1u
#define NODE_INSIDE 2u
#define CELL_VALID 0x80u          // bit 7 of a node's vertex mask: the cell whose low corner it is is valid

// scratch of gsr_mesh_count, shared with gsr_mesh_emit (which only reads it): N nodes in `nblocks` blocks
struct MeshScratch {
	uint8_t* cls;          // N        node class
	uint8_t* vmask;        // N        vertex mask | CELL_VALID
	uint8_t* tcnt;         // N        triangles of the node's cell (0..12)
	uint32_t* vert_off;    // N        exclusive vertex offset of the node
	uint32_t* tri_off;     // N        exclusive triangle offset of the node's cell
	uint32_t* part;        // nblocks  block sums: vertices | triangles << 16
	uint32_t* vbase;       // nblocks  vertices in front of the block
	uint32_t* tbase;       // nblocks  triangles in front of the block
	size_t bytes;
	uint32_t nblocks;
};
static MeshScratch mesh_carve(void* base, uint64_t N) {
	Carver c(base);
	MeshScratch s;
	s.nblocks = (uint32_t)((N + MESH_BLOCK - 1) / MESH_BLOCK);
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

// Case table of a positively oriented tetrahedron, indexed by the inside mask over (p0..p3): bits 0-1 the triangle count, then three
// bits per corner, the edges numbered 01, 02, 03, 12, 13, 23 = 0..5 (include/gsr_hip_mesh.h states the rule; tests/mesh_ref.py generates
// the same table from it).
__constant__ uint32_t TET_CASES[16] = {0x00000u, 0x00221u, 0x00381u, 0x70c46u, 0x00565u, 0xad30au, 0x34582u, 0x00589u,
                                       0x004a9u, 0x94522u, 0xa9a0eu, 0x003a5u, 0x50c66u, 0x00461u, 0x00141u, 0x00000u};
// the two ends of edge 0..5 as local vertices, two bits each: lo in bits 0-1, hi in bits 2-3
#define EDGE_ENDS(e) ((0xed9c84u >> (4 * (e))) & 15u)      // 01 -> 0x4, 02 -> 0x8, 03 -> 0xc, 12 -> 0x9, 13 -> 0xd, 23 -> 0xe
// direction number of a corner difference given as bits (x = 1, y = 2, z = 4): 100, 010, 110, 001, 101, 011, 111 -> 0, 1, 3, 2, 4, 5, 6
#define DIR_OF_BITS(m) ((0x65423100u >> (4 * (m))) & 7u)

__device__ __forceinline__ uint32_t tet_triangles(uint32_t inside4) { return TET_CASES[inside4] & 3u; }

// corner offsets (bits x = 1, y = 2, z = 4) of p0..p3 of tetrahedron t, one nibble each
__device__ __forceinline__ uint32_t tet_corner_bits(int t) {
	// (a, b) = (0,1) (0,2) (1,0) (1,2) (2,0) (2,1): the second axis is the (t & 1)'th of the two that are not a
	const int a = t >> 1;
	const int b2 = (a == 0) ? 1 + (t & 1) : (a == 1) ? 2 * (t & 1) : (t & 1);
	const uint32_t p1 = 1u << a, p2 = p1 | (1u << b2);
	return (p1 << 4) | (p2 << 8) | (7u << 12);
}

__device__ __forceinline__ void node_ijk(uint32_t n, int nx, int ny, int& i, int& j, int& k) {
	const uint32_t row = n / (uint32_t)nx;
	i = (int)(n - row * (uint32_t)nx);
	k = (int)(row / (uint32_t)ny);
	j = (int)(row - (uint32_t)k * (uint32_t)ny);
}

__global__ void __launch_bounds__(MESH_BLOCK)
mesh_classify_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight, uint32_t N, float min_weight, uint8_t* __restrict__ cls) {
	const uint32_t n = blockIdx.x * MESH_BLOCK + threadIdx.x;
	if (n >= N) return;
	cls[n] = (uint8_t)((weight[n] >= min_weight ? NODE_VALID : 0u) | (tsdf[n] < 0.f ? NODE_INSIDE : 0u));
}

__global__ void __launch_bounds__(MESH_BLOCK)
mesh_count_kernel(const uint8_t* __restrict__ cls, uint32_t N, int nx, int ny, int nz, uint8_t* __restrict__ vmask, uint8_t* __restrict__ tcnt,
                  uint32_t* __restrict__ part) {
	__shared__ uint32_t lds[4];
	const uint32_t n = blockIdx.x * MESH_BLOCK + threadIdx.x;
	uint32_t vm = 0, nt = 0;
	// an invalid node starts no vertex and its cell is invalid: most of a fused volume is unobserved, and leaves here after one byte
	if (n < N && !(cls[n] & NODE_VALID)) {
		vmask[n] = 0;
		tcnt[n] = 0;
	} else if (n < N) {
		int i, j, k;
		node_ijk(n, nx, ny, i, j, k);
		// valid and inside bits of the 27 nodes around n, bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); outside the grid: invalid
		uint32_t valid = 0, inside = 0;
#pragma unroll
		for (int dz = -1; dz <= 1; dz++)
#pragma unroll
			for (int dy = -1; dy <= 1; dy++)
#pragma unroll
				for (int dx = -1; dx <= 1; dx++) {
					const int x = i + dx, y = j + dy, z = k + dz;
					if (x < 0 || y < 0 || z < 0 || x >= nx || y >= ny || z >= nz) continue;
					const uint32_t c = cls[(size_t)n + (ptrdiff_t)dx + (ptrdiff_t)dy * nx + (ptrdiff_t)dz * ((ptrdiff_t)nx * ny)];
					const int bit = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1);
					valid |= (c & NODE_VALID) << bit;
					inside |= ((c & NODE_INSIDE) >> 1) << bit;
				}
		// the eight nodes of the cell whose low corner is the node at bit 0: bits {0,1} + {0,3} + {0,9}
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
			const int db = (e < 3) ? (1 << e) : (e == 3) ? 3 : (e == 4) ? 5 : (e == 5) ? 6 : 7;     // x = 1, y = 2, z = 4
			const int far = centre + (db & 1) + ((db >> 1) & 1) * 3 + (db >> 2) * 9;
			if (!((valid >> centre) & (valid >> far) & 1u) || ((inside >> far) & 1u) == in0) continue;
			// cells that hold the edge: low corner n on the axes of the edge (cell coordinate 1), n or n - 1 on the others
			uint32_t held = 0;
#pragma unroll
			for (int c = 0; c < 8; c++)
				if ((c & db) == db) held |= (cell_ok >> c) & 1u;
			if (held) vm |= 1u << e;
		}
		if ((cell_ok >> 7) & 1u) {           // the node's own cell
			vm |= CELL_VALID;
			// inside bits of the cell's corners, bit (x + 2y + 4z)
			uint32_t corner = 0;
#pragma unroll
			for (int c = 0; c < 8; c++) corner |= ((inside >> (centre + (c & 1) + ((c >> 1) & 1) * 3 + (c >> 2) * 9)) & 1u) << c;
#pragma unroll
			for (int t = 0; t < 6; t++) {
				const uint32_t p = tet_corner_bits(t);
				const uint32_t m = (corner & 1u) | (((corner >> ((p >> 4) & 7u)) & 1u) << 1) | (((corner >> ((p >> 8) & 7u)) & 1u) << 2) |
				                   (((corner >> 7) & 1u) << 3);
				nt += tet_triangles(m);
			}
		}
		vmask[n] = (uint8_t)vm;
		tcnt[n] = (uint8_t)nt;
	}
	const uint32_t sum = block_sum(__popc(vm & 0x7fu) | (nt << 16), lds);
	if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(MESH_BLOCK)
mesh_offsets_kernel(const uint8_t* __restrict__ vmask, const uint8_t* __restrict__ tcnt, uint32_t N, const uint32_t* __restrict__ vbase,
                    const uint32_t* __restrict__ tbase, uint32_t* __restrict__ vert_off, uint32_t* __restrict__ tri_off) {
	__shared__ uint32_t lds[4];
	const uint32_t n = blockIdx.x * MESH_BLOCK + threadIdx.x;
	const uint32_t v = n < N ? (uint32_t)__popc(vmask[n] & 0x7fu) : 0u, t = n < N ? (uint32_t)tcnt[n] : 0u;
	const uint32_t ex = block_exclusive(v | (t << 16), lds);         // (a block sums to at most 1792 | 3072 << 16)
	if (n < N) {
		vert_off[n] = vbase[blockIdx.x] + (ex & 0xffffu);
		tri_off[n] = tbase[blockIdx.x] + (ex >> 16);
	}
}

struct EmitArgs {
	const float* tsdf; const float* color;
	const uint8_t* cls; const uint8_t* vmask; const uint32_t* vert_off; const uint32_t* tri_off;
	float* verts; float* vcolor; int* faces;
	uint32_t N, nV, nT;
	int nx, ny, nz;
	float ox, oy, oz, voxel;
};

__global__ void __launch_bounds__(MESH_BLOCK)
mesh_emit_kernel(const EmitArgs a) {
	const uint32_t n = blockIdx.x * MESH_BLOCK + threadIdx.x;
	if (n >= a.N) return;
	const uint32_t vm = a.vmask[n];
	if (vm == 0) return;
	int i, j, k;
	node_ijk(n, a.nx, a.ny, i, j, k);
	const size_t sx = 1, sy = (size_t)a.nx, sz = (size_t)a.nx * a.ny;
	if (vm & 0x7fu) {
		const float ta = a.tsdf[n];
		const float ax = fmaf(a.voxel, (float)i, a.ox), ay = fmaf(a.voxel, (float)j, a.oy), az = fmaf(a.voxel, (float)k, a.oz);
		uint32_t at = a.vert_off[n];
		for (int e = 0; e < 7; e++) {
			if (!((vm >> e) & 1u)) continue;
			const int db = (e < 3) ? (1 << e) : (e == 3) ? 3 : (e == 4) ? 5 : (e == 5) ? 6 : 7;
			const int dx = db & 1, dy = (db >> 1) & 1, dz = db >> 2;
			const size_t m = (size_t)n + dx * sx + dy * sy + dz * sz;      // in the grid: the count kernel set the bit only there
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
				const size_t vol = sz * a.nz;
#pragma unroll
				for (int c = 0; c < 3; c++) {
					const float ca = a.color[c * vol + n], cb = a.color[c * vol + m];
					a.vcolor[3 * (size_t)vi + c] = ca + (cb - ca) * f;
				}
			}
		}
	}
	if (vm & CELL_VALID) {
		// the cell's corners (bit x + 2y + 4z): inside bits, and for the seven that start an edge their vertex masks and offsets
		uint32_t corner = 0, cmask[8], coff[8];
#pragma unroll
		for (int c = 0; c < 8; c++) {
			const size_t m = (size_t)n + (c & 1) * sx + ((c >> 1) & 1) * sy + (c >> 2) * sz;
			corner |= (((uint32_t)a.cls[m] >> 1) & 1u) << c;
			cmask[c] = c < 7 ? (uint32_t)a.vmask[m] : 0u;
			coff[c] = c < 7 ? a.vert_off[m] : 0u;
		}
		uint32_t at = a.tri_off[n];
		for (int t = 0; t < 6; t++) {
			const uint32_t p = tet_corner_bits(t);
			const uint32_t m = (corner & 1u) | (((corner >> ((p >> 4) & 7u)) & 1u) << 1) | (((corner >> ((p >> 8) & 7u)) & 1u) << 2) |
			                   (((corner >> 7) & 1u) << 3);
			uint32_t code = TET_CASES[m];
			const uint32_t ntri = code & 3u;
			code >>= 2;
			const bool positive = (t == 0 || t == 3 || t == 4);
			for (uint32_t r = 0; r < ntri; r++) {
				int id[3];
#pragma unroll
				for (int q = 0; q < 3; q++, code >>= 3) {
					const uint32_t ends = EDGE_ENDS(code & 7u);
					const uint32_t lo = (p >> (4 * (ends & 3u))) & 7u, hi = (p >> (4 * (ends >> 2))) & 7u;      // corner bits of the edge's ends
					const uint32_t dir = DIR_OF_BITS(hi ^ lo);
					// the selects below keep cmask / coff in registers (a dynamic index would spill them to scratch memory)
					uint32_t cm = 0, co = 0;
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
// The volume's size limits: the node count of a volume the entries take (every dimension at least 2, nx * ny * nz below 2^31), else 0.
static uint64_t volume_nodes(int nx, int ny, int nz) {
	if (nx < 2 || ny < 2 || nz < 2) return 0;
	const uint64_t xy = (uint64_t)nx * (uint64_t)ny;               // < 2^62
	return xy < LIMIT_2_31 && xy * (uint64_t)nz < LIMIT_2_31 ? xy * (uint64_t)nz : 0;
}
// Returns 0 and the node count, or GSR_E_INVALID with the message set.
static int volume_check(const char* entry, int nx, int ny, int nz, uint64_t* N) {
	*N = volume_nodes(nx, ny, nz);
	if (*N) return 0;
	if (nx < 2 || ny < 2 || nz < 2) set_error("%s: every dimension of the volume must be at least 2 (got %d x %d x %d)", entry, nx, ny, nz);
	else set_error("%s: nx * ny * nz must be below 2^31 (got %d x %d x %d)", entry, nx, ny, nz);
	return GSR_E_INVALID;
}

}  // namespace gsr

using namespace gsr;

extern "C" int gsr_tsdf_integrate(float* tsdf, float* weight, float* color, int nx, int ny, int nz, float ox, float oy, float oz, float voxel,
                                  const float* depth, const float* rgb, const float* alpha, float alpha_min, int W, int H,
                                  const float* viewmatrix, const float* projmatrix, float sdf_trunc, float depth_trunc, void* stream_) {
	const char* entry = "gsr_tsdf_integrate";
	hipStream_t stream = (hipStream_t)stream_;
	if (!tsdf || !weight || !depth || !viewmatrix || !projmatrix) { set_error("%s: invalid argument (NULL pointer)", entry); return GSR_E_INVALID; }
	if ((color != nullptr) != (rgb != nullptr)) { set_error("%s: color and rgb must both be given or both be NULL", entry); return GSR_E_INVALID; }
	if (int rc = pointers_check(entry, {tsdf, weight, color, depth, rgb, alpha, viewmatrix, projmatrix})) return rc;
	uint64_t N;
	if (int rc = volume_check(entry, nx, ny, nz, &N)) return rc;
	if (int rc = placement_check(entry, "voxel", voxel, "origin", ox, oy, oz)) return rc;
	if (int rc = image_check(entry, W, H)) return rc;
	if (!positive_finite(sdf_trunc) || !positive_finite(depth_trunc)) {
		set_error("%s: sdf_trunc and depth_trunc must be positive and finite (got %g, %g)", entry, (double)sdf_trunc, (double)depth_trunc);
		return GSR_E_INVALID;
	}
	if (!std::isfinite(alpha_min)) { set_error("%s: alpha_min is not finite", entry); return GSR_E_INVALID; }
	TsdfArgs a;
	a.tsdf = tsdf; a.weight = weight; a.color = color; a.depth = depth; a.rgb = rgb; a.alpha = alpha; a.view = viewmatrix; a.proj = projmatrix;
	a.nx = nx; a.ny = ny; a.nz = nz; a.W = W; a.H = H;
	a.ox = ox; a.oy = oy; a.oz = oz; a.voxel = voxel; a.alpha_min = alpha_min; a.sdf_trunc = sdf_trunc; a.depth_trunc = depth_trunc;
	a.bx = ((uint32_t)nx + 63u) / 64u;
	a.bxy = a.bx * (((uint32_t)ny + TSDF_ROWS - 1u) / TSDF_ROWS);
	// (for n >= 2 each of ceil(n / 64), ceil(n / 4) and ceil(n / 8) is at most n / 2: the product is at most nx ny nz / 8 < 2^28)
	a.nblocks = a.bxy * (((uint32_t)nz + TSDF_KZ - 1u) / TSDF_KZ);
	// at most 2^16 blocks are launched (a thousand waves per CU) and each strides over the blocks beyond: a volume of 2 x 2 x 2^29 nodes
	// has 2^26 blocks of its own
	const uint32_t grid = a.nblocks < TSDF_MAX_GRID ? a.nblocks : TSDF_MAX_GRID;
	tsdf_integrate_kernel<<<grid, 64 * TSDF_ROWS, 0, stream>>>(a);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" size_t gsr_mesh_scratch_bytes(int nx, int ny, int nz) {
	const uint64_t N = volume_nodes(nx, ny, nz);
	return N ? mesh_carve(nullptr, N).bytes : 0;
}

extern "C" int gsr_mesh_count(const float* tsdf, const float* weight, int nx, int ny, int nz, float min_weight, void* scratch, size_t scratch_bytes,
                              uint64_t* counts, void* stream_) {
	const char* entry = "gsr_mesh_count";
	hipStream_t stream = (hipStream_t)stream_;
	if (!tsdf || !weight || !scratch || !counts) { set_error("%s: invalid argument (NULL pointer)", entry); return GSR_E_INVALID; }
	if (int rc = pointers_check(entry, {tsdf, weight})) return rc;
	if (int rc = aligned_check(entry, "scratch", scratch, 16)) return rc;
	if (int rc = aligned_check(entry, "counts", counts, 8)) return rc;
	uint64_t N64;
	if (int rc = volume_check(entry, nx, ny, nz, &N64)) return rc;
	if (std::isnan(min_weight)) { set_error("%s: min_weight is NaN", entry); return GSR_E_INVALID; }
	const MeshScratch s = mesh_carve(scratch, N64);
	if (scratch_bytes < s.bytes) {
		set_error("%s: scratch of %zu bytes, gsr_mesh_scratch_bytes(%d, %d, %d) = %zu", entry, scratch_bytes, nx, ny, nz, s.bytes);
		return GSR_E_INVALID;
	}
	const uint32_t N = (uint32_t)N64;
	mesh_classify_kernel<<<s.nblocks, MESH_BLOCK, 0, stream>>>(tsdf, weight, N, min_weight, s.cls);
	GSR_LAUNCH_CHECK(0, stream);
	mesh_count_kernel<<<s.nblocks, MESH_BLOCK, 0, stream>>>(s.cls, N, nx, ny, nz, s.vmask, s.tcnt, s.part);
	GSR_LAUNCH_CHECK(0, stream);
	scan_spine_kernel<<<1, 1024, 0, stream>>>(s.part, s.nblocks, s.vbase, s.tbase, (unsigned long long*)counts);
	GSR_LAUNCH_CHECK(0, stream);
	mesh_offsets_kernel<<<s.nblocks, MESH_BLOCK, 0, stream>>>(s.vmask, s.tcnt, N, s.vbase, s.tbase, s.vert_off, s.tri_off);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_mesh_emit(const float* tsdf, const float* weight, const float* color, int nx, int ny, int nz, float ox, float oy, float oz,
                             float voxel, float min_weight, const void* scratch, float* verts, float* vcolor, int* faces, uint64_t nV, uint64_t nT,
                             void* stream_) {
	const char* entry = "gsr_mesh_emit";
	hipStream_t stream = (hipStream_t)stream_;
	(void)min_weight;             // the classification is the one gsr_mesh_count left in the scratch
	if (!tsdf || !weight || !scratch) { set_error("%s: invalid argument (NULL pointer)", entry); return GSR_E_INVALID; }
	if (int rc = pointers_check(entry, {tsdf, weight, color, verts, vcolor, faces})) return rc;
	if (int rc = aligned_check(entry, "scratch", scratch, 16)) return rc;
	uint64_t N64;
	if (int rc = volume_check(entry, nx, ny, nz, &N64)) return rc;
	if (int rc = placement_check(entry, "voxel", voxel, "origin", ox, oy, oz)) return rc;
	if (nV >= LIMIT_2_31 || nT >= LIMIT_2_31 || 3 * nT >= LIMIT_2_31) {
		set_error("%s: nV and 3 * nT must be below 2^31 (got %llu vertices, %llu triangles)", entry, (unsigned long long)nV, (unsigned long long)nT);
		return GSR_E_INVALID;
	}
	if (nV == 0) return 0;
	if (!verts || (nT > 0 && !faces)) { set_error("%s: invalid argument (NULL verts or faces)", entry); return GSR_E_INVALID; }
	if ((color != nullptr) != (vcolor != nullptr)) { set_error("%s: color and vcolor must both be given or both be NULL", entry); return GSR_E_INVALID; }
	const MeshScratch s = mesh_carve(const_cast<void*>(scratch), N64);      // (read only: EmitArgs takes the arrays as pointers to const)
	EmitArgs a;
	a.tsdf = tsdf; a.color = color;
	a.cls = s.cls; a.vmask = s.vmask; a.vert_off = s.vert_off; a.tri_off = s.tri_off;
	a.verts = verts; a.vcolor = vcolor; a.faces = faces;
	a.N = (uint32_t)N64; a.nV = (uint32_t)nV; a.nT = (uint32_t)nT;
	a.nx = nx; a.ny = ny; a.nz = nz;
	a.ox = ox; a.oy = oy; a.oz = oz; a.voxel = voxel;
	mesh_emit_kernel<<<s.nblocks, MESH_BLOCK, 0, stream>>>(a);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}
