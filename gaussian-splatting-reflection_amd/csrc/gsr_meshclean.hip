// Mesh clean-up (include/gsr_hip_meshclean.h has the contract): the connected components of an indexed triangle mesh by a union-find on
// the device, the cluster_to_keep largest kept, and the mesh compacted.  One thread per vertex or per face, 256 per block, ceil(n / 256)
// blocks (nV < 2^31 and 3 nT < 2^31 keep that inside grid.x).
//
// gsr_mesh_clean_count, in launch order (a kernel boundary is the only coherence these kernels rely on; inside a launch only atomics
// carry information between workgroups, and no kernel waits for another workgroup):
//   init      vertex -> parent = itself, size = 0, used = 0; the digit histograms and the two counters that are added to
//   union     face   -> unite(a, b), unite(b, c) on parent, which keeps parent[v] <= v: atomic minimum only (see unite)
//   flatten   vertex -> parent = its root, which is the smallest index of its component: parent IS the label from here on
//   sizes     face   -> tri_label; size[label] += 1, added up per wave and then per block first (the faces of a block mostly share a
//             label); the ignored faces
//   digits    x 4, vertex -> a radix select of the k-th largest root size, most significant byte first: each pass counts one byte of
//             the sizes that match the bytes chosen so far; every block re-derives those from the earlier passes' histograms
//   threshold ONE block -> counts[2] = C, counts[4] = thr
//   flag      face   -> tri_size; keep = size >= thr; used[a] = used[b] = used[c] = 1 for a kept face
//   count     block  -> sums of used and keep (gsr_scan.hpp's packing); the kept components
//   spine     ONE block scans the block sums (gsr_scan.hpp) and writes counts[0..1]
//   offsets   vertex, face -> its new row
// gsr_mesh_clean_emit is one kernel: a used vertex copies its row(s), a kept face writes the new rows of its corners.
//
// EVERY LOOP ENDS WHATEVER ANOTHER WORKGROUP DOES.  All stores to parent[] are the initial parent[v] = v and atomic minima, so every
// value parent[v] ever holds is <= v, and a load — however stale — returns one of them.  Each loop below names the integer that strictly
// decreases in it.  There is no compare-and-swap retry and no spin on a value another workgroup writes.
// Host side: the checks that are not specific to an entry are gsr_host.hpp's; the scratch is CleanScratch, typed pointers carved by
// clean_carve (a NULL base answers gsr_mesh_clean_scratch_bytes).
#include "gsr_host.hpp"
#include "gsr_scan.hpp"
#include "../../include/gsr_hip_meshclean.h"

namespace gsr {

#define CLEAN_BLOCK SCAN_BLOCK
#define CLEAN_PASSES 4            // bytes of a size, most significant first
#define CLEAN_AGG_ROUNDS 4        // labels a wave adds up before its remaining lanes add for themselves

// scratch of gsr_mesh_clean_count, shared with gsr_mesh_clean_emit (which only reads it): nV vertices in `vblocks` blocks, nT faces in
// `tblocks`; nblocks is the larger of the two
struct CleanScratch {
	uint32_t* parent;      // nV       union-find parent; behind `flatten` the label
	uint32_t* size;        // nV       counted faces of the component, at its root
	uint32_t* vert_off;    // nV       new row of the vertex
	uint32_t* tri_off;     // nT       new row of the face
	uint8_t* used;         // nV       a kept face names the vertex
	uint8_t* keep;         // nT       the face is kept
	uint32_t* hist;        // 256 * CLEAN_PASSES  digit counts of the radix select, 256 per pass
	uint32_t* part;        // nblocks  block sums: used vertices | kept faces << 16; block b has vertices AND faces 256 b ...
	uint32_t* vbase;       // nblocks  used vertices in front of the block
	uint32_t* tbase;       // nblocks  kept faces in front of the block
	size_t bytes;
	uint32_t vblocks, tblocks, nblocks;
};
static CleanScratch clean_carve(void* base, uint64_t nV, uint64_t nT) {
	Carver c(base);
	CleanScratch s;
	s.vblocks = (uint32_t)((nV + CLEAN_BLOCK - 1) / CLEAN_BLOCK);
	s.tblocks = (uint32_t)((nT + CLEAN_BLOCK - 1) / CLEAN_BLOCK);
	s.nblocks = s.vblocks > s.tblocks ? s.vblocks : s.tblocks;
	s.parent = c.take<uint32_t>(nV);
	s.size = c.take<uint32_t>(nV);
	s.vert_off = c.take<uint32_t>(nV);
	s.tri_off = c.take<uint32_t>(nT);
	s.used = c.take<uint8_t>(nV);
	s.keep = c.take<uint8_t>(nT);
	s.hist = c.take<uint32_t>(256 * CLEAN_PASSES);
	s.part = c.take<uint32_t>(s.nblocks);
	s.vbase = c.take<uint32_t>(s.nblocks);
	s.tbase = c.take<uint32_t>(s.nblocks);
	s.bytes = c.size();
	return s;
}

// ------------------------------------------------------------------------------------------------------------ the union-find
// The walks read parent[] with PLAIN loads, which this CU's L1 may serve: whatever they return is a value parent[x] has held, and that is
// all the arguments below ask of a load.  (L2-served agent-scope loads were measured beside them: 0.73 against 0.635 ms for the whole
// clean-up of a 1.28 M-face mesh; DESIGN.md, "Mesh clean-up".)  The minimum is an agent-scope atomic: it is executed at the memory side
// and returns the value it replaced, whichever XCD asks.
__device__ __forceinline__ uint32_t parent_load(const uint32_t* p) { return *p; }
__device__ __forceinline__ uint32_t parent_min(uint32_t* p, uint32_t v) {
	return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// An ancestor of x that was a root when it was read, with path halving.  Halving stores the grandparent by atomic minimum: both it and
// the value it replaces have been parents of x, and all of those stay connected among themselves below x, so no link is lost.
__device__ __forceinline__ uint32_t find_root(uint32_t* parent, uint32_t x) {
	// ENDS: x strictly decreases.  Every value parent[x] ever held is <= x, so p < x or the loop leaves, and gp < p likewise; x >= 0.
	for (;;) {
		const uint32_t p = parent_load(parent + x);
		if (p >= x) return x;
		const uint32_t gp = parent_load(parent + p);
		if (gp >= p) return p;
		parent_min(parent + x, gp);
		x = gp;
	}
}

// Joins the components of a and b.  A link is parent[hi] = lo with lo < hi, made by atomic minimum, which tells what it replaced:
//   hi        hi was a root and now hangs under lo: done
//   lo        the link was there: done
//   another   `old` was (old < lo: still is) the parent of hi.  Either way hi is linked to min(old, lo), and what is left to join is
//             old with lo; their roots serve as well, since a root is connected to its vertex.
__device__ __forceinline__ void unite(uint32_t* parent, uint32_t a, uint32_t b) {
	a = find_root(parent, a);
	b = find_root(parent, b);
	uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
	// ENDS: hi strictly decreases.  old <= hi always (above) and the loop leaves at old == hi, so old < hi; lo < hi; find_root(x) <= x:
	// the next pair's larger element is below hi.  No step waits for, or repeats because of, what another workgroup did.
	while (hi != lo) {
		const uint32_t old = parent_min(parent + hi, lo);
		if (old >= hi || old == lo) break;
		const uint32_t ra = find_root(parent, old), rb = find_root(parent, lo);
		hi = ra > rb ? ra : rb;
		lo = ra > rb ? rb : ra;
	}
}

// The three indices of face t, and whether the face is counted: all in [0, nV) (one unsigned compare each) and pairwise distinct.
__device__ __forceinline__ bool counted_face(const int* __restrict__ faces, uint32_t t, uint32_t nV, uint32_t& a, uint32_t& b, uint32_t& c) {
	const int* f = faces + 3 * (size_t)t;
	a = (uint32_t)f[0];
	b = (uint32_t)f[1];
	c = (uint32_t)f[2];
	return a < nV && b < nV && c < nV && a != b && b != c && a != c;
}

__global__ void __launch_bounds__(CLEAN_BLOCK)
clean_init_kernel(uint32_t nV, uint32_t* __restrict__ parent, uint32_t* __restrict__ size, uint8_t* __restrict__ used, uint32_t* __restrict__ hist,
                  unsigned long long* __restrict__ counts) {
	const uint32_t v = blockIdx.x * CLEAN_BLOCK + threadIdx.x;
	if (v < nV) {
		parent[v] = v;
		size[v] = 0;
		used[v] = 0;
	}
	if (blockIdx.x == 0) {
#pragma unroll
		for (int p = 0; p < CLEAN_PASSES; p++) hist[p * 256 + threadIdx.x] = 0;
		if (threadIdx.x == 0) { counts[3] = 0; counts[5] = 0; }
	}
}

__global__ void __launch_bounds__(CLEAN_BLOCK)
clean_union_kernel(const int* __restrict__ faces, uint32_t nV, uint32_t nT, uint32_t* parent) {
	const uint32_t t = blockIdx.x * CLEAN_BLOCK + threadIdx.x;
	uint32_t a, b, c;
	if (t >= nT || !counted_face(faces, t, nV, a, b, c)) return;
	unite(parent, a, b);
	unite(parent, b, c);
}

// No link is made in this launch, so a vertex that reads as its own parent IS a root (a vertex that hangs under another did so when the
// launch began), and the root of a component is its smallest index: the minimum below leaves exactly the root in parent[v].
__global__ void __launch_bounds__(CLEAN_BLOCK)
clean_flatten_kernel(uint32_t nV, uint32_t* parent) {
	const uint32_t v = blockIdx.x * CLEAN_BLOCK + threadIdx.x;
	if (v >= nV) return;
	const uint32_t root = find_root(parent, v);
	if (root != v) parent_min(parent + v, root);
}

__global__ void __launch_bounds__(CLEAN_BLOCK)
clean_sizes_kernel(const int* __restrict__ faces, uint32_t nV, uint32_t nT, const uint32_t* __restrict__ label, uint32_t* size, int* __restrict__ tri_label,
                   unsigned long long* counts) {
	const uint32_t t = blockIdx.x * CLEAN_BLOCK + threadIdx.x;
	const int lane = threadIdx.x & 63;
	uint32_t a, b, c, l = 0;
	const bool in = t < nT, ok = in && counted_face(faces, t, nV, a, b, c);
	if (ok) l = label[a];
	if (in && tri_label) tri_label[t] = ok ? (int)l : -1;
	if (in && !ok) atomicAdd(counts + 5, 1ull);              // (the compiler adds the wave's lanes up: one atomic per wave)
	// one add per (wave, label) for the first labels of the wave; a wave of floaters leaves the loop after CLEAN_AGG_ROUNDS.  The first
	// label's count goes through LDS: where the four waves of the block agree on it (inside a large component they do), wave 0 adds once.
	__shared__ uint32_t first_label[CLEAN_BLOCK / 64], first_count[CLEAN_BLOCK / 64];
	const int wave = threadIdx.x >> 6;
	if (lane == 0) first_count[wave] = 0;
	bool pending = ok;
	for (int r = 0; r < CLEAN_AGG_ROUNDS; r++) {
		const unsigned long long todo = __ballot(pending);
		if (todo == 0) break;
		const int leader = __ffsll((long long)todo) - 1;
		const uint32_t ll = __shfl(l, leader);
		const bool mine = pending && l == ll;
		const unsigned long long same = __ballot(mine);
		if (lane == leader) {
			if (r == 0) { first_label[wave] = ll; first_count[wave] = (uint32_t)__popcll(same); }
			else atomicAdd(size + ll, (uint32_t)__popcll(same));
		}
		pending = pending && !mine;
	}
	__syncthreads();
	if (threadIdx.x < CLEAN_BLOCK / 64 && first_count[threadIdx.x]) {
		// lane w speaks for wave w: the first wave that holds a label adds for all the waves that hold it
		uint32_t sum = 0;
		bool first = true;
		for (int w = 0; w < CLEAN_BLOCK / 64; w++) {
			if (first_count[w] == 0 || first_label[w] != first_label[threadIdx.x]) continue;
			if (w < (int)threadIdx.x) first = false;
			sum += first_count[w];
		}
		if (first) atomicAdd(size + first_label[threadIdx.x], sum);
	}
	if (pending) atomicAdd(size + l, 1u);
}

// ------------------------------------------------------------------------------------------------------------ the k-th largest size
// The radix select's state after the first `upto` passes, re-derived by a whole block from their histograms: the bytes chosen so far
// (prefix), the rank k that is left among the sizes that carry them, and C.  lds: 6 words.  Thread t looks at digit 255 - t, so that the
// block's exclusive scan counts the sizes with a LARGER digit.
struct CleanSelect { uint32_t prefix, k, C; };
__device__ __forceinline__ uint32_t clean_shift(int pass) { return 8u * (uint32_t)(CLEAN_PASSES - 1 - pass); }
__device__ CleanSelect clean_select(const uint32_t* __restrict__ hist, int upto, unsigned long long cluster_to_keep, uint32_t* lds) {
	CleanSelect s = {0u, 0u, 0u};
	const uint32_t digit = 255u - threadIdx.x;
	for (int q = 0; q < upto; q++) {
		const uint32_t h = hist[q * 256 + digit];
		if (q == 0) {
			s.C = block_sum(h, lds);                              // every root of size >= 1 is in the first histogram
			s.k = cluster_to_keep < s.C ? (uint32_t)cluster_to_keep : s.C;      // the clamp
			if (s.C == 0) return s;
		}
		if (threadIdx.x == 0) { lds[4] = 0; lds[5] = 1; }
		const uint32_t above = block_exclusive(h, lds);
		if (above < s.k && s.k <= above + h) { lds[4] = digit; lds[5] = s.k - above; }       // exactly one digit
		__syncthreads();
		s.prefix |= lds[4] << clean_shift(q);
		s.k = lds[5];
		__syncthreads();
	}
	return s;
}

__global__ void __launch_bounds__(CLEAN_BLOCK)
clean_digits_kernel(uint32_t nV, const uint32_t* __restrict__ label, const uint32_t* __restrict__ size, uint32_t* hist, int pass,
                    unsigned long long cluster_to_keep) {
	__shared__ uint32_t lds[6], local[256];
	local[threadIdx.x] = 0;
	__syncthreads();
	const CleanSelect s = clean_select(hist, pass, cluster_to_keep, lds);
	if (pass > 0 && s.C == 0) return;
	const uint32_t v = blockIdx.x * CLEAN_BLOCK + threadIdx.x;
	if (v < nV && label[v] == v) {
		const uint32_t sz = size[v];
		const bool match = pass == 0 || (sz >> clean_shift(pass - 1)) == (s.prefix >> clean_shift(pass - 1));
		if (sz >= 1 && match) atomicAdd(local + ((sz >> clean_shift(pass)) & 255u), 1u);
	}
	__syncthreads();
	if (local[threadIdx.x]) atomicAdd(hist + pass * 256 + threadIdx.x, local[threadIdx.x]);
}

__global__ void __launch_bounds__(CLEAN_BLOCK)
clean_threshold_kernel(const uint32_t* __restrict__ hist, unsigned long long cluster_to_keep, unsigned long long min_triangles,
                       unsigned long long* __restrict__ counts) {
	__shared__ uint32_t lds[6];
	const CleanSelect s = clean_select(hist, CLEAN_PASSES, cluster_to_keep, lds);
	if (threadIdx.x == 0) {
		const unsigned long long kth = s.C ? (unsigned long long)s.prefix : 0ull;
		counts[2] = s.C;
		counts[4] = kth > min_triangles ? kth : min_triangles;
	}
}

__global__ void __launch_bounds__(CLEAN_BLOCK)
clean_flag_kernel(const int* __restrict__ faces, uint32_t nV, uint32_t nT, const uint32_t* __restrict__ label, const uint32_t* __restrict__ size,
                  const unsigned long long* __restrict__ counts, int* __restrict__ tri_size, uint8_t* __restrict__ keep, uint8_t* used) {
	const uint32_t t = blockIdx.x * CLEAN_BLOCK + threadIdx.x;
	if (t >= nT) return;
	uint32_t a, b, c, sz = 0;
	const bool ok = counted_face(faces, t, nV, a, b, c);
	if (ok) sz = size[label[a]];
	if (tri_size) tri_size[t] = (int)sz;
	const bool kept = ok && (unsigned long long)sz >= counts[4];
	keep[t] = kept ? 1 : 0;
	if (kept) { used[a] = 1; used[b] = 1; used[c] = 1; }      // (whoever stores, stores 1)
}

__global__ void __launch_bounds__(CLEAN_BLOCK)
clean_count_kernel(uint32_t nV, uint32_t nT, const uint32_t* __restrict__ label, const uint32_t* __restrict__ size, const uint8_t* __restrict__ used,
                   const uint8_t* __restrict__ keep, uint32_t* __restrict__ part, unsigned long long* counts) {
	__shared__ uint32_t lds[4];
	const uint32_t n = blockIdx.x * CLEAN_BLOCK + threadIdx.x;
	const uint32_t u = n < nV ? (uint32_t)used[n] : 0u, k = n < nT ? (uint32_t)keep[n] : 0u;
	const uint32_t sum = block_sum(u | (k << 16), lds);
	uint32_t comp = 0;
	if (n < nV && label[n] == n) {
		const uint32_t sz = size[n];
		comp = (sz >= 1 && (unsigned long long)sz >= counts[4]) ? 1u : 0u;
	}
	const uint32_t comps = block_sum(comp, lds);
	if (threadIdx.x == 0) {
		part[blockIdx.x] = sum;
		if (comps) atomicAdd(counts + 3, (unsigned long long)comps);
	}
}

__global__ void __launch_bounds__(CLEAN_BLOCK)
clean_offsets_kernel(uint32_t nV, uint32_t nT, const uint8_t* __restrict__ used, const uint8_t* __restrict__ keep, const uint32_t* __restrict__ vbase,
                     const uint32_t* __restrict__ tbase, uint32_t* __restrict__ vert_off, uint32_t* __restrict__ tri_off) {
	__shared__ uint32_t lds[4];
	const uint32_t n = blockIdx.x * CLEAN_BLOCK + threadIdx.x;
	const uint32_t u = n < nV ? (uint32_t)used[n] : 0u, k = n < nT ? (uint32_t)keep[n] : 0u;
	const uint32_t ex = block_exclusive(u | (k << 16), lds);         // (a block sums to at most 256 | 256 << 16)
	if (n < nV) vert_off[n] = vbase[blockIdx.x] + (ex & 0xffffu);
	if (n < nT) tri_off[n] = tbase[blockIdx.x] + (ex >> 16);
}

// nV == 0 or nT == 0: no component, no threshold; every face is ignored.
__global__ void __launch_bounds__(CLEAN_BLOCK)
clean_empty_kernel(uint32_t nT, int* __restrict__ tri_label, int* __restrict__ tri_size, unsigned long long* __restrict__ counts) {
	const uint32_t t = blockIdx.x * CLEAN_BLOCK + threadIdx.x;
	if (t < nT) {
		if (tri_label) tri_label[t] = -1;
		if (tri_size) tri_size[t] = 0;
	}
	if (t < 6) counts[t] = t == 5 ? (unsigned long long)nT : 0ull;
}

struct CleanEmitArgs {
	const float* verts; const float* vcolor; const int* faces;
	const uint8_t* used; const uint8_t* keep; const uint32_t* vert_off; const uint32_t* tri_off;
	float* verts_out; float* vcolor_out; int* faces_out;
	uint32_t nV, nT, nV_out, nT_out;
};

__global__ void __launch_bounds__(CLEAN_BLOCK)
clean_emit_kernel(const CleanEmitArgs a) {
	const uint32_t n = blockIdx.x * CLEAN_BLOCK + threadIdx.x;
	if (n < a.nV && a.used[n]) {
		const uint32_t at = a.vert_off[n];
		if (at < a.nV_out) {                                           // (always with the counts of this scratch: no row beyond nV_out)
			// the rows move as words: bit for bit, NaN payloads included
			const uint32_t* src = (const uint32_t*)a.verts + 3 * (size_t)n;
			uint32_t* dst = (uint32_t*)a.verts_out + 3 * (size_t)at;
			dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
			if (a.vcolor_out) {
				const uint32_t* cs = (const uint32_t*)a.vcolor + 3 * (size_t)n;
				uint32_t* cd = (uint32_t*)a.vcolor_out + 3 * (size_t)at;
				cd[0] = cs[0]; cd[1] = cs[1]; cd[2] = cs[2];
			}
		}
	}
	if (n < a.nT && a.keep[n]) {
		uint32_t i, j, k;
		const uint32_t at = a.tri_off[n];
		// (a kept face is a counted one; asked again so that no scratch, whatever it holds, turns an index of the mesh into an address)
		if (at < a.nT_out && counted_face(a.faces, n, a.nV, i, j, k)) {
			int* o = a.faces_out + 3 * (size_t)at;
			o[0] = (int)a.vert_off[i];
			o[1] = (int)a.vert_off[j];
			o[2] = (int)a.vert_off[k];
		}
	}
}

// ------------------------------------------------------------------------------------------------------------ host side
// nV < 2^31 and 3 nT < 2^31
static bool clean_sizes_fit(uint64_t nV, uint64_t nT) { return nV < LIMIT_2_31 && nT < LIMIT_2_31 && 3 * nT < LIMIT_2_31; }
static int clean_size_check(const char* entry, uint64_t nV, uint64_t nT) {
	if (!clean_sizes_fit(nV, nT)) {
		set_error("%s: nV and 3 * nT must be below 2^31 (got %llu vertices, %llu faces)", entry, (unsigned long long)nV, (unsigned long long)nT);
		return GSR_E_INVALID;
	}
	return 0;
}

}  // namespace gsr

using namespace gsr;

extern "C" size_t gsr_mesh_clean_scratch_bytes(uint64_t nV, uint64_t nT) {
	if (!clean_sizes_fit(nV, nT)) return 0;
	return clean_carve(nullptr, nV, nT).bytes;
}

extern "C" int gsr_mesh_clean_count(const int* faces, uint64_t nV64, uint64_t nT64, uint64_t cluster_to_keep, uint64_t min_triangles, int* tri_label,
                                    int* tri_size, void* scratch, size_t scratch_bytes, uint64_t* counts_, void* stream_) {
	const char* entry = "gsr_mesh_clean_count";
	hipStream_t stream = (hipStream_t)stream_;
	const bool empty = nV64 == 0 || nT64 == 0;
	if (!counts_ || (!empty && (!faces || !scratch))) { set_error("%s: invalid argument (NULL pointer)", entry); return GSR_E_INVALID; }
	if (int rc = pointers_check(entry, {faces, tri_label, tri_size})) return rc;
	if (int rc = aligned_check(entry, "scratch", scratch, 16)) return rc;
	if (int rc = aligned_check(entry, "counts", counts_, 8)) return rc;
	if (int rc = clean_size_check(entry, nV64, nT64)) return rc;
	if (cluster_to_keep == 0) { set_error("%s: cluster_to_keep must be at least 1", entry); return GSR_E_INVALID; }
	const CleanScratch s = clean_carve(scratch, nV64, nT64);
	if (!empty && scratch_bytes < s.bytes) {
		set_error("%s: scratch of %zu bytes, gsr_mesh_clean_scratch_bytes(%llu, %llu) = %zu", entry, scratch_bytes, (unsigned long long)nV64,
		          (unsigned long long)nT64, s.bytes);
		return GSR_E_INVALID;
	}
	unsigned long long* counts = (unsigned long long*)counts_;
	const uint32_t nV = (uint32_t)nV64, nT = (uint32_t)nT64;
	if (empty) {
		clean_empty_kernel<<<s.tblocks ? s.tblocks : 1u, CLEAN_BLOCK, 0, stream>>>(nT, tri_label, tri_size, counts);
		GSR_LAUNCH_CHECK(0, stream);
		return 0;
	}
	clean_init_kernel<<<s.vblocks, CLEAN_BLOCK, 0, stream>>>(nV, s.parent, s.size, s.used, s.hist, counts);
	GSR_LAUNCH_CHECK(0, stream);
	clean_union_kernel<<<s.tblocks, CLEAN_BLOCK, 0, stream>>>(faces, nV, nT, s.parent);
	GSR_LAUNCH_CHECK(0, stream);
	clean_flatten_kernel<<<s.vblocks, CLEAN_BLOCK, 0, stream>>>(nV, s.parent);
	GSR_LAUNCH_CHECK(0, stream);
	clean_sizes_kernel<<<s.tblocks, CLEAN_BLOCK, 0, stream>>>(faces, nV, nT, s.parent, s.size, tri_label, counts);
	GSR_LAUNCH_CHECK(0, stream);
	for (int pass = 0; pass < CLEAN_PASSES; pass++) {
		clean_digits_kernel<<<s.vblocks, CLEAN_BLOCK, 0, stream>>>(nV, s.parent, s.size, s.hist, pass, cluster_to_keep);
		GSR_LAUNCH_CHECK(0, stream);
	}
	clean_threshold_kernel<<<1, CLEAN_BLOCK, 0, stream>>>(s.hist, cluster_to_keep, min_triangles, counts);
	GSR_LAUNCH_CHECK(0, stream);
	clean_flag_kernel<<<s.tblocks, CLEAN_BLOCK, 0, stream>>>(faces, nV, nT, s.parent, s.size, counts, tri_size, s.keep, s.used);
	GSR_LAUNCH_CHECK(0, stream);
	clean_count_kernel<<<s.nblocks, CLEAN_BLOCK, 0, stream>>>(nV, nT, s.parent, s.size, s.used, s.keep, s.part, counts);
	GSR_LAUNCH_CHECK(0, stream);
	scan_spine_kernel<<<1, 1024, 0, stream>>>(s.part, s.nblocks, s.vbase, s.tbase, counts);
	GSR_LAUNCH_CHECK(0, stream);
	clean_offsets_kernel<<<s.nblocks, CLEAN_BLOCK, 0, stream>>>(nV, nT, s.used, s.keep, s.vbase, s.tbase, s.vert_off, s.tri_off);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}

extern "C" int gsr_mesh_clean_emit(const float* verts, const float* vcolor, const int* faces, uint64_t nV, uint64_t nT, const void* scratch,
                                   float* verts_out, float* vcolor_out, int* faces_out, uint64_t nV_out, uint64_t nT_out, void* stream_) {
	const char* entry = "gsr_mesh_clean_emit";
	hipStream_t stream = (hipStream_t)stream_;
	if (int rc = pointers_check(entry, {verts, vcolor, faces, verts_out, vcolor_out, faces_out})) return rc;
	if (int rc = aligned_check(entry, "scratch", scratch, 16)) return rc;
	if (int rc = clean_size_check(entry, nV, nT)) return rc;
	if (nV_out > nV || nT_out > nT) {
		set_error("%s: nV_out and nT_out cannot exceed nV and nT (got %llu of %llu vertices, %llu of %llu faces)", entry, (unsigned long long)nV_out,
		          (unsigned long long)nV, (unsigned long long)nT_out, (unsigned long long)nT);
		return GSR_E_INVALID;
	}
	if (nT_out == 0) return 0;
	if (!verts || !faces || !scratch || !verts_out || !faces_out) { set_error("%s: invalid argument (NULL pointer)", entry); return GSR_E_INVALID; }
	if ((vcolor != nullptr) != (vcolor_out != nullptr)) { set_error("%s: vcolor and vcolor_out must both be given or both be NULL", entry); return GSR_E_INVALID; }
	const CleanScratch s = clean_carve(const_cast<void*>(scratch), nV, nT);      // (read only: CleanEmitArgs takes the arrays as pointers to const)
	CleanEmitArgs a;
	a.verts = verts; a.vcolor = vcolor; a.faces = faces;
	a.used = s.used; a.keep = s.keep; a.vert_off = s.vert_off; a.tri_off = s.tri_off;
	a.verts_out = verts_out; a.vcolor_out = vcolor_out; a.faces_out = faces_out;
	a.nV = (uint32_t)nV; a.nT = (uint32_t)nT; a.nV_out = (uint32_t)nV_out; a.nT_out = (uint32_t)nT_out;
	clean_emit_kernel<<<s.nblocks, CLEAN_BLOCK, 0, stream>>>(a);
	GSR_LAUNCH_CHECK(0, stream);
	return 0;
}
