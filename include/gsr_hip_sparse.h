/* Block-sparse TSDF entries of libgsr_hip.so: the volume of gsr_hip_mesh.h cut into blocks of 8 x 8 x 8 nodes, of which only the blocks
 * near the surface get storage, so that a box of 2501^3 nodes at upstream 2DGS's voxel of 0.004 costs what its surface costs.
 * gsr_mesh.py drives them (SparseTSDFVolume) and utils/mesh_utils.py's extract_mesh_bounded(sparse=True) sits on top.  Upstream took this
 * from open3d's ScalableTSDFVolume (a hash of blocks on the host); the contract below is this project's own, and tests/sparse_ref.py
 * restates it in float64 on top of tests/mesh_ref.py.
 *
 * These entries were added under ABI 102 without a version change, as those of gsr_hip_mesh.h were: declared here, looked up by name,
 * gsr_version() stays 102.  The conventions of gsr_hip.h hold (float32 device pointers, the caller's stream, no host synchronisation, no
 * allocation, a refusal (GSR_E_INVALID) comes before any device work and launches nothing, gsr_last_error() names the entry), and so does
 * the promise of gsr_hip_mesh.h: no kernel of these entries uses a global atomic or waits for another workgroup, so the same inputs give
 * the same bytes.
 *
 * THE VOLUME is described as a dense one: nx x ny x nz nodes, origin (ox, oy, oz), voxel; node (i, j, k) sits at
 *       (fmaf(voxel, i, ox), fmaf(voxel, j, oy), fmaf(voxel, k, oz))
 *   the very expression of the dense kernels.  Block (bi, bj, bk) holds the nodes 8 bi .. 8 bi + 7 on each axis; the block grid is
 *   gx = ceil(nx / 8), gy, gz likewise; the block's linear index is (bk * gy + bj) * gx + bi and a node's local index in its block
 *   (lk * 8 + lj) * 8 + li.  A node of an edge block with i >= nx, j >= ny or k >= nz does not exist: it is never read as valid and
 *   never written.  Each dimension is >= 2, G = gx * gy * gz < 2^31, and a pool of `capacity` slots satisfies capacity * 512 < 2^31.
 *   All storage is the caller's:
 *     table          int32 [G], a DIRECT table (no hash: at 2501^3 nodes it is 123 MB, needs no probing and keeps every result a pure
 *                    function of the inputs): -1 untouched, -2 touched and waiting for a slot, >= 0 the block's slot.  Fresh: all -1.
 *     block_of_slot  int32 [capacity]: the block linear index of each slot
 *     tsdf, weight   float32 [capacity, 512];  color  float32 [capacity, 3, 512], optional.  The caller hands in zeros.
 *     counts         uint64 [2] on the device, 8-byte aligned: {slots allocated, slots wanted}; a fresh volume has {0, 0}
 *   The pool node index of a node is slot * 512 + local.  Slots at and beyond the allocated count (n_slots, or counts[0]) are never read
 *   or written by any entry; a table entry that names such a slot counts as a block without storage.
 *
 * gsr_sparse_tsdf_touch: marks the blocks one view needs.  For every node that exists, steps 1-3 of gsr_tsdf_integrate, word for word the
 *   rule of gsr_hip_mesh.h (z and p; the rasterizer's pixel (u, v) by rintf; d = depth[v, u] with 0 < d <= depth_trunc; alpha >= alpha_min).
 *   Then sdf = d - z, and the node is a BAND node iff -sdf_trunc <= sdf < sdf_trunc.  Every block that holds an existing node within one
 *   node (Chebyshev distance) of a band node, the band node's own block included, becomes -2 if it was -1; a block with a slot is never
 *   changed.  Nothing but `table` is written, and the only stores are plain stores of -2.  The kernel leaves a whole block before its
 *   node loop only when no node of it can pass steps 1-2 (its box lies behind the camera, or off one side of the image), decided with a
 *   margin far above float32's rounding.
 *
 * gsr_sparse_tsdf_allocate_scratch_bytes, gsr_sparse_tsdf_allocate: slots counts[0], counts[0] + 1, ... go to the -2 blocks in ascending
 *   block linear index while the slot is below `capacity`; block_of_slot is written for the new slots, the blocks that did not fit stay
 *   -2.  Then counts[0] = slots now allocated and counts[1] = allocated + still waiting: a caller that reads counts[1] > capacity makes a
 *   larger pool, copies the old slots and calls again, and the allocation continues where it stopped.  Two-level scan, no atomics.
 *   block_of_slot may be NULL when capacity is 0.  The scratch is 16-byte aligned and holds at least what the size query says, which is
 *   host arithmetic only and 0 for a size the entries refuse.
 *
 * gsr_sparse_tsdf_integrate: one view into the slots [0, n_slots), n_slots a host integer (the caller knows it from allocate's counts).
 *   Every existing node of those slots gets exactly steps 1-5 of gsr_tsdf_integrate with the same skip rules; a skipped node is NOT
 *   written: no plane, no byte.  color and rgb are both given or both NULL.  n_slots == 0 returns 0 without a launch.
 *
 * THE ISO-SURFACE (gsr_sparse_mesh_scratch_bytes, gsr_sparse_mesh_count, gsr_sparse_mesh_emit).  The definitions of gsr_hip_mesh.h hold:
 *   valid and inside, cell validity, the Kuhn split, the seven edge directions, the vertex-existence rule, the triangle tables and their
 *   orientation, and the rule for tsdf == 0.  They are evaluated over the pool: a node of a block without storage is invalid; a cell
 *   exists iff its low corner exists and i < nx - 1, j < ny - 1, k < nz - 1; the other seven nodes of a cell, and the cells below a node,
 *   are found through `table`.  Vertex order: ascending (pool node index, direction).  Triangle order: ascending (pool cell index = that of
 *   its low corner, tetrahedron, triangle).  Positions and colours are formed by the dense emit's arithmetic on the global (i, j, k).
 *   gsr_sparse_mesh_scratch_bytes(n_slots): host arithmetic; 0 for n_slots == 0 (nothing is needed) and for n_slots * 512 >= 2^31.
 *   gsr_sparse_mesh_count writes counts[0] = nV and counts[1] = nT (two uint64 on the device, exact); with n_slots == 0 both are 0 and the
 *   scratch may be NULL.  gsr_sparse_mesh_emit, with the scratch the count left, writes verts [nV, 3], vcolor [nV, 3] (given iff color is)
 *   and faces [nT, 3], exactly those rows; nV == 0 is a no-op that returns 0.
 *
 * WHY THE SURFACE IS THE DENSE ONE.  Touch every view, allocate once, then integrate every view.  A cell that emits a triangle has a
 *   node whose fused tsdf is negative, so some view gave that node t < 0: it was a band node of that view (t < 0 <=> sdf < 0, and it
 *   was not skipped, so sdf >= -sdf_trunc).  The one-node margin then allocated every block that holds a node of a cell around that
 *   node: the whole cell, and every cell that shares one of its sign-change edges (each such edge has an inside end).  With every view
 *   touched before any is fused, an allocated node receives the same updates in the same order as in a dense volume and holds the dense
 *   values; a cell with a node that has no storage has no inside node (the margin would have allocated it), so the dense volume emits
 *   nothing there either.  Checked in float64 on the fusion fixture at three voxel sizes: vertices, colours and faces identical (tests/test_sparse_ref.py).
 *
 * GSR_E_INVALID: a NULL table, counts, depth, viewmatrix or projmatrix; a NULL block_of_slot, tsdf, weight or scratch where slots are in
 *   use (capacity > 0 for allocate, n_slots > 0 elsewhere); color without rgb or rgb without color; (nV > 0) NULL verts, (nT > 0) NULL
 *   faces, vcolor without color or color without vcolor; a dimension below 2 or 2^31 blocks or more; capacity * 512 >= 2^31;
 *   n_slots > capacity; voxel, sdf_trunc or depth_trunc not positive and finite; an origin or alpha_min that is not finite; W or H
 *   below 1 or W * H >= 2^31; a min_weight that is NaN; a scratch that is too small or not 16-byte aligned; counts not 8-byte aligned;
 *   another pointer not 4-byte aligned; nV >= 2^31 or 3 * nT >= 2^31. */
#ifndef GSR_HIP_SPARSE_H_
#define GSR_HIP_SPARSE_H_

#include "gsr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int gsr_sparse_tsdf_touch(int32_t* table, int nx, int ny, int nz, float ox, float oy, float oz, float voxel, const float* depth,
                          const float* alpha, float alpha_min, int W, int H, const float* viewmatrix, const float* projmatrix, float sdf_trunc,
                          float depth_trunc, void* stream);
size_t gsr_sparse_tsdf_allocate_scratch_bytes(int nx, int ny, int nz);
int gsr_sparse_tsdf_allocate(int32_t* table, int nx, int ny, int nz, int32_t* block_of_slot, uint64_t capacity, uint64_t* counts, void* scratch,
                             size_t scratch_bytes, void* stream);
int gsr_sparse_tsdf_integrate(const int32_t* block_of_slot, uint64_t n_slots, uint64_t capacity, float* tsdf, float* weight, float* color, int nx,
                              int ny, int nz, float ox, float oy, float oz, float voxel, const float* depth, const float* rgb, const float* alpha,
                              float alpha_min, int W, int H, const float* viewmatrix, const float* projmatrix, float sdf_trunc, float depth_trunc,
                              void* stream);
size_t gsr_sparse_mesh_scratch_bytes(uint64_t n_slots);
int gsr_sparse_mesh_count(const int32_t* table, const int32_t* block_of_slot, uint64_t n_slots, uint64_t capacity, const float* tsdf,
                          const float* weight, int nx, int ny, int nz, float min_weight, void* scratch, size_t scratch_bytes, uint64_t* counts,
                          void* stream);
int gsr_sparse_mesh_emit(const int32_t* table, const int32_t* block_of_slot, uint64_t n_slots, uint64_t capacity, const float* tsdf,
                         const float* weight, const float* color, int nx, int ny, int nz, float ox, float oy, float oz, float voxel, float min_weight,
                         const void* scratch, float* verts, float* vcolor, int* faces, uint64_t nV, uint64_t nT, void* stream);

#ifdef __cplusplus
}
#endif
#endif
