/* Mesh-extraction entries of libgsr_hip.so: TSDF fusion of rendered surface-depth maps into a dense voxel grid, and the iso-surface of
 * that grid as an indexed triangle mesh (marching tetrahedra on the Kuhn split).  gsr_mesh.py drives them (TSDFVolume, Mesh,
 * save_mesh_ply) and utils/mesh_utils.py puts the reference's GaussianExtractor on top.  The reference has no code for this (it dropped
 * its open3d path), so the contract below is this project's own; tests/mesh_ref.py restates both halves in float64.
 *
 * These entries were added under ABI 102 without a version change (as the knn, metrics, viewer, raw-parameter, env-scope, environment-map
 * and densification-plan entries were): they are declared here and not in gsr_hip.h, gsr_version() stays 102, and a binding looks them up
 * by name (a library built before them lacks them).  The conventions of gsr_hip.h hold: float32 device pointers, the caller's stream, no
 * host synchronisation, no allocation, a refusal (GSR_E_INVALID) comes before any device work and launches nothing, gsr_last_error()
 * names the entry.  In addition: no kernel of these entries uses an atomic or waits for another workgroup (the two scans are two-level:
 * per-block sums, one block over the sums, per-block offsets), so the same inputs give the same bytes.
 *
 * THE VOLUME.  nx x ny x nz nodes, x fastest: node (i, j, k) has the linear index (k * ny + j) * nx + i and sits at
 *       (fmaf(voxel, i, ox), fmaf(voxel, j, oy), fmaf(voxel, k, oz))
 *   Planes, all float32 and caller-owned: tsdf [nz, ny, nx], weight [nz, ny, nx], optional color [3, nz, ny, nx].  A fresh volume is all
 *   zeros.  Each dimension is >= 2 and nx * ny * nz < 2^31.
 *
 * gsr_tsdf_integrate: one view into the volume.  viewmatrix and projmatrix are device pointers to 16 floats each in the layout every
 *   rasterizer entry takes (the reference's transposed matrices: element [4 * c + r] multiplies coordinate c into output r).  color and
 *   rgb are both given or both NULL.  Per node at world position X, in this order:
 *     1. z = V[2] X.x + V[6] X.y + V[10] X.z + V[14] and the homogeneous p = projmatrix applied to X (the rasterizers' transformPoint4x4).
 *        The node is skipped unless z > 0 and p.w > 0.
 *     2. px = ((p.x / p.w + 1) * W - 1) / 2, py = ((p.y / p.w + 1) * H - 1) / 2: continuous pixel coordinates in the RASTERIZER's
 *        convention, in which pixel (u, v) is centred on (u, v).  This is deliberately not the grid of utils/point_utils.py's
 *        depths_to_points, which is shifted by half a pixel against the rasterizer: a depth the rasterizer wrote into pixel (u, v) is
 *        read back by the nodes that project into that pixel's square.  u = rintf(px), v = rintf(py) (ties to even); skipped unless
 *        0 <= u < W and 0 <= v < H.
 *     3. d = depth[v, u]; skipped unless d > 0 and d <= depth_trunc (a NaN depth skips).  With alpha: skipped unless
 *        alpha[v, u] >= alpha_min (a NaN alpha skips).
 *     4. sdf = d - z; skipped if sdf < -sdf_trunc; t = fminf(1, sdf / sdf_trunc).
 *     5. with w = weight[node]:  tsdf = (tsdf * w + t) / (w + 1);  every colour channel c likewise from rgb[c, v, u];  weight = w + 1.
 *   A skipped node is NOT written: no plane, no byte.  (Contraction of a multiply and an add into an fma is left to the compiler; the
 *   decisions of steps 1-4 are what tests pin exactly, away from their thresholds.)
 *   GSR_E_INVALID: a NULL tsdf, weight, depth, viewmatrix or projmatrix; color without rgb or rgb without color; voxel, sdf_trunc or
 *   depth_trunc that is not positive and finite; an origin or alpha_min that is not finite; W or H below 1 or W * H >= 2^31; a dimension
 *   below 2 or nx * ny * nz >= 2^31; a pointer that is not 4-byte aligned.
 *
 * THE ISO-SURFACE (gsr_mesh_scratch_bytes, gsr_mesh_count, gsr_mesh_emit).
 *   Node state: valid = weight >= min_weight (a NaN weight is invalid); inside = tsdf < 0 (a node with tsdf == 0, or NaN, is outside).
 *   A cell (eight nodes, low corner c) is valid iff all eight nodes are valid; its linear index is that of its low corner among the
 *   (nx-1) x (ny-1) x (nz-1) cells, x fastest.  Each valid cell is cut into six tetrahedra, one per ordered pair (a, b) of distinct axes:
 *       p0 = c,  p1 = c + e_a,  p2 = c + e_a + e_b,  p3 = c + (1,1,1)
 *   numbered 0..5 for (a, b) = (x,y) (x,z) (y,x) (y,z) (z,x) (z,y).  Tetrahedra 0, 3 and 4 are positively oriented
 *   (det[p1-p0, p2-p0, p3-p0] > 0), 1, 2 and 5 negatively.
 *   Lattice edges: every tetrahedron edge leaves a node in one of seven directions, numbered 0..6 = 100, 010, 001, 110, 101, 011, 111
 *   (x first).  A VERTEX exists on the lattice edge (node n, direction e) iff both end nodes are valid and differ in `inside`, and at
 *   least one valid cell contains the edge (the cells whose low corner equals n on the axes where e is 1 and is n or n - 1 on the others).
 *   Hence no vertex is unreferenced and no index dangles.  With a = position of n, b = position of n + e, f = tsdf_a / (tsdf_a - tsdf_b)
 *   (0 <= f <= 1) the vertex lies at a + (b - a) * f and its colour is color_a + (color_b - color_a) * f per channel.
 *   Vertex order: ascending (node linear index, direction).  Triangle order: ascending (cell linear index, tetrahedron number, triangle
 *   within the tetrahedron).
 *   Triangles of a positively oriented tetrahedron, ij = the vertex on edge p_i p_j:
 *       one inside    p0: (01,02,03)   p1: (01,13,12)   p2: (02,12,23)   p3: (03,23,13)
 *       one outside   p0: (01,03,02)   p1: (01,12,13)   p2: (02,23,12)   p3: (03,13,23)
 *       two inside {p_a, p_b}, a < b, outside {p_c, p_d} ordered so that (a, b, c, d) is an even permutation of (0, 1, 2, 3): the quad
 *       (ac, ad, bd, bc) is split along ac-bd into (ac, ad, bd) and (ac, bd, bc), in that order
 *   and a negatively oriented tetrahedron swaps the last two corners of each triangle.  The normal (right-hand rule) then points to the
 *   positive, free-space side.  A node with tsdf == 0 counts as outside, its vertices coincide with it (f = 1 or 0), and the zero-area
 *   triangles that result are kept: the mesh stays closed.
 *
 *   gsr_mesh_scratch_bytes: the scratch gsr_mesh_count needs for a volume of that size (host arithmetic only); 0 for a size the entries
 *   refuse.
 *   gsr_mesh_count: classifies, counts and scans.  It leaves the node classes, the per-node vertex offsets and the per-cell triangle
 *   offsets in `scratch` (16-byte aligned, at least gsr_mesh_scratch_bytes) and writes counts[0] = nV and counts[1] = nT, two uint64, on
 *   the device (counts 8-byte aligned).  Those 16 bytes are all a caller reads back.  Both totals are exact in 64 bits even where
 *   gsr_mesh_emit would refuse them.
 *   gsr_mesh_emit: with the scratch gsr_mesh_count left for the same volume, writes verts[nV, 3], vcolor[nV, 3] (given iff color is) and
 *   faces[nT, 3] (int32 vertex indices), exactly those rows and nothing else (no row beyond nV / nT is written whatever the scratch
 *   holds).  The classification is the one in the scratch: min_weight is not evaluated again.  nV == 0 is a no-op that returns 0 (verts,
 *   vcolor and faces may then be NULL); faces may be NULL when nT == 0.
 *   GSR_E_INVALID: a NULL tsdf, weight, scratch, counts, or (nV > 0) verts, (nT > 0) faces; vcolor without color or color without vcolor
 *   (nV > 0); scratch_bytes below gsr_mesh_scratch_bytes; a scratch that is not 16-byte aligned, counts not 8-byte aligned, another
 *   pointer not 4-byte aligned; a min_weight that is NaN; voxel not positive and finite or an origin not finite; the size limits of the
 *   volume; nV >= 2^31 or 3 * nT >= 2^31. */
#ifndef GSR_HIP_MESH_H_
#define GSR_HIP_MESH_H_

#include "gsr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int gsr_tsdf_integrate(float* tsdf, float* weight, float* color, int nx, int ny, int nz, float ox, float oy, float oz, float voxel,
                       const float* depth, const float* rgb, const float* alpha, float alpha_min, int W, int H, const float* viewmatrix,
                       const float* projmatrix, float sdf_trunc, float depth_trunc, void* stream);
size_t gsr_mesh_scratch_bytes(int nx, int ny, int nz);
int gsr_mesh_count(const float* tsdf, const float* weight, int nx, int ny, int nz, float min_weight, void* scratch, size_t scratch_bytes,
                   uint64_t* counts, void* stream);
int gsr_mesh_emit(const float* tsdf, const float* weight, const float* color, int nx, int ny, int nz, float ox, float oy, float oz, float voxel,
                  float min_weight, const void* scratch, float* verts, float* vcolor, int* faces, uint64_t nV, uint64_t nT, void* stream);

#ifdef __cplusplus
}
#endif
#endif
