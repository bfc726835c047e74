/* Unbounded mesh extraction of libgsr_hip.so: TSDF fusion of rendered surface-depth maps into a lattice in CONTRACTED space, per-vertex
 * colouring of world points, and the map from contracted coordinates back to the world.  The iso-surface itself is gsr_hip_mesh.h's
 * (gsr_mesh_count, gsr_mesh_emit on the lattice), the clean-up gsr_hip_meshclean.h's.  gsr_mesh.py drives the entries
 * (ContractedTSDFVolume, color_vertices), utils/mesh_utils.py puts GaussianExtractor.extract_mesh_unbounded on top and utils/mcube_utils.py
 * the reference's marching_cubes_with_contraction.  Upstream 2DGS has this path in Python; the reference ships only its second half, so
 * the contract below is this project's own, and the places where it deliberately differs from upstream are marked (+).
 * tests/unbounded_ref.py restates it in float64.
 *
 * These entries were added under ABI 102 without a version change: they are declared here and not in gsr_hip.h, gsr_version() stays 102,
 * and a binding looks them up by name.  The conventions of gsr_hip_mesh.h hold: float32 device pointers, the caller's stream, no host
 * synchronisation, no allocation, a refusal (GSR_E_INVALID) comes before any device work and launches nothing, gsr_last_error() names
 * the entry; no kernel uses an atomic or waits for another workgroup, so the same inputs give the same bytes; an element that is
 * skipped is NOT written: no plane, no byte.  Every entry is one kernel with one thread per element and plain loads and stores.
 *
 * THE CONTRACTION.  A world point X has the normalised coordinate x = (X - c) / radius.  The unit ball is kept and everything beyond
 *   it is folded into the shell 1 <= |y| < 2:  y = x for |x| <= 1, y = x (2 - 1 / |x|) / |x| otherwise.  The inverse, with m = |y|:
 *       m <= 1:      x = y
 *       1 < m < 2:   x = y / (m (2 - m))
 *   and X = c + radius * x.  Both halves agree at m = 1.
 *
 * gsr_tsdf_integrate_contracted: one view into a cubic lattice of n x n x n nodes, x fastest: node (i, j, k) has the linear index
 *   (k * n + j) * n + i, as in gsr_hip_mesh.h, and sits at the contracted coordinate
 *       y = (fmaf(step, i, lo), fmaf(step, j, lo), fmaf(step, k, lo))
 *   Planes, float32 and caller-owned: tsdf [n, n, n] and weight [n, n, n]; there are no colour planes (gsr_points_fuse_view colours the
 *   vertices afterwards).  A fresh volume is tsdf = 1 and weight = 1 (upstream's initial state): a node no view has seen is free space,
 *   and every cell is valid for gsr_mesh_count(min_weight = 1).  `voxel` is the world size the truncation is counted in.  viewmatrix and
 *   projmatrix are device pointers to 16 floats each in the layout every rasterizer entry takes.  Per node, in this order:
 *     1. m = |y|.  The node is skipped unless m < 2 (+ upstream maps such nodes through a negative scale).  x as above, and
 *            trunc = 5 voxel                          for m <= 1
 *            trunc = 5 voxel / (2 - min(m, 1.9))      for 1 < m < 2
 *        (continuous at m = 1, growing with the distance, at most 50 voxel).  X = c + radius * x.
 *     2. z = V[2] X.x + V[6] X.y + V[10] X.z + V[14] and the homogeneous p = projmatrix applied to X, exactly as in step 1 of
 *        gsr_tsdf_integrate.  Skipped unless z > 0 and p.w > 0.  With q = p.xy / p.w: skipped unless -1 < q.x < 1 and -1 < q.y < 1.
 *     3. px = ((q.x + 1) W - 1) / 2, py = ((q.y + 1) H - 1) / 2: continuous pixel coordinates in the RASTERIZER's convention, in which
 *        pixel (u, v) is centred on (u, v), the same as gsr_tsdf_integrate (+ upstream's grid_sample(align_corners=True) is shifted
 *        against it).  px is clamped to [0, W - 1] and py to [0, H - 1] (border).  x0 = floor(px), x1 = min(x0 + 1, W - 1), a = px - x0;
 *        y0, y1 and b likewise.  The four taps d00 = depth[y0, x0], d01 = depth[y0, x1], d10 = depth[y1, x0], d11 = depth[y1, x1]:
 *        skipped unless all four are > 0; a NaN tap skips (+ upstream blends the background's zeros into silhouettes).
 *            d = (d00 (1 - a) + d01 a) (1 - b) + (d10 (1 - a) + d11 a) b
 *     4. sdf = d - z; skipped unless sdf > -trunc; t = min(1, max(-1, sdf / trunc)).
 *     5. with w = weight[node]:  tsdf = (tsdf * w + t) / (w + 1);  weight = w + 1.
 *   Every skip is decided before tsdf or weight is touched.  (Contraction of a multiply and an add into an fma is left to the compiler;
 *   the decisions of steps 1-4 are what tests pin exactly, away from their thresholds.)
 *   GSR_E_INVALID: a NULL tsdf, weight, depth, viewmatrix or projmatrix; n below 2 or n^3 >= 2^31; a step, radius or voxel that is not
 *   positive and finite; a lo or a centre that is not finite; W or H below 1 or W * H >= 2^31; a pointer that is not 4-byte aligned.
 *
 * gsr_points_fuse_view: one view into per-point colours.  points [n_points, 3] are WORLD positions; color [n_points, 3] and weight
 *   [n_points] are the running state; rgb is [3, H, W].  Per point: steps 2-4 above with X = the point and trunc = sdf_trunc; s[c] =
 *   the same four taps of rgb[c] with the same weights; then
 *       color[c] = (color[c] * w + s[c]) / (w + 1)  with w = weight[point],  weight = w + 1
 *   (+) Fresh state is color = 0 and weight = 0, so a vertex ends with the mean over the views that saw it (upstream starts the weight
 *   at 1 and so darkens the vertices few views saw).  A skipped point is not written.  n_points == 0 is a no-op that returns 0 (points,
 *   color and weight may then be NULL); every other refusal comes in front of it.
 *   GSR_E_INVALID: a NULL depth, rgb, viewmatrix or projmatrix, or (n_points > 0) points, color or weight; n_points >= 2^31; an
 *   sdf_trunc that is not positive and finite; W or H below 1 or W * H >= 2^31; a pointer that is not 4-byte aligned.
 *
 * gsr_uncontract_points: dst[p] = clamp(c + radius * x(src[p]), -max_range, max_range) per coordinate, src and dst [n_points, 3], x
 *   as in THE CONTRACTION.  A point with m >= 2 takes m = the largest float32 below 2 in the divisor: that cannot occur on the vertices
 *   of a lattice whose surface lies among live nodes, and it gives a finite result (clamped), never a NaN.  dst may equal src; they may
 *   not overlap otherwise.  Exactly the n_points rows are written.  n_points == 0 is a no-op that returns 0 (src and dst may then be
 *   NULL); every other refusal comes in front of it.
 *   GSR_E_INVALID: (n_points > 0) a NULL src or dst; n_points >= 2^31; a radius or max_range that is not positive and finite; a centre
 *   that is not finite; a pointer that is not 4-byte aligned. */
#ifndef GSR_HIP_UNBOUNDED_H_
#define GSR_HIP_UNBOUNDED_H_

#include "gsr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int gsr_tsdf_integrate_contracted(float* tsdf, float* weight, int n, float lo, float step, float cx, float cy, float cz, float radius,
                                  float voxel, const float* depth, int W, int H, const float* viewmatrix, const float* projmatrix,
                                  void* stream);
int gsr_points_fuse_view(const float* points, uint64_t n_points, float* color, float* weight, const float* depth, const float* rgb, int W,
                         int H, const float* viewmatrix, const float* projmatrix, float sdf_trunc, void* stream);
int gsr_uncontract_points(const float* src, float* dst, uint64_t n_points, float cx, float cy, float cz, float radius, float max_range,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
