/* Mesh clean-up entries of libgsr_hip.so: the connected triangle clusters of an indexed mesh, the largest of them kept, the small ones and
 * the vertices nobody references any more dropped, on the device.  This is what upstream 2DGS runs on the mesh of extract_mesh_bounded
 * before it writes it (post_process_mesh: open3d's cluster_connected_triangles, remove_triangles_by_mask, remove_unreferenced_vertices).
 * gsr_mesh.py drives the entries (cluster_connected_triangles, clean_mesh) and utils/mesh_utils.py puts post_process_mesh on top.  The
 * reference has no code for this, so the contract below is this project's own; tests/meshclean_ref.py restates it in integers.
 *
 * These entries were added under ABI 102 without a version change (as the mesh entries of gsr_hip_mesh.h were): they are declared here
 * and not in gsr_hip.h, gsr_version() stays 102, and a binding looks them up by name (a library built before them lacks them).  The
 * conventions of gsr_hip.h hold: device pointers, the caller's stream, no host synchronisation, no allocation, a refusal (GSR_E_INVALID)
 * comes before any device work and launches nothing, gsr_last_error() names the entry.
 *
 * DETERMINISM.  These entries do use atomics (gsr_hip_mesh.h's sentence is about its own entries): an integer minimum on the union-find's
 * parent array and integer adds on counters.  A component's label is the smallest vertex index in it and every count is an integer sum,
 * so no result depends on the order in which the atomics arrive: the same inputs give the same bytes, run to run.  No kernel waits for
 * another workgroup, and every loop ends whatever another workgroup does ("Mesh clean-up", has the arguments).
 *
 * INPUT.  verts [nV, 3] float32, optional vcolor [nV, 3] float32, faces [nT, 3] int32; nV < 2^31 and 3 * nT < 2^31;
 *   cluster_to_keep >= 1 and min_triangles >= 0, both uint64.
 *
 * COUNTED FACES.  A face is counted iff its three indices lie in [0, nV) and are pairwise distinct.  Any other face is IGNORED: it
 *   connects nothing, counts for nothing and is not emitted, and its indices are never used as addresses (a mesh with a bad index causes
 *   no out-of-bounds access).
 *
 * COMPONENTS.  Two vertices are connected when a counted face holds both; a component is a class of the transitive closure.  Its label
 *   is the smallest vertex index in it, its size the number of counted faces in it.  A vertex in no counted face is its own component
 *   of size 0.  This is VERTEX connectivity; open3d's cluster_connected_triangles joins triangles over shared EDGES.  On the indexed
 *   marching-tetrahedra meshes gsr_mesh_emit writes, the two differ only where surfaces touch in a single vertex.
 *
 * THRESHOLD.  Let s_1 >= s_2 >= ... >= s_C be the sizes of the C components of size >= 1.
 *       thr = max(s_min(cluster_to_keep, C), min_triangles),   and with C == 0:  thr = min_triangles
 *   A counted face is KEPT iff its component's size is >= thr.  Ties at thr are all kept, as upstream keeps them.  Upstream raises when
 *   cluster_to_keep > C; here cluster_to_keep is clamped to C.
 *
 * OUTPUT.  The kept faces, in input order; the vertices referenced by at least one kept face, in input order, their rows gathered bit
 *   for bit (colours likewise); the faces re-indexed to the new vertex rows.  Zero-area triangles with distinct indices are counted and
 *   kept like any other: the extraction's closed-surface rule (gsr_hip_mesh.h).
 *
 * gsr_mesh_clean_scratch_bytes: the scratch gsr_mesh_clean_count needs for nV vertices and nT faces (host arithmetic only); 0 for sizes
 *   the entries refuse.  (For nV == 0 or nT == 0 it is positive and the scratch is not touched.)
 * gsr_mesh_clean_count: labels, sizes, selects thr, flags and scans; leaves the labels, the flags and the new row of every vertex and
 *   face in `scratch` (16-byte aligned, at least gsr_mesh_clean_scratch_bytes; it may hold anything beforehand) and writes six uint64
 *   to `counts` on the device (8-byte aligned), all a caller reads back:
 *       counts[0] = nV_out   counts[1] = nT_out   counts[2] = C   counts[3] = the components kept (size >= 1 and >= thr)
 *       counts[4] = thr      counts[5] = the ignored faces
 *   tri_label [nT] and tri_size [nT], int32, are each optional (NULL): per face its component's label and size; an ignored face gets -1
 *   and 0.  nV == 0 or nT == 0 is accepted: no threshold is formed and all counts are zero except counts[5] = nT (with no vertex every
 *   face is ignored); faces and scratch are then not read and may be NULL, tri_label and tri_size are still filled.
 *   GSR_E_INVALID: a NULL counts, or (nV > 0 and nT > 0) a NULL faces or scratch; faces, tri_label or tri_size not 4-byte aligned, a
 *   scratch not 16-byte aligned, counts not 8-byte aligned; scratch_bytes below gsr_mesh_clean_scratch_bytes(nV, nT);
 *   cluster_to_keep == 0; nV >= 2^31 or 3 * nT >= 2^31.
 * gsr_mesh_clean_emit: with the scratch gsr_mesh_clean_count left for the same faces, and nV_out = counts[0], nT_out = counts[1],
 *   writes verts_out [nV_out, 3], vcolor_out [nV_out, 3] (given iff vcolor is) and faces_out [nT_out, 3]: exactly those rows and
 *   nothing beyond them, whatever the scratch holds.  nT_out == 0 is a no-op that returns 0 (every pointer may then be NULL).
 *   GSR_E_INVALID: a pointer not 4-byte aligned, a scratch not 16-byte aligned; nV >= 2^31 or 3 * nT >= 2^31; nV_out > nV or
 *   nT_out > nT; and with nT_out > 0: a NULL verts, faces, scratch, verts_out or faces_out; vcolor without vcolor_out or vcolor_out
 *   without vcolor. */
#ifndef GSR_HIP_MESHCLEAN_H_
#define GSR_HIP_MESHCLEAN_H_

#include "gsr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int gsr_mesh_clean_count(const int* faces, uint64_t nV, uint64_t nT, uint64_t cluster_to_keep, uint64_t min_triangles, int* tri_label,
                         int* tri_size, void* scratch, size_t scratch_bytes, uint64_t* counts, void* stream);
size_t gsr_mesh_clean_scratch_bytes(uint64_t nV, uint64_t nT);
int gsr_mesh_clean_emit(const float* verts, const float* vcolor, const int* faces, uint64_t nV, uint64_t nT, const void* scratch,
                        float* verts_out, float* vcolor_out, int* faces_out, uint64_t nV_out, uint64_t nT_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
