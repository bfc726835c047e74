/* Densification-plan entries of libgsr_hip.so: the DECISIONS of the reference's adaptive density control
 *     GaussianModel.densify_and_prune   (scene/gaussian_model.py:548-576: prune by weight -> clone -> split -> prune big points)
 *     GaussianModel.prune_points        (scene/gaussian_model.py:429-446)
 * taken on the device.  gsr_hip.h has the data movement (gsr_gather_rows), the statistics (gsr_densification_stats) and the split children
 * (gsr_split_children); the entries here produce the row maps gsr_gather_rows consumes, so that a host which uses only the C ABI can
 * densify, and so that the Python layer reads 16 bytes where its torch plan runs some forty ops with ten boolean indexes.
 *
 * These entries were added under ABI 102 without a version change (as the knn, metrics, viewer, raw-parameter, env-scope and
 * environment-map entries were): they are declared here and not in gsr_hip.h, gsr_version() stays 102, and a binding looks them up by name
 * (a library built before them lacks them).  The conventions of gsr_hip.h hold: device pointers unless said otherwise, a refusal
 * (GSR_E_INVALID) comes before any device work and launches nothing, gsr_last_error() names the entry.  Everything runs on the caller's
 * stream; nothing synchronises with the host, nothing is allocated (the caller supplies `scratch`), no kernel waits for another
 * workgroup and no position comes from an atomic: the order of every output is the index order, the same run to run.
 *
 * THE PLAN.  For old row i, in float32 with IEEE division:
 *     w = denom_w[i] == 0 ? 0 : accum_w[i] / denom_w[i];                      pruned by weight  iff  w < min_weight       (0.01f)
 *     g = xyz_gradient_accum[i] / denom[i], NaN -> 0 (inf stays);             m = max_k expf(scaling[i, k])   (NaN if any term is)
 *     a survivor is cloned        iff  |g| >= max_grad  &&  m <= dense_limit
 *     a survivor is a split parent iff   g  >= max_grad  &&  m >  dense_limit          dense_limit = (float)(percent_dense * extent)
 * The sequence before the last prune is the reference's: surviving originals that are not parents, in index order; clones, in index order
 * of their originals; copy 1 of every parent's child with the parents in index order; copy 2 likewise; ... up to copy N.  With
 * size_prune != 0 an element of the sequence is dropped iff
 *     (m > big_near && d2 < extent2)  ||  (m > big_far && !(d2 < extent2)),     d2 = sum_k (xyz[k] - mean[k])^2
 * (big_near = (float)(0.1 * extent), big_far = (float)(1.5 * extent), extent2 = (float)(extent * extent)); originals and clones are
 * judged on xyz / scaling of their old row, children on child_xyz / child_scaling as gsr_split_children produced them.  max_radii2D
 * takes no part: the reference resets it before it looks at it.  With size_prune == 0 nothing is dropped.
 * max_grad > 0 is required: a clone enters the reference's split test with gradient 0 and must fail it.
 *
 * Call order:  gsr_densify_plan_select  ->  (the host reads counts[2] = k, forms child j's parent = parents[j % k] for j < N k and calls
 * gsr_split_children)  ->  gsr_densify_plan_rows  ->  gsr_gather_rows with map_param on the parameters and with map_moment on both Adam
 * moments  ->  gsr_scatter_rows with child_of to place child_xyz and child_scaling.  `scratch` carries the state from select to rows: the
 * same buffer, untouched in between; rows leaves select's part of it as it was (it may be called again).
 *
 * Kernel shape (csrc/gsr_densify.hip): classify + rank inside workgroups of 256 rows (wave64 ballots and popcounts, an LDS prefix over the
 * four waves), a separate one-workgroup launch that scans the per-workgroup counts in chunks of 256, an emit launch. */
#ifndef GSR_HIP_DENSIFY_H_
#define GSR_HIP_DENSIFY_H_

#include "gsr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* host memory; every threshold already rounded to float32 by the caller */
typedef struct {
	float max_grad;
	float min_weight;
	float dense_limit;
	float big_near;
	float big_far;
	float extent2;
	float mean[3];
	int size_prune;
	int N;
	int scale_dims;
} gsr_densify_plan;

/* Bytes of `scratch` for P old rows and N children per parent (sized for the worst case of P parents): what all three entries below ask
 * for (gsr_prune_rows: with N = 1).  0 for arguments the entries refuse (P < 0, N < 1, P * (N + 1) >= 2^31). */
size_t gsr_densify_plan_scratch_bytes(int P, int N);

/* Classes of the P old rows.  Out: counts int32[4] = {survivors of the weight prune, clones, parents k, 0}; parents int32[P], of which
 * the first k are written: the old rows of the split parents in index order.
 * P == 0: counts = zeros, nothing else is touched, returns 0.
 * GSR_E_INVALID: P < 0; NULL plan; plan->N < 1; plan->scale_dims not 2 or 3; P * (N + 1) >= 2^31; max_grad <= 0 (or NaN); NULL counts;
 * and for P > 0: any other NULL buffer, scratch not 16-byte aligned, scratch_bytes < gsr_densify_plan_scratch_bytes(P, plan->N). */
int gsr_densify_plan_select(int P, const gsr_densify_plan* plan, const float* xyz_gradient_accum, const float* denom, const float* accum_w,
                            const float* denom_w, const float* scaling /* [P, scale_dims] log-scales */, void* scratch, size_t scratch_bytes,
                            int* counts /* [4] */, int* parents /* [P] */, void* stream);

/* The row maps.  In: scratch as select left it (same P and plan), xyz [P,3], scaling [P, scale_dims], parents as select wrote them, the
 * children of gsr_split_children (child_xyz [N k, 3], child_scaling [N k, scale_dims]) and k = select's counts[2] as the host read it.
 * Out, per KEPT element in sequence order (the caller sizes the three maps for the whole sequence, survivors - k + clones + N k entries;
 * entries behind the kept ones are not written):
 *     map_param[r]   old row whose parameters new row r takes (a child: its parent's)
 *     map_moment[r]  the same for an original, -1 (zeros in gsr_gather_rows) for a clone or a child
 *     child_of[r]    j for child j of child_xyz / child_scaling, -1 otherwise
 * counts int32[4] = {rows kept, rows dropped as big, children kept, 0}.
 * P == 0: counts = zeros, returns 0.  k == 0: parents, child_xyz and child_scaling are not read and may be NULL.
 * GSR_E_INVALID: what select refuses; k < 0 or k > P; k > 0 with NULL parents, child_xyz or child_scaling; and for P > 0 a NULL xyz,
 * scaling, map or counts. */
int gsr_densify_plan_rows(int P, const gsr_densify_plan* plan, void* scratch, size_t scratch_bytes, const float* xyz, const float* scaling,
                          const int* parents, const float* child_xyz, const float* child_scaling, int k, int* map_param, int* map_moment,
                          int* child_of, int* counts /* [4] */, void* stream);

/* prune_points: remove[i] != 0 (bytes, torch.bool storage) marks the rows that go.  Out: row_map int32[P], of which the first
 * counts[0] are written: the old rows that stay, in index order; counts int32[4] = {rows kept, rows removed, 0, 0}.
 * P == 0: counts = zeros, returns 0.
 * GSR_E_INVALID: P < 0; P >= 2^30; NULL counts; and for P > 0: NULL remove, scratch or row_map, scratch not 16-byte aligned,
 * scratch_bytes < gsr_densify_plan_scratch_bytes(P, 1). */
int gsr_prune_rows(int P, const uint8_t* remove /* [P] */, void* scratch, size_t scratch_bytes, int* row_map /* [P] */, int* counts /* [4] */,
                   void* stream);

/* The mirror of gsr_gather_rows for rows that come from a second source: for every group g and row r with slot[r] >= 0,
 *     dst[g.dst_offset + r*g.width + c] = src[g.src_offset + slot[r]*g.width + c];
 * rows with slot[r] < 0 are left as they are.  slot int32[n_rows] (device); groups: host array, at most 16; offsets in floats.
 * n_rows == 0 or num_groups == 0: a no-op.  GSR_E_INVALID: num_groups < 0 or > 16, a NULL argument, a zero-width group. */
int gsr_scatter_rows(const float* src, float* dst, const int* slot, uint64_t n_rows, const gsr_gather_group* groups, int num_groups,
                     void* stream);

/* The per-view densification statistics under a boolean filter:
 *     GaussianModel.add_densification_stats(viewspace_point_tensor, update_filter, render_weight)   (scene/gaussian_model.py:579-584)
 * as the reference's loop calls it every iteration (train.py:244).  gsr_densification_stats of gsr_hip.h takes the int32 radii and also
 * keeps the running maximum max_radii2D (train.py:243 fused in); this entry takes the filter the caller already holds and leaves
 * max_radii2D to the caller's own line.  Added under ABI 102 after the five entries above, likewise by name.  The kernel runs on the
 * caller's stream, nothing synchronises with the host and nothing is allocated.
 *
 * For every row i < P, in float32:
 *     update_filter[i] != 0 :  xyz_gradient_accum[i] += sqrtf(gx^2 + gy^2 + gz^2) of grad_means2D[i, 0..2];  denom[i] += 1
 *     gaussian_weights[i] > 0:  accum_w[i] += gaussian_weights[i];                                            denom_w[i] += 1
 * the arithmetic gsr_densification_stats applies to the rows with radii > 0, bit for bit (one device function serves both kernels).
 * Rows with the filter off and a weight that is not positive keep their bits.  update_filter is bytes, torch.bool storage.
 * P == 0: a no-op, returns 0.  GSR_E_INVALID: P < 0; for P > 0 any NULL buffer. */
int gsr_densification_stats_filter(int P, const float* grad_means2D /* [P,3] */, const uint8_t* update_filter /* [P] */,
                                   const float* gaussian_weights /* [P] */, float* xyz_gradient_accum, float* denom, float* accum_w,
                                   float* denom_w, void* stream);

#ifdef __cplusplus
}
#endif
#endif
