/* The per-view densification statistics under a boolean filter:
 *     GaussianModel.add_densification_stats(viewspace_point_tensor, update_filter, render_weight)   (scene/gaussian_model.py:579-584)
 * as the reference's loop calls it every iteration (train.py:244).  gsr_densification_stats of gsr_hip.h takes the int32 radii and also
 * keeps the running maximum max_radii2D (train.py:243 fused in); this entry takes the filter the caller already holds and leaves
 * max_radii2D to the caller's own line.
 *
 * Added under ABI 102 without a version change, as the entries of gsr_hip_densify.h were: gsr_version() stays 102 and a binding looks the
 * entry up by name (a library built before it lacks it).  gsr_hip_densify.h includes this header, so a host that includes that one has
 * the whole densification interface.  The conventions of gsr_hip.h hold: device pointers, a refusal (GSR_E_INVALID) comes before any
 * device work and launches nothing, gsr_last_error() names the entry; the kernel runs on the caller's stream, nothing synchronises with
 * the host and nothing is allocated. */
#ifndef GSR_HIP_DENSIFY_STATS_H_
#define GSR_HIP_DENSIFY_STATS_H_

#include "gsr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For every row i < P, in float32:
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
