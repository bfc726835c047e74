/* Raw-parameter training step of libgsr_hip.so: the entries that train the reference's RAW parameters (scene/gaussian_model.py:42-52,
 * 123-147: sigmoid(_opacity), exp(_scaling), normalize(_rotation), sigmoid(_refl_strength)) with the activation's chain rule in front
 * of the fused Adam update of gsr_adam_step_range and the activation behind it.
 *
 * These entries were added under ABI 102 without a version change (as the knn, metrics and viewer entries were): they are declared
 * here and not in gsr_hip.h, gsr_version() stays 102, and a binding looks them up by name (a library built before them lacks them).
 * The conventions of gsr_hip.h hold: float32 device pointers, 16-byte alignment where stated, every argument checked before any device
 * work (GSR_E_INVALID, nothing launched), gsr_last_error() names the entry.  Launches are timed under GSR_STAGE_ADAM.
 *
 * Layout.  `raw`, `grad`, `exp_avg` and `exp_avg_sq` are float[n] laid out identically, as for gsr_adam_step.  `act` is a second,
 * COMPACT buffer float[n_act] that holds the activated copy of the activated segments only (8 floats per surfel: opacity, two or three
 * scales, four quaternion components, reflection strength; every slice padded to a multiple of 4 floats as the flat buffers are), so
 * that the rasterizer reads activated values that nobody had to compute with separate launches.  The rasterizer's backward leaves
 * dL/d(activated) in the gradient slots of those segments; the step turns it into dL/d(raw) in registers.
 *
 * Per element i of a segment of kind K, with r = raw[i], g = grad[i]:
 *   GSR_ACT_NONE        nothing is written to act; g enters Adam as it is.  Bit for bit the update of gsr_adam_step_range (one kernel
 *                       serves both entries).
 *   GSR_ACT_SIGMOID     a = 1 / (1 + exp(-r));  g * a * (1 - a) enters Adam
 *   GSR_ACT_EXP         a = exp(r);             g * a enters Adam
 *   GSR_ACT_NORMALIZE4  rows of four: a = q / max(|q|, 1e-12);  |q| > 1e-12: (g - a (a . g)) / |q| enters Adam, otherwise g / 1e-12
 *                       (what torch.nn.functional.normalize differentiates to, the zero row included)
 *   K | GSR_ACT_FROZEN  the element is skipped: raw, both moments and act stay bit for bit (freeze_xyz, scene/gaussian_model.py:213-215)
 * The gradient is formed from raw as it is BEFORE the step (the activation is recomputed in registers; act is never read), then the
 * Adam update of gsr_adam_step runs on (raw, that gradient, exp_avg, exp_avg_sq), then act(raw after the step) is stored at
 * act[act_begin + (i - begin)].  Traffic: 28 bytes per parameter as gsr_adam_step, plus 4 bytes per activated parameter. */
#ifndef GSR_HIP_TRAIN_H_
#define GSR_HIP_TRAIN_H_

#include "gsr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_ACT_NONE 0
#define GSR_ACT_SIGMOID 1
#define GSR_ACT_EXP 2
#define GSR_ACT_NORMALIZE4 3
#define GSR_ACT_FROZEN 0x100   /* flag, or-ed to a kind */

typedef struct {
	uint64_t begin, end;     /* as gsr_adam_segment */
	float lr, lr2;
	uint32_t period, split;
	uint32_t kind;           /* GSR_ACT_NONE, _SIGMOID, _EXP or _NORMALIZE4, optionally | GSR_ACT_FROZEN */
	uint64_t act_begin;      /* first element of this segment in `act`; ignored for GSR_ACT_NONE */
} gsr_act_segment;

/* One step over elements [range_begin, range_end) (gsr_adam_step_range's range; the whole buffer is [0, n)).
 * GSR_E_INVALID: everything gsr_adam_step_range refuses (a NULL or misaligned buffer, step < 1, more than 16 segments, segments that do not
 * tile [0, n) in order, split > period, a range outside [0, n) or with a bound that is not a multiple of 4 other than range_end == n);
 * an unknown kind or flag bit; and for an activated segment (kind other than NONE): a NULL or misaligned act, a begin or act_begin that
 * is not a multiple of 4, a NORMALIZE4 segment whose length is not a multiple of 4, act_begin + (end - begin) > n_act.
 * n == 0 and an empty range are no-ops. */
int gsr_adam_act_step(float* raw, const float* grad, float* exp_avg, float* exp_avg_sq, float* act, uint64_t n, uint64_t n_act,
                      const gsr_act_segment* segments, int num_segments, float beta1, float beta2, float eps, int step,
                      uint64_t range_begin, uint64_t range_end, void* stream);
/* The forward alone: act = act(raw) for every activated segment (GSR_ACT_FROZEN is ignored here: a frozen group's copy is filled too);
 * no gradient, no moments, raw is not written.  For construction, after densification and after a reset.  lr, lr2, period and split are
 * not used but are checked as above (the same table serves both entries).  Refusals as above, without the moment, step and range ones. */
int gsr_activate(const float* raw, float* act, uint64_t n, uint64_t n_act, const gsr_act_segment* segments, int num_segments,
                 void* stream);

#ifdef __cplusplus
}
#endif
#endif
