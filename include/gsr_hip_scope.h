/* Env-scope entries of libgsr_hip.so: the sphere test of the reference's bounded scenes (opt.use_env_scope; train.py:56-63) and its
 * reflection-mask loss (train.py:176-179),
 *     outside = torch.sum((xyz - center[None])**2, dim=-1) > radius**2;    loss += 0.4 * refl[outside].mean()
 * as one pass over the points each way, with no host read anywhere (the boolean index of the torch form runs a nonzero and waits for it).
 *
 * These entries were added under ABI 102 without a version change (as the knn, metrics, viewer and raw-parameter entries were): they are
 * declared here and not in gsr_hip.h, gsr_version() stays 102, and a binding looks them up by name (a library built before them lacks
 * them).  The conventions of gsr_hip.h hold: float32 device pointers, a refusal (GSR_E_INVALID) comes before any device work and launches
 * nothing, gsr_last_error() names the entry.  Sizes and values are checked on every call; the pointer checks of the forward apply for
 * P > 0 only (an empty scene's tensors have NULL data pointers, and nothing is read or written through them: see P == 0 below).
 * Everything runs on the caller's stream: no side stream, no allocation, no host read.  Launches are timed under GSR_STAGE_LOSS_FWD /
 * GSR_STAGE_LOSS_BWD.
 *
 * Forward, per point, in float32 without fused multiply-add (the roundings of the torch expression):
 *     dx = x - cx, dy = y - cy, dz = z - cz;   d2 = (dx*dx + dy*dy) + dz*dz;   inside = d2 < radius2;   outside = d2 > radius2
 * Neither mask is the negation of the other: a point with d2 == radius2 and a point with a NaN coordinate are in NEITHER, as in the torch
 * expressions (render()'s `< radius**2` and the loss's `> radius**2`); a coordinate of +-inf is outside.  The caller passes the centre
 * already rounded to float32 (what torch.tensor(center) holds) and radius2 = (float)((double)radius * radius), the value torch compares
 * against.  Masks are bytes 0 / 1 (torch.bool storage).
 * With refl: sums[0] = sum of refl over the outside points, sums[1] = their number.  Every block leaves one partial pair in scratch
 * (gsr_env_scope_scratch_floats() floats); a second one-block launch adds the pairs in double in a fixed order: no float atomics, the
 * sums are bitwise reproducible run to run.  The count is accumulated in float32 and is exact up to 2^24 points.
 *
 * Backward: grad_refl[i] (+)= outside[i] ? g_loss[0] / sums[1] : 0, one IEEE division of two device floats.  accumulate = 0 writes
 * every element (zeros where the point is not outside); accumulate = 1 touches outside elements only.  sums[1] == 0 (no point outside:
 * torch's mean is NaN there but sends no gradient to any row): zeros with accumulate = 0, nothing written with accumulate = 1, never a
 * NaN or inf. */
#ifndef GSR_HIP_SCOPE_H_
#define GSR_HIP_SCOPE_H_

#include "gsr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* floats of the forward's `scratch` (a constant: one pair per block of a capped grid) */
size_t gsr_env_scope_scratch_floats(void);
/* refl NULL: masks only (sums and scratch are not used).  refl given: [P] ACTIVATED reflection strengths; outside, sums [2] and scratch are
 * required, inside stays optional.
 * P == 0 is valid: no pointer but sums is looked at, nothing is read, no mask is written, and sums = (0, 0) when sums is given (the
 * one-block second stage over no pair at all: scratch is not read and may be NULL).
 * GSR_E_INVALID: P < 0; a centre coordinate that is not finite; radius2 not finite or negative; and for P > 0: NULL means3D; refl with a
 * NULL outside, sums or scratch; no refl and both masks NULL (nothing to do). */
int gsr_env_scope_forward(int P, const float* means3D /* [P,3] */, const float* refl /* [P] or NULL */, float cx, float cy, float cz,
                          float radius2, uint8_t* inside /* [P] or NULL */, uint8_t* outside /* [P]; NULL only without refl */,
                          float* sums /* [2] */, float* scratch, void* stream);
/* outside and sums as the forward left them; g_loss: the upstream gradient of the MEAN sums[0] / sums[1], one float on the device.
 * GSR_E_INVALID: P < 0, any NULL pointer, accumulate other than 0 or 1.  P == 0 is a no-op. */
int gsr_env_scope_backward(int P, const uint8_t* outside /* [P] */, const float* sums /* [2] */, const float* g_loss /* [1] */,
                           float* grad_refl /* [P] */, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif
