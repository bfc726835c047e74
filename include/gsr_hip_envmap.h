/* Environment-map entries of libgsr_hip.so: the two texture transforms of the reference's training schedule,
 *     gaussians.double_env_map()   (train.py:229-230; scene/gaussian_model.py:375-393; CubemapEncoder.resize)
 *     gaussians.filter_env_map()   (scene/gaussian_model.py:380-382; CubemapEncoder.filter)
 * on the [6, C, L, L] texture where it lies: a slice of a flat parameter buffer in, a slice of another one out (gsr_envmap.py does the
 * state transition around them).  Neither is a hot path — each runs once or a few times per training run — so both are one thread per
 * output texel and nothing more.
 *
 * These entries were added under ABI 102 without a version change (as the knn, metrics, viewer, raw-parameter and env-scope entries were):
 * they are declared here and not in gsr_hip.h, gsr_version() stays 102, and a binding looks them up by name (a library built before them
 * lacks them).  The conventions of gsr_hip.h hold: float32 device pointers, a refusal (GSR_E_INVALID) comes before any device work and
 * launches nothing, gsr_last_error() names the entry.  Both entries write every element of dst and nothing else, run on the caller's
 * stream, do not synchronise with the host, allocate nothing and launch under no timing stage.
 *
 * `planes` is 6 * C: the planes are contiguous L x L images, one after the other (the [6, C, L, L] layout of the texture).
 *
 * gsr_envmap_resize: torch.nn.functional.interpolate(src, size=(L_dst, L_dst), mode='bicubic', align_corners=True) restated.
 *   Cubic convolution with A = -0.75, four taps per axis at i-1 .. i+2, tap indices clamped to [0, L_src-1]; the four rows are combined
 *   along x first, then the four results along y.  The source coordinate of output node d comes from integers, not from a rounded float
 *   scale:
 *       n = d * (L_src - 1);   i = n / (L_dst - 1);   t = (float)(n % (L_dst - 1)) / (float)(L_dst - 1);     L_dst == 1: i = 0, t = 0
 *   so the fraction carries a single rounding and is exactly 0 wherever an output node coincides with a source node.  The weights are
 *   Horner forms in t, 1 - t, t + 1 and 2 - t,
 *       w(i)   = ((A + 2) * t - (A + 3)) * t * t + 1            w(i+1) = the same in 1 - t
 *       w(i-1) = ((A * u - 5A) * u + 8A) * u - 4A,  u = t + 1     w(i+2) = the same in u = 2 - t
 *   which give (0, 1, 0, 0) exactly at t == 0.  Hence an output node that coincides with a source node IS that source texel (finite
 *   texels; a zero keeps its value, not necessarily its sign): the four corners always, every texel when L_dst == L_src, every even node
 *   when L_dst == 2 * L_src - 1, and every output when L_src == 1.  Any L_dst >= 1 is accepted, smaller than L_src too; there is no
 *   antialiasing, as in torch.
 *
 * gsr_envmap_sharpen: inverse_sigmoid(adjust_sharpness(sigmoid(x), factor).clamp(lo, hi)) in one pass (cubemap_encoder.py:107-113 of the
 *   reference; _adjust_sharpness of this project's cubemapencoder).  Per plane, with s = 1 / (1 + exp(-x)):
 *       interior texels (they exist only when L > 2):   b = (sum of the 3x3 neighbourhood of s + 4 * s_centre) / 13
 *                                                       o = clamp(factor * s + (1 - factor) * b, 0, 1)
 *       border texels, and every texel when L <= 2:     o = s
 *       then   o = clamp(o, lo, hi);   dst = log(o / (1 - o))
 *   The reference uses factor = 2, lo = 1e-3, hi = 1 - 1e-3.
 *
 * GSR_E_INVALID, both entries: a NULL pointer; a pointer that is not 4-byte aligned; planes < 1; a resolution < 1; planes * L * L >= 2^31
 * for either resolution; src and dst ranges that overlap (neither entry works in place).  gsr_envmap_sharpen also: a factor that is not
 * finite; anything but 0 < lo < hi < 1. */
#ifndef GSR_HIP_ENVMAP_H_
#define GSR_HIP_ENVMAP_H_

#include "gsr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int gsr_envmap_resize(const float* src /* [planes, L_src, L_src] */, float* dst /* [planes, L_dst, L_dst] */, int planes, int L_src, int L_dst,
                      void* stream);
int gsr_envmap_sharpen(const float* src /* [planes, L, L] */, float* dst /* [planes, L, L] */, int planes, int L, float factor, float lo,
                       float hi, void* stream);

#ifdef __cplusplus
}
#endif
#endif
