"""Timing aid (not a test; needs a GPU): the optimizer step of the C3 layout (P = 10^6 surfels, 16 SH coefficients, 2 scales, a 128^2
cubemap: 59.3 M floats) three ways:

  B  FlatAdam.step (gsr_adam_step_range): steps whatever the flat buffer holds.  The floor: 28 bytes per parameter.
  A  what training raw parameters costs without the new entry: the four torch activations forward (sigmoid, exp, normalize, sigmoid), their
     autograd backward from dL/d(activated) into the flat gradient buffer, then B.
  C  RawAdam.step (gsr_adam_act_step): chain rule, Adam and the activated copy in one launch; by bytes B x (28 * 59 + 4 * 8) / (28 * 59) = B x 1.019.

Calls alternate in one process on one device after a warm-up; a sample is `--inner` steps between two device events, the figures are per
step.  Prints one JSON line: the three medians, each one's spread (min, max) and the ratios.

    python tests/raw_step_timing.py [--repeats N] [--inner K] [--warmup W] [--points P]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-reflection_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=1_000_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("raw_step_timing.py measures on the GPU; none is available")
    from gsr_train import GaussianTrainState, RawTrainState
    P, M, L = args.points, 16, 128
    g = torch.Generator(device="cuda").manual_seed(1)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    raw = dict(means3D=rn(P, 3), shs=rn(P, M, 3), opacities=2 * rn(P, 1), scales=-3 + rn(P, 2), rotations=rn(P, 4), refl_strengths=2 * rn(P, 1),
               cubemap=rn(6, 3, L, L), fail=rn(3))
    plain = GaussianTrainState(raw, "cuda")              # (B and A: the flat buffer holds the raw values; FlatAdam steps them as they are)
    fused = RawTrainState(raw, "cuda")
    for st in (plain, fused):
        st.grads.flat.copy_(1e-3 * rn(st.params.total))
    names = RawTrainState.ACTIVATED
    dact = {k: plain.grads.view(k).clone() for k in names}
    acts = dict(opacities=torch.sigmoid, scales=torch.exp, rotations=torch.nn.functional.normalize, refl_strengths=torch.sigmoid)

    def step_b():
        plain.optimizer.step()

    def step_a():
        out = [acts[k](plain.p[k]) for k in names]
        torch.autograd.backward(out, [dact[k] for k in names])     # accumulates into the .grad views of the flat gradient buffer
        plain.optimizer.step()

    def step_c():
        fused.optimizer.step()

    fns = {"B_flat_adam": step_b, "A_torch_activations_then_adam": step_a, "C_adam_act_step": step_c}
    for _ in range(args.warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.inner)
    n, n_act = fused.params.total, fused.optimizer.act.numel()
    out = {"what": "optimizer step of %d floats (%d activated): device-event ms per step, alternating calls" % (n, n_act),
           "repeats": args.repeats, "inner": args.inner}
    for k in fns:
        out[k + "_ms_p50"] = round(float(np.median(ms[k])), 4)
        out[k + "_ms_min"] = round(float(np.min(ms[k])), 4)
        out[k + "_ms_max"] = round(float(np.max(ms[k])), 4)
    b, a, c = (float(np.median(ms[k])) for k in fns)
    out["C_over_B"] = round(c / b, 4)
    out["A_over_B"] = round(a / b, 4)
    out["C_over_B_by_bytes"] = round((28.0 * n + 4.0 * n_act) / (28.0 * n), 4)
    out["B_GBps"] = round(28.0 * n / (b * 1e-3) / 1e9, 1)
    out["C_GBps"] = round((28.0 * n + 4.0 * n_act) / (c * 1e-3) / 1e9, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
