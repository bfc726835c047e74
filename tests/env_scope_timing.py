"""Timing aid (not a test; needs a GPU): the env-scope term of one iteration at the C3 size (P = 10^6 points), forward and backward to the
activated reflection strengths, two ways:

  A  the reference's torch chain (its train.py, env-scope branch): outside = sum((xyz - centre)^2, -1) > radius^2;
     (0.4 * refl[outside].mean()).backward() — six elementwise / reduction kernels, a boolean index (nonzero: the host WAITS for the
     device), the mean, and autograd's backward through the index.
  B  utils.loss_utils.refl_scope_loss + backward into a gradient sink (gsr_env_scope_forward / _backward): two launches forward, one
     backward, no host read.

Calls alternate in one process on one device after a warm-up.  Two figures each:
  device  `--inner` calls between two device events, per call.
  host    the host clock over the call FOLLOWED BY a chain of `--chain` enqueued kernels (the rest of an iteration; each streams a
          `--filler-mb` buffer, so it runs longer than it takes to enqueue), with the same chain already enqueued in front of it (the
          device is behind the host, as it is in training): a call that only enqueues lets the host run ahead and the figure is the
          enqueue cost alone; a call that reads from the device (A's nonzero) holds the host until the leading chain and its own
          kernels have finished, and the trailing chain is enqueued that much later.
Prints one JSON line: medians and spread (min, max) of both figures for A and B, and the time of B's kernels alone by the library's
stage events (two launches forward, one backward).

    python tests/env_scope_timing.py [--repeats N] [--inner K] [--warmup W] [--points P] [--chain C] [--filler-mb M]
"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--chain", type=int, default=40)
    ap.add_argument("--filler-mb", type=int, default=256, help="size of the buffer each chain kernel reads and writes")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("env_scope_timing.py measures on the GPU; none is available")
    from utils.loss_utils import refl_scope_loss
    P = args.points
    g = torch.Generator(device="cuda").manual_seed(1)
    centre, radius = [0.3, -1.2, 2.5], 1.7
    xyz = torch.tensor(centre, device="cuda")[None] + torch.randn(P, 3, device="cuda", generator=g) * 1.1      # about half outside
    refl = torch.rand(P, 1, device="cuda", generator=g).requires_grad_(True)
    sink = torch.zeros(P, 1, device="cuda")
    centre_dev = torch.tensor(centre, device="cuda")
    filler = torch.zeros(args.filler_mb << 18, device="cuda")      # (each chain kernel must run longer than it takes to enqueue: the device falls behind)

    def step_a():
        outside = torch.sum((xyz - centre_dev[None]) ** 2, dim=-1) > radius ** 2
        refl.grad = None
        (0.4 * refl[outside].mean()).backward()

    def step_b():
        loss = refl_scope_loss(refl, xyz, centre, radius, grad_sink=sink, accumulate=False)[0]
        (0.4 * loss).backward()

    fns = {"A_torch_chain": step_a, "B_refl_scope_loss": step_b}
    for _ in range(args.warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    dev_ms = {k: [] for k in fns}
    host_ms = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                f()
            e1.record()
            e1.synchronize()
            dev_ms[k].append(e0.elapsed_time(e1) / args.inner)
        for k, f in fns.items():
            torch.cuda.synchronize()
            for _ in range(args.chain):
                filler.add_(1.0)
            t0 = time.perf_counter()
            f()
            for _ in range(args.chain):
                filler.add_(1.0)
            host_ms[k].append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.chain):
        filler.add_(1.0)
    enqueue = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    chain = (time.perf_counter() - t0) * 1e3
    # B's kernels alone, by the library's own stage events (B's device figure above is bounded by what the host takes to enqueue a call)
    import _gsr
    _gsr.profile_enable(True)
    for _ in range(args.inner):
        step_b()
    torch.cuda.synchronize()
    stages = _gsr.profile_collect()
    _gsr.profile_enable(False)
    out = {"what": "env-scope term at P = %d, forward + backward, alternating calls: device-event ms per call, and host ms over the call and a trailing "
                   "chain of %d enqueued kernels, behind a leading chain of the same length" % (P, args.chain),
           "repeats": args.repeats, "inner": args.inner, "outside_fraction": round(float((torch.sum((xyz - centre_dev[None]) ** 2, dim=-1) > radius ** 2).float().mean()), 3),
           "chain_enqueue_ms": round(enqueue, 3), "chain_run_ms": round(chain, 3)}
    for k in fns:
        for name, ms in (("device", dev_ms[k]), ("host_with_chain", host_ms[k])):
            out[f"{k}_{name}_ms_p50"] = round(float(np.median(ms)), 4)
            out[f"{k}_{name}_ms_min"] = round(float(np.min(ms)), 4)
            out[f"{k}_{name}_ms_max"] = round(float(np.max(ms)), 4)
    for name, stage in (("forward", "loss_fwd"), ("backward", "loss_bwd")):
        total, launches = stages[stage]
        out[f"B_kernels_{name}_us"] = round(1e3 * total / max(launches, 1), 2)
    out["B_over_A_device"] = round(float(np.median(dev_ms["B_refl_scope_loss"]) / np.median(dev_ms["A_torch_chain"])), 4)
    out["B_over_A_host_with_chain"] = round(float(np.median(host_ms["B_refl_scope_loss"]) / np.median(host_ms["A_torch_chain"])), 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
