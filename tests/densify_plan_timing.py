"""Timing aid (not a test; needs a GPU): one densify_and_prune at the C3 size (P = 10^6 surfels, statistics and scales as in
tests/densify_fixtures.py, a size threshold given), the row map composed two ways:

  A  plan="torch"    the host composes the map with torch ops: some forty ops, about ten boolean indexes (each a nonzero the host WAITS for)
                     and a dozen P-sized temporaries.
  B  plan="device"   libgsr_hip.so composes it (gsr_densify_plan_select / _rows, include/gsr_hip_densify.h): two 16-byte reads.

Everything behind the plan (the successor state, three gathers, the env group's copies) is shared and inside both figures.  Calls alternate
in one process on one device after a warm-up.  Per plan:
  device  the time between two device events around one call.
  host    the host clock over the call FOLLOWED BY a chain of `--chain` enqueued kernels (the rest of an iteration; each streams a
          `--filler-mb` buffer, so it runs longer than it takes to enqueue), with the same chain already enqueued in front of it (the
          device is behind the host, as it is in training): every read holds the host until the device has caught up.
  peak    torch.cuda.max_memory_allocated over the call, less what was allocated before it.
Prints one JSON line: medians with [min, max], and first checks once at this size that both plans return the same state bit for bit.

    python tests/densify_plan_timing.py [--repeats N] [--warmup W] [--points P] [--chain C] [--filler-mb M]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--chain", type=int, default=40)
    ap.add_argument("--filler-mb", type=int, default=256, help="size of the buffer each chain kernel reads and writes")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("densify_plan_timing.py measures on the GPU; none is available")
    import densify_fixtures as F
    import gsr_synth as S
    from gsr_densify import DensifyStats, densify_and_prune
    from gsr_train import GaussianTrainState
    P = args.points
    fx = F.make(P, 7, mix="views", stats_seed=3)
    bad_scale, bad_d2, _ = F.bands(fx)
    assert bad_scale.size == 0 and bad_d2.size == 0
    tex, fail = S.make_cubemap(8, 3, 7)
    tensors = {k: torch.from_numpy(fx["scene"][k]) for k in F.GROUPS}
    tensors["cubemap"], tensors["fail"] = torch.from_numpy(tex), torch.from_numpy(fail)
    st = GaussianTrainState(tensors, "cuda")
    st.optimizer.exp_avg.normal_()
    st.optimizer.exp_avg_sq.uniform_()
    stats = DensifyStats(P, "cuda")
    stats.buf.copy_(torch.from_numpy(np.stack([fx["stats"][k] for k in F.STAT_NAMES])))
    k = int(F.classes(fx)[2].sum())
    noise = torch.from_numpy(fx["noise_pool"][:fx["N"] * k]).cuda()
    mean = torch.tensor(fx["mean"])
    filler = torch.zeros(args.filler_mb << 18, device="cuda")      # (each chain kernel must run longer than it takes to enqueue: the device falls behind)

    def call(plan):
        return densify_and_prune(st, stats, F.MAX_GRAD, F.MIN_OPACITY, mean, fx["extent"], 20, noise=noise, plan=plan)

    # the outputs-equal check at this size, once
    (a, sa, ia), (b, sb, ib) = call("torch"), call("device")
    assert ia == ib, (ia, ib)
    assert torch.equal(a.params.flat, b.params.flat) and torch.equal(a.optimizer.exp_avg, b.optimizer.exp_avg)
    assert torch.equal(a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq) and torch.equal(sa.buf, sb.buf)
    assert min(ia["pruned_by_weight"], ia["cloned"], ia["split"], ia["pruned_big"]) > 100
    info = ia
    del a, b, sa, sb

    plans = {"A_torch_plan": "torch", "B_device_plan": "device"}
    for _ in range(args.warmup):
        for p in plans.values():
            call(p)
    torch.cuda.synchronize()
    dev_ms, host_ms, peak_mb = ({k: [] for k in plans} for _ in range(3))
    for _ in range(args.repeats):
        for name, p in plans.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call(p)
            e1.record()
            e1.synchronize()
            dev_ms[name].append(e0.elapsed_time(e1))
            peak_mb[name].append((torch.cuda.max_memory_allocated() - base) / 2 ** 20)
            del out
        for name, p in plans.items():
            torch.cuda.synchronize()
            for _ in range(args.chain):
                filler.add_(1.0)
            t0 = time.perf_counter()
            out = call(p)
            for _ in range(args.chain):
                filler.add_(1.0)
            host_ms[name].append((time.perf_counter() - t0) * 1e3)
            del out
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.chain):
        filler.add_(1.0)
    enqueue = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    chain = (time.perf_counter() - t0) * 1e3
    out = {"what": "densify_and_prune at P = %d with a size threshold, alternating calls: device-event ms per call; host ms over the call and a trailing "
                   "chain of %d enqueued kernels, behind a leading chain of the same length; peak MiB allocated over the call" % (P, args.chain),
           "repeats": args.repeats, "info": info, "outputs_equal": True, "chain_enqueue_ms": round(enqueue, 3), "chain_run_ms": round(chain, 3)}
    for name in plans:
        for what, v in (("device_ms", dev_ms[name]), ("host_with_chain_ms", host_ms[name]), ("peak_mib", peak_mb[name])):
            out[f"{name}_{what}"] = [round(float(np.median(v)), 3), [round(float(np.min(v)), 3), round(float(np.max(v)), 3)]]
    for what, v in (("device", dev_ms), ("host_with_chain", host_ms), ("peak", peak_mb)):
        out[f"B_over_A_{what}"] = round(float(np.median(v["B_device_plan"]) / np.median(v["A_torch_plan"])), 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
