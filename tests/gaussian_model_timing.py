"""Timing aid (not a test; needs a GPU): what scene.GaussianModel costs per iteration, and the statistics kernel under a boolean filter.

  1  HOST time of the model's calls of one iteration at P points (default 10^6): the seven getters render() reads, add_densification_stats,
     optimizer.step() and optimizer.zero_grad(), against the same iteration wired by hand on a RawTrainState + DensifyStats (its dict
     lookups, DensifyStats.update, state.optimizer.step(), state.grads.zero_()).  The host clock runs over the calls only (they enqueue);
     the device is idle before each sample and is waited for after it.  Variants alternate inside one process:
        hand     the hand-wired iteration (everything in it exists without the class)
        model    the reference's lines: the max_radii2D line is NOT in it (it is the caller's, in both worlds), add_densification_stats
                 with the boolean filter
        radii    the same with add_densification_stats(..., radii=): the fused entry the hand-wired iteration calls
  2  DEVICE time of gsr_densification_stats_filter against gsr_densification_stats at the same P, by device events around batches of
     `--batch` launches, alternating; the two write the same four statistics (checked once, bit for bit).

Prints one JSON line: sample counts, medians with [min, max].

    python tests/gaussian_model_timing.py [--points P] [--repeats N] [--warmup W] [--batch B]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-reflection_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def summary(v, digits=4):
    return [round(float(np.median(v)), digits), [round(float(np.min(v)), digits), round(float(np.max(v)), digits)]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gaussian_model_timing.py measures on the GPU; none is available")
    import _gsr
    import gsr_synth as S
    from gsr_densify import DensifyStats
    from gsr_train import DEFAULT_LRS, RawTrainState, inverse_sigmoid
    from scene import GaussianModel
    from scene.ply_io import save_ply
    import tempfile
    P = args.points
    sc = S.make_scene(P, "S", seed=7, mu=-3.0)
    tex, fail = S.make_cubemap(16, 3, 7)
    t = {k: torch.from_numpy(sc[k]) for k in ("means3D", "shs", "opacities", "scales", "rotations", "refl_strengths")}
    raw = dict(t, opacities=inverse_sigmoid(t["opacities"]), refl_strengths=inverse_sigmoid(t["refl_strengths"]), scales=torch.log(t["scales"]),
               cubemap=torch.from_numpy(tex), fail=torch.from_numpy(fail))
    opt = types.SimpleNamespace(**dict(DEFAULT_LRS, percent_dense=0.01))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "point_cloud.ply")
        save_ply(path, raw["means3D"], raw["shs"], raw["opacities"], raw["refl_strengths"], raw["scales"], raw["rotations"], cubemap=tex, fail_value=fail)
        m = GaussianModel(3)
        m.load_ply(path)
    m.spatial_lr_scale = 1.0
    m.training_setup(opt)
    st = RawTrainState(raw, "cuda", spatial_lr_scale=1.0, lrs={k: getattr(opt, k) for k in DEFAULT_LRS})
    stats = DensifyStats(P, "cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    viewspace = torch.zeros(P, 3, device="cuda", requires_grad=True)
    viewspace.grad = torch.randn(P, 3, device="cuda", generator=gen) * 2e-4
    radii = (torch.randint(1, 40, (P,), device="cuda", generator=gen) * (torch.rand(P, device="cuda", generator=gen) < 0.6)).to(torch.int32)
    visibility_filter = radii > 0
    weights = torch.rand(P, device="cuda", generator=gen) * (torch.rand(P, device="cuda", generator=gen) < 0.5)
    for s in (m._state, st):
        s.grads.flat.normal_(generator=gen).mul_(1e-3)

    def hand():
        x = (st.p["means3D"], st.p["shs"], st.a["opacities"], st.a["scales"], st.a["rotations"], st.a["refl_strengths"], st.p["cubemap"])
        stats.update(viewspace.grad, radii, weights)
        st.optimizer.step()
        st.grads.zero_()
        return x

    def model():
        x = (m.get_xyz, m.get_features, m.get_opacity, m.get_scaling, m.get_rotation, m.get_refl, m.get_envmap)
        m.add_densification_stats(viewspace, visibility_filter, weights)
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
        return x

    def with_radii():
        x = (m.get_xyz, m.get_features, m.get_opacity, m.get_scaling, m.get_rotation, m.get_refl, m.get_envmap)
        m.add_densification_stats(viewspace, visibility_filter, weights, radii=radii)
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
        return x

    variants = {"hand": hand, "model": model, "radii": with_radii}
    for _ in range(args.warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    host_us = {k: [] for k in variants}
    for _ in range(args.repeats):
        for name, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            host_us[name].append((time.perf_counter() - t0) * 1e6)
            torch.cuda.synchronize()

    # ---- the two statistics kernels
    a, b = DensifyStats(P, "cuda"), DensifyStats(P, "cuda")
    f8 = visibility_filter.view(torch.uint8)
    r01 = visibility_filter.to(torch.int32)
    stream = _gsr.stream_ptr(a.buf.device)
    g = viewspace.grad

    def filt():
        _gsr.check(_gsr.lib.gsr_densification_stats_filter(P, g.data_ptr(), f8.data_ptr(), weights.data_ptr(), a.buf[0].data_ptr(), a.buf[1].data_ptr(),
                                                           a.buf[2].data_ptr(), a.buf[3].data_ptr(), stream), "gsr_densification_stats_filter")

    def fused():
        _gsr.check(_gsr.lib.gsr_densification_stats(P, g.data_ptr(), r01.data_ptr(), weights.data_ptr(), b.buf[0].data_ptr(), b.buf[1].data_ptr(),
                                                    b.buf[2].data_ptr(), b.buf[3].data_ptr(), b.buf[4].data_ptr(), stream), "gsr_densification_stats")
    filt()
    fused()
    torch.cuda.synchronize()
    assert torch.equal(a.buf[:4], b.buf[:4]) and not a.buf[4].any()
    kernels = {"filter": filt, "fused": fused}
    for _ in range(args.warmup):
        for f in kernels.values():
            f()
    dev_us = {k: [] for k in kernels}
    for _ in range(args.repeats):
        for name, f in kernels.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.batch):
                f()
            e1.record()
            e1.synchronize()
            dev_us[name].append(e0.elapsed_time(e1) * 1e3 / args.batch)
    out = {"what": "P = %d: host microseconds of the model calls of one iteration (enqueue only, device idle before, waited for after); device "
                   "microseconds per launch of the two statistics kernels (events around batches of %d)" % (P, args.batch),
           "samples": args.repeats, "warmup": args.warmup}
    for name in variants:
        out[f"host_us_{name}"] = summary(host_us[name], 1)
    out["host_us_model_minus_hand"] = round(float(np.median(host_us["model"]) - np.median(host_us["hand"])), 1)
    out["host_us_radii_minus_hand"] = round(float(np.median(host_us["radii"]) - np.median(host_us["hand"])), 1)
    for name in kernels:
        out[f"device_us_{name}"] = summary(dev_us[name], 2)
    out["filter_median_not_above_fused_max"] = bool(np.median(dev_us["filter"]) <= max(dev_us["fused"]))
    out["bytes_per_point"] = {"filter": 12 + 1 + 4 + 4 * 8, "fused": 12 + 4 + 4 + 5 * 8}      # all rows updated: reads + read-modify-writes
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
