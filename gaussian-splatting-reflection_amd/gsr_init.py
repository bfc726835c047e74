"""A training state from a point cloud: the reference's fetchPly (scene/dataset_readers.py:142-151) and
GaussianModel.create_from_pcd (scene/gaussian_model.py:160-187) in this port's parametrisation.

GaussianTrainState and render() take ACTIVATED values (scales, opacities, reflection strengths as the rasterizer consumes them, see
tests/test_gpu_train.py), so init_from_point_cloud returns the activations of the reference's initial raw parameters:
    shs             (P, (D+1)^2, 3)  DC = RGB2SH(rgb) = (rgb - 0.5) / C0, the rest zero
    scales          (P, 2)           sqrt(clamp_min(distCUDA2(points), 1e-7))      (reference: log of it, activated with exp)
    rotations       (P, 4)           normalize(rand(P, 4))                          (reference: raw rand, normalised on use)
    opacities       (P, 1)           init_opacity                                   (reference: inverse_sigmoid of it)
    refl_strengths  (P, 1)           init_refl
    cubemap         (6, 3, L, L)     rand - 0.5 (cubemap_encoder.py), fail (3,) zeros
"""
import numpy as np
import torch

from scene.ply_io import read_ply_vertices
from simple_knn._C import distCUDA2

SH_C0 = 0.28209479177387814


def load_point_cloud(path, seed=None):
    """fetchPly: (points float32 (P, 3), colors float32 (P, 3) in [0, 1]).  A cloud without red/green/blue gets
    np.random.random((P, 3)) / 255 as the reference does; `seed` makes that draw reproducible."""
    v = read_ply_vertices(path)
    names = v.dtype.names
    points = np.stack([np.asarray(v[n], dtype=np.float32) for n in ("x", "y", "z")], axis=1)
    if "red" in names:
        colors = np.stack([np.asarray(v[n], dtype=np.float64) for n in ("red", "green", "blue")], axis=1) / 255.0
    else:
        rng = np.random if seed is None else np.random.RandomState(seed)
        colors = rng.random_sample((points.shape[0], 3)) / 255.0
    return points, colors.astype(np.float32)


def init_from_point_cloud(points, colors, sh_degree=3, init_opacity=0.1, init_refl=1e-3, cubemap_resolution=128, generator=None):
    """create_from_pcd on the points' device (a GPU: distCUDA2 runs there).  `points` / `colors` are (P, 3) tensors or arrays;
    arrays go to the current GPU.  `generator` (a torch.Generator on that device) seeds the random rotations and cubemap.
    Returns {name: tensor} with the keys of GaussianTrainState.ORDER."""
    pts = torch.as_tensor(points, dtype=torch.float32)
    if not pts.is_cuda:
        pts = pts.cuda()
    dev = pts.device
    rgb = torch.as_tensor(colors, dtype=torch.float32).to(dev)
    P, M = pts.shape[0], (sh_degree + 1) ** 2
    shs = torch.zeros(P, M, 3, dtype=torch.float32, device=dev)
    shs[:, 0, :] = (rgb - 0.5) / SH_C0
    dist2 = torch.clamp_min(distCUDA2(pts), 1e-7)
    scales = torch.sqrt(dist2)[:, None].repeat(1, 2)
    rots = torch.rand(P, 4, device=dev, generator=generator)
    rots = torch.nn.functional.normalize(rots, dim=1)
    L = cubemap_resolution
    return dict(means3D=pts.contiguous(), shs=shs, opacities=torch.full((P, 1), float(init_opacity), device=dev),
                scales=scales.contiguous(), rotations=rots, refl_strengths=torch.full((P, 1), float(init_refl), device=dev),
                cubemap=torch.rand(6, 3, L, L, device=dev, generator=generator) - 0.5, fail=torch.zeros(3, device=dev))
