"""The reference's `scene` package as far as this port goes: GaussianModel (scene/gaussian_model.py) and the on-disk formats
(scene/ply_io.py).  `from scene import GaussianModel` resolves on first use, so that `import scene.ply_io` stays host-side only."""


def __getattr__(name):
    if name == "GaussianModel":
        from scene.gaussian_model import GaussianModel
        return GaussianModel
    raise AttributeError(f"module 'scene' has no attribute {name!r}")
