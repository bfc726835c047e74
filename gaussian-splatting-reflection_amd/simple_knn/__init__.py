"""MI355X drop-in for the reference's `simple_knn` package (submodules/simple-knn): `from simple_knn._C import distCUDA2`
(scene/gaussian_model.py:20) resolves to the exact 3-nearest-neighbour kernel of libgsr_hip.so (csrc/gsr_knn.hip)."""
from . import _C  # noqa: F401
