"""The unbounded-extraction entries (include/gsr_hip_unbounded.h: gsr_tsdf_integrate_contracted, gsr_points_fuse_view,
gsr_uncontract_points) on a machine without a GPU: every refusal the header lists returns GSR_E_INVALID with a message naming the entry,
the documented no-ops return 0, the extremes the header allows are not refused, and the Python layer asks for a rebuild when the entries
are missing while the rest of gsr_mesh keeps working.  (That the header, the library and the binding agree is tests/test_cabi.py's, for
every header.)  The calls are made with fake pointers in a child process that sees no GPU (tests/cabi_child.py);
`python test_cabi_unbounded.py` is that child."""
import sys

import pytest

import cabi_child
from cabi_args import FAKE

ENTRIES = ("gsr_tsdf_integrate_contracted", "gsr_points_fuse_view", "gsr_uncontract_points")


def test_python_layer_asks_for_a_rebuild_when_the_entries_are_missing(hip_lib_built, monkeypatch):
    import gsr_mesh
    real = gsr_mesh.lib

    class Old:
        """A library built before the unbounded entries: everything but them."""
        def __getattr__(self, name):
            if name in ENTRIES:
                raise AttributeError(name)
            return getattr(real, name)
    monkeypatch.setattr(gsr_mesh, "lib", Old())

    class Volume:                                    # (the check comes first: nothing of the volume is looked at)
        integrate, extract = gsr_mesh.ContractedTSDFVolume.integrate, gsr_mesh.ContractedTSDFVolume.extract
    for call, entry in ((lambda: Volume().integrate(None, None), "gsr_tsdf_integrate_contracted"), (lambda: Volume().extract(), "gsr_uncontract_points"),
                        (lambda: gsr_mesh.color_vertices(None, [], 0.1), "gsr_points_fuse_view")):
        with pytest.raises(ImportError, match=r"does not export %s \(csrc/gsr_unbounded\.hip\).*rebuild" % entry):
            call()
    # the module itself, and what it had before the group, need no such entry
    assert gsr_mesh.lib.gsr_mesh_scratch_bytes(23, 19, 17) > 0 and gsr_mesh.lib.gsr_mesh_clean_scratch_bytes(10, 10) > 0


def test_python_layer_refuses_a_lattice_it_cannot_lay_out(hip_lib_built):
    """Before any allocation: the extent outside (0, 1.9], a resolution below 2 or beyond 2^31 - 1 nodes, a radius that is not positive."""
    import gsr_mesh
    for kw in (dict(extent=0.0), dict(extent=-1.0), dict(extent=1.91), dict(extent=float("nan")), dict(resolution=1), dict(resolution=1291),
               dict(radius=0.0), dict(radius=float("inf")), dict(center=(0.0, float("nan"), 0.0)), dict(center=(0.0, 0.0))):
        args = dict(dict(center=(0.0, 0.0, 0.0), radius=1.0, resolution=8, extent=1.5, device="cpu"), **kw)
        with pytest.raises(ValueError, match="ContractedTSDFVolume"):
            gsr_mesh.ContractedTSDFVolume(**args)
    vol = gsr_mesh.ContractedTSDFVolume((0.5, 0.0, -1.0), 2.0, 5, 1.9, "cpu")
    assert (vol.lo, vol.step, vol.voxel_size) == (-1.9, 0.95, 0.8) and float(vol.tsdf.min()) == 1.0 == float(vol.weight.max())
    vol.tsdf.zero_()
    vol.reset()
    assert float(vol.tsdf.min()) == 1.0 and tuple(vol.tsdf.shape) == (5, 5, 5)


def test_marching_cubes_with_contraction_wants_a_cube(hip_lib_built):
    from utils.mcube_utils import marching_cubes_with_contraction
    for kw in (dict(bounding_box_max=(1.0, 1.0, 2.0)), dict(bounding_box_min=(-1.0, 0.0, -1.0)), dict(bounding_box_max=(-1.0, -1.0, -1.0)),
               dict(resolution=1), dict(resolution=1291)):
        with pytest.raises(ValueError, match="marching_cubes_with_contraction"):
            marching_cubes_with_contraction(lambda p: p[:, 0], **dict(dict(resolution=8), **kw))


# ------------------------------------------------------------------------------------------------- the refusals
ARGS = {
    "gsr_tsdf_integrate_contracted": ("tsdf", "weight", "n", "lo", "step", "cx", "cy", "cz", "radius", "voxel", "depth", "W", "H", "viewmatrix",
                                      "projmatrix", "stream"),
    "gsr_points_fuse_view": ("points", "n_points", "color", "weight", "depth", "rgb", "W", "H", "viewmatrix", "projmatrix", "sdf_trunc", "stream"),
    "gsr_uncontract_points": ("src", "dst", "n_points", "cx", "cy", "cz", "radius", "max_range", "stream"),
}
A = lambda k: FAKE + (k << 32)          # fake ranges far apart
INF, NAN = float("inf"), float("nan")
BASE = {
    "gsr_tsdf_integrate_contracted": dict(tsdf=A(0), weight=A(1), n=33, lo=-1.9, step=0.11875, cx=-0.2, cy=0.1, cz=0.8, radius=0.5, voxel=0.03,
                                          depth=A(2), W=61, H=45, viewmatrix=A(3), projmatrix=A(4), stream=None),
    "gsr_points_fuse_view": dict(points=A(0), n_points=5000, color=A(1), weight=A(2), depth=A(3), rgb=A(4), W=61, H=45, viewmatrix=A(5),
                                 projmatrix=A(6), sdf_trunc=0.15, stream=None),
    "gsr_uncontract_points": dict(src=A(0), dst=A(1), n_points=5000, cx=-0.2, cy=0.1, cz=0.8, radius=0.5, max_range=32.0, stream=None),
}
_IMAGE = {"W=0": dict(W=0), "H=0": dict(H=0), "W=-1": dict(W=-1), "H=-5": dict(H=-5), "WH=2^31": dict(W=2 ** 16, H=2 ** 15),
          "WH-wraps-in-32-bits": dict(W=2 ** 31 - 1, H=2 ** 31 - 1)}
_CENTRE = {"cx=nan": dict(cx=NAN), "cy=inf": dict(cy=INF), "cz=-inf": dict(cz=-INF), "radius=0": dict(radius=0.0), "radius<0": dict(radius=-0.5),
           "radius=inf": dict(radius=INF), "radius=nan": dict(radius=NAN)}
_POINTS = {"n_points=2^31": dict(n_points=2 ** 31), "n_points=2^32": dict(n_points=2 ** 32), "n_points=2^64-1": dict(n_points=2 ** 64 - 1)}
REFUSED = {
    "gsr_tsdf_integrate_contracted": dict(_IMAGE, **_CENTRE, **{
        "null:tsdf": dict(tsdf=None), "null:weight": dict(weight=None), "null:depth": dict(depth=None), "null:viewmatrix": dict(viewmatrix=None),
        "null:projmatrix": dict(projmatrix=None),
        "misaligned:tsdf": dict(tsdf=A(0) + 2), "misaligned:weight": dict(weight=A(1) + 1), "misaligned:depth": dict(depth=A(2) + 2),
        "misaligned:viewmatrix": dict(viewmatrix=A(3) + 3), "misaligned:projmatrix": dict(projmatrix=A(4) + 2),
        "n=1": dict(n=1), "n=0": dict(n=0), "n=-3": dict(n=-3), "n^3=2^31-and-more": dict(n=1291), "n^3-wraps-in-32-bits": dict(n=1626),
        "n^3-wraps-in-64-bits": dict(n=2 ** 31 - 1), "n=2^22": dict(n=2 ** 22),
        "step=0": dict(step=0.0), "step<0": dict(step=-0.1), "step=inf": dict(step=INF), "step=nan": dict(step=NAN),
        "voxel=0": dict(voxel=0.0), "voxel<0": dict(voxel=-0.03), "voxel=inf": dict(voxel=INF), "voxel=nan": dict(voxel=NAN),
        "lo=nan": dict(lo=NAN), "lo=inf": dict(lo=INF), "lo=-inf": dict(lo=-INF),
    }),
    "gsr_points_fuse_view": dict(_IMAGE, **_POINTS, **{
        "null:points": dict(points=None), "null:color": dict(color=None), "null:weight": dict(weight=None), "null:depth": dict(depth=None),
        "null:rgb": dict(rgb=None), "null:viewmatrix": dict(viewmatrix=None), "null:projmatrix": dict(projmatrix=None),
        "null:depth-in-front-of-the-no-op": dict(n_points=0, depth=None), "null:rgb-in-front-of-the-no-op": dict(n_points=0, rgb=None),
        "misaligned:points": dict(points=A(0) + 2), "misaligned:color": dict(color=A(1) + 1), "misaligned:weight": dict(weight=A(2) + 2),
        "misaligned:depth": dict(depth=A(3) + 2), "misaligned:rgb": dict(rgb=A(4) + 3), "misaligned:viewmatrix": dict(viewmatrix=A(5) + 2),
        "misaligned:projmatrix": dict(projmatrix=A(6) + 2), "misaligned:color-in-front-of-the-no-op": dict(n_points=0, color=A(1) + 2),
        "sdf_trunc=0": dict(sdf_trunc=0.0), "sdf_trunc<0": dict(sdf_trunc=-0.15), "sdf_trunc=inf": dict(sdf_trunc=INF), "sdf_trunc=nan": dict(sdf_trunc=NAN),
        "sdf_trunc=0-in-front-of-the-no-op": dict(n_points=0, sdf_trunc=0.0), "W=0-in-front-of-the-no-op": dict(n_points=0, W=0),
    }),
    "gsr_uncontract_points": dict(_CENTRE, **_POINTS, **{
        "null:src": dict(src=None), "null:dst": dict(dst=None), "misaligned:src": dict(src=A(0) + 2), "misaligned:dst": dict(dst=A(1) + 1),
        "max_range=0": dict(max_range=0.0), "max_range<0": dict(max_range=-32.0), "max_range=inf": dict(max_range=INF), "max_range=nan": dict(max_range=NAN),
        "radius=0-in-front-of-the-no-op": dict(n_points=0, radius=0.0), "misaligned:dst-in-front-of-the-no-op": dict(n_points=0, dst=A(1) + 2),
    }),
}
# calls that must NOT be refused (without a device the launch fails: any code but GSR_E_INVALID)
ACCEPTED = {
    "gsr_tsdf_integrate_contracted": {
        "well-formed": {}, "n=2": dict(n=2), "largest-lattice": dict(n=1290), "largest-image": dict(W=2 ** 31 - 1, H=1), "tall-image": dict(W=1, H=2 ** 31 - 1),
        "one-pixel": dict(W=1, H=1), "lo>0": dict(lo=0.5), "tiny-scalars": dict(step=1e-38, voxel=1e-38, radius=1e-38),
        "huge-scalars": dict(step=3e38, voxel=3e38, radius=3e38, lo=-3e38, cx=3e38, cy=-3e38, cz=3e38)},
    "gsr_points_fuse_view": {"well-formed": {}, "one-point": dict(n_points=1), "most-points": dict(n_points=2 ** 31 - 1),
                             "largest-image": dict(W=2 ** 31 - 1, H=1), "tiny-sdf_trunc": dict(sdf_trunc=1e-38), "huge-sdf_trunc": dict(sdf_trunc=3e38)},
    "gsr_uncontract_points": {"well-formed": {}, "in-place": dict(dst=A(0)), "one-point": dict(n_points=1), "most-points": dict(n_points=2 ** 31 - 1),
                              "tiny-scalars": dict(radius=1e-38, max_range=1e-38), "huge-scalars": dict(radius=3e38, max_range=3e38, cx=-3e38)},
}
# n_points == 0: nothing to do, returns 0 without a launch (the per-point pointers may be NULL)
NOOP = {
    "gsr_points_fuse_view": {"n_points=0": dict(n_points=0), "n_points=0-null-pointers": dict(n_points=0, points=None, color=None, weight=None)},
    "gsr_uncontract_points": {"n_points=0": dict(n_points=0), "n_points=0-null-pointers": dict(n_points=0, src=None, dst=None)},
}
TABLES = (("accepted", ACCEPTED), ("refused", REFUSED), ("noop", NOOP))


CASES = cabi_child.cases(ENTRIES, TABLES)


def _call(gsr, entry, case):
    args = dict(BASE[entry], **cabi_child.changes(TABLES, entry, case))
    return getattr(gsr.lib, entry)(*[args[k] for k in ARGS[entry]])


@pytest.fixture(scope="module")
def outcomes(hip_lib_built):
    return cabi_child.run(__file__)


@pytest.mark.parametrize("entry, case, expect", CASES, ids=lambda v: v)
def test_refusal(outcomes, entry, case, expect):
    cabi_child.check(outcomes, entry, case, expect)


if __name__ == "__main__":
    sys.exit(cabi_child.serve([c[:2] for c in CASES], _call))
