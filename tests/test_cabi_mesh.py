"""The mesh entries (include/gsr_hip_mesh.h: gsr_tsdf_integrate, gsr_mesh_scratch_bytes, gsr_mesh_count, gsr_mesh_emit) on a machine
without a GPU: every refusal the header lists returns GSR_E_INVALID with a message naming the entry, the documented no-op returns 0, and
the Python layer asks for a rebuild when the entries are missing.  (That the header, the library and the binding agree is
tests/test_cabi.py's, for every header.)  The calls are made with fake pointers in a child process that sees no GPU (tests/cabi_child.py);
`python test_cabi_mesh.py` is that child."""
import importlib
import sys

import pytest

import cabi_child
from cabi_args import FAKE

ENTRIES = ("gsr_tsdf_integrate", "gsr_mesh_count", "gsr_mesh_emit")


def test_python_layer_asks_for_a_rebuild_when_the_entries_are_missing(hip_lib_built, monkeypatch):
    import _gsr
    import gsr_mesh
    real = _gsr.lib

    class Old:
        """A library built before the mesh entries: everything but them."""
        def __getattr__(self, name):
            if name in ENTRIES + ("gsr_mesh_scratch_bytes",):
                raise AttributeError(name)
            return getattr(real, name)
    monkeypatch.setattr(_gsr, "lib", Old())
    try:
        with pytest.raises(ImportError, match=r"does not export gsr_tsdf_integrate \(csrc/gsr_mesh\.hip\).*rebuild"):
            importlib.reload(gsr_mesh)
    finally:
        monkeypatch.undo()
        importlib.reload(gsr_mesh)


def test_scratch_bytes_is_host_arithmetic(hip_lib_built):
    import _gsr
    q = _gsr.lib.gsr_mesh_scratch_bytes
    n = 23 * 19 * 17
    assert q(23, 19, 17) >= 11 * n and q(23, 19, 17) % 256 == 0           # three byte arrays and two word arrays per node
    assert q(23, 19, 17) < q(24, 19, 17)
    for bad in ((1, 19, 17), (23, 0, 17), (23, 19, -4), (2048, 1024, 1024), (65536, 65536, 2)):
        assert q(*bad) == 0, bad
    assert q(2047, 1024, 1024) > 0


def test_scratch_sizes_are_the_recorded_ones(hip_lib_built):
    """The three size queries whose layouts are carved by one function each (mesh_carve, clean_carve, knn_carve): the values below were
    read from the library as it was before the layouts moved onto Carver, at one node, block and leaf on either side of a boundary, at
    empty arrays and at the largest sizes.  A caller's buffer sized by an older library must still fit: none of them may change."""
    import _gsr
    mesh = {(2, 2, 2): 2048, (23, 19, 17): 83712, (64, 4, 8): 23296, (65, 5, 9): 33536, (2047, 1024, 1024): 23711399936,
            (1, 19, 17): 0, (23, 0, 17): 0, (23, 19, -4): 0, (2048, 1024, 1024): 0, (65536, 65536, 2): 0}
    clean = {(1, 1): 6400, (255, 257): 9984, (256, 256): 9472, (70000, 0): 918272, (0, 0): 4096, (0, 1504): 12544,
             (2 ** 31 - 1, (2 ** 31 - 1) // 3): 31597094400, (2 ** 31, 1504): 0, (754, (2 ** 31 + 2) // 3): 0}
    knn = {(1,): 20736, (255,): 28416, (256,): 28416, (257,): 29952, (100000,): 3768320, (2 ** 30 - 1,): 40273851648,
           (0,): 0, (-1,): 0, (2 ** 30,): 0}
    for name, table in (("gsr_mesh_scratch_bytes", mesh), ("gsr_mesh_clean_scratch_bytes", clean), ("gsr_knn_scratch_bytes", knn)):
        for sizes, expected in table.items():
            assert int(getattr(_gsr.lib, name)(*sizes)) == expected, (name, sizes)


# ------------------------------------------------------------------------------------------------- the refusals
ARGS = {
    "gsr_tsdf_integrate": ("tsdf", "weight", "color", "nx", "ny", "nz", "ox", "oy", "oz", "voxel", "depth", "rgb", "alpha", "alpha_min", "W", "H",
                           "viewmatrix", "projmatrix", "sdf_trunc", "depth_trunc", "stream"),
    "gsr_mesh_count": ("tsdf", "weight", "nx", "ny", "nz", "min_weight", "scratch", "scratch_bytes", "counts", "stream"),
    "gsr_mesh_emit": ("tsdf", "weight", "color", "nx", "ny", "nz", "ox", "oy", "oz", "voxel", "min_weight", "scratch", "verts", "vcolor", "faces",
                      "nV", "nT", "stream"),
}
NX, NY, NZ = 23, 19, 17
A = lambda k: FAKE + (k << 32)          # fake ranges far apart
SCRATCH = "scratch-bytes"               # replaced in the child by gsr_mesh_scratch_bytes(nx, ny, nz) + the case's delta
BASE = {
    "gsr_tsdf_integrate": dict(tsdf=A(0), weight=A(1), color=A(2), nx=NX, ny=NY, nz=NZ, ox=-1.0, oy=-0.5, oz=0.25, voxel=0.1, depth=A(3), rgb=A(4),
                               alpha=A(5), alpha_min=0.5, W=61, H=45, viewmatrix=A(6), projmatrix=A(7), sdf_trunc=0.25, depth_trunc=3.0, stream=None),
    "gsr_mesh_count": dict(tsdf=A(0), weight=A(1), nx=NX, ny=NY, nz=NZ, min_weight=1.0, scratch=A(2), scratch_bytes=(SCRATCH, 0), counts=A(3),
                           stream=None),
    "gsr_mesh_emit": dict(tsdf=A(0), weight=A(1), color=A(2), nx=NX, ny=NY, nz=NZ, ox=-1.0, oy=-0.5, oz=0.25, voxel=0.1, min_weight=1.0,
                          scratch=A(3), verts=A(4), vcolor=A(5), faces=A(6), nV=754, nT=1504, stream=None),
}
INF, NAN = float("inf"), float("nan")
_SIZES = {
    "nx=1": dict(nx=1), "ny=1": dict(ny=1), "nz=1": dict(nz=1), "nx=0": dict(nx=0), "ny<0": dict(ny=-19), "nz<0": dict(nz=-1),
    "nx*ny*nz=2^31": dict(nx=2048, ny=1024, nz=1024), "nx*ny=2^32": dict(nx=65536, ny=65536, nz=2),
    "nx*ny*nz-beyond-64-bits": dict(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1),
}
_GRID = {"voxel=0": dict(voxel=0.0), "voxel<0": dict(voxel=-0.1), "voxel=inf": dict(voxel=INF), "voxel=nan": dict(voxel=NAN),
         "ox=nan": dict(ox=NAN), "oy=inf": dict(oy=INF), "oz=-inf": dict(oz=-INF)}
REFUSED = {
    "gsr_tsdf_integrate": dict(_SIZES, **_GRID, **{
        "null:tsdf": dict(tsdf=None), "null:weight": dict(weight=None), "null:depth": dict(depth=None), "null:viewmatrix": dict(viewmatrix=None),
        "null:projmatrix": dict(projmatrix=None), "color-without-rgb": dict(rgb=None), "rgb-without-color": dict(color=None),
        "misaligned:tsdf": dict(tsdf=A(0) + 2), "misaligned:weight": dict(weight=A(1) + 1), "misaligned:color": dict(color=A(2) + 2),
        "misaligned:depth": dict(depth=A(3) + 3), "misaligned:rgb": dict(rgb=A(4) + 2), "misaligned:alpha": dict(alpha=A(5) + 1),
        "misaligned:viewmatrix": dict(viewmatrix=A(6) + 2), "misaligned:projmatrix": dict(projmatrix=A(7) + 2),
        "sdf_trunc=0": dict(sdf_trunc=0.0), "sdf_trunc<0": dict(sdf_trunc=-0.25), "sdf_trunc=inf": dict(sdf_trunc=INF), "sdf_trunc=nan": dict(sdf_trunc=NAN),
        "depth_trunc=0": dict(depth_trunc=0.0), "depth_trunc<0": dict(depth_trunc=-3.0), "depth_trunc=inf": dict(depth_trunc=INF),
        "depth_trunc=nan": dict(depth_trunc=NAN), "alpha_min=nan": dict(alpha_min=NAN), "W=0": dict(W=0), "H=0": dict(H=0), "W<0": dict(W=-61),
        "H<0": dict(H=-1), "W*H=2^31": dict(W=65536, H=32768),
    }),
    "gsr_mesh_count": dict(_SIZES, **{
        "null:tsdf": dict(tsdf=None), "null:weight": dict(weight=None), "null:scratch": dict(scratch=None), "null:counts": dict(counts=None),
        "misaligned:tsdf": dict(tsdf=A(0) + 2), "misaligned:weight": dict(weight=A(1) + 2), "misaligned:scratch": dict(scratch=A(2) + 8),
        "misaligned:counts": dict(counts=A(3) + 4), "scratch-one-byte-short": dict(scratch_bytes=(SCRATCH, -1)), "scratch_bytes=0": dict(scratch_bytes=0),
        "min_weight=nan": dict(min_weight=NAN),
    }),
    "gsr_mesh_emit": dict(_SIZES, **_GRID, **{
        "null:tsdf": dict(tsdf=None), "null:weight": dict(weight=None), "null:scratch": dict(scratch=None), "null:verts": dict(verts=None),
        "null:faces": dict(faces=None), "vcolor-without-color": dict(color=None), "color-without-vcolor": dict(vcolor=None),
        "misaligned:tsdf": dict(tsdf=A(0) + 2), "misaligned:color": dict(color=A(2) + 1), "misaligned:scratch": dict(scratch=A(3) + 4),
        "misaligned:verts": dict(verts=A(4) + 2), "misaligned:vcolor": dict(vcolor=A(5) + 2), "misaligned:faces": dict(faces=A(6) + 2),
        "nV=2^31": dict(nV=2 ** 31), "3nT=2^31+1": dict(nT=(2 ** 31 + 1) // 3 + 1), "nT=2^63": dict(nT=2 ** 63), "nV=2^64-1": dict(nV=2 ** 64 - 1),
    }),
}
# calls that must NOT be refused (without a device the launch fails: any code but GSR_E_INVALID)
ACCEPTED = {
    "gsr_tsdf_integrate": {
        "well-formed": {}, "no-colour": dict(color=None, rgb=None), "no-alpha": dict(alpha=None), "smallest": dict(nx=2, ny=2, nz=2, W=1, H=1),
        "largest": dict(nx=2047, ny=1024, nz=1024), "alpha_min<0": dict(alpha_min=-1.0),
    },
    "gsr_mesh_count": {"well-formed": {}, "min_weight=0": dict(min_weight=0.0), "min_weight=inf": dict(min_weight=INF),
                       "scratch-larger": dict(scratch_bytes=(SCRATCH, 4096))},
    "gsr_mesh_emit": {"well-formed": {}, "no-colour": dict(color=None, vcolor=None), "largest-counts": dict(nV=2 ** 31 - 1, nT=(2 ** 31 - 1) // 3),
                      "no-triangles-no-faces": dict(nT=0, faces=None)},
}
# nV == 0: nothing to write, returns 0 without a launch (the outputs may be NULL)
NOOP = {"gsr_mesh_emit": {"nV=0": dict(nV=0, nT=0), "nV=0-null-outputs": dict(nV=0, nT=0, verts=None, vcolor=None, faces=None)}}
TABLES = (("accepted", ACCEPTED), ("refused", REFUSED), ("noop", NOOP))


CASES = cabi_child.cases(ENTRIES, TABLES)


def _call(gsr, entry, case):
    args = dict(BASE[entry], **cabi_child.changes(TABLES, entry, case))
    if isinstance(args.get("scratch_bytes"), tuple):
        args["scratch_bytes"] = int(gsr.lib.gsr_mesh_scratch_bytes(NX, NY, NZ)) + args["scratch_bytes"][1]
    return getattr(gsr.lib, entry)(*[args[k] for k in ARGS[entry]])


@pytest.fixture(scope="module")
def outcomes(hip_lib_built):
    return cabi_child.run(__file__)


@pytest.mark.parametrize("entry, case, expect", CASES, ids=lambda v: v)
def test_refusal(outcomes, entry, case, expect):
    cabi_child.check(outcomes, entry, case, expect)


if __name__ == "__main__":
    sys.exit(cabi_child.serve([c[:2] for c in CASES], _call))
