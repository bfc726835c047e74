"""The sparse-volume entries (include/gsr_hip_sparse.h: gsr_sparse_tsdf_touch, gsr_sparse_tsdf_allocate, gsr_sparse_tsdf_integrate,
gsr_sparse_mesh_count, gsr_sparse_mesh_emit and the two size queries) on a machine without a GPU: every refusal the header lists returns
GSR_E_INVALID with a message naming the entry, the documented no-ops return 0, the size queries are host arithmetic, and the Python layer
asks for a rebuild when the entries are missing.  (That the header, the library and the binding agree is tests/test_cabi.py's, for every
header.)  The calls are made with fake pointers in a child process that sees no GPU (tests/cabi_child.py); `python test_cabi_sparse.py` is
that child."""
import sys

import pytest

import cabi_child
from cabi_args import FAKE

ENTRIES = ("gsr_sparse_tsdf_touch", "gsr_sparse_tsdf_allocate", "gsr_sparse_tsdf_integrate", "gsr_sparse_mesh_count", "gsr_sparse_mesh_emit")
QUERIES = ("gsr_sparse_tsdf_allocate_scratch_bytes", "gsr_sparse_mesh_scratch_bytes")


def test_python_layer_asks_for_a_rebuild_when_the_entries_are_missing(hip_lib_built, monkeypatch):
    import _gsr
    import gsr_mesh
    real = _gsr.lib

    class Old:
        """A library built before the sparse entries: everything but them."""
        def __getattr__(self, name):
            if name in ENTRIES + QUERIES:
                raise AttributeError(name)
            return getattr(real, name)
    monkeypatch.setattr(gsr_mesh, "lib", Old())
    with pytest.raises(ImportError, match=r"does not export gsr_sparse_tsdf_touch \(csrc/gsr_sparse\.hip\).*rebuild"):
        gsr_mesh.SparseTSDFVolume((0, 0, 0), 0.1, (9, 9, 9), "cpu")


def test_python_layer_refuses_what_the_entries_would(hip_lib_built):
    import gsr_mesh
    assert gsr_mesh.sparse_blocks((67, 55, 49)) == (9, 7, 7) and gsr_mesh.sparse_blocks((2, 8, 9)) == (1, 1, 2)
    for dims in ((1, 9, 9), (9, 9), (2 ** 14 * 8, 2 ** 14 * 8, 64)):
        with pytest.raises(ValueError, match="SparseTSDFVolume"):
            gsr_mesh.SparseTSDFVolume((0, 0, 0), 0.1, dims, "cpu")
    for voxel in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size"):
            gsr_mesh.SparseTSDFVolume((0, 0, 0), voxel, (9, 9, 9), "cpu")


def test_scratch_bytes_are_host_arithmetic(hip_lib_built):
    import _gsr
    alloc, mesh = _gsr.lib.gsr_sparse_tsdf_allocate_scratch_bytes, _gsr.lib.gsr_sparse_mesh_scratch_bytes
    # three words per 256 table entries and the two totals, each array on a 256-byte boundary
    assert alloc(67, 55, 49) == 1024 and alloc(2, 2, 2) == 1024
    g = 313 ** 3                                           # 2501^3 nodes
    assert 12 * (g // 256) <= alloc(2501, 2501, 2501) <= 12 * (g // 256 + 1) + 1024
    for bad in ((1, 19, 17), (23, 0, 17), (23, 19, -4), (8 * 2048, 8 * 1024, 8 * 1024), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        assert alloc(*bad) == 0, bad
    assert alloc(8 * 2047, 8 * 1024, 8 * 1024) > 0
    # eleven bytes per pool node, three words per 256 pool nodes
    assert mesh(83) >= 11 * 83 * 512 and mesh(83) % 256 == 0 and mesh(83) < mesh(84)
    assert mesh(0) == 0 and mesh(2 ** 22) == 0 and mesh(2 ** 63) == 0 and mesh(2 ** 22 - 1) > 11 * (2 ** 31 - 512)


# ------------------------------------------------------------------------------------------------- the refusals
_VOL = ("nx", "ny", "nz")
_PLACE = ("ox", "oy", "oz", "voxel")
_VIEW = ("alpha_min", "W", "H", "viewmatrix", "projmatrix", "sdf_trunc", "depth_trunc", "stream")
ARGS = {
    "gsr_sparse_tsdf_touch": ("table",) + _VOL + _PLACE + ("depth", "alpha") + _VIEW,
    "gsr_sparse_tsdf_allocate": ("table",) + _VOL + ("block_of_slot", "capacity", "counts", "scratch", "scratch_bytes", "stream"),
    "gsr_sparse_tsdf_integrate": ("block_of_slot", "n_slots", "capacity", "tsdf", "weight", "color") + _VOL + _PLACE + ("depth", "rgb", "alpha") + _VIEW,
    "gsr_sparse_mesh_count": ("table", "block_of_slot", "n_slots", "capacity", "tsdf", "weight") + _VOL + ("min_weight", "scratch", "scratch_bytes",
                                                                                                       "counts", "stream"),
    "gsr_sparse_mesh_emit": ("table", "block_of_slot", "n_slots", "capacity", "tsdf", "weight", "color") + _VOL + _PLACE + (
        "min_weight", "scratch", "verts", "vcolor", "faces", "nV", "nT", "stream"),
}
NX, NY, NZ, SLOTS, CAPACITY = 67, 55, 49, 83, 100
A = lambda k: FAKE + (k << 32)          # fake ranges far apart
SCRATCH = "scratch-bytes"               # replaced in the child by the entry's size query + the case's delta
_V = dict(nx=NX, ny=NY, nz=NZ)
_P = dict(ox=-1.0, oy=-0.5, oz=0.25, voxel=0.1)
_W = dict(alpha_min=0.5, W=61, H=45, viewmatrix=A(6), projmatrix=A(7), sdf_trunc=0.25, depth_trunc=3.0, stream=None)
_POOL = dict(block_of_slot=A(8), n_slots=SLOTS, capacity=CAPACITY, tsdf=A(0), weight=A(1))
BASE = {
    "gsr_sparse_tsdf_touch": dict(_V, **_P, **_W, table=A(9), depth=A(3), alpha=A(5)),
    "gsr_sparse_tsdf_allocate": dict(_V, table=A(9), block_of_slot=A(8), capacity=CAPACITY, counts=A(10), scratch=A(2), scratch_bytes=(SCRATCH, 0),
                                     stream=None),
    "gsr_sparse_tsdf_integrate": dict(_V, **_P, **_W, **_POOL, color=A(2), depth=A(3), rgb=A(4), alpha=A(5)),
    "gsr_sparse_mesh_count": dict(_V, **_POOL, table=A(9), min_weight=1.0, scratch=A(2), scratch_bytes=(SCRATCH, 0), counts=A(10), stream=None),
    "gsr_sparse_mesh_emit": dict(_V, **_P, **_POOL, table=A(9), color=A(2), min_weight=1.0, scratch=A(3), verts=A(4), vcolor=A(5), faces=A(6), nV=4709,
                                 nT=8670, stream=None),
}
INF, NAN = float("inf"), float("nan")
_SIZES = {
    "nx=1": dict(nx=1), "ny=1": dict(ny=1), "nz=1": dict(nz=1), "nx=0": dict(nx=0), "ny<0": dict(ny=-19), "nz<0": dict(nz=-1),
    "blocks=2^31": dict(nx=8 * 2048, ny=8 * 1024, nz=8 * 1024), "gx*gy=2^32": dict(nx=8 * 65536, ny=8 * 65536, nz=2),
    "blocks-beyond-64-bits-of-nodes": dict(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1),
}
_GRID = {"voxel=0": dict(voxel=0.0), "voxel<0": dict(voxel=-0.1), "voxel=inf": dict(voxel=INF), "voxel=nan": dict(voxel=NAN),
         "ox=nan": dict(ox=NAN), "oy=inf": dict(oy=INF), "oz=-inf": dict(oz=-INF)}
_VIEWS = {
    "null:depth": dict(depth=None), "null:viewmatrix": dict(viewmatrix=None), "null:projmatrix": dict(projmatrix=None),
    "misaligned:depth": dict(depth=A(3) + 3), "misaligned:alpha": dict(alpha=A(5) + 1), "misaligned:viewmatrix": dict(viewmatrix=A(6) + 2),
    "misaligned:projmatrix": dict(projmatrix=A(7) + 2),
    "sdf_trunc=0": dict(sdf_trunc=0.0), "sdf_trunc<0": dict(sdf_trunc=-0.25), "sdf_trunc=inf": dict(sdf_trunc=INF), "sdf_trunc=nan": dict(sdf_trunc=NAN),
    "depth_trunc=0": dict(depth_trunc=0.0), "depth_trunc<0": dict(depth_trunc=-3.0), "depth_trunc=inf": dict(depth_trunc=INF),
    "depth_trunc=nan": dict(depth_trunc=NAN), "alpha_min=nan": dict(alpha_min=NAN), "W=0": dict(W=0), "H=0": dict(H=0), "W<0": dict(W=-61),
    "H<0": dict(H=-1), "W*H=2^31": dict(W=65536, H=32768),
}
_POOLS = {
    "null:block_of_slot": dict(block_of_slot=None), "null:tsdf": dict(tsdf=None), "null:weight": dict(weight=None),
    "misaligned:block_of_slot": dict(block_of_slot=A(8) + 2), "misaligned:tsdf": dict(tsdf=A(0) + 2), "misaligned:weight": dict(weight=A(1) + 1),
    "n_slots>capacity": dict(n_slots=CAPACITY + 1), "capacity*512=2^31": dict(capacity=2 ** 22), "capacity=2^63": dict(capacity=2 ** 63, n_slots=2 ** 63),
}
REFUSED = {
    "gsr_sparse_tsdf_touch": dict(_SIZES, **_GRID, **_VIEWS, **{"null:table": dict(table=None), "misaligned:table": dict(table=A(9) + 2)}),
    "gsr_sparse_tsdf_allocate": dict(_SIZES, **{
        "null:table": dict(table=None), "null:block_of_slot": dict(block_of_slot=None), "null:counts": dict(counts=None), "null:scratch": dict(scratch=None),
        "misaligned:table": dict(table=A(9) + 2), "misaligned:block_of_slot": dict(block_of_slot=A(8) + 1), "misaligned:counts": dict(counts=A(10) + 4),
        "misaligned:scratch": dict(scratch=A(2) + 8), "scratch-one-byte-short": dict(scratch_bytes=(SCRATCH, -1)), "scratch_bytes=0": dict(scratch_bytes=0),
        "capacity*512=2^31": dict(capacity=2 ** 22), "capacity=2^64-1": dict(capacity=2 ** 64 - 1),
    }),
    "gsr_sparse_tsdf_integrate": dict(_SIZES, **_GRID, **_VIEWS, **_POOLS, **{
        "color-without-rgb": dict(rgb=None), "rgb-without-color": dict(color=None), "misaligned:color": dict(color=A(2) + 2),
        "misaligned:rgb": dict(rgb=A(4) + 2),
    }),
    "gsr_sparse_mesh_count": dict(_SIZES, **_POOLS, **{
        "null:table": dict(table=None), "null:scratch": dict(scratch=None), "null:counts": dict(counts=None), "misaligned:table": dict(table=A(9) + 2),
        "misaligned:scratch": dict(scratch=A(2) + 8), "misaligned:counts": dict(counts=A(10) + 4), "scratch-one-byte-short": dict(scratch_bytes=(SCRATCH, -1)),
        "scratch_bytes=0": dict(scratch_bytes=0), "min_weight=nan": dict(min_weight=NAN),
    }),
    "gsr_sparse_mesh_emit": dict(_SIZES, **_GRID, **_POOLS, **{
        "null:table": dict(table=None), "null:scratch": dict(scratch=None), "null:verts": dict(verts=None), "null:faces": dict(faces=None),
        "vcolor-without-color": dict(color=None), "color-without-vcolor": dict(vcolor=None), "misaligned:table": dict(table=A(9) + 2),
        "misaligned:color": dict(color=A(2) + 1), "misaligned:scratch": dict(scratch=A(3) + 4), "misaligned:verts": dict(verts=A(4) + 2),
        "misaligned:vcolor": dict(vcolor=A(5) + 2), "misaligned:faces": dict(faces=A(6) + 2), "nV=2^31": dict(nV=2 ** 31),
        "3nT=2^31+1": dict(nT=(2 ** 31 + 1) // 3 + 1), "nT=2^63": dict(nT=2 ** 63), "nV=2^64-1": dict(nV=2 ** 64 - 1),
    }),
}
# calls that must NOT be refused (without a device the launch fails: any code but GSR_E_INVALID)
_BOX_2501 = dict(nx=2501, ny=2501, nz=2501)                 # upstream's voxel over a box of +-5: what the dense entries refuse
ACCEPTED = {
    "gsr_sparse_tsdf_touch": {"well-formed": {}, "no-alpha": dict(alpha=None), "smallest": dict(nx=2, ny=2, nz=2, W=1, H=1), "2501^3": _BOX_2501,
                              "largest": dict(nx=8 * 2047, ny=8 * 1024, nz=8 * 1024), "alpha_min<0": dict(alpha_min=-1.0)},
    "gsr_sparse_tsdf_allocate": {"well-formed": {}, "scratch-larger": dict(scratch_bytes=(SCRATCH, 4096)), "largest-capacity": dict(capacity=2 ** 22 - 1),
                                 "capacity=0-without-block_of_slot": dict(capacity=0, block_of_slot=None), "2501^3": _BOX_2501},
    "gsr_sparse_tsdf_integrate": {"well-formed": {}, "no-colour": dict(color=None, rgb=None), "no-alpha": dict(alpha=None), "2501^3": _BOX_2501,
                                  "n_slots=capacity": dict(n_slots=CAPACITY), "largest-pool": dict(n_slots=2 ** 22 - 1, capacity=2 ** 22 - 1)},
    "gsr_sparse_mesh_count": {"well-formed": {}, "min_weight=0": dict(min_weight=0.0), "min_weight=inf": dict(min_weight=INF),
                              "scratch-larger": dict(scratch_bytes=(SCRATCH, 4096)), "2501^3": _BOX_2501},
    "gsr_sparse_mesh_emit": {"well-formed": {}, "no-colour": dict(color=None, vcolor=None), "largest-counts": dict(nV=2 ** 31 - 1, nT=(2 ** 31 - 1) // 3),
                             "no-triangles-no-faces": dict(nT=0, faces=None), "2501^3": _BOX_2501},
}
# nothing to do: returns 0 without a launch (the pool and the outputs may be NULL)
_NO_POOL = dict(n_slots=0, block_of_slot=None, tsdf=None, weight=None)
NOOP = {
    "gsr_sparse_tsdf_integrate": {"n_slots=0": dict(n_slots=0), "n_slots=0-null-pool": dict(_NO_POOL, color=None, rgb=None, capacity=0)},
    "gsr_sparse_mesh_emit": {"nV=0": dict(nV=0, nT=0), "nV=0-null-outputs": dict(nV=0, nT=0, verts=None, vcolor=None, faces=None),
                             "n_slots=0-null-pool": dict(_NO_POOL, color=None, vcolor=None, scratch=None, capacity=0)},
}
TABLES = (("accepted", ACCEPTED), ("refused", REFUSED), ("noop", NOOP))


CASES = cabi_child.cases(ENTRIES, TABLES)


def _call(gsr, entry, case):
    args = dict(BASE[entry], **cabi_child.changes(TABLES, entry, case))
    if isinstance(args.get("scratch_bytes"), tuple):
        need = (gsr.lib.gsr_sparse_tsdf_allocate_scratch_bytes(args["nx"], args["ny"], args["nz"]) if entry == "gsr_sparse_tsdf_allocate"
                else gsr.lib.gsr_sparse_mesh_scratch_bytes(args["n_slots"]))
        args["scratch_bytes"] = int(need) + args["scratch_bytes"][1]
    return getattr(gsr.lib, entry)(*[args[k] for k in ARGS[entry]])


@pytest.fixture(scope="module")
def outcomes(hip_lib_built):
    return cabi_child.run(__file__)


@pytest.mark.parametrize("entry, case, expect", CASES, ids=lambda v: v)
def test_refusal(outcomes, entry, case, expect):
    cabi_child.check(outcomes, entry, case, expect)


if __name__ == "__main__":
    sys.exit(cabi_child.serve([c[:2] for c in CASES], _call))
