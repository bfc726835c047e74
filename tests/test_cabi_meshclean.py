"""The mesh clean-up entries (include/gsr_hip_meshclean.h: gsr_mesh_clean_count, gsr_mesh_clean_scratch_bytes, gsr_mesh_clean_emit) on a
machine without a GPU: every refusal the header lists returns GSR_E_INVALID with a message naming the entry, the documented no-op returns
0, and the Python layer asks for a rebuild when the entries are missing while the rest of gsr_mesh keeps working.  (That the header, the
library and the binding agree is tests/test_cabi.py's, for every header.)  The calls are made with fake pointers in a child process that
sees no GPU (tests/cabi_child.py); `python test_cabi_meshclean.py` is that child."""
import sys

import pytest

import cabi_child
from cabi_args import FAKE

ENTRIES = ("gsr_mesh_clean_count", "gsr_mesh_clean_emit")


def test_python_layer_asks_for_a_rebuild_when_the_entries_are_missing(hip_lib_built, monkeypatch):
    import gsr_mesh
    real = gsr_mesh.lib

    class Old:
        """A library built before the clean-up entries: everything but them."""
        def __getattr__(self, name):
            if name in ENTRIES + ("gsr_mesh_clean_scratch_bytes",):
                raise AttributeError(name)
            return getattr(real, name)
    monkeypatch.setattr(gsr_mesh, "lib", Old())
    mesh = gsr_mesh.Mesh(None, None, None)           # (the check comes first: nothing of the mesh is looked at)
    for call in (lambda: gsr_mesh.clean_mesh(mesh), lambda: gsr_mesh.cluster_connected_triangles(mesh)):
        with pytest.raises(ImportError, match=r"does not export gsr_mesh_clean_count \(csrc/gsr_meshclean\.hip\).*rebuild"):
            call()
    from utils.mesh_utils import post_process_mesh
    with pytest.raises(ImportError, match=r"does not export gsr_mesh_clean_count"):
        post_process_mesh(mesh, cluster_to_keep=1)
    # the module itself, and what it had before the group, need no such entry
    assert gsr_mesh.lib.gsr_mesh_scratch_bytes(23, 19, 17) > 0


def test_scratch_bytes_is_host_arithmetic(hip_lib_built):
    import _gsr
    q = _gsr.lib.gsr_mesh_clean_scratch_bytes
    nV, nT = 754, 1504
    assert q(nV, nT) >= 13 * nV + 5 * nT and q(nV, nT) % 256 == 0       # three word arrays and a byte array per vertex, one of each per face
    assert q(nV, nT) < q(nV + 256, nT) and q(nV, nT) < q(nV, nT + 256)
    assert q(0, nT) > 0 and q(nV, 0) > 0 and q(0, 0) > 0
    for bad in ((2 ** 31, nT), (nV, (2 ** 31 + 2) // 3), (2 ** 64 - 1, 1), (1, 2 ** 63), (1, 2 ** 64 - 1)):
        assert q(*bad) == 0, bad
    assert q(2 ** 31 - 1, (2 ** 31 - 1) // 3) > 0


# ------------------------------------------------------------------------------------------------- the refusals
ARGS = {
    "gsr_mesh_clean_count": ("faces", "nV", "nT", "cluster_to_keep", "min_triangles", "tri_label", "tri_size", "scratch", "scratch_bytes", "counts",
                             "stream"),
    "gsr_mesh_clean_emit": ("verts", "vcolor", "faces", "nV", "nT", "scratch", "verts_out", "vcolor_out", "faces_out", "nV_out", "nT_out", "stream"),
}
NV, NT = 754, 1504
A = lambda k: FAKE + (k << 32)          # fake ranges far apart
SCRATCH = "scratch-bytes"               # replaced in the child by gsr_mesh_clean_scratch_bytes(nV, nT) + the case's delta
BASE = {
    "gsr_mesh_clean_count": dict(faces=A(0), nV=NV, nT=NT, cluster_to_keep=1000, min_triangles=50, tri_label=A(1), tri_size=A(2), scratch=A(3),
                                 scratch_bytes=(SCRATCH, 0), counts=A(4), stream=None),
    "gsr_mesh_clean_emit": dict(verts=A(0), vcolor=A(1), faces=A(2), nV=NV, nT=NT, scratch=A(3), verts_out=A(4), vcolor_out=A(5), faces_out=A(6),
                                nV_out=700, nT_out=1400, stream=None),
}
_SIZES = {"nV=2^31": dict(nV=2 ** 31), "3nT=2^31+1": dict(nT=(2 ** 31 + 1) // 3 + 1), "nT=2^63": dict(nT=2 ** 63), "nV=2^64-1": dict(nV=2 ** 64 - 1),
          "3nT-wraps-in-64-bits": dict(nT=(2 ** 64) // 3 + 1)}
REFUSED = {
    "gsr_mesh_clean_count": dict(_SIZES, **{
        "null:faces": dict(faces=None), "null:scratch": dict(scratch=None), "null:counts": dict(counts=None),
        "null:counts-empty-mesh": dict(nT=0, counts=None),
        "misaligned:faces": dict(faces=A(0) + 2), "misaligned:tri_label": dict(tri_label=A(1) + 1), "misaligned:tri_size": dict(tri_size=A(2) + 2),
        "misaligned:scratch": dict(scratch=A(3) + 8), "misaligned:counts": dict(counts=A(4) + 4),
        "scratch-one-byte-short": dict(scratch_bytes=(SCRATCH, -1)), "scratch_bytes=0": dict(scratch_bytes=0),
        "cluster_to_keep=0": dict(cluster_to_keep=0), "cluster_to_keep=0-empty-mesh": dict(cluster_to_keep=0, nV=0),
    }),
    "gsr_mesh_clean_emit": dict(_SIZES, **{
        "null:verts": dict(verts=None), "null:faces": dict(faces=None), "null:scratch": dict(scratch=None), "null:verts_out": dict(verts_out=None),
        "null:faces_out": dict(faces_out=None), "vcolor-without-vcolor_out": dict(vcolor_out=None), "vcolor_out-without-vcolor": dict(vcolor=None),
        "misaligned:verts": dict(verts=A(0) + 2), "misaligned:vcolor": dict(vcolor=A(1) + 1), "misaligned:faces": dict(faces=A(2) + 2),
        "misaligned:scratch": dict(scratch=A(3) + 4), "misaligned:verts_out": dict(verts_out=A(4) + 2), "misaligned:vcolor_out": dict(vcolor_out=A(5) + 2),
        "misaligned:faces_out": dict(faces_out=A(6) + 2),
        "nV_out>nV": dict(nV_out=NV + 1), "nT_out>nT": dict(nT_out=NT + 1), "nV_out>nV-in-front-of-the-no-op": dict(nV_out=NV + 1, nT_out=0),
    }),
}
# calls that must NOT be refused (without a device the launch fails: any code but GSR_E_INVALID)
ACCEPTED = {
    "gsr_mesh_clean_count": {
        "well-formed": {}, "no-labels": dict(tri_label=None, tri_size=None), "labels-only": dict(tri_size=None), "scratch-larger": dict(scratch_bytes=(SCRATCH, 4096)),
        "largest-parameters": dict(cluster_to_keep=2 ** 64 - 1, min_triangles=2 ** 64 - 1), "min_triangles=0": dict(min_triangles=0),
        "largest-sizes": dict(nV=2 ** 31 - 1, nT=(2 ** 31 - 1) // 3, scratch_bytes=2 ** 40),
        "nT=0": dict(nT=0, faces=None, scratch=None, scratch_bytes=0), "nV=0": dict(nV=0, scratch=None, scratch_bytes=0),
    },
    "gsr_mesh_clean_emit": {"well-formed": {}, "no-colour": dict(vcolor=None, vcolor_out=None), "everything-kept": dict(nV_out=NV, nT_out=NT),
                            "largest-sizes": dict(nV=2 ** 31 - 1, nT=(2 ** 31 - 1) // 3)},
}
# nT_out == 0: nothing to write, returns 0 without a launch (every pointer may be NULL)
NOOP = {"gsr_mesh_clean_emit": {"nT_out=0": dict(nV_out=0, nT_out=0),
                                "nT_out=0-null-pointers": dict(nV_out=0, nT_out=0, verts=None, vcolor=None, faces=None, scratch=None, verts_out=None,
                                                               vcolor_out=None, faces_out=None),
                                "nT_out=0-empty-mesh": dict(nV=0, nT=0, nV_out=0, nT_out=0, verts=None, faces=None, verts_out=None, faces_out=None)}}
TABLES = (("accepted", ACCEPTED), ("refused", REFUSED), ("noop", NOOP))


CASES = cabi_child.cases(ENTRIES, TABLES)


def _call(gsr, entry, case):
    args = dict(BASE[entry], **cabi_child.changes(TABLES, entry, case))
    if isinstance(args.get("scratch_bytes"), tuple):
        args["scratch_bytes"] = int(gsr.lib.gsr_mesh_clean_scratch_bytes(args["nV"], args["nT"])) + args["scratch_bytes"][1]
    return getattr(gsr.lib, entry)(*[args[k] for k in ARGS[entry]])


@pytest.fixture(scope="module")
def outcomes(hip_lib_built):
    return cabi_child.run(__file__)


@pytest.mark.parametrize("entry, case, expect", CASES, ids=lambda v: v)
def test_refusal(outcomes, entry, case, expect):
    cabi_child.check(outcomes, entry, case, expect)


if __name__ == "__main__":
    sys.exit(cabi_child.serve([c[:2] for c in CASES], _call))
