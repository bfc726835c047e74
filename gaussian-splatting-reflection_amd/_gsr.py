"""ctypes binding of libgsr_hip.so (C ABI declared in include/gsr_hip.h).

This is the only place the product path touches native code.  There is NO CPU fallback: if the
library is missing or cannot be loaded, importing the rasterizer packages fails loudly.
torch is used for device memory, streams and autograd plumbing only.
"""
import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GSR_LIB") or os.path.join(_HERE, "libgsr_hip.so")   # GSR_LIB: development A/B builds only

c_void_p, c_int, c_float, c_size_t, c_uint32, c_char_p = (ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t,
                                                         ctypes.c_uint32, ctypes.c_char_p)
ALLOC_FN = ctypes.CFUNCTYPE(c_void_p, c_void_p, c_int, c_size_t)

GSR_BUF_GEOM, GSR_BUF_BINNING, GSR_BUF_IMAGE = 0, 1, 2
GSR_PRESENT_CLAMP, GSR_PRESENT_QUANT8 = 1, 2     # presentation flags of gsr_image_metrics
GSR_VIEW_HALF, GSR_VIEW_SOBEL, GSR_VIEW_COLORMAP = 1, 2, 4     # flags of gsr_present_view


class GsrError(RuntimeError):
    pass


class GatherGroup(ctypes.Structure):
    """gsr_gather_group of include/gsr_hip.h."""
    _fields_ = [("src_offset", ctypes.c_uint64), ("dst_offset", ctypes.c_uint64), ("width", c_uint32)]


class DensifyPlan(ctypes.Structure):
    """gsr_densify_plan of include/gsr_hip_densify.h."""
    _fields_ = [("max_grad", c_float), ("min_weight", c_float), ("dense_limit", c_float), ("big_near", c_float), ("big_far", c_float),
                ("extent2", c_float), ("mean", c_float * 3), ("size_prune", c_int), ("N", c_int), ("scale_dims", c_int)]


class AdamSegment(ctypes.Structure):
    """gsr_adam_segment of include/gsr_hip.h."""
    _fields_ = [("begin", ctypes.c_uint64), ("end", ctypes.c_uint64), ("lr", c_float), ("lr2", c_float), ("period", c_uint32),
                ("split", c_uint32)]


GSR_ACT_NONE, GSR_ACT_SIGMOID, GSR_ACT_EXP, GSR_ACT_NORMALIZE4, GSR_ACT_FROZEN = 0, 1, 2, 3, 0x100     # include/gsr_hip_train.h


class ActSegment(ctypes.Structure):
    """gsr_act_segment of include/gsr_hip_train.h."""
    _fields_ = [("begin", ctypes.c_uint64), ("end", ctypes.c_uint64), ("lr", c_float), ("lr2", c_float), ("period", c_uint32),
                ("split", c_uint32), ("kind", c_uint32), ("act_begin", ctypes.c_uint64)]


class ReflForward(ctypes.Structure):
    """gsr_refl_forward of include/gsr_hip.h."""
    _fields_ = [("cam", c_void_p), ("cubemap", c_void_p), ("fail_value", c_void_p), ("L", c_uint32), ("cubemap_rgba", c_void_p),
                ("out_final", c_void_p), ("out_refl_color", c_void_p), ("out_normal_world", c_void_p), ("sort_keys", c_void_p),
                ("scratch", c_void_p), ("scratch_floats", c_size_t), ("async_sort", c_int)]


GSR_ABI_VERSION = 102      # GSR_ABI_VERSION of include/gsr_hip.h this binding was written against


# ------------------------------------------------------------------ the C ABI, once: one group per header and source file, one row per entry
# A group is (header under include/, file under this directory its entries live in, added later?, [(entry, restype, argtypes)]).  The groups
# that are not `later` are ABI 102 as it was frozen: a library that lacks one of their symbols does not load.  A `later` group was added
# under ABI 102 by name, without a version change: it is bound only when its FIRST entry is present, and the Python layer that needs it
# calls require_entry(lib, <that entry>), so a library built before the group keeps serving everything else.  Adding an entry is one row
# here beside its prototype in the header ("Adding an entry under ABI 102"); tests/test_cabi.py holds every row to its header.
P, I, F, U32, U64 = c_void_p, c_int, c_float, c_uint32, ctypes.c_uint64
_SURFEL_FWD = [ALLOC_FN, P, I, I, I, P, I, I, P, P, P, P, P, P, P, F, P, P, P, P, P, F, F, I, P, P, P, P, P, I, P]
_SURFEL_BWD = [I, I, I, I, P, I, I, P, P, P, P, P, F, P, P, P, P, P, F, F, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, I, P]
_GAUSS_BWD = [I, I, I, I, P, I, I, P, P, P, P, P, P, P, F, P, P, P, P, P, F, F, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, I,
              I, P]
_REFL_FWD = [P, P, P, P, P, P, U32, I, I, P, P, P, P]
_REFL_BWD = [P, P, P, P, P, P, U32, I, I, P, P, P, P, P, P, P, P, P, c_size_t, P]
_ADAM = [P, P, P, P, U64, ctypes.POINTER(AdamSegment), I, F, F, F, I, P]
_ROWS_BY_MAP = [P, P, P, U64, ctypes.POINTER(GatherGroup), I, P]

ABI = [
    ("gsr_hip.h", "csrc/gsr_common.hip", False, [
        ("gsr_last_error", c_char_p, None),        # (void): argtypes is left unset, as for gsr_version
        ("gsr_version", I, None),
        ("gsr_set_option", I, [c_char_p, I]),
        ("gsr_profile_enable", I, [I]),
        ("gsr_profile_collect", I, [P, P]),
        ("gsr_mark_visible", I, [I, P, P, P, P, P]),
        ("gsr_debug_fetch", I, [I, c_char_p, I, I, I, I, P, P, P, P, P])]),
    ("gsr_hip.h", "csrc/gsr_surfel.hip", False, [
        ("gsr_surfel_forward", I, _SURFEL_FWD),
        ("gsr_surfel_forward_refl", I, _SURFEL_FWD[:-2] + [ctypes.POINTER(ReflForward), I, P]),
        ("gsr_surfel_forward_eval", I, [ALLOC_FN, P, I, I, I, P, I, I, P, P, P, P, P, P, F, P, P, P, P, P, F, F, I, P, P, P, P, P,
                                        ctypes.POINTER(ReflForward), I, P]),
        ("gsr_surfel_backward", I, _SURFEL_BWD),
        ("gsr_surfel_backward_accum", I, _SURFEL_BWD[:-2] + [I, I, P]),
        ("gsr_surfel_backward_ex", I, _SURFEL_BWD[:-2] + [I, P, I, P])]),
    ("gsr_hip.h", "csrc/gsr_gauss.hip", False, [
        ("gsr_gauss_forward", I, [ALLOC_FN, P, I, I, I, P, I, I, P, P, P, P, P, P, P, F, P, P, P, P, P, F, F, I, P, P, P, P, I, P, I, P]),
        ("gsr_gauss_backward", I, _GAUSS_BWD),
        ("gsr_gauss_backward_accum", I, _GAUSS_BWD[:-2] + [I, I, P])]),
    ("gsr_hip.h", "csrc/gsr_cubemap.hip", False, [
        ("gsr_cubemap_forward", I, [P, P, P, P, U32, U32, U32, U32, U32, P]),
        ("gsr_cubemap_backward", I, [P, P, P, P, P, P, U32, U32, U32, U32, U32, P]),
        ("gsr_deferred_reflection_forward", I, _REFL_FWD),
        ("gsr_deferred_reflection_forward_ex", I, _REFL_FWD[:-1] + [P, P]),
        ("gsr_deferred_reflection_forward_keys", I, _REFL_FWD[:-1] + [P, P, P]),
        ("gsr_deferred_reflection_scratch_floats", c_size_t, [U32, I, I, I]),
        ("gsr_deferred_reflection_backward", I, _REFL_BWD),
        ("gsr_deferred_reflection_backward_accum", I, _REFL_BWD[:-1] + [I, P]),
        ("gsr_deferred_reflection_backward_ex", I, _REFL_BWD[:-1] + [I, I, P, P]),
        ("gsr_deferred_reflection_backward_keys", I, _REFL_BWD[:-1] + [I, I, P, P, I, P]),
        ("gsr_side_join", I, [P]),
        ("gsr_normal_world_forward", I, [P, P, I, I, P, P]),
        ("gsr_normal_world_backward", I, [P, P, I, I, P, P, P])]),
    ("gsr_hip.h", "csrc/gsr_loss.hip", False, [
        ("gsr_ssim_l1_scratch_floats", c_size_t, [I, I, I]),
        ("gsr_ssim_l1_forward", I, [P, P, I, I, I, F, F, P, P, P, P, P, P, P]),
        ("gsr_ssim_l1_backward", I, [P, P, I, I, I, P, P, P, P, P, P])]),
    ("gsr_hip.h", "csrc/gsr_train.hip", False, [
        ("gsr_normal_loss_scratch_floats", c_size_t, []),
        ("gsr_normal_loss_forward", I, [P, P, P, I, I, P, P, P]),
        ("gsr_normal_loss_backward", I, [P, P, P, I, I, P, P, P, P]),
        ("gsr_adam_step", I, _ADAM),
        ("gsr_adam_step_range", I, _ADAM[:-1] + [U64, U64, P])]),
    ("gsr_hip.h", "csrc/gsr_surface.hip", False, [
        ("gsr_surface_forward", I, [P, P, F, I, I, P, P, P]),
        ("gsr_surface_backward", I, [P, P, F, I, I, P, P, P, P, P])]),
    ("gsr_hip.h", "csrc/gsr_densify.hip", False, [
        ("gsr_densification_stats", I, [I, P, P, P, P, P, P, P, P, P]),
        ("gsr_gather_rows", I, _ROWS_BY_MAP),
        ("gsr_split_children", I, [I, I, I, P, P, P, P, P, P, P, P])]),
    # simple_knn refuses to import without these two, while the rasterizers keep working
    ("gsr_hip.h", "csrc/gsr_knn.hip", True, [
        ("gsr_knn_mean_dist", I, [I, P, P, P, c_size_t, P]),
        ("gsr_knn_scratch_bytes", c_size_t, [I])]),
    # the evaluation metrics: utils.image_utils, utils.mae_utils and gsr_eval
    ("gsr_hip.h", "csrc/gsr_metrics.hip", True, [
        ("gsr_image_metrics", I, [P, P, I, I, I, I, P, P, P, P, P, c_size_t, P, P, P]),
        ("gsr_image_metrics_scratch_floats", c_size_t, [I, I, I]),
        ("gsr_normal_mae_scratch_floats", c_size_t, [I, I]),
        ("gsr_normal_mae", I, [P, P, I, I, F, F, F, P, P, c_size_t, P, P])]),
    # the viewer presentation: utils.image_utils
    ("gsr_hip.h", "csrc/gsr_viewer.hip", True, [
        ("gsr_present_view", I, [P, I, I, I, I, P, P, P, P, c_size_t, P]),
        ("gsr_present_view_scratch_floats", c_size_t, [I, I, I, I])]),
    # the composited loss and the SSIM-map gradient: utils.loss_utils
    ("gsr_hip.h", "csrc/gsr_loss.hip", True, [
        ("gsr_photometric_forward", I, [P, P, P, P, P, I, I, I, F, F, P, P, P, P, P, P]),
        ("gsr_photometric_scratch_floats", c_size_t, [I, I, I]),
        ("gsr_photometric_backward", I, [P, P, P, P, P, I, I, I, P, P, P, P, P, P, P]),
        ("gsr_ssim_map_backward", I, [P, P, I, I, I, P, P, P, P, P, P])]),
    # the raw-parameter step: gsr_train.RawTrainState
    ("gsr_hip_train.h", "csrc/gsr_train.hip", True, [
        ("gsr_adam_act_step", I, [P, P, P, P, P, U64, U64, ctypes.POINTER(ActSegment), I, F, F, F, I, U64, U64, P]),
        ("gsr_activate", I, [P, P, U64, U64, ctypes.POINTER(ActSegment), I, P])]),
    # the env-scope masks and the reflection-mask loss: utils.loss_utils.env_scope_masks, refl_scope_loss
    ("gsr_hip_scope.h", "csrc/gsr_scope.hip", True, [
        ("gsr_env_scope_forward", I, [I, P, P, F, F, F, F, P, P, P, P, P]),
        ("gsr_env_scope_scratch_floats", c_size_t, []),
        ("gsr_env_scope_backward", I, [I, P, P, P, P, I, P])]),
    # the environment map's bicubic resize and its sharpening in sigmoid space: gsr_envmap
    ("gsr_hip_envmap.h", "csrc/gsr_envmap.hip", True, [
        ("gsr_envmap_resize", I, [P, P, I, I, I, P]),
        ("gsr_envmap_sharpen", I, [P, P, I, I, F, F, F, P])]),
    # the densification plan on the device, prune_points, the scatter of the split children: gsr_densify
    ("gsr_hip_densify.h", "csrc/gsr_densify.hip", True, [
        ("gsr_densify_plan_select", I, [I, ctypes.POINTER(DensifyPlan), P, P, P, P, P, P, c_size_t, P, P, P]),
        ("gsr_densify_plan_scratch_bytes", c_size_t, [I, I]),
        ("gsr_densify_plan_rows", I, [I, ctypes.POINTER(DensifyPlan), P, c_size_t, P, P, P, P, P, I, P, P, P, P, P]),
        ("gsr_prune_rows", I, [I, P, P, c_size_t, P, P, P]),
        ("gsr_scatter_rows", I, _ROWS_BY_MAP)]),
    # add_densification_stats under the reference's boolean filter: scene.GaussianModel (one commit younger than the five above)
    ("gsr_hip_densify.h", "csrc/gsr_densify.hip", True, [
        ("gsr_densification_stats_filter", I, [I, P, P, P, P, P, P, P, P])]),
    # TSDF fusion of rendered depth maps and the iso-surface as an indexed mesh: gsr_mesh, utils.mesh_utils
    ("gsr_hip_mesh.h", "csrc/gsr_mesh.hip", True, [
        ("gsr_tsdf_integrate", I, [P, P, P, I, I, I, F, F, F, F, P, P, P, F, I, I, P, P, F, F, P]),
        ("gsr_mesh_scratch_bytes", c_size_t, [I, I, I]),
        ("gsr_mesh_count", I, [P, P, I, I, I, F, P, c_size_t, P, P]),
        ("gsr_mesh_emit", I, [P, P, P, I, I, I, F, F, F, F, F, P, P, P, P, U64, U64, P])]),
    # connected-component clean-up of an indexed mesh: gsr_mesh.clean_mesh, utils.mesh_utils.post_process_mesh
    ("gsr_hip_meshclean.h", "csrc/gsr_meshclean.hip", True, [
        ("gsr_mesh_clean_count", I, [P, U64, U64, U64, U64, P, P, P, c_size_t, P, P]),
        ("gsr_mesh_clean_scratch_bytes", c_size_t, [U64, U64]),
        ("gsr_mesh_clean_emit", I, [P, P, P, U64, U64, P, P, P, P, U64, U64, P])]),
    # TSDF fusion on a lattice in contracted space, per-vertex colours, un-contraction: gsr_mesh.ContractedTSDFVolume, color_vertices
    ("gsr_hip_unbounded.h", "csrc/gsr_unbounded.hip", True, [
        ("gsr_tsdf_integrate_contracted", I, [P, P, I, F, F, F, F, F, F, F, P, I, I, P, P, P]),
        ("gsr_points_fuse_view", I, [P, U64, P, P, P, P, I, I, P, P, F, P]),
        ("gsr_uncontract_points", I, [P, P, U64, F, F, F, F, F, P])]),
    # the block-sparse TSDF volume: gsr_mesh.SparseTSDFVolume, utils.mesh_utils extract_mesh_bounded(sparse=True)
    ("gsr_hip_sparse.h", "csrc/gsr_sparse.hip", True, [
        ("gsr_sparse_tsdf_touch", I, [P, I, I, I, F, F, F, F, P, P, F, I, I, P, P, F, F, P]),
        ("gsr_sparse_tsdf_allocate_scratch_bytes", c_size_t, [I, I, I]),
        ("gsr_sparse_tsdf_allocate", I, [P, I, I, I, P, U64, P, P, c_size_t, P]),
        ("gsr_sparse_tsdf_integrate", I, [P, U64, U64, P, P, P, I, I, I, F, F, F, F, P, P, P, F, I, I, P, P, F, F, P]),
        ("gsr_sparse_mesh_scratch_bytes", c_size_t, [U64]),
        ("gsr_sparse_mesh_count", I, [P, P, U64, U64, P, P, I, I, I, F, P, c_size_t, P, P]),
        ("gsr_sparse_mesh_emit", I, [P, P, U64, U64, P, P, P, I, I, I, F, F, F, F, F, P, P, P, P, U64, U64, P])]),
]

ENTRIES_BY_HEADER = {}          # {header file name: [entry names]}, what tests/test_cabi.py holds each header to
for _header, _, _, _rows in ABI:
    ENTRIES_BY_HEADER.setdefault(_header, []).extend(name for name, _, _ in _rows)
EXPORTED = ENTRIES_BY_HEADER["gsr_hip.h"]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension has not been built. Run "
            f"`python {os.path.join(_HERE, 'csrc', 'build.py')}` (hipcc, gfx950). There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    lib.gsr_version.restype = c_int
    if lib.gsr_version() != GSR_ABI_VERSION:
        # an entry point never changes its signature, but a library built from another header may lack (or, once, have changed) symbols
        # this binding calls: refuse it instead of passing shifted arguments
        raise ImportError(f"{LIB_PATH} reports ABI version {lib.gsr_version()}, this binding was written against {GSR_ABI_VERSION} "
                          f"(include/gsr_hip.h): rebuild with `python {os.path.join(_HERE, 'csrc', 'build.py')} --force`")
    for _, _, later, rows in ABI:
        if later and not hasattr(lib, rows[0][0]):
            continue
        for name, restype, argtypes in rows:
            fn = getattr(lib, name)         # (an AttributeError names the symbol a frozen group lacks)
            fn.restype = restype
            if argtypes is not None:
                fn.argtypes = argtypes
    return lib


lib = _load()


def require_entry(library, name):
    """The check in front of an entry of a `later` group of ABI: `library` is the calling module's `lib` (a module that cannot work without
    the group calls this at import, with the group's first entry)."""
    if not hasattr(library, name):
        source_file = next(source for _, source, _, rows in ABI if any(name == row[0] for row in rows))
        raise ImportError(f"{LIB_PATH} does not export {name} ({source_file}): it was built before that entry was added; "
                          f"rebuild with `python {os.path.join(_HERE, 'csrc', 'build.py')} --force`.  There is no torch fallback.")


def compiled_binding():
    """The optional compiled torch/pybind binding (csrc/gsr_torch_binding.cpp -> _gsr_C.so): marshaling in C++ over the same C
    ABI, about half the host cost per call of the ctypes path (tests/host_overhead.py at C1: 25 vs 49 us per backward).
    GSR_BINDING=pybind requires it (an error if it is not built), GSR_BINDING=ctypes never uses it; unset: used when present and
    loadable (it is built against the running torch; both bindings drive the same HIP library, so this choice is not a
    fallback away from native code)."""
    want = os.environ.get("GSR_BINDING", "auto")
    if want == "ctypes":
        return None
    import importlib.util
    path = os.path.join(_HERE, "_gsr_C.so")
    if not os.path.exists(path):
        if want == "pybind":
            raise ImportError(f"GSR_BINDING=pybind but {path} is not built: run `python {os.path.join(_HERE, 'csrc', 'build.py')} --binding`")
        return None
    try:
        spec = importlib.util.spec_from_file_location("_gsr_C", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    except Exception:
        if want == "pybind":
            raise
        return None


PYBIND = compiled_binding()

STAGES = ["preprocess", "scan_readback", "emit_keys", "sort", "tile_ranges", "render_fwd", "render_bwd", "preprocess_bwd", "refl_fwd",
          "refl_bwd", "cubemap_fwd", "cubemap_bwd", "loss_fwd", "loss_bwd", "adam", "surface_fwd", "surface_bwd", "refl_bwd_tail"]


def set_option(name, value):
    check(lib.gsr_set_option(name.encode(), int(value)), f"gsr_set_option({name})")


_side_held = {}          # device index -> [(tensor the side stream of THAT device still reads or writes, stream it was allocated / last used on)]
_side_held_mu = threading.Lock()     # two host threads: an entry appended to a list another thread's side_join() has just popped would be dropped unjoined


def side_hold(*tensors):
    """Keeps device tensors alive that work on the library's side stream still reads (see side_join), and remembers the stream that is
    current now — the one the caching allocator will hand their blocks back to."""
    entries = []
    for t in tensors:
        if t is None:
            continue
        dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
        entries.append((dev, (t, torch.cuda.current_stream(t.device).cuda_stream)))
    with _side_held_mu:
        for dev, entry in entries:
            _side_held.setdefault(dev, []).append(entry)


def side_join(device=None):
    """Makes the current stream of `device` wait for everything the library has put on its side stream (the texel-gradient tail
    of deferred_reflection(..., async_tail=True)), then lets go of the scratch tensors held for it.  No host synchronisation.
    Call before anything reads the cubemap / fail-value gradient sink: gsr_dist.FlatGrads and gsr_train.FlatAdam do."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    # always ask the library (a stream-wait on an event that has completed, or was never recorded, costs nothing): a second
    # consumer stream must be ordered behind the tail too, and another device's held tensors are none of this call's business
    with _side_held_mu:
        held = _side_held.pop(dev.index, [])
    with torch.cuda.device(dev):
        cur = torch.cuda.current_stream(dev).cuda_stream
        check(lib.gsr_side_join(cur), "gsr_side_join")
        # The held tensors go back to the caching allocator, which re-issues a block to work on the stream it was ALLOCATED on — not
        # necessarily the stream joining here (an all-reduce or optimizer stream, bench.py --view-streams).  Every such stream is ordered
        # behind the tail as well, so whatever reuses the memory cannot run while the tail still reads or writes it.
        for s in {s for _, s in held if s != cur}:
            check(lib.gsr_side_join(s), "gsr_side_join")
    del held


def profile_enable(on=True):
    lib.gsr_profile_enable(1 if on else 0)


def profile_collect():
    """Returns {stage: (total_ms, launches)} measured with hipEvents on the launch stream since the last call."""
    ms = (ctypes.c_float * len(STAGES))()
    n = (ctypes.c_int * len(STAGES))()
    lib.gsr_profile_collect(ctypes.cast(ms, c_void_p), ctypes.cast(n, c_void_p))
    return {STAGES[i]: (float(ms[i]), int(n[i])) for i in range(len(STAGES))}


def check(rc, what):
    if rc < 0:
        msg = lib.gsr_last_error()
        raise GsrError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")
    return rc


def ptr(t):
    """Device pointer of a tensor, or NULL for None / empty tensors (the reference passes
    `.contiguous().data<float>()`, which is nullptr for empty tensors, and tests `== nullptr`)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


def stream_ptr(device):
    return torch.cuda.current_stream(device).cuda_stream


def require_cuda(t, name):
    # CHECK_INPUT of DSR rasterize_points.cu:27-28
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")


def f32c(t, name, aligned=False):
    """Contiguous float32 view (reference: `.contiguous().data<float>()` throws on other dtypes).  aligned: on a 16-byte boundary as well —
    a contiguous view at an odd offset of a packed buffer (the SH coefficients of one flat parameter buffer) is copied, where the library
    would refuse it (include/gsr_hip.h, "alignment")."""
    if t.numel() and t.dtype != torch.float32:
        raise RuntimeError(f"expected scalar type Float but found {t.dtype} for {name}")
    t = t.contiguous()
    if aligned and t.numel() and t.data_ptr() % 16:
        t = t.clone()
    return t


# ------------------------------------------------------------------ what the two rasterizer bindings share
# (diff_gaussian_rasterization._C and diff_surfel_rasterization._C, over their ctypes paths)

def sh_coeffs(sh, empty_scene_counts=True):
    """M, the SH coefficients per Gaussian: an omitted input is a 1-D empty placeholder, an empty scene's shs are (0, M, 3).  Variant S takes
    M from the shape; variant G (empty_scene_counts=False) takes 0 for any empty sh, as the reference's RasterizeGaussiansCUDA does, so its
    dL_dsh of an empty scene is (0, 0, 3).  (The compiled binding, gsr_torch_binding.cpp, takes M = 0 for any empty sh in both variants; the
    two differ only at P = 0, where the library reads nothing and autograd drops the empty gradient, and gradient sinks always take ctypes.)"""
    if empty_scene_counts:
        return sh.size(1) if sh.dim() > 1 else 0
    return sh.size(1) if sh.numel() != 0 else 0


def check_backward_keywords(grad_sink, accumulate, unused, sinkable, M, unused_needs, unused_message):
    """The keyword-only extensions of both `rasterize_gaussians_backward`: `grad_sink` names come from `sinkable`; `accumulate` needs a sink
    for every one of them (minus shs without SH input): the kernel has ONE accumulate switch for all parameter gradients, and fresh
    (uninitialised) tensors cannot be added to; `unused_needs` maps each name `unused` may hold to whether the input that makes that
    gradient unused was supplied.  Returns `unused` as a frozenset."""
    if grad_sink:
        unknown = set(grad_sink) - sinkable
        if unknown:
            raise ValueError(f"grad sink: unknown gradient name(s) {sorted(unknown)}; expected a subset of {sorted(sinkable)}")
    if accumulate and (not grad_sink or not set(grad_sink) >= (sinkable - ({"shs"} if M == 0 else set()))):
        raise ValueError("accumulate=True needs a sink for every parameter gradient: " + ", ".join(sorted(sinkable)))
    unused = frozenset(unused)
    if unused - set(unused_needs) or not all(unused_needs[name] for name in unused):
        raise ValueError(unused_message % (sorted(unused),))
    return unused


def check_sink_tensor(prefix, name, t, shape, dev, aligned):
    """The check of a caller-owned gradient tensor a backward kernel writes into: contiguous float32 of `shape` on `dev`, and with `aligned`,
    storage that starts on a 16-byte boundary.  The ValueError's text opens with "<prefix> '<name>':"."""
    if tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
        raise ValueError(f"{prefix} '{name}': expected contiguous float32 {tuple(shape)} on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}")
    if aligned and t.data_ptr() % 16:
        # the kernel stores dL_dsh / dL_drot rows as float4 (include/gsr_hip.h, "alignment"); the C ABI refuses too
        raise ValueError(f"{prefix} '{name}': storage must be 16-byte aligned (got {t.data_ptr():#x}); pad the slices of a packed buffer "
                         "to multiples of 4 floats as gsr_dist.FlatGrads does")


def grad_allocator(grad_sink, dev, mk0):
    """mk(shape, sink_name=None, **kw) for the outputs of a backward: the caller-owned tensor `grad_sink[sink_name]` where there is one (the
    kernel then writes that gradient straight into it), checked for shape, dtype, device and alignment; otherwise mk0(shape, **kw)."""
    def mk(shape, sink_name=None, **kw):
        t = grad_sink.get(sink_name) if (grad_sink and sink_name is not None) else None
        if t is None:
            return mk0(shape, **kw)
        check_sink_tensor("grad sink", sink_name, t, shape, dev, aligned=True)
        return t
    return mk


def mark_visible(means3D, viewmatrix, projmatrix):
    """`_C.mark_visible` of both variants (markVisible of the references' rasterize_points.cu)."""
    if PYBIND is not None:
        return PYBIND.mark_visible(means3D, viewmatrix, projmatrix)
    P = means3D.size(0)
    m3, vm, pm = f32c(means3D, "means3D"), f32c(viewmatrix, "viewmatrix"), f32c(projmatrix, "projmatrix")     # dtype checks in front of the allocation
    present = torch.zeros((P,), dtype=torch.bool, device=means3D.device)
    if P != 0:
        with torch.cuda.device(means3D.device):
            check(lib.gsr_mark_visible(P, ptr(m3), ptr(vm), ptr(pm), ptr(present), stream_ptr(means3D.device)), "gsr_mark_visible")
    return present


class Workspace:
    """The three opaque byte buffers of one forward call (geomBuffer, binningBuffer, imgBuffer of
    DSR rasterize_points.cu:102-108), allocated by torch when the library asks for them."""

    def __init__(self, device):
        self.device = device
        self.bufs = [torch.empty(0, dtype=torch.uint8, device=device) for _ in range(3)]
        self.error = None

        def _alloc(user, which, nbytes):
            try:
                t = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.device)
                self.bufs[which] = t
                return t.data_ptr()
            except Exception as e:  # surfaced as GSR_E_ALLOC by the library
                self.error = e
                return 0

        self.cb = ALLOC_FN(_alloc)

    def check(self, rc, what):
        """check() for the forward call that was given this workspace's callback.  An exception the allocation raised (the caching
        allocator's torch.OutOfMemoryError) comes first: the library answers the NULL it got with GSR_E_ALLOC, and the caller — a training
        loop that catches the allocator's exception, as it can with the reference's resize callback — gets that very object, the library's
        message as its context.  A GSR_E_ALLOC the callback did not cause is a GsrError like every other failure."""
        if self.error is None:
            return check(rc, what)
        err, self.error = self.error, None      # (the exception's traceback holds this object through _alloc's frame: do not keep it in turn)
        try:
            check(rc, what)
        except GsrError as lib_err:
            raise err from lib_err
        raise err


def debug_fetch(variant, name, P, R, W, H, geom, binning, img, dtype, shape):
    """Parity-test helper: copy a named workspace array out (see gsr_debug_fetch in gsr_hip.h)."""
    out = torch.empty(shape, dtype=dtype, device=geom.device)
    check(lib.gsr_debug_fetch(variant, name.encode(), P, R, W, H, ptr(geom), ptr(binning), ptr(img), ptr(out) if out.numel() else None,
                              stream_ptr(geom.device)), f"gsr_debug_fetch({name})")
    return out
