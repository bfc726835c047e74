"""What include/gsr_hip.h says about every argument of every exported entry, as a table, and the calls that follow from it.

One Row per entry that takes a pointer or a size.  A row is a WELL-FORMED call (device pointers are a fake aligned address that is never
dereferenced, what the entry reads on the host is real host memory) whose arguments carry their status:

    R   required pointer                      -> case "null:<name>"
    O   optional pointer (given or not)       -> no case of its own; its condition is an explicit Case of the row
    N   signed size, smallest valid value     -> "neg:<name>", and "zero:<name>" unless zero is valid or a documented no-op
    U   unsigned size                         -> "zero:<name>" where zero is refused
    V   plain value (degree, flags, switches) -> explicit Cases
    aligned=k on a pointer                    -> "misaligned:<name>" (offset by 4 bytes)

and the explicit Cases hold the either/or groups, the "needs its partner" pairs, the SH degree / coefficient count and each entry's own
limits.  Every case must be refused with GSR_E_INVALID, a message that names the entry (or its family: the _accum, _ex, _keys and _refl
forms report under their base name) and no call of the allocation callback; the untouched row must NOT be refused.

tests/test_cabi_refusals.py makes the calls in a child process (tests/cabi_child.py) that hides every GPU (HIDE_GPUS), asks the HIP runtime
for the device count (_visible_devices), and only with none visible goes on — a missing check plus a fake pointer must never reach a device."""
import ctypes

FAKE = 0x7f0000000000        # 256-byte aligned, never touched
GSR_E_INVALID = -1


class Arg:
    def __init__(self, kind, name, value, **kw):
        self.kind, self.name, self.value = kind, name, value
        self.aligned = kw.get("aligned", 0)
        self.min = kw.get("min", 1)
        self.zero = kw.get("zero", "invalid")       # "invalid", "valid" or "noop"


def R(name, aligned=0): return Arg("req", name, FAKE, aligned=aligned)
def O(name, given=False, aligned=0): return Arg("opt", name, FAKE if given else None, aligned=aligned)
def N(name, value, min=1, zero="invalid"): return Arg("size", name, value, min=min, zero=zero if min > 0 else "valid")
def U(name, value, zero="invalid"): return Arg("usize", name, value, zero=zero)
def V(name, value): return Arg("val", name, value)
def H(name, make): return Arg("host", name, make)             # required pointer to host memory: make(ctx) builds it


ALLOC = Arg("alloc", "alloc", None)
USER = Arg("val", "alloc_user", None)
STREAM = Arg("val", "stream", None)


class Case:
    """One bad call: the row with `changes` ({argument name: value, or a function of the child's context that builds one})."""
    def __init__(self, id, why="", **changes):
        self.id, self.why, self.changes, self.ok = id, why, changes, False


def Ok(id, **changes):
    """A second well-formed call of a row (another branch of its checks): it must NOT be refused."""
    c = Case("well-formed:" + id, **changes)
    c.ok = True
    return c


class Row:
    def __init__(self, entry, args, cases=(), family=None, query=False, note=""):
        self.entry, self.args, self.family, self.query, self.note = entry, args, family or entry, query, note
        self.cases = self._generated() + list(cases)
        ids = [c.id for c in self.cases]
        assert len(ids) == len(set(ids)), (entry, ids)

    def _generated(self):
        out = []
        for a in self.args:
            if a.kind == "alloc":
                out.append(Case("null:alloc", alloc="NULL"))
            elif a.kind in ("req", "host"):
                out.append(Case(f"null:{a.name}", **{a.name: None}))
            elif a.kind == "size":
                out.append(Case(f"neg:{a.name}", **{a.name: -1}))
                if a.min > 0 and a.zero == "invalid":
                    out.append(Case(f"zero:{a.name}", **{a.name: 0}))
            elif a.kind == "usize" and a.zero == "invalid":
                out.append(Case(f"zero:{a.name}", **{a.name: 0}))
            if a.aligned and a.value is not None:
                out.append(Case(f"misaligned:{a.name}", **{a.name: FAKE + 4}))
        return out


# Entries without a row: they take neither a pointer nor a size.
NO_ARGUMENTS = {"gsr_last_error": "no argument", "gsr_version": "no argument", "gsr_normal_loss_scratch_floats": "no argument",
                "gsr_profile_enable": "one switch, every value is valid"}

# ---------------------------------------------------------------------------------------------------------------- the rasterizers
P0, W0, H0, L0 = 100, 64, 48, 16


def _refl(**kw):
    """A reflection descriptor (gsr_refl_forward) as a function of the child's context."""
    def make(ctx):
        d = dict(cam=FAKE, cubemap=FAKE, fail_value=FAKE, L=L0, cubemap_rgba=FAKE, out_final=FAKE, out_refl_color=FAKE, out_normal_world=FAKE,
                 sort_keys=None, scratch=None, scratch_floats=0, async_sort=0)
        d.update({k: (v(ctx) if callable(v) else v) for k, v in kw.items()})
        return ctx.keep(ctx.gsr.ReflForward(*d.values()))
    return make


def _sorted_floats(delta=0):
    return lambda ctx: int(ctx.gsr.lib.gsr_deferred_reflection_scratch_floats(L0, W0, H0, 1)) + delta


_SORTING = dict(sort_keys=FAKE, scratch=FAKE, scratch_floats=_sorted_floats(), async_sort=1)

_SH_CASES = [Case("sh:D<0", D=-1), Case("sh:D>3", D=4), Case("sh:(D+1)^2>M", "an SH row read past its end", D=3, M=4)]
_SCENE_CASES_S = [Case("either:shs|colors_precomp", shs=None, colors_precomp=None),
                  Case("either:scales+rotations|transMat_precomp", scales=None, rotations=None, transMat_precomp=None),
                  Case("partner:scales-without-rotations", rotations=None), Case("partner:rotations-without-scales", scales=None)] + _SH_CASES
_REFL_FIELDS = ("cam", "cubemap", "fail_value", "cubemap_rgba", "out_final", "out_refl_color", "out_normal_world")
_REFL_CASES = [Case(f"refl:null:{f}", refl=_refl(**{f: None})) for f in _REFL_FIELDS] + [
    Case("refl:L=0", refl=_refl(L=0)), Case("refl:6L^2>=2^32", refl=_refl(L=30000)),
    Case("refl:misaligned:cubemap_rgba", refl=_refl(cubemap_rgba=FAKE + 4))]


def _surfel_forward(entry, refl_arg=False, **kw):
    a = [ALLOC, USER, N("P", P0, min=0), V("D", 3), V("M", 16), R("background"), N("width", W0), N("height", H0), R("means3D"), O("env_scope_mask", True),
         O("shs", True, aligned=16), O("colors_precomp"), R("refl_strengths"), R("opacities"), O("scales", True), V("scale_modifier", 1.0),
         O("rotations", True), O("transMat_precomp"), R("viewmatrix"), R("projmatrix"), R("cam_pos"), V("tan_fovx", 0.5), V("tan_fovy", 0.5),
         V("prefiltered", 0), R("out_color"), R("out_others"), R("out_refl_strength_map"), R("radii"), R("gaussian_weights")]
    if refl_arg:
        a.append(O("refl"))
    return Row(entry, a + [V("debug", 0), STREAM], **kw)


def _surfel_backward(entry, extra, **kw):
    a = [N("P", P0, min=0), V("D", 3), V("M", 16), N("R", 10, min=0), R("background"), N("width", W0), N("height", H0), R("means3D"),
         O("shs", True, aligned=16), O("colors_precomp"), R("refl_strengths"), O("scales", True), V("scale_modifier", 1.0), O("rotations", True),
         O("transMat_precomp"), R("viewmatrix"), R("projmatrix"), R("cam_pos"), V("tan_fovx", 0.5), V("tan_fovy", 0.5), R("radii"),
         R("geom_buffer"), R("binning_buffer"), R("image_buffer"), R("dL_dpix"), R("dL_dothers"), R("dL_drefl_strength_map"), R("dL_dmean2D"),
         O("dL_dnormal"), R("dL_dopacity"), O("dL_dcolor"), R("dL_drefl_strengths"), R("dL_dmean3D"), O("dL_dtransMat"),
         O("dL_dsh", True, aligned=16), R("dL_dscale"), R("dL_drot", aligned=16)]
    cases = _SCENE_CASES_S + [
        Case("needs:dL_dsh-with-shs", dL_dsh=None),
        Case("needs:dL_dcolor-without-shs", shs=None, colors_precomp=FAKE, dL_dsh=None, dL_dcolor=None),
        Case("needs:dL_dtransMat-without-scales", scales=None, rotations=None, transMat_precomp=FAKE, dL_dtransMat=None)]
    return Row(entry, a + extra + [V("debug", 0), STREAM], cases, family="gsr_surfel_backward", **kw)


def _gauss_scene():
    return [R("means3D"), O("shs", True, aligned=16), O("colors_precomp"), R("normals"), R("refl_strengths"), R("opacities"), O("scales", True),
            V("scale_modifier", 1.0), O("rotations", True), O("cov3D_precomp"), R("viewmatrix"), R("projmatrix"), R("cam_pos"), V("tan_fovx", 0.5),
            V("tan_fovy", 0.5)]


_SCENE_CASES_G = [Case("either:shs|colors_precomp", shs=None, colors_precomp=None),
                  Case("either:scales+rotations|cov3D_precomp", scales=None, rotations=None, cov3D_precomp=None),
                  Case("partner:scales-without-rotations", rotations=None), Case("partner:rotations-without-scales", scales=None)] + _SH_CASES


def _gauss_backward(entry, extra):
    a = [N("P", P0, min=0), V("D", 3), V("M", 16), N("R", 10, min=0), R("background"), N("width", W0), N("height", H0)] + _gauss_scene() + [
        R("radii"), R("geom_buffer"), R("binning_buffer"), R("image_buffer"), R("dL_dpix"), R("dL_dnormal_map"), R("dL_drefl_strength_map"),
        O("dL_invdepths"), O("dL_dmean2D"), R("dL_dmean2D_pixels"), O("dL_dconic", True, aligned=16), R("dL_dopacity"), O("dL_dcolor"),
        R("dL_dnormals"), R("dL_drefl_strengths"), O("dL_dinvdepth"), R("dL_dmean3D"), O("dL_dcov3D"), O("dL_dsh", True, aligned=16),
        R("dL_dscale"), R("dL_drot", aligned=16), V("antialiasing", 0)]
    cases = _SCENE_CASES_G + [
        Case("needs:dL_dsh-with-shs", dL_dsh=None),
        Case("needs:dL_dcolor-without-shs", shs=None, colors_precomp=FAKE, dL_dsh=None, dL_dcolor=None),
        Case("needs:dL_dcov3D-without-scales", scales=None, rotations=None, cov3D_precomp=FAKE, dL_dcov3D=None),
        Case("needs:dL_dinvdepth-with-dL_invdepths", dL_invdepths=FAKE)]
    return Row(entry, a + extra + [V("debug", 0), STREAM], cases, family="gsr_gauss_backward")


_TRAIN_REFL_CASES = _REFL_CASES + [
    Ok("refl", refl=_refl()), Ok("refl+early-sort", refl=_refl(**_SORTING)),
    Case("refl:partner:scratch-without-sort_keys", refl=_refl(scratch=FAKE, scratch_floats=_sorted_floats())),
    Case("refl:scratch-one-float-short", "judged before the first allocation, not after the last kernel",
         refl=_refl(**dict(_SORTING, scratch_floats=_sorted_floats(-1)))),
    Case("refl:misaligned:scratch", "32-byte aligned", refl=_refl(**dict(_SORTING, scratch=FAKE + 4)))]

RASTER = [
    _surfel_forward("gsr_surfel_forward", cases=_SCENE_CASES_S, note="P = 0 is an empty scene: zero planes, returns 0"),
    _surfel_forward("gsr_surfel_forward_refl", refl_arg=True, cases=_SCENE_CASES_S + _TRAIN_REFL_CASES, family="gsr_surfel_forward"),
    Row("gsr_surfel_forward_eval",
        [ALLOC, USER, N("P", P0, min=0), V("D", 3), V("M", 16), R("background"), N("width", W0), N("height", H0), R("means3D"),
         O("shs", True, aligned=16), O("colors_precomp"), R("refl_strengths"), R("opacities"), O("scales", True), V("scale_modifier", 1.0),
         O("rotations", True), O("transMat_precomp"), R("viewmatrix"), R("projmatrix"), R("cam_pos"), V("tan_fovx", 0.5), V("tan_fovy", 0.5),
         V("prefiltered", 0), R("out_color"), R("out_alpha"), O("out_normal_view", True), R("out_refl_strength_map"), R("radii"), O("refl"),
         V("debug", 0), STREAM],
        _SCENE_CASES_S + _REFL_CASES + [
            Ok("refl-without-out_normal_view", out_normal_view=None, refl=_refl()),
            Case("needs:out_normal_view-without-refl", out_normal_view=None),
            Case("refl:sort_keys", "there is no backward to hand them to", out_normal_view=None, refl=_refl(sort_keys=FAKE)),
            Case("refl:scratch", refl=_refl(scratch=FAKE, scratch_floats=1024))]),
    _surfel_backward("gsr_surfel_backward", []),
    _surfel_backward("gsr_surfel_backward_accum", [V("accumulate", 1)]),
    _surfel_backward("gsr_surfel_backward_ex", [V("accumulate", 0), O("dL_dnormal_extra", True)]),
    Row("gsr_gauss_forward",
        [ALLOC, USER, N("P", P0, min=0), V("D", 3), V("M", 16), R("background"), N("width", W0), N("height", H0)] + _gauss_scene() + [
            V("prefiltered", 0), R("out_color"), R("out_normal_map"), R("out_refl_strength_map"), O("out_invdepth", True), V("antialiasing", 1),
            R("radii"), V("debug", 0), STREAM], _SCENE_CASES_G),
    _gauss_backward("gsr_gauss_backward", []),
    _gauss_backward("gsr_gauss_backward_accum", [V("accumulate", 1)]),
    Row("gsr_mark_visible", [N("P", P0, min=0), R("means3D"), R("viewmatrix"), O("projmatrix", True), R("present"), STREAM],
        note="projmatrix is not read (the test is on view-space depth alone): NULL is accepted"),
    Row("gsr_debug_fetch",
        [V("variant", 0), V("name", b"depths"), N("P", P0, min=0), N("R", 10, min=0), N("width", W0), N("height", H0), R("geom_buffer"),
         O("binning_buffer", True), O("image_buffer", True), R("dst"), STREAM],
        [Case("variant=2", variant=2), Case("null:name", name=None), Case("unknown-name", name=b"no-such-array"),
         Case("needs:binning_buffer-for-point_list", name=b"point_list", binning_buffer=None),
         Case("needs:image_buffer-for-ranges", name=b"ranges", image_buffer=None),
         Case("needs:geom_buffer-for-keys", name=b"keys", geom_buffer=None)],
        note="a buffer is required exactly when the named array lives in it and the call copies something out of it"),
]

# ---------------------------------------------------------------------------------------------------------------- cubemap, reflection
_ATOMIC_FLOATS = (6 * L0 * L0 + 1) * 4


def _refl_forward(entry, extra):
    a = [R("normal_view"), R("base_color"), R("refl_strength"), R("cam"), R("cubemap"), R("fail_value"), U("L", L0), N("width", W0), N("height", H0),
         R("out_final"), R("out_refl_color"), R("out_normal_world")]
    return Row(entry, a + extra + [STREAM], [Case("6L^2>=2^32", "texel ids and sort keys are 32-bit", L=30000)], family="gsr_deferred_reflection_forward")


def _refl_backward(entry, extra, cases=()):
    a = [R("normal_view"), R("base_color"), R("refl_strength"), R("cam"), R("cubemap"), R("fail_value"), U("L", L0), N("width", W0), N("height", H0),
         R("g_final"), O("g_refl_color"), O("g_normal_world", True), R("g_normal_view"), R("g_base"), R("g_strength"), R("g_cubemap"), R("g_fail"),
         R("scratch", aligned=16), V("scratch_floats", _ATOMIC_FLOATS)]
    return Row(entry, a + extra + [STREAM], [Case("6L^2>=2^32", L=30000, scratch_floats=1 << 40),
                                             Case("scratch-one-float-short", scratch_floats=_ATOMIC_FLOATS - 1)] + list(cases),
               family="gsr_deferred_reflection_backward")


REFLECTION = [
    Row("gsr_cubemap_forward", [R("inputs"), R("cubemap"), R("fail_value"), R("outputs"), V("interp", 1), V("seamless", 1), U("B", 1000, zero="noop"),
                                U("C", 3), U("L", L0), STREAM]),
    Row("gsr_cubemap_backward", [R("grad_outputs"), R("inputs"), R("cubemap"), R("grad_cubemap"), R("grad_inputs"), R("grad_fail"), V("interp", 1),
                                 V("seamless", 1), U("B", 1000, zero="noop"), U("C", 3), U("L", L0), STREAM]),
    _refl_forward("gsr_deferred_reflection_forward", []),
    _refl_forward("gsr_deferred_reflection_forward_ex", [O("cubemap_rgba", True, aligned=16)]),
    _refl_forward("gsr_deferred_reflection_forward_keys", [O("cubemap_rgba", True, aligned=16), O("sort_keys", True)]),
    Row("gsr_deferred_reflection_scratch_floats", [U("L", L0), N("width", W0), N("height", H0), V("binned", 1)], query=True),
    _refl_backward("gsr_deferred_reflection_backward", []),
    _refl_backward("gsr_deferred_reflection_backward_accum", [V("accumulate", 1)]),
    _refl_backward("gsr_deferred_reflection_backward_ex", [V("accumulate", 0), V("async_tail", 0), O("cubemap_rgba", True, aligned=16)]),
    _refl_backward("gsr_deferred_reflection_backward_keys",
                   [V("accumulate", 0), V("async_tail", 0), O("cubemap_rgba", True, aligned=16), O("sort_keys", True), V("keys_sorted", 0)],
                   [Ok("sorted-path", scratch_floats=_sorted_floats(), keys_sorted=1, async_tail=1),
                    Case("partner:keys_sorted-without-sort_keys", keys_sorted=1, sort_keys=None),
                    Case("keys_sorted-with-the-atomics-scratch", "the forward sorted into the scratch of the sorted path", keys_sorted=1)]),
    Row("gsr_side_join", [STREAM], note="a stream handle only: nothing to refuse"),
    Row("gsr_normal_world_forward", [R("normal_view"), R("cam"), N("width", W0), N("height", H0), R("out_normal_world"), STREAM]),
    Row("gsr_normal_world_backward", [R("normal_view"), R("cam"), N("width", W0), N("height", H0), R("g_normal_world"), R("g_normal_view"), STREAM]),
]

# ---------------------------------------------------------------------------------------------------------------- the training step
_C, _Hh, _Ww = 3, 48, 64
_PLANES = [O("dm_dmu1"), O("dm_dsigma1_sq"), O("dm_dsigma12")]
_PLANES_REQ = [R("dm_dmu1"), R("dm_dsigma1_sq"), R("dm_dsigma12")]
_PARTIAL = [Case("partner:one-derivative-plane", dm_dmu1=FAKE), Case("partner:two-derivative-planes", dm_dmu1=FAKE, dm_dsigma12=FAKE)]
_COMPOSITE = [Case("needs:background-with-alpha", alpha=FAKE), Case("needs:background-with-gt_mask", gt_mask=FAKE)]


def _segments(*segs):
    def make(ctx):
        arr = (ctx.gsr.AdamSegment * max(len(segs), 17))()
        for i, s in enumerate(segs):
            arr[i] = ctx.gsr.AdamSegment(*s)
        return ctx.keep(arr)
    return make


def _groups(*gs):
    def make(ctx):
        arr = (ctx.gsr.GatherGroup * 17)()
        for i in range(17):
            arr[i] = ctx.gsr.GatherGroup(*(gs[i] if i < len(gs) else (0, 0, 1)))
        return ctx.keep(arr)
    return make


def _adam(entry, extra, cases=()):
    a = [R("param", aligned=16), R("grad", aligned=16), R("exp_avg", aligned=16), R("exp_avg_sq", aligned=16), U("n", 1000, zero="noop"),
         H("segments", _segments((0, 1000, 1e-3, 0.0, 0, 0))), N("num_segments", 1), V("beta1", 0.9), V("beta2", 0.999), V("eps", 1e-15), V("step", 1)]
    return Row(entry, a + extra + [STREAM],
               [Case("num_segments>16", num_segments=17), Case("step=0", "the step counter is 1-based", step=0), Case("step<0", step=-1),
                Case("segments-stop-short-of-n", segments=_segments((0, 996, 1e-3, 0.0, 0, 0))),
                Case("segments-out-of-order", segments=_segments((0, 600, 1e-3, 0.0, 0, 0), (500, 1000, 1e-3, 0.0, 0, 0)), num_segments=2),
                Case("segment-split>period", segments=_segments((0, 1000, 1e-3, 0.0, 48, 49)))] + list(cases), family="gsr_adam_step")


TRAINING = [
    Row("gsr_ssim_l1_scratch_floats", [N("C", _C), N("H", _Hh), N("W", _Ww)], query=True),
    Row("gsr_ssim_l1_forward", [R("img1"), R("img2"), N("C", _C, zero="noop"), N("H", _Hh, zero="noop"), N("W", _Ww, zero="noop"), V("C1", 1e-4),
                                V("C2", 9e-4), R("sums"), R("scratch"), O("ssim_map")] + _PLANES + [STREAM], _PARTIAL,
        note="an empty image (a zero among C, H, W) is a no-op that zeroes sums"),
    Row("gsr_ssim_l1_backward", [R("img1"), R("img2"), N("C", _C, zero="noop"), N("H", _Hh, zero="noop"), N("W", _Ww, zero="noop"), R("weights")] +
        _PLANES_REQ + [R("dL_dimg1"), STREAM]),
    Row("gsr_surface_forward", [R("allmap"), R("raymat"), V("depth_ratio", 0.0), N("H", _Hh, zero="noop"), N("W", _Ww, zero="noop"), R("surf_depth"),
                                R("surf_normal"), STREAM]),
    Row("gsr_surface_backward", [R("allmap"), R("raymat"), V("depth_ratio", 0.0), N("H", _Hh, zero="noop"), N("W", _Ww, zero="noop"), R("surf_depth"),
                                 O("g_surf_depth", True), O("g_surf_normal"), R("g_allmap"), STREAM]),
    Row("gsr_densification_stats", [N("P", P0, zero="noop"), R("grad_means2D"), R("radii"), R("gaussian_weights"), R("xyz_gradient_accum"), R("denom"),
                                    R("accum_w"), R("denom_w"), R("max_radii2D"), STREAM]),
    Row("gsr_gather_rows", [R("src"), R("dst"), R("row_map"), U("n_rows", 50, zero="noop"), H("groups", _groups((0, 0, 3), (150, 150, 48))),
                            N("num_groups", 2, zero="noop"), STREAM],
        [Case("num_groups>16", num_groups=17), Case("zero-width-group", groups=_groups((0, 0, 3), (150, 150, 0)))]),
    Row("gsr_split_children", [N("n_children", 40, zero="noop"), V("scale_dims", 2), N("N", 2), R("parent"), R("xyz"), R("scaling"), R("rotation"),
                               R("noise"), R("child_xyz"), R("child_scaling"), STREAM],
        [Case("scale_dims=1", scale_dims=1), Case("scale_dims=4", scale_dims=4)]),
    Row("gsr_photometric_scratch_floats", [N("C", _C), N("H", _Hh), N("W", _Ww)], query=True),
    Row("gsr_photometric_forward", [R("rgb"), O("alpha"), R("gt"), O("gt_mask"), O("background"), N("C", _C), N("H", _Hh), N("W", _Ww), V("C1", 1e-4),
                                    V("C2", 9e-4), R("sums"), R("scratch")] + _PLANES + [STREAM],
        _PARTIAL + _COMPOSITE + [Case("C>65535", "a grid dimension", C=65536)]),
    Row("gsr_photometric_backward", [R("rgb"), O("alpha"), R("gt"), O("gt_mask"), O("background"), N("C", _C), N("H", _Hh), N("W", _Ww), R("weights")] +
        _PLANES_REQ + [O("dL_drgb", True), O("dL_dalpha"), STREAM], _COMPOSITE + [Case("needs:alpha-with-dL_dalpha", dL_dalpha=FAKE)]),
    Row("gsr_ssim_map_backward", [R("img1"), R("img2"), N("planes", 6), N("H", _Hh), N("W", _Ww), R("dL_dmap")] + _PLANES_REQ + [R("dL_dimg1"), STREAM],
        [Case("planes>65535", "a grid dimension", planes=65536)]),
    Row("gsr_normal_loss_forward", [R("rend_normal"), R("surf_normal"), O("mask"), N("H", _Hh), N("W", _Ww), R("sum2"), R("scratch"), STREAM]),
    Row("gsr_normal_loss_backward", [R("rend_normal"), R("surf_normal"), O("mask", True), N("H", _Hh), N("W", _Ww), R("g_sum"), R("g_rend_normal"),
                                     R("g_surf_normal"), STREAM]),
    _adam("gsr_adam_step", []),
    _adam("gsr_adam_step_range", [V("range_begin", 0), V("range_end", 1000)],
          [Case("range_begin-not-a-multiple-of-4", range_begin=2), Case("range_end>n", range_end=1004), Case("range_begin>range_end", range_begin=8, range_end=4),
           Case("range_end-inside-not-a-multiple-of-4", range_end=998)]),
]

# ---------------------------------------------------------------------------------------------------------------- initialisation, evaluation, viewer
def _knn_bytes(delta=0):
    return lambda ctx: int(ctx.gsr.lib.gsr_knn_scratch_bytes(P0)) + delta


def _metric_floats(delta=0):
    return lambda ctx: int(ctx.gsr.lib.gsr_image_metrics_scratch_floats(_C, _Hh, _Ww)) + delta


def _mae_floats(delta=0):
    return lambda ctx: int(ctx.gsr.lib.gsr_normal_mae_scratch_floats(_Hh, _Ww)) + delta


_LUT = dict(C=1, flags=4, table=FAKE, scratch=FAKE, scratch_floats=4)       # gsr_present_view with a colour map (GSR_VIEW_COLORMAP)

EVALUATION = [
    Row("gsr_knn_scratch_bytes", [N("P", P0)], query=True),
    Row("gsr_knn_mean_dist", [N("P", P0, zero="noop"), R("points"), R("mean_dist"), R("scratch", aligned=16), V("scratch_bytes", _knn_bytes()), STREAM],
        [Case("P=2^30", P=1 << 30), Case("scratch-one-byte-short", scratch_bytes=_knn_bytes(-1))]),
    Row("gsr_image_metrics_scratch_floats", [N("C", _C), N("H", _Hh), N("W", _Ww)], query=True),
    Row("gsr_image_metrics", [R("img"), R("gt"), N("C", _C), N("H", _Hh), N("W", _Ww), V("flags", 3), O("alpha"), O("gt_mask"), O("background"),
                              R("row", aligned=8), R("scratch", aligned=16), V("scratch_floats", _metric_floats()), O("img_u8", True), O("gt_u8"), STREAM],
        _COMPOSITE + [Case("unknown-flag-bit", flags=4), Case("needs:QUANT8-with-a-uint8-output", flags=1),
                      Case("scratch-one-float-short", scratch_floats=_metric_floats(-1)), Case("C>65535", C=65536)]),
    Row("gsr_normal_mae_scratch_floats", [N("H", _Hh), N("W", _Ww)], query=True),
    Row("gsr_normal_mae", [R("pred"), R("gt"), N("H", _Hh), N("W", _Ww), V("pred_divisor", 1.0), V("gt_divisor", 255.0), V("eps", 1e-8),
                           R("row", aligned=8), R("scratch", aligned=16), V("scratch_floats", _mae_floats()), O("error_map", True), STREAM],
        [Case("pred_divisor=0", pred_divisor=0.0), Case("gt_divisor<0", gt_divisor=-1.0), Case("eps<0", eps=-1e-8),
         Case("scratch-one-float-short", scratch_floats=_mae_floats(-1))]),
    Row("gsr_present_view_scratch_floats", [N("C", 1), N("H", _Hh), N("W", _Ww), V("flags", 4)], query=True),
    Row("gsr_present_view", [R("src"), N("C", 3), N("H", _Hh), N("W", _Ww), V("flags", 1), O("table"), O("out_f32", True), O("out_u8"), O("scratch"),
                             V("scratch_floats", 0), STREAM],
        [Ok("colour-map", **_LUT), Ok("colour-map+sobel", **dict(_LUT, C=3, flags=7, scratch_floats=4 + _Hh * _Ww)),
         Case("either:out_f32|out_u8", out_f32=None), Case("C=2", C=2), Case("unknown-flag-bit", flags=8),
         Case("colour-map-on-three-channels", **dict(_LUT, C=3)), Case("needs:table-with-COLORMAP", **dict(_LUT, table=None)),
         Case("needs:scratch-with-COLORMAP", **dict(_LUT, scratch=None)), Case("scratch-one-float-short", **dict(_LUT, scratch_floats=3)),
         Case("scratch-short-with-SOBEL", **dict(_LUT, flags=6, scratch_floats=4 + _Hh * _Ww - 1)),
         Case("misaligned:scratch", **dict(_LUT, scratch=FAKE + 4))]),
    Row("gsr_set_option", [V("name", b"cull"), V("value", 1)], [Case("unknown-name", name=b"no-such-option"), Case("null:name", name=None)]),
    Row("gsr_profile_collect", [H("ms_out", lambda ctx: ctx.keep((ctypes.c_float * 64)())), H("launches_out", lambda ctx: ctx.keep((ctypes.c_int * 64)()))],
        note="either array may be NULL (it is then not returned): nothing to refuse"),
]
EVALUATION[-1].cases = []       # (the two host arrays are optional)

TABLE = RASTER + REFLECTION + TRAINING + EVALUATION
ROWS = {r.entry: r for r in TABLE}
assert len(ROWS) == len(TABLE)

WELL_FORMED = "well-formed"


def case_ids():
    """[(entry, case id)] of every call the child makes, the untouched row of each entry first."""
    return [(r.entry, c) for r in TABLE for c in [WELL_FORMED] + [k.id for k in r.cases]]


# ---------------------------------------------------------------------------------------------------------------- the child process
HIDE_GPUS = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1", "GPU_DEVICE_ORDINAL": "-1"}


class _Ctx:
    def __init__(self, gsr):
        self.gsr, self.kept, self.allocs = gsr, [], []
        self.cb = gsr.ALLOC_FN(lambda user, which, nbytes: self.allocs.append((which, nbytes)) or 0)     # records the request, returns NULL

    def keep(self, obj):
        self.kept.append(obj)
        return obj


def _visible_devices():
    """The HIP runtime's device count; 0 when it reports an error (hipErrorNoDevice)."""
    hip = None
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = ctypes.CDLL(name)
            break
        except OSError:
            continue
    if hip is None:
        return -1
    n = ctypes.c_int(0)
    return n.value if hip.hipGetDeviceCount(ctypes.byref(n)) == 0 else 0


def _call(ctx, row, changes):
    fn = getattr(ctx.gsr.lib, row.entry)
    values = []
    for a, ctype in zip(row.args, fn.argtypes):
        v = changes[a.name] if a.name in changes else a.value
        if a.kind == "alloc":
            v = ctx.gsr.ALLOC_FN() if v == "NULL" else ctx.cb
        elif callable(v):
            v = v(ctx)
        if v is not None and isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer) and not isinstance(v, ctypes.Array):
            v = ctypes.byref(v)
        values.append(v)
    assert len(values) == len(fn.argtypes), (row.entry, len(values), len(fn.argtypes))
    del ctx.allocs[:]
    return int(fn(*values)), len(ctx.allocs)


_ctx = None


def call(gsr, entry, case):
    """One call of the table for tests/cabi_child.py's loop: (rc, {"allocs": requests the allocation callback saw})."""
    global _ctx
    _ctx = _ctx or _Ctx(gsr)
    row = ROWS[entry]
    changes = {} if case == WELL_FORMED else next(c for c in row.cases if c.id == case).changes
    rc, allocs = _call(_ctx, row, changes)
    return rc, {"allocs": allocs}
