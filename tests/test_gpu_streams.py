"""Stream ordering of every entry point, and batches of views over several streams.

Almost the whole suite runs on the default stream, where everything serialises.  The library is not stateless: one side stream per device
with four events and two flags (csrc/gsr_cubemap.hip), one read-back slot per thread and device (csrc/gsr_common.hip), the scratch
tensors `_gsr._side_held` keeps per stream, the camera and ray blocks `gaussian_renderer._cached_block` keeps, the sums
`utils.loss_utils._last_sums` shares between two calls.  Here each entry runs under `torch.cuda.stream(s)` on inputs that hold NaN until
a delay on `s` has run out (tests/stream_probe.py), views are interleaved on one stream and overtake each other on two, and bench.py's
`--view-streams` schedule is restated and compared with the one-stream loop.

The serial reference is always the same call with the same inputs on the default stream, in this process, with nothing else in flight;
never a second multi-stream run.  Bars: forward outputs and integer state bit-identical; gradients summed with float
atomics 5e-5 of the tensor's maximum; cubemap and fail-value sinks after side_join 1e-5.

Known limit: both rasterizer forwards block the host on `num_rendered`.  The late-input arrangement therefore proves the ordering of
everything enqueued up to that wait (preprocess, statistics, depth sort) and of every entry without a host wait; it does not prove the
ordering of the forward's kernels behind the wait (they take the same `stream` variable).  For the same reason a delay in front of a
forward holds the host: in family 4 the views' forwards are enqueued in host order, and the delay sits between view 0's forward and its
backward.  A second host wait: `_cam_block`'s builder uploads K^-1 with a blocking copy, so the entries that take a camera
(deferred_reflection, rasterize_reflect, render_fast) get ready camera tensors with a cached block and only their other inputs late
(ready_camera); with late camera tensors the host would wait out the delay before their first kernel.

Each test prints `STREAMS <family> <case>: ...` with its worst deviations; every test ends with torch.cuda.synchronize()."""
import contextlib

import numpy as np
import pytest
import torch

import stream_probe as SP
from helpers import HipGauss, HipSurfel, S, scene_kwargs

pytestmark = pytest.mark.gpu

ATOMIC, SINK = 5e-5, 1e-5
NAN = float("nan")

# view: P, W, H, seed, mu, eye of the camera (both look at (0, 0, 5))
VIEWS = {"A": (4097, 200, 136, 62, -3.0, (0.3, -0.2, -0.8)),          # ragged 16x16 tiles on both axes
         "B": (257, 96, 64, 61, -1.6, (-0.5, 0.3, -0.6))}            # another camera, smaller: another workspace size
SIZES = (16, 128)                                                     # cubemap L: the 8-bit and the 9-bit key-sort configuration

_streams = []
_control = {}
_serial = {}


def streams(n):
    """The first n of the module's three side streams (four streams with the default one).  The negative control chose them: each is
    shown to run beside the default stream and beside the other two."""
    assert n <= 3 and len(_streams) == 3, "the negative control has not chosen the streams"
    return _streams[:n]


@contextlib.contextmanager
def drained():
    """Nothing in flight before, nothing left pending after."""
    torch.cuda.synchronize()
    try:
        yield
    finally:
        torch.cuda.synchronize()


def reads_poison(late_stream, op_stream):
    """The late-input arrangement around a torch op that is deliberately issued under ANOTHER stream with no event.  True: the op read
    the poison, so the delay held the inputs back and the two streams ran side by side.  (It reads stale data; it cannot fault.)"""
    with drained():
        x = SP.late_inputs(late_stream, {"x": np.ones(4096, np.float32)})["x"]
        with torch.cuda.stream(op_stream):
            y = x * 2
        got = SP.fetch(op_stream, {"y": y})["y"]
        ordered = SP.fetch(late_stream, {"x": x})["x"]
    assert (ordered == 1).all(), "the ordered read of the late inputs is wrong"
    return not np.isfinite(got).all()


CANDIDATES = 12


@pytest.fixture(scope="session", autouse=True)
def negative_control():
    """Runs first; every test of the module depends on it.  The HIP runtime maps its streams onto a few hardware queues (four by
    default), in an order that depends on what the process created before, and two streams on one queue serialise: behind such a pair
    every test here would pass whatever the library did.  So the module's three streams are chosen by the control itself: a candidate is
    kept when an op issued, without an event, on the default stream and on each stream already kept reads the poison of late inputs on the
    candidate, and the other way round.  Candidates are tried one at a time and the tests use the three kept and the default stream.  If three such
    streams cannot be found the delay does not hold the inputs back on this machine, and every test of the module errors out here
    instead of passing vacuously."""
    default = torch.cuda.default_stream()
    tried = 0
    while len(_streams) < 3 and tried < CANDIDATES:
        c = torch.cuda.Stream()
        tried += 1
        with drained():                  # an op's first launch and a stream's first allocation can take the host longer than the delay
            for st in (c, default):
                with torch.cuda.stream(st):
                    torch.ones(4096, device="cuda") * 2
        if reads_poison(c, default) and all(reads_poison(c, k) and reads_poison(k, c) for k in _streams):
            _streams.append(c)
        del c
    _control.update(streams=len(_streams), tried=tried, cycles_per_ms=SP.cycles_per_ms())
    print("STREAMS control: %.0f sleep cycles per ms; %d of %d candidate streams run beside the default stream and each other: "
          "the unordered reads come back as poison (a mismatch, as it must be)" % (_control["cycles_per_ms"], len(_streams), tried))
    if len(_streams) < 3:
        raise RuntimeError("stream tests: the %g ms delay held the late inputs back on %d of %d candidate streams only; three are needed: %r"
                           % (SP.DEFAULT_DELAY_MS, len(_streams), tried, _control))
    yield


def test_0_negative_control_reports_a_mismatch():
    """What the control found, and once more on the pair family 1 uses: an op on the default stream reads the poison."""
    assert _control["streams"] == 3 and _control["cycles_per_ms"] > 0
    assert reads_poison(streams(1)[0], torch.cuda.default_stream())


# ------------------------------------------------------------------------------------------------------------ comparing
def check(family, what, got, ref, exact=(), atomic=(), sink=(), may_be_zero=("g_fail", "g_means2D")):
    """exact: the same bits; atomic / sink: within 5e-5 / 1e-5 of the serial tensor's maximum and finite.  A float reference that is all
    zero would compare nothing, so it is refused (the fail-value gradient apart: no pixel of these views takes the fail value)."""
    fails, worst = [], {"atomic": 0.0, "sink": 0.0}
    for k in exact:
        if ref[k].dtype.kind == "f" and ref[k].size and k not in may_be_zero:
            assert np.nanmax(np.abs(ref[k])) > 0, (what, k, "the serial reference is all zero")
        if not SP.same_bits(got[k], ref[k]):
            fails.append((k, "bits differ", SP.deviation(got[k], ref[k])))
    for keys, bar, name in ((atomic, ATOMIC, "atomic"), (sink, SINK, "sink")):
        for k in keys:
            assert k in may_be_zero or np.abs(ref[k]).max() > 0, (what, k, "the serial reference is all zero")
            d = SP.deviation(got[k], ref[k])
            worst[name] = max(worst[name], d)
            if not SP.close_to_serial(got[k], ref[k], bar):
                fails.append((k, "deviation", d, "bar", bar))
    print("STREAMS %s %s: %d tensors bit-identical; worst of the %g bar %.3g, of the %g bar %.3g"
          % (family, what, len(exact) - sum(1 for f in fails if f[1] == "bits differ"), ATOMIC, worst["atomic"], SINK, worst["sink"]))
    assert not fails, (family, what, fails)


def on_device(arrays):
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in arrays.items()}


def host(tensors):
    return {k: (None if v is None else v.detach().cpu().numpy()) for k, v in tensors.items()}


def serial(key, arrays, fn):
    """fn on the default stream with nothing else in flight: computed once per key, never modified."""
    if key not in _serial:
        with drained():
            _serial[key] = host(fn(on_device(arrays)))
    return _serial[key]


_ready = {}


def ready_camera(arrays, cam):
    """The `cam_*` tensors of `arrays` on the device, made once and complete, with their camera block built on the default stream.
    `_cam_block`'s builder uploads K^-1 with a blocking copy, which drains the stream it runs on: were the camera tensors late, the
    host would wait out the delay there, before the entry's first kernel is enqueued, and a kernel on a wrong stream would read good
    inputs.  With ready camera tensors and a cached block (a hit makes the calling stream wait for the block's event, the host for
    nothing) no host wait precedes the kernels."""
    import gaussian_renderer as gr
    with drained():
        if id(arrays) not in _ready:
            _ready[id(arrays)] = on_device({k: v for k, v in arrays.items() if k.startswith("cam_")})
        fixed = _ready[id(arrays)]
        gr._cam_block(fixed["cam_viewmatrix"], (int(cam["H"]), int(cam["W"]), cam["K"]), fixed["cam_R"], fixed["cam_T"])
    return fixed


def late(family, what, arrays, fn, exact=(), atomic=(), sink=(), key=None, camera=None, **kw):
    """Family 1: fn under a side stream on late inputs, fetched on that stream alone, against fn on the default stream.  camera: the
    `cam_*` entries are not late but ready, with their camera block cached (ready_camera)."""
    fixed = {}
    if camera is not None:
        fixed = ready_camera(arrays, camera)
        arrays = {k: v for k, v in arrays.items() if k not in fixed}
    ref = serial(key or (family, what), arrays, lambda t: fn(dict(t, **fixed)))
    s = streams(1)[0]
    with drained():
        inp = dict(SP.late_inputs(s, arrays), **fixed)
        with torch.cuda.stream(s):
            out = fn(inp)
        got = SP.fetch(s, out)
    check(family, what, got, ref, exact, atomic, sink, **kw)


@contextlib.contextmanager
def binding(which):
    import _gsr
    saved = _gsr.PYBIND
    if which == "compiled" and saved is None:
        pytest.skip("the compiled binding is not built")
    _gsr.PYBIND = saved if which == "compiled" else None
    try:
        yield
    finally:
        _gsr.PYBIND = saved


# ------------------------------------------------------------------------------------------------------------ the views
_arrays = {}


def camera_of(view):
    _, W, H, _, _, eye = VIEWS[view]
    return S.look_at_camera(W, H, eye=eye, target=(0, 0, 5))


def raster_arrays(view, variant):
    """Scene, camera and upstream gradients of one view as numpy (scalars as they are)."""
    key = ("raster", view, variant)
    if key not in _arrays:
        P, W, H, seed, mu, _ = VIEWS[view]
        kw, _, _ = scene_kwargs(variant, P, W, H, seed, mu, 3, (0.2, 0.1, 0.3), cam=camera_of(view))
        g = S.make_upstream_grads(H, W, seed)
        _arrays[key] = dict(kw, **{"up_" + k: v for k, v in g.items()})
    return _arrays[key]


class RasterView:
    """One view through a rasterizer alone (variant S, or G with antialiasing), in two phases."""
    FORWARD = {"S": ("color", "radii", "allmap", "refl_map", "gw"), "G": ("color", "radii", "invdepth", "normal_map", "refl_map")}
    STATE = ("num_rendered", "point_list", "ranges", "n_contrib")

    def __init__(self, variant, t):
        self.variant, self.t = variant, t

    def fwd(self):
        import _gsr
        t, v = self.t, self.variant
        kw = {k: x for k, x in t.items() if not k.startswith("up_")}
        hip = self.hip = HipSurfel(kw) if v == "S" else HipGauss(kw, antialiasing=True)
        self.out = {k: getattr(hip, k) for k in self.FORWARD[v]}
        geom, binning, img = hip.ctx.saved_tensors[-3:]
        P, R, W, H = hip.P, hip.R, hip.W, hip.H
        spec = {"point_list": (R,), "ranges": (((W + 15) // 16) * ((H + 15) // 16), 2), "n_contrib": (2 if v == "S" else 1, H, W)}
        for name, shape in spec.items():
            self.out[name] = _gsr.debug_fetch(0 if v == "S" else 1, name, P, R, W, H, geom, binning, img, torch.int32, shape)
        self.out["num_rendered"] = torch.tensor([R], dtype=torch.int32)

    def bwd(self):
        hip, t = self.hip, self.t
        loss = (hip.color * t["up_dL_dcolor"]).sum() + (hip.refl_map * t["up_dL_drefl"]).sum()
        if self.variant == "S":
            loss = loss + (hip.allmap * t["up_dL_dplanes"]).sum()
        else:
            loss = loss + (hip.invdepth * t["up_dL_dinvdepth"]).sum() + (hip.normal_map * t["up_dL_dnormal"]).sum()
        loss.backward()

    def grads(self):
        hip = self.hip
        names = dict(means3D=hip.means3D, means2D=hip.means2D, opacities=hip.opac, shs=hip.shs, refl_strengths=hip.refl, scales=hip.scales,
                     rotations=hip.rots)
        if self.variant == "G":
            names["normals"] = hip.normals
        return names

    def results(self):
        return dict(self.out, **{"g_" + k: leaf.grad for k, leaf in self.grads().items()})

    def keys(self):
        g = ("means3D", "means2D", "opacities", "shs", "refl_strengths", "scales", "rotations") + (("normals",) if self.variant == "G" else ())
        return dict(exact=self.FORWARD[self.variant] + self.STATE, atomic=tuple("g_" + k for k in g))


PARAMS = ("means3D", "shs", "opacities", "scales", "rotations", "refl_strengths", "cubemap", "fail")
CAMERA = ("viewmatrix", "projmatrix", "campos", "R", "T")


def refl_arrays(view, L, camera=None):
    """Scene with a cubemap of size L, camera tensors and the training loop's pair of upstream gradients, as numpy."""
    key = ("refl", view, L, None if camera is None else id(camera))
    if key not in _arrays:
        P, W, H, seed, mu, _ = VIEWS[view]
        sc = S.make_scene(P, "S", seed=seed, mu=mu)
        tex, fail = S.make_cubemap(L, 3, seed)
        cam = camera or camera_of(view)
        gen = torch.Generator().manual_seed(seed + L)
        a = {k: sc[k] for k in PARAMS[:6]}
        a.update(cubemap=tex, fail=fail + np.float32(0.25), mask=sc["env_scope_mask"], bg=np.array([0.1, 0.2, 0.3], np.float32))
        a.update({"cam_" + k: np.ascontiguousarray(cam[k]) for k in CAMERA})
        a.update(up_final=(torch.randn(3, H, W, generator=gen) / (H * W)).numpy(), up_allmap=(torch.randn(8, H, W, generator=gen) / (H * W)).numpy())
        _arrays[key] = (a, cam)
    return _arrays[key]


class ReflView:
    """One view through rasterizer + deferred reflection (fused node or two nodes) with both gradient sinks into its own flat buffer,
    in two phases.  `shared`: (leaves, FlatGrads, accumulate) of a batch that sums its views into one buffer."""
    FORWARD = ("final", "refl_color", "nworld", "base", "radii", "allmap", "refl_map", "gw")

    def __init__(self, t, cam, fused, async_tail, shared=None):
        from gsr_dist import FlatGrads
        self.t, self.cam, self.fused, self.async_tail = t, cam, fused, async_tail
        if shared is None:
            self.p = {k: t[k].clone().requires_grad_(True) for k in PARAMS}
            self.fg = FlatGrads(self.p)
            self.fg.flat.fill_(NAN)
            self.accumulate = False
        else:
            self.p, self.fg, self.accumulate = shared

    def fwd(self):
        import test_gpu_fused as F
        t, cam = self.t, self.cam
        ct = {k: t["cam_" + k] for k in CAMERA}
        self.out, _ = F._run(self.fused, self.p, t["mask"], cam, ct, int(cam["W"]), int(cam["H"]), t["bg"], None, raster_sink=self.fg.sink(),
                             refl_sink=self.fg.sink(names=("cubemap", "fail")), accumulate=self.accumulate, async_tail=self.async_tail)

    def bwd(self):
        torch.autograd.backward([self.out["final"], self.out["allmap"]], [self.t["up_final"], self.t["up_allmap"]])

    def results(self):
        """(joins the library's side stream into the current stream first)"""
        import _gsr
        _gsr.side_join()
        return dict(self.out, **{"g_" + k: self.fg.view(k) for k in PARAMS})

    def keys(self):
        return dict(exact=self.FORWARD, atomic=tuple("g_" + k for k in PARAMS[:6]), sink=("g_cubemap", "g_fail"))


KINDS = {"S": lambda view, L: (raster_arrays(view, "S"), lambda t: RasterView("S", t)),
         "G": lambda view, L: (raster_arrays(view, "G"), lambda t: RasterView("G", t)),
         "two_node": lambda view, L: (refl_arrays(view, L)[0], lambda t: ReflView(t, refl_arrays(view, L)[1], False, False)),
         "two_node_async": lambda view, L: (refl_arrays(view, L)[0], lambda t: ReflView(t, refl_arrays(view, L)[1], False, True)),
         "fused": lambda view, L: (refl_arrays(view, L)[0], lambda t: ReflView(t, refl_arrays(view, L)[1], True, False)),
         "fused_async": lambda view, L: (refl_arrays(view, L)[0], lambda t: ReflView(t, refl_arrays(view, L)[1], True, True))}


def whole(make):
    def fn(t):
        v = make(t)
        v.fwd()
        v.bwd()
        return v.results()
    return fn


def serial_view(kind, view, L):
    arrays, make = KINDS[kind](view, L)
    return serial(("view", kind, view, L if kind not in ("S", "G") else 0), arrays, whole(make))


# ============================================================================================== 1. late inputs, one entry at a time
@pytest.mark.parametrize("which", ["ctypes", "compiled"])
@pytest.mark.parametrize("view", ["A", "B"])
def test_1_surfel_forward_backward(view, which):
    arrays, make = KINDS["S"](view, 0)
    with binding(which):
        late("1", "S %s %s" % (view, which), arrays, whole(make), key=("view", "S", view, 0, which), **make(None).keys())


@pytest.mark.parametrize("which", ["ctypes", "compiled"])
@pytest.mark.parametrize("view", ["A", "B"])
def test_1_gauss_forward_backward_with_antialiasing(view, which):
    arrays, make = KINDS["G"](view, 0)
    with binding(which):
        late("1", "G %s %s" % (view, which), arrays, whole(make), key=("view", "G", view, 0, which), **make(None).keys())


@pytest.mark.parametrize("which", ["ctypes", "compiled"])
def test_1_mark_visible(which):
    import _gsr
    a = raster_arrays("A", "S")
    arrays = {k: a[k] for k in ("means3D", "viewmatrix", "projmatrix")}
    arrays["means3D"] = arrays["means3D"].copy()
    arrays["means3D"][64:320, 2] = -3.0 - np.abs(arrays["means3D"][64:320, 2])       # behind the camera: a mixed answer, which no poison gives
    with binding(which):
        late("1", "mark_visible " + which, arrays, lambda t: dict(present=_gsr.mark_visible(t["means3D"], t["viewmatrix"], t["projmatrix"])),
             exact=("present",))
    ref = _serial[("1", "mark_visible " + which)]["present"]
    assert ref.any() and not ref.all()


def _pixel_arrays(view, L):
    key = ("pixels", view, L)
    if key not in _arrays:
        _, W, H, seed, _, _ = VIEWS[view]
        cam = camera_of(view)
        g = torch.Generator().manual_seed(seed * 7 + L)
        a = dict(nv=torch.randn(3, H, W, generator=g).numpy(), base=torch.rand(3, H, W, generator=g).numpy(), strength=torch.rand(1, H, W, generator=g).numpy(),
                 tex=(torch.rand(6, 3, L, L, generator=g) - 0.5).numpy(), fail=(torch.randn(3, generator=g) * 0.5).numpy())
        a.update({"up_" + k: torch.randn(3, H, W, generator=g).numpy() for k in ("final", "refl", "nworld")})
        a.update({"cam_" + k: np.ascontiguousarray(cam[k]) for k in ("viewmatrix", "R", "T")})
        _arrays[key] = (a, cam)
    return _arrays[key]


def _deferred_reflection(path, cam):
    def fn(t):
        import _gsr
        import gaussian_renderer as gr
        from test_gpu_fused import _Env
        H, W = t["nv"].shape[1:]
        saved = gr.REFLECTION_BACKWARD_BINNED, gr.REFLECTION_FORWARD_KEYS
        try:
            gr.REFLECTION_BACKWARD_BINNED = path != "atomics"
            gr.REFLECTION_FORWARD_KEYS = path in ("forward_keys", "async_tail")
            nv, base, s, tex, fail = (t[k].clone().requires_grad_(True) for k in ("nv", "base", "strength", "tex", "fail"))
            kw = {}
            if path == "async_tail":
                sink_t = {"cubemap": torch.full_like(tex, NAN), "fail": torch.full_like(fail, NAN)}
                kw = dict(grad_sink=sink_t, async_tail=True)
            f, c, n = gr.deferred_reflection(nv, base, s, _Env(tex, fail), t["cam_viewmatrix"], (H, W, cam["K"]), t["cam_R"], t["cam_T"], **kw)
            ((f * t["up_final"]).sum() + (c * t["up_refl"]).sum() + (n * t["up_nworld"]).sum()).backward()
            if path == "async_tail":
                assert tex.grad is None
                _gsr.side_join()
                g_tex, g_fail = sink_t["cubemap"], sink_t["fail"]
            else:
                g_tex, g_fail = tex.grad, fail.grad
            return dict(final=f, refl=c, nworld=n, g_nv=nv.grad, g_base=base.grad, g_s=s.grad, g_cubemap=g_tex, g_fail=g_fail)
        finally:
            gr.REFLECTION_BACKWARD_BINNED, gr.REFLECTION_FORWARD_KEYS = saved
    return fn


@pytest.mark.parametrize("L", SIZES)
@pytest.mark.parametrize("path", ["forward_keys", "backward_keys", "atomics", "async_tail"])
def test_1_deferred_reflection(path, L):
    """The two-node pixel pass alone: planes, cubemap, fail value and upstream gradients late, the camera ready (ready_camera)."""
    arrays, cam = _pixel_arrays("A", L)
    texel = dict(atomic=("g_cubemap", "g_fail")) if path == "atomics" else dict(sink=("g_cubemap", "g_fail"))
    late("1", "deferred_reflection %s L=%d" % (path, L), arrays, _deferred_reflection(path, cam),
         exact=("final", "refl", "nworld", "g_nv", "g_base", "g_s"), camera=cam, **texel)


@pytest.mark.parametrize("L", SIZES)
@pytest.mark.parametrize("async_tail", [False, True])
def test_1_rasterize_reflect(async_tail, L):
    kind = "fused_async" if async_tail else "fused"
    arrays, make = KINDS[kind]("A", L)
    late("1", "rasterize_reflect async_tail=%s L=%d" % (async_tail, L), arrays, whole(make), key=("view", kind, "A", L, "ready camera"),
         camera=refl_arrays("A", L)[1], **make_keys(kind))


def make_keys(kind):
    return (RasterView(kind, None) if kind in ("S", "G") else ReflView.__new__(ReflView)).keys()


def _model_and_view(t, cam):
    from test_gpu_dropin import _model
    from test_gpu_fused import _Env
    W, H = int(cam["W"]), int(cam["H"])

    class View:
        FoVx, FoVy, image_width, image_height = cam["FoVx"], cam["FoVy"], W, H
        world_view_transform, full_proj_transform, camera_center = t["cam_viewmatrix"], t["cam_projmatrix"], t["cam_campos"]
        HWK, R, T, znear, zfar = (H, W, cam["K"]), t["cam_R"], t["cam_T"], cam["znear"], cam["zfar"]
    return _model(t, _Env(t["cubemap"], t["fail"])), View


def test_1_render_fast_under_no_grad():
    """render_fast -> rasterize_eval (the inference-only forward with the reflection epilogue)."""
    from gaussian_renderer import render_fast
    from test_gpu_dropin import _Pipe
    arrays, cam = refl_arrays("A", 16)

    def fn(t):
        PC, View = _model_and_view(t, cam)
        with torch.no_grad():
            return dict(render_fast(View, PC, _Pipe, t["bg"]))
    late("1", "render_fast", arrays, fn, exact=("render", "rend_alpha", "rend_normal", "refl_strength_map", "refl_color_map", "base_color_map"),
         camera=cam)


@pytest.mark.parametrize("B", [257, 4097])
def test_1_cubemap_encoder(B):
    from cubemapencoder.cubemap_encoder import cubemap_encode
    g = torch.Generator().manual_seed(B)
    arrays = dict(d=torch.randn(B, 3, generator=g).numpy(), cm=(torch.rand(6, 3, 16, 16, generator=g) - 0.5).numpy(), fv=torch.randn(3, generator=g).numpy(),
                  go=torch.randn(3, B, generator=g).numpy())
    arrays["d"][0] = 0.0                  # the zero vector: the fail value

    def fn(t):
        D, CM, FV = (t[k].clone().requires_grad_(True) for k in ("d", "cm", "fv"))
        out = cubemap_encode(D, CM, FV, 1, 1)
        (out * t["go"]).sum().backward()
        return dict(out=out, g_dirs=D.grad, g_cubemap=CM.grad, g_fail=FV.grad)
    late("1", "cubemap_encode B=%d" % B, arrays, fn, exact=("out", "g_dirs"), atomic=("g_cubemap", "g_fail"), may_be_zero=())


def test_1_photometric_l1_and_ssim_losses():
    """photometric_loss with its backward; then l1_loss + ssim, which share one forward through `_last_sums`, with theirs."""
    import loss_bounds as LB
    from utils.loss_utils import clear_cache, l1_loss, photometric_loss, ssim
    x, y = LB.loss_pair("uniform", (3, 67, 131), 72)

    def fn(t):
        clear_cache()
        a = t["x"].clone().requires_grad_(True)
        loss = photometric_loss(a, t["y"], 0.2)
        loss.backward()
        clear_cache()
        b = t["x"].clone().requires_grad_(True)
        l1, ss = l1_loss(b, t["y"]), ssim(b, t["y"])
        (0.8 * l1 + 0.2 * (1.0 - ss)).backward()
        clear_cache()
        return dict(loss=loss, grad=a.grad, l1=l1, ssim=ss, grad2=b.grad)
    late("1", "losses", dict(x=x, y=y), fn, exact=("loss", "grad", "l1", "ssim", "grad2"))


def test_1_normal_consistency_loss():
    from utils.loss_utils import normal_consistency_loss
    g = torch.Generator().manual_seed(9)
    H, W = 67, 131
    arrays = dict(rn=torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0).numpy(),
                  sn=torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0).numpy(), mask=(torch.rand(1, H, W, generator=g) < 0.7).float().numpy())

    def fn(t):
        rn, sn = t["rn"].clone().requires_grad_(True), t["sn"].clone().requires_grad_(True)
        loss = normal_consistency_loss(rn, sn, 0.05, t["mask"])
        (loss * 3.0).backward()
        return dict(loss=loss, g_rn=rn.grad, g_sn=sn.grad)
    late("1", "normal_consistency_loss", arrays, fn, exact=("loss", "g_rn", "g_sn"))


def test_1_surface_pass():
    import gaussian_renderer as gr
    import loss_bounds as LB
    H, W = 67, 131
    am, ray = LB.surface_scene(H, W, 70)
    rs = np.random.RandomState(H + W)
    arrays = dict(am=am, ray=ray, gsd=rs.randn(H, W).astype(np.float32), gsn=rs.randn(3, H, W).astype(np.float32))

    def fn(t):
        A = t["am"].clone().requires_grad_(True)
        sd, sn = gr._SurfacePass.apply(A, t["ray"], 0.3)
        ((sd[0] * t["gsd"]).sum() + (sn * t["gsn"]).sum()).backward()
        return dict(sd=sd, sn=sn, g=A.grad)
    late("1", "surface_pass", arrays, fn, exact=("sd", "sn", "g"))


def _train_tensors(P, seed):
    sc = S.make_scene(P, "S", seed=seed, mu=-3.2)
    tex, fail = S.make_cubemap(8, 3, seed)
    a = {k: sc[k] for k in PARAMS[:6]}
    a.update(cubemap=tex, fail=fail)
    return a


def test_1_flat_adam_step():
    from gsr_train import GaussianTrainState
    P = 4097
    arrays = _train_tensors(P, 12)
    n = sum((v.size + 3) // 4 * 4 for v in arrays.values())
    rs = np.random.RandomState(2)
    arrays.update(grad=rs.randn(n).astype(np.float32), m=rs.randn(n).astype(np.float32), v=rs.rand(n).astype(np.float32))

    def fn(t):
        st = GaussianTrainState({k: t[k] for k in PARAMS}, "cuda")
        assert st.params.total == n
        st.grads.flat.copy_(t["grad"])
        st.optimizer.exp_avg.copy_(t["m"])
        st.optimizer.exp_avg_sq.copy_(t["v"])
        st.optimizer.step_count = 17
        st.optimizer.step()
        return dict(params=st.params.flat, m=st.optimizer.exp_avg, v=st.optimizer.exp_avg_sq)
    late("1", "FlatAdam.step", arrays, fn, exact=("params", "m", "v"))


def test_1_densification_stats_and_densify_and_prune():
    """DensifyStats.update over two views, then densify_and_prune with the caller's noise.  (densify_and_prune reads counts back on its
    stream, so the host waits there for the late inputs; the statistics kernel has no host wait.)"""
    from gsr_densify import DensifyStats, densify_and_prune
    from gsr_train import GaussianTrainState
    P = 9001
    arrays = _train_tensors(P, 11)
    rs = np.random.RandomState(5)
    for i in range(2):
        arrays.update({"vg%d" % i: (rs.randn(P, 3) * 1e-3).astype(np.float32),
                       "radii%d" % i: (rs.rand(P) < 0.6).astype(np.int32) * rs.randint(1, 40, P).astype(np.int32),
                       "w%d" % i: (rs.rand(P) * (rs.rand(P) < 0.5)).astype(np.float32)})
    denom, dw = rs.randint(0, 5, P).astype(np.float32), rs.randint(0, 4, P).astype(np.float32)
    arrays["stats"] = np.stack([(rs.rand(P) * 8e-4 * denom).astype(np.float32), denom, (rs.rand(P) * 0.05 * dw).astype(np.float32), dw,
                                rs.randint(0, 60, P).astype(np.float32)])
    arrays["scales"] = np.log(np.exp(rs.randn(P, 2) * 1.2) * 0.03).astype(np.float32)
    arrays["noise"] = rs.randn(2 * P, 2).astype(np.float32)
    n = sum((arrays[k].size + 3) // 4 * 4 for k in PARAMS)
    arrays.update(m=rs.randn(n).astype(np.float32), v=rs.rand(n).astype(np.float32))
    k_split = []

    def fn(t):
        seen = DensifyStats(P, "cuda")
        for i in range(2):
            seen.update(t["vg%d" % i], t["radii%d" % i], t["w%d" % i])
        st = GaussianTrainState({k: t[k] for k in PARAMS}, "cuda")
        st.optimizer.exp_avg.copy_(t["m"])
        st.optimizer.exp_avg_sq.copy_(t["v"])
        stats = DensifyStats(P, "cuda")
        stats.buf.copy_(t["stats"])
        if not k_split:          # (the serial run comes first: the number of split parents sizes the caller's noise)
            k_split.append(densify_and_prune(st, stats, 0.0002, 0.05, torch.zeros(3), 3.0, 20)[2]["split"])
        new, new_stats, info = densify_and_prune(st, stats, 0.0002, 0.05, torch.zeros(3), 3.0, 20, noise=t["noise"][:2 * k_split[0]])
        assert info["split"] == k_split[0] > 20 and info["cloned"] > 20
        return dict(seen=seen.buf, params=new.params.flat, m=new.optimizer.exp_avg, v=new.optimizer.exp_avg_sq, new_stats=new_stats.buf)
    late("1", "densify", arrays, fn, exact=("seen", "params", "m", "v", "new_stats"), may_be_zero=("new_stats",))


@pytest.mark.parametrize("mode", ["RGB", "Depth", "Curvature"])
def test_1_present_view_and_the_8bit_frame(mode):
    """gsr_present_view: the float image and the uint8 frame; Depth and Curvature take the min/max slots in the per-stream scratch."""
    import viewer_ref as VR
    from utils import image_utils as IU
    m = VR.ITEMS.index(mode)
    family = "normals" if mode == "Curvature" else "smooth"
    assert VR.defined(family, VR.ITEMS, m, 64, 65)
    rgb, pkg = VR.package(family, 64, 65, 11)
    arrays = dict(pkg, rgb=rgb)

    def fn(t):
        pk = {k: v for k, v in t.items() if k != "rgb"}
        return dict(frame=IU.present_bytes(t["rgb"], pk, VR.ITEMS, m), image=IU.render_net_image(t["rgb"], pk, VR.ITEMS, m, None).clone())
    late("1", "present_view " + mode, arrays, fn, exact=("frame", "image"))


def test_1_metrics_table_normal_mae():
    import metrics_ref as MR
    from gsr_eval import MetricsTable
    H, W = 65, 64
    p, g = MR.normal_pair("random", H, W, 50)

    def fn(t):
        table = MetricsTable(2, "cuda")
        err = torch.full((H, W), -1.0, device="cuda")
        table.normals(0, t["p"], t["g"], error_map=err)
        return dict(rows=table.rows, err=err)
    late("1", "MetricsTable.normals", dict(p=p, g=g), fn, exact=("rows", "err"))
    row = _serial[("1", "MetricsTable.normals")]["rows"]
    assert row[0, 1] > 0 and row[0, 3] == H * W and np.isnan(row[1]).all()


# ============================================================================================== 2. interleaved views on one stream
@pytest.mark.parametrize("order", ["ABAB", "ABBA"])
@pytest.mark.parametrize("kind", ["S", "two_node_async", "fused_async", "G"])
def test_2_interleaved_views_on_one_stream(kind, order):
    """A.fwd, B.fwd, then the backwards in either order, all on the default stream: the one-stream baseline for the per-device flags (a
    forward that arms the gate, sorts early or records `done` between another view's forward and its backward).  two_node_async is S +
    deferred_reflection with forward keys and the tail on the side stream; fused_async adds the forward's early sort."""
    L = 16
    refs = {v: serial_view(kind, v, L) for v in "AB"}
    with drained():
        views = {v: KINDS[kind](v, L)[1](on_device(KINDS[kind](v, L)[0])) for v in "AB"}
        views["A"].fwd()
        views["B"].fwd()
        for v in ("AB" if order == "ABAB" else "BA"):
            views[v].bwd()
        got = {v: host(views[v].results()) for v in "AB"}
    for v in "AB":
        check("2", "%s %s view %s" % (kind, order, v), got[v], refs[v], **make_keys(kind))


# ============================================================================================== 3. B overtakes A on two streams
@pytest.mark.parametrize("L", SIZES)
@pytest.mark.parametrize("kind", ["fused", "fused_async", "two_node", "two_node_async"])
def test_3_view_b_overtakes_view_a_on_two_streams(kind, L):
    """sA: A.fwd, delay, A.bwd.  sB meanwhile: all of B.  Leaves and sinks are separate per view, so no backward waits for the other:
    the device runs A.fwd, B.fwd, B.bwd, A.bwd — an order one stream never produces (with the asynchronous tail: A.fwd, B.fwd, then both
    backwards through the one side stream; see the events below)."""
    refs = {v: serial_view(kind, v, L) for v in "AB"}
    sA, sB = streams(2)
    with drained():
        with torch.cuda.stream(sA):
            A = KINDS[kind]("A", L)[1](on_device(KINDS[kind]("A", L)[0]))
            A.fwd()
        SP.delay(sA)
        end_a, end_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(sA):
            A.bwd()
            end_a.record(sA)
        with torch.cuda.stream(sB):
            B = KINDS[kind]("B", L)[1](on_device(KINDS[kind]("B", L)[0]))
            B.fwd()
            fwd_b = torch.cuda.Event(enable_timing=True)
            fwd_b.record(sB)
            B.bwd()
            end_b.record(sB)
            rb = B.results()
        got_b = SP.fetch(sB, rb)
        with torch.cuda.stream(sA):
            ra = A.results()
        got_a = SP.fetch(sA, ra)
        torch.cuda.synchronize()
        lead, lead_fwd = end_b.elapsed_time(end_a), fwd_b.elapsed_time(end_a)
    # The schedule under test really happened: B's forward was over before A's backward, and without the asynchronous tail B's backward
    # too.  (A backward that came to block the host would run A.bwd before B is even enqueued, and this would silently become a serial
    # schedule.)  With the asynchronous tail B's backward cannot overtake: the library has ONE in-order side stream per device, A's tail
    # waits there for A's delayed pixel kernel, and B's tile backward waits at its gate for the side stream behind it.
    print("STREAMS 3 %s L=%d: view B's forward ended %.1f ms and its backward %.1f ms before view A's backward" % (kind, L, lead_fwd, lead))
    assert lead_fwd > 0, "view B's forward did not overtake view A's backward: the schedule under test did not happen"
    assert lead > 0 or kind.endswith("_async"), "view B's backward did not overtake view A's"
    check("3", "%s L=%d view B" % (kind, L), got_b, refs["B"], **make_keys(kind))
    check("3", "%s L=%d view A" % (kind, L), got_a, refs["A"], **make_keys(kind))


# ============================================================================================== 4. the --view-streams pattern
N_VIEWS = 5


def _batch_arrays(L):
    key = ("batch", L)
    if key not in _arrays:
        _, W, H, _, _, _ = VIEWS["A"]
        cams = S.circle_cameras(W, H, n=N_VIEWS)
        _arrays[key] = [refl_arrays("A", L, camera=c) for c in cams]
        _arrays[("batch-cams", L)] = cams           # (kept alive: refl_arrays keys them by identity)
    return _arrays[key]


def _batch_step(L, fused, side_streams, delay_first):
    """bench.py's step_into: a fork event; views round-robin over the streams; the first view overwrites one FlatGrads buffer and the
    later ones accumulate into it; each backward waits for the previous view's event; main waits for the last.  No side streams: the
    plain loop on the current stream.  delay_first: a delay between view 0's forward and its backward.  (In front of view 0's forward it
    would only hold the host, which waits in that forward for `num_rendered`: every forward blocks the host, so the views' forwards are
    always ENQUEUED in host order.)  Returns per-view forward outputs and the flat buffer's views, on the host."""
    from gsr_dist import FlatGrads
    batch = _batch_arrays(L)
    t0 = on_device(batch[0][0])
    p = {k: t0[k].clone().requires_grad_(True) for k in PARAMS}
    fg = FlatGrads(p)
    fg.flat.fill_(NAN)
    tensors = [on_device(a) for a, _ in batch]
    main = torch.cuda.current_stream()
    views, done, fwd_end = [], [], []
    if side_streams:
        fork = torch.cuda.Event()
        fork.record(main)
    for i, (t, (_, cam)) in enumerate(zip(tensors, batch)):
        v = ReflView(t, cam, fused, True, shared=(p, fg, i > 0))
        views.append(v)
        if not side_streams:
            v.fwd()
            v.bwd()
            continue
        st = side_streams[i % len(side_streams)]
        if i < len(side_streams):
            st.wait_event(fork)
        with torch.cuda.stream(st):
            v.fwd()
            fwd_end.append(torch.cuda.Event(enable_timing=True))
            fwd_end[-1].record(st)
        if i == 0 and delay_first:
            SP.delay(st)                 # view 0's backward is late: the other streams' forwards overtake it, the chained backwards queue behind it
        with torch.cuda.stream(st):
            if done:
                st.wait_event(done[-1])
            v.bwd()
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(st)
            done.append(ev)
    if side_streams:
        main.wait_event(done[-1])
    fg.all_reduce()                      # (no process group: only FlatGrads' join of the library's side stream, as bench.py's step does)
    got = SP.fetch(main, dict({"g_" + k: fg.view(k) for k in PARAMS}, **{"%s%d" % (k, i): v.out[k] for i, v in enumerate(views) for k in ReflView.FORWARD}))
    if side_streams and delay_first:
        torch.cuda.synchronize()
        # the forwards of the views on the other streams ran before view 0's backward was over: the schedule under test happened
        leads = [fwd_end[i].elapsed_time(done[0]) for i in range(1, len(side_streams))]
        print("STREAMS 4 forwards of views 1..%d ended %s ms before view 0's backward" % (len(leads), ", ".join("%.1f" % x for x in leads)))
        assert all(x > 0 for x in leads), leads
    return got


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two_node"])
@pytest.mark.parametrize("n_streams", [2, 3])
def test_4_view_streams_batch_equals_the_one_stream_loop(n_streams, fused):
    L = 16
    key = ("batch", L, fused)
    if key not in _serial:
        with drained():
            _serial[key] = _batch_step(L, fused, [], False)
    ref = _serial[key]
    with drained():
        got = _batch_step(L, fused, streams(n_streams), True)
    check("4", "%d streams %s" % (n_streams, "fused" if fused else "two_node"), got, ref,
          exact=tuple("%s%d" % (k, i) for i in range(N_VIEWS) for k in ReflView.FORWARD), atomic=tuple("g_" + k for k in PARAMS[:6]),
          sink=("g_cubemap", "g_fail"))


# ============================================================================================== 5. one camera, two streams
RENDER_KEYS = ("render", "rend_normal", "refl_color_map", "base_color_map", "rend_alpha", "surf_depth", "surf_normal", "refl_strength_map")


def _render(t, cam):
    """gaussian_renderer.render() under no_grad: the fused path takes the camera block, the surface pass the ray block."""
    from gaussian_renderer import render
    from test_gpu_dropin import _Pipe
    PC, View = _model_and_view(t, cam)
    with torch.no_grad():
        pkg = render(View, PC, _Pipe, t["bg"])
    return {k: pkg[k] for k in RENDER_KEYS}


@pytest.mark.parametrize("pair", ["first_on_a_delayed_stream", "built_on_a_stream_hit_on_the_default_stream"])
def test_5_one_camera_on_two_streams(pair):
    """The camera and ray blocks are cached per camera tensors and built with torch ops on the stream current at first use; a later hit
    returns the block on whichever stream is current then.  Fresh camera tensors (the cache misses), the first render on one stream, at
    once a second render with the SAME camera tensors on another: both equal the serial render bit for bit.  The second render is
    ordered behind the block's construction by an event the block carries (gaussian_renderer._Block)."""
    arrays, cam = refl_arrays("A", 16)
    ref = serial(("5", "render"), arrays, lambda t: _render(t, cam))
    sA, sB = streams(2)
    with drained():
        t = on_device(arrays)                # fresh camera tensors, ready for every stream
        torch.cuda.synchronize()
        if pair == "first_on_a_delayed_stream":
            first, second = sA, sB
            SP.delay(sA)
        else:
            first, second = sB, torch.cuda.default_stream()
        with torch.cuda.stream(first):
            r1 = _render(t, cam)
        with torch.cuda.stream(second):
            r2 = _render(t, cam)
        got2 = SP.fetch(second, r2)
        got1 = SP.fetch(first, r1)
    check("5", pair + " first", got1, ref, exact=RENDER_KEYS)
    check("5", pair + " second", got2, ref, exact=RENDER_KEYS)


def test_5_a_block_built_without_a_host_wait_is_ordered_for_a_second_stream():
    """The same cache with a builder that never blocks the host, so that the window is the whole delay instead of a few microseconds
    (the camera block's builder uploads K^-1 synchronously and the ray block's inverts on the device, which reads a status back: both
    drain the building stream before their last few ops).  Built on sA behind a delay, hit on sB at once: without the block's event sB
    reads the poison."""
    import gaussian_renderer as gr
    sA, sB = streams(2)
    want = np.arange(33, dtype=np.float32) * 2
    with drained():
        src = torch.arange(33, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def build():
            value = torch.full((33,), NAN, device="cuda")
            sA.synchronize()                 # the poison is in memory
            SP.delay(sA)
            value.copy_(src * 2)
            return value
        try:
            with torch.cuda.stream(sA):
                built = gr._cached_block("stream-probe", (src,), 0, build)
            with torch.cuda.stream(sB):
                hit = gr._cached_block("stream-probe", (src,), 0, build)
                assert hit is built
                seen = hit.clone()
            got_b = SP.fetch(sB, {"v": seen})["v"]
            got_a = SP.fetch(sA, {"v": built})["v"]
        finally:
            gr._blocks.pop("stream-probe", None)
    assert SP.same_bits(got_a, want)
    assert SP.same_bits(got_b, want), "the second stream read the block before the building stream had written it"


def test_5_a_cached_block_orders_each_new_stream_once():
    """The block's event: a hit from the building stream or from a stream already ordered behind it adds nothing; a hit from a new
    stream waits once and is remembered."""
    import gaussian_renderer as gr
    cam = camera_of("B")
    sA, sB = streams(2)
    with drained():
        ct = on_device({k: np.ascontiguousarray(cam[k]) for k in ("viewmatrix", "R", "T")})
        torch.cuda.synchronize()
        args = (ct["viewmatrix"], (64, 96, cam["K"]), ct["R"], ct["T"])
        with torch.cuda.stream(sA):
            block = gr._cam_block(*args)
        entry = gr._blocks["cam"][-1]
        assert entry.value is block and entry.ordered == {sA.cuda_stream}
        with torch.cuda.stream(sA):
            assert gr._cam_block(*args) is block and entry.ordered == {sA.cuda_stream}
        with torch.cuda.stream(sB):
            assert gr._cam_block(*args) is block
        assert entry.ordered == {sA.cuda_stream, sB.cuda_stream}
        with torch.cuda.stream(sB):
            assert gr._cam_block(*args) is block
        assert gr._blocks["cam"][-1] is entry and len(entry.ordered) == 2


# ============================================================================================== 6. allocator reuse behind the tail
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two_node"])
def test_6_scratch_is_not_reused_before_the_asynchronous_tail_is_over(fused):
    """On sA a backward with async_tail=True into a sink, held behind a delay so that its tail is still pending; every reference to its
    outputs and graph dropped.  Under sB, and after side_join() on the default stream also under sA — the stream the scratch was allocated
    on, whose pool the caching allocator returns it to —, tensors of the scratch's sizes are allocated and filled with NaN at once.  The
    sink, read on the default stream behind side_join(), equals the serial run: `_gsr._side_held` kept the scratch until the join and the
    join ordered sA behind the tail."""
    import _gsr
    L = 128
    kind = "fused_async" if fused else "two_node_async"
    ref = serial_view(kind, "A", L)
    arrays, make = KINDS[kind]("A", L)
    _, W, H, _, _, _ = VIEWS["A"]
    sizes = (int(_gsr.lib.gsr_deferred_reflection_scratch_floats(L, W, H, 1)), H * W)
    sA, sB = streams(2)

    def refill():
        return [torch.full((n,), NAN, dtype=torch.float32, device="cuda") for n in sizes for _ in range(2)]
    with drained():
        with torch.cuda.stream(sA):
            v = make(on_device(arrays))
            v.fwd()
        SP.delay(sA)
        with torch.cuda.stream(sA):
            v.bwd()
        fg = v.fg
        v.out = v.t = v.p = None
        del v
        assert _gsr._side_held.get(torch.cuda.current_device()), "nothing is held for the side stream: the tail did not take this path"
        with torch.cuda.stream(sB):
            junk = refill()
        _gsr.side_join()
        with torch.cuda.stream(sA):
            junk += refill()
        got = SP.fetch(torch.cuda.default_stream(), {"g_" + k: fg.view(k) for k in ("cubemap", "fail")})
    check("6", kind, got, ref, sink=("g_cubemap", "g_fail"))
