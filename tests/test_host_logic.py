"""Host-side logic of the drop-in packages that runs without a GPU: argument validation mirrors the reference's
wrappers (same exceptions, same messages), settings tuples have the reference's fields, synthetic data is seeded."""
import os
import sys

import numpy as np
import pytest
import torch

import gsr_synth as S


def test_settings_fields_match_reference(hip_lib_built):
    from diff_surfel_rasterization import GaussianRasterizationSettings as SS
    from diff_gaussian_rasterization import GaussianRasterizationSettings as GS
    base = ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix", "sh_degree",
            "campos", "prefiltered", "debug")
    assert SS._fields == base                      # DSR __init__.py:170-182
    assert GS._fields == base + ("antialiasing",)  # DGR __init__.py:157-170


def _settings(cls, **extra):
    z = torch.zeros(3)
    return cls(image_height=8, image_width=8, tanfovx=0.5, tanfovy=0.5, bg=z, scale_modifier=1.0, viewmatrix=torch.eye(4),
               projmatrix=torch.eye(4), sh_degree=0, campos=z, prefiltered=False, debug=False, **extra)


def test_surfel_rasterizer_argument_errors(hip_lib_built):
    from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    r = GaussianRasterizer(_settings(GaussianRasterizationSettings))
    m = torch.zeros(4, 3)
    with pytest.raises(Exception, match="either SHs or precomputed colors"):
        r(means3D=m, means2D=m, opacities=torch.zeros(4, 1))                      # neither
    with pytest.raises(Exception, match="either SHs or precomputed colors"):
        r(means3D=m, means2D=m, opacities=torch.zeros(4, 1), shs=torch.zeros(4, 16, 3), colors_precomp=torch.zeros(4, 3))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(means3D=m, means2D=m, opacities=torch.zeros(4, 1), shs=torch.zeros(4, 16, 3))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(means3D=m, means2D=m, opacities=torch.zeros(4, 1), shs=torch.zeros(4, 16, 3), scales=torch.zeros(4, 2),
          rotations=torch.zeros(4, 4), cov3D_precomp=torch.zeros(4, 9))
    # CPU tensors are refused like CHECK_INPUT does (DSR rasterize_points.cu:27-28); nothing reaches the device
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        r(means3D=m, means2D=m, opacities=torch.zeros(4, 1), shs=torch.zeros(4, 16, 3), refl_strengths=torch.zeros(4, 1),
          scales=torch.zeros(4, 2), rotations=torch.zeros(4, 4))


def test_gauss_rasterizer_argument_errors(hip_lib_built):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    r = GaussianRasterizer(_settings(GaussianRasterizationSettings, antialiasing=False))
    m = torch.zeros(4, 3)
    with pytest.raises(Exception, match="either SHs or precomputed colors"):
        r(means3D=m, means2D=m, opacities=torch.zeros(4, 1))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(means3D=m, means2D=m, opacities=torch.zeros(4, 1), colors_precomp=torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="means3D must have dimensions"):
        from diff_gaussian_rasterization import _C
        _C.rasterize_gaussians(torch.zeros(3), torch.zeros(4), *([torch.zeros(0)] * 6), 1.0, torch.zeros(0), torch.eye(4), torch.eye(4),
                               0.5, 0.5, 8, 8, torch.zeros(0), 0, torch.zeros(3), False, False, False)


def test_output_taps_are_a_surfel_only_extension(hip_lib_built):
    from diff_gaussian_rasterization import GaussianRasterizationSettings as SG, GaussianRasterizer as RG
    from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    r = GaussianRasterizer(_settings(GaussianRasterizationSettings))
    r.set_output_taps(("normal_view",))
    r.set_output_taps(())
    with pytest.raises(NotImplementedError, match="no output tap"):
        r.set_output_taps(("depth",))
    with pytest.raises(NotImplementedError, match="no output tap"):
        RG(_settings(SG, antialiasing=False)).set_output_taps(("normal_view",))


def test_cubemap_encoder_host_side(hip_lib_built):
    from cubemapencoder import CubemapEncoder
    enc = CubemapEncoder(output_dim=3, resolution=8)
    assert enc.params["Cubemap_texture"].shape == (6, 3, 8, 8) and enc.params["Cubemap_failv"].shape == (3,)
    assert enc.n_elems == 6 * 3 * 8 * 8 + 3 and enc.seamless == 1 and enc.interp_id == 1
    assert -0.5 <= float(enc.params["Cubemap_texture"].min()) and float(enc.params["Cubemap_texture"].max()) <= 0.5
    enc.resize(16)                                                            # reference cubemap_encoder.py:102-105
    assert enc.params["Cubemap_texture"].shape == (6, 3, 16, 16) and enc.resolution == 16
    enc.filter(torch.sigmoid, lambda x: torch.log(x / (1 - x)))               # :107-113 (sharpen in activated space)
    assert torch.isfinite(enc.params["Cubemap_texture"]).all()
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        enc(torch.randn(4, 3))                                                # CHECK_CUDA of cubemapencoder.cu:23


def test_adjust_sharpness_identity_and_borders(hip_lib_built):
    from cubemapencoder.cubemap_encoder import _adjust_sharpness
    x = torch.rand(6, 3, 9, 9)
    assert torch.allclose(_adjust_sharpness(x, 1.0), x)          # factor 1 = original image
    y = _adjust_sharpness(x, 2.0)
    assert torch.equal(y[..., 0, :], x[..., 0, :]) and torch.equal(y[..., :, -1], x[..., :, -1])   # borders untouched


def test_synthetic_scene_is_seeded_and_shaped():
    a = S.make_scene(1000, "S", seed=1003, mu=-4.75)
    b = S.make_scene(1000, "S", seed=1003, mu=-4.75)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    assert a["scales"].shape == (1000, 2) and S.make_scene(10, "G")["scales"].shape == (10, 3)
    assert a["shs"].shape == (1000, 16, 3) and a["env_scope_mask"].dtype == bool
    np.testing.assert_allclose(np.linalg.norm(a["rotations"], axis=1), 1.0, atol=1e-5)
    assert (a["means3D"][:20, 2] <= 0.3).all()          # 2 % near-plane points exercise the cull
    cams = S.circle_cameras(64, 48, n=8)
    assert len(cams) == 8
    for c in cams:
        # every circle camera looks at the origin: the origin projects to the image centre
        o = np.array([0, 0, 0, 1.0], np.float32) @ c["projmatrix"]
        np.testing.assert_allclose(o[:2] / o[3], 0.0, atol=1e-5)


def test_flat_grads_views_and_accumulation():
    from gsr_dist import FlatGrads
    p = {"a": torch.zeros(5, 3, requires_grad=True), "b": torch.zeros(4, requires_grad=True)}
    fg = FlatGrads(p)
    ((p["a"] * 2).sum() + (p["b"] * 3).sum()).backward()
    # every slice starts on a 16-byte boundary (float4 stores of the backward kernels into sink views): "a" (15 floats) is padded to 16
    assert fg.slices == {"a": (0, 15), "b": (16, 20)} and fg.flat.numel() == 20
    assert torch.equal(fg.view("a"), torch.full((5, 3), 2.0)) and torch.equal(fg.view("b"), torch.full((4,), 3.0)) and fg.flat[15] == 0
    ((p["a"] * 1).sum()).backward()                      # accumulates in place into the same buffer
    assert torch.equal(fg.view("a"), torch.full((5, 3), 3.0))
    fg.all_reduce()                                      # no process group: no-op
    fg.zero_()
    assert float(fg.flat.abs().sum()) == 0 and p["a"].grad.data_ptr() == fg.flat.data_ptr()


def test_bench_refuses_a_world_size_that_differs_from_gpus():
    """bench.py: `--gpus 4` inside a torchrun environment of another size exits with status 2 before any GPU call (runs here, without a GPU);
    round 2's bench silently measured one GPU in that situation."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "4"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert p.returncode == 2 and "--gpus 4" in p.stderr and "WORLD_SIZE=2" in p.stderr and not p.stdout.strip()


def test_bench_dump_outputs_is_a_fixed_bounded_sample(tmp_path):
    """bench.py --dump-outputs: float32 files under the 64 MiB budget; small arrays whole, large ones as the same seeded sample of elements on
    every call (two builds of the project compare output for output)."""
    import bench
    g = torch.Generator().manual_seed(0)
    arrays = {"final": torch.rand(3, 540, 960, generator=g), "radii": torch.randint(0, 300, (1_000_000,), dtype=torch.int32, generator=g),
              "grad_fail": torch.randn(3, generator=g)}
    arrays.update({"big%d" % i: torch.rand(4_000_000, generator=g) for i in range(40)})
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), arrays)
    bench.dump_outputs(str(b), arrays)
    names = sorted(p.name for p in a.iterdir())
    assert names == sorted(k + ".npy" for k in arrays)
    assert sum((a / n).stat().st_size for n in names) <= 64 * 2 ** 20
    for n in names:
        x = np.load(a / n)
        assert x.dtype == np.float32 and x.ndim == 1 and np.array_equal(x, np.load(b / n))
    assert np.array_equal(np.load(a / "grad_fail.npy"), arrays["grad_fail"].numpy())
    r = np.load(a / "radii.npy")
    assert 0 < r.size < 1_000_000 and np.isin(r, arrays["radii"].numpy().astype(np.float32)).all()


def test_surfel_backward_takes_an_empty_scene_with_sh_input(hip_lib_built):
    """An empty scene's SH tensor is (0, M, 3): the backward binding keeps M for its gradient (a FlatGrads sink has that shape) and does
    not mistake it for the 1-D placeholder of an omitted input.  Past those checks the CPU tensors are refused."""
    from diff_surfel_rasterization import _C
    z = torch.empty(0)
    args = lambda sh: (z, torch.empty(0, 3), z, z, z, torch.empty(0, 2), torch.empty(0, 4), 1.0, z, z, z, 1.0, 1.0, torch.zeros(3, 4, 4),
                       torch.zeros(8, 4, 4), None, sh, 3, z, z, 0, z, z, False)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C.rasterize_gaussians_backward(*args(torch.empty(0, 16, 3)), unused=("colors",), grad_sink={"shs": torch.empty(0, 16, 3)})
    with pytest.raises(ValueError, match="'colors' needs shs as the colour input"):
        _C.rasterize_gaussians_backward(*args(z), unused=("colors",))


# ------------------------------------------------------------------ _raster_api.call_forward / call_backward over a fake _C module
class _FakeC:
    """Stands in for a package's `_C`: CPU tensors in, tensors of the right arity out, every call recorded."""
    NAMES = ("means3D", "means2D", "sh", "colors_precomp", "opacities", "scales", "cov3Ds_precomp")

    def __init__(self, P=3, fail=None):
        self.calls, self.fail = [], fail
        shapes = dict(means3D=(P, 3), means2D=(P, 3), sh=(P, 1, 3), colors_precomp=(P, 3), opacities=(P, 1), scales=(P, 2), cov3Ds_precomp=(P, 9))
        self.grads = {n: torch.full(shapes[n], float(i + 1)) for i, n in enumerate(self.NAMES)}
        self.P = P

    def rasterize_gaussians(self, *args, **kw):
        self.calls.append(("fw", args, kw))
        if self.fail == "fw":
            raise RuntimeError("fake forward failed")
        z = torch.zeros(4, dtype=torch.uint8)
        return 7, torch.ones(3, 2, 2), torch.ones(self.P, dtype=torch.int32), z, z.clone(), z.clone()

    def rasterize_gaussians_backward(self, *args, **kw):
        self.calls.append(("bw", args, kw))
        if self.fail == "bw":
            raise RuntimeError("fake backward failed")
        return tuple(self.grads[n] for n in self.NAMES)


def _fake_variant(c, snapshot_on_debug=True):
    from _raster_api import Variant
    names = _FakeC.NAMES

    def split_forward(ret):
        n, color, radii, geom, binning, img = ret
        return n, (color, radii), (geom, binning, img), radii
    return Variant(
        c_module=c, extra_settings=(), tensors=names, settings_pos=4, forward_kwargs=(), module_to_apply={},
        placeholder=lambda name, device: torch.empty(0), pack_forward=lambda t, s: tuple(t[n] for n in names) + (s.debug,),
        split_forward=split_forward, nondiff_outputs=(1,), saved=("means3D", "sh", "colors_precomp", "scales", "cov3Ds_precomp"),
        pack_backward=lambda saved, s, grads, num_rendered, buffers, radii: (saved["means3D"], grads[0], num_rendered, radii) + tuple(buffers),
        grads_of=lambda ret: dict(zip(names, ret)), optional_grads=("sh", "colors_precomp", "scales", "cov3Ds_precomp"),
        sinkable={"means3D": "means3D", "sh": "shs", "opacities": "opacities"},
        skippable={"colors_precomp": "colors", "cov3Ds_precomp": "cov3D"}, snapshot_on_debug=snapshot_on_debug)


def _fake_inputs(c, omitted):
    """The fake variant's tensors by name (P = 3), an empty placeholder for each name in `omitted`; all require grad."""
    return {n: (torch.empty(0) if n in omitted else torch.rand(c.grads[n].shape)).requires_grad_(True) for n in _FakeC.NAMES}


# (inputs passed as empty placeholders, sink keys, accumulate) -> (the `unused` keyword or None, tensor names whose gradient is None)
_PLUMBING_CASES = [
    (("colors_precomp", "scales"), None, False, ("colors",), {"colors_precomp", "scales"}),
    (("sh", "scales"), None, False, None, {"sh", "scales"}),
    (("colors_precomp", "cov3Ds_precomp"), ("means3D", "shs"), True, ("colors", "cov3D"), {"colors_precomp", "cov3Ds_precomp", "means3D", "sh"}),
    (("sh", "cov3Ds_precomp"), (), False, ("cov3D",), {"sh", "cov3Ds_precomp"}),          # a sink without tensors (taps only)
]


def _check_backward_call(c, sink_keys, accumulate, unused, sink_tensors):
    kind, _, kw = c.calls[-1]
    assert kind == "bw"
    assert kw.get("unused") == unused and ("unused" in kw) == (unused is not None)
    if sink_keys:
        assert kw["grad_sink"] == sink_tensors and kw["accumulate"] is accumulate
    else:
        assert "grad_sink" not in kw and "accumulate" not in kw


@pytest.mark.parametrize("omitted,sink_keys,accumulate,unused,none_grads", _PLUMBING_CASES)
def test_call_backward_keywords_and_gradient_filter(omitted, sink_keys, accumulate, unused, none_grads):
    from _raster_api import GradSink, build_api, call_backward
    c = _FakeC()
    v = _fake_variant(c)
    Settings, _, rasterize_gaussians, _ = build_api(v)
    settings = _settings(Settings)
    sink_tensors = {k: torch.zeros(1) for k in sink_keys or ()}
    sink = None if sink_keys is None else GradSink(sink_tensors, accumulate)
    # through the autograd node of build_api
    t = _fake_inputs(c, omitted)
    args = [t[n] for n in v.tensors]
    args.insert(v.settings_pos, settings)
    color, radii = rasterize_gaussians(*args, grad_sink=sink)
    assert c.calls[-1][0] == "fw" and c.calls[-1][2] == {} and not radii.requires_grad
    color.sum().backward()
    _check_backward_call(c, sink_keys, accumulate, unused, sink_tensors)
    for n in v.tensors:
        assert (t[n].grad is None) if n in none_grads else torch.equal(t[n].grad, c.grads[n]), n
    # the function alone
    saved = {n: t[n].detach() for n in v.saved}
    z = torch.zeros(4, dtype=torch.uint8)
    out = call_backward(v, saved, settings, [torch.ones(3, 2, 2), None], 7, (z, z, z), radii, sink, extra_normal_grad="tap")
    _check_backward_call(c, sink_keys, accumulate, unused, sink_tensors)
    assert c.calls[-1][2]["extra_normal_grad"] == "tap" and c.calls[-1][1][2] == 7
    assert isinstance(out, list) and len(out) == len(v.tensors)
    for n, g in zip(v.tensors, out):
        assert (g is None) if n in none_grads else (g is c.grads[n]), n


@pytest.mark.parametrize("debug,snapshot_on_debug", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("fail", ["fw", "bw"])
def test_debug_snapshot_is_written_by_the_shared_calls(tmp_path, monkeypatch, fail, debug, snapshot_on_debug):
    """settings.debug with Variant.snapshot_on_debug: a _C call that raises leaves host copies of its arguments in snapshot_fw.dump /
    snapshot_bw.dump in the working directory and the exception propagates — through the autograd node and through the functions alone."""
    from _raster_api import build_api, call_backward, call_forward
    monkeypatch.chdir(tmp_path)
    c = _FakeC(fail=fail)
    v = _fake_variant(c, snapshot_on_debug)
    Settings, _, rasterize_gaussians, _ = build_api(v)
    settings = _settings(Settings)._replace(debug=debug)
    t = _fake_inputs(c, ("colors_precomp", "cov3Ds_precomp"))
    args = [t[n] for n in v.tensors]
    args.insert(v.settings_pos, settings)
    dump = tmp_path / ("snapshot_%s.dump" % fail)
    z = torch.zeros(4, dtype=torch.uint8)
    direct = ((lambda: call_forward(v, t, settings)) if fail == "fw" else
              (lambda: call_backward(v, {n: t[n].detach() for n in v.saved}, settings, [torch.ones(3, 2, 2), None], 7, (z, z, z), z, None)))
    through_node = (lambda: rasterize_gaussians(*args)) if fail == "fw" else (lambda: rasterize_gaussians(*args)[0].sum().backward())
    for run in (through_node, direct):
        with pytest.raises(RuntimeError, match="fake (forward|backward) failed"):
            run()
        assert dump.exists() == (debug and snapshot_on_debug)
        assert sorted(p.name for p in tmp_path.iterdir()) == ([dump.name] if debug and snapshot_on_debug else [])
        if dump.exists():
            kept = torch.load(dump)
            assert len(kept) == len(c.calls[-1][1]) and torch.equal(kept[0], t["means3D"].detach())
            dump.unlink()


def test_sink_tensor_check_is_one_helper(hip_lib_built):
    """_gsr.check_sink_tensor: shape, float32, contiguous, device, and the 16-byte alignment as a switch; every refusal is a ValueError that
    names the sink.  grad_allocator asks for alignment, the reflection's sinks do not."""
    import _gsr
    cpu = torch.device("cpu")
    good = torch.zeros(3, 4)
    misaligned = torch.zeros(13)[1:].view(3, 4)
    assert misaligned.is_contiguous() and misaligned.data_ptr() % 16 == 4
    _gsr.check_sink_tensor("grad sink", "rotations", good, (3, 4), cpu, aligned=True)
    bad = {"shape": torch.zeros(4, 3), "dtype": torch.zeros(3, 4, dtype=torch.float64), "view": torch.zeros(4, 3).T,
           "device": torch.zeros(3, 4, device="meta")}
    assert not bad["view"].is_contiguous() and bad["view"].shape == (3, 4)
    for aligned in (True, False):
        for t in bad.values():
            with pytest.raises(ValueError, match=r"^reflection grad sink 'rotations': expected contiguous float32 \(3, 4\) on cpu"):
                _gsr.check_sink_tensor("reflection grad sink", "rotations", t, (3, 4), cpu, aligned=aligned)
    with pytest.raises(ValueError, match=r"^grad sink 'rotations': storage must be 16-byte aligned"):
        _gsr.check_sink_tensor("grad sink", "rotations", misaligned, (3, 4), cpu, aligned=True)
    _gsr.check_sink_tensor("grad sink", "rotations", misaligned, (3, 4), cpu, aligned=False)
    # grad_allocator: the sink tensor itself where there is one, checked with alignment on; mk0 otherwise
    mk = _gsr.grad_allocator({"rotations": good, "shs": misaligned}, cpu, torch.empty)
    assert mk((3, 4), "rotations") is good and mk((3, 4), "scales").shape == (3, 4) and mk((2,)).shape == (2,)
    with pytest.raises(ValueError, match="^grad sink 'shs': storage must be 16-byte aligned"):
        mk((3, 4), "shs")
    with pytest.raises(ValueError, match="^grad sink 'rotations': expected contiguous float32"):
        mk((4, 4), "rotations")


def test_reflection_sink_checks_keep_their_order(hip_lib_built):
    """_reflection_backward refuses a bad sink before any library call (CPU tensors get that far): the accumulate check, then the tensor
    checks without an alignment requirement, then the async_tail check."""
    import gaussian_renderer as GR
    from _raster_api import GradSink
    img = torch.zeros(3, 2, 2)
    cm, fv = torch.zeros(6, 3, 2, 2), torch.zeros(3)
    saved = (img, img, torch.zeros(1, 2, 2), cm, fv, torch.zeros(33), torch.zeros(96))
    run = lambda tensors, **kw: GR._reflection_backward(saved, (img, None, None), GradSink(tensors, **kw), None)
    with pytest.raises(ValueError, match="^reflection grad sink: accumulate=True needs both"):
        run({"cubemap": torch.zeros(5)}, accumulate=True, async_tail=True)
    with pytest.raises(ValueError, match="^reflection grad sink 'cubemap': expected contiguous float32"):
        run({"cubemap": torch.zeros(5)}, async_tail=True)
    with pytest.raises(ValueError, match="^reflection grad sink 'fail': expected contiguous float32"):
        run({"cubemap": torch.zeros_like(cm), "fail": torch.zeros(3, dtype=torch.float64)}, accumulate=True, async_tail=True)
    misaligned_cm = torch.zeros(cm.numel() + 1)[1:].view(cm.shape)
    assert misaligned_cm.data_ptr() % 16 == 4
    with pytest.raises(ValueError, match="^reflection grad sink: async_tail=True needs both"):
        run({"cubemap": misaligned_cm}, async_tail=True)          # the misaligned plane passed its check
