"""CPU: the targeted deferred-reflection inputs of tests/helpers_refl.py land in the lookup class they were made for, at the margin they
were placed at, for every cubemap size the GPU tests run (tests/test_gpu_refl_seams.py)."""
import numpy as np
import pytest

import helpers_refl as R

SIZES = [1, 2, 3, 16, 104, 105, 128, 209, 210, 418, 419, 1024]
W, H = R.SEAM_W, R.SEAM_H
seam_camera = R.seam_camera


@pytest.mark.parametrize("L", SIZES)
def test_targets_land_in_their_class(L):
    cam = seam_camera()
    t = R.make_targets(cam, W, H, L, seed=L)
    kind, want = t["kind"], t["want"]
    cls, face, flag, margin, lu, lv = R.classify_image(t["nv"], cam, W, H, L)
    dl = R.delta(L)
    counts = {R.KIND_NAMES[k]: int((kind == k).sum()) for k in range(len(R.KIND_NAMES))}

    def placed(k, c):
        s = kind == k
        assert (cls[s] == c).all(), (R.KIND_NAMES[k], np.unique(cls[s]))
        assert (margin[s] >= 4 * dl).all(), (R.KIND_NAMES[k], float(margin[s].min()), dl)
        return s
    if L >= 2:
        placed(R.K_INTERIOR, R.INTERIOR)
        s = placed(R.K_BORDER, R.INTERIOR)
        near = np.minimum(np.abs(lu - 0.5 - np.round(lu - 0.5)), np.abs(lv - 0.5 - np.round(lv - 0.5)))
        assert (near[s] <= 8 * dl + 1 / 32 + 1e-3).all()
        s = placed(R.K_RIM, R.RIM)
        assert (R.edge_id(face[s], flag[s]) == want[s]).all()
        assert np.bincount(want[s], minlength=24).min() >= 16
    else:
        assert counts["rim"] == 0 and counts["interior"] == 0 and counts["near_border"] == 0
        assert (cls[kind == R.K_RANDOM] == R.VERTEX).all()        # L = 1: every footprint is a cube vertex
    s = placed(R.K_VERTEX, R.VERTEX)
    assert (R.corner_id(face[s], flag[s]) == want[s]).all()
    assert np.bincount(want[s], minlength=24).min() >= 16
    s = kind == R.K_CENTRE
    if L % 2 == 0:
        placed(R.K_CENTRE, R.INTERIOR)
    else:
        assert (margin[s] < dl).all()        # L/2 is a cell border (a rim threshold at L = 1)
    for k in R.AMBIGUOUS_KINDS:
        s = kind == k
        assert s.sum() >= 32 and (margin[s] < dl).all(), (R.KIND_NAMES[k], float(margin[s].max()))
    s = placed(R.K_ZERO, cls[kind == R.K_ZERO])
    assert s.sum() == 64 and not t["nv"].reshape(3, -1)[:, s].any()
    s = kind == R.K_TINY
    assert s.sum() == 128 and (margin[s] >= 4 * dl).all()
    n = np.linalg.norm(t["nv"].reshape(3, -1)[:, s].astype(np.float64), axis=0)
    assert n.min() >= 0.99e-7 and n.max() <= 1.01e-4
    assert (cls != R.FAIL).all()
    # the random band: what random normals give
    s = kind == R.K_RANDOM
    assert s.sum() > 5000


@pytest.mark.parametrize("L", [1, 2, 16, 1024])
def test_classifier_round_trip_and_pushes(L):
    """direction_of inverts cube_coords; pushed_normals move a pixel's direction by the promised texel offsets and nowhere else."""
    rng = np.random.default_rng(7)
    face = rng.integers(0, 6, 4000)
    lu, lv = rng.random(4000) * L, rng.random(4000) * L
    f2, lu2, lv2, _, _ = R.cube_coords(R.direction_of(face, lu, lv, L) * rng.uniform(0.1, 3, (4000, 1)), L)
    keep = np.minimum(np.minimum(lu, L - lu), np.minimum(lv, L - lv)) > 1e-9 * L
    assert (f2[keep] == face[keep]).all()
    np.testing.assert_allclose(lu2, lu, atol=1e-12 * L)
    np.testing.assert_allclose(lv2, lv, atol=1e-12 * L)
    cam = seam_camera()
    t = R.make_targets(cam, W, H, L, seed=3)
    amb = np.nonzero(np.isin(t["kind"], R.AMBIGUOUS_KINDS))[0]
    base = R.chain_dirs(t["nv"], cam, W, H)
    faces_seen = set()
    for i, img in enumerate(R.pushed_normals(t["nv"], cam, W, H, L, amb)):
        r = R.chain_dirs(img, cam, W, H)
        other = np.setdiff1d(np.arange(W * H), amb)
        assert np.array_equal(r[other], base[other])
        _, _, _, mg, _, _ = R.classify(r[amb], L)
        # a push keeps the normal's orientation (n and -n reflect alike, their gradients differ in sign)
        assert ((img.reshape(3, -1)[:, amb] * t["nv"].reshape(3, -1)[:, amb]).sum(axis=0) > 0).all()
        if i in (0, 2, 5, 7):                       # the diagonal pushes leave every discontinuity behind
            assert (mg >= 0.2 * R.delta(L)).all(), (i, float(mg.min()))
        faces_seen |= set(zip(amb.tolist(), R.cube_coords(r[amb], L)[0].tolist()))
    # an exact cube vertex is pushed onto all three of its faces, an exact edge onto both of its faces
    per_px = {}
    for p, f in faces_seen:
        per_px.setdefault(p, set()).add(f)
    k = t["kind"]
    assert all(len(per_px[p]) == 3 for p in amb if k[p] == R.K_CORNER)
    assert all(len(per_px[p]) >= 2 for p in amb if k[p] == R.K_EDGE)


def test_envelope_check_bounds_ambiguous_normal_gradients():
    """The envelope check on ambiguous pixels takes its floor from the pixel's |normal| decade: the reference passes, and a normal gradient
    one envelope-magnitude beyond the envelope fails on every ambiguous pixel — tiny normals elsewhere in the image (gradients ~1e6 times
    larger) do not widen it."""
    L = 16
    inp = R.seam_inputs(L, seed=L)
    ref = R.reference_run(inp, texel_grads=False)
    env = R.envelope(inp, ref)["g_nv"]
    amb = inp["amb"]
    assert amb.sum() >= 80 and (inp["kind"] == R.K_TINY).sum() == 128
    assert not R.outside_envelope(ref["g_nv"], amb, env, L, ref["g_nv"], inp).any()
    lo, hi = env
    mag = np.maximum(np.abs(lo), np.abs(hi)).max(axis=0)
    bad = ref["g_nv"].reshape(3, -1).copy()
    bad[0, amb] = hi[0] + mag
    assert R.outside_envelope(bad.reshape(ref["g_nv"].shape), amb, env, L, ref["g_nv"], inp).all()
