"""CPU: every scene family of tests/adversarial_scenes.py reaches the branches it was built for, measured on the float32 oracle's lists
with the pairs re-evaluated in float64 (adversarial_scenes.reach).  A family that misses its target tests nothing on the GPU.  The scenes
are the ones tests/test_gpu_adversarial.py renders (same family, size and seed)."""
import numpy as np
import pytest

import adversarial_scenes as A


def _reach(name, variant):
    P, W, H, seed = A.SCENES[name]
    return A.reach(variant, A.family(name, variant, P, W, H, seed), antialiasing=True)


@pytest.mark.parametrize("variant", ["S", "G"])
def test_surface_family_saturates_and_fills_backward_batches(variant):
    c = _reach("surface", variant)
    assert c["saturated"] >= 2000, c                      # opaque layers end lists at T < 1e-4
    assert c["alpha_edge"] >= 1000, c
    assert c["tied_keys"] >= 1000, c                      # the back wall sits at one depth
    if variant == "S":
        # the backward cuts a batch with more than S_CAP (row, entry) pairs: default 48, 32 in the rare-path build
        assert c["batch_pairs_gt48"] >= 0.1 * c["batches"], c
        assert c["batch_pairs_gt32"] >= 0.25 * c["batches"], c


def test_grazing_family_straddles_both_grazing_thresholds():
    c = _reach("grazing", "S")
    assert c["pz_lt_1e4"] >= 5000, c                      # the forward's grazing branch
    assert c["pz_1e6_1e4"] >= 5000, c                     # grazing in the forward, not in the backward
    assert c["pz_lt_1e4"] - c["pz_1e6_1e4"] >= 100, c     # grazing in both
    assert c["low_pass"] >= 5000, c


def test_grazing_family_with_degenerate_homographies():
    c = _reach("grazing_T", "S")
    assert c["pz_eq0"] >= 100_000, c                      # the camera centre in the splat plane: p.z == 0 exactly
    assert c["pz_1e6_1e4"] >= 5000, c


@pytest.mark.parametrize("variant", ["S", "G"])
def test_threshold_family_sits_on_the_thresholds(variant):
    c = _reach("threshold", variant)
    assert c["alpha_edge"] >= 1000, c                     # alpha in [1/255, 1.05/255]
    assert c["alpha_clamp"] >= 500, c                     # the 0.99 clamp
    assert c["saturated"] >= 5000, c
    if variant == "S":
        assert c["low_pass"] >= 1000, c                   # sub-pixel splats: the low-pass disc wins
        assert c["cam_plane"] >= 20, c                    # cutoff disc through the camera plane: the cull record's "always a hit"
        assert c["near_skip"] >= 1000, c


@pytest.mark.parametrize("name", ["dup_surface", "dup_threshold"])
@pytest.mark.parametrize("variant", ["S", "G"])
def test_duplicates_tie_depth_keys(name, variant):
    c = _reach(name, variant)
    assert c["tied_keys"] >= 0.2 * c["num_rendered"], c


def test_threshold_family_values_are_exact():
    P, W, H, seed = A.SCENES["threshold"]
    kw = A.family("threshold", "S", P, W, H, seed)
    op = kw["opacities"].reshape(-1)
    third = np.float32(1 / 255)
    for v in (third, np.nextafter(third, np.float32(0)), np.nextafter(third, np.float32(1)), np.float32(0.995), np.float32(1.0)):
        assert (op == v).sum() >= P // 10, v
    z = kw["means3D"][:, 2]
    assert (z == np.float32(0.2)).any() and (z == np.nextafter(np.float32(0.2), np.float32(1))).any()
    ratio = kw["scales"].min(1) / kw["scales"].max(1)
    assert (ratio < 2e-4).sum() >= P // 10
