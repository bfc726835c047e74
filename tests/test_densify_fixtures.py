"""tests/densify_fixtures.py on the CPU: every fixture the GPU tests of the densification plan use (tests/test_gpu_densify_plan.py) is clear
of the thresholds across which torch's kernels and the library's may round differently — the condition under which those tests ask for bit
equality of the two plans — and holds the classes the tests are about."""
import numpy as np
import pytest

import densify_fixtures as F


@pytest.mark.parametrize("key", F.ALL, ids=lambda k: "P%d-%s" % (k[0], k[2]))
def test_no_row_and_no_child_lies_within_a_band_of_a_threshold(key):
    fx = F.get(key)
    bad_scale, bad_d2, _ = F.bands(fx)
    assert bad_scale.size == 0 and bad_d2.size == 0
    assert fx["moved"] <= max(8, fx["P"] // 1000)                # the draws are the fixture: a handful of rows at the most were moved
    # the check itself, stated once more without the helper: every largest scale and every squared distance, rows and children
    lim = F.limits(fx["extent"])
    pruned, clone, parent, m = F.classes(fx)
    par, cxyz, cm = F.children(fx, parent)
    mean = np.asarray(fx["mean"], np.float64)
    d2 = ((fx["scene"]["means3D"].astype(np.float64) - mean) ** 2).sum(-1)
    cd2 = ((cxyz - mean) ** 2).sum(-1)
    for v in (m, cm):
        for L in ("dense", "near", "far"):
            assert not (np.abs(v / np.float64(lim[L]) - 1) < 1e-5).any(), L
    for v in (d2, cd2):
        assert not (np.abs(v / np.float64(lim["extent2"]) - 1) < 1e-5).any()
    assert par.size == fx["N"] * int(parent.sum()) and not (clone & parent).any()


@pytest.mark.parametrize("key", [k for k in F.ALL if k[2] in ("views", "denoms") and k[0] >= 2000], ids=lambda k: "P%d-%s" % (k[0], k[2]))
def test_the_seeded_fixtures_hold_more_than_100_rows_of_each_class(key):
    """(The shapes below 2000 rows and the hand-made class mixes cannot: they are there for their sizes and for their single class.)"""
    s = F.summary(F.get(key))
    assert min(s["pruned"], s["cloned"], s["split"], s["kept"]) > 100, s
    assert s["big"] > 0, s                                        # every one of them is run with a size threshold


def test_the_class_mixes_are_what_their_names_say():
    P = 300
    got = {k[2]: F.summary(F.get(k)) for k in F.MIXES}
    s = got["identity"]                                           # (run without a size threshold: what would be big is not looked at)
    assert (s["pruned"], s["cloned"], s["split"], s["kept"], s["length"]) == (0, 0, 0, P, P)
    assert (got["clones"]["cloned"], got["clones"]["pruned"], got["clones"]["split"], got["clones"]["big"]) == (P, 0, 0, 0)
    s = got["parents"]
    assert (s["split"], s["kept"], s["cloned"], s["pruned"]) == (P - 5, 5, 0, 0)
    assert s["big"] == 2 * (P - 5) and s["length"] - s["big"] == 5       # every child is dropped, the five unsplit rows remain
    assert (got["one"]["pruned"], got["one"]["kept"], got["one"]["length"]) == (P - 1, 1, 1)


def test_the_denominator_rows():
    fx = F.get(F.DENOMS)
    pruned, clone, parent, m = F.classes(fx)
    r = np.arange(8, 56)
    assert not (pruned | clone | parent)[r[:16]].any()           # 0 / 0: NaN -> 0, not selected
    assert clone[r[16:24]].all() and parent[r[24:32]].all()      # x / 0: inf, selected
    assert pruned[r[32:]].all()                                  # denom_w == 0
    assert (fx["stats"]["denom"][r[:32]] == 0).all() and (fx["stats"]["denom_w"][r[32:]] == 0).all()


def test_fixtures_are_seeded():
    a, b = F.make(*F.SMALL[4][:2], mix="views", stats_seed=F.SMALL[4][3]), F.get(F.SMALL[4])
    for k in a["scene"]:
        assert np.array_equal(a["scene"][k], b["scene"][k])
    for k in a["stats"]:
        assert np.array_equal(a["stats"][k], b["stats"][k])
    assert np.array_equal(a["noise_pool"], b["noise_pool"])
