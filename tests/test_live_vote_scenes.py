"""CPU: the scenes of tests/live_vote_scenes.py do what tests/test_gpu_live_vote.py needs them for.  By the oracle, at least a quarter of the
image's pixels retire before their tile's list ends (a scene in which nothing retires leaves the vote's live box the whole block and tests
nothing), and `stack` puts at least 130 entries on one tile, so that a box is rebuilt between batches."""
import pytest

import live_vote_scenes as L


@pytest.mark.parametrize("variant", ["S", "G"])
@pytest.mark.parametrize("size", L.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", L.NAMES)
def test_pixels_retire_before_their_list_ends(name, size, variant):
    share, longest = L.retired_fraction(name, variant, *size)
    print("%s %dx%d %s: %.2f of the pixels retire before their list ends, longest list %d" % (name, size[0], size[1], variant, share, longest))
    assert share >= 0.25
    if name in ("stack", "rare"):
        assert longest >= 130
