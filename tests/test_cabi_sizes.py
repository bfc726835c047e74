"""The scratch-size queries of the loss, metrics, viewer, training, env-scope, densification and reflection entries, pinned.  (Those of
the mesh, clean-up and k-NN entries are pinned in tests/test_cabi_mesh.py.)  Host arithmetic: the built library, no device."""

P_FIRST_REFUSED = -(-2 ** 31 // 3)        # the first P at which P * (N + 1) reaches 2^31 for N = 2


def _each_position(well_formed):
    """`well_formed` with zero, then a negative value, in each position."""
    return [well_formed[:i] + (bad,) + well_formed[i + 1:] for i in range(len(well_formed)) for bad in (0, -1)]


def test_scratch_sizes_are_the_recorded_ones(hip_lib_built):
    """The values below were read from the library as it was before the entries' host checks moved to csrc/gsr_host.hpp: 1 x 1, one SSIM
    tile plus a ragged edge each way (3, 33, 31), 1080p, each viewer flag set that changes the layout, the densification plan on either
    side of P * (N + 1) = 2^31, both reflection paths at both cubemap sizes, and 0 for a zero or a negative value in any position.  A
    caller's buffer sized by an older library must still fit: none of them may change."""
    import _gsr
    view = {0: {(1, 1, 1): 0, (3, 33, 31): 0, (3, 1080, 1920): 0}, 4: {(1, 1, 1): 4, (3, 33, 31): 4, (3, 1080, 1920): 4},
            6: {(1, 1, 1): 5, (3, 33, 31): 1027, (3, 1080, 1920): 2073604}}
    recorded = {
        "gsr_ssim_l1_scratch_floats": {(1, 1, 1): 2, (3, 33, 31): 12, (3, 1080, 1920): 12240},
        "gsr_photometric_scratch_floats": {(1, 1, 1): 2, (3, 33, 31): 12, (3, 1080, 1920): 12240},
        "gsr_image_metrics_scratch_floats": {(1, 1, 1): 4, (3, 33, 31): 24, (3, 1080, 1920): 24480},
        "gsr_normal_mae_scratch_floats": {(1, 1): 4, (33, 31): 16, (1080, 1920): 4096},
        "gsr_present_view_scratch_floats": {size + (flags,): n for flags, table in view.items() for size, n in table.items()},
        "gsr_normal_loss_scratch_floats": {(): 2048},
        "gsr_env_scope_scratch_floats": {(): 2048},
        "gsr_densify_plan_scratch_bytes": {(0, 2): 256, (1, 1): 1280, (1000, 2): 16896, (P_FIRST_REFUSED - 1, 2): 11632203776, (P_FIRST_REFUSED, 2): 0,
                                           (-1, 2): 0, (1000, 0): 0, (1000, -1): 0},
        "gsr_deferred_reflection_scratch_floats": {(128, 1920, 1080, 0): 393220, (128, 1920, 1080, 1): 28129224, (256, 1920, 1080, 0): 1572868,
                                                   (256, 1920, 1080, 1): 29308872, (128, 1, 1, 0): 393220, (128, 1, 1, 1): 396115, (128, 31, 33, 1): 409277},
    }
    for name in ("gsr_ssim_l1_scratch_floats", "gsr_photometric_scratch_floats", "gsr_image_metrics_scratch_floats"):
        recorded[name].update({bad: 0 for bad in _each_position((3, 33, 31))})
    recorded["gsr_normal_mae_scratch_floats"].update({bad: 0 for bad in _each_position((33, 31))})
    recorded["gsr_present_view_scratch_floats"].update({bad + (flags,): 0 for flags in (0, 4, 6) for bad in _each_position((3, 33, 31))})
    recorded["gsr_deferred_reflection_scratch_floats"].update({bad + (binned,): 0 for binned in (0, 1) for bad in _each_position((128, 1920, 1080))
                                                               if bad[0] >= 0})        # (L is unsigned)
    assert P_FIRST_REFUSED * 3 >= 2 ** 31 > (P_FIRST_REFUSED - 1) * 3
    for name, table in recorded.items():
        for sizes, expected in table.items():
            assert int(getattr(_gsr.lib, name)(*sizes)) == expected, (name, sizes)
