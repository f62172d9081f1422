"""The per-lane cores of the view forms and of the temporal split (csrc/rays_core.h rays_view_dir, csrc/view_update_core.h), compiled for the host by
tests/rays_host and tests/view_update_host, held to the numpy restatements at the cameras of tests/view_cameras.py: rolled, zoomed between two
frames, portrait, at the horizon and the zenith, a previous camera that looks elsewhere, very narrow, very wide.  A unit test of device code, not a
render path.  Every comparison is bit for bit; what each case is there for is asserted from the reference alone (view_cameras.assert_shares)."""
import numpy as np
import pytest

import clouds_rays_reference as RR
import view_cameras as VC
import view_update_reference as VU
from test_clouds_rays_host import host_view_dirs, rays_host  # noqa: F401  (module-scoped fixture)
from test_view_update_host import core_classify, core_tap, vu_host  # noqa: F401  (module-scoped fixture)


@pytest.mark.parametrize("name", VC.NAMES)
def test_every_case_holds_the_pixel_kinds_it_is_in_the_table_for(name):
    VC.assert_shares(name)
    if name in VC.MIRRORED:                                          # the pixels a missing `front` would tap are holes or fresh, never taps
        kind = VC.classify(name, 4, 5)["kind"]
        m = VC.mirror_valid(name)
        assert ((kind[m] == VU.HOLE) | (kind[m] == VU.FRESH)).all() and (kind[m] == VU.HOLE).sum() >= 0.09 * kind.size


@pytest.mark.parametrize("block,phase", VC.PAIRS)
@pytest.mark.parametrize("name", VC.NAMES)
def test_classification_and_coordinates_are_the_restatement_bit_for_bit(vu_host, name, block, phase):  # noqa: F811
    b, fov, pb, pfov, w, h = VC.views(name)
    ref = VU.classify(b, fov, pb, pfov, w, h, block, phase)
    kind, ux, uy, d = core_classify(vu_host, VU.view_floats(b, fov), VU.view_floats(pb, pfov), w, h, block, phase)
    print("%s B = %d phase %d: %s" % (name, block, phase, VC.counts(ref["kind"])))
    assert (d.view(np.uint32) == ref["e"].view(np.uint32)).all()
    assert (kind == ref["kind"]).all(), np.argwhere(kind != ref["kind"])[:4]
    ran = (kind == VU.TAP) | (kind == VU.HOLE)                        # where the history formula ran
    assert ran.sum() > 0.2 * w * h and not (kind == VU.COPY).any()
    assert (ux.view(np.uint32)[ran] == ref["ux"].view(np.uint32)[ran]).all() and (uy.view(np.uint32)[ran] == ref["uy"].view(np.uint32)[ran]).all()
    t = kind == VU.TAP                                               # a tap's coordinates lie inside the image: no address from anything else
    assert (ux[t] >= 0).all() and (ux[t] <= w - 1).all() and (uy[t] >= 0).all() and (uy[t] <= h - 1).all()


@pytest.mark.parametrize("name", ["roll-both", "zoom-out"])
def test_taps_of_subnormal_negative_and_largest_halves_are_the_restatement(vu_host, name):  # noqa: F811
    """The host core's taps of view_cameras.edge_frame at a case's own coordinates: what the GPU test holds the device's taps to."""
    b, fov, pb, pfov, w, h = VC.views(name)
    prev = VC.edge_frame(h, w, 0)
    for block, phase in VC.PAIRS:
        ref = VU.classify(b, fov, pb, pfov, w, h, block, phase)
        t = ref["kind"] == VU.TAP
        want = VU.tap(prev, ref["ux"][t], ref["uy"][t])
        sub, neg, big = VC.tap_edge_shares(want)
        print("%s B = %d phase %d: of %d expected halves %.1f %% subnormal, %.1f %% negative, %d at 0x7BFF or above" % (name, block, phase, want.size, 100 * sub, 100 * neg, big))
        assert sub >= 0.01 and neg >= 0.20 and big >= 1
        got = core_tap(vu_host, prev, ref["ux"][t], ref["uy"][t])
        assert (got.view(np.uint16) == want.view(np.uint16)).all()


@pytest.mark.parametrize("name", VC.NAMES)
def test_numpy_view_directions_equal_the_core_bit_for_bit(rays_host, name):  # noqa: F811
    b, fov, _, _, w, h = VC.views(name)
    got = host_view_dirs(rays_host, b, fov, w, h)
    ref = RR.view_dirs(b, fov, w, h)
    assert (got.view(np.uint32) == ref.view(np.uint32)).all()
    l2 = (got.astype(np.float64) ** 2).sum(-1)
    assert np.abs(l2 - 1.0).max() < 1e-6                             # unit directions at every fov: the accept band rejects by e.y alone
    assert (RR.accept(got) == (got[..., 1] > 0)).all()
