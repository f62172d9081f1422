"""The cameras the view forms and the temporal split are held at beyond clouds_rays_reference.VIEW and its one neighbour (test infrastructure, not
product): rolled, zoomed between two frames, portrait, at the horizon and at the zenith, with the previous camera looking elsewhere, very narrow,
very wide, and an image whose fresh sub-grid is wider than one workgroup.

A camera is (pitch, yaw, roll, fov) in degrees: clouds_rays_reference.camera_basis(pitch, yaw) rolled about its own back axis.  A case is the
current camera, the previous camera and the image size.

The shares of the pixel kinds of view_update_reference.classify at B = 4, phase 5, in % of all pixels (mirror-valid: mirror_valid below):

    case        zero   tap   hole  mirror-valid
    roll        18.1  65.9  10.9    0
    roll-both   16.8  51.9  26.1    0
    zoom-in      0    93.8   0      0
    zoom-out    27.8  26.5  40.8    0
    portrait    10.9  62.6  21.0    0
    horizon     63.9  29.9   4.1    0
    zenith       0    52.2  41.5    0
    behind      44.4  26.0  26.1   22.2
    opposite    16.7   0    77.8   79.6
    narrow       0    57.0  36.8    0
    wide        47.2  25.0  24.3   16.1
    wide-sub    12.5  59.2  23.1    0

assert_shares holds every case to conditions with margin against these figures, from the reference alone, before anything is compared."""
import numpy as np

import clouds_rays_reference as RR
import view_update_reference as VU

F = np.float32
PAIRS = [(4, 5), (2, 1), (8, 37)]                    # the (B, phase) pairs every case is classified at

#        case          current (pitch, yaw, roll, fov)   previous                      W    H
CASES = {
    "roll":      ((25.0, 40.0, 25.0, 70.0),  (25.0, 40.0, 0.0, 70.0),    64, 36),
    "roll-both": ((30.0, 50.0, -40.0, 70.0), (25.0, 40.0, 15.0, 70.0),   64, 36),
    "zoom-in":   ((27.0, 43.0, 0.0, 40.0),   (25.0, 40.0, 0.0, 70.0),    64, 36),
    "zoom-out":  ((27.0, 43.0, 0.0, 100.0),  (25.0, 40.0, 0.0, 70.0),    64, 36),
    "portrait":  ((29.0, 48.0, 0.0, 70.0),   (25.0, 40.0, 0.0, 70.0),    36, 64),
    "horizon":   ((-10.0, 40.0, 0.0, 70.0),  (-6.0, 32.0, 0.0, 70.0),    64, 36),
    "zenith":    ((88.0, 10.0, 0.0, 70.0),   (84.0, 100.0, 0.0, 70.0),   64, 36),
    "behind":    ((20.0, 40.0, 0.0, 150.0),  (20.0, 150.0, 0.0, 150.0),  64, 36),
    "opposite":  ((25.0, 40.0, 0.0, 70.0),   (-25.0, 220.0, 0.0, 70.0),  64, 36),
    "narrow":    ((30.0, 40.0, 0.0, 2.0),    (30.5, 40.7, 0.0, 2.0),     64, 36),
    "wide":      ((35.0, 40.0, 0.0, 170.0),  (30.0, 50.0, 0.0, 170.0),   64, 36),
    "wide-sub":  ((29.0, 48.0, 0.0, 70.0),   (25.0, 40.0, 0.0, 70.0),    160, 24),
}
NAMES = list(CASES)
MIRRORED = ("behind", "wide", "opposite")            # a previous camera that has accepted pixels of the current one behind it


def basis(pitch, yaw, roll=0.0):
    """3x3 float32, columns = right / up / back: clouds_rays_reference.camera_basis(pitch, yaw) @ Rz(roll), in float64, rounded to float32 once"""
    p, y, r = np.radians(pitch), np.radians(yaw), np.radians(roll)
    rx = np.array([[1, 0, 0], [0, np.cos(p), -np.sin(p)], [0, np.sin(p), np.cos(p)]])
    ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]])
    rz = np.array([[np.cos(r), -np.sin(r), 0], [np.sin(r), np.cos(r), 0], [0, 0, 1]])
    b = (ry @ rx @ rz).astype(F)
    if roll == 0.0:
        assert b.tobytes() == RR.camera_basis(pitch, yaw).tobytes()
    return b


def views(name):
    """(basis, fov, previous basis, previous fov, W, H) of a case"""
    cur, prev, w, h = CASES[name]
    return basis(*cur[:3]), cur[3], basis(*prev[:3]), prev[3], w, h


def classify(name, block, phase):
    b, fov, pb, pfov, w, h = views(name)
    return VU.classify(b, fov, pb, pfov, w, h, block, phase)


def mirror_valid(name):
    """bool [H, W]: the accepted pixels BEHIND the previous camera (qz >= 0) whose coordinates by the formula of the definition nevertheless lie
    inside the image: what an update without the `front` test would tap.  float64."""
    b, fov, pb, pfov, w, h = views(name)
    e = RR.view_dirs(b, fov, w, h)
    c = RR.column_major(pb).astype(np.float64)
    x, y, z = (e[..., k].astype(np.float64) for k in range(3))
    th, asp = float(RR.tan_half_fov(pfov)), w / h
    with np.errstate(all="ignore"):
        qx, qy, qz = (c[k] * x + c[k + 1] * y + c[k + 2] * z for k in (0, 3, 6))
        ux = ((qx / -qz) / (th * asp) + 1.0) * 0.5 * w - 0.5
        uy = (1.0 - (qy / -qz) / th) * 0.5 * h - 0.5
        return RR.accept(e) & (qz >= 0.0) & (ux >= 0.0) & (ux <= w - 1) & (uy >= 0.0) & (uy <= h - 1)


def tap_texels(prev, ux, uy):
    """uint16 [n, 4 texels, 4 halves]: the four texels of prev that view_update_reference.tap reads at the coordinates ux, uy"""
    h, w = prev.shape[:2]
    x0, y0 = np.floor(ux).astype(np.int64), np.floor(uy).astype(np.int64)
    x1, y1 = np.clip(x0 + 1, 0, w - 1), np.clip(y0 + 1, 0, h - 1)
    p = np.ascontiguousarray(prev).view(np.uint16)
    return np.stack([p[y0, x0], p[y0, x1], p[y1, x0], p[y1, x1]], 1)


def mixed_zero_taps(prev, ux, uy):
    """bool [n]: the taps that read at least one texel of four zero halves and at least one that is not"""
    zero = ~tap_texels(prev, ux, uy).any(-1)
    return zero.any(-1) & ~zero.all(-1)


def edge_frame(h, w, seed):
    """test_view_update_host.random_frame with two kinds of 4 x 4 texel patches laid over it: every fourth patch (at random) holds subnormals of both
    signs, every tenth +-0x7BFF (65504), one sign per patch and channel.  random_frame alone cannot give what the tap test asks of its expected
    taps: a bilinear tap of four independent random halves is subnormal in 0.1..0.4 % of the results and never reaches 0x7BFF, whatever the seed.
    Inside a patch a tap mixes four subnormals, or four equal 0x7BFF (which it must return as they are); on a patch's rim it mixes them with the
    random halves around, 65504 against -65504 included."""
    from test_view_update_host import random_frame
    a = np.ascontiguousarray(random_frame(h, w, seed)).view(np.uint16).copy()
    r = np.random.default_rng(1000 + seed)
    for y in range(0, h, 4):
        for x in range(0, w, 4):
            pick = r.random()
            n = a[y:y + 4, x:x + 4].shape
            if pick < 0.25:
                a[y:y + 4, x:x + 4] = r.integers(1, 0x400, n).astype(np.uint16) | (r.integers(0, 2, n).astype(np.uint16) << 15)
            elif pick < 0.35:
                a[y:y + 4, x:x + 4] = np.uint16(0x7BFF) | (r.integers(0, 2, 4).astype(np.uint16) << 15)
    return a.view(np.float16)


def tap_edge_shares(taps):
    """(subnormal, negative) shares of the halves float16 [..., 4] and the number at or above 0x7BFF in magnitude"""
    x = np.ascontiguousarray(taps).view(np.uint16)
    m = x & 0x7FFF
    return float(((m > 0) & (m < 0x400)).mean()), float(((x >> 15 == 1) & (m > 0)).mean()), int((m >= 0x7BFF).sum())


CHAIN_MOVING, CHAIN_STILL = 24, 16


def chain_cameras():
    """[(basis, fov)] of the forty calls of the chain test: 24 cameras from clouds_rays_reference.VIEW on, each pitched 0.5, yawed 1.5 and rolled
    1.0 degrees further than the one before, the fov going from 70 to 58 in equal steps; then the last camera sixteen times more."""
    v = RR.VIEW
    cams = [(basis(v["pitch"] + 0.5 * k, v["yaw"] + 1.5 * k, 1.0 * k), v["fov"] - 12.0 * k / (CHAIN_MOVING - 1)) for k in range(CHAIN_MOVING)]
    return cams + [cams[-1]] * CHAIN_STILL


def counts(kind):
    return "zero %d, fresh %d, copy %d, tap %d, hole %d of %d pixels" % tuple([int((kind == k).sum()) for k in (VU.ZERO, VU.FRESH, VU.COPY, VU.TAP, VU.HOLE)] + [kind.size])


def assert_shares(name, kind=None):
    """The conditions a case is in the table for, at B = 4, phase 5, from the reference alone."""
    if kind is None:
        kind = classify(name, 4, 5)["kind"]
    zero, tap, hole, mirror = (float(x.mean()) for x in (kind == VU.ZERO, kind == VU.TAP, kind == VU.HOLE, mirror_valid(name)))
    print("%s, reference at B = 4, phase 5: zero %.1f %%, tap %.1f %%, hole %.1f %%, mirror-valid %.1f %%" % (name, 100 * zero, 100 * tap, 100 * hole, 100 * mirror))
    assert tap == 0.0 if name == "opposite" else tap >= 0.20
    assert hole == 0.0 if name == "zoom-in" else hole >= 0.03        # zoom-in: the previous frame covers everything
    if name == "horizon":
        assert zero >= 0.50
    assert mirror >= 0.10 if name in MIRRORED else mirror == 0.0
    return zero, tap, hole, mirror
