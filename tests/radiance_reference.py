"""Independent numpy (float64) restatement of the radiance cubemap's contract (include/cloudsky.h, csky_render_radiance*): the face map,
its inverse, the texel solid angles, the source-cube block mean and the GGX prefilter sum.  Written from the header's text, not from
csrc/radiance_core.h."""
import numpy as np

# face f: (sc, tc) -> unnormalised direction (Vulkan major-axis rule), faces +X, -X, +Y, -Y, +Z, -Z
_FACE = [lambda s, t: (np.ones_like(s), -t, -s), lambda s, t: (-np.ones_like(s), -t, s), lambda s, t: (s, np.ones_like(s), t),
         lambda s, t: (s, -np.ones_like(s), -t), lambda s, t: (s, -t, np.ones_like(s)), lambda s, t: (-s, -t, -np.ones_like(s))]

# camera basis columns (right, up, back) that see face f through a square 90-degree screen (the header's layer-0 table)
FACE_BASIS = [((0, 0, -1), (0, 1, 0), (-1, 0, 0)), ((0, 0, 1), (0, 1, 0), (1, 0, 0)), ((1, 0, 0), (0, 0, -1), (0, -1, 0)),
              ((1, 0, 0), (0, 0, 1), (0, 1, 0)), ((1, 0, 0), (0, 1, 0), (0, 0, -1)), ((-1, 0, 0), (0, 1, 0), (0, 0, 1))]


def face_basis(f):
    """3x3 basis of face f, columns = right / up / back (the layout tests/test_compositor.py's camera_basis returns)."""
    return np.array(FACE_BASIS[f], np.float32).T


def face_dirs(n):
    """Unit texel-centre directions [6, n, n, 3] (row j, column i)."""
    c = (np.arange(n) + 0.5) * 2.0 / n - 1.0
    tc, sc = np.meshgrid(c, c, indexing="ij")
    out = np.zeros((6, n, n, 3))
    for f in range(6):
        v = np.stack(_FACE[f](sc, tc), -1)
        out[f] = v / np.linalg.norm(v, axis=-1, keepdims=True)
    return out


def dir_to_texel(d, n):
    """Inverse major-axis rule: direction(s) [..., 3] -> (face, i, j) of an n x n cube."""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    face = np.where((ax >= ay) & (ax >= az), np.where(x > 0, 0, 1), np.where(ay >= az, np.where(y > 0, 2, 3), np.where(z > 0, 4, 5)))
    # (sc, tc) = (s / |ma|, t / |ma|) with the s / t of each face read off the forward map
    ma = np.choose(face, [ax, ax, ay, ay, az, az])
    s = np.choose(face, [-z, z, x, x, x, -x])
    t = np.choose(face, [-y, -y, z, -z, -y, -y])
    sc, tc = s / ma, t / ma
    i = np.clip(np.floor((sc + 1.0) * 0.5 * n), 0, n - 1).astype(int)
    j = np.clip(np.floor((tc + 1.0) * 0.5 * n), 0, n - 1).astype(int)
    return face, i, j


def _area(x, y):
    return np.arctan2(x * y, np.sqrt(x * x + y * y + 1.0))


def solid_angles(n):
    """Exact texel solid angles of one face [n, n] (row j, column i); the same on every face."""
    e = np.arange(n + 1) * 2.0 / n - 1.0
    y0, x0 = np.meshgrid(e[:-1], e[:-1], indexing="ij")
    y1, x1 = np.meshgrid(e[1:], e[1:], indexing="ij")
    return _area(x0, y0) - _area(x0, y1) - _area(x1, y0) + _area(x1, y1)


def block_mean(cube, ns):
    """[6, S, S, C] -> [6, ns, ns, C]: the mean of each (S/ns)^2 block (float64)."""
    cube = np.asarray(cube, np.float64)
    S = cube.shape[1]
    k = S // ns
    return cube.reshape(6, ns, k, ns, k, cube.shape[-1]).mean(axis=(2, 4))


def layer_alpha2(k, L):
    r = k / (L - 1)
    return (r * r) ** 2


def prefilter(cube, layers, source_size=0, texels=None, chunk=1024):
    """The contract's filter on a float cube [6, S, S, 4] (fp16 values as the library reads them), float64.
    Returns [layers - 1, M, 3]: layers 1..L-1 (RGB) for the receiver texels `texels` = (face, row, col) index arrays (default: every texel in
    [face][row][col] order, M = 6 S^2)."""
    cube = np.asarray(cube, np.float64)
    S = cube.shape[1]
    ns = min(S, 64) if source_size == 0 else source_size
    src = block_mean(cube[..., :3], ns).reshape(-1, 3)
    Ld = face_dirs(ns).reshape(-1, 3)
    om = np.broadcast_to(solid_angles(ns), (6, ns, ns)).reshape(-1)
    Nd = face_dirs(S)
    N = Nd.reshape(-1, 3) if texels is None else Nd[texels[0], texels[1], texels[2]]
    out = np.zeros((layers - 1, N.shape[0], 3))
    for a in range(0, N.shape[0], chunk):
        c = N[a:a + chunk] @ Ld.T
        cp = np.maximum(c, 0.0)
        for k in range(1, layers):
            a2 = layer_alpha2(k, layers)
            w = cp * om / (c * (a2 - 1.0) / 2.0 + (a2 + 1.0) / 2.0) ** 2
            out[k - 1, a:a + chunk] = (w @ src) / w.sum(axis=1, keepdims=True)
    return out


def smooth_cube(S, seed=0):
    """A test cube: a smooth sky-like gradient plus 20 % texel noise, float16 [6, S, S, 4], alpha 1."""
    rng = np.random.default_rng(seed)
    d = face_dirs(S)
    rgb = (1.0 + 0.8 * d[..., 1:2] + 0.3 * d[..., 0:1] * d[..., 2:3]) * np.array([1.0, 0.8, 0.6]) + 0.2 * rng.random((6, S, S, 3))
    return np.concatenate([rgb, np.ones((6, S, S, 1))], -1).astype(np.float16)


DISC_DIR = np.array([0.5, 0.6, 0.62]) / np.linalg.norm([0.5, 0.6, 0.62])   # near the +Y / +Z seam
DISC_RADIUS = 0.02


def disc_angle(S):
    """Angle [6, S, S] (radians) between each texel-centre direction and the centre of hdr_cube's disc."""
    return np.arccos(np.clip(face_dirs(S) @ DISC_DIR, -1.0, 1.0))


def hdr_cube(S, value=30000.0, seed=3):
    """A high-dynamic-range test cube: smooth_cube(S, seed) with a sun-like disc (radius DISC_RADIUS around DISC_DIR) of RGB `value`."""
    cube = smooth_cube(S, seed)
    cube[disc_angle(S) < DISC_RADIUS, :3] = value
    return cube
