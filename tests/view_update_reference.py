"""The temporal split of a view frame (include/cloudsky.h csky_render_clouds_view_update) restated in numpy for the tests (test
infrastructure, not product).

For pixel (i, j) of a W x H image, block B, phase in [0, B * B), the current camera `view` and the previous one `prev_view`, in this order:

    e        clouds_rays_reference.view_dirs of `view`: exactly csky_render_clouds_view's direction
    accept   clouds_rays_reference.accept(e).  Not accepted: the texel is (0, 0, 0, 0), whatever follows
    fresh    i % B == phase % B  and  j % B == phase // B
    same     there is a previous frame and the ten floats of the two views are equal bit for bit
    history  no previous frame: none.    same: prev(i, j), bit for bit.    otherwise, c = prev_view's basis column-major, th = tan(prev fov / 2), asp = W / H:
               qx = (c[0]*e.x + c[1]*e.y) + c[2]*e.z     qy with c[3..5]     qz with c[6..8]
               front = qz < 0;   nx = qx / (-qz);   ny = qy / (-qz)
               u = (nx / (th * asp) + 1) * 0.5;     v = (1 - ny / th) * 0.5
               ux = u * W - 0.5;   uy = v * H - 0.5
               valid = front and 0 <= ux <= W - 1 and 0 <= uy <= H - 1
               valid: the bilinear tap of prev at (ux, uy), each channel rounded to a half
    texel    accepted and (fresh or no valid history): marched;  accepted, not fresh, valid history: the history texel

Written from the definition, not from csrc/view_update_core.h: float32 throughout, one operation per line in the order written (numpy's float32 add,
multiply, divide and floor are IEEE: exactly the operations of code compiled without contraction; astype(float16) rounds to nearest even)."""
import numpy as np

import clouds_rays_reference as RR

F = np.float32
ZERO, FRESH, COPY, TAP, HOLE = 0, 1, 2, 3, 4         # what becomes of a pixel (the numbering of csrc/view_update_core.h ViewUpdateKind)
MOVED = dict(pitch=RR.VIEW["pitch"] + 4.0, yaw=RR.VIEW["yaw"] + 8.0)   # the moved camera of the tests, against clouds_rays_reference.VIEW


def view_floats(basis, fov):
    """the ten floats of a csky_view"""
    return np.concatenate([RR.column_major(basis), np.array([fov], F)]).astype(F)


def classify(basis, fov, prev_basis, prev_fov, width, height, block, phase, same=None):
    """-> dict(kind uint8 [H, W], ux, uy float32 [H, W] (defined where the history formula ran: not `same`, accepted, not fresh), e float32 [H, W, 3]).
    prev_basis None: no previous frame.  same: None = by the rule; False = the formula even for equal cameras (what the rule is there to avoid)."""
    e = RR.view_dirs(basis, fov, width, height)
    ok = RR.accept(e)
    i = np.arange(width)[None, :] + np.zeros((height, 1), np.int64)
    j = np.arange(height)[:, None] + np.zeros((1, width), np.int64)
    fresh = (i % block == phase % block) & (j % block == phase // block)
    kind = np.full((height, width), HOLE, np.uint8)
    ux, uy = np.zeros((height, width), F), np.zeros((height, width), F)
    if prev_basis is not None:
        if same is None:
            same = view_floats(basis, fov).tobytes() == view_floats(prev_basis, prev_fov).tobytes()
        if same:
            kind[:] = COPY
        else:
            c = RR.column_major(prev_basis)
            th = RR.tan_half_fov(prev_fov)
            asp = F(width) / F(height)
            x, y, z = e[..., 0], e[..., 1], e[..., 2]
            with np.errstate(all="ignore"):
                def row(k):
                    q = c[k] * x
                    q = q + c[k + 1] * y
                    q = q + c[k + 2] * z
                    return q
                qx, qy, qz = row(0), row(3), row(6)
                front = qz < F(0.0)
                nx = qx / (-qz)
                ny = qy / (-qz)
                u = nx / (th * asp)
                u = u + F(1.0)
                u = u * F(0.5)
                v = ny / th
                v = F(1.0) - v
                v = v * F(0.5)
                ux = u * F(width)
                ux = ux - F(0.5)
                uy = v * F(height)
                uy = uy - F(0.5)
                valid = front & (ux >= F(0.0)) & (ux <= F(width - 1)) & (uy >= F(0.0)) & (uy <= F(height - 1))
            assert ux.dtype == F and uy.dtype == F
            kind[valid] = TAP
    kind[fresh] = FRESH
    kind[~ok] = ZERO
    return dict(kind=kind, ux=ux, uy=uy, e=e)


def tap(prev, ux, uy):
    """composite_core.h tap_half_clamp's arithmetic from (ux, uy) on: prev float16 [H, W, 4], ux / uy float32 [...] inside the image -> float16 [..., 4]"""
    h, w = prev.shape[:2]
    ux, uy = np.asarray(ux, F), np.asarray(uy, F)
    fx0, fy0 = np.floor(ux), np.floor(uy)
    ax, ay = ux - fx0, uy - fy0
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    x1, y1 = np.clip(x0 + 1, 0, w - 1), np.clip(y0 + 1, 0, h - 1)
    x0, y0 = np.clip(x0, 0, w - 1), np.clip(y0, 0, h - 1)
    p = prev.astype(F)
    a, b, c, d = p[y0, x0], p[y0, x1], p[y1, x0], p[y1, x1]
    ax, ay = ax[..., None], ay[..., None]

    def lerp(s, t, f):
        r = t - s
        r = r * f
        return s + r
    r = lerp(lerp(a, b, ax), lerp(c, d, ax), ay)
    assert r.dtype == F
    return r.astype(np.float16)


def compose(cls, full, prev):
    """The update's frame from the classification `cls`, the full view frame of the current camera (float16 [H, W, 4]: the marched texels) and prev."""
    kind = cls["kind"]
    out = np.zeros(full.shape, np.float16)
    marched = (kind == FRESH) | (kind == HOLE)
    out[marched] = full[marched]
    if (kind == COPY).any():
        out[kind == COPY] = prev[kind == COPY]
    t = kind == TAP
    if t.any():
        out[t] = tap(prev, cls["ux"][t], cls["uy"][t])
    return out


def shares(kind):
    """(holes, tapped) as shares of all pixels"""
    return float((kind == HOLE).mean()), float((kind == TAP).mean())


def bayer_phases(block):
    """phase k of the list: the pixel (phase % B, phase // B) whose ordered-dither index is k; M(2n) = [[4M, 4M + 2], [4M + 3, 4M + 1]]"""
    m = np.zeros((1, 1), np.int64)
    while m.shape[0] < block:
        m = np.block([[4 * m, 4 * m + 2], [4 * m + 3, 4 * m + 1]])
    order = np.zeros(block * block, np.int64)
    order[m.reshape(-1)] = np.arange(block * block)
    return [int(x) for x in order]
