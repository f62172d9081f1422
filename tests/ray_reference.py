"""The cloud march's ray (clouds.glsl:258-262, :248-256, :218-231, :143-145) restated in numpy for the tests (test infrastructure, not product):
the one restatement that tests/clouds_rays_reference.py and tests/cloud_depth_reference.py share.

    e        pixel (i, j) of a W x H hemisphere frame at update_position 0: uv = (i / W, j / H), oct_to_vec3(uv), .xzy
    ray      from a direction e with e.y > 0: t0, t1 = intersectSphere(camPos, e, Rb / Rt); start, end; shelldist = |end - start|;
             raystep = e * shelldist / N; ss = |raystep|; dir = raystep / ss; inc = dir * ss; p = start

Written from the definition, one operation per line, not from csrc/cloud_core.h: float32 throughout, in the order written (dot products summed
left to right; numpy's float32 add, multiply, divide and sqrt are IEEE: exactly the operations of code compiled without contraction)."""
import numpy as np

F = np.float32
RG, RB, RT = F(6000000.0), F(6001500.0), F(6004000.0)   # clouds.glsl:43-45


def pixel_dirs(width, height):
    """clouds.glsl:258-262, :248-256 at update_position 0: the normalised direction of every pixel, float32 [height, width, 3]."""
    i = np.arange(width, dtype=F)[None, :] + np.zeros((height, 1), F)
    j = np.arange(height, dtype=F)[:, None] + np.zeros((1, width), F)
    ex = i / F(width)
    ey = j / F(height)
    nx = ex - ey
    ny = ex + ey
    ny = ny - F(1.0)
    nz = F(1.0) - np.abs(nx)
    nz = nz - np.abs(ny)
    assert (nz >= 0).all()                                           # oct_wrap (:239-244) is dead for uv in [0, 1)^2
    nl = nx * nx
    nl = nl + ny * ny
    nl = nl + nz * nz
    nl = np.sqrt(nl)
    e = np.stack([nx / nl, nz / nl, ny / nl], -1)                    # .xzy
    assert e.dtype == F
    return e


def intersect_sphere_cam(dx, dy, dz, r):   # clouds.glsl:97-105 with pos = camPos = (0, g_radius, 0): the larger root, NaN where the line misses
    a = dx * dx
    a = a + dy * dy
    a = a + dz * dz
    b = dx * F(0.0)
    b = b + dy * RG
    b = b + dz * F(0.0)
    b = F(2.0) * b
    c = F(0.0) * F(0.0) + RG * RG
    c = c + F(0.0) * F(0.0)
    c = c - r * r
    e = F(4.0) * a
    e = e * c
    d = b * b
    d = d - e
    d = np.sqrt(d)
    p = -b - d
    p2 = -b + d
    return np.maximum(p, p2) / (F(2.0) * a)


def ray(e, steps):
    """The ray of directions float32 [..., 3] at `steps` primary steps (clouds.glsl:221-230, :143-145 with `steps` for 128): dict(p, inc, dir
    float32 [..., 3]; ss, t0 float32 [...]), t0 the distance of the shell entry p.  A direction with e.y <= 0 has no ray: its entries hold whatever
    the arithmetic gives, and nothing may read them."""
    e = np.asarray(e, F)
    dx, dy, dz = e[..., 0], e[..., 1], e[..., 2]
    n = F(steps)
    with np.errstate(invalid="ignore", divide="ignore"):
        t0 = intersect_sphere_cam(dx, dy, dz, RB)
        t1 = intersect_sphere_cam(dx, dy, dz, RT)
        sx, sy, sz = F(0.0) + dx * t0, RG + dy * t0, F(0.0) + dz * t0    # start, :224
        ex, ey, ez = F(0.0) + dx * t1, RG + dy * t1, F(0.0) + dz * t1    # end, :225
        qx, qy, qz = ex - sx, ey - sy, ez - sz
        sd = qx * qx
        sd = sd + qy * qy
        sd = sd + qz * qz
        sd = np.sqrt(sd)
        rx, ry, rz = dx * sd / n, dy * sd / n, dz * sd / n               # :230
        ss = rx * rx
        ss = ss + ry * ry
        ss = ss + rz * rz
        ss = np.sqrt(ss)                                                 # :143
        ux, uy, uz = rx / ss, ry / ss, rz / ss                           # :144
        inc = np.stack([ux * ss, uy * ss, uz * ss], -1)                  # dir * ss, :173
    assert ss.dtype == F and inc.dtype == F and t0.dtype == F
    return dict(p=np.stack([sx, sy, sz], -1), dir=np.stack([ux, uy, uz], -1), inc=inc, ss=ss, t0=t0)
