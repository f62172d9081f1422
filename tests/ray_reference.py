"""The cloud march's ray (clouds.glsl:258-262, :248-256, :218-231, :143-145) restated in numpy for the tests (test infrastructure, not product):
the one restatement that tests/clouds_rays_reference.py and tests/cloud_depth_reference.py share.

    e        pixel (i, j) of a W x H hemisphere frame at update_position 0: uv = (i / W, j / H), oct_to_vec3(uv), .xzy
    ray      from a direction e with e.y > 0: t0, t1 = intersectSphere(camPos, e, Rb / Rt); start, end; shelldist = |end - start|;
             raystep = e * shelldist / N; ss = |raystep|; dir = raystep / ss; inc = dir * ss; p = start

Written from the definition, one operation per line, not from csrc/cloud_core.h: float32 throughout, in the order written (dot products summed
left to right; numpy's float32 add, multiply, divide and sqrt are IEEE: exactly the operations of code compiled without contraction).

Every function takes an optional `rec`, a dict with lists "sqrt" and "div": the operands of every square root and every division it evaluates are
appended there (tests/test_primitives_host.py collects the ray set-up's own operands for the device's sqrt and divide with it)."""
import numpy as np

F = np.float32
RG, RB, RT = F(6000000.0), F(6001500.0), F(6004000.0)   # clouds.glsl:43-45


def _sqrt(x, rec):
    if rec is not None:
        rec["sqrt"].append(np.asarray(x, F).reshape(-1))
    return np.sqrt(x)


def _div(a, b, rec):
    if rec is not None:
        a2, b2 = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F))
        rec["div"].append((a2.reshape(-1), b2.reshape(-1)))
    return a / b


def pixel_dirs(width, height, rec=None):
    """clouds.glsl:258-262, :248-256 at update_position 0: the normalised direction of every pixel, float32 [height, width, 3]."""
    i = np.arange(width, dtype=F)[None, :] + np.zeros((height, 1), F)
    j = np.arange(height, dtype=F)[:, None] + np.zeros((1, width), F)
    ex = _div(i, F(width), rec)
    ey = _div(j, F(height), rec)
    nx = ex - ey
    ny = ex + ey
    ny = ny - F(1.0)
    nz = F(1.0) - np.abs(nx)
    nz = nz - np.abs(ny)
    assert (nz >= 0).all()                                           # oct_wrap (:239-244) is dead for uv in [0, 1)^2
    nl = nx * nx
    nl = nl + ny * ny
    nl = nl + nz * nz
    nl = _sqrt(nl, rec)
    e = np.stack([_div(nx, nl, rec), _div(nz, nl, rec), _div(ny, nl, rec)], -1)                    # .xzy
    assert e.dtype == F
    return e


def intersect_sphere_cam(dx, dy, dz, r, rec=None):   # clouds.glsl:97-105 with pos = camPos = (0, g_radius, 0): the larger root, NaN where the line misses
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
    d = _sqrt(d, rec)
    p = -b - d
    p2 = -b + d
    return _div(np.maximum(p, p2), F(2.0) * a, rec)


def ray(e, steps, rec=None):
    """The ray of directions float32 [..., 3] at `steps` primary steps (clouds.glsl:221-230, :143-145 with `steps` for 128): dict(p, inc, dir
    float32 [..., 3]; ss, t0 float32 [...]), t0 the distance of the shell entry p.  A direction with e.y <= 0 has no ray: its entries hold whatever
    the arithmetic gives, and nothing may read them."""
    e = np.asarray(e, F)
    dx, dy, dz = e[..., 0], e[..., 1], e[..., 2]
    n = F(steps)
    with np.errstate(invalid="ignore", divide="ignore"):
        t0 = intersect_sphere_cam(dx, dy, dz, RB, rec)
        t1 = intersect_sphere_cam(dx, dy, dz, RT, rec)
        sx, sy, sz = F(0.0) + dx * t0, RG + dy * t0, F(0.0) + dz * t0    # start, :224
        ex, ey, ez = F(0.0) + dx * t1, RG + dy * t1, F(0.0) + dz * t1    # end, :225
        qx, qy, qz = ex - sx, ey - sy, ez - sz
        sd = qx * qx
        sd = sd + qy * qy
        sd = sd + qz * qz
        sd = _sqrt(sd, rec)
        rx, ry, rz = _div(dx * sd, n, rec), _div(dy * sd, n, rec), _div(dz * sd, n, rec)   # :230
        ss = rx * rx
        ss = ss + ry * ry
        ss = ss + rz * rz
        ss = _sqrt(ss, rec)                                              # :143
        ux, uy, uz = _div(rx, ss, rec), _div(ry, ss, rec), _div(rz, ss, rec)   # :144
        inc = np.stack([ux * ss, uy * ss, uz * ss], -1)                  # dir * ss, :173
    assert ss.dtype == F and inc.dtype == F and t0.dtype == F
    return dict(p=np.stack([sx, sy, sz], -1), dir=np.stack([ux, uy, uz], -1), inc=inc, ss=ss, t0=t0)
