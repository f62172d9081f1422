"""The direct cloud march's definition (include/cloudsky.h) restated in numpy for the tests (test infrastructure, not product).

For pixel (i, j) of a W x H image, N = the context's primary steps:

    e        dirs form: the three floats of dirs[j * W + i], used as given
             view form: the compositor's EYEDIR of screen pixel (i, j): view_mode 1 with out_w = W, out_h = H, cam = view.basis,
                        tan(fov_y / 2) and aspect = W / H as csky_composite_view computes them
    accept   e.y > 0  and  0.99 <= (e.x*e.x + e.y*e.y) + e.z*e.z <= 1.01      float32, one operation per line; NaN fails every test
             not accepted: the texel is (0, 0, 0, 0) and the ray takes no sample
    ray      clouds.glsl:221-230, :143-145 from e: t0, t1 = intersectSphere(camPos, e, Rb / Rt); start, end; shelldist = |end - start|;
             raystep = e * shelldist / N; ss = |raystep|; dir = raystep / ss; inc = dir * ss; p = start      (tests/ray_reference.py)
    texel    march() of clouds.glsl:139-215 on that ray, exactly as the hemisphere frame's

Written from the definition, not from csrc/rays_core.h: float32 throughout, one operation per line in the order written (numpy's float32 add,
multiply, divide and sqrt are IEEE: exactly the operations of code compiled without contraction).  The one transcendental, tan(fov_y / 2), is
computed once per call on the host by the C library's tanf, which is not correctly rounded for every argument (for 70 degrees it is one ulp under
the rounded double value) and which numpy's float32 tan need not equal: the restatement calls the C library's."""
import ctypes
import ctypes.util

import numpy as np

from ray_reference import ray  # noqa: F401  (RR.ray: the one restatement of the ray, shared with the depth frame's)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.tanf.restype = ctypes.c_float
_libm.tanf.argtypes = [ctypes.c_float]

F = np.float32

VIEW = dict(width=64, height=36, fov=70.0, pitch=25.0, yaw=40.0)   # the camera of the view tests


def camera_basis(pitch_deg, yaw_deg):
    """3x3 float32, columns = the camera's right / up / back axes: looking down -z, pitched up by pitch_deg, then yawed about y by yaw_deg."""
    p, y = np.radians(pitch_deg), np.radians(yaw_deg)
    rx = np.array([[1, 0, 0], [0, np.cos(p), -np.sin(p)], [0, np.sin(p), np.cos(p)]])
    ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]])
    return (ry @ rx).astype(F)


def column_major(basis):
    """csky_view.basis: the nine floats, column by column."""
    return np.ascontiguousarray(np.asarray(basis, F).T.reshape(-1))


def tan_half_fov(fov_y_degrees):
    a = F(fov_y_degrees) * F(0.5)
    a = a * F(3.14159265358979323846)
    a = a / F(180.0)
    return F(_libm.tanf(float(a)))


def view_dirs(basis, fov_y_degrees, width, height):
    """float32 [height, width, 3]: EYEDIR of every screen pixel, the order written in composite_core.h composite_eyedir (view_mode 1)."""
    cam = column_major(basis)
    i = np.arange(width, dtype=F)[None, :] + np.zeros((height, 1), F)
    j = np.arange(height, dtype=F)[:, None] + np.zeros((1, width), F)
    u = (i + F(0.5)) / F(width)
    v = (j + F(0.5)) / F(height)
    th = tan_half_fov(fov_y_degrees)
    aspect = F(width) / F(height)
    vx = u * F(2.0)
    vx = vx - F(1.0)
    vx = vx * th
    vx = vx * aspect
    vy = v * F(2.0)
    vy = F(1.0) - vy
    vy = vy * th
    vz = F(-1.0)

    def row(k):
        w = cam[k] * vx
        w = w + cam[3 + k] * vy
        w = w + cam[6 + k] * vz
        return w
    wx, wy, wz = row(0), row(1), row(2)
    l = wx * wx
    l = l + wy * wy
    l = l + wz * wz
    l = np.sqrt(l)
    return np.stack([wx / l, wy / l, wz / l], axis=-1).astype(F)


def accept(e):
    """bool [...]: which directions float32 [..., 3] are marched."""
    e = np.asarray(e, F)
    x, y, z = e[..., 0], e[..., 1], e[..., 2]
    with np.errstate(all="ignore"):
        l2 = x * x
        l2 = l2 + y * y
        l2 = l2 + z * z
        return (y > F(0.0)) & (l2 >= F(0.99)) & (l2 <= F(1.01))
