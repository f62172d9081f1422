"""What csky_set_noise builds from three 8-bit textures, restated in numpy: the 2x2x2 box mips, the polynomial cells of the three device layouts
(csrc/csky_common.h) as fp16 pairs and as exact fp32, the unpacked fp16 detail chain, and the values the context keeps from the bake (inexact
count, weather range, detail LOD 5).

Written from the layouts' description, with whole-array arithmetic: forward differences with wrap instead of per-texel corner gathers, numpy's
float16 conversion instead of f2h.  It includes and imports nothing of csrc/bake_core.h, csrc/bake.h or tests/hostsim -- the host bake is the
same header as the device bake, so a wrong sign, a wrong wrap or a wrong level offset passes a comparison of those two.
tests/test_bake_reference.py holds this file against the host bake, tests/test_gpu_bake.py holds the kernels against this file.

Arrays are indexed [z, y, x, channel] (volumes) and [y, x, channel] (the weather map): x is the last spatial axis and the fastest in memory."""
import numpy as np

SHAPE_N, SHAPE_LEVELS = 128, 8          # RGBA8
DETAIL_N, DETAIL_LEVELS = 32, 6         # RGB8
WEATHER_N = 512                         # RGB8, no mips


def mips(level0, levels):
    """The levels of a box-filtered chain as [n, n, n, ch] uint8 arrays, level 0 first: each texel is (sum of its 2x2x2 parents + 4) >> 3."""
    a = np.ascontiguousarray(level0, np.uint8)
    if a.ndim != 4 or not (a.shape[0] == a.shape[1] == a.shape[2]) or levels < 1 or (a.shape[0] >> (levels - 1)) < 1:
        raise ValueError("mips: a cube [n, n, n, ch] and 1 <= levels with n >> (levels - 1) >= 1")
    out = [a]
    for l in range(1, levels):
        nd, ch = a.shape[0] >> l, a.shape[3]
        p = out[-1][:2 * nd, :2 * nd, :2 * nd].astype(np.uint32)
        s = p.reshape(nd, 2, nd, 2, nd, 2, ch).sum(axis=(1, 3, 5))
        out.append(((s + 4) >> 3).astype(np.uint8))
    return out


def chain(levels):
    """The levels back to back as flat bytes, level 0 first."""
    return np.concatenate([np.ascontiguousarray(l, np.uint8).reshape(-1) for l in levels])


def split_chain(flat, n, ch, levels):
    """The inverse of chain()."""
    out, off = [], 0
    for l in range(levels):
        m = n >> l
        out.append(np.asarray(flat[off:off + m * m * m * ch], np.uint8).reshape(m, m, m, ch))
        off += m * m * m * ch
    if off != len(flat):
        raise ValueError("split_chain: %d bytes for a chain of %d" % (len(flat), off))
    return out


def cells(v, ndim):
    """Polynomial-cell coefficients of the cell that starts at every texel of the integer array v, whose LAST ndim axes are spatial (x last):
    forward differences with wrap (REPEAT addressing).  Returns v.shape + (2**ndim,), indexed by the bit mask x | y<<1 | z<<2 of the axes
    differenced: [0] the value, [1] d_x, [2] d_y, [3] d_xy, [4] d_z, [5] d_xz, [6] d_yz, [7] d_xyz."""
    v = np.asarray(v)
    if v.dtype.kind != "i":
        raise TypeError("cells: a signed integer array (differences go negative)")
    c = {0: v}
    for bit in range(ndim):
        axis = v.ndim - 1 - bit
        for mask in [m for m in c if m < (1 << bit)]:
            c[mask | (1 << bit)] = np.roll(c[mask], -1, axis) - c[mask]
    return np.stack([c[m] for m in range(1 << ndim)], axis=-1)


def halves(c):
    """Integer coefficients -> (float16 array, how many of them the half does not hold exactly).  Round to nearest even."""
    f = c.astype(np.float32)
    h = f.astype(np.float16)
    return h, int((h.astype(np.float32) != f).sum())


def shape_channels(level):
    """The two values the shape layout stores per RGBA8 texel: R, and the fbm numerator 5g + 2b + a."""
    t = level.astype(np.int32)
    return t[..., 0], 5 * t[..., 1] + 2 * t[..., 2] + t[..., 3]


def detail_numerator(level):
    t = level.astype(np.int32)
    return 5 * t[..., 0] + 2 * t[..., 1] + t[..., 2]


def _texels(parts):
    """Per-texel records: the coefficient arrays of `parts` side by side on the last axis, texels x fastest, then y, then z (C order)."""
    return np.ascontiguousarray(np.concatenate(parts, axis=-1))


def shape_cells(levels, rank):
    """Integer cells of every level: per texel the eight coefficients of R, then the eight of the fbm numerator.  Rank 3 only (xyz cells, 32 bytes
    per texel as halves); the build's other ranks store other records and are not guessed here."""
    if rank != 3:
        raise NotImplementedError("bake_reference: the shape layout of CSKY_SHAPE_POLY == %r is not restated (only rank 3)" % (rank,))
    return [_texels([cells(ch, 3) for ch in shape_channels(l)]) for l in levels]


def detail_cells(levels):
    return [cells(detail_numerator(l), 3) for l in levels]


def weather_cells(weather):
    """Per texel {R: c0..c3}{B: c0..c3}; G is not stored."""
    w = np.asarray(weather, np.uint8).reshape(WEATHER_N, WEATHER_N, 3).astype(np.int32)
    return _texels([cells(w[..., 0], 2), cells(w[..., 2], 2)])


def _bytes(arrays):
    return np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in arrays])


class Bake:
    """Everything a bind of (large [128,128,128,4], small [32,32,32,3], weather [512,512,3]) leaves on the device and in the context, as flat uint8
    byte arrays in the order csky_read_baked_texture numbers them, plus the derived values."""

    def __init__(self, large, small, weather, rank=3):
        large = np.ascontiguousarray(large, np.uint8).reshape(SHAPE_N, SHAPE_N, SHAPE_N, 4)
        small = np.ascontiguousarray(small, np.uint8).reshape(DETAIL_N, DETAIL_N, DETAIL_N, 3)
        self.weather_rgb = np.ascontiguousarray(weather, np.uint8).reshape(WEATHER_N, WEATHER_N, 3)
        self.large_levels, self.small_levels = mips(large, SHAPE_LEVELS), mips(small, DETAIL_LEVELS)
        self.large_chain, self.small_chain = chain(self.large_levels), chain(self.small_levels)           # which 3, 4
        sc, dc, wc = shape_cells(self.large_levels, rank), detail_cells(self.small_levels), weather_cells(self.weather_rgb)
        self.inexact = 0
        packed = []
        for group in (sc, dc, [wc]):
            hs = [halves(c) for c in group]
            self.inexact += sum(bad for _, bad in hs)
            packed.append(_bytes([h for h, _ in hs]))
        self.shape, self.detail, self.weather = packed                                                     # which 0, 1, 2
        self.detail_h = _bytes([halves(detail_numerator(l))[0] for l in self.small_levels])                # which 5 (not counted: 0..2040 fit)
        self.shape32, self.detail32, self.weather32 = (_bytes([c.astype(np.float32) for c in g]) for g in (sc, dc, [wc]))   # which 6, 7, 8
        r, b = self.weather_rgb[..., 0], self.weather_rgb[..., 2]
        self.range = (int(r.min()), int(r.max()), int(b.max()))
        self.lod5 = np.float32(int(detail_numerator(self.small_levels[5])[0, 0, 0])) * np.float32(1.0 / (8 * 255))

    def held(self):
        """The 24 bytes of which == 9: uint64 inexact; int32 rmin, rmax, bmax; float32 lod5."""
        rec = np.zeros(1, np.dtype([("inexact", "<u8"), ("rmin", "<i4"), ("rmax", "<i4"), ("bmax", "<i4"), ("lod5", "<f4")]))
        rec["inexact"], (rec["rmin"], rec["rmax"], rec["bmax"]), rec["lod5"] = self.inexact, self.range, self.lod5
        return rec.view(np.uint8)


# ---- the two texture sets both test files bind
def white_noise_set():
    """Set W: white noise, the worst case for fp16 cells."""
    rng = np.random.default_rng(11)                                # drawn as bytes, in this order: 105498 inexact coefficients
    return tuple(rng.integers(0, 256, shape, dtype=np.uint8) for shape in ((128, 128, 128, 4), (32, 32, 32, 3), (512, 512, 3)))


def ramp_volume(n, coeffs):
    """Channel i is (a x + b y + c z + k) % 251 with coeffs[i] = (a, b, c, k): smooth inside, a jump at the wrap seam of every axis (n a, n b, n c
    are no multiples of 251), so addressing that clamps where it should repeat shows in exactly the seam cells of every level."""
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    return np.stack([((a * x + b * y + c * z + k) % 251) for a, b, c, k in coeffs], axis=-1).astype(np.uint8)


def seam_weather(r=128, g=9, b=77, spikes=True):
    """A constant map, with three single texels that alone set the range: the first lane of the first wave, the last lane of the last wave and a
    lane 63 of the device's 64-lane reductions."""
    w = np.empty((WEATHER_N, WEATHER_N, 3), np.uint8)
    w[...] = (r, g, b)
    if spikes:
        w[0, 0, 0], w[511, 511, 0], w[200, 63, 2] = 250, 3, 201
    return w


def seam_set():
    """Set S."""
    return (ramp_volume(128, ((1, 3, 5, 0), (3, 5, 7, 40), (5, 7, 1, 90), (7, 1, 3, 170))), ramp_volume(32, ((3, 1, 7, 11), (5, 3, 1, 100), (1, 7, 5, 200))),
            seam_weather())


# ---- the mip builders' cases, host and device
MIP_SHAPES = [(2, 1, 2), (2, 4, 1), (4, 2, 3), (8, 3, 4), (16, 4, 5), (64, 1, 7)]      # (n, channels, levels)


def mip_inputs(n, ch):
    """name -> level 0: random bytes, all 255 (the largest sum: 2040 + 4), and every 2x2x2 group summing to 8k + 4, the half that rounds UP."""
    rng = np.random.default_rng(100 * n + ch)
    k = rng.integers(0, 255, (n // 2, n // 2, n // 2, ch))                            # k <= 254: four parents k, four k + 1
    up = np.repeat(np.repeat(np.repeat(k, 2, 0), 2, 1), 2, 2)
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    up = up + ((x + y + z) & 1)[..., None]                                             # a 3-D checkerboard: 4 of every 2x2x2 group
    return {"random": rng.integers(0, 256, (n, n, n, ch)).astype(np.uint8), "all255": np.full((n, n, n, ch), 255, np.uint8),
            "half_up": up.astype(np.uint8), "half_up_k": k}
