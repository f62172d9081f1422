"""Host mirror of cloud_sky/cloud_sky.gd (the `Sky` resource that drives clouds.glsl).

Same property names, defaults, call order and push-constant packing as the GDScript, over the C ABI of
libcloudsky.so.  Differences, all deliberate (BASELINE.json north_star):
  * `frames_to_update = 1` is allowed and is the default: the full hemisphere is rendered every call instead of
    being split over 64 frames (the reference's 4/16/64/256 temporal split is still available);
  * the texture may be rectangular (`texture_size = (W, H)`; the shader's `texture_size` is a vec2, clouds.glsl:19);
  * `clock` is injectable (the reference reads `Time.get_ticks_msec()`, cloud_sky.gd:176) so that benchmarks and
    tests can freeze the wind;
  * textures are numpy float16 arrays (host form) or torch int16 CUDA tensors (device form, `device_buffers=True`).
"""
import math
import time as _time

import numpy as np

from . import assets as _assets
from . import tiling as _tiling
from ._lib import Context
from ._lib import _observer
from ._lib import _scene_depth
from ._lib import aerial_shadow_rect as _aerial_shadow_rect
from .sky_lut import SkyLut
from .transmittance_lut import TransmittanceLut


def srgb_to_linear(c):
    """Color.srgb_to_linear() (cloud_sky.gd:79)."""
    c = np.asarray(c, np.float64)
    return np.where(c < 0.04045, c * (1.0 / 12.92), ((c + 0.055) * (1.0 / 1.055)) ** 2.4).astype(np.float32)


class FrameData:
    """cloud_sky.gd:56-79: everything the compute shader reads, frozen for a whole update pass."""

    def __init__(self):
        self.wind_direction = np.array([1.0, 0.0])
        self.wind_speed = 1.0
        self.density = 0.05
        self.cloud_coverage = 0.25
        self.time_offset = 0.0
        self.ground_color = np.array([1.0, 1.0, 1.0, 1.0])
        self._time = 0.0
        self._cloud_pos = np.zeros(2)
        self._detailed_pos = np.zeros(2)
        self._weather_pos = np.zeros(2)
        self.LIGHT_DIRECTION = np.array([0.0, -1.0, 0.0])   # cloud_sky.gd:72 (no light attached: sun below horizon)
        self.LIGHT_ENERGY = 1.0
        self.LIGHT_COLOR = np.array([1.0, 1.0, 1.0, 1.0])

    def update_light_data(self, light):  # cloud_sky.gd:76-79
        b = np.asarray(light.basis, np.float64)  # 3x3, columns = basis vectors
        d = b @ np.array([0.0, 0.0, 1.0])
        self.LIGHT_DIRECTION = d / np.linalg.norm(d)
        self.LIGHT_ENERGY = float(light.light_energy)
        c = np.asarray(light.light_color, np.float64)
        self.LIGHT_COLOR = np.concatenate([srgb_to_linear(c[:3]), c[3:4] if c.size > 3 else [1.0]])


class DirectionalLight:
    """Stand-in for the DirectionalLight3D that sun.gd registers (sun.gd:11-13): only what update_light_data reads."""

    def __init__(self, direction=None, basis=None, light_energy=1.0, light_color=(1.0, 1.0, 1.0, 1.0)):
        if basis is None:
            d = np.asarray(direction, np.float64)
            d = d / np.linalg.norm(d)
            basis = np.zeros((3, 3))
            basis[:, 2] = d                      # basis * (0,0,1) = third column = direction towards the sun
        self.basis = np.asarray(basis, np.float64)
        self.light_energy = light_energy
        self.light_color = light_color


class CloudSky:
    """cloud_sky.gd.  Construct, optionally set `sun`, then call `update_sky()` once per frame."""

    FRAMES_TO_UPDATE_CHOICES = (1, 4, 16, 64, 256)   # cloud_sky.gd:36 plus 1 = full hemisphere per call

    def __init__(self, device_id=0, texture_size=768, frames_to_update=1, noise=None, clock=None, device_buffers=False,
                 rank=0, world_size=1, dist=None, ctx=None, async_host=False, mapping=None):
        # exported properties, cloud_sky.gd:5-50 with the defaults of the script (clouds_sky.tres overrides some)
        self.wind_direction = 0.0
        self.wind_speed = 1.0
        self.density = 0.05
        self.cloud_coverage = 0.25
        self.time_offset = 0.0
        self.sun_disk_scale = 1.0
        self.ground_color = np.array([1.0, 1.0, 1.0, 1.0])
        self._frames_to_update = int(frames_to_update)
        self._texture_size = self._as_size(texture_size)
        self.sun = None
        self.frame_data = FrameData()
        self.update_position = [0, 0]
        self.update_region_size = [96, 96]
        self.num_workgroups = [12, 12]
        self.textures = [None, None, None]
        self.texture_to_update, self.texture_to_blend_from, self.texture_to_blend_to = 0, 1, 2
        self.frame = 0
        self.blend_amount = 0.0
        self.can_run = False
        self.needs_full_sky_init = True
        if clock is None:           # Time.get_ticks_msec() counts from engine start (cloud_sky.gd:176): seconds since construction, so the
            t0 = _time.monotonic()  # first delta is ~0 like the reference's and wind offsets stay in fp32's accurate range
            clock = lambda: _time.monotonic() - t0  # noqa: E731
        self.clock = clock
        self.device_buffers = bool(device_buffers)
        # async_host: the host-buffer path through csky_submit_clouds / csky_collect (what the GDExtension's submit_clouds() / collect() wrap,
        # INTEGRATION.md): _render_process() collects the tile submitted by the PREVIOUS call into its texture and submits this call's tile, so
        # march + copy of one tile overlap the host's work on the next; the textures trail by one call, flush() collects the last tile.  The
        # reference's loop tolerates that by construction: it draws with the textures finished in earlier passes (cloud_sky.gd:137-148).
        self.async_host = bool(async_host) and not self.device_buffers
        self._pending = None
        self.rank, self.world_size, self.dist = int(rank), int(world_size), dist
        self.last_frame = None
        self._side_stream = None
        self._temporal = None            # cloud_view_temporal's history
        # the sky's radiance cubemap (radiance_cubemap / update_radiance): [L, 6, S, S, 4] float16, its (S, L, Ss) and the layer the next
        # update_radiance() call refreshes
        self.radiance = None
        self._radiance_geom = None
        self._radiance_next = 0
        # render-thread side (cloud_sky.gd:218-232): the C-ABI context owns every device resource
        self.ctx = ctx if ctx is not None else Context(device_id)
        self.mapping = mapping           # the transmittance LUT's parametrization: 'reference', 'bruneton' (cloudsky.h CSKY_TLUT_*) or None = the context's own (reference unless changed)
        self.transmittance_tex = TransmittanceLut(self.ctx, mapping=mapping)   # cloud_sky.gd:92
        self.sky_lut = SkyLut(self.ctx, self.transmittance_tex, device_buffers=self.device_buffers)   # cloud_sky.gd:91
        large, small, weather = noise if noise is not None else _assets.load_default_noise()
        self.ctx.set_noise(large, small, weather)                              # _create_noise_uniform_set, :298-341
        self.update_performance()

    def set_weather(self, weather=None, *, seed=None, **knobs):
        """Replace the weather map alone (cloud type in R, coverage in B) between two passes: `weather` is a numpy uint8 [512, 512, 3] array or a
        contiguous uint8 CUDA tensor of that shape on the context's device (csky_set_weather / csky_set_weather_device); or, with `seed`, the map of
        assets.generate_weather(seed, **knobs) generated on the GPU (csky_set_weather_generated).  The call waits for the device; tiles marched
        before it are of the old map, later ones of the new: the textures change over one tile at a time, as they do when the sun moves
        (request_full_sky_init() for a cut).  The temporal split's history is dropped."""
        if (weather is None) == (seed is None):
            raise ValueError("set_weather: give a weather map or a seed")
        if weather is not None:
            if knobs:
                raise ValueError("set_weather: generator knobs go with a seed, not with a map")
            self.ctx.set_weather(weather)
        else:
            self.ctx.set_weather_generated(seed, **knobs)
        self._temporal = None

    # ---- clouds_sky.tres:11-18 ----------------------------------------------------------------------------
    @classmethod
    def from_default_resource(cls, **kw):
        """The demo's `clouds_sky.tres` values (the benchmark configuration)."""
        sky = cls(**kw)
        sky.wind_direction, sky.wind_speed = 0.0, 1.0
        sky.density, sky.cloud_coverage, sky.time_offset = 0.05, 0.2, 0.0
        sky.sun_disk_scale = 2.0
        sky.ground_color = np.array([0.270588, 0.188235, 0.027451, 1.0])
        return sky

    @staticmethod
    def _as_size(v):
        if np.isscalar(v):
            return [int(v), int(v)]
        return [int(v[0]), int(v[1])]

    @property
    def frames_to_update(self):
        return self._frames_to_update

    @frames_to_update.setter
    def frames_to_update(self, value):  # cloud_sky.gd:37-42
        self._frames_to_update = int(value)
        self.cleanup()
        self.update_performance()
        self.request_full_sky_init()

    @property
    def texture_size(self):
        return tuple(self._texture_size)

    @texture_size.setter
    def texture_size(self, value):  # cloud_sky.gd:45-50
        self._texture_size = self._as_size(value)
        self.cleanup()
        self.update_performance()
        self.request_full_sky_init()

    def update_performance(self):  # cloud_sky.gd:109-118
        if self._frames_to_update not in self.FRAMES_TO_UPDATE_CHOICES:
            raise ValueError("frames_to_update must be one of %s" % (self.FRAMES_TO_UPDATE_CHOICES,))
        frames_sqrt = int(math.isqrt(self._frames_to_update))
        for k in range(2):
            self.update_region_size[k] = self._texture_size[k] // frames_sqrt
            if self._texture_size[k] % frames_sqrt != 0:
                self._texture_size[k] = self.update_region_size[k] * frames_sqrt
                print("texture_size is not a multiple of sqrt(frames_to_update), changing to: ", self._texture_size[k])
            self.num_workgroups[k] = (self.update_region_size[k] + 7) // 8
        self._initialize_compute_code()

    def request_full_sky_init(self):  # cloud_sky.gd:120-121
        self.needs_full_sky_init = True

    def initialize_sky(self):  # cloud_sky.gd:124-127
        self._update_per_frame_data()
        for _ in range(self._frames_to_update * 2):
            self.update_sky()

    def update_sky(self):  # cloud_sky.gd:129-163
        if not self.can_run:
            return None
        if self.needs_full_sky_init:
            self.needs_full_sky_init = False
            self.initialize_sky()
        if self.frame >= self._frames_to_update:
            self.texture_to_update = (self.texture_to_update + 1) % 3
            self.texture_to_blend_from = (self.texture_to_blend_from + 1) % 3
            self.texture_to_blend_to = (self.texture_to_blend_to + 1) % 3
            self._update_per_frame_data()  # only once per pass, otherwise tiles get out of sync (cloud_sky.gd:142)
            self.frame = 0
        self.blend_amount = float(self.frame) / float(self._frames_to_update)
        out = self._render_process(self.texture_to_update)
        self.update_position[0] += self.update_region_size[0]
        if self.update_position[0] >= self._texture_size[0]:
            self.update_position[0] = 0
            self.update_position[1] += self.update_region_size[1]
        if self.update_position[1] >= self._texture_size[1]:
            self.update_position = [0, 0]
        self.frame += 1
        return out

    def _update_per_frame_data(self):  # cloud_sky.gd:165-187
        fd = self.frame_data
        if self.sun is not None:
            fd.update_light_data(self.sun)
        fd.wind_direction = np.array([math.cos(self.wind_direction), math.sin(self.wind_direction)])  # Vector2.from_angle
        fd.wind_speed = self.wind_speed
        fd.density = self.density
        fd.cloud_coverage = self.cloud_coverage
        fd.time_offset = self.time_offset
        fd.ground_color = np.asarray(self.ground_color, np.float64)
        t = float(self.clock())
        delta = t - fd._time
        delta2 = delta * 0.001 + 0.005 * fd.time_offset
        wdn = fd.wind_direction / np.linalg.norm(fd.wind_direction)
        fd._time = t
        fd._detailed_pos = fd._detailed_pos + delta * wdn
        fd._cloud_pos = fd._cloud_pos + delta * wdn * fd.wind_speed
        fd._weather_pos = fd._weather_pos + delta2 * wdn * fd.wind_speed
        stream, done = self._march_stream()
        self.sky_lut.update_lut(fd.LIGHT_DIRECTION, stream)
        done()

    def flush(self):
        """async_host: wait for the tile in flight (if any) and write it into its texture."""
        if self._pending is not None:
            ticket, texidx, (x0, y0, rw, rh) = self._pending
            self._pending = None
            tile = self.ctx.collect(ticket, copy=False)
            if self.textures[texidx] is not None:
                self.textures[texidx][y0:y0 + rh, x0:x0 + rw] = tile

    def cleanup(self):  # cloud_sky.gd:197-212
        if getattr(self, "_pending", None) is not None:                     # a tile of the old geometry is in flight: drop it
            try:
                self.ctx.collect(self._pending[0], copy=False)
            except Exception:
                pass
            self._pending = None
        self.can_run = False
        self.frame = 0
        self.texture_to_update, self.texture_to_blend_from, self.texture_to_blend_to = 0, 1, 2
        self.update_position = [0, 0]
        self.textures = [None, None, None]
        self._temporal = None                                               # cloud_view_temporal's two frames, previous camera and call counter

    def close(self):  # NOTIFICATION_PREDELETE, cloud_sky.gd:193-195
        self.cleanup()
        self.ctx.close()

    def sky_panorama(self, out_w=2048, out_h=1024):
        """What clouds_material.tres + clouds.gdshader draw: the two blend textures cross-faded by blend_amount over the
        atmosphere with the sun disk, evaluated on an equirectangular panorama (csky_composite_sky).  float16 [h, w, 4]."""
        def host(t):
            return t.cpu().numpy() if hasattr(t, "cpu") else t
        self.flush()
        bf, bt = host(self.textures[self.texture_to_blend_from]), host(self.textures[self.texture_to_blend_to])
        sf, st = (host(t) for t in self.sky_lut.back_texture)   # sky_blend_from/to_texture = the two OLDER ring copies (cloud_sky.gd:147-148)
        return self.ctx.composite_sky(bf, bt, sf, st, self.frame_data.LIGHT_DIRECTION, self.blend_amount, self.sun_disk_scale, out_w, out_h)

    def cloud_view(self, basis, fov_y_degrees=75.0, out_w=1152, out_h=648, aerial=False, aerial_steps=16, position=None, max_distance=float("inf"), scene_depth=None,
                   depth_kind="distance"):
        """The clouds of the current frame data marched along the rays of a perspective camera's SCREEN pixels instead of the hemisphere frame's
        (csky_render_clouds_view; the definition: include/cloudsky.h): float16 [out_h, out_w, 4], what the hemisphere frame would store for each
        ray, at the camera's own angular resolution; zero under the horizon.  The block _fill_push_constant() packs, the context's step counts.
        basis as sky_view takes it.  A torch CUDA tensor with device_buffers=True.  Not called by update_sky().
        aerial=True: the air in front of the view's clouds under the current sun, aerial_steps steps per pixel (the view's own depth frame, then
        csky_apply_cloud_aerial_view; with device_buffers=True the three kernels run back to back on the march stream).  Alpha is unchanged.
        position: the observer's place, three numbers in metres from the reference's camera (y up; under, inside or above the layer), with
        max_distance the cap on a ray's length from there (csky_render_clouds_view_from).  None: the reference's observer, the call made without it.
        The aerial step is the ground observer's: aerial=True with a position is a ValueError.
        scene_depth: the host's scene in front of the camera, float32 [out_h, out_w] metres along each pixel's ray (depth_kind "distance") or along
        the camera's forward axis ("view_z"): each ray ends at its pixel's depth, so the frame holds the cloud in front of the geometry
        (csky_render_clouds_view_from_depth).  A numpy array without device_buffers, a torch CUDA tensor with them.  Beside it position=None
        means (0, 0, 0); aerial=True is refused as beside a position."""
        if (position is not None or scene_depth is not None) and aerial:
            raise ValueError("cloud_view: aerial=True is the ground observer's step and takes no position and no scene depth")
        if scene_depth is not None and position is None:
            position = (0.0, 0.0, 0.0)
        pc = self._fill_push_constant()
        sun = self.frame_data.LIGHT_DIRECTION
        if position is not None:
            _observer("cloud_view", position, max_distance)      # refused before a frame is allocated
            if scene_depth is not None:
                if _scene_depth("cloud_view", scene_depth, depth_kind, out_w, out_h, True)[1] != bool(self.device_buffers):
                    raise ValueError("cloud_view: scene_depth must be a numpy array without device_buffers and a tensor on the GPU with them")
                march, extra = self.ctx.render_clouds_view_from_depth, (scene_depth, depth_kind, max_distance)
            else:
                march, extra = self.ctx.render_clouds_view_from, (max_distance,)
            if not self.device_buffers:
                return march(pc, basis, fov_y_degrees, out_w, out_h, position, *extra)
            import torch
            out = torch.empty((int(out_h), int(out_w), 4), dtype=torch.float16, device=torch.device("cuda", self.ctx.device_id))
            stream, done = self._march_stream()
            march(pc, basis, fov_y_degrees, out_w, out_h, position, *extra, out=out, stream=stream)
            done()
            return out
        if not self.device_buffers:
            cv = self.ctx.render_clouds_view(pc, basis, fov_y_degrees, out_w, out_h)
            if not aerial:
                return cv
            return self.ctx.apply_cloud_aerial_view(sun, basis, fov_y_degrees, cv, self.ctx.render_cloud_depth_view(pc, basis, fov_y_degrees, out_w, out_h),
                                                    aerial_steps)
        import torch
        dev = torch.device("cuda", self.ctx.device_id)
        out = torch.empty((int(out_h), int(out_w), 4), dtype=torch.float16, device=dev)
        stream, done = self._march_stream()
        self.ctx.render_clouds_view(pc, basis, fov_y_degrees, out_w, out_h, out=out, stream=stream)
        if aerial:
            depth = torch.empty((int(out_h), int(out_w), 4), dtype=torch.float16, device=dev)
            self.ctx.render_cloud_depth_view(pc, basis, fov_y_degrees, out_w, out_h, out=depth, stream=stream)   # the apply step reads both on the same stream
            self.ctx.apply_cloud_aerial_view(sun, basis, fov_y_degrees, out, depth, aerial_steps, out=out, stream=stream)   # in place
        done()
        return out

    TEMPORAL_BLOCK_CHOICES = (1, 2, 4, 8)

    @staticmethod
    def temporal_phases(block):
        """The order in which the block x block pixels of a block are refreshed: phase k of the list is the pixel (phase % block, phase // block)
        whose ordered-dither (Bayer) index is k, so that any run of consecutive calls spreads its fresh pixels evenly over the block."""
        m = [[0]]
        while len(m) < block:                                    # M(2n) = [[4M, 4M + 2], [4M + 3, 4M + 1]]
            m = [[4 * v for v in r] + [4 * v + 2 for v in r] for r in m] + [[4 * v + 3 for v in r] + [4 * v + 1 for v in r] for r in m]
        order = [0] * (block * block)
        for y, row in enumerate(m):
            for x, v in enumerate(row):
                order[v] = y * block + x
        return order

    def cloud_view_temporal(self, basis, fov_y_degrees=75.0, out_w=1152, out_h=648, block=4):
        """cloud_view spread over block * block calls (csky_render_clouds_view_update; the definition: include/cloudsky.h): each call marches one
        pixel of every block x block pixels, in the order of temporal_phases(block), and takes the others from the frame of the call before
        through that call's camera; what that frame does not cover is marched.  The first call, and the first after a change of the size or of
        `block` or after cleanup(), has no history and marches every pixel.  With a still camera and unchanged frame data, block * block calls
        give cloud_view's frame; with changing frame data a pixel is up to block * block - 1 calls old.  The object keeps two frames and
        alternates between them: the returned frame is valid until the call after the next.  float16 [out_h, out_w, 4]; a torch CUDA tensor with
        device_buffers=True.  Not called by update_sky()."""
        if block not in self.TEMPORAL_BLOCK_CHOICES:
            raise ValueError("block must be one of %s" % (self.TEMPORAL_BLOCK_CHOICES,))
        key = (int(out_w), int(out_h), int(block))
        t = self._temporal
        if t is None or t["key"] != key:
            t = self._temporal = {"key": key, "frames": [None, None], "prev": None, "calls": 0}
        shape = (key[1], key[0], 4)
        at = t["calls"] % 2
        if t["frames"][at] is None:
            if self.device_buffers:
                import torch
                t["frames"][at] = torch.empty(shape, dtype=torch.float16, device=torch.device("cuda", self.ctx.device_id))
            else:
                t["frames"][at] = np.zeros(shape, np.float16)
        out = t["frames"][at]
        prev, prev_view = (t["frames"][1 - at], t["prev"]) if t["prev"] is not None else (None, (None, None))
        phase = self.temporal_phases(block)[t["calls"] % (block * block)]
        stream, done = self._march_stream()
        self.ctx.render_clouds_view_update(self._fill_push_constant(), basis, fov_y_degrees, key[0], key[1], block, phase, prev=prev, prev_basis=prev_view[0],
                                           prev_fov=prev_view[1], out=out, stream=stream)
        done()
        t["prev"] = (np.array(basis, np.float32), float(fov_y_degrees))
        t["calls"] += 1
        return out

    def cloud_view_depth(self, basis, fov_y_degrees=75.0, out_w=1152, out_h=648):
        """Where along each ray of cloud_view's image the clouds of the current frame data sit: the mean, first and last distance from the
        observer in km and the view frame's alpha, float16 [out_h, out_w, 4] at the context's step count, so that the samples are the view
        frame's (csky_render_cloud_depth_view; the definition: include/cloudsky.h).  A torch CUDA tensor with device_buffers=True.  Independent
        of the sky LUTs and of the blend textures; not called by update_sky()."""
        pc = self._fill_push_constant()
        if not self.device_buffers:
            return self.ctx.render_cloud_depth_view(pc, basis, fov_y_degrees, out_w, out_h)
        import torch
        out = torch.empty((int(out_h), int(out_w), 4), dtype=torch.float16, device=torch.device("cuda", self.ctx.device_id))
        stream, done = self._march_stream()
        self.ctx.render_cloud_depth_view(pc, basis, fov_y_degrees, out_w, out_h, out=out, stream=stream)
        done()
        return out

    def sky_view(self, basis, fov_y_degrees=75.0, out_w=1152, out_h=648, direct=False, aerial=False):
        """The same through a perspective camera: one EYEDIR per SCREEN pixel, the way the engine evaluates clouds.gdshader
        (csky_composite_view).  basis: 3x3, columns = the camera's right / up / back axes (Camera3D.global_transform.basis).
        direct=True: the clouds are marched for this very view (cloud_view) instead of tapped from the hemisphere frames, and composited with
        csky_composite_view_frames; both cloud images are that one frame, so blend_amount has no effect on the clouds.
        aerial=True (with direct=True only: ValueError otherwise): the view frame gets the air in front of its clouds before it is composited
        (cloud_view(aerial=True)); for the hemisphere frames that step is aerial_clouds()."""
        def host(t):
            return t.cpu().numpy() if hasattr(t, "cpu") else t
        if aerial and not direct:
            raise ValueError("sky_view: aerial=True needs direct=True (the hemisphere frames take their air from aerial_clouds())")
        self.flush()
        if direct:
            cv = host(self.cloud_view(basis, fov_y_degrees, out_w, out_h, aerial=aerial))
            sf, st = (host(t) for t in self.sky_lut.back_texture)
            return self.ctx.composite_view_frames(cv, cv, sf, st, self.frame_data.LIGHT_DIRECTION, basis, fov_y_degrees, self.blend_amount, self.sun_disk_scale)
        bf, bt = host(self.textures[self.texture_to_blend_from]), host(self.textures[self.texture_to_blend_to])
        sf, st = (host(t) for t in self.sky_lut.back_texture)
        return self.ctx.composite_view(bf, bt, sf, st, self.frame_data.LIGHT_DIRECTION, basis, fov_y_degrees, self.blend_amount, self.sun_disk_scale, out_w, out_h)

    def radiance_cubemap(self, face_size=64, layers=8, source_size=0):
        """The sky's radiance cubemap, all layers now: layer 0 = the same sky() as sky_panorama on the six faces of a face_size cube map,
        layers 1..L-1 GGX-prefiltered for roughness k / (L-1) (csky_render_radiance; layout and maths: include/cloudsky.h).  clouds_sky.tres
        asks the engine for 64 x 64 faces; 8 layers is the engine's default.  float16 [L, 6, S, S, 4] (a torch CUDA tensor with
        device_buffers=True).  Not called by update_sky()."""
        self._radiance_setup(face_size, layers, source_size)
        self._radiance_render(0, layers)
        self._radiance_next = 0
        return self.radiance

    def update_radiance(self, face_size=64, layers=8, source_size=0):
        """Incremental processing (the engine's PROCESS_MODE_INCREMENTAL, clouds_sky.tres process_mode = 2): each call refreshes ONE layer,
        cycling 0, 1, ..., L-1; layer 0 re-renders the faces and takes the source cube the following layers filter.  A change of
        (face_size, layers, source_size) starts over at layer 0.  Returns the cubemap array (self.radiance)."""
        if self._radiance_geom != (int(face_size), int(layers), int(source_size)):
            self._radiance_setup(face_size, layers, source_size)
            self._radiance_next = 0
        k = self._radiance_next
        self._radiance_render(k, 1)
        self._radiance_next = (k + 1) % int(layers)
        return self.radiance

    def _radiance_setup(self, face_size, layers, source_size):
        S, L = int(face_size), int(layers)
        geom = (S, L, int(source_size))
        if self._radiance_geom != geom or self.radiance is None:
            if self.device_buffers:
                import torch
                self.radiance = torch.zeros((L, 6, S, S, 4), dtype=torch.float16, device=torch.device("cuda", self.ctx.device_id))
            else:
                self.radiance = np.zeros((L, 6, S, S, 4), np.float16)
            self._radiance_geom = geom

    def _radiance_render(self, first_layer, n_layers):
        S, L, Ss = self._radiance_geom
        self.flush()
        bf, bt = self.textures[self.texture_to_blend_from], self.textures[self.texture_to_blend_to]
        sf, st = self.sky_lut.back_texture           # the same blend textures and sky-LUT ring copies as sky_panorama
        if first_layer == 0 and (bf is None or bt is None or sf is None or st is None):
            raise RuntimeError("radiance: no sky yet (call update_sky() first)")
        fd = self.frame_data
        if not self.device_buffers:
            self.ctx.render_radiance(bf, bt, sf, st, fd.LIGHT_DIRECTION, self.blend_amount, self.sun_disk_scale, S, L, Ss, first_layer, n_layers, out=self.radiance)
            return
        stream, done = self._march_stream()
        ptr = lambda t: t.data_ptr() if (first_layer == 0 and t is not None) else 0   # noqa: E731  (layers >= 1 read only the snapshot)
        wh = lambda t: (t.shape[1], t.shape[0]) if t is not None else (1, 1)           # noqa: E731
        self.ctx.render_radiance_device(ptr(bf), ptr(bt), ptr(sf), ptr(st), wh(bf), wh(sf), fd.LIGHT_DIRECTION,
                                        self.blend_amount, self.sun_disk_scale, S, L, Ss, first_layer, n_layers, self.radiance.data_ptr(), stream)
        done()

    def cloud_shadow_map(self, size=512, extent=16384.0, center=(0.0, 0.0), steps=64):
        """What the clouds of the current frame data do to the ground: the sun's transmittance at size x size (or (w, h)) points of the square
        (or (x, z) rectangle) of `extent` metres around `center` in the observer's tangent plane, float16 [h, w] (csky_render_cloud_shadow; the
        definition and the lookup uv = ((x, z) - center) / extent + 0.5: include/cloudsky.h).  A torch CUDA tensor with device_buffers=True.
        Independent of the sky LUTs and of the blend textures; not called by update_sky()."""
        w, h = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
        ext = (float(extent), float(extent)) if np.isscalar(extent) else (float(extent[0]), float(extent[1]))
        pc = self._fill_push_constant()
        if not self.device_buffers:
            return self.ctx.render_cloud_shadow(pc, w, h, center, ext, steps)
        import torch
        out = torch.empty((h, w), dtype=torch.float16, device=torch.device("cuda", self.ctx.device_id))
        stream, done = self._march_stream()
        self.ctx.render_cloud_shadow(pc, w, h, center, ext, steps, out=out, stream=stream)
        done()
        return out

    def aerial_perspective(self, width=32, height=32, depth=32, far_km=32.0, steps_per_slice=2, view=None, cloud_shadows=False, shadow_size=256):
        """What the atmosphere does in front of the scene's geometry under the current sun (the one update_sky() hands the sky LUT): in-scattered
        light and transmittance per view direction and depth slice, float16 [depth, height, width, 4] (csky_render_aerial_perspective; the
        definition and the host's lookup: include/cloudsky.h).  view: None = the panorama over the whole sphere, which depends on
        the sun alone; or (basis, fov_y_degrees) as sky_view takes them, the aspect ratio being width / height.  A torch CUDA tensor with
        device_buffers=True.  Independent of the noise, the sky LUTs and the blend textures; not called by update_sky().
        cloud_shadows=True: light shafts.  The clouds of the current frame data shadow the volume's direct sun
        (csky_render_aerial_perspective_shadowed): a shadow_size x shadow_size (or (w, h)) cloud shadow map is rendered over the rectangle
        aerial_shadow_rect gives for far_km and the sun, and the volume taps it; with device_buffers=True both run back to back on the march
        stream, without a host hop.  A sun at or below the horizon casts no shafts: the plain volume is rendered.  A sun so low that the rectangle
        leaves the shadow map's range (within a quarter of a degree of the horizon at 32 km) raises CloudSkyError, as aerial_shadow_rect does;
        above that limit every texel of the map, and so every half of the volume, is defined (sun lines that pass over the cloud base far out:
        include/cloudsky.h)."""
        sun = self.frame_data.LIGHT_DIRECTION
        if cloud_shadows and float(np.float32(sun[1])) > 0.0:
            return self._aerial_perspective_shadowed(sun, width, height, depth, far_km, steps_per_slice, view, shadow_size)
        if not self.device_buffers:
            return self.ctx.render_aerial_perspective(sun, width, height, depth, far_km, steps_per_slice, view)
        import torch
        out = torch.empty((int(depth), int(height), int(width), 4), dtype=torch.float16, device=torch.device("cuda", self.ctx.device_id))
        stream, done = self._march_stream()
        self.ctx.render_aerial_perspective(sun, width, height, depth, far_km, steps_per_slice, view, out=out, stream=stream)
        done()
        return out

    def _aerial_perspective_shadowed(self, sun, width, height, depth, far_km, steps_per_slice, view, shadow_size):
        mw, mh = (int(shadow_size), int(shadow_size)) if np.isscalar(shadow_size) else (int(shadow_size[0]), int(shadow_size[1]))
        center, extent = _aerial_shadow_rect(sun, far_km)
        pc = self._fill_push_constant()
        if not self.device_buffers:
            shadow = self.ctx.render_cloud_shadow(pc, mw, mh, center, extent)
            return self.ctx.render_aerial_perspective_shadowed(sun, shadow, center, extent, width, height, depth, far_km, steps_per_slice, view)
        import torch
        dev = torch.device("cuda", self.ctx.device_id)
        shadow = torch.empty((mh, mw), dtype=torch.float16, device=dev)
        out = torch.empty((int(depth), int(height), int(width), 4), dtype=torch.float16, device=dev)
        stream, done = self._march_stream()
        self.ctx.render_cloud_shadow(pc, mw, mh, center, extent, out=shadow, stream=stream)          # the volume reads the map on the same stream
        self.ctx.render_aerial_perspective_shadowed(sun, shadow, center, extent, width, height, depth, far_km, steps_per_slice, view, out=out, stream=stream)
        done()                                           # torch's stream is behind both launches: the map's memory may be reused on it from here
        return out

    def cloud_depth(self):
        """Where along each ray of the hemisphere frame the clouds of the current frame data sit: the mean, first and last distance from the
        observer in km and the frame's alpha, float16 [h, w, 4] at the frame's size and the context's step count, so that the samples are the
        frame's (csky_render_cloud_depth; the definition: include/cloudsky.h).  A torch CUDA tensor with device_buffers=True.  Independent of
        the sky LUTs and of the blend textures; not called by update_sky()."""
        W, H = self._texture_size
        pc = self._fill_push_constant()
        if not self.device_buffers:
            return self.ctx.render_cloud_depth(pc, W, H)
        import torch
        out = torch.empty((H, W, 4), dtype=torch.float16, device=torch.device("cuda", self.ctx.device_id))
        stream, done = self._march_stream()
        self.ctx.render_cloud_depth(pc, W, H, out=out, stream=stream)
        done()
        return out

    def aerial_clouds(self, frame=None, steps=16):
        """The current frame (or `frame`, a float16 [h, w, 4] image at the frame's size) with the air in front of its clouds under the current
        sun: the depth frame of the current frame data places every pixel's cloud, and the atmosphere's extinction and in-scattering over that
        distance are applied (csky_render_cloud_depth + csky_apply_cloud_aerial; the definition: include/cloudsky.h).  A new image, alpha
        unchanged; a host binds it in place of the frame.  With device_buffers=True both kernels run back to back on the march
        stream, without a host hop.  A sun at or under the horizon still applies the extinction.  Not called by update_sky().
        `frame` may be a numpy array or a torch tensor on either side: it is moved to where this object keeps its frames (the GPU with
        device_buffers=True, the host without), and the result is of that kind.  With frames_to_update > 1 the current frame is a texture that
        update_sky() refreshes tile by tile, while the depth frame describes the current frame data as a whole: call this once per finished
        pass (`self.frame == self.frames_to_update`), on the texture the pass completed, as INTEGRATION.md tells a C host."""
        self.flush()
        if frame is None:
            frame = self.last_frame
        if frame is None:
            raise RuntimeError("aerial_clouds: no frame yet (call update_sky() first)")
        W, H = self._texture_size
        is_tensor = hasattr(frame, "data_ptr")
        if not is_tensor and not isinstance(frame, np.ndarray):
            raise ValueError("aerial_clouds: frame must be a numpy float16 array or a torch float16 tensor, not %s" % type(frame).__name__)
        if tuple(int(x) for x in frame.shape) != (H, W, 4) or str(frame.dtype).split(".")[-1] != "float16":
            raise ValueError("aerial_clouds: frame must be a float16 [%d, %d, 4] image, the size of the hemisphere frame" % (H, W))
        sun = self.frame_data.LIGHT_DIRECTION
        pc = self._fill_push_constant()
        if not self.device_buffers:
            if is_tensor:
                frame = frame.cpu().numpy()
            return self.ctx.apply_cloud_aerial(sun, frame, self.ctx.render_cloud_depth(pc, W, H), steps)
        import torch
        dev = torch.device("cuda", self.ctx.device_id)
        if not is_tensor:
            frame = torch.from_numpy(np.ascontiguousarray(frame))
        frame = frame.to(dev).contiguous()
        depth = torch.empty((H, W, 4), dtype=torch.float16, device=dev)
        out = torch.empty((H, W, 4), dtype=torch.float16, device=dev)
        stream, done = self._march_stream()
        self.ctx.render_cloud_depth(pc, W, H, out=depth, stream=stream)            # the apply step reads the depth frame on the same stream
        self.ctx.apply_cloud_aerial(sun, frame, depth, steps, out=out, stream=stream)
        done()                                           # torch's stream is behind both launches: the depth frame's memory may be reused on it from here
        return out

    # ---- render thread ------------------------------------------------------------------------------------
    def _march_stream(self):
        """(hip stream handle, done()) for one batch of library calls in device-buffer mode.  The work is enqueued on torch's CURRENT
        stream so that torch work before it (tensor creation / fills) and after it (copies, .cpu(), collectives) is ordered around it
        without a device-wide synchronise.  torch's default stream is the HIP null stream, whose handle is 0 = "use the context's own
        non-blocking stream" to the library, which the null stream does NOT order against: in that case the batch runs
        on a private side stream that waits for the default stream first, and done() makes the default stream wait for it."""
        if not self.device_buffers:
            return None, (lambda: None)
        import torch
        cur = torch.cuda.current_stream()
        if cur.cuda_stream != 0:
            return cur.cuda_stream, (lambda: None)
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(device=torch.device("cuda", self.ctx.device_id))
        side = self._side_stream
        side.wait_stream(cur)
        return side.cuda_stream, (lambda: cur.wait_stream(side))

    def _fill_push_constant(self):  # cloud_sky.gd:251-289, same order incl. padding
        fd = self.frame_data
        pc = [self._texture_size[0], self._texture_size[1], self.update_position[0], self.update_position[1],
              fd._cloud_pos[0], fd._cloud_pos[1], fd._detailed_pos[0], fd._detailed_pos[1],
              fd._weather_pos[0], fd._weather_pos[1], 0.0, 0.0,
              fd.ground_color[0], fd.ground_color[1], fd.ground_color[2], fd.ground_color[3],
              fd.LIGHT_DIRECTION[0], fd.LIGHT_DIRECTION[1], fd.LIGHT_DIRECTION[2], fd.LIGHT_ENERGY,
              fd.LIGHT_COLOR[0], fd.LIGHT_COLOR[1], fd.LIGHT_COLOR[2], fd._time,
              0.0, fd.density, fd.cloud_coverage, fd.time_offset]
        return np.asarray(pc, np.float32)

    def _initialize_compute_code(self):  # cloud_sky.gd:355-408: three RGBA16F textures cleared to (1,0,0,0),(0,1,0,0),(0,0,1,0)
        w, h = self._texture_size
        if self.device_buffers:
            import torch
            dev = torch.device("cuda", self.ctx.device_id)
            self.textures = []
            for i in range(3):
                t = torch.zeros((h, w, 4), dtype=torch.float16, device=dev)
                t[..., i] = 1.0
                self.textures.append(t)
        else:
            self.textures = []
            for i in range(3):
                t = np.zeros((h, w, 4), np.float16)
                t[..., i] = 1.0
                self.textures.append(t)
        self.can_run = True

    def _render_process(self, p_texture_to_update):  # cloud_sky.gd:234-248
        pc = self._fill_push_constant()
        tex = self.textures[p_texture_to_update]
        W, H = self._texture_size
        rw, rh = self.update_region_size
        x0, y0 = self.update_position
        if self.async_host:
            self.flush()                                                    # the previous call's tile -> its texture (rd.texture_update there)
            self._pending = (self.ctx.submit_clouds(pc, rw, rh), p_texture_to_update, (x0, y0, rw, rh))
            self.last_frame = tex
            return tex
        if not self.device_buffers:
            tile = self.ctx.render_clouds(pc, rw, rh)                       # dispatch(num_workgroups, num_workgroups, 1)
            tex[y0:y0 + rh, x0:x0 + rw] = tile
            self.last_frame = tex
            return tex
        import torch
        if self._frames_to_update == 1:
            # full hemisphere per call, sharded over the ranks of one node
            def render_bands(bands, out):
                stream, done = self._march_stream()                             # after `out` was created / cleared on torch's stream
                self.ctx.render_clouds_device(pc, W, bands, out.data_ptr(), W * 8, stream)
                done()                                                          # the gather / interleave that follow run on torch's stream
            frame = _tiling.render_sharded(render_bands, H, W, self.rank, self.world_size, self.dist, tex.device)
            if frame is not None:
                self.textures[p_texture_to_update] = frame.view(torch.float16)
                self.last_frame = self.textures[p_texture_to_update]
            return self.last_frame if self.rank == 0 else None
        region = torch.empty((rh, rw, 4), dtype=torch.float16, device=tex.device)
        stream, done = self._march_stream()
        self.ctx.render_clouds_device(pc, rw, (rh, 0, 1, 1), region.data_ptr(), rw * 8, stream)
        done()
        tex[y0:y0 + rh, x0:x0 + rw] = region
        self.last_frame = tex
        return tex
