"""ctypes binding of libcloudsky.so (include/cloudsky.h).  Fails loudly: a missing library or a missing GPU is
an error, never a silent fallback."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_IO, ERR_STATE = 0, -1, -2, -3, -4, -5
TLUT_REFERENCE, TLUT_BRUNETON = 0, 1   # include/cloudsky.h CSKY_TLUT_*: the transmittance LUT's parametrization
_TLUT_NAMES = {"reference": TLUT_REFERENCE, "bruneton": TLUT_BRUNETON}


def tlut_mapping(mapping):
    """'reference' / 'bruneton' (or CSKY_TLUT_* itself) -> the C ABI's value."""
    if isinstance(mapping, str):
        if mapping not in _TLUT_NAMES:
            raise ValueError("transmittance mapping must be 'reference' or 'bruneton', got %r" % (mapping,))
        return _TLUT_NAMES[mapping]
    return int(mapping)


def transmittance_uv(r_km, mu, mapping=TLUT_BRUNETON, w=256, h=64):
    """csky_transmittance_uv (host only, no GPU): where a reader taps a w x h transmittance LUT for radius r_km and zenith cosine mu.
    Returns (u, v, hits_ground); a ray that hits the ground has transmittance 0 in the Bruneton mapping and is not tapped."""
    uv, hit = (C.c_float * 2)(), C.c_int(0)
    rc = lib().csky_transmittance_uv(tlut_mapping(mapping), int(w), int(h), float(r_km), float(mu), uv, C.byref(hit))
    if rc != OK:
        raise CloudSkyError(rc, (lib().csky_last_error(None) or b"").decode())
    return float(uv[0]), float(uv[1]), bool(hit.value)


def aerial_shadow_rect(sun, far_km=32.0):
    """csky_aerial_shadow_rect (host only, no GPU): the rectangle (center, extent), two (x, z) pairs in metres, that a cloud shadow map must cover
    for an aerial-perspective volume of reach far_km under the sun `sun`.  Raises CloudSkyError (CSKY_ERR_INVALID) when the sun is not above the
    horizon, or so low that the rectangle leaves the range of csky_shadow_params."""
    p = _aerial_params(sun, 0, 0, 0, far_km, 0, 0.0)
    center, extent = (C.c_float * 2)(), (C.c_float * 2)()
    rc = lib().csky_aerial_shadow_rect(C.byref(p), center, extent)
    if rc != OK:
        raise CloudSkyError(rc, (lib().csky_last_error(None) or b"").decode())
    return (float(center[0]), float(center[1])), (float(extent[0]), float(extent[1]))


class CloudSkyError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libcloudsky error %d: %s" % (code, msg))
        self.code = code


class CloudParams(C.Structure):  # clouds.glsl:18-40
    _fields_ = [("f", C.c_float * 28)]


class SkyParams(C.Structure):  # sky-lut.glsl:12-18
    _fields_ = [("f", C.c_float * 8)]


class TransParams(C.Structure):  # transmittance-lut.glsl:12-15
    _fields_ = [("f", C.c_float * 4)]


class Bands(C.Structure):
    _fields_ = [("band_rows", C.c_int), ("first_band", C.c_int), ("band_stride", C.c_int), ("n_bands", C.c_int)]


class CompositeParams(C.Structure):
    _fields_ = [("out_w", C.c_int), ("out_h", C.c_int), ("cloud_w", C.c_int), ("cloud_h", C.c_int), ("sky_w", C.c_int), ("sky_h", C.c_int),
                ("blend_amount", C.c_float), ("sun_disk_scale", C.c_float), ("light_direction", C.c_float * 3)]


class RadianceParams(C.Structure):
    """csky_radiance_params (include/cloudsky.h): face size S, layer count L, source-cube size Ss (0 = min(S, 64))."""
    _fields_ = [("face_size", C.c_int), ("layers", C.c_int), ("source_size", C.c_int)]


class ShadowParams(C.Structure):
    """csky_shadow_params (include/cloudsky.h): the cloud shadow map's size, rectangle of the tangent plane and step count."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("center", C.c_float * 2), ("extent", C.c_float * 2), ("steps", C.c_int)]


class AerialParams(C.Structure):
    """csky_aerial_params (include/cloudsky.h): the aerial-perspective volume's sizes, reach, screen aspect and sun."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("depth", C.c_int), ("steps_per_slice", C.c_int), ("far_km", C.c_float), ("aspect", C.c_float),
                ("sun_direction", C.c_float * 3)]


class DepthParams(C.Structure):
    """csky_depth_params (include/cloudsky.h): the cloud depth frame's size and step count."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("steps", C.c_int)]


class CloudAerialParams(C.Structure):
    """csky_cloud_aerial_params (include/cloudsky.h): the size of the cloud frame and its depth frame, the step count and the sun."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("steps", C.c_int), ("sun_direction", C.c_float * 3)]


class View(C.Structure):
    """csky_view (include/cloudsky.h): the camera's basis, column-major, and its vertical field of view."""
    _fields_ = [("basis", C.c_float * 9), ("fov_y_degrees", C.c_float)]


class Observer(C.Structure):
    """csky_observer (include/cloudsky.h): the observer's position relative to the reference's camera, in metres, and the cap on a ray's length."""
    _fields_ = [("position", C.c_float * 3), ("max_distance", C.c_float)]


class SceneDepth(C.Structure):
    """csky_scene_depth (include/cloudsky.h): a float32 depth buffer of the host's scene, its row pitch in bytes and the kind of its texels."""
    _fields_ = [("texels", C.c_void_p), ("pitch_bytes", C.c_size_t), ("kind", C.c_int)]


DEPTH_KINDS = {"distance": 0, "view_z": 1}           # CSKY_DEPTH_DISTANCE, CSKY_DEPTH_VIEW_Z


class CloudStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("primary_samples", C.c_uint64), ("incloud_samples", C.c_uint64)]


class ShapeNoiseParams(C.Structure):
    """csky_shape_noise_params (include/cloudsky.h): the knobs of the stand-in shape-noise generator."""
    _fields_ = [("perlin_freq", C.c_int32), ("perlin_octaves", C.c_int32), ("worley_freq", C.c_int32), ("perlin_gain", C.c_float), ("dilate", C.c_float),
                ("centre", C.c_float), ("contrast", C.c_float), ("offset", C.c_float)]


class WeatherParams(C.Structure):
    """csky_weather_params (include/cloudsky.h): the knobs of the weather-map generator."""
    _fields_ = [("coverage_freq", C.c_int32), ("coverage_octaves", C.c_int32), ("type_freq", C.c_int32), ("type_octaves", C.c_int32), ("phase", C.c_float),
                ("coverage_gain", C.c_float), ("dilate", C.c_float), ("coverage_centre", C.c_float), ("coverage_contrast", C.c_float),
                ("coverage_offset", C.c_float), ("coverage_floor", C.c_float), ("type_mean", C.c_float), ("type_spread", C.c_float)]


MULTI_STATS_MAX = 16


class MultiStats(C.Structure):
    """csky_multi_stats (include/cloudsky_internal.h)."""
    _fields_ = [("n_devices", C.c_int32), ("staged", C.c_int32), ("all_peer", C.c_int32), ("groups", C.c_int32), ("frames_in_flight", C.c_int32), ("timing", C.c_int32),
                ("device_id", C.c_int32 * MULTI_STATS_MAX), ("peer_access", C.c_int32 * MULTI_STATS_MAX), ("march_ms", C.c_float * MULTI_STATS_MAX),
                ("copy_ms", C.c_float * MULTI_STATS_MAX)]


def shape_noise_params(**knobs):
    """The generator's defaults with the given fields replaced."""
    p = ShapeNoiseParams()
    lib().csky_shape_noise_default_params(C.byref(p))
    for k, v in knobs.items():
        if k not in dict(ShapeNoiseParams._fields_):
            raise TypeError("unknown shape-noise knob %r" % k)
        setattr(p, k, v)
    return p


def weather_params(**knobs):
    """The weather generator's defaults with the given fields replaced."""
    p = WeatherParams()
    lib().csky_weather_default_params(C.byref(p))
    for k, v in knobs.items():
        if k not in dict(WeatherParams._fields_):
            raise TypeError("unknown weather knob %r" % k)
        setattr(p, k, v)
    return p


WEATHER_SHAPE = (512, 512, 3)


def _weather_arg(name, weather, device_id):
    """The weather map a rebind takes: a numpy uint8 [512, 512, 3] array (-> its pointer, False) or a contiguous uint8 tensor of that shape on the
    context's GPU (-> its pointer, True).  Anything else is refused here, before any library call."""
    if isinstance(weather, np.ndarray):
        if weather.shape != WEATHER_SHAPE or weather.dtype != np.uint8 or not weather.flags.c_contiguous:
            raise ValueError("%s: a host weather map is a contiguous uint8 [512, 512, 3] array" % name)
        return _ptr(weather), False
    if hasattr(weather, "data_ptr"):
        import torch
        dev = getattr(weather, "device", None)
        index = dev.index if dev is not None and dev.index is not None else (torch.cuda.current_device() if dev is not None and dev.type == "cuda" else None)
        if tuple(weather.shape) != WEATHER_SHAPE or weather.dtype != torch.uint8 or not weather.is_contiguous() or dev is None or dev.type != "cuda" or index != device_id:
            raise ValueError("%s: a device weather map is a contiguous uint8 [512, 512, 3] tensor on cuda:%d" % (name, device_id))
        return C.c_void_p(int(weather.data_ptr())), True
    raise ValueError("%s: weather must be a numpy uint8 [512, 512, 3] array or a torch tensor of that shape on the GPU" % name)


# every symbol include/cloudsky.h and include/cloudsky_internal.h declare: (name, restype, argtypes); INTERNAL names the second header's (the lab bench)
SYMBOLS = [
    ("csky_abi_version", C.c_int, []),
    ("csky_device_count", C.c_int, []),
    ("csky_create", C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    ("csky_destroy", None, [C.c_void_p]),
    ("csky_last_error", C.c_char_p, [C.c_void_p]),
    ("csky_set_noise", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csky_set_noise_mips", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csky_noise_inexact_coeffs", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("csky_encode_bc7", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    ("csky_encode_bc7_quality", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    ("csky_set_march", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("csky_set_early_out", C.c_int, [C.c_void_p, C.c_float]),
    ("csky_set_transmittance_mapping", C.c_int, [C.c_void_p, C.c_int]),
    ("csky_get_transmittance_mapping", C.c_int, [C.c_void_p]),
    ("csky_multi_set_transmittance_mapping", C.c_int, [C.c_void_p, C.c_int]),
    ("csky_transmittance_uv", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    ("csky_render_transmittance", C.c_int, [C.c_void_p, C.POINTER(TransParams), C.c_void_p]),
    ("csky_render_sky_lut", C.c_int, [C.c_void_p, C.POINTER(SkyParams), C.c_void_p]),
    ("csky_render_clouds", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    ("csky_render_sky_lut_device", C.c_int, [C.c_void_p, C.POINTER(SkyParams), C.c_void_p]),
    ("csky_render_clouds_device", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.c_int, C.POINTER(Bands), C.c_void_p, C.c_size_t, C.c_void_p]),
    ("csky_copy_sky_lut_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csky_render_sky_lut_rows_device", C.c_int, [C.c_void_p, C.POINTER(SkyParams), C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("csky_interleave_bands_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    ("csky_sync", C.c_int, [C.c_void_p]),
    ("csky_set_host_ring", C.c_int, [C.c_void_p, C.c_int]),
    ("csky_submit_clouds", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    ("csky_collect", C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    ("csky_poll", C.c_int, [C.c_void_p, C.c_int64]),
    ("csky_external_frame_import_fd", C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    ("csky_external_frame_import_semaphore_fd", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("csky_external_frame_signal", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csky_external_frame_fence", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csky_external_frame_ready", C.c_int, [C.c_void_p, C.c_void_p]),
    ("csky_external_frame_wait", C.c_int, [C.c_void_p, C.c_void_p]),
    ("csky_external_frame_release", None, [C.c_void_p]),
    ("csky_read_transmittance", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("csky_read_sky_lut", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("csky_composite_sky", C.c_int, [C.c_void_p, C.POINTER(CompositeParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csky_composite_view", C.c_int, [C.c_void_p, C.POINTER(CompositeParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csky_render_radiance_device", C.c_int, [C.c_void_p, C.POINTER(CompositeParams), C.POINTER(RadianceParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("csky_render_radiance", C.c_int, [C.c_void_p, C.POINTER(CompositeParams), C.POINTER(RadianceParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_int, C.c_void_p]),
    ("csky_prefilter_cube", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    ("csky_render_cloud_shadow", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.POINTER(ShadowParams), C.c_void_p]),
    ("csky_render_cloud_shadow_device", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.POINTER(ShadowParams), C.c_void_p, C.c_size_t, C.c_void_p]),
    ("csky_render_aerial_perspective", C.c_int, [C.c_void_p, C.POINTER(AerialParams), C.POINTER(View), C.c_void_p]),
    ("csky_render_aerial_perspective_device", C.c_int, [C.c_void_p, C.POINTER(AerialParams), C.POINTER(View), C.c_void_p, C.c_void_p]),
    ("csky_render_aerial_perspective_shadowed", C.c_int, [C.c_void_p, C.POINTER(AerialParams), C.POINTER(View), C.POINTER(ShadowParams), C.c_void_p, C.c_void_p]),
    ("csky_render_aerial_perspective_shadowed_device", C.c_int, [C.c_void_p, C.POINTER(AerialParams), C.POINTER(View), C.POINTER(ShadowParams), C.c_void_p, C.c_size_t,
                                                                 C.c_void_p, C.c_void_p]),
    ("csky_aerial_shadow_rect", C.c_int, [C.POINTER(AerialParams), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("csky_render_cloud_depth", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.POINTER(DepthParams), C.c_void_p]),
    ("csky_render_cloud_depth_device", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.POINTER(DepthParams), C.c_void_p, C.c_size_t, C.c_void_p]),
    ("csky_apply_cloud_aerial", C.c_int, [C.c_void_p, C.POINTER(CloudAerialParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csky_apply_cloud_aerial_device", C.c_int, [C.c_void_p, C.POINTER(CloudAerialParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csky_render_clouds_dirs", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("csky_render_clouds_dirs_device", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("csky_render_clouds_view", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.POINTER(View), C.c_int, C.c_int, C.c_void_p]),
    ("csky_render_clouds_view_device", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.POINTER(View), C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("csky_render_clouds_view_update", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.POINTER(View), C.POINTER(View), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("csky_render_clouds_view_update_device", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.POINTER(View), C.POINTER(View), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                        C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("csky_render_clouds_view_from", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.POINTER(View), C.POINTER(Observer), C.c_int, C.c_int, C.c_void_p]),
    ("csky_render_clouds_view_from_device", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.POINTER(View), C.POINTER(Observer), C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                                      C.c_void_p]),
    ("csky_render_clouds_dirs_from", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.c_int, C.c_int, C.c_void_p, C.POINTER(Observer), C.c_void_p]),
    ("csky_render_clouds_dirs_from_device", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.c_int, C.c_int, C.c_void_p, C.POINTER(Observer), C.c_void_p, C.c_size_t,
                                                      C.c_void_p]),
    ("csky_render_clouds_view_from_depth", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.POINTER(View), C.POINTER(Observer), C.c_int, C.c_int, C.POINTER(SceneDepth),
                                                     C.c_void_p]),
    ("csky_render_clouds_view_from_depth_device", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.POINTER(View), C.POINTER(Observer), C.c_int, C.c_int, C.POINTER(SceneDepth),
                                                            C.c_void_p, C.c_size_t, C.c_void_p]),
    ("csky_render_clouds_dirs_from_depth", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.c_int, C.c_int, C.c_void_p, C.POINTER(Observer), C.POINTER(SceneDepth),
                                                     C.c_void_p]),
    ("csky_render_clouds_dirs_from_depth_device", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.c_int, C.c_int, C.c_void_p, C.POINTER(Observer), C.POINTER(SceneDepth),
                                                            C.c_void_p, C.c_size_t, C.c_void_p]),
    ("csky_render_cloud_depth_dirs", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("csky_render_cloud_depth_dirs_device", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("csky_render_cloud_depth_view", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.POINTER(View), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    ("csky_render_cloud_depth_view_device", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.POINTER(View), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("csky_apply_cloud_aerial_dirs", C.c_int, [C.c_void_p, C.POINTER(CloudAerialParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csky_apply_cloud_aerial_dirs_device", C.c_int, [C.c_void_p, C.POINTER(CloudAerialParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csky_apply_cloud_aerial_view", C.c_int, [C.c_void_p, C.POINTER(CloudAerialParams), C.POINTER(View), C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csky_apply_cloud_aerial_view_device", C.c_int, [C.c_void_p, C.POINTER(CloudAerialParams), C.POINTER(View), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csky_composite_view_frames", C.c_int, [C.c_void_p, C.POINTER(CompositeParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csky_time_clouds", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.c_int, C.POINTER(Bands), C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(CloudStats)]),
    ("csky_get_cloud_stats", C.c_int, [C.c_void_p, C.POINTER(CloudStats)]),
    ("csky_set_kernel_timing", C.c_int, [C.c_void_p, C.c_int]),
    ("csky_get_kernel_ms", C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    ("csky_set_frames_in_flight", C.c_int, [C.c_void_p, C.c_int]),
    ("csky_set_variant", C.c_int, [C.c_void_p, C.c_int]),
    ("csky_variant_count", C.c_int, []),
    ("csky_set_schedule", C.c_int, [C.c_void_p, C.c_int]),
    ("csky_set_height_window", C.c_int, [C.c_void_p, C.c_int]),
    ("csky_set_segments", C.c_int, [C.c_void_p, C.c_int]),
    ("csky_set_exact_cells", C.c_int, [C.c_void_p, C.c_int]),
    ("csky_last_warning", C.c_char_p, [C.c_void_p]),
    ("csky_variant_name", C.c_char_p, [C.c_int]),
    ("csky_multi_create", C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int]),
    ("csky_multi_destroy", None, [C.c_void_p]),
    ("csky_multi_device_count", C.c_int, [C.c_void_p]),
    ("csky_multi_ctx", C.c_void_p, [C.c_void_p, C.c_int]),
    ("csky_multi_last_error", C.c_char_p, [C.c_void_p]),
    ("csky_multi_last_warning", C.c_char_p, [C.c_void_p]),
    ("csky_multi_set_timing", C.c_int, [C.c_void_p, C.c_int]),
    ("csky_multi_get_stats", C.c_int, [C.c_void_p, C.c_void_p]),
    ("csky_multi_set_noise", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csky_multi_set_noise_mips", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csky_multi_set_frames_in_flight", C.c_int, [C.c_void_p, C.c_int]),
    ("csky_multi_set_groups", C.c_int, [C.c_void_p, C.c_int]),
    ("csky_multi_set_staged", C.c_int, [C.c_void_p, C.c_int]),
    ("csky_multi_set_march", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("csky_multi_render_sky_lut", C.c_int, [C.c_void_p, C.POINTER(SkyParams)]),
    ("csky_multi_render_clouds_device", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("csky_multi_render_clouds", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    ("csky_multi_sync", C.c_int, [C.c_void_p]),
    ("csky_multi_set_host_ring", C.c_int, [C.c_void_p, C.c_int]),
    ("csky_multi_submit_clouds", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    ("csky_multi_collect", C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    ("csky_load_bmp_rgb8", C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_size_t]),
    ("csky_load_tga_rgba8", C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_size_t]),
    ("csky_strip_to_volume", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    ("csky_generate_shape_noise", C.c_int, [C.c_uint32, C.c_int, C.c_void_p]),
    ("csky_generate_shape_noise_device", C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]),
    ("csky_shape_noise_default_params", None, [C.c_void_p]),
    ("csky_check_shape_noise_params", C.c_int, [C.c_void_p, C.c_int]),
    ("csky_generate_shape_noise_tuned", C.c_int, [C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]),
    ("csky_generate_shape_noise_tuned_device", C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]),
    ("csky_set_weather", C.c_int, [C.c_void_p, C.c_void_p]),
    ("csky_set_weather_device", C.c_int, [C.c_void_p, C.c_void_p]),
    ("csky_set_weather_generated", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    ("csky_weather_default_params", None, [C.c_void_p]),
    ("csky_check_weather_params", C.c_int, [C.c_void_p]),
    ("csky_generate_weather", C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p]),
    ("csky_generate_weather_device", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("csky_generate_detail_noise", C.c_int, [C.c_uint32, C.c_int, C.c_void_p]),
    ("csky_generate_detail_noise_device", C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]),
    ("csky_build_mips_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    ("csky_read_baked_texture", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("csky_test_sqrt_shell", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    ("csky_test_primitive", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    ("csky_test_static_order", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]),
    ("csky_test_lpt_order", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csky_census_clouds", C.c_int, [C.c_void_p, C.POINTER(CloudParams), C.c_int, C.POINTER(Bands), C.c_void_p, C.c_int]),
    ("csky_mip_offset", C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    ("csky_build_mips", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    ("csky_decode_bc7", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    ("csky_load_ctex", C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_size_t]),
    ("csky_load_ctex3d", C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_size_t]),
    ("csky_assets_last_error", C.c_char_p, []),
]

# include/cloudsky_lut_hooks.h (which cloudsky_internal.h includes): the switch and the launch counter of the sky LUT's reuse
LUT_HOOK_SYMBOLS = [
    ("csky_set_sky_lut_reuse", C.c_int, [C.c_void_p, C.c_int]),
    ("csky_sky_lut_launches", C.c_int64, [C.c_void_p]),
]

# include/cloudsky_shadow_hooks.h (likewise): the A/B switch of the cloud shadow map's exact end
SHADOW_HOOK_SYMBOLS = [
    ("csky_set_shadow_exact_end", C.c_int, [C.c_void_p, C.c_int]),
]


DEFAULT_VARIANT = 3   # include/cloudsky.h CSKY_DEFAULT_VARIANT ("compact"); set_variant(-1) selects it
ABI_VERSION = 9       # include/cloudsky.h CSKY_ABI_VERSION


def library_path():
    # CSKY_LIBRARY: explicit path of an alternative build (A/B timing of kernel experiments); default = the in-tree build
    return os.environ.get("CSKY_LIBRARY") or os.path.join(_HERE, "libcloudsky.so")


def lib():
    """Load libcloudsky.so (built in-tree by __graft_entry__.build() / csrc/Makefile)."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise CloudSkyError(ERR_IO, "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                        "(hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
        try:
            # torch bundles its own libamdhip64; it must be the FIRST HIP runtime in the process so that libcloudsky's
            # DT_NEEDED resolves to the same (already loaded) runtime and device pointers / streams can be shared.
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(path)
        for name, res, args in SYMBOLS + LUT_HOOK_SYMBOLS + SHADOW_HOOK_SYMBOLS:
            fn = getattr(L, name)  # AttributeError = ABI mismatch, surfaced loudly
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# csky_test_primitive (include/cloudsky_internal.h, csrc/primitives_core.h): name -> (op, inputs, outputs), an array = (dtype, words per element)
_F, _U, _I = np.float32, np.uint32, np.int32
PRIMITIVES = {
    "sqrt_exact": (0, [(_F, 1)], [(_F, 1)]), "sqrtf": (1, [(_F, 1)], [(_F, 1)]), "div": (2, [(_F, 1), (_F, 1)], [(_F, 1)]),
    "split_coord": (3, [(_F, 1)], [(_I, 1), (_F, 1)]), "lerp_h": (4, [(_U, 1), (_F, 1)], [(_F, 1)]), "lerp_h2": (5, [(_U, 1), (_F, 1)], [(_F, 1)]),
    "f2h_normal": (6, [(_F, 1)], [(_U, 1)]), "fast_rcp": (7, [(_F, 1)], [(_F, 1)]), "fast_exp2": (8, [(_F, 1)], [(_F, 1)]),
    "fast_log2": (9, [(_F, 1)], [(_F, 1)]), "fast_exp": (10, [(_F, 1)], [(_F, 1)]), "fast_pow": (11, [(_F, 1), (_F, 1)], [(_F, 1)]),
    "rad_rcp": (12, [(_F, 1)], [(_F, 1)]), "ray": (13, [(_F, 3), (_F, 1)], [(_F, 10)]), "pixel_dir": (14, [(_I, 2), (_F, 2)], [(_F, 3)]),
}


def run_primitive(call, op, arrays):
    """One primitive over arrays: `call(op code, in0, in1, in2, out0, out1, n)` is csky_test_primitive bound to a context, or the host build's
    export of the same table (tests/hostsim).  Inputs are [n] or [n, words] arrays of the op's types; -> the output array, or a tuple of two."""
    code, ins, outs = PRIMITIVES[op]
    if len(arrays) != len(ins):
        raise ValueError("%s takes %d arrays" % (op, len(ins)))
    a = [np.ascontiguousarray(x, dt).reshape(-1, w) for x, (dt, w) in zip(arrays, ins)]
    n = a[0].shape[0]
    if any(x.shape[0] != n for x in a):
        raise ValueError("%s: arrays of different lengths" % op)
    o = [np.zeros((n, w) if w > 1 else (n,), dt) for dt, w in outs]
    ptr = [_ptr(x) for x in a] + [None] * (3 - len(a)) + [_ptr(x) for x in o] + [None] * (2 - len(o))
    call(code, *ptr, n)
    return o[0] if len(o) == 1 else tuple(o)


def cloud_params(values):
    p = CloudParams()
    v = np.asarray(values, np.float32).reshape(-1)
    if v.size != 28:
        raise ValueError("cloud push-constant block is 28 floats (clouds.glsl:18-40), got %d" % v.size)
    for i in range(28):
        p.f[i] = float(v[i])
    return p


# ---- the structs of include/cloudsky.h from the methods' arguments: each is built here and nowhere else
def _sun3(v):
    return (C.c_float * 3)(*[float(x) for x in v])   # used as given


def _frame_size(p, tile_w, tile_h):
    """(w, h) of a cloud frame: the push constants' texture_size where the caller names none."""
    return int(p.f[0]) if tile_w is None else int(tile_w), int(p.f[1]) if tile_h is None else int(tile_h)


def _sky_params(sun_dir, w, h):
    p = SkyParams()
    p.f[0], p.f[1] = float(w), float(h)
    p.f[4], p.f[5], p.f[6] = [float(x) for x in sun_dir]
    return p


def _view(basis, fov_y_degrees):
    return View((C.c_float * 9)(*[float(x) for x in np.asarray(basis, np.float32).T.reshape(-1)]), float(fov_y_degrees))   # column-major basis


def _observer(name, position, max_distance):
    """csky_observer from a position of three numbers and a cap; what the library would refuse for its shape or sign is refused here."""
    pos = [float(x) for x in np.asarray(position, np.float64).reshape(-1)]
    if len(pos) != 3 or not all(np.isfinite(pos)):
        raise ValueError("%s: position must be three finite numbers (metres from the reference's camera)" % name)
    if not float(max_distance) > 0.0:
        raise ValueError("%s: max_distance must be > 0 (inf: no cap)" % name)
    return Observer((C.c_float * 3)(*pos), float(max_distance))


def _scene_depth(name, depth, depth_kind, w, h, is_view):
    """(csky_scene_depth, whether it lies on the device) from a float32 [h, w] depth buffer: a numpy array (the host forms) or a torch tensor (the
    device forms), its texels contiguous and its row stride the pitch.  Nothing is converted or copied: the struct points into `depth`."""
    if depth_kind not in DEPTH_KINDS:
        raise ValueError("%s: depth_kind must be one of %s" % (name, sorted(DEPTH_KINDS)))
    if depth_kind == "view_z" and not is_view:
        raise ValueError("%s: a view_z depth needs a camera: the dirs form takes distances along its rays" % name)
    device = hasattr(depth, "data_ptr")
    shape = (int(h), int(w))
    if device:
        import torch
        ok = depth.dtype == torch.float32 and tuple(depth.shape) == shape
        stride, ptr = (tuple(depth.stride()), int(depth.data_ptr())) if ok else ((0, 0), 0)
    else:
        ok = isinstance(depth, np.ndarray) and depth.dtype == np.float32 and depth.shape == shape
        stride, ptr = (tuple(s // 4 if s % 4 == 0 else 0 for s in depth.strides), depth.ctypes.data) if ok else ((0, 0), 0)
    ok = ok and (shape[1] == 1 or stride[1] == 1) and (shape[0] == 1 or stride[0] >= shape[1])
    if not ok:
        raise ValueError("%s: depth must be a float32 %s array (or torch tensor on the GPU) whose texels are contiguous, its row stride the pitch" % (name, shape))
    pitch = stride[0] * 4 if shape[0] > 1 else shape[1] * 4
    return SceneDepth(C.c_void_p(ptr), pitch, DEPTH_KINDS[depth_kind]), device


def _composite_params(out_w, out_h, cloud_wh, sky_wh, light_dir, blend_amount, sun_disk_scale):
    return CompositeParams(int(out_w), int(out_h), int(cloud_wh[0]), int(cloud_wh[1]), int(sky_wh[0]), int(sky_wh[1]), float(blend_amount), float(sun_disk_scale),
                           _sun3(light_dir[k] for k in range(3)))   # the first three of a longer vector, as these methods always took them


def _shadow_params(w, h, center, extent, steps):
    return ShadowParams(int(w), int(h), (C.c_float * 2)(float(center[0]), float(center[1])), (C.c_float * 2)(float(extent[0]), float(extent[1])), int(steps))


def _aerial_params(sun, width, height, depth, far_km, steps_per_slice, aspect):
    return AerialParams(int(width), int(height), int(depth), int(steps_per_slice), float(far_km), float(aspect), _sun3(sun))


def _aerial_args(sun, width, height, depth, far_km, steps_per_slice, view, aspect):
    """(the volume's shape, its csky_aerial_params, its csky_view by reference or None for the panorama) of the two aerial-perspective methods."""
    p = _aerial_params(sun, width, height, depth, far_km, steps_per_slice, aspect)
    return (p.depth, p.height, p.width, 4), p, None if view is None else C.byref(_view(view[0], view[1]))


# ---- image arguments.  Every refusal is a ValueError that names the method, raised before any library call.
def _host_frames(cloud_from, cloud_to, sky_from, sky_to):
    """The compositor's four float16 [h, w, 4] host inputs as the library reads them, and (w, h) of the cloud frames and of the sky LUTs."""
    a = [np.ascontiguousarray(x).view(np.uint16) for x in (cloud_from, cloud_to, sky_from, sky_to)]
    return a, (a[0].shape[1], a[0].shape[0]), (a[2].shape[1], a[2].shape[0])


def _host_image(name, shape, out):
    """The host image a call writes: `out` if it can be written in place, a new one for None."""
    if out is None:
        return np.zeros(shape, np.float16)
    if out.shape != shape or out.dtype != np.float16 or not out.flags.c_contiguous:
        raise ValueError("%s: out must be a contiguous float16 %s array" % (name, shape))
    return out


def _device_image(name, what, shape, t, pitched=False):
    """The row pitch in bytes of the device image `t`: a torch tensor of `shape` and 2-byte elements whose rows t[j], of whatever rank, are each
    contiguous (a dimension of one element has no stride to test).  The pitch is stride(0)'s, and a row's own size for a single row, whatever its
    stride(0) says; unless `pitched`, the call has no pitch argument and the rows must follow each other: a contiguous tensor."""
    ok = hasattr(t, "data_ptr") and tuple(t.shape) == tuple(shape) and t.element_size() == 2
    if ok:
        row = 1
        for n, s in zip(reversed(shape[1:]), reversed(t.stride()[1:])):
            ok, row = ok and (n == 1 or s == row), row * n
        pitch = t.stride(0) * 2 if shape[0] > 1 else row * 2
        ok = ok and (pitched or pitch == row * 2)
    if not ok:
        raise ValueError("%s: %s must be a %s tensor of 2-byte elements, %s" % (name, what, tuple(shape), "its rows contiguous" if pitched else "contiguous"))
    return pitch


def _dirs_size(name, dirs):
    if len(dirs.shape) != 3 or int(dirs.shape[2]) != 3:
        raise ValueError("%s: dirs must be a [h, w, 3] float32 array (or torch tensor on the GPU)" % name)
    return int(dirs.shape[1]), int(dirs.shape[0])


def _dirs_arg(name, dirs, device):
    """The pointer argument for a direction image: a device call takes a contiguous float32 tensor as it is, a host call an array, converted if need be."""
    if device:
        import torch
        if not hasattr(dirs, "data_ptr") or dirs.dtype != torch.float32 or not dirs.is_contiguous():
            raise ValueError("%s: with a device frame, dirs must be a contiguous float32 tensor" % name)
        return C.c_void_p(int(dirs.data_ptr()))
    if hasattr(dirs, "data_ptr"):
        raise ValueError("%s: with host frames, dirs must be a numpy array" % name)
    return _ptr(np.ascontiguousarray(dirs, np.float32))   # (the pointer object keeps the array alive)


class Context:
    """One csky_ctx = one GPU.  Thin, explicit wrapper; raises CloudSkyError on any non-zero return."""

    def __init__(self, device_id=0, _borrowed=None):
        self._L = lib()
        self._owned = _borrowed is None
        if _borrowed is not None:                 # a context owned by a MultiContext (csky_multi_ctx): never destroyed from here
            self._h = C.c_void_p(_borrowed)
            self.device_id = int(device_id)
            return
        h = C.c_void_p()
        rc = self._L.csky_create(C.byref(h), int(device_id))
        if rc != OK:
            raise CloudSkyError(rc, (self._L.csky_last_error(None) or b"").decode())
        self._h = h
        self.device_id = int(device_id)

    def _chk(self, rc):
        if rc != OK:
            raise CloudSkyError(rc, (self._L.csky_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            if self._owned:
                self._L.csky_destroy(self._h)
            self._h = None

    __del__ = close

    # ---- inputs
    def set_noise(self, large_rgba8, small_rgb8, weather_rgb8):
        a = np.ascontiguousarray(large_rgba8, np.uint8)
        b = np.ascontiguousarray(small_rgb8, np.uint8)
        c = np.ascontiguousarray(weather_rgb8, np.uint8)
        if a.size != 128 ** 3 * 4 or b.size != 32 ** 3 * 3 or c.size != 512 * 512 * 3:
            raise ValueError("set_noise: expected 128^3 RGBA8, 32^3 RGB8, 512^2 RGB8")
        self._chk(self._L.csky_set_noise(self._h, _ptr(a), _ptr(b), _ptr(c)))   # (textures that do not fit the fp16 cells are marched on exact fp32 cells: last_warning() says so)

    def set_noise_mips(self, large_chain_rgba8, small_chain_rgb8, weather_rgb8):
        """csky_set_noise_mips: full mip chains supplied by the caller (all levels back to back), e.g. the importer's own from
        assets.load_ctex3d; no box filter is applied by the library."""
        a = np.ascontiguousarray(large_chain_rgba8, np.uint8)
        b = np.ascontiguousarray(small_chain_rgb8, np.uint8)
        c = np.ascontiguousarray(weather_rgb8, np.uint8)
        if a.size != self._L.csky_mip_offset(128, 8, 4) or b.size != self._L.csky_mip_offset(32, 6, 3) or c.size != 512 * 512 * 3:
            raise ValueError("set_noise_mips: expected the 8-level 128^3 RGBA8 chain, the 6-level 32^3 RGB8 chain, 512^2 RGB8")
        self._chk(self._L.csky_set_noise_mips(self._h, _ptr(a), _ptr(b), _ptr(c)))

    def set_weather(self, weather):
        """The weather map alone, in a context that set_noise has bound: a numpy uint8 [512, 512, 3] array (csky_set_weather) or a contiguous uint8
        tensor of that shape on this context's GPU (csky_set_weather_device, only read).  Afterwards the context is as if set_noise had been given
        this map; the shape and detail volumes, the LUTs and the cell format are untouched."""
        ptr, device = _weather_arg("set_weather", weather, self.device_id)
        self._chk((self._L.csky_set_weather_device if device else self._L.csky_set_weather)(self._h, ptr))

    def set_weather_generated(self, seed=1, **knobs):
        """csky_set_weather_generated: the map of generate_weather(seed, **knobs) made on the GPU in the context's own buffer and bound (knobs: WeatherParams fields)."""
        p = weather_params(**knobs)
        self._chk(self._L.csky_set_weather_generated(self._h, int(seed), C.byref(p)))

    def generate_weather(self, seed=1, device=True, **knobs):
        """A generated weather map, uint8 [512, 512, 3]: the HIP kernel (device=True) or the host generator; byte-identical (knobs: WeatherParams fields)."""
        p = weather_params(**knobs)
        out = np.zeros(WEATHER_SHAPE, np.uint8)
        if device:
            self._chk(self._L.csky_generate_weather_device(self._h, int(seed), C.byref(p), _ptr(out)))
        else:
            rc = self._L.csky_generate_weather(int(seed), C.byref(p), _ptr(out))
            if rc != OK:
                raise CloudSkyError(rc, (self._L.csky_assets_last_error() or b"").decode())
        return out

    def encode_bc7(self, images, quality=0):
        """csky_encode_bc7[_quality]: [n, h, w, 4] (or [h, w, 4]) uint8 -> [n, ceil(h/4), ceil(w/4), 16] uint8 BC7 blocks, encoded on the GPU
        (quality 1: more partitions + end-point coordinate descent, the sensitivity study's second encoder)."""
        a = np.ascontiguousarray(images, np.uint8)
        if a.ndim == 3:
            a = a[None]
        if a.ndim != 4 or a.shape[3] != 4:
            raise ValueError("encode_bc7: expected [n, h, w, 4] uint8")
        n, h, w = a.shape[:3]
        out = np.zeros((n, (h + 3) // 4, (w + 3) // 4, 16), np.uint8)
        self._chk(self._L.csky_encode_bc7_quality(self._h, _ptr(a), w, h, n, int(quality), _ptr(out)))
        return out

    def noise_inexact_coeffs(self):
        """Finite-difference coefficients of the bound textures that fp16 could not hold exactly (0 for natural noise)."""
        n = C.c_uint64()
        self._chk(self._L.csky_noise_inexact_coeffs(self._h, C.byref(n)))
        return n.value

    def set_march(self, primary_steps=128, light_steps=6):
        self._chk(self._L.csky_set_march(self._h, primary_steps, light_steps))

    def set_transmittance_mapping(self, mapping):
        """'reference' (default) or 'bruneton' (cloudsky.h CSKY_TLUT_*).  A change drops the transmittance LUT, the sky LUT and the radiance
        snapshot: render a sky LUT again before the next frame."""
        self._chk(self._L.csky_set_transmittance_mapping(self._h, tlut_mapping(mapping)))

    def transmittance_mapping(self):
        return self._L.csky_get_transmittance_mapping(self._h)

    def set_sky_lut_reuse(self, enabled=True):
        """True (default): a sky-LUT call for what the context already holds launches nothing (the rows form: one device copy).  False: a launch per
        call, the A/B switch.  The results are identical."""
        self._chk(self._L.csky_set_sky_lut_reuse(self._h, int(bool(enabled))))

    def sky_lut_launches(self):
        """Sky-LUT kernels this context has launched, whole and rows form together."""
        n = self._L.csky_sky_lut_launches(self._h)
        if n < 0:
            self._chk(int(n))
        return int(n)

    def set_early_out(self, eps):
        self._chk(self._L.csky_set_early_out(self._h, float(eps)))

    def set_schedule(self, mode):
        self._chk(self._L.csky_set_schedule(self._h, int(mode)))

    def set_height_window(self, enabled):
        self._chk(self._L.csky_set_height_window(self._h, int(bool(enabled))))

    def set_segments(self, n):
        self._chk(self._L.csky_set_segments(self._h, int(n)))

    def set_variant(self, v):
        self._chk(self._L.csky_set_variant(self._h, int(v)))

    def set_exact_cells(self, mode):
        """1: build and march the exact fp32-coefficient cells at the next set_noise whatever the textures need; 0: only when a coefficient does not fit fp16."""
        self._chk(self._L.csky_set_exact_cells(self._h, int(mode)))

    def last_warning(self):
        return (self._L.csky_last_warning(self._h) or b"").decode()

    # ---- kernels, host-buffer forms
    def render_transmittance(self, w=256, h=64):
        p = TransParams()
        p.f[0], p.f[1] = float(w), float(h)
        out = np.zeros((h, w, 4), np.uint16)
        self._chk(self._L.csky_render_transmittance(self._h, C.byref(p), _ptr(out)))
        return out.view(np.float16)

    def render_sky_lut(self, sun_dir, w=200, h=100, readback=True):
        p = _sky_params(sun_dir, w, h)
        out = np.zeros((h, w, 4), np.uint16) if readback else None
        self._chk(self._L.csky_render_sky_lut(self._h, C.byref(p), _ptr(out) if readback else None))
        return out.view(np.float16) if readback else None

    def render_clouds(self, params, tile_w=None, tile_h=None):
        p = cloud_params(params)
        w, h = _frame_size(p, tile_w, tile_h)
        out = np.zeros((h, w, 4), np.uint16)
        self._chk(self._L.csky_render_clouds(self._h, C.byref(p), w, h, _ptr(out), w * 8))
        return out.view(np.float16)

    # ---- device-buffer forms
    def render_sky_lut_device(self, sun_dir, w=200, h=100, stream=None):
        p = _sky_params(sun_dir, w, h)
        self._chk(self._L.csky_render_sky_lut_device(self._h, C.byref(p), C.c_void_p(stream or 0)))

    def render_sky_lut_rows_device(self, sun_dir, first_row, row_stride, d_rows_out, capacity_bytes, w=200, h=100, stream=None):
        """One rank's rows first_row::row_stride of the sky LUT (N processes splitting a frame), compact RGBA16F into the caller's device buffer
        on `stream`; the context keeps no LUT, render_clouds_device renders the texels its frame set-up needs itself."""
        p = _sky_params(sun_dir, w, h)
        self._chk(self._L.csky_render_sky_lut_rows_device(self._h, C.byref(p), int(first_row), int(row_stride), C.c_void_p(int(d_rows_out)),
                                                          C.c_size_t(int(capacity_bytes)), C.c_void_p(stream or 0)))

    def render_clouds_device(self, params, tile_w, bands, d_out, pitch_bytes, stream=None):
        p = cloud_params(params)
        b = Bands(*[int(x) for x in bands])
        self._chk(self._L.csky_render_clouds_device(self._h, C.byref(p), int(tile_w), C.byref(b), C.c_void_p(int(d_out)), int(pitch_bytes),
                                                    C.c_void_p(stream or 0)))

    def interleave_bands_device(self, d_gathered, member_stride_bytes, members, band_bytes, total_bands, d_frame, stream=None):
        """The gathering rank's interleave: frame band k = member k % members, local band k // members of the gathered rank-major buffer."""
        self._chk(self._L.csky_interleave_bands_device(self._h, C.c_void_p(int(d_gathered)), C.c_size_t(int(member_stride_bytes)), int(members), C.c_size_t(int(band_bytes)),
                                                       int(total_bands), C.c_void_p(int(d_frame)), C.c_void_p(stream or 0)))

    def copy_sky_lut_device(self, d_out, stream=None):
        """Async device copy of the sky LUT rendered last (w*h*8 bytes of RGBA16F) into a caller-owned device buffer."""
        self._chk(self._L.csky_copy_sky_lut_device(self._h, C.c_void_p(int(d_out)), C.c_void_p(stream or 0)))

    def render_cloud_shadow(self, params, width, height, center=(0.0, 0.0), extent=(16384.0, 16384.0), steps=64, out=None, stream=None):
        """The cloud shadow map (csky_render_cloud_shadow*, definition: include/cloudsky.h): the sun's transmittance through the clouds of the
        push-constant block `params` to width x height ground points of the rectangle `extent` (metres along x, z) around `center`, float16
        [height, width], row j = z, column i = x.  Host path (out None or a numpy float16 array): blocks, returns numpy.  Device path (out a
        2-D torch tensor of 2-byte elements on this context's GPU, unit column stride; its row stride is the pitch): asynchronous on `stream`,
        returns the tensor.  Needs the noise and no LUT."""
        sp = _shadow_params(width, height, center, extent, steps)
        return self._render_image("render_cloud_shadow", params, (C.byref(sp),), (sp.height, sp.width), out, stream)

    def render_aerial_perspective(self, sun, width=32, height=32, depth=32, far_km=32.0, steps_per_slice=2, view=None, aspect=0.0, out=None, stream=None):
        """The aerial-perspective volume (csky_render_aerial_perspective*, definition: include/cloudsky.h): in-scattered light (rgb, the sky LUT's
        units) and transmittance (a) of the atmosphere in front of geometry, float16 [depth, height, width, 4]; slice k is the state at distance
        (k + 1) * far_km / depth along the column's ray.  view: None = the equirectangular panorama over the whole sphere, or (basis 3x3 with the
        camera's right / up / back axes as columns, fov_y_degrees) with `aspect` the screen's width / height (0 = width / height).  Host path (out
        None or a numpy float16 array): blocks, returns numpy.  Device path (out a contiguous torch tensor of 2-byte elements on this context's
        GPU): asynchronous on `stream`, written in place, returns the tensor.  Needs the transmittance LUT and nothing else."""
        shape, p, v = _aerial_args(sun, width, height, depth, far_km, steps_per_slice, view, aspect)
        if out is not None and hasattr(out, "data_ptr"):
            _device_image("render_aerial_perspective", "out", shape, out)
            self._chk(self._L.csky_render_aerial_perspective_device(self._h, C.byref(p), v, C.c_void_p(int(out.data_ptr())), C.c_void_p(stream or 0)))
            return out
        out = _host_image("render_aerial_perspective", shape, out)
        self._chk(self._L.csky_render_aerial_perspective(self._h, C.byref(p), v, _ptr(out)))
        return out

    def render_aerial_perspective_shadowed(self, sun, shadow, center, extent, width=32, height=32, depth=32, far_km=32.0, steps_per_slice=2, view=None, aspect=0.0,
                                           out=None, stream=None):
        """The aerial-perspective volume with a cloud shadow map inside it: light shafts (csky_render_aerial_perspective_shadowed*, definition:
        include/cloudsky.h).  `shadow` is the map render_cloud_shadow made for the rectangle `extent` around `center` (metres along x, z) under the
        same sun; the other arguments and the result are render_aerial_perspective's.  Host path (shadow a numpy float16 [h, w] array; out None or a
        numpy float16 array): blocks, returns numpy.  Device path (shadow a 2-D torch tensor of 2-byte elements on this context's GPU with unit
        column stride, whose row stride gives the pitch; out a contiguous torch tensor of 2-byte elements or None): asynchronous on `stream`, on
        which the map is read; returns the tensor.  Needs the transmittance LUT and nothing else."""
        name = "render_aerial_perspective_shadowed"
        shape, p, v = _aerial_args(sun, width, height, depth, far_km, steps_per_slice, view, aspect)
        if hasattr(shadow, "data_ptr"):
            if shadow.dim() != 2:
                raise ValueError("%s: shadow must be a 2-D tensor of 2-byte elements with unit column stride" % name)
            pitch = _device_image(name, "shadow", tuple(shadow.shape), shadow, pitched=True)
            sp = _shadow_params(shadow.shape[1], shadow.shape[0], center, extent, 0)
            if out is None:
                import torch
                out = torch.empty(shape, dtype=torch.float16, device=shadow.device)
            _device_image(name, "out", shape, out)
            self._chk(self._L.csky_render_aerial_perspective_shadowed_device(self._h, C.byref(p), v, C.byref(sp), C.c_void_p(int(shadow.data_ptr())), C.c_size_t(pitch),
                                                                             C.c_void_p(int(out.data_ptr())), C.c_void_p(stream or 0)))
            return out
        shadow = np.asarray(shadow)
        if shadow.ndim != 2 or shadow.dtype != np.float16:
            raise ValueError("%s: shadow must be a float16 [h, w] array (or a 2-D torch tensor on the GPU)" % name)
        shadow = np.ascontiguousarray(shadow)
        sp = _shadow_params(shadow.shape[1], shadow.shape[0], center, extent, 0)
        if out is not None and not isinstance(out, np.ndarray):   # this method alone refuses what is no array at all (the others fail on its missing attributes)
            raise ValueError("%s: with a host map, out must be a numpy array" % name)
        out = _host_image(name, shape, out)
        self._chk(self._L.csky_render_aerial_perspective_shadowed(self._h, C.byref(p), v, C.byref(sp), _ptr(shadow), _ptr(out)))
        return out

    def render_cloud_depth(self, params, width, height, steps=0, out=None, stream=None):
        """The cloud depth frame (csky_render_cloud_depth*, definition: include/cloudsky.h): for the rays of a width x height hemisphere frame
        of the push-constant block `params`, the cloud's mean, first and last distance from the observer in km and the frame's alpha, float16
        [height, width, 4].  steps 0 = the context's primary step count.  Host path (out None or a numpy float16 array): blocks, returns numpy.
        Device path (out a [height, width, 4] torch tensor of 2-byte elements on this context's GPU whose texels are contiguous; its row stride
        is the pitch): asynchronous on `stream`, written in place, returns the tensor.  Needs the noise and no LUT."""
        dp = DepthParams(int(width), int(height), int(steps))
        return self._render_image("render_cloud_depth", params, (C.byref(dp),), (dp.height, dp.width, 4), out, stream)

    def apply_cloud_aerial(self, sun, cloud, depth, steps=16, out=None, stream=None):
        """The air in front of a cloud frame (csky_apply_cloud_aerial*, definition: include/cloudsky.h): `cloud` a hemisphere frame and `depth`
        its depth frame (render_cloud_depth), both float16 [h, w, 4]; the result is the frame with the atmosphere's extinction and in-scattering
        over each pixel's mean cloud distance under the sun `sun` (used as given), its alpha unchanged.  Host path (numpy arrays): blocks,
        returns numpy.  Device path (contiguous torch tensors of 2-byte elements on this context's GPU): asynchronous on `stream`, returns
        `out`, a new tensor unless given; out may be `cloud`.  Needs the transmittance LUT and nothing else."""
        return self._apply_rays("apply_cloud_aerial", (), sun, cloud, depth, steps, out, stream)

    def _render_image(self, name, params, mid, shape, out, stream, dirs=None, after=()):
        """The one path of every method that renders an image of `shape` from a push-constant block: csky_<name>(ctx, params, *mid[, dirs], *after, out) for a
        host image (None: a new one), csky_<name>_device(ctx, params, *mid[, dirs], *after, out, pitch, stream) for a tensor, whose row stride is the pitch.  With
        `dirs` ([h, w, 3]) the directions decide which of the two it is: `out` must be of their kind, and a missing device `out` is made next to them."""
        p = cloud_params(params)
        device = hasattr(out if dirs is None else dirs, "data_ptr")
        if dirs is not None:
            mid += (_dirs_arg(name, dirs, device),)
        mid += tuple(after)
        if device:
            if out is None:
                import torch
                out = torch.empty(shape, dtype=torch.float16, device=dirs.device)
            pitch = _device_image(name, "out", shape, out, pitched=True)     # (refuses a numpy out beside device dirs)
            self._chk(getattr(self._L, "csky_%s_device" % name)(self._h, C.byref(p), *mid, C.c_void_p(int(out.data_ptr())), C.c_size_t(pitch), C.c_void_p(stream or 0)))
        else:
            out = _host_image(name, shape, out)                              # (refuses a tensor beside host dirs: it is no float16 array)
            self._chk(getattr(self._L, "csky_" + name)(self._h, C.byref(p), *mid, _ptr(out)))
        return out

    def render_clouds_dirs(self, params, dirs, out=None, stream=None):
        """The direct cloud march over caller-given rays (csky_render_clouds_dirs*, definition: include/cloudsky.h): `dirs` is [h, w, 3] float32, a
        direction per pixel, used as given; the result is what the hemisphere frame stores for that ray, float16 [h, w, 4].  A direction at or
        under the horizon, or whose squared length is outside [0.99, 1.01], gives a zero texel.  texture_size and update_position of `params`
        are not read.  Host path (dirs a numpy array; out None or a numpy float16 array): blocks, returns numpy.  Device path (dirs a contiguous
        float32 torch tensor on this context's GPU; out a [h, w, 4] tensor of 2-byte elements whose texels are contiguous, its row stride the
        pitch, or None for a new one): asynchronous on `stream`, returns the tensor.  Needs the noise and a sky LUT."""
        w, h = _dirs_size("render_clouds_dirs", dirs)
        return self._render_image("render_clouds_dirs", params, (w, h), (h, w, 4), out, stream, dirs=dirs)

    def render_clouds_view(self, params, basis, fov_y_degrees, width, height, out=None, stream=None):
        """The direct cloud march of a camera view (csky_render_clouds_view*, definition: include/cloudsky.h): the ray of every SCREEN pixel of a
        width x height perspective camera, the EYEDIR composite_view uses (basis: 3x3, columns = the camera's right / up / back axes), marched as
        the hemisphere frame's rays are; float16 [height, width, 4], zero under the horizon.  Host path (out None or a numpy float16 array):
        blocks, returns numpy.  Device path (out a [height, width, 4] torch tensor of 2-byte elements on this context's GPU whose texels are
        contiguous; its row stride is the pitch): asynchronous on `stream`, written in place, returns the tensor.  Needs the noise and a sky LUT."""
        v = _view(basis, fov_y_degrees)
        return self._render_image("render_clouds_view", params, (C.byref(v), int(width), int(height)), (int(height), int(width), 4), out, stream)

    def render_clouds_view_from(self, params, basis, fov_y_degrees, width, height, position, max_distance=float("inf"), out=None, stream=None):
        """render_clouds_view for an observer who stands at `position` (csky_render_clouds_view_from*, definition: include/cloudsky.h): three numbers,
        metres from the reference's camera, y up; under, inside or above the cloud layer.  Each ray's first segment through the layer is marched, at
        most `max_distance` metres from the observer; a ray without one gives a zero texel.  position (0, 0, 0) without a cap gives
        render_clouds_view's bytes.  Host and device path as there."""
        name = "render_clouds_view_from"
        v, o = _view(basis, fov_y_degrees), _observer(name, position, max_distance)
        return self._render_image(name, params, (C.byref(v), C.byref(o), int(width), int(height)), (int(height), int(width), 4), out, stream)

    def render_clouds_dirs_from(self, params, dirs, position, max_distance=float("inf"), out=None, stream=None):
        """render_clouds_dirs for an observer who stands at `position` (csky_render_clouds_dirs_from*; see render_clouds_view_from).  A direction may
        point under the horizon; one whose squared length is outside [0.99, 1.01] gives a zero texel.  Host and device path as render_clouds_dirs."""
        name = "render_clouds_dirs_from"
        w, h = _dirs_size(name, dirs)
        o = _observer(name, position, max_distance)
        return self._render_image(name, params, (w, h), (h, w, 4), out, stream, dirs=dirs, after=(C.byref(o),))

    def render_clouds_view_from_depth(self, params, basis, fov_y_degrees, width, height, position, depth, depth_kind="distance", max_distance=float("inf"), out=None,
                                      stream=None):
        """render_clouds_view_from behind the host's scene (csky_render_clouds_view_from_depth*, definition: include/cloudsky.h): `depth` is a float32
        [height, width] buffer in metres, along each pixel's ray from the observer (depth_kind "distance") or along the camera's forward axis
        ("view_z", a rasteriser's linear depth).  Each ray ends at its pixel's depth as well as at max_distance: the frame holds the cloud in front
        of the geometry.  inf: nothing in the way; 0, negatives and NaN: geometry at the lens, a zero texel.  The kind of `depth` selects the path:
        a numpy array the host path (out None or a numpy float16 array; blocks, returns numpy), a float32 torch tensor on this context's GPU whose
        texels are contiguous, its row stride the pitch, the device path (out as render_clouds_view's or None for a new tensor; asynchronous on
        `stream`).  depth and out must not overlap."""
        name = "render_clouds_view_from_depth"
        shape = (int(height), int(width), 4)
        v, o = _view(basis, fov_y_degrees), _observer(name, position, max_distance)
        d, device = _scene_depth(name, depth, depth_kind, width, height, True)
        if out is not None and hasattr(out, "data_ptr") != device:
            raise ValueError("%s: depth and out must both be numpy arrays or both be tensors on the GPU" % name)
        if device and out is None:
            import torch
            out = torch.empty(shape, dtype=torch.float16, device=depth.device)
        return self._render_image(name, params, (C.byref(v), C.byref(o), int(width), int(height), C.byref(d)), shape, out, stream)

    def render_clouds_dirs_from_depth(self, params, dirs, position, depth, depth_kind="distance", max_distance=float("inf"), out=None, stream=None):
        """render_clouds_dirs_from behind the host's scene (csky_render_clouds_dirs_from_depth*; see render_clouds_view_from_depth): `depth` is a
        float32 [h, w] buffer of metres along each of the caller's rays; "distance" is its only kind.  dirs and depth are both numpy arrays (the
        host path) or both tensors on this context's GPU (the device path)."""
        name = "render_clouds_dirs_from_depth"
        w, h = _dirs_size(name, dirs)
        o = _observer(name, position, max_distance)
        d, device = _scene_depth(name, depth, depth_kind, w, h, False)
        if hasattr(dirs, "data_ptr") != device:
            raise ValueError("%s: dirs and depth must both be numpy arrays or both be tensors on the GPU" % name)
        return self._render_image(name, params, (w, h), (h, w, 4), out, stream, dirs=dirs, after=(C.byref(o), C.byref(d)))

    def render_clouds_view_update(self, params, basis, fov_y_degrees, width, height, block, phase, prev=None, prev_basis=None, prev_fov=None, out=None, stream=None):
        """The temporal split of a view frame (csky_render_clouds_view_update*, definition: include/cloudsky.h): one pixel of every block x block
        pixels (the one at (phase % block, phase // block)) is marched as render_clouds_view marches it, every other pixel is taken from `prev`,
        the view frame of the camera (prev_basis, prev_fov), through that camera; a pixel `prev` does not cover is marched.  prev None: no
        history, the result is render_clouds_view's.  float16 [height, width, 4].  Host path (prev None or a numpy float16 array; out None or a
        numpy float16 array): blocks, returns numpy.  Device path (prev and out [height, width, 4] torch tensors of 2-byte elements on this
        context's GPU whose texels are contiguous, each with its own row stride as its pitch; out None for a new one beside prev): asynchronous
        on `stream`, returns the tensor.  prev and out must not overlap.  Needs the noise and a sky LUT."""
        name = "render_clouds_view_update"
        p = cloud_params(params)
        v = _view(basis, fov_y_degrees)
        shape = (int(height), int(width), 4)
        if prev is not None and (prev_basis is None or prev_fov is None):
            raise ValueError("%s: prev needs prev_basis and prev_fov" % name)
        pv = None if prev is None else C.byref(_view(prev_basis, prev_fov))
        mid = (C.byref(v), pv, shape[1], shape[0], int(block), int(phase))
        if hasattr(out if prev is None else prev, "data_ptr"):
            if out is None:
                import torch
                out = torch.empty(shape, dtype=torch.float16, device=prev.device)
            prev_pitch = 0 if prev is None else _device_image(name, "prev", shape, prev, pitched=True)
            pitch = _device_image(name, "out", shape, out, pitched=True)     # (refuses a numpy out beside a device prev)
            self._chk(self._L.csky_render_clouds_view_update_device(self._h, C.byref(p), *mid, None if prev is None else C.c_void_p(int(prev.data_ptr())), C.c_size_t(prev_pitch),
                                                                    C.c_void_p(int(out.data_ptr())), C.c_size_t(pitch), C.c_void_p(stream or 0)))
            return out
        if prev is not None:
            prev = np.ascontiguousarray(prev)
            if prev.shape != shape or prev.dtype != np.float16:
                raise ValueError("%s: prev must be a float16 %s array (or a torch tensor on the GPU)" % (name, shape))
        out = _host_image(name, shape, out)                                  # (refuses a tensor beside a host prev: it is no float16 array)
        self._chk(self._L.csky_render_clouds_view_update(self._h, C.byref(p), *mid, None if prev is None else _ptr(prev), _ptr(out)))
        return out

    def render_cloud_depth_dirs(self, params, dirs, steps=0, out=None, stream=None):
        """The depth frame of a ray frame (csky_render_cloud_depth_dirs*, definition: include/cloudsky.h): for each direction of `dirs`
        ([h, w, 3] float32, used as given, accepted as render_clouds_dirs accepts them) the cloud's mean, first and last distance in km and the
        ray's alpha, float16 [h, w, 4]; zero where the direction is not accepted.  steps 0 = the context's primary step count, render_clouds_dirs'
        own.  Host path (dirs a numpy array): blocks, returns numpy.  Device path (dirs a contiguous float32 torch tensor on this context's GPU;
        out a [h, w, 4] tensor of 2-byte elements whose texels are contiguous, its row stride the pitch, or None for a new one): asynchronous
        on `stream`, returns the tensor.  Needs the noise and no LUT."""
        w, h = _dirs_size("render_cloud_depth_dirs", dirs)
        return self._render_image("render_cloud_depth_dirs", params, (w, h, int(steps)), (h, w, 4), out, stream, dirs=dirs)

    def render_cloud_depth_view(self, params, basis, fov_y_degrees, width, height, steps=0, out=None, stream=None):
        """The depth frame of a camera view (csky_render_cloud_depth_view*, definition: include/cloudsky.h): render_cloud_depth for the rays of
        render_clouds_view's image, float16 [height, width, 4].  steps 0 = the context's primary step count, the view frame's own.  Host path
        (out None or a numpy float16 array): blocks, returns numpy.  Device path (out a [height, width, 4] torch tensor of 2-byte elements on
        this context's GPU whose texels are contiguous; its row stride is the pitch): asynchronous on `stream`, written in place, returns the
        tensor.  Needs the noise and no LUT."""
        v = _view(basis, fov_y_degrees)
        return self._render_image("render_cloud_depth_view", params, (C.byref(v), int(width), int(height), int(steps)), (int(height), int(width), 4), out, stream)

    def _apply_rays(self, name, mid, sun, cloud, depth, steps, out, stream, dirs=None):
        """The one path of apply_cloud_aerial and its ray forms: csky_<name>(ctx, params, *mid[, dirs], cloud, depth, out) for host frames,
        csky_<name>_device(..., stream) for tensors; `cloud` decides which, and every other image must be of its kind.  These calls take no pitch."""
        shape = tuple(int(x) for x in cloud.shape)
        if len(shape) != 3 or shape[2] != 4 or tuple(int(x) for x in depth.shape) != shape:
            raise ValueError("%s: cloud and depth must be [h, w, 4] images of one size" % name)
        if dirs is not None and tuple(int(x) for x in dirs.shape) != (shape[0], shape[1], 3):
            raise ValueError("%s: dirs must be a [h, w, 3] float32 image of the frames' size" % name)
        p = CloudAerialParams(shape[1], shape[0], int(steps), _sun3(sun))
        device = hasattr(cloud, "data_ptr")
        if dirs is not None:
            mid += (_dirs_arg(name, dirs, device),)
        if device:
            if out is None:
                import torch
                out = torch.empty(shape, dtype=torch.float16, device=cloud.device)
            for what, t in (("cloud", cloud), ("depth", depth), ("out", out)):
                _device_image(name, what, shape, t)
            self._chk(getattr(self._L, "csky_%s_device" % name)(self._h, C.byref(p), *mid, *[C.c_void_p(int(t.data_ptr())) for t in (cloud, depth, out)],
                                                                 C.c_void_p(stream or 0)))
            return out
        cloud, depth = np.ascontiguousarray(cloud), np.ascontiguousarray(depth)
        if cloud.dtype != np.float16 or depth.dtype != np.float16:
            raise ValueError("%s: cloud and depth must be float16 arrays (or torch tensors on the GPU)" % name)
        out = _host_image(name, shape, out)
        self._chk(getattr(self._L, "csky_" + name)(self._h, C.byref(p), *mid, _ptr(cloud), _ptr(depth), _ptr(out)))
        return out

    def apply_cloud_aerial_dirs(self, sun, dirs, cloud, depth, steps=16, out=None, stream=None):
        """apply_cloud_aerial for a ray frame (csky_apply_cloud_aerial_dirs*, definition: include/cloudsky.h): `cloud` the image of
        render_clouds_dirs for `dirs` ([h, w, 3] float32) and `depth` that of render_cloud_depth_dirs.  A pixel whose direction the march does
        not accept leaves as it came.  Host path (numpy arrays) and device path (contiguous torch tensors on this context's GPU) as
        apply_cloud_aerial's; out may be `cloud`.  Needs the transmittance LUT and nothing else."""
        return self._apply_rays("apply_cloud_aerial_dirs", (), sun, cloud, depth, steps, out, stream, dirs=dirs)

    def apply_cloud_aerial_view(self, sun, basis, fov_y_degrees, cloud, depth, steps=16, out=None, stream=None):
        """apply_cloud_aerial for a view frame (csky_apply_cloud_aerial_view*, definition: include/cloudsky.h): `cloud` the image of
        render_clouds_view for this camera and `depth` that of render_cloud_depth_view, both float16 [h, w, 4].  Host path (numpy arrays) and
        device path (contiguous torch tensors on this context's GPU) as apply_cloud_aerial's; out may be `cloud`.  Needs the transmittance LUT
        and nothing else."""
        v = _view(basis, fov_y_degrees)
        return self._apply_rays("apply_cloud_aerial_view", (C.byref(v),), sun, cloud, depth, steps, out, stream)

    def set_shadow_exact_end(self, enabled=True):
        """A/B switch (cloudsky_internal.h): False makes every texel of the shadow map take all its samples; the maps are byte-identical."""
        self._chk(self._L.csky_set_shadow_exact_end(self._h, int(bool(enabled))))

    def sync(self):
        self._chk(self._L.csky_sync(self._h))

    def import_external_frame(self, fd, allocation_bytes, offset_bytes, frame_bytes):
        """Zero-copy interop (csky_external_frame_import_fd): memory another API allocated, handed over as a POSIX fd (the library owns the fd on
        success).  Returns an ExternalFrame whose `.ptr` is usable as d_out of render_clouds_device."""
        ef, dptr = C.c_void_p(), C.c_void_p()
        self._chk(self._L.csky_external_frame_import_fd(self._h, int(fd), C.c_size_t(int(allocation_bytes)), C.c_size_t(int(offset_bytes)), C.c_size_t(int(frame_bytes)),
                                                        C.byref(ef), C.byref(dptr)))
        return ExternalFrame(self, ef, dptr.value)

    def census_clouds(self, params, tile_w, bands, n=256):
        """Basic-block execution counts of one launch (non-zero only with the census build of the library, tools/isa_profile.py)."""
        p = cloud_params(params)
        b = Bands(*[int(x) for x in bands])
        out = np.zeros(n, np.uint32)
        self._chk(self._L.csky_census_clouds(self._h, C.byref(p), int(tile_w), C.byref(b), _ptr(out), int(n)))
        return out

    # ---- asynchronous host form (pinned ring)
    def set_host_ring(self, slots):
        self._chk(self._L.csky_set_host_ring(self._h, int(slots)))

    def submit_clouds(self, params, tile_w=None, tile_h=None):
        """Enqueue march + copy into a pinned ring slot; returns the ticket at once."""
        p = cloud_params(params)
        w, h = _frame_size(p, tile_w, tile_h)
        t = C.c_int64(-1)
        self._chk(self._L.csky_submit_clouds(self._h, C.byref(p), w, h, C.byref(t)))
        self._shapes = getattr(self, "_shapes", {})
        self._shapes[t.value] = (h, w)
        return t.value

    def collect(self, ticket, copy=True):
        """Wait for the frame of `ticket`: float16 [h, w, 4].  copy=False returns a VIEW of the pinned ring slot (valid until the slot is reused)."""
        ptr, n = C.c_void_p(), C.c_size_t()
        self._chk(self._L.csky_collect(self._h, int(ticket), C.byref(ptr), C.byref(n)))
        h, w = self._shapes.pop(int(ticket))
        a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint16)), shape=(h, w, 4))
        return (a.copy() if copy else a).view(np.float16)

    def poll(self, ticket):
        rc = self._L.csky_poll(self._h, int(ticket))
        if rc < 0:
            self._chk(rc)
        return rc == 1

    def read_transmittance(self):
        w, h = C.c_int(), C.c_int()
        self._chk(self._L.csky_read_transmittance(self._h, None, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value, 4), np.uint16)
        self._chk(self._L.csky_read_transmittance(self._h, _ptr(out), C.byref(w), C.byref(h)))
        return out.view(np.float16)

    def read_sky_lut(self):
        w, h = C.c_int(), C.c_int()
        self._chk(self._L.csky_read_sky_lut(self._h, None, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value, 4), np.uint16)
        self._chk(self._L.csky_read_sky_lut(self._h, _ptr(out), C.byref(w), C.byref(h)))
        return out.view(np.float16)

    def composite_sky(self, cloud_from, cloud_to, sky_from, sky_to, light_dir, blend_amount=0.0, sun_disk_scale=2.0, out_w=2048, out_h=1024):
        """clouds.gdshader sky() on an equirectangular panorama; inputs float16 [h, w, 4] host arrays."""
        return self._composite(self._L.csky_composite_sky, (), (cloud_from, cloud_to, sky_from, sky_to), light_dir, blend_amount, sun_disk_scale, out_w, out_h)

    def composite_view(self, cloud_from, cloud_to, sky_from, sky_to, light_dir, basis, fov_y_degrees, blend_amount=0.0, sun_disk_scale=2.0, out_w=1152, out_h=648):
        """clouds.gdshader sky() per SCREEN pixel of a perspective camera (basis: 3x3, columns = the camera's right / up / back axes)."""
        v = _view(basis, fov_y_degrees)
        return self._composite(self._L.csky_composite_view, (C.byref(v),), (cloud_from, cloud_to, sky_from, sky_to), light_dir, blend_amount, sun_disk_scale, out_w, out_h)

    def composite_view_frames(self, cloud_from, cloud_to, sky_from, sky_to, light_dir, basis, fov_y_degrees, blend_amount=0.0, sun_disk_scale=2.0):
        """composite_view with cloud_from / cloud_to being VIEW frames of the same camera (render_clouds_view), float16 [out_h, out_w, 4]: each
        screen pixel reads its own cloud texel instead of tapping a hemisphere frame (csky_composite_view_frames)."""
        v = _view(basis, fov_y_degrees)
        out_h, out_w = np.shape(cloud_from)[:2]
        return self._composite(self._L.csky_composite_view_frames, (C.byref(v),), (cloud_from, cloud_to, sky_from, sky_to), light_dir, blend_amount, sun_disk_scale, out_w, out_h)

    def _composite(self, call, view, frames, light_dir, blend_amount, sun_disk_scale, out_w, out_h):
        """The compositor's host forms: call(ctx, params, *view, the four frames, out) -> the out_h x out_w image, float16 [out_h, out_w, 4]."""
        a, cloud_wh, sky_wh = _host_frames(*frames)
        p = _composite_params(out_w, out_h, cloud_wh, sky_wh, light_dir, blend_amount, sun_disk_scale)
        out = np.zeros((out_h, out_w, 4), np.uint16)
        self._chk(call(self._h, C.byref(p), *view, *[_ptr(x) for x in a], _ptr(out)))
        return out.view(np.float16)

    def render_radiance(self, cloud_from, cloud_to, sky_from, sky_to, light_dir, blend_amount=0.0, sun_disk_scale=2.0, face_size=64, layers=8, source_size=0,
                        first_layer=0, n_layers=None, out=None):
        """The sky's radiance cubemap (csky_render_radiance): layer 0 = clouds.gdshader sky() on the six faces, layers 1..L-1 GGX-prefiltered.
        Inputs float16 [h, w, 4] host arrays.  Returns float16 [L, 6, S, S, 4]; only layers [first_layer, first_layer + n_layers) are written
        (into `out` when given)."""
        S, L = int(face_size), int(layers)
        n_layers = L - int(first_layer) if n_layers is None else int(n_layers)
        a, cloud_wh, sky_wh = _host_frames(cloud_from, cloud_to, sky_from, sky_to)
        p = _composite_params(S, S, cloud_wh, sky_wh, light_dir, blend_amount, sun_disk_scale)
        rp = RadianceParams(S, L, int(source_size))
        out = _host_image("render_radiance", (L, 6, S, S, 4), out)
        self._chk(self._L.csky_render_radiance(self._h, C.byref(p), C.byref(rp), *[_ptr(x) for x in a], int(first_layer), n_layers, _ptr(out)))
        return out

    def render_radiance_device(self, d_cloud_from, d_cloud_to, d_sky_from, d_sky_to, cloud_wh, sky_wh, light_dir, blend_amount, sun_disk_scale, face_size,
                               layers, source_size, first_layer, n_layers, d_out, stream=None):
        """csky_render_radiance_device: device pointers in and out (d_out: the whole [L, 6, S, S, 4] half array), asynchronous on `stream`."""
        S = int(face_size)
        p = _composite_params(S, S, cloud_wh, sky_wh, light_dir, blend_amount, sun_disk_scale)
        rp = RadianceParams(S, int(layers), int(source_size))
        ptrs = [C.c_void_p(int(x) if x else 0) for x in (d_cloud_from, d_cloud_to, d_sky_from, d_sky_to)]
        self._chk(self._L.csky_render_radiance_device(self._h, C.byref(p), C.byref(rp), *ptrs, int(first_layer), int(n_layers), C.c_void_p(int(d_out)),
                                                      C.c_void_p(stream or 0)))

    def prefilter_cube(self, cube, layers=8, source_size=0, first_layer=0, n_layers=None):
        """csky_prefilter_cube: the radiance filter applied to a caller cube, float16 [6, S, S, 4] -> float16 [L, 6, S, S, 4] (layer 0 = the
        input; layers outside [first_layer, first_layer + n_layers) stay zero)."""
        c = np.ascontiguousarray(cube, np.float16)
        if c.ndim != 4 or c.shape[0] != 6 or c.shape[1] != c.shape[2] or c.shape[3] != 4:
            raise ValueError("prefilter_cube: expected float16 [6, S, S, 4]")
        S, L = c.shape[1], int(layers)
        n_layers = L - int(first_layer) if n_layers is None else int(n_layers)
        out = np.zeros((L, 6, S, S, 4), np.float16)
        self._chk(self._L.csky_prefilter_cube(self._h, _ptr(c), S, L, int(source_size), int(first_layer), n_layers, _ptr(out)))
        return out

    def generate_shape_noise(self, seed=1, n=128, **knobs):
        """GPU bake of the stand-in shape volume: uint8 [n, n, n, 4], byte-identical to assets.generate_shape_noise (knobs: ShapeNoiseParams fields)."""
        vol = np.zeros((n, n, n, 4), np.uint8)
        p = shape_noise_params(**knobs)
        self._chk(self._L.csky_generate_shape_noise_tuned_device(self._h, seed, n, C.byref(p), _ptr(vol)))
        return vol

    def generate_detail_noise(self, seed=1, n=32):
        """GPU bake of a generated detail volume: uint8 [n, n, n, 3], byte-identical to assets.generate_detail_noise."""
        vol = np.zeros((n, n, n, 3), np.uint8)
        self._chk(self._L.csky_generate_detail_noise_device(self._h, seed, n, _ptr(vol)))
        return vol

    def build_mips(self, level0, levels):
        """2x2x2 box mip chain on the GPU (flat uint8, level 0 first): byte-identical to assets.build_mips."""
        level0 = np.ascontiguousarray(level0, np.uint8)
        n, ch = level0.shape[0], level0.shape[3]
        buf = np.zeros(self._L.csky_mip_offset(n, levels, ch), np.uint8)
        buf[: level0.size] = level0.reshape(-1)
        self._chk(self._L.csky_build_mips_device(self._h, _ptr(buf), n, ch, levels))
        return buf

    def test_sqrt_shell(self, x):
        """Test hook: cloud_core.h::sqrt_shell on the device over a float32 array."""
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros_like(x)
        self._chk(self._L.csky_test_sqrt_shell(self._h, _ptr(x), _ptr(out), x.size))
        return out

    def test_primitive(self, op, *arrays):
        """Test hook: one of the march's arithmetic primitives (PRIMITIVES) on the device over arrays, one element per lane."""
        return run_primitive(lambda *a: self._chk(self._L.csky_test_primitive(self._h, *a)), op, arrays)

    def test_static_order(self, mode, tiles_x, slabs):
        """Test hook: the static workgroup order (mode 1, 2 or 5) of a tiles_x x slabs launch as the device writes it; its length is the launch's grid."""
        grid = C.c_int()
        self._chk(self._L.csky_test_static_order(self._h, int(mode), int(tiles_x), int(slabs), None, 0, C.byref(grid)))
        out = np.zeros(grid.value, np.uint32)
        self._chk(self._L.csky_test_static_order(self._h, int(mode), int(tiles_x), int(slabs), _ptr(out), out.size, C.byref(grid)))
        return out

    def test_lpt_order(self, cost, shift, rounds=1):
        """Test hook: the cost-feedback sort, `rounds` times on the same device buffers -> (order of the last round, cost as left, the 2048 scratch words as left)."""
        cost = np.ascontiguousarray(cost, np.uint32)
        order, left, scratch = np.zeros(cost.size, np.uint32), np.ones(cost.size, np.uint32), np.ones(2048, np.uint32)
        self._chk(self._L.csky_test_lpt_order(self._h, _ptr(cost), cost.size, int(shift), int(rounds), _ptr(order), _ptr(left), _ptr(scratch)))
        return order, left, scratch

    def read_baked_texture(self, which):
        """Test hook: the device layouts / mip chains csky_set_noise built, as raw bytes (0 shape, 1 detail, 2 weather, 3 / 4 8-bit chains, 5 the
        unpacked fp16 detail chain, 6 / 7 / 8 the exact fp32 cells of shape / detail / weather -- CloudSkyError with code CSKY_ERR_STATE when the
        bound set has none --, 9 the 24 bytes the context holds from the bake: uint64 inexact; int32 rmin, rmax, bmax; float32 lod5)."""
        n = C.c_size_t()
        self._chk(self._L.csky_read_baked_texture(self._h, int(which), None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint8)
        self._chk(self._L.csky_read_baked_texture(self._h, int(which), _ptr(out), out.nbytes, C.byref(n)))
        return out

    # ---- measurement
    def time_clouds(self, params, tile_w, bands, warmup=2, iters=10):
        p = cloud_params(params)
        b = Bands(*[int(x) for x in bands])
        ms = C.c_float()
        st = CloudStats()
        self._chk(self._L.csky_time_clouds(self._h, C.byref(p), int(tile_w), C.byref(b), warmup, iters, C.byref(ms), C.byref(st)))
        return ms.value, dict(rays=st.rays, primary_samples=st.primary_samples, incloud_samples=st.incloud_samples)

    def set_frames_in_flight(self, frames):
        self._chk(self._L.csky_set_frames_in_flight(self._h, int(frames)))

    def set_kernel_timing(self, enabled=True):
        self._chk(self._L.csky_set_kernel_timing(self._h, int(bool(enabled))))

    def kernel_ms(self):
        """(sum of cloud-kernel durations in ms, launches) since the last call; waits for those launches."""
        ms, n = C.c_float(), C.c_int()
        self._chk(self._L.csky_get_kernel_ms(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def cloud_stats(self):
        st = CloudStats()
        self._chk(self._L.csky_get_cloud_stats(self._h, C.byref(st)))
        return dict(rays=st.rays, primary_samples=st.primary_samples, incloud_samples=st.incloud_samples)


class ExternalFrame:
    """A frame that lives in imported memory.  Ordering is the host-side fence (ROCm 7.2 on Linux refuses external semaphores)."""

    def __init__(self, ctx, handle, ptr):
        self._ctx, self._h, self.ptr = ctx, handle, ptr

    def fence(self, stream=None):
        self._ctx._chk(self._ctx._L.csky_external_frame_fence(self._ctx._h, self._h, C.c_void_p(stream or 0)))

    def ready(self):
        rc = self._ctx._L.csky_external_frame_ready(self._ctx._h, self._h)
        if rc < 0:
            self._ctx._chk(rc)
        return bool(rc)

    def wait(self):
        self._ctx._chk(self._ctx._L.csky_external_frame_wait(self._ctx._h, self._h))

    def release(self):
        if self._h is not None:
            self._ctx._L.csky_external_frame_release(self._h)
            self._h, self.ptr = None, 0


class MultiContext:
    """csky_multi: the GPUs of one node behind one handle, one host thread (include/cloudsky.h).  Device i of n renders the
    8-row bands i, i+n, ... and stores them straight into the frame on the first device (xGMI peer access)."""

    def __init__(self, device_ids):
        self._L = lib()
        ids = (C.c_int * len(device_ids))(*[int(d) for d in device_ids])
        h = C.c_void_p()
        rc = self._L.csky_multi_create(C.byref(h), ids, len(device_ids))
        if rc != OK:
            raise CloudSkyError(rc, (self._L.csky_multi_last_error(None) or b"").decode())
        self._h = h
        self.device_ids = [int(d) for d in device_ids]

    def _chk(self, rc):
        if rc != OK:
            raise CloudSkyError(rc, (self._L.csky_multi_last_error(self._h) or b"").decode())

    def __len__(self):
        return self._L.csky_multi_device_count(self._h)

    def last_warning(self):
        """"" or what csky_multi_create fell back on (a device without peer access to the first: staged copies, whole LUT on the first device)."""
        return (self._L.csky_multi_last_warning(self._h) or b"").decode()

    def set_timing(self, enabled=True):
        self._chk(self._L.csky_multi_set_timing(self._h, 1 if enabled else 0))

    def stats(self):
        """Preconditions + (set_timing) the last frame's per-device march / peer-copy milliseconds; waits for the handle's work."""
        st = MultiStats()
        self._chk(self._L.csky_multi_get_stats(self._h, C.byref(st)))
        n = min(st.n_devices, MULTI_STATS_MAX)
        return dict(n_devices=st.n_devices, staged=bool(st.staged), all_peer=bool(st.all_peer), groups=st.groups, frames_in_flight=st.frames_in_flight, timing=bool(st.timing),
                    device_id=list(st.device_id[:n]), peer_access=list(st.peer_access[:n]), march_ms=[round(float(x), 4) for x in st.march_ms[:n]],
                    copy_ms=[round(float(x), 4) for x in st.copy_ms[:n]])

    def ctx(self, i):
        """The per-device context (borrowed: per-context settings such as set_variant / set_schedule go through it)."""
        p = self._L.csky_multi_ctx(self._h, int(i))
        if not p:
            raise IndexError(i)
        return Context(self.device_ids[i], _borrowed=p)

    def close(self):
        if getattr(self, "_h", None):
            self._L.csky_multi_destroy(self._h)
            self._h = None

    __del__ = close

    def set_noise(self, large_rgba8, small_rgb8, weather_rgb8):
        a, b, c = (np.ascontiguousarray(x, np.uint8) for x in (large_rgba8, small_rgb8, weather_rgb8))
        if a.size != 128 ** 3 * 4 or b.size != 32 ** 3 * 3 or c.size != 512 * 512 * 3:
            raise ValueError("set_noise: expected 128^3 RGBA8, 32^3 RGB8, 512^2 RGB8")
        self._chk(self._L.csky_multi_set_noise(self._h, _ptr(a), _ptr(b), _ptr(c)))

    def set_noise_mips(self, large_chain_rgba8, small_chain_rgb8, weather_rgb8):
        a, b, c = (np.ascontiguousarray(x, np.uint8) for x in (large_chain_rgba8, small_chain_rgb8, weather_rgb8))
        if a.size != self._L.csky_mip_offset(128, 8, 4) or b.size != self._L.csky_mip_offset(32, 6, 3) or c.size != 512 * 512 * 3:
            raise ValueError("set_noise_mips: expected the 8-level 128^3 RGBA8 chain, the 6-level 32^3 RGB8 chain, 512^2 RGB8")
        self._chk(self._L.csky_multi_set_noise_mips(self._h, _ptr(a), _ptr(b), _ptr(c)))

    def set_march(self, primary_steps=128, light_steps=6):
        self._chk(self._L.csky_multi_set_march(self._h, primary_steps, light_steps))

    def set_transmittance_mapping(self, mapping):
        self._chk(self._L.csky_multi_set_transmittance_mapping(self._h, tlut_mapping(mapping)))

    def set_frames_in_flight(self, frames):
        """2..8: consecutive render_clouds_device calls rotate that many consumer streams (per frame group); every device does too."""
        self._chk(self._L.csky_multi_set_frames_in_flight(self._h, int(frames)))

    def set_groups(self, groups):
        """Frame groups for throughput workloads: consecutive frames go to `groups` groups of len(self)/groups devices in turn."""
        self._chk(self._L.csky_multi_set_groups(self._h, int(groups)))

    def set_staged(self, staged):
        """True: local band buffers + one strided peer copy per device instead of in-place peer stores from inside the march."""
        self._chk(self._L.csky_multi_set_staged(self._h, 1 if staged else 0))

    def render_sky_lut(self, sun_dir, w=200, h=100):
        p = _sky_params(sun_dir, w, h)
        self._chk(self._L.csky_multi_render_sky_lut(self._h, C.byref(p)))

    def render_clouds(self, params, tile_w=None, tile_h=None):
        p = cloud_params(params)
        w, h = _frame_size(p, tile_w, tile_h)
        out = np.zeros((h, w, 4), np.uint16)
        self._chk(self._L.csky_multi_render_clouds(self._h, C.byref(p), w, h, _ptr(out), w * 8))
        return out.view(np.float16)

    def render_clouds_device(self, params, tile_w, tile_h, d_out, pitch_bytes, stream=None):
        p = cloud_params(params)
        self._chk(self._L.csky_multi_render_clouds_device(self._h, C.byref(p), int(tile_w), int(tile_h), C.c_void_p(int(d_out)), int(pitch_bytes),
                                                          C.c_void_p(stream or 0)))

    def sync(self):
        self._chk(self._L.csky_multi_sync(self._h))

    def set_host_ring(self, slots):
        self._chk(self._L.csky_multi_set_host_ring(self._h, int(slots)))

    def submit_clouds(self, params, tile_w=None, tile_h=None):
        p = cloud_params(params)
        w, h = _frame_size(p, tile_w, tile_h)
        t = C.c_int64(-1)
        self._chk(self._L.csky_multi_submit_clouds(self._h, C.byref(p), w, h, C.byref(t)))
        self._shapes = getattr(self, "_shapes", {})
        self._shapes[t.value] = (h, w)
        return t.value

    def collect(self, ticket, copy=True):
        ptr, n = C.c_void_p(), C.c_size_t()
        self._chk(self._L.csky_multi_collect(self._h, int(ticket), C.byref(ptr), C.byref(n)))
        h, w = self._shapes.pop(int(ticket))
        a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint16)), shape=(h, w, 4))
        return (a.copy() if copy else a).view(np.float16)
