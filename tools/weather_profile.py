"""The timing run of the weather-only rebind and of the weather generator (raw output: profiles/r32/weather.txt).

    python tools/weather_profile.py
One process, one context with the shipped set bound.  Every call below blocks its caller and leaves the context idle, so a pair of events on the
process's own stream around the WHOLE call spans what the call costs its host: the wait for the device, the upload, the kernels, the read-back
of the range.  The host's clock around the same call is printed beside it.  Groups of 3 warm-up and 20 measured calls, in the order

    csky_set_noise, csky_set_weather, csky_set_weather_device, csky_set_weather_generated, csky_set_noise

(the comparator first and last, so that a drifting clock shows), alternating between the shipped map and `stratus` so that no call binds what is
bound already.  Then the generator kernel alone: csky_set_kernel_timing's events around its launch inside csky_set_weather_generated."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, N = 3, 20


def main():
    sys.path.insert(0, ROOT)
    import torch

    import gvcd_amd
    large, small, weather = gvcd_amd.assets.load_default_noise()
    stratus = weather.copy(); stratus[..., 0] //= 2; stratus[..., 2] = np.minimum(stratus[..., 2], 200)
    maps = [np.ascontiguousarray(stratus), np.ascontiguousarray(weather)]
    ctx = gvcd_amd.Context(0)
    ctx.set_noise(large, small, weather)
    print("library %s" % os.path.relpath(gvcd_amd.library_path(), ROOT), flush=True)
    d_maps = [torch.from_numpy(m).cuda() for m in maps]
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(label, call):
        for k in range(WARM):
            call(k)
        ev, host = [], []
        for k in range(N):
            e0.record()
            t0 = time.perf_counter()
            call(k)
            t1 = time.perf_counter()
            e1.record()
            e1.synchronize()
            ev.append(e0.elapsed_time(e1)); host.append((t1 - t0) * 1e3)
        ev, host = np.asarray(ev), np.asarray(host)
        print("%-36s events: median %8.3f  min %8.3f  max %8.3f ms     host clock: median %8.3f ms" %
              (label, np.median(ev), ev.min(), ev.max(), np.median(host)), flush=True)
        return float(np.median(ev))

    calls = {
        "csky_set_noise": lambda k: ctx.set_noise(large, small, maps[k & 1]),
        "csky_set_weather": lambda k: ctx.set_weather(maps[k & 1]),
        "csky_set_weather_device": lambda k: ctx.set_weather(d_maps[k & 1]),
        "csky_set_weather_generated": lambda k: ctx.set_weather_generated(1 + (k & 1)),
    }
    med = {}
    for label in ("csky_set_noise", "csky_set_weather", "csky_set_weather_device", "csky_set_weather_generated"):
        med[label] = timed(label, calls[label])
    again = timed("csky_set_noise (again)", calls["csky_set_noise"])
    base = 0.5 * (med["csky_set_noise"] + again)
    print("csky_set_noise, first and last group: %.3f and %.3f ms (%.1f %% apart)" % (med["csky_set_noise"], again, 100 * abs(again - med["csky_set_noise"]) / base))
    for label in ("csky_set_weather", "csky_set_weather_device", "csky_set_weather_generated"):
        print("%-36s %.2f x cheaper than csky_set_noise (%.3f of %.3f ms)" % (label, base / med[label], med[label], base))

    ctx.set_kernel_timing(True)
    for k in range(WARM):
        calls["csky_set_weather_generated"](k)
    ctx.kernel_ms()
    for k in range(N):
        calls["csky_set_weather_generated"](k)
    ms, n = ctx.kernel_ms()
    ctx.set_kernel_timing(False)
    assert n == N, n
    print("weather_noise_kernel alone                  mean %8.4f ms over %d launches (csky_set_kernel_timing)" % (ms / n, n))
    ctx.close()


if __name__ == "__main__":
    main()
