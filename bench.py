#!/usr/bin/env python
"""bench.py -- headline benchmark of the cloud hot path on MI355X.

One "step" = one full-hemisphere frame of the reference's per-frame work: sky-view LUT refresh for the sun
(sky_lut.gd:43-52, called from cloud_sky.gd:187 once per update pass) + the per-pixel cloud march of clouds.glsl
over the whole W x H hemisphere texture (+ the RCCL gather of the bands to rank 0 when N > 1).  Inputs (noise
volumes, weather map, transmittance LUT) are resident in HBM before the timed region; the output frame stays in
HBM.  Workload = BASELINE.json configs[2] (C3): 2048x1024, 128 primary x 6 light steps, default noise + weather,
default clouds_sky.tres parameters, sun = (1,1,0)/sqrt(2), wind frozen.

N > 1: one process per GPU (torch.distributed, backend nccl = RCCL); the frame's 8-row bands are interleaved over
the ranks with no collective during the march and ONE gather to rank 0 per frame ("scaling": "strong": the frame
is fixed, each rank renders 1/N of it).  The 200x100 sky LUT is split the same way (rank r renders rows r, r+N, ... into the
tail of its band buffer; rank 0 interleaves both out of the one gather): N identical LUTs would cost every rank 33 us of a
whole chip per frame.

Two protocols, both in the line.  Round 6: `value` / `ms_per_step` ARE the protocol exactly as asked -- W warm-up steps and exactly K timed steps, run
FIRST on a GPU that has done nothing since the asset load (what rounds 1-3 reported as `value` and what the driver's own clock sees; `value_as_asked`
is kept as an alias for one round).  Then ~120 ms of the workload's own frames, untimed, bring the GPU clocks up (`config.clock_prewarm_frames`;
`--no-prewarm` leaves them out: the W warm-up steps asked for are 1-9 ms of activity for this path, too short for a GPU that idled through the imports;
a short timed region reads 2 % (N = 1) to 9 % (a 1/8 share) under the steady state), and the same W + K run again -> `value_prewarmed` /
`ms_per_step_prewarmed`, the steady-state rate of a renderer that is called every frame (rounds 4-5 reported THIS as `value`).
`config.with_early_out`: a labelled NON-headline secondary at N = 1 with the north star's wave-ballot early-out (eps = 1e-3): rate + largest error.

Consecutive frames are independent, so by default every rank keeps two frames in flight (alternating streams; EIGHT for a
rank share of a quarter frame or less, whose launches do not fill the chip): the tail of frame k's launch overlaps the head of
the following ones and, at N > 1, frame k's gather (`--frames-in-flight 1` = strictly one frame at a time).  `value` is the pipelined whole-job rate; the same K frames strictly one at a time are timed right after it and
reported next to it (`value_one_frame_at_a_time`): quote both.

`roofline`: the path is not HBM-bound (82 MB of baked inputs live in L2 / Infinity Cache) and has no contraction, so neither "hbm" nor "mfma"
bounds it; the binding unit is VALU issue, with the vector-L1 gather path close behind.  Everything is measured in this run, after the timed
region: executed instructions = basic-block execution counts of the CENSUS build of the library (the product's own assembly with a counter per
block, tools/isa_profile.py; its frame is byte-identical) x the static per-block histogram, cross-checked against the hardware totals (rocprofv3
--pmc passes in child processes, tools/pmc_collect.py).  Round 4: the TOP LEVEL is the dominant kernel ALONE at the guide's
issue rates -- achieved = (full x 2 + half x 4 + transcendental x 8) / 1024 SIMDs from `valu_issue.valu_by_class`, peak = `kernel_alone.kernel_ms`
(HIP events around single launches) x the shader clock sampled while they ran (tools/sclk.py) -- recomputable in one line; `frac_calibrated`
prices every kind with the TIME it costs in a differential micro-benchmark (profiles/r04/valu_issue_time_gfx950.json, no clock reading);
`frac_timed_region` is the persistent form's instructions over `ms_per_step` (launches overlap there: a chip-busy figure).  Nothing is read from a
committed counter file: without rocprofv3 / the census library the fields are null.  The contract's algorithmic-bytes figure is kept as
`hbm_algorithmic` with its ratio to the HBM peak (> 1); `executed_tap_bytes` next to it is what the kernel's lanes actually request
(tools/executed_tap_bytes.py: the exact rejects skip 42 % of the algorithmic bytes, the rest is served by L1 / L2 / Infinity Cache).

`value_host_form`: the same frames delivered into PINNED HOST memory through csky_submit_clouds / csky_collect (what the GDExtension's
submit_clouds() / collect() wrap), with one and two frames in flight: PCIe-inclusive, never the headline `value`.

N > 1 without a launcher around it (`python bench.py --gpus 8`): bench.py starts its own ranks.  `--single-process`: the N devices behind ONE
csky_multi handle (no torch.distributed).  `--groups G`: consecutive frames go to G groups of devices / ranks in turn (throughput workloads).

A plain run (`python bench.py --gpus 1 --steps K --warmup W`) does only what the headline needs: set-up, the W warm-up and K timed steps,
`--dump-outputs DIR` if given, and the line (`metric`, `value`, `unit`, `ms_per_step`, `higher_is_better`, `dtype`, ...).  Everything else above --
the clock pre-warm and `value_prewarmed`, `value_one_frame_at_a_time`, `value_host_form`, `config.with_early_out`, `roofline`, `cpu_baseline`,
`per_rank_share_ms`, the frame checks (`config.finite`, `gathered_frame_check`, `multi_stats`) -- runs with `--full` only; their fields are null otherwise.

`--dump-outputs DIR`: what the timed path delivered in its last timed step, as float32 .npy files (clouds.npy = the H x W x 4 RGBA16F frame;
sky_lut.npy = the 100 x 200 x 4 sky LUT where the path delivers one); a frame over 48 MB is written as a fixed, seeded sample of its rows
(clouds.npy + clouds_rows.npy, the row indices).  The inputs are fixed (shipped assets, seeded shape noise, constant push constants), so two builds
run with the same arguments can be compared array for array.

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

# Two frames in flight need their two streams on DIFFERENT hardware queues.  The HIP runtime multiplexes all streams of a process
# onto GPU_MAX_HW_QUEUES (default 4) queues, in first-use order; with torch's default stream, the library's two internal streams
# and the two frame streams, four are not enough to keep the frame streams apart (measured: no overlap at 4, overlap at 8).  Must
# be set before the HIP runtime initialises, i.e. before torch / libcloudsky are imported.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")   # (8 until round 4: a rank share keeps up to eight frames in flight now)

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {
    # name: (W, H, primary, light, sun)
    "C2": (512, 256, 64, 4, (0.0, 1.0, 0.0)),
    "C3": (2048, 1024, 128, 6, (1.0, 1.0, 0.0)),
    "C5frame": (4096, 2048, 128, 6, (1.0, 1.0, 0.0)),
    # BASELINE configs[4]: 64-frame animated sun sweep, sun = (cos th, sin th, 0), th = 2..178 degrees, sky LUT recomputed per frame
    "C5": (4096, 2048, 128, 6, "sweep"),
}
BYTES_PER_SAMPLE = 80        # weather bilinear (4 texels) + shape trilinear (8) + detail trilinear (8), RGBA8
HBM_PEAK_GBS = 8000.0        # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def default_params(w, h, sun, coverage=0.2, density=0.05):
    """clouds_sky.tres:11-17 packed like cloud_sky.gd:251-289 with the wind frozen."""
    s = np.asarray(sun, np.float64)
    s = (s / np.linalg.norm(s)).astype(np.float32)
    return np.array([w, h, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.270588, 0.188235, 0.027451, 1.0, s[0], s[1], s[2], 1.0, 1.0, 1.0,
                     1.0, 0.0, 0.0, density, coverage, 0.0], np.float32), s


def usable_cores():
    """Host cores this process may actually use: the affinity mask capped by the cgroup CPU quota (the GPU box shows 256 logical
    CPUs but a cpu.max of 16 CPUs; running 128 OpenMP threads there only adds scheduling overhead and misreports `cores`)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // per))
        except (OSError, ValueError):
            pass
    return n


def cpu_baseline(large, small, weather, params, sun, W, H, primary, light, every=4):
    """Time the CPU oracle (kind "port": a scalar fp32 restatement of the GLSL, oracle/cloudsky_oracle.c) on a
    bounded sample of the SAME frame: every `every`-th 8-row band, all columns (evenly spread over elevation), on all
    usable host cores (affinity capped by the cgroup CPU quota) via OpenMP over (row, 64-column chunk) items.  Reported baseline only, never the optimisation target."""
    from oracle import oracle as O

    cores = max(1, min(O.max_threads(), usable_cores()))
    tex = O.OracleTextures(large, small, weather)
    tr = O.transmittance_lut(256, 64)
    sk = O.sky_lut(sun, tr, 200, 100)
    nb = (H // 8 + every - 1) // every
    O.clouds_bands(tex, params, sk, W, (8, 0, every * 4, max(1, nb // 4)), primary, light, nthreads=cores)   # warm up threads/caches
    t0 = time.perf_counter()
    _, st = O.clouds_bands(tex, params, sk, W, (8, 0, every, nb), primary, light, nthreads=cores)
    dt = time.perf_counter() - t0
    rays = nb * 8 * W
    # SURVEY 8(d) also asks for the single-thread rate: a smaller sample (every 16th band, the first quarter of the columns)
    nb1, w1 = max(1, (H // 8 + 15) // 16), max(8, W // 4)
    t0 = time.perf_counter()
    O.clouds_bands(tex, params, sk, w1, (8, 0, 16, nb1), primary, light, nthreads=1)
    dt1 = time.perf_counter() - t0
    return {"value": rays / dt / 1e6, "unit": "Mrays/s", "cores": cores, "kind": "port",
            "sample": "every %dth 8-row band of the %dx%d frame (%d rays, %.2f s wall, %.0f core-seconds), oracle/cloudsky_oracle.c "
                      "gcc -O2 fp32, OpenMP %d threads" % (every, W, H, rays, dt, dt * cores, cores),
            "single_thread": {"value": nb1 * 8 * w1 / dt1 / 1e6, "unit": "Mrays/s", "cores": 1,
                              "sample": "every 16th 8-row band, columns 0..%d (%d rays, %.2f s)" % (w1 - 1, nb1 * 8 * w1, dt1)}}


DUMP_FRAME_LIMIT = 48 << 20   # --dump-outputs: a float32 frame above this is sampled by rows (everything written stays under 64 MB)


def dump_outputs(out_dir, frame, sky_lut=None):
    """--dump-outputs: the last timed step's frame (int16 tensor holding RGBA16F, H x W x 4) and sky LUT (the same as a tensor, or the float16
    array of read_sky_lut; None where the path delivers none) as float32 .npy files.  A frame over DUMP_FRAME_LIMIT keeps a fixed, seeded
    sample of its rows, whose indices go to clouds_rows.npy."""
    def f32(x):
        if not isinstance(x, np.ndarray):
            x = x.cpu().numpy().view(np.float16)
        return x.astype(np.float32)

    os.makedirs(out_dir, exist_ok=True)
    fr = f32(frame)
    if fr.nbytes > DUMP_FRAME_LIMIT:
        rows = np.sort(np.random.default_rng(0).choice(fr.shape[0], DUMP_FRAME_LIMIT // fr[0].nbytes, replace=False))
        fr = fr[rows]
        np.save(os.path.join(out_dir, "clouds_rows.npy"), rows.astype(np.float64))
    np.save(os.path.join(out_dir, "clouds.npy"), fr)
    if sky_lut is not None:
        np.save(os.path.join(out_dir, "sky_lut.npy"), f32(sky_lut))


def free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def self_launch(n):
    """`python bench.py --gpus N` without a launcher around it: start the N ranks ourselves (one process per GPU, torch.distributed.run on
    127.0.0.1) with the same arguments and pass rank 0's JSON line through.  The driver's own `python -m torch.distributed.run ... bench.py`
    command sets WORLD_SIZE and never comes here."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    r = subprocess.run(cmd, env=env)
    raise SystemExit(r.returncode)


def main_single_process(args):
    """N devices behind ONE handle (csky_multi_*, include/cloudsky.h): the same step (sky LUT + march of every device's bands into the frame on
    device 0) timed by the same loop; `frames in flight` consumer streams rotate per frame group.  CSKY_BENCH_ONE_GPU_DEBUG=1 puts all N contexts
    on device 0 (exercises the path on a one-GPU box; its number is meaningless)."""
    import torch

    import gvcd_amd

    if not torch.cuda.is_available():
        raise SystemExit("bench.py: no GPU visible; the cloud path has no CPU fallback")
    debug_one_gpu = os.environ.get("CSKY_BENCH_ONE_GPU_DEBUG") == "1"
    n = args.gpus
    if not debug_one_gpu and torch.cuda.device_count() < n:
        raise SystemExit("bench.py --single-process: %d devices requested, %d visible" % (n, torch.cuda.device_count()))
    G = args.groups
    if G < 1 or n % G:
        raise SystemExit("bench.py: --groups must divide --gpus")
    W, H, primary, light, sun = CONFIGS[args.config]
    sweep = None
    if isinstance(sun, str):
        th = np.radians(np.linspace(2.0, 178.0, 64))
        sweep = [default_params(W, H, (np.cos(t), np.sin(t), 0.0)) for t in th]
        sun = (np.cos(th[16]), np.sin(th[16]), 0.0)
    params, sun_n = default_params(W, H, sun)
    large, small, weather = gvcd_amd.assets.load_default_noise()
    ids = [0] * n if debug_one_gpu else list(range(n))
    m = gvcd_amd.MultiContext(ids)
    m.set_noise(large, small, weather)
    m.set_march(primary, light)
    for i in range(n):
        c = m.ctx(i)
        if c.noise_inexact_coeffs() != 0:
            raise SystemExit("bench.py: the benchmark textures must bake exactly")
        c.set_early_out(args.early_out)
        c.render_transmittance(256, 64)
    per = n // G
    tiles_per_dev = ((W + 7) // 8) * ((H // 8 + per - 1) // per)
    fif_default = max(2, 8 // G) if (per > 1 and 3072 <= tiles_per_dev < 12288) else 2    # (frames in flight x groups <= 8 behind one handle)
    fif = max(1, min(8 // G, args.frames_in_flight if args.frames_in_flight is not None else fif_default))
    m.set_groups(G)
    m.set_frames_in_flight(fif)
    if args.staged:
        m.set_staged(True)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    slots = fif * G
    streams = [torch.cuda.Stream(device=dev) for _ in range(slots)]
    frames = [torch.zeros((H, W, 4), dtype=torch.int16, device=dev) for _ in range(slots)]
    counter = [0]

    def step():
        k = counter[0]
        counter[0] += 1
        fp, fs = (params, sun_n) if sweep is None else sweep[k % len(sweep)]
        b = k % slots
        m.render_sky_lut(fs, 200, 100)                                                            # sky_lut.gd:122-148 (on the devices of this frame's group)
        m.render_clouds_device(fp, W, H, frames[b].data_ptr(), W * 8, streams[b].cuda_stream)     # cloud_sky.gd:234-248, every device of the group

    def sync_all():
        m.sync()
        for i in range(1 if debug_one_gpu else n):
            torch.cuda.synchronize(i)

    def region():
        for _ in range(max(args.warmup, slots)):
            step()
        sync_all()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        sync_all()
        e = time.perf_counter() - t0
        n_run = counter[0]
        counter[0] = 0
        return e, n_run

    # both protocols, as in the process-per-GPU form below: `value` = as asked (run first, cold); then the clock pre-warm and the same region again -> `value_prewarmed`
    elapsed, n_last = region()
    if args.dump_outputs:                                                 # the frame of the last timed step and the LUT its devices rendered (read through device 0)
        dump_outputs(args.dump_outputs, frames[(n_last - 1) % slots], m.ctx(0).read_sky_lut())
    prewarmed = None
    prewarm_frames = 0
    if args.full and not args.no_prewarm:
        est_ms = 1.7 * tiles_per_dev / 32768.0 * primary / 128.0
        prewarm_frames = int(min(1024, max(16, np.ceil(120.0 / max(est_ms, 1e-3))))) * G
        for _ in range(prewarm_frames):
            step()
        sync_all()
        counter[0] = 0
        e_warm, n_last = region()
        prewarmed = {"value": W * H * args.steps / e_warm / 1e6, "ms_per_step": e_warm / args.steps * 1e3}
    as_asked = {"value": W * H * args.steps / elapsed / 1e6, "ms_per_step": elapsed / args.steps * 1e3}
    # every device's share alone (one launch at a time on that device): what bounds the split
    share_ms = [] if args.full else None
    for i in range(n if args.full else 0):
        k = i % per
        total = H // 8
        nb = (total - k + per - 1) // per
        ms, _ = m.ctx(i).time_clouds(params, W, (8, k, per, nb), warmup=1, iters=3)
        share_ms.append(ms)
    fr = frames[(n_last - 1) % slots].view(torch.float16)               # the last frame the last region rendered (region() returns how many it ran)
    multi_stats = alpha_mean = finite = frame_check = None
    if args.full:
        # the handle's preconditions (peer access of every device to the first) and, outside the timed regions, HIP-event timings of one more frame:
        # every device's march of its bands and (staged form) its peer copy -- csky_multi_get_stats
        sync_all()
        m.set_timing(True)
        fp_t, fs_t = (params, sun_n) if sweep is None else sweep[0]
        m.render_sky_lut(fs_t, 200, 100)
        scratch = torch.zeros((H, W, 4), dtype=torch.int16, device=dev)
        m.render_clouds_device(fp_t, W, H, scratch.data_ptr(), W * 8, streams[0].cuda_stream)
        multi_stats = m.stats()
        multi_stats["warning"] = m.last_warning()
        m.set_timing(False)
        alpha_mean = float(fr[..., 3].float().mean().item())
        finite = bool(torch.isfinite(fr.float()).all().item())
    if args.full:                                                         # the assembled frame must equal a single-context render of the same frame (outside the timed region)
        c0 = m.ctx(0)
        full = torch.zeros((H, W, 4), dtype=torch.int16, device=dev)
        k_last = n_last - 1
        fp, fs = (params, sun_n) if sweep is None else sweep[k_last % len(sweep)]
        c0.set_segments(1); c0.set_frames_in_flight(1)
        c0.render_sky_lut_device(fs, 200, 100, streams[0].cuda_stream)
        c0.render_clouds_device(fp, W, (H, 0, 1, 1), full.data_ptr(), W * 8, streams[0].cuda_stream)
        torch.cuda.synchronize(0)
        a, b = full.view(torch.float16).float(), fr.float()
        err = (a - b).abs()
        ok = float((err <= 5e-4 + 2e-3 * a.abs()).float().mean().item())
        frame_check = {"max_abs_diff": float(err.max().item()), "within_1_fp16_ulp_frac": ok, "bit_identical_frac": float((full == fr.view(torch.int16)).float().mean().item()),
                       "what": "the last frame of the run (assembled on device 0 by peer stores) vs the same frame rendered whole by context 0"}
        print("check: %d-device frame vs single-context frame: max|d| = %.3g, within 1 fp16 ulp-ish: %.6f" % (n, frame_check["max_abs_diff"], ok), file=sys.stderr, flush=True)
        if ok < 0.9999:
            raise SystemExit("bench.py: multi-device frame differs from the single-context frame")
    out = {
        "metric": "Mrays/s + hemisphere fps, 2048x1024 @ 128x6 steps, 1/2/4/8 MI355X",
        "value": W * H * args.steps / elapsed / 1e6, "unit": "Mrays/s", "hemisphere_fps": args.steps / elapsed,
        "n_gpus": n, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
        "protocol": "as asked: W warm-up + K timed steps, run first (cold); the clock-pre-warmed figure is value_prewarmed",
        "value_prewarmed": (prewarmed or as_asked)["value"], "ms_per_step_prewarmed": (prewarmed or as_asked)["ms_per_step"],
        "value_as_asked": as_asked["value"], "ms_per_step_as_asked": as_asked["ms_per_step"],
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "ranks_seen": len(m), "per_rank_share_ms": share_ms, "gathered_frame_check": frame_check, "multi_stats": multi_stats,
        "config": {"workload": "%s: %dx%d hemisphere, %d primary x %d light steps, sun (%.4f,%.4f,%.4f), clouds_sky.tres defaults, weather.bmp + worlnoise.bmp "
                               "+ generated 128^3 shape noise (seed 1), wind frozen" % (args.config, W, H, primary, light, sun_n[0], sun_n[1], sun_n[2]),
                   "texture_size": [W, H], "primary_steps": primary, "light_steps": light, "early_out_eps": args.early_out,
                   "parallelism": "single-process csky_multi: %d group(s) x %d-way bands, %s" % (G, per, "staged peer copies" if args.staged else "in-place xGMI peer stores"),
                   "frames_in_flight": fif, "frame_groups": G, "clock_prewarm_frames": prewarm_frames, "device_ids": ids, "alpha_mean": alpha_mean, "finite": finite},
        "roofline": None, "note": "roofline and cpu_baseline are reported by the N = 1 run with --full (same kernel); this line times the multi-device step only",
    }
    print(json.dumps(out), flush=True)
    m.close()


def valu_roofline(census, clocks, pmc, vi, k_solo_ms, ms_per_step):
    """The VALU-issue roofline from the instruction census and the sampled clocks (see the `roofline.note` of the JSON line).

    Top level = the dominant kernel ALONE at the guide's issue rates:
        achieved = (full x 2 + half x 4 + transcendental x 8) / 1024 SIMDs        executed wave64 VALU instructions by class (census)
        peak     = kernel_ms (HIP events around one launch with the GPU to itself) x the shader clock sampled while those launches ran
        frac     = achieved / peak
    `frac_calibrated`: the same launch priced with the TIME each instruction kind costs (differential micro-benchmark, ns per instruction,
    profiles/r04/valu_issue_time_gfx950.json) over kernel_ms: no clock reading in it.  `frac_timed_region` (+ `_calibrated`): the persistent form's
    instructions over ms_per_step, the effective per-frame time of the timed region where two launches overlap."""
    out = {"achieved": None, "peak": None, "frac": None, "frac_calibrated": None, "frac_timed_region": None, "frac_timed_region_calibrated": None,
           "kernel_alone": None, "timed_region": None, "valu_issue": None, "clocks": clocks}
    if not census:
        return out
    kp = census["kernels"].get("plain") or {}
    kq = census["kernels"].get("persistent") or {}
    mix = census.get("mixed_stream_factor") or {}
    out["valu_issue"] = {"source": "census", "guide_cycles_per_class": census.get("guide_cycles_per_class"), "time_calibration": census.get("time_calibration"),
                         "round3_calibration": census.get("calibration"), "mixed_stream_factor": mix,
                         "executed": kp.get("executed"), "valu_by_class": kp.get("valu_by_class"),
                         "issue_cycles_guide_per_simd": kp.get("valu_issue_cycles_guide_per_simd"), "issue_time_ms_per_simd": kp.get("valu_issue_time_ms_per_simd"),
                         "issue_cycles_round3_calibration_per_simd": kp.get("valu_issue_cycles_per_simd"),
                         "persistent_form": {"valu_by_class": kq.get("valu_by_class"), "issue_cycles_guide_per_simd": kq.get("valu_issue_cycles_guide_per_simd"),
                                             "issue_time_ms_per_simd": kq.get("valu_issue_time_ms_per_simd")},
                         "priced_by_measured_kind_fraction": kp.get("valu_priced_by_measured_kind_fraction"),
                         "frame_identical_to_product": kp.get("frame_identical_to_product"),
                         "scratch_instructions_per_wavefront": {"plain": kp.get("scratch_instructions_per_wavefront"), "persistent": kq.get("scratch_instructions_per_wavefront")},
                         "top_kinds": (kp.get("top_kinds") or [])[:12]}
    cnt = ((pmc or {}).get("counters_per_launch") or {})
    ins = cnt.get("insts") or cnt.get("valu") or {}
    if ins and kp.get("executed"):
        ex = kp["executed"]
        pairs = {"valu": "SQ_INSTS_VALU", "salu": "SQ_INSTS_SALU", "smem": "SQ_INSTS_SMEM", "vmem_load": "SQ_INSTS_VMEM_RD", "lds": "SQ_INSTS_LDS"}
        out["valu_issue"]["census_over_hardware_counters"] = {k: (ex[k] / ins[c] if ins.get(c) else None) for k, c in pairs.items()}
    ck = (clocks or {}).get("kernel_alone") or {}
    nominal = (clocks or {}).get("nominal_mhz")          # no hwmon node readable: the device's maximum clock (fractions come out LOW, never above 1 by that)
    mhz = (ck.get("sclk") or {}).get("mean_mhz") or nominal
    ach, ach_ms = kp.get("valu_issue_cycles_guide_per_simd"), kp.get("valu_issue_time_ms_per_simd")
    if ach and mhz:
        k_ms = ck.get("kernel_ms") or k_solo_ms
        peak = k_ms * 1e-3 * mhz * 1e6
        out["kernel_alone"] = {"kernel": "clouds_kernel<3,1>", "kernel_ms": k_ms, "sclk_mhz": mhz, "achieved": ach, "peak": peak, "frac": ach / peak,
                               "frac_calibrated": (ach_ms / k_ms) if ach_ms else None,
                               "recompute": "(full x 2 + half x 4 + trans x 8) / 1024 / (kernel_ms x 1e-3 x sclk_mhz x 1e6) with valu_issue.valu_by_class"}
        out.update({"achieved": ach, "peak": peak, "frac": ach / peak, "frac_calibrated": out["kernel_alone"]["frac_calibrated"],
                    "peak_source": "kernel alone: %.4f ms (HIP events around single launches) x %.0f MHz sampled while they ran" % (k_ms, mhz)})
    ch = (clocks or {}).get("headline") or {}
    mhz_h = (ch.get("sclk") or {}).get("mean_mhz") or nominal
    achq, achq_ms = kq.get("valu_issue_cycles_guide_per_simd") or ach, kq.get("valu_issue_time_ms_per_simd") or ach_ms
    if achq and mhz_h:
        peak_h = ms_per_step * 1e-3 * mhz_h * 1e6
        out["timed_region"] = {"kernel": "clouds_kernel_persistent<3>, two launches overlapping", "ms_per_step": ms_per_step, "sclk_mhz": mhz_h, "achieved": achq, "peak": peak_h,
                               "frac": achq / peak_h, "frac_calibrated": (achq_ms / ms_per_step) if achq_ms else None, "ms_per_frame_while_sampling": ch.get("ms_per_frame")}
        out["frac_timed_region"] = achq / peak_h
        out["frac_timed_region_calibrated"] = out["timed_region"]["frac_calibrated"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)   # the pipeline fills and drains once per timed region: ~0.4 ms, 0.1 % of 200 steps
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", default="C3", choices=sorted(CONFIGS))
    ap.add_argument("--variant", type=int, default=None)
    ap.add_argument("--early-out", type=float, default=0.0, help="wave early-out threshold on transmittance (0 = reference behaviour)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--also-early-out", action="store_true", help="(accepted, no effect: since round 6 the early-out secondary is part of every N = 1 line)")
    ap.add_argument("--no-early-out-leg", action="store_true", help="skip the labelled non-headline early-out measurement (config.with_early_out)")
    ap.add_argument("--kernel-iters", type=int, default=1, help="solo (one launch in flight) cloud-kernel launches timed after the timed region")
    ap.add_argument("--no-pmc", action="store_true", help="skip the live rocprofv3 counter passes (roofline fractions become null)")
    ap.add_argument("--no-host-form", action="store_true", help="skip the value_host_form leg (frames delivered to pinned host memory): for profiling the timed region alone")
    ap.add_argument("--frames-in-flight", type=int, default=None,
                    help="consecutive frames rotate over this many streams per rank, 1..8 (default 2: the tail of frame k overlaps the head of "
                         "frame k+1 and, at N > 1, its gather; 8 for rank shares of 3072..12287 tiles; 1 = strictly one frame at a time)")
    ap.add_argument("--single-process", action="store_true",
                    help="N > 1 behind the C ABI: ONE process, one host thread, csky_multi_* over the N devices (every device stores its bands straight "
                         "into the frame on device 0 over xGMI; no torch.distributed, no RCCL): the form a GDExtension host can use")
    ap.add_argument("--groups", type=int, default=1,
                    help="frame groups for throughput workloads (single-process form): consecutive frames go to G groups of N/G devices in turn, each "
                         "group splits its frame (N/G)-way; 1 = every device works on every frame (the C4 split)")
    ap.add_argument("--no-prewarm", action="store_true", help="skip the ~120 ms of untimed frames at the end of the set-up that bring the GPU clocks up (see config.clock_prewarm_frames)")
    ap.add_argument("--whole-lut", action="store_true", help="N > 1: every rank renders the whole sky LUT (rounds 1-3) instead of its rows of it")
    ap.add_argument("--staged", action="store_true", help="single-process form: local band buffers + strided peer copies instead of in-place peer stores")
    ap.add_argument("--shape-noise", default="", help="NOT the benchmark workload: knobs of the stand-in shape generator as key=value,... (csky_shape_noise_params: perlin_freq, "
                                                        "perlin_octaves, worley_freq, perlin_gain, dilate, centre, contrast, offset), to see what the missing asset's character does to "
                                                        "the frame time (config.workload says so; roofline census / executed_tap_bytes then describe another frame than the pinned one)")
    ap.add_argument("--coverage", type=float, default=0.2, help="cloud_coverage of the push-constant block (0.2 = clouds_sky.tres = the benchmark workload)")
    ap.add_argument("--full", action="store_true", help="also run every secondary measurement and check (pre-warmed rerun, one frame at a time, host form, "
                                                         "early-out leg, roofline, CPU baseline, frame checks); a plain run times the steps only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step delivered to DIR/<name>.npy (float32)")
    args = ap.parse_args()

    if args.gpus > 1 and not args.single_process and "WORLD_SIZE" not in os.environ:
        return self_launch(args.gpus)
    if args.single_process:
        return main_single_process(args)

    import torch

    import gvcd_amd
    from gvcd_amd import tiling

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (launch N>1 with torch.distributed.run)" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py: no GPU visible; the cloud path has no CPU fallback")
    # CSKY_BENCH_ONE_GPU_DEBUG=1: every rank renders on cuda:0 and the gather goes through gloo on host copies.  It exists
    # only to exercise the N > 1 code path (band split, gather, interleave) on a single-GPU box; its number is meaningless.
    debug_one_gpu = os.environ.get("CSKY_BENCH_ONE_GPU_DEBUG") == "1"
    if debug_one_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if debug_one_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        # The unattended SCALE run must not print a plausible line from a broken launch: every rank checks that the communicator
        # has the size asked for and that no two ranks sit on the same device; any rank that sees otherwise exits non-zero BEFORE anything is timed
        # (all ranks see the same gathered list, so all of them exit: no JSON line, non-zero return code).
        if dist.get_world_size() != args.gpus:
            raise SystemExit("bench.py: --gpus %d but the process group has %d ranks" % (args.gpus, dist.get_world_size()))
        if not debug_one_gpu or os.environ.get("CSKY_BENCH_FAKE_SHARED_DEVICE") == "1":
            import socket
            pr = torch.cuda.get_device_properties(local_rank)
            # the PHYSICAL identity: PCI domain:bus:device (plain ints in torch's device properties; a device index would be 0 on every rank under a launcher
            # that narrows each rank's visibility to one GPU, and the `uuid` property is an opaque object whose text is not portable); no PCI fields: the index
            if isinstance(getattr(pr, "pci_bus_id", None), int):
                ident = "%s|pci %04x:%02x:%02x" % (socket.gethostname(), getattr(pr, "pci_domain_id", 0) or 0, pr.pci_bus_id, getattr(pr, "pci_device_id", 0) or 0)
            else:
                ident = "%s|device index %d" % (socket.gethostname(), local_rank)
            idents = [None] * world
            dist.all_gather_object(idents, ident)
            if len(set(idents)) != world:
                raise SystemExit("bench.py: %d ranks but only %d distinct devices (%s): one process per GPU is the contract (LOCAL_RANK must select the device)"
                                 % (world, len(set(idents)), ", ".join(sorted(set(idents)))))

    W, H, primary, light, sun = CONFIGS[args.config]
    sweep = None
    if isinstance(sun, str):
        th = np.radians(np.linspace(2.0, 178.0, 64))
        sweep = [default_params(W, H, (np.cos(t), np.sin(t), 0.0)) for t in th]      # one push-constant block + sun per frame
        sun = (np.cos(th[16]), np.sin(th[16]), 0.0)                                    # representative frame for the kernel-only timing
    params, sun_n = default_params(W, H, sun, coverage=args.coverage)
    if sweep is not None and args.coverage != 0.2:
        sweep = [default_params(W, H, (np.cos(t), np.sin(t), 0.0), coverage=args.coverage) for t in th]
    large, small, weather = gvcd_amd.assets.load_default_noise()
    knobs = {}
    if args.shape_noise:
        for kv in args.shape_noise.split(","):
            k, v = kv.split("=")
            knobs[k.strip()] = int(v) if k.strip() in ("perlin_freq", "perlin_octaves", "worley_freq") else float(v)
        large = gvcd_amd.assets.generate_shape_noise(gvcd_amd.assets.SHAPE_SEED, 128, **knobs)
    off_workload = bool(knobs) or args.coverage != 0.2

    ctx = gvcd_amd.Context(local_rank)
    ctx.set_noise(large, small, weather)            # inputs -> HBM (mip chains + device layouts baked on the GPU, once)
    if ctx.noise_inexact_coeffs() != 0 and not off_workload:      # (an off-workload volume that does not fit fp16 pairs marches on exact fp32 cells: another kernel instantiation, config says so)
        raise SystemExit("bench.py: the benchmark textures must bake exactly (fp16 finite differences)")
    ctx.set_march(primary, light)
    ctx.set_early_out(args.early_out)
    if args.variant is not None:
        ctx.set_variant(args.variant)
    ctx.render_transmittance(256, 64)               # once at load, transmittance_lut.gd:15-18

    # Frames are independent and a launch ends in a tail of few, long wavefronts; with two frames in flight on two streams the next
    # frame's workgroups fill that tail (the library keeps per-frame state in eight-deep rings ordered by events).  Measured on one
    # GPU: whole frame 2.19 -> 1.90 ms; one rank's 1/2, 1/4, 1/8 share 1.09 -> 0.96, 0.67 -> 0.52, 0.43 -> 0.34 ms per frame
    # (tools/share_matrix.py).  Buffer set b = frame number mod frames in flight: band buffer, stream, gather target.
    # The rings are eight deep; more than two frames in flight only pay for small rank shares (a 1/8 share of C3: 0.31 -> 0.25 -> 0.22 ms per
    # frame as whole rays with 2 -> 4 -> 8), so the default is 8 for 3072..12287 tiles per rank at N > 1 and 2 everywhere else.
    # Frame groups (--groups G, throughput workloads such as C5's 64-frame sweep): the ranks are split into G groups of world / G; consecutive
    # frames go to the groups in turn and the ranks of a group split THEIR frame's bands (world / G)-way.  A rank's share is G times larger
    # (fewer, fuller launches), every frame is still gathered on rank 0: group g's collective runs on a communicator of {0} + its ranks, to
    # which rank 0 contributes an unused dummy when it is not a member.  G = 1 (default): every rank works on every frame (the C4 split).
    G = max(1, args.groups)
    if world % G:
        raise SystemExit("bench.py: --groups must divide --gpus")
    fg = tiling.FrameGroups(rank, world, G, dist)     # (creates the per-group communicators: a collective)
    per = fg.per
    bands = fg.bands(H)
    tiles_per_rank = ((W + 7) // 8) * bands[3]
    # measured per frame (round 4, rings eight deep, 16 hardware queues; profiles/r04/frames_in_flight_depth.txt), x2 / x4 / x8:
    # 1/2 share 0.82 / 0.82 / 0.82, 1/4 share 0.487 / 0.446 / 0.415, 1/8 share 0.31 / 0.247 / 0.224 (round 3, x2 / x4: 1/16 share 0.191 / 0.250)
    fif_default = 8 if (per > 1 and 3072 <= tiles_per_rank < 12288) else 2
    fif = max(1, min(8, args.frames_in_flight if args.frames_in_flight is not None else fif_default))
    if os.environ.get("CSKY_BENCH_SYNC_GATHER") == "1":
        fif = 1                                      # debugging aid: gather-then-render, one frame at a time
    ctx.set_frames_in_flight(fif)
    # rank 0 takes part in every frame's gather (G x fif in flight), the others in their group's frames only
    nbuf = fif * G if (rank == 0 and G > 1) else fif
    streams = [torch.cuda.Stream(device=dev) for _ in range(nbuf)]   # always real streams: handle 0 (torch's default stream) would select the
    stream = streams[0].cuda_stream                                  # library's own non-blocking stream, unordered against the gather
    mb = fg.max_bands(H)
    # N > 1: the gather of frame k (RCCL, its own stream, ordered behind the stream of frame k at the call) overlaps the march of
    # the following frames on the other streams; wait() orders frame k's stream behind its collective before that buffer set is reused.
    overlap = world > 1 and nbuf > 1
    # N > 1: each rank renders rows index::per of the 200 x 100 sky LUT instead of all of it (csky_render_sky_lut_rows_device: the LUT costs 33 us
    # of a whole chip, 12 % of a 1/8 frame share) and its rows ride behind its bands in the same gather; rank 0 interleaves both.
    # --whole-lut: every rank renders the whole LUT as rounds 1-3 did (A/B).
    LW, LH = 200, 100
    split_lut = per > 1 and not args.whole_lut
    band_bytes = mb * tiling.BAND_ROWS * W * 8
    lut_bytes = fg.max_lut_rows(LH) * LW * 8 if split_lut else 0
    local_b = [torch.zeros(band_bytes + lut_bytes, dtype=torch.uint8, device=dev) for _ in range(nbuf)]   # collectives move raw bytes (RCCL has no int16 type)
    local = [t[:band_bytes].view(torch.int16).view(mb * tiling.BAND_ROWS, W, 4) for t in local_b]
    lut_rows = fg.lut_rows(LH)
    gdev = "cpu" if debug_one_gpu else dev
    gathered = [torch.empty((fg.max_members, band_bytes + lut_bytes), dtype=torch.uint8, device=gdev) for _ in range(nbuf)] if (world > 1 and rank == 0) else [None] * nbuf
    sky_lut = [None]
    # rank 0's delivered textures, one per buffer set: the interleave of the gathered bands / LUT rows writes into them (csky_interleave_bands_device)
    frame_out = [torch.zeros((H, W, 4), dtype=torch.int16, device=dev) for _ in range(nbuf)] if (world > 1 and rank == 0) else []
    lut_out = [torch.zeros((LH, LW, 4), dtype=torch.int16, device=dev) for _ in range(nbuf)] if (world > 1 and rank == 0 and split_lut) else []
    staged_g = [None] * nbuf
    pending = [None] * nbuf
    pend_frame = [0] * nbuf
    frame = [None]
    frame_k = [0]                                    # index of the frame `frame[0]` holds (the checks below read this, not the step counter)
    counter = [0]
    taken = [0]                                      # frames this rank took part in: its buffer-set rotation

    def finish(o):
        """Frame in buffer set o has been gathered: order ITS stream behind the collective and assemble the frame on rank 0."""
        with torch.cuda.stream(streams[o]):
            pending[o].wait()
            pending[o] = None
            if rank == 0:
                staged_g[o] = gathered[o].to(dev) if debug_one_gpu else gathered[o]      # (kept alive until the buffer set comes round again)
                fg.assemble_device(pend_frame[o], staged_g[o], ctx, streams[o].cuda_stream, H, W, frame_out[o], LH if split_lut else 0, LW, lut_out[o] if split_lut else None)
                frame[0] = frame_out[o]
                frame_k[0] = pend_frame[o]
                if split_lut:
                    sky_lut[0] = lut_out[o]

    def step():
        k = counter[0]
        counter[0] += 1
        if not fg.takes_part(k):
            return
        bset = taken[0] % nbuf
        taken[0] += 1
        fp, fs = (params, sun_n) if sweep is None else sweep[k % len(sweep)]
        st_k = streams[bset].cuda_stream
        if fg.renders(k):
            if split_lut:                                                                          # sky_lut.gd:122-148, this rank's rows, behind its bands
                ctx.render_sky_lut_rows_device(fs, lut_rows[0], lut_rows[1], local_b[bset].data_ptr() + band_bytes, lut_bytes, LW, LH, st_k)
            else:
                ctx.render_sky_lut_device(fs, LW, LH, st_k)                                        # sky_lut.gd:122-148
            ctx.render_clouds_device(fp, W, bands, local[bset].data_ptr(), W * 8, st_k)           # cloud_sky.gd:234-248
        if world == 1:
            frame[0] = local[bset]
            frame_k[0] = k
            return
        with torch.cuda.stream(streams[bset]):       # the collective is ordered behind the CURRENT stream: make it this frame's
            src = local_b[bset].cpu() if debug_one_gpu else local_b[bset]
            pending[bset] = fg.gather(k, src, gathered[bset], async_op=True)
            pend_frame[bset] = k
        if overlap:
            o = (bset + 1) % nbuf          # the oldest frame in flight (its buffer set is the next one to be reused):
            if pending[o] is not None:     # its gather ran while the younger frames were marching
                finish(o)
        else:
            finish(bset)

    def drain():
        for i in range(1, nbuf + 1):       # oldest first
            o = (taken[0] - 1 + i) % nbuf
            if pending[o] is not None:
                finish(o)

    # Clock pre-warm (part of the set-up, disclosed in config.clock_prewarm_frames; --no-prewarm leaves it out): a frame of this path is 0.2-1.7 ms, so
    # the W warm-up steps the caller asks for (the driver: 5) are 1-9 ms of GPU activity, and a GPU that sat idle through the imports and the asset
    # load needs ~20 ms of work before its clocks are up: measured on one box, `--steps 20 --warmup 5` reads 1.714 ms per frame, `--warmup 80` 1.676
    # (a 1/8 rank share, whose whole 20-step region lasts 5 ms: 0.245 cold against 0.224).  The throughput of a renderer is its steady state, so the
    # set-up ends with ~120 ms of the workload's own frames (the same number on every rank: a deterministic estimate, not a clock reading), then the
    # W warm-up steps and the K timed steps run exactly as asked.
    def region():
        """W warm-up steps, then exactly K timed steps between barrier + synchronize on both sides; the maximum over the ranks."""
        for _ in range(args.warmup):
            step()
        drain()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        ctx.set_kernel_timing(True)                  # HIP event pairs around every cloud-kernel launch of the timed region, on its stream
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        drain()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        e = time.perf_counter() - t0
        kt, kl = ctx.kernel_ms()
        ctx.set_kernel_timing(False)
        if world > 1:
            t = torch.tensor([e], dtype=torch.float64, device="cpu" if debug_one_gpu else dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            e = float(t.item())
        counter[0] = 0; taken[0] = 0                 # every region sees the same frame sequence
        return e, kt, kl

    # Both protocols in one line.  Round 6: `value` / `ms_per_step` ARE the caller's W warm-up + K timed steps exactly as asked, run
    # FIRST on a GPU that has done nothing since the asset load (rounds 1-3 and the driver's own clock measure this); THEN ~120 ms of untimed frames bring
    # the clocks up and the same W + K run again -> `value_prewarmed` / `ms_per_step_prewarmed` (what rounds 4-5 called `value`).  `value_as_asked` stays
    # as an alias of `value` for one round so that r05 and r06 records compare key by key.  --no-prewarm: one region, the two are the same number.
    elapsed, k_total, k_launches = region()
    if args.dump_outputs and rank == 0:              # what the last timed step delivered, before anything else renders into the buffer sets
        dump_outputs(args.dump_outputs, frame[0], ctx.read_sky_lut() if world == 1 else (sky_lut[0] if split_lut else None))
    prewarmed = None
    prewarm_frames = 0
    if args.full and not args.no_prewarm:
        est_ms = 1.7 * (((W + 7) // 8) * mb) / 32768.0 * primary / 128.0       # from the LARGEST rank share: every rank must run the same number of frames (collectives)
        prewarm_frames = int(min(1024, max(16, np.ceil(120.0 / max(est_ms, 1e-3))))) * G
        for _ in range(prewarm_frames):
            step()
        drain()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        counter[0] = 0; taken[0] = 0                 # the warm-up and the timed region see the same frame sequence as without the pre-warm
        e_warm, kt_w, kl_w = region()
        prewarmed = {"value": W * H * args.steps / e_warm / 1e6, "ms_per_step": e_warm / args.steps * 1e3, "hemisphere_fps": args.steps / e_warm,
                     "kernel_ms_in_flight": kt_w / max(1, kl_w),
                     "what": "the same %d warm-up + %d timed steps run AGAIN after %d untimed frames (~120 ms) that bring the GPU clocks up: the steady state of a "
                             "renderer that is called every frame; rounds 4-5 reported this as `value`" % (args.warmup, args.steps, prewarm_frames)}
    as_asked = {"value": W * H * args.steps / elapsed / 1e6, "ms_per_step": elapsed / args.steps * 1e3, "hemisphere_fps": args.steps / elapsed,
                "what": "alias of value / ms_per_step (round 6: the headline IS the protocol as asked): %d warm-up + %d timed steps run first, before any clock pre-warm"
                        % (args.warmup, args.steps)}

    # dominant kernel (clouds_kernel): with two frames in flight a launch shares the GPU with its neighbour and lasts ~2 frame times, which
    # measures nothing: the roofline uses the kernel ALONE.  k_inflight = mean launch duration over the timed region (event pairs
    # on each launch's stream, inside libcloudsky; what rocprofv3 --kernel-trace reports for this command); k_solo = the same kernel with the
    # GPU to itself, timed over solo launches right here (also reads the sample counters).
    k_inflight = k_total / max(1, k_launches)
    ranks_seen = dist.get_world_size() if world > 1 else 1
    share_ms = f_incloud = None
    if args.full:
        k_solo, st = ctx.time_clouds(params, W, bands, warmup=1, iters=max(3, args.kernel_iters))
        # every rank's share alone (solo launches): what bounds the split; gathered so that rank 0 can print them
        share_ms = [k_solo]
        if world > 1:
            t = torch.zeros(world, dtype=torch.float64, device="cpu" if debug_one_gpu else dev)
            t[rank] = k_solo
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            share_ms = [float(x) for x in t.tolist()]
        rays_launch = bands[3] * bands[0] * W
        f_incloud = st["incloud_samples"] / max(1, st["primary_samples"])
        floor_bytes = rays_launch * (8 + BYTES_PER_SAMPLE * primary)                           # 10 248 B/ray at 128 steps
        total_bytes = rays_launch * 8 + BYTES_PER_SAMPLE * (st["primary_samples"] + (light + 1) * st["incloud_samples"])

    # the same K frames strictly one at a time (sky LUT + set-up + march [+ gather] per frame, nothing overlapped): N = 1 only
    one_at_a_time = None
    if args.full and world == 1 and fif > 1:
        ctx.set_frames_in_flight(1)
        s0 = streams[0]
        def step1(k):
            fp, fs = (params, sun_n) if sweep is None else sweep[k % len(sweep)]
            ctx.render_sky_lut_device(fs, 200, 100, s0.cuda_stream)
            ctx.render_clouds_device(fp, W, bands, local[0].data_ptr(), W * 8, s0.cuda_stream)
        for k in range(max(2, args.warmup)):
            step1(k)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for k in range(args.steps):
            step1(k)
        torch.cuda.synchronize()
        e1 = time.perf_counter() - t1
        one_at_a_time = {"value": W * H * args.steps / e1 / 1e6, "ms_per_step": e1 / args.steps * 1e3, "hemisphere_fps": args.steps / e1}
        ctx.set_frames_in_flight(fif)
        frame[0] = local[0]

    # The host form (N = 1): frames delivered into PINNED HOST memory per second through csky_submit_clouds / csky_collect (what the GDExtension's
    # submit_clouds() / collect() wrap), with 1 and 2 frames in flight.  PCIe-inclusive: never the headline `value` (frames resident in HBM).
    host_form = None
    if args.full and world == 1 and not args.no_host_form:
        host_form = {}
        nh = max(10, min(args.steps, 100))
        for slots in (1, 2):
            ctx.set_host_ring(slots)
            tickets = []

            def hstep(k):
                fp, fs = (params, sun_n) if sweep is None else sweep[k % len(sweep)]
                if len(tickets) == slots:
                    ctx.collect(tickets.pop(0), copy=False)
                ctx.render_sky_lut_device(fs, 200, 100, None)
                tickets.append(ctx.submit_clouds(fp, W, H))
            for k in range(4):
                hstep(k)
            while tickets:
                ctx.collect(tickets.pop(0), copy=False)
            t1 = time.perf_counter()
            for k in range(nh):
                hstep(k)
            while tickets:
                ctx.collect(tickets.pop(0), copy=False)
            eh = time.perf_counter() - t1
            host_form["%d_in_flight" % slots] = {"ms_per_frame": eh / nh * 1e3, "frames_per_s": nh / eh, "Mrays_per_s": W * H * nh / eh / 1e6, "frames": nh,
                                                 "GB_per_s_to_host": W * H * 8 * nh / eh / 1e9}
        ctx.set_frames_in_flight(fif)

    # secondary figure, N = 1 only, labelled NON-HEADLINE: the same frames with the wave early-out the north star describes (a wave stops once all 64 lanes
    # have T < eps = 1e-3; clouds.glsl:172-212 has no early-out, so `value` keeps eps = 0).  max_abs_err_vs_eps0 = the largest |difference| of any RGBA16F
    # value between one frame rendered with and without it (the tail a ray drops is bounded by eps x the largest radiance).  --no-early-out-leg skips it.
    early = None
    if args.full and world == 1 and args.early_out == 0.0 and not args.no_early_out_leg:
        ref_frame = torch.zeros((bands[3] * bands[0], W, 4), dtype=torch.int16, device=dev)
        eo_frame = torch.zeros_like(ref_frame)
        s0e = streams[0].cuda_stream
        ctx.render_sky_lut_device(sun_n, 200, 100, s0e)
        ctx.render_clouds_device(params, W, bands, ref_frame.data_ptr(), W * 8, s0e)
        ctx.set_early_out(1e-3)
        ctx.render_clouds_device(params, W, bands, eo_frame.data_ptr(), W * 8, s0e)
        torch.cuda.synchronize()
        a_e, b_e = ref_frame.view(torch.float16).float(), eo_frame.view(torch.float16).float()
        n_eo = max(10, min(args.steps, 100))
        for _ in range(3):
            step()
        drain()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(n_eo):
            step()
        drain()
        torch.cuda.synchronize()
        e_eo = time.perf_counter() - t1
        early = {"eps": 1e-3, "Mrays_per_s": W * H * n_eo / e_eo / 1e6, "ms_per_step": e_eo / n_eo * 1e3, "frames": n_eo,
                 "max_abs_err_vs_eps0": float((a_e - b_e).abs().max().item()), "values_changed_frac": float((ref_frame != eo_frame).float().mean().item()),
                 "headline": False, "what": "NOT the headline: wave-ballot early-out at T < 1e-3 (north_star), same frames, measured after the timed regions"}
        ctx.set_early_out(0.0)
        counter[0] = 0; taken[0] = 0
        step()
        drain()
        torch.cuda.synchronize()

    if rank == 0:
        fr = frame[0].view(torch.float16)
        alpha_mean = float(fr[..., 3].float().mean().item()) if args.full else None
        finite = bool(torch.isfinite(fr.float()).all().item()) if args.full else None
        frame_check = None
        if args.full and world > 1:       # the gathered frame must equal a single-context full-frame render of the same push constants (outside the timed region)
            full = torch.zeros((H, W, 4), dtype=torch.int16, device=dev)
            ctx.set_segments(1)
            fp_l, fs_l = (params, sun_n) if sweep is None else sweep[frame_k[0] % len(sweep)]   # the frame rank 0 holds (the last one gathered, whatever group rendered it)
            ctx.render_sky_lut_device(fs_l, 200, 100, stream)
            ctx.render_clouds_device(fp_l, W, (H, 0, 1, 1), full.data_ptr(), W * 8, stream)
            torch.cuda.synchronize()
            a, b = full.view(torch.float16).float(), frame[0].view(torch.float16).float()
            err = (a - b).abs()
            ok = float((err <= 5e-4 + 2e-3 * a.abs()).float().mean().item())
            frame_check = {"max_abs_diff": float(err.max().item()), "within_1_fp16_ulp_frac": ok, "bit_identical_frac": float((full == frame[0]).float().mean().item()),
                           "what": "the last gathered frame of the run vs the same frame rendered whole on rank 0's GPU (segmented small launches re-associate the compositing sums)"}
            print("gathered %d-rank frame vs single-rank frame: max|d| = %.3g, within 1 fp16 ulp-ish: %.6f" % (world, frame_check["max_abs_diff"], ok), file=sys.stderr, flush=True)
            if ok < 0.9999:
                raise SystemExit("bench.py: multi-rank frame differs from the single-rank frame")
            if split_lut:                 # ... and the sky LUT interleaved from the ranks' rows must BE the LUT rank 0 has just rendered whole
                whole = torch.from_numpy(ctx.read_sky_lut().view(np.int16)).to(dev)
                same = bool((whole == sky_lut[0]).all().item())
                frame_check["sky_lut"] = {"rows_per_rank": fg.max_lut_rows(LH), "assembled_equals_whole": same}
                if not same:
                    raise SystemExit("bench.py: the sky LUT assembled from the ranks' rows differs from the whole LUT")
        # ---- hardware counters of the cloud kernel, collected now (child processes; the timed region is over)
        pmc, pmc_note = None, "not collected: N > 1, --no-pmc or no --full"
        pmc_cfg = "C5frame" if args.config == "C5" else args.config          # the sweep's frames cost the same: profile one of them
        if args.full and world == 1 and not args.no_pmc and not off_workload:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import pmc_collect
            t_p = time.perf_counter()
            try:
                keep = os.path.join(ROOT, "gpurun_out", "bench_pmc_%s.json" % args.config) if os.path.isdir(os.path.join(ROOT, "gpurun_out")) else None
                pmc, pmc_note = pmc_collect.collect(pmc_cfg, frames=6, keep=keep)
            except Exception as e:   # the bench line is still valid without the fractions
                pmc, pmc_note = None, "pmc collection failed: %s" % str(e)[:200]
            pmc_s = time.perf_counter() - t_p
        # ---- the clock of each region + the instruction census (round 3)
        # SQ_BUSY_CYCLES / 32 is NOT the kernel's duration in cycles when shader engines idle in the launch tail (C3 alone: 2.01 "GHz", C5 alone: 2.31,
        # profiles/r02), so cycles available = duration x the shader clock SAMPLED during that region (tools/sclk.py: amdgpu hwmon freq1_input).
        # Every region is re-run for >= 0.4 s with the sampler on; the headline `value` above was timed without it.
        clocks, census, census_note = None, None, "not collected: N > 1, --no-pmc or no --full"
        if args.full and world == 1 and not args.no_pmc and not off_workload:
            import sclk
            import isa_profile
            pr = torch.cuda.get_device_properties(local_rank)
            bus = "%04x:%02x:%02x.0" % (getattr(pr, "pci_domain_id", 0), pr.pci_bus_id, getattr(pr, "pci_device_id", 0)) if isinstance(getattr(pr, "pci_bus_id", None), int) else None
            node = sclk.hwmon_freq_path(bus)
            clocks = {"source": node, "nominal_mhz": (getattr(pr, "clock_rate", 0) or 2400000) / 1e3}

            def clocked(run_frames, frames_per_call):
                run_frames()                                     # warm
                torch.cuda.synchronize()
                n = 0
                with sclk.SclkSampler(node) as sm:
                    t1 = time.perf_counter()
                    while time.perf_counter() - t1 < 0.4:
                        run_frames(); n += frames_per_call
                    torch.cuda.synchronize()
                    e = time.perf_counter() - t1
                return {"ms_per_frame": e / n * 1e3, "frames": n, "sclk": sm.stats()}

            ctx.set_frames_in_flight(fif)
            clocks["headline"] = clocked(lambda: ([step() for _ in range(20)], drain()), 20)
            ctx.set_frames_in_flight(1)
            s0c = streams[0]

            def one_by_one():
                for k in range(10):
                    fp, fs = (params, sun_n) if sweep is None else sweep[k % len(sweep)]
                    ctx.render_sky_lut_device(fs, 200, 100, s0c.cuda_stream)
                    ctx.render_clouds_device(fp, W, bands, local[0].data_ptr(), W * 8, s0c.cuda_stream)
            clocks["one_frame_at_a_time"] = clocked(one_by_one, 10)
            solo_ms = []
            clocks["kernel_alone"] = clocked(lambda: solo_ms.append(ctx.time_clouds(params, W, bands, warmup=0, iters=20)[0]), 20)
            clocks["kernel_alone"]["kernel_ms"] = sum(solo_ms[1:]) / max(1, len(solo_ms) - 1)
            ctx.set_frames_in_flight(fif)
            ok_c, census_note = isa_profile.census_available()
            if ok_c:
                try:
                    cen = isa_profile.report(isa_profile.run_counts(pmc_cfg, quiet=True), quiet=True)
                    census = cen
                    census_note = "live in this run (tools/isa_profile.py: the census build of the library, frame byte-identical to the product build)"
                except BaseException as e:
                    census, census_note = None, "census failed: %s" % str(e)[:200]
        vi = (pmc or {}).get("valu_issue") or {}
        # the bytes the kernel's lanes REQUEST per frame (its own reject logic walked on the host over every ray: tools/executed_tap_bytes.py), next to
        # the contractual 80 B/sample: why the algorithmic figure exceeds the HBM peak without any work being skipped
        executed_taps = None
        tap_file = os.path.join(ROOT, "profiles", "r04", "executed_tap_bytes_C3.json")
        if args.full and args.config == "C3" and world == 1 and not off_workload and os.path.exists(tap_file):
            et = json.load(open(tap_file))
            executed_taps = {"bytes_per_launch": et["executed_tap_bytes"], "over_algorithmic": et["executed_over_algorithmic"], "primary": et["primary"]["bytes"], "light": et["light"]["bytes"],
                             "achieved_GBps_solo": et["executed_tap_bytes"] / (k_solo * 1e-3) / 1e9, "source": "profiles/r04/executed_tap_bytes_C3.json (host walk of cloud_core.h, lane-level)",
                             "in_cloud_samples_match_this_run": et["primary"]["in_cloud"] == st["incloud_samples"] or abs(et["primary"]["in_cloud"] - st["incloud_samples"]) <= 64}
        l1 = (pmc or {}).get("l1_gather") or {}
        hb = (pmc or {}).get("hbm_traffic") or {}
        traffic = hb.get("bytes")
        out = {
            "metric": "Mrays/s + hemisphere fps, 2048x1024 @ 128x6 steps, 1/2/4/8 MI355X",
            "value": W * H * args.steps / elapsed / 1e6,
            "unit": "Mrays/s",
            "hemisphere_fps": args.steps / elapsed,
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "protocol": "as asked: W warm-up + K timed steps, run first (cold); the clock-pre-warmed figure is value_prewarmed",
            "value_prewarmed": (prewarmed or as_asked)["value"], "ms_per_step_prewarmed": (prewarmed or as_asked)["ms_per_step"], "prewarmed": prewarmed,
            "value_as_asked": as_asked["value"], "ms_per_step_as_asked": as_asked["ms_per_step"], "as_asked": as_asked,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "value_one_frame_at_a_time": one_at_a_time,
            "value_host_form": host_form,
            "ranks_seen": ranks_seen, "per_rank_share_ms": share_ms, "gathered_frame_check": frame_check,
            "config": {"workload": "%s: %dx%d hemisphere, %d primary x %d light steps, sun (%.4f,%.4f,%.4f), clouds_sky.tres defaults, "
                                   "weather.bmp + worlnoise.bmp + generated 128^3 shape noise (seed 1), wind frozen"
                                   % (args.config, W, H, primary, light, sun_n[0], sun_n[1], sun_n[2])
                                   + ("  [NOT THE BENCHMARK WORKLOAD: cloud_coverage %g, shape-generator knobs %s]" % (args.coverage, knobs or "default") if off_workload else ""),
                       "off_workload": off_workload, "incloud_fraction": f_incloud, "exact_fp32_cells": bool(ctx.noise_inexact_coeffs() != 0),
                       "texture_size": [W, H], "primary_steps": primary, "light_steps": light, "early_out_eps": args.early_out, "with_early_out": early,
                       "variant": gvcd_amd.lib().csky_variant_name(args.variant if args.variant is not None else gvcd_amd._lib.DEFAULT_VARIANT).decode(),
                       "parallelism": "bands%d%s%s" % (per, "+overlapped-gather" if overlap else "", " x %d frame groups" % G if G > 1 else ""), "frames_in_flight": fif, "frame_groups": G,
                       "clock_prewarm_frames": prewarm_frames,
                       "alpha_mean": alpha_mean, "finite": finite},
            "roofline": None if not args.full else dict(valu_roofline(census, clocks, pmc, vi, k_solo, elapsed / args.steps * 1e3), **{
                # neither "hbm" nor "mfma" binds this path (docstring): the top-level fields are the VALU-issue roof, the one closest to 1
                "bound": "valu", "kernel": "the cloud march.  Top level: clouds_kernel<3,1> alone (one launch with the GPU to itself) at the guide's issue rates; `timed_region`: the same body as clouds_kernel_persistent<3> over the timed region, two launches overlapping",
                "unit": "SIMD issue cycles per launch",
                "traffic": traffic,
                "kernel_ms_solo": k_solo, "kernel_ms_in_flight": k_inflight, "kernel_launches_timed": k_launches, "frames_in_flight": fif,
                "valu_issue_class_counter_model": vi or None,
                "census_note": census_note,
                "l1_gather": l1 or None,
                "hbm": None if traffic is None else {"bytes_per_launch": traffic, "achieved_GBps": traffic / (k_solo * 1e-3) / 1e9, "peak_GBps": HBM_PEAK_GBS,
                                                     "frac": traffic / (k_solo * 1e-3) / 1e9 / HBM_PEAK_GBS, "l2_hit": hb.get("l2_hit"),
                                                     "fetch_size_correction": hb.get("fetch_size_correction"),
                                                     "note": "memory-side bytes of the L2: FETCH_SIZE x its calibrated correction + WRITE_SIZE (KiB -> bytes), Infinity-Cache hits "
                                                             "included.  The correction is measured on gather patterns with known byte counts (profiles/r03/"
                                                             "issue_cost_calibration_tables.txt): one L2 miss per 128-byte line, FETCH_SIZE tallies 64 bytes per miss => x2.00"},
                "hbm_algorithmic": {"bytes_per_sample": BYTES_PER_SAMPLE, "rays_per_launch": rays_launch, "bytes_per_launch": floor_bytes,
                                    "bytes_per_launch_incl_light_march": total_bytes, "incloud_fraction": f_incloud,
                                    "achieved_GBps": floor_bytes / (k_solo * 1e-3) / 1e9, "ratio_to_hbm_peak": floor_bytes / (k_solo * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                    "note": "SURVEY 8(d)'s contractual figure: 80 B/sample x primary steps + 8 B/ray against the 8 TB/s HBM peak, solo launch.  It exceeds 1 "
                                            "(taps are served by L1/L2, 44 % of the primary samples are rejected before the shape tap) and therefore measures nothing: kept "
                                            "for continuity with round 1 only"},
                "pmc": {"collected": "live in this run (tools/pmc_collect.py)" if pmc else None, "note": pmc_note, "source_hash": (pmc or {}).get("source_hash"),
                        "calibration": (pmc or {}).get("calibration"), "seconds": pmc_s if pmc else None},
                "executed_tap_bytes": executed_taps,
                "note": "achieved = EXECUTED wave64 VALU instructions by class (basic-block counts of the census build x the static per-block histogram: valu_issue.valu_by_class) "
                        "at the guide's issue rates, full 2 / half 4 / transcendental 8 cycles per instruction on a SIMD-32, per SIMD (/ 1024); peak = the cycles a SIMD had = "
                        "the launch's duration alone (HIP events) x the shader clock sampled while it ran.  frac_calibrated prices every kind with the time it costs in a "
                        "differential micro-benchmark (profiles/r04/valu_issue_time_gfx950.json: ns per instruction, no clock reading) over the same duration: an upper "
                        "estimate, pure streams run the chip at 2.0-2.35 GHz where this kernel runs at 2.38.  frac_timed_region: the persistent form's instructions over ms_per_step "
                        "(two launches overlap there; a per-launch duration means nothing, elapsed / launches is the effective one): a chip-busy figure, not the kernel's.  "
                        "valu_issue_class_counter_model is round 2's model (hardware class counters, 28 % unclassified) kept for comparison; l1_gather = TA_TA_BUSY / (256 CUs x "
                        "kernel cycles by SQ_BUSY_CYCLES/32), ~1.0 in every saturated pattern of tools/ubench/gather_rates.hip"}),
        }
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(large, small, weather, params, sun_n, W, H, primary, light)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    ctx.close()


if __name__ == "__main__":
    main()
